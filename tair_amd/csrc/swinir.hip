// Kernels of the SwinIR cleaner (swinir.py:37-151 WindowAttention, :245-285 SwinTransformerBlock, :841-894 forward):
// the shifted-window attention, the LayerNorm over a channel count that is no multiple of 8 (180, in rows padded
// to 192) and the in-place LeakyReLU of the upsampler.  The network's linears and 3x3 convs are the MFMA GEMM;
// tair_amd/swinir_hip.py drives them.
//
// Window attention, 8x8 windows, head dim d <= 32 stored in 32 columns per head:
//  * one workgroup (4 waves) per (batch, window, head); the cyclic shift and the window partition are addressing:
//    token (iy, ix) of window (wy, wx) is pixel ((8 wy + iy + shift) mod H, (8 wx + ix + shift) mod W), for the
//    reads of q / k / v and for the write of o.  Columns d..31 of a head are zero-filled on load (they may hold
//    anything, NaN included) and written as zeros;
//  * the window's 64 keys are staged once in the LDS (K row-major, V transposed), with the head's 225 relative-
//    position biases and the tokens' shift-mask regions; one barrier, after which the waves run independently;
//  * a wave owns 16 queries: S^T = K Q^T is one K-step of the bf16 16x16x32 MFMA per 16 keys (attention.hip's
//    operand conventions), s = S scale + bias[(iy_q - iy_k + 7) 15 + (ix_q - ix_k + 7)] - 100 [regions differ],
//    softmax in fp32 over the 64 keys in one pass (no running rescale), P rounded to bf16, O^T = V^T P^T.
//  * the mask (swinir.py:222-243): in the shifted frame y' = 8 wy + iy has region 0 (y' < H - 8), 1 (y' < H - shift)
//    or 2, likewise x'; two tokens whose (region_y, region_x) differ get the reference's finite -100.
#include "kernels.h"

namespace tair {
namespace {

constexpr int WS = 8, WT = 64;  // window side / tokens per window
constexpr int VT_LD = 68;       // row stride of the transposed V tile (elements): 8-byte rows, banks spread

TAIR_DEV float xmax16(float x) {  // max(x[l], x[l ^ 16])
  const auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(x), __float_as_uint(x), false, false);
  return fmaxf(__uint_as_float(r[0]), __uint_as_float(r[1]));
}
TAIR_DEV float xmax32(float x) {
  const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(x), false, false);
  return fmaxf(__uint_as_float(r[0]), __uint_as_float(r[1]));
}
TAIR_DEV float xsum16(float x) {
  const auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(x), __float_as_uint(x), false, false);
  return __uint_as_float(r[0]) + __uint_as_float(r[1]);
}
TAIR_DEV float xsum32(float x) {
  const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(x), false, false);
  return __uint_as_float(r[0]) + __uint_as_float(r[1]);
}

TAIR_DEV int kswz(int row, int chunk) { return row * 32 + ((chunk ^ ((row >> 1) & 3)) << 3); }

// 8 channels c0 .. c0 + 7 of a head's row; channels >= d read as zero whatever the memory holds
TAIR_DEV bf16x8 load_head8(const bf16* p, int c0, int d) {
  bf16x8 v = *(const bf16x8*)(p + c0);
#pragma unroll
  for (int e = 0; e < 8; ++e)
    if (c0 + e >= d) v[e] = f2bf(0.f);
  return v;
}

__global__ __launch_bounds__(256) void window_attn_kernel(const bf16* __restrict__ q, int ldq,
                                                          const bf16* __restrict__ k, int ldk,
                                                          const bf16* __restrict__ v, int ldv, bf16* __restrict__ o,
                                                          int ldo, int H, int W, int heads, int d, int shift,
                                                          const float* __restrict__ bias_table, float scale) {
  __shared__ __attribute__((aligned(16))) bf16 sK[WT * 32];
  __shared__ __attribute__((aligned(16))) bf16 sVt[32 * VT_LD];
  __shared__ float sBias[225];
  __shared__ int sRow[WT];  // pixel row (b H W + y W + x) of the window's tokens
  __shared__ int sReg[WT];  // 3 region_y + region_x
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int hi = lane >> 4, lo = lane & 15;
  const int h = blockIdx.y;
  const int nwx = W / WS, nwy = H / WS;
  const int win = blockIdx.x;
  const int b = win / (nwx * nwy), wr = win - b * (nwx * nwy);
  const int wy = wr / nwx, wx = wr - wy * nwx;

  if (tid < WT) {
    const int ys = wy * WS + (tid >> 3), xs = wx * WS + (tid & 7);  // the shifted frame
    int y = ys + shift, x = xs + shift;
    if (y >= H) y -= H;
    if (x >= W) x -= W;
    sRow[tid] = (b * H + y) * W + x;
    const int ry = ys < H - WS ? 0 : ys < H - shift ? 1 : 2;
    const int rx = xs < W - WS ? 0 : xs < W - shift ? 1 : 2;
    sReg[tid] = shift ? 3 * ry + rx : 0;
  }
  if (tid < 225) sBias[tid] = bias_table[tid * heads + h];
  __syncthreads();

  {  // stage K (row-major) and V (transposed): 64 keys x 4 chunks of 8 channels, one per thread
    const int key = tid >> 2, chunk = tid & 3;
    const size_t row = (size_t)sRow[key];
    *(bf16x8*)(&sK[kswz(key, chunk)]) = load_head8(k + row * ldk + h * 32, chunk * 8, d);
    const bf16x8 vv = load_head8(v + row * ldv + h * 32, chunk * 8, d);
#pragma unroll
    for (int e = 0; e < 8; ++e) sVt[(chunk * 8 + e) * VT_LD + key] = vv[e];
  }
  // Q^T fragment (MFMA B operand): lane holds Q[q = lo][d = 8hi .. 8hi + 7]
  const int qt = wid * 16 + lo;
  const size_t qrow = (size_t)sRow[qt];
  const bf16x8 qf = load_head8(q + qrow * ldq + h * 32, 8 * hi, d);
  __syncthreads();  // from here on the waves run independently

  // S^T blocks: sacc[kb][r] = S[q = lo][key = 16kb + 4hi + r]
  f32x4 sacc[4];
#pragma unroll
  for (int kb = 0; kb < 4; ++kb) {
    const bf16x8 kf = *(const bf16x8*)(sK + kswz(kb * 16 + lo, hi));
    sacc[kb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf, qf, f32x4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
  }
  const int qy = qt >> 3, qx = qt & 7, qreg = sReg[qt];
  float sv[4][4];
  float mx = -INFINITY;
#pragma unroll
  for (int kb = 0; kb < 4; ++kb)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int kt = kb * 16 + hi * 4 + r;
      float s = __builtin_fmaf(sacc[kb][r], scale, sBias[(qy - (kt >> 3) + 7) * 15 + (qx - (kt & 7) + 7)]);
      if (sReg[kt] != qreg) s += -100.f;
      sv[kb][r] = s;
      mx = fmaxf(mx, s);
    }
  mx = xmax32(xmax16(mx));
  float ls = 0.f;
#pragma unroll
  for (int kb = 0; kb < 4; ++kb)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      sv[kb][r] = __expf(sv[kb][r] - mx);
      ls += sv[kb][r];
    }
  const float inv = 1.f / xsum32(xsum16(ls));
  bf16x8 pf[2];
#pragma unroll
  for (int s = 0; s < 2; ++s)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      pf[s][r] = f2bf(sv[2 * s][r]);
      pf[s][4 + r] = f2bf(sv[2 * s + 1][r]);
    }
  // O^T += V^T P^T: A operand = V^T[d = 16db + lo][keys 32s + 4hi + j | 32s + 16 + 4hi + j]
  f32x4 oacc[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
#pragma unroll
  for (int s = 0; s < 2; ++s)
#pragma unroll
    for (int db = 0; db < 2; ++db) {
      const bf16* vr = sVt + (db * 16 + lo) * VT_LD + 32 * s + 4 * hi;
      const bf16x4 v0 = *(const bf16x4*)vr, v1 = *(const bf16x4*)(vr + 16);
      const bf16x8 vf = {v0[0], v0[1], v0[2], v0[3], v1[0], v1[1], v1[2], v1[3]};
      oacc[db] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf, pf[s], oacc[db], 0, 0, 0);
    }
  // O^T[d = 16db + 4hi + r][q = lo]
  bf16* orow = o + qrow * ldo + h * 32;
#pragma unroll
  for (int db = 0; db < 2; ++db) {
    bf16x4 w;
#pragma unroll
    for (int r = 0; r < 4; ++r) w[r] = db * 16 + hi * 4 + r < d ? f2bf(oacc[db][r] * inv) : f2bf(0.f);
    *(bf16x4*)(orow + db * 16 + hi * 4) = w;
  }
}

// LayerNorm over columns [0, C) of a (two-plane) row, C % 4 == 0, into bf16 rows of Cp >= C columns with zeros at
// [C, Cp): layernorm_split_kernel's arithmetic (fp32, two-pass variance).  One wave per token, 4 channels per lane
// and step.
constexpr int LNP_VPL = 4;  // C <= 64 * 4 * LNP_VPL
__global__ __launch_bounds__(256) void layernorm_split_pad_kernel(const bf16* __restrict__ x, int ldx, int x_lo, int T,
                                                                  int C, int Cp, const float* __restrict__ gamma,
                                                                  const float* __restrict__ beta, float eps,
                                                                  bf16* __restrict__ y, int ldy) {
  const int lane = threadIdx.x & 63;
  const int t = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (t >= T) return;
  const int cv = C / 4, cpv = Cp / 4;
  const bf16* xr = x + (size_t)t * ldx;
  float v[LNP_VPL][4];
  float sum = 0.f;
#pragma unroll
  for (int j = 0; j < LNP_VPL; ++j) {
    const int vi = lane + 64 * j;
    if (vi < cv) {
      const bf16x4 a = *(const bf16x4*)(xr + vi * 4);
#pragma unroll
      for (int e = 0; e < 4; ++e) v[j][e] = bf2f(a[e]);
      if (x_lo) {
        const bf16x4 l = *(const bf16x4*)(xr + x_lo + vi * 4);
#pragma unroll
        for (int e = 0; e < 4; ++e) v[j][e] += bf2f(l[e]);
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) sum += v[j][e];
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) v[j][e] = 0.f;
    }
  }
  const float mean = wave_sum(sum) / C;
  float sq = 0.f;
#pragma unroll
  for (int j = 0; j < LNP_VPL; ++j)
    if (lane + 64 * j < cv) {
#pragma unroll
      for (int e = 0; e < 4; ++e) { const float dd = v[j][e] - mean; sq += dd * dd; }
    }
  const float rstd = rsqrtf(wave_sum(sq) / C + eps);
  bf16* yr = y + (size_t)t * ldy;
#pragma unroll
  for (int j = 0; j < LNP_VPL; ++j) {
    const int vi = lane + 64 * j;
    if (vi < cv) {
      const float4 g = *(const float4*)(gamma + vi * 4), bb = *(const float4*)(beta + vi * 4);
      const bf16x4 w = {f2bf((v[j][0] - mean) * rstd * g.x + bb.x), f2bf((v[j][1] - mean) * rstd * g.y + bb.y),
                        f2bf((v[j][2] - mean) * rstd * g.z + bb.z), f2bf((v[j][3] - mean) * rstd * g.w + bb.w)};
      *(bf16x4*)(yr + vi * 4) = w;
    } else if (vi < cpv) {
      *(bf16x4*)(yr + vi * 4) = bf16x4{f2bf(0.f), f2bf(0.f), f2bf(0.f), f2bf(0.f)};
    }
  }
}

// one thread per 8 channels of a row
__global__ __launch_bounds__(256) void leaky_relu_kernel(bf16* __restrict__ x, int ld, long n8, int c8, float slope) {
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= n8) return;
  const long row = idx / c8;
  const int c = (int)(idx - row * c8) * 8;
  bf16x8* p = (bf16x8*)(x + (size_t)row * ld + c);
  bf16x8 a = *p;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const float f = bf2f(a[e]);
    a[e] = f > 0.f ? a[e] : f2bf(f * slope);
  }
  *p = a;
}

bool al16(const void* p) { return p && ((uintptr_t)p & 15) == 0; }

}  // namespace

hipError_t window_attention(const bf16* q, int ldq, const bf16* k, int ldk, const bf16* v, int ldv, bf16* o, int ldo,
                            int B, int H, int W, int heads, int d, int shift, const float* bias_table, float scale,
                            hipStream_t s) {
  const int need = heads * 32;
  if (B < 1 || H < WS || W < WS || (H % WS) || (W % WS) || heads < 1 || heads > 65535 || d < 1 || d > 32 || shift < 0 ||
      shift >= WS || !(scale > 0.f) || !bias_table || ((uintptr_t)bias_table & 3) || !al16(q) || !al16(k) || !al16(v) ||
      !al16(o) || ((ldq | ldk | ldv | ldo) & 7) || ldq < need || ldk < need || ldv < need || ldo < need ||
      (long)B * H * W > 0x7fffffffL)
    return hipErrorInvalidValue;
  const int wins = B * (H / WS) * (W / WS);
  hipLaunchKernelGGL(window_attn_kernel, dim3(wins, heads), dim3(256), 0, s, q, ldq, k, ldk, v, ldv, o, ldo, H, W, heads,
                     d, shift, bias_table, scale);
  return hipGetLastError();
}

hipError_t layernorm_split_pad(const bf16* x, int ldx, int x_lo, int T, int C, int Cp, const float* gamma,
                               const float* beta, float eps, bf16* y, int ldy, hipStream_t s) {
  if (!x || !y || !gamma || !beta || T < 1 || C < 4 || (C & 3) || C > 64 * 4 * LNP_VPL || Cp < C || (Cp & 3) ||
      x_lo < 0 || (x_lo && x_lo < C) || (x_lo & 3) || ldx < x_lo + C || (ldx & 3) || ldy < Cp || (ldy & 3) ||
      ((uintptr_t)x & 7) || ((uintptr_t)y & 7) || ((uintptr_t)gamma & 15) || ((uintptr_t)beta & 15))
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(layernorm_split_pad_kernel, dim3(cdiv(T, 4)), dim3(256), 0, s, x, ldx, x_lo, T, C, Cp, gamma, beta,
                     eps, y, ldy);
  return hipGetLastError();
}

hipError_t leaky_relu(bf16* x, int ld, int rows, int C, float slope, hipStream_t s) {
  if (!al16(x) || rows < 1 || C < 8 || (C & 7) || ld < C || (ld & 7)) return hipErrorInvalidValue;
  const long n8 = (long)rows * (C / 8);
  if ((n8 + 255) / 256 > 0x7fffffffL) return hipErrorInvalidValue;
  hipLaunchKernelGGL(leaky_relu_kernel, dim3((unsigned)((n8 + 255) / 256)), dim3(256), 0, s, x, ld, n8, C / 8, slope);
  return hipGetLastError();
}

}  // namespace tair
