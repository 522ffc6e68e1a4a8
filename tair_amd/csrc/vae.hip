// Kernels of the split-precision VAE decoder (reference: terediff/model/vae.py:120-282 AttnBlock,
// 429-559 Decoder) that are not GEMMs or GroupNorms: the attention softmax and the V transpose.
// Values are carried as three bf16 planes (hi, lo, hi) / (hi, hi, lo) so that bf16 MFMA GEMMs over
// 3K reproduce fp32 products to ~2^-16 (kernels.h GemmArgs::out_split).
#include "kernels.h"

namespace tair {
namespace {

// One block per row: P = softmax(S[row, :L]) written as hi / lo / hi planes [3L].
__global__ __launch_bounds__(256) void softmax_split_kernel(const float* __restrict__ S, int lds, int L,
                                                            bf16* __restrict__ P) {
  const float* s = S + (size_t)blockIdx.x * lds;
  bf16* p = P + (size_t)blockIdx.x * 3 * L;
  __shared__ float red[4];
  float m = -INFINITY;
  for (int i = threadIdx.x; i < L; i += 256) m = fmaxf(m, s[i]);
  m = wave_max(m);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
  __syncthreads();
  m = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
  __syncthreads();
  float sum = 0.f;
  for (int i = threadIdx.x; i < L; i += 256) sum += expf(s[i] - m);
  sum = wave_sum(sum);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = sum;
  __syncthreads();
  const float inv = 1.f / ((red[0] + red[1]) + (red[2] + red[3]));
  for (int i = threadIdx.x; i < L; i += 256) {
    const float v = expf(s[i] - m) * inv;
    const bf16 hi = f2bf(v);
    p[i] = hi;
    p[L + i] = f2bf(v - bf2f(hi));
    p[2 * L + i] = hi;
  }
}

// x [B][L][3C] (hi, lo, hi) -> y [B][C][3L] (hi, hi, lo), through 64 x 64 LDS tiles.
__global__ __launch_bounds__(256) void transpose_split_kernel(const bf16* __restrict__ x, int L, int C,
                                                              bf16* __restrict__ y) {
  __shared__ bf16 th[64][65], tl[64][65];
  const int b = blockIdx.z;
  const int l0 = blockIdx.x * 64, c0 = blockIdx.y * 64;
  const bf16* xb = x + (size_t)b * L * 3 * C;
  bf16* yb = y + (size_t)b * C * 3 * L;
  for (int e = threadIdx.x; e < 64 * 64; e += 256) {
    const int r = e / 64, c = e % 64;  // r: l within tile, c: channel within tile (coalesced on c)
    const int l = l0 + r, ch = c0 + c;
    if (l < L && ch < C) {
      th[r][c] = xb[(size_t)l * 3 * C + ch];
      tl[r][c] = xb[(size_t)l * 3 * C + C + ch];
    }
  }
  __syncthreads();
  for (int e = threadIdx.x; e < 64 * 64; e += 256) {
    const int r = e / 64, c = e % 64;  // r: channel within tile, c: l within tile (coalesced on l)
    const int ch = c0 + r, l = l0 + c;
    if (l < L && ch < C) {
      bf16* o = yb + (size_t)ch * 3 * L + l;
      o[0] = th[c][r];
      o[L] = th[c][r];
      o[2 * L] = tl[c][r];
    }
  }
}

// softmax_split_kernel for a key count L that is no multiple of the GEMM's K-tile: the planes are Lp = roundup(L, 64)
// columns wide, P [rows][3 Lp], zero at columns L..Lp of every plane (the padded keys add exactly nothing to P.V).
// The max / sum loops run to L: the padded columns of S are never read.
__global__ __launch_bounds__(256) void softmax_split_pad_kernel(const float* __restrict__ S, int lds, int L, int Lp,
                                                                bf16* __restrict__ P) {
  const float* s = S + (size_t)blockIdx.x * lds;
  bf16* p = P + (size_t)blockIdx.x * 3 * Lp;
  __shared__ float red[4];
  float m = -INFINITY;
  for (int i = threadIdx.x; i < L; i += 256) m = fmaxf(m, s[i]);
  m = wave_max(m);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
  __syncthreads();
  m = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
  __syncthreads();
  float sum = 0.f;
  for (int i = threadIdx.x; i < L; i += 256) sum += expf(s[i] - m);
  sum = wave_sum(sum);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = sum;
  __syncthreads();
  const float inv = 1.f / ((red[0] + red[1]) + (red[2] + red[3]));
  const bf16 zero = f2bf(0.f);
  for (int i = threadIdx.x; i < Lp; i += 256) {
    bf16 hi = zero, lo = zero;
    if (i < L) {
      const float v = expf(s[i] - m) * inv;
      hi = f2bf(v);
      lo = f2bf(v - bf2f(hi));
    }
    p[i] = hi;
    p[Lp + i] = lo;
    p[2 * Lp + i] = hi;
  }
}

// transpose_split_kernel with padded rows: x [B][L][3C] (hi, lo, hi) -> y [B][C][3 Lp] (hi, hi, lo), zero at
// columns L..Lp of every plane.
__global__ __launch_bounds__(256) void transpose_split_pad_kernel(const bf16* __restrict__ x, int L, int Lp, int C,
                                                                  bf16* __restrict__ y) {
  __shared__ bf16 th[64][65], tl[64][65];
  const int b = blockIdx.z;
  const int l0 = blockIdx.x * 64, c0 = blockIdx.y * 64;
  const bf16* xb = x + (size_t)b * L * 3 * C;
  bf16* yb = y + (size_t)b * C * 3 * Lp;
  const bf16 zero = f2bf(0.f);
  for (int e = threadIdx.x; e < 64 * 64; e += 256) {
    const int r = e / 64, c = e % 64;
    const int l = l0 + r, ch = c0 + c;
    const bool in = l < L && ch < C;
    th[r][c] = in ? xb[(size_t)l * 3 * C + ch] : zero;
    tl[r][c] = in ? xb[(size_t)l * 3 * C + C + ch] : zero;
  }
  __syncthreads();
  for (int e = threadIdx.x; e < 64 * 64; e += 256) {
    const int r = e / 64, c = e % 64;
    const int ch = c0 + r, l = l0 + c;
    if (l < Lp && ch < C) {
      bf16* o = yb + (size_t)ch * 3 * Lp + l;
      o[0] = th[c][r];
      o[Lp] = th[c][r];
      o[2 * Lp] = tl[c][r];
    }
  }
}

// Cross-tile GroupNorm of the tiled VAE (tilevae.py:232-278 GroupNormParam.summary): one thread per (image, group)
// reads its (sum, sum^2) from the 8 replicas of each of the T tiles' slots, forms each tile's biased mean / var,
// merges them with the tiles' pixel shares (a weighted average of variances, not the union's variance) and
// rewrites every slot so that gn_apply's finalisation over that tile's own count returns the merged pair.
__global__ __launch_bounds__(256) void gn_stats_merge_kernel(const GnMergeArgs a) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= a.B * a.G) return;
  double total = 0.0;
  for (int t = 0; t < a.T; ++t) total += (double)a.pixels[t];
  double mean = 0.0, var = 0.0;
  for (int t = 0; t < a.T; ++t) {
    const double* q = a.slots + (size_t)t * a.slot_stride + (size_t)i * 2;
    double s1 = 0.0, s2 = 0.0;
#pragma unroll
    for (int r = 0; r < STAT_REPL; ++r) {
      s1 += q[(size_t)r * a.st_rs];
      s2 += q[(size_t)r * a.st_rs + 1];
    }
    const double cnt = (double)a.pixels[t] * a.cg;
    const double mt = s1 / cnt;
    const double vt = fmax(s2 / cnt - mt * mt, 0.0);
    const double w = (double)a.pixels[t] / total;
    mean += w * mt;
    var += w * vt;
  }
  for (int t = 0; t < a.T; ++t) {
    double* q = a.slots + (size_t)t * a.slot_stride + (size_t)i * 2;
    const double cnt = (double)a.pixels[t] * a.cg;
    q[0] = mean * cnt;
    q[1] = (var + mean * mean) * cnt;
#pragma unroll
    for (int r = 1; r < STAT_REPL; ++r) {
      q[(size_t)r * a.st_rs] = 0.0;
      q[(size_t)r * a.st_rs + 1] = 0.0;
    }
  }
}

}  // namespace

hipError_t softmax_split_pad(const float* S, int lds, int rows, int L, int Lp, bf16* P, hipStream_t s) {
  if (!S || !P || rows < 1 || L < 1 || Lp < L || Lp % 64 || lds < L) return hipErrorInvalidValue;
  hipLaunchKernelGGL(softmax_split_pad_kernel, dim3(rows), dim3(256), 0, s, S, lds, L, Lp, P);
  return hipGetLastError();
}

hipError_t transpose_split_pad(const bf16* x, int B, int L, int Lp, int C, bf16* y, hipStream_t s) {
  if (!x || !y || B < 1 || C < 1 || L < 1 || Lp < L || Lp % 64) return hipErrorInvalidValue;
  hipLaunchKernelGGL(transpose_split_pad_kernel, dim3(Lp / 64, cdiv(C, 64), B), dim3(256), 0, s, x, L, Lp, C, y);
  return hipGetLastError();
}

hipError_t gn_stats_merge(const GnMergeArgs& a, hipStream_t s) {
  if (!a.slots || a.T < 1 || a.T > GN_MERGE_MAX_TILES || a.B < 1 || a.G < 1 || a.cg < 1 ||
      a.st_rs < a.B * a.G * 2 || (a.T > 1 && a.slot_stride < (long long)STAT_REPL * a.st_rs))
    return hipErrorInvalidValue;
  for (int t = 0; t < a.T; ++t)
    if (a.pixels[t] < 1) return hipErrorInvalidValue;
  hipLaunchKernelGGL(gn_stats_merge_kernel, dim3(cdiv(a.B * a.G, 256)), dim3(256), 0, s, a);
  return hipGetLastError();
}

hipError_t softmax_split(const float* S, int lds, int rows, int L, bf16* P, hipStream_t s) {
  hipLaunchKernelGGL(softmax_split_kernel, dim3(rows), dim3(256), 0, s, S, lds, L, P);
  return hipGetLastError();
}

hipError_t transpose_split(const bf16* x, int B, int L, int C, bf16* y, hipStream_t s) {
  hipLaunchKernelGGL(transpose_split_kernel, dim3(cdiv(L, 64), cdiv(C, 64), B), dim3(256), 0, s, x, L, C, y);
  return hipGetLastError();
}

}  // namespace tair
