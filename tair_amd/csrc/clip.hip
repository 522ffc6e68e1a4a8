// Kernels of the CLIP-H text tower (clip.py:8-61, open_clip transformer.py:199-256): the causal self-attention
// and the token + positional embedding.  The tower's linears are the MFMA GEMM (GELU: act 3), its LayerNorms
// layernorm_split (norm.hip); tair_amd/clip_hip.py drives them.
//
// Causal attention, head dim 64, S <= 128 tokens: softmax(Q K^T * scale + mask) V with the additive mask of
// build_attention_mask (transformer.py:589-595): query i sees keys 0..i, and there is no padding mask (tokens
// after EOT attend like any other).  Every query sees key 0, so no row is fully masked.
//  * one workgroup (4 waves) per (batch, head, 64-query block); the keys the block can see (at most its last
//    query's index + 1 <= 128) are staged ONCE in the LDS as two 64-key tiles, in attention.hip's layouts
//    (K: chunk ^ (row & 7); V row-major with chunk ^ (2 * ((row >> 1) & 3)), read transposed by
//    ds_read_b64_tr_b16); one barrier, after which the waves run independently;
//  * a wave owns 16 queries and runs the key tiles up to its diagonal only (the second tile is skipped by the
//    waves of the first 64 queries); S^T = K Q^T and O^T = V^T P^T on the bf16 16x16x32 MFMA as in attention.hip,
//    softmax in fp32 (base 2), P rounded to bf16 before P V; the two tiles are merged by the running (max, sum)
//    rescale;
//  * keys past a query are masked to -inf before the row max, so their p is exactly 0: the output rows <= i do
//    not depend on the k / v rows > i (rows past the block's last query are not even read).
#include "kernels.h"

namespace tair {
namespace {

constexpr int KT = 64;  // keys per LDS tile

typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) s16x4 lds_s16x4;

TAIR_DEV int kswz(int row, int chunk) { return row * 64 + ((chunk ^ (row & 7)) << 3); }
TAIR_DEV int vswz(int row, int chunk) { return row * 64 + ((chunk ^ (((row >> 1) & 3) << 1)) << 3); }

TAIR_DEV float xmax16(float x) {  // max(x[l], x[l ^ 16])
  const auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(x), __float_as_uint(x), false, false);
  return fmaxf(__uint_as_float(r[0]), __uint_as_float(r[1]));
}
TAIR_DEV float xmax32(float x) {  // max(x[l], x[l ^ 32])
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
TAIR_DEV s16x4 tr_read(const bf16* p) { return __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)p); }

__global__ __launch_bounds__(256) void attn_causal_kernel(const bf16* __restrict__ q, int ldq,
                                                          const bf16* __restrict__ k, int ldk,
                                                          const bf16* __restrict__ v, int ldv, bf16* __restrict__ o,
                                                          int ldo, int H, int S, float c) {
  __shared__ __attribute__((aligned(16))) bf16 sK[2][KT * 64];
  __shared__ __attribute__((aligned(16))) bf16 sV[2][KT * 64];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int hi = lane >> 4, lo = lane & 15;
  const int bh = blockIdx.y;
  const int b = bh / H, h = bh - b * H;
  const int qb0 = blockIdx.x * 64;
  const int kmax = min(S, qb0 + 64);      // keys 0 .. kmax - 1: all that the block's queries see
  const int ntile = (kmax + KT - 1) / KT;  // 1 or 2
  const int q0 = qb0 + wid * 16;

  // stage the block's keys: 64 keys x 8 chunks per tile and operand, 2 per thread; rows past kmax re-read the
  // last visible key (finite data, masked to p = 0)
  const bf16* kb = k + (size_t)b * S * ldk + h * 64;
  const bf16* vb = v + (size_t)b * S * ldv + h * 64;
  const int srow = tid >> 3, schunk = tid & 7;
  for (int t = 0; t < ntile; ++t) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int row = srow + 32 * i;
      const int src = min(t * KT + row, kmax - 1);
      *(u32x4*)(&sK[t][kswz(row, schunk)]) = *(const u32x4*)(kb + (size_t)src * ldk + schunk * 8);
      *(u32x4*)(&sV[t][vswz(row, schunk)]) = *(const u32x4*)(vb + (size_t)src * ldv + schunk * 8);
    }
  }
  // Q^T fragments (MFMA B operand): lane holds Q[q = lo][d = 32s + 8hi .. +7]; queries past S re-read the last
  const int qme = min(q0 + lo, S - 1);
  bf16x8 qf[2];
  {
    const bf16* qr = q + ((size_t)b * S + qme) * ldq + h * 64;
#pragma unroll
    for (int s = 0; s < 2; ++s) qf[s] = *(const bf16x8*)(qr + 32 * s + 8 * hi);
  }
  __syncthreads();  // the only barrier: from here on the waves run independently
  if (q0 >= S) return;

  // per-lane transposed-read offsets (elements) of V rows 4hi + (lo >> 2) (+16), d = 16db + 4(lo & 3)
  int voff[2][4];
#pragma unroll
  for (int e = 0; e < 2; ++e)
#pragma unroll
    for (int db = 0; db < 4; ++db) {
      const int row = 16 * e + 4 * hi + (lo >> 2);
      const int chunk = 2 * db + ((lo & 3) >> 1);
      voff[e][db] = vswz(row, chunk) + 4 * (lo & 1);  // + 32 rows per s step: same swizzle
    }

  float m_run = -INFINITY, l_run = 0.f;
  f32x4 oacc[4];  // O^T[d = 16db + 4hi + r][q = lo]
#pragma unroll
  for (int db = 0; db < 4; ++db) oacc[db] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int wtile = min(ntile, (q0 + 15) / KT + 1);  // key tiles at or below the wave's diagonal
  for (int t = 0; t < wtile; ++t) {
    const int key0 = t * KT;
    const bf16* Ks = sK[t];
    const bf16* Vs = sV[t];
    // S^T blocks: sacc[kb][r] = S[q = lo][key = key0 + 16kb + 4hi + r]
    f32x4 sacc[4];
#pragma unroll
    for (int kb4 = 0; kb4 < 4; ++kb4) sacc[kb4] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
      for (int kb4 = 0; kb4 < 4; ++kb4) {
        const bf16x8 kf = *(const bf16x8*)(Ks + kswz(kb4 * 16 + lo, 4 * s + hi));
        sacc[kb4] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf, qf[s], sacc[kb4], 0, 0, 0);
      }
    // causal mask (covers the keys past S as well: qme < S)
#pragma unroll
    for (int kb4 = 0; kb4 < 4; ++kb4)
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if (key0 + kb4 * 16 + hi * 4 + r > qme) sacc[kb4][r] = -INFINITY;
    // softmax in base 2 with the running (max, sum): p = 2^(s c - m).  The tile's first key is visible to every
    // query of the wave (key0 <= q0), so mx is finite
    float mx = fmaxf(fmaxf(sacc[0][0], sacc[0][1]), fmaxf(sacc[0][2], sacc[0][3]));
#pragma unroll
    for (int kb4 = 1; kb4 < 4; ++kb4)
      mx = fmaxf(mx, fmaxf(fmaxf(sacc[kb4][0], sacc[kb4][1]), fmaxf(sacc[kb4][2], sacc[kb4][3])));
    mx = xmax32(xmax16(mx));
    const float mold = m_run;
    const float mnew = fmaxf(mold, mx * c);
    m_run = mnew;
    float ls = 0.f;
    float pv[4][4];
#pragma unroll
    for (int kb4 = 0; kb4 < 4; ++kb4)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float pe = __builtin_amdgcn_exp2f(__builtin_fmaf(sacc[kb4][r], c, -mnew));
        pv[kb4][r] = pe;
        ls += pe;
      }
    const float alpha = __builtin_amdgcn_exp2f(mold - mnew);
    l_run = l_run * alpha + ls;
#pragma unroll
    for (int db = 0; db < 4; ++db)
#pragma unroll
      for (int r = 0; r < 4; ++r) oacc[db][r] *= alpha;
    bf16x8 pf[2];
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        pf[s][r] = f2bf(pv[2 * s][r]);
        pf[s][4 + r] = f2bf(pv[2 * s + 1][r]);
      }
    // O^T += V^T P^T: A operand = V^T[d = 16db + lo][keys 32s + 4hi + j | 32s + 16 + 4hi + j]
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
      for (int db = 0; db < 4; ++db) {
        const s16x4 vv[2] = {tr_read(Vs + 32 * s * 64 + voff[0][db]), tr_read(Vs + 32 * s * 64 + voff[1][db])};
        bf16x8 vf;
        __builtin_memcpy(&vf, vv, 16);
        oacc[db] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf, pf[s], oacc[db], 0, 0, 0);
      }
  }

  const float inv = 1.f / xsum32(xsum16(l_run));
  const int qi = q0 + lo;
  if (qi < S) {
    bf16* orow = o + ((size_t)b * S + qi) * ldo + h * 64;
#pragma unroll
    for (int db = 0; db < 4; ++db) {
      const bf16x4 w = {f2bf(oacc[db][0] * inv), f2bf(oacc[db][1] * inv), f2bf(oacc[db][2] * inv),
                        f2bf(oacc[db][3] * inv)};
      *(bf16x4*)(orow + db * 16 + hi * 4) = w;
    }
  }
}

// one thread per 4 channels of a token
__global__ __launch_bounds__(256) void embed_tokens_kernel(const int64_t* __restrict__ ids, int rows, int L,
                                                           const float* __restrict__ table, int vocab,
                                                           const float* __restrict__ pos, int C,
                                                           bf16* __restrict__ out, int out_lo, int ld, int* fault) {
  const int c4n = C >> 2;
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (long)rows * c4n) return;
  const int row = (int)(idx / c4n), c = (int)(idx - (long)row * c4n) * 4;
  long id = ids[row];
  if (id < 0 || id >= vocab) {  // never an out-of-bounds read: clamped, and reported through the fault counter
    if (c == 0 && fault) atomicAdd(fault, 1);
    id = id < 0 ? 0 : vocab - 1;
  }
  const float4 t = *(const float4*)(table + (size_t)id * C + c);
  const float4 p = *(const float4*)(pos + (size_t)(row % L) * C + c);
  const float x[4] = {t.x + p.x, t.y + p.y, t.z + p.z, t.w + p.w};
  bf16x4 h4, l4;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    h4[e] = f2bf(x[e]);
    l4[e] = f2bf(x[e] - bf2f(h4[e]));
  }
  bf16* orow = out + (size_t)row * ld + c;
  *(bf16x4*)orow = h4;
  *(bf16x4*)(orow + out_lo) = l4;
}

bool al16p(const void* p) { return p && ((uintptr_t)p & 15) == 0; }

}  // namespace

hipError_t attention_causal(const bf16* q, int ldq, const bf16* k, int ldk, const bf16* v, int ldv, bf16* o, int ldo,
                            int B, int H, int S, float scale, hipStream_t s) {
  if (S < 1 || S > CAUSAL_MAX_S || B < 1 || H < 1 || (long)B * H > 65535 || !(scale > 0.f) || !al16p(q) ||
      !al16p(k) || !al16p(v) || !al16p(o) || ((ldq | ldk | ldv | ldo) & 7) || ldq < H * 64 || ldk < H * 64 ||
      ldv < H * 64 || ldo < H * 64)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(attn_causal_kernel, dim3(cdiv(S, 64), B * H), dim3(256), 0, s, q, ldq, k, ldk, v, ldv, o, ldo, H,
                     S, scale * 1.4426950408889634f);
  return hipGetLastError();
}

hipError_t embed_tokens(const int64_t* ids, int B, int L, const float* table, int vocab, const float* pos, int C,
                        bf16* out, int out_lo, int ld, hipStream_t s) {
  if (!ids || !al16p(table) || !al16p(pos) || !out || ((uintptr_t)out & 7) || B < 1 || L < 1 || vocab < 1 || C < 4 ||
      (C & 3) || out_lo < C || (out_lo & 3) || ld < out_lo + C || (ld & 3))
    return hipErrorInvalidValue;
  TAIR_HIP_CHECK(gemm_init());  // (allocates the fault counter on first use; a no-op afterwards)
  const long n = (long)B * L * (C / 4);
  hipLaunchKernelGGL(embed_tokens_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, ids, B * L, L, table,
                     vocab, pos, C, out, out_lo, ld, gemm_fault_word());
  return hipGetLastError();
}

}  // namespace tair
