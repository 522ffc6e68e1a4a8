// Latent tiling inside the fused sampling loop (utils/common.py:125-234 make_tiled_fn, wired as in
// ddim_sampler.py:165-180): the whole latent [B, H, W, C] is larger than the network's S x S input, so every
// step runs the network on overlapping S x S windows and blends the window outputs with Gaussian weights
// before the sampler update runs on the whole latent.  Two kernels sit between the whole latent and the
// per-window rows of one forward ("chunk"): a gather before it and a blend / update after it.
//
// Window k = ih * nw + iw of an image starts at (min(ih * stride, H - S), min(iw * stride, W - S)): the
// strided starts plus one flush with the edge when the stride does not divide (sliding_windows).  Job row
// j = b * T + k (image-major); chunk c runs job rows [c * rpc, (c + 1) * rpc), rows past the job's end ("pad")
// repeat the last window and are never blended.
#include "kernels.h"

namespace tair {
namespace {

struct Geo {
  int B, H, W, S, stride, nh, nw, rpc, n_chunks;
};

__host__ __device__ inline int win_count(int n, int S, int stride) { return (n - S + stride - 1) / stride + 1; }
__device__ inline int win_start(int i, int n, int S, int stride) { return min(i * stride, n - S); }
// the first window index that can cover coordinate p: earlier strided windows end before p
__device__ inline int ih0_of(int p, int S, int stride) { return p >= S ? (p - S) / stride + 1 : 0; }

// One thread per (chunk row, window pixel, channel): channels [0, C) are the latent, [C, C + hc) the hint
// (only with in_c).  Writes the (hi, lo, hi) bf16 planes sampler_update_kernel writes for an untiled step.
__global__ __launch_bounds__(256) void tile_gather_kernel(const float* __restrict__ x, const float* __restrict__ hint,
                                                          const float* __restrict__ hint_u,
                                                          const int* __restrict__ chunkp, bf16* in_u, bf16* in_c,
                                                          int C, int hc, int ld, int ldc, size_t half_off, Geo g) {
  const int CH = in_c ? C + hc : C;
  const long total = (long)g.rpc * g.S * g.S * CH;
  const long i = blockIdx.x * 256L + threadIdx.x;
  if (i >= total) return;
  const int chunk = chunkp[0];
  if (chunk < 0 || chunk >= g.n_chunks) return;
  const int ch = (int)(i % CH);
  const long rp = i / CH;
  const int p = (int)(rp % (g.S * g.S));
  const int r = (int)(rp / (g.S * g.S));
  const int T = g.nh * g.nw;
  const int j = min(chunk * g.rpc + r, g.B * T - 1);  // a pad row repeats the job's last window
  const int b = j / T, k = j - b * T;
  const int y = win_start(k / g.nw, g.H, g.S, g.stride) + p / g.S;
  const int xq = win_start(k % g.nw, g.W, g.S, g.stride) + p % g.S;
  const size_t src = ((size_t)b * g.H + y) * g.W + xq;
  const size_t row = (size_t)r * g.S * g.S + p;
  if (ch < C) {
    const float v = x[src * C + ch];
    const bf16 hi = (bf16)v, lo = (bf16)(v - (float)hi);
    bf16* u = in_u + row * ld + ch;
    u[0] = hi;
    u[C] = lo;
    u[2 * C] = hi;
    if (half_off) {
      u[half_off] = hi;
      u[half_off + C] = lo;
      u[half_off + 2 * C] = hi;
    }
    if (in_c) {
      bf16* q = in_c + row * ld + ch;
      q[0] = hi;
      q[ldc] = lo;
      q[2 * ldc] = hi;
      if (half_off) {
        q[half_off] = hi;
        q[half_off + ldc] = lo;
        q[half_off + 2 * ldc] = hi;
      }
    }
  } else {
    const int c = ch - C;
    const float v = hint[src * hc + c];
    const bf16 hi = (bf16)v, lo = (bf16)(v - (float)hi);
    bf16* q = in_c + row * ld + C + c;
    q[0] = hi;
    q[ldc] = lo;
    q[2 * ldc] = hi;
    if (half_off) {  // the uncond half reads its own hint when it has one
      const float vu = hint_u ? hint_u[src * hc + c] : v;
      const bf16 hu = (bf16)vu, lu = (bf16)(vu - (float)hu);
      q[half_off] = hu;
      q[half_off + ldc] = lu;
      q[half_off + 2 * ldc] = hu;
    }
  }
}

// One thread per whole-latent element (b, y, x, c): a gather over the windows of the current chunk that cover
// the pixel, in ascending window order (no atomics, so the sums do not depend on how the rows were chunked):
//   acc += v_k * w,  cnt += w        (acc_u likewise from the uncond half of a guided forward)
// On the step's last chunk: v = acc / cnt, guidance v = v_u + s_i (v_c - v_u), the p_sample arithmetic of
// sampler_update_kernel against the whole-latent noise, and the accumulators are cleared for the next step.
// A pixel that a single window covers takes that window's output unchanged (acc holds v itself): the
// reference's fl(fl(v w) / w) is within one ulp of it, and one ulp in x is enough to move the bf16 network's
// next output by ~1e-3, so only the exact value lets a one-window latent reproduce the untiled run.
__global__ __launch_bounds__(256) void tile_blend_kernel(float* xs, const float* __restrict__ v, size_t vu_off,
                                                         float* v_blend, float* acc, float* acc_u, float* cnt,
                                                         const float* __restrict__ w, const float* __restrict__ tabs,
                                                         const float* __restrict__ scales,
                                                         const int* __restrict__ counter,
                                                         const int* __restrict__ chunkp,
                                                         const float* __restrict__ noise, int C, Geo g) {
  const long n = (long)g.B * g.H * g.W * C;
  const long e = blockIdx.x * 256L + threadIdx.x;
  if (e >= n) return;
  const int chunk = chunkp[0];
  const int it = counter[0], ns = counter[1];
  if (chunk < 0 || chunk >= g.n_chunks || it < 0 || it >= ns) return;
  const int c = (int)(e % C);
  const long px = e / C;
  const int xq = (int)(px % g.W);
  const int y = (int)((px / g.W) % g.H);
  const int b = (int)(px / ((long)g.W * g.H));
  const int T = g.nh * g.nw;
  const int j0 = chunk * g.rpc, j1 = min(j0 + g.rpc, g.B * T);  // pad rows lie past j1: never read
  float a = acc[e], au = acc_u ? acc_u[e] : 0.f, cn = cnt[e];
  // windows of the whole job that cover the pixel (geometry only: the same in every chunk)
  int ncov = 0;
  for (int ih = ih0_of(y, g.S, g.stride); ih < g.nh && win_start(ih, g.H, g.S, g.stride) <= y; ++ih)
    for (int iw = ih0_of(xq, g.S, g.stride); iw < g.nw && win_start(iw, g.W, g.S, g.stride) <= xq; ++iw) ++ncov;
  const bool single = ncov == 1;
  const int ih0 = ih0_of(y, g.S, g.stride), iw0 = ih0_of(xq, g.S, g.stride);
  for (int ih = ih0; ih < g.nh; ++ih) {
    const int y0 = win_start(ih, g.H, g.S, g.stride);
    if (y0 > y) break;
    for (int iw = iw0; iw < g.nw; ++iw) {
      const int x0 = win_start(iw, g.W, g.S, g.stride);
      if (x0 > xq) break;
      const int j = b * T + ih * g.nw + iw;
      if (j < j0 || j >= j1) continue;
      const int q = (y - y0) * g.S + (xq - x0);
      const size_t src = ((size_t)(j - j0) * g.S * g.S + q) * C + c;
      const float wq = w[q];
      a += single ? v[src] : __fmul_rn(v[src], wq);
      if (acc_u) au += single ? v[src + vu_off] : __fmul_rn(v[src + vu_off], wq);
      cn += wq;
    }
  }
  if (chunk != g.n_chunks - 1) {
    acc[e] = a;
    if (acc_u) acc_u[e] = au;
    cnt[e] = cn;
    return;
  }
  acc[e] = 0.f;
  if (acc_u) acc_u[e] = 0.f;
  cnt[e] = 0.f;
  float vi = single ? a : a / cn;
  if (acc_u) {
    const float vu = single ? au : au / cn;
    vi = vu + scales[it] * (vi - vu);
  }
  v_blend[e] = vi;
  const int t = ns - 1 - it;
  const float sa = tabs[t], s1a = tabs[ns + t], c1 = tabs[2 * ns + t], c2 = tabs[3 * ns + t], var = tabs[4 * ns + t];
  const float xv = xs[e];
  const float x0 = sa * xv - s1a * vi;
  const float mean = c1 * x0 + c2 * xv;
  xs[e] = (t != 0) ? mean + sqrtf(var) * noise[(size_t)it * n + e] : mean;
}

// After the blend of chunk c: the next chunk, or the next step from chunk 0.
__global__ void tile_advance_kernel(int* counter, int* chunkp, int n_chunks) {
  if (threadIdx.x != 0) return;
  const int c = chunkp[0];
  if (c < 0 || c >= n_chunks) return;
  if (c == n_chunks - 1) {
    chunkp[0] = 0;
    counter[0] += 1;
  } else {
    chunkp[0] = c + 1;
  }
}

bool geo_of(const TileGeom& t, int C, Geo* g) {
  if (t.B < 1 || t.S < 1 || t.H < t.S || t.W < t.S || t.stride < 1 || t.rows_per_chunk < 1 || t.n_chunks < 1 ||
      C < 1)
    return false;
  const long nh = win_count(t.H, t.S, t.stride), nw = win_count(t.W, t.S, t.stride);
  const long N = t.B * nh * nw;
  // every chunk holds at least one job row, and the chunks cover the job
  if ((long)t.n_chunks * t.rows_per_chunk < N || (long)(t.n_chunks - 1) * t.rows_per_chunk >= N) return false;
  if ((long)t.B * t.H * t.W * C > 0x7fffffffL || N > 0x7fffffffL) return false;
  *g = Geo{t.B, t.H, t.W, t.S, t.stride, (int)nh, (int)nw, t.rows_per_chunk, t.n_chunks};
  return true;
}

}  // namespace

int tile_windows(int H, int W, int S, int stride) {
  if (S < 1 || H < S || W < S || stride < 1) return 0;
  return win_count(H, S, stride) * win_count(W, S, stride);
}

hipError_t tile_gather(const TileGatherArgs& a, hipStream_t s) {
  Geo g;
  if (!a.x || !a.chunk || !a.in_u || !geo_of(a.g, a.C, &g) || a.ld < 3 * a.C || a.half_rows < 0) return hipErrorInvalidValue;
  const long prow = (long)g.rpc * g.S * g.S;  // plane rows one half writes
  if (a.half_rows && a.half_rows < prow) return hipErrorInvalidValue;
  if (a.in_c && (!a.hint || a.hc < 1 || a.ldc < a.C + a.hc || 2 * a.ldc + a.C + a.hc > a.ld)) return hipErrorInvalidValue;
  if (((long)a.half_rows + prow) * a.ld > 0x7fffffffL) return hipErrorInvalidValue;
  const long total = prow * (a.in_c ? a.C + a.hc : a.C);
  hipLaunchKernelGGL(tile_gather_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, a.x, a.hint, a.hint_u,
                     a.chunk, a.in_u, a.in_c, a.C, a.hc, a.ld, a.ldc, (size_t)a.half_rows * a.ld, g);
  return hipGetLastError();
}

hipError_t tile_blend_step(const TileBlendArgs& a, hipStream_t s) {
  Geo g;
  if (!a.x || !a.v || !a.v_blend || !a.acc || !a.cnt || !a.w || !a.tabs || !a.counter || !a.chunk || !a.noise ||
      !geo_of(a.g, a.C, &g) || (a.acc_u && !a.scales))
    return hipErrorInvalidValue;
  const long half = (long)g.rpc * g.S * g.S * a.C;  // elements of one half of the forward's output
  if (2 * half > 0x7fffffffL) return hipErrorInvalidValue;
  const long n = (long)g.B * g.H * g.W * a.C;
  hipLaunchKernelGGL(tile_blend_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, a.x, a.v,
                     a.acc_u ? (size_t)half : (size_t)0, a.v_blend, a.acc, a.acc_u, a.cnt, a.w, a.tabs, a.scales,
                     a.counter, a.chunk, a.noise, a.C, g);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(tile_advance_kernel, dim3(1), dim3(64), 0, s, a.counter, a.chunk, g.n_chunks);
  return hipGetLastError();
}

}  // namespace tair
