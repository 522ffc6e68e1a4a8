// Tiling of the SwinIR cleaner over an image larger than one tile (utils/common.py:174-234 make_tiled_fn as
// pipeline.py:371-397 wraps the cleaner in it: scale 1, Gaussian weights, fp32 accumulators, no padding).  The image
// [B, 3, H, W] fp32 NCHW is cut into S x S windows (S a multiple of 64) at `stride`, the last window of a row / column
// flush with the edge (sliding_windows), so a window may start at any pixel.  Job row j = b * T + k (image-major, then
// row-major window order); the network runs chunks of job rows, and two kernels sit around each chunk:
//  * the gather writes every chunk row's window as the network's input: mean-subtracted, pixel-unshuffled by 8 to a
//    token map of S/8 x S/8 tokens with column c * 64 + dy * 8 + dx, split into the planes hi | lo (what
//    HipSwinIR.forward prepares with torch ops for an untiled image);
//  * the blend adds the chunk's output (conv_last's fp32 NHWC rows, as they stand) into the whole-image accumulators
//    with the Gaussian weights and, on the last chunk, divides by the accumulated weight into the NCHW output.
// A chunk row past the job's last row ("pad") is gathered as the last window and never blended.
#include "kernels.h"

namespace tair {
namespace {

constexpr int UNSHUF = 8;                    // pixel-unshuffle factor: a token is an 8 x 8 pixel block
constexpr int TOK_C = 3 * UNSHUF * UNSHUF;   // 192 columns of a token
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));

struct IGeo {
  int B, H, W, S, stride, nh, nw;
};

__host__ __device__ inline int iwin_count(int n, int S, int stride) { return (n - S + stride - 1) / stride + 1; }
__device__ inline int iwin_start(int i, int n, int S, int stride) { return min(i * stride, n - S); }
// the first window index that can cover coordinate p: earlier strided windows end before p
__device__ inline int iwin_first(int p, int S, int stride) { return p >= S ? (p - S) / stride + 1 : 0; }

// One lane per pair of adjacent columns of a token (96 lanes a token): two pixels of one image row in, one 4-byte
// store to each plane out; consecutive lanes write consecutive addresses.
__global__ __launch_bounds__(256) void image_tile_gather_kernel(const float* __restrict__ x,
                                                                const float* __restrict__ mean, bf16* __restrict__ in,
                                                                int ld, int lo_off, int first, long total, IGeo g) {
  const long i = blockIdx.x * 256L + threadIdx.x;
  if (i >= total) return;
  const int col = (int)(i % (TOK_C / 2)) * 2;
  const long tok = i / (TOK_C / 2);
  const int t = g.S / UNSHUF, tt = t * t;
  const int p = (int)(tok % tt);
  const int r = (int)(tok / tt);
  const int T = g.nh * g.nw;
  const int j = min(first + r, g.B * T - 1);  // a pad row repeats the job's last window
  const int b = j / T, k = j - b * T;
  const int c = col >> 6, dy = (col >> 3) & 7, dx = col & 7;
  const int y = iwin_start(k / g.nw, g.H, g.S, g.stride) + (p / t) * UNSHUF + dy;
  const int xq = iwin_start(k % g.nw, g.W, g.S, g.stride) + (p % t) * UNSHUF + dx;
  const float* src = x + (((size_t)b * 3 + c) * g.H + y) * g.W + xq;  // xq + 1 < W: dx is even, the window fits
  const float m = mean[c];
  const float u0 = __fsub_rn(src[0], m), u1 = __fsub_rn(src[1], m);
  const bf16 h0 = f2bf(u0), h1 = f2bf(u1);
  bf16* dst = in + ((size_t)r * tt + p) * ld + col;
  *(bf16x2*)dst = bf16x2{h0, h1};
  *(bf16x2*)(dst + lo_off) = bf16x2{f2bf(__fsub_rn(u0, (float)h0)), f2bf(__fsub_rn(u1, (float)h1))};
}

// One thread per image element (b, c, y, x), x along the lanes: a gather over the job rows [first, j1) whose window
// covers the pixel, in ascending window order (no atomics: chunks ascend and windows ascend inside a chunk, so the
// sums are the reference loop's whatever the chunking).  The product is rounded before it is added, as the
// reference's `out += fn(x) * weights` does; a pixel under a single window is fl(fl(v w) / w), as there.
__global__ __launch_bounds__(256) void image_tile_blend_kernel(const float* __restrict__ v, const float* __restrict__ w,
                                                               float* acc, float* cnt, float* __restrict__ out,
                                                               int first, int j1, int finalize, IGeo g) {
  const long n = (long)g.B * 3 * g.H * g.W;
  const long e = blockIdx.x * 256L + threadIdx.x;
  if (e >= n) return;
  const int xq = (int)(e % g.W);
  const int y = (int)((e / g.W) % g.H);
  const int bc = (int)(e / ((long)g.W * g.H));
  const int b = bc / 3, c = bc - b * 3;
  const int T = g.nh * g.nw;
  float a = 0.f, cn = 0.f;
  if (first != 0) {
    a = acc[e];
    cn = cnt[e];
  }
  const int iw0 = iwin_first(xq, g.S, g.stride);
  for (int ih = iwin_first(y, g.S, g.stride); ih < g.nh; ++ih) {
    const int y0 = iwin_start(ih, g.H, g.S, g.stride);
    if (y0 > y) break;
    for (int iw = iw0; iw < g.nw; ++iw) {
      const int x0 = iwin_start(iw, g.W, g.S, g.stride);
      if (x0 > xq) break;
      const int j = b * T + ih * g.nw + iw;
      if (j < first || j >= j1) continue;  // pad rows lie past j1: never read
      const int q = (y - y0) * g.S + (xq - x0);
      const float wq = w[q];
      a = __fadd_rn(a, __fmul_rn(v[((size_t)(j - first) * g.S * g.S + q) * 3 + c], wq));
      cn = __fadd_rn(cn, wq);
    }
  }
  if (finalize) {
    out[e] = __fdiv_rn(a, cn);
  } else {
    acc[e] = a;
    cnt[e] = cn;
  }
}

bool igeo_of(const ImageTileGeom& t, IGeo* g) {
  if (t.B < 1 || t.S < 64 || (t.S % 64) || t.H < t.S || t.W < t.S || t.stride < 1 || t.rows < 1 || t.first < 0)
    return false;
  const long nh = iwin_count(t.H, t.S, t.stride), nw = iwin_count(t.W, t.S, t.stride);
  const long N = t.B * nh * nw;
  if ((long)t.B * 3 * t.H * t.W > 0x7fffffffL || N > 0x7fffffffL || t.first >= N) return false;
  if ((long)t.first + t.rows > 0x7fffffffL || (long)t.rows * t.S * t.S > 0x7fffffffL / 3) return false;
  *g = IGeo{t.B, t.H, t.W, t.S, t.stride, (int)nh, (int)nw};
  return true;
}

}  // namespace

hipError_t image_tile_gather(const float* x, const float* mean, const ImageTileGeom& t, bf16* in, int ld, int lo_off,
                             hipStream_t s) {
  IGeo g;
  if (!x || !mean || !in || ((uintptr_t)in & 3) || !igeo_of(t, &g) || (ld & 1) || (lo_off & 1) || lo_off < TOK_C ||
      ld < lo_off + TOK_C)
    return hipErrorInvalidValue;
  const long tokens = (long)t.rows * (g.S / UNSHUF) * (g.S / UNSHUF);
  if (tokens * ld > 0x7fffffffL) return hipErrorInvalidValue;
  const long total = tokens * (TOK_C / 2);
  hipLaunchKernelGGL(image_tile_gather_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, x, mean, in, ld,
                     lo_off, t.first, total, g);
  return hipGetLastError();
}

hipError_t image_tile_blend(const float* v, const float* w, float* acc, float* cnt, float* out, int finalize,
                            const ImageTileGeom& t, hipStream_t s) {
  IGeo g;
  if (!v || !w || !acc || !cnt || !igeo_of(t, &g) || (finalize && !out)) return hipErrorInvalidValue;
  const long N = (long)g.B * g.nh * g.nw;
  const long j1 = (long)t.first + t.rows < N ? (long)t.first + t.rows : N;
  if (finalize && j1 != N) return hipErrorInvalidValue;  // the division belongs to the chunk that ends the job
  const long n = (long)g.B * 3 * g.H * g.W;
  hipLaunchKernelGGL(image_tile_blend_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, v, w, acc, cnt, out,
                     t.first, (int)j1, finalize ? 1 : 0, g);
  return hipGetLastError();
}

}  // namespace tair
