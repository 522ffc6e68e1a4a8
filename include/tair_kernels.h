/* tair_kernels.h — kernel-level C ABI of libtair_cldm.so (test and integration hooks).
 *
 * These expose the individual gfx950 kernels the ControlLDM runtime is built from, on raw device
 * pointers in the runtime's native layouts (NHWC bf16 activations, [N][ldw] bf16 K-major weights),
 * so each one can be checked in isolation.  The reference has no equivalent FFI; each hook names
 * the reference op it computes.  All are asynchronous on `stream` and allocate nothing.
 */
#ifndef TAIR_KERNELS_H
#define TAIR_KERNELS_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Activation operand modes of the MFMA GEMM. */
#define TAIR_A_DENSE 0
#define TAIR_A_CONV3 1
#define TAIR_A_CONV3_S2 2
#define TAIR_A_CONV3_UP 3
#define TAIR_A_CONV3_SMALLC 4

typedef struct {
  int M, N, K, amode;
  const void* A; int lda; int C; int Bn, H, W, Ho, Wo;
  const void* X; int ldx; int Kx;
  const void* Wt; int ldw;
  float alpha; int scale_bias; int act;
  const float* bias;
  const float* emb; int ld_emb; const int* emb_row; int rows_per_b;
  const void* res; int ld_res;
  void* out; int ldo; int out_f32;
  float* partial; int64_t partial_cap; /* split-K workspace (fp32 elements) or NULL */
  int force_bm, force_bn, force_splits;  /* 0 = heuristic */
  int force_stages;                      /* 4: the 4-phase 256-row kernel; 2: 2-stage 64-row dense tiles;
                                            100 + S: S-deep 64-row ring; 203: two-K-group 64-row tiles */
  int* tile_sem; int sem_cap;            /* split-K tickets (zeroed ints, one per output tile) or NULL:
                                            the last K-slice reduces in-kernel, else a reduce kernel */
  /* split-precision operands (the fp32-accurate VAE decoder): out_split 1 writes hi/lo/hi, 2 hi/hi/lo
   * bf16 planes at columns n, N+n, 2N+n (ldo >= 3N); res_lo > 0: residual = res[n] + res[res_lo + n] */
  int out_split; int res_lo;
  /* GroupNorm statistics of the output for the GroupNorm that consumes it (or st_acc = NULL):
   * fp64 (sum, sum^2) per (batch, group) in 8 replicas of st_rs doubles, groups of st_cg channels */
  double* st_acc; int st_rs, st_cg, st_G, st_coff, st_hw;
  /* two-plane residual-stream storage: out_lo > 0 also writes lo = bf16(v - bf16(v)) at element offset
   * out_lo; x_wrap > 0: the K-extension reads X channel (k - K) mod x_wrap (Kx = 2 x_wrap) */
  int out_lo; int x_wrap;
  int probe; /* measurement probes (0): bit 0 no epilogue stores, bit 1 no epilogue, bit 2 in-kernel split-K at any split count */
  /* f8 != 0: A and Wt hold OCP e4m3 bytes; K, lda, ldw count PAIRS of bytes (K % 64 == 0); dense
   * or stride-1 3x3 conv (A operand e4m3 [pixel][C] bytes, lda = row bytes / 2, K order as the bf16 conv
   * at one byte per value: a 128-value K-tile = two (64-channel chunk, tap) slots; an optional bf16
   * K-extension follows the fp8 K-tiles in each weight row); the epilogue first multiplies by
   * (row_scale ? row_scale[m] : 1) * col_scale[n] */
  int f8; const float* row_scale; const float* col_scale;
  /* stride-2 conv only: 1 = the SD VAE Downsample's padding (0, 1, 0, 1) then pad 0 (vae.py:85-105),
   * 0 = symmetric pad 1 (the UNet Downsample, unet.py:82-108) */
  int s2_shift;
  /* GroupNorm(+SiLU) applied to the activation as it is loaded (unet.py:203-223, attention.py:305; replaces a
   * separate apply pass): gn_st != NULL normalises A per (batch element, channel) with the producer's fp64
   * statistics (the st_acc layout: 8 replicas gn_rs doubles apart, (b * gn_G + g) * 2) over rows_per_b
   * pixels, gamma / beta [C], eps; gn_silu 1 adds SiLU.  Stride-1 conv (rows_per_b = H * W) or dense
   * (C = K); conv padding and the K-extension are not normalised.  Bitwise tair_k_gn_apply_stats + GEMM. */
  const double* gn_st; int gn_rs; int gn_G; float gn_eps; const float* gn_gamma; const float* gn_beta; int gn_silu;
  /* measurement only (a library built with -DTAIR_STAMPS=1; ignored otherwise): per workgroup 8 s_memrealtime
   * stamps (100 MHz) of the kernel's phases, [linear block id][8] u64; null = none */
  unsigned long long* stamps;
  /* LayerNorm folded into this linear (attention.py:265-274 norm1/2/3 -> to_qkv / to_q / GEGLU proj):
   * rst != NULL makes the producer accumulate per output row the fp64 (sum, sum of squares) of its stored bf16
   * values into rst[2m], rst[2m + 1]; lnst != NULL makes the consumer, run on the raw LayerNorm input against
   * W' = W diag(gamma), form v = rstd_m (acc - mean_m lncs[n]) + bias' with mean / rstd from lnst over
   * ln_c channels (eps ln_eps), lncs[n] = sum_k W'[n][k], bias' = bias + W beta. */
  double* rst; const double* lnst; const float* lncs; float ln_c; float ln_eps;
  /* second GroupNorm statistics target (or st2_acc = NULL; needs st_acc): the same output also feeds a second
   * GroupNorm, e.g. the decoder's norm over cat([h, skip]) in which this output's channels start at st2_coff.
   * Its own accumulator, replica stride, group width and group count; it shares st_hw.  st_coff / st2_coff need
   * not be multiples of the group width: a group may receive channels from two producers. */
  double* st2_acc; int st2_rs, st2_cg, st2_G, st2_coff;
} tair_gemm_desc;

/* act: 0 none, 1 SiLU, 2 GEGLU — output channels packed as (x_2q, x_2q+1, gate_2q, gate_2q+1) groups,
 * y[:, 2q+i] = x_2q+i * gelu(gate_2q+i) written to out (N/2 bf16 columns); 3 GELU, y = gelu_erf(alpha acc + bias
 * [+ res]) (nn.GELU of the CLIP text tower's MLP, open_clip transformer.py:199-256): dense bf16 GEMMs on the
 * <= 128 x 128 tile kernels, split-K included; a plan that does not carry it is refused.  Any other act: error.
 * nn.Linear / nn.Conv2d (3x3 pad 1, stride 1|2, nearest-x2 upsample fused) + bias + time-emb +
 * residual epilogue (unet.py:51-223, attention.py:19-353). */
int tair_k_gemm(const tair_gemm_desc* d, void* stream);
/* Faults the GEMM kernels detected on the current device since the last reset (a cooperative split-K slice
 * that gave up waiting for its tile's other slices, so its sums are incomplete; a token id outside the embedding
 * table that tair_k_embed_tokens clamped): *count receives the number;
 * reset != 0 clears it.  Synchronous (reads one device int): call after the work is synchronised, outside
 * stream capture.  A non-zero count means the results of that work are invalid. */
int tair_fault_count(int reset, int* count);
/* sizeof(tair_gemm_desc) as compiled into the library (bindings check their struct mirror against it). */
int tair_k_gemm_desc_bytes(void);
/* The plan tair_k_gemm would launch for d, without launching (host only, no device needed): tile bm x bn
 * (bm < 0: the BK = 32 ring tiles), K splits, kernel (0 tile, 1 4-phase, 2 2-stage shallow, 3 halo conv, 4 deep ring,
 * 5 two-K-group 64-row tile).
 * Returns the validation status tair_k_gemm would report. */
int tair_k_gemm_plan(const tair_gemm_desc* d, int* bm, int* bn, int* splits, int* kern);
/* Grouped launches (tests of the two-lane path): d is an array of n (1 or 2) descriptors of one shape, mode and
 * epilogue kind, run as lanes 0 .. n - 1 of ONE launch (a UNet layer and the same ControlNet layer in the product).
 * The plan is lane 0's request (force_*, probe) for n lanes; every lane brings its own operands, outputs, split-K
 * workspace and tickets.  out_f32 and out_split are shared; out_lo, the time embedding, the residual and the
 * statistics targets may differ.  Any other n: refused, nothing launched. */
int tair_k_gemm_grouped(const tair_gemm_desc* d, int n, void* stream);
/* tair_k_gemm_plan for `lanes` (1 or 2) lanes of d. */
int tair_k_gemm_plan_lanes(const tair_gemm_desc* d, int lanes, int* bm, int* bn, int* splits, int* kern);
/* The validation and planning of tair_k_gemm_grouped for the n descriptors at d, without launching (host only, no
 * device needed): 0, or -2 with tair_last_error. */
int tair_k_gemm_grouped_check(const tair_gemm_desc* d, int n);
/* tair_k_attention_tk for n (1 or 2) lanes of one shape in one launch: each lane its own q / k / v / o, key-split
 * workspace (or NULL) and tickets (or NULL). */
typedef struct {
  const void* q; int ldq; const void* k; int ldk; const void* v; int ldv; void* o; int ldo; int kv_bstride;
  void* ws; int64_t ws_bytes; int* tickets; int tickets_cap;
} tair_attn_lane;
int tair_k_attention_grouped(const tair_attn_lane* lanes, int n, int B, int H, int Sq, int Skv, float scale,
                             int force_qsets, int force_splits, void* stream);
/* tair_k_layernorm (y) / tair_k_layernorm_fp8 (y8, s8, ld8; y may be NULL) for n (1 or 2) lanes in one launch. */
typedef struct {
  const void* x; const float* gamma; const float* beta; void* y; void* y8; float* s8; int ld8;
} tair_ln_lane;
int tair_k_layernorm_grouped(const tair_ln_lane* lanes, int n, int T, int C, float eps, void* stream);
/* GroupNorm for n (1 or 2) lanes per launch.  tair_k_groupnorm_grouped: statistics (tickets in every lane: one
 * launch; else two) into ss, then the apply from ss, as tair_k_groupnorm_ex.  tair_k_gn_apply_stats_grouped: the
 * apply from producer statistics st (every lane), as tair_k_gn_apply_stats (y, y_split) or tair_k_gn_apply_fp8 (y8,
 * ld8, inv8), with x_lo. */
typedef struct {
  const void* x; int ldx; const float* gamma; const float* beta; float* ss; float* ws; int* tickets;
  void* y; int ldy; const double* st; int st_rs; int x_lo; int y_split; void* y8; int ld8; const float* inv8;
} tair_gn_lane;
int tair_k_groupnorm_grouped(const tair_gn_lane* lanes, int n, int B, int HW, int C, int G, float eps, int silu,
                             void* stream);
int tair_k_gn_apply_stats_grouped(const tair_gn_lane* lanes, int n, int B, int HW, int C, int G, float eps, int silu,
                                  void* stream);
/* The two-K-group 64-row tiles (kernel 5; force_stages 203 forces them): loop trips of both K-groups over the
 * workgroup's K-tile slice [kt0, kt1), and the K-tile group g (0 | 1) takes on a trip (a tile >= kt1: no MFMAs). */
int tair_k_kgroup_trips(int kt0, int kt1);
/* Tests only (process-wide): on != 0 makes every planned 3-stage 64-row tile plan the two-K-group kernel is built for
 * take it, with half the K slices.  Returns the number of two-K-group launches since the previous call. */
int tair_k_gemm_kgroup_force(int on);
int tair_k_kgroup_tile(int kt0, int g, int trip);
/* The plan tair_k_attention would launch (host only, no device needed): queries per wave / 16 (qsets),
 * key splits and keys per split, for a workspace of ws_bytes (< 0: unbounded). 0 on success. */
int tair_k_attention_plan(int B, int H, int Sq, int Skv, int64_t ws_bytes, int* qsets, int* splits, int* kv_split);
/* Same for the forced forms (force_qsets / force_splits of tair_k_attention_ex / _tk, 0 = heuristic): the plan
 * that call launches, after the clamps to the key-tile count and to the workspace. */
int tair_k_attention_plan_ex(int B, int H, int Sq, int Skv, int64_t ws_bytes, int force_qsets, int force_splits,
                             int* qsets, int* splits, int* kv_split);
/* softmax(Q K^T * scale) V, head dim 64 (attention.py:168-216). */
int tair_k_attention(const void* q, int ldq, const void* k, int ldk, const void* v, int ldv, void* o, int ldo,
                     int B, int H, int Sq, int Skv, int kv_bstride, float scale, void* stream);
/* Same, with a workspace for the key-split (flash-decoding) partials: per split B*Sq*H*136 bytes.
 * force_qsets (1|2 x 16 queries per wave) / force_splits override the heuristic (0 = heuristic). */
int tair_k_attention_ex(const void* q, int ldq, const void* k, int ldk, const void* v, int ldv, void* o, int ldo,
                        int B, int H, int Sq, int Skv, int kv_bstride, float scale, void* ws, int64_t ws_bytes,
                        int force_qsets, int force_splits, void* stream);
/* Same, with arrival tickets (tickets_cap zeroed ints, left zeroed): the key splits of each (query block, head)
 * are merged in-kernel by the last split to arrive (bitwise the separate merge) when tickets_cap covers
 * 32 ints per block, otherwise by the merge kernel as above. */
int tair_k_attention_tk(const void* q, int ldq, const void* k, int ldk, const void* v, int ldv, void* o, int ldo,
                        int B, int H, int Sq, int Skv, int kv_bstride, float scale, void* ws, int64_t ws_bytes,
                        int* tickets, int tickets_cap, int force_qsets, int force_splits, void* stream);
/* softmax(Q K^T * scale + causal mask) V, head dim 64: the text tower's self-attention (open_clip
 * transformer.py:199-256 with the additive mask of build_attention_mask, :589-595: query i sees keys 0..i; no
 * padding mask).  Rows b * S + i of q / k / v / o, head h at columns h * 64 (operands may be strided out of one
 * fused [T, 3C] q|k|v buffer; leading dimensions % 8 == 0, 16-byte aligned pointers), bf16 in and out, 1 <= S <= 128.
 * One workgroup per (batch, head, 64-query block) stages its keys once in the LDS; a wave owns 16 queries and skips
 * the key tiles wholly above its diagonal.  Bad arguments: -1 with a message, before any launch. */
int tair_k_attention_causal(const void* q, int ldq, const void* k, int ldk, const void* v, int ldv, void* o, int ldo,
                            int B, int H, int S, float scale, void* stream);
/* x = token_embedding[id] + positional_embedding in fp32 (clip.py:38-39), written as
 * two bf16 planes: hi = bf16(x) at out_hi[(b * L + l) * ld + c], lo = bf16(x - hi) out_lo_offset elements further
 * on.  ids [B * L] int64 on the device (capturable); table [vocab][C], pos [L][C] fp32; C % 4 == 0.  An id outside
 * [0, vocab) is clamped into the table and counted in the fault counter (tair_fault_count). */
int tair_k_embed_tokens(const void* ids, int B, int L, const float* table, int vocab, const float* pos, int C,
                        void* out_hi, int out_lo_offset, int ld, void* stream);
/* GroupNorm(G, eps) [+ SiLU] on NHWC bf16 (util.py:191-193, attention.py:48-51). ss: [B][C][2] fp32,
 * ws: [B*G*64*2] fp32 scratch. */
int tair_k_groupnorm(const void* x, int ldx, int B, int HW, int C, int G, float eps, const float* gamma,
                     const float* beta, int silu, void* y, int ldy, float* ss, float* ws, void* stream);
/* Same; tickets = B*G zeroed ints (left zeroed): the statistics pass also finalizes (one launch less). */
int tair_k_groupnorm_ex(const void* x, int ldx, int B, int HW, int C, int G, float eps, const float* gamma,
                        const float* beta, int silu, void* y, int ldy, float* ss, float* ws, int* tickets,
                        void* stream);
/* LayerNorm over C (attention.py:255-257). */
int tair_k_layernorm(const void* x, int T, int C, const float* gamma, const float* beta, float eps, void* y,
                     void* stream);
/* LayerNorm over C of a two-plane residual stream (the text tower's ln_1 / ln_2 / ln_final, open_clip
 * transformer.py:199-256, clip.py:43): x = x[t * ldx + c] + x[t * ldx + x_lo + c] (x_lo = 0: one plane), statistics
 * and apply in fp32; out_f32 0 writes bf16 rows (the next GEMM's operand), 1 fp32 rows (ln_final: the context the
 * sampler takes), row stride ldy elements.  C % 8 == 0, C <= 2560. */
int tair_k_layernorm_split(const void* x, int ldx, int x_lo, int T, int C, const float* gamma, const float* beta,
                           float eps, void* y, int ldy, int out_f32, void* stream);
/* The SwinIR cleaner's shifted-window attention (swinir.py:37-151 WindowAttention, :222-285 SwinTransformerBlock):
 * softmax(q k^T * scale + relative-position bias + shift mask) v per 8x8 window and head of a [B, H, W] token map.
 * Rows are pixels b * H * W + y * W + x, bf16; head h is at columns 32 h of q / k / v / o (operands may be strided
 * out of one fused [T, 3 * 32 heads] buffer; leading dimensions % 8 == 0, 16-byte aligned pointers); d <= 32 is the
 * real head dim: columns d..31 of a head are read as zero whatever they hold and written as zero in o.  The cyclic
 * shift (torch.roll by -shift, :260-266) and window_partition (:37-51) are addressing: token (iy, ix) of window
 * (wy, wx) is pixel ((8 wy + iy + shift) mod H, (8 wx + ix + shift) mod W), for the reads and for the write.  The mask
 * (:222-243) comes from coordinates: y' = 8 wy + iy has region 0 if y' < H - 8, 1 if y' < H - shift, else 2, likewise
 * x'; two tokens whose regions differ get the reference's finite -100; shift = 0: no mask.  bias_table fp32
 * [225][heads] as the checkpoint stores it, entry (iy_q - iy_k + 7) * 15 + (ix_q - ix_k + 7) (:99-117).  Softmax in
 * fp32 over the window's 64 keys in one pass, P rounded to bf16, both products on the bf16 MFMA.  H, W multiples of
 * 8, 0 <= shift < 8.  Bad arguments: -1 with a message, before any launch. */
int tair_k_window_attention(const void* q, int ldq, const void* k, int ldk, const void* v, int ldv, void* o, int ldo,
                            int B, int H, int W, int heads, int d, int shift, const float* bias_table, float scale,
                            void* stream);
/* tair_k_layernorm_split for a channel count that is a multiple of 4 but not of 8 (SwinIR's 180: norm1 / norm2,
 * patch_embed.norm, norm; swinir.py:245-285, :841-860), in rows padded to Cp columns: statistics over columns [0, C)
 * of hi + lo (x_lo = 0: one plane), bf16 rows of stride ldy with zeros written to columns [C, Cp) (the next GEMM's
 * K padding).  C % 4 == 0, C <= 1024, Cp >= C, Cp % 4 == 0.  Bad arguments: -1 with a message, before any launch. */
int tair_k_layernorm_split_pad(const void* x, int ldx, int x_lo, int T, int C, int Cp, const float* gamma,
                               const float* beta, float eps, void* y, int ldy, void* stream);
/* LeakyReLU in place on bf16 rows (swinir.py:868-880: conv_before_upsample slope 0.01, conv_up* / conv_hr slope 0.2):
 * x[r * ld + c] = x > 0 ? x : bf16(float(x) * slope) for c < C, bitwise F.leaky_relu on bf16.  C % 8 == 0, ld % 8 == 0,
 * ld >= C.  Bad arguments: -1 with a message, before any launch. */
int tair_k_leaky_relu(void* x, int ld, int rows, int C, float slope, void* stream);
/* LayerNorm over C with e4m3 output for the fp8 linears (configs[4]): y8 [T][ld8] bytes (OCP e4m3,
 * bytes C..ld8 zeroed), s8 [T] per-token scale (max |y| / 448): y ~= y8 * s8. */
int tair_k_layernorm_fp8(const void* x, int T, int C, const float* gamma, const float* beta, float eps, void* y8,
                         int ld8, float* s8, void* stream);
/* Per-output-channel e4m3 quantisation of a bf16 weight [rows][ldw] (first K columns) into q [rows][ldq]
 * bytes (zero-padded) and scale [rows] = max |w| / 448. */
int tair_k_quant_rows_fp8(const void* w, int rows, int K, int ldw, void* q, int ldq, float* scale, void* stream);
/* fp8 weights of a GroupNorm-fed consumer (configs[4] ResBlock convs / proj_in, unet.py:203-223): q[r][k] =
 * e4m3(w[r][k] a[k] / s[r]) for k < K (zero to k8), s[r] = the power of two >= max |w a| / 448, a = the
 * static per-K-column activation scale (null = 1), then the Kx bf16 K-extension columns as w[r][K+j] / s[r]
 * at byte k8 + 2j; q rows of ldq bytes. */
int tair_k_quant_rows_fp8_ex(const void* w, int rows, int K, int Kx, int ldw, const float* a, void* q, int ldq, int k8,
                             float* scale, void* stream);
/* GroupNorm(+SiLU) apply from producer statistics with e4m3 output: y8[row][c] = e4m3(bf16(y) * inv8[c])
 * (inv8 = 1 / the consumer's static power-of-two activation scale), rows of ld8 bytes, C..ld8 zeroed. */
int tair_k_gn_apply_fp8(const void* x, int ldx, int x_lo, int B, int HW, int C, int G, float eps, const float* gamma,
                        const float* beta, int silu, const double* st, int st_rs, const float* inv8, void* y8, int ld8,
                        void* stream);
/* Host routine (no device work): the composed FF-out + proj_out weight of a SpatialTransformer as finalize packs it.
 * wpout [C][C], wff2 [C][4C], bff2 [C], bpout [C] fp32 -> packed [C][ldp] bf16 bits (ldp >= 5C; row n holds
 * sum_j wpout[n][j] wff2[j][k] for k < 4C, then wpout[n][k - 4C] for 4C <= k < 5C, zeros beyond) and bias [C] =
 * wpout . bff2 + bpout.  The GEMM reads it with K = 4C against the GEGLU output and Kx = C against the
 * transformer stream. */
int tair_k_compose_ffpout(const float* wpout, const float* wff2, const float* bff2, const float* bpout, int C,
                          void* packed, int ldp, float* bias);
/* GEGLU: [T, 2D] -> x * gelu(gate) (attention.py:19-26). */
int tair_k_geglu(const void* xg, int T, int D, void* y, void* stream);

/* One fused SpacedSampler update on caller-owned device buffers (spaced_sampler.py:141-189; the kernel
 * tair_sampler_run launches per step), for a caller that drives its own loop:
 *   v  = v_uncond ? v_uncond + scales[i] * (v - v_uncond) : v            (classifier-free guidance, :163)
 *   x0 = tab0[t] x - tab1[t] v;  mean = tab2[t] x0 + tab3[t] x;  x = mean + [t != 0] sqrt(tab4[t]) noise[i]
 * with i = counter[0] (loop index), n = counter[1] (steps of the schedule), t = n - 1 - i, all read on the
 * device (the call is capturable and never synchronises; i outside [0, n) writes nothing; the caller
 * advances the counter).  x [rows, C] fp32 NHWC in/out; v [rows, C] fp32, the guided v is written back to
 * it when v_uncond is given; tables = the 5 rows of tair_sampler_set_schedule, [5][n]; scales [n] guidance
 * scale per loop index (may be NULL without v_uncond); noise [n][rows, C].  The new x also leaves as
 * (hi, lo, hi) bf16 planes, hi = bf16(x), lo = bf16(x - hi): in_u[row * ld + {0, C, 2C} + c] and, unless
 * in_c is NULL, in_c[row * ld + {0, ldc, 2 ldc} + c]; half_rows > 0 writes the same planes again half_rows
 * rows further on (the uncond half of a 2B-row model input).  Other channels of a row are left alone. */
int tair_k_sampler_step(float* x, float* v, const float* v_uncond, const float* tables, const float* scales,
                        const int* counter, const float* noise, int rows, int C, void* in_u, void* in_c, int ld,
                        int ldc, int half_rows, void* stream);

/* Latent tiling inside the sampling loop on caller-owned device buffers (utils/common.py:125-234
 * make_tiled_fn; the two kernels tair_sampler_run launches around every forward of a tiled run), for a
 * caller that drives its own loop.  Geometry: B images of a whole latent H x W, tile x tile windows at
 * `stride` (starts 0, stride, ... plus one flush with the edge when the stride does not divide; row-major;
 * T per image), job rows j = b * T + k run as n_chunks forwards of rows_per_chunk rows each
 * (n_chunks * rows_per_chunk >= B * T and every chunk holds a job row; the surplus rows of the last chunk
 * are pad).  *chunk is the current chunk, read on the device; a value outside [0, n_chunks) writes nothing.
 * Both calls are capturable and never synchronise; a bad shape argument is -1 with a message, before any
 * launch.
 *
 * tair_k_tile_gather: x [B*H*W, C] fp32 NHWC (the whole-latent state), hint [B*H*W, hint_channels] (needed
 * with in_c).  Row r of the chunk gets its window as (hi, lo, hi) bf16 planes, hi = bf16(x), lo =
 * bf16(x - hi): in_u[(r * tile^2 + p) * ld + {0, C, 2C} + c] and, unless in_c is NULL,
 * in_c[... + {0, ldc, 2 ldc} + c] with the hint planes at channel C (the layout tair_k_sampler_step
 * writes).  half_rows > 0 writes the planes again half_rows plane rows further on (the uncond half of a
 * guided forward), with hint_uncond (NULL = hint) as that half's hint.  A pad row gets the job's last
 * window.  Other channels of a row are left alone. */
int tair_k_tile_gather(const float* x, const float* hint, const float* hint_uncond, const int* chunk, int B, int H,
                       int W, int tile, int stride, int rows_per_chunk, int n_chunks, int C, int hint_channels,
                       void* in_u, void* in_c, int ld, int ldc, int half_rows, void* stream);
/* tair_k_tile_blend_step: v [rows_per_chunk * tile^2, C] fp32 is the forward's output for the chunk (guided,
 * acc_uncond != NULL: the uncond half follows rows_per_chunk * tile^2 rows further on).  One thread per
 * whole-latent element adds, over the chunk's windows that cover its pixel in ascending window order,
 *   acc += v_k * w,  cnt += w        (weights [tile^2] fp32; acc, acc_uncond, cnt [B*H*W, C] fp32, zero at start)
 * so the sums do not depend on the chunking; pad rows are never read.  A pixel that only one window of the
 * job covers accumulates v itself and keeps it unchanged (the reference's fl(fl(v w) / w) is within one ulp of
 * it; a latent of one window thereby reproduces the untiled step exactly).  On the last chunk of the step:
 *   v = acc / cnt  (guided: v_u + scales[i] * (v_c - v_u), both halves blended first, spaced_sampler.py:149-164)
 * is stored to v_blend [B*H*W, C], x [B*H*W, C] gets the update of tair_k_sampler_step against noise
 * [n][B*H*W, C] with i = counter[0], n = counter[1] (i outside [0, n) writes nothing), and the accumulators
 * are cleared.  Then *chunk advances, or returns to 0 with counter[0] += 1 after the last chunk. */
int tair_k_tile_blend_step(float* x, const float* v, float* v_blend, float* acc, float* acc_uncond, float* cnt,
                           const float* weights, const float* tables, const float* scales, int* counter, int* chunk,
                           const float* noise, int B, int H, int W, int tile, int stride, int rows_per_chunk,
                           int n_chunks, int C, void* stream);

/* Tiling of the SwinIR cleaner over an image larger than one tile (utils/common.py:174-234 make_tiled_fn as
 * pipeline.py:371-397 wraps the cleaner: scale 1, Gaussian weights, fp32 accumulators, no padding), the two kernels
 * HipSwinIR.forward_tiled launches around every chunk of window rows.  Geometry: B images [3, H, W], tile x tile
 * windows (tile a multiple of 64, <= H and W) at `stride` (starts 0, stride, ... plus one flush with the edge when
 * the stride does not divide, so a window may start at any pixel; row-major; T per image), job rows j = b * T + k.
 * A call handles the `rows` chunk rows that start at job row `first` (0 <= first < B * T, rows >= 1); a chunk row
 * past the job's last row is a pad row.  Both calls are capturable and never synchronise; a bad argument (tile not
 * a multiple of 64 or larger than the image, stride < 1, first / rows out of range, a null pointer, ld too small)
 * is -1 with a message, before any launch.
 *
 * tair_k_image_tile_gather: x [B, 3, H, W] fp32 NCHW, mean [3] fp32.  Chunk row r gets its window as the network's
 * input: token (ty, tx) of the tile/8 x tile/8 token map is row r * (tile/8)^2 + ty * (tile/8) + tx of `in` (bf16,
 * ld elements a row), column c * 64 + dy * 8 + dx holds pixel (8 ty + dy, 8 tx + dx) of channel c of the window as
 * two planes, hi = bf16(u) at the column and lo = bf16(u - float(hi)) lo_off columns further on, u = fl(x - mean[c]):
 * bitwise the torch expression pixel_unshuffle(x - mean, 8) split hi | lo.  lo_off >= 192, lo_off + 192 <= ld, both
 * even, `in` 4-byte aligned.  A pad row gets the job's last window; other columns of a row are left alone. */
int tair_k_image_tile_gather(const float* x, const float* mean, int B, int H, int W, int tile, int stride, int first,
                             int rows, void* in, int ld, int lo_off, void* stream);
/* tair_k_image_tile_blend: v [rows * tile^2, 3] fp32 NHWC is the network's output for the chunk (conv_last's rows as
 * they stand), weights [tile^2] fp32.  One thread per image element (b, c, y, x) adds, over the chunk's job rows
 * whose window covers the pixel, in ascending window order,
 *   acc = fl(acc + fl(v * w)),  cnt = fl(cnt + w)     (the product is rounded before it is added)
 * into acc, cnt [B, 3, H, W] fp32; with first == 0 both start from zero inside the kernel (no memset).  Chunks
 * ascend and windows ascend inside a chunk, so the sums are the reference loop's and do not depend on the chunking;
 * pad rows are never read.  finalize != 0 (only on the chunk that ends the job): out [B, 3, H, W] = acc / cnt, an
 * IEEE-rounded division, instead of storing the accumulators.  A pixel under a single window is fl(fl(v w) / w),
 * as in the reference (unlike tair_k_tile_blend_step). */
int tair_k_image_tile_blend(const float* v, const float* weights, float* acc, float* cnt, float* out, int B, int H,
                            int W, int tile, int stride, int first, int rows, int finalize, void* stream);

/* Overlap-blend stitch of decoded tiles on the device (val_patches.py:114-206 merge_patches_with_overlap,
 * stride generalised): tiles [n_tiles][C][patch][patch] fp32 on a raster nh x nw grid, out [C][H][W]
 * fp32 cropped; rtab[i] = fp32((i+1)/overlap), i < overlap (device).  Bitwise the reference loop. */
int tair_k_merge_overlap(const float* tiles, int n_tiles, int nh, int nw, int patch, int overlap, int stride,
                         float* out, int C, int H, int W, const float* rtab, void* stream);

/* configs[3] stitch fused with the tile exchange (replaces the all-gather + merge of
 * val_patches.py:114-206 / image_splitter.py:23-51 across ranks): src_ptrs = device array of `world`
 * pointers, rank r's contiguous block of per_rank tiles [C][patch][patch] fp32 (peer buffers mapped by
 * tair_ipc_open); the image-major global tile list g -> (g / per_rank, g % per_rank).  out
 * [n_images][C][H][W] fp32 = the global images first_image .. first_image + n_images - 1 (a rank stitches
 * the images it owns, reading only the tiles that cover them).  mode 0: non-overlap placement (H = nh * patch); mode 1: overlap blend,
 * bitwise tair_k_merge_overlap (rtab as there). */
int tair_k_stitch_peers(const void* src_ptrs, int per_rank, int first_image, int n_images, int tiles_per_image,
                        int nh, int nw,
                        int mode, int patch, int overlap, int stride, float* out, int C, int H, int W,
                        const float* rtab, void* stream);
/* IPC export / import of a device buffer for peer reads: handle_out receives TAIR_IPC_HANDLE_BYTES
 * (the allocation's handle) and *offset the buffer's byte offset inside that allocation; tair_ipc_open
 * maps a peer's allocation (base pointer; add the exporter's offset), tair_ipc_close unmaps it. */
#define TAIR_IPC_HANDLE_BYTES 64
int tair_ipc_get_handle(const void* dev_ptr, void* handle_out, unsigned long long* offset);
int tair_ipc_open(const void* handle, void** dev_ptr);
int tair_ipc_close(void* dev_ptr);

/* GroupNorm(+SiLU) apply from producer statistics (a GEMM epilogue's st_acc; vae.py:18-21 eps 1e-6,
 * util.py:191-193): x_lo > 0 reads a split input x[c] + x[x_lo + c]; y_split writes hi/lo/hi planes. */
int tair_k_gn_apply_stats(const void* x, int ldx, int x_lo, int B, int HW, int C, int G, float eps, const float* gamma,
                          const float* beta, int silu, const double* st, int st_rs, void* y, int ldy, int y_split,
                          void* stream);
/* Row softmax of fp32 scores (rows x L, row stride lds) into hi/lo/hi bf16 planes [rows][3L]
 * (vae.py:120-180 AttnBlock, softmax over the keys). */
int tair_k_softmax_split(const float* S, int lds, int rows, int L, void* P, void* stream);
/* [B][L][3C] (hi, lo, hi) -> [B][C][3L] (hi, hi, lo): the V^T operand of P.V. */
int tair_k_transpose_split(const void* x, int B, int L, int C, void* y, void* stream);
/* The two above for a token count L that is no multiple of 64 (the tiles of the tiled VAE, tilevae.py:307-579:
 * 30x30, 30x24, ... latent): the planes are Lp columns wide (Lp >= L, Lp % 64 == 0), P [rows][3 Lp] and
 * y [B][C][3 Lp], with zeros at columns L..Lp of every plane, so P.V runs as a GEMM over K = 3 Lp and the padded
 * keys contribute exactly zero.  Columns L.. of S are never read.  Bad arguments: -1 with a message, no launch. */
int tair_k_softmax_split_pad(const float* S, int lds, int rows, int L, int Lp, void* P, void* stream);
int tair_k_transpose_split_pad(const void* x, int B, int L, int Lp, int C, void* y, void* stream);
/* Cross-tile GroupNorm of the tiled VAE (tilevae.py:232-278 GroupNormParam.summary).  slots: T statistics slots
 * in the st_acc layout (8 replicas st_rs doubles apart, (b * G + g) * 2 = (sum x, sum x^2)), slot t at
 * slots + t * slot_stride doubles, filled by the GEMM that produced tile t: pixels[t] (host array) pixels per
 * image, groups of cg channels.  Per (b, g) in fp64: mean_t, var_t = max(sum x^2 / cnt_t - mean_t^2, 0) with
 * cnt_t = pixels[t] * cg; mean = sum_t w_t mean_t, var = sum_t w_t var_t, w_t = pixels[t] / sum pixels (the
 * reference's weighted average of variances, not the union's variance); every slot is rewritten as replica 0 =
 * (mean cnt_t, (var + mean^2) cnt_t), replicas 1-7 = 0, so tair_k_gn_apply_stats with that tile's own HW
 * normalises with the merged pair.  T <= 256.  Bad arguments (T < 1, B < 1, a pixel count < 1, null pointers,
 * st_rs < 2 B G, overlapping slots): -1 with a message, before any launch. */
int tair_k_gn_stats_merge(double* slots, int64_t slot_stride, int T, const int* pixels, int B, int G, int cg,
                          int st_rs, void* stream);
/* Multi-scale deformable attention sampling of the stage-3 TESTR spotter, replacing the reference's
 * MSDeformAttnFunction / ms_deformable_im2col_gpu_kernel (testr/adet/layers/ms_deform_attn.py:19-37,
 * csrc/DeformAttn/ms_deform_im2col_cuda.cuh:238-299): fp32 value (N, S, M, D), level shapes
 * level_hw[2l] = H_l, [2l+1] = W_l (host array, L <= 8, levels consecutive along S), loc (N, Q, M, L, P, 2)
 * as (x, y) in [0, 1], attn (N, Q, M, L, P) -> out (N, Q, M*D).  grid_sample bilinear semantics
 * (align_corners = False, zero padding). */
int tair_k_ms_deform_attn(const float* value, int N, int S, int M, int D, const int* level_hw, int L, int Q, int P,
                          const float* loc, const float* attn, float* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* TAIR_KERNELS_H */
