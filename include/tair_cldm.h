/* tair_cldm.h — C ABI of the MI355X-native ControlLDM denoising path (libtair_cldm.so).
 *
 * The reference exposes this path only as Python nn.Module calls (no FFI); each entry point below
 * names the reference interface it replaces.  Conventions:
 *   - every function returns 0 (TAIR_OK) or a negative status; never throws across the ABI;
 *     tair_last_error() returns a thread-local message for the last failure;
 *   - device pointers are plain `void*`/`float*` into HBM; the stream is a hipStream_t;
 *   - forward/step/run perform no host synchronisation and no allocation (workspace is sized at
 *     create for max_batch), so they can be captured into a hipGraph; one handle per device,
 *     re-entrant per (handle, stream) only.
 */
#ifndef TAIR_CLDM_H
#define TAIR_CLDM_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TAIR_OK 0
#define TAIR_ERR_ARG (-1)
#define TAIR_ERR_HIP (-2)
#define TAIR_ERR_STATE (-3)
#define TAIR_ERR_KEY (-4)

#define TAIR_DTYPE_F32 0
#define TAIR_DTYPE_BF16 1
/* compute_dtype TAIR_DTYPE_FP8: configs[4]'s fp8 weights -- a selectable set of layer classes runs as OCP
 * e4m3 x e4m3 MX-scale MFMA (environment TAIR_FP8_OPS, bit mask: 1 ResBlock conv1, 2 identity-skip ResBlock
 * conv2, 4 skip-conv ResBlock conv2, 8 SpatialTransformer proj_in, 16 the LayerNorm-fed linears attn1 q|k|v,
 * attn2 q and GEGLU proj).  Default 18 = the LayerNorm-fed linears (per-output-channel weight scales,
 * per-token activation scales written by the LayerNorm) + identity-skip conv2 (static per-channel activation
 * scales of the GroupNorm output folded into the weights): the set that keeps the 50-step image gate
 * (DESIGN.md §4.6).  The attention out-projections, FF-out and proj_out always stay bf16. */
#define TAIR_DTYPE_FP8 2

typedef struct tair_cldm tair_cldm;
typedef void* tair_stream_t; /* hipStream_t */

/* Architecture hyper-parameters — configs/val/val_terediff_baidu_crop.yaml:6-67 (unet_cfg,
 * controlnet_cfg).  attention_ds lists the downsample factors that carry a SpatialTransformer. */
typedef struct {
  int model_channels;      /* 320 */
  int num_levels;          /* len(channel_mult) = 4 */
  int channel_mult[8];     /* 1,2,4,4 */
  int num_res_blocks;      /* 2 */
  int num_attention_ds;    /* 3 */
  int attention_ds[8];     /* 4,2,1 */
  int head_channels;       /* 64 */
  int context_dim;         /* 1024 */
  int context_len;         /* 77 */
  int in_channels;         /* 4 */
  int hint_channels;       /* 4 */
  int out_channels;        /* 4 */
  int groups;              /* 32 */
  int max_batch;           /* tiles per forward (workspace sizing) */
  int latent_h, latent_w;  /* 64 x 64 for a 512^2 tile */
  int compute_dtype;       /* TAIR_DTYPE_BF16, or TAIR_DTYPE_FP8 (see above) */
  int manifest_only;       /* 1: build the parameter manifest only, no device allocation (CPU) */
} tair_cldm_cfg;

/* Replaces: ControlLDM.__init__ (terediff/model/cldm.py:22-31) with the yaml above. */
int tair_cldm_default_cfg(tair_cldm_cfg* cfg);
int tair_cldm_create(const tair_cldm_cfg* cfg, tair_cldm** out);
int tair_cldm_destroy(tair_cldm* h);

/* Parameter manifest in reference state_dict naming ("unet.*", "controlnet.*"):
 * Replaces: ControlLDM.state_dict() key layout (cldm.py:33-66, initialize.py:86-100). */
int tair_cldm_param_count(const tair_cldm* h, int* n);
int tair_cldm_param_info(const tair_cldm* h, int i, const char** key, int64_t shape[4], int* ndim);
/* Replaces: load_pretrained_sd / load_controlnet_from_ckpt (cldm.py:33-66).  src is a HOST
 * pointer to a contiguous tensor of the given dtype/shape; weights are packed (NHWC-K-major,
 * fused q|k|v, fused skip-conv K-extension, concatenated emb_layers) into device bf16 buffers. */
int tair_cldm_load_param(tair_cldm* h, const char* key, const void* src, int src_dtype,
                         const int64_t* shape, int ndim);
/* Checks every parameter was loaded and uploads the fused bias vectors. */
int tair_cldm_finalize(tair_cldm* h);

typedef struct {
  int batch;                   /* B <= max_batch */
  const float* x;              /* [B, 4, h, w] fp32 NCHW (x_noisy) */
  const int64_t* t;            /* [B] raw model timesteps 0..999 */
  const float* c_txt;          /* [c_txt_batch, 77, 1024] fp32 */
  int c_txt_batch;             /* 1 = broadcast to every tile, or B */
  const float* c_img;          /* [B, 4, h, w] fp32 or NULL (no ControlNet) */
  const float* control_scales; /* HOST [13] or NULL (= 1.0) */
  float* out;                  /* [B, 4, h, w] fp32 v-prediction */
  float* feats[4];             /* NCHW fp32 decoder features (out blocks 2,5,8,11) or NULL */
} tair_cldm_io;

/* Replaces: ControlLDM.forward(x_noisy, t, cond) -> (v, extracted_feats) (cldm.py:160-179). */
int tair_cldm_forward(tair_cldm* h, const tair_cldm_io* io, tair_stream_t stream);

/* ---- fused SpacedSampler (spaced_sampler.py:77-243) ------------------------------------- */
/* Replaces: SpacedSampler.make_schedule (spaced_sampler.py:77-121).  model_t[i] = timestep used at
 * loop index i (descending, 999..0); tables = 5 rows x n_steps fp32, indexed by t = n-1-i:
 * sqrt_alphas_cumprod, sqrt_one_minus_alphas_cumprod, posterior_mean_coef1,
 * posterior_mean_coef2, posterior_variance (all HOST pointers). */
int tair_sampler_set_schedule(tair_cldm* h, int n_steps, const int64_t* model_t, const float* tables);

typedef struct {
  int batch;
  const float* x_T;            /* [B,4,h,w] fp32 */
  const float* noise;          /* [n_steps, B, 4, h, w] fp32 (explicit per-step noise) */
  const float* c_txt;          /* [c_txt_batch, 77, 1024] */
  int c_txt_batch;
  const float* c_img;          /* [B,4,h,w] or NULL */
  const float* control_scales; /* HOST [13] or NULL */
} tair_sampler_io;

/* Uploads the per-restoration invariants: time-embedding tables for every step (one batched GEMM),
 * cross-attention K/V of c_txt, hint/x_T layout conversion, noise re-layout; resets step counter. */
int tair_sampler_prepare(tair_cldm* h, const tair_sampler_io* io, tair_stream_t stream);

/* Classifier-free guidance (spaced_sampler.py:149-167, sampler.py:31-38): the negative-prompt half of a
 * guided restoration.  Each step then runs the network once at batch 2B (rows [0,B) cond, [B,2B) uncond)
 * and the fused update forms v = v_uncond + scales[i] * (v_cond - v_uncond) before p_sample. */
typedef struct {
  const float* c_txt;    /* [c_txt_batch, 77, ctx] negative-prompt context */
  int c_txt_batch;       /* 1 or B, independent of the cond's */
  const float* c_img;    /* [B,4,h,w], or NULL = the cond's c_img */
  const float* scales;   /* HOST [n_steps]: guidance scale at loop index i */
} tair_guidance_io;
/* tair_sampler_prepare with guidance.  g == NULL is exactly tair_sampler_prepare.  Otherwise 2 * batch <=
 * max_batch, and ControlNet runs for both halves or neither (g->c_img without io->c_img is an error):
 * TAIR_ERR_ARG with a message.  The scales are copied into a device table at a fixed address (this call
 * waits for that copy on the host; tair_sampler_run never synchronises), so other scales need no new
 * graph, while a guided and an unguided run never replay each other's.  After a guided prepare:
 * tair_sampler_set_context re-encodes the cond half only (the negative context stays), tair_sampler_get_x
 * returns the decoder features of the cond half (rows [0,B)), and tair_sampler_get_v the guided v. */
int tair_sampler_prepare_guided(tair_cldm* h, const tair_sampler_io* io, const tair_guidance_io* g,
                                tair_stream_t stream);
/* Latent tiling inside the sampling loop (utils/common.py:125-234 make_tiled_fn, wired as in
 * ddim_sampler.py:165-180 and passed to every sampler by pipeline.py:211-213): a whole latent larger than the
 * handle's latent_h x latent_w tile.  Every step runs the network on the overlapping tile-sized windows of
 * the latent (sliding_windows: starts 0, stride, ... plus one flush with the edge; row-major), blends the
 * window outputs with Gaussian weights (gaussian_weights, var 0.01) and runs p_sample on the whole latent. */
typedef struct {
  int height, width; /* the whole latent, H x W >= latent_h x latent_w */
  int stride;        /* window stride in latent pixels, >= 1 */
} tair_tiling_io;
/* tair_sampler_prepare_guided with latent tiling.  t == NULL is exactly tair_sampler_prepare_guided.
 * Otherwise io->batch is the number of images B (any B >= 1), io->x_T and io->c_img (and g->c_img) are
 * [B,4,H,W], io->noise is [n_steps,B,4,H,W], and the contexts are shared by every window: c_txt_batch must
 * be 1 for both halves.  The N = B * T window rows of a step (image-major, then window order) run as
 * ceil(N / cap) forwards of equal row count, cap = max_batch (g == NULL) or max_batch / 2 (guided: cond
 * rows, then uncond rows, each half blended before the guidance sum); the unused rows of the last forward
 * repeat the last window and are never blended.  TAIR_ERR_ARG with a message: latent_h != latent_w, H or W
 * below the tile, stride < 1, a c_txt_batch other than 1, cap == 0.  The whole-latent buffers (state, noise,
 * hints, accumulators, blended v, weight table) are allocated here, never in tair_sampler_run; they only
 * grow, so their addresses stay fixed across replays, and a reallocation drops the captured graphs.  After
 * a tiled prepare: tair_sampler_run(n) runs n steps of n_chunks forwards each (one captured graph per
 * forward, replayed with the chunk index on the device; a tiled and an untiled run never replay each
 * other's graph), tair_sampler_get_x returns [B,4,H,W] and refuses feats (per-window decoder features have
 * no whole-image meaning: TAIR_ERR_ARG), tair_sampler_get_v returns the blended (guided) v [B,4,H,W], and
 * tair_sampler_set_context accepts a batch-1 context. */
int tair_sampler_prepare_tiled(tair_cldm* h, const tair_sampler_io* io, const tair_guidance_io* g,
                               const tair_tiling_io* t, tair_stream_t stream);
/* The plan of the last tiled prepare: windows per image, forwards per step, window rows per forward, unused
 * rows of the last forward (all 0 after an untiled prepare). */
int tair_sampler_tiling_info(const tair_cldm* h, int* windows, int* chunks, int* rows_per_chunk, int* pad);
/* Re-encodes the cross-attention K/V caches from a new c_txt (stage-3 val_sample, :317). */
int tair_sampler_set_context(tair_cldm* h, const float* c_txt, int c_txt_batch, tair_stream_t stream);
/* Runs n steps of p_sample (ControlNet + UNet + fused update) from the device step counter.
 * use_graph != 0 captures one step into a hipGraph on first use and replays it. */
int tair_sampler_run(tair_cldm* h, int n_steps, int use_graph, tair_stream_t stream);
/* Current latent x as [B,4,h,w] fp32; optional decoder features of the last step. */
int tair_sampler_get_x(tair_cldm* h, float* x_out, float* feats[4], tair_stream_t stream);
/* The v-prediction of the last step that ran, as [B,4,h,w] fp32 (the model output p_sample consumed:
 * x0_hat = sqrt_alphas_cumprod[t] * x_t - sqrt_one_minus_alphas_cumprod[t] * v, spaced_sampler.py:141-147).
 * Parity instrumentation for the per-step x0 check; not needed by the sampling loop. */
int tair_sampler_get_v(tair_cldm* h, float* v_out, tair_stream_t stream);

/* ---- instrumentation -------------------------------------------------------------------- */
/* Per kernel-class timing with HIP events around every launch on the given stream (eager
 * only).  class ids: 0 gemm/conv, 1 attention, 2 groupnorm, 3 layernorm, 4 other. */
int tair_profile_enable(tair_cldm* h, int enable);
int tair_profile_read(tair_cldm* h, int cls, double* total_ms, int* launches, double* flops);
/* Per-launch CSV (class, microseconds, GFLOP, TFLOP/s, shape tag) of the profiled launches. */
int tair_profile_dump(tair_cldm* h, const char* path);
/* Algorithmic FLOPs of one forward at the given batch (convs + linears + attention bmm). */
int tair_cldm_flops(const tair_cldm* h, int batch, double* flops);

const char* tair_last_error(void);
const char* tair_version(void);

#ifdef __cplusplus
}
#endif
#endif /* TAIR_CLDM_H */
