// Kernel-level C ABI (include/tair_kernels.h): thin, allocation-free wrappers over the launchers.
#include <cstring>
#include "kernels.h"
#include "tair_kernels.h"

using namespace tair;

extern "C" {

namespace {
GemmArgs gemm_args_of(const tair_gemm_desc* d) {
  GemmArgs a{};
  a.M = d->M; a.N = d->N; a.K = d->K; a.amode = d->amode;
  a.A = (const bf16*)d->A; a.lda = d->lda; a.C = d->C;
  a.Bn = d->Bn; a.H = d->H; a.W = d->W; a.Ho = d->Ho; a.Wo = d->Wo;
  a.X = (const bf16*)d->X; a.ldx = d->ldx; a.Kx = d->Kx;
  a.Wt = (const bf16*)d->Wt; a.ldw = d->ldw;
  a.alpha = d->alpha; a.scale_bias = d->scale_bias; a.act = d->act;
  a.bias = d->bias;
  a.emb = d->emb; a.ld_emb = d->ld_emb; a.emb_row = d->emb_row; a.rows_per_b = d->rows_per_b > 0 ? d->rows_per_b : 1;
  a.res = (const bf16*)d->res; a.ld_res = d->ld_res;
  a.out = d->out; a.ldo = d->ldo; a.out_f32 = d->out_f32;
  a.splits = 1; a.partial = d->partial; a.partial_cap = (size_t)d->partial_cap;
  a.force_bm = d->force_bm; a.force_bn = d->force_bn; a.force_splits = d->force_splits;
  a.force_stages = d->force_stages;
  a.tile_sem = d->tile_sem; a.sem_cap = d->sem_cap;
  a.out_split = d->out_split; a.res_lo = d->res_lo;
  a.out_lo = d->out_lo; a.x_wrap = d->x_wrap; a.probe = d->probe;
  a.f8 = d->f8; a.row_scale = d->row_scale; a.col_scale = d->col_scale;
  a.s2_shift = d->s2_shift;
  a.gn_st = d->gn_st;
  a.gn_rs = d->gn_rs;
  a.gn_G = d->gn_G;
  a.gn_eps = d->gn_eps;
  a.gn_gamma = d->gn_gamma;
  a.gn_beta = d->gn_beta;
  a.gn_silu = d->gn_silu;
  a.stamps = d->stamps;
  a.rst = d->rst; a.lnst = d->lnst; a.lncs = d->lncs; a.ln_c = d->ln_c; a.ln_eps = d->ln_eps;
  if (d->st_acc) {
    a.st[0].acc = d->st_acc; a.st[0].rs = d->st_rs; a.st[0].cg = d->st_cg; a.st[0].G = d->st_G;
    a.st[0].c_off = d->st_coff; a.st[0].hw = d->st_hw;
  }
  if (d->st2_acc) {  // (without st_acc: refused by gemm_grouped)
    a.st[1].acc = d->st2_acc; a.st[1].rs = d->st2_rs; a.st[1].cg = d->st2_cg; a.st[1].G = d->st2_G;
    a.st[1].c_off = d->st2_coff; a.st[1].hw = d->st_hw;
  }
  return a;
}
}  // namespace

int tair_k_gemm(const tair_gemm_desc* d, void* stream) {
  if (!d) return -1;
  const GemmArgs a = gemm_args_of(d);
  return gemm(a, (hipStream_t)stream) == hipSuccess ? 0 : -2;
}

int tair_fault_count(int reset, int* count) {
  if (!count) return -1;
  return gemm_fault_count(count, reset != 0) == hipSuccess ? 0 : -2;
}

int tair_k_gemm_desc_bytes(void) { return (int)sizeof(tair_gemm_desc); }

int tair_k_compose_ffpout(const float* wpout, const float* wff2, const float* bff2, const float* bpout, int C,
                          void* packed, int ldp, float* bias) {
  if (!wpout || !wff2 || !bff2 || !bpout || !packed || !bias || C < 1 || ldp < 5 * C) return -1;
  compose_ffpout(wpout, wff2, bff2, bpout, C, (uint16_t*)packed, ldp, bias);
  return 0;
}

int tair_k_gemm_plan(const tair_gemm_desc* d, int* bm, int* bn, int* splits, int* kern) {
  if (!d || !bm || !bn || !splits || !kern) return -1;
  const GemmArgs a = gemm_args_of(d);
  return gemm_plan_query(a, bm, bn, splits, kern) == hipSuccess ? 0 : -2;
}

namespace {
// the lanes of a grouped test entry: at most MAX_GROUP are converted; a count outside 1..MAX_GROUP goes to the
// launcher as it is, which refuses it before any launch
int lanes_of(int n) { return n < 0 ? 0 : n > MAX_GROUP ? MAX_GROUP : n; }
GnArgs gn_args_of(const tair_gn_lane& l, float eps) {
  GnArgs g{};
  g.x = (const bf16*)l.x; g.ldx = l.ldx; g.gamma = l.gamma; g.beta = l.beta; g.ss = l.ss; g.ws = l.ws;
  g.tickets = l.tickets; g.y = (bf16*)l.y; g.ldy = l.ldy; g.st = l.st; g.st_rs = l.st_rs; g.eps = eps;
  g.x_lo = l.x_lo; g.y_split = l.y_split; g.y8 = (uint8_t*)l.y8; g.ld8 = l.ld8; g.inv8 = l.inv8;
  return g;
}
}  // namespace

int tair_k_gemm_grouped(const tair_gemm_desc* d, int n, void* stream) {
  if (!d) return -1;
  GemmArgs a[MAX_GROUP] = {};
  for (int i = 0; i < lanes_of(n); ++i) a[i] = gemm_args_of(d + i);
  return gemm_grouped(a, n, (hipStream_t)stream) == hipSuccess ? 0 : -2;
}

int tair_k_gemm_plan_lanes(const tair_gemm_desc* d, int lanes, int* bm, int* bn, int* splits, int* kern) {
  if (!d || !bm || !bn || !splits || !kern || lanes < 1 || lanes > MAX_GROUP) return -1;
  const GemmArgs a = gemm_args_of(d);
  return gemm_plan_query(a, bm, bn, splits, kern, lanes) == hipSuccess ? 0 : -2;
}

int tair_k_gemm_grouped_check(const tair_gemm_desc* d, int n) {
  if (!d) return -1;
  GemmArgs a[MAX_GROUP] = {};
  for (int i = 0; i < lanes_of(n); ++i) a[i] = gemm_args_of(d + i);
  return gemm_grouped_check(a, n) == hipSuccess ? 0 : -2;
}

int tair_k_attention_grouped(const tair_attn_lane* l, int n, int B, int H, int Sq, int Skv, float scale,
                             int force_qsets, int force_splits, void* stream) {
  if (!l) return -1;
  AttnArgs a[MAX_GROUP] = {};
  for (int i = 0; i < lanes_of(n); ++i)
    a[i] = AttnArgs{(const bf16*)l[i].q, l[i].ldq, (const bf16*)l[i].k, l[i].ldk, (const bf16*)l[i].v, l[i].ldv,
                    (bf16*)l[i].o, l[i].ldo, l[i].kv_bstride, l[i].ws, l[i].ws ? (size_t)l[i].ws_bytes : 0,
                    l[i].tickets, l[i].tickets_cap};
  return attention_grouped(a, n, B, H, Sq, Skv, scale, (hipStream_t)stream, force_qsets, force_splits) == hipSuccess
             ? 0 : -2;
}

int tair_k_layernorm_grouped(const tair_ln_lane* l, int n, int T, int C, float eps, void* stream) {
  if (!l) return -1;
  LnArgs a[MAX_GROUP] = {};
  for (int i = 0; i < lanes_of(n); ++i)
    a[i] = LnArgs{(const bf16*)l[i].x, l[i].gamma, l[i].beta, (bf16*)l[i].y, (uint8_t*)l[i].y8, l[i].s8, l[i].ld8};
  return layernorm_grouped(a, n, T, C, eps, (hipStream_t)stream) == hipSuccess ? 0 : -2;
}

int tair_k_groupnorm_grouped(const tair_gn_lane* l, int n, int B, int HW, int C, int G, float eps, int silu,
                             void* stream) {
  if (!l) return -1;
  GnArgs a[MAX_GROUP] = {};
  for (int i = 0; i < lanes_of(n); ++i) {
    a[i] = gn_args_of(l[i], eps);
    a[i].st = nullptr;  // (this entry applies from the scale / shift it has just made)
  }
  hipStream_t s = (hipStream_t)stream;
  if (groupnorm_stats_grouped(a, n, B, HW, C, G, eps, s) != hipSuccess) return -2;
  return groupnorm_apply_grouped(a, n, B, HW, C, silu, s, G) == hipSuccess ? 0 : -2;
}

int tair_k_gn_apply_stats_grouped(const tair_gn_lane* l, int n, int B, int HW, int C, int G, float eps, int silu,
                                  void* stream) {
  if (!l) return -1;
  GnArgs a[MAX_GROUP] = {};
  for (int i = 0; i < lanes_of(n); ++i) a[i] = gn_args_of(l[i], eps);
  if (n >= 1 && n <= MAX_GROUP)
    for (int i = 0; i < n; ++i)
      if (!a[i].st) {
        set_error("gn_apply_stats_grouped: lane %d without producer statistics", i);
        return -1;
      }
  return groupnorm_apply_grouped(a, n, B, HW, C, silu, (hipStream_t)stream, G) == hipSuccess ? 0 : -2;
}

int tair_k_gemm_kgroup_force(int on) { return (int)gemm_set_kgroup_force(on != 0); }
int tair_k_kgroup_trips(int kt0, int kt1) { return kgroup_trips(kt0, kt1); }
int tair_k_kgroup_tile(int kt0, int g, int trip) { return kgroup_tile(kt0, g, trip); }

int tair_k_attention_plan(int B, int H, int Sq, int Skv, int64_t ws_bytes, int* qsets, int* splits, int* kv_split) {
  if (!qsets || !splits || !kv_split || B < 1 || H < 1 || Sq < 1 || Skv < 1) return -1;
  const AttnPlan p = attention_plan(B, H, Sq, Skv, ws_bytes < 0 ? (size_t)-1 : (size_t)ws_bytes);
  *qsets = p.qsets;
  *splits = p.splits;
  *kv_split = p.kv_split;
  return 0;
}

int tair_k_attention_plan_ex(int B, int H, int Sq, int Skv, int64_t ws_bytes, int force_qsets, int force_splits,
                             int* qsets, int* splits, int* kv_split) {
  if (!qsets || !splits || !kv_split || B < 1 || H < 1 || Sq < 1 || Skv < 1 || force_qsets < 0 || force_qsets > 2 ||
      force_splits < 0)
    return -1;
  const AttnPlan p = attention_plan(B, H, Sq, Skv, ws_bytes < 0 ? (size_t)-1 : (size_t)ws_bytes, force_qsets,
                                    force_splits);
  *qsets = p.qsets;
  *splits = p.splits;
  *kv_split = p.kv_split;
  return 0;
}

int tair_k_attention(const void* q, int ldq, const void* k, int ldk, const void* v, int ldv, void* o, int ldo,
                     int B, int H, int Sq, int Skv, int kv_bstride, float scale, void* stream) {
  return attention((const bf16*)q, ldq, (const bf16*)k, ldk, (const bf16*)v, ldv, (bf16*)o, ldo, B, H, Sq, Skv,
                   kv_bstride, scale, (hipStream_t)stream) == hipSuccess ? 0 : -2;
}

int tair_k_attention_ex(const void* q, int ldq, const void* k, int ldk, const void* v, int ldv, void* o, int ldo,
                        int B, int H, int Sq, int Skv, int kv_bstride, float scale, void* ws, int64_t ws_bytes,
                        int force_qsets, int force_splits, void* stream) {
  return attention((const bf16*)q, ldq, (const bf16*)k, ldk, (const bf16*)v, ldv, (bf16*)o, ldo, B, H, Sq, Skv,
                   kv_bstride, scale, (hipStream_t)stream, ws, ws ? (size_t)ws_bytes : 0, force_qsets,
                   force_splits) == hipSuccess ? 0 : -2;
}

int tair_k_attention_tk(const void* q, int ldq, const void* k, int ldk, const void* v, int ldv, void* o, int ldo,
                        int B, int H, int Sq, int Skv, int kv_bstride, float scale, void* ws, int64_t ws_bytes,
                        int* tickets, int tickets_cap, int force_qsets, int force_splits, void* stream) {
  AttnArgs a{(const bf16*)q, ldq, (const bf16*)k, ldk, (const bf16*)v, ldv, (bf16*)o, ldo, kv_bstride, ws,
             ws ? (size_t)ws_bytes : 0, tickets, tickets_cap};
  return attention_grouped(&a, 1, B, H, Sq, Skv, scale, (hipStream_t)stream, force_qsets, force_splits) ==
                 hipSuccess ? 0 : -2;
}

int tair_k_attention_causal(const void* q, int ldq, const void* k, int ldk, const void* v, int ldv, void* o, int ldo,
                            int B, int H, int S, float scale, void* stream) {
  const hipError_t e = attention_causal((const bf16*)q, ldq, (const bf16*)k, ldk, (const bf16*)v, ldv, (bf16*)o, ldo, B,
                                        H, S, scale, (hipStream_t)stream);
  if (e == hipErrorInvalidValue) {
    set_error("attention_causal: bad arguments (B %d, H %d, S %d (1..%d), scale %g, ld %d / %d / %d / %d: %% 8 and "
              ">= 64 H, 16-byte aligned pointers)", B, H, S, CAUSAL_MAX_S, (double)scale, ldq, ldk, ldv, ldo);
    return -1;
  }
  return e == hipSuccess ? 0 : -2;
}

int tair_k_embed_tokens(const void* ids, int B, int L, const float* table, int vocab, const float* pos, int C,
                        void* out_hi, int out_lo_offset, int ld, void* stream) {
  const hipError_t e = embed_tokens((const int64_t*)ids, B, L, table, vocab, pos, C, (bf16*)out_hi, out_lo_offset, ld,
                                    (hipStream_t)stream);
  if (e == hipErrorInvalidValue) {
    set_error("embed_tokens: bad arguments (B %d, L %d, vocab %d, C %d (%% 4), lo offset %d (>= C), ld %d)", B, L, vocab,
              C, out_lo_offset, ld);
    return -1;
  }
  return e == hipSuccess ? 0 : -2;
}

int tair_k_layernorm_split(const void* x, int ldx, int x_lo, int T, int C, const float* gamma, const float* beta,
                           float eps, void* y, int ldy, int out_f32, void* stream) {
  const hipError_t e = layernorm_split((const bf16*)x, ldx, x_lo, T, C, gamma, beta, eps, y, ldy, out_f32,
                                       (hipStream_t)stream);
  return e == hipSuccess ? 0 : e == hipErrorInvalidValue ? -1 : -2;
}

int tair_k_window_attention(const void* q, int ldq, const void* k, int ldk, const void* v, int ldv, void* o, int ldo,
                            int B, int H, int W, int heads, int d, int shift, const float* bias_table, float scale,
                            void* stream) {
  const hipError_t e = window_attention((const bf16*)q, ldq, (const bf16*)k, ldk, (const bf16*)v, ldv, (bf16*)o, ldo, B,
                                        H, W, heads, d, shift, bias_table, scale, (hipStream_t)stream);
  if (e == hipErrorInvalidValue) {
    set_error("window_attention: bad arguments (B %d, token map %dx%d (multiples of 8), heads %d, d %d (1..32), shift %d "
              "(0..7), scale %g, bias table %p, ld %d / %d / %d / %d: %% 8 and >= 32 heads, 16-byte aligned pointers)",
              B, H, W, heads, d, shift, (double)scale, (const void*)bias_table, ldq, ldk, ldv, ldo);
    return -1;
  }
  return e == hipSuccess ? 0 : -2;
}

int tair_k_layernorm_split_pad(const void* x, int ldx, int x_lo, int T, int C, int Cp, const float* gamma,
                               const float* beta, float eps, void* y, int ldy, void* stream) {
  const hipError_t e = layernorm_split_pad((const bf16*)x, ldx, x_lo, T, C, Cp, gamma, beta, eps, (bf16*)y, ldy,
                                           (hipStream_t)stream);
  if (e == hipErrorInvalidValue) {
    set_error("layernorm_split_pad: bad arguments (T %d, C %d (%% 4, <= 1024), Cp %d (>= C, %% 4), ldx %d, x_lo %d, "
              "ldy %d (>= Cp); ld %% 4, 8-byte aligned rows, 16-byte aligned gamma / beta)", T, C, Cp, ldx, x_lo, ldy);
    return -1;
  }
  return e == hipSuccess ? 0 : -2;
}

int tair_k_leaky_relu(void* x, int ld, int rows, int C, float slope, void* stream) {
  const hipError_t e = leaky_relu((bf16*)x, ld, rows, C, slope, (hipStream_t)stream);
  if (e == hipErrorInvalidValue) {
    set_error("leaky_relu: bad arguments (rows %d, C %d, ld %d: C, ld %% 8, ld >= C, 16-byte aligned pointer)", rows, C,
              ld);
    return -1;
  }
  return e == hipSuccess ? 0 : -2;
}

int tair_k_groupnorm(const void* x, int ldx, int B, int HW, int C, int G, float eps, const float* gamma,
                     const float* beta, int silu, void* y, int ldy, float* ss, float* ws, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  if (groupnorm_scale_shift((const bf16*)x, ldx, B, HW, C, G, eps, gamma, beta, ss, ws, s) != hipSuccess) return -2;
  return groupnorm_apply((const bf16*)x, ldx, B, HW, C, ss, silu, (bf16*)y, ldy, s) == hipSuccess ? 0 : -2;
}

int tair_k_groupnorm_ex(const void* x, int ldx, int B, int HW, int C, int G, float eps, const float* gamma,
                        const float* beta, int silu, void* y, int ldy, float* ss, float* ws, int* tickets,
                        void* stream) {
  hipStream_t s = (hipStream_t)stream;
  if (groupnorm_scale_shift((const bf16*)x, ldx, B, HW, C, G, eps, gamma, beta, ss, ws, s, tickets) != hipSuccess)
    return -2;
  return groupnorm_apply((const bf16*)x, ldx, B, HW, C, ss, silu, (bf16*)y, ldy, s) == hipSuccess ? 0 : -2;
}

int tair_k_layernorm(const void* x, int T, int C, const float* gamma, const float* beta, float eps, void* y,
                     void* stream) {
  return layernorm((const bf16*)x, T, C, gamma, beta, eps, (bf16*)y, (hipStream_t)stream) == hipSuccess ? 0 : -2;
}

int tair_k_layernorm_fp8(const void* x, int T, int C, const float* gamma, const float* beta, float eps, void* y8,
                         int ld8, float* s8, void* stream) {
  LnArgs a{(const bf16*)x, gamma, beta, nullptr, (uint8_t*)y8, s8, ld8};
  return layernorm_grouped(&a, 1, T, C, eps, (hipStream_t)stream) == hipSuccess ? 0 : -2;
}

int tair_k_quant_rows_fp8(const void* w, int rows, int K, int ldw, void* q, int ldq, float* scale, void* stream) {
  return quant_rows_fp8((const bf16*)w, rows, K, ldw, (uint8_t*)q, ldq, scale, (hipStream_t)stream) == hipSuccess
             ? 0 : -2;
}

int tair_k_quant_rows_fp8_ex(const void* w, int rows, int K, int Kx, int ldw, const float* a, void* q, int ldq, int k8,
                             float* scale, void* stream) {
  return quant_rows_fp8_ex((const bf16*)w, rows, K, Kx, ldw, a, (uint8_t*)q, ldq, k8, scale, (hipStream_t)stream) ==
                 hipSuccess ? 0 : -2;
}

int tair_k_gn_apply_fp8(const void* x, int ldx, int x_lo, int B, int HW, int C, int G, float eps, const float* gamma,
                        const float* beta, int silu, const double* st, int st_rs, const float* inv8, void* y8, int ld8,
                        void* stream) {
  GnArgs g{};
  g.x = (const bf16*)x; g.ldx = ldx; g.gamma = gamma; g.beta = beta;
  g.st = st; g.st_rs = st_rs; g.eps = eps; g.x_lo = x_lo;
  g.y8 = (uint8_t*)y8; g.ld8 = ld8; g.inv8 = inv8;
  return groupnorm_apply_grouped(&g, 1, B, HW, C, silu, (hipStream_t)stream, G) == hipSuccess ? 0 : -2;
}

int tair_k_geglu(const void* xg, int T, int D, void* y, void* stream) {
  return geglu((const bf16*)xg, T, D, (bf16*)y, (hipStream_t)stream) == hipSuccess ? 0 : -2;
}

int tair_k_sampler_step(float* x, float* v, const float* v_uncond, const float* tables, const float* scales,
                        const int* counter, const float* noise, int rows, int C, void* in_u, void* in_c, int ld,
                        int ldc, int half_rows, void* stream) {
  SamplerUpdateArgs a{x, v, v_uncond, tables, scales, counter, noise, rows, C, (bf16*)in_u, (bf16*)in_c, ld, ldc,
                      half_rows};
  const hipError_t e = sampler_update(a, (hipStream_t)stream);
  if (e == hipErrorInvalidValue) {
    set_error("sampler_step: bad arguments (rows %d, C %d, ld %d, ldc %d, half_rows %d)", rows, C, ld, ldc, half_rows);
    return -1;
  }
  return e == hipSuccess ? 0 : -2;
}

int tair_k_tile_gather(const float* x, const float* hint, const float* hint_uncond, const int* chunk, int B, int H,
                       int W, int tile, int stride, int rows_per_chunk, int n_chunks, int C, int hint_channels,
                       void* in_u, void* in_c, int ld, int ldc, int half_rows, void* stream) {
  TileGatherArgs a{x, hint, hint_uncond, chunk, (bf16*)in_u, (bf16*)in_c, C, hint_channels, ld, ldc, half_rows,
                   TileGeom{B, H, W, tile, stride, rows_per_chunk, n_chunks}};
  const hipError_t e = tile_gather(a, (hipStream_t)stream);
  if (e == hipErrorInvalidValue) {
    set_error("tile_gather: bad arguments (B %d, latent %dx%d, tile %d, stride %d, rows_per_chunk %d, n_chunks %d, "
              "C %d, hint_channels %d, ld %d, ldc %d, half_rows %d)", B, H, W, tile, stride, rows_per_chunk, n_chunks,
              C, hint_channels, ld, ldc, half_rows);
    return -1;
  }
  return e == hipSuccess ? 0 : -2;
}

int tair_k_tile_blend_step(float* x, const float* v, float* v_blend, float* acc, float* acc_uncond, float* cnt,
                           const float* weights, const float* tables, const float* scales, int* counter, int* chunk,
                           const float* noise, int B, int H, int W, int tile, int stride, int rows_per_chunk,
                           int n_chunks, int C, void* stream) {
  TileBlendArgs a{x, v, v_blend, acc, acc_uncond, cnt, weights, tables, scales, counter, chunk, noise, C,
                  TileGeom{B, H, W, tile, stride, rows_per_chunk, n_chunks}};
  const hipError_t e = tile_blend_step(a, (hipStream_t)stream);
  if (e == hipErrorInvalidValue) {
    set_error("tile_blend_step: bad arguments (B %d, latent %dx%d, tile %d, stride %d, rows_per_chunk %d, "
              "n_chunks %d, C %d, guided %d)", B, H, W, tile, stride, rows_per_chunk, n_chunks, C, acc_uncond != nullptr);
    return -1;
  }
  return e == hipSuccess ? 0 : -2;
}

int tair_k_image_tile_gather(const float* x, const float* mean, int B, int H, int W, int tile, int stride, int first,
                             int rows, void* in, int ld, int lo_off, void* stream) {
  const hipError_t e = image_tile_gather(x, mean, ImageTileGeom{B, H, W, tile, stride, first, rows}, (bf16*)in, ld,
                                         lo_off, (hipStream_t)stream);
  if (e == hipErrorInvalidValue) {
    set_error("image_tile_gather: bad arguments (B %d, image %dx%d, tile %d (%% 64, <= H, W), stride %d, first %d, "
              "rows %d, ld %d, lo_off %d (>= 192, even, lo_off + 192 <= ld), null x %d, mean %d, in %d)", B, H, W, tile,
              stride, first, rows, ld, lo_off, x == nullptr, mean == nullptr, in == nullptr);
    return -1;
  }
  return e == hipSuccess ? 0 : -2;
}

int tair_k_image_tile_blend(const float* v, const float* weights, float* acc, float* cnt, float* out, int B, int H,
                            int W, int tile, int stride, int first, int rows, int finalize, void* stream) {
  const hipError_t e = image_tile_blend(v, weights, acc, cnt, out, finalize,
                                        ImageTileGeom{B, H, W, tile, stride, first, rows}, (hipStream_t)stream);
  if (e == hipErrorInvalidValue) {
    set_error("image_tile_blend: bad arguments (B %d, image %dx%d, tile %d (%% 64, <= H, W), stride %d, first %d, "
              "rows %d, finalize %d (only on the chunk that ends the job, with out), null v %d, weights %d, acc %d, "
              "cnt %d, out %d)", B, H, W, tile, stride, first, rows, finalize, v == nullptr, weights == nullptr,
              acc == nullptr, cnt == nullptr, out == nullptr);
    return -1;
  }
  return e == hipSuccess ? 0 : -2;
}

int tair_k_merge_overlap(const float* tiles, int n_tiles, int nh, int nw, int patch, int overlap, int stride,
                         float* out, int C, int H, int W, const float* rtab, void* stream) {
  return merge_overlap(tiles, n_tiles, nh, nw, patch, overlap, stride, out, C, H, W, rtab, (hipStream_t)stream) ==
                 hipSuccess ? 0 : -2;
}

int tair_k_stitch_peers(const void* src_ptrs, int per_rank, int first_image, int n_images, int tiles_per_image,
                        int nh, int nw,
                        int mode, int patch, int overlap, int stride, float* out, int C, int H, int W,
                        const float* rtab, void* stream) {
  return stitch_peers((const float* const*)src_ptrs, per_rank, first_image, n_images, tiles_per_image, nh, nw, mode, patch, overlap,
                      stride, out, C, H, W, rtab, (hipStream_t)stream) == hipSuccess ? 0 : -2;
}

// IPC export / import of a device buffer (the peer-read stitch): the handle names the whole allocation,
// so the exporter also reports the buffer's byte offset inside it
int tair_ipc_get_handle(const void* dev_ptr, void* handle_out, unsigned long long* offset) {
  if (!dev_ptr || !handle_out || !offset) {
    set_error("ipc_get_handle: null argument");
    return -1;
  }
  void* base = nullptr;
  size_t size = 0;
  hipError_t e = hipMemGetAddressRange((hipDeviceptr_t*)&base, &size, (hipDeviceptr_t)dev_ptr);
  if (e != hipSuccess) {
    set_error("ipc_get_handle: hipMemGetAddressRange: %s", hipGetErrorString(e));
    return -2;
  }
  hipIpcMemHandle_t h;
  e = hipIpcGetMemHandle(&h, base);
  if (e != hipSuccess) {
    set_error("ipc_get_handle: hipIpcGetMemHandle: %s", hipGetErrorString(e));
    return -2;
  }
  static_assert(sizeof(hipIpcMemHandle_t) <= TAIR_IPC_HANDLE_BYTES, "IPC handle size");
  std::memset(handle_out, 0, TAIR_IPC_HANDLE_BYTES);
  std::memcpy(handle_out, &h, sizeof(h));
  *offset = (unsigned long long)((const char*)dev_ptr - (const char*)base);
  return 0;
}

int tair_ipc_open(const void* handle, void** dev_ptr) {
  if (!handle || !dev_ptr) {
    set_error("ipc_open: null argument");
    return -1;
  }
  hipIpcMemHandle_t h;
  std::memcpy(&h, handle, sizeof(h));
  hipError_t e = hipIpcOpenMemHandle(dev_ptr, h, hipIpcMemLazyEnablePeerAccess);
  if (e != hipSuccess) {
    set_error("ipc_open: hipIpcOpenMemHandle: %s", hipGetErrorString(e));
    return -2;
  }
  return 0;
}

int tair_ipc_close(void* dev_ptr) {
  hipError_t e = hipIpcCloseMemHandle(dev_ptr);
  if (e != hipSuccess) {
    set_error("ipc_close: hipIpcCloseMemHandle: %s", hipGetErrorString(e));
    return -2;
  }
  return 0;
}

int tair_k_gn_apply_stats(const void* x, int ldx, int x_lo, int B, int HW, int C, int G, float eps, const float* gamma,
                          const float* beta, int silu, const double* st, int st_rs, void* y, int ldy, int y_split,
                          void* stream) {
  GnArgs g{};
  g.x = (const bf16*)x; g.ldx = ldx; g.gamma = gamma; g.beta = beta; g.y = (bf16*)y; g.ldy = ldy;
  g.st = st; g.st_rs = st_rs; g.eps = eps; g.x_lo = x_lo; g.y_split = y_split;
  return groupnorm_apply_grouped(&g, 1, B, HW, C, silu, (hipStream_t)stream, G) == hipSuccess ? 0 : -2;
}

int tair_k_softmax_split(const float* S, int lds, int rows, int L, void* P, void* stream) {
  return softmax_split(S, lds, rows, L, (bf16*)P, (hipStream_t)stream) == hipSuccess ? 0 : -2;
}

int tair_k_transpose_split(const void* x, int B, int L, int C, void* y, void* stream) {
  return transpose_split((const bf16*)x, B, L, C, (bf16*)y, (hipStream_t)stream) == hipSuccess ? 0 : -2;
}

int tair_k_softmax_split_pad(const float* S, int lds, int rows, int L, int Lp, void* P, void* stream) {
  const hipError_t e = softmax_split_pad(S, lds, rows, L, Lp, (bf16*)P, (hipStream_t)stream);
  if (e == hipErrorInvalidValue) {
    set_error("softmax_split_pad: bad arguments (lds %d, rows %d, L %d, Lp %d)", lds, rows, L, Lp);
    return -1;
  }
  return e == hipSuccess ? 0 : -2;
}

int tair_k_transpose_split_pad(const void* x, int B, int L, int Lp, int C, void* y, void* stream) {
  const hipError_t e = transpose_split_pad((const bf16*)x, B, L, Lp, C, (bf16*)y, (hipStream_t)stream);
  if (e == hipErrorInvalidValue) {
    set_error("transpose_split_pad: bad arguments (B %d, L %d, Lp %d, C %d)", B, L, Lp, C);
    return -1;
  }
  return e == hipSuccess ? 0 : -2;
}

int tair_k_gn_stats_merge(double* slots, int64_t slot_stride, int T, const int* pixels, int B, int G, int cg,
                          int st_rs, void* stream) {
  GnMergeArgs a{};
  a.slots = slots; a.slot_stride = slot_stride;
  a.T = T; a.B = B; a.G = G; a.cg = cg; a.st_rs = st_rs;
  hipError_t e = hipErrorInvalidValue;
  if (pixels && T >= 1 && T <= GN_MERGE_MAX_TILES) {
    for (int t = 0; t < T; ++t) a.pixels[t] = pixels[t];
    e = gn_stats_merge(a, (hipStream_t)stream);
  }
  if (e == hipErrorInvalidValue) {
    set_error("gn_stats_merge: bad arguments (slots %p, slot_stride %lld, T %d (1..%d), pixel counts %s, B %d, G %d, "
              "cg %d, st_rs %d)", (void*)slots, (long long)slot_stride, T, GN_MERGE_MAX_TILES,
              pixels ? "must be >= 1" : "null", B, G, cg, st_rs);
    return -1;
  }
  return e == hipSuccess ? 0 : -2;
}

int tair_k_ms_deform_attn(const float* value, int N, int S, int M, int D, const int* level_hw, int L, int Q, int P,
                          const float* loc, const float* attn, float* out, void* stream) {
  if (!level_hw || L < 1 || L > MSDA_MAX_LEVELS) {
    set_error("ms_deform_attn: %d levels (1..%d)", L, MSDA_MAX_LEVELS);
    return -1;
  }
  MsdaArgs a{};
  a.N = N; a.S = S; a.M = M; a.D = D; a.L = L; a.P = P; a.Q = Q;
  int start = 0;
  for (int l = 0; l < L; ++l) {
    a.h[l] = level_hw[2 * l];
    a.w[l] = level_hw[2 * l + 1];
    a.start[l] = start;
    start += a.h[l] * a.w[l];
  }
  return ms_deform_attn(a, value, loc, attn, out, (hipStream_t)stream) == hipSuccess ? 0 : -2;
}

}  // extern "C"
