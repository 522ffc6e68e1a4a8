"""SD VAE decoder and encoder on the HIP kernels, fp32-accurate (reference: terediff/model/vae.py:60-559
Encoder / Decoder, cldm.py:92-141 vae_encode / vae_decode).

The parity gate is on the decoded image (rel-L2 <= 1e-3): a bf16 decoder misses it (7.1e-3 measured,
profiles/r02_parity_batched.jsonl), so every tensor is carried as a split pair hi = bf16(x),
lo = bf16(x - hi) in three bf16 channel planes and every convolution / projection is ONE bf16 MFMA
GEMM over 3x the reduction: activations (hi, lo, hi) x weights (hi, hi, lo) = hi*hi + lo*hi + hi*lo,
the fp32 product to ~2^-16 (the dropped lo*lo term is ~2^-18).  Accumulation, biases, GroupNorm
statistics (fp64, from the producing GEMM's epilogue) and softmax stay fp32.

Layout: NHWC, [B*H*W, 3C] per tensor.  Kernels (libtair_cldm.so, include/tair_kernels.h):
* 3x3 convs / nearest-x2 upsample convs / 1x1 convs: tair_k_gemm (implicit GEMM, modes CONV3 /
  CONV3_UP / DENSE, first conv CONV3_SMALLC), epilogue writes the split planes (+ GroupNorm statistics
  of the output for the GroupNorm that consumes it, + split residual x + h of the ResnetBlock; the
  nin_shortcut 1x1 conv rides as a K-extension of conv2);
* GroupNorm(32, eps 1e-6) + SiLU: tair_k_gn_apply_stats (statistics finalised from the producer's);
* AttnBlock (1 head, d = 512, 4096 tokens at 64^2): S = Q K^T (GEMM, K in weight-order planes) ->
  tair_k_softmax_split -> O = P V (GEMM against V^T from tair_k_transpose_split; the v bias is added
  once after, softmax rows sum to 1) -> proj_out + residual.
post_quant_conv (1x1, 4 -> 4 channels on the 64^2 latent, 0.03 % of the FLOPs) runs in torch fp32.
The encoder (HipVAEEncoder: prepare_condition's c_img, cldm.py:92-119) adds the Downsample (pad (0, 1,
0, 1) then a stride-2 3x3 conv: mode CONV3_S2 with s2_shift = 1) and the 3-channel conv_in (CONV3_SMALLC);
quant_conv (1x1, 8 -> 8 on the 64^2 latent) and the posterior mode (its first 4 channels) run in torch fp32.

Tiled (decode_tiled / encode_mode_tiled; utils/tilevae/tilevae.py:307-579 with fast mode off, as cldm.py:92-141 uses
it): overlapping tiles (vae.split_tiles) run the same blocks layer-major; after every statistics-producing GEMM one
tair_k_gn_stats_merge gives all tiles' slots the merged (mean, var) of the reference's cross-tile GroupNorm; attention
is local to a tile (token counts off multiples of 64 take tair_k_softmax_split_pad / tair_k_transpose_split_pad);
each finished tile is cropped into the result.  The untiled AttnBlock's S [HW, HW] fp32 + P [HW, 3 HW] bf16 (2.7 GB at
a 128^2 latent, ~43 GB at 256^2) is what the tiling removes; the tiles' activations all stay on the device, so peak
memory is linear in the image area.
"""
from __future__ import annotations

import ctypes
from typing import Dict, List, Optional, Tuple

import torch

from . import _lib
from .vae import place_tile, split_tiles, tiling_needed

A_DENSE, A_CONV3, A_CONV3_S2, A_CONV3_UP, A_SMALLC = 0, 1, 2, 3, 4
STAT_REPL = 8
G = 32
EPS = 1e-6


def _split(x: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    hi = x.to(torch.bfloat16)
    return hi, (x - hi.float()).to(torch.bfloat16)


def _pack_act(x: torch.Tensor) -> torch.Tensor:
    """[..., C] fp32 -> [..., 3C] bf16 planes (hi, lo, hi)."""
    hi, lo = _split(x)
    return torch.cat([hi, lo, hi], dim=-1).contiguous()


def _pack_weight(w: torch.Tensor, taps: int, ldw: int) -> torch.Tensor:
    """w [Cout, Cin, kh, kw] fp32 -> [Cout, ldw] bf16 over the plane channel space c' = plane*Cin + c,
    planes (hi, hi, lo).  3x3 convs with 3Cin % 64 == 0 take the GEMM's channel-chunk-major K order
    k = (c'/64 * 9 + tap) * 64 + c'%64 (kernels.h A_CONV3); otherwise k = tap*3Cin + c'."""
    co, ci = w.shape[:2]
    wt = w.permute(0, 2, 3, 1).reshape(co, taps, ci).float()
    hi, lo = _split(wt)
    planes = torch.stack([hi, hi, lo], dim=2).reshape(co, taps, 3 * ci)
    if taps == 9 and (3 * ci) % 64 == 0:
        planes = planes.reshape(co, 9, 3 * ci // 64, 64).permute(0, 2, 1, 3)
    packed = planes.reshape(co, taps * 3 * ci)
    out = torch.zeros((co, ldw), dtype=torch.bfloat16, device=w.device)
    out[:, :packed.shape[1]] = packed
    return out


def _r64(n: int) -> int:
    return (n + 63) // 64 * 64


class _Conv:
    def __init__(self, conv: torch.nn.Conv2d, dev, skip: Optional[torch.nn.Conv2d] = None):
        w = conv.weight.detach().float().to(dev)
        self.cout, self.cin, kh, _ = w.shape
        self.taps = kh * kh
        self.K = _r64(self.taps * 3 * self.cin) if self.cin * 3 % 64 else self.taps * 3 * self.cin
        self.Kx = 3 * skip.weight.shape[1] if skip is not None else 0
        ldw = _r64(self.K + self.Kx)
        self.w = _pack_weight(w, self.taps, ldw)
        if skip is not None:
            sw = _pack_weight(skip.weight.detach().float().to(dev), 1, self.Kx)
            self.w[:, self.K:self.K + self.Kx] = sw
        b = conv.bias.detach().float().to(dev)
        if skip is not None:
            b = b + skip.bias.detach().float().to(dev)
        self.bias = b.contiguous()
        self.ldw = ldw


class _Norm:
    def __init__(self, gn: torch.nn.GroupNorm, dev):
        self.gamma = gn.weight.detach().float().to(dev).contiguous()
        self.beta = gn.bias.detach().float().to(dev).contiguous()


def _res(blk, dev):
    skip = getattr(blk, "nin_shortcut", None)
    return ("res", dict(n1=_Norm(blk.norm1, dev), c1=_Conv(blk.conv1, dev), n2=_Norm(blk.norm2, dev),
                        c2=_Conv(blk.conv2, dev, skip), cin=blk.in_channels, cout=blk.out_channels))


def _attn_block(a, dev):
    return ("attn", dict(n=_Norm(a.norm, dev), q=_Conv(a.q, dev), k=_Conv(a.k, dev), v=_Conv(a.v, dev),
                         o=_Conv(a.proj_out, dev), bv=a.v.bias.detach().float().to(dev)))


class _HipVAEBase:
    """Launch helpers and blocks shared by the decoder and the encoder (split-precision planes)."""

    def _init_pool(self, dev, max_batch):
        self.dev, self.max_batch = dev, max_batch
        self.n_stats = 64
        self.st_rs = max_batch * G * 2
        self.stats = torch.zeros(self.n_stats * STAT_REPL * self.st_rs, dtype=torch.float64, device=dev)
        self.part = torch.empty(64 << 20, dtype=torch.float32, device=dev)
        self.L = _lib.lib()

    def _ensure_stats(self, n):
        """The tiled passes take one slot per tile and statistics-producing GEMM: grow the pool to n slots."""
        if n > self.n_stats:
            self.n_stats = n
            self.stats = torch.zeros(n * STAT_REPL * self.st_rs, dtype=torch.float64, device=self.dev)

    # ---------------------------------------------------------------- launches
    def _stream(self):
        return ctypes.c_void_p(torch.cuda.current_stream(self.dev).cuda_stream)

    def _stat(self):
        i = self._next_stat
        self._next_stat += 1
        if i >= self.n_stats:
            raise _lib.TairError("HipVAEDecoder: statistics pool exhausted")
        return self.stats.data_ptr() + i * STAT_REPL * self.st_rs * 8

    def _gemm(self, mode, A, lda, cw: _Conv, M, out, ldo, *, B=1, H=0, W=0, Ho=0, Wo=0, C=0, X=None, ldx=0,
              res=None, ld_res=0, res_lo=0, out_split=1, out_f32=0, st=None, hw=0, alpha=1.0, bias=True,
              N=None, K=None, Wt=None, ldw=None, s2_shift=0):
        if st is not None and hw % 64 and M > hw:
            # a statistics tile of the GEMM must not straddle two images: images whose pixel count is no multiple
            # of 64 (tiles of the tiled passes, e.g. 30 x 24) go one launch each, into their rows of the slot
            rin = H * W if mode != A_DENSE else hw
            for b in range(M // hw):
                o = slice(b * hw, (b + 1) * hw)
                self._gemm(mode, A[b * rin:(b + 1) * rin], lda, cw, hw, out[o], ldo, B=1, H=H, W=W, Ho=Ho, Wo=Wo, C=C,
                           X=None if X is None else X[o], ldx=ldx, res=None if res is None else res[o], ld_res=ld_res,
                           res_lo=res_lo, out_split=out_split, out_f32=out_f32, st=st + b * G * 2 * 8, hw=hw,
                           alpha=alpha, bias=bias, N=N, K=K, Wt=Wt, ldw=ldw, s2_shift=s2_shift)
            return
        d = _lib.GemmDesc()
        d.M, d.N, d.K, d.amode = M, N or cw.cout, K or cw.K, mode
        d.A, d.lda, d.C, d.Bn, d.H, d.W, d.Ho, d.Wo = A.data_ptr(), lda, C, B, H, W, Ho, Wo
        if X is not None:
            d.X, d.ldx, d.Kx = X.data_ptr(), ldx, cw.Kx
        d.Wt = (Wt if Wt is not None else cw.w).data_ptr()
        d.ldw = ldw or cw.ldw
        d.alpha = alpha
        d.bias = cw.bias.data_ptr() if (bias and cw is not None) else None
        d.rows_per_b = Ho * Wo if mode != A_DENSE else 1
        if res is not None:
            d.res, d.ld_res, d.res_lo = res.data_ptr(), ld_res, res_lo
        d.out, d.ldo, d.out_f32, d.out_split = out.data_ptr(), ldo, out_f32, out_split
        d.partial, d.partial_cap = self.part.data_ptr(), self.part.numel()
        if st is not None:
            d.st_acc, d.st_rs, d.st_cg, d.st_G, d.st_coff, d.st_hw = st, self.st_rs, d.N // G, G, 0, hw
        d.s2_shift = s2_shift
        _lib.check(self.L.tair_k_gemm(ctypes.byref(d), self._stream()), "vae gemm")

    def _gn(self, x, C, B, HW, norm: _Norm, st, silu) -> torch.Tensor:
        y = torch.empty((B * HW, 3 * C), dtype=torch.bfloat16, device=self.dev)
        _lib.check(self.L.tair_k_gn_apply_stats(x.data_ptr(), 3 * C, C, B, HW, C, G, EPS, norm.gamma.data_ptr(),
                                                norm.beta.data_ptr(), silu, ctypes.c_void_p(st), self.st_rs,
                                                y.data_ptr(), 3 * C, 1, self._stream()), "vae groupnorm")
        return y

    def _conv3(self, x, cw: _Conv, B, H, Wd, *, up=False, **kw) -> torch.Tensor:
        Ho, Wo = (2 * H, 2 * Wd) if up else (H, Wd)
        out = torch.empty((B * Ho * Wo, 3 * cw.cout), dtype=torch.bfloat16, device=self.dev)
        self._gemm(A_CONV3_UP if up else A_CONV3, x, 3 * cw.cin, cw, B * Ho * Wo, out, 3 * cw.cout, B=B, H=H, W=Wd,
                   Ho=Ho, Wo=Wo, C=3 * cw.cin, **kw)
        return out

    # ---------------------------------------------------------------- blocks
    # Every stage between two GroupNorms is "apply the GroupNorm from the input's slot, then the GEMM that fills the
    # output's slot": the untiled passes chain them on one tensor, the tiled passes run each stage over all tiles
    # and merge the tiles' slots before the next.
    def _conv_in_to(self, x0, B, H, Wd, st):
        ci = self.conv_in
        h = torch.empty((B * H * Wd, 3 * ci.cout), dtype=torch.bfloat16, device=self.dev)
        self._gemm(A_SMALLC, x0, 3 * ci.cin, ci, B * H * Wd, h, 3 * ci.cout, B=B, H=H, W=Wd, Ho=H, Wo=Wd,
                   C=3 * ci.cin, st=st, hw=H * Wd)
        return h

    def _res_a(self, x, st_x, p, B, H, Wd, s1):
        t = self._gn(x, p["cin"], B, H * Wd, p["n1"], st_x, 1)
        return self._conv3(t, p["c1"], B, H, Wd, st=s1, hw=H * Wd)

    def _res_b(self, x, h1, s1, p, B, H, Wd, s_out):
        HW = H * Wd
        cin, cout = p["cin"], p["cout"]
        t2 = self._gn(h1, cout, B, HW, p["n2"], s1, 1)
        if cin != cout:
            return self._conv3(t2, p["c2"], B, H, Wd, X=x, ldx=3 * cin, st=s_out, hw=HW)
        return self._conv3(t2, p["c2"], B, H, Wd, res=x, ld_res=3 * cin, res_lo=cin, st=s_out, hw=HW)

    def _resblock(self, x, st_x, p, B, H, Wd):
        s1 = self._stat()
        h1 = self._res_a(x, st_x, p, B, H, Wd, s1)
        s_out = self._stat()
        return self._res_b(x, h1, s1, p, B, H, Wd, s_out), s_out

    def _attn(self, x, st_x, p, B, H, Wd):
        s_out = self._stat()
        return self._attn_to(x, st_x, p, B, H, Wd, s_out), s_out

    def _attn_to(self, x, st_x, p, B, H, Wd, s_out):
        HW, C = H * Wd, p["q"].cout
        Lp = _r64(HW)  # token counts off the GEMM's K-tile (tiles of the tiled passes): zero-padded planes
        y = self._gn(x, C, B, HW, p["n"], st_x, 0)
        M = B * HW
        q = torch.empty((M, 3 * C), dtype=torch.bfloat16, device=self.dev)
        k = torch.empty_like(q)
        v = torch.empty_like(q)
        self._gemm(A_DENSE, y, 3 * C, p["q"], M, q, 3 * C, out_split=1)
        self._gemm(A_DENSE, y, 3 * C, p["k"], M, k, 3 * C, out_split=2)
        self._gemm(A_DENSE, y, 3 * C, p["v"], M, v, 3 * C, out_split=1, bias=False)
        vt = torch.empty((B, C, 3 * Lp), dtype=torch.bfloat16, device=self.dev)
        if Lp == HW:
            _lib.check(self.L.tair_k_transpose_split(v.data_ptr(), B, HW, C, vt.data_ptr(), self._stream()), "transpose")
        else:
            _lib.check(self.L.tair_k_transpose_split_pad(v.data_ptr(), B, HW, Lp, C, vt.data_ptr(), self._stream()),
                       "transpose (padded)")
        S = torch.empty((HW, Lp), dtype=torch.float32, device=self.dev)
        P = torch.empty((HW, 3 * Lp), dtype=torch.bfloat16, device=self.dev)
        o = torch.empty((M, 3 * C), dtype=torch.bfloat16, device=self.dev)
        scale = float(C) ** -0.5
        for b in range(B):  # per image: S = Q K^T * d^-1/2, P = softmax(S), O = P V + b_v
            qb, kb = q[b * HW:(b + 1) * HW], k[b * HW:(b + 1) * HW]
            self._gemm(A_DENSE, qb, 3 * C, None, HW, S, Lp, N=HW, K=3 * C, Wt=kb, ldw=3 * C, out_split=0, out_f32=1,
                       alpha=scale, bias=False)
            if Lp == HW:
                _lib.check(self.L.tair_k_softmax_split(S.data_ptr(), HW, HW, HW, P.data_ptr(), self._stream()), "softmax")
            else:
                _lib.check(self.L.tair_k_softmax_split_pad(S.data_ptr(), Lp, HW, HW, Lp, P.data_ptr(), self._stream()),
                           "softmax (padded)")
            self._gemm(A_DENSE, P, 3 * Lp, _BiasOnly(p["bv"]), HW, o[b * HW:(b + 1) * HW], 3 * C, N=C, K=3 * Lp,
                       Wt=vt[b], ldw=3 * Lp, out_split=1)
        out = torch.empty((M, 3 * C), dtype=torch.bfloat16, device=self.dev)
        self._gemm(A_DENSE, o, 3 * C, p["o"], M, out, 3 * C, res=x, ld_res=3 * C, res_lo=C, st=s_out, hw=HW)
        return out

    def _up_to(self, h, p, B, H, Wd, s2):
        """nearest-x2 upsample + 3x3 conv, statistics for the next ResnetBlock."""
        return self._conv3(h, p, B, H, Wd, up=True, st=s2, hw=4 * H * Wd)

    def _down_to(self, h, p, B, H, Wd, s2):
        """Downsample: pad (0, 1, 0, 1) + 3x3 stride-2 conv."""
        Ho, Wo = H // 2, Wd // 2
        out = torch.empty((B * Ho * Wo, 3 * p.cout), dtype=torch.bfloat16, device=self.dev)
        self._gemm(A_CONV3_S2, h, 3 * p.cin, p, B * Ho * Wo, out, 3 * p.cout, B=B, H=H, W=Wd, Ho=Ho, Wo=Wo,
                   C=3 * p.cin, st=s2, hw=Ho * Wo, s2_shift=1)
        return out

    def _conv_out_f32(self, h, st, B, H, Wd):
        """norm_out + SiLU + conv_out -> [B*H*W, cout] fp32 (NHWC)."""
        c = self.conv_out.cin
        t = self._gn(h, c, B, H * Wd, self.norm_out, st, 1)
        out = torch.empty((B * H * Wd, self.conv_out.cout), dtype=torch.float32, device=self.dev)
        self._gemm(A_CONV3, t, 3 * c, self.conv_out, B * H * Wd, out, self.conv_out.cout, B=B, H=H, W=Wd, Ho=H,
                   Wo=Wd, C=3 * c, out_split=0, out_f32=1)
        return out

    # ---------------------------------------------------------------- tiled passes
    def _merge(self, slots, dims, B, C):
        """Cross-tile GroupNorm (tilevae.py:232-278): one merge over the T tiles' slots of a stage, C channels."""
        T = len(slots)
        px = (ctypes.c_int * T)(*[h * w for h, w in dims])
        _lib.check(self.L.tair_k_gn_stats_merge(ctypes.c_void_p(slots[0]), STAT_REPL * self.st_rs, T, px, B, G,
                                                C // G, self.st_rs, self._stream()), "vae statistics merge")

    def _run_tiles(self, x0s, dims, B):
        """The network over T tiles (x0s[t]: packed input planes of B images of dims[t] = (H, W)), layer-major:
        every stage runs over all tiles into T fresh consecutive slots, then one merge gives all tiles the same
        (mean, var) for the GroupNorm that follows (tilevae.py:507-575 with fast mode off).  All tiles'
        activations of the current stage stay on the device: peak memory is linear in the image area; what the
        tiling removes is the attention's O((HW)^2) scores.  Returns the tiles' conv_out [B*H*W, cout] fp32
        and their final dims."""
        T = len(x0s)
        self._ensure_stats(T * (1 + sum(2 if kind == "res" else 1 for kind, _ in self.blocks)))
        self.stats.zero_()
        self._next_stat = 0
        rng = range(T)

        def slots():
            return [self._stat() for _ in rng]
        sts = slots()
        hs = [self._conv_in_to(x0s[t], B, *dims[t], sts[t]) for t in rng]
        self._merge(sts, dims, B, self.conv_in.cout)
        for kind, p in self.blocks:
            if kind == "res":
                s1 = slots()
                h1 = [self._res_a(hs[t], sts[t], p, B, *dims[t], s1[t]) for t in rng]
                self._merge(s1, dims, B, p["cout"])
                so = slots()
                hs = [self._res_b(hs[t], h1[t], s1[t], p, B, *dims[t], so[t]) for t in rng]
                self._merge(so, dims, B, p["cout"])
            elif kind == "attn":
                so = slots()
                hs = [self._attn_to(hs[t], sts[t], p, B, *dims[t], so[t]) for t in rng]
                self._merge(so, dims, B, p["q"].cout)
            elif kind == "up":
                so = slots()
                hs = [self._up_to(hs[t], p, B, *dims[t], so[t]) for t in rng]
                dims = [(2 * h, 2 * w) for h, w in dims]
                self._merge(so, dims, B, p.cout)
            else:
                so = slots()
                hs = [self._down_to(hs[t], p, B, *dims[t], so[t]) for t in rng]
                dims = [(h // 2, w // 2) for h, w in dims]
                self._merge(so, dims, B, p.cout)
            sts = so
        return [self._conv_out_f32(hs[t], sts[t], B, *dims[t]) for t in rng], dims

    def _tiled(self, x, ins, outs, is_decoder):
        """x [B, C, H, W] fp32 (whole input) -> the network's output [B, cout, 8H | H/8, 8W | W/8] fp32, each
        finished tile cropped to its output box (tilevae.py:218-229, 555)."""
        B, Cx, H, Wd = x.shape
        dims = [(b[3] - b[2], b[1] - b[0]) for b in ins]
        x0s = [_pack_act(x[:, :, b[2]:b[3], b[0]:b[1]].permute(0, 2, 3, 1).reshape(-1, Cx)) for b in ins]
        tiles, dims = self._run_tiles(x0s, dims, B)
        Ho, Wo = (8 * H, 8 * Wd) if is_decoder else (H // 8, Wd // 8)
        result = torch.zeros((B, self.conv_out.cout, Ho, Wo), dtype=torch.float32, device=self.dev)
        for t, (h, w), ib, ob in zip(tiles, dims, ins, outs):
            place_tile(result, t.view(B, h, w, -1).permute(0, 3, 1, 2), ib, ob, is_decoder)
        return result


class HipVAEDecoder(_HipVAEBase):
    """decode(z) == AutoencoderKL.decode(z) in fp32 semantics, on the HIP kernels.  `vae` is the
    product stock-PyTorch AutoencoderKL (tair_amd/vae.py) holding the weights (reference keys)."""

    def __init__(self, vae, device, max_batch: int = 4):
        dev = torch.device(device)
        self._init_pool(dev, max_batch)
        d = vae.decoder
        self.pq_w = vae.post_quant_conv.weight.detach().float().to(dev)
        self.pq_b = vae.post_quant_conv.bias.detach().float().to(dev)
        self.conv_in = _Conv(d.conv_in, dev)
        self.blocks: List[Tuple[str, object]] = []  # execution order
        self.blocks.append(_res(d.mid.block_1, dev))
        self.blocks.append(_attn_block(d.mid.attn_1, dev))
        self.blocks.append(_res(d.mid.block_2, dev))
        for i in reversed(range(len(d.up))):
            st = d.up[i]
            for blk in st.block:
                self.blocks.append(_res(blk, dev))
            if hasattr(st, "upsample"):
                self.blocks.append(("up", _Conv(st.upsample.conv, dev)))
        self.norm_out = _Norm(d.norm_out, dev)
        self.conv_out = _Conv(d.conv_out, dev)

    # ---------------------------------------------------------------- decode
    @torch.no_grad()
    def decode(self, z: torch.Tensor) -> torch.Tensor:
        """z [B, 4, h, w] (already / scale_factor) -> image [B, 3, 8h, 8w] fp32 (before clamp)."""
        B, _, H, Wd = z.shape
        if B > self.max_batch:
            return torch.cat([self.decode(z[i:i + self.max_batch]) for i in range(0, B, self.max_batch)])
        self.stats.zero_()
        self._next_stat = 0
        zz = torch.nn.functional.conv2d(z.float(), self.pq_w, self.pq_b)
        x0 = _pack_act(zz.permute(0, 2, 3, 1).reshape(B * H * Wd, -1))
        st = self._stat()
        h = self._conv_in_to(x0, B, H, Wd, st)
        for kind, p in self.blocks:
            if kind == "res":
                h, st = self._resblock(h, st, p, B, H, Wd)
            elif kind == "attn":
                h, st = self._attn(h, st, p, B, H, Wd)
            else:
                s2 = self._stat()
                h = self._up_to(h, p, B, H, Wd, s2)
                st, H, Wd = s2, 2 * H, 2 * Wd
        out = self._conv_out_f32(h, st, B, H, Wd)
        return out.view(B, H, Wd, -1).permute(0, 3, 1, 2).contiguous()

    @torch.no_grad()
    def decode_tiled(self, z: torch.Tensor, tile_size: int) -> torch.Tensor:
        """The reference's tiled decode (cldm.py:121-141 with tiled=True: post_quant_conv on the whole latent, then
        VAEHook with fast mode off): tile_size in latent pixels; a latent of at most 2 * 11 + tile_size per side
        runs decode() itself.  Not equal to decode(): attention is local to a tile and the GroupNorm statistics
        are the tiles' merged ones."""
        B, _, H, Wd = z.shape
        if not tiling_needed(H, Wd, tile_size, True):
            return self.decode(z)
        if B > self.max_batch:
            return torch.cat([self.decode_tiled(z[i:i + self.max_batch], tile_size)
                              for i in range(0, B, self.max_batch)])
        ins, outs = split_tiles(H, Wd, tile_size, True)
        zz = torch.nn.functional.conv2d(z.float(), self.pq_w, self.pq_b)
        return self._tiled(zz, ins, outs, True)


class _BiasOnly:
    """Stand-in conv for the P.V GEMM: carries the v bias (added once: softmax rows sum to 1)."""

    def __init__(self, b):
        self.bias = b
        self.cout = b.numel()
        self.K = 0
        self.Kx = 0
        self.w = None
        self.ldw = 0


class HipVAEEncoder(_HipVAEBase):
    """AutoencoderKL.encode_mode(x) (the posterior mean, distributions.py:24-46 .mode(); cldm.py:92-119)
    in fp32 semantics on the HIP kernels: x [B, 3, 8h, 8w] in [-1, 1] -> [B, 4, h, w] (before the
    0.18215 latent scale)."""

    def __init__(self, vae, device, max_batch: int = 4):
        dev = torch.device(device)
        self._init_pool(dev, max_batch)
        e = vae.encoder
        self.q_w = vae.quant_conv.weight.detach().float().to(dev)
        self.q_b = vae.quant_conv.bias.detach().float().to(dev)
        self.conv_in = _Conv(e.conv_in, dev)
        self.blocks: List[Tuple[str, object]] = []
        for st in e.down:
            for blk in st.block:
                self.blocks.append(_res(blk, dev))
            if hasattr(st, "downsample"):
                self.blocks.append(("down", _Conv(st.downsample.conv, dev)))
        self.blocks.append(_res(e.mid.block_1, dev))
        self.blocks.append(_attn_block(e.mid.attn_1, dev))
        self.blocks.append(_res(e.mid.block_2, dev))
        self.norm_out = _Norm(e.norm_out, dev)
        self.conv_out = _Conv(e.conv_out, dev)

    @torch.no_grad()
    def encode_mode(self, x: torch.Tensor) -> torch.Tensor:
        B, _, H, Wd = x.shape
        if B > self.max_batch:
            return torch.cat([self.encode_mode(x[i:i + self.max_batch]) for i in range(0, B, self.max_batch)])
        if H % 8 or Wd % 8:
            raise _lib.TairError(f"HipVAEEncoder: image size {H}x{Wd} is not a multiple of 8")
        self.stats.zero_()
        self._next_stat = 0
        x0 = _pack_act(x.float().permute(0, 2, 3, 1).reshape(B * H * Wd, -1))
        st = self._stat()
        h = self._conv_in_to(x0, B, H, Wd, st)
        for kind, p in self.blocks:
            if kind == "res":
                h, st = self._resblock(h, st, p, B, H, Wd)
            elif kind == "attn":
                h, st = self._attn(h, st, p, B, H, Wd)
            else:
                s2 = self._stat()
                h = self._down_to(h, p, B, H, Wd, s2)
                st, H, Wd = s2, H // 2, Wd // 2
        out = self._conv_out_f32(h, st, B, H, Wd)
        moments = torch.nn.functional.conv2d(out.view(B, H, Wd, -1).permute(0, 3, 1, 2), self.q_w, self.q_b)
        return moments[:, :moments.shape[1] // 2].contiguous()

    @torch.no_grad()
    def encode_mode_tiled(self, x: torch.Tensor, tile_size: int) -> torch.Tensor:
        """The reference's tiled encode (cldm.py:92-119 with tiled=True: VAEHook with fast mode off over the
        encoder, then quant_conv and the posterior mode on the whole output): tile_size in image pixels; an image
        of at most 2 * 32 + tile_size per side runs encode_mode() itself.  Every tile edge must be a multiple of 8
        image pixels (three stride-2 stages); the reference's size chooser yields multiples of 32 for the usual
        sizes."""
        B, _, H, Wd = x.shape
        if not tiling_needed(H, Wd, tile_size, False):
            return self.encode_mode(x)
        if B > self.max_batch:
            return torch.cat([self.encode_mode_tiled(x[i:i + self.max_batch], tile_size)
                              for i in range(0, B, self.max_batch)])
        if H % 8 or Wd % 8:
            raise ValueError(f"HipVAEEncoder: image size {H}x{Wd} is not a multiple of 8")
        ins, outs = split_tiles(H, Wd, tile_size, False)
        for b in ins:
            if any(v % 8 for v in b):
                raise ValueError(f"HipVAEEncoder: tile box [x {b[0]}:{b[1]}, y {b[2]}:{b[3]}] of the {H}x{Wd} image at "
                                 f"tile size {tile_size} is not on multiples of 8 image pixels")
        out = self._tiled(x.float(), ins, outs, False)
        moments = torch.nn.functional.conv2d(out, self.q_w, self.q_b)
        return moments[:, :moments.shape[1] // 2].contiguous()
