"""The GEMM plans of the split-precision VAE (tair_amd/vae_hip.py), shared by tests/test_vae_plans_cpu.py (which
plans does the VAE launch at the workload's shape: no device) and tests/test_vae_kernels_gpu.py (each of those
plans against fp64).

A recorded tair_k_gemm call is reduced to a signature

    (amode, kernel, bm, bn, splits > 1, out_split, out_f32, statistics, res_lo, K-extension, s2_shift, C % 64 != 0)

with (kernel, bm, bn, splits) from tair_k_gemm_plan on the call's descriptor.  SIGNATURES lists every signature
the decoder and the encoder produce at latent 64x64 / image 512x512 with B = 1 and B = 2; CASES are the GEMM
cases of the GPU tests, each of which names the kind of launch it covers (a signature without its plan part) and
is run under every plan SIGNATURES holds for that kind.

Operands come from the product's packers (_pack_act, _pack_weight, _Conv); the reference is plain torch fp64 on
the values the bf16 planes hold (hi + lo), the emulation the same arithmetic as the kernel's (three plane products
accumulated in fp32, epilogue in fp32, hi + lo output storage) with torch on the CPU.
"""
import ctypes
import math
from typing import Dict, List, Tuple

import torch
import torch.nn.functional as F

A_DENSE, A_CONV3, A_CONV3_S2, A_CONV3_UP, A_SMALLC = 0, 1, 2, 3, 4
KERN_TILE = 0
G = 32  # GroupNorm groups of the VAE

FIELDS = ("amode", "kernel", "bm", "bn", "split_k", "out_split", "out_f32", "stats", "res_lo", "k_ext", "s2_shift",
          "c_not_64")

# (amode, kernel, bm, bn, splits > 1, out_split, out_f32, statistics, res_lo, K-extension, s2_shift, C % 64 != 0)
SIGNATURES = {
    # conv_in: 4 latent channels (decoder, C = 12) and 3 image channels (encoder, C = 9)
    (A_SMALLC, 0, 64, 128, False, 1, 0, True, False, False, 0, True),
    (A_SMALLC, 0, 64, 64, False, 1, 0, True, False, False, 0, True),
    # ResnetBlock conv1 / conv2 (residual) / conv2 with the nin_shortcut as the K-extension
    (A_CONV3, 0, 128, 256, True, 1, 0, True, False, False, 0, False),
    (A_CONV3, 0, 128, 256, False, 1, 0, True, False, False, 0, False),
    (A_CONV3, 0, 64, 64, False, 1, 0, True, False, False, 0, False),
    (A_CONV3, 0, 128, 256, True, 1, 0, True, True, False, 0, False),
    (A_CONV3, 0, 128, 256, False, 1, 0, True, True, False, 0, False),
    (A_CONV3, 0, 64, 64, False, 1, 0, True, True, False, 0, False),
    (A_CONV3, 0, 128, 256, False, 1, 0, True, False, True, 0, False),
    (A_CONV3, 0, 64, 64, False, 1, 0, True, False, True, 0, False),
    # AttnBlock: q / v / P.V, k, S = alpha Q K^T, proj_out
    (A_DENSE, 0, 128, 256, True, 1, 0, False, False, False, 0, False),
    (A_DENSE, 0, 128, 256, True, 2, 0, False, False, False, 0, False),
    (A_DENSE, 0, 128, 256, False, 0, 1, False, False, False, 0, False),
    (A_DENSE, 0, 128, 256, True, 1, 0, True, True, False, 0, False),
    # Upsample, Downsample
    (A_CONV3_UP, 0, 128, 256, False, 1, 0, True, False, False, 0, False),
    (A_CONV3_S2, 0, 64, 64, False, 1, 0, True, False, False, 1, False),
    (A_CONV3_S2, 0, 128, 256, True, 1, 0, True, False, False, 1, False),
    (A_CONV3_S2, 0, 128, 256, False, 1, 0, True, False, False, 1, False),
    # conv_out (fp32 image / moments)
    (A_CONV3, 0, 64, 64, False, 0, 1, False, False, False, 0, False),
    (A_CONV3, 0, 64, 64, True, 0, 1, False, False, False, 0, False),
}


def plans_of(kind: tuple) -> List[tuple]:
    """The (kernel, bm, bn, splits > 1) plans SIGNATURES holds for a kind (amode, out_split, out_f32, statistics,
    res_lo, K-extension, s2_shift, C % 64 != 0)."""
    return sorted(s[1:5] for s in SIGNATURES if (s[0],) + s[5:] == kind)


def plan_of(d) -> Tuple[int, Tuple[int, int, int, int]]:
    """(status, (bm, bn, splits, kernel)) of tair_k_gemm_plan on a GemmDesc: host only."""
    from tair_amd import _lib
    out = [ctypes.c_int() for _ in range(4)]
    rc = _lib.lib().tair_k_gemm_plan(ctypes.byref(d), *[ctypes.byref(o) for o in out])
    return rc, tuple(o.value for o in out)


def signature(d, plan) -> tuple:
    bm, bn, splits, kern = plan
    return (d.amode, kern, bm, bn, splits > 1, d.out_split, d.out_f32, bool(d.st_acc), d.res_lo > 0, d.Kx > 0,
            d.s2_shift, d.amode != A_DENSE and d.C % 64 != 0)


# ------------------------------------------------------------------------------------------------ recording
class RecordingLib:
    """Stand-in for the loaded library inside HipVAEDecoder / HipVAEEncoder: tair_k_gemm plans the descriptor with
    the real host-side planner and records it; every other entry point returns 0.  Nothing touches a device."""

    def __init__(self):
        self.calls: List[Tuple[tuple, tuple]] = []  # (signature, (M, N, K, Kx, plan status))

    def tair_k_gemm(self, dref, stream):
        d = dref._obj  # the GemmDesc behind ctypes.byref
        rc, plan = plan_of(d)
        self.calls.append((signature(d, plan), (d.M, d.N, d.K, d.Kx, rc)))
        return 0

    def __getattr__(self, name):
        if not name.startswith("tair_"):
            raise AttributeError(name)
        return lambda *a: 0


_MODEL = []


def record_workload(which: str, B: int, latent: int = 64):
    """The (signature, (M, N, K, Kx, plan status)) list of one decode ('dec') or encode_mode ('enc') of B images of
    8 * latent pixels a side, run on the CPU: outputs are garbage, only the descriptors matter."""
    from tair_amd.vae import AutoencoderKL
    from tair_amd.vae_hip import HipVAEDecoder, HipVAEEncoder
    if not _MODEL:
        _MODEL.append(AutoencoderKL().eval())
    hip = (HipVAEDecoder if which == "dec" else HipVAEEncoder)(_MODEL[0], "cpu", max_batch=2)
    hip.part = torch.empty(1, dtype=torch.float32).expand(64 << 20)  # the pool's size, without its memory
    rec = RecordingLib()
    hip.L = rec
    hip._stream = lambda: ctypes.c_void_p(None)
    if which == "dec":
        hip.decode(torch.zeros(B, 4, latent, latent))
    else:
        hip.encode_mode(torch.zeros(B, 3, 8 * latent, 8 * latent))
    return rec.calls


# ------------------------------------------------------------------------------------------------ operands
class Ops:
    """One GEMM case at one shape: the descriptor's fields (tensors are replaced by their pointers in desc()),
    the fp64 reference [M, N] and the fp32 emulation of the kernel's arithmetic (both on the CPU, computed on
    first use and kept)."""

    def __init__(self, fields: Dict, ref_fn, emu_fn, B: int, hw: int):
        self.fields, self._ref_fn, self._emu_fn, self.B, self.hw = fields, ref_fn, emu_fn, B, hw
        self._ref = self._emu = None
        self.M, self.N = fields["M"], fields["N"]
        self.out_split, self.out_f32 = fields.get("out_split", 0), fields.get("out_f32", 0)
        self.stats = fields.pop("stats", False)
        self.ldo_pad = fields.pop("ldo_pad", 0)  # extra output columns past the planes, which must stay untouched

    @property
    def ref(self) -> torch.Tensor:  # fp64 [M, N] on the CPU, computed once
        if self._ref is None:
            self._ref = self._ref_fn()
        return self._ref

    @property
    def emu(self) -> torch.Tensor:
        if self._emu is None:
            self._emu = self._emu_fn()
        return self._emu

    def desc(self, **extra):
        from tair_amd import _lib
        d = _lib.GemmDesc()
        d.alpha = 1.0
        for k, v in dict(self.fields, **extra).items():
            if v is not None:
                setattr(d, k, v.data_ptr() if torch.is_tensor(v) else v)
        return d

    def kind(self) -> tuple:
        f = self.fields
        return (f["amode"], self.out_split, self.out_f32, self.stats, f.get("res_lo", 0) > 0, f.get("Kx", 0) > 0,
                f.get("s2_shift", 0), f["amode"] != A_DENSE and f["C"] % 64 != 0)


def _val(hi, lo):
    return hi.cpu().double() + lo.cpu().double()


def _f32(t):
    return t.cpu().float()


def _store(v32: torch.Tensor, out_split: int) -> torch.Tensor:
    """The value a consumer reads back from the kernel's output: fp32, or hi + lo bf16 planes of it."""
    if not out_split:
        return v32.double()
    hi = v32.to(torch.bfloat16)
    return _val(hi, (v32 - hi.float()).to(torch.bfloat16))


def _weights(gen, cout, cin, k):
    """Weights with a positive mean (1.5 / fan-in): batch elements whose inputs have different means then have
    clearly different output means, so a statistics slot of the wrong batch element cannot pass."""
    fan = cin * k * k
    return torch.randn(cout, cin, k, k, generator=gen) / math.sqrt(fan) + 1.5 / fan


MEANS = (1.0, -2.0, 0.5)


def conv_ops(dev, amode, B, H, W, cin, cout, *, stats=True, res=False, skip_cin=0, out_f32=False, seed=0) -> Ops:
    """A 3x3 conv of the VAE over 3 * cin plane channels: stride 1 (CONV3, or CONV3_SMALLC for cin = 3 / 4),
    nearest-x2 upsample + conv (CONV3_UP), pad (0, 1, 0, 1) + stride 2 (CONV3_S2 with s2_shift = 1); optional
    split residual (res_lo) or 1x1 skip conv over skip_cin channels as the K-extension."""
    from tair_amd.vae_hip import _Conv, _pack_act, _split
    gen = torch.Generator().manual_seed(seed)
    s2, up = amode == A_CONV3_S2, amode == A_CONV3_UP
    Ho, Wo = (H // 2, W // 2) if s2 else (2 * H, 2 * W) if up else (H, W)
    conv = torch.nn.Conv2d(cin, cout, 3, 2 if s2 else 1, 0 if s2 else 1)
    conv.weight.data = _weights(gen, cout, cin, 3)
    conv.bias.data = torch.randn(cout, generator=gen) * 0.3
    skip = None
    if skip_cin:
        skip = torch.nn.Conv2d(skip_cin, cout, 1)
        skip.weight.data = _weights(gen, cout, skip_cin, 1)
        skip.bias.data = torch.randn(cout, generator=gen) * 0.3
    mu = torch.tensor(MEANS[:B]).view(B, 1, 1, 1)
    x = torch.randn(B, H, W, cin, generator=gen) + mu
    cw = _Conv(conv, dev, skip)
    xp = _pack_act(x.reshape(-1, cin).to(dev))
    M = B * Ho * Wo
    f = dict(M=M, N=cout, K=cw.K, amode=amode, A=xp, lda=3 * cin, C=3 * cin, Bn=B, H=H, W=W, Ho=Ho, Wo=Wo, Wt=cw.w,
             ldw=cw.ldw, bias=cw.bias, rows_per_b=Ho * Wo, out_split=0 if out_f32 else 1, out_f32=int(out_f32),
             s2_shift=int(s2), stats=stats)
    xs = rp = None
    if skip is not None:
        xs = _pack_act((torch.randn(B, Ho, Wo, skip_cin, generator=gen) - mu).reshape(-1, skip_cin).to(dev))
        f.update(X=xs, ldx=3 * skip_cin, Kx=cw.Kx)
    if res:
        rp = _pack_act((torch.randn(B, Ho, Wo, cout, generator=gen) * 1.5 + mu).reshape(-1, cout).to(dev))
        f.update(res=rp, ld_res=3 * cout, res_lo=cout)

    def pre(t):  # NHWC rows -> the NCHW tensor the stride-1 / stride-2 conv sees
        t = t.view(B, H, W, -1).permute(0, 3, 1, 2)
        if up:
            t = F.interpolate(t, scale_factor=2, mode="nearest")
        return F.pad(t, (0, 1, 0, 1)) if s2 else t

    def run(xin, w, wskip, xskip, b, r):
        y = F.conv2d(pre(xin), w, None, 2 if s2 else 1, 0 if s2 else 1).permute(0, 2, 3, 1).reshape(M, cout)
        if wskip is not None:
            y = y + xskip @ wskip.t()
        y = y + b
        return y + r if r is not None else y

    whi, wlo = _split(conv.weight.detach().float())
    shi, slo = _split(skip.weight.detach().float().view(cout, -1)) if skip is not None else (None, None)

    def ref():
        return run(_val(xp[:, :cin], xp[:, cin:2 * cin]), _val(whi, wlo), None if skip is None else _val(shi, slo),
                   None if skip is None else _val(xs[:, :skip_cin], xs[:, skip_cin:2 * skip_cin]),
                   cw.bias.cpu().double(), None if rp is None else _val(rp[:, :cout], rp[:, cout:2 * cout]))

    def emu():  # planes (hi, lo, hi) x (hi, hi, lo) in fp32, bias and residual in fp32, hi + lo storage
        v = run(_f32(xp), torch.cat([whi, whi, wlo], 1).float(),
                None if skip is None else torch.cat([shi, shi, slo], 1).float(), None if skip is None else _f32(xs),
                _f32(cw.bias), None if rp is None else _f32(rp[:, :cout]) + _f32(rp[:, cout:2 * cout]))
        return _store(v, f["out_split"])

    o = Ops(f, ref, emu, B, Ho * Wo)
    o.keep = (cw, xp, xs, rp)
    return o


def dense_ops(dev, B, hw, C, N, *, out_split=1, bias=True, stats=False, res=False, seed=0) -> Ops:
    """A 1x1 conv of the AttnBlock over 3C plane channels (q / k / v, and proj_out with split residual and
    statistics), M = B * hw rows."""
    from tair_amd.vae_hip import _Conv, _pack_act, _split
    gen = torch.Generator().manual_seed(seed)
    conv = torch.nn.Conv2d(C, N, 1)
    conv.weight.data = _weights(gen, N, C, 1)
    conv.bias.data = torch.randn(N, generator=gen) * 0.3
    M = B * hw
    mu = torch.tensor(MEANS[:B]).view(B, 1, 1)
    x = (torch.randn(B, hw, C, generator=gen) + mu).reshape(M, C)
    cw = _Conv(conv, dev)
    xp = _pack_act(x.to(dev))
    f = dict(M=M, N=N, K=cw.K, amode=A_DENSE, Bn=1, A=xp, lda=3 * C, Wt=cw.w, ldw=cw.ldw, bias=cw.bias if bias else None,
             rows_per_b=1, out_split=out_split, stats=stats, ldo_pad=32 if N % 128 else 0)
    rp = None
    if res:
        rp = _pack_act((torch.randn(B, hw, N, generator=gen) * 1.5 - mu).reshape(M, N).to(dev))
        f.update(res=rp, ld_res=3 * N, res_lo=N)
    whi, wlo = _split(conv.weight.detach().float().view(N, C))

    def ref():
        r = _val(xp[:, :C], xp[:, C:2 * C]) @ _val(whi, wlo).t()
        if bias:
            r = r + cw.bias.cpu().double()
        return r + _val(rp[:, :N], rp[:, N:2 * N]) if rp is not None else r

    def emu():
        v = _f32(xp) @ torch.cat([whi, whi, wlo], 1).float().t()
        if bias:
            v = v + _f32(cw.bias)
        if rp is not None:
            v = v + (_f32(rp[:, :N]) + _f32(rp[:, N:2 * N]))
        return _store(v, out_split)

    o = Ops(f, ref, emu, B, hw)
    o.keep = (cw, xp, rp)
    return o


def scores_ops(dev, M, N, C, *, seed=0) -> Ops:
    """S = alpha Q K^T: Q [M, 3C] in activation-order planes (hi, lo, hi) against K [N, 3C] in weight-order
    planes (hi, hi, lo), fp32 output, alpha = C^-1/2, no bias."""
    from tair_amd.vae_hip import _pack_act, _pack_weight, _split
    gen = torch.Generator().manual_seed(seed)
    q = (torch.randn(M, C, generator=gen) * 2 + 0.5).to(dev)
    k = (torch.randn(N, C, generator=gen) * 2 - 0.3).to(dev)
    qp = _pack_act(q)
    kp = _pack_weight(k.view(N, C, 1, 1), 1, 3 * C)
    alpha = ctypes.c_float(float(C) ** -0.5).value
    f = dict(M=M, N=N, K=3 * C, amode=A_DENSE, Bn=1, A=qp, lda=3 * C, Wt=kp, ldw=3 * C, rows_per_b=1, out_split=0,
             out_f32=1, alpha=alpha, ldo_pad=16 if M == 64 else 0)
    khi, klo = _split(k.cpu())
    o = Ops(f, lambda: alpha * (_val(qp[:, :C], qp[:, C:2 * C]) @ _val(khi, klo).t()),
            lambda: (alpha * (_f32(qp) @ torch.cat([khi, khi, klo], 1).float().t())).double(), 1, M)
    o.keep = (qp, kp)
    return o


def softmax_planes(S: torch.Tensor, L: int) -> torch.Tensor:
    """tair_k_softmax_split on the device; the same arithmetic in torch fp32 on the CPU (emulation inputs)."""
    rows = S.shape[0]
    P = torch.empty(rows, 3 * L, dtype=torch.bfloat16, device=S.device)
    if S.is_cuda:
        from tair_amd import _lib
        _lib.check(_lib.lib().tair_k_softmax_split(S.data_ptr(), S.stride(0), rows, L, P.data_ptr(),
                                                   ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), "softmax")
    else:
        p = torch.softmax(S[:, :L].float(), -1)
        hi = p.to(torch.bfloat16)
        P.copy_(torch.cat([hi, (p - hi.float()).to(torch.bfloat16), hi], 1))
    return P


def transpose_planes(v: torch.Tensor, B: int, L: int, C: int) -> torch.Tensor:
    """tair_k_transpose_split on the device ([B][L][3C] (hi, lo, hi) -> [B][C][3L] (hi, hi, lo)); permute on the CPU."""
    y = torch.empty(B, C, 3 * L, dtype=torch.bfloat16, device=v.device)
    if v.is_cuda:
        from tair_amd import _lib
        _lib.check(_lib.lib().tair_k_transpose_split(v.data_ptr(), B, L, C, y.data_ptr(),
                                                     ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), "transpose")
    else:
        y.copy_(transpose_ref(v, B, L, C))
    return y


def transpose_ref(v: torch.Tensor, B: int, L: int, C: int) -> torch.Tensor:
    x = v.view(B, L, 3, C)
    return torch.stack([x[:, :, 0], x[:, :, 0], x[:, :, 1]], 1).permute(0, 3, 1, 2).reshape(B, C, 3 * L).contiguous()


def pv_ops(dev, L, C, *, seed=0) -> Ops:
    """O = P V + b_v over K = 3L: P from the softmax kernel's output on fp32 scores, V^T from the transpose
    kernel's output on a packed V (the operands the AttnBlock really feeds this GEMM)."""
    from tair_amd.vae_hip import _pack_act
    gen = torch.Generator().manual_seed(seed)
    S = (torch.randn(L, L, generator=gen) * 3).to(dev)
    vp = _pack_act((torch.randn(L, C, generator=gen) + 0.5).to(dev))
    bv = (torch.randn(C, generator=gen) * 0.3).to(dev)
    P = softmax_planes(S, L)
    vt = transpose_planes(vp, 1, L, C)[0]
    f = dict(M=L, N=C, K=3 * L, amode=A_DENSE, Bn=1, A=P, lda=3 * L, Wt=vt, ldw=3 * L, bias=bv, rows_per_b=1, out_split=1)
    o = Ops(f, lambda: _val(P[:, :L], P[:, L:2 * L]) @ _val(vt[:, :L], vt[:, 2 * L:]).t() + bv.cpu().double(),
            lambda: _store(_f32(P) @ _f32(vt).t() + _f32(bv), 1), 1, L)
    o.keep = (P, vt, bv, S, vp)
    return o


# ------------------------------------------------------------------------------------------------ the cases
class Case:
    """A GEMM case: build(dev, shape) -> Ops; `shapes` run under the planner's own plan, and every plan of
    the case's kind is forced at the first of `grow` (shapes in growing order) at which the validator accepts it
    and the planner really launches it."""

    def __init__(self, name, build, shapes, grow=None):
        self.name, self.build, self.shapes, self.grow = name, build, shapes, grow or shapes

    def ops(self, dev, shape) -> Ops:
        return self.build(dev, shape)


def _conv_case(name, amode, shapes, grow, **kw):
    seed = sum(map(ord, name))
    return Case(name, lambda dev, s: conv_ops(dev, amode, *s, seed=seed, **kw), shapes, grow)


def _dense_case(name, shapes, grow=None, **kw):
    seed = sum(map(ord, name))
    return Case(name, lambda dev, s: dense_ops(dev, *s, seed=seed, **kw), shapes, grow)


# conv shapes (B, H, W, cin, cout): 8x8 (one 64-row tile per image), 16x16 (one 256-row tile), the non-square 8x16
_RES = [(2, 8, 8, 128, 128), (2, 8, 16, 128, 128), (2, 16, 16, 128, 128)]
# a 256-column tile takes at most 62 groups (STAT_NG): 32 groups need >= 8 channels each, so Cout = 256
_RES_GROW = _RES + [(2, 8, 16, 128, 256), (2, 16, 16, 128, 256)]
_RES_GROW_SQ = _RES + [(2, 8, 16, 256, 256), (2, 16, 16, 256, 256)]  # residual: cin == cout

CASES = [
    _conv_case("conv_in4", A_SMALLC, [(2, 8, 8, 4, 128), (2, 8, 16, 4, 128)], None),
    _conv_case("conv_in3", A_SMALLC, [(2, 8, 8, 3, 128), (2, 8, 16, 3, 128)], None),
    _conv_case("res_conv1", A_CONV3, _RES, _RES_GROW),
    _conv_case("res_conv2_residual", A_CONV3, _RES, _RES_GROW_SQ, res=True),
    _conv_case("res_conv2_shortcut", A_CONV3, _RES, _RES_GROW, skip_cin=256),
    _conv_case("upsample", A_CONV3_UP, [(2, 8, 8, 128, 128), (2, 8, 16, 128, 128)],
               [(2, 8, 8, 128, 128), (2, 8, 16, 128, 128), (2, 8, 8, 128, 256)]),
    _conv_case("downsample", A_CONV3_S2, [(2, 16, 16, 128, 128), (2, 16, 32, 128, 128)],
               [(2, 16, 16, 128, 128), (2, 16, 32, 128, 128), (2, 16, 32, 128, 256)]),
    _conv_case("conv_out3", A_CONV3, [(2, 8, 8, 128, 3), (2, 8, 16, 128, 3)], None, stats=False, out_f32=True),
    _conv_case("conv_out8", A_CONV3, [(2, 8, 8, 128, 8)], None, stats=False, out_f32=True),
    # dense shapes (B, hw, C, N); M = 200: a ragged last tile; N = 96 runs with ldo > 3N
    _dense_case("q", [(1, 200, 128, 128), (1, 200, 128, 96)], out_split=1, bias=True),
    _dense_case("k", [(1, 200, 128, 128), (1, 200, 128, 96)], out_split=2, bias=True),
    _dense_case("v", [(1, 200, 128, 128), (1, 200, 128, 96)], out_split=1, bias=False),
    _dense_case("k_nobias", [(1, 200, 128, 128), (1, 200, 128, 96)], out_split=2, bias=False),
    _dense_case("proj_out", [(2, 64, 128, 128)], [(2, 64, 128, 128), (2, 128, 128, 128), (2, 128, 256, 256)],
                stats=True, res=True),
    Case("scores", lambda dev, s: scores_ops(dev, *s, seed=31), [(64, 64, 128), (256, 256, 128)]),
    Case("pv", lambda dev, s: pv_ops(dev, *s, seed=37), [(64, 128), (256, 128)]),
]
CASE = {c.name: c for c in CASES}


def force_fields(plan) -> Dict:
    kern, bm, bn, split = plan
    assert kern == KERN_TILE  # (every plan of the table is a 3-stage tile plan)
    return dict(force_bm=bm, force_bn=bn, force_splits=2 if split else 1, force_stages=3)


_PART = 1 << 24  # split-K workspace of the tests (fp32 elements)


def forced_shape(case: Case, plan, dev="cpu"):
    """(shape, Ops) of the first shape of case.grow at which the forced plan validates and is what would launch."""
    for shape in case.grow:
        o = case.ops(dev, shape)
        st = torch.zeros(1, dtype=torch.float64)
        d = o.desc(partial=1, partial_cap=_PART, out=1, ldo=3 * o.N, **force_fields(plan),
                   **(stat_fields(st.data_ptr(), o) if o.stats else {}))
        rc, (bm, bn, splits, kern) = plan_of(d)
        if rc == 0 and (kern, bm, bn, splits > 1) == tuple(plan):
            return shape, o
    return None, None


def stat_fields(ptr: int, o: Ops) -> Dict:
    return dict(st_acc=ptr, st_rs=2 * o.B * G, st_cg=o.N // G, st_G=G, st_coff=0, st_hw=o.hw)


def runs():
    """Every (case name, shape or None, plan or None) the GPU tests run: the planner's own plan at each shape of the
    case, and each plan of the case's kind forced (shape None: resolve() picks the smallest shape that takes it)."""
    out = []
    for c in CASES:
        out += [(c.name, s, None) for s in c.shapes]
        out += [(c.name, None, plan) for plan in plans_of(c.ops("cpu", c.shapes[0]).kind())]
    return out


def run_id(run) -> str:
    name, shape, plan = run
    return name + "-" + ("x".join(map(str, shape)) if plan is None else
                         "force%dx%d%s" % (plan[1], plan[2], "-splitk" if plan[3] else ""))


_OPS: Dict[tuple, Ops] = {}


def resolve(run, dev="cpu") -> Ops:
    """The operands of a run on dev, built (and their reference computed) once per (case, shape, device)."""
    name, shape, plan = run
    if shape is None:
        shape, _ = forced_shape(CASE[name], plan)
        assert shape is not None, f"{name}: no shape of the case takes the forced plan {plan}"
    key = (name, shape, str(dev))
    if key not in _OPS:
        _OPS[key] = CASE[name].ops(dev, shape)
    return _OPS[key]


# ------------------------------------------------------------------------------------------------ the checks
TOL_ALL = 2e-5   # whole tensor, hi + lo outputs against fp64 (tests/test_kernels_gpu.py two-plane trunk)
SKIP_BELOW = 1e-3  # rows / columns whose reference norm is below this share of the RMS row / column norm
MAX_SKIPPED = 0.01
R_ROWCOL = 4.4e-5  # every row, every column: 4 x the worst value of the fp32 emulation, 1.093e-5 (test_vae_plans_cpu.py)


def rowcol_errors(got: torch.Tensor, ref: torch.Tensor):
    """(worst per-row rel-L2, worst per-column rel-L2, share of rows skipped, share of columns skipped)."""
    got, ref = got.double(), ref.double()
    res = []
    for dim in (1, 0):
        nr = ref.norm(dim=dim)
        keep = nr >= SKIP_BELOW * nr.pow(2).mean().sqrt()
        e = (got - ref).norm(dim=dim)[keep] / nr[keep]
        res.append((e.max().item(), 1.0 - keep.double().mean().item()))
    return res[0][0], res[1][0], res[0][1], res[1][1]
