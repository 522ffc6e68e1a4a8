"""The kernels of the split-precision VAE (tair_amd/vae_hip.py), one by one against fp64.

Every GEMM epilogue and loader path that only the VAE uses -- out_split 1 (hi, lo, hi) and 2 (hi, hi, lo), res_lo
with out_split, st_acc statistics of the fp32 value, the CONV3 / CONV3_UP / CONV3_S2 + s2_shift / CONV3_SMALLC
loaders over 3 Cin plane channels (C = 9 and 12 included), fp32 output of a split-operand GEMM with alpha -- runs
at the smallest shapes where it can go wrong, under the planner's own plan and under every tile plan the VAE
launches at the workload's shape (tests/_vae_cases.py SIGNATURES, pinned by tests/test_vae_plans_cpu.py), forced
with force_bm / force_bn / force_splits / force_stages.  Operands come from the product's packers (_pack_act,
_pack_weight, _Conv); the reference is plain torch fp64 on the values the stored bf16 planes hold (hi + lo).

GEMM tolerances
* whole tensor: rel-L2 <= 2e-5, the project's figure for hi + lo outputs (test_gemm_two_plane_trunk_and_split_skip);
* every output row and, separately, every output column: rel-L2 <= R = 4.4e-5.  R is 4 x the worst per-row /
  per-column value that a CPU emulation of the same arithmetic (the three plane products accumulated in fp32 by
  torch, fp32 epilogue, hi + lo storage) reaches against fp64 over these very inputs: 1.093e-5, a 3-element row of
  conv_out (the other cases stay under 6.5e-6); tests/test_vae_plans_cpu.py measures it again and holds R to it.
  The factor covers another summation order on the device (measured on MI355X: whole tensor 1.9e-6 .. 3.7e-6,
  worst row 1.25e-5 -- the same conv_out rows -- and 5.5e-6 elsewhere, worst column 6.4e-6).  One lost lo plane
  costs ~1e-3 (dropping the residual's lo term: 8.3e-4 .. 1.5e-3 on the whole tensor);
* rows / columns whose reference norm is below 1e-3 of the RMS row / column norm are skipped, at most 1 % per case
  (none at these seeds: checked on the CPU);
* the redundant plane equals the hi plane bitwise; rows past M, columns past the planes and guard elements around
  the buffer keep their sentinel;
* statistics: st.sum(0) against the fp64 sums of the reconstructed output per (batch element, group), with the
  bounds of tests/test_ffpout_gpu.py _check_stats; the batch elements have clearly different means.

tair_k_softmax_split: |hi + lo - softmax_fp64| <= 2^-15 ref where ref >= 1e-30, <= 1e-30 below (fp32 exp of an
argument up to ~60 in magnitude carries <= ~7e-6 relative error, hi + lo storage adds 2^-18); row sums within 1e-5
of 1 (measured: 9.0e-6 and 2.9e-6).  tair_k_transpose_split: bitwise.  tair_k_gn_apply_stats with x_lo / y_split: rel-L2 <= 2e-5 per batch
element, as the existing case.
"""
import ctypes

import pytest
import torch

import _vae_cases as vc

pytestmark = pytest.mark.gpu

DEV = "cuda"
GUARD = 64       # sentinel elements before and after every output buffer
EXTRA_ROWS = 8   # sentinel rows past M
SENTINEL = 768.0  # exact in bf16, far from every value of the cases


def _L():
    from tair_amd import _lib
    return _lib.lib(), _lib


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def rel_l2(a, b):
    a, b = a.double(), b.double()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def _guarded(rows, ld, dtype):
    """(flat buffer, [rows, ld] view GUARD elements into it), all SENTINEL."""
    flat = torch.full((2 * GUARD + rows * ld,), SENTINEL, dtype=dtype, device=DEV)
    return flat, flat[GUARD:GUARD + rows * ld].view(rows, ld)


def _guards_intact(flat, n):
    return bool((flat[:GUARD] == SENTINEL).all()) and bool((flat[GUARD + n:] == SENTINEL).all())


_WS = {}


def _workspace():
    if not _WS:
        _WS["part"] = torch.empty(vc._PART, dtype=torch.float32, device=DEV)
    return _WS["part"]


@pytest.mark.parametrize("run", vc.runs(), ids=vc.run_id)
def test_vae_gemm_against_fp64(run):
    from test_ffpout_gpu import _check_stats
    L, lib = _L()
    name, _, plan = run
    o = vc.resolve(run, DEV)
    M, N = o.M, o.N
    planes = 3 if o.out_split else 1
    ldo = planes * N + o.ldo_pad
    flat, out = _guarded(M + EXTRA_ROWS, ldo, torch.float32 if o.out_f32 else torch.bfloat16)
    part = _workspace()
    extra = dict(out=out, ldo=ldo, partial=part, partial_cap=part.numel())
    st = None
    if o.stats:
        st = torch.zeros(8, 2 * o.B * vc.G, dtype=torch.float64, device=DEV)
        extra.update(vc.stat_fields(st.data_ptr(), o))
    if plan is not None:
        extra.update(vc.force_fields(plan))
    d = o.desc(**extra)
    rc, (bm, bn, splits, kern) = vc.plan_of(d)
    assert rc == 0, L.tair_last_error()
    if plan is not None:  # the forced plan is the one that launches
        assert (kern, bm, bn, splits > 1) == tuple(plan), (bm, bn, splits, kern)
    assert L.tair_k_gemm(ctypes.byref(d), _stream()) == 0, L.tair_last_error()
    torch.cuda.synchronize()
    lib.check_faults(name)

    # nothing outside [M][planes * N]
    assert _guards_intact(flat, out.numel())
    assert bool((out[M:] == SENTINEL).all()), "rows past M written"
    assert bool((out[:, planes * N:] == SENTINEL).all()), "columns past the planes written"
    if o.out_split:
        hi = out[:M, :N]
        lo, dup = (out[:M, N:2 * N], out[:M, 2 * N:3 * N]) if o.out_split == 1 else (out[:M, 2 * N:3 * N], out[:M, N:2 * N])
        assert torch.equal(dup, hi), "the redundant plane differs from the hi plane"
        got = hi.double() + lo.double()
    else:
        got = out[:M, :N].double()
    got = got.cpu()
    assert bool(torch.isfinite(got).all())
    e = rel_l2(got, o.ref)
    er, ec, sr, sc = vc.rowcol_errors(got, o.ref)
    print(f"vae gemm {vc.run_id(run)} M={M} N={N} plan {bm}x{bn}/{splits} kernel {kern}: whole {e:.3e} worst row "
          f"{er:.3e} worst column {ec:.3e} skipped {sr:.3f}/{sc:.3f}")
    assert sr <= vc.MAX_SKIPPED and sc <= vc.MAX_SKIPPED, (sr, sc)
    assert e <= vc.TOL_ALL, e
    assert er <= vc.R_ROWCOL, er
    assert ec <= vc.R_ROWCOL, ec
    if o.stats:
        _check_stats(st, torch.stack([hi, lo]), o.B, o.hw, N, vc.G)


# ------------------------------------------------------------------------------------------------ softmax
def _softmax_rows(L, group, gen):
    r = (torch.rand(3, L, generator=gen) - 0.5) * 30           # random rows with a spread of ~30
    if group == 0:
        r[1] = torch.randn(L, generator=gen)                     # one-hot dominant
        r[1, (7 * L) // 11] += 40.0
        r[2] = 2.5                                               # all equal
    else:
        r[0] += 3.0e4                                            # the max subtraction
        r[1, ::3] = -1.0e4                                       # exact zeros
        if L > 1:
            r[1, 1] = 4.0
    return r


@pytest.mark.parametrize("group", [0, 1], ids=["random-onehot-equal", "shifted-zeros-random"])
@pytest.mark.parametrize("L", [1, 63, 64, 100, 255, 256, 257, 1000])
def test_softmax_split_against_fp64(L, group):
    Lb, _ = _L()
    rows, lds = 3, L + 5
    gen = torch.Generator().manual_seed(100 * L + group)
    S = torch.full((rows, lds), float("nan"))
    S[:, :L] = _softmax_rows(L, group, gen)
    ref = torch.softmax(S[:, :L].double(), -1)
    Sd = S.to(DEV)
    flat, P = _guarded(rows, 3 * L, torch.bfloat16)
    assert Lb.tair_k_softmax_split(Sd.data_ptr(), lds, rows, L, P.data_ptr(), _stream()) == 0
    torch.cuda.synchronize()
    assert _guards_intact(flat, P.numel())
    assert torch.equal(P[:, 2 * L:], P[:, :L]), "third plane differs from the first"
    p = (P[:, :L].double() + P[:, L:2 * L].double()).cpu()
    assert bool(torch.isfinite(p).all())
    big = ref >= 1e-30
    rel = ((p - ref).abs()[big] / ref[big]).max().item()
    small = (p - ref).abs()[~big].max().item() if bool((~big).any()) else 0.0
    sums = (p.sum(-1) - 1).abs().max().item()
    print(f"softmax_split L={L} group {group}: worst relative error {rel:.3e}, below 1e-30: {small:.3e}, "
          f"row sums off by {sums:.3e}")
    assert rel <= 2.0 ** -15, rel
    assert small <= 1e-30, small
    assert sums <= 1e-5, sums
    if group == 1 and L > 3:
        assert bool((p[1, ::3] == 0).all())  # the entries at -1e4 are exact zeros


# ------------------------------------------------------------------------------------------------ transpose
@pytest.mark.parametrize("L,C", [(1, 1), (64, 64), (100, 96), (65, 130), (256, 512)])
def test_transpose_split_bitwise(L, C):
    Lb, _ = _L()
    B = 2
    gen = torch.Generator().manual_seed(L * 1000 + C)
    x = (torch.randn(B, L, 3 * C, generator=gen) * 3).to(torch.bfloat16).to(DEV)  # three independent planes
    flat, y = _guarded(B * C, 3 * L, torch.bfloat16)
    assert Lb.tair_k_transpose_split(x.data_ptr(), B, L, C, y.data_ptr(), _stream()) == 0
    torch.cuda.synchronize()
    assert _guards_intact(flat, y.numel())
    assert torch.equal(y.view(B, C, 3 * L), vc.transpose_ref(x, B, L, C))


# ------------------------------------------------------------------------------------------------ GroupNorm apply
@pytest.mark.parametrize("B,HW,C,silu", [(2, 64, 512, 1), (3, 256, 128, 1), (2, 64, 512, 0)])
def test_gn_apply_split_planes_per_batch_element(B, HW, C, silu):
    """tair_k_gn_apply_stats with x_lo and y_split (the VAE's GroupNorm): batch elements of different means with
    |mean| ~ 10 std, so statistics read from another batch element's slot cannot pass."""
    import torch.nn.functional as F
    Lb, _ = _L()
    eps, G = 1e-6, vc.G
    gen = torch.Generator().manual_seed(B * 1000 + C)
    mean = torch.tensor([10.0, -10.0, 5.0][:B]).view(B, 1, 1)
    std = torch.tensor([1.0, 1.0, 0.5][:B]).view(B, 1, 1)
    xf = (torch.randn(B, HW, C, generator=gen) * std + mean).to(DEV)
    hi = xf.to(torch.bfloat16)
    lo = (xf - hi.float()).to(torch.bfloat16)
    xs = torch.cat([hi, lo, hi], -1).contiguous()
    xval = hi.double() + lo.double()
    gr = xval.view(B, HW, G, C // G)
    sums = torch.stack([gr.sum(dim=(1, 3)), (gr * gr).sum(dim=(1, 3))], -1).flatten()
    rs = B * G * 2
    st = torch.zeros(8, rs, device=DEV, dtype=torch.float64)
    st[1], st[6] = sums * 0.25, sums * 0.75  # spread over replicas as the epilogues do
    g = (torch.rand(C, generator=gen) + 0.5).to(DEV)
    be = torch.randn(C, generator=gen).to(DEV)
    flat, y = _guarded(B * HW, 3 * C, torch.bfloat16)
    assert Lb.tair_k_gn_apply_stats(xs.data_ptr(), 3 * C, C, B, HW, C, G, eps, g.data_ptr(), be.data_ptr(), silu,
                                    st.data_ptr(), rs, y.data_ptr(), 3 * C, 1, _stream()) == 0
    torch.cuda.synchronize()
    assert _guards_intact(flat, y.numel())
    ref = F.group_norm(xval.permute(0, 2, 1), G, g.double(), be.double(), eps)
    if silu:
        ref = F.silu(ref)
    assert torch.equal(y[:, :C], y[:, 2 * C:]), "third plane differs from the first"
    got = (y[:, :C].double() + y[:, C:2 * C].double()).view(B, HW, C).permute(0, 2, 1)
    errs = [rel_l2(got[b], ref[b]) for b in range(B)]
    print(f"gn_apply split B={B} HW={HW} C={C} silu={silu}: rel-L2 per batch element {errs}")
    assert max(errs) <= 2e-5, errs
