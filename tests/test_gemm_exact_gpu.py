"""The bf16 / fp8 MFMA GEMM and implicit-GEMM conv families (tair_k_gemm) on exact-answer inputs: every case of
tests/_exact_cases.py must reproduce its int64 reference bit for bit -- in the bf16 output, the fp32 output, the hi
plane of a hi / lo pair and of the three split planes (the lo planes exactly zero) -- under the plan it names, which
tests/test_exact_cases_cpu.py has shown it to resolve to and which is asserted again here before the launch.  With
small-integer operands the summation order, the K split, the combine, the ring depth and the tile shape cannot
change a bit, so an addressing defect shows however few outputs it touches: a dropped K element, a tile edge, an
image border, a neighbour taken from the previous image row.

Inputs live between NaN guard rows and NaN padding columns, outputs between sentinel rows and columns that must
survive (_guarded / _guards_intact of tests/test_clip_hip_gpu.py); the split-K workspace starts as NaN.  With tickets
the launch runs twice on the same tickets, which must be back at zero, and gives the same bits; the device fault
counter stays 0.  test_plans_agree runs one descriptor under every forced plan that accepts it: all outputs agree
bitwise with the reference and so with one another.

Measured on MI355X: all 716 cases and the three all-plans descriptors exact; the module runs in about 9 s.  The
cooperative combine is requested (tickets), not verified: tair_k_gemm_plan reports kernel, tile and slices only, and
the launcher falls back to the last-arriver combine when the grid is not resident.  Sensitivity, on scratch builds: a
stride-1 conv's left border clamped to x = 0 instead of padded fails 48 cases when made in the 4-wave tile family and
56 in the deep-ring family (where the earlier suites see it in one statistics case only); dropping the last K-tile
of the last slice in gemm_tile_kernel fails 69."""
import ctypes

import pytest
import torch

import _exact_cases as ec

pytestmark = pytest.mark.gpu

GEMM_PARAMS = ec.CASES
AGREE_PARAMS = [c for c, _ in ec.AGREE]
DEV = "cuda"
SENTINEL = 768.0  # exact in bf16 and far from every value of the cases
NAN = float("nan")


def _L():
    from tair_amd import _lib
    return _lib.lib(), _lib


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _helpers():
    from test_clip_hip_gpu import _guarded, _guards_intact
    return _guarded, _guards_intact


_WS = {}


def _ws():
    if not _WS:
        _WS["part"] = torch.full((ec.PART_CAP,), NAN, dtype=torch.float32, device=DEV)
        _WS["sem"] = torch.zeros(ec.SEM_CAP, dtype=torch.int32, device=DEV)
    return _WS["part"], _WS["sem"]


def _e4m3_bytes(t: torch.Tensor) -> torch.Tensor:
    """-1 / 0 / +1 as OCP e4m3 bytes: 1.0 = 0x38, the sign in bit 7."""
    t = t.to(torch.int16)
    return (t.abs() * ec.E4M3_ONE + (t < 0) * 0x80).to(torch.uint8)


class DevOps:
    """The operands of an _exact_cases.Ops in guarded device buffers, the descriptor fields that point at them and the
    expected output (computed once per operand set and left unchanged)."""

    def __init__(self, o: ec.Ops):
        guarded, _ = _helpers()
        self.o = o
        ld = ec.leading_dims(o)
        f = dict(o.fields(), **ld)
        keep = self.keep = []

        def put(vals, dtype, guard=8, pad=ec.PAD, fill=NAN):
            buf, view = guarded(vals.shape[0], vals.shape[1], fill, dtype, pad, guard)
            view.copy_(vals.to(DEV))
            keep.append(buf)
            return view

        # a conv's padding taps lie up to W + 1 pixel rows outside the image: NaN guard rows there
        a_guard = 8 if o.src[0] == "dense" else (o.W + 2 + 7) // 8 * 8
        a2 = o.a.reshape(-1, o.a.shape[-1])
        if o.f8:
            A = put(_e4m3_bytes(a2), torch.uint8, a_guard, ec.PAD, ec.E4M3_NAN)
            assert A.stride(0) == 2 * ld["lda"]
        else:
            A = put(a2, torch.bfloat16, a_guard)
            assert A.stride(0) == ld["lda"]
        f["A"] = A.data_ptr()
        pw = o.packed_w()
        if o.f8:  # rows of e4m3 bytes, then the bf16 K-extension columns
            kv = 2 * o.Kd
            rows = torch.full((o.N, kv + 2 * o.Kx), 0, dtype=torch.uint8)
            rows[:, :kv] = _e4m3_bytes(pw[:, :kv])
            if o.Kx:
                rows[:, kv:] = pw[:, kv:].contiguous().to(torch.bfloat16).view(torch.uint8).reshape(o.N, 2 * o.Kx)
            Wt = put(rows, torch.uint8, 8, 2 * ec.PAD, ec.E4M3_NAN)
            assert Wt.stride(0) == 2 * ld["ldw"]
        else:
            Wt = put(pw, torch.bfloat16, 8, 64)
            assert Wt.stride(0) == ld["ldw"]
        f["Wt"] = Wt.data_ptr()
        if o.Kx:
            X = put(o.x, torch.bfloat16)
            f["X"] = X.data_ptr()
        if o.has_bias:
            bias = torch.full((o.N + 16,), NAN, dtype=torch.float32, device=DEV)
            bias[8:8 + o.N] = o.bias.to(DEV)
            keep.append(bias)
            f["bias"] = bias[8:].data_ptr()
        if o.emb is not None:
            e = o.emb.float().clone()
            e[0] = NAN  # row 0 is never read (emb_row permutes 1 .. B)
            emb = put(e, torch.float32, 8)
            rows = o.emb_row.to(DEV)
            keep.append(rows)
            f.update(emb=emb.data_ptr(), emb_row=rows.data_ptr())
        if o.res is not None:
            f["res"] = put(o.res, torch.bfloat16).data_ptr()
        if o.f8:
            cs = o.col_scale.float().to(DEV)
            keep.append(cs)
            f["col_scale"] = cs.data_ptr()
            if o.row_scale is not None:
                rs = o.row_scale.float().to(DEV)
                keep.append(rs)
                f["row_scale"] = rs.data_ptr()
        self.fields = f
        self.ldo = ld["ldo"]
        self.want = o.value(DEV)  # fp64 [M, N], exact


_DEV: dict = {}


def _devops(case) -> DevOps:
    key = (case.src, case.N, case.epi)
    if key not in _DEV:
        _DEV[key] = DevOps(ec.operands(case))
    return _DEV[key]


def _where(case, o, bad):
    """'(m, n)' of the first wrong elements, with (b, y, x) of a conv's output pixel."""
    idx = bad.nonzero()[:8].tolist()
    if not case.is_conv:
        return ", ".join(f"({m}, {n})" for m, n in idx)
    Ho, Wo = ec.out_hw(case.src)
    rows = bad.any(1).nonzero().flatten()
    ys, xs = sorted(set((rows % (Ho * Wo) // Wo).tolist())), sorted(set((rows % Wo).tolist()))
    first = ", ".join(f"({m}, {n}) = pixel (b {m // (Ho * Wo)}, y {m % (Ho * Wo) // Wo}, x {m % Wo})" for m, n in idx)
    return f"{first}; {rows.numel()} wrong pixels of {o.M}, with y in {ys[:12]} and x in {xs[:12]} (image {Ho} x {Wo})"


def _bits_equal(got: torch.Tensor, want64: torch.Tensor):
    """Elementwise: got (bf16 or fp32) holds exactly the bits of want (fp64 values that both formats represent)."""
    w = want64.to(got.dtype)
    itype = torch.int16 if got.dtype == torch.bfloat16 else torch.int32
    return got.contiguous().view(itype) == w.contiguous().view(itype)


def run_case(case, force=None, combine=None):
    """Launch the case (or its descriptor under another forced plan) and check everything; returns the output planes."""
    L, _ = _L()
    guarded, guards_intact = _helpers()
    d_ops = _devops(case)
    o = d_ops.o
    part, sem = _ws()
    M, N = o.M, o.N
    f32, split, out_lo = bool(o.f.get("out_f32")), o.f.get("out_split", 0), bool(o.f.get("out_lo"))
    dtype = torch.float32 if f32 else torch.bfloat16
    cols = 3 * N if split else N
    rows = 2 * M + 16 if out_lo else M
    buf, view = guarded(rows, cols, SENTINEL, dtype)
    assert view.stride(0) == d_ops.ldo
    kw = dict(d_ops.fields, out=view.data_ptr(), **ec.force_fields(force or case.force),
              **ec.combine_fields(combine or case.combine, part.data_ptr(), sem.data_ptr()))
    if out_lo:
        kw["out_lo"] = (M + 16) * d_ops.ldo
    d = ec.make_desc(**kw)
    rc, plan = ec.plan_of(d)
    assert rc == 0, L.tair_last_error()
    expect = case.expect if force is None else ec.expect_forced(case.src, force)
    assert plan == expect, (plan, expect)
    tickets = (combine or case.combine) in ("coop", "last") and plan[3] > 1
    outs = []
    for _ in range(2 if tickets else 1):
        view.fill_(SENTINEL)
        rc = L.tair_k_gemm(ctypes.byref(d), _stream())
        assert rc == 0, L.tair_last_error()
        torch.cuda.synchronize()
        assert int(sem.count_nonzero()) == 0, "split-K tickets not back at zero"
        outs.append(view.clone())
    cnt = ctypes.c_int(-1)
    assert L.tair_fault_count(1, ctypes.byref(cnt)) == 0 and cnt.value == 0, f"device fault counter {cnt.value}"
    got = outs[0]
    planes = {"hi": got[:M, :N]}
    if out_lo:
        planes["lo"] = got[M + 16:, :N]
        assert bool((got[M:M + 16] == SENTINEL).all()), "rows between the hi and lo planes written"
    if split:  # (hi, lo, hi) or (hi, hi, lo)
        second, third = got[:, N:2 * N], got[:, 2 * N:]
        planes["lo"] = second if split == 1 else third
        planes["hi2"] = third if split == 1 else second
    for name, p in planes.items():
        want = d_ops.want if name != "lo" else torch.zeros_like(d_ops.want)
        ok = _bits_equal(p, want)
        if not bool(ok.all()):
            bad = ~ok
            m, n = bad.nonzero()[0].tolist()
            raise AssertionError(f"{case.name} plan {plan}: {int(bad.sum())} of {M * N} elements of the {name} plane "
                                 f"differ from the int64 answer; first at {_where(case, o, bad)}; got "
                                 f"{p[m, n].item()!r}, want {want[m, n].item()!r}")
    assert guards_intact(buf, view, SENTINEL), "output guard rows / padding columns written"
    if tickets:
        assert torch.equal(outs[0].view(torch.int16 if not f32 else torch.int32),
                           outs[1].view(torch.int16 if not f32 else torch.int32)), "second launch on the same tickets differs"
    return got


@pytest.mark.parametrize("case", GEMM_PARAMS, ids=repr)
def test_gemm_exact(case):
    run_case(case)


@pytest.mark.parametrize("case", AGREE_PARAMS, ids=repr)
def test_plans_agree(case):
    """One descriptor under every forced plan of ALL_PLANS that accepts it (how many: tests/test_exact_cases_cpu.py):
    every output equals the int64 answer bit for bit (run_case), and so the plans agree with one another, which is
    asserted as well."""
    accepting = dict((c.name, n) for c, n in ec.AGREE)[case.name]
    first, n = None, 0
    part, sem = _ws()
    for force in ec.ALL_PLANS:
        probe = ec.make_desc(**dict(_devops(case).fields, out=64, **ec.force_fields(force),
                                    **ec.combine_fields("reduce", part.data_ptr(), sem.data_ptr())))
        if ec.plan_of(probe)[0] != 0:
            continue  # a plan the library refuses for this descriptor (counted on the CPU)
        for combine in (("reduce", "last") if force[0] == 64 and force[2] > 1 and force[3] != 2 else ("reduce",)):
            got = run_case(case, force, combine)
            if first is None:
                first = got
            assert torch.equal(got.view(torch.int16), first.view(torch.int16)), (force, combine)
        n += 1
    assert n == accepting, (n, accepting)
