"""Two lanes in ONE launch (tair_k_gemm_grouped), kernel by kernel, with exact answers: every pair of
tests/_exact_cases.py GROUP_CASES goes out as one grouped launch into two guarded outputs, and every plane of BOTH
lanes -- bf16, fp32, the hi / lo pair, the three split planes with lo exactly zero -- must equal its own lane's int64
answer bit for bit.  The lanes' operands are independent draws and their feature sets may differ, and
tests/test_grouped_cases_cpu.py has shown that the two answers differ in at least half of their elements and that any
single operand taken from the other lane changes the answer: a tile computed by the wrong lane, a bias, residual or
embedding row read from the other lane, or a slab of lane 1 summed into lane 0 shows in the lane, plan and first
(m, n) the failure names.  Each lane has its own NaN-filled split-K workspace and its own zeroed tickets; after every
launch both ticket arrays are back at zero, a ticketed launch runs twice and gives the same bits; sentinels around
both outputs survive and the device fault counter stays 0.  The plan of two lanes is asserted before every launch
(tair_k_gemm_plan_lanes).

Also here, with two lanes:
* GroupNorm producer statistics (both targets of each lane, distinct group widths and offsets per lane): the stored
  values are integers of at most 8 bits, so the (sum, sum of squares) per (batch element, group) are integers that
  fp64 holds exactly whatever the atomics' order: the sum over the 8 replicas of each lane's accumulators equals the
  int64 sums exactly, every slot the lane does not own stays zero.
* LayerNorm row statistics (rst): each lane's (sum, sum of squares) per output row, exact integers, equal.
* A folded-LayerNorm consumer pair (lnst / lncs) and GroupNorm on load (gn_st; a halo plan, whose 2-stage ring is chosen
  per lane, and a tile plan) have no exact answer: both lanes bitwise equal to the same descriptor launched alone
  under the same forced plan.

Measured on MI355X: all 117 pairs exact in both lanes, the 9 statistics, 5 row-statistics, 3 folded-LayerNorm and
3 GroupNorm-on-load cases pass (137 tests); the module runs in about 6 s, most of it the blocked-order case's operands
and the first launch.  No defect of the grouped path was found.  Sensitivity, on scratch builds (this module's 137 and
the 74 tests of tests/test_grouped_kernels_gpu.py, which none of the three defects touches): lane 0's bias read for
both lanes in gemm_tile_kernel's epilogue_tile call fails 59 (48 pairs, 6 statistics, 4 row-statistics cases, 1
folded-LayerNorm case); splitk_reduce_kernel summing lane 0's slabs for both lanes fails 41 (38 pairs, 2 statistics
cases, the split GroupNorm-on-load case); the last m-tile of lane 0 taken for lane 1 in the 4-phase kernel (the tile
index kept from the true lane, so every address stays in bounds) fails 3, the three 4-phase pairs.
"""
import ctypes

import pytest
import torch

import _exact_cases as ec

pytestmark = pytest.mark.gpu

GROUP_PARAMS = ec.GROUP_CASES
DEV = "cuda"
SENTINEL = 768.0
NAN = float("nan")
STAT_REPL = 8


def _L():
    from tair_amd import _lib
    return _lib.lib(), _lib


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _helpers():
    from test_clip_hip_gpu import _guarded, _guards_intact
    return _guarded, _guards_intact


def _single():
    import test_gemm_exact_gpu as tg
    return tg


_WS = {}


def _ws(lane):
    """Lane `lane`'s own split-K workspace (NaN) and tickets (zero)."""
    if lane not in _WS:
        _WS[lane] = (torch.full((ec.PART_CAP,), NAN, dtype=torch.float32, device=DEV),
                     torch.zeros(ec.SEM_CAP, dtype=torch.int32, device=DEV))
    return _WS[lane]


_DEV: dict = {}


def _devops(case):
    key = (case.src, case.N, case.epi, case.lane)
    if key not in _DEV:
        _DEV[key] = _single().DevOps(ec.operands(case))
    return _DEV[key]


class LaneOut:
    """A lane's guarded output and the descriptor fields that point at it."""

    def __init__(self, d_ops):
        guarded, _ = _helpers()
        o = self.o = d_ops.o
        self.f32, self.split, self.out_lo = bool(o.f.get("out_f32")), o.f.get("out_split", 0), bool(o.f.get("out_lo"))
        cols = 3 * o.N if self.split else o.N
        rows = 2 * o.M + 16 if self.out_lo else o.M
        self.buf, self.view = guarded(rows, cols, SENTINEL, torch.float32 if self.f32 else torch.bfloat16)
        assert self.view.stride(0) == d_ops.ldo
        self.fields = dict(out=self.view.data_ptr())
        if self.out_lo:
            self.fields["out_lo"] = (o.M + 16) * d_ops.ldo

    def planes(self, got):
        o, M, N = self.o, self.o.M, self.o.N
        p = {"hi": got[:M, :N]}
        if self.out_lo:
            p["lo"] = got[M + 16:, :N]
            assert bool((got[M:M + 16] == SENTINEL).all()), "rows between the hi and lo planes written"
        if self.split:
            second, third = got[:, N:2 * N], got[:, 2 * N:]
            p["lo"] = second if self.split == 1 else third
            p["hi2"] = third if self.split == 1 else second
        return p


def launch_pair(arr, outs, tickets, reset=None):
    """One grouped launch (two when ticketed) of the descriptor pair; returns per launch the clones of both outputs.
    reset: called before every launch (accumulators that a launch adds to start from zero each time)."""
    L, _ = _L()
    runs = []
    for _ in range(2 if tickets else 1):
        for lo in outs:
            lo.view.fill_(SENTINEL)
        if reset:
            reset()
        rc = L.tair_k_gemm_grouped(arr, 2, _stream())
        assert rc == 0, L.tair_last_error()
        torch.cuda.synchronize()
        for i in range(2):
            assert int(_ws(i)[1].count_nonzero()) == 0, f"lane {i}: split-K tickets not back at zero"
        runs.append([lo.view.clone() for lo in outs])
    cnt = ctypes.c_int(-1)
    assert L.tair_fault_count(1, ctypes.byref(cnt)) == 0 and cnt.value == 0, f"device fault counter {cnt.value}"
    return runs


def pair_fields(gc, extra=None):
    """Per lane: the device operands' descriptor fields, the forced plan, the lane's own workspace and tickets, its own
    guarded output (and whatever `extra[i]` adds)."""
    d_ops = [_devops(gc.lane(i)) for i in range(2)]
    outs = [LaneOut(d) for d in d_ops]
    ptrs = []
    for i in range(2):
        part, sem = _ws(i)
        ptrs.append(dict(d_ops[i].fields, **outs[i].fields, **ec.force_fields(gc.force),
                         **ec.combine_fields(gc.combine, part.data_ptr(), sem.data_ptr()), **((extra or [{}, {}])[i])))
    return d_ops, outs, ptrs


def check_lanes(gc, plan, d_ops, outs, got):
    tg = _single()
    _, guards_intact = _helpers()
    for i in range(2):
        o = d_ops[i].o
        for name, p in outs[i].planes(got[i]).items():
            want = d_ops[i].want if name != "lo" else torch.zeros_like(d_ops[i].want)
            ok = tg._bits_equal(p, want)
            if not bool(ok.all()):
                bad = ~ok
                m, n = bad.nonzero()[0].tolist()
                other = tg._bits_equal(p, d_ops[1 - i].want if name != "lo" else want)
                raise AssertionError(
                    f"{gc.name} lane {i} ({gc.epis[i]}) plan {plan}: {int(bad.sum())} of {o.M * o.N} elements of the "
                    f"{name} plane differ from the lane's int64 answer ({int((bad & other).sum())} of them hold the OTHER "
                    f"lane's answer); first at {tg._where(gc.lane(i), o, bad)}; got {p[m, n].item()!r}, want "
                    f"{want[m, n].item()!r}")
        assert guards_intact(outs[i].buf, outs[i].view, SENTINEL), f"lane {i}: output guard rows / padding columns written"


def run_pair(gc, extra=None, reset=None):
    d_ops, outs, ptrs = pair_fields(gc, extra)
    arr = ec.pair_descs(gc, ptrs)
    rc, plan = ec.plan_of_lanes(arr[0], 2)
    assert rc == 0, _L()[0].tair_last_error()
    assert plan == gc.expect, (plan, gc.expect)
    tickets = gc.combine in ("coop", "last") and plan[3] > 1
    runs = launch_pair(arr, outs, tickets, reset)
    check_lanes(gc, plan, d_ops, outs, runs[0])
    if tickets:
        for i in range(2):
            it = torch.int32 if outs[i].f32 else torch.int16
            assert torch.equal(runs[0][i].view(it), runs[1][i].view(it)), f"lane {i}: second launch on the same tickets differs"
    return d_ops, outs, runs[0]


@pytest.mark.parametrize("gc", GROUP_PARAMS, ids=repr)
def test_grouped_exact(gc):
    run_pair(gc)


# ---- GroupNorm producer statistics, two lanes ---------------------------------------------------------------------------
# per lane two targets (cg, G, c_off) over the N = 200 output channels; every channel falls into a group below G
ST_TGT = (((8, 32, 0), (20, 32, 40)), ((10, 32, 20), (40, 16, 0)))
ST_SRC = {64: ec.conv(ec.A_CONV3, 2, 8, 8, 64), 256: ec.conv(ec.A_CONV3, 2, 16, 16, 64)}
# (hw, forced plan, combine, the plan it resolves to: a tile must not straddle two batch elements, so with hw = 64 the
# 128 x 128 request becomes 64 x 128 -- tests/_gn_stat_cases.py states the rule)
ST_PLANS = [
    (64, (64, 64, 1, ec.T3), None, (ec.K_TILE, 64, 64, 1)),
    (256, (64, 64, 1, ec.T3), None, (ec.K_TILE, 64, 64, 1)),
    (64, (128, 128, 1, ec.T3), None, (ec.K_TILE, 64, 128, 1)),
    (256, (128, 128, 1, ec.T3), None, (ec.K_TILE, 128, 128, 1)),
    (64, (64, 64, 3, ec.T3), "coop", (ec.K_TILE, 64, 64, 3)),
    (256, (64, 64, 3, ec.T3), "last", (ec.K_TILE, 64, 64, 3)),
    (64, (64, 64, 3, ec.T3), "reduce", (ec.K_TILE, 64, 64, 3)),
    (256, (128, 128, 2, ec.T3), "reduce", (ec.K_TILE, 128, 128, 2)),
    (256, (256, 128, 1, 9), None, (ec.K_HALO, 256, 128, 1)),
]
ST_PAIRS = (("b", "ber"), ("lo", "br"), ("br", "b"))


def _group_sums(v, B, hw, tgt):
    """int64-exact fp64 [B, G, 2]: (sum, sum of squares) of the stored values v [B hw, N] per group of target tgt."""
    cg, G, c_off = tgt
    N = v.shape[1]
    gi = (c_off + torch.arange(N, device=v.device)) // cg
    assert int(gi.max()) < G
    v = v.view(B, hw, N)
    out = torch.zeros(2, B, G, dtype=torch.float64, device=v.device)
    out.index_add_(2, gi, torch.stack([v.sum(1), (v * v).sum(1)]))
    return out.permute(1, 2, 0).contiguous()


@pytest.mark.parametrize("hw,force,combine,expect", ST_PLANS,
                         ids=[f"hw{p[0]}-{ec._gkind(p[1])}-s{p[3][3]}" + (f"-{p[2]}" if p[2] else "") for p in ST_PLANS])
def test_grouped_groupnorm_statistics_exact(hw, force, combine, expect):
    i = ST_PLANS.index((hw, force, combine, expect))
    gc = ec.GroupCase(f"gstat-hw{hw}-{ec._gkind(force)}", ST_SRC[hw], 200, ST_PAIRS[i % 3], force, expect, combine)
    B = 2
    accs, extra = [], []
    for lane in range(2):
        f = {}
        per = []
        for k, (cg, G, c_off) in enumerate(ST_TGT[lane]):
            rs = 2 * B * G + 16 * (lane + k)  # replica strides of their own
            acc = torch.zeros(STAT_REPL, rs, dtype=torch.float64, device=DEV)
            per.append((acc, rs))
            pre = "st_" if k == 0 else "st2_"
            f.update({pre + "acc": acc.data_ptr(), pre + "rs": rs, pre + "cg": cg, pre + "G": G, pre + "coff": c_off})
        f["st_hw"] = hw
        accs.append(per)
        extra.append(f)
    d_ops, outs, got = run_pair(gc, extra, lambda: [acc.zero_() for per in accs for acc, _ in per])
    assert int(ec.operands(gc.lane(0)).value().abs().max()) <= 256
    for lane in range(2):
        o = d_ops[lane].o
        assert (o.B, o.hw) == (B, hw)
        for k, tgt in enumerate(ST_TGT[lane]):
            acc, rs = accs[lane][k]
            G = tgt[1]
            have = acc.sum(0)
            want = torch.zeros(rs, dtype=torch.float64, device=DEV)
            want[:2 * B * G] = _group_sums(d_ops[lane].want, B, hw, tgt).flatten()
            bad = have != want
            if bool(bad.any()):
                j = int(bad.nonzero()[0])
                foreign = _group_sums(d_ops[1 - lane].want, B, hw, tgt).flatten()
                raise AssertionError(
                    f"{gc.name} plan {expect} lane {lane} target {k} (cg {tgt[0]}, c_off {tgt[2]}): {int(bad.sum())} of "
                    f"{rs} accumulator entries differ from the exact sums; first entry {j} = (b {j // (2 * G)}, group "
                    f"{j % (2 * G) // 2}, {'sum' if j % 2 == 0 else 'sum of squares'}): got {have[j].item()!r}, want "
                    f"{want[j].item()!r} (the other lane's values would give "
                    f"{foreign[j].item() if j < foreign.numel() else 0.0!r})")


# ---- LayerNorm row statistics (rst), two lanes --------------------------------------------------------------------------
RST_PLANS = [
    (ec.dense(130, 320), 200, ("b", "br"), (64, 64, 1, ec.T3), None),
    (ec.dense(257, 256, 64), 70, ("lo", "br"), (64, 128, 1, ec.T3), None),
    (ec.dense(130, 320), 200, ("br", "b"), (128, 128, 1, ec.T3), None),
    (ec.dense(257, 320), 200, ("ber", "b"), (64, 64, 3, ec.T3), "coop"),
    (ec.dense(63, 192), 70, ("b", "ber"), (64, 64, 1, 2), None),
]


@pytest.mark.parametrize("src,N,pair,force,combine", RST_PLANS,
                         ids=[f"{ec._gkind(p[3])}-{ec.src_name(p[0])}-n{p[1]}-s{p[3][2]}-{p[2][0]}+{p[2][1]}" for p in RST_PLANS])
def test_grouped_row_statistics_exact(src, N, pair, force, combine):
    gc = ec.GroupCase("grst-" + ec._gkind(force), src, N, pair, force, ec.expect_forced(src, force), combine)
    M = ec.src_shape(src)[2]
    rst = [torch.zeros(M + 16, 2, dtype=torch.float64, device=DEV) for _ in range(2)]  # 8 guard rows either side
    d_ops, outs, got = run_pair(gc, [dict(rst=r[8:].data_ptr()) for r in rst], lambda: [r.zero_() for r in rst])
    for lane in range(2):
        v = d_ops[lane].want
        want = torch.zeros_like(rst[lane])
        want[8:8 + M] = torch.stack([v.sum(1), (v * v).sum(1)], -1)
        bad = (rst[lane] != want).any(1)
        if bool(bad.any()):
            m = int(bad.nonzero()[0]) - 8
            raise AssertionError(f"{gc.name} lane {lane}: {int(bad.sum())} rows of the row statistics differ from the "
                                 f"exact sums; first row {m}: got {rst[lane][m + 8].tolist()}, want {want[m + 8].tolist()}")


# ---- no exact answer: both lanes bitwise equal to the lane launched alone ------------------------------------------------
def _alone_and_grouped(descs, outs):
    """descs: two GemmDesc (same forced plan); outs: their output tensors.  Launches each alone, then both as one
    group; returns ([alone0, alone1], [grouped0, grouped1]) clones."""
    L, lib = _L()
    alone = []
    for d, o in zip(descs, outs):
        o.fill_(SENTINEL)
        assert L.tair_k_gemm(ctypes.byref(d), _stream()) == 0, L.tair_last_error()
        torch.cuda.synchronize()
        alone.append(o.clone())
    arr = (lib.GemmDesc * 2)()
    for i, d in enumerate(descs):
        ctypes.memmove(ctypes.byref(arr[i]), ctypes.byref(d), ctypes.sizeof(lib.GemmDesc))
        outs[i].fill_(SENTINEL)
    assert L.tair_k_gemm_grouped(arr, 2, _stream()) == 0, L.tair_last_error()
    torch.cuda.synchronize()
    cnt = ctypes.c_int(-1)
    assert L.tair_fault_count(1, ctypes.byref(cnt)) == 0 and cnt.value == 0
    return alone, [o.clone() for o in outs]


def _assert_same(name, alone, grouped, M, N):
    for lane in range(2):
        a, g = alone[lane].view(torch.int16), grouped[lane].view(torch.int16)
        assert bool((alone[lane][:M, :N] != SENTINEL).any()), "nothing written"
        if not torch.equal(a, g):
            bad = a != g
            m, n = bad.nonzero()[0].tolist()
            raise AssertionError(f"{name} lane {lane}: {int(bad.sum())} elements differ from the lane launched alone; first "
                                 f"({m}, {n}): grouped {grouped[lane][m, n].item()!r}, alone {alone[lane][m, n].item()!r}")
        assert not torch.equal(alone[0][:M, :N], alone[1][:M, :N])


@pytest.mark.parametrize("M,N,force", [(130, 200, (64, 64, 1, 3)), (257, 320, (128, 320, 1, 3)), (63, 72, (64, 128, 1, 2))],
                         ids=lambda v: str(v).replace(" ", ""))
def test_grouped_folded_layernorm_consumers_equal_alone(M, N, force):
    from test_lnfold_gpu import _fold_operands
    C = 320
    keep, descs, outs = [], [], []
    for lane in range(2):
        x, wf, cs, bias, lnst = _fold_operands(M, C, N, seed=11 + lane + M)
        out = torch.full((M + 16, N + 32), SENTINEL, dtype=torch.bfloat16, device=DEV)
        keep.append((x, wf, cs, bias, lnst))
        outs.append(out)
        descs.append(ec.make_desc(M=M, N=N, K=C, amode=0, A=x.data_ptr(), lda=C, Wt=wf.data_ptr(), ldw=C,
                                  bias=bias.data_ptr(), out=out.data_ptr(), ldo=N + 32, lnst=lnst.data_ptr(),
                                  lncs=cs.data_ptr(), ln_c=float(C), ln_eps=1e-5, **ec.force_fields(force)))
    alone, grouped = _alone_and_grouped(descs, outs)
    _assert_same(f"lnfold {M}x{N} {force}", alone, grouped, M, N)
    for g in grouped:
        assert bool((g[M:] == SENTINEL).all()) and bool((g[:, N:] == SENTINEL).all())


@pytest.mark.parametrize("force", [(256, 160, 1, 9), (256, 128, 2, 9), (256, 128, 1, 3)], ids=lambda v: str(v).replace(" ", ""))
def test_grouped_groupnorm_on_load_equals_alone(force):
    """GroupNorm(+SiLU) on load with two lanes (own statistics, gamma, beta and input per lane): the 256 x 160 halo
    tiles take the 2-stage weight ring per lane while the LDS is sized from lane 0; a split halo plan; a tile plan."""
    from test_kernels_gpu import _gn_stats, pack_conv_w
    B, W, Cin, Cout, G = 2, 16, 128, 200, 8
    HW, M = W * W, 2 * W * W
    keep, descs, outs = [], [], []
    for lane in range(2):
        g = torch.Generator(device=DEV).manual_seed(100 + lane)
        x = (torch.randn(M, Cin, device=DEV, generator=g) * (1.5 - lane) + 0.7 - lane).to(torch.bfloat16)
        st, rs = _gn_stats(x, B, HW, Cin, G)
        gamma = torch.rand(Cin, device=DEV, generator=g) + 0.5
        beta = torch.randn(Cin, device=DEV, generator=g) * 0.3
        w = (torch.randn(Cout, Cin, 3, 3, device=DEV, generator=g) / (9 * Cin) ** 0.5).to(torch.bfloat16)
        wp, ldw = pack_conv_w(w)
        bias = torch.randn(Cout, device=DEV, generator=g)
        part = torch.full((4 * M * Cout,), NAN, dtype=torch.float32, device=DEV)
        out = torch.full((M + 16, Cout + 32), SENTINEL, dtype=torch.bfloat16, device=DEV)
        keep.append((x, st, gamma, beta, wp, bias, part))
        outs.append(out)
        descs.append(ec.make_desc(M=M, N=Cout, K=9 * Cin, amode=1, A=x.data_ptr(), lda=Cin, C=Cin, Bn=B, H=W, W=W, Ho=W,
                                  Wo=W, rows_per_b=HW, Wt=wp.data_ptr(), ldw=ldw, bias=bias.data_ptr(),
                                  out=out.data_ptr(), ldo=Cout + 32, partial=part.data_ptr(), partial_cap=part.numel(),
                                  gn_st=st.data_ptr(), gn_rs=rs, gn_G=G, gn_eps=1e-5, gn_gamma=gamma.data_ptr(),
                                  gn_beta=beta.data_ptr(), gn_silu=1, **ec.force_fields(force)))
    rc, plan = ec.plan_of_lanes(descs[0], 2)
    assert rc == 0 and plan == ec.expect_forced(ec.conv(ec.A_CONV3, B, W, W, Cin), force), (rc, plan)
    alone, grouped = _alone_and_grouped(descs, outs)
    _assert_same(f"gn_st {force}", alone, grouped, M, Cout)
    for gch in grouped:
        assert bool((gch[M:] == SENTINEL).all()) and bool((gch[:, Cout:] == SENTINEL).all())
