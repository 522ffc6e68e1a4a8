"""The two-lane case tables (tests/_exact_cases.py GROUP_CASES, GROUP_ATTN_CASES) and gemm_grouped's refusals, without
a device.

Per pair: both lanes keep the exactness bound; the two expected outputs differ in at least half of their elements, so
a swapped or duplicated lane cannot pass; for every per-lane operand in turn (activation, weights, K-extension, bias,
time-embedding table and row index, residual, fp8 scales) the reference with that ONE operand taken from the other
lane differs from the true one, so any single mixed-up pointer is visible; tair_k_gemm_plan_lanes resolves the pair
to the plan it names (and, for the planner's own plans, one lane to the other plan the case states); the dry
tair_k_gemm_grouped_check accepts the pair.  The coverage the table promises is asserted from the table.

Refusals go through tair_k_gemm_grouped_check alone, which launches nothing: lanes that differ in shape, mode,
activation, output kind, operand type or in the LayerNorm / GroupNorm-on-load roles, and every per-descriptor rule
broken in ONE lane -- lane 1 only and lane 0 only.  Before this module the per-descriptor rules (a split output's
ldo >= 3N and plain epilogue, a two-plane output's plain bf16 epilogue, x_wrap's Kx = 2 x_wrap, the LayerNorm roles'
own conditions) read lane 0 alone: a lane 1 that broke one was launched.  out_split must now be the same in both
lanes (the split planes change the output's width: it belongs to the output kind, like out_f32); out_lo may differ
and the lo | br pairs cover that.
"""
import ctypes

import pytest
import torch

import _exact_cases as ec


def _L():
    from tair_amd import _lib
    return _lib.lib(), _lib


def _err():
    return (_L()[0].tair_last_error() or b"").decode()


@pytest.mark.parametrize("gc", ec.GROUP_CASES, ids=repr)
def test_group_case(gc):
    L, _ = _L()
    o = [ec.operands(gc.lane(i)) for i in range(2)]
    assert o[0] is not o[1] and (o[0].lane, o[1].lane) == (0, 1)
    # -- what the launcher makes the lanes share
    f = [x.fields() for x in o]
    for k in ("M", "N", "K", "Kx", "amode", "out_f32", "out_split", "f8"):
        assert f[0][k] == f[1][k], k
    # -- the exactness bound and the value's representability, per lane
    for x in o:
        assert int(x.magnitude().max()) <= 256
        v = x.value()
        assert torch.equal(v.to(torch.bfloat16).double(), v)
        if x.half:
            assert int(x.ref2().abs().max()) < 256
    # -- the lanes' answers differ in at least half of their elements
    r = [x.ref2() for x in o]
    differ = int((r[0] != r[1]).sum())
    assert 2 * differ >= r[0].numel(), (differ, r[0].numel())
    # -- any ONE operand taken from the other lane shows
    seen = set()
    for i in range(2):
        for what in ec.SWAPS:
            m = ec.swapped_ref2(o[i], o[1 - i], what)
            if m is None:
                continue
            if what == "emb_row" and o[i].B == 1:
                continue  # (one batch element has one row to read: both lanes index row 1)
            assert not torch.equal(m, r[i]), (i, what)
            seen.add(what)
    assert {"a", "w"} <= seen and (not o[0].has_bias or "bias" in seen)
    # -- the plan of two lanes, and of one where the case says it differs
    rc, plan = ec.plan_of_lanes(ec.planning_desc(gc.lane(0)), 2)
    assert rc == 0, _err()
    assert plan == gc.expect, (plan, gc.expect)
    if gc.expect_one is not None:
        rc, plan1 = ec.plan_of_lanes(ec.planning_desc(gc.lane(0)), 1)
        assert rc == 0 and plan1 == gc.expect_one and plan1 != plan, (plan1, gc.expect_one)
        assert (rc, plan1) == ec.plan_of(ec.planning_desc(gc.lane(0)))
    elif gc.force is not None:
        assert plan == ec.expect_forced(gc.src, gc.force)
    # -- the dry check takes the pair as it is launched, either way round
    arr = ec.pair_descs(gc)
    assert L.tair_k_gemm_grouped_check(arr, 2) == 0, _err()
    assert L.tair_k_gemm_grouped_check(arr, 1) == 0, _err()


def test_lane_salt_keeps_lane_zero():
    """Salt 0 draws what Ops has always drawn (the seed is the crc of the unsalted key); salt 1 differs everywhere."""
    import zlib
    src, N, epi = ec.dense(130, 320, 64), 200, "ber"
    a, b = ec.Ops(src, N, epi), ec.Ops(src, N, epi, lane=1)
    gen = torch.Generator().manual_seed(zlib.crc32(repr((src, N, epi)).encode()))
    assert torch.equal(a.a, ec._sparse_rows(130, 320, ec.A_NNZ_DENSE, gen))
    assert torch.equal(a.emb_row, torch.tensor([3, 2, 1], dtype=torch.int32))
    assert torch.equal(b.emb_row, torch.tensor([1, 2, 3], dtype=torch.int32))
    for t in ("a", "w_main", "w_x", "x", "bias", "emb", "res"):
        assert not torch.equal(getattr(a, t), getattr(b, t)), t
    c = ec.CASE["own-dense-m257n200k320x64-lo"]
    assert c.lane == 0 and ec.operands(c).lane == 0


def test_group_table_covers_what_the_issue_lists():
    cs = ec.GROUP_CASES
    un = lambda c: c.expect[3] == 1  # noqa: E731
    sp = lambda c: c.expect[3] > 1  # noqa: E731
    bf = lambda c: not c.src[6 if not c.is_conv else 8]  # noqa: E731

    def plans(kern, sel):
        return {c.expect[1:3] for c in cs if c.expect[0] == kern and bf(c) and c.force and sel(c)}
    # families, unsplit and split
    tiles = {(64, 64), (64, 128), (128, 128), (128, 320), (256, 128), (256, 160)}
    rings = {(-64, 64), (-128, 256), (-256, 128)}
    for sel in (un, sp):
        assert plans(ec.K_TILE, sel) >= tiles | rings
        assert {c.force[3] - 100 for c in cs if c.expect[0] == ec.K_DEEP and sel(c)} >= {4, 8}
        assert plans(ec.K_DEEP, sel) == {(64, 64)}
        assert plans(ec.K_KGROUP, sel) == {(64, 64), (64, 128)}
        assert all(c.force[3] == 203 for c in cs if c.expect[0] == ec.K_KGROUP and c.force)
        assert {c.src[4] for c in cs if c.expect[0] == ec.K_HALO and sel(c)} == {16, 32, 64}
        f8 = [c for c in cs if not bf(c) and sel(c)]
        assert {c.is_conv for c in f8} == {False, True}
    assert plans(ec.K_PHASE, un) == {(256, 256), (256, 320)} and plans(ec.K_SHALLOW, un) == {(64, 64), (64, 128)}
    assert not plans(ec.K_PHASE, sp) and not plans(ec.K_SHALLOW, sp)  # (they never split)
    # mixed pairs, both ways round
    pairs = {c.epis for c in cs}
    for a, b in (("b", "ber"), ("br", "b"), ("lo", "br"), ("half", "b")):
        assert (a, b) in pairs and (b, a) in pairs, (a, b)
    assert {e for c in cs for e in c.epis} == set(ec.EPI)
    # the lane boundary: tiles_m 1 / 3 / 5 (64 rows) with N = 70 and 200, workgroup counts on both sides of % 8
    dense = [c for c in cs if not c.is_conv and bf(c)]
    for sel in (un, sp):
        b64 = [c for c in dense if c.expect[:3] == (ec.K_TILE, 64, 64) and sel(c)]
        assert {(c.src[2], c.N) for c in b64} >= {(m, n) for m in ec.G_M for n in ec.G_N}
        assert {ec.cdiv(c.src[2], 64) for c in b64} >= {1, 3, 5}
    assert {(ec.cdiv(c.src[2], 128), ec.cdiv(c.src[2], 256)) for c in dense} >= {(1, 1), (2, 1), (3, 2)}
    wg = {c.workgroups() % 8 == 0 for c in cs if "boundary" in c.tags}
    assert wg == {True, False}
    assert any(c.workgroups() % 8 for c in cs if sp(c)) and any(c.workgroups() % 8 == 0 for c in cs if sp(c))
    # conv sources
    c1 = [c for c in cs if c.is_conv and c.src[1] == ec.A_CONV3 and bf(c) and c.expect[0] != ec.K_HALO]
    assert {c.src[2:5] for c in c1} >= {(3, 5, 7), (2, 8, 16), (1, 30, 24)} and {c.src[5] for c in c1} == {64, 192}
    assert {(c.src[6], c.src[7]) for c in c1} == {(0, 0), (64, 0), (128, 64)}
    s2 = [c for c in cs if c.is_conv and c.src[1] == ec.A_CONV3_S2]
    assert {c.src[9] for c in s2} == {0, 1} and {un(c) for c in s2} == {True, False}
    up = [c for c in cs if c.is_conv and c.src[1] == ec.A_CONV3_UP]
    assert {c.src[2:5] for c in up} == {(2, 4, 8)} and {un(c) for c in up} == {True, False}
    assert {un(c) for c in cs if c.is_conv and c.src[1] == ec.A_SMALLC} == {True, False}
    halo = [c for c in cs if c.expect[0] == ec.K_HALO]
    assert {c.src[2:5] for c in halo} >= {(1, 16, 16), (2, 32, 16), (1, 64, 64)}
    assert {(c.src[4], c.expect[2]) for c in halo} == {(16, 128), (16, 160), (32, 192), (64, 64)}
    # every combine: reduce, last and coop at 2, 3 and 5 slices on both dense sources and on a conv
    for src in (ec.SPLIT_SRC, ec.SPLIT_SRC_X, ec.CS_SRC):
        got = {(c.expect[3], c.combine) for c in cs if c.src == src and c.expect[1] == 64 and c.expect[0] == ec.K_TILE}
        assert got >= {(s, m) for s in (2, 3, 5) for m in ("coop", "last", "reduce")}, src
    assert {c.combine for c in cs if c.expect[0] == ec.K_KGROUP and sp(c)} == {"coop", "last", "reduce"}
    assert {c.combine for c in cs if c.expect[0] == ec.K_DEEP and sp(c)} == {"last", "reduce"}
    assert all(c.combine == "reduce" for c in cs if sp(c) and abs(c.expect[1]) != 64)
    # the planner's own two-lane plans differ from one lane's; one blocked-order case
    own = [c for c in cs if c.force is None]
    assert len(own) >= 2 and all(c.expect_one and c.expect_one != c.expect for c in own)
    assert {c.expect[0] for c in own} == {ec.K_TILE, ec.K_KGROUP}
    blocked = [c for c in cs if "blocked" in c.tags]
    assert len(blocked) == 1


def test_blocked_case_meets_the_host_rule():
    """The blocked-order case: the rule picks a block for two lanes and none for one; nothing smaller does at its M."""
    M, N, K = ec.BLOCKED
    gc = [c for c in ec.GROUP_CASES if "blocked" in c.tags][0]
    assert gc.src == ec.dense(M, K) and gc.N == N and gc.expect == (ec.K_TILE, 64, 64, 1) and N % 64 == 6
    assert ec.blocked_pick(M, N, K, 64, 64, 2) == (2, 11) and ec.blocked_pick(M, N, K, 64, 64, 1) == (0, 0)
    gx, gy = 2 * ec.cdiv(M, 64), ec.cdiv(N, 64)
    assert gx * gy > 512 and gy * 64 * K * 2 > (2 << 20)
    assert gx % 2 == 0 and ec.cdiv(M, 64) % 2 == 1  # a block row of 2 m-tiles holds tiles of both lanes
    # no smaller weight matrix with more than one K-tile: K in 128 .. 192 x every narrower grid
    for k in (128, 192):
        for g in range(1, gy + 400 if k == 128 else gy):
            if g * 64 * k < gy * 64 * K:
                assert ec.blocked_pick(M, 64 * g - 58, k, 64, 64, 2) == (0, 0), (k, g)


@pytest.mark.parametrize("case", ec.GROUP_ATTN_CASES, ids=repr)
def test_group_attention_case(case):
    rc = ctypes.c_int()
    out = [ctypes.c_int() for _ in range(3)]
    L, _ = _L()
    rc = L.tair_k_attention_plan_ex(case.B, case.H, case.Sq, case.Skv, case.ws_bytes, case.force[0], case.force[1],
                                    *[ctypes.byref(x) for x in out])
    plan = tuple(x.value for x in out)
    assert rc == 0 and plan == case.expect, (plan, case.expect)
    assert (plan[1] > 1) == (case.api != "unsplit")
    o = [ec.AttnOps(case, lane=i) for i in range(2)]
    req = ec.required_targets(case.Skv, plan[1], plan[2])
    for x in o:
        for T in x.sets.values():
            assert set(req) <= set(T) and len(T) <= 64
    # the lanes differ in V and in what the queries select; the expected outputs in most rows
    assert not torch.equal(o[0].v, o[1].v) and not torch.equal(o[0].q, o[1].q)
    e = [x.expected() for x in o]
    rows = (e[0] != e[1]).any(-1)
    assert 2 * int(rows.sum()) >= rows.numel()
    # lane 0's V read with lane 1's selection (a mixed-up q / k pointer), and the reverse, are both wrong
    B, Sq, H = o[0].q.shape[:3]
    for i in range(2):
        mixed = torch.zeros_like(e[i])
        for b in range(B):
            for h in range(H):
                mixed[b, :, h] = o[i].v[b if o[i].Bk > 1 else 0, o[1 - i].tgt[b, h], h]
        assert not torch.equal(mixed, e[i])


def test_group_attention_table_covers_what_the_issue_lists():
    cs = ec.GROUP_ATTN_CASES
    for mode in ("unsplit", "split", "tk"):
        sel = [c for c in cs if c.api == mode]
        assert {(c.Sq, c.Skv) for c in sel} == {(q, k) for q in ec.G_ATTN_SQ for k in ec.G_ATTN_SKV}
        assert {c.B * c.H for c in sel} == {2, 3, 4}
        assert {c.layout for c in sel} == {"rows", "shared"}
        assert {c.expect[0] for c in sel} == {1, 2}
    assert {c.expect[1] for c in cs} >= {1, 2, 3, 5}


# ---- refusals: tair_k_gemm_grouped_check, nothing is launched -----------------------------------------------------------
def _pair(src, N, epis, force):
    gc = ec.GroupCase("refusal", src, N, epis, force, (0, 0, 0, 0), "reduce")
    return ec.pair_descs(gc)


BASE = (ec.dense(130, 320, 64), 200, ("b", "b"), (64, 64, 1, ec.T3))
SHARE = "must share"
DIFFER = [
    ("M", dict(M=131), SHARE), ("N", dict(N=208), SHARE), ("K", dict(K=256), SHARE), ("Kx", dict(Kx=0), SHARE),
    ("mode", dict(amode=ec.A_CONV3), SHARE), ("act", dict(act=1), SHARE), ("out_f32", dict(out_f32=1), SHARE),
    ("operand-type", dict(f8=1, col_scale=64), "operand type|fp8 operands"),
    ("rst-role", dict(rst=64), "LayerNorm roles"),
    ("gn_st-role", dict(gn_st=64, gn_gamma=64, gn_beta=64, gn_G=32, gn_rs=64), "GroupNorm-on-load role"),
]


def _check(arr, n=2):
    rc = _L()[0].tair_k_gemm_grouped_check(arr, n)
    return rc, _err()


@pytest.mark.parametrize("name,change,msg", DIFFER, ids=[d[0] for d in DIFFER])
@pytest.mark.parametrize("lane", (1, 0))
def test_lanes_that_differ_are_refused(name, change, msg, lane):
    arr = _pair(*BASE)
    assert _check(arr)[0] == 0, _err()
    for k, v in change.items():
        setattr(arr[lane], k, v)
    rc, err = _check(arr)
    assert rc == -2 and any(m in err for m in msg.split("|")), (rc, err)


@pytest.mark.parametrize("lane", (1, 0))
def test_folded_layernorm_role_must_be_shared(lane):
    src = ec.dense(130, 320)
    arr = _pair(src, 200, ("b", "b"), (64, 64, 1, ec.T3))
    assert _check(arr)[0] == 0, _err()
    for k, v in dict(lnst=64, lncs=64, ln_c=320.0, ln_eps=1e-5).items():
        setattr(arr[lane], k, v)
    rc, err = _check(arr)
    assert rc == -2 and "LayerNorm roles" in err, (rc, err)
    for k, v in dict(lnst=64, lncs=64, ln_c=320.0, ln_eps=1e-5).items():  # both lanes: a well-formed consumer pair
        setattr(arr[1 - lane], k, v)
    assert _check(arr)[0] == 0, _err()
    arr[lane].lncs = None  # ... and the folded LayerNorm's own rule, in one lane
    rc, err = _check(arr)
    assert rc == -2 and "folded LayerNorm" in err, (rc, err)


def _rule_cases():
    """(name, pair arguments, the change to ONE lane, message): each per-descriptor rule of gemm_grouped."""
    d, N, F = ec.dense(130, 320, 64), 200, (64, 64, 1, ec.T3)
    return [
        ("split-ldo", (d, N, ("sp1", "sp1"), F), dict(ldo=N + ec.PAD), "split output"),
        ("split-f32", (d, N, ("f32", "f32"), F), dict(out_split=1, ldo=3 * N + ec.PAD), SHARE + "|split output"),
        ("lo-f32", (d, N, ("f32", "f32"), F), dict(out_lo=4096), "two-plane"),
        ("lo-split", (d, N, ("sp1", "sp1"), F), dict(out_lo=4096), "two-plane"),
        ("x_wrap", (d, N, ("b", "br"), F), dict(x_wrap=64), "x_wrap"),
        ("rst-f32", (ec.dense(130, 320), N, ("f32", "f32"), F), dict(rst=64), "LayerNorm row statistics|LayerNorm roles"),
        ("stat-cg", (ec.dense(256, 320), 320, ("b", "br"), (128, 320, 1, ec.T3)), dict(st_cg=4), "too narrow"),
    ]


RULES = _rule_cases()


@pytest.mark.parametrize("name,pair,change,msg", RULES, ids=[r[0] for r in RULES])
@pytest.mark.parametrize("lane", (1, 0))
def test_rule_broken_in_one_lane_is_refused(name, pair, change, msg, lane):
    """The pair is accepted; with the rule broken in lane `lane` alone it is refused, with the rule's message (or, where
    the break also makes the lanes' output kinds differ, the sharing rule's)."""
    arr = _pair(*pair)
    if name == "stat-cg":  # a statistics target per lane, with accumulators of its own: 32 groups of 10 channels
        for i in range(2):
            for k, v in dict(st_acc=64 + 4096 * i, st_rs=64, st_cg=10, st_G=32, st_coff=0, st_hw=256).items():
                setattr(arr[i], k, v)
    assert _check(arr)[0] == 0, _err()
    for k, v in change.items():
        setattr(arr[lane], k, v)
    rc, err = _check(arr)
    assert rc == -2 and any(m in err for m in msg.split("|")), (rc, err)


def test_split_planes_are_part_of_the_output_kind():
    """out_split differing between the lanes is refused (both orders of planes are fine when shared); out_lo may
    differ."""
    d, N, F = ec.dense(130, 320, 64), 200, (64, 64, 1, ec.T3)
    arr = _pair(d, N, ("sp1", "sp1"), F)
    arr[1].out_split = 2
    rc, err = _check(arr)
    assert rc == -2 and SHARE in err, (rc, err)
    arr[0].out_split = 2
    assert _check(arr)[0] == 0, _err()
    assert _check(_pair(d, N, ("lo", "br"), F))[0] == 0, _err()
    assert _check(_pair(d, N, ("br", "lo"), F))[0] == 0, _err()


@pytest.mark.parametrize("n", (0, 3, -1))
def test_group_sizes_outside_one_and_two_are_refused(n):
    arr = _pair(*BASE)
    rc, err = _check(arr, n)
    assert rc == -2 and "group of" in err, (rc, err)
    out = [ctypes.c_int() for _ in range(4)]
    assert _L()[0].tair_k_gemm_plan_lanes(arr, n, *[ctypes.byref(x) for x in out]) == -1


def test_counts_add_up():
    """One CPU test per GPU parameter: the GPU modules run every pair and skip none."""
    import test_grouped_exact_gpu as tg
    import test_grouped_kernels_gpu as tk
    assert tg.GROUP_PARAMS == ec.GROUP_CASES and tk.ATTN_PARAMS == ec.GROUP_ATTN_CASES
