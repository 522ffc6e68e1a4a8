"""The exact-answer case tables (tests/_exact_cases.py) without a device.  Per GEMM / conv case: the operands keep the
exactness bound (sum_k |a||w| + |bias| + |emb| + |res| <= 256, half-integers below 128), the int64 reference equals
the fp64 reference of the same operands and survives the bf16 rounding unchanged, the weights of every 64-column
output block cover every K position, and tair_k_gemm_plan (host only) resolves the request to the (kernel, bm, bn,
splits) the case names.  The forced plans that the library must refuse are listed as refusals with their message:
the GPU module runs every other case and skips none.  Per attention case: the library's effective plan is the one the
case claims, the target sets hold the positions that plan makes critical, and an fp64 softmax of the scores puts
weight exactly 1.0f on the target.

The number of tests here is the GPU modules' parameter count plus the refusals (test_counts_add_up)."""
import math

import pytest
import torch

import _exact_cases as ec


def _L():
    from tair_amd import _lib
    return _lib.lib(), _lib


@pytest.mark.parametrize("case", ec.CASES, ids=repr)
def test_gemm_case(case):
    L, _ = _L()
    o = ec.operands(case)
    # -- the operand rule
    for t in (o.a, o.w_main, o.w_x, o.x):
        if t is not None and t.numel():
            assert int(t.abs().max()) <= 1
    per_pixel = (o.a != 0).reshape(-1, o.a.shape[-1]).sum(1)
    nnz = (ec.F8_A_NNZ if o.f8 else ec.A_NNZ) if case.is_conv else (ec.F8_A_NNZ_DENSE if o.f8 else ec.A_NNZ_DENSE)
    assert bool((per_pixel == min(nnz, o.a.shape[-1])).all())
    for t in (o.bias, o.emb, o.res):
        if t is not None:
            assert int(t.abs().max()) <= ec.SMALL
    w = torch.cat([o.w_main, o.w_x], 1)
    ktot = w.shape[1]
    assert ktot == o.Kreal + o.Kx
    row_nnz = (w != 0).sum(1)
    assert all(int(row_nnz[n]) <= ec.weight_cap(o.N, ktot, n) for n in range(o.N))
    # -- the exactness bound, and the value's representability
    mag = o.magnitude()
    assert int(mag.max()) <= 256, int(mag.max())
    ref2 = o.ref2()
    assert bool((ref2.abs() <= 2 * mag).all())
    if o.half:
        assert int(ref2.abs().max()) < 256  # half-integers below 128
    else:
        assert bool((ref2 % 2 == 0).all())
    v = o.value()
    assert torch.equal(v.to(torch.bfloat16).double(), v) and torch.equal(v.float().double(), v)
    # -- int64 against fp64 of the same operands (the conv through torch's own convolution)
    wd = o.w_main.double()
    if not case.is_conv:
        y = o.a.double() @ wd.t()
    else:
        w4 = wd.view(o.N, 3, 3, o.C).permute(0, 3, 1, 2)
        x = o.a.double().permute(0, 3, 1, 2)
        if o.amode == ec.A_CONV3_UP:
            y = torch.nn.functional.conv2d(torch.nn.functional.interpolate(x, scale_factor=2, mode="nearest"), w4, padding=1)
        elif o.amode == ec.A_CONV3_S2 and o.s2_shift:
            y = torch.nn.functional.conv2d(torch.nn.functional.pad(x, (0, 1, 0, 1)), w4, stride=2)
        elif o.amode == ec.A_CONV3_S2:
            y = torch.nn.functional.conv2d(x, w4, stride=2, padding=1)
        else:
            y = torch.nn.functional.conv2d(x, w4, padding=1)
        y = y.permute(0, 2, 3, 1).reshape(o.M, o.N)
    if o.Kx:
        xe = torch.cat([o.x, o.x], 1) if o.x_wrap else o.x
        y = y + xe.double() @ o.w_x.double().t()
    y = (0.5 if o.half else 1.0) * (y * o.scale().double() + o.bias.double())
    if o.emb is not None:
        y = y + o.emb[o.emb_row.long()].double()[torch.arange(o.M) // o.hw]
    if o.res is not None:
        y = y + o.res.double()
    assert torch.equal(y, v)
    # -- K coverage: the rows of every 64-column output block together hold every K position
    for n0 in range(0, o.N, 64):
        assert bool((w[n0:n0 + 64] != 0).any(0).all()), n0
    # ... also after packing into the kernel's K order (pack_conv_w): the packed columns are a permutation of them
    pw = o.packed_w()
    kv = o.Kd * (2 if o.f8 else 1)
    assert pw.shape[1] == kv + o.Kx and int((pw != 0).sum()) == int((w != 0).sum())
    assert int((pw != 0).any(0).sum()) == ktot  # the padding columns (small-channel mode, fp8 K-tiles) stay zero
    # -- the plan
    rc, plan = ec.plan_of(ec.planning_desc(case))
    assert rc == 0, L.tair_last_error()
    assert plan == case.expect, (plan, case.expect)


@pytest.mark.parametrize("case", ec.REFUSALS, ids=repr)
def test_gemm_refusal(case):
    L, _ = _L()
    rc, plan = ec.plan_of(ec.planning_desc(case))
    msg = (L.tair_last_error() or b"").decode()
    assert rc != 0 and case.refusal in msg, (rc, plan, msg)


@pytest.mark.parametrize("case,accepting", ec.AGREE, ids=[repr(c) for c, _ in ec.AGREE])
def test_agree_plans(case, accepting):
    """The all-plans-agree descriptors: how many of ALL_PLANS the library accepts for each, and that the accepted ones
    span every kernel."""
    kerns, n = set(), 0
    for force in ec.ALL_PLANS:
        c = ec.Case(case.name, case.src, case.N, case.epi, force, None, "reduce")
        rc, plan = ec.plan_of(ec.planning_desc(c))
        if rc == 0:
            assert plan == ec.expect_forced(case.src, force), (force, plan)
            kerns.add(plan[0])
            n += 1
    assert n == accepting, (n, accepting)
    assert kerns >= {ec.K_TILE, ec.K_PHASE, ec.K_DEEP, ec.K_KGROUP}
    assert (ec.K_SHALLOW in kerns) == (not case.is_conv)


def test_case_table_covers_what_the_issue_lists():
    cs = ec.CASES
    dense = [c for c in cs if not c.is_conv and not c.src[6]]
    assert {c.src[2] for c in dense} >= set(ec.D_M) and {c.N for c in dense} >= set(ec.D_N)
    assert {c.src[3] for c in dense} >= set(ec.D_K)
    assert {c.src[3] for c in dense if c.force and c.force[0] < 0} >= {96, 160}

    def plans(kern, sel=lambda c: True):
        return {c.expect[1:3] for c in cs if c.expect[0] == kern and sel(c)}
    for mode, name in ((lambda c: not c.is_conv, "dense"), (lambda c: c.is_conv and c.src[1] == ec.A_CONV3, "conv")):
        un = lambda c: mode(c) and c.expect[3] == 1 and not c.src[6 if not c.is_conv else 8]  # noqa: E731
        assert plans(ec.K_TILE, un) >= set(ec.TILES) | {(-bm, bn) for bm, bn in ec.RINGS}, name
        assert plans(ec.K_PHASE, un) == set(ec.PHASES), name
        assert plans(ec.K_KGROUP, un) == set(ec.KGROUPS), name
        deep = {(c.expect[2], c.force[3] - 100) for c in cs if c.expect[0] == ec.K_DEEP and un(c)}
        assert deep == set(ec.DEEPS), name
    assert plans(ec.K_SHALLOW) == set(ec.SHALLOWS)
    assert {(c.expect[2], c.force[3] - 100) for c in dense if c.expect[0] == ec.K_DEEP and c.src[3] == 64} == set(ec.DEEPS)
    assert {c.src[3] // 64 for c in dense if c.expect[0] == ec.K_KGROUP and c.expect[3] == 1} >= {1, 2, 3, 4, 5, 6}
    # split-K: the three combines on every 64-row family that takes them, the reduce kernel everywhere else; a count
    # that does not divide the K-tiles, one equal to them, one above them (lowered)
    for kern, tiles, modes in ((ec.K_TILE, [(64, 64), (64, 128)], {"coop", "last", "reduce"}),
                               (ec.K_KGROUP, ec.KGROUPS, {"coop", "last", "reduce"}),
                               (ec.K_DEEP, [(64, 64), (64, 128)], {"last", "reduce"}),
                               (ec.K_TILE, [t for t in ec.TILES if t[0] != 64] + [(-a, b) for a, b in ec.RINGS], {"reduce"})):
        for tile in tiles:
            sp = [c for c in dense if c.expect[0] == kern and c.expect[1:3] == tile and c.expect[3] > 1]
            assert {c.combine for c in sp} == modes, (kern, tile)
            units = 10 if tile[0] < 0 else 5
            assert {c.expect[3] for c in sp} == ({3, 10} if tile[0] < 0 else {2, 5}), (kern, tile)
            assert any(c.force[2] > units and c.expect[3] == units for c in sp), (kern, tile)
    conv1 = [c for c in cs if c.is_conv and c.src[1] == ec.A_CONV3 and not c.src[8] and c.expect[0] != ec.K_HALO]
    assert {c.src[2:5] for c in conv1} == set(ec.C_SHAPES)
    assert {c.src[5] for c in conv1} == set(ec.C_C) and {c.N for c in conv1} == set(ec.C_N)
    assert {(c.src[6], c.src[7]) for c in conv1} == {(0, 0), (64, 0), (128, 64)}
    assert {c.epi for c in conv1} >= {"b", "be", "br", "ber"}
    halo = [c for c in cs if c.expect[0] == ec.K_HALO]
    assert {c.src[2:5] for c in halo} == set(ec.H_SHAPES)
    assert all(c.src[3] * c.src[4] % 256 == 0 for c in halo)
    assert {(c.src[4], c.expect[2]) for c in halo} == {(w, bn) for w, bns in ec.HALO_BN.items() for bn in bns}
    assert {(c.force[2], c.expect[3]) for c in halo if c.src[5] == 192} == {(1, 1), (2, 2), (3, 3)}
    s2 = [c for c in cs if c.is_conv and c.src[1] == ec.A_CONV3_S2 and c.force]
    assert {(c.src[2:5], c.src[9]) for c in s2} == {(s, sh) for s in ec.S2_SHAPES for sh in (0, 1)}
    assert {c.src[2:5] for c in cs if c.is_conv and c.src[1] == ec.A_CONV3_UP} == set(ec.UP_SHAPES)
    sc = [c for c in cs if c.is_conv and c.src[1] == ec.A_SMALLC]
    assert {c.src[5] for c in sc} == {4, 8} and {c.N for c in sc} == {64, 72}
    assert {c.src[2:5] for c in sc} == {(1, 8, 8), (2, 8, 16), (3, 5, 7)}
    f8d = [c for c in cs if not c.is_conv and c.src[6] and c.force]
    assert {c.src[2] for c in f8d} == {65, 257} and {c.N for c in f8d} == {70, 200}
    assert all(c.src[3] % 128 == 0 for c in f8d) and {c.expect[1:3] for c in f8d} == set(ec.F8_TILES)
    f8c = [c for c in cs if c.is_conv and c.src[8]]
    assert {c.src[2:5] for c in f8c} == {(2, 8, 16), (3, 5, 7)} and {c.src[5] for c in f8c} == {64, 128}
    assert {bool(c.src[6]) for c in f8c} == {False, True}
    assert {c.epi for c in cs} == set(ec.EPI)
    assert sum(c.force is None for c in cs) >= 4


@pytest.mark.parametrize("case", ec.ATTN_CASES, ids=repr)
def test_attention_case(case):
    rc, plan = ec.attn_plan_of(case)
    assert rc == 0 and plan == case.expect, (rc, plan, case.expect)
    qsets, splits, kv_split = plan
    assert kv_split % ec.KT == 0 and (splits - 1) * kv_split < case.Skv <= splits * kv_split  # no empty split
    o = ec.AttnOps(case)
    req = ec.required_targets(case.Skv, splits, kv_split)
    assert {0, case.Skv - 1} <= set(req)
    assert all(k in req for k in (63, 64) if k < case.Skv)
    for T in o.sets.values():
        assert len(T) <= 64 and set(req) <= set(T) and len(set(T)) == len(T)
    for t in (o.q, o.k, o.v):
        assert torch.equal(t.to(torch.bfloat16).float(), t)
    # every target is selected by some query of some (batch, head) when there are queries enough; always: key 0 or
    # Skv - 1 and whatever the cycle reaches
    assert bool((o.tgt >= 0).all()) and bool((o.tgt < case.Skv).all())
    # an fp64 softmax of the scores (scale 0.125): weight exactly 1.0f on the target, 0.0f elsewhere
    B, Sq, H = o.q.shape[:3]
    for b in range(B):
        kb = b if o.Bk > 1 else 0
        s = torch.einsum("qhd,khd->hqk", o.q[b].double(), o.k[kb].double()) * 0.125
        assert bool((s.gather(2, o.tgt[b][:, :, None]) == 256).all())
        p = torch.softmax(s, -1).float()
        want = torch.zeros_like(p).scatter_(2, o.tgt[b][:, :, None], 1.0)
        assert torch.equal(p, want)
    assert math.exp(-256) < 2.0 ** -149  # below the smallest fp32 denormal


def test_attention_table_covers_what_the_issue_lists():
    cs = ec.ATTN_CASES
    assert {(c.Sq, c.Skv) for c in cs} >= {(q, k) for q in ec.A_SQ for k in ec.A_SKV}
    assert {c.B for c in cs} >= {1, 3} and {c.H for c in cs} >= {1, 2, 5}
    assert {c.api for c in cs} == {"plain", "ex", "tk"}
    assert {(c.api, c.force[0]) for c in cs} >= {("ex", 1), ("ex", 2), ("tk", 1), ("tk", 2)}
    assert {c.layout for c in cs} == {"rows", "shared", "fused"}
    forced = [c for c in cs if c.api != "plain"]
    assert {c.force[1] for c in forced} >= {1, 2}
    tiles = lambda c: ec.cdiv(c.Skv, ec.KT)  # noqa: E731
    # a last split of one partial tile; a count above the key tiles; a workspace that lowers the forced count
    assert any(c.expect[1] > 1 and c.Skv % ec.KT and c.Skv - (c.expect[1] - 1) * c.expect[2] < ec.KT for c in forced)
    assert any(c.force[1] > tiles(c) > 1 and c.expect[1] == tiles(c) for c in forced)
    assert any(1 < c.expect[1] < min(c.force[1], tiles(c)) for c in forced)
    assert any(c.expect[1] == 1 and min(c.force[1], tiles(c)) > 1 for c in forced)


def test_counts_add_up():
    """This module's per-case tests = the GPU modules' parameters + the refusals; nothing is skipped on the GPU."""
    import test_attention_exact_gpu as ta
    import test_gemm_exact_gpu as tg
    assert tg.GEMM_PARAMS == ec.CASES and [c for c, _ in ec.AGREE] == tg.AGREE_PARAMS
    assert ta.ATTN_PARAMS == ec.ATTN_CASES
    n_cpu = len(ec.CASES) + len(ec.REFUSALS) + len(ec.AGREE) + len(ec.ATTN_CASES)
    n_gpu = len(tg.GEMM_PARAMS) + len(tg.AGREE_PARAMS) + len(ta.ATTN_PARAMS)
    assert n_cpu == n_gpu + len(ec.REFUSALS)
