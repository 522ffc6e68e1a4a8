"""The case table of the GroupNorm-statistics tests (tests/_gn_stat_cases.py) without a device: every case resolves,
through tair_k_gemm_plan, to the kernel, tile and split count it names; the statistics targets the launcher refuses;
the descriptor mirror; and the fp64 reference helpers against brute-force loops on a tiny case."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

import _gn_stat_cases as gc


def _L():
    from tair_amd import _lib
    return _lib.lib(), _lib


@pytest.mark.parametrize("case", gc.CASES + list(gc.chain_cases(960)) + list(gc.chain_cases(1920)), ids=repr)
def test_case_resolves_to_its_plan(case):
    L, _ = _L()
    rc, plan = gc.plan_of(gc.planning_desc(case))
    assert rc == 0, L.tair_last_error()
    assert plan == case.expect, (plan, case.expect)


def test_case_table_covers_what_it_claims():
    kerns = {c.expect[0] for c in gc.CASES}
    assert kerns == {0, 1, 2, 3, 4, 5}
    tiles0 = {c.expect[1:3] for c in gc.CASES if c.expect[0] == 0 and c.expect[3] == 1}
    assert {(64, 64), (64, 128), (128, 128), (128, 256), (128, 320), (256, 128)} <= tiles0
    assert {(256, 160), (256, 256), (256, 320)} <= tiles0
    # every plan of the tile kernels, the BK = 32 rings, the 4-phase kernel, the deep ring and the two-K-group tiles
    # runs dense and as a stride-1 conv
    for kern, tiles in ((0, [(64, 64), (64, 128), (128, 128), (128, 256), (128, 320), (256, 128), (256, 160),
                             (256, 256), (256, 320), (-64, 64), (-64, 128), (-128, 128), (-128, 256), (-128, 320),
                             (-256, 128), (-256, 256)]),
                        (1, [(256, 256), (256, 320)]), (4, [(64, 64)]), (5, [(64, 64), (64, 128)])):
        for tile in tiles:
            modes = {c.src[0] if c.src[0] == "dense" else c.src[1] for c in gc.CASES
                     if c.expect[0] == kern and c.expect[1:3] == tile and c.expect[3] == 1}
            assert {"dense", gc.A_CONV3} <= modes, (kern, tile, modes)
    assert {c.expect[1:3] for c in gc.CASES if c.expect[0] == 1} == {(256, 256), (256, 320)}
    assert {c.expect[1:3] for c in gc.CASES if c.expect[0] == 2} == {(64, 64), (64, 128)}
    assert {c.expect[2] for c in gc.CASES if c.expect[0] == 3} == {64, 128, 160, 192}
    assert {c.src[1] for c in gc.CASES if c.src[0] == "conv"} == {1, 2, 3, 4}
    assert {(c.epi, len(c.targets)) for c in gc.CASES} >= {("emb", 1), ("reslo", 1), ("reslo", 2), ("outlo", 1),
                                                           ("outlo", 2), ("plain", 2), ("silu", 1)}
    for bn in (64, 128):
        for s in (2, 3):
            assert {c.combine for c in gc.CASES if c.expect == (0, 64, bn, s) and c.src == gc.D2} == \
                {"coop", "last", "reduce"}
    # B >= 2 everywhere but on the one-image 30 x 30 conv (M = hw = 900), which runs under two plans: a forced
    # 128-row tile that must shrink, and the planner's own (two cases, one operand source)
    assert {c.name for c in gc.CASES if gc.src_shape(c.src)[0] == 1} == {"m900-128x128", "m900-own"}
    assert gc.CASE["m900-128x128"].src == gc.CASE["m900-own"].src == gc.C900
    # the producer-to-case table: every product producer is named by a case
    named = " | ".join(c.stands_for for c in gc.CASES)
    assert all(p in named for p in gc.PRODUCERS), [p for p in gc.PRODUCERS if p not in named]
    # every target of the table: 10 .. 80-channel groups, offsets that are no multiple of the group width included
    tg = {t for c in gc.CASES for t in c.targets}
    assert {t.cg for t in tg} == {10, 20, 30, 40, 60, 80}
    assert any(t.c_off % t.cg for t in tg)


def _plain_desc(**kw):
    f = dict(M=256, N=320, K=64, amode=0, A=64, lda=64, Wt=64, ldw=64, out=64, ldo=320, rows_per_b=128)
    f.update(kw)
    return gc.make_desc(**f)


def test_refused_statistics_targets():
    L, _ = _L()

    def refused(d, text):
        rc, _ = gc.plan_of(d)
        msg = (L.tair_last_error() or b"").decode()
        assert rc != 0 and text in msg, (rc, msg)

    ok = dict(st_acc=64, st_rs=128, st_cg=10, st_G=32, st_coff=0, st_hw=128)
    assert gc.plan_of(_plain_desc(**ok))[0] == 0, L.tair_last_error()
    assert gc.plan_of(_plain_desc(st2_acc=64, st2_rs=128, st2_cg=30, st2_G=32, st2_coff=640, **ok))[0] == 0
    # a second target without the first
    refused(_plain_desc(st2_acc=64, st2_rs=128, st2_cg=30, st2_G=32, st2_coff=640, st_hw=128),
            "unsupported GroupNorm statistics target")
    # 4-channel groups at an offset that is not 4-aligned (on either target); 4-aligned is taken
    assert gc.plan_of(_plain_desc(**dict(ok, st_cg=4, st_coff=8)))[0] == 0, L.tair_last_error()
    refused(_plain_desc(**dict(ok, st_cg=4, st_coff=2)), "unsupported GroupNorm statistics target")
    refused(_plain_desc(st2_acc=64, st2_rs=128, st2_cg=4, st2_G=32, st2_coff=2, **ok),
            "unsupported GroupNorm statistics target")
    # hw does not divide M
    refused(_plain_desc(**dict(ok, st_hw=96)), "unsupported GroupNorm statistics target")
    # several batch elements whose hw is no multiple of 64; one batch element of the same hw is taken
    refused(_plain_desc(M=192, **dict(ok, st_hw=96)), "need hw % 64 == 0")
    assert gc.plan_of(_plain_desc(M=96, **dict(ok, st_hw=96)))[0] == 0, L.tair_last_error()


def test_descriptor_mirror_matches_the_library():
    L, lib = _L()
    assert L.tair_k_gemm_desc_bytes() == ctypes.sizeof(lib.GemmDesc)
    names = [f[0] for f in lib.GemmDesc._fields_]
    assert names[-5:] == ["st2_acc", "st2_rs", "st2_cg", "st2_G", "st2_coff"]  # appended: no earlier offset moved
    assert lib.GemmDesc.ln_eps.offset < lib.GemmDesc.st2_acc.offset


# ---- the reference helpers against brute force -------------------------------------------------------------
def test_conv_ref_matches_conv2d_and_loops():
    gen = torch.Generator().manual_seed(1)
    x = torch.randn(2, 4, 6, 3, generator=gen, dtype=torch.float64)
    w = torch.randn(5, 3, 3, 3, generator=gen, dtype=torch.float64)
    xn = x.permute(0, 3, 1, 2)
    want = {
        gc.A_CONV3: F.conv2d(xn, w, padding=1),
        gc.A_CONV3_S2: F.conv2d(xn, w, stride=2, padding=1),
        gc.A_CONV3_UP: F.conv2d(F.interpolate(xn, scale_factor=2, mode="nearest"), w, padding=1),
    }
    for amode, y in want.items():
        got = gc.conv_ref(x, w, amode)
        assert torch.allclose(got, y.permute(0, 2, 3, 1).reshape(-1, 5), rtol=0, atol=1e-12), amode
    # stride 1 by loops: out[b, y, x, n] = sum w[n, c, ky, kx] x[b, y + ky - 1, x + kx - 1, c]
    got = gc.conv_ref(x, w, gc.A_CONV3).view(2, 4, 6, 5)
    for b, yy, xx, n in [(0, 0, 0, 0), (1, 3, 5, 4), (0, 2, 3, 1)]:
        acc = 0.0
        for ky in range(3):
            for kx in range(3):
                iy, ix = yy + ky - 1, xx + kx - 1
                if 0 <= iy < 4 and 0 <= ix < 6:
                    acc += float((w[n, :, ky, kx] * x[b, iy, ix]).sum())
        assert abs(acc - got[b, yy, xx, n].item()) < 1e-12


def test_pack_conv_w_k_order():
    w = torch.arange(2 * 128 * 9, dtype=torch.float32).view(2, 128, 3, 3)
    p = gc.pack_conv_w(w)
    assert p.shape == (2, 9 * 128)
    for n, c, tap in [(0, 0, 0), (1, 70, 5), (1, 127, 8), (0, 63, 4)]:
        assert p[n, (c // 64 * 9 + tap) * 64 + c % 64] == w[n, c, tap // 3, tap % 3]
    w4 = torch.arange(3 * 4 * 9, dtype=torch.float32).view(3, 4, 3, 3)
    p4 = gc.pack_conv_w(w4)
    assert p4.shape == (3, 64) and bool((p4[:, 36:] == 0).all())
    for n, c, tap in [(0, 0, 0), (2, 3, 8), (1, 2, 4)]:
        assert p4[n, tap * 4 + c] == w4[n, c, tap // 3, tap % 3]


def test_slot_sums_by_loops():
    gen = torch.Generator().manual_seed(2)
    B, hw, N = 2, 3, 20
    v = torch.randn(B * hw, N, generator=gen, dtype=torch.float64)
    for t in (gc.Tgt(10, 4, 0), gc.Tgt(6, 8, 14), gc.Tgt(30, 32, 640 - 630)):
        s, q, sa, cnt = gc.slot_sums(v, B, hw, t)
        ws, wq, wa, wc = (torch.zeros(B, t.G, dtype=torch.float64) for _ in range(4))
        for m in range(B * hw):
            for n in range(N):
                g = (t.c_off + n) // t.cg
                if g < t.G:
                    x = v[m, n].item()
                    ws[m // hw, g] += x
                    wq[m // hw, g] += x * x
                    wa[m // hw, g] += abs(x)
                    wc[m // hw, g] += 1
        for a, b in ((s, ws), (q, wq), (sa, wa), (cnt, wc)):
            assert torch.allclose(a, b, rtol=0, atol=1e-12)
    # the bounds: an exact result passes, a value in the neighbouring group or batch element does not
    sums = gc.slot_sums(v, B, hw, gc.Tgt(6, 8, 14))
    got = torch.stack([sums[0], sums[1]], -1)
    es, eq, own = gc.slot_errors(got, sums, hilo=False)
    assert es == 0 and eq == 0 and int(own.sum()) == B * 4  # channels 14 .. 33: groups 2 .. 5
    for hilo in (False, True):
        bad = got.clone()
        bad[0, 2, 0] -= v[0, 3].item()  # one value of group 2 lost ...
        bad[0, 3, 0] += v[0, 3].item()  # ... to group 3
        assert gc.slot_errors(bad, sums, hilo)[0] > 1
        assert gc.slot_errors(got.flip(0), sums, hilo)[0] > 1


def test_dense_reference_by_loops():
    o = gc.Ops(gc.dense(2, 4, 64, 64), 320, "emb", "cpu")
    t = o.t
    for m, n in [(0, 0), (5, 319), (7, 11)]:
        acc = sum(float(t["A"][m, k]) * float(t["Wt"][n, k]) for k in range(64))
        acc += sum(float(t["X"][m, k]) * float(t["Wt"][n, 64 + k]) for k in range(64))
        acc += float(t["bias"][n]) + float(t["emb"][int(t["emb_row"][m // 4]), n])
        assert abs(acc - o.ref[m, n].item()) < 1e-9
    o2 = gc.Ops(gc.dense(2, 4, 64), 320, "reslo", "cpu")
    m, n = 6, 100
    acc = sum(float(o2.t["A"][m, k]) * float(o2.t["Wt"][n, k]) for k in range(64)) + float(o2.t["bias"][n])
    acc += float(o2.t["res"][0, m, n]) + float(o2.t["res"][1, m, n])
    assert abs(acc - o2.ref[m, n].item()) < 1e-9
    o3 = gc.Ops(gc.dense(2, 4, 64), 320, "silu", "cpu")
    pre = o3.t["A"].double() @ o3.t["Wt"].double().t() + o3.t["bias"].double()
    assert torch.allclose(o3.ref, F.silu(pre), rtol=0, atol=1e-12)
    # the batch elements' outputs differ in mean by more than their spread within a group
    means = o.ref.view(2, 4, 320).mean((1, 2))
    assert abs(means[0] - means[1]) > 3


def test_group_norm_reference_and_emulation():
    gen = torch.Generator().manual_seed(3)
    B, hw, C = 2, 8, 960
    x = (torch.randn(B * hw, C, generator=gen) * 2 + 1).to(torch.bfloat16)
    gamma, beta = gc.gn_params(C)
    ref = gc.gn_ref(x, B, hw, gamma, beta)
    b, g = 1, 21  # by loops: the group that two producers share in the product
    blk = x.double().view(B, hw, C)[b, :, 30 * g:30 * g + 30]
    mean = blk.sum() / blk.numel()
    var = (blk * blk).sum() / blk.numel() - mean * mean
    want = (blk - mean) / torch.sqrt(var + gc.GN_EPS) * gamma[30 * g:30 * g + 30].double() + beta[30 * g:30 * g + 30].double()
    assert torch.allclose(ref.view(B, hw, C)[b, :, 30 * g:30 * g + 30], want, rtol=0, atol=1e-10)
    r = gc.block_ratios(gc.gn_emulate(x, B, hw, gamma, beta), ref, B, hw)
    assert r.shape == (B, gc.G) and float(r.max()) < 1.5 and float(r.min()) > 0.5
