"""Two-K-group 64-row tiles (gemm_kern.h gemm_kgroup_kernel), host side: the K-tile schedule of the two groups
(the same kgroup_trips / kgroup_tile functions the kernel runs, through the C ABI) and the planner rule
(tair_k_gemm_plan dry runs; kernel id 5, forced by force_stages = 203).
"""
import ctypes

import pytest

KERN_TILE, KERN_KGROUP = 0, 5


def _L():
    from tair_amd import _lib
    return _lib.lib(), _lib


@pytest.mark.parametrize("kt0", [0, 3, 10])
def test_trip_count_covers_every_tile_once(kt0):
    L, _ = _L()
    for ntiles in range(0, 10):
        kt1 = kt0 + ntiles
        trips = L.tair_k_kgroup_trips(kt0, kt1)  # one count: both groups run it
        assert trips == (ntiles + 1) // 2
        seen = []
        for g in (0, 1):
            real = [L.tair_k_kgroup_tile(kt0, g, j) for j in range(trips)]
            assert all(t >= kt0 for t in real)
            seen += [t for t in real if t < kt1]
            # a trip past the slice (group 1, odd count) is the group's last one only
            assert all(t < kt1 for t in real[:-1])
        assert sorted(seen) == list(range(kt0, kt1)), (kt0, ntiles)
        if ntiles <= 1:  # group 1 has no real tile
            assert [L.tair_k_kgroup_tile(kt0, 1, j) for j in range(trips) if
                    L.tair_k_kgroup_tile(kt0, 1, j) < kt1] == []
    assert L.tair_k_kgroup_trips(5, 3) == 0  # an empty slice


def _plan(**kw):
    L, lib = _L()
    d = lib.GemmDesc()
    d.alpha = 1.0
    d.partial, d.partial_cap, d.tile_sem, d.sem_cap = 1, 1 << 40, 1, 1 << 16
    for k, v in kw.items():
        setattr(d, k, v)
    out = [ctypes.c_int() for _ in range(4)]
    rc = L.tair_k_gemm_plan(ctypes.byref(d), *[ctypes.byref(o) for o in out])
    return rc, tuple(o.value for o in out)


def _conv(B, side, C, N, **kw):
    return dict(M=B * side * side, N=N, K=9 * C, amode=1, A=1, lda=C, C=C, Bn=B, H=side, W=side, Ho=side, Wo=side,
                rows_per_b=side * side, Wt=1, ldw=9 * C, out=1, ldo=N, **kw)


def _dense(M, N, K, **kw):
    return dict(M=M, N=N, K=K, amode=0, A=1, lda=K, Wt=1, ldw=K, out=1, ldo=N, **kw)


# the B = 1 shapes the rule names (gemm.hip kgroup_rule, profiles/kgroup_sweep.log): descriptor, tile width, the
# 4-wave plan's K slices -> the two-K-group plan's
RULE_SHAPES = [
    (_conv(1, 64, 320, 320), 128, 2, 1), (_conv(1, 64, 640, 320), 128, 2, 1), (_conv(1, 32, 640, 640), 128, 5, 3),
    (_conv(1, 32, 320, 640), 128, 5, 3), (_conv(1, 32, 1920, 640), 128, 5, 3), (_conv(1, 16, 1280, 1280), 128, 10, 6),
    (_conv(1, 16, 640, 1280), 128, 10, 6), (_conv(1, 16, 2560, 1280), 128, 10, 6),
]


@pytest.mark.parametrize("desc,bn,s4,s2", RULE_SHAPES)
def test_rule_shapes_take_the_new_kernel_with_fewer_slices(desc, bn, s4, s2):
    rc, plan4 = _plan(force_stages=3, **desc)  # the planner's 4-wave plan (a forced kernel keeps the rule off)
    assert rc == 0 and plan4 == (64, bn, s4, KERN_TILE)
    rc, plan = _plan(**desc)
    assert rc == 0 and plan == (64, bn, s2, KERN_KGROUP)
    tiles = -(-desc["M"] // 64) * -(-desc["N"] // bn)
    ktiles = desc["K"] // 64
    # one round of the 256 CUs, no more slices than the 4-wave plan (half or fewer where it split: the sweep's
    # exception is the 16x16 level, 10 -> 6), each K-group >= 2 K-tiles
    assert tiles * s2 <= 256 and s2 <= s4 and ktiles // s2 >= 4


@pytest.mark.parametrize("desc", [
    _conv(1, 8, 1280, 1280),                                                   # the 8x8 level: < 32 tiles
    _conv(1, 64, 960, 320),                                                    # one slice of 135 K-tiles: a tie
    # the linears: faster in isolation, no gain in the step
    _dense(1024, 640, 640), _dense(256, 1280, 1280), _dense(256, 3840, 1280), _dense(64, 1280, 5120),
    _dense(4096, 320, 320), _dense(4096, 960, 320), _dense(1024, 1920, 640),
    dict(_dense(1024, 640, 2560), X=1, ldx=640, Kx=640, ldw=3200),             # FF-out composed with proj_out
    dict(_conv(1, 32, 640, 640), tile_sem=0, sem_cap=0),                       # no split-K tickets
    # the two-image (guided) step, not swept: its grids keep their plans
    _conv(2, 64, 320, 320), _conv(2, 32, 640, 640), _conv(2, 32, 1280, 640), _conv(2, 16, 1280, 1280),
    _conv(2, 16, 2560, 1280), _conv(2, 8, 1280, 1280), _dense(2048, 640, 640), _dense(512, 1280, 1280),
])
def test_shapes_the_sweep_kept_on_the_4_wave_tiles(desc):
    rc, (_, _, _, kern) = _plan(**desc)
    assert rc == 0 and kern == KERN_TILE


@pytest.mark.parametrize("desc", [_conv(64, 16, 1280, 1280), _conv(64, 8, 1280, 1280), _dense(64 * 256, 1280, 5120),
                                  _dense(64 * 64, 1280, 5120), _dense(64 * 1024, 640, 2560)])
def test_batched_grids_never_take_it(desc):
    rc, (_, _, _, kern) = _plan(**desc)
    assert rc == 0 and kern != KERN_KGROUP


def test_fp8_and_groupnorm_on_load_never_take_it():
    # fp8 linears at B = 1 (K counts byte pairs): the planner keeps its e4m3 tiles, a forced request is an error
    f8 = dict(f8=1, col_scale=1)
    rc, (_, _, _, kern) = _plan(**_dense(256, 1280, 2560, **f8))
    assert rc == 0 and kern != KERN_KGROUP
    rc, _ = _plan(**_dense(256, 1280, 2560, force_bm=64, force_bn=64, force_splits=1, force_stages=203, **f8))
    assert rc != 0
    gn = dict(gn_st=1, gn_rs=64, gn_G=32, gn_eps=1e-5, gn_gamma=1, gn_beta=1, gn_silu=1)
    # (a B = 1 conv with GroupNorm on load has no tile plan at all: the 4-wave 3-stage tiles keep the plain loop)
    assert _plan(**_conv(1, 16, 1280, 1280, **gn))[0] != 0
    rc, (_, _, _, kern) = _plan(**_conv(16, 16, 1280, 1280, **gn))  # the halo tiles take it
    assert rc == 0 and kern == 3
    rc, _ = _plan(**_conv(1, 16, 1280, 1280, force_bm=64, force_bn=128, force_splits=5, force_stages=203, **gn))
    assert rc != 0


def test_forced_request_reports_the_kernel_and_refuses_unbuilt_tiles():
    L, _ = _L()
    rc, plan = _plan(**_dense(256, 1280, 1280, force_bm=64, force_bn=128, force_splits=2, force_stages=203))
    assert rc == 0 and plan == (64, 128, 2, KERN_KGROUP)
    rc, plan = _plan(**_conv(1, 8, 1280, 1280, force_bm=64, force_bn=64, force_splits=8, force_stages=203))
    assert rc == 0 and plan == (64, 64, 8, KERN_KGROUP)
    for bad in [dict(force_bm=128, force_bn=128), dict(force_bm=128, force_bn=64), dict(force_bm=64, force_bn=256)]:
        rc, _ = _plan(**_dense(4096, 1280, 1280, force_splits=1, force_stages=203, **bad))
        assert rc != 0 and b"two-K-group" in L.tair_last_error()
    rc, _ = _plan(**_dense(256, 1280, 1280, force_bm=64, force_bn=64, force_splits=1, force_stages=204))  # 4 stages
    assert rc != 0
    # stride-2 and upsampling convs are not built
    d = _conv(1, 16, 640, 640, force_bm=64, force_bn=64, force_splits=1, force_stages=203)
    d.update(amode=2, H=32, W=32)
    assert _plan(**d)[0] != 0
