"""FF-out composed with proj_out, the host side: the packing routine finalize uses
(tair_k_compose_ffpout) against numpy fp64, and the parameter manifest, which the composite must not enter.

    out = x + (X2 + F Wff2^T + b_ff2) Wpout^T + b_pout = x + [F | X2] [Wpout Wff2 | Wpout]^T + (Wpout b_ff2 + b_pout)

Tolerance (written here): a packed value is ONE bf16 rounding of a product formed at fp32 accuracy or better, so it
lies within half a bf16 ulp (at most 2^-8 relative: 8 significand bits) of the fp64 value plus the fp32-level error of the sum (1e-6 of the
row's magnitude sum); the copied Wpout columns are exactly bf16(Wpout); the bias is an fp64 sum rounded to fp32.
"""
import ctypes

import numpy as np
import pytest


def _bf16_bits_to_f64(b):
    return (b.astype(np.uint32) << 16).view(np.float32).astype(np.float64)


def _bf16_round_bits(x32):
    u = x32.astype(np.float32).view(np.uint32).astype(np.uint64)
    u = u + 0x7FFF + ((u >> 16) & 1)
    return (u >> 16).astype(np.uint16)


def _compose(wp, wf, bf, bp, ldp):
    from tair_amd import _lib
    L = _lib.lib()
    C = wp.shape[0]
    packed = np.full((C, ldp), 0x7FC0, dtype=np.uint16)  # NaN bits: every column must be written
    bias = np.full(C, np.nan, dtype=np.float32)
    rc = L.tair_k_compose_ffpout(wp.ctypes.data, wf.ctypes.data, bf.ctypes.data, bp.ctypes.data, C,
                                 packed.ctypes.data, ldp, bias.ctypes.data)
    assert rc == 0
    return packed, bias


@pytest.mark.parametrize("C,pad", [(64, 0), (320, 0), (320, 64), (72, 24)])
def test_compose_against_fp64(C, pad):
    rng = np.random.default_rng(C + pad)
    wp = (rng.standard_normal((C, C)) / np.sqrt(C)).astype(np.float32)
    wf = (rng.standard_normal((C, 4 * C)) / np.sqrt(4 * C)).astype(np.float32)
    bf = (rng.standard_normal(C) * 0.3).astype(np.float32)
    bp = (rng.standard_normal(C) * 0.3).astype(np.float32)
    ldp = 5 * C + pad
    packed, bias = _compose(wp, wf, bf, bp, ldp)
    assert packed.shape == (C, ldp)
    got = _bf16_bits_to_f64(packed)
    prod = wp.astype(np.float64) @ wf.astype(np.float64)                      # [C][4C]
    mag = np.abs(wp).astype(np.float64) @ np.abs(wf).astype(np.float64)
    # column order [Wpout Wff2 | Wpout | 0]; one rounding of the product
    err = np.abs(got[:, :4 * C] - prod)
    assert np.all(err <= 2.0 ** -8 * np.abs(prod) + 1e-6 * mag + 1e-37), float(err.max())
    # rounded once, not twice: almost every entry IS the bf16 rounding of the fp64 product (the rest sit on a
    # rounding boundary within the fp32-level error of the sum)
    exact = _bf16_round_bits(prod.astype(np.float32))
    assert np.mean(packed[:, :4 * C] == exact) >= 0.995
    assert np.array_equal(packed[:, 4 * C:5 * C], _bf16_round_bits(wp))
    assert not packed[:, 5 * C:].any()
    want_b = wp.astype(np.float64) @ bf.astype(np.float64) + bp
    assert np.allclose(bias, want_b, rtol=1e-6, atol=1e-7)


def test_compose_rejects_short_rows():
    from tair_amd import _lib
    L = _lib.lib()
    z = np.zeros(64 * 256, dtype=np.float32)
    out = np.zeros(64 * 320, dtype=np.uint16)
    assert L.tair_k_compose_ffpout(z.ctypes.data, z.ctypes.data, z.ctypes.data, z.ctypes.data, 64, out.ctypes.data,
                                   319, z.ctypes.data) != 0


@pytest.mark.parametrize("M,C,want", [
    # B = 1: 64^2, 32^2, 16^2, 8^2 (profiles/ffpout_sweep.log)
    (4096, 320, (64, 128, 1)), (1024, 640, (64, 64, 3)), (256, 1280, (64, 64, 6)), (64, 1280, (64, 64, 10)),
    # the guided B = 2 step
    (8192, 320, (64, 128, 1)), (2048, 640, (64, 128, 3)), (512, 1280, (64, 64, 3)), (128, 1280, (64, 64, 6)),
])
def test_planner_chooses_the_composite_shapes_explicitly(M, C, want):
    """The composite (dense, N = C, K = 4C, Kx = C) on one lane: 64-row tile-kernel plans whose slices combine
    in-kernel, the tile width and split count of the sweep."""
    from tair_amd import _lib
    L = _lib.lib()
    d = _lib.GemmDesc()
    d.alpha = 1.0
    d.partial, d.partial_cap, d.tile_sem, d.sem_cap = 1, 1 << 40, 1, 1 << 14
    d.M, d.N, d.K, d.Kx, d.amode = M, C, 4 * C, C, 0
    d.A, d.lda, d.X, d.ldx, d.Wt, d.ldw, d.out, d.ldo = 1, 4 * C, 1, C, 1, 5 * C, 1, C
    out = [ctypes.c_int() for _ in range(4)]
    assert L.tair_k_gemm_plan(ctypes.byref(d), *[ctypes.byref(o) for o in out]) == 0
    bm, bn, splits, kern = (o.value for o in out)
    assert kern == 0 and (bm, bn, splits) == want


def test_manifest_has_no_composite_entry():
    """The composite has no backing parameter: the manifest is the reference state dict's key set (every
    SpatialTransformer contributes ff.net.2 and proj_out, weight and bias, and nothing else new)."""
    from oracle.ldm_ref import CLDMConfig, ControlLDMRef
    from tair_amd import _lib
    from tair_amd.weights import manifest
    import torch
    c = _lib.default_cfg()
    c.model_channels, c.num_levels, c.num_res_blocks = 64, 2, 1
    c.channel_mult[0], c.channel_mult[1] = 1, 2
    c.num_attention_ds = 2
    c.attention_ds[0], c.attention_ds[1] = 1, 2
    c.head_channels, c.context_dim = 64, 64
    ent = manifest(c)
    with torch.device("meta"):
        ref = ControlLDMRef(CLDMConfig(model_channels=64, channel_mult=(1, 2), num_res_blocks=1,
                                       attention_resolutions=(1, 2), head_channels=64, context_dim=64))
    want = {k: tuple(v.shape) for k, v in ref.state_dict().items()}
    got = {k: tuple(s) for k, s in ent}
    assert len(ent) == len(got)
    assert got == want
    assert not [k for k in got if "fpo" in k or "compos" in k]
