"""Latent tiling inside the fused sampler: the host-side pieces that need no GPU (windows, weights and the chunk
plan against known answers, the C ABI's new symbols and their ctypes mirror, argument checking on a device-less
handle and in the kernel hooks, the device-free argument rules of Pipeline.apply_cldm)."""
import ctypes
import types

import numpy as np
import pytest
import torch

from tair_amd import _lib


# ------------------------------------------------------------------------------------------ planning
def test_sliding_windows_known_answers():
    from tair_amd.tiling import sliding_windows
    assert sliding_windows(24, 36, 16, 8) == [(0, 16, 0, 16), (0, 16, 8, 24), (0, 16, 16, 32), (0, 16, 20, 36),
                                              (8, 24, 0, 16), (8, 24, 8, 24), (8, 24, 16, 32), (8, 24, 20, 36)]
    assert len(sliding_windows(64, 96, 64, 32)) == 2
    assert len(sliding_windows(128, 128, 64, 32)) == 9
    assert sliding_windows(16, 16, 16, 8) == [(0, 16, 0, 16)]
    assert sliding_windows(20, 16, 16, 8) == [(0, 16, 0, 16), (4, 20, 0, 16)]


def _close(a, b):
    return abs(a - b) <= 1e-15 * abs(b)


def test_gaussian_weights_known_answers():
    from tair_amd.tiling import gaussian_weights
    w = gaussian_weights(16, 16)
    assert w.dtype == np.float64 and w.shape == (16, 16)
    assert _close(w[0, 0], 1.004239794128151e-09)
    assert _close(w[8, 7], 15.157038243117928) and _close(w[8, 8], 15.157038243117928)
    assert w.max() == w[8, 7]
    assert _close(w[15, 15], 1.8801155515267566e-08)
    w = gaussian_weights(64, 64)
    assert _close(w[0, 0], 3.256709375915912e-10)
    assert _close(w[63, 63], 7.027002728209685e-10)
    assert _close(w[32, 31], 15.866998112053906) and w.max() == w[32, 31]
    assert w[0, 0] != w[63, 63]  # the reference's asymmetric row midpoint is kept


def test_weights_and_windows_equal_the_test_restatement():
    from tair_amd.tiling import gaussian_weights, sliding_windows
    from tests._tiled_ref import weights_ref, windows_ref
    for s in (16, 64):
        assert np.allclose(gaussian_weights(s, s), weights_ref(s), rtol=1e-14, atol=0)
    for geo in [(24, 36, 16, 8), (16, 40, 16, 8), (64, 96, 64, 32), (17, 16, 16, 5)]:
        assert sliding_windows(*geo) == windows_ref(*geo)


@pytest.mark.parametrize("B,H,W,size,stride,max_batch,guided,want", [
    (1, 24, 36, 16, 8, 8, False, (8, 8, 1, 8, 0)),
    (1, 24, 36, 16, 8, 3, False, (8, 3, 3, 3, 1)),
    (2, 24, 36, 16, 8, 6, False, (16, 6, 3, 6, 2)),
    (2, 24, 36, 16, 8, 6, True, (16, 3, 6, 3, 2)),
    (1, 128, 128, 64, 32, 2, False, (9, 2, 5, 2, 1)),
])
def test_plan_known_answers(B, H, W, size, stride, max_batch, guided, want):
    from tair_amd.tiling import plan_latent_tiles, sliding_windows
    p = plan_latent_tiles(B, H, W, size, stride, max_batch, guided)
    assert (p["rows"], p["cap"], p["n_chunks"], p["rows_per_chunk"], p["pad"]) == want
    assert p["windows"] == sliding_windows(H, W, size, stride)
    assert p["n_chunks"] * p["rows_per_chunk"] - p["pad"] == p["rows"]
    assert (p["n_chunks"] - 1) * p["rows_per_chunk"] < p["rows"]  # every chunk holds a job row


def test_plan_rejects_no_room_and_bad_geometry():
    from tair_amd.tiling import plan_latent_tiles
    with pytest.raises(ValueError, match="max_batch"):
        plan_latent_tiles(1, 24, 36, 16, 8, 1, True)  # cap = 1 // 2 = 0
    with pytest.raises(ValueError, match="smaller than the tile"):
        plan_latent_tiles(1, 12, 36, 16, 8, 4, False)
    with pytest.raises(ValueError, match="stride"):
        plan_latent_tiles(1, 24, 36, 16, 0, 4, False)


@pytest.mark.parametrize("geo", [(24, 36, 16, 8), (16, 40, 16, 8), (128, 128, 64, 32), (17, 23, 16, 5)])
def test_plan_covers_every_pixel(geo):
    from tair_amd.tiling import plan_latent_tiles
    H, W, size, stride = geo
    cover = np.zeros((H, W), dtype=np.int64)
    for y0, y1, x0, x1 in plan_latent_tiles(1, H, W, size, stride, 4, False)["windows"]:
        assert 0 <= y0 and y1 <= H and 0 <= x0 and x1 <= W and y1 - y0 == size and x1 - x0 == size
        cover[y0:y1, x0:x1] += 1
    assert cover.min() >= 1
    if geo == (24, 36, 16, 8):
        assert cover.max() == 6


# --------------------------------------------------------------------------------------------- C ABI
NEW = ("tair_sampler_prepare_tiled", "tair_sampler_tiling_info", "tair_k_tile_gather", "tair_k_tile_blend_step")


def test_library_exports_tiling_entry_points():
    L = _lib.lib()
    for name in NEW:
        assert getattr(L, name) is not None
        assert name in _lib.SIGNATURES
    assert ctypes.sizeof(_lib.TilingIO) == 12
    assert [f[0] for f in _lib.TilingIO._fields_] == ["height", "width", "stride"]
    assert _lib.SIGNATURES["tair_sampler_prepare_tiled"][1][3]._type_ is _lib.TilingIO
    assert len(_lib.SIGNATURES["tair_k_tile_gather"][1]) == 19
    assert len(_lib.SIGNATURES["tair_k_tile_blend_step"][1]) == 21


def test_sampler_has_the_tiled_surface():
    import inspect
    from tair_amd.sampler import SpacedSampler
    for fn in (SpacedSampler.sample, SpacedSampler.sample_trace):
        assert {"tiled", "tile_size", "tile_stride"} <= set(inspect.signature(fn).parameters)
    assert hasattr(SpacedSampler, "_sample_tiled_host")
    from tair_amd.diffusion import Diffusion
    s = SpacedSampler(Diffusion(linear_start=0.00085, linear_end=0.012, zero_snr=True, parameterization="v").betas)
    assert s.last_tiling is None


def test_tiled_prepare_on_manifest_only_and_null_handle_fails_loudly():
    L = _lib.lib()
    c = _lib.default_cfg()
    c.manifest_only = 1
    c.max_batch = 2
    h = ctypes.c_void_p()
    _lib.check(L.tair_cldm_create(ctypes.byref(c), ctypes.byref(h)))
    try:
        io = _lib.SamplerIO()
        io.batch = 1
        io.c_txt_batch = 1
        t = _lib.TilingIO(64, 96, 32)
        rc = L.tair_sampler_prepare_tiled(h, ctypes.byref(io), None, ctypes.byref(t), None)
        assert rc < 0
        with pytest.raises(_lib.TairError, match="manifest_only"):
            _lib.check(rc, "sampler_prepare_tiled")
        assert L.tair_sampler_prepare_tiled(None, ctypes.byref(io), None, ctypes.byref(t), None) < 0
        assert L.tair_last_error()
        # t == NULL is tair_sampler_prepare_guided: the same status, with and without guidance
        scales = _lib.float_array([4.0])
        g = _lib.GuidanceIO()
        g.c_txt_batch = 1
        g.scales = ctypes.cast(scales, ctypes.POINTER(ctypes.c_float))
        for gp in (None, ctypes.byref(g)):
            assert (L.tair_sampler_prepare_tiled(h, ctypes.byref(io), gp, None, None) ==
                    L.tair_sampler_prepare_guided(h, ctypes.byref(io), gp, None))
        w, ch, r, p = (ctypes.c_int(-1) for _ in range(4))
        assert L.tair_sampler_tiling_info(h, ctypes.byref(w), ctypes.byref(ch), ctypes.byref(r), ctypes.byref(p)) == 0
        assert (w.value, ch.value, r.value, p.value) == (0, 0, 0, 0)  # nothing tiled was prepared
        assert L.tair_sampler_tiling_info(None, ctypes.byref(w), ctypes.byref(ch), ctypes.byref(r), ctypes.byref(p)) < 0
    finally:
        L.tair_cldm_destroy(h)


def test_kernel_hooks_reject_bad_arguments_without_a_device():
    """Both hooks check their shape arguments before any launch (fake pointers: nothing may be dereferenced)."""
    L = _lib.lib()
    p = ctypes.c_void_p(16)

    def gather(B=2, H=24, W=36, S=16, stride=8, rpc=6, nch=3, C=4, hc=4, in_c=p, hint=p, ld=64, ldc=8, half=0):
        return L.tair_k_tile_gather(p, hint, None, p, B, H, W, S, stride, rpc, nch, C, hc, p, in_c, ld, ldc, half, None)

    assert gather(H=12) == -1            # latent below the tile
    assert b"tile_gather" in L.tair_last_error()
    assert gather(stride=0) == -1
    assert gather(rpc=6, nch=2) == -1    # 12 rows do not cover the 16 job rows
    assert gather(rpc=6, nch=4) == -1    # a chunk with no job row
    assert gather(ld=8) == -1            # a row narrower than the three planes
    assert gather(ldc=4) == -1           # hint planes do not fit
    assert gather(hint=None) == -1       # in_c without a hint
    assert gather(half=5) == -1          # the second half would overlap the first
    assert gather(B=0) == -1

    def blend(B=2, H=24, W=36, S=16, stride=8, rpc=6, nch=3, C=4, acc_u=None, scales=None, w=p):
        return L.tair_k_tile_blend_step(p, p, p, p, acc_u, p, w, p, scales, p, p, p, B, H, W, S, stride, rpc, nch, C,
                                        None)

    assert blend(W=15) == -1
    assert b"tile_blend_step" in L.tair_last_error()
    assert blend(stride=-1) == -1
    assert blend(rpc=5, nch=3) == -1
    assert blend(acc_u=p) == -1          # guided without a scale table
    assert blend(w=None) == -1
    assert blend(C=0) == -1


# ------------------------------------------------------------------------------------------ pipeline
def _pipe(latent_hw=(64, 64)):
    from tair_amd.diffusion import Diffusion
    from tair_amd.pipeline import Pipeline
    cldm = types.SimpleNamespace(latent_hw=latent_hw, control_scales=[1.0] * 13)
    d = Diffusion(linear_start=0.00085, linear_end=0.012, zero_snr=True, parameterization="v")
    return Pipeline(None, cldm, d, None, "cpu", text_encoder=lambda p: torch.zeros(len(p), 77, 1024))


def _apply(pipe, img, **kw):
    a = dict(steps=2, strength=1.0, vae_encoder_tiled=False, vae_encoder_tile_size=256, vae_decoder_tiled=False,
             vae_decoder_tile_size=256, cldm_tiled=True, cldm_tile_size=512, cldm_tile_stride=256, pos_prompt="a",
             neg_prompt="b", cfg_scale=1.0, start_point_type="noise", sampler_type="spaced", noise_aug=0,
             rescale_cfg=False)
    a.update(kw)
    return pipe.apply_cldm(img, **a)


def test_pipeline_tile_size_rules_need_no_device():
    img = torch.zeros(1, 3, 512, 768)
    with pytest.raises(ValueError, match="multiple of 64"):
        _apply(_pipe(), img, cldm_tile_size=500)
    with pytest.raises(ValueError, match="built for 64x64"):
        _apply(_pipe(), img, cldm_tile_size=256)      # a 32x32 latent tile on a 64x64 handle
    with pytest.raises(ValueError, match="built for 16x16"):
        _apply(_pipe((16, 16)), img, cldm_tile_size=512)
    with pytest.raises(NotImplementedError, match="tiled VAE"):
        _apply(_pipe(), img, vae_decoder_tiled=True)  # still out of scope
