"""Classifier-free guidance in the fused sampler: the host-side pieces that need no GPU (the per-step scale
table, the C ABI's symbols and their ctypes mirror, argument checking on a device-less handle)."""
import ctypes

import numpy as np
import pytest

from tair_amd import _lib
from tair_amd.diffusion import Diffusion
from tair_amd.sampler import SpacedSampler


def _sampler(rescale):
    d = Diffusion(linear_start=0.00085, linear_end=0.012, zero_snr=True, parameterization="v")
    return SpacedSampler(d.betas, "v", rescale)


@pytest.mark.parametrize("rescale", [False, True])
@pytest.mark.parametrize("cfg_scale", [4.0, 0.5])
def test_guidance_scales_equal_oracle_bitwise(rescale, cfg_scale):
    """The device table is float32(get_cfg_scale(cfg_scale, model_t[i])) per loop index (sampler.py:31-38;
    the rescale rule only fires above 1)."""
    from oracle.sampler_ref import SpacedScheduleRef, cfg_scale_ref, diffusion_betas
    steps = 50
    got = _sampler(rescale)._guidance_scales(cfg_scale, steps)
    assert got.dtype == np.float32 and got.shape == (steps,)
    model_t = np.flip(SpacedScheduleRef(diffusion_betas(), steps).timesteps)
    want = np.asarray([cfg_scale_ref(cfg_scale, int(t), rescale) for t in model_t]).astype(np.float32)
    assert got.tobytes() == want.tobytes()
    if rescale and cfg_scale > 1:
        assert len(set(got.tolist())) > 1  # a schedule, not a constant
    else:
        assert set(got.tolist()) == {np.float32(cfg_scale).item()}


def test_library_exports_guidance_entry_points():
    L = _lib.lib()
    for name in ("tair_sampler_prepare_guided", "tair_k_sampler_step"):
        assert getattr(L, name) is not None
        assert name in _lib.SIGNATURES


def test_lib_declares_guidance_mirror():
    res, args = _lib.SIGNATURES["tair_sampler_prepare_guided"]
    assert res is ctypes.c_int
    assert args[1] is ctypes.POINTER(_lib.SamplerIO) or args[1]._type_ is _lib.SamplerIO
    assert args[2]._type_ is _lib.GuidanceIO
    assert [f[0] for f in _lib.GuidanceIO._fields_] == ["c_txt", "c_txt_batch", "c_img", "scales"]
    # the C struct: pointer, int (+ padding), pointer, pointer
    p = ctypes.sizeof(ctypes.c_void_p)
    assert ctypes.sizeof(_lib.GuidanceIO) == 4 * p
    assert _lib.GuidanceIO.c_img.offset == 2 * p and _lib.GuidanceIO.scales.offset == 3 * p
    assert len(_lib.SIGNATURES["tair_k_sampler_step"][1]) == 15


def test_guided_prepare_on_manifest_only_handle_fails_loudly():
    L = _lib.lib()
    c = _lib.default_cfg()
    c.manifest_only = 1
    c.max_batch = 2
    h = ctypes.c_void_p()
    _lib.check(L.tair_cldm_create(ctypes.byref(c), ctypes.byref(h)))
    try:
        io = _lib.SamplerIO()
        io.batch = 1
        scales = _lib.float_array([4.0])
        g = _lib.GuidanceIO()
        g.c_txt_batch = 1
        g.scales = ctypes.cast(scales, ctypes.POINTER(ctypes.c_float))
        rc = L.tair_sampler_prepare_guided(h, ctypes.byref(io), ctypes.byref(g), None)
        assert rc < 0
        assert L.tair_last_error()
        with pytest.raises(_lib.TairError, match="manifest_only"):
            _lib.check(rc, "sampler_prepare_guided")
        assert L.tair_sampler_prepare_guided(None, ctypes.byref(io), ctypes.byref(g), None) < 0
        assert L.tair_last_error()
    finally:
        L.tair_cldm_destroy(h)


def test_kernel_entry_rejects_bad_arguments_without_a_device():
    """tair_k_sampler_step checks its shape arguments before any launch: a plane row narrower than the three
    planes it writes, or a missing scale table under guidance, is an error, not an out-of-bounds store."""
    L = _lib.lib()
    p = ctypes.c_void_p(16)
    assert L.tair_k_sampler_step(p, p, None, p, None, p, p, 8, 4, p, None, 8, 8, 0, None) == -1   # ld < 3C
    assert L.tair_k_sampler_step(p, p, p, p, None, p, p, 8, 4, p, None, 64, 8, 8, None) == -1     # no scales
    assert L.tair_k_sampler_step(p, p, None, p, None, p, p, 8, 4, p, p, 16, 8, 0, None) == -1     # in_c planes > ld
    assert b"sampler_step" in L.tair_last_error()
