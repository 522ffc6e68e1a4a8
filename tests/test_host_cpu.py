"""CPU tests of the C-ABI library (load + symbols + manifest) and of the host-side logic."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

from tair_amd import _lib
from tair_amd.diffusion import Diffusion, spaced_tables, space_timesteps as prod_space
from oracle.merge_ref import merge_patches_with_overlap, ramp_window
from tair_amd.tiling import (patch_grid, shard_range,
                             split_image_with_overlap, split_nonoverlap, stitch_nonoverlap)
from tair_amd.weights import manifest, synthetic_state_dict

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared_symbols():
    syms = set()
    for hdr in ("tair_cldm.h", "tair_kernels.h"):
        txt = open(os.path.join(ROOT, "include", hdr)).read()
        syms |= set(re.findall(r"^\s*(?:int|const char\*)\s+(tair_\w+)\s*\(", txt, re.M))
    return syms


def test_library_exports_every_declared_symbol():
    L = _lib.lib()
    declared = _declared_symbols()
    assert len(declared) >= 20
    for s in declared:
        assert hasattr(L, s), s
    assert declared <= set(_lib.SIGNATURES), declared - set(_lib.SIGNATURES)
    assert L.tair_version().startswith(b"tair_amd")
    # the ctypes mirror of tair_gemm_desc has the C struct's size (a field added on one side only is caught)
    assert ctypes.sizeof(_lib.GemmDesc) == L.tair_k_gemm_desc_bytes()


def test_error_path_is_loud():
    L = _lib.lib()
    h = ctypes.c_void_p()
    rc = L.tair_cldm_create(None, ctypes.byref(h))
    assert rc != 0 and b"null" in L.tair_last_error()
    c = _lib.default_cfg()
    c.head_channels = 80
    c.manifest_only = 1
    assert L.tair_cldm_create(ctypes.byref(c), ctypes.byref(h)) != 0


def test_manifest_matches_oracle_state_dict():
    from oracle.ldm_ref import ControlLDMRef
    m = dict(manifest())
    with torch.device("meta"):
        o = ControlLDMRef()
    sd = {k: tuple(v.shape) for k, v in o.state_dict().items()}
    assert m == sd


def test_manifest_only_handle_refuses_compute():
    L = _lib.lib()
    c = _lib.default_cfg()
    c.manifest_only = 1
    h = ctypes.c_void_p()
    _lib.check(L.tair_cldm_create(ctypes.byref(c), ctypes.byref(h)))
    assert L.tair_cldm_finalize(h) != 0
    f = ctypes.c_double()
    _lib.check(L.tair_cldm_flops(h, 1, ctypes.byref(f)))
    # analytic ControlLDM work per 512^2 tile per step: 1.0734 TFLOP (UNet + CN).  The
    # per-step body here excludes what depends only on (t, c_txt) and is hoisted to once per
    # restoration: cross-attn K/V projections of the 77 context tokens (4*77*1024*sum(C) over the
    # 23 transformers = 5.75 GF) and the time-embedding MLP + emb_layers (~0.09 GF).
    sum_c = 2 * 320 + 2 * 640 + 2 * 1280 + 1280 + 3 * 1280 + 3 * 640 + 3 * 320 + (2 * 320 + 2 * 640 + 2 * 1280 + 1280)
    kv = 4 * 77 * 1024 * sum_c
    temb = 2 * 2 * (320 * 1280 + 1280 * 1280) + 2 * 1280 * (20160 + 9600)
    assert f.value + kv + temb == pytest.approx(1.0734e12, rel=2e-4)
    f2 = ctypes.c_double()
    _lib.check(L.tair_cldm_flops(h, 4, ctypes.byref(f2)))
    assert f2.value == pytest.approx(4 * f.value, rel=1e-9)
    L.tair_cldm_destroy(h)


def test_product_schedule_equals_oracle_bitwise():
    from oracle.sampler_ref import SpacedScheduleRef, diffusion_betas
    d = Diffusion(timesteps=1000, linear_start=0.00085, linear_end=0.012, zero_snr=True, parameterization="v")
    ob = diffusion_betas()
    assert np.array_equal(d.betas, ob)
    for n in (1, 2, 10, 50, 1000):
        ts, tabs = spaced_tables(d.betas, n)
        ref = SpacedScheduleRef(ob, n)
        assert ts.tolist() == ref.timesteps.tolist()
        for k, v in ref.tables.items():
            a = torch.from_numpy(tabs[k])
            assert torch.equal(a, v) or (torch.isinf(a) == torch.isinf(v)).all() and torch.equal(
                a[~torch.isinf(a)], v[~torch.isinf(v)]), k
    assert prod_space(1000, "ddim25") == set(range(0, 1000, 40))


def test_synthetic_weights_deterministic_and_scaled():
    ent = [("unet.input_blocks.1.0.in_layers.2.weight", (320, 320, 3, 3)),
           ("unet.input_blocks.1.0.in_layers.2.bias", (320,)),
           ("unet.input_blocks.1.0.out_layers.3.weight", (320, 320, 3, 3)),
           ("unet.input_blocks.1.0.in_layers.0.weight", (320,)),
           ("unet.input_blocks.1.0.in_layers.0.bias", (320,))]
    a = synthetic_state_dict(ent, seed=0)
    b = synthetic_state_dict(list(reversed(ent)), seed=0)
    for k in a:
        assert torch.equal(a[k], b[k])
    bound = 1 / math.sqrt(320 * 9)
    assert a[ent[0][0]].abs().max() <= bound and a[ent[0][0]].abs().max() > 0.9 * bound
    assert a[ent[2][0]].abs().max() <= 0.1 * bound + 1e-9
    assert torch.equal(a[ent[3][0]], torch.ones(320)) and torch.equal(a[ent[4][0]], torch.zeros(320))


def test_split_merge_roundtrip_overlap():
    rng = np.random.default_rng(0)
    img = rng.integers(0, 255, size=(300, 250, 3), dtype=np.uint8)
    patches = split_image_with_overlap(img, 128, 16)
    nh, nw = patch_grid(300, 250)
    assert (nh, nw) == (math.ceil(284 / 112), math.ceil(234 / 112))
    assert len(patches) == nh * nw and patches[0].shape == (128, 128, 3)
    # identity "restoration" at scale 1: merging the LQ patches returns the image exactly
    t = [torch.from_numpy(p.astype(np.float32)).permute(2, 0, 1)[None] for p in patches]
    merged = merge_patches_with_overlap(t, (300, 250), patch_size=128, overlap=16)
    assert merged.shape == (1, 3, 300, 250)
    assert torch.allclose(merged[0].permute(1, 2, 0), torch.from_numpy(img.astype(np.float32)), atol=1e-3)


def test_ramp_window_matches_reference_rule():
    w = ramp_window(512, 64)
    assert w[0, 0] == pytest.approx((1 / 64) ** 2)
    assert w[63, 256] == pytest.approx(1.0)
    assert w[256, 256] == 1.0
    assert torch.allclose(w, w.flip(0)) and torch.allclose(w, w.t())


def test_nonoverlap_split_and_stitch():
    img = np.arange(2048 * 2048 * 3, dtype=np.uint32).reshape(2048, 2048, 3) % 251
    tiles = split_nonoverlap(img, 128)
    assert len(tiles) == 256
    t = torch.from_numpy(np.stack(tiles).astype(np.float32)).permute(0, 3, 1, 2)
    back = stitch_nonoverlap(t, 16, 16)
    assert torch.equal(back[0].permute(1, 2, 0), torch.from_numpy(img.astype(np.float32)))


def test_shard_range_covers_everything():
    for n in (1, 7, 64, 256, 513):
        for w in (1, 2, 3, 8):
            got = []
            for r in range(w):
                lo, hi = shard_range(n, r, w)
                got.extend(range(lo, hi))
            assert got == list(range(n))


def test_fresh_checkout_builds_library_on_first_use(tmp_path):
    """A clone carries no *.so (git-ignored): the first lib() call must compile it in-tree."""
    import shutil
    import subprocess
    import sys
    dst = tmp_path / "repo"
    # the sources as a clone carries them: everything under tair_amd/ and include/ but the build's own products
    # (the tree is walked, not asked of git: an exported or foreign-owned checkout has no usable .git)
    products = shutil.ignore_patterns("*.so", "*.srchash", "*.tmp", "*.o", ".build.lock", "__pycache__", "*.pyc")
    for d in ("tair_amd", "include"):
        shutil.copytree(os.path.join(ROOT, d), dst / d, ignore=products)
    assert (dst / "tair_amd" / "csrc").is_dir() and (dst / "include" / "tair_cldm.h").exists()
    assert not (dst / "tair_amd" / "libtair_cldm.so").exists()
    code = ("import sys; sys.path.insert(0, %r); from tair_amd import _lib; L = _lib.lib(); "
            "print(L.tair_version().decode())" % str(dst))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "tair_amd" in r.stdout
    assert (dst / "tair_amd" / "libtair_cldm.so").exists()
    assert "linked" in r.stderr  # it was built here, not found
    # second use: up to date, no rebuild
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "building" not in r.stderr
