"""The tiled cleaner's host side, no GPU: the plan of HipSwinIR.forward_tiled (tiling.plan_image_tiles), the
stock-torch tiling.make_tiled_fn against the reference loop restated in tests/_swinir_tiled_ref.py (bitwise: the same
fp32 operations in the same order), SwinIRPipeline.apply_cleaner's tiled rules (pipeline.py:371-397), the ABI of the
two image-tile kernels and their argument checks (a refused call launches nothing, so it needs no device)."""
import ctypes

import pytest
import torch

from tests._swinir_emul import randomize
from tests._swinir_tiled_ref import tiled_ref, weights32, windows_ref

REDUCED = dict(depths=[2, 2], num_heads=[6, 6])
TINY = dict(img_size=16, embed_dim=24, depths=[1], num_heads=[2], window_size=4, mlp_ratio=2, sf=4,
            upsampler="nearest+conv", unshuffle=True, unshuffle_scale=4)


def _stock(params=None, seed=5):
    from tair_amd.config import SWINIR_VAL_PARAMS
    from tair_amd.swinir import SwinIR
    p = dict(SWINIR_VAL_PARAMS, **REDUCED) if params is None else params
    return randomize(SwinIR(**p), seed).eval()


# --------------------------------------------------------------------------------------------- plan
def test_plan_windows_chunks_and_pad():
    from tair_amd.tiling import plan_image_tiles, sliding_windows
    p = plan_image_tiles(2, 100, 75, 64, 48, 3)
    assert p["windows"] == [(0, 64, 0, 64), (0, 64, 11, 75), (36, 100, 0, 64), (36, 100, 11, 75)]  # the last are flush
    assert (p["rows"], p["n_chunks"], p["rows_per_chunk"], p["pad"]) == (8, 3, 3, 1)
    assert p["chunks"] == [(0, 3), (3, 3), (6, 2)]
    p = plan_image_tiles(2, 200, 136, 128, 96, 3)
    assert p["windows"] == [(0, 128, 0, 128), (0, 128, 8, 136), (72, 200, 0, 128), (72, 200, 8, 136)]
    assert (p["rows"], p["n_chunks"], p["rows_per_chunk"], p["pad"]) == (8, 3, 3, 1)
    p = plan_image_tiles(2, 200, 136, 128, 96, 16)  # max_batch larger than the job: one chunk, no pad
    assert (p["n_chunks"], p["rows_per_chunk"], p["pad"], p["chunks"]) == (1, 8, 0, [(0, 8)])
    p = plan_image_tiles(1, 128, 128, 128, 96, 4)  # one window
    assert p["windows"] == [(0, 128, 0, 128)] and (p["n_chunks"], p["rows_per_chunk"], p["pad"]) == (1, 1, 0)
    p = plan_image_tiles(1, 1024, 1024, 512, 256, 4)  # the README's large image: 9 windows in 3 chunks of 3
    assert (p["rows"], p["n_chunks"], p["rows_per_chunk"], p["pad"]) == (9, 3, 3, 0)
    p = plan_image_tiles(3, 320, 256, 128, 64, 4)  # equal chunks: 36 rows in 9 chunks of 4
    assert (p["rows"], p["n_chunks"], p["rows_per_chunk"], p["pad"]) == (36, 9, 4, 0)
    for H, W, size, stride in [(100, 75, 64, 48), (200, 136, 128, 96), (1024, 1024, 512, 256), (131, 64, 64, 1)]:
        assert sliding_windows(H, W, size, stride) == windows_ref(H, W, size, stride)
    for bad in [(1, 200, 136, 96, 96, 4), (1, 100, 136, 128, 96, 4), (1, 200, 136, 128, 0, 4), (1, 200, 136, 128, 96, 0)]:
        with pytest.raises(ValueError):
            plan_image_tiles(*bad)


def test_input_check_of_forward_tiled():
    from tair_amd.swinir_hip import check_tiled_input
    assert check_tiled_input((2, 3, 200, 136), 128, 96, (16, 16)) == (2, 200, 136, 16)
    assert check_tiled_input((1, 3, 1024, 1024), 512, 256, (64, 64)) == (1, 1024, 1024, 64)
    for shape, tile, stride in [((2, 3, 200, 136), 256, 96),    # a token map of 32 x 32 above max_hw
                                ((2, 3, 100, 136), 128, 96),    # the image is smaller than the tile
                                ((2, 3, 200, 136), 96, 96),     # not a multiple of 64
                                ((2, 3, 200, 136), 128, 0), ((2, 1, 200, 136), 128, 96), ((3, 200, 136), 128, 96)]:
        with pytest.raises(ValueError):
            check_tiled_input(shape, tile, stride, (16, 16))


# ------------------------------------------------------------------------------------ make_tiled_fn
@pytest.fixture(scope="module")
def stock():
    return _stock()


def test_make_tiled_fn_is_the_reference_loop(stock):
    from tair_amd.tiling import gaussian_weights, make_tiled_fn
    x = torch.rand((2, 3, 200, 136), generator=torch.Generator().manual_seed(3))
    assert windows_ref(200, 136, 128, 96) == [(y, y + 128, xx, xx + 128) for y in (0, 72) for xx in (0, 8)]
    assert torch.equal(torch.tensor(gaussian_weights(128, 128), dtype=torch.float32), weights32(128))
    with torch.no_grad():
        got = make_tiled_fn(stock, 128, 96)(x)
    want = tiled_ref(stock, x, 128, 96)
    assert got.dtype == torch.float32 and tuple(got.shape) == (2, 3, 200, 136)
    assert torch.equal(got, want)
    with pytest.raises(ValueError):
        make_tiled_fn(stock, 128, 96)(torch.zeros(1, 3, 100, 136))
    with pytest.raises(ValueError):
        make_tiled_fn(stock, 128, 0)


def test_one_window_is_the_untiled_call_weighted_and_divided(stock):
    from tair_amd.tiling import make_tiled_fn
    x = torch.rand((1, 3, 128, 128), generator=torch.Generator().manual_seed(4))
    with torch.no_grad():
        y = stock(x)
        got = make_tiled_fn(stock, 128, 96)(x)
    w = weights32(128)
    assert torch.equal(got, (y * w) / w)  # fl(fl(y w) / w): within an ulp of y, not y itself
    assert (got - y).abs().max().item() <= 2.0 ** -22 * y.abs().max().item()


# ----------------------------------------------------------------------------------------- pipeline
@pytest.fixture(scope="module")
def tiny():
    return _stock(TINY, seed=6)


def test_apply_cleaner_tiled_rules(tiny):
    from tair_amd.pipeline import SwinIRPipeline, resize_short_edge_to
    from tair_amd.tiling import make_tiled_fn
    pipe = SwinIRPipeline(tiny, None, None, None, "cpu")
    g = torch.Generator().manual_seed(7)
    with torch.no_grad():
        small = torch.rand((1, 3, 96, 80), generator=g)  # below the tile: "tiny and unnecessary to tile"
        assert torch.equal(pipe.apply_cleaner(small, True, 128, 96), pipe.apply_cleaner(small, False, 128, 96))
        x = torch.rand((2, 3, 200, 136), generator=g)
        with pytest.raises(ValueError):
            pipe.apply_cleaner(x, True, 96, 96)
        # a stock SwinIR is served by make_tiled_fn on the unpadded image; the short edge (136) is resized afterwards
        got = pipe.apply_cleaner(x, True, 128, 96)
        tiled = make_tiled_fn(tiny, 128, 96)(x)
        assert tuple(tiled.shape) == (2, 3, 200, 136) and torch.equal(tiled, tiled_ref(tiny, x, 128, 96))
        assert min(got.shape[2:]) == 512 and torch.equal(got, resize_short_edge_to(tiled, 512))
        assert not torch.equal(got, pipe.apply_cleaner(x, False, 128, 96))  # (the untiled rule resizes first)
        big = torch.rand((1, 3, 520, 512), generator=g)  # no resize at 512 and above
        assert torch.equal(pipe.apply_cleaner(big, True, 256, 192), tiled_ref(tiny, big, 256, 192))


def test_apply_cleaner_dispatch():
    from tair_amd.pipeline import SwinIRPipeline
    from tair_amd.swinir import SwinIR
    from tair_amd.swinir_hip import HipSwinIR
    assert SwinIR.tiling is True and HipSwinIR.tiling is True and callable(HipSwinIR.forward_tiled)
    x = torch.rand((1, 3, 520, 512), generator=torch.Generator().manual_seed(8))
    for cleaner in (None, lambda t: t, torch.nn.Identity()):  # no `tiling`: refused as before, whatever the size
        pipe = SwinIRPipeline(cleaner, None, None, None, "cpu")
        with pytest.raises(NotImplementedError, match="tiled SwinIR"):
            pipe.apply_cleaner(x, True, 256, 192)
        with pytest.raises(NotImplementedError, match="tiled SwinIR"):
            pipe.apply_cleaner(x[..., :64, :64], True, 256, 192)

    class Tiled:  # a cleaner with its own tiled form (HipSwinIR's interface) gets the image as it is
        tiling = True

        def __init__(self):
            self.calls = []

        def forward_tiled(self, t, size, stride):
            self.calls.append((tuple(t.shape), size, stride))
            return t + 1

        def __call__(self, t):
            raise AssertionError("the untiled form was called")

    c = Tiled()
    out = SwinIRPipeline(c, None, None, None, "cpu").apply_cleaner(x, True, 256, 192)
    assert c.calls == [((1, 3, 520, 512), 256, 192)] and torch.equal(out, x + 1)


# ---------------------------------------------------------------------------------------------- ABI
def test_abi_declares_the_image_tile_kernels():
    import os
    from tair_amd import _lib
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "tair_kernels.h")).read()
    for name, nargs in (("tair_k_image_tile_gather", 13), ("tair_k_image_tile_blend", 14)):
        assert f"int {name}(" in hdr
        assert len(_lib.SIGNATURES[name][1]) == nargs
        assert getattr(_lib.lib(), name).restype is ctypes.c_int


GATHER_OK = dict(x=1 << 20, mean=1 << 20, B=2, H=100, W=75, tile=64, stride=48, first=0, rows=3, out=1 << 20, ld=384, lo=192)
BLEND_OK = dict(v=1 << 20, w=1 << 20, acc=1 << 20, cnt=1 << 20, out=1 << 20, B=2, H=100, W=75, tile=64, stride=48, first=6,
                rows=3, finalize=1)
GATHER_BAD = [dict(tile=96), dict(tile=0), dict(tile=128), dict(H=63), dict(stride=0), dict(first=-1), dict(first=8),
              dict(rows=0), dict(B=0), dict(x=None), dict(mean=None), dict(out=None), dict(ld=382), dict(lo=190),
              dict(lo=193, ld=386), dict(ld=200)]
BLEND_BAD = [dict(tile=96), dict(tile=128), dict(W=63), dict(stride=0), dict(first=-1), dict(first=8), dict(rows=0),
             dict(B=0), dict(v=None), dict(w=None), dict(acc=None), dict(cnt=None), dict(out=None),
             dict(first=3)]  # (finalize on a chunk that does not end the job)


def call_gather(L, a, stream=None):
    return L.tair_k_image_tile_gather(a["x"], a["mean"], a["B"], a["H"], a["W"], a["tile"], a["stride"], a["first"],
                                      a["rows"], a["out"], a["ld"], a["lo"], stream)


def call_blend(L, a, stream=None):
    return L.tair_k_image_tile_blend(a["v"], a["w"], a["acc"], a["cnt"], a["out"], a["B"], a["H"], a["W"], a["tile"],
                                     a["stride"], a["first"], a["rows"], a["finalize"], stream)


@pytest.mark.parametrize("bad", GATHER_BAD + BLEND_BAD, ids=lambda d: ",".join(f"{k}={v}" for k, v in d.items()))
def test_bad_arguments_are_refused_on_the_host(bad):
    """The checks run before any launch and read no operand: fake addresses, no device."""
    from tair_amd import _lib
    L = _lib.lib()
    if any(bad is b for b in GATHER_BAD):
        assert call_gather(L, dict(GATHER_OK, **bad)) == -1 and b"image_tile_gather" in L.tair_last_error()
    else:
        assert call_blend(L, dict(BLEND_OK, **bad)) == -1 and b"image_tile_blend" in L.tair_last_error()
