"""Patch split / stitch of the val_patches driver (reference: val_patches.py:25-206, image_splitter.py:23-51).

* ``split_image_with_overlap``: stride = patch - overlap, right/bottom zero pad so that
  ceil((H - overlap) / stride) x ceil((W - overlap) / stride) patches cover the image (val_patches.py:25-92).
* ``merge_patches_with_overlap_device``: linear-ramp window of ``overlap`` pixels on all four sides,
  weighted sum / weight map, crop to scale * original size (val_patches.py:114-206), one HIP kernel.
  The reference hard-codes the LQ stride 112 / patch 128 (val_patches.py:134-138); they are parameters
  here with the same defaults.  Its host restatement (the checker) is oracle/merge_ref.py.
* ``split_nonoverlap``: floor(W/tile) x floor(H/tile) crops in raster order (image_splitter.py:23-51).
* ``sliding_windows`` / ``gaussian_weights`` / ``plan_latent_tiles``: the host plan of latent tiling inside the
  sampling loop (utils/common.py:125-234 make_tiled_fn): overlapping windows of the whole latent, Gaussian
  blend weights, and the split of the B x T window rows into equal chunks of at most the handle's batch.
"""
from __future__ import annotations

import math
from typing import Dict, List, Sequence, Tuple

import numpy as np
import torch


def patch_grid(height: int, width: int, patch: int = 128, overlap: int = 16) -> Tuple[int, int]:
    stride = patch - overlap
    return math.ceil((height - overlap) / stride), math.ceil((width - overlap) / stride)


def split_image_with_overlap(img: np.ndarray, patch_size: int = 128, overlap: int = 16) -> List[np.ndarray]:
    """img: HxW or HxWxC uint8 array -> list of patch arrays (row-major)."""
    arr = np.asarray(img)
    squeeze = arr.ndim == 2
    if squeeze:
        arr = arr[:, :, None]
    h, w = arr.shape[:2]
    stride = patch_size - overlap
    nh, nw = patch_grid(h, w, patch_size, overlap)
    ph, pw = (nh - 1) * stride + patch_size, (nw - 1) * stride + patch_size
    padded = np.pad(arr, ((0, ph - h), (0, pw - w), (0, 0)), mode="constant", constant_values=0)
    out = []
    for i in range(nh):
        for j in range(nw):
            p = padded[i * stride:i * stride + patch_size, j * stride:j * stride + patch_size]
            out.append(p[:, :, 0] if squeeze else p)
    return out


def merge_patches_with_overlap_device(tiles: torch.Tensor, original_size: Tuple[int, int], patch_size: int = 512,
                                      overlap: int = 64, lq_patch: int = 128, lq_overlap: int = 16) -> torch.Tensor:
    """merge_patches_with_overlap on the GPU in one HIP kernel (tair_k_merge_overlap): tiles (N, C, P, P)
    fp32 on a ROCm device -> (1, C, scale*H, scale*W); bitwise equal to the reference loop
    (oracle/merge_ref.py, tests/test_val_patches_gpu.py)."""
    import ctypes
    from . import _lib
    if not tiles.is_cuda:
        raise _lib.TairError("merge_patches_with_overlap_device: tiles must be on a ROCm device")
    t = tiles.detach().to(torch.float32).contiguous()
    n, c, p, q = t.shape
    assert p == q == patch_size
    stride = patch_size - overlap
    lq_stride = lq_patch - lq_overlap
    oh, ow = original_size
    nh = math.ceil((oh - lq_overlap) / lq_stride)
    nw = math.ceil((ow - lq_overlap) / lq_stride)
    scale = patch_size / lq_patch
    H, W = int(oh * scale), int(ow * scale)
    rtab = torch.tensor([(i + 1) / overlap for i in range(overlap)], dtype=torch.float32).to(t.device)
    out = torch.empty((1, c, H, W), device=t.device, dtype=torch.float32)
    L = _lib.lib()
    _lib.check(L.tair_k_merge_overlap(t.data_ptr(), n, nh, nw, patch_size, overlap, stride, out.data_ptr(), c, H, W,
                                      rtab.data_ptr(), ctypes.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)),
               "merge_overlap")
    return out


def split_nonoverlap(img: np.ndarray, tile: int = 128) -> List[np.ndarray]:
    """image_splitter.py:23-51 (rows = H // tile, cols = W // tile, raster order)."""
    arr = np.asarray(img)
    h, w = arr.shape[:2]
    return [arr[i * tile:(i + 1) * tile, j * tile:(j + 1) * tile] for i in range(h // tile) for j in range(w // tile)]


def stitch_nonoverlap(tiles: torch.Tensor, rows: int, cols: int) -> torch.Tensor:
    """Inverse of split_nonoverlap for (rows*cols, C, P, P) restored tiles -> (1, C, rows*P, cols*P)."""
    n, c, p, q = tiles.shape
    assert n == rows * cols
    return tiles.view(rows, cols, c, p, q).permute(2, 0, 3, 1, 4).reshape(1, c, rows * p, cols * q)


def shard_range(n_items: int, rank: int, world: int) -> Tuple[int, int]:
    """Contiguous block [r*ceil(T/W), ...) of the global raster order."""
    per = (n_items + world - 1) // world
    lo = min(n_items, rank * per)
    return lo, min(n_items, lo + per)


def image_tile_grid(lq_h: int, lq_w: int, split: str = "nonoverlap", tile: int = 128, overlap: int = 16):
    """(rows, cols) of the 128^2 LQ tiles of one image: image_splitter.py:23-51 (floor, no overlap) or
    val_patches.py:25-92 (stride 112, zero pad)."""
    if split == "nonoverlap":
        return lq_h // tile, lq_w // tile
    if split == "overlap":
        return patch_grid(lq_h, lq_w, tile, overlap)
    raise ValueError(f"split {split!r}")


def stitch_images(tiles: torch.Tensor, n_images: int, lq_hw: Tuple[int, int], split: str = "nonoverlap",
                  tile: int = 128, overlap: int = 16) -> torch.Tensor:
    """All restored tiles of n_images images (image-major, raster order inside an image; scale 4) ->
    (n_images, C, H', W'): non-overlap placement (H' = 4 * rows * tile) or the device overlap-blend
    merge (H' = 4 * lq_h, val_patches.py:114-206 with the LQ size as original_size)."""
    rows, cols = image_tile_grid(lq_hw[0], lq_hw[1], split, tile, overlap)
    per = rows * cols
    assert tiles.shape[0] == n_images * per, (tiles.shape, n_images, per)
    outs = []
    for k in range(n_images):
        t = tiles[k * per:(k + 1) * per]
        if split == "nonoverlap":
            outs.append(stitch_nonoverlap(t, rows, cols))
        else:
            outs.append(merge_patches_with_overlap_device(t, lq_hw, patch_size=4 * tile, overlap=4 * overlap,
                                                          lq_patch=tile, lq_overlap=overlap))
    return torch.cat(outs)


# ---------------------------------------------------------------------------------------------------
# latent tiling inside the sampling loop (utils/common.py:125-234)
# ---------------------------------------------------------------------------------------------------
def _starts(n: int, size: int, stride: int) -> List[int]:
    out = list(range(0, n - size + 1, stride))
    if (n - size) % stride != 0:  # the last window is appended flush with the edge
        out.append(n - size)
    return out


def sliding_windows(h: int, w: int, size: int, stride: int) -> List[Tuple[int, int, int, int]]:
    """utils/common.py:125-140: (y0, y1, x0, x1) of every size x size window, row-major."""
    return [(y, y + size, x, x + size) for y in _starts(h, size, stride) for x in _starts(w, size, stride)]


def gaussian_weights(tile_width: int, tile_height: int) -> np.ndarray:
    """utils/common.py:144-171: float64 [tile_height, tile_width] blend weights, var = 0.01.  The column
    midpoint is (width - 1) / 2 and the row midpoint height / 2: the reference's asymmetry is kept."""
    var = 0.01
    norm = np.sqrt(2 * np.pi * var)
    mx = (tile_width - 1) / 2
    xp = [np.exp(-(x - mx) * (x - mx) / (tile_width * tile_width) / (2 * var)) / norm for x in range(tile_width)]
    my = tile_height / 2
    yp = [np.exp(-(y - my) * (y - my) / (tile_height * tile_height) / (2 * var)) / norm for y in range(tile_height)]
    return np.outer(yp, xp)


def plan_latent_tiles(B: int, H: int, W: int, size: int, stride: int, max_batch: int, guided: bool) -> Dict:
    """The rows one tiled sampler step runs: N = B * T window rows (image-major, then window order) in
    n_chunks forwards of rows_per_chunk rows each (x 2 when guided: cond rows, then uncond rows).  All chunks
    have the same row count, so the network runs at one batch size with one set of plans; the `pad` unused
    rows of the last chunk repeat the job's last window and are never blended."""
    if stride < 1:
        raise ValueError(f"tile stride {stride} must be >= 1")
    if H < size or W < size:
        raise ValueError(f"latent {H}x{W} is smaller than the tile {size}")
    cap = max_batch // 2 if guided else max_batch
    if cap < 1:
        raise ValueError(f"max_batch {max_batch} leaves no room for a {'guided ' if guided else ''}window row")
    windows = sliding_windows(H, W, size, stride)
    n = B * len(windows)
    n_chunks = -(-n // cap)
    rows_per_chunk = -(-n // n_chunks)
    return dict(windows=windows, rows=n, cap=cap, n_chunks=n_chunks, rows_per_chunk=rows_per_chunk,
                pad=n_chunks * rows_per_chunk - n)


# ---------------------------------------------------------------------------------------------------
# tiled cleaner (utils/common.py:174-234 make_tiled_fn as pipeline.py:371-397 wraps the cleaner in it)
# ---------------------------------------------------------------------------------------------------
def plan_image_tiles(B: int, H: int, W: int, size: int, stride: int, max_batch: int) -> Dict:
    """The rows one tiled cleaner call runs: plan_latent_tiles without guidance on an image of H x W pixels, plus
    `chunks`, the (first job row, job rows) of every forward (the last one is `pad` rows short of rows_per_chunk)."""
    if size < 1 or size % 64 != 0:
        raise ValueError(f"SwinIR (cleaner) tile size {size} must be a multiple of 64")
    if H < size or W < size:
        raise ValueError(f"image {H}x{W} is smaller than the tile {size}")
    plan = plan_latent_tiles(B, H, W, size, stride, max_batch, guided=False)
    rpc, n = plan["rows_per_chunk"], plan["rows"]
    plan["chunks"] = [(c * rpc, min(rpc, n - c * rpc)) for c in range(plan["n_chunks"])]
    return plan


def make_tiled_fn(fn, size: int, stride: int):
    """utils/common.py:174-234 in the form pipeline.py:389-394 uses (scale 1, Gaussian weights): fn runs on every
    size x size window of x [B, C, H, W] (all images of the batch at once, windows in sliding_windows order), each
    output is multiplied by the fp32 Gaussian weights and added into an fp32 accumulator, the weights into a second
    one, and the result is their quotient.  Stock torch, on x's device; for cleaners that are ordinary modules."""
    if stride < 1:
        raise ValueError(f"tile stride {stride} must be >= 1")

    def tiled_fn(x: torch.Tensor) -> torch.Tensor:
        b, c, h, w = x.shape
        if h < size or w < size:
            raise ValueError(f"image {h}x{w} is smaller than the tile {size}")
        out = torch.zeros((b, c, h, w), dtype=torch.float32, device=x.device)
        count = torch.zeros_like(out)
        weights = torch.tensor(gaussian_weights(size, size)[None, None], dtype=torch.float32, device=x.device)
        for y0, y1, x0, x1 in sliding_windows(h, w, size, stride):
            out[..., y0:y1, x0:x1] += fn(x[..., y0:y1, x0:x1]) * weights
            count[..., y0:y1, x0:x1] += weights
        return out / count
    return tiled_fn
