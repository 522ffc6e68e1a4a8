"""TEST INFRASTRUCTURE ONLY -- the reference loop of the tiled cleaner (utils/common.py:174-234 make_tiled_fn as
pipeline.py:389-394 wraps the cleaner in it: scale 1, Gaussian weights, fp32 accumulators), restated for the tests of
tair_amd.tiling.make_tiled_fn, the image-tile kernels and HipSwinIR.forward_tiled.  The windows, the weights and the
blend are tests/_tiled_ref.py's (themselves restated independently of tair_amd.tiling); this adds the loop over a
cleaner and the job-row bookkeeping of the chunked form.
"""
import torch

from tests._tiled_ref import blend_ref, weights_ref, windows_ref


def weights32(size, device="cpu"):
    """The fp32 weights the reference multiplies by: the float64 table rounded once."""
    return torch.tensor(weights_ref(size), dtype=torch.float32, device=device)


@torch.no_grad()
def tiled_ref(fn, x, size, stride):
    """fn on every window of x [B, C, H, W] (the whole batch at once), blended in window order in fp32."""
    wins = windows_ref(x.shape[2], x.shape[3], size, stride)
    outs = [fn(x[..., y0:y1, x0:x1]) for (y0, y1, x0, x1) in wins]
    return blend_ref(outs, wins, x.shape, weights32(size, outs[0].device))


def job_rows(B, H, W, size, stride):
    """(b, (y0, y1, x0, x1)) of job row j = b * T + k, image-major."""
    wins = windows_ref(H, W, size, stride)
    return [(b, win) for b in range(B) for win in wins]


def blend_rows_ref(rows_out, B, H, W, size, stride):
    """The reference blend of per-job-row outputs rows_out[j] [C, size, size] (fp32, CPU): window k's output is the
    stack over the images of rows b * T + k, as the reference's call on the whole batch returns it."""
    wins = windows_ref(H, W, size, stride)
    T = len(wins)
    outs = [torch.stack([rows_out[b * T + k] for b in range(B)]) for k in range(T)]
    return blend_ref(outs, wins, (B, outs[0].shape[1], H, W), weights32(size))


def cover_counts(H, W, size, stride):
    """[H, W] int: how many windows cover each pixel."""
    n = torch.zeros(H, W, dtype=torch.int64)
    for y0, y1, x0, x1 in windows_ref(H, W, size, stride):
        n[y0:y1, x0:x1] += 1
    return n
