"""TEST INFRASTRUCTURE ONLY -- the fp32 reference loop of latent tiling inside the sampling loop
(utils/common.py:125-234 make_tiled_fn wired as in ddim_sampler.py:165-180, spaced_sampler.py:149-164), restated
for the GPU tests of the fused tiled sampler: per step the model runs on every overlapping window of the whole
latent (its hint is the same window of c_img, the context is shared), the outputs are blended with Gaussian
weights in fp32 in ascending window order, guidance combines the blended halves, and p_sample updates the whole
latent.  The model is oracle.ldm_ref.ControlLDMRef; the update and the guidance scale are oracle.sampler_ref's.

The windows and weights are restated here too, independently of tair_amd.tiling.
"""
import math

import numpy as np
import torch

from oracle.sampler_ref import SpacedScheduleRef, cfg_scale_ref, diffusion_betas, p_sample_v


def windows_ref(h, w, size, stride):
    def starts(n):
        s = list(range(0, n - size + 1, stride))
        if (n - size) % stride != 0:
            s.append(n - size)
        return s
    return [(y, y + size, x, x + size) for y in starts(h) for x in starts(w)]


def weights_ref(size):
    """float64 [size, size]: var 0.01, column midpoint (size - 1) / 2, row midpoint size / 2."""
    var = 0.01
    col = [math.exp(-(x - (size - 1) / 2) ** 2 / (size * size) / (2 * var)) / math.sqrt(2 * math.pi * var)
           for x in range(size)]
    row = [math.exp(-(y - size / 2) ** 2 / (size * size) / (2 * var)) / math.sqrt(2 * math.pi * var)
           for y in range(size)]
    return np.outer(np.asarray(row, dtype=np.float64), np.asarray(col, dtype=np.float64))


def blend_ref(outs, wins, shape, w):
    """acc += v_k * w, cnt += w over the windows in order, then acc / cnt, in the dtype of `w`.
    outs[k]: [B, C, size, size] output of window k."""
    acc = torch.zeros(shape, dtype=w.dtype, device=w.device)
    cnt = torch.zeros(shape, dtype=w.dtype, device=w.device)
    for v, (y0, y1, x0, x1) in zip(outs, wins):
        acc[..., y0:y1, x0:x1] += v.to(w.dtype) * w
        cnt[..., y0:y1, x0:x1] += w
    return acc / cnt


@torch.no_grad()
def tiled_model_ref(model, x, model_t, cond, size, stride):
    wins = windows_ref(x.shape[2], x.shape[3], size, stride)
    w = torch.from_numpy(weights_ref(size)).to(device=x.device, dtype=torch.float32)
    outs = []
    for (y0, y1, x0, x1) in wins:
        c = {"c_txt": cond["c_txt"].expand(x.shape[0], -1, -1)}
        if cond.get("c_img") is not None:
            c["c_img"] = cond["c_img"][..., y0:y1, x0:x1].contiguous()
        outs.append(model(x[..., y0:y1, x0:x1].contiguous(), model_t, c)[0])
    return blend_ref(outs, wins, x.shape, w)


@torch.no_grad()
def sample_tiled_ref(model, steps, x_T, cond, noise, size, stride, uncond=None, cfg_scale=1.0, trace=None):
    """The whole tiled loop -> x_0 [B, 4, H, W]; trace (optional list) receives (x_t, v) per step."""
    sched = SpacedScheduleRef(diffusion_betas(), steps)
    x = x_T
    ts = np.flip(sched.timesteps)
    for i, cur in enumerate(ts):
        mt = torch.full((x.shape[0],), int(cur), dtype=torch.long, device=x.device)
        v = tiled_model_ref(model, x, mt, cond, size, stride)
        if uncond is not None and cfg_scale != 1.0:
            vu = tiled_model_ref(model, x, mt, uncond, size, stride)
            v = vu + cfg_scale_ref(cfg_scale, int(cur), False) * (v - vu)
        if trace is not None:
            trace.append((x, v))
        x = p_sample_v(sched, x, v, steps - i - 1, noise[i])
    return x
