#!/usr/bin/env python
"""Guided (classifier-free guidance) sampling: the fused step graph against the host loop.

Workload: full-width synthetic weights, one 512^2 tile (B = 1, max_batch = 2, 64^2 latent, ControlNet on),
50 steps, cfg_scale = 4, explicit noise.  Two paths compute the same restoration:

* host   `SpacedSampler._sample_cfg`: per step two eager B = 1 forwards + torch elementwise ops
* fused  `SpacedSampler.sample(uncond=..., cfg_scale=4)`: per step one replay of the captured step graph
         at batch 2 with the guided update kernel (includes the per-restoration prepare)

Method: one warm-up restoration per path (code objects, graph capture), then `--pairs` alternating
(host, fused) pairs, each restoration timed with a host clock around work that ends in a device
synchronise; the figure is ms per step = restoration time / steps; medians over the pairs.  The unguided
fused step (B = 1) is timed the same way for scale.  `--path host` runs the host loop alone (it needs
nothing newer than `_sample_cfg`, so it also runs on older checkouts); `--path fused` the fused path alone.

    python tools/cfg_bench.py [--path both|host|fused] [--pairs 5] [--steps 50] [--log profiles/cfg_bench.jsonl]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--path", choices=["both", "host", "fused"], default="both")
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--cfg-scale", type=float, default=4.0)
    ap.add_argument("--log", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("cfg_bench: no GPU (a timing needs the device; there is no CPU fallback)")
    from tair_amd.cldm import ControlLDM
    from tair_amd.diffusion import Diffusion
    from tair_amd.sampler import SpacedSampler
    from tair_amd.weights import manifest, perturb_norms, synthetic_state_dict
    m = ControlLDM(max_batch=2, with_vae=False)
    m.load_state_dict(perturb_norms(synthetic_state_dict(manifest(), seed=0)))
    g = torch.Generator().manual_seed(3)
    x = torch.randn(1, 4, 64, 64, generator=g).cuda()
    c_img = torch.randn(1, 4, 64, 64, generator=g).cuda()
    cond = {"c_txt": torch.randn(1, 77, 1024, generator=g).cuda(), "c_img": c_img}
    uncond = {"c_txt": torch.randn(1, 77, 1024, generator=g).cuda(), "c_img": c_img}
    noise = torch.randn(a.steps, 1, 4, 64, 64, generator=g).cuda()
    s = SpacedSampler(Diffusion(linear_start=0.00085, linear_end=0.012, zero_snr=True, parameterization="v").betas,
                      "v", False)

    def host():
        return s._sample_cfg(m, a.steps, x, cond, uncond, a.cfg_scale, noise)[0]

    def fused():
        z = s.sample(m, "cuda", a.steps, x.shape, cond, uncond=uncond, cfg_scale=a.cfg_scale, x_T=x, noise=noise)[0]
        if getattr(s, "last_guided_fused", None) is not True:
            sys.exit("cfg_bench: sample() did not take the fused guided path")
        return z

    def unguided():
        return s.sample(m, "cuda", a.steps, x.shape, cond, x_T=x, noise=noise)[0]

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        z = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / a.steps, z

    paths = {"host": host, "fused": fused}
    run = ["host", "fused"] if a.path == "both" else [a.path]
    log = []

    def emit(rec):
        print(json.dumps(rec), flush=True)
        log.append(rec)

    with torch.no_grad():
        outs = {p: timed(paths[p])[1] for p in run}  # warm-up
        timed(unguided)
        if len(run) == 2:  # faster and different is not faster: the two paths compute the same restoration
            d = ((outs["fused"].double() - outs["host"].double()).norm() / outs["host"].double().norm()).item()
            emit(dict(kind="agreement", rel_l2_fused_vs_host=d))
        ms = {p: [] for p in run}
        ung = []
        for i in range(a.pairs):
            rec = dict(kind="pair", pair=i)
            for p in run:
                t, _ = timed(paths[p])
                ms[p].append(t)
                rec[f"{p}_ms_per_step"] = round(t, 4)
            t, _ = timed(unguided)
            ung.append(t)
            rec["unguided_ms_per_step"] = round(t, 4)
            emit(rec)
    out = dict(kind="result", workload=f"B=1 512^2 tile, {a.steps} steps, cfg_scale {a.cfg_scale}, full width",
               pairs=a.pairs, unguided_ms_per_step=round(statistics.median(ung), 4))
    for p in run:
        out[f"{p}_ms_per_step"] = round(statistics.median(ms[p]), 4)
    if len(run) == 2:
        out["host_over_fused"] = round(out["host_ms_per_step"] / out["fused_ms_per_step"], 3)
        out["fused_faster_in_every_pair"] = all(f < h for f, h in zip(ms["fused"], ms["host"]))
    emit(out)
    if a.log:
        os.makedirs(os.path.dirname(os.path.abspath(a.log)), exist_ok=True)
        with open(a.log, "w") as f:
            for rec in log:
                f.write(json.dumps(rec) + "\n")
    m.close()
    if len(run) == 2 and not out["fused_faster_in_every_pair"]:
        sys.exit(2)


if __name__ == "__main__":
    main()
