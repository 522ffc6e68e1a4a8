#!/usr/bin/env python
"""Latent tiling inside the sampling loop: the fused tiled sampler against the host loop and the untiled batch.

Workload: full-width synthetic weights, one 1024^2 image (whole latent 128 x 128, tile 64, stride 32: 9 windows),
ControlNet on, 50 steps, explicit noise, max_batch = 9 (all windows in one forward).  Three paths:

* tiled    `SpacedSampler.sample(tiled=True)`: per step one replay of the captured chunk graph (gather, the
           network at batch 9, blend + whole-latent update); includes the per-restoration prepare
* host     `SpacedSampler._sample_tiled_host`: per step torch slicing, one eager batch-9 forward, torch blending
* untiled  `SpacedSampler.sample` at batch 9 on nine independent 64 x 64 latents: the same nine forwards per step
           with no tiling work (a different result; it is the cost floor of the network itself)

Method: one warm-up restoration per path (code objects, graph capture), then `--pairs` rounds that run the
paths in alternating order, each restoration timed with a host clock around work that ends in a device
synchronise; ms per step = restoration time / steps; medians over the rounds; the spread is (max - min) / median
of each path.  Mpix/s counts the 1024^2 output pixels per restoration second.  `--chunked N` also runs the tiled
path once on a second handle with max_batch = N (N = 4: three chunks of three) to show the cost of chunking.

    python tools/tiled_bench.py [--pairs 5] [--steps 50] [--chunked 4] [--log profiles/tiled_bench_pairs.jsonl]
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

LAT, TILE, STRIDE = 128, 64, 32


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--chunked", type=int, default=4, help="max_batch of the extra chunked tiled run (0: skip)")
    ap.add_argument("--log", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("tiled_bench: no GPU (a timing needs the device; there is no CPU fallback)")
    from tair_amd.cldm import ControlLDM
    from tair_amd.diffusion import Diffusion
    from tair_amd.sampler import SpacedSampler
    from tair_amd.tiling import sliding_windows
    from tair_amd.weights import manifest, perturb_norms, synthetic_state_dict
    n_win = len(sliding_windows(LAT, LAT, TILE, STRIDE))
    sd = perturb_norms(synthetic_state_dict(manifest(), seed=0))
    m = ControlLDM(max_batch=n_win, with_vae=False)
    m.load_state_dict(sd)
    g = torch.Generator().manual_seed(3)
    x = torch.randn(1, 4, LAT, LAT, generator=g).cuda()
    cond = {"c_txt": torch.randn(1, 77, 1024, generator=g).cuda(), "c_img": torch.randn(1, 4, LAT, LAT, generator=g).cuda()}
    noise = torch.randn(a.steps, 1, 4, LAT, LAT, generator=g).cuda()
    xb = torch.randn(n_win, 4, TILE, TILE, generator=g).cuda()
    cond_b = {"c_txt": cond["c_txt"], "c_img": torch.randn(n_win, 4, TILE, TILE, generator=g).cuda()}
    noise_b = torch.randn(a.steps, n_win, 4, TILE, TILE, generator=g).cuda()
    s = SpacedSampler(Diffusion(linear_start=0.00085, linear_end=0.012, zero_snr=True, parameterization="v").betas,
                      "v", False)

    def tiled(model=m):
        return s.sample(model, "cuda", a.steps, x.shape, cond, x_T=x, noise=noise, tiled=True, tile_size=TILE,
                        tile_stride=STRIDE)[0]

    def host():
        return s._sample_tiled_host(m, a.steps, x, cond, None, 1.0, TILE, STRIDE, noise)[0]

    def untiled():
        return s.sample(m, "cuda", a.steps, xb.shape, cond_b, x_T=xb, noise=noise_b)[0]

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        z = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / a.steps, z

    paths = {"tiled": tiled, "host": host, "untiled": untiled}
    log = []

    def emit(rec):
        print(json.dumps(rec), flush=True)
        log.append(rec)

    mpix = (8 * LAT) ** 2 / 1e6
    with torch.no_grad():
        outs = {}
        for p, fn in paths.items():  # warm-up
            outs[p] = timed(fn)[1]
            if p == "tiled":
                plan = s.last_tiling
        d = ((outs["tiled"].double() - outs["host"].double()).norm() / outs["host"].double().norm()).item()
        emit(dict(kind="agreement", rel_l2_tiled_vs_host=d, plan=plan))
        ms = {p: [] for p in paths}
        order = list(paths)
        for i in range(a.pairs):
            rec = dict(kind="pair", pair=i, order=list(order))
            for p in order:
                t, _ = timed(paths[p])
                ms[p].append(t)
                rec[f"{p}_ms_per_step"] = round(t, 4)
            emit(rec)
            order = order[1:] + order[:1]  # alternate which path goes first
        out = dict(kind="result", pairs=a.pairs,
                   workload=f"1024^2 image, latent {LAT}x{LAT}, tile {TILE}, stride {STRIDE}, {n_win} windows, "
                            f"{a.steps} steps, full width, max_batch {n_win}")
        for p in paths:
            med = statistics.median(ms[p])
            out[f"{p}_ms_per_step"] = round(med, 4)
            out[f"{p}_mpix_per_s"] = round(mpix / (med * a.steps / 1e3), 4)
            out[f"{p}_spread"] = round((max(ms[p]) - min(ms[p])) / med, 4)
        out["tiled_over_untiled"] = round(out["tiled_ms_per_step"] / out["untiled_ms_per_step"], 4)
        out["host_over_tiled"] = round(out["host_ms_per_step"] / out["tiled_ms_per_step"], 4)
        emit(out)
        if a.chunked > 0:
            mc = ControlLDM(max_batch=a.chunked, with_vae=False)
            mc.load_state_dict(sd)
            timed(lambda: tiled(mc))  # warm-up
            t, zc = timed(lambda: tiled(mc))
            dc = ((zc.double() - outs["tiled"].double()).norm() / outs["tiled"].double().norm()).item()
            emit(dict(kind="chunked", max_batch=a.chunked, plan=s.last_tiling, tiled_ms_per_step=round(t, 4),
                      tiled_mpix_per_s=round(mpix / (t * a.steps / 1e3), 4), rel_l2_vs_one_chunk=dc))
            mc.close()
    if a.log:
        os.makedirs(os.path.dirname(os.path.abspath(a.log)), exist_ok=True)
        with open(a.log, "w") as f:
            for rec in log:
                f.write(json.dumps(rec) + "\n")
    m.close()


if __name__ == "__main__":
    main()
