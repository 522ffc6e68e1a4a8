#!/usr/bin/env python
"""FF-out composed with proj_out: paired A/B of the product library against the variant library
that keeps the two launches at every shape.

The variant is the same sources with one compile-time macro (no runtime switch in the product library):

    python -m tair_amd.build --variant noffpout -D TAIR_NO_FFPOUT

Each run is `bench.py` itself (default workload: B = 1, 512^2, 50 steps, VAE decode included; `--config 2` for the
batched configs[2]) in a FRESH child process, the library selected by TAIR_LIB_VARIANT in the child's environment;
the runs alternate (variant, product), the order swapped from pair to pair, for `--pairs` pairs on one box
(`--variant NAME`: the same A/B against another baseline build, e.g. nokgroup = -DTAIR_NO_KGROUP).  One JSON line per run goes to `--log`, then a
summary line: per-pair gain, median gain, and the spread (max - min) of the variant's own runs, the noise the gain has
to clear.  `--finalize` instead times tair_cldm_finalize of the full-width model once per library (fresh children).

    python tools/ffpout_bench.py [--pairs 5] [--steps 20] [--warmup 5] [--config 1] [--log profiles/ffpout_bench_pairs.jsonl]
    python tools/ffpout_bench.py --finalize [--log ...]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VARIANT = "noffpout"


def child_env(variant: str):
    env = dict(os.environ)
    env.pop("TAIR_LIB_VARIANT", None)
    if variant:
        env["TAIR_LIB_VARIANT"] = variant
    return env


def run_bench(variant: str, a) -> dict:
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(a.steps), "--warmup", str(a.warmup)]
    if a.config != 1:
        cmd += ["--config", str(a.config)]
    t0 = time.time()
    r = subprocess.run(cmd, cwd=ROOT, env=child_env(variant), capture_output=True, text=True, timeout=a.timeout)
    if r.returncode != 0:
        sys.stderr.write(r.stderr[-4000:])
        sys.exit(f"ffpout_bench: bench.py failed with status {r.returncode} (library: {variant or 'product'})")
    rec = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    bd = rec.get("breakdown_ms") or {}  # (only a --full bench splits the step from the decode)
    return dict(kind="run", lib=variant or "product", config=a.config, value=rec["value"], unit=rec["unit"],
                ms_per_step=rec.get("ms_per_step"), denoise_step_ms=bd.get("per_denoise_step_per_micro_batch"),
                vae_decode_ms=bd.get("vae_decode"), steps=a.steps, warmup=a.warmup, wall_s=round(time.time() - t0, 1))


FINALIZE_CHILD = r"""
import json, sys, time
sys.path.insert(0, sys.argv[1])
import torch
from tair_amd.cldm import ControlLDM
from tair_amd.weights import manifest, perturb_norms, synthetic_state_dict
m = ControlLDM(max_batch=1, with_vae=False)
sd = perturb_norms(synthetic_state_dict(manifest(), seed=0))
t0 = time.perf_counter()
for k, v in sd.items():
    m._load_one(k, v)
t1 = time.perf_counter()
m.finalize()
torch.cuda.synchronize()
t2 = time.perf_counter()
pk = next(k for k in sd if k.endswith(".1.proj_out.weight"))
m._load_one(pk, sd[pk])
t3 = time.perf_counter()
m.finalize()  # a partial reload: one proj_out weight
torch.cuda.synchronize()
t4 = time.perf_counter()
print(json.dumps(dict(load_params_s=round(t1 - t0, 3), finalize_s=round(t2 - t1, 3), refinalize_one_proj_out_s=round(t4 - t3, 3))))
m.close()
"""


def run_finalize(variant: str, a) -> dict:
    r = subprocess.run([sys.executable, "-c", FINALIZE_CHILD, ROOT], cwd=ROOT, env=child_env(variant), capture_output=True,
                       text=True, timeout=a.timeout)
    if r.returncode != 0:
        sys.stderr.write(r.stderr[-4000:])
        sys.exit(f"ffpout_bench: finalize timing failed with status {r.returncode} (library: {variant or 'product'})")
    rec = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    return dict(kind="finalize", lib=variant or "product", model="full width, max_batch 1", **rec)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--config", type=int, default=1, choices=[1, 2])
    ap.add_argument("--finalize", action="store_true")
    ap.add_argument("--timeout", type=int, default=900, help="seconds per child")
    ap.add_argument("--log", default="")
    ap.add_argument("--variant", default=VARIANT, help="the baseline variant library (another paired A/B of the same "
                    "kind, e.g. nokgroup: python -m tair_amd.build --variant nokgroup -D TAIR_NO_KGROUP)")
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    from tair_amd import build
    variant = a.variant
    if not os.path.exists(build.variant_lib(variant)):
        sys.exit(f"ffpout_bench: {build.variant_lib(variant)} not built "
                 f"(python -m tair_amd.build --variant {variant} -D <the macro that makes it the baseline>, e.g. "
                 "noffpout: TAIR_NO_FFPOUT, nokgroup: TAIR_NO_KGROUP)")
    build.ensure_built()
    hashes = dict(product=build.library_hash(), **{variant: build.library_hash(build.variant_lib(variant))})
    log = open(a.log, "a") if a.log else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if log:
            log.write(line + "\n")
            log.flush()

    if a.finalize:
        for v in (variant, ""):
            emit(dict(run_finalize(v, a), srchash=hashes[v or "product"]))
        return
    runs = {variant: [], "product": []}
    for i in range(a.pairs):
        for v in ((variant, "") if i % 2 == 0 else ("", variant)):  # the order alternates from pair to pair
            rec = dict(run_bench(v, a), pair=i, srchash=hashes[v or "product"])
            runs[v or "product"].append(rec["value"])
            emit(rec)
    gains = [p / q - 1.0 for p, q in zip(runs["product"], runs[variant])]
    base = runs[variant]
    spread = (max(base) - min(base)) / statistics.median(base)
    emit(dict(kind="summary", config=a.config, pairs=a.pairs, unit="Mpix/s",
              product_median=round(statistics.median(runs["product"]), 4), variant_median=round(statistics.median(base), 4),
              gain_per_pair=[round(g, 4) for g in gains], median_gain=round(statistics.median(gains), 4),
              variant_spread=round(spread, 4), product_faster_in_every_pair=all(g > 0 for g in gains),
              median_gain_exceeds_variant_spread=statistics.median(gains) > spread))


if __name__ == "__main__":
    main()
