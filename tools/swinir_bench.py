"""Time the SwinIR cleaner: stock torch (fp32, eager) vs the HIP backend eager vs the HIP backend's graph replay.

python tools/swinir_bench.py [--reps 10] [--rounds 5] [--log profiles/swinir_hip_bench.log]

The val-config network (config.SWINIR_VAL_PARAMS, build_swinir's synthetic weights) on 512^2 inputs at B = 1 and
B = 4.  The three forms run alternately in one process, `rounds` times `reps` forwards each, timed with device
events after a warm-up; the figure is the median round's time per forward.  Eager forms include their host launch
overhead (the stock module issues on the order of a thousand small launches), the graph replay does not.  The HIP
figures include the boundary torch ops (mean, pixel-unshuffle, hi / lo split, NHWC -> NCHW).  One JSON line per batch
size, printed and appended to the log.
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def time_ms(fns, reps, rounds):
    """fns: {name: callable}; alternating rounds of `reps` calls; median round, ms per call."""
    times = {k: [] for k in fns}
    for _ in range(rounds):
        for name, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            fn()
            e0.record()
            for _ in range(reps):
                fn()
            e1.record()
            e1.synchronize()
            times[name].append(e0.elapsed_time(e1) / reps)
    return {k: statistics.median(v) for k, v in times.items()}, times


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "swinir_hip_bench.log"))
    a = ap.parse_args()
    from tair_amd.config import build_swinir
    torch.backends.cuda.matmul.allow_tf32 = False
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    torch.manual_seed(0)
    stock = build_swinir(None, dev)
    torch.manual_seed(0)  # (the same default-initialised biases)
    hip = build_swinir(None, dev, backend="hip", max_batch=4)
    lines = []
    for B in (1, 4):
        x = torch.rand((B, 3, 512, 512), generator=torch.Generator().manual_seed(B)).to(dev)
        with torch.no_grad():
            ys, yh = stock(x), hip(x)  # warm-up: plans, first-use setup
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                yg = hip(x)
            graph.replay()
        torch.cuda.synchronize()
        err = ((yh.double() - ys.double()).norm() / ys.double().norm()).item()

        def run_stock():
            with torch.no_grad():
                stock(x)
        med, allr = time_ms({"stock": run_stock, "hip_eager": lambda: hip(x), "hip_graph": graph.replay}, a.reps, a.rounds)
        hip.check_faults()
        lines.append(json.dumps({
            "what": "SwinIR cleaner, val config, 512^2", "batch": B, "device": torch.cuda.get_device_name(dev),
            "stock_fp32_eager_ms": round(med["stock"], 3), "hip_eager_ms": round(med["hip_eager"], 3),
            "hip_graph_ms": round(med["hip_graph"], 3), "stock_over_hip_eager": round(med["stock"] / med["hip_eager"], 2),
            "stock_over_hip_graph": round(med["stock"] / med["hip_graph"], 2),
            "rounds_ms": {k: [round(t, 3) for t in v] for k, v in allr.items()},
            "hip_launches": hip.launch_count(B), "graph_bitwise_eager": bool(torch.equal(yg, yh)),
            "hip_vs_stock_rel_l2": float(f"{err:.3e}"),
            "hip_vs_stock_max_abs": float(f"{(yh - ys).abs().max().item():.3e}")}))
        print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(a.log), exist_ok=True)
    with open(a.log, "a") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
