"""Time the SwinIR cleaner: stock torch (fp32, eager) vs the HIP backend eager vs the HIP backend's graph replay.

python tools/swinir_bench.py [--reps 10] [--rounds 5] [--log profiles/swinir_hip_bench.log]

The val-config network (config.SWINIR_VAL_PARAMS, build_swinir's synthetic weights) on 512^2 inputs at B = 1 and
B = 4.  The three forms run alternately in one process, `rounds` times `reps` forwards each, timed with device
events after a warm-up; the figure is the median round's time per forward.  Eager forms include their host launch
overhead (the stock module issues on the order of a thousand small launches), the graph replay does not.  The HIP
figures include the boundary torch ops (mean, pixel-unshuffle, hi / lo split, NHWC -> NCHW).  One JSON line per batch
size, printed and appended to the log.

python tools/swinir_bench.py --tiled [--size 1024 --tile-size 512 --tile-stride 256] [--log profiles/swinir_tiled_bench.log]

The tiled cleaner over one size^2 image in four forms, timed the same way: the host loop of tiling.make_tiled_fn over
the stock module, the same host loop over HipSwinIR.forward (one window per forward, torch blend), and
HipSwinIR.forward_tiled eager and replayed from one graph.  For each form also torch.cuda.max_memory_allocated over one
call, as the peak and as its increase over what was resident before the call.  One JSON line.
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


def peak_mib(fn, dev):
    """(peak, increase over what was resident before the call) of torch.cuda.max_memory_allocated over one call, MiB."""
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(dev)
    before = torch.cuda.memory_allocated(dev)
    fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated(dev)
    return round(peak / 2 ** 20, 1), round((peak - before) / 2 ** 20, 1)


def tiled(a, stock, hip, dev):
    """One JSON line: the tiled cleaner over a size^2 image, B = 1, in four forms."""
    from tair_amd.tiling import make_tiled_fn
    x = torch.rand((1, 3, a.size, a.size), generator=torch.Generator().manual_seed(1)).to(dev)
    stock_loop = make_tiled_fn(stock, a.tile_size, a.tile_stride)   # the host loop over the stock module
    hip_loop = make_tiled_fn(hip, a.tile_size, a.tile_stride)       # the same loop over HipSwinIR.forward, torch blend
    with torch.no_grad():
        ys, yl, yt = stock_loop(x), hip_loop(x), hip.forward_tiled(x, a.tile_size, a.tile_stride)  # warm-up
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            yg = hip.forward_tiled(x, a.tile_size, a.tile_stride)
        graph.replay()
    torch.cuda.synchronize()
    rel = lambda p, q: ((p.double() - q.double()).norm() / q.double().norm()).item()  # noqa: E731

    def run_stock():
        with torch.no_grad():
            stock_loop(x)
    fns = {"stock_loop": run_stock, "hip_loop": lambda: hip_loop(x),
           "forward_tiled_eager": lambda: hip.forward_tiled(x, a.tile_size, a.tile_stride),
           "forward_tiled_graph": graph.replay}
    mem = {k: peak_mib(fn, dev) for k, fn in fns.items()}
    med, allr = time_ms(fns, a.reps, a.rounds)
    hip.check_faults()
    plan = hip.last_tiling
    return json.dumps({
        "what": f"tiled SwinIR cleaner, val config, {a.size}^2, tile {a.tile_size}, stride {a.tile_stride}", "batch": 1,
        "device": torch.cuda.get_device_name(dev), "windows": plan["rows"], "chunks": plan["n_chunks"],
        "rows_per_chunk": plan["rows_per_chunk"], "pad": plan["pad"],
        "ms": {k: round(v, 3) for k, v in med.items()},
        "hip_loop_over_forward_tiled_eager": round(med["hip_loop"] / med["forward_tiled_eager"], 2),
        "hip_loop_over_forward_tiled_graph": round(med["hip_loop"] / med["forward_tiled_graph"], 2),
        "stock_loop_over_forward_tiled_graph": round(med["stock_loop"] / med["forward_tiled_graph"], 2),
        "rounds_ms": {k: [round(t, 3) for t in v] for k, v in allr.items()},
        "peak_mib": {k: v[0] for k, v in mem.items()}, "peak_increase_mib": {k: v[1] for k, v in mem.items()},
        "graph_bitwise_eager": bool(torch.equal(yg, yt)),
        "forward_tiled_vs_hip_loop_max_abs": float(f"{(yt - yl).abs().max().item():.3e}"),
        "forward_tiled_vs_stock_loop_rel_l2": float(f"{rel(yt, ys):.3e}"),
        "hip_loop_vs_stock_loop_rel_l2": float(f"{rel(yl, ys):.3e}")})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--log", default=None)
    ap.add_argument("--tiled", action="store_true", help="time the tiled cleaner over one large image instead")
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--tile-size", type=int, default=512)
    ap.add_argument("--tile-stride", type=int, default=256)
    a = ap.parse_args()
    if a.log is None:
        a.log = os.path.join(ROOT, "profiles", "swinir_tiled_bench.log" if a.tiled else "swinir_hip_bench.log")
    from tair_amd.config import build_swinir
    torch.backends.cuda.matmul.allow_tf32 = False
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    torch.manual_seed(0)
    stock = build_swinir(None, dev)
    torch.manual_seed(0)  # (the same default-initialised biases)
    hip = build_swinir(None, dev, backend="hip", max_batch=4)
    if a.tiled:
        line = tiled(a, stock, hip, dev)
        print(line, flush=True)
        os.makedirs(os.path.dirname(a.log), exist_ok=True)
        with open(a.log, "a") as f:
            f.write(line + "\n")
        return
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
