"""Time the CLIP-H text tower: graph-replayed stock torch (fp32) vs graph-replayed HIP tower (clip_hip.py).

python tools/clip_bench.py [--reps 30] [--rounds 5] [--no-stage3] [--stage3-steps 6]

The full tower (24 layers, width 1024, penultimate, random weights: bench.py stage3_models) at B = 1 and B = 8.  Both
towers are captured by testr.GraphedTextEncoder and their graphs replayed alternately in one process, `rounds` times
`reps` replays each, timed with device events; the figure is the median round's time per replay.  Floors: the HIP
tower streams 0.58 GB of bf16 weights per encode (~105 us at the 5.5 TB/s weight-stream rate of DESIGN.md §7), the
stock fp32 tower twice that.  --stage3 (default) adds one paired configs[4]-style step time per backend: val_sample
(fp8 layer set, full-size TESTR) with text_encoder= each tower, alternating, one untimed capture run first.
One JSON line per measurement.
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WEIGHT_RATE = 5.5e12  # bytes/s, DESIGN.md §7


def replay_us(entries, reps, rounds):
    """entries: {name: CUDAGraph}; alternating rounds of `reps` replays; median round, us per replay."""
    times = {k: [] for k in entries}
    for _ in range(rounds):
        for name, g in entries.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            g.replay()
            e0.record()
            for _ in range(reps):
                g.replay()
            e1.record()
            e1.synchronize()
            times[name].append(e0.elapsed_time(e1) * 1e3 / reps)
    return {k: statistics.median(v) for k, v in times.items()}, times


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--no-stage3", action="store_true")
    ap.add_argument("--stage3-steps", type=int, default=6)
    a = ap.parse_args()
    import bench
    from tair_amd.clip_hip import HipTextTower
    from tair_amd.testr import GraphedTextEncoder
    torch.backends.cuda.matmul.allow_tf32 = False
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    det, stock_enc = bench.stage3_models(dev)
    stock = stock_enc.tower
    hip = HipTextTower(stock, max_batch=8, device=dev)
    hip_enc = GraphedTextEncoder(hip, stock_enc.tokenize)
    bf16_bytes = sum(getattr(hip, n)[:hip.layers - hip.layer_idx].numel() * 2 for n in ("w_qkv", "w_out", "w_fc", "w_proj"))
    prompt = 'A realistic scene where the texts "OPEN", "24", "HOURS" appear clearly on signs, boards, buildings.'
    for B in (1, 8):
        texts = [prompt] * B if B > 1 else prompt
        with torch.no_grad():
            ys, yh = stock_enc(texts), hip_enc(texts)  # captures
        torch.cuda.synchronize()
        err = ((yh.double() - ys.double()).norm() / ys.double().norm()).item()
        shape = (B, 77)
        med, allr = replay_us({"stock": stock_enc._graphs[shape][0], "hip": hip_enc._graphs[shape][0]}, a.reps, a.rounds)
        hip.check_faults()
        print(json.dumps({
            "what": "text tower graph replay", "batch": B, "layers_run": hip.layers - hip.layer_idx, "width": hip.width,
            "stock_fp32_us": round(med["stock"], 1), "hip_us": round(med["hip"], 1),
            "stock_over_hip": round(med["stock"] / med["hip"], 3),
            "rounds_us": {k: [round(t, 1) for t in v] for k, v in allr.items()},
            "hip_launches": hip.launch_count(B), "hip_weight_bytes": bf16_bytes,
            "hip_weight_floor_us": round(bf16_bytes / WEIGHT_RATE * 1e6, 1),
            "stock_weight_floor_us": round(2 * bf16_bytes / WEIGHT_RATE * 1e6, 1),
            "hip_vs_stock_rel_l2": float(f"{err:.3e}")}), flush=True)
    if a.no_stage3:
        return
    # one configs[4]-style step per backend: bench.py's model and loop, text_encoder= swapped
    from tair_amd.cldm import ControlLDM
    from tair_amd.diffusion import Diffusion
    from tair_amd.pipeline import synthetic_context, synthetic_tiles
    from tair_amd.sampler import SpacedSampler
    from tair_amd.weights import manifest, synthetic_state_dict
    S = a.stage3_steps
    model = ControlLDM(max_batch=1, device=dev, fp8=True, with_vae=False)
    model.load_state_dict(synthetic_state_dict(manifest(), seed=0))
    sampler = SpacedSampler(Diffusion(linear_start=0.00085, linear_end=0.012, zero_snr=True,
                                      parameterization="v").betas, "v", False)
    x_T, noise, c_img = (t.to(dev) for t in synthetic_tiles(range(1), S))
    cond = {"c_txt": synthetic_context().to(dev), "c_img": c_img}
    ms = {"stock": [], "hip": []}
    for rnd in range(1 + a.rounds):  # round 0 captures the graphs (untimed)
        for name, enc in (("stock", stock_enc), ("hip", hip_enc)):
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            with torch.no_grad():
                _, res = sampler.val_sample(model, dev, S, tuple(x_T.shape), dict(cond), x_T=x_T, noise=noise,
                                            ts_model=det, text_encoder=enc, prompt_style="CAPTION")
            torch.cuda.synchronize(dev)
            if rnd:
                ms[name].append((time.perf_counter() - t0) / S * 1e3)
    s, h = statistics.median(ms["stock"]), statistics.median(ms["hip"])
    print(json.dumps({
        "what": "configs[4]-style stage-3 step (val_sample, fp8 layer set, B = 1), ms per step", "steps": S,
        "stock_ms": round(s, 3), "hip_ms": round(h, 3), "removed_ms": round(s - h, 3),
        "removed_share": round((s - h) / s, 4), "rounds_ms": {k: [round(t, 3) for t in v] for k, v in ms.items()},
        "words_per_step": [len(r["pred_texts"]) for r in res]}), flush=True)


if __name__ == "__main__":
    main()
