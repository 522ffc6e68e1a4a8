"""Time the VAE decode paths on one GPU: HIP split-precision decoder vs stock torch fp32 / bf16.

python tools/vae_bench.py [--batch 1] [--reps 5] [--latent 64] [--tiled --tile-size 64] [--hip-only]

--latent N decodes an N x N latent (an 8N x 8N image); --tiled runs HipVAEDecoder.decode_tiled with --tile-size latent
pixels (the reference's tiled VAE: tile-local attention, merged GroupNorm statistics) instead of decode.  hip_peak_gb
is torch.cuda.max_memory_allocated over the HIP leg (the decoder's weights and workspace included).
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--latent", type=int, default=64)
    ap.add_argument("--tiled", action="store_true")
    ap.add_argument("--tile-size", type=int, default=64)
    ap.add_argument("--hip-only", action="store_true", help="skip the stock-torch legs")
    a = ap.parse_args()
    from tair_amd.pipeline import vae_synthetic_state_dict
    from tair_amd.vae import AutoencoderKL
    from tair_amd.vae_hip import HipVAEDecoder
    torch.backends.cudnn.allow_tf32 = False
    vae = AutoencoderKL().cuda().eval()
    vae.load_state_dict(vae_synthetic_state_dict(vae, seed=0))
    hip = HipVAEDecoder(vae, "cuda", max_batch=a.batch)
    z = torch.randn(a.batch, 4, a.latent, a.latent, device="cuda")

    def timeit(fn):
        with torch.no_grad():
            fn()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.reps):
                fn()
            torch.cuda.synchronize()
        return (time.perf_counter() - t0) / a.reps * 1e3

    res = {"batch": a.batch, "latent": a.latent, "tiled": a.tiled}
    if a.tiled:
        res["tile_size"] = a.tile_size
    torch.cuda.reset_peak_memory_stats()
    res["hip_ms"] = timeit((lambda: hip.decode_tiled(z, a.tile_size)) if a.tiled else (lambda: hip.decode(z)))
    res["hip_peak_gb"] = torch.cuda.max_memory_allocated() / 2 ** 30
    if not a.hip_only:
        dec = (lambda: vae.decode_tiled(z, a.tile_size)) if a.tiled else (lambda: vae.decode(z))
        res["torch_fp32_ms"] = timeit(dec)
        vae.set_compute_dtype(torch.bfloat16)
        res["torch_bf16_ms"] = timeit(dec)
    print(json.dumps({k: round(v, 3) if isinstance(v, float) else v for k, v in res.items()}), flush=True)


if __name__ == "__main__":
    main()
