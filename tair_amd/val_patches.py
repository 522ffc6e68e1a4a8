"""Patch-level restoration driver (reference: val_patches.py:209-380).

The reference loops over the 128^2 LQ patches of an image one at a time: bicubic x4 resize to 512^2
(`preprocess_lq`, :283-287), SwinIR clean, `prepare_condition`, a 50-step `val_sample` with
x_T = randn(1,4,64,64) from a device generator (:327-348), VAE decode + clamp((x+1)/2) (:369), then
`merge_patches_with_overlap` (:374).  Here the patch loop becomes a tile *batch*: every patch of the
image (and, under torch.distributed, only this rank's contiguous block of them) runs
through one hipGraph-replayed 50-step sampler call per micro-batch of at most `tile_batch` tiles; the
decoded tiles are all-gathered over RCCL and stitched on every rank.

Deliberate differences, each documented in DESIGN.md:
* the x4 resize is PIL's own bicubic on the host (bit-exact with the reference's torchvision Resize of a
  PIL patch), the /255 on the device;
* the overlap merge gets the LQ image size as `original_size` (the correct grid).  The reference passes
  the GT size (val_patches.py:375, 4x the LQ size), which computes a 4x wider patch grid and places a
  multi-patch image's tiles in the wrong cells (and crops to 4x the GT size); `merge_size="gt"`
  reproduces that call exactly (tests/test_val_patches_gpu.py pins both against oracle/merge_ref.py);
* SwinIR (`--swinir`, stock torch, tair_amd/swinir.py) cleans the patches when asked for; by default
  `cleaner` is identity (stock, untimed);
* stage 3 (`--config_testr`, the reference's terediff_stage3 path): every micro-batch runs
  `SpacedSampler.val_sample` with the TESTR spotter (tair_amd/testr.py, stock torch) re-prompting CLIP
  after each graph-replayed denoise step, one prompt per tile; without it the prompt is a fixed
  context tensor `c_txt` ("" through CLIP in the reference);
* x_T and the per-step noise come from a CPU generator seeded by the *global* tile id
  (`pipeline.synthetic_tiles`), so a tile's result is independent of batching and of the world size.

    python -m tair_amd.val_patches --lq path/to/lq.png --out restored.png          (real image)
    python -m tair_amd.val_patches --synthetic 256x384 --steps 50                   (synthetic LQ)
"""
from __future__ import annotations

import argparse
import time
from typing import Callable, Optional

import numpy as np
import torch
import torch.nn.functional as F

from . import dist as tdist
from .pipeline import Restorer, synthetic_tiles
from .tiling import merge_patches_with_overlap_device, patch_grid, shard_range, split_image_with_overlap

LQ_PATCH, LQ_OVERLAP, SCALE = 128, 16, 4
STAGE3_SCORE_THRESHOLD = 0.5  # models['testr'].test_score_threshold before val_sample (val_patches.py:330)


def preprocess_lq(patches: np.ndarray, device) -> torch.Tensor:
    """(N, 128, 128, 3) uint8 -> (N, 3, 512, 512) fp32 in [0, 1], exactly the reference's
    `T.Compose([T.Resize((512, 512), BICUBIC), T.ToTensor()])` on the PIL patch (val_patches.py:290-294,
    317-318): torchvision's Resize of a PIL image is `PIL.Image.resize(size, BICUBIC)` (PIL's 8-bit
    fixed-point bicubic, a = -0.5, uint8 result) and ToTensor is `uint8 -> float32 / 255`.  The resize
    runs on the host with PIL itself (bit-exact by construction); the division on the device."""
    from PIL import Image
    arr = np.ascontiguousarray(patches)
    n, h, w = arr.shape[:3]
    up = np.empty((n, SCALE * h, SCALE * w) + arr.shape[3:], dtype=np.uint8)
    for i in range(n):
        up[i] = np.asarray(Image.fromarray(arr[i]).resize((SCALE * w, SCALE * h), Image.BICUBIC))
    t = torch.from_numpy(up).to(device)
    t = t.permute(0, 3, 1, 2) if t.dim() == 4 else t[:, None]
    return t.contiguous().float().div(255)


@torch.no_grad()
def restore_image(model, sampler, lq: np.ndarray, c_txt: torch.Tensor, steps: int = 50, tile_batch: int = 16,
                  cleaner: Optional[Callable[[torch.Tensor], torch.Tensor]] = None, seed: int = 25,
                  rank: int = 0, world: int = 1, use_graph: bool = True, ts_model=None,
                  text_encoder: Optional[Callable] = None, prompt_style: str = "CAPTION",
                  merge_size: str = "lq") -> torch.Tensor:
    """lq: (H, W, 3) uint8 -> restored (1, 3, 4H, 4W) fp32 in [0, 1] on the model's device, every rank.
    merge_size="gt" passes the GT size (4H, 4W) as the merge's original_size, exactly as the reference's
    call (val_patches.py:375): its grid is then 4x too wide and the output is (1, 3, 16H, 16W)."""
    dev = model.device
    patches = np.stack(split_image_with_overlap(lq, LQ_PATCH, LQ_OVERLAP))
    n = len(patches)
    lo, hi = shard_range(n, rank, world)
    restorer = Restorer(model, sampler, steps=steps, use_graph=use_graph)
    outs = []
    for b0 in range(lo, hi, tile_batch):
        ids = range(b0, min(hi, b0 + tile_batch))
        val_lq = preprocess_lq(patches[ids.start:ids.stop], dev)
        clean = cleaner(val_lq) if cleaner is not None else val_lq
        cond = model.prepare_condition(clean, c_txt=c_txt)
        x_T, noise, _ = synthetic_tiles(ids, steps, latent_hw=(64, 64), seed=seed)
        if ts_model is None:
            outs.append(restorer(x_T.to(dev), noise.to(dev), cond).float())
        else:  # stage 3: TESTR + CLIP re-prompt between denoise steps (val_patches.py:330-348)
            ts_model.test_score_threshold = STAGE3_SCORE_THRESHOLD
            z, _ = sampler.val_sample(model, dev, steps, tuple(x_T.shape), cond, x_T=x_T.to(dev), noise=noise.to(dev),
                                      ts_model=ts_model, pure_cldm=model, text_encoder=text_encoder,
                                      prompt_style=prompt_style, use_graph=use_graph)
            outs.append(restorer.decode(z).float())
    local = torch.cat(outs) if outs else torch.zeros((0, 3, LQ_PATCH * SCALE, LQ_PATCH * SCALE), device=dev)
    tiles = tdist.gather_tiles(local, n, world)
    if merge_size not in ("lq", "gt"):
        raise ValueError(f"merge_size {merge_size!r} (lq or gt)")
    size = lq.shape[:2] if merge_size == "lq" else (SCALE * lq.shape[0], SCALE * lq.shape[1])
    return merge_patches_with_overlap_device(tiles, size, patch_size=LQ_PATCH * SCALE,
                                             overlap=LQ_OVERLAP * SCALE, lq_patch=LQ_PATCH, lq_overlap=LQ_OVERLAP)


def _parse():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--lq", help="LQ image (png/jpg); omit with --synthetic")
    ap.add_argument("--synthetic", default=None, help="HxW of a synthetic uniform LQ image (seed 29)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--tile-batch", type=int, default=16)
    ap.add_argument("--weights", default=None, help="state dict (.pt/.safetensors) with reference keys; "
                                                   "default: synthetic random-init weights")
    ap.add_argument("--config", default=None, help="val YAML (configs/val/*.yaml): model.cldm / model.diffusion "
                                                  "params build the model (val_patches.py:218-241)")
    ap.add_argument("--config_testr", default=None, help="TESTR yaml (testr/configs/TESTR/*.yaml): enables the "
                                                        "stage-3 prompt loop (needs CLIP: TAIR_CLIP_BPE + --weights)")
    ap.add_argument("--testr-weights", default=None, help="TESTR checkpoint ({'model': state dict}, reference keys)")
    ap.add_argument("--prompt-style", default=None, choices=["CAPTION", "TAG"],
                    help="stage-3 prompt style (default: the config's exp_args.prompt_style, else CAPTION)")
    ap.add_argument("--swinir", action="store_true", help="clean the LQ patches with SwinIR (val_patches.py:324); "
                    "params from --config model.swinir (else the val config's), weights from --swinir-weights "
                    "(else synthetic)")
    ap.add_argument("--swinir-weights", default=None, help="SwinIR state dict (.pth / .safetensors, reference keys)")
    ap.add_argument("--swinir-backend", choices=("torch", "hip"), default="torch",
                    help="SwinIR cleaner on stock torch (default) or on the HIP kernels (tair_amd/swinir_hip.py)")
    ap.add_argument("--merge-size", default="lq", choices=["lq", "gt"],
                    help="original_size of the overlap merge: the LQ size (correct grid) or the GT size as the "
                         "reference passes it (val_patches.py:375; mis-grids multi-patch images)")
    ap.add_argument("--prompt", default="", help="text prompt for CLIP (needs TAIR_CLIP_BPE for non-empty prompts); "
                                                 "default: synthetic c_txt when no CLIP weights are given")
    ap.add_argument("--clip-backend", default="torch", choices=["torch", "hip"],
                    help="CLIP text tower: stock torch (default) or the HIP kernels (tair_amd/clip_hip.py)")
    return ap.parse_args()


def main():
    args = _parse()
    from .cldm import ControlLDM
    from .diffusion import Diffusion
    from .pipeline import synthetic_context, vae_synthetic_state_dict
    from .sampler import SpacedSampler
    from .weights import manifest, synthetic_state_dict

    rank, world, local = tdist.init_from_env()
    dev = torch.device("cuda", local)
    torch.cuda.set_device(dev)
    if args.lq:
        from PIL import Image
        lq = np.asarray(Image.open(args.lq).convert("RGB"))
    else:
        h, w = (int(v) for v in (args.synthetic or "256x256").split("x"))
        lq = np.random.default_rng(29).integers(0, 256, size=(h, w, 3), dtype=np.uint8)
    cfg = None
    if args.config:
        from .config import build_diffusion, build_model, load_config
        cfg = load_config(args.config)
        model = build_model(cfg, max_batch=args.tile_batch, device=dev, with_clip=bool(args.weights),
                            clip_backend=args.clip_backend)
    else:
        model = ControlLDM(max_batch=args.tile_batch, device=dev)
    if args.weights:
        if args.weights.endswith(".safetensors"):
            from safetensors.torch import load_file
            sd = load_file(args.weights)
        else:
            sd = torch.load(args.weights, map_location="cpu", weights_only=True)
        model.load_state_dict(sd)
    else:
        model.load_state_dict(synthetic_state_dict(manifest(), seed=0))
        model.vae.load_state_dict(vae_synthetic_state_dict(model.vae, seed=0))
    diffusion = build_diffusion(cfg) if cfg is not None else Diffusion(linear_start=0.00085, linear_end=0.012,
                                                                       zero_snr=True, parameterization="v")
    sampler = SpacedSampler(diffusion.betas, diffusion.parameterization, False)
    nh, nw = patch_grid(lq.shape[0], lq.shape[1], LQ_PATCH, LQ_OVERLAP)
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    if model.clip is not None:
        c_txt = model.clip.encode([args.prompt]).float()
    else:
        c_txt = synthetic_context().to(dev)
    cleaner = None
    if args.swinir:
        from .config import build_swinir
        cleaner = build_swinir(cfg, dev, args.swinir_weights, backend=args.swinir_backend)
    ts_model, style = None, args.prompt_style
    if args.config_testr:
        from .config import build_testr
        if model.clip is None:
            raise SystemExit("stage 3 re-encodes prompts with CLIP: pass --weights with the clip.* keys")
        ts_model = build_testr(args.config_testr, dev, args.testr_weights)
        ts_model.test_score_threshold = STAGE3_SCORE_THRESHOLD
        style = style or ((cfg or {}).get("exp_args") or {}).get("prompt_style") or "CAPTION"
    img = restore_image(model, sampler, lq, c_txt, steps=args.steps, tile_batch=args.tile_batch, cleaner=cleaner,
                        rank=rank, world=world, ts_model=ts_model, prompt_style=style or "CAPTION",
                        merge_size=args.merge_size)
    torch.cuda.synchronize(dev)
    dt = tdist.max_over_ranks(time.perf_counter() - t0, dev)
    if rank == 0:
        mpix = img.shape[-1] * img.shape[-2] / 1e6
        print(f"[val_patches] {lq.shape[0]}x{lq.shape[1]} LQ -> {nh}x{nw} patches -> "
              f"{img.shape[-2]}x{img.shape[-1]} in {dt:.2f}s on {world} GPU(s): {mpix / dt:.3f} Mpix/s")
        if args.out:
            from PIL import Image
            arr = (img[0].permute(1, 2, 0).clamp(0, 1) * 255).round().byte().cpu().numpy()
            Image.fromarray(arr).save(args.out)
    model.close()
    if world > 1:
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
