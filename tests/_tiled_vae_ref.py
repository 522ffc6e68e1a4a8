"""TEST INFRASTRUCTURE ONLY — the reference's tiled VAE with fast mode off, restated over oracle/vae_ref.py.

* ``terediff/utils/tilevae/tilevae.py:307-323``  VAEHook: pad 11 (decoder, latent px) / 32 (encoder, image px); an
  input of at most 2 pad + tile_size per side runs the plain network
* ``:325-397``  get_best_tile_size / split_tiles: input boxes (core + pad, clipped) and output boxes (core,
  extended to a border within pad of it, x 8 or // 8), each [x1, x2, y1, y2]
* ``:77-165``   the task queue of one tile: conv_in, ResnetBlocks (store_res, pre_norm, silu, conv1, pre_norm, silu,
  conv2, add_res), the AttnBlock (store_res, pre_norm, attention, add_res), up / down sampling, norm_out, conv_out
* ``:177-215``  get_var_mean (biased, per (image, group) over the tile's pixels) / custom_group_norm (a batch_norm
  with the given mean and var, eps 1e-6, then the affine)
* ``:232-278``  GroupNormParam.summary: var and mean = the tiles' values weighted by their pixel counts
  (pixels / max, then / sum): a weighted average of variances, not the variance of the union
* ``:442-579``  vae_tile_forward: every tile runs its queue up to the next pre_norm; once all tiles are there the
  merged statistics normalise every tile; a finished tile is cropped (``:218-229``) into the result
* ``terediff/model/cldm.py:92-141``  post_quant_conv before the tiled decoder; quant_conv and the posterior mode
  after the tiled encoder

`union_variance=True` is NOT the reference: it normalises with the exact variance of the union of the tiles' pixels
(overlaps counted in every tile), so a test can show that its gate tells the two apart.
"""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F

GROUPS = 32


def pad_of(is_decoder: bool) -> int:
    return 11 if is_decoder else 32


def is_tiny(h: int, w: int, tile_size: int, is_decoder: bool) -> bool:
    return max(h, w) <= pad_of(is_decoder) * 2 + tile_size


def best_tile_size(lowerbound: int, upperbound: int) -> int:
    divider = 32
    while divider >= 2:
        remainder = lowerbound % divider
        if remainder == 0:
            return lowerbound
        candidate = lowerbound - remainder + divider
        if candidate <= upperbound:
            return candidate
        divider //= 2
    return lowerbound


def split_tiles(h: int, w: int, tile_size: int, is_decoder: bool):
    pad = pad_of(is_decoder)
    rows = max(math.ceil((h - 2 * pad) / tile_size), 1)
    cols = max(math.ceil((w - 2 * pad) / tile_size), 1)
    tile_h = best_tile_size(math.ceil((h - 2 * pad) / rows), tile_size)
    tile_w = best_tile_size(math.ceil((w - 2 * pad) / cols), tile_size)
    in_boxes, out_boxes = [], []
    for i in range(rows):
        for j in range(cols):
            x1, x2 = pad + j * tile_w, min(pad + (j + 1) * tile_w, w)
            y1, y2 = pad + i * tile_h, min(pad + (i + 1) * tile_h, h)
            out = [x1 if x1 > pad else 0, x2 if x2 < w - pad else w, y1 if y1 > pad else 0, y2 if y2 < h - pad else h]
            out_boxes.append([v * 8 if is_decoder else v // 8 for v in out])
            in_boxes.append([max(0, x1 - pad), min(w, x2 + pad), max(0, y1 - pad), min(h, y2 + pad)])
    return in_boxes, out_boxes


def group_var_mean(x: torch.Tensor):
    """Biased var and mean per (image, group) over the tile's own pixels, each [B * 32]."""
    b, c = x.shape[:2]
    y = x.contiguous().view(1, b * GROUPS, c // GROUPS, *x.shape[2:])
    return torch.var_mean(y, dim=[0, 2, 3, 4], unbiased=False)


def merge_stats(vars_, means, pixels, union_variance: bool = False):
    """GroupNormParam.summary: the tiles' var / mean [T][B * 32] weighted by their pixel counts."""
    var, mean = torch.vstack(vars_), torch.vstack(means)
    w = torch.tensor(pixels, dtype=torch.float32, device=var.device) / max(pixels)
    w = (w / w.sum()).unsqueeze(1)
    m = torch.sum(mean * w, dim=0)
    if union_variance:  # not the reference: E[x^2] - E[x]^2 over all tiles' pixels
        return torch.sum((var + mean * mean) * w, dim=0) - m * m, m
    return torch.sum(var * w, dim=0), m


def fixed_group_norm(x, mean, var, norm, eps=1e-6):
    b, c = x.shape[:2]
    y = x.contiguous().view(1, b * GROUPS, c // GROUPS, *x.shape[2:])
    y = F.batch_norm(y, mean.to(x), var.to(x), weight=None, bias=None, training=False, momentum=0, eps=eps)
    y = y.view(b, c, *x.shape[2:])
    return y * norm.weight.view(1, -1, 1, 1) + norm.bias.view(1, -1, 1, 1)


def _attention(a, y):
    """AttnBlock's body after its norm (oracle/vae_ref.py AttnBlock.forward), within one tile."""
    b, c, hh, ww = y.shape
    q, k, v = (m(y).reshape(b, c, hh * ww).transpose(1, 2) for m in (a.q, a.k, a.v))
    w = torch.softmax(torch.bmm(q, k.transpose(1, 2)) * (c ** -0.5), dim=-1)
    return a.proj_out(torch.bmm(w, v).transpose(1, 2).reshape(b, c, hh, ww))


def _res_tasks(q, blk):
    q.append(("store_res", blk.nin_shortcut if blk.cin != blk.cout else (lambda x: x)))
    q.append(("pre_norm", blk.norm1))
    q.append(("apply", F.silu))
    q.append(("apply", blk.conv1))
    q.append(("pre_norm", blk.norm2))
    q.append(("apply", F.silu))
    q.append(("apply", blk.conv2))
    q.append(("add_res", None))


def _attn_tasks(q, a):
    q.append(("store_res", lambda x: x))
    q.append(("pre_norm", a.norm))
    q.append(("apply", lambda y, a=a: _attention(a, y)))
    q.append(("add_res", None))


def _mid_tasks(q, net):
    _res_tasks(q, net.mid.block_1)
    _attn_tasks(q, net.mid.attn_1)
    _res_tasks(q, net.mid.block_2)


def task_queue(net, is_decoder: bool):
    q = [("apply", net.conv_in)]
    if is_decoder:
        _mid_tasks(q, net)
        for lvl in reversed(range(len(net.up))):
            for blk in net.up[lvl].block:
                _res_tasks(q, blk)
            if lvl != 0:
                q.append(("apply", net.up[lvl].upsample))
    else:
        for lvl, d in enumerate(net.down):
            for blk in d.block:
                _res_tasks(q, blk)
            if lvl != len(net.down) - 1:
                q.append(("apply", d.downsample))
        _mid_tasks(q, net)
    q.append(("pre_norm", net.norm_out))
    q.append(("apply", F.silu))
    q.append(("apply", net.conv_out))
    return q


def crop_valid_region(x, in_box, out_box, is_decoder: bool):
    scaled = [v * 8 if is_decoder else v // 8 for v in in_box]
    m = [out_box[k] - scaled[k] for k in range(4)]
    return x[:, :, m[2]:x.size(2) + m[3], m[0]:x.size(3) + m[1]]


@torch.no_grad()
def tiled_forward(net, x: torch.Tensor, tile_size: int, is_decoder: bool, union_variance: bool = False):
    """VAEHook(net, tile_size, is_decoder, fast_decoder=False, fast_encoder=False)(x)."""
    n, _, h, w = x.shape
    if is_tiny(h, w, tile_size, is_decoder):
        return net(x)
    in_boxes, out_boxes = split_tiles(h, w, tile_size, is_decoder)
    tiles = [x[:, :, b[2]:b[3], b[0]:b[1]].clone() for b in in_boxes]
    queues = [list(task_queue(net, is_decoder)) for _ in tiles]
    residual = [None] * len(tiles)
    result, done = None, 0
    while done < len(tiles):
        vars_, means, pixels, norm = [], [], [], None
        for i in range(len(tiles)):
            t, q = tiles[i], queues[i]
            while q:
                kind, fn = q.pop(0)
                if kind == "pre_norm":
                    v, m = group_var_mean(t)
                    vars_.append(v)
                    means.append(m)
                    pixels.append(t.shape[2] * t.shape[3])
                    norm = fn
                    break
                if kind == "store_res":
                    residual[i] = fn(t)
                elif kind == "add_res":
                    t = t + residual[i]
                    residual[i] = None
                else:
                    t = fn(t)
            tiles[i] = t
            if not q:
                done += 1
                if result is None:
                    result = torch.zeros((n, t.shape[1], h * 8 if is_decoder else h // 8,
                                          w * 8 if is_decoder else w // 8), dtype=t.dtype, device=t.device)
                ob = out_boxes[i]
                result[:, :, ob[2]:ob[3], ob[0]:ob[1]] = crop_valid_region(t, in_boxes[i], ob, is_decoder)
        if vars_:
            var, mean = merge_stats(vars_, means, pixels, union_variance)
            tiles = [fixed_group_norm(t, mean, var, norm) for t in tiles]
    return result


@torch.no_grad()
def decode_tiled(vae, z, tile_size: int, union_variance: bool = False):
    """cldm.py:121-141 with tiled=True, on z already divided by the scale factor (tile_size in latent pixels)."""
    return tiled_forward(vae.decoder, vae.post_quant_conv(z), tile_size, True, union_variance)


@torch.no_grad()
def encode_mode_tiled(vae, x, tile_size: int):
    """cldm.py:92-119 with tiled=True, sample=False, before the scale factor (tile_size in image pixels)."""
    moments = vae.quant_conv(tiled_forward(vae.encoder, x, tile_size, False))
    return torch.chunk(moments, 2, dim=1)[0]


def ramp_latent(B: int, h: int, w: int, seed: int, amp: float = 2.0) -> torch.Tensor:
    """randn plus a per-channel spatial ramp, so the tiles' means differ (a gate on the tiled result can then see
    the merge rule): channel c ramps by +-amp along y (even c) or x (odd c)."""
    z = torch.randn(B, 4, h, w, generator=torch.Generator().manual_seed(seed))
    ys = torch.linspace(-1, 1, h).view(1, 1, h, 1)
    xs = torch.linspace(-1, 1, w).view(1, 1, 1, w)
    for c in range(4):
        z[:, c:c + 1] += amp * (1 - 2 * (c // 2)) * (ys if c % 2 == 0 else xs)
    return z
