"""SD AutoencoderKL on stock PyTorch-ROCm (reference: terediff/model/vae.py:13-591).

Role: this module holds the VAE's parameters (reference names, so
``vae.*`` / SD-checkpoint ``first_stage_model.*`` keys load unchanged) and a stock PyTorch-ROCm forward
(MIOpen convolutions, SDPA, channels-last; fp32 or bf16) kept as ``vae_backend="torch"``.  The default
backend ``"hip"`` runs both directions on the library's kernels from these same parameters:
``tair_amd/vae_hip.py`` HipVAEDecoder (decode) and HipVAEEncoder (prepare_condition's encode), in split
precision (hi + lo bf16 planes, fp32-accurate).

The tiled VAE (utils/tilevae/tilevae.py, fast mode off) lives here as geometry shared by both backends
(``split_tiles``, ``tiling_needed``, ``place_tile``) and as the stock-torch fp32 path ``decode_tiled`` /
``encode_mode_tiled`` / ``encode_sample_tiled``.
"""
from __future__ import annotations

import torch
import torch.nn as nn
import torch.nn.functional as F


def _norm(c: int) -> nn.GroupNorm:
    return nn.GroupNorm(num_groups=32, num_channels=c, eps=1e-6, affine=True)  # vae.py:18-21


class ResnetBlock(nn.Module):
    """vae.py:60-117 with temb_channels=0, dropout 0."""

    def __init__(self, in_channels: int, out_channels: int):
        super().__init__()
        self.in_channels, self.out_channels = in_channels, out_channels
        self.norm1 = _norm(in_channels)
        self.conv1 = nn.Conv2d(in_channels, out_channels, 3, 1, 1)
        self.norm2 = _norm(out_channels)
        self.conv2 = nn.Conv2d(out_channels, out_channels, 3, 1, 1)
        if in_channels != out_channels:
            self.nin_shortcut = nn.Conv2d(in_channels, out_channels, 1)

    def forward(self, x):
        h = self.conv2(F.silu(self.norm2(self.conv1(F.silu(self.norm1(x))))))
        if self.in_channels != self.out_channels:
            x = self.nin_shortcut(x)
        return x + h


class AttnBlock(nn.Module):
    """vae.py:120-282: single-head spatial attention, d = C."""

    def __init__(self, c: int):
        super().__init__()
        self.norm = _norm(c)
        self.q = nn.Conv2d(c, c, 1)
        self.k = nn.Conv2d(c, c, 1)
        self.v = nn.Conv2d(c, c, 1)
        self.proj_out = nn.Conv2d(c, c, 1)

    def forward(self, x):
        b, c, h, w = x.shape
        y = self.norm(x)
        q, k, v = (m(y).flatten(2).transpose(1, 2).unsqueeze(1) for m in (self.q, self.k, self.v))
        o = F.scaled_dot_product_attention(q, k, v)
        o = o.squeeze(1).transpose(1, 2).reshape(b, c, h, w)
        return x + self.proj_out(o)


class Upsample(nn.Module):
    def __init__(self, c: int):
        super().__init__()
        self.conv = nn.Conv2d(c, c, 3, 1, 1)

    def forward(self, x):
        return self.conv(F.interpolate(x, scale_factor=2.0, mode="nearest"))


class Downsample(nn.Module):
    def __init__(self, c: int):
        super().__init__()
        self.conv = nn.Conv2d(c, c, 3, 2, 0)

    def forward(self, x):
        return self.conv(F.pad(x, (0, 1, 0, 1)))


class _Stage(nn.Module):
    pass


class Encoder(nn.Module):
    """vae.py:306-426."""

    def __init__(self, ch=128, ch_mult=(1, 2, 4, 4), num_res_blocks=2, in_channels=3, z_channels=4,
                 double_z=True, **_):
        super().__init__()
        self.conv_in = nn.Conv2d(in_channels, ch, 3, 1, 1)
        mults = (1,) + tuple(ch_mult)
        self.down = nn.ModuleList()
        bin_ = ch
        for i, m in enumerate(ch_mult):
            st = _Stage()
            st.block = nn.ModuleList()
            st.attn = nn.ModuleList()
            bin_ = ch * mults[i]
            for _ in range(num_res_blocks):
                st.block.append(ResnetBlock(bin_, ch * m))
                bin_ = ch * m
            if i != len(ch_mult) - 1:
                st.downsample = Downsample(bin_)
            self.down.append(st)
        self.mid = _Stage()
        self.mid.block_1 = ResnetBlock(bin_, bin_)
        self.mid.attn_1 = AttnBlock(bin_)
        self.mid.block_2 = ResnetBlock(bin_, bin_)
        self.norm_out = _norm(bin_)
        self.conv_out = nn.Conv2d(bin_, 2 * z_channels if double_z else z_channels, 3, 1, 1)

    def forward(self, x):
        h = self.conv_in(x)
        for i, st in enumerate(self.down):
            for blk in st.block:
                h = blk(h)
            if hasattr(st, "downsample"):
                h = st.downsample(h)
        h = self.mid.block_2(self.mid.attn_1(self.mid.block_1(h)))
        return self.conv_out(F.silu(self.norm_out(h)))


class Decoder(nn.Module):
    """vae.py:429-559."""

    def __init__(self, ch=128, out_ch=3, ch_mult=(1, 2, 4, 4), num_res_blocks=2, z_channels=4, **_):
        super().__init__()
        bin_ = ch * ch_mult[-1]
        self.conv_in = nn.Conv2d(z_channels, bin_, 3, 1, 1)
        self.mid = _Stage()
        self.mid.block_1 = ResnetBlock(bin_, bin_)
        self.mid.attn_1 = AttnBlock(bin_)
        self.mid.block_2 = ResnetBlock(bin_, bin_)
        stages = [None] * len(ch_mult)
        for i in reversed(range(len(ch_mult))):
            st = _Stage()
            st.block = nn.ModuleList()
            st.attn = nn.ModuleList()
            for _ in range(num_res_blocks + 1):
                st.block.append(ResnetBlock(bin_, ch * ch_mult[i]))
                bin_ = ch * ch_mult[i]
            if i != 0:
                st.upsample = Upsample(bin_)
            stages[i] = st
        self.up = nn.ModuleList(stages)
        self.norm_out = _norm(bin_)
        self.conv_out = nn.Conv2d(bin_, out_ch, 3, 1, 1)

    def forward(self, z):
        h = self.conv_in(z)
        h = self.mid.block_2(self.mid.attn_1(self.mid.block_1(h)))
        for i in reversed(range(len(self.up))):
            st = self.up[i]
            for blk in st.block:
                h = blk(h)
            if i != 0:
                h = st.upsample(h)
        return self.conv_out(F.silu(self.norm_out(h)))


# ---------------------------------------------------------------------------------------------------
# Tiled VAE (utils/tilevae/tilevae.py:307-579 VAEHook with fast_encoder = fast_decoder = False, as
# cldm.py:92-141 uses it): overlapping tiles run layer by layer; attention is local to a tile; every
# GroupNorm normalises with statistics merged over all tiles.  The geometry below is shared by the
# stock-torch path here and the HIP path (vae_hip.py).
# ---------------------------------------------------------------------------------------------------
DECODER_PAD, ENCODER_PAD = 11, 32  # tilevae.py:315: latent pixels / image pixels


def tile_pad(is_decoder: bool) -> int:
    return DECODER_PAD if is_decoder else ENCODER_PAD


def tiling_needed(h: int, w: int, tile_size: int, is_decoder: bool) -> bool:
    """tilevae.py:317-323: an input of at most 2 pad + tile_size per side runs untiled."""
    return max(h, w) > 2 * tile_pad(is_decoder) + tile_size


def _best_tile_size(lower: int, upper: int) -> int:
    """tilevae.py:325-338: the smallest multiple of 32 (else 16, 8, 4, 2) in [lower, upper]."""
    div = 32
    while div >= 2:
        rem = lower % div
        if rem == 0:
            return lower
        cand = lower - rem + div
        if cand <= upper:
            return cand
        div //= 2
    return lower


def split_tiles(h: int, w: int, tile_size: int, is_decoder: bool):
    """tilevae.py:340-397 -> (input boxes, output boxes), each [x1, x2, y1, y2], row-major over the tile grid.
    An input box is the tile's core grown by pad and clipped to the input; an output box is the core, extended
    to the border where the core is within pad of it, times 8 (decoder) or // 8 (encoder).  The output boxes
    partition the result."""
    pad = tile_pad(is_decoder)
    nh = max(-(-(h - 2 * pad) // tile_size), 1)
    nw = max(-(-(w - 2 * pad) // tile_size), 1)
    th = _best_tile_size(-(-(h - 2 * pad) // nh), tile_size)
    tw = _best_tile_size(-(-(w - 2 * pad) // nw), tile_size)
    ins, outs = [], []
    for i in range(nh):
        for j in range(nw):
            core = [pad + j * tw, min(pad + (j + 1) * tw, w), pad + i * th, min(pad + (i + 1) * th, h)]
            out = [core[0] if core[0] > pad else 0, core[1] if core[1] < w - pad else w,
                   core[2] if core[2] > pad else 0, core[3] if core[3] < h - pad else h]
            outs.append([v * 8 if is_decoder else v // 8 for v in out])
            ins.append([max(0, core[0] - pad), min(w, core[1] + pad), max(0, core[2] - pad), min(h, core[3] + pad)])
    return ins, outs


def crop_margins(in_box, out_box, is_decoder: bool):
    """tilevae.py:218-229 crop_valid_region: (left, right, top, bottom) margins of the output box inside the
    finished tile (right / bottom <= 0, counted from the tile's end)."""
    scaled = [v * 8 if is_decoder else v // 8 for v in in_box]
    return [out_box[k] - scaled[k] for k in range(4)]


def place_tile(result: torch.Tensor, tile: torch.Tensor, in_box, out_box, is_decoder: bool) -> None:
    """result[:, :, out box] = the tile cropped to its output box (NCHW)."""
    m = crop_margins(in_box, out_box, is_decoder)
    result[:, :, out_box[2]:out_box[3], out_box[0]:out_box[1]] = \
        tile[:, :, m[2]:tile.shape[2] + m[3], m[0]:tile.shape[3] + m[1]]


def _merged_group_norm(tiles, norm: nn.GroupNorm, silu: bool):
    """tilevae.py:232-278 GroupNormParam: per (image, group) every tile's biased var and mean over its own
    pixels, merged with the tiles' pixel shares (overlap pixels count in every tile that holds them; a
    weighted average of variances, not the variance of the union); every tile normalises with that pair."""
    G = norm.num_groups
    px = [t.shape[2] * t.shape[3] for t in tiles]
    total = float(sum(px))
    mean = var = None
    for t, n in zip(tiles, px):
        b, c = t.shape[:2]
        v, m = torch.var_mean(t.reshape(b, G, -1), dim=2, unbiased=False)
        mean = m * (n / total) if mean is None else mean + m * (n / total)
        var = v * (n / total) if var is None else var + v * (n / total)
    rstd = torch.rsqrt(var + norm.eps)
    outs = []
    for t in tiles:
        b, c, hh, ww = t.shape
        y = (t.reshape(b, G, -1) - mean[:, :, None]) * rstd[:, :, None]
        y = y.reshape(b, c, hh, ww) * norm.weight.view(1, -1, 1, 1) + norm.bias.view(1, -1, 1, 1)
        outs.append(F.silu(y) if silu else y)
    return outs


def _res_tiled(blk: ResnetBlock, xs):
    h = [blk.conv1(t) for t in _merged_group_norm(xs, blk.norm1, True)]
    h = [blk.conv2(t) for t in _merged_group_norm(h, blk.norm2, True)]
    if blk.in_channels != blk.out_channels:
        xs = [blk.nin_shortcut(x) for x in xs]
    return [x + t for x, t in zip(xs, h)]


def _attn_tiled(a: AttnBlock, xs):
    outs = []
    for x, y in zip(xs, _merged_group_norm(xs, a.norm, False)):
        b, c, h, w = x.shape
        q, k, v = (m(y).flatten(2).transpose(1, 2).unsqueeze(1) for m in (a.q, a.k, a.v))
        o = F.scaled_dot_product_attention(q, k, v).squeeze(1).transpose(1, 2).reshape(b, c, h, w)
        outs.append(x + a.proj_out(o))
    return outs


def _mid_tiled(mid, hs):
    return _res_tiled(mid.block_2, _attn_tiled(mid.attn_1, _res_tiled(mid.block_1, hs)))


def _run_tiled(net, x: torch.Tensor, tile_size: int, is_decoder: bool) -> torch.Tensor:
    """The encoder / decoder `net` over x, tiled: all tiles advance together from one GroupNorm to the next."""
    B, _, H, W = x.shape
    if not tiling_needed(H, W, tile_size, is_decoder):
        return net(x)
    ins, outs = split_tiles(H, W, tile_size, is_decoder)
    hs = [net.conv_in(x[:, :, b[2]:b[3], b[0]:b[1]]) for b in ins]
    if is_decoder:
        hs = _mid_tiled(net.mid, hs)
        for i in reversed(range(len(net.up))):
            for blk in net.up[i].block:
                hs = _res_tiled(blk, hs)
            if i != 0:
                hs = [net.up[i].upsample(t) for t in hs]
    else:
        for st in net.down:
            for blk in st.block:
                hs = _res_tiled(blk, hs)
            if hasattr(st, "downsample"):
                hs = [st.downsample(t) for t in hs]
        hs = _mid_tiled(net.mid, hs)
    hs = [net.conv_out(t) for t in _merged_group_norm(hs, net.norm_out, True)]
    result = torch.zeros((B, hs[0].shape[1], H * 8 if is_decoder else H // 8, W * 8 if is_decoder else W // 8),
                         dtype=hs[0].dtype, device=x.device)
    for t, ib, ob in zip(hs, ins, outs):
        place_tile(result, t, ib, ob, is_decoder)
    return result


class AutoencoderKL(nn.Module):
    """vae.py:562-591 (+ DiagonalGaussianDistribution.mode/sample, distributions.py:24-46)."""

    def __init__(self, embed_dim: int = 4, z_channels: int = 4, ch: int = 128, ch_mult=(1, 2, 4, 4),
                 num_res_blocks: int = 2, in_channels: int = 3, out_ch: int = 3, double_z: bool = True, **_):
        super().__init__()
        self.encoder = Encoder(ch=ch, ch_mult=ch_mult, num_res_blocks=num_res_blocks, in_channels=in_channels,
                               z_channels=z_channels, double_z=double_z)
        self.decoder = Decoder(ch=ch, out_ch=out_ch, ch_mult=ch_mult, num_res_blocks=num_res_blocks,
                               z_channels=z_channels)
        self.quant_conv = nn.Conv2d(2 * z_channels, 2 * embed_dim, 1)
        self.post_quant_conv = nn.Conv2d(embed_dim, z_channels, 1)
        self.compute_dtype = torch.float32

    def set_compute_dtype(self, dtype: torch.dtype):
        self.compute_dtype = dtype
        self.to(dtype=dtype, memory_format=torch.channels_last)
        return self

    def _moments(self, x):
        return self.quant_conv(self.encoder(x))

    def encode_mode(self, x):
        x = x.to(self.compute_dtype).contiguous(memory_format=torch.channels_last)
        return torch.chunk(self._moments(x), 2, dim=1)[0].float()

    def encode_sample(self, x, generator=None):
        x = x.to(self.compute_dtype).contiguous(memory_format=torch.channels_last)
        mean, logvar = torch.chunk(self._moments(x).float(), 2, dim=1)
        std = torch.exp(0.5 * torch.clamp(logvar, -30.0, 20.0))
        return mean + std * torch.randn(mean.shape, generator=generator, device=mean.device)

    def decode(self, z):
        z = z.to(self.compute_dtype).contiguous(memory_format=torch.channels_last)
        return self.decoder(self.post_quant_conv(z)).float()

    # tiled (cldm.py:92-141 with tiled=True): tile_size in image pixels for the encoder, latent pixels for the
    # decoder; post_quant_conv runs before the tiling and quant_conv after it, on the whole tensor
    def _moments_tiled(self, x, tile_size: int):
        x = x.to(self.compute_dtype)
        return self.quant_conv(_run_tiled(self.encoder, x, tile_size, is_decoder=False))

    def encode_mode_tiled(self, x, tile_size: int):
        if not tiling_needed(x.shape[2], x.shape[3], tile_size, False):
            return self.encode_mode(x)
        return torch.chunk(self._moments_tiled(x, tile_size), 2, dim=1)[0].float()

    def encode_sample_tiled(self, x, tile_size: int, generator=None):
        if not tiling_needed(x.shape[2], x.shape[3], tile_size, False):
            return self.encode_sample(x, generator=generator)
        mean, logvar = torch.chunk(self._moments_tiled(x, tile_size).float(), 2, dim=1)
        std = torch.exp(0.5 * torch.clamp(logvar, -30.0, 20.0))
        return mean + std * torch.randn(mean.shape, generator=generator, device=mean.device)

    def decode_tiled(self, z, tile_size: int):
        if not tiling_needed(z.shape[2], z.shape[3], tile_size, True):
            return self.decode(z)
        z = z.to(self.compute_dtype)
        return _run_tiled(self.decoder, self.post_quant_conv(z), tile_size, is_decoder=True).float()
