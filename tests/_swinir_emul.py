"""Test helper: a stock-torch restatement of the val-config SwinIR AS THE HIP PATH ROUNDS IT (tair_amd/swinir_hip.py),
for the parity gate of tests/test_swinir_hip_gpu.py.  It is not the code under test and shares none of it (the
window partition, relative-position index and shift mask are the stock module's, tair_amd/swinir.py).

Rounding points (bf16, round to nearest even): the linear and conv weights; every GEMM operand (the LayerNorm
outputs, patch_embed.norm's and norm's included; the q|k|v GEMM output; P, rounded before it is normalised, and the
attention output; the GELU output; the hi plane of the stream where a 3x3 conv reads it; the upsampler's
activations before and after each LeakyReLU).  Everything else is fp32: the residual stream and conv_first's
output (the HIP path's hi + lo planes carry them to ~2^-16), the mean-subtracted input (two planes as well),
biases, LayerNorm, softmax, conv_last's output.  The distance of this emulation from the fp32 oracle is the error
the bf16 operands alone cost; the HIP path may add accumulation order and the hi + lo step to it, nothing else.
"""
import torch
import torch.nn.functional as F

from tair_amd.swinir import RGB_MEAN, _from_windows, _rel_index, _to_windows, shift_mask

WS, HEADS, SF = 8, 6, 8
# The test weights' q / k rows (logits of a few units) and proj rows (the attention branch's share of the stream) are
# raised above the fan-in scale so that the attention scale matters to the output: with both at 1 the bf16 roundings
# of the upsampler's activations (~2e-3 of the image) hide a 3 % change of the logits (gate teeth,
# test_swinir_hip_cpu.py).  A larger q / k gain saturates the softmax and raises the bf16 error faster than the
# scale's effect.
QK_GAIN = 1.5
PROJ_GAIN = 2.0


def _bf(t):
    return t.to(torch.bfloat16).float()


def randomize(module, seed):
    """Every parameter random (build_swinir's synthetic init leaves the 1-D ones at their defaults): weights at
    fan-in scale with the q / k rows raised by QK_GAIN and proj by PROJ_GAIN, biases 0.1, LayerNorm gains 1 +- 0.1, bias tables 0.5."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, p in module.named_parameters():
            r = torch.randn(p.shape, generator=g)
            if name.endswith("relative_position_bias_table"):
                p.copy_(r * 0.5)
            elif p.dim() > 1:
                p.copy_(r * p[0].numel() ** -0.5)
                if name.endswith("attn.qkv.weight"):
                    p[:2 * p.shape[0] // 3] *= QK_GAIN
                if name.endswith("attn.proj.weight"):
                    p.mul_(PROJ_GAIN)
            elif "norm" in name and name.endswith("weight"):
                p.copy_(1.0 + 0.1 * r)
            else:
                p.copy_(0.1 * r)
    return module


def _conv(x, sd, key, up=False):
    if up:
        x = F.interpolate(x, scale_factor=2, mode="nearest")
    return F.conv2d(x, _bf(sd[key + ".weight"].float()), sd[key + ".bias"].float(), padding=1)


def _ln(x, sd, key):
    return _bf(F.layer_norm(x, (x.shape[-1],), sd[key + ".weight"].float(), sd[key + ".bias"].float(), 1e-5))


def _lin(x, sd, key):
    return F.linear(x, _bf(sd[key + ".weight"].float()), sd[key + ".bias"].float())


@torch.no_grad()
def emulate(sd, depths, x, scale=30 ** -0.5):
    """sd: reference-key state dict (on x's device); x [B, 3, H, W] fp32, H and W multiples of 64 -> [B, 3, H, W]."""
    mean = torch.tensor(RGB_MEAN, device=x.device).reshape(1, 3, 1, 1)
    f = _conv(F.pixel_unshuffle(x.float() - mean, SF), sd, "conv_first.1")
    B, C, H, W = f.shape
    d = C // HEADS
    idx = _rel_index(WS).reshape(-1).to(x.device)
    t = _ln(f.flatten(2).transpose(1, 2), sd, "patch_embed.norm")
    for i, depth in enumerate(depths):
        t0 = t
        for j in range(depth):
            p = f"layers.{i}.residual_group.blocks.{j}"
            shift = WS // 2 if j % 2 else 0
            y = _ln(t, sd, p + ".norm1").reshape(B, H, W, C)
            if shift:
                y = torch.roll(y, (-shift, -shift), (1, 2))
            win = _to_windows(y, WS)
            n, L, _ = win.shape
            q, k, v = _bf(_lin(win, sd, p + ".attn.qkv")).reshape(n, L, 3, HEADS, d).permute(2, 0, 3, 1, 4)
            s = q @ k.transpose(-1, -2) * scale
            s = s + sd[p + ".attn.relative_position_bias_table"].float()[idx].reshape(L, L, HEADS).permute(2, 0, 1)[None]
            if shift:
                m = shift_mask(H, W, WS, shift).to(x.device)
                s = (s.reshape(n // m.shape[0], m.shape[0], HEADS, L, L) + m[None, :, None]).reshape(n, HEADS, L, L)
            e = torch.exp(s - s.amax(-1, keepdim=True))
            o = _bf((_bf(e) @ v) / e.sum(-1, keepdim=True)).transpose(1, 2).reshape(n, L, C)
            o = _from_windows(_lin(o, sd, p + ".attn.proj"), WS, B, H, W)
            if shift:
                o = torch.roll(o, (shift, shift), (1, 2))
            t = t + o.reshape(B, H * W, C)
            t = t + _lin(_bf(F.gelu(_lin(_ln(t, sd, p + ".norm2"), sd, p + ".mlp.fc1"))), sd, p + ".mlp.fc2")
        t = _conv(_bf(t).transpose(1, 2).reshape(B, C, H, W), sd, f"layers.{i}.conv").flatten(2).transpose(1, 2) + t0
    feat = _ln(t, sd, "norm").transpose(1, 2).reshape(B, C, H, W)
    body = _conv(feat, sd, "conv_after_body") + f
    h = _bf(F.leaky_relu(_bf(_conv(_bf(body), sd, "conv_before_upsample.0")), 0.01))
    for i in range(3):
        h = _bf(F.leaky_relu(_bf(_conv(h, sd, f"conv_up{i + 1}", up=True)), 0.2))
    h = _bf(F.leaky_relu(_bf(_conv(h, sd, "conv_hr")), 0.2))
    return _conv(h, sd, "conv_last") + mean
