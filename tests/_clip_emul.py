"""Test helper: a stock-torch restatement of the text tower AS THE HIP TOWER ROUNDS IT (tair_amd/clip_hip.py), for
the parity gate of tests/test_clip_hip_gpu.py.  It is not the code under test and shares none of it.

Rounding points (bf16, round to nearest even): the linear weights; every GEMM input (the LayerNorm outputs, the
attention output, the GELU output); the attention inputs (the q|k|v GEMM output); the GELU and attention outputs.
Everything else is fp32: the residual stream (the HIP tower's hi + lo planes carry it to ~2^-16), biases,
LayerNorm, softmax.  The distance of this emulation from the fp32 oracle is the error the bf16 operands alone
cost; the HIP tower may add accumulation order and the hi + lo step to it, nothing else.
"""
import torch
import torch.nn.functional as F


def _bf(t):
    return t.to(torch.bfloat16).float()


@torch.no_grad()
def emulate(sd, tokens, heads, layer_idx):
    """sd: reference-key state dict (fp32, on tokens' device); tokens [B, L] int64 -> fp32 [B, L, C]."""
    p = "model.transformer.resblocks."
    n = 0
    while f"{p}{n}.ln_1.weight" in sd:
        n += 1
    x = sd["model.token_embedding.weight"][tokens] + sd["model.positional_embedding"][:tokens.shape[1]]
    B, L, C = x.shape
    d = C // heads
    mask = torch.full((L, L), float("-inf"), device=x.device).triu_(1)
    for i in range(n - layer_idx):
        g = lambda k: sd[f"{p}{i}.{k}"].float()  # noqa: E731
        y = _bf(F.layer_norm(x, (C,), g("ln_1.weight"), g("ln_1.bias"), 1e-5))
        qkv = _bf(F.linear(y, _bf(g("attn.in_proj_weight")), g("attn.in_proj_bias")))
        q, k, v = (t.transpose(1, 2) for t in qkv.view(B, L, 3, heads, d).unbind(2))
        s = (q @ k.transpose(-1, -2)) * d ** -0.5 + mask
        o = _bf(torch.softmax(s, -1) @ v).transpose(1, 2).reshape(B, L, C)
        x = x + F.linear(o, _bf(g("attn.out_proj.weight")), g("attn.out_proj.bias"))
        y = _bf(F.layer_norm(x, (C,), g("ln_2.weight"), g("ln_2.bias"), 1e-5))
        h = _bf(F.gelu(F.linear(y, _bf(g("mlp.c_fc.weight")), g("mlp.c_fc.bias"))))
        x = x + F.linear(h, _bf(g("mlp.c_proj.weight")), g("mlp.c_proj.bias"))
    return F.layer_norm(x, (C,), sd["model.ln_final.weight"].float(), sd["model.ln_final.bias"].float(), 1e-5)
