"""The CLIP-H text tower on the HIP kernels (tair_amd/clip_hip.py, csrc/clip.hip): every new kernel through the
C ABI against fp64 on the same bf16 operands, the tower against the oracle (oracle/clip_ref.py), graph replay,
and the stage-3 loop with the HIP tower.

Operands sit in buffers with guard rows and padded leading dimensions: inputs are surrounded by NaN (a read
outside the operand poisons the result), outputs by a sentinel that must survive.

Gates (none is derived from what the code gives):
* causal attention: rel-L2 <= 1e-2 against fp64, the project's attention gate (test_kernels_gpu.py
  test_attention: P is rounded to bf16 before P V); rows <= i bitwise independent of k / v rows > i;
* GELU epilogue, two-plane LayerNorm with bf16 output: one bf16 rounding of an fp32 value, 1.3 x the rounding
  floor rel-L2(bf16(ref), ref) of the fp64 reference (test_lnfold_gpu.py _floor); fp32 LayerNorm output: 1e-5,
  the gate test_stage3_gpu.py holds the fp32 tower to;
* embedding: bitwise torch (fp32 add, then the hi / lo split);
* tower: rel-L2(HIP, oracle) <= 1.5 x rel-L2(emulation, oracle), the emulation (tests/_clip_emul.py) being stock
  torch with the tower's bf16 rounding points and an fp32 stream: 1.5 x allows for accumulation order and the
  hi + lo stream's ~2^-16 step; a missed rounding point or a lost lo plane shows as >= 2 x;
* stage-3 loop: latent rel-L2 <= 5e-3 against the oracle loop (test_stage3_loop_matches_oracle's gate).
"""
import ctypes

import pytest
import torch

from tests._clip_emul import emulate
from tests.test_stage3_gpu import STEPS, VOCAB, Spy, byte_tokens, env, rel  # noqa: F401  (env: the r4 fixture)

pytestmark = pytest.mark.gpu

ATTN_GATE = 1e-2
FLOOR_RATIO = 1.3
NAN = float("nan")


def _L():
    from tair_amd import _lib
    return _lib.lib(), _lib


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def _floor(ref):
    return rel(ref.to(torch.bfloat16), ref)


def _guarded(rows, cols, fill, dtype=torch.bfloat16, pad=32, guard=8):
    """A [rows, cols] view inside a buffer of `guard` rows above and below and `pad` columns to the right."""
    buf = torch.full((rows + 2 * guard, cols + pad), fill, device="cuda", dtype=dtype)
    return buf, buf[guard:guard + rows, :cols]


def _guards_intact(buf, view, fill):
    mask = torch.ones_like(buf, dtype=torch.bool)
    g = (buf.shape[0] - view.shape[0]) // 2
    mask[g:g + view.shape[0], :view.shape[1]] = False
    return bool((buf[mask] == fill).all())


# --------------------------------------------------------------------------------- causal attention
CAUSAL_SHAPES = [(1, 2, 1), (1, 2, 16), (2, 2, 17), (1, 16, 64), (1, 16, 77), (3, 2, 77), (1, 2, 128)]


def _causal_run(qkv, o, B, H, S):
    L, _ = _L()
    C = H * 64
    ld = qkv.stride(0)
    rc = L.tair_k_attention_causal(_p(qkv), ld, _p(qkv[:, C:]), ld, _p(qkv[:, 2 * C:]), ld, _p(o), o.stride(0), B, H, S,
                                   0.125, _stream())
    assert rc == 0, L.tair_last_error()
    torch.cuda.synchronize()


def _causal_ref(qkv, B, H, S):
    C = H * 64
    q, k, v = (t.transpose(1, 2) for t in qkv.double().view(B, S, 3, H, 64).unbind(2))
    s = q @ k.transpose(-1, -2) * 0.125 + torch.full((S, S), float("-inf"), device=qkv.device).triu_(1).double()
    return (torch.softmax(s, -1) @ v).transpose(1, 2).reshape(B * S, C)


@pytest.mark.parametrize("B,H,S", CAUSAL_SHAPES)
def test_causal_attention(B, H, S):
    g = torch.Generator(device="cuda").manual_seed(100 * B + 10 * H + S)
    C, T = H * 64, B * S
    ibuf, qkv = _guarded(T, 3 * C, NAN, pad=64)  # q | k | v strided out of one fused [T, 3C] buffer
    x = torch.randn(T, 3 * C, device="cuda", generator=g)
    x[:, :2 * C] *= 2  # q, k (test_attention's operands)
    qkv.copy_(x.to(torch.bfloat16))
    obuf, o = _guarded(T, C, 7.0)
    _causal_run(qkv, o, B, H, S)
    e = rel(o, _causal_ref(qkv, B, H, S))
    print(f"causal attention B={B} H={H} S={S}: rel-L2 {e:.2e}")
    assert e <= ATTN_GATE, e
    assert _guards_intact(obuf, o, 7.0)
    # causality, bitwise: new k and v at rows > i leave the output rows <= i unchanged
    for i in sorted({0, S // 2, S - 2} & set(range(S - 1))):
        q2 = qkv.clone().view(B, S, 3 * C)
        q2[:, i + 1:, C:] = (torch.randn(B, S - i - 1, 2 * C, device="cuda", generator=g) * 3).to(torch.bfloat16)
        ibuf2, qkv2 = _guarded(T, 3 * C, NAN, pad=64)
        qkv2.copy_(q2.view(T, 3 * C))
        obuf2, o2 = _guarded(T, C, 7.0)
        _causal_run(qkv2, o2, B, H, S)
        a, b = o.contiguous().view(B, S, C)[:, :i + 1], o2.contiguous().view(B, S, C)[:, :i + 1]
        assert torch.equal(a.view(torch.int16), b.view(torch.int16)), i
        if i + 1 < S:
            assert not torch.equal(o.contiguous().view(B, S, C)[:, i + 1:], o2.contiguous().view(B, S, C)[:, i + 1:])


@pytest.mark.parametrize("S", [0, 129])
def test_causal_attention_refuses_bad_lengths(S):
    L, _ = _L()
    qkv = torch.zeros(130, 3 * 128, device="cuda", dtype=torch.bfloat16)
    o = torch.full((130, 128), 7.0, device="cuda", dtype=torch.bfloat16)
    rc = L.tair_k_attention_causal(_p(qkv), 384, _p(qkv[:, 128:]), 384, _p(qkv[:, 256:]), 384, _p(o), 128, 1, 2, S, 0.125,
                                   _stream())
    torch.cuda.synchronize()
    assert rc == -1 and b"attention_causal" in L.tair_last_error()
    assert bool((o == 7.0).all())  # nothing was launched


# ------------------------------------------------------------------------------------ GELU epilogue
def _gelu_case(M, N, K, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    _, A = _guarded(M, K, NAN)
    A.copy_(torch.randn(M, K, device="cuda", generator=g).to(torch.bfloat16))
    W = (torch.randn(N, K, device="cuda", generator=g) / K ** 0.5).to(torch.bfloat16)
    bias = torch.randn(N, device="cuda", generator=g) * 0.5
    ref = torch.nn.functional.gelu(A.double() @ W.double().t() + bias.double())
    return A, W, bias, ref


def _gelu_run(A, W, bias, M, N, K, force, tickets=True, probe=0):
    L, lib = _L()
    obuf, out = _guarded(M, N, 7.0)
    part = torch.empty(8 << 20, device="cuda")
    sem = torch.zeros(1 << 16, device="cuda", dtype=torch.int32)
    d = lib.GemmDesc()
    d.M, d.N, d.K, d.amode, d.alpha, d.act, d.rows_per_b = M, N, K, 0, 1.0, 3, 1
    d.A, d.lda, d.Wt, d.ldw, d.bias = A.data_ptr(), A.stride(0), W.data_ptr(), K, bias.data_ptr()
    d.out, d.ldo = out.data_ptr(), out.stride(0)
    d.partial, d.partial_cap = part.data_ptr(), part.numel()
    if tickets:
        d.tile_sem, d.sem_cap = sem.data_ptr(), sem.numel()
    d.force_bm, d.force_bn, d.force_splits = force
    d.probe = probe
    rc = L.tair_k_gemm(ctypes.byref(d), _stream())
    assert rc == 0, L.tair_last_error()
    torch.cuda.synchronize()
    assert torch.count_nonzero(sem) == 0
    assert _guards_intact(obuf, out, 7.0)
    return out


@pytest.mark.parametrize("M,N,K", [(77, 256, 128), (154, 4096, 1024)])
def test_gelu_epilogue(M, N, K):
    A, W, bias, ref = _gelu_case(M, N, K, seed=M + N)
    fl = _floor(ref)
    # the planner's own choice, forced 64x64 and 64x128 tiles, and a forced 4-way split three ways: summed by the
    # reduce kernel (no tickets), combined cooperatively (tickets), combined by the last slice to arrive (probe 4)
    runs = {"planner": ((0, 0, 0), True, 0), "64x64": ((64, 64, 1), True, 0), "64x128": ((64, 128, 1), True, 0),
            "split4 reduce": ((64, 64, 4), False, 0), "split4 coop": ((64, 64, 4), True, 0),
            "split4 in-kernel": ((64, 64, 4), True, 4)}
    outs = {}
    for name, (force, tickets, probe) in runs.items():
        outs[name] = _gelu_run(A, W, bias, M, N, K, force, tickets, probe)
        e = rel(outs[name], ref)
        print(f"gelu {M}x{N}x{K} {name}: rel-L2 {e:.3e} (floor {fl:.3e}, ratio {e / fl:.3f})")
        assert e <= FLOOR_RATIO * fl, (name, e, fl)
    # what test_kernels_gpu.py claims for act 0: the three combines of one split plan give the same bits
    assert torch.equal(outs["split4 reduce"], outs["split4 coop"])
    assert torch.equal(outs["split4 reduce"], outs["split4 in-kernel"])


def test_gelu_is_not_skipped_by_a_refused_plan():
    L, lib = _L()
    A, W, bias, _ = _gelu_case(154, 512, 128, seed=5)
    out = torch.full((154, 512), 7.0, device="cuda", dtype=torch.bfloat16)
    d = lib.GemmDesc()
    d.M, d.N, d.K, d.amode, d.alpha, d.act, d.rows_per_b = 154, 512, 128, 0, 1.0, 3, 1
    d.A, d.lda, d.Wt, d.ldw, d.bias = A.data_ptr(), A.stride(0), W.data_ptr(), 128, bias.data_ptr()
    d.out, d.ldo = out.data_ptr(), 512
    d.force_bm, d.force_bn = 256, 128
    assert L.tair_k_gemm(ctypes.byref(d), _stream()) != 0
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())


# ---------------------------------------------------------------------------------------- embedding
@pytest.mark.parametrize("B", [1, 3])
def test_embed_tokens_bitwise(B):
    L, _ = _L()
    V, C, ctx = 600, 1024, 77
    g = torch.Generator(device="cuda").manual_seed(B)
    table = torch.randn(V, C, device="cuda", generator=g) * 0.02
    pos = torch.randn(ctx, C, device="cuda", generator=g) * 0.02
    ids = torch.randint(0, V, (B, ctx), device="cuda", generator=g)
    ids[0, 0], ids[0, 1], ids[-1, -1] = 0, V - 1, V - 1
    obuf, out = _guarded(B * ctx, 2 * C, 7.0)
    rc = L.tair_k_embed_tokens(_p(ids), B, ctx, _p(table), V, _p(pos), C, _p(out), C, out.stride(0), _stream())
    assert rc == 0, L.tair_last_error()
    torch.cuda.synchronize()
    x = (table[ids] + pos).view(B * ctx, C)
    hi = x.to(torch.bfloat16)
    lo = (x - hi.float()).to(torch.bfloat16)
    assert torch.equal(out[:, :C].contiguous().view(torch.int16), hi.view(torch.int16))
    assert torch.equal(out[:, C:].contiguous().view(torch.int16), lo.view(torch.int16))
    assert _guards_intact(obuf, out, 7.0)


def test_embed_tokens_clamps_and_counts_ids_outside_the_table():
    L, _ = _L()
    V, C, ctx = 50, 128, 8
    n = ctypes.c_int(0)
    assert L.tair_fault_count(1, ctypes.byref(n)) == 0  # (clear whatever an earlier test left)
    g = torch.Generator(device="cuda").manual_seed(9)
    tbuf, table = _guarded(V, C, NAN, dtype=torch.float32, pad=0)  # a read past either end of the table is NaN
    table.copy_(torch.randn(V, C, device="cuda", generator=g))
    pos = torch.randn(ctx, C, device="cuda", generator=g)
    ids = torch.randint(0, V, (1, ctx), device="cuda", generator=g)
    ids[0, 2], ids[0, 5] = V + 5, -3
    out = torch.empty(ctx, 2 * C, device="cuda", dtype=torch.bfloat16)
    rc = L.tair_k_embed_tokens(_p(ids), 1, ctx, _p(table), V, _p(pos), C, _p(out), C, 2 * C, _stream())
    assert rc == 0, L.tair_last_error()
    torch.cuda.synchronize()
    x = table[ids.clamp(0, V - 1)][0] + pos
    assert torch.equal(out[:, :C], x.to(torch.bfloat16))
    assert L.tair_fault_count(1, ctypes.byref(n)) == 0 and n.value == 2
    assert L.tair_fault_count(0, ctypes.byref(n)) == 0 and n.value == 0


# ------------------------------------------------------------------------------ two-plane LayerNorm
@pytest.mark.parametrize("C", [128, 1024])
@pytest.mark.parametrize("f32", [0, 1])
def test_layernorm_split(C, f32):
    L, _ = _L()
    T = 77
    g = torch.Generator(device="cuda").manual_seed(C + f32)
    x = torch.randn(T, C, device="cuda", generator=g) * (torch.rand(T, 1, device="cuda", generator=g) + 0.5) + \
        torch.randn(T, 1, device="cuda", generator=g) * 1.5
    hi = x.to(torch.bfloat16)
    lo = (x - hi.float()).to(torch.bfloat16)
    _, xin = _guarded(T, 2 * C, NAN)
    xin[:, :C], xin[:, C:] = hi, lo
    gamma = torch.rand(C, device="cuda", generator=g) + 0.5
    beta = torch.randn(C, device="cuda", generator=g) * 0.2
    obuf, y = _guarded(T, C, 7.0, dtype=torch.float32 if f32 else torch.bfloat16)
    rc = L.tair_k_layernorm_split(_p(xin), xin.stride(0), C, T, C, _p(gamma), _p(beta), 1e-5, _p(y), y.stride(0), f32,
                                  _stream())
    assert rc == 0, L.tair_last_error()
    torch.cuda.synchronize()
    ref = torch.nn.functional.layer_norm(hi.double() + lo.double(), (C,), gamma.double(), beta.double(), 1e-5)
    e = rel(y, ref)
    print(f"layernorm_split C={C} f32={f32}: rel-L2 {e:.3e}" + ("" if f32 else f" (floor {_floor(ref):.3e})"))
    assert e <= (1e-5 if f32 else FLOOR_RATIO * _floor(ref)), e
    assert _guards_intact(obuf, y, 7.0)
    # the lo plane is read: hi alone is a different (one-plane) input
    y1 = torch.empty(T, C, device="cuda", dtype=torch.float32)
    assert L.tair_k_layernorm_split(_p(xin), xin.stride(0), 0, T, C, _p(gamma), _p(beta), 1e-5, _p(y1), C, 1, _stream()) == 0
    torch.cuda.synchronize()
    assert rel(y1, torch.nn.functional.layer_norm(hi.double(), (C,), gamma.double(), beta.double(), 1e-5)) <= 1e-5


# --------------------------------------------------------------------------- tower against the oracle
PROMPTS = ["", "a storefront sign that reads OPEN 24 HOURS",
           "A realistic scene where the texts " + ", ".join(f'"WORD{i}"' for i in range(12)) + " appear clearly"]


def _towers(width, layers, layer):
    """(stock fp32 tower on the GPU, oracle, HIP tower) with test_stage3_gpu.py's weight initialisation."""
    from oracle.clip_ref import FrozenOpenCLIPEmbedderRef
    from tair_amd.clip import FrozenOpenCLIPEmbedder
    from tair_amd.clip_hip import HipTextTower
    torch.backends.cuda.matmul.allow_tf32 = False
    heads = width // 64
    clip = FrozenOpenCLIPEmbedder(width, text_cfg=dict(width=width, layers=layers, heads=heads, vocab_size=VOCAB),
                                  layer=layer).eval()
    g = torch.Generator().manual_seed(8 + width + layers)
    with torch.no_grad():
        for name, p in clip.named_parameters():
            ln_gain = ".ln_" in name and name.endswith("weight")
            p.copy_(torch.randn(p.shape, generator=g) * (0.1 if ln_gain else 0.02) + (1.0 if ln_gain else 0.0))
    ref = FrozenOpenCLIPEmbedderRef(width, width, layers, heads, 77, VOCAB, layer=layer).cuda().eval()
    ref.load_state_dict(clip.state_dict(), strict=True)
    clip = clip.cuda()
    return clip, ref, HipTextTower(clip, max_batch=3)


@pytest.fixture(scope="module", params=[(128, 2), (1024, 2)], ids=["w128", "w1024"])
def towers(request):
    width, layers = request.param
    return {layer: _towers(width, layers, layer) for layer in ("penultimate", "last")}


def _parity(clip, ref, hip, tokens):
    with torch.no_grad():
        want = ref(tokens)
        got = hip(tokens)
        emu = emulate({k: v for k, v in clip.state_dict().items()}, tokens, clip.model.transformer.resblocks[0].attn.heads,
                      clip.layer_idx)
    assert got.dtype == torch.float32 and got.shape == want.shape
    return rel(got, want), rel(emu, want)


@pytest.mark.parametrize("layer", ["penultimate", "last"])
@pytest.mark.parametrize("B", [1, 3])
def test_tower_matches_oracle(towers, layer, B):
    clip, ref, hip = towers[layer]
    assert len(byte_tokens(PROMPTS[2])[0].nonzero()) == 77  # longer than the context: truncated
    tokens = byte_tokens(PROMPTS if B == 3 else PROMPTS[1]).cuda()
    e_hip, e_emu = _parity(clip, ref, hip, tokens)
    print(f"tower width {hip.width} layer={layer} B={B}: HIP {e_hip:.3e}, emulation {e_emu:.3e}, "
          f"ratio {e_hip / e_emu:.2f}")
    assert e_hip <= 1.5 * e_emu, (e_hip, e_emu)
    if B == 3:  # a batch row == the same prompt alone: no state shared between rows.  Both sit within the gate of
        # the oracle's row, so within twice the gate of each other (the GEMMs' split-K plans differ with M)
        for r in (0, 2):
            assert rel(hip(tokens[r:r + 1]), hip(tokens)[r:r + 1]) <= 2 * 1.5 * rel(
                emulate(clip.state_dict(), tokens[r:r + 1], hip.heads, hip.layer_idx), ref(tokens[r:r + 1]))
    hip.check_faults()


@pytest.mark.slow
def test_tower_24_layers_matches_oracle():
    clip, ref, hip = _towers(1024, 24, "penultimate")
    e_hip, e_emu = _parity(clip, ref, hip, byte_tokens(PROMPTS[1:]).cuda())
    print(f"tower width 1024, 24 layers, penultimate, B=2: HIP {e_hip:.3e}, emulation {e_emu:.3e}, "
          f"ratio {e_hip / e_emu:.2f}; {hip.launch_count()} launches")
    assert e_hip <= 1.5 * e_emu, (e_hip, e_emu)
    hip.check_faults()


def test_tower_loads_reference_keys_in_place(towers):
    """load_state_dict with the reference key names (a checkpoint's clip.* keys) repacks into the same buffers."""
    clip, ref, hip = towers["penultimate"]
    tokens = byte_tokens(PROMPTS[1]).cuda()
    before = hip(tokens)
    ptr = hip.w_fc.data_ptr()
    sd = {k: v.clone() for k, v in clip.state_dict().items()}
    sd["model.transformer.resblocks.0.mlp.c_fc.bias"] += 0.5
    hip.load_state_dict(sd)
    assert hip.w_fc.data_ptr() == ptr and rel(hip(tokens), before) > 1e-3
    hip.load_state_dict(clip.state_dict())
    assert torch.equal(hip(tokens), before)
    with pytest.raises(RuntimeError):
        hip.load_state_dict({k: v for k, v in clip.state_dict().items() if "ln_final" not in k})
    # more prompts than max_batch (3): runs of max_batch through the same workspaces, never a reallocation
    five = byte_tokens([PROMPTS[1], PROMPTS[2], "", PROMPTS[1], PROMPTS[2]]).cuda()
    out5 = hip(five)
    assert out5.shape == (5, 77, hip.width) and hip.w_fc.data_ptr() == ptr
    assert torch.equal(out5[:3], hip(five[:3])) and torch.equal(out5[3:], hip(five[3:]))
    with pytest.raises(Exception):
        hip(torch.zeros(1, 78, dtype=torch.long))  # longer than the context


def test_controlldm_clip_backend_wiring():
    """ControlLDM(clip_backend="hip"): model.clip is the HIP tower with the stock tower's surface, and both
    checkpoint routes (load_state_dict's clip.* keys, load_pretrained_sd's cond_stage_model.* keys) repack it."""
    from __graft_entry__ import TINY_UNET
    from oracle.clip_ref import FrozenOpenCLIPEmbedderRef
    from tair_amd.cldm import ControlLDM
    from tair_amd.clip import FrozenOpenCLIPEmbedder, tokenize
    from tair_amd.clip_hip import HipTextTower
    cfg = dict(embed_dim=128, text_cfg=dict(width=128, layers=2, heads=2), layer="penultimate")  # (the real vocabulary)
    kw = dict(clip_cfg=cfg, max_batch=1, latent_hw=(16, 16), with_vae=False)
    m0 = ControlLDM(TINY_UNET, **kw)
    assert type(m0.clip) is FrozenOpenCLIPEmbedder and m0.clip_backend == "torch"
    m0.close()
    m = ControlLDM(TINY_UNET, clip_backend="hip", **kw)
    assert isinstance(m.clip, HipTextTower) and m.clip.model.positional_embedding.shape == (77, 128)
    ref = FrozenOpenCLIPEmbedderRef(128, 128, 2, 2, 77, 49408).cuda().eval()
    tokens = tokenize("", 77, m.clip._tok).cuda()  # the empty prompt tokenises without the merge table: SOT, EOT
    for seed, prefix, load in ((1, "clip.", lambda sd: m.load_state_dict(sd, strict=False)),
                               (2, "cond_stage_model.", m.load_pretrained_sd)):
        stock = FrozenOpenCLIPEmbedder(**cfg).eval()
        g = torch.Generator().manual_seed(seed)
        with torch.no_grad():
            for name, p in stock.named_parameters():
                ln_gain = ".ln_" in name and name.endswith("weight")
                p.copy_(torch.randn(p.shape, generator=g) * (0.1 if ln_gain else 0.02) + (1.0 if ln_gain else 0.0))
        load({prefix + k: v for k, v in stock.state_dict().items()})
        ref.load_state_dict(stock.state_dict(), strict=True)
        with torch.no_grad():
            want = ref(tokens)
            e_emu = rel(emulate({k: v.cuda() for k, v in stock.state_dict().items()}, tokens, 2, 1), want)
        e_hip = rel(m.clip.encode(""), want)
        print(f"ControlLDM clip_backend=hip, {prefix}* keys: HIP {e_hip:.3e}, emulation {e_emu:.3e}")
        assert e_hip <= 1.5 * e_emu, (prefix, e_hip, e_emu)
    m.close()


# ---------------------------------------------------------------------------------------------- graph
def test_graphed_tower_is_bitwise_eager_and_stateless(towers):
    from tair_amd.testr import GraphedTextEncoder
    _, _, hip = towers["penultimate"]
    a, b = PROMPTS[1], PROMPTS[2]
    eager_a, eager_b = hip(byte_tokens(a).cuda()), hip(byte_tokens(b).cuda())
    assert eager_a.data_ptr() != eager_b.data_ptr() and not torch.equal(eager_a, eager_b)
    enc = GraphedTextEncoder(hip, byte_tokens)
    ga1, gb, ga2 = enc(a), enc(b), enc(a)
    torch.cuda.synchronize()
    assert len(enc._graphs) == 1
    assert torch.equal(ga1, eager_a) and torch.equal(gb, eager_b) and torch.equal(ga2, eager_a)
    hip.check_faults()


# ------------------------------------------------------------------------------------- stage-3 loop
def _stage3(env, tower):  # noqa: F811
    """test_stage3_gpu._run at B = 1 with `tower` as the loop's text encoder: (product latent, oracle latent)."""
    import numpy as np
    from oracle.sampler_ref import SpacedScheduleRef, diffusion_betas, p_sample_v
    from tair_amd.diffusion import Diffusion
    from tair_amd.sampler import SpacedSampler
    m, ref, det, _, clip_ref = env
    gen = torch.Generator().manual_seed(32)
    x_T = torch.randn(1, 4, 32, 32, generator=gen).cuda()
    c_img = torch.randn(1, 4, 32, 32, generator=gen).cuda()
    c0 = torch.randn(1, 77, 1024, generator=gen).cuda()
    noise = torch.randn(STEPS, 1, 4, 32, 32, generator=gen).cuda()
    s = SpacedSampler(Diffusion(linear_start=0.00085, linear_end=0.012, zero_snr=True, parameterization="v").betas,
                      "v", False)
    with torch.no_grad():
        z, res = s.val_sample(m, "cuda", STEPS, tuple(x_T.shape), {"c_txt": c0, "c_img": c_img}, x_T=x_T, noise=noise,
                              ts_model=Spy(det), text_encoder=lambda t: tower(byte_tokens(t).cuda()),
                              prompt_style="CAPTION")
        sched = SpacedScheduleRef(diffusion_betas(), STEPS)
        ts = np.flip(sched.timesteps)
        x, ctx = x_T, c0
        for i in range(STEPS):
            mt = torch.full((1,), int(ts[i]), dtype=torch.long, device="cuda")
            v, _ = ref(x, mt, {"c_txt": ctx, "c_img": c_img})
            x = p_sample_v(sched, x, v, STEPS - i - 1, noise[i])
            ctx = clip_ref(byte_tokens([res[i]["pred_prompt"]]).cuda())  # the oracle CLIP on the product's prompts
    assert sum(len(r["pred_texts"]) for r in res) > 0
    return z, x


def test_stage3_loop_with_hip_tower(env):  # noqa: F811
    from tair_amd.clip_hip import HipTextTower
    from tair_amd.sampler import _check_device_faults
    _, _, _, clip, _ = env
    hip = HipTextTower(clip, max_batch=2)
    z, zr = _stage3(env, hip)
    e_hip = rel(z, zr)
    z, zr = _stage3(env, clip)
    e_stock = rel(z, zr)
    print(f"stage3 B=1, {STEPS} steps: latent rel-L2 HIP tower {e_hip:.3e}, stock tower {e_stock:.3e}")
    assert e_hip <= 5e-3, e_hip
    _check_device_faults(torch.device("cuda"), "stage 3 with the HIP text tower")
