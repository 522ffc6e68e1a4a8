"""The SwinIR cleaner on the HIP kernels (tair_amd/swinir_hip.py, csrc/swinir.hip): every new kernel through the C ABI
against fp64 on the same bf16 operands, the network against the oracle (oracle/swinir_ref.py), graph replay, and
restore_image with the HIP cleaner.

Operands sit in buffers with guard rows and padded leading dimensions: inputs are surrounded by NaN (a read outside
the operand poisons the result), outputs by a sentinel that must survive.

Gates (none is derived from what the code gives):
* window attention: rel-L2 <= 1e-2 against fp64, the project's attention gate (test_clip_hip_gpu.py ATTN_GATE: P is
  rounded to bf16 before P V); the reference is the module's own formulation (torch.roll, window partition,
  _rel_index, shift_mask), not the kernel's addressing;
* padded LayerNorm: one bf16 rounding of an fp32 value, 1.3 x the rounding floor rel-L2(bf16(ref), ref) of the fp64
  reference (test_clip_hip_gpu.py FLOOR_RATIO); pad columns exactly zero;
* LeakyReLU: bitwise F.leaky_relu on bf16;
* network: rel-L2(HIP, oracle) <= 1.5 x rel-L2(emulation, oracle), the emulation (tests/_swinir_emul.py) being stock
  torch with the HIP path's bf16 rounding points and an fp32 stream: 1.5 x allows for accumulation order and the
  hi + lo stream's ~2^-16 step; a missed rounding point or the padded head dim's scale shows as >= 2 x
  (test_swinir_hip_cpu.py test_gate_has_teeth).
"""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from tests._swinir_emul import emulate, randomize

pytestmark = pytest.mark.gpu

ATTN_GATE = 1e-2
FLOOR_RATIO = 1.3
NAN = float("nan")
REDUCED = dict(depths=[2, 2], num_heads=[6, 6])


def rel(a, b):
    a, b = a.double(), b.double().to(a.device)
    return ((a - b).norm() / b.norm()).item()


def _L():
    from tair_amd import _lib
    return _lib.lib()


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


# --------------------------------------------------------------------------------- window attention
def _attn_run(qkv, o, B, heads, H, W, d, shift, table, scale):
    L = _L()
    Cw, ld = heads * 32, qkv.stride(0)
    rc = L.tair_k_window_attention(_p(qkv), ld, _p(qkv[:, Cw:]), ld, _p(qkv[:, 2 * Cw:]), ld, _p(o), o.stride(0), B, H, W,
                                   heads, d, shift, _p(table), scale, _stream())
    assert rc == 0, L.tair_last_error()
    torch.cuda.synchronize()


def _attn_ref(qkv, B, heads, H, W, d, shift, table, scale):
    """fp64, the module's formulation (swinir.py _Block / _Attn): roll, partition, bias by _rel_index, shift_mask."""
    from tair_amd.swinir import _from_windows, _rel_index, _to_windows, shift_mask
    x = qkv.contiguous().double().view(B, H, W, 3, heads, 32)[..., :d].reshape(B, H, W, 3 * heads * d)
    if shift:
        x = torch.roll(x, (-shift, -shift), (1, 2))
    win = _to_windows(x, 8)
    n = win.shape[0]
    q, k, v = win.reshape(n, 64, 3, heads, d).permute(2, 0, 3, 1, 4)
    s = q @ k.transpose(-1, -2) * scale
    s = s + table.double()[_rel_index(8).reshape(-1).cuda()].reshape(64, 64, heads).permute(2, 0, 1)[None]
    if shift:
        m = shift_mask(H, W, 8, shift).double().cuda()
        s = (s.reshape(B, m.shape[0], heads, 64, 64) + m[None, :, None]).reshape(n, heads, 64, 64)
    o = (torch.softmax(s, -1) @ v).transpose(1, 2).reshape(n, 64, heads * d)
    o = _from_windows(o, 8, B, H, W)
    if shift:
        o = torch.roll(o, (shift, shift), (1, 2))
    return o.reshape(B * H * W, heads, d)


def _attn_case(B, heads, H, W, d, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    T, Cw = B * H * W, heads * 32
    ibuf, qkv = _guarded(T, 3 * Cw, NAN, pad=64)  # q | k | v strided out of one fused buffer
    x = torch.randn(T, 3 * Cw, device="cuda", generator=g)
    x[:, :2 * Cw] *= 2  # q, k (test_attention's operands)
    qkv.copy_(x.to(torch.bfloat16))
    if d < 32:  # the pad columns of every head of q, k and v hold NaN: they are never used
        qkv.view(T, 3 * heads, 32)[:, :, d:] = NAN
    table = torch.randn(225, heads, device="cuda", generator=g) * 0.5
    return qkv, table


ATTN_SHAPES = [(1, 1, 8, 8, 0, 30), (1, 1, 8, 8, 4, 30), (1, 6, 16, 16, 4, 30), (2, 6, 16, 24, 4, 30),
               (1, 6, 64, 64, 0, 30), (1, 6, 64, 64, 4, 30), (2, 6, 16, 24, 4, 32)]


@pytest.mark.parametrize("B,heads,H,W,shift,d", ATTN_SHAPES)
def test_window_attention(B, heads, H, W, shift, d):
    scale = d ** -0.5
    qkv, table = _attn_case(B, heads, H, W, d, seed=B + 10 * heads + H + W + shift + d)
    T = B * H * W
    obuf, o = _guarded(T, heads * 32, 7.0)
    _attn_run(qkv, o, B, heads, H, W, d, shift, table, scale)
    ov = o.contiguous().view(T, heads, 32)
    assert bool(torch.isfinite(ov).all())
    assert bool((ov[:, :, d:] == 0).all())  # o's pad columns are written, as zeros
    e = rel(ov[:, :, :d], _attn_ref(qkv, B, heads, H, W, d, shift, table, scale))
    print(f"window attention B={B} heads={heads} {H}x{W} shift={shift} d={d}: rel-L2 {e:.2e}")
    assert e <= ATTN_GATE, e
    assert _guards_intact(obuf, o, 7.0)


def test_window_attention_windows_are_independent():
    """shift 0: a window's output is bitwise unchanged when another window's k / v rows change."""
    B, heads, H, W, d = 1, 6, 16, 16, 30
    qkv, table = _attn_case(B, heads, H, W, d, seed=3)
    _, o = _guarded(H * W, heads * 32, 7.0)
    _attn_run(qkv, o, B, heads, H, W, d, 0, table, d ** -0.5)
    q2buf, qkv2 = _guarded(H * W, 3 * heads * 32, NAN, pad=64)
    qkv2.copy_(qkv)
    v2 = qkv2.view(H, W, 3 * heads * 32)
    g = torch.Generator(device="cuda").manual_seed(4)
    v2[8:, 8:, heads * 32:] = (torch.randn(8, 8, 2 * heads * 32, device="cuda", generator=g) * 3).to(torch.bfloat16)  # window (1, 1)
    _, o2 = _guarded(H * W, heads * 32, 7.0)
    _attn_run(qkv2, o2, B, heads, H, W, d, 0, table, d ** -0.5)
    a, b = o.contiguous().view(H, W, -1), o2.contiguous().view(H, W, -1)
    same = torch.ones(H, W, dtype=torch.bool, device="cuda")
    same[8:, 8:] = False
    assert torch.equal(a[same].view(torch.int16), b[same].view(torch.int16))
    assert not torch.equal(a[8:, 8:], b[8:, 8:])


@pytest.mark.parametrize("bad", [dict(H=12), dict(W=0), dict(d=33), dict(d=0), dict(shift=8), dict(shift=-1), dict(heads=0),
                                 dict(ld=100), dict(scale=0.0), dict(table=None)])
def test_window_attention_refuses_bad_arguments(bad):
    L = _L()
    a = dict(B=1, H=16, W=16, heads=6, d=30, shift=4, ld=576, scale=0.18, table=1)
    a.update(bad)
    qkv = torch.zeros(256, 576, device="cuda", dtype=torch.bfloat16)
    o = torch.full((256, 192), 7.0, device="cuda", dtype=torch.bfloat16)
    table = torch.zeros(225, 6, device="cuda")
    rc = L.tair_k_window_attention(_p(qkv), a["ld"], _p(qkv[:, 192:]), a["ld"], _p(qkv[:, 384:]), a["ld"], _p(o), 192, a["B"],
                                   a["H"], a["W"], a["heads"], a["d"], a["shift"], _p(table) if a["table"] else None,
                                   a["scale"], _stream())
    torch.cuda.synchronize()
    assert rc == -1 and b"window_attention" in L.tair_last_error()
    assert bool((o == 7.0).all())  # nothing was launched


# ----------------------------------------------------------------------------------- LayerNorm pad
def _ln_inputs(T, C, planes, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.randn(T, C, device="cuda", generator=g) * (torch.rand(T, 1, device="cuda", generator=g) + 0.5) + \
        torch.randn(T, 1, device="cuda", generator=g) * 1.5
    hi = x.to(torch.bfloat16)
    lo = (x - hi.float()).to(torch.bfloat16)
    gamma = torch.rand(C, device="cuda", generator=g) + 0.5
    beta = torch.randn(C, device="cuda", generator=g) * 0.2
    return hi, lo, gamma, beta


@pytest.mark.parametrize("T", [1, 5, 4096])
@pytest.mark.parametrize("planes", [1, 2])
def test_layernorm_split_pad(T, planes):
    L = _L()
    C, Cp = 180, 192
    hi, lo, gamma, beta = _ln_inputs(T, C, planes, seed=T + planes)
    _, xin = _guarded(T, 2 * Cp, NAN)  # columns C..Cp of both planes stay NaN: the statistics never read them
    xin[:, :C] = hi
    if planes == 2:
        xin[:, Cp:Cp + C] = lo
    obuf, y = _guarded(T, Cp, 7.0)
    rc = L.tair_k_layernorm_split_pad(_p(xin), xin.stride(0), Cp if planes == 2 else 0, T, C, Cp, _p(gamma), _p(beta), 1e-5,
                                      _p(y), y.stride(0), _stream())
    assert rc == 0, L.tair_last_error()
    torch.cuda.synchronize()
    x64 = hi.double() + (lo.double() if planes == 2 else 0)
    ref = F.layer_norm(x64, (C,), gamma.double(), beta.double(), 1e-5)
    e, fl = rel(y[:, :C], ref), _floor(ref)
    print(f"layernorm_split_pad T={T} planes={planes}: rel-L2 {e:.3e} (floor {fl:.3e}, ratio {e / fl:.3f})")
    assert e <= FLOOR_RATIO * fl, (e, fl)
    assert bool((y[:, C:] == 0).all())
    assert _guards_intact(obuf, y, 7.0)


def test_layernorm_split_pad_refuses_bad_arguments():
    L = _L()
    x = torch.zeros(8, 384, device="cuda", dtype=torch.bfloat16)
    y = torch.full((8, 192), 7.0, device="cuda", dtype=torch.bfloat16)
    g = torch.ones(192, device="cuda")
    for C, Cp, ldy in [(182, 192, 192), (180, 176, 192), (180, 192, 188), (180, 190, 192)]:
        rc = L.tair_k_layernorm_split_pad(_p(x), 384, 192, 8, C, Cp, _p(g), _p(g), 1e-5, _p(y), ldy, _stream())
        assert rc == -1 and b"layernorm_split_pad" in L.tair_last_error()
    torch.cuda.synchronize()
    assert bool((y == 7.0).all())


def test_layernorm_split_keeps_its_code_path():
    """tair_k_layernorm_split at C = 1024 (its own kernel, untouched): against a torch fp32 LayerNorm of hi + lo at
    test_clip_hip_gpu.py test_layernorm_split's gates, and not through the padded entry point (C % 8 == 0 there too,
    but the two are separate kernels)."""
    L = _L()
    T, C = 77, 1024
    hi, lo, gamma, beta = _ln_inputs(T, C, 2, seed=11)
    xin = torch.cat([hi, lo], 1).contiguous()
    for f32 in (0, 1):
        y = torch.empty(T, C, device="cuda", dtype=torch.float32 if f32 else torch.bfloat16)
        assert L.tair_k_layernorm_split(_p(xin), 2 * C, C, T, C, _p(gamma), _p(beta), 1e-5, _p(y), C, f32, _stream()) == 0
        torch.cuda.synchronize()
        ref32 = F.layer_norm(hi.float() + lo.float(), (C,), gamma, beta, 1e-5)
        ref = F.layer_norm(hi.double() + lo.double(), (C,), gamma.double(), beta.double(), 1e-5)
        assert rel(y, ref) <= (1e-5 if f32 else FLOOR_RATIO * _floor(ref))
        assert rel(y, ref32) <= (2e-5 if f32 else 2 * FLOOR_RATIO * _floor(ref))


# --------------------------------------------------------------------------------------- LeakyReLU
@pytest.mark.parametrize("slope", [0.01, 0.2])
@pytest.mark.parametrize("rows,C", [(1, 8), (7, 64), (1000, 64)])
def test_leaky_relu_bitwise(rows, C, slope):
    L = _L()
    g = torch.Generator(device="cuda").manual_seed(rows + C)
    buf, x = _guarded(rows, C, 7.0)
    src = (torch.randn(rows, C, device="cuda", generator=g) * 4).to(torch.bfloat16)
    src[0, :2] = torch.tensor([0.0, -0.0], device="cuda").to(torch.bfloat16)
    x.copy_(src)
    assert x.stride(0) > C
    rc = L.tair_k_leaky_relu(_p(x), x.stride(0), rows, C, slope, _stream())
    assert rc == 0, L.tair_last_error()
    torch.cuda.synchronize()
    assert torch.equal(x.contiguous().view(torch.int16), F.leaky_relu(src, slope).view(torch.int16))
    assert _guards_intact(buf, x, 7.0)
    assert L.tair_k_leaky_relu(_p(x), x.stride(0), rows, C + 4, slope, _stream()) == -1


# ----------------------------------------------------------------------------------------- network
def _models(params_over, seed, max_batch, max_hw):
    from tair_amd.config import SWINIR_VAL_PARAMS
    from tair_amd.swinir import SwinIR
    from tair_amd.swinir_hip import HipSwinIR
    torch.backends.cuda.matmul.allow_tf32 = False
    torch.backends.cudnn.allow_tf32 = False
    p = dict(SWINIR_VAL_PARAMS, **params_over)
    stock = randomize(SwinIR(**p), seed).eval()
    hip = HipSwinIR(stock, p, max_batch=max_batch, max_hw=max_hw, device="cuda")
    return stock, p, hip


@pytest.fixture(scope="module")
def reduced():
    return _models(REDUCED, 5, 2, (24, 16))


def _parity(stock, p, hip, x):
    from oracle.swinir_ref import swinir_forward_ref
    sd = stock.state_dict()
    want = swinir_forward_ref(sd, p, x)
    got = hip(x.cuda())
    emu = emulate({k: v.cuda() for k, v in sd.items()}, p["depths"], x.cuda())
    assert got.dtype == torch.float32 and tuple(got.shape) == tuple(want.shape)
    return rel(got, want), rel(emu, want), (got.cpu() - want).abs().max().item()


@pytest.mark.parametrize("shape", [(1, 3, 128, 128), (2, 3, 192, 128)])
def test_network_matches_oracle(reduced, shape):
    stock, p, hip = reduced
    x = torch.rand(shape, generator=torch.Generator().manual_seed(shape[0]))
    e_hip, e_emu, amax = _parity(stock, p, hip, x)
    print(f"SwinIR reduced {shape}: HIP {e_hip:.3e}, emulation {e_emu:.3e}, ratio {e_hip / e_emu:.2f}, max |d| {amax:.3e}")
    assert e_hip <= 1.5 * e_emu, (e_hip, e_emu)
    hip.check_faults()


def test_full_network_matches_oracle():
    stock, p, hip = _models({}, 6, 1, (64, 64))
    x = torch.rand((1, 3, 512, 512), generator=torch.Generator().manual_seed(2))
    e_hip, e_emu, amax = _parity(stock, p, hip, x)
    print(f"SwinIR val config 512^2: HIP {e_hip:.3e}, emulation {e_emu:.3e}, ratio {e_hip / e_emu:.2f}, "
          f"max |HIP - oracle| {amax:.3e}; {hip.launch_count(1)} launches")
    assert e_hip <= 1.5 * e_emu, (e_hip, e_emu)
    hip.check_faults()


def test_network_loads_reference_keys_in_place_and_checks_inputs(reduced):
    stock, p, hip = reduced
    x = torch.rand((1, 3, 128, 128), generator=torch.Generator().manual_seed(7)).cuda()
    before = hip(x)
    ptr = hip.w_fc1.data_ptr()
    sd = {k: v.clone() for k, v in stock.state_dict().items()}
    sd["layers.1.residual_group.blocks.0.mlp.fc1.bias"] += 0.5
    hip.load_state_dict(sd)
    assert hip.w_fc1.data_ptr() == ptr and rel(hip(x), before) > 1e-4
    hip.load_state_dict(stock.state_dict())
    assert torch.equal(hip(x), before)
    with pytest.raises(RuntimeError):
        hip.load_state_dict({k: v for k, v in stock.state_dict().items() if k != "norm.bias"})
    three = torch.rand((3, 3, 128, 128), generator=torch.Generator().manual_seed(8)).cuda()  # more than max_batch (2)
    out3 = hip(three)
    assert torch.equal(out3[:2], hip(three[:2])) and torch.equal(out3[2:], hip(three[2:]))
    for shape in [(1, 3, 96, 64), (1, 3, 256, 192)]:  # not a multiple of 64; larger than the workspaces
        with pytest.raises(ValueError):
            hip(torch.zeros(shape, device="cuda"))


# ------------------------------------------------------------------------------------------- graph
def test_graph_replay_is_bitwise_eager_and_stateless(reduced):
    _, _, hip = reduced
    g = torch.Generator().manual_seed(9)
    a, b = (torch.rand((2, 3, 192, 128), generator=g).cuda() for _ in range(2))
    eager_a, eager_b = hip(a), hip(b)
    assert not torch.equal(eager_a, eager_b)
    xin = a.clone()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        hip(xin)  # (warm-up on the side stream: plans and first-use setup outside the capture)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = hip(xin)
    outs = []
    for src in (a, b, a):
        xin.copy_(src)
        graph.replay()
        outs.append(out.clone())
    torch.cuda.synchronize()
    assert torch.equal(outs[0], eager_a) and torch.equal(outs[1], eager_b) and torch.equal(outs[2], eager_a)
    hip.check_faults()


# ----------------------------------------------------------------------------------------- surface
def test_restore_image_with_the_hip_cleaner():
    import glob
    import os

    import numpy as np
    from PIL import Image

    from tair_amd.cldm import ControlLDM
    from tair_amd.config import SWINIR_VAL_PARAMS, build_swinir
    from tair_amd.diffusion import Diffusion
    from tair_amd.pipeline import vae_synthetic_state_dict
    from tair_amd.sampler import SpacedSampler
    from tair_amd.swinir_hip import HipSwinIR
    from tair_amd.val_patches import restore_image
    from tair_amd.weights import perturb_norms, synthetic_state_dict
    from tests.test_val_patches_gpu import TINY
    dev = torch.device("cuda", 0)
    root = os.path.dirname(os.path.abspath(__file__))
    lq = np.asarray(Image.open(sorted(glob.glob(os.path.join(root, "golden", "lq", "*.jpg")))[0]).convert("RGB"))
    assert lq.shape == (128, 128, 3)
    m = ControlLDM(TINY, max_batch=4, device=dev)
    m.load_state_dict(perturb_norms(synthetic_state_dict(m.param_manifest(), seed=7)))
    m.vae.load_state_dict(vae_synthetic_state_dict(m.vae, seed=0))
    s = SpacedSampler(Diffusion(linear_start=0.00085, linear_end=0.012, zero_snr=True, parameterization="v").betas,
                      "v", False)
    c_txt = torch.randn(1, 77, 64, generator=torch.Generator().manual_seed(28)).to(dev)
    torch.manual_seed(12)  # (the synthetic weights leave nn.Linear / nn.Conv2d biases at their default, global-RNG init)
    stock = build_swinir(None, dev)
    torch.manual_seed(12)
    hip = build_swinir(None, dev, backend="hip", max_batch=1)
    assert isinstance(hip, HipSwinIR) and type(stock).__name__ == "SwinIR"
    seen = {}

    def spy(name, fn):
        def run(x):
            seen[name + "_in"], seen[name] = x, fn(x)
            return seen[name]
        return run
    try:
        img = restore_image(m, s, lq, c_txt, steps=2, tile_batch=4, cleaner=spy("hip", hip))
        restore_image(m, s, lq, c_txt, steps=2, tile_batch=4, cleaner=spy("stock", stock))
    finally:
        m.close()
    assert tuple(img.shape) == (1, 3, 512, 512) and bool(torch.isfinite(img).all())
    assert torch.equal(seen["hip_in"], seen["stock_in"]) and tuple(seen["hip"].shape) == (1, 3, 512, 512)
    emu = emulate(stock.state_dict(), SWINIR_VAL_PARAMS["depths"], seen["stock_in"])
    e_hip, e_emu = rel(seen["hip"], seen["stock"]), rel(emu, seen["stock"])
    print(f"restore_image cleaner, val config, synthetic weights: HIP vs torch {e_hip:.3e}, emulation {e_emu:.3e}")
    assert e_hip <= 1.5 * e_emu, (e_hip, e_emu)
    hip.check_faults()
