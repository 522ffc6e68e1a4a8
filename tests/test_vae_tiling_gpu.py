"""Tiled VAE on the HIP kernels (HipVAEDecoder.decode_tiled, HipVAEEncoder.encode_mode_tiled through
ControlLDM.prepare_condition) against the restatement of the reference's tiled VAE (tests/_tiled_vae_ref.py over
oracle/vae_ref.py, torch fp32), with full-width synthetic weights as tests/test_vae_gpu.py.  The restatement runs on
the CPU: on the device every new tile shape costs the convolution library a kernel search (13 s for the six-tile case
against 2 s on 16 CPU threads).

Gates (written here):
* tiled decode / encode vs the restatement: rel-L2 <= 2e-4, the gate of tests/test_vae_gpu.py with its reasoning
  unchanged (split planes hi + lo carry ~16 mantissa bits per product; the statistics and their merge are fp64).
  tests/test_vae_tiling_cpu.py shows that this gate tells the merge rule from its neighbours (>= 10 x 2e-4).
  Measured: decode 4.8e-5 (B=1, 40x32) and 4.7e-5 (B=2, 32x24), encode 1.9e-5; the untiled results are 2.1e-1 to
  4.3e-1 away.
* tair_k_gn_stats_merge vs torch fp64: the (mean, var) recovered from every rewritten slot within 1e-12 relative;
  replicas 1-7 exactly zero; doubles of a replica past the B * G pairs untouched.
* tair_k_softmax_split_pad at L = 900: hi + lo vs the fp64 softmax rel-L2 <= 1e-5 (the gate of the Downsample kernel
  test), columns L..Lp of every plane exactly zero, with 1e30 in the padded columns of S (they must never reach the
  max / sum).  tair_k_transpose_split_pad: bitwise, padded columns exactly zero.
* the tiny rule: bitwise decode().
"""
import ctypes
import json
import os

import pytest
import torch

import _tiled_vae_ref as tr
from test_cldm_gpu import OUT  # the suite's directory for measured parity values (parity.jsonl)

pytestmark = pytest.mark.gpu

GATE = 2e-4


def rel_l2(a, b):
    a, b = a.double(), b.double()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def _log(test, value):
    os.makedirs(OUT, exist_ok=True)
    with open(os.path.join(OUT, "parity.jsonl"), "a") as f:
        f.write(json.dumps({"test": test, "rel_l2": value}) + "\n")


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


@pytest.fixture(scope="module")
def vaes():
    from oracle.vae_ref import AutoencoderKLRef
    from tair_amd.pipeline import vae_synthetic_state_dict
    from tair_amd.vae import AutoencoderKL
    from tair_amd.vae_hip import HipVAEDecoder
    ref = AutoencoderKLRef().eval()  # fp32 on the CPU
    sd = vae_synthetic_state_dict(ref, seed=0)
    ref.load_state_dict(sd, strict=True)
    prod = AutoencoderKL().cuda().eval()
    prod.load_state_dict(sd, strict=True)
    return ref, HipVAEDecoder(prod, "cuda", max_batch=2)


@pytest.mark.parametrize("B,h,w", [(1, 40, 32),   # six tiles 30x30 / 30x24 / 24x30 / 24x24: unequal pixel weights,
                                                  # L = 900 / 720 / 576, M off multiples of 64
                                   (2, 32, 24)])  # statistics per image
@torch.no_grad()
def test_hip_tiled_decode_vs_restatement(vaes, B, h, w):
    ref, hip = vaes
    z = tr.ramp_latent(B, h, w, seed=7)
    want = tr.decode_tiled(ref, z, 8)
    z = z.cuda()
    out = hip.decode_tiled(z, 8).cpu()
    assert out.shape == want.shape == (B, 3, 8 * h, 8 * w)
    assert torch.isfinite(out).all()
    e = rel_l2(out, want)
    e_untiled = rel_l2(hip.decode(z).cpu(), want)
    print(f"hip tiled decode B={B} {h}x{w}: rel-L2 {e:.3e} (the untiled decode is {e_untiled:.3e} away)")
    _log(f"vae_hip_decode_tiled_b{B}_{h}x{w}", e)
    assert e <= GATE, e
    assert e_untiled >= 10 * GATE  # the tiled algorithm, not the untiled one


@torch.no_grad()
def test_hip_tiled_encode_through_prepare_condition(vaes):
    from tair_amd.cldm import ControlLDM
    from tair_amd.pipeline import vae_synthetic_state_dict
    ref, _ = vaes
    m = ControlLDM(max_batch=2, with_vae=True)
    try:
        m.vae.load_state_dict(vae_synthetic_state_dict(m.vae, seed=0), strict=True)
        assert m.vae_tiling and m.vae_backend == "hip"
        clean = torch.rand(1, 3, 200, 128, generator=torch.Generator().manual_seed(9))
        clean = (clean * 0.6 + 0.2 + 0.2 * torch.linspace(-1, 1, 200).view(1, 1, 200, 1)).cuda()
        c_txt = torch.randn(1, 77, 1024, device="cuda")
        cond = m.prepare_condition(clean, c_txt=c_txt, tiled=True, tile_size=64)
        want = tr.encode_mode_tiled(ref, clean.cpu() * 2 - 1, 64) * 0.18215
        assert cond["c_img"].shape == want.shape == (1, 4, 25, 16)
        assert m._vae_hip_enc is not None  # the HIP encoder really ran
        e = rel_l2(cond["c_img"].cpu(), want)
        e_untiled = rel_l2(m.prepare_condition(clean, c_txt=c_txt)["c_img"].cpu(), want)
        print(f"hip tiled encode 200x128: rel-L2 {e:.3e} (the untiled encode is {e_untiled:.3e} away)")
        _log("vae_encode_cond_tiled_hip_b1_200x128", e)
        assert e <= GATE, e
        # vae_decode passes the flags on too (tiny rule: 25 <= 22 + 8)
        z = cond["c_img"]
        assert torch.equal(m.vae_decode(z, tiled=True, tile_size=8), m.vae_decode(z))
    finally:
        m.close()


@torch.no_grad()
def test_hip_tiny_rule_is_bitwise_decode(vaes):
    _, hip = vaes
    z = torch.randn(2, 4, 30, 24, generator=torch.Generator().manual_seed(1)).cuda()  # 30 = 2 * 11 + 8
    assert torch.equal(hip.decode_tiled(z, 8), hip.decode(z))


def test_gn_stats_merge_against_fp64():
    from tair_amd import _lib
    L = _lib.lib()
    T, B, G, cg, rs, R = 3, 2, 32, 16, 192, 8  # rs > 2 B G: a pool sized for a larger batch
    px = [900, 720, 576]
    g = torch.Generator().manual_seed(21)
    mean_t = torch.randn(T, B * G, generator=g, dtype=torch.float64) * 0.5 + 3  # (away from 0: relative errors)
    var_t = torch.rand(T, B * G, generator=g, dtype=torch.float64) * 3 + 0.1
    cnt = torch.tensor(px, dtype=torch.float64).view(T, 1) * cg
    sums = torch.stack([mean_t * cnt, (var_t + mean_t * mean_t) * cnt], dim=-1)  # [T][B*G][2]
    share = torch.rand(T, R, B * G, 2, generator=g, dtype=torch.float64) + 0.1  # every replica populated
    share = share / share.sum(dim=1, keepdim=True)
    slots = torch.full((T, R, rs), -7.0, dtype=torch.float64)
    slots[:, :, :B * G * 2] = (share * sums.unsqueeze(1)).reshape(T, R, B * G * 2)
    # what the replicas sum to, as the kernel sees it
    tot = slots[:, :, :B * G * 2].sum(dim=1).view(T, B * G, 2)
    m_in = tot[..., 0] / cnt
    v_in = (tot[..., 1] / cnt - m_in * m_in).clamp_min(0)
    wgt = torch.tensor(px, dtype=torch.float64).view(T, 1) / sum(px)
    mean, var = (wgt * m_in).sum(0), (wgt * v_in).sum(0)
    d = slots.cuda()
    arr = (ctypes.c_int * T)(*px)
    assert L.tair_k_gn_stats_merge(d.data_ptr(), R * rs, T, arr, B, G, cg, rs, _stream()) == 0
    torch.cuda.synchronize()
    got = d.cpu()
    assert torch.equal(got[:, 1:, :B * G * 2], torch.zeros(T, R - 1, B * G * 2, dtype=torch.float64))
    assert torch.equal(got[:, :, B * G * 2:], slots[:, :, B * G * 2:])  # past the B * G pairs: untouched
    r0 = got[:, 0, :B * G * 2].view(T, B * G, 2)
    m_out = r0[..., 0] / cnt
    v_out = r0[..., 1] / cnt - m_out * m_out
    em = ((m_out - mean).abs() / mean.abs()).max().item()
    ev = ((v_out - var).abs() / var.abs()).max().item()
    print(f"gn_stats_merge: worst relative error mean {em:.3e}, var {ev:.3e}")
    assert em <= 1e-12 and ev <= 1e-12, (em, ev)
    # the merge is the reference's weighted average of variances, not the union's variance
    union = (wgt * (v_in + m_in * m_in)).sum(0) - mean * mean
    assert ((union - var).abs() / var).mean().item() > 1e-2  # (Σ w (mean_t - mean)² against var ~ 1.5)


def test_softmax_split_pad_against_fp64():
    from tair_amd import _lib
    Lb = _lib.lib()
    rows, L, Lp = 96, 900, 960
    g = torch.Generator().manual_seed(33)
    S = torch.randn(rows, Lp, generator=g) * 4
    S[:, L:] = 1e30  # padded lanes: a read would take over the max and zero the row
    P = torch.full((rows, 3 * Lp), 3.0, dtype=torch.bfloat16, device="cuda")
    Sd = S.cuda()
    assert Lb.tair_k_softmax_split_pad(Sd.data_ptr(), Lp, rows, L, Lp, P.data_ptr(), _stream()) == 0
    torch.cuda.synchronize()
    p = P.cpu().view(rows, 3, Lp)
    assert torch.equal(p[:, :, L:], torch.zeros(rows, 3, Lp - L, dtype=torch.bfloat16))
    assert torch.equal(p[:, 0], p[:, 2])
    want = torch.softmax(S[:, :L].double(), dim=-1)
    e = rel_l2(p[:, 0, :L].double() + p[:, 1, :L].double(), want)
    print(f"softmax_split_pad L={L}: rel-L2 {e:.3e}")
    assert e <= 1e-5, e


def test_transpose_split_pad_bitwise():
    from tair_amd import _lib
    Lb = _lib.lib()
    B, L, Lp, C = 2, 900, 960, 128
    g = torch.Generator().manual_seed(35)
    x = torch.randn(B, L, 3 * C, generator=g).to(torch.bfloat16)
    y = torch.full((B, C, 3 * Lp), 3.0, dtype=torch.bfloat16, device="cuda")
    xd = x.cuda()
    assert Lb.tair_k_transpose_split_pad(xd.data_ptr(), B, L, Lp, C, y.data_ptr(), _stream()) == 0
    torch.cuda.synchronize()
    got = y.cpu().view(B, C, 3, Lp)
    hi, lo = x[:, :, :C].transpose(1, 2), x[:, :, C:2 * C].transpose(1, 2)  # [B][C][L]
    assert torch.equal(got[:, :, 0, :L], hi) and torch.equal(got[:, :, 1, :L], hi) and torch.equal(got[:, :, 2, :L], lo)
    assert torch.equal(got[:, :, :, L:], torch.zeros(B, C, 3, Lp - L, dtype=torch.bfloat16))
