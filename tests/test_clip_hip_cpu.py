"""The HIP text tower's host side (tair_amd/clip_hip.py), no GPU: the GEMM plans of the tower's four linears
(tair_k_gemm_plan is a host routine), the GELU activation code's validation, weight packing, and the
``clip_backend`` argument."""
import ctypes

import pytest
import torch


def _plan(M, N, K, act=0, stream_res=False, **kw):
    from tair_amd import _lib
    L = _lib.lib()
    assert L.tair_k_gemm_desc_bytes() == ctypes.sizeof(_lib.GemmDesc)
    d = _lib.GemmDesc()
    d.M, d.N, d.K, d.amode = M, N, K, 0
    fake = 1 << 20  # planning reads no operand: any aligned non-null address
    d.A, d.lda, d.Wt, d.ldw, d.bias = fake, K, fake, K, fake
    d.alpha, d.act, d.rows_per_b = 1.0, act, 1
    d.out, d.ldo = fake, N
    if stream_res:  # the two-plane residual stream, read and rewritten in place
        d.res, d.ld_res, d.res_lo, d.out_lo, d.ldo = fake, 2 * N, N, N, 2 * N
    d.partial, d.partial_cap = fake, 6 * 640 * 4096
    d.tile_sem, d.sem_cap = fake, 32768
    for k, v in kw.items():
        setattr(d, k, v)
    out = [ctypes.c_int() for _ in range(4)]
    rc = L.tair_k_gemm_plan(ctypes.byref(d), *[ctypes.byref(o) for o in out])
    return rc, [o.value for o in out], (L.tair_last_error() or b"").decode()


TOWER_GEMMS = [(3072, 1024, 0, False), (1024, 1024, 0, True), (4096, 1024, 3, False), (1024, 4096, 0, True)]


@pytest.mark.parametrize("M", [77, 616])
@pytest.mark.parametrize("N,K,act,res", TOWER_GEMMS)
def test_tower_gemm_plans(M, N, K, act, res):
    rc, (bm, bn, splits, kern), msg = _plan(M, N, K, act, res)
    assert rc == 0, msg
    assert bm in (64, 128) and bn in (64, 128) and 1 <= splits <= 16


def test_unknown_activation_is_an_error():
    rc, _, msg = _plan(77, 4096, 1024, act=4)
    assert rc != 0 and "act 4" in msg
    rc, _, msg = _plan(77, 4096, 1024, act=-1)
    assert rc != 0


def test_gelu_refused_by_plans_that_do_not_carry_it():
    """A forced wide tile would run an epilogue without the activation: refused, never skipped; the plan query
    reports the status the launch would."""
    assert _plan(154, 4096, 1024, act=3, force_bm=64, force_bn=128)[0] == 0
    assert _plan(154, 4096, 1024, act=3, force_bm=64, force_bn=64, force_splits=4)[0] == 0
    rc, _, msg = _plan(154, 4096, 1024, act=3, force_bm=256, force_bn=128)
    assert rc != 0 and "GELU" in msg
    rc, _, msg = _plan(4096, 5120, 1280, act=3, force_bm=256, force_bn=256, force_stages=4)
    assert rc != 0 and "GELU" in msg
    rc, _, msg = _plan(154, 4096, 1024, act=3, out_split=1, ldo=3 * 4096)
    assert rc != 0 and "GELU" in msg


def _stock(width=128, layers=3, vocab=50, layer="penultimate"):
    from tair_amd.clip import FrozenOpenCLIPEmbedder
    m = FrozenOpenCLIPEmbedder(width, text_cfg=dict(width=width, layers=layers, heads=width // 64, vocab_size=vocab),
                               layer=layer).eval()
    g = torch.Generator().manual_seed(3)
    with torch.no_grad():
        for p in m.parameters():
            p.copy_(torch.randn(p.shape, generator=g) * 0.05)
    return m


def test_pack_unpack_reproduces_bf16_weights_and_fp32_rest():
    from tair_amd import clip_hip
    sd = _stock().state_dict()
    packed = clip_hip.pack_state_dict(sd)
    assert packed["w_qkv"].shape == (3, 384, 128) and packed["w_qkv"].dtype == torch.bfloat16
    assert packed["w_proj"].shape == (3, 128, 512) and packed["b_fc"].shape == (3, 512)
    assert all(t.is_contiguous() for t in packed.values())
    back = clip_hip.unpack_state_dict(packed)
    unused = {"model.text_projection", "model.logit_scale"}
    assert set(back) == set(sd) - unused
    for k, v in back.items():
        linear = k.endswith(("in_proj_weight", "out_proj.weight", "c_fc.weight", "c_proj.weight"))
        if linear:
            assert v.dtype == torch.bfloat16 and torch.equal(v, sd[k].to(torch.bfloat16)), k
        else:
            assert v.dtype == torch.float32 and torch.equal(v, sd[k]), k


def test_pack_needs_blocks():
    from tair_amd import _lib, clip_hip
    with pytest.raises(_lib.TairError):
        clip_hip.pack_state_dict({"model.positional_embedding": torch.zeros(77, 128)})


def test_clip_backend_argument():
    from tair_amd import _lib
    from tair_amd.cldm import ControlLDM
    from tair_amd.clip import FrozenOpenCLIPEmbedder
    from tair_amd.clip_hip import build_text_tower
    cfg = dict(embed_dim=128, text_cfg=dict(width=128, layers=1, heads=2, vocab_size=20))
    assert type(build_text_tower(cfg, device="cpu")) is FrozenOpenCLIPEmbedder  # the default: the stock class
    assert type(build_text_tower(cfg, "torch", device="cpu")) is FrozenOpenCLIPEmbedder
    with pytest.raises(ValueError):
        build_text_tower(cfg, "triton", device="cpu")
    with pytest.raises(ValueError):  # checked before anything touches a device
        ControlLDM(clip_cfg=cfg, clip_backend="rocblas", device="cpu")
    with pytest.raises(_lib.TairError):  # no CPU fallback
        build_text_tower(cfg, "hip", device="cpu")


def test_val_tools_take_the_flag():
    import inspect

    from tair_amd import config, val, val_patches
    assert inspect.signature(config.build_model).parameters["clip_backend"].default == "torch"
    a = val._parse(["--clip-backend", "hip"])
    assert a.clip_backend == "hip" and val._parse([]).clip_backend == "torch"
    assert "--clip-backend" in inspect.getsource(val_patches._parse)
