"""The HIP SwinIR's host side (tair_amd/swinir_hip.py), no GPU: weight packing, the kernel's coordinate mask rule, the
GEMM plans of the launch list (tair_k_gemm_plan is a host routine), the ``backend`` argument and the CLI flag, and
the parity gate's emulation (tests/_swinir_emul.py) against the oracle."""
import ctypes
import inspect

import pytest
import torch

from tests._swinir_emul import emulate, randomize

REDUCED = dict(depths=[2, 2], num_heads=[6, 6])


def rel(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm()).item()


def _stock(seed=5, **over):
    from tair_amd.config import SWINIR_VAL_PARAMS
    from tair_amd.swinir import SwinIR
    p = dict(SWINIR_VAL_PARAMS, **REDUCED)
    p.update(over)
    return randomize(SwinIR(**p), seed).eval(), p


# ------------------------------------------------------------------------------------------ packing
def test_pack_shapes_pads_and_round_trip():
    from tair_amd import swinir_hip as sh
    m, _ = _stock()
    sd = m.state_dict()
    pk = sh.pack_state_dict(sd)
    bf, f32 = torch.bfloat16, torch.float32
    want = {"w_qkv": ((4, 576, 192), bf), "b_qkv": ((4, 576), f32), "w_proj": ((4, 192, 192), bf),
            "b_proj": ((4, 192), f32), "w_fc1": ((4, 384, 192), bf), "b_fc1": ((4, 384), f32),
            "w_fc2": ((4, 192, 384), bf), "b_fc2": ((4, 192), f32), "g_ln1": ((4, 180), f32), "b_ln2": ((4, 180), f32),
            "bias_tab": ((4, 225, 6), f32), "w_gconv": ((2, 192, 1728), bf), "b_gconv": ((2, 192), f32),
            "w_first": ((192, 3456), bf), "b_first": ((192,), f32), "w_cab": ((192, 1728), bf),
            "w_cbu": ((64, 1728), bf), "w_up1": ((64, 576), bf), "w_up3": ((64, 576), bf), "w_hr": ((64, 576), bf),
            "w_last": ((3, 576), bf), "b_last": ((3,), f32), "g_pn": ((180,), f32), "b_n": ((180,), f32)}
    for name, (shape, dt) in want.items():
        assert tuple(pk[name].shape) == shape and pk[name].dtype == dt, name
    assert all(t.is_contiguous() for t in pk.values()) and pk["depths"].tolist() == [2, 2]
    # the pads are exactly zero: stream columns 180..191, head columns 30..31, hidden 360..383
    z = lambda t: bool((t == 0).all())  # noqa: E731
    assert z(pk["w_qkv"][:, :, 180:]) and z(pk["w_qkv"].view(4, 18, 32, 192)[:, :, 30:]) and z(pk["b_qkv"].view(4, 18, 32)[:, :, 30:])
    assert z(pk["w_proj"][:, 180:]) and z(pk["w_proj"].view(4, 192, 6, 32)[..., 30:]) and z(pk["b_proj"][:, 180:])
    assert z(pk["w_fc1"][:, 360:]) and z(pk["w_fc1"][:, :, 180:]) and z(pk["b_fc1"][:, 360:])
    assert z(pk["w_fc2"][:, 180:]) and z(pk["w_fc2"][:, :, 360:]) and z(pk["b_fc2"][:, 180:])
    for name in ("w_gconv", "w_cab", "w_cbu"):  # K = (chunk, tap, 64 channels): channels 180..191 sit in chunk 2
        assert z(pk[name].reshape(-1, 3, 9, 64)[:, 2, :, 52:]), name
    assert z(pk["w_gconv"][:, 180:]) and z(pk["w_cab"][180:]) and z(pk["b_gconv"][:, 180:]) and z(pk["b_first"][180:])
    wf = pk["w_first"].reshape(192, 6, 9, 64)  # two planes of 192 channels: the same weights twice
    assert torch.equal(wf[:, :3], wf[:, 3:]) and z(pk["w_first"][180:])
    # head regrouping: head h of q is rows 32 h .. 32 h + 29 of the packed weight
    w = sd["layers.0.residual_group.blocks.1.attn.qkv.weight"].to(bf)
    assert torch.equal(pk["w_qkv"][1, 192 + 2 * 32:192 + 2 * 32 + 30, :180], w[180 + 60:180 + 90])  # k, head 2
    back = sh.unpack_state_dict(pk)
    assert set(back) == {k for k in sd if not k.endswith(("relative_position_index", "attn_mask"))}
    for k, v in back.items():
        if v.dtype == bf:
            assert k.endswith("weight") and sd[k].dim() > 1 and torch.equal(v, sd[k].to(bf)), k
        else:
            assert v.dtype == f32 and torch.equal(v, sd[k]), k


def test_pack_needs_the_val_network():
    from tair_amd import _lib
    from tair_amd import swinir_hip as sh
    with pytest.raises(_lib.TairError):
        sh.pack_state_dict({"conv_first.1.weight": torch.zeros(180, 192, 3, 3)})
    from tair_amd.swinir import SwinIR
    small = SwinIR(img_size=16, embed_dim=24, depths=[2], num_heads=[2], window_size=4, mlp_ratio=2, sf=4,
                   upsampler="nearest+conv", unshuffle=True, unshuffle_scale=4)
    with pytest.raises(_lib.TairError):
        sh.pack_state_dict(small.state_dict())


# --------------------------------------------------------------------------------------------- mask
def _kernel_mask(H, W, shift):
    """The coordinate rule of tair_k_window_attention (csrc/swinir.hip), restated on the host."""
    out = torch.zeros(H // 8 * (W // 8), 64, 64)
    reg = lambda p, n: 0 if p < n - 8 else 1 if p < n - shift else 2  # noqa: E731
    for wy in range(H // 8):
        for wx in range(W // 8):
            r = [(reg(wy * 8 + t // 8, H), reg(wx * 8 + t % 8, W)) for t in range(64)]
            for a in range(64):
                for b in range(64):
                    if r[a] != r[b]:
                        out[wy * (W // 8) + wx, a, b] = -100.0
    return out


@pytest.mark.parametrize("H,W", [(8, 8), (16, 16), (16, 24), (24, 16), (64, 64)])
def test_coordinate_mask_is_shift_mask(H, W):
    from tair_amd.swinir import shift_mask
    assert torch.equal(_kernel_mask(H, W, 4), shift_mask(H, W, 8, 4))


# -------------------------------------------------------------------------------------------- plans
def _launch_gemms(B, h, w):
    """(name, M, N, K, lda, ldo, keywords) of every distinct GEMM of HipSwinIR._plan."""
    T, fake = B * h * w, 1 << 20
    stream = dict(res=fake, res_lo=192, out_lo=192)
    conv = lambda cin, hh, ww, up=False: (3 if up else 1, cin, B, hh, ww, hh * (2 if up else 1), ww * (2 if up else 1))  # noqa: E731
    out = [("qkv", T, 576, 192, 192, 576, {}), ("proj", T, 192, 192, 192, 384, stream),
           ("proj, first block", T, 192, 192, 192, 384, dict(stream, res_lo=0)),
           ("fc1", T, 384, 192, 192, 384, dict(act=3)), ("fc2", T, 192, 384, 384, 384, stream),
           ("conv_first", T, 192, 9 * 384, 384, 384, dict(conv=conv(384, h, w), out_lo=192)),
           ("group conv", T, 192, 9 * 192, 384, 384, dict(stream, conv=conv(192, h, w))),
           ("group conv, first", T, 192, 9 * 192, 384, 384, dict(stream, res_lo=0, conv=conv(192, h, w))),
           ("conv_after_body", T, 192, 9 * 192, 192, 384, dict(stream, conv=conv(192, h, w))),
           ("conv_before_upsample", T, 64, 9 * 192, 384, 64, dict(conv=conv(192, h, w)))]
    for i in range(3):
        out.append((f"conv_up{i + 1}", T * 4 ** (i + 1), 64, 576, 64, 64, dict(conv=conv(64, h << i, w << i, True))))
    out.append(("conv_hr", 64 * T, 64, 576, 64, 64, dict(conv=conv(64, 8 * h, 8 * w))))
    out.append(("conv_last", 64 * T, 3, 576, 64, 3, dict(conv=conv(64, 8 * h, 8 * w), out_f32=1)))
    return out


@pytest.mark.parametrize("B", [1, 4])
def test_launch_list_gemms_plan(B):
    from tair_amd import _lib
    from tair_amd import swinir_hip as sh
    L = _lib.lib()
    assert L.tair_k_gemm_desc_bytes() == ctypes.sizeof(_lib.GemmDesc)
    fake = 1 << 20
    for name, M, N, K, lda, ldo, kw in _launch_gemms(B, 64, 64):
        assert M == 4096 * B or name.startswith(("conv_up", "conv_hr", "conv_last"))
        d = sh.gemm_desc(L, name, M, N, K, fake, lda, fake, fake, fake, ldo, (fake, 16 << 20), (fake, 1 << 16), **kw)
        plan = [ctypes.c_int() for _ in range(4)]
        assert L.tair_k_gemm_plan(ctypes.byref(d), *[ctypes.byref(v) for v in plan]) == 0, (name, L.tair_last_error())
        if name == "fc1":  # the plan carries the GELU epilogue: a <= 128 x 128 tile
            assert d.act == 3 and 0 < plan[0].value <= 128 and plan[1].value <= 128
    with pytest.raises(_lib.TairError):  # a refused plan is an error, never a skipped launch
        sh.gemm_desc(L, "fc1", 4096, 384, 200, fake, 200, fake, fake, fake, 384, (fake, 16 << 20), (fake, 1 << 16), act=3)


# ---------------------------------------------------------------------------------------- arguments
def test_backend_argument():
    from tair_amd import _lib, config
    from tair_amd.swinir import SwinIR
    assert inspect.signature(config.build_swinir).parameters["backend"].default == "torch"
    tiny = {"model": {"swinir": {"params": dict(img_size=16, embed_dim=24, depths=[1], num_heads=[2], window_size=4,
                                                  mlp_ratio=2, sf=4, upsampler="nearest+conv", unshuffle=True,
                                                  unshuffle_scale=4)}}}
    assert type(config.build_swinir(tiny, "cpu")) is SwinIR and type(config.build_swinir(tiny, "cpu", None, "torch")) is SwinIR
    with pytest.raises(ValueError):  # checked before anything touches a device
        config.build_swinir(None, "cuda:99", backend="triton")
    with pytest.raises(_lib.TairError):  # no CPU fallback
        config.build_swinir(None, "cpu", backend="hip")
    with pytest.raises(ValueError):  # not the val-config network
        config.build_swinir(tiny, "cpu", backend="hip")


@pytest.mark.parametrize("over", [dict(embed_dim=96), dict(window_size=7), dict(upsampler="pixelshuffle"),
                                  dict(num_heads=[6, 3]), dict(mlp_ratio=4), dict(resi_connection="3conv")])
def test_unsupported_configs_are_refused(over):
    from tair_amd import swinir_hip as sh
    from tair_amd.config import SWINIR_VAL_PARAMS
    sh.check_params(dict(SWINIR_VAL_PARAMS))
    sh.check_params(dict(SWINIR_VAL_PARAMS, **REDUCED))
    p = dict(SWINIR_VAL_PARAMS, **REDUCED)
    p.update(over)
    with pytest.raises(ValueError):
        sh.check_params(p)
    with pytest.raises(ValueError):  # before the state dict or a device is looked at
        sh.HipSwinIR({}, p, device="cpu")


def test_input_sizes_are_checked_before_any_launch():
    from tair_amd import swinir_hip as sh
    assert sh.check_input((2, 3, 192, 128), (64, 64)) == (2, 24, 16)
    for shape in [(1, 3, 96, 64), (1, 3, 64, 96), (1, 3, 0, 64), (1, 1, 64, 64), (3, 64, 64)]:
        with pytest.raises(ValueError):
            sh.check_input(shape, (64, 64))
    with pytest.raises(ValueError):  # larger than the workspaces
        sh.check_input((1, 3, 576, 512), (64, 64))


def test_tools_take_the_flag():
    from tair_amd import val, val_patches
    a = val._parse(["--swinir-backend", "hip"])
    assert a.swinir_backend == "hip" and val._parse([]).swinir_backend == "torch"
    with pytest.raises(SystemExit):
        val._parse(["--swinir-backend", "triton"])
    assert "--swinir-backend" in inspect.getsource(val_patches._parse)
    assert "backend=args.swinir_backend" in inspect.getsource(val_patches)


def test_tiled_cleaner_stays_out_of_scope():
    from tair_amd.pipeline import SwinIRPipeline
    pipe = SwinIRPipeline(lambda x: x, None, None, None, "cpu")
    with pytest.raises(NotImplementedError):
        pipe.apply_cleaner(torch.zeros(1, 3, 64, 64), True, 512, 256)


# ---------------------------------------------------------------------------------------- emulation
@pytest.fixture(scope="module")
def emu_case():
    from oracle.swinir_ref import swinir_forward_ref
    m, p = _stock()
    x = torch.rand((1, 3, 128, 128), generator=torch.Generator().manual_seed(1))
    return m.state_dict(), p, x, swinir_forward_ref(m.state_dict(), p, x)


def test_emulation_is_close_to_the_oracle(emu_case):
    """The bf16 operands alone cost a few 1e-3 of the image (DESIGN.md §2.9 quotes the value); an emulation that were
    the oracle itself (no rounding) or far from it would make the GPU gate meaningless."""
    sd, p, x, ref = emu_case
    e = rel(emulate(sd, p["depths"], x), ref)
    print(f"emulation vs oracle, reduced config, 128^2: rel-L2 {e:.3e}")
    assert 2.0 ** -12 < e < 2.0 ** -6, e  # between a tenth of and ten times one bf16 rounding (2^-9)


def test_gate_has_teeth(emu_case):
    """The network gate (HIP <= 1.5 x emulation) can fail: the same emulation with the attention scale of the padded
    head dim, 32^-1/2 instead of 30^-1/2, is at least twice as far from the oracle."""
    sd, p, x, ref = emu_case
    e = rel(emulate(sd, p["depths"], x), ref)
    e32 = rel(emulate(sd, p["depths"], x, scale=32 ** -0.5), ref)
    print(f"emulation {e:.3e}, with scale 32^-1/2 {e32:.3e}, ratio {e32 / e:.2f}")
    assert e32 >= 2.0 * e, (e32, e)
