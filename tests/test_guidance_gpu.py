"""Classifier-free guidance inside the fused sampler step graph (spaced_sampler.py:149-167, sampler.py:31-38).

A guided step is ONE forward at batch 2B (rows [0,B) cond, [B,2B) uncond) followed by the fused update
kernel, which forms v = v_u + s_i (v_c - v_u) with the step's scale from a device table before p_sample.

* kernel (`tair_k_sampler_step`, tiny shapes): x against the same formula in fp64, gate = 4 x the error fp32
  torch (`oracle.sampler_ref.p_sample_v`) shows against fp64 on the same inputs (floor 2^-23; both measured
  here as max |error| / max |fp64|; the margin covers FMA contraction and the order of the guidance sum);
  the (hi, lo, hi) bf16 planes bitwise from the kernel's own x, in both halves, pad channels untouched;
  guided with s = 1, v_u = v_c bitwise the unguided update.
* model, full width (B = 1, max_batch = 2, 3 steps, cfg_scale 4, rescale off / on): rel-L2 to the oracle CFG
  loop <= 4 x FWD_TOL (the project's CFG gate, tests/test_cldm_gpu.py), graph replay vs eager <= 1e-6, decoder
  features = the cond half's.
* model, tiny (B = 3, max_batch = 6, per-tile cond context, broadcast uncond context, an uncond c_img of its
  own, 4 steps): the same gates; the host-loop fallback when 2B > max_batch; no state leaks between guided
  and unguided runs, or between two guidance scales, on one handle.
* stage 3 (`val_sample`, stub spotter / encoder): guided val_sample == guided sample when the prompt never
  changes, != unguided; with a changing prompt the negative half keeps its context.

Measured on MI355X: full width 5.7e-3 / 2.0e-3 (rescale off / on), tiny B = 3 4.5e-3, stage 3
with a replaced prompt 4.7e-3 against the 2e-2 gate; graph vs eager and the state-hygiene reruns equal; kernel x
error at or below fp32 torch's (<= 1.6e-7).
"""
import ctypes
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

FWD_TOL = 5e-3          # the project's one-forward gate (tests/test_cldm_gpu.py)
CFG_TOL = 4 * FWD_TOL   # its CFG gate: s = 4 scales the two forwards' errors by up to ~s
FEAT_TOL = 2e-2         # its decoder-feature gate (test_forward_parity_batch2)
REPLAY_TOL = 1e-6       # graph replay vs eager (fp64 statistics atomics: last-bit noise only)


TINY = dict(model_channels=64, channel_mult=[1, 2], num_res_blocks=1, attention_resolutions=[1, 2],
            num_head_channels=64, context_dim=64, in_channels=4, out_channels=4)


def rel_l2(a, b):
    a, b = a.double(), b.double()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def _record(name, **vals):
    """One line of measured errors in the suite's parity log (the file tests/test_cldm_gpu.py writes)."""
    from tests.test_cldm_gpu import _record as record
    record(name, **vals)


def _sampler(rescale=False):
    from tair_amd.diffusion import Diffusion
    from tair_amd.sampler import SpacedSampler
    return SpacedSampler(Diffusion(linear_start=0.00085, linear_end=0.012, zero_snr=True,
                                   parameterization="v").betas, "v", rescale)


# ---------------------------------------------------------------------------------------------- kernel
LD, LDC = 64, 8  # the library's conv_in row (64 channels) and the ControlNet plane stride (4 latent + 4 hint)
SENTINEL = 7.0


def _err(a, ref64):
    return ((a.double() - ref64).abs().max() / ref64.abs().max()).item()


def _planes_of(x):
    hi = x.to(torch.bfloat16)
    lo = (x - hi.float()).to(torch.bfloat16)
    return hi, lo


def _k_step(L, x, v, v_u, tabs, scales, counter, noise, in_u, in_c, half_rows):
    from tair_amd import _lib
    from tair_amd.cldm import _stream_ptr
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())  # noqa: E731
    rows, C = x.shape
    _lib.check(L.tair_k_sampler_step(p(x), p(v), p(v_u), p(tabs), p(scales), p(counter), p(noise), rows, C, p(in_u),
                                     p(in_c), LD, LDC, half_rows, _stream_ptr(x.device)), "k_sampler_step")


def _kernel_inputs(rows, n_steps=3, seed=5):
    from oracle.sampler_ref import SpacedScheduleRef, diffusion_betas
    sched = SpacedScheduleRef(diffusion_betas(), n_steps)
    names = ["sqrt_alphas_cumprod", "sqrt_one_minus_alphas_cumprod", "posterior_mean_coef1", "posterior_mean_coef2",
             "posterior_variance"]
    tabs = torch.stack([sched.tables[k] for k in names]).contiguous().cuda()
    g = torch.Generator().manual_seed(seed + rows)
    x = torch.randn(rows, 4, generator=g).cuda()
    vc = torch.randn(n_steps, rows, 4, generator=g).cuda()
    vu = torch.randn(n_steps, rows, 4, generator=g).cuda()
    noise = torch.randn(n_steps, rows, 4, generator=g).cuda()
    return sched, tabs, x, vc, vu, noise


def _check_planes(buf, x, rows, halves, plane, what):
    """buf [halves * rows, LD] bf16: channels plane*k + c (k = 0, 1, 2) of every row hold (hi, lo, hi) of the
    kernel's own x, bit for bit, in every half; all other channels keep the sentinel."""
    hi, lo = _planes_of(x)
    want = torch.full((rows, LD), SENTINEL, dtype=torch.bfloat16, device=x.device)
    want[:, 0:4], want[:, plane:plane + 4], want[:, 2 * plane:2 * plane + 4] = hi, lo, hi
    for h in range(halves):
        got = buf[h * rows:(h + 1) * rows]
        assert torch.equal(got.view(torch.int16), want.view(torch.int16)), (what, h)
    assert torch.all(buf[halves * rows:] == SENTINEL), what  # rows past the written halves


@pytest.mark.parametrize("with_c", [False, True])
@pytest.mark.parametrize("mode", ["unguided", "guided"])
@pytest.mark.parametrize("rows", [37, 515])
@torch.no_grad()
def test_kernel_step_vs_fp64(rows, mode, with_c):
    from oracle.sampler_ref import p_sample_v
    from tair_amd import _lib
    L = _lib.lib()
    n_steps = 3
    sched, tabs, x, vc, vu, noise = _kernel_inputs(rows, n_steps)
    guided = mode == "guided"
    scales = torch.tensor([4.0, 2.5, 0.75], dtype=torch.float32).cuda()
    in_u = torch.full((2 * rows + 3, LD), SENTINEL, dtype=torch.bfloat16).cuda()
    in_c = torch.full((2 * rows + 3, LD), SENTINEL, dtype=torch.bfloat16).cuda() if with_c else None
    for i in range(n_steps):  # every counter value, the last is t = 0 (no noise)
        t = n_steps - 1 - i
        x_in = x.clone()
        v = vc[i].clone()
        counter = torch.tensor([i, n_steps], dtype=torch.int32).cuda()
        _k_step(L, x, v, vu[i] if guided else None, tabs, scales if guided else None, counter, noise, in_u, in_c,
                rows if guided else 0)
        # fp64: the same formula on the same fp32 inputs and fp32 tables
        T = [tabs[k, t].double() for k in range(5)]
        v64 = vu[i].double() + scales[i].double() * (vc[i].double() - vu[i].double()) if guided else vc[i].double()
        x0 = T[0] * x_in.double() - T[1] * v64
        want = T[2] * x0 + T[3] * x_in.double() + (torch.sqrt(T[4]) * noise[i].double() if t != 0 else 0.0)
        # fp32 torch on the same inputs: the yardstick of the gate
        v32 = vu[i] + scales[i] * (vc[i] - vu[i]) if guided else vc[i]
        x32 = p_sample_v(sched, x_in, v32, t, noise[i])
        e_torch, e_hip = _err(x32, want), _err(x, want)
        gate = max(4 * e_torch, 2.0 ** -23)
        print(f"k_sampler_step rows={rows} {mode} in_c={with_c} i={i}: hip {e_hip:.3e} torch {e_torch:.3e} gate {gate:.3e}")
        assert e_hip <= gate, (i, e_hip, e_torch)
        if t == 0:  # no noise at the last step: x is the posterior mean
            assert _err(x, T[2] * x0 + T[3] * x_in.double()) <= gate
        ev_t, ev = _err(v32, v64), _err(v, v64)  # the stored v is what p_sample consumed
        assert ev <= max(4 * ev_t, 2.0 ** -23), (i, ev, ev_t)
        if not guided:
            assert torch.equal(v, vc[i])
        halves = 2 if guided else 1
        _check_planes(in_u, x, rows, halves, 4, ("in_u", i))
        if with_c:
            _check_planes(in_c, x, rows, halves, LDC, ("in_c", i))


@pytest.mark.parametrize("rows", [37, 515])
@torch.no_grad()
def test_kernel_guided_scale_one_is_bitwise_unguided(rows):
    """v = v_u + s (v_c - v_u) with s = 1 and v_u = v_c is v_c exactly, so the guided kernel must reproduce
    the unguided one bit for bit: x, the stored v and the planes of the cond half."""
    from tair_amd import _lib
    L = _lib.lib()
    n_steps = 3
    _, tabs, x0, vc, _, noise = _kernel_inputs(rows, n_steps, seed=9)
    ones = torch.ones(n_steps, dtype=torch.float32).cuda()
    xa, xb = x0.clone(), x0.clone()
    ua, ub = (torch.full((2 * rows, LD), SENTINEL, dtype=torch.bfloat16).cuda() for _ in range(2))
    ca, cb = (torch.full((2 * rows, LD), SENTINEL, dtype=torch.bfloat16).cuda() for _ in range(2))
    for i in range(n_steps):
        counter = torch.tensor([i, n_steps], dtype=torch.int32).cuda()
        va, vb = vc[i].clone(), vc[i].clone()
        _k_step(L, xa, va, None, tabs, None, counter, noise, ua, ca, 0)
        _k_step(L, xb, vb, vc[i].clone(), tabs, ones, counter, noise, ub, cb, rows)
        assert torch.equal(xa.view(torch.int32), xb.view(torch.int32)), i
        assert torch.equal(va.view(torch.int32), vb.view(torch.int32)), i
        assert torch.equal(ua[:rows].view(torch.int16), ub[:rows].view(torch.int16)), i
        assert torch.equal(ca[:rows].view(torch.int16), cb[:rows].view(torch.int16)), i
        assert torch.equal(ub[rows:].view(torch.int16), ub[:rows].view(torch.int16)), i  # both halves alike


# ---------------------------------------------------------------------------------- model, full width
@pytest.fixture(scope="module")
def models():
    from oracle.ldm_ref import ControlLDMRef
    from tair_amd.cldm import ControlLDM
    from tair_amd.weights import manifest, perturb_norms, synthetic_state_dict
    torch.backends.cuda.matmul.allow_tf32 = False
    torch.backends.cudnn.allow_tf32 = False
    sd = perturb_norms(synthetic_state_dict(manifest(), seed=0))
    m = ControlLDM(max_batch=2, with_vae=False)
    m.load_state_dict(sd)
    ref = ControlLDMRef().cuda().eval()
    ref.load_state_dict(sd, strict=True)
    del sd
    yield m, ref
    m.close()


def _full_inputs(steps=3):
    g = torch.Generator().manual_seed(71)
    x = torch.randn(1, 4, 64, 64, generator=g).cuda()
    c_img = torch.randn(1, 4, 64, 64, generator=g).cuda()
    c_txt = torch.randn(1, 77, 1024, generator=g).cuda()
    c_neg = torch.randn(1, 77, 1024, generator=g).cuda()
    noise = torch.randn(steps, 1, 4, 64, 64, generator=g).cuda()
    return x, {"c_txt": c_txt, "c_img": c_img}, {"c_txt": c_neg, "c_img": c_img}, noise


@pytest.mark.parametrize("rescale", [False, True])
@torch.no_grad()
def test_full_width_guided_fused_vs_oracle(models, rescale):
    from oracle.sampler_ref import SpacedScheduleRef, diffusion_betas, sample_cfg_ref
    m, ref = models
    steps = 3
    x, cond, uncond, noise = _full_inputs(steps)
    s = _sampler(rescale)
    z, feats = s.sample(m, "cuda", steps, x.shape, cond, uncond=uncond, cfg_scale=4.0, x_T=x, noise=noise)
    assert s.last_guided_fused is True
    assert feats == []
    ze, _ = s.sample(m, "cuda", steps, x.shape, cond, uncond=uncond, cfg_scale=4.0, x_T=x, noise=noise, use_graph=False)
    assert s.last_guided_fused is True
    zr = sample_cfg_ref(ref, SpacedScheduleRef(diffusion_betas(), steps), x, cond, uncond, 4.0, noise, rescale)
    e, er = rel_l2(z, zr), rel_l2(z, ze)
    print(f"guided fused full width rescale={rescale}: rel-L2 to oracle {e:.3e}, graph vs eager {er:.3e}")
    _record(f"guided_fused_full_rescale{int(rescale)}", rel_l2_z=e, graph_vs_eager=er)
    assert e <= CFG_TOL, e
    assert er <= REPLAY_TOL, er


@torch.no_grad()
def test_full_width_guided_features_are_the_cond_half(models):
    m, ref = models
    steps = 3
    x, cond, uncond, noise = _full_inputs(steps)
    s = _sampler()
    cfg = types.SimpleNamespace(exp_args={"unet_feat_sampling_timestep": [1]})
    _, sampled = s.sample(m, "cuda", steps, x.shape, cond, uncond=uncond, cfg_scale=4.0, x_T=x, noise=noise, cfg=cfg)
    assert s.last_guided_fused is True
    assert len(sampled) == 1 and sampled[0][0] == 1
    _, model_t, feats = sampled[0]
    assert model_t == int(np.flip(s.timesteps)[0])
    t = torch.full((1,), model_t, dtype=torch.long, device="cuda")
    fc, fu = ref(x, t, cond)[1], ref(x, t, uncond)[1]
    assert len(feats) == 4 and [tuple(f.shape) for f in feats] == [tuple(f.shape) for f in fc]
    assert all(f.shape[0] == 1 for f in feats)
    ec = [rel_l2(a, b) for a, b in zip(feats, fc)]
    eu = [rel_l2(a, b) for a, b in zip(feats, fu)]
    print(f"guided features: to cond oracle {ec}, to uncond oracle {eu}")
    _record("guided_fused_full_feats", rel_l2_feats_cond=ec, rel_l2_feats_uncond=eu)
    assert max(ec) < FEAT_TOL, ec
    assert min(eu) > 1e-3, eu


# ----------------------------------------------------------------------------------------- model, tiny
def _make_tiny(max_batch, sd=None):
    from tair_amd.cldm import ControlLDM
    from tair_amd.weights import perturb_norms, synthetic_state_dict
    m = ControlLDM(TINY, max_batch=max_batch, latent_hw=(16, 16), with_vae=False, device=torch.device("cuda", 0))
    if sd is None:
        sd = perturb_norms(synthetic_state_dict(m.param_manifest(), seed=7))
    m.load_state_dict(sd)
    return m, sd


@pytest.fixture(scope="module")
def tiny():
    from oracle.ldm_ref import CLDMConfig, ControlLDMRef
    torch.backends.cuda.matmul.allow_tf32 = False
    torch.backends.cudnn.allow_tf32 = False
    m, sd = _make_tiny(6)
    ref = ControlLDMRef(CLDMConfig(model_channels=64, channel_mult=(1, 2), num_res_blocks=1,
                                   attention_resolutions=(1, 2), head_channels=64, context_dim=64)).cuda().eval()
    ref.load_state_dict(sd, strict=True)
    B, steps = 3, 4
    g = torch.Generator().manual_seed(81)
    x = torch.randn(B, 4, 16, 16, generator=g).cuda()
    cond = {"c_txt": torch.randn(B, 77, 64, generator=g).cuda(), "c_img": torch.randn(B, 4, 16, 16, generator=g).cuda()}
    uncond = {"c_txt": torch.randn(1, 77, 64, generator=g).cuda(), "c_img": torch.randn(B, 4, 16, 16, generator=g).cuda()}
    noise = torch.randn(steps, B, 4, 16, 16, generator=g).cuda()
    env = types.SimpleNamespace(m=m, sd=sd, ref=ref, B=B, steps=steps, x=x, cond=cond, uncond=uncond, noise=noise,
                                oracle={})
    yield env
    m.close()


def _tiny_oracle(env, cfg_scale=4.0):
    """The tiny oracle CFG loop, computed once per scale and shared."""
    from oracle.sampler_ref import SpacedScheduleRef, diffusion_betas, sample_cfg_ref
    if cfg_scale not in env.oracle:
        unc = dict(env.uncond, c_txt=env.uncond["c_txt"].expand(env.B, -1, -1))
        env.oracle[cfg_scale] = sample_cfg_ref(env.ref, SpacedScheduleRef(diffusion_betas(), env.steps), env.x, env.cond,
                                               unc, cfg_scale, env.noise, False)
    return env.oracle[cfg_scale]


def _tiny_sample(s, m, env, cfg_scale=None, **kw):
    g = {} if cfg_scale is None else dict(uncond=env.uncond, cfg_scale=cfg_scale)
    return s.sample(m, "cuda", env.steps, env.x.shape, env.cond, x_T=env.x, noise=env.noise, **g, **kw)[0]


@torch.no_grad()
def test_tiny_guided_fused_vs_oracle(tiny):
    s = _sampler()
    z = _tiny_sample(s, tiny.m, tiny, 4.0)
    assert s.last_guided_fused is True
    ze = _tiny_sample(s, tiny.m, tiny, 4.0, use_graph=False)
    e, er = rel_l2(z, _tiny_oracle(tiny)), rel_l2(z, ze)
    print(f"guided fused tiny B=3: rel-L2 to oracle {e:.3e}, graph vs eager {er:.3e}")
    _record("guided_fused_tiny_b3", rel_l2_z=e, graph_vs_eager=er)
    assert e <= CFG_TOL, e
    assert er <= REPLAY_TOL, er


@torch.no_grad()
def test_tiny_fallback_when_two_b_exceeds_max_batch(tiny):
    m4, _ = _make_tiny(4, tiny.sd)
    try:
        s = _sampler()
        z = _tiny_sample(s, m4, tiny, 4.0)
        assert s.last_guided_fused is False
        e = rel_l2(z, _tiny_oracle(tiny))
        _record("guided_host_fallback_tiny_b3", rel_l2_z=e)
        assert e <= CFG_TOL, e
        _tiny_sample(s, m4, tiny)
        assert s.last_guided_fused is None
    finally:
        m4.close()


@torch.no_grad()
def test_tiny_state_hygiene_on_one_handle(tiny):
    """unguided -> guided (4.0) -> guided (2.0) -> unguided on one handle: each equals the same call on a
    fresh handle (no graph of the other kind replayed, no scale baked into a captured graph)."""
    s = _sampler()
    calls = [None, 4.0, 2.0, None]
    got = [_tiny_sample(s, tiny.m, tiny, c) for c in calls]
    for k, c in enumerate(calls):
        fresh, _ = _make_tiny(6, tiny.sd)
        try:
            want = _tiny_sample(_sampler(), fresh, tiny, c)
        finally:
            fresh.close()
        e = rel_l2(got[k], want)
        print(f"state hygiene call {k} (cfg_scale {c}): rel-L2 to a fresh handle {e:.3e}")
        assert e <= REPLAY_TOL, (k, c, e)
    assert rel_l2(got[1], got[2]) > 1e-3
    assert rel_l2(got[1], got[0]) > 1e-3


# --------------------------------------------------------------------------------------------- stage 3
class _NoWords:
    """Stub spotter: finds nothing (empty polygons / recs per tile), so the prompt is the encoder's call."""

    def __call__(self, feats, targets, mode):
        B, dev = feats[0].shape[0], feats[0].device
        tile = types.SimpleNamespace(polygons=torch.zeros(0, 32, device=dev), recs=torch.zeros(0, 25, dtype=torch.long, device=dev))
        return None, [tile] * B


@pytest.fixture(scope="module")
def stage3():
    from oracle.ldm_ref import CLDMConfig, ControlLDMRef
    torch.backends.cuda.matmul.allow_tf32 = False
    torch.backends.cudnn.allow_tf32 = False
    m, sd = _make_tiny(2)
    ref = ControlLDMRef(CLDMConfig(model_channels=64, channel_mult=(1, 2), num_res_blocks=1,
                                   attention_resolutions=(1, 2), head_channels=64, context_dim=64)).cuda().eval()
    ref.load_state_dict(sd, strict=True)
    steps = 4
    g = torch.Generator().manual_seed(91)
    x = torch.randn(1, 4, 16, 16, generator=g).cuda()
    c_img = torch.randn(1, 4, 16, 16, generator=g).cuda()
    c0, c_alt, c_neg = (torch.randn(1, 77, 64, generator=g).cuda() for _ in range(3))
    noise = torch.randn(steps, 1, 4, 16, 16, generator=g).cuda()
    yield types.SimpleNamespace(m=m, ref=ref, steps=steps, x=x, c_img=c_img, c0=c0, c_alt=c_alt, c_neg=c_neg, noise=noise)
    m.close()


def _val(s, e, enc, guided):
    g = dict(uncond={"c_txt": e.c_neg, "c_img": e.c_img}, cfg_scale=4.0) if guided else {}
    z, res = s.val_sample(e.m, "cuda", e.steps, e.x.shape, {"c_txt": e.c0, "c_img": e.c_img}, x_T=e.x, noise=e.noise,
                          ts_model=_NoWords(), text_encoder=enc, **g)
    assert len(res) == e.steps
    return z


@torch.no_grad()
def test_stage3_guided_val_sample_same_context(stage3):
    e = stage3
    s = _sampler()
    enc = lambda prompt: e.c0.clone()  # noqa: E731
    zg = _val(s, e, enc, True)
    zs, _ = s.sample(e.m, "cuda", e.steps, e.x.shape, {"c_txt": e.c0, "c_img": e.c_img},
                     uncond={"c_txt": e.c_neg, "c_img": e.c_img}, cfg_scale=4.0, x_T=e.x, noise=e.noise)
    assert s.last_guided_fused is True
    zu = _val(s, e, enc, False)
    d_same, d_unguided = rel_l2(zg, zs), rel_l2(zg, zu)
    print(f"stage 3 guided val_sample: to guided sample {d_same:.3e}, to unguided val_sample {d_unguided:.3e}")
    assert d_same <= REPLAY_TOL, d_same
    assert d_unguided > 1e-3, d_unguided


@torch.no_grad()
def test_stage3_guided_val_sample_keeps_the_negative_context(stage3):
    """The encoder returns another context from step 1 on: set_context must replace the cond half only."""
    from oracle.sampler_ref import SpacedScheduleRef, cfg_scale_ref, diffusion_betas, p_sample_v
    e = stage3
    z = _val(_sampler(), e, lambda prompt: e.c_alt.clone(), True)
    sched = SpacedScheduleRef(diffusion_betas(), e.steps)
    ts = np.flip(sched.timesteps)
    x = e.x
    for i in range(e.steps):
        mt = torch.full((1,), int(ts[i]), dtype=torch.long, device="cuda")
        vc, _ = e.ref(x, mt, {"c_txt": e.c0 if i == 0 else e.c_alt, "c_img": e.c_img})
        vu, _ = e.ref(x, mt, {"c_txt": e.c_neg, "c_img": e.c_img})
        sc = cfg_scale_ref(4.0, int(ts[i]), False)
        x = p_sample_v(sched, x, vu + sc * (vc - vu), e.steps - i - 1, e.noise[i])
    err = rel_l2(z, x)
    print(f"stage 3 guided val_sample, alternate context: rel-L2 to the oracle loop {err:.3e}")
    _record("guided_val_sample_alt_context", rel_l2_z=err)
    assert err <= CFG_TOL, err


@torch.no_grad()
def test_val_sample_guided_without_room_raises(tiny):
    """val_sample never runs unguided when guidance was asked for: 2B > max_batch is an error."""
    m4, _ = _make_tiny(4, tiny.sd)
    try:
        with pytest.raises(ValueError, match="max_batch"):
            _sampler().val_sample(m4, "cuda", tiny.steps, tiny.x.shape, dict(tiny.cond), uncond=tiny.uncond,
                                  cfg_scale=4.0, x_T=tiny.x, noise=tiny.noise, ts_model=_NoWords(),
                                  text_encoder=lambda p: tiny.cond["c_txt"])
    finally:
        m4.close()
