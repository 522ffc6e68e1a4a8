"""Latent tiling inside the fused sampler (utils/common.py:125-234 make_tiled_fn wired as in
ddim_sampler.py:165-180): a whole latent larger than the handle's tile runs, per step, the network on its
overlapping windows in equal chunks, a Gaussian blend of the window outputs and p_sample on the whole latent.

* kernels (`tair_k_tile_gather`, `tair_k_tile_blend_step`; B = 2, whole latent 24 x 36, tile 16, stride 8: 8
  windows per image with an appended last column, N = 16 rows): the gathered (hi, lo, hi) planes bit for bit from
  the torch slice for the chunks (0,16), (6,6), (12,6) (2 pad rows = window 15), hints likewise, the guided second
  half with the uncond hint, sentinels elsewhere; blend / step against the same formula in fp64 on the same fp32
  inputs, gate = 4 x the error of the fp32 torch restatement (floor 2^-23, both max|err| / max|fp64|: the gate of
  tests/test_guidance_gpu.py), NaN in the pad rows' v harmless; 1 chunk of 16 and 3 chunks of 6 bitwise equal.
* model, tiny (4 steps): unguided in 1 chunk (max_batch 16) and 3 chunks (max_batch 6) against the fp32 reference
  loop tests/_tiled_ref.py <= FWD_TOL, graph vs eager <= REPLAY_TOL; guided (cfg_scale 4, uncond with its own
  c_img, 6 chunks of 3) <= CFG_TOL; one window = the untiled step within REPLAY_TOL + 2^-22 (the forward is the
  same computation up to the statistics atomics and fl(fl(w v) / w) adds at most 2^-23 relative); state hygiene
  across untiled / tiled / another tiled geometry / untiled on one handle; the argument rules raise ValueError.
* full width (max_batch 2, whole latent 64 x 96, stride 32, 3 steps) against ControlLDMRef <= FWD_TOL.
* pipeline (full width with the VAE, 512 x 768 condition image, 4 steps): apply_cldm(cldm_tiled=True) against
  encode -> reference loop -> decode with oracle.vae_ref on the same draws, image rel-L2 <= 6e-3
  (tests/test_pipeline_gpu.py's gate for 4 unguided steps); a 512 x 512 input tiled == untiled.

Measured errors are recorded through tests.test_cldm_gpu._record and quoted in DESIGN.md §4.2.  On MI355X: tiny
1 / 3 chunks 1.7e-3 / 1.7e-3, guided 4.6e-3, full width 2.0e-3, pipeline image 3.0e-3, graph vs eager, state hygiene
and both one-window comparisons equal; blend / step errors <= 1.2 x fp32 torch's (<= 1.7e-7).

On the one-window gates: with the reference's arithmetic alone (v = fl(fl(w v) / w) where a single window covers a
pixel) the 512 x 512 pipeline comparison measured 2.2e-3, not <= 1.2e-6: the step-0 v agreed to 2.4e-8, but the
one-ulp difference it leaves in x moves the next step's v by 1.1e-3.  That is the bf16 network's sensitivity, not
the tiling: perturbing x_T of an untiled full-width run by one fp32 ulp moved step-0 v by 1.2e-3 and the 4-step
latent by 1.4e-3.  The blend kernel therefore passes a single-covered pixel's v through unchanged,
which is what these gates now measure.
"""
import ctypes
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

FWD_TOL = 5e-3          # the project's gate for multi-step unguided runs (tests/test_cldm_gpu.py)
CFG_TOL = 4 * FWD_TOL   # its CFG gate
REPLAY_TOL = 1e-6       # graph replay vs eager
ONE_WINDOW_TOL = REPLAY_TOL + 2.0 ** -22

TINY = dict(model_channels=64, channel_mult=[1, 2], num_res_blocks=1, attention_resolutions=[1, 2],
            num_head_channels=64, context_dim=64, in_channels=4, out_channels=4)
B, H, W, S, STRIDE = 2, 24, 36, 16, 8
T, N = 8, 16
LD, LDC, C, HC = 64, 8, 4, 4
SENTINEL = 7.0


def rel_l2(a, b):
    a, b = a.double(), b.double()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def _record(name, **vals):
    from tests.test_cldm_gpu import _record as record
    record(name, **vals)


def _sampler():
    from tair_amd.diffusion import Diffusion
    from tair_amd.sampler import SpacedSampler
    return SpacedSampler(Diffusion(linear_start=0.00085, linear_end=0.012, zero_snr=True,
                                   parameterization="v").betas, "v", False)


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _jobs():
    from tests._tiled_ref import windows_ref
    return [(b, win) for b in range(B) for win in windows_ref(H, W, S, STRIDE)]


def _nhwc(x):
    """[B, C, H, W] -> the library's whole-latent layout [B*H*W, C]."""
    return x.permute(0, 2, 3, 1).reshape(-1, x.shape[1]).contiguous()


# ---------------------------------------------------------------------------------------------- gather
def _planes(x):
    hi = x.to(torch.bfloat16)
    return hi, (x - hi.float()).to(torch.bfloat16)


def _window_rows(x, job):
    """[S*S, ch] rows of one job's window of x [B, ch, H, W]."""
    b, (y0, y1, x0, x1) = job
    return x[b, :, y0:y1, x0:x1].permute(1, 2, 0).reshape(S * S, -1)


@pytest.mark.parametrize("guided", [False, True])
@pytest.mark.parametrize("chunk,rpc,nch", [(0, 16, 1), (1, 6, 3), (2, 6, 3)])
@torch.no_grad()
def test_gather_planes_bitwise(chunk, rpc, nch, guided):
    from tair_amd import _lib
    from tair_amd.cldm import _stream_ptr
    L = _lib.lib()
    g = torch.Generator().manual_seed(11)
    x = torch.randn(B, C, H, W, generator=g).cuda()
    hint = torch.randn(B, HC, H, W, generator=g).cuda()
    hint_u = torch.randn(B, HC, H, W, generator=g).cuda()
    halves = 2 if guided else 1
    prow = rpc * S * S
    rows_total = halves * prow + 5
    in_u = torch.full((rows_total, LD), SENTINEL, dtype=torch.bfloat16).cuda()
    in_c = torch.full((rows_total, LD), SENTINEL, dtype=torch.bfloat16).cuda()
    cdev = torch.tensor([chunk], dtype=torch.int32).cuda()
    xs, hs, hus = _nhwc(x), _nhwc(hint), _nhwc(hint_u)
    _lib.check(L.tair_k_tile_gather(_p(xs), _p(hs), _p(hus) if guided else None, _p(cdev), B, H, W, S, STRIDE, rpc, nch,
                                    C, HC, _p(in_u), _p(in_c), LD, LDC, prow if guided else 0, _stream_ptr(x.device)),
               "k_tile_gather")
    jobs = _jobs()
    want_u = torch.full((rows_total, LD), SENTINEL, dtype=torch.bfloat16).cuda()
    want_c = torch.full((rows_total, LD), SENTINEL, dtype=torch.bfloat16).cuda()
    for half in range(halves):
        for r in range(rpc):
            j = min(chunk * rpc + r, N - 1)  # pad rows hold window 15
            hi, lo = _planes(_window_rows(x, jobs[j]))
            hh, hl = _planes(_window_rows(hint_u if half else hint, jobs[j]))
            sl = slice(half * prow + r * S * S, half * prow + (r + 1) * S * S)
            for k, pl in enumerate((hi, lo, hi)):
                want_u[sl, k * C:k * C + C] = pl
                want_c[sl, k * LDC:k * LDC + C] = pl
            for k, pl in enumerate((hh, hl, hh)):
                want_c[sl, k * LDC + C:k * LDC + C + HC] = pl
    assert torch.equal(in_u.view(torch.int16), want_u.view(torch.int16))
    assert torch.equal(in_c.view(torch.int16), want_c.view(torch.int16))
    if chunk == 2:  # the last two rows are pad: window 15 again
        last = slice((rpc - 1) * S * S, rpc * S * S)
        prev = slice((rpc - 3) * S * S, (rpc - 2) * S * S)
        assert torch.equal(in_u[last].view(torch.int16), in_u[prev].view(torch.int16))


@torch.no_grad()
def test_gather_out_of_range_chunk_writes_nothing():
    from tair_amd import _lib
    from tair_amd.cldm import _stream_ptr
    L = _lib.lib()
    x = torch.randn(B * H * W, C).cuda()
    in_u = torch.full((6 * S * S, LD), SENTINEL, dtype=torch.bfloat16).cuda()
    for c in (-1, 3):
        cdev = torch.tensor([c], dtype=torch.int32).cuda()
        _lib.check(L.tair_k_tile_gather(_p(x), None, None, _p(cdev), B, H, W, S, STRIDE, 6, 3, C, HC, _p(in_u), None,
                                        LD, LDC, 0, _stream_ptr(x.device)), "k_tile_gather")
    assert torch.all(in_u == SENTINEL)


# ------------------------------------------------------------------------------------------ blend/step
def _blend_inputs(n_steps=3, seed=23):
    from oracle.sampler_ref import SpacedScheduleRef, diffusion_betas
    from tests._tiled_ref import weights_ref
    sched = SpacedScheduleRef(diffusion_betas(), n_steps)
    names = ["sqrt_alphas_cumprod", "sqrt_one_minus_alphas_cumprod", "posterior_mean_coef1", "posterior_mean_coef2",
             "posterior_variance"]
    tabs = torch.stack([sched.tables[k] for k in names]).contiguous().cuda()
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, C, H, W, generator=g).cuda()
    vc = torch.randn(n_steps, N, C, S, S, generator=g).cuda()   # per step, per job row: the window's output
    vu = torch.randn(n_steps, N, C, S, S, generator=g).cuda()
    noise = torch.randn(n_steps, B, C, H, W, generator=g).cuda()
    w = torch.from_numpy(weights_ref(S)).float().cuda()
    return sched, tabs, x, vc, vu, noise, w


def _rows(v):
    """[n, C, S, S] window outputs -> the forward's output layout [n * S * S, C]."""
    return v.permute(0, 2, 3, 1).reshape(-1, v.shape[1])


def _run_blend(L, x, vc_i, vu_i, tabs, scales, i, n_steps, noise, w, rpc, nch, nan_pad=True):
    """One tiled step through the hook on chunks of rpc rows: returns (x', v_blend) as [B, C, H, W]."""
    from tair_amd import _lib
    from tair_amd.cldm import _stream_ptr
    guided = vu_i is not None
    n = B * H * W
    xs = _nhwc(x).clone()
    acc, acc_u, cnt = (torch.zeros(n, C).cuda() for _ in range(3))
    v_blend = torch.full((n, C), SENTINEL).cuda()
    counter = torch.tensor([i, n_steps], dtype=torch.int32).cuda()
    cdev = torch.zeros(1, dtype=torch.int32).cuda()
    nz = _nhwc(noise.reshape(-1, C, H, W)).reshape(n_steps, n, C).contiguous()
    pad_val = float("nan") if nan_pad else 0.0
    for c in range(nch):
        j0, j1 = c * rpc, min((c + 1) * rpc, N)
        v = torch.full((2 * rpc * S * S, C), pad_val).cuda()
        v[:(j1 - j0) * S * S] = _rows(vc_i[j0:j1])
        if guided:
            v[rpc * S * S:(rpc + j1 - j0) * S * S] = _rows(vu_i[j0:j1])
        assert cdev.item() == c and counter[0].item() == i
        _lib.check(L.tair_k_tile_blend_step(_p(xs), _p(v), _p(v_blend), _p(acc), _p(acc_u) if guided else None, _p(cnt),
                                            _p(w), _p(tabs), _p(scales) if guided else None, _p(counter), _p(cdev),
                                            _p(nz), B, H, W, S, STRIDE, rpc, nch, C, _stream_ptr(x.device)),
                   "k_tile_blend_step")
    assert cdev.item() == 0 and counter[0].item() == i + 1      # the step advanced, the chunk index is back at 0
    assert not acc.any() and not cnt.any() and not acc_u.any()  # cleared for the next step
    back = lambda t: t.reshape(B, H, W, C).permute(0, 3, 1, 2).contiguous()  # noqa: E731
    return back(xs), back(v_blend)


def _err(a, ref64):
    return ((a.double() - ref64).abs().max() / ref64.abs().max()).item()


@pytest.mark.parametrize("mode", ["unguided", "guided"])
@torch.no_grad()
def test_blend_step_vs_fp64(mode):
    from oracle.sampler_ref import p_sample_v
    from tair_amd import _lib
    from tests._tiled_ref import blend_ref, windows_ref
    L = _lib.lib()
    n_steps = 3
    sched, tabs, x, vc, vu, noise, w = _blend_inputs(n_steps)
    guided = mode == "guided"
    scales = torch.tensor([4.0, 2.5, 0.75], dtype=torch.float32).cuda()
    wins = windows_ref(H, W, S, STRIDE)
    per_win = lambda v: [v.reshape(B, T, C, S, S)[:, k] for k in range(T)]  # noqa: E731
    for i in range(n_steps):  # every counter value, the last is t = 0 (no noise)
        t = n_steps - 1 - i
        xn, vb = _run_blend(L, x, vc[i], vu[i] if guided else None, tabs, scales, i, n_steps, noise, w, 6, 3)
        assert torch.isfinite(xn).all() and torch.isfinite(vb).all()  # NaN in the pad rows never entered
        # fp64: the same formula on the same fp32 inputs, weights and tables
        w64 = w.double()
        v64 = blend_ref(per_win(vc[i]), wins, x.shape, w64)
        v32 = blend_ref(per_win(vc[i]), wins, x.shape, w)
        if guided:
            u64, u32 = blend_ref(per_win(vu[i]), wins, x.shape, w64), blend_ref(per_win(vu[i]), wins, x.shape, w)
            v64 = u64 + scales[i].double() * (v64 - u64)
            v32 = u32 + scales[i] * (v32 - u32)
        Tb = [tabs[k, t].double() for k in range(5)]
        x0 = Tb[0] * x.double() - Tb[1] * v64
        want = Tb[2] * x0 + Tb[3] * x.double() + (torch.sqrt(Tb[4]) * noise[i].double() if t != 0 else 0.0)
        x32 = p_sample_v(sched, x, v32, t, noise[i])
        e_t, e_h = _err(x32, want), _err(xn, want)
        ev_t, ev_h = _err(v32, v64), _err(vb, v64)
        gx, gv = max(4 * e_t, 2.0 ** -23), max(4 * ev_t, 2.0 ** -23)
        print(f"k_tile_blend_step {mode} i={i}: x hip {e_h:.3e} torch {e_t:.3e} gate {gx:.3e}; "
              f"v hip {ev_h:.3e} torch {ev_t:.3e} gate {gv:.3e}")
        _record(f"tile_blend_step_{mode}_i{i}", x_hip=e_h, x_torch=e_t, v_hip=ev_h, v_torch=ev_t)
        assert e_h <= gx, (i, e_h, e_t)
        assert ev_h <= gv, (i, ev_h, ev_t)


@pytest.mark.parametrize("mode", ["unguided", "guided"])
@torch.no_grad()
def test_chunking_is_invisible_bitwise(mode):
    from tair_amd import _lib
    L = _lib.lib()
    n_steps = 3
    _, tabs, x, vc, vu, noise, w = _blend_inputs(n_steps, seed=29)
    scales = torch.tensor([4.0, 2.5, 0.75], dtype=torch.float32).cuda()
    u = vu[1] if mode == "guided" else None
    xa, va = _run_blend(L, x, vc[1], u, tabs, scales, 1, n_steps, noise, w, 16, 1)
    xb, vb = _run_blend(L, x, vc[1], u, tabs, scales, 1, n_steps, noise, w, 6, 3)
    assert torch.equal(xa.view(torch.int32), xb.view(torch.int32))
    assert torch.equal(va.view(torch.int32), vb.view(torch.int32))


# ----------------------------------------------------------------------------------------- model, tiny
def _make_tiny(max_batch, sd=None):
    from tair_amd.cldm import ControlLDM
    from tair_amd.weights import perturb_norms, synthetic_state_dict
    m = ControlLDM(TINY, max_batch=max_batch, latent_hw=(S, S), with_vae=False, device=torch.device("cuda", 0))
    if sd is None:
        sd = perturb_norms(synthetic_state_dict(m.param_manifest(), seed=7))
    m.load_state_dict(sd)
    return m, sd


@pytest.fixture(scope="module")
def tiny():
    from oracle.ldm_ref import CLDMConfig, ControlLDMRef
    torch.backends.cuda.matmul.allow_tf32 = False
    torch.backends.cudnn.allow_tf32 = False
    m6, sd = _make_tiny(6)
    ref = ControlLDMRef(CLDMConfig(model_channels=64, channel_mult=(1, 2), num_res_blocks=1,
                                   attention_resolutions=(1, 2), head_channels=64, context_dim=64)).cuda().eval()
    ref.load_state_dict(sd, strict=True)
    steps = 4
    g = torch.Generator().manual_seed(83)
    x = torch.randn(B, 4, H, W, generator=g).cuda()
    cond = {"c_txt": torch.randn(1, 77, 64, generator=g).cuda(), "c_img": torch.randn(B, 4, H, W, generator=g).cuda()}
    uncond = {"c_txt": torch.randn(1, 77, 64, generator=g).cuda(), "c_img": torch.randn(B, 4, H, W, generator=g).cuda()}
    noise = torch.randn(steps, B, 4, H, W, generator=g).cuda()
    env = types.SimpleNamespace(m6=m6, sd=sd, ref=ref, steps=steps, x=x, cond=cond, uncond=uncond, noise=noise, oracle={})
    yield env
    m6.close()


def _oracle(env, cfg_scale=None):
    """The reference loop, computed once per guidance setting and shared."""
    from tests._tiled_ref import sample_tiled_ref
    if cfg_scale not in env.oracle:
        env.oracle[cfg_scale] = sample_tiled_ref(env.ref, env.steps, env.x, env.cond, env.noise, S, STRIDE,
                                                 uncond=None if cfg_scale is None else env.uncond,
                                                 cfg_scale=cfg_scale or 1.0)
    return env.oracle[cfg_scale]


def _tiled(s, m, env, cfg_scale=None, x=None, cond=None, noise=None, **kw):
    g = {} if cfg_scale is None else dict(uncond=env.uncond, cfg_scale=cfg_scale)
    x = env.x if x is None else x
    return s.sample(m, "cuda", env.steps, x.shape, cond or env.cond, x_T=x, noise=env.noise if noise is None else noise,
                    tiled=True, tile_size=S, tile_stride=STRIDE, **g, **kw)[0]


@torch.no_grad()
def test_tiny_unguided_one_chunk(tiny):
    from tair_amd.tiling import plan_latent_tiles
    m16, _ = _make_tiny(16, tiny.sd)
    try:
        s = _sampler()
        z = _tiled(s, m16, tiny)
        assert s.last_tiling == dict(windows=T, chunks=1, rows=16, pad=0) == s.tiling_info(m16)
        assert plan_latent_tiles(B, H, W, S, STRIDE, 16, False)["n_chunks"] == 1
        ze = _tiled(s, m16, tiny, use_graph=False)
    finally:
        m16.close()
    e, er = rel_l2(z, _oracle(tiny)), rel_l2(z, ze)
    print(f"tiled tiny 1 chunk: rel-L2 to the reference loop {e:.3e}, graph vs eager {er:.3e}")
    _record("tiled_tiny_unguided_1chunk", rel_l2_z=e, graph_vs_eager=er)
    assert z.shape == tiny.x.shape
    assert e <= FWD_TOL, e
    assert er <= REPLAY_TOL, er


@torch.no_grad()
def test_tiny_unguided_three_chunks(tiny):
    from tair_amd.tiling import plan_latent_tiles
    s = _sampler()
    z = _tiled(s, tiny.m6, tiny)
    p = plan_latent_tiles(B, H, W, S, STRIDE, 6, False)
    want = dict(windows=len(p["windows"]), chunks=p["n_chunks"], rows=p["rows_per_chunk"], pad=p["pad"])
    assert want == dict(windows=8, chunks=3, rows=6, pad=2)
    assert s.last_tiling == want and s.tiling_info(tiny.m6) == want
    ze = _tiled(s, tiny.m6, tiny, use_graph=False)
    e, er = rel_l2(z, _oracle(tiny)), rel_l2(z, ze)
    print(f"tiled tiny 3 chunks: rel-L2 to the reference loop {e:.3e}, graph vs eager {er:.3e}")
    _record("tiled_tiny_unguided_3chunks", rel_l2_z=e, graph_vs_eager=er)
    assert e <= FWD_TOL, e
    assert er <= REPLAY_TOL, er


@torch.no_grad()
def test_tiny_guided_six_chunks(tiny):
    s = _sampler()
    z = _tiled(s, tiny.m6, tiny, 4.0)
    assert s.last_tiling == dict(windows=8, chunks=6, rows=3, pad=2) == s.tiling_info(tiny.m6)
    assert s.last_guided_fused is True
    ze = _tiled(s, tiny.m6, tiny, 4.0, use_graph=False)
    e, er = rel_l2(z, _oracle(tiny, 4.0)), rel_l2(z, ze)
    print(f"tiled tiny guided 6 chunks: rel-L2 to the reference loop {e:.3e}, graph vs eager {er:.3e}")
    _record("tiled_tiny_guided_6chunks", rel_l2_z=e, graph_vs_eager=er)
    assert e <= CFG_TOL, e
    assert er <= REPLAY_TOL, er
    assert rel_l2(z, _oracle(tiny)) > 1e-3  # guidance did something


@torch.no_grad()
def test_tiny_one_window_is_the_untiled_step(tiny):
    g = torch.Generator().manual_seed(85)
    x = torch.randn(1, 4, S, S, generator=g).cuda()
    cond = {"c_txt": tiny.cond["c_txt"], "c_img": torch.randn(1, 4, S, S, generator=g).cuda()}
    noise = torch.randn(tiny.steps, 1, 4, S, S, generator=g).cuda()
    s = _sampler()
    _, tr_t = s.sample_trace(tiny.m6, tiny.steps, x, cond, noise, tiled=True, tile_size=S, tile_stride=STRIDE)
    assert s.last_tiling == dict(windows=1, chunks=1, rows=1, pad=0)
    _, tr_u = s.sample_trace(tiny.m6, tiny.steps, x, cond, noise)
    assert s.last_tiling is None
    e = rel_l2(tr_t[0][1], tr_u[0][1])
    print(f"tiled one window: step-0 v rel-L2 to the untiled step {e:.3e}")
    _record("tiled_tiny_one_window", rel_l2_v0=e)
    assert e <= ONE_WINDOW_TOL, e


@torch.no_grad()
def test_tiny_state_hygiene_on_one_handle(tiny):
    """untiled -> tiled 24x36 -> tiled 16x40 -> untiled on one handle: each equals the same call on a fresh handle
    (no graph of the other kind or geometry replayed, no whole-latent buffer of the other size read)."""
    g = torch.Generator().manual_seed(87)
    xu = torch.randn(3, 4, S, S, generator=g).cuda()
    cu = {"c_txt": tiny.cond["c_txt"], "c_img": torch.randn(3, 4, S, S, generator=g).cuda()}
    nu = torch.randn(tiny.steps, 3, 4, S, S, generator=g).cuda()
    xw = torch.randn(B, 4, 16, 40, generator=g).cuda()
    cw = {"c_txt": tiny.cond["c_txt"], "c_img": torch.randn(B, 4, 16, 40, generator=g).cuda()}
    nw = torch.randn(tiny.steps, B, 4, 16, 40, generator=g).cuda()

    def untiled(s, m):
        return s.sample(m, "cuda", tiny.steps, xu.shape, cu, x_T=xu, noise=nu)[0]
    calls = [untiled, lambda s, m: _tiled(s, m, tiny), lambda s, m: _tiled(s, m, tiny, x=xw, cond=cw, noise=nw), untiled]
    s = _sampler()
    got = [c(s, tiny.m6) for c in calls]
    for k, c in enumerate(calls):
        fresh, _ = _make_tiny(6, tiny.sd)
        try:
            want = c(_sampler(), fresh)
        finally:
            fresh.close()
        e = rel_l2(got[k], want)
        print(f"tiled state hygiene call {k}: rel-L2 to a fresh handle {e:.3e}")
        assert got[k].shape == want.shape
        assert e <= REPLAY_TOL, (k, e)
    assert got[1].shape != got[2].shape
    assert rel_l2(got[1][..., :16, :36], got[2][..., :16, :36]) > 1e-3  # the two tiled results differ


@torch.no_grad()
def test_tiled_argument_rules_raise_value_error(tiny):
    s = _sampler()
    small = torch.randn(1, 4, 12, 36).cuda()
    with pytest.raises(ValueError, match="smaller than the tile"):
        s.sample(tiny.m6, "cuda", 2, small.shape, {"c_txt": tiny.cond["c_txt"]}, x_T=small, tiled=True, tile_size=S,
                 tile_stride=STRIDE)
    two = dict(tiny.cond, c_txt=tiny.cond["c_txt"].expand(2, -1, -1).contiguous())
    with pytest.raises(ValueError, match="c_txt batch 2 must be 1"):
        _tiled(s, tiny.m6, tiny, cond=two)
    cfg = types.SimpleNamespace(exp_args={"unet_feat_sampling_timestep": [1]})
    with pytest.raises(ValueError, match="feature steps"):
        _tiled(s, tiny.m6, tiny, cfg=cfg)
    with pytest.raises(ValueError, match="tile_size 8 must equal"):
        s.sample(tiny.m6, "cuda", 2, tiny.x.shape, tiny.cond, x_T=tiny.x, tiled=True, tile_size=8, tile_stride=4)


# ---------------------------------------------------------------------------------- model, full width
@pytest.fixture(scope="module")
def full():
    from oracle.ldm_ref import ControlLDMRef
    from oracle.vae_ref import AutoencoderKLRef
    from tair_amd.cldm import ControlLDM
    from tair_amd.pipeline import vae_synthetic_state_dict
    from tair_amd.weights import manifest, perturb_norms, synthetic_state_dict
    torch.backends.cuda.matmul.allow_tf32 = False
    torch.backends.cudnn.allow_tf32 = False
    sd = perturb_norms(synthetic_state_dict(manifest(), seed=0))
    m = ControlLDM(max_batch=2, with_vae=True)
    m.load_state_dict(sd)
    ref = ControlLDMRef().cuda().eval()
    ref.load_state_dict(sd, strict=True)
    del sd
    vae_ref = AutoencoderKLRef().cuda().eval()
    vsd = vae_synthetic_state_dict(vae_ref, seed=0)
    vae_ref.load_state_dict(vsd, strict=True)
    m.vae.load_state_dict(vsd, strict=True)
    m._vae_hip = m._vae_hip_enc = None
    yield m, ref, vae_ref
    m.close()


@torch.no_grad()
def test_full_width_tiled_vs_oracle(full):
    from tests._tiled_ref import sample_tiled_ref
    m, ref, _ = full
    steps = 3
    g = torch.Generator().manual_seed(73)
    x = torch.randn(1, 4, 64, 96, generator=g).cuda()
    cond = {"c_txt": torch.randn(1, 77, 1024, generator=g).cuda(), "c_img": torch.randn(1, 4, 64, 96, generator=g).cuda()}
    noise = torch.randn(steps, 1, 4, 64, 96, generator=g).cuda()
    s = _sampler()
    z, feats = s.sample(m, "cuda", steps, x.shape, cond, x_T=x, noise=noise, tiled=True, tile_size=64, tile_stride=32)
    assert feats == [] and s.last_tiling == dict(windows=2, chunks=1, rows=2, pad=0)
    zr = sample_tiled_ref(ref, steps, x, cond, noise, 64, 32)
    e = rel_l2(z, zr)
    print(f"tiled full width 64x96: rel-L2 to the reference loop {e:.3e}")
    _record("tiled_full_64x96", rel_l2_z=e)
    assert e <= FWD_TOL, e


def _ctx(prompts):
    out = []
    for p in prompts:
        g = torch.Generator().manual_seed(sum(map(ord, p)) + 7 * len(p))
        out.append(torch.randn(77, 1024, generator=g))
    return torch.stack(out).cuda()


def _apply(pipe, img, tiled, steps=4):
    return pipe.apply_cldm(img, steps, 0.8, False, 256, False, 256, tiled, 512, 256, "a sign with words",
                           "low quality", 1.0, "noise", "spaced", 0, False, seed=123)


@torch.no_grad()
def test_pipeline_tiled_vs_oracle(full):
    from oracle.pipeline_ref import vae_encode_cond
    from tair_amd.diffusion import Diffusion
    from tair_amd.pipeline import Pipeline
    from tests._tiled_ref import sample_tiled_ref
    m, ref, vae_ref = full
    steps = 4
    d = Diffusion(linear_start=0.00085, linear_end=0.012, zero_snr=True, parameterization="v")
    pipe = Pipeline(None, m, d, None, "cuda", text_encoder=_ctx)
    img = torch.rand(1, 3, 512, 768, generator=torch.Generator().manual_seed(13)).cuda()
    x_hip = _apply(pipe, img, True, steps)
    assert x_hip.shape == (1, 3, 512, 768)
    assert m.control_scales == [1.0] * 13
    # the reference on the same draws, in the order apply_cldm draws them
    gen = torch.Generator(device="cuda").manual_seed(123)
    r = lambda shape: torch.randn(shape, generator=gen, device="cuda", dtype=torch.float32)  # noqa: E731
    x_T, noise = r((1, 4, 64, 96)), r((steps, 1, 4, 64, 96))
    c_img = vae_encode_cond(vae_ref, img)
    saved = ref.control_scales
    ref.control_scales = [0.8] * 13
    try:
        z = sample_tiled_ref(ref, steps, x_T, {"c_txt": _ctx(["a sign with words"]), "c_img": c_img}, noise, 64, 32)
    finally:
        ref.control_scales = saved
    x_ref = vae_ref.decode(z / 0.18215)
    e = rel_l2(x_hip, x_ref)
    print(f"[pipeline] cldm_tiled 512x768: apply_cldm image rel-L2 {e:.3e}")
    _record("tiled_pipeline_512x768", rel_l2_image=e)
    assert e <= 6e-3, e


@torch.no_grad()
def test_pipeline_tiled_one_window_equals_untiled(full):
    from tair_amd.diffusion import Diffusion
    from tair_amd.pipeline import Pipeline
    m, _, _ = full
    d = Diffusion(linear_start=0.00085, linear_end=0.012, zero_snr=True, parameterization="v")
    pipe = Pipeline(None, m, d, None, "cuda", text_encoder=_ctx)
    img = torch.rand(1, 3, 512, 512, generator=torch.Generator().manual_seed(15)).cuda()
    a, b = _apply(pipe, img, True), _apply(pipe, img, False)
    e = rel_l2(a, b)
    print(f"[pipeline] cldm_tiled 512x512 vs untiled: rel-L2 {e:.3e}")
    _record("tiled_pipeline_one_window", rel_l2_image=e)
    assert e <= ONE_WINDOW_TOL, e
