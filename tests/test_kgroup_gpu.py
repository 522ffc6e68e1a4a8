"""Two-K-group 64-row tiles (gemm_kern.h gemm_kgroup_kernel; kernel id 5), forced through force_stages = 203 at
the smallest shapes that can go wrong: one K-tile (K-group 1 idle), odd tile counts (group 1 idle on the last
trip), ragged M / N, several workgroups, K slices of 2-2-1 tiles, the three split-K combines (cooperative,
last arriver, reduce kernel), stride-1 3x3 convs with and without the skip K-extension, and one case per
epilogue set of the denoise step.

Reference: the fp64 product of the same bf16 operands.  Gate (tests/test_lnfold_gpu.py): the output is ONE bf16
rounding of an fp32 value, so its rel-L2 against fp64 may exceed the rounding floor (rel-L2 of bf16(ref) vs ref)
by at most 15%.  Statistics equal fp64 sums of the stored values (rel 1e-12: fp64 adds in another order).  Guard
rows / columns stay untouched, tickets return to zero, and a second launch gives the same bits.
"""
import ctypes

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

ONE_ROUNDING = 1.15
KG = 203  # force_stages: two K-groups, 3-stage rings
KERN_KGROUP = 5


def _L():
    from tair_amd import _lib
    return _lib.lib(), _lib


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def rel_l2(a, b):
    a, b = a.double(), b.double()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def _floor(ref):
    return rel_l2(ref.to(torch.bfloat16), ref)


def _desc(**kw):
    _, lib = _L()
    d = lib.GemmDesc()
    d.alpha = 1.0
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def _gemm(d):
    L, _ = _L()
    out = [ctypes.c_int() for _ in range(4)]
    assert L.tair_k_gemm_plan(ctypes.byref(d), *[ctypes.byref(o) for o in out]) == 0, L.tair_last_error()
    assert out[3].value == KERN_KGROUP and out[2].value == d.force_splits, [o.value for o in out]
    rc = L.tair_k_gemm(ctypes.byref(d), _stream())
    assert rc == 0, L.tair_last_error()
    torch.cuda.synchronize()
    cnt = ctypes.c_int()
    assert L.tair_fault_count(1, ctypes.byref(cnt)) == 0 and cnt.value == 0


_WS = {}


def _ws():
    """split-K workspace and tickets, shared by every case (tickets must come back zeroed)"""
    if not _WS:
        _WS["part"] = torch.empty(4 << 20, device="cuda")
        _WS["sem"] = torch.zeros(1 << 14, device="cuda", dtype=torch.int32)
    return _WS["part"], _WS["sem"]


def _combine_kw(mode):
    """coop: tickets (the grid is resident: cooperative combine); last: tickets + probe bit 2 (last-arriver combine
    at any split count); reduce: no tickets (fp32 slabs summed by the reduce kernel)"""
    part, sem = _ws()
    kw = dict(partial=part.data_ptr(), partial_cap=part.numel())
    if mode in ("coop", "last"):
        kw.update(tile_sem=sem.data_ptr(), sem_cap=sem.numel())
    if mode == "last":
        kw.update(probe=4)
    return kw


def _run_guarded(M, N, make_desc, check):
    """two launches into fresh guarded buffers: guards untouched, bits equal; check(out) on the first"""
    outs = []
    for _ in range(2):
        buf = torch.full((M + 64, N + 32), 5.0, device="cuda", dtype=torch.bfloat16)
        _gemm(make_desc(buf))
        assert bool((buf[M:] == 5.0).all()) and bool((buf[:, N:] == 5.0).all())
        outs.append(buf[:M, :N])
    check(outs[0])
    assert torch.equal(outs[0], outs[1])
    assert torch.count_nonzero(_ws()[1]) == 0


_DENSE = {}


def _dense_operands(K):
    """A [200][K], W [200][K] bf16, bias, and the fp64 product + bias of the whole block (computed once per K)"""
    if K not in _DENSE:
        g = torch.Generator(device="cuda").manual_seed(1000 + K)
        A = torch.randn(200, K, device="cuda", generator=g).to(torch.bfloat16)
        W = (torch.randn(200, K, device="cuda", generator=g) / K ** 0.5).to(torch.bfloat16)
        bias = torch.randn(200, device="cuda", generator=g)
        _DENSE[K] = (A, W, bias, A.double() @ W.double().t() + bias.double())
    return _DENSE[K]


# K = 64: K-group 1 has no tile; 192: odd count; 320 in 3 slices: 2-2-1 tiles; 192 in 3: one tile per slice
@pytest.mark.parametrize("bn", [64, 128])
@pytest.mark.parametrize("K,splits", [(64, 1), (128, 1), (192, 1), (320, 1), (128, 2), (320, 2), (320, 3), (192, 3)])
def test_dense_shapes_and_combines(bn, K, splits):
    A, W, bias, ref_all = _dense_operands(K)
    modes = ["none"] if splits == 1 else ["coop", "last", "reduce"]
    # (64, 64) one full tile; ragged M = 40, N = 72; (168, 200): 3 x 4 (or 3 x 2) workgroups, ragged both ways
    for M, N in [(64, 64), (40, 64), (64, 72), (40, 72), (168, 200)]:
        ref = ref_all[:M, :N]
        fl = _floor(ref)
        for mode in modes:
            kw = _combine_kw(mode) if splits > 1 else {}

            def make(buf):
                return _desc(M=M, N=N, K=K, amode=0, A=A.data_ptr(), lda=K, Wt=W.data_ptr(), ldw=K,
                             bias=bias.data_ptr(), out=buf.data_ptr(), ldo=N + 32, force_bm=64, force_bn=bn,
                             force_splits=splits, force_stages=KG, **kw)

            def check(out):
                e = rel_l2(out, ref)
                print(f"dense 64x{bn} K={K} s={splits} {mode} M={M} N={N}: rel-L2 {e:.3e} floor {fl:.3e}")
                assert e <= ONE_ROUNDING * fl, (M, N, mode, e, fl)

            _run_guarded(M, N, make, check)


def _pack_conv_w(w):
    """[Cout, Cin, 3, 3] -> [Cout][9 Cin] in the GEMM's channel-chunk-major K order (kernels.h A_CONV3)"""
    co, ci = w.shape[:2]
    p = w.permute(0, 2, 3, 1).reshape(co, 9, ci // 64, 64).permute(0, 2, 1, 3)
    return p.reshape(co, 9 * ci)


@pytest.mark.parametrize("bn", [64, 128])
@pytest.mark.parametrize("C,skip,splits", [(64, False, 1), (64, True, 1), (128, False, 1), (128, True, 2),
                                           (64, False, 2), (64, True, 3)])
def test_conv3_8x8(bn, C, skip, splits):
    """8 x 8 image, N = 64: C = 64 is nine K-tiles (odd), + a 64-channel 1x1 skip conv as the K-extension"""
    g = torch.Generator(device="cuda").manual_seed(7 * C + skip)
    H, N, Cx = 8, 64, 64
    M = H * H
    x = torch.randn(1, C, H, H, device="cuda", generator=g).to(torch.bfloat16)
    w = (torch.randn(N, C, 3, 3, device="cuda", generator=g) / (9 * C) ** 0.5).to(torch.bfloat16)
    xs = torch.randn(M, Cx, device="cuda", generator=g).to(torch.bfloat16)
    wsk = (torch.randn(N, Cx, device="cuda", generator=g) / Cx ** 0.5).to(torch.bfloat16)
    bias = torch.randn(N, device="cuda", generator=g)
    ref = F.conv2d(x.double(), w.double(), padding=1).permute(0, 2, 3, 1).reshape(M, N) + bias.double()
    Kx = Cx if skip else 0
    if skip:
        ref = ref + xs.double() @ wsk.double().t()
    wp = torch.zeros(N, 9 * C + Kx, device="cuda", dtype=torch.bfloat16)
    wp[:, :9 * C] = _pack_conv_w(w)
    if skip:
        wp[:, 9 * C:] = wsk
    a = x.permute(0, 2, 3, 1).reshape(M, C).contiguous()
    fl = _floor(ref)
    for mode in (["none"] if splits == 1 else ["coop", "last", "reduce"]):
        kw = _combine_kw(mode) if splits > 1 else {}
        if skip:
            kw.update(X=xs.data_ptr(), ldx=Cx, Kx=Kx)

        def make(buf):
            return _desc(M=M, N=N, K=9 * C, amode=1, A=a.data_ptr(), lda=C, C=C, Bn=1, H=H, W=H, Ho=H, Wo=H,
                         rows_per_b=M, Wt=wp.data_ptr(), ldw=9 * C + Kx, bias=bias.data_ptr(), out=buf.data_ptr(),
                         ldo=N + 32, force_bm=64, force_bn=bn, force_splits=splits, force_stages=KG, **kw)

        def check(out):
            e = rel_l2(out, ref)
            print(f"conv 64x{bn} C={C} skip={skip} s={splits} {mode}: rel-L2 {e:.3e} floor {fl:.3e}")
            assert e <= ONE_ROUNDING * fl, (mode, e, fl)

        _run_guarded(M, N, make, check)


_EPI = {}


def _epi_operands():
    """M = 128 (two row tiles of two 64-pixel images), N = 128, K = 192 (odd tile count): a LayerNorm-input-like A"""
    if not _EPI:
        g = torch.Generator(device="cuda").manual_seed(42)
        M, N, K = 128, 128, 192
        mu = torch.randn(M, 1, device="cuda", generator=g) * 1.5
        sd = torch.rand(M, 1, device="cuda", generator=g) + 0.5
        A = (torch.randn(M, K, device="cuda", generator=g) * sd + mu).to(torch.bfloat16)
        W = (torch.randn(N, K, device="cuda", generator=g) / K ** 0.5).to(torch.bfloat16)
        bias = torch.randn(N, device="cuda", generator=g) * 0.2
        r0 = (torch.randn(M, N, device="cuda", generator=g) * 2 + 0.5).to(torch.bfloat16)
        _EPI.update(M=M, N=N, K=K, A=A, W=W, bias=bias, r0=r0, prod=A.double() @ W.double().t())
    return _EPI


EPI_SETS = ["bias", "bias_res", "bias_res_rowst", "lnfold", "geglu", "gnstats", "hilo"]


@pytest.mark.parametrize("bn", [64, 128])
@pytest.mark.parametrize("splits", [1, 2])
@pytest.mark.parametrize("kind", EPI_SETS)
def test_epilogue_sets(kind, splits, bn):
    o = _epi_operands()
    M, N, K, A, W, bias, r0, prod = (o[k] for k in ("M", "N", "K", "A", "W", "bias", "r0", "prod"))
    nout = N // 2 if kind == "geglu" else N
    kw = dict(M=M, N=N, K=K, amode=0, A=A.data_ptr(), lda=K, Wt=W.data_ptr(), ldw=K, bias=bias.data_ptr(),
              force_bm=64, force_bn=bn, force_splits=splits, force_stages=KG)
    if splits > 1:
        kw.update(_combine_kw("coop"))
    ref = prod + bias.double()
    res = kind in ("bias_res", "bias_res_rowst")
    if res:
        ref = ref + r0.double()
    rst = torch.zeros(M, 2, device="cuda", dtype=torch.float64)
    if kind == "bias_res_rowst":
        kw.update(rst=rst.data_ptr())
    if kind == "lnfold":
        ad = A.double()
        lnst = torch.stack([ad.sum(1), (ad * ad).sum(1)], -1).contiguous()
        cs = W.double().sum(1).float()
        mean = lnst[:, 0:1] / K
        rstd = 1.0 / torch.sqrt((lnst[:, 1:2] / K - mean * mean).clamp_min(0) + 1e-5)
        ref = rstd * (prod - mean * cs.double()) + bias.double()
        kw.update(lnst=lnst.data_ptr(), lncs=cs.data_ptr(), ln_c=float(K), ln_eps=1e-5)
    if kind == "geglu":  # column quads (x, x, gate, gate) -> two output columns
        h = ref.view(M, N // 4, 2, 2)
        ref = (h[:, :, 0, :] * F.gelu(h[:, :, 1, :])).reshape(M, nout)
        kw.update(act=2)
    G, hw = 8, 64
    st = torch.zeros(8, (M // hw) * G * 2, device="cuda", dtype=torch.float64)
    if kind == "gnstats":
        kw.update(st_acc=st.data_ptr(), st_rs=st.shape[1], st_cg=N // G, st_G=G, st_coff=0, st_hw=hw, rows_per_b=hw)
    fl = _floor(ref)
    outs = []
    for _ in range(2):
        planes = 2 if kind == "hilo" else 1
        buf = torch.full((planes, M + 64, nout + 32), 5.0, device="cuda", dtype=torch.bfloat16)
        if res:
            buf[0, :M, :nout] = r0
        k2 = dict(kw, out=buf.data_ptr(), ldo=nout + 32)
        if res:
            k2.update(res=buf.data_ptr(), ld_res=nout + 32)
        if kind == "hilo":
            k2.update(out_lo=buf[1].data_ptr() - buf[0].data_ptr() >> 1)
        rst.zero_()
        st.zero_()
        _gemm(_desc(**k2))
        assert bool((buf[:, M:] == 5.0).all()) and bool((buf[:, :, nout:] == 5.0).all())
        outs.append(buf[:, :M, :nout].clone())
    out = outs[0][0]
    e = rel_l2(out, ref)
    print(f"epilogue {kind} 64x{bn} s={splits}: rel-L2 {e:.3e} floor {fl:.3e}")
    assert e <= ONE_ROUNDING * fl, (e, fl)
    assert torch.equal(outs[0], outs[1])
    assert torch.count_nonzero(_ws()[1]) == 0
    od = out.double()
    if kind == "bias_res_rowst":
        want = torch.stack([od.sum(1), (od * od).sum(1)], -1)
        assert rel_l2(rst, want) <= 1e-12, rel_l2(rst, want)
    if kind == "gnstats":
        gr = od.view(M // hw, hw, G, N // G)
        want = torch.stack([gr.sum(dim=(1, 3)), (gr * gr).sum(dim=(1, 3))], -1).flatten()
        assert rel_l2(st.sum(0), want) <= 1e-12, rel_l2(st.sum(0), want)
    if kind == "hilo":  # lo = bf16(v - hi): hi + lo carries v to ~2^-16
        e2 = rel_l2(outs[0][0].float() + outs[0][1].float(), ref)
        print(f"  hi + lo rel-L2 {e2:.3e}")
        assert e2 <= 2e-5, e2


@torch.no_grad()
def test_tiny_model_forward_on_forced_two_group_plans():
    """The tiny ControlLDM forward (the smoke model: 64 / 128 channels, two 16 x 16 latents) with every 64-row
    3-stage tile plan forced onto the two-K-group kernel (tair_k_gemm_kgroup_force: one- and two-K-tile linears,
    9 / 18 K-tile convs with and without the skip K-extension, every epilogue of the network), against the fp32
    oracle inside the forward gate of smoke() and tests/test_cldm_gpu.py: rel-L2 < 5e-3."""
    from oracle.ldm_ref import CLDMConfig, ControlLDMRef
    from tair_amd.cldm import ControlLDM
    from tair_amd.weights import perturb_norms, synthetic_state_dict
    L, _ = _L()
    tiny = dict(model_channels=64, channel_mult=[1, 2], num_res_blocks=1, attention_resolutions=[1, 2],
                num_head_channels=64, context_dim=64, in_channels=4, out_channels=4)
    dev = torch.device("cuda", 0)
    m = ControlLDM(tiny, max_batch=2, latent_hw=(16, 16), device=dev, with_vae=False)
    sd = perturb_norms(synthetic_state_dict(m.param_manifest(), seed=3))
    m.load_state_dict(sd)
    ref = ControlLDMRef(CLDMConfig(model_channels=64, channel_mult=(1, 2), num_res_blocks=1,
                                   attention_resolutions=(1, 2), head_channels=64, context_dim=64)).eval()
    ref.load_state_dict(sd, strict=True)
    g = torch.Generator().manual_seed(5)
    x = torch.randn(2, 4, 16, 16, generator=g)
    c_img = torch.randn(2, 4, 16, 16, generator=g)
    c_txt = torch.randn(1, 77, 64, generator=g)
    t = torch.tensor([999, 341])
    cond = {"c_txt": c_txt.to(dev), "c_img": c_img.to(dev)}
    rv, _ = ref(x, t, {"c_txt": c_txt.expand(2, -1, -1), "c_img": c_img})
    v0, _ = m(x.to(dev), t.to(dev), cond, want_feats=False)  # the planner's own plans
    torch.cuda.synchronize()
    L.tair_k_gemm_kgroup_force(1)
    try:
        v1, _ = m(x.to(dev), t.to(dev), cond, want_feats=False)
        torch.cuda.synchronize()
    finally:
        launches = L.tair_k_gemm_kgroup_force(0)
    m.close()
    e0, e1 = rel_l2(v0.cpu(), rv), rel_l2(v1.cpu(), rv)
    print(f"tiny forward rel-L2 vs oracle: planner's plans {e0:.3e}, two-group plans forced {e1:.3e} "
          f"({launches} two-K-group launches)")
    assert launches >= 20, launches  # the forward's convs and linears did run on the new kernel
    assert e1 < 5e-3, e1
