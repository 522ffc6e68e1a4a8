"""Tiled VAE (tair_amd/vae.py split_tiles / decode_tiled / encode_mode_tiled, ControlLDM.vae_tiling,
Pipeline.apply_cldm) against the restatement of the reference's tiled VAE, tests/_tiled_vae_ref.py (host only).

Gates (written here):
* torch-backend tiled decode / encode vs the restatement: rel-L2 <= 1e-5 -- the same fp32 arithmetic in another
  order (batch_norm with given statistics against (x - mean) * rstd; bmm + softmax against SDPA).
* The gate of the GPU tests (2e-4, tests/test_vae_tiling_gpu.py) can see the semantics: on the restatement alone,
  the tiled decode of the test latent differs from the untiled decode and from a variant that normalises with the
  union's exact variance by at least 10 x 2e-4 each (measured with ch = 32: 4.3e-1 and 7.8e-2).
"""
import ctypes
import types

import pytest
import torch

import _tiled_vae_ref as tr

GPU_GATE = 2e-4
CH = 32  # both constructors take a width: a quarter of the full one keeps these tests to seconds


def rel_l2(a, b):
    a, b = a.double(), b.double()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def _axis(fn, extent, tile, is_decoder):
    """The boxes along x of a square input: [lo, hi] of the first row of tiles."""
    ins, outs = fn(extent, extent, tile, is_decoder)
    n = len({tuple(b[:2]) for b in ins})
    assert len(ins) == n * n
    return [b[:2] for b in ins[:n]], [b[:2] for b in outs[:n]]


KNOWN = [  # (is_decoder, extent, tile, input boxes, output boxes | None): by hand from tilevae.py:325-397
    (True, 40, 8, [[0, 30], [8, 38], [16, 40]], [[0, 152], [152, 216], [216, 320]]),
    (True, 32, 8, [[0, 30], [8, 32]], [[0, 152], [152, 256]]),
    (True, 128, 64, [[0, 86], [64, 128]], None),
    (False, 200, 64, [[0, 128], [64, 192], [128, 200]], [[0, 12], [12, 20], [20, 25]]),
    (False, 128, 64, [[0, 128]], [[0, 16]]),
    (False, 1024, 512, [[0, 544], [480, 1024]], None),
]


@pytest.mark.parametrize("which", ["product", "restatement"])
@pytest.mark.parametrize("is_decoder,extent,tile,want_in,want_out", KNOWN)
def test_split_known_answers(which, is_decoder, extent, tile, want_in, want_out):
    from tair_amd.vae import split_tiles
    ins, outs = _axis(split_tiles if which == "product" else tr.split_tiles, extent, tile, is_decoder)
    assert ins == want_in
    if want_out is not None:
        assert outs == want_out


def test_split_agrees_with_the_restatement_and_partitions_the_result():
    from tair_amd.vae import split_tiles, tiling_needed
    n = 0
    for is_decoder, extents, tiles in ((True, range(8, 72, 3), (8, 16, 24)), (False, range(64, 400, 24), (64, 96, 128))):
        for h in extents:
            for w in extents:
                for tile in tiles:
                    assert tiling_needed(h, w, tile, is_decoder) == (not tr.is_tiny(h, w, tile, is_decoder))
                    if not tiling_needed(h, w, tile, is_decoder):
                        continue
                    got = split_tiles(h, w, tile, is_decoder)
                    assert got == tr.split_tiles(h, w, tile, is_decoder), (is_decoder, h, w, tile)
                    oh, ow = (8 * h, 8 * w) if is_decoder else (h // 8, w // 8)
                    cover = torch.zeros(oh, ow, dtype=torch.int32)
                    for ib, ob in zip(*got):
                        cover[ob[2]:ob[3], ob[0]:ob[1]] += 1
                        s = [v * 8 if is_decoder else v // 8 for v in ib]  # the output box lies inside the tile
                        assert s[0] <= ob[0] < ob[1] <= s[1] and s[2] <= ob[2] < ob[3] <= s[3], (h, w, tile, ib, ob)
                    assert bool((cover == 1).all()), (is_decoder, h, w, tile)
                    n += 1
    assert n > 1000


def test_merge_of_two_tiles_by_hand():
    """Tiles of 4 and 12 pixels, (mean, var) = (1, 2) and (5, 6): weights 1/4 and 3/4 give mean 4 and var 5 -- the
    union's variance would be 5 + (1/4) 3^2 + (3/4) 1^2 = 8."""
    v = [torch.tensor([2.0]), torch.tensor([6.0])]
    m = [torch.tensor([1.0]), torch.tensor([5.0])]
    var, mean = tr.merge_stats(v, m, [4, 12])
    assert mean.item() == pytest.approx(4.0, rel=1e-6) and var.item() == pytest.approx(5.0, rel=1e-6)
    var_u, mean_u = tr.merge_stats(v, m, [4, 12], union_variance=True)
    assert mean_u.item() == pytest.approx(4.0, rel=1e-6) and var_u.item() == pytest.approx(8.0, rel=1e-6)
    # and the product's torch path on two real tiles: constant tiles 1 and 5 -> var 0, mean 4; x = 5 normalises to
    # (5 - 4) / sqrt(0 + 1e-6)
    from tair_amd.vae import _merged_group_norm
    gn = torch.nn.GroupNorm(32, 32, eps=1e-6)
    a, b = torch.full((1, 32, 2, 2), 1.0), torch.full((1, 32, 2, 6), 5.0)
    ya, yb = _merged_group_norm([a, b], gn, False)
    assert torch.allclose(yb, torch.full_like(yb, 1e3), rtol=1e-5) and torch.allclose(ya, torch.full_like(ya, -3e3), rtol=1e-5)


@pytest.fixture(scope="module")
def vaes():
    from oracle.vae_ref import AutoencoderKLRef, Decoder, Encoder
    from tair_amd.pipeline import vae_synthetic_state_dict
    from tair_amd.vae import AutoencoderKL
    ref = AutoencoderKLRef()
    ref.encoder, ref.decoder = Encoder(ch=CH), Decoder(ch=CH)
    ref.eval()
    sd = vae_synthetic_state_dict(ref, seed=0)
    ref.load_state_dict(sd, strict=True)
    prod = AutoencoderKL(ch=CH).eval()
    prod.load_state_dict(sd, strict=True)
    return ref, prod


@pytest.fixture(scope="module")
def decoded(vaes):
    """The restatement's tiled decode of the test latent, computed once."""
    ref, _ = vaes
    z = tr.ramp_latent(1, 40, 32, seed=7)
    return z, tr.decode_tiled(ref, z, 8)


@torch.no_grad()
def test_tiny_rule_is_bitwise_the_untiled_call(vaes):
    _, prod = vaes
    z = torch.randn(1, 4, 30, 24, generator=torch.Generator().manual_seed(1))  # 30 = 2 * 11 + 8
    assert torch.equal(prod.decode_tiled(z, 8), prod.decode(z))
    x = torch.rand(1, 3, 128, 96, generator=torch.Generator().manual_seed(2)) * 2 - 1  # 128 = 2 * 32 + 64
    assert torch.equal(prod.encode_mode_tiled(x, 64), prod.encode_mode(x))
    g1, g2 = torch.Generator().manual_seed(3), torch.Generator().manual_seed(3)
    assert torch.equal(prod.encode_sample_tiled(x, 64, generator=g1), prod.encode_sample(x, generator=g2))


@torch.no_grad()
def test_torch_tiled_decode_matches_the_restatement(vaes, decoded):
    _, prod = vaes
    z, want = decoded
    got = prod.decode_tiled(z, 8)
    assert got.shape == want.shape == (1, 3, 320, 256)
    e = rel_l2(got, want)
    print(f"torch tiled decode vs restatement: rel-L2 {e:.3e}")
    assert e <= 1e-5, e


@torch.no_grad()
def test_torch_tiled_encode_matches_the_restatement(vaes):
    ref, prod = vaes
    x = torch.rand(1, 3, 200, 128, generator=torch.Generator().manual_seed(9)) * 2 - 1
    x = x + 0.5 * torch.linspace(-1, 1, 200).view(1, 1, 200, 1)
    want = tr.encode_mode_tiled(ref, x, 64)
    got = prod.encode_mode_tiled(x, 64)
    assert got.shape == want.shape == (1, 4, 25, 16)
    e = rel_l2(got, want)
    print(f"torch tiled encode vs restatement: rel-L2 {e:.3e}")
    assert e <= 1e-5, e
    # the sampled posterior shares the mean: with the same generator state, sample - mode = std * noise, finite
    s = prod.encode_sample_tiled(x, 64, generator=torch.Generator().manual_seed(4))
    assert s.shape == got.shape and torch.isfinite(s).all() and not torch.equal(s, got)


@torch.no_grad()
def test_the_gpu_gate_can_see_the_semantics(vaes, decoded):
    ref, _ = vaes
    z, tiled = decoded
    e_untiled = rel_l2(ref.decode(z), tiled)
    e_union = rel_l2(tr.decode_tiled(ref, z, 8, union_variance=True), tiled)
    print(f"restatement: tiled vs untiled {e_untiled:.3e}, tiled vs union-variance {e_union:.3e}")
    assert e_untiled >= 10 * GPU_GATE, e_untiled
    assert e_union >= 10 * GPU_GATE, e_union


def test_gn_stats_merge_rejects_bad_arguments_without_a_device():
    from tair_amd import _lib
    L = _lib.lib()
    assert "tair_k_gn_stats_merge" in _lib.SIGNATURES and "tair_k_softmax_split_pad" in _lib.SIGNATURES
    p = ctypes.c_void_p(0x1000)  # never dereferenced: every call below is refused before any launch

    def merge(slots=p, stride=8 * 128, T=3, px=(900, 720, 576), B=2, G=32, cg=16, rs=128):
        arr = (ctypes.c_int * len(px))(*px) if px is not None else None
        return L.tair_k_gn_stats_merge(slots, stride, T, arr, B, G, cg, rs, None)

    assert merge(T=0) == -1
    assert b"gn_stats_merge" in L.tair_last_error()
    assert merge(B=0) == -1
    assert merge(px=(900, 0, 576)) == -1
    assert merge(slots=None) == -1
    assert merge(px=None) == -1
    assert merge(T=257, px=(1,) * 257) == -1
    assert merge(rs=64) == -1            # a replica narrower than B * G pairs
    assert merge(stride=128) == -1       # slots that overlap
    assert merge(cg=0) == -1 and merge(G=0) == -1
    assert b"gn_stats_merge" in L.tair_last_error()
    # the padded attention helpers refuse a plane width that is no multiple of 64 or below L
    assert L.tair_k_softmax_split_pad(p, 960, 900, 900, 900, p, None) == -1
    assert b"softmax_split_pad" in L.tair_last_error()
    assert L.tair_k_softmax_split_pad(p, 960, 900, 900, 896, p, None) == -1
    assert L.tair_k_transpose_split_pad(p, 1, 900, 900, 512, p, None) == -1
    assert b"transpose_split_pad" in L.tair_last_error()
    assert L.tair_k_transpose_split_pad(None, 1, 900, 960, 512, p, None) == -1


def test_hip_passes_plan_on_the_host_and_size_their_statistics_pool():
    """decode_tiled / encode_mode_tiled on the CPU with the recording stand-in of tests/_vae_cases.py: every GEMM of
    the tiled passes (tiles of 30x30, 30x24, 24x24 latent: M and the attention's L off multiples of 64; B = 2 images
    of 720 pixels go one launch per image) is a plan the library accepts, the attention's reduction is padded to a
    multiple of 64, and the pool holds one slot per tile and statistics-producing GEMM."""
    import _vae_cases as vc
    from tair_amd.vae import AutoencoderKL
    from tair_amd.vae_hip import HipVAEDecoder, HipVAEEncoder
    prod = AutoencoderKL().eval()  # full width: the GEMM takes channel counts in multiples of 64
    W = 512

    def record(cls, fn, x, tile):
        hip = cls(prod, "cpu", max_batch=2)
        hip.part = torch.empty(1, dtype=torch.float32).expand(64 << 20)
        hip.L = rec = vc.RecordingLib()
        hip._stream = lambda: ctypes.c_void_p(None)
        getattr(hip, fn)(x, tile)
        assert rec.calls and all(c[1][4] == 0 for c in rec.calls), [c[1] for c in rec.calls if c[1][4]]
        assert all(K % 64 == 0 for _, (M, N, K, Kx, rc) in rec.calls if K > 64)
        return hip, rec.calls

    hip, calls = record(HipVAEDecoder, "decode_tiled", torch.zeros(1, 4, 40, 32), 8)
    n_producers = 1 + sum(2 if kind == "res" else 1 for kind, _ in hip.blocks)
    assert hip._next_stat == 6 * n_producers and hip.n_stats >= hip._next_stat > 64
    assert {(M, K) for sig, (M, N, K, Kx, rc) in calls if sig[0] == 0 and N == W and K != 3 * W} == \
        {(900, 3 * 960), (720, 3 * 768), (576, 3 * 576)}  # P.V: K = 3 roundup(L, 64)
    hip, calls2 = record(HipVAEDecoder, "decode_tiled", torch.zeros(2, 4, 32, 24), 8)
    assert hip._next_stat == 2 * n_producers
    assert 720 in {M for _, (M, N, K, Kx, rc) in calls2} and 1440 in {M for _, (M, N, K, Kx, rc) in calls2}
    record(HipVAEEncoder, "encode_mode_tiled", torch.zeros(1, 3, 200, 128), 64)
    # the untiled passes keep the 64-slot pool
    hip, _ = record(HipVAEDecoder, "decode_tiled", torch.zeros(1, 4, 30, 24), 8)
    assert hip.n_stats == 64


def test_gemm_statistics_take_one_image_of_any_pixel_count():
    """The GEMM's statistics epilogue gives a whole 64-row tile to one image: several images need hw % 64 == 0, one
    image (M == hw) may have any pixel count -- which is how the tiled passes launch tiles such as 30 x 24."""
    import _vae_cases as vc
    from tair_amd import _lib

    def status(M, hw):
        d = _lib.GemmDesc()
        d.M, d.N, d.K, d.amode, d.alpha, d.rows_per_b = M, 512, 1536, 0, 1.0, 1
        d.A = d.Wt = d.out = 0x1000  # planning only: never dereferenced
        d.lda = d.ldw = d.ldo = 1536
        d.out_split = 1
        d.st_acc, d.st_rs, d.st_cg, d.st_G, d.st_coff, d.st_hw = 0x1000, 128, 16, 32, 0, hw
        return vc.plan_of(d)[0]

    assert status(720, 720) == 0 and status(900, 900) == 0 and status(1152, 576) == 0
    assert status(1440, 720) != 0  # two images of 720 pixels: a tile would straddle them
    assert b"hw % 64" in _lib.lib().tair_last_error()


def test_hip_encoder_names_a_tile_box_off_multiples_of_8(vaes):
    from tair_amd.vae_hip import HipVAEEncoder
    _, prod = vaes
    enc = HipVAEEncoder(prod, "cpu", max_batch=1)
    with pytest.raises(ValueError, match=r"x 0:84"):  # 104 wide at tile 20: boxes [0, 84] and [20, 104]
        enc.encode_mode_tiled(torch.zeros(1, 3, 104, 104), 20)


# ------------------------------------------------------------------------------------------ pipeline
class _RecordingCldm:
    """Stands in for ControlLDM: records how apply_cldm calls the VAE entry points."""
    vae_tiling = True

    def __init__(self, latent_hw=(64, 64)):
        self.latent_hw, self.control_scales, self.calls = latent_hw, [1.0] * 13, []

    def prepare_condition(self, cond_img, txt=None, c_txt=None, tiled=False, tile_size=-1):
        self.calls.append(("prepare_condition", tuple(cond_img.shape[2:]), tiled, tile_size))
        return dict(c_txt=c_txt, c_img=torch.zeros(cond_img.shape[0], 4, cond_img.shape[2] // 8, cond_img.shape[3] // 8))

    def vae_decode(self, z, tiled=False, tile_size=-1):
        self.calls.append(("vae_decode", tuple(z.shape[2:]), tiled, tile_size))
        return torch.zeros(z.shape[0], 3, 8 * z.shape[2], 8 * z.shape[3])


def _apply(cldm, img, monkeypatch, **kw):
    from tair_amd import sampler
    from tair_amd.diffusion import Diffusion
    from tair_amd.pipeline import Pipeline
    monkeypatch.setattr(sampler.SpacedSampler, "sample", lambda self, **k: (torch.zeros(k["x_size"]), None))
    d = Diffusion(linear_start=0.00085, linear_end=0.012, zero_snr=True, parameterization="v")
    pipe = Pipeline(None, cldm, d, None, "cpu", text_encoder=lambda p: torch.zeros(len(p), 77, 1024))
    a = dict(steps=2, strength=1.0, vae_encoder_tiled=True, vae_encoder_tile_size=512, vae_decoder_tiled=True,
             vae_decoder_tile_size=512, cldm_tiled=True, cldm_tile_size=512, cldm_tile_stride=256, pos_prompt="a",
             neg_prompt="b", cfg_scale=1.0, start_point_type="noise", sampler_type="spaced", noise_aug=0,
             rescale_cfg=False)
    a.update(kw)
    return pipe.apply_cldm(img, **a)


def test_pipeline_passes_the_tile_sizes_as_the_reference_does(monkeypatch):
    c = _RecordingCldm()
    out = _apply(c, torch.zeros(1, 3, 1021, 1024), monkeypatch)  # padded to 8: 1024 x 1024
    assert out.shape == (1, 3, 1021, 1024)
    assert c.calls == [("prepare_condition", (1024, 1024), True, 512), ("vae_decode", (128, 128), True, 64)]
    assert c.control_scales == [1.0] * 13
    # classifier-free guidance off the latent-tiled path: both conditions are encoded with the same flags
    c = _RecordingCldm()
    _apply(c, torch.zeros(1, 3, 512, 512), monkeypatch, cldm_tiled=False, cfg_scale=4.0, vae_encoder_tile_size=256,
           vae_decoder_tile_size=256)
    assert c.calls == [("prepare_condition", (512, 512), True, 256)] * 2 + [("vae_decode", (64, 64), True, 32)]


def test_pipeline_runs_untiled_below_the_tile_size(monkeypatch):
    c = _RecordingCldm()
    _apply(c, torch.zeros(1, 3, 512, 768), monkeypatch, vae_encoder_tile_size=1024, vae_decoder_tile_size=1024)
    assert c.calls == [("prepare_condition", (512, 768), False, 1024), ("vae_decode", (64, 96), False, 128)]
    c = _RecordingCldm()  # one side below is enough (pipeline.py:106-111, 220-224)
    _apply(c, torch.zeros(1, 3, 512, 768), monkeypatch, vae_encoder_tile_size=640, vae_decoder_tile_size=640)
    assert [x[2] for x in c.calls] == [False, False]
    c = _RecordingCldm()  # only the decoder tiled: the encoder flag stays off
    _apply(c, torch.zeros(1, 3, 512, 768), monkeypatch, vae_encoder_tiled=False)
    assert c.calls == [("prepare_condition", (512, 768), False, 512), ("vae_decode", (64, 96), True, 64)]


def test_pipeline_rejects_an_encoder_tile_size_off_multiples_of_8(monkeypatch):
    with pytest.raises(ValueError, match="multiple of 8"):
        _apply(_RecordingCldm(), torch.zeros(1, 3, 512, 768), monkeypatch, vae_encoder_tile_size=500)
    # a handle without the tiled VAE keeps refusing, with the text it always had
    stub = types.SimpleNamespace(latent_hw=(64, 64), control_scales=[1.0] * 13)
    with pytest.raises(NotImplementedError, match="tiled VAE is out of scope"):
        _apply(stub, torch.zeros(1, 3, 512, 768), monkeypatch)


def test_control_ldm_advertises_the_tiled_vae():
    from tair_amd.cldm import ControlLDM
    assert ControlLDM.vae_tiling is True
