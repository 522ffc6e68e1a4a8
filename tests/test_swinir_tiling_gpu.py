"""The tiled cleaner on the GPU: the two image-tile kernels through the C ABI (csrc/image_tile.hip), HipSwinIR.forward_tiled
on the reduced network, its graph replay, and SwinIRPipeline.apply_cleaner(tiled=True).

Operands sit in guarded buffers as in test_swinir_hip_gpu.py: inputs are surrounded by NaN (a read outside the operand
poisons the result), outputs by a sentinel that must survive; the accumulators start as NaN (the first chunk must not
read them).

Gates (none is derived from what the code gives):
* gather: bitwise the torch expression HipSwinIR.forward prepares its input with, on each window;
* blend: bitwise the reference loop (tests/_swinir_tiled_ref.py) in fp32 on the CPU, for every chunking;
* forward_tiled: bitwise a host loop that runs ``hip()`` on the same chunk batches and blends on the CPU with the
  reference loop; against the oracle tiled by the same loop, rel-L2(HIP, oracle) <= 1.5 x rel-L2(emulation, oracle),
  the gate test_swinir_hip_gpu.py derives for the untiled network (the blend is a convex combination of window
  outputs, the same for all three, so it adds nothing to the ratio).

The kernel geometry is B = 2, 100 x 75, tile 64, stride 48: window starts 0, 36 x 0, 11 (neither flush start is a
multiple of 8), T = 4, 8 job rows.  In chunks of 3 that is three calls, the third with one pad row.
"""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from tests._swinir_emul import emulate
from tests._swinir_tiled_ref import blend_rows_ref, cover_counts, job_rows, tiled_ref, weights32
from tests.test_swinir_hip_gpu import REDUCED, _guarded, _guards_intact, _L, _models, _p, _stream, rel
from tests.test_swinir_tiling_cpu import BLEND_BAD, BLEND_OK, GATHER_BAD, GATHER_OK, call_blend, call_gather

pytestmark = pytest.mark.gpu

NAN = float("nan")
GEO = dict(B=2, H=100, W=75, tile=64, stride=48)
CP = 192


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _flat_guarded(shape, fill, guard=4096):
    """A contiguous tensor of `shape` with `guard` elements of `fill` before and after it."""
    n = 1
    for s in shape:
        n *= s
    buf = torch.full((n + 2 * guard,), fill, device="cuda", dtype=torch.float32)
    return buf, buf[guard:guard + n].view(shape)


def _flat_intact(buf, view, fill):
    g = (buf.numel() - view.numel()) // 2
    return bool((buf[:g] == fill).all()) and bool((buf[g + view.numel():] == fill).all())


# ------------------------------------------------------------------------------------------- gather
@pytest.mark.parametrize("chunks", [[(0, 3), (3, 3), (6, 3)], [(0, 4), (4, 5)], [(0, 8)], [(7, 2)]],
                         ids=["3+3+3", "4+5", "8", "last+pad"])
def test_gather_is_the_torch_expression(chunks):
    L = _L()
    B, H, W, S, stride = (GEO[k] for k in ("B", "H", "W", "tile", "stride"))
    g = torch.Generator(device="cuda").manual_seed(21)
    _, x = _flat_guarded((B, 3, H, W), NAN)
    x.copy_(torch.rand((B, 3, H, W), device="cuda", generator=g))
    _, mean = _flat_guarded((3,), NAN, guard=64)
    mean.copy_(torch.tensor([0.4488, 0.4371, 0.4040]))
    rows_of = job_rows(B, H, W, S, stride)
    assert [w[0] for _, w in rows_of[:4]] == [0, 0, 36, 36] and [w[2] for _, w in rows_of[:4]] == [0, 11, 0, 11]
    tt = (S // 8) ** 2
    lo_off, cols = 200, 400  # the planes at [0, 192) and [200, 392): the columns between and after them stay as they are
    for first, rows in chunks:
        obuf, out = _guarded(rows * tt, cols, 7.0)
        rc = L.tair_k_image_tile_gather(_p(x), _p(mean), B, H, W, S, stride, first, rows, _p(out), out.stride(0), lo_off,
                                        _stream())
        assert rc == 0, L.tair_last_error()
        torch.cuda.synchronize()
        for r in range(rows):
            b, (y0, y1, x0, x1) = rows_of[min(first + r, len(rows_of) - 1)]  # a pad row holds the job's last window
            u = F.pixel_unshuffle(x[b:b + 1, :, y0:y1, x0:x1] - mean.view(1, 3, 1, 1), 8).permute(0, 2, 3, 1).reshape(tt, CP)
            hi = u.to(torch.bfloat16)
            lo = (u - hi.float()).to(torch.bfloat16)
            got = out[r * tt:(r + 1) * tt]
            assert torch.equal(_bits(got[:, :CP]), _bits(hi)), (first, r)
            assert torch.equal(_bits(got[:, lo_off:lo_off + CP]), _bits(lo)), (first, r)
        assert bool((out[:, CP:lo_off] == 7.0).all()) and bool((out[:, lo_off + CP:] == 7.0).all())
        assert _guards_intact(obuf, out, 7.0)


# -------------------------------------------------------------------------------------------- blend
def _blend_run(V, w, chunks, B, H, W, S, stride):
    """The kernel over `chunks` [(first, rows)] of the job outputs V [N, S * S, 3]; pad rows of a chunk are NaN."""
    L = _L()
    abuf, acc = _flat_guarded((B, 3, H, W), NAN)
    cbuf, cnt = _flat_guarded((B, 3, H, W), NAN)
    obuf, out = _flat_guarded((B, 3, H, W), 7.0)
    N = V.shape[0]
    for i, (first, rows) in enumerate(chunks):
        vbuf, v = _flat_guarded((rows * S * S, 3), NAN)
        n = min(rows, N - first)
        v[:n * S * S] = V[first:first + n].reshape(n * S * S, 3)
        rc = L.tair_k_image_tile_blend(_p(v), _p(w), _p(acc), _p(cnt), _p(out), B, H, W, S, stride, first, rows,
                                       int(i == len(chunks) - 1), _stream())
        assert rc == 0, L.tair_last_error()
        torch.cuda.synchronize()
    assert bool((abuf[:4096] != abuf[:4096]).all()) and bool((cbuf[-4096:] != cbuf[-4096:]).all())  # NaN guards
    assert _flat_intact(obuf, out, 7.0)
    return out.clone()


def test_blend_is_the_reference_loop_for_every_chunking():
    B, H, W, S, stride = (GEO[k] for k in ("B", "H", "W", "tile", "stride"))
    cover = cover_counts(H, W, S, stride)
    assert {1, 2, 4} <= set(cover.unique().tolist())  # pixels under one, two and four windows
    N = B * 4
    V = torch.randn((N, S * S, 3), generator=torch.Generator().manual_seed(22))
    w = weights32(S)
    want = blend_rows_ref([V[j].reshape(S, S, 3).permute(2, 0, 1) for j in range(N)], B, H, W, S, stride)
    Vd, wd = V.cuda(), w.cuda().contiguous()
    outs = {}
    for name, chunks in [("one chunk", [(0, 8)]), ("two chunks", [(0, 4), (4, 4)]),
                         ("one window a chunk", [(j, 1) for j in range(N)]),
                         ("chunks of 3, one pad row", [(0, 3), (3, 3), (6, 3)])]:
        outs[name] = _blend_run(Vd, wd, chunks, B, H, W, S, stride).cpu()
        assert bool(torch.isfinite(outs[name]).all()), name  # no NaN of a pad row or of the accumulators' start
        assert torch.equal(_bits(outs[name]), _bits(want)), name
    single = (cover == 1)[None, None].expand(B, 3, H, W)  # under one window: fl(fl(v w) / w), not v itself
    k0 = V[0].reshape(S, S, 3).permute(2, 0, 1)
    top = single[0, :, :S, :S]
    assert torch.equal(outs["one chunk"][0, :, :S, :S][top], ((k0 * w) / w)[top])


# --------------------------------------------------------------------------------- argument refusal
def test_bad_arguments_launch_nothing():
    L = _L()
    B, H, W, S = GEO["B"], GEO["H"], GEO["W"], GEO["tile"]
    x = torch.rand((B, 3, H, W), device="cuda")
    mean = torch.zeros(3, device="cuda")
    tin = torch.full((3 * 64, 2 * CP), 7.0, device="cuda", dtype=torch.bfloat16)
    real = dict(x=x.data_ptr(), mean=mean.data_ptr(), out=tin.data_ptr())
    for bad in GATHER_BAD:
        a = dict(GATHER_OK, **real)
        a.update(bad)
        assert call_gather(L, a, _stream()) == -1 and b"image_tile_gather" in L.tair_last_error(), bad
    v = torch.rand((3 * S * S, 3), device="cuda")
    w = torch.ones(S * S, device="cuda")
    acc, cnt, out = (torch.full((B, 3, H, W), 7.0, device="cuda") for _ in range(3))
    real = dict(v=v.data_ptr(), w=w.data_ptr(), acc=acc.data_ptr(), cnt=cnt.data_ptr(), out=out.data_ptr())
    for bad in BLEND_BAD:
        a = dict(BLEND_OK, **real)
        a.update(bad)
        assert call_blend(L, a, _stream()) == -1 and b"image_tile_blend" in L.tair_last_error(), bad
    torch.cuda.synchronize()
    assert bool((tin == 7.0).all()) and all(bool((t == 7.0).all()) for t in (acc, cnt, out))  # nothing was launched


# ------------------------------------------------------------------------------------ forward_tiled
TILE, STRIDE = 128, 96


@pytest.fixture(scope="module")
def reduced():
    return _models(REDUCED, 5, 3, (16, 16))


def _host_loop(hip, x, size, stride, rpc):
    """hip() on the chunk batches forward_tiled runs (rows of rpc windows, the last padded with the job's last window),
    then the reference blend on the CPU."""
    B, _, H, W = x.shape
    rows_of = job_rows(B, H, W, size, stride)
    N = len(rows_of)
    outs = []
    for first in range(0, N, rpc):
        idx = [min(first + r, N - 1) for r in range(rpc)]
        batch = torch.stack([x[b, :, y0:y1, x0:x1] for b, (y0, y1, x0, x1) in (rows_of[j] for j in idx)])
        y = hip(batch.contiguous()).cpu()
        outs += [y[r] for r in range(min(rpc, N - first))]
    return blend_rows_ref(outs, B, H, W, size, stride)


def test_forward_tiled_is_the_host_loop_and_matches_the_oracle(reduced):
    from oracle.swinir_ref import swinir_forward_ref
    stock, p, hip = reduced
    x = torch.rand((2, 3, 200, 136), generator=torch.Generator().manual_seed(23))
    got = hip.forward_tiled(x.cuda(), TILE, STRIDE)
    assert got.dtype == torch.float32 and tuple(got.shape) == (2, 3, 200, 136)
    plan = hip.last_tiling
    assert (plan["rows"], plan["n_chunks"], plan["rows_per_chunk"], plan["pad"]) == (8, 3, 3, 1)
    assert plan["windows"] == [(0, 128, 0, 128), (0, 128, 8, 136), (72, 200, 0, 128), (72, 200, 8, 136)]
    assert plan["chunks"] == [(0, 3), (3, 3), (6, 2)]
    assert torch.equal(_bits(got.cpu()), _bits(_host_loop(hip, x.cuda(), TILE, STRIDE, 3)))
    sd = stock.state_dict()
    sdc = {k: v.cuda() for k, v in sd.items()}
    want = tiled_ref(lambda t: swinir_forward_ref(sd, p, t.contiguous()), x, TILE, STRIDE)
    emu = tiled_ref(lambda t: emulate(sdc, p["depths"], t.contiguous()), x.cuda(), TILE, STRIDE)
    e_hip, e_emu = rel(got, want), rel(emu, want)
    print(f"forward_tiled reduced 200x136, tile {TILE}, stride {STRIDE}: HIP {e_hip:.3e}, emulation {e_emu:.3e}, "
          f"ratio {e_hip / e_emu:.2f}")
    assert e_hip <= 1.5 * e_emu, (e_hip, e_emu)
    hip.check_faults()


def test_forward_tiled_graph_replay_is_bitwise_eager_and_stateless(reduced):
    _, _, hip = reduced
    g = torch.Generator().manual_seed(24)
    a, b = (torch.rand((2, 3, 200, 136), generator=g).cuda() for _ in range(2))
    eager_a, eager_b = hip.forward_tiled(a, TILE, STRIDE), hip.forward_tiled(b, TILE, STRIDE)
    assert eager_a.data_ptr() != eager_b.data_ptr() and not torch.equal(eager_a, eager_b)
    xin = a.clone()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        hip.forward_tiled(xin, TILE, STRIDE)  # (warm-up on the side stream: plans and first-use setup outside the capture)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = hip.forward_tiled(xin, TILE, STRIDE)
    outs = []
    for src in (a, b, a):
        xin.copy_(src)
        graph.replay()
        outs.append(out.clone())
    torch.cuda.synchronize()
    assert torch.equal(outs[0], eager_a) and torch.equal(outs[1], eager_b) and torch.equal(outs[2], eager_a)
    hip.check_faults()


def test_forward_tiled_checks_its_input_before_any_launch(reduced):
    _, _, hip = reduced
    torch.cuda.synchronize()
    hip._in.fill_(7.0)
    try:
        for shape, tile, stride in [((1, 3, 512, 512), 256, 128),   # a 32 x 32 token map above max_hw (16, 16)
                                    ((1, 3, 100, 136), 128, 96),    # smaller than the tile
                                    ((1, 3, 200, 136), 96, 96),     # not a multiple of 64
                                    ((1, 3, 200, 136), 128, 0)]:
            with pytest.raises(ValueError):
                hip.forward_tiled(torch.zeros(shape, device="cuda"), tile, stride)
        torch.cuda.synchronize()
        assert bool((hip._in == 7.0).all())  # the gather, the first launch of a call, never ran
    finally:
        hip._in.zero_()


# ----------------------------------------------------------------------------------------- pipeline
@torch.no_grad()
def test_pipeline_serves_both_cleaners_tiled(reduced):
    from tair_amd.pipeline import SwinIRPipeline
    stock, p, hip = reduced
    stock_gpu = stock.cuda()
    try:
        x = torch.rand((1, 3, 512, 520), generator=torch.Generator().manual_seed(25)).cuda()
        got = SwinIRPipeline(hip, None, None, None, "cuda").apply_cleaner(x, True, TILE, STRIDE)
        assert hip.last_tiling["rows"] == 30 and hip.last_tiling["n_chunks"] == 10 and hip.last_tiling["pad"] == 0
        assert torch.equal(got, hip.forward_tiled(x, TILE, STRIDE))  # 512 and above: no resize after cleaning
        want = SwinIRPipeline(stock_gpu, None, None, None, "cuda").apply_cleaner(x, True, TILE, STRIDE)
        assert torch.equal(want, tiled_ref(stock_gpu, x, TILE, STRIDE))
        sdc = stock_gpu.state_dict()
        emu = tiled_ref(lambda t: emulate(sdc, p["depths"], t.contiguous()), x, TILE, STRIDE)
        e_hip, e_emu = rel(got, want), rel(emu, want)
        print(f"apply_cleaner tiled 512x520: HIP vs stock {e_hip:.3e}, emulation {e_emu:.3e}, ratio {e_hip / e_emu:.2f}")
        assert e_hip <= 1.5 * e_emu, (e_hip, e_emu)
        small = torch.rand((1, 3, 200, 136), generator=torch.Generator().manual_seed(26)).cuda()
        out = SwinIRPipeline(hip, None, None, None, "cuda").apply_cleaner(small, True, TILE, STRIDE)
        assert min(out.shape[2:]) == 512  # a short edge below 512 is resized after cleaning
        hip.check_faults()
    finally:
        stock.cpu()
