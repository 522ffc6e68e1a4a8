"""The grouped launchers other than the GEMM with two lanes in one launch: attention_grouped, layernorm_grouped,
groupnorm_stats_grouped and groupnorm_apply_grouped (tair_k_attention_grouped, tair_k_layernorm_grouped,
tair_k_groupnorm_grouped, tair_k_gn_apply_stats_grouped).

* Attention (tests/_exact_cases.py GROUP_ATTN_CASES: Sq 17 / 65 / 129, Skv 77 / 130 / 257, B H of 2 .. 4, 16 and 32
  queries per wave, the "rows" layout and one shared context with kv_bstride = 0): one-hot scores, each lane with
  target sets, Hadamard rows and V of its own, so each lane's output row must be ITS V[target], bit for bit --
  unsplit, split with the merge kernel (lane = blockIdx.y), split with tickets (lane from blockIdx.z / splits).  Each
  lane has its own workspace and tickets; the tickets are back at zero; a ticketed launch runs twice.
* layernorm_grouped (T 1 / 5 / 77, C 320 / 1280; bf16 and e4m3 outputs) and the GroupNorm pair ((B, HW, C, G) =
  (1, 64, 320, 32), (2, 16, 640, 32), (3, 64, 128, 32); statistics with tickets in one launch and without in two, then
  the apply from scale / shift; the apply from producer statistics with a hi + lo input, three-plane output and the
  e4m3 form): lanes differ in x, gamma and beta.  These kernels are order-deterministic, so both lanes must be
  bitwise equal to the same lane launched alone through the single entry points, which the earlier suites gate
  against references.  Guard rows and padding stay intact.
* Group sizes 0 and 3 are refused by every grouped entry, nothing written.

Measured on MI355X: all 27 attention cases exact in both lanes; the 18 LayerNorm, 12 + 15 GroupNorm cases bitwise
equal to the lane alone; both group sizes refused (74 tests); the module runs in about 2 s.  The planted GEMM lane
defects of tests/test_grouped_exact_gpu.py's docstring do not reach these kernels: 0 of the 74 fail under them.
"""
import ctypes

import pytest
import torch

import _exact_cases as ec

pytestmark = pytest.mark.gpu

ATTN_PARAMS = ec.GROUP_ATTN_CASES
DEV = "cuda"
SENTINEL = 768.0
NAN = float("nan")
TICKETS = 16384


def _L():
    from tair_amd import _lib
    return _lib.lib(), _lib


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _helpers():
    from test_clip_hip_gpu import _guarded, _guards_intact
    return _guarded, _guards_intact


def _p(t):
    return t.data_ptr() if t is not None else None


# ---- attention ------------------------------------------------------------------------------------------------------------
_WS = {}


def _attn_ws(lane):
    if lane not in _WS:
        _WS[lane] = (torch.empty(8 << 20, dtype=torch.uint8, device=DEV),
                     torch.zeros(TICKETS, dtype=torch.int32, device=DEV))
    return _WS[lane]


class AttnLaneBufs:
    def __init__(self, c, o: ec.AttnOps):
        guarded, _ = _helpers()
        B, H, Sq, Skv = c.B, c.H, c.Sq, c.Skv
        C = H * 64
        self.qb, self.q = guarded(B * Sq, C, NAN)
        self.kb, self.k = guarded(o.Bk * Skv, C, NAN)
        self.vb, self.v = guarded(o.Bk * Skv, C, NAN)
        self.q.copy_(o.q.reshape(B * Sq, C).to(DEV))
        self.k.copy_(o.k.reshape(-1, C).to(DEV))
        self.v.copy_(o.v.reshape(-1, C).to(DEV))
        self.ob, self.o = guarded(B * Sq, C, SENTINEL)
        self.want = o.expected().to(torch.bfloat16)
        self.tgt = o.tgt


@pytest.mark.parametrize("case", ATTN_PARAMS, ids=repr)
def test_grouped_attention_selection(case):
    L, lib = _L()
    _, guards_intact = _helpers()
    c = case
    B, H, Sq, Skv = c.B, c.H, c.Sq, c.Skv
    rc, plan = ec.attn_plan_of(ec.AttnCase(c.name, B, H, Sq, Skv, "ex", c.force, c.ws_bytes, c.expect, c.layout))
    assert rc == 0 and plan == c.expect, (plan, c.expect)
    ops = [ec.AttnOps(c, lane=i) for i in range(2)]
    assert (c.layout == "shared") == (ops[0].Bk == 1 and B > 1)
    bufs = [AttnLaneBufs(c, o) for o in ops]
    ws_bytes = ec.attn_per_split(B, H, Sq) * plan[1] if plan[1] > 1 else 0
    lanes = (lib.AttnLane * 2)()
    for i, b in enumerate(bufs):
        ws, tk = _attn_ws(i)
        assert ws_bytes + 65536 <= ws.numel()
        ws[ws_bytes:ws_bytes + 65536].fill_(0xA5)
        ln = lanes[i]
        ln.q, ln.ldq, ln.k, ln.ldk, ln.v, ln.ldv = _p(b.q), b.q.stride(0), _p(b.k), b.k.stride(0), _p(b.v), b.v.stride(0)
        ln.o, ln.ldo, ln.kv_bstride = _p(b.o), b.o.stride(0), 0 if c.layout == "shared" else Skv
        if plan[1] > 1:
            ln.ws, ln.ws_bytes = _p(ws), ws_bytes
        if c.api == "tk":
            ln.tickets, ln.tickets_cap = _p(tk), TICKETS
    runs = []
    for _ in range(2 if c.api == "tk" else 1):
        for b in bufs:
            b.o.fill_(SENTINEL)
        rc = L.tair_k_attention_grouped(lanes, 2, B, H, Sq, Skv, 0.125, c.force[0], c.force[1], _stream())
        assert rc == 0, L.tair_last_error()
        torch.cuda.synchronize()
        for i in range(2):
            assert int(_attn_ws(i)[1].count_nonzero()) == 0, f"lane {i}: attention tickets not left zeroed"
        runs.append([b.o.clone() for b in bufs])
    for i, b in enumerate(bufs):
        got = runs[0][i].view(B, Sq, H, 64).cpu()
        ok = got.view(torch.int16) == b.want.view(torch.int16)
        if not bool(ok.all()):
            rows = (~ok).any(-1).nonzero()[:6].tolist()
            other = (got.view(torch.int16) == bufs[1 - i].want.view(torch.int16)).all(-1)
            desc = ", ".join(f"(b {bb}, query {q}, head {h}: target key {int(b.tgt[bb, h, q])})" for bb, q, h in rows)
            raise AssertionError(f"{c.name} lane {i} plan {plan}: {int((~ok).any(-1).sum())} of {ok[..., 0].numel()} rows "
                                 f"differ from the lane's V[target] ({int((other & (~ok).any(-1)).sum())} of them are the "
                                 f"OTHER lane's rows); first {desc}")
        assert guards_intact(b.ob, b.o, SENTINEL), f"lane {i}: output guard rows / padding columns written"
        assert bool((_attn_ws(i)[0][ws_bytes:ws_bytes + 65536] == 0xA5).all()), f"lane {i}: workspace written past ws_bytes"
        if len(runs) > 1:
            assert torch.equal(runs[0][i].view(torch.int16), runs[1][i].view(torch.int16)), \
                f"lane {i}: second launch on the tickets differs"


# ---- layernorm_grouped ------------------------------------------------------------------------------------------------------
def _ln_lane(T, C, lane):
    g = torch.Generator(device=DEV).manual_seed(1000 * T + C + lane)
    x = (torch.randn(T, C, device=DEV, generator=g) * (3 - lane) + 0.5 - 2 * lane).to(torch.bfloat16)
    gamma = torch.randn(C, device=DEV, generator=g) * 0.5 + 1
    beta = torch.randn(C, device=DEV, generator=g) * 0.2
    return x, gamma, beta


@pytest.mark.parametrize("C", (320, 1280))
@pytest.mark.parametrize("T", (1, 5, 77))
@pytest.mark.parametrize("form", ("bf16", "e4m3", "mixed"))
def test_grouped_layernorm_equals_alone(T, C, form):
    """Both lanes bitwise equal to the lane alone; `mixed`: lane 0 writes bf16, lane 1 e4m3 (the form is per lane)."""
    L, lib = _L()
    guarded, guards_intact = _helpers()
    ld8 = (C + 127) // 128 * 128 + 128
    f8 = [form == "e4m3", form != "bf16"]
    ins = [_ln_lane(T, C, i) for i in range(2)]

    def outputs():
        out = []
        for i in range(2):
            if f8[i]:
                buf = torch.full((T + 16, ld8), 0x55, dtype=torch.uint8, device=DEV)
                out.append((buf, buf[8:8 + T], torch.full((T + 16,), SENTINEL, device=DEV)))
            else:
                buf, view = guarded(T, C, SENTINEL, torch.bfloat16, 0)
                out.append((buf, view, None))
        return out

    alone = outputs()
    for i, (x, gamma, beta) in enumerate(ins):
        buf, view, s8 = alone[i]
        if f8[i]:
            rc = L.tair_k_layernorm_fp8(_p(x), T, C, _p(gamma), _p(beta), 1e-5, _p(view), ld8, _p(s8[8:]), _stream())
        else:
            rc = L.tair_k_layernorm(_p(x), T, C, _p(gamma), _p(beta), 1e-5, _p(view), _stream())
        assert rc == 0, L.tair_last_error()
    grouped = outputs()
    lanes = (lib.LnLane * 2)()
    for i, (x, gamma, beta) in enumerate(ins):
        buf, view, s8 = grouped[i]
        lanes[i].x, lanes[i].gamma, lanes[i].beta = _p(x), _p(gamma), _p(beta)
        if f8[i]:
            lanes[i].y8, lanes[i].s8, lanes[i].ld8 = _p(view), _p(s8[8:]), ld8
        else:
            lanes[i].y = _p(view)
    assert L.tair_k_layernorm_grouped(lanes, 2, T, C, 1e-5, _stream()) == 0, L.tair_last_error()
    torch.cuda.synchronize()
    for i in range(2):
        (ab, av, as8), (gb, gv, gs8) = alone[i], grouped[i]
        assert torch.equal(ab.view(torch.uint8 if f8[i] else torch.int16), gb.view(torch.uint8 if f8[i] else torch.int16)), \
            f"lane {i}: {int((av != gv).sum())} elements differ from the lane alone"
        if f8[i]:
            assert torch.equal(as8.view(torch.int32), gs8.view(torch.int32)), f"lane {i}: row scales differ"
            assert bool((gb[:8] == 0x55).all()) and bool((gb[8 + T:] == 0x55).all()), f"lane {i}: guard rows written"
            assert bool((gs8[:8] == SENTINEL).all()) and bool((gs8[8 + T:] == SENTINEL).all())
            assert bool((gv[:, C:] == 0).all()), "bytes C .. ld8 not zeroed"
            assert bool((gv[:, :C] != 0x55).any())
        else:
            assert guards_intact(gb, gv, SENTINEL), f"lane {i}: guard rows written"
            assert bool((gv != SENTINEL).any())
    if f8[0] == f8[1]:
        assert not torch.equal(grouped[0][1], grouped[1][1])


# ---- groupnorm_stats_grouped / groupnorm_apply_grouped ------------------------------------------------------------------------
GN_SHAPES = [(1, 64, 320, 32), (2, 16, 640, 32), (3, 64, 128, 32)]


def _gn_lane(B, HW, C, lane, planes=1):
    """x [B HW, ldx] (ldx = planes * C + 64: padding columns of NaN), gamma, beta; planes = 3: (hi, lo, hi)."""
    g = torch.Generator(device=DEV).manual_seed(B * 1000 + HW + C + 7 * lane)
    xf = torch.randn(B * HW, C, device=DEV, generator=g) * (2 - lane) + 3 - 5 * lane
    hi = xf.to(torch.bfloat16)
    x = torch.full((B * HW + 16, planes * C + 64), NAN, dtype=torch.bfloat16, device=DEV)
    xv = x[8:8 + B * HW]
    xv[:, :C] = hi
    if planes == 3:
        lo = (xf - hi.float()).to(torch.bfloat16)
        xv[:, C:2 * C], xv[:, 2 * C:3 * C] = lo, hi
    gamma = torch.rand(C, device=DEV, generator=g) + 0.5
    beta = torch.randn(C, device=DEV, generator=g)
    val = hi.double() + (lo.double() if planes == 3 else 0)
    return x, xv, gamma, beta, val


@pytest.mark.parametrize("B,HW,C,G", GN_SHAPES, ids=lambda v: str(v))
@pytest.mark.parametrize("fused", (True, False), ids=("tickets", "two-launch"))
@pytest.mark.parametrize("silu", (0, 1))
def test_grouped_groupnorm_equals_alone(B, HW, C, G, fused, silu):
    L, lib = _L()
    guarded, guards_intact = _helpers()
    eps = 1e-5
    ins = [_gn_lane(B, HW, C, i) for i in range(2)]

    def bufs():
        out = []
        for _ in range(2):
            yb, y = guarded(B * HW, C, SENTINEL)
            out.append(dict(yb=yb, y=y, ss=torch.full((B * C * 2 + 64,), SENTINEL, device=DEV),
                            ws=torch.full((B * G * 64 * 2 + 64,), NAN, device=DEV),
                            tk=torch.zeros(B * G, dtype=torch.int32, device=DEV)))
        return out

    alone, grouped = bufs(), bufs()
    for i, (x, xv, gamma, beta, _) in enumerate(ins):
        b = alone[i]
        rc = L.tair_k_groupnorm_ex(_p(xv), xv.stride(0), B, HW, C, G, eps, _p(gamma), _p(beta), silu, _p(b["y"]),
                                   b["y"].stride(0), _p(b["ss"]), _p(b["ws"]), _p(b["tk"]) if fused else None, _stream())
        assert rc == 0, L.tair_last_error()
    lanes = (lib.GnLane * 2)()
    for i, (x, xv, gamma, beta, _) in enumerate(ins):
        b, ln = grouped[i], lanes[i]
        ln.x, ln.ldx, ln.gamma, ln.beta, ln.ss, ln.ws = _p(xv), xv.stride(0), _p(gamma), _p(beta), _p(b["ss"]), _p(b["ws"])
        ln.tickets = _p(b["tk"]) if fused else None
        ln.y, ln.ldy = _p(b["y"]), b["y"].stride(0)
    for _ in range(2 if fused else 1):  # tickets reset themselves: the second launch gives the same
        assert L.tair_k_groupnorm_grouped(lanes, 2, B, HW, C, G, eps, silu, _stream()) == 0, L.tair_last_error()
    torch.cuda.synchronize()
    for i in range(2):
        a, g = alone[i], grouped[i]
        assert int(g["tk"].count_nonzero()) == 0, f"lane {i}: tickets not back at zero"
        assert torch.equal(a["ss"].view(torch.int32), g["ss"].view(torch.int32)), f"lane {i}: scale / shift differ from the lane alone"
        assert bool((g["ss"][B * C * 2:] == SENTINEL).all()) and bool((g["ss"][:B * C * 2] != SENTINEL).any())
        assert torch.equal(a["yb"].view(torch.int16), g["yb"].view(torch.int16)), \
            f"lane {i}: {int((a['y'] != g['y']).sum())} output elements differ from the lane alone"
        assert guards_intact(g["yb"], g["y"], SENTINEL) and bool((g["y"] != SENTINEL).any())
    assert not torch.equal(grouped[0]["y"], grouped[1]["y"])


def _prod_stats(val, B, HW, C, G, lane):
    """Producer statistics of the values val in the epilogues' layout, spread over two replicas (others per lane)."""
    gr = val.view(B, HW, G, C // G)
    s = torch.stack([gr.sum(dim=(1, 3)), (gr * gr).sum(dim=(1, 3))], -1).flatten()
    rs = B * G * 2 + 8 * lane
    st = torch.zeros(8, rs, device=DEV, dtype=torch.float64)
    st[1 + lane, :B * G * 2] = s * 0.25
    st[6 - lane, :B * G * 2] = s * 0.75
    return st, rs


@pytest.mark.parametrize("B,HW,C,G", GN_SHAPES, ids=lambda v: str(v))
@pytest.mark.parametrize("form", ("plain", "x_lo", "x_lo+y_split", "y8", "x_lo+y8"))
def test_grouped_groupnorm_apply_from_statistics_equals_alone(B, HW, C, G, form):
    L, lib = _L()
    guarded, guards_intact = _helpers()
    eps, silu = 1e-6, 1
    x_lo, y_split, y8 = "x_lo" in form, "y_split" in form, "y8" in form
    ld8 = (C + 127) // 128 * 128
    ins = [_gn_lane(B, HW, C, i, 3 if x_lo else 1) for i in range(2)]
    stats = [_prod_stats(ins[i][4], B, HW, C, G, i) for i in range(2)]
    inv8 = [torch.full((C,), 0.25 * (i + 1), device=DEV) for i in range(2)]

    def bufs():
        out = []
        for _ in range(2):
            if y8:
                buf = torch.full((B * HW + 16, ld8), 0x55, dtype=torch.uint8, device=DEV)
                out.append((buf, buf[8:8 + B * HW]))
            else:
                out.append(guarded(B * HW, 3 * C if y_split else C, SENTINEL))
        return out

    alone, grouped = bufs(), bufs()
    for i, (x, xv, gamma, beta, _) in enumerate(ins):
        st, rs = stats[i]
        buf, y = alone[i]
        if y8:
            rc = L.tair_k_gn_apply_fp8(_p(xv), xv.stride(0), C if x_lo else 0, B, HW, C, G, eps, _p(gamma), _p(beta), silu,
                                       _p(st), rs, _p(inv8[i]), _p(y), ld8, _stream())
        else:
            rc = L.tair_k_gn_apply_stats(_p(xv), xv.stride(0), C if x_lo else 0, B, HW, C, G, eps, _p(gamma), _p(beta),
                                         silu, _p(st), rs, _p(y), y.stride(0), int(y_split), _stream())
        assert rc == 0, L.tair_last_error()
    lanes = (lib.GnLane * 2)()
    for i, (x, xv, gamma, beta, _) in enumerate(ins):
        st, rs = stats[i]
        buf, y = grouped[i]
        ln = lanes[i]
        ln.x, ln.ldx, ln.gamma, ln.beta, ln.st, ln.st_rs = _p(xv), xv.stride(0), _p(gamma), _p(beta), _p(st), rs
        ln.x_lo, ln.y_split = C if x_lo else 0, int(y_split)
        if y8:
            ln.y8, ln.ld8, ln.inv8 = _p(y), ld8, _p(inv8[i])
        else:
            ln.y, ln.ldy = _p(y), y.stride(0)
    assert L.tair_k_gn_apply_stats_grouped(lanes, 2, B, HW, C, G, eps, silu, _stream()) == 0, L.tair_last_error()
    torch.cuda.synchronize()
    it = torch.uint8 if y8 else torch.int16
    for i in range(2):
        (ab, ay), (gb, gy) = alone[i], grouped[i]
        assert torch.equal(ab.view(it), gb.view(it)), f"lane {i}: {int((ay != gy).sum())} elements differ from the lane alone"
        if y8:
            assert bool((gb[:8] == 0x55).all()) and bool((gb[8 + B * HW:] == 0x55).all()), f"lane {i}: guard rows written"
            assert bool((gy[:, C:] == 0).all()) and bool((gy[:, :C] != 0x55).any())
        else:
            assert guards_intact(gb, gy, SENTINEL) and bool((gy != SENTINEL).any())
    assert not torch.equal(grouped[0][1], grouped[1][1])


# ---- group sizes 0 and 3 -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", (0, 3))
def test_group_sizes_outside_one_and_two_are_refused(n):
    """Every grouped entry refuses n = 0 and n = 3 (-2 with a message) and writes nothing: the outputs keep their
    sentinel.  The lane arrays hold three well-formed lanes."""
    L, lib = _L()
    T = C = 64
    x = torch.randn(3, T, C, device=DEV).to(torch.bfloat16)
    w = torch.randn(3, C, C, device=DEV).to(torch.bfloat16)
    f32 = torch.ones(3, 4 * C, device=DEV)
    out = torch.full((3, T, C), SENTINEL, dtype=torch.bfloat16, device=DEV)
    out32 = torch.full((3, 4096), SENTINEL, device=DEV)
    st = torch.ones(3, 8, 64, dtype=torch.float64, device=DEV)

    def refused(rc, what):
        assert rc == -2 and b"group of" in (L.tair_last_error() or b""), (what, rc, L.tair_last_error())

    gd = (lib.GemmDesc * 3)()
    for i in range(3):
        d = ec.make_desc(M=T, N=C, K=C, amode=0, A=_p(x[i]), lda=C, Wt=_p(w[i]), ldw=C, out=_p(out[i]), ldo=C)
        ctypes.memmove(ctypes.byref(gd[i]), ctypes.byref(d), ctypes.sizeof(lib.GemmDesc))
    refused(L.tair_k_gemm_grouped(gd, n, _stream()), "gemm")
    refused(L.tair_k_gemm_grouped_check(gd, n), "gemm check")
    al = (lib.AttnLane * 3)()
    for i in range(3):
        al[i].q, al[i].k, al[i].v, al[i].o = _p(x[i]), _p(x[i]), _p(x[i]), _p(out[i])
        al[i].ldq = al[i].ldk = al[i].ldv = al[i].ldo = C
        al[i].kv_bstride = T
    refused(L.tair_k_attention_grouped(al, n, 1, 1, T, T, 0.125, 0, 0, _stream()), "attention")
    ll = (lib.LnLane * 3)()
    for i in range(3):
        ll[i].x, ll[i].gamma, ll[i].beta, ll[i].y = _p(x[i]), _p(f32[i]), _p(f32[i]), _p(out[i])
    refused(L.tair_k_layernorm_grouped(ll, n, T, C, 1e-5, _stream()), "layernorm")
    gl = (lib.GnLane * 3)()
    for i in range(3):
        gl[i].x, gl[i].ldx, gl[i].gamma, gl[i].beta, gl[i].y, gl[i].ldy = _p(x[i]), C, _p(f32[i]), _p(f32[i]), _p(out[i]), C
        gl[i].ss, gl[i].ws, gl[i].st, gl[i].st_rs = _p(out32[i]), _p(out32[i, 1024:]), _p(st[i]), 64
    refused(L.tair_k_groupnorm_grouped(gl, n, 1, T, C, 8, 1e-5, 0, _stream()), "groupnorm")
    refused(L.tair_k_gn_apply_stats_grouped(gl, n, 1, T, C, 8, 1e-5, 0, _stream()), "groupnorm apply")
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all()) and bool((out32 == SENTINEL).all())
