"""The d = 64 flash attention (tair_k_attention, tair_k_attention_ex with forced 16 / 32 queries per wave and forced key
splits, tair_k_attention_tk with arrival tickets) on inputs that say WHICH keys a query attended to and HOW MANY:
the cases of tests/_exact_cases.py (Sq 1 .. 129, Skv 1 .. 1000, ragged query blocks, key counts below one tile, a
last split of one partial tile, a forced split count above the key tiles, a workspace too small for the forced
count, one context for all batch elements, q / k / v strided out of one fused [T, 3C] buffer), each under the
effective plan that tests/test_exact_cases_cpu.py has shown the library to choose and that is asserted again here.
q, k and v live between NaN guard rows and NaN padding columns, o between sentinel rows and columns that must
survive; with tickets the launch runs twice and the tickets must be back at zero.

* Selection.  One-hot scores (Hadamard keys, _exact_cases.AttnOps): the target's score is 256, every other 0, so
  the output row must be V[target], bit for bit, under every plan.  No ulp is allowed on split plans, from the code
  (tair_amd/csrc/attention.hip): in the target's tile mnew = fl(2048 c) = 2048 c exactly (a power of two times c), so
  p = 2^(fma(2048, c, -mnew)) = 2^0 = 1 = bf16(p) and l = 1 + 0; earlier tiles are rescaled by alpha = 2^(0 - 369) = 0,
  later ones add p = 2^-369 = 0.  The split's row is bf16(V[t] / 1) = V[t]; a split without the target has m = 0, so
  the merge weighs it 2^(0 - 369) l = 0 and the target's split 2^0 * 1: acc = V[t], W = 1, output bf16(V[t]) = V[t].
* Counting.  q = 0: every valid key weighs exactly 1 / Skv; V[j] = the unit vector e_(j mod 64), so output column d is
  count_d / Skv.  Per element against fp64 to relative 2^-7 (two bf16 roundings of 2^-9, partial and final, plus fp32
  noise).  A key dropped, counted twice, or a padded key left unmasked moves a column by >= 1 / (ceil(Skv / 64) + 1)
  >= 1 / 17 at these shapes.
* Per-query rows on random operands (tests/test_kernels_gpu.py test_attention's distribution: q and k scaled by 2):
  the rel-L2 of every (batch, query, head) row against fp64, gated at 2 x the worst row of an fp64 emulation of the
  kernel's rounding points under the case's plan -- P rounded to bf16 before P V (the row sum keeps the unrounded P),
  split partials rounded to bf16, the output rounded to bf16 -- computed from the reference operands alone.  The
  factor 2 covers the accumulation order; a row with a mis-weighted key tile exceeds it by far.

Measured on MI355X: selection exact in all 61 cases; counts within 2.4e-3 relative (gate 7.8e-3), exactly 0 in the
columns without keys; worst kernel row / worst emulation row 0.998 .. 1.000 over the 54 cases with more than one key
(worst rows 1.7e-3 .. 4.0e-3), both 0 in the 7 cases with Skv = 1.  The three tests run in about 3 s.  Sensitivity, on a
scratch build: masking keys >= kend - 1 instead of >= kend fails 141 of these 183 tests (49 selection, 39 counting,
53 rows) and 6 of the 21 attention tests of tests/test_kernels_gpu.py.
"""
import ctypes

import pytest
import torch

import _exact_cases as ec

pytestmark = pytest.mark.gpu

ATTN_PARAMS = ec.ATTN_CASES
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


_WS = {}


def _ws():
    if not _WS:
        _WS["ws"] = torch.empty(ec.WS_BIG + 65536, dtype=torch.uint8, device=DEV)
        _WS["tk"] = torch.zeros(TICKETS, dtype=torch.int32, device=DEV)
    return _WS["ws"], _WS["tk"]


def launch(c: ec.AttnCase, q: torch.Tensor, k: torch.Tensor, v: torch.Tensor) -> torch.Tensor:
    """q [B, Sq, H, 64], k / v [Bk, Skv, H, 64] (Bk = 1: one context for all batch elements) as float tensors of bf16
    values -> o [B, Sq, H, 64] (bf16), after the checks every launch gets."""
    L, _ = _L()
    guarded, guards_intact = _helpers()
    B, H, Sq, Skv = c.B, c.H, c.Sq, c.Skv
    C = H * 64
    rc, plan = ec.attn_plan_of(c)
    assert rc == 0 and plan == c.expect, (plan, c.expect)
    if c.layout == "fused":
        assert Sq == Skv and k.shape[0] == B
        fb, fv = guarded(B * Sq, 3 * C, NAN)
        fv.copy_(torch.cat([q.reshape(B * Sq, C), k.reshape(B * Sq, C), v.reshape(B * Sq, C)], 1).to(DEV))
        qv, kv_, vv = fv[:, :C], fv[:, C:2 * C], fv[:, 2 * C:]
        keep = [fb]
    else:
        qb, qv = guarded(B * Sq, C, NAN)
        kb, kv_ = guarded(k.shape[0] * Skv, C, NAN)
        vb, vv = guarded(k.shape[0] * Skv, C, NAN)
        qv.copy_(q.reshape(B * Sq, C).to(DEV))
        kv_.copy_(k.reshape(-1, C).to(DEV))
        vv.copy_(v.reshape(-1, C).to(DEV))
        keep = [qb, kb, vb]
    bstride = 0 if c.layout == "shared" else Skv
    assert (c.layout == "shared") == (k.shape[0] == 1 and B > 1)
    ob, ov = guarded(B * Sq, C, SENTINEL)
    ws, tk = _ws()
    marker = None
    if c.api != "plain" and c.ws_bytes < ec.WS_BIG:
        marker = ws[c.ws_bytes:c.ws_bytes + 65536]
        marker.fill_(0xA5)
    args = (qv.data_ptr(), qv.stride(0), kv_.data_ptr(), kv_.stride(0), vv.data_ptr(), vv.stride(0), ov.data_ptr(),
            ov.stride(0), B, H, Sq, Skv, bstride, 0.125)
    outs = []
    for _ in range(2 if c.api == "tk" else 1):
        ov.fill_(SENTINEL)
        if c.api == "plain":
            rc = L.tair_k_attention(*args, _stream())
        elif c.api == "ex":
            rc = L.tair_k_attention_ex(*args, ws.data_ptr(), c.ws_bytes, c.force[0], c.force[1], _stream())
        else:
            rc = L.tair_k_attention_tk(*args, ws.data_ptr(), c.ws_bytes, tk.data_ptr(), TICKETS, c.force[0], c.force[1],
                                       _stream())
        assert rc == 0, L.tair_last_error()
        torch.cuda.synchronize()
        assert int(tk.count_nonzero()) == 0, "attention tickets not left zeroed"
        outs.append(ov.clone())
    assert guards_intact(ob, ov, SENTINEL), "output guard rows / padding columns written"
    if marker is not None:
        assert bool((marker == 0xA5).all()), "workspace written past ws_bytes"
    if len(outs) > 1:
        assert torch.equal(outs[0].view(torch.int16), outs[1].view(torch.int16)), "second launch on the tickets differs"
    del keep
    return outs[0].view(B, Sq, H, 64)


@pytest.mark.parametrize("case", ATTN_PARAMS, ids=repr)
def test_selection(case):
    """One-hot scores: the output row is V[target], bit for bit, under every plan (see the module docstring for why
    the merge leaves no last-bit freedom)."""
    o = ec.AttnOps(case)
    got = launch(case, o.q, o.k, o.v).cpu()
    want = o.expected().to(torch.bfloat16)
    ok = got.view(torch.int16) == want.view(torch.int16)
    if not bool(ok.all()):
        rows = (~ok).any(-1).nonzero()[:6].tolist()
        desc = ", ".join(f"(b {b}, query {i}, head {h}: target key {int(o.tgt[b, h, i])})" for b, i, h in rows)
        raise AssertionError(f"{case.name} plan {case.expect}: {int((~ok).any(-1).sum())} of {ok[..., 0].numel()} "
                             f"rows differ from V[target]; first {desc}")


def _rand_bf16(shape, gen, scale=1.0):
    return (torch.randn(shape, generator=gen) * scale).to(torch.bfloat16).float()


def _kv_batches(case):
    return 1 if case.layout == "shared" else case.B


@pytest.mark.parametrize("case", ATTN_PARAMS, ids=repr)
def test_counting(case):
    """q = 0, V[j] = e_(j mod 64): output column d = (number of keys j = d mod 64) / Skv, to relative 2^-7."""
    B, H, Sq, Skv = case.B, case.H, case.Sq, case.Skv
    gen = torch.Generator().manual_seed(Sq * 1009 + Skv)
    q = torch.zeros(B, Sq, H, 64)
    k = _rand_bf16((_kv_batches(case), Skv, H, 64), gen, 2.0)
    v = torch.zeros(_kv_batches(case), Skv, H, 64)
    v[:, torch.arange(Skv), :, torch.arange(Skv) % 64] = 1.0
    got = launch(case, q, k, v).double().cpu()
    count = torch.bincount(torch.arange(Skv) % 64, minlength=64).double()
    want = (count / Skv).expand(B, Sq, H, 64)
    err = (got - want).abs()
    worst = (err / want.clamp_min(1e-300)).max().item() if bool((want > 0).all()) else \
        (err[want > 0] / want[want > 0]).max().item()
    print(f"{case.name}: worst relative deviation of a count {worst:.3e} (gate {2.0 ** -7:.3e})")
    bad = err > 2.0 ** -7 * want  # (a column without keys must be exactly 0)
    if bool(bad.any()):
        b, i, h, d = bad.nonzero()[0].tolist()
        raise AssertionError(f"{case.name} plan {case.expect}: {int(bad.sum())} elements off; first (b {b}, query {i}, "
                             f"head {h}, column {d}): got {got[b, i, h, d].item() * Skv:.4f} keys of {Skv}, want "
                             f"{int(count[d])}")


def _bf(x: torch.Tensor) -> torch.Tensor:
    return x.to(torch.bfloat16).double()


def emulate(q, k, v, splits, kv_split):
    """fp64 attention with the kernel's rounding points under (splits, kv_split): per 64-key tile of a split the
    online softmax with P rounded to bf16 for P V and unrounded in the row sum; a split's partial O / l rounded to
    bf16 when there are several; the merge sum_p w_p O_p / sum_p w_p, w_p = e^(m_p - M) l_p; the output rounded to
    bf16.  q [B, Sq, H, 64], k / v [B, Skv, H, 64] double -> [B, Sq, H, 64] double."""
    s = torch.einsum("bqhd,bkhd->bhqk", q, k) * 0.125
    vt = v.permute(0, 2, 1, 3)  # [B, H, Skv, 64]
    Skv = k.shape[1]
    parts = []
    for p in range(splits):
        kb, ke = p * kv_split, min(Skv, (p + 1) * kv_split)
        m = torch.full(s.shape[:3], float("-inf"), dtype=torch.float64)
        l = torch.zeros(s.shape[:3], dtype=torch.float64)
        O = torch.zeros(*s.shape[:3], 64, dtype=torch.float64)
        for t in range(kb, ke, ec.KT):
            st = s[..., t:min(t + ec.KT, ke)]
            mnew = torch.maximum(m, st.max(-1).values)
            pe = torch.exp(st - mnew[..., None])
            alpha = torch.exp(m - mnew)
            l = l * alpha + pe.sum(-1)
            O = O * alpha[..., None] + _bf(pe) @ vt[:, :, t:min(t + ec.KT, ke)]
            m = mnew
        parts.append((m, l, O / l[..., None]))
    if splits == 1:
        out = _bf(parts[0][2])
    else:
        M = torch.stack([m for m, _, _ in parts]).max(0).values
        W = torch.zeros_like(M)
        acc = torch.zeros_like(parts[0][2])
        for m, l, Op in parts:
            w = torch.exp(m - M) * l
            W = W + w
            acc = acc + w[..., None] * _bf(Op)
        out = _bf(acc / W[..., None])
    return out.permute(0, 2, 1, 3)


def _row_rel(a, ref):
    return (a - ref).norm(dim=-1) / ref.norm(dim=-1)


@pytest.mark.parametrize("case", ATTN_PARAMS, ids=repr)
def test_rows_random(case):
    """Random operands: every (batch, query, head) row's rel-L2 against fp64 <= 2 x the worst row of the emulation."""
    B, H, Sq, Skv = case.B, case.H, case.Sq, case.Skv
    gen = torch.Generator().manual_seed(Sq * 7919 + Skv)
    q = _rand_bf16((B, Sq, H, 64), gen, 2.0)
    k = _rand_bf16((_kv_batches(case), Skv, H, 64), gen, 2.0)
    v = _rand_bf16((_kv_batches(case), Skv, H, 64), gen)
    got = launch(case, q, k, v).double().cpu()
    qd, kd, vd = q.double(), k.double().expand(B, -1, -1, -1), v.double().expand(B, -1, -1, -1)
    s = torch.einsum("bqhd,bkhd->bhqk", qd, kd) * 0.125
    ref = (torch.softmax(s, -1) @ vd.permute(0, 2, 1, 3)).permute(0, 2, 1, 3)
    emu = emulate(qd, kd, vd, case.expect[1], case.expect[2])
    e_emu, e_got = _row_rel(emu, ref), _row_rel(got, ref)
    gate = 2 * e_emu.max().item()
    worst = e_got.max().item()
    print(f"{case.name}: worst row {worst:.3e}, worst emulation row {e_emu.max().item():.3e}, ratio "
          f"{worst / max(e_emu.max().item(), 1e-300):.3f} (gate 2)")
    assert bool(torch.isfinite(got).all())
    bad = e_got > gate
    if bool(bad.any()):
        b, i, h = bad.nonzero()[0].tolist()
        raise AssertionError(f"{case.name} plan {case.expect}: {int(bad.sum())} rows above 2 x the emulation's worst row "
                             f"({gate:.3e}); first (b {b}, query {i}, head {h}) at {e_got[b, i, h].item():.3e}")
