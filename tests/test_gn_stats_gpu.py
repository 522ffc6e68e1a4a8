"""GroupNorm statistics epilogues (StatTgt, GemmArgs::st[2]; stat_add / stat8_add / lds_stat_add / stat_flush in
tair_amd/csrc/gemm_kern.h, the split-K reduce in gemm.hip) at the UNet's group geometry, one producer at a time
against fp64: 10 .. 80-channel groups whose boundaries fall inside the epilogue's 8-channel items and 4-channel
fragments and straddle the tiles, a second target with a channel offset (tair_gemm_desc st2_*), groups that two
producers share, every kernel family and split-K combine.  Cases and references: tests/_gn_stat_cases.py; that each
case launches the plan it names: tests/test_gn_stats_cpu.py and, again, here before every launch.

Product producer -> the case that stands for it
    ResBlock conv1 (bias + emb + stats)                 tile64x64-conv, halo128-w16 / halo64-w64 (batched halo tiles),
                                                        m900-own (B = 1: two-K-group tiles), phase256x256-conv
    conv2 without the skip K-extension (hi + lo trunk   tile128x128-conv, halo192-w16, kgroup64x128-conv,
      residual, out_lo, one or two targets)             tile128x256-conv, ring128x320-conv
    conv2 with the skip K-extension (out_lo)            tile64x128-conv
    the composite proj_out (K-extension, hi + lo        tile64x128-dense, tile64x128-dense-s{2,3}-{coop,last,reduce}
      residual, two targets)
    Downsample / Upsample convs                         downsample (CONV3_S2), upsample (CONV3_UP), planner's plans
    input conv (4 channels)                             input-conv (CONV3_SMALLC)
    concat norm over 960 = 640 + 320 channels           skip320 / h640of960 geometries; test_concat_groupnorm_chain[960]
    concat norm over 1920 = 1280 + 640 channels         skip640 / h1280of1920 geometries; ...chain[1920]

Per case: guarded output (sentinel rows past M, columns past N, guard elements around the buffer), statistics
buffers [8][rs] of zeros between sentinel guard doubles; every slot the launch does not own stays exactly zero.
* output: plain bf16, rel-L2 <= 1.15 x the bf16 rounding floor (tests/test_kgroup_gpu.py ONE_ROUNDING); hi + lo,
  <= 2e-5, and the hi plane alone at the plain gate;
* statistics, per (batch element, group) and per target, against the fp64 sums of the stored values, with the
  bounds of _gn_stat_cases.slot_errors (plain: the any-order fp64 summation bound 2 n 2^-53 sum|v|; hi + lo: the
  bounds of tests/test_ffpout_gpu.py _check_stats);
* split-K: tickets back at zero; a second launch into zeroed statistics gives the same output bits, statistics
  within the same bounds against the reference, and statistics that differ from the first launch's, per target and
  slot, by at most the any-order summation bound 2 n 2^-53 sum|v| / sum v^2 (both launches add the same fp32
  values, hi + lo outputs included).  The combine is requested (tickets: cooperative; tickets + probe 4: last
  arriver; no tickets: reduce kernel), not verified: tair_k_gemm_plan reports kernel, tile and slices only, and
  the launcher falls back from the cooperative to the last-arriver combine when the grid is not resident;
* the listed two-target feature sets against the generic items loop (probe = 4, which at one K slice only makes
  epi_mask return E_GENERIC: gemm_grouped reads bit 2 only where splits > 1, regstage_set is off with statistics
  anyway, the kernels' other probe bits are 1, 2, 8 .. 32 and 128): same output bits; the generic loop's statistics
  within the bounds against the reference, and within the summation bound of the listed loop's (_check_same_sums).

The concat GroupNorm (two producers into one [M][C] buffer and one statistics slot, then tair_k_gn_apply_stats)
against fp64 F.group_norm of the stored concat tensor, per (batch element, group) block at CHAIN_GATE x the block's
own bf16 rounding floor.  The yardstick is the CPU emulation of the apply with exact statistics
(_gn_stat_cases.gn_emulate) on bf16(fp64 reference) of these very producers: worst block 1.0000 x its floor, to
four digits, at 960 and at 1920 channels (measure_chain_emulation below; the fp32 affine moves a bf16 rounding only
rarely), under 1.15, so the gate is 1.15.

Measured on MI355X (ranges over the cases of a family; statistics as worst deviation / bound over the slots).  Every
output is 1.0000 x its floor to four digits (floors 1.645e-3 .. 1.671e-3); the hi + lo outputs are at
2.427e-6 .. 2.466e-6.  On plain bf16 outputs the sums are exact (deviation 0: bf16 values of one group add up
without rounding in fp64) and the sums of squares stay below 3.4e-4 of the summation bound.
    family (kernel)                             hi + lo: sum / bound   sum^2 / bound    plain: sum^2 / bound
    4-wave 64 / 128-row tiles (0)               3.8e-3 .. 2.1e-2       4.2e-3 .. 2.5e-2   0 .. 3.4e-4
    8-wave 128x256 .. 256x320 tiles (0)         4.8e-3 .. 7.3e-3       5.6e-3 .. 9.0e-3   6.0e-5 .. 2.3e-4
    4-phase 256-row kernel (1)                  7.4e-3 .. 1.1e-2       1.0e-2 .. 1.6e-2   3.4e-5 .. 5.5e-5
    2-stage tiles (2)                           1.1e-2                 1.6e-2             1.0e-4
    halo tiles (3), chunk split included        5.1e-3 .. 7.4e-3       6.9e-3 .. 1.0e-2   0 .. 3.0e-4
    deep ring (4)                               7.3e-3 .. 8.6e-3       9.0e-3 .. 1.3e-2   -
    BK = 32 rings (0, bm < 0)                   6.4e-3 .. 9.0e-3       7.4e-3 .. 1.3e-2   4.6e-5 .. 3.0e-4
    two-K-group tiles (5)                       5.7e-3 .. 8.0e-3       7.1e-3 .. 1.0e-2   3.7e-5 .. 9.7e-5
    CONV3_S2 / CONV3_UP / CONV3_SMALLC          5.9e-3 .. 9.2e-3       8.6e-3 .. 1.3e-2   -
    split-K, 64-row tiles, three combines       5.8e-3 .. 7.8e-3       6.6e-3 .. 1.1e-2   0 .. 1.6e-4
    split-K reduce kernel on 128 / 256 rows     -                      -                  0
The coop, last-arriver and reduce combines of one case give the same figures, as do the listed feature set and the
generic loop.  Launch against launch (second split-K launch against the first, generic loop against listed set): the
sums are identical, the sums of squares differ by at most 9.9e-4 of the summation bound.  Concat norm: shared slot
sums exact, sums of squares 1.1e-4 (960) and 5.8e-5 (1920) of the bound; apply worst block 1.0000 x its floor, the
shared group 21 included.  The whole file runs in about 4 s.

Sensitivity, checked once each on a scratch build: computing bnd in stat_add / stat8_add without c_off fails 53 of
these 77 tests (every case whose offset is no multiple of the group width and whose boundary falls inside a
fragment, both chains); taking target 1's cg from target 0 in stat_flush fails 57 (every two-target case, both
chains).
"""
import ctypes

import pytest
import torch

import _gn_stat_cases as gc

pytestmark = pytest.mark.gpu

DEV = "cuda"
ONE_ROUNDING = 1.15  # tests/test_kgroup_gpu.py, tests/test_lnfold_gpu.py
HILO_TOL = 2e-5      # hi + lo outputs (tests/test_kernels_gpu.py two-plane trunk)
CHAIN_GATE = 1.15
GUARD = 64           # sentinel elements before and after every output buffer
EXTRA_ROWS = 8       # sentinel rows past M
PAD_COLS = 24        # sentinel columns past N (ldo % 8 == 0: the listed feature sets stay eligible)
SENTINEL = 768.0     # exact in bf16, far from every value of the cases
ST_GUARD = 16        # sentinel doubles before and after a statistics buffer
ST_PAD = 6           # zero doubles between the replicas (rs = 2 B G + ST_PAD)
ST_SENTINEL = -12345.0


def _L():
    from tair_amd import _lib
    return _lib.lib(), _lib


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


_WS = {}


def _ws():
    if not _WS:
        _WS["part"] = torch.empty(gc.PART_CAP, dtype=torch.float32, device=DEV)
        _WS["sem"] = torch.zeros(gc.SEM_CAP, dtype=torch.int32, device=DEV)
    return _WS["part"], _WS["sem"]


class StatBuf:
    """[8][rs] zeroed doubles between ST_GUARD sentinel doubles."""

    def __init__(self, B, Gn):
        self.B, self.G, self.rs = B, Gn, 2 * B * Gn + ST_PAD
        self.flat = torch.full((2 * ST_GUARD + gc.STAT_REPL * self.rs,), ST_SENTINEL, dtype=torch.float64, device=DEV)
        self.st = self.flat[ST_GUARD:ST_GUARD + gc.STAT_REPL * self.rs].view(gc.STAT_REPL, self.rs)
        self.st.zero_()

    def ptr(self):
        return self.st.data_ptr()

    def got(self):
        """[B, G, 2]: the replicas added up."""
        return self.st[:, :2 * self.B * self.G].sum(0).view(self.B, self.G, 2)

    def check_untouched(self, own):
        """guards, the padding between the replicas, and every (batch element, group) outside `own` [B, G]"""
        assert bool((self.flat[:ST_GUARD] == ST_SENTINEL).all()) and bool((self.flat[-ST_GUARD:] == ST_SENTINEL).all()), \
            "statistics guard doubles written"
        assert bool((self.st[:, 2 * self.B * self.G:] == 0).all()), "doubles between the replicas written"
        slots = self.st[:, :2 * self.B * self.G].view(gc.STAT_REPL, self.B, self.G, 2)
        assert bool((slots[:, ~own] == 0).all()), "a slot outside the launch's groups written"


class OutBuf:
    """planes x [M + EXTRA_ROWS][N + PAD_COLS] bf16 of SENTINEL between GUARD sentinel elements."""

    def __init__(self, M, N, planes, ld=None, col0=0):
        self.M, self.N, self.planes, self.col0 = M, N, planes, col0
        self.rows, self.ld = M + EXTRA_ROWS, ld or N + PAD_COLS
        n = planes * self.rows * self.ld
        self.flat = torch.full((2 * GUARD + n,), SENTINEL, dtype=torch.bfloat16, device=DEV)
        self.buf = self.flat[GUARD:GUARD + n].view(planes, self.rows, self.ld)

    def fields(self):
        f = dict(out=self.buf[0, 0, self.col0:].data_ptr(), ldo=self.ld)
        if self.planes == 2:
            f.update(out_lo=self.rows * self.ld)
        return f

    def check_guards(self):
        assert bool((self.flat[:GUARD] == SENTINEL).all()) and bool((self.flat[-GUARD:] == SENTINEL).all()), \
            "guard elements written"
        assert bool((self.buf[:, self.M:] == SENTINEL).all()), "rows past M written"
        assert bool((self.buf[:, :, :self.col0] == SENTINEL).all()), "columns before the output written"
        assert bool((self.buf[:, :, self.col0 + self.N:] == SENTINEL).all()), "columns past N written"

    def planes_out(self):
        return self.buf[:, :self.M, self.col0:self.col0 + self.N]


def _launch(case, o, out, sts, probe=None):
    """plan check + launch of `case` into out (OutBuf) and sts (one StatBuf per target)"""
    L, lib = _L()
    part, sem = _ws()
    kw = dict(o.fields(), **out.fields(), **gc.force_fields(case.force),
              **gc.stat_fields(case.targets, [s.ptr() for s in sts], [s.rs for s in sts], o.hw),
              **gc.combine_fields(case.combine, part.data_ptr(), sem.data_ptr()))
    if probe is not None:
        kw["probe"] = probe
    d = gc.make_desc(**kw)
    rc, plan = gc.plan_of(d)
    assert rc == 0, L.tair_last_error()
    assert plan == case.expect, (plan, case.expect)  # the plan the case names is the one that launches
    assert L.tair_k_gemm(ctypes.byref(d), _stream()) == 0, L.tair_last_error()
    torch.cuda.synchronize()
    lib.check_faults(case.name)
    assert torch.count_nonzero(sem) == 0, "split-K tickets not back at zero"


def _check_stats(case, o, stored, sts, what):
    """every target's slots against the fp64 sums of the stored values; -> worst (sum, sum^2) deviation / bound"""
    worst = [0.0, 0.0]
    for k, (t, sb) in enumerate(zip(case.targets, sts)):
        sums = gc.slot_sums(stored, o.B, o.hw, t)
        es, eq, own = gc.slot_errors(sb.got(), sums, case.hilo)
        sb.check_untouched(own)
        worst = [max(worst[0], es), max(worst[1], eq)]
        assert es <= 1 and eq <= 1, (what, "target", k, t, es, eq)
    return worst


def _check_same_sums(case, o, stored, sts_a, sts_b, what):
    """Two launches add the same fp32 values, only in another order: per target and slot their statistics differ by
    at most the any-order fp64 summation bound 2 n 2^-53 sum|v| (2 n 2^-53 sum v^2), also where the values are
    stored as hi + lo.  -> worst (sum, sum^2) difference / bound"""
    worst = [0.0, 0.0]
    for k, (t, a, b) in enumerate(zip(case.targets, sts_a, sts_b)):
        _, q, sa, cnt = gc.slot_sums(stored, o.B, o.hw, t)
        own = cnt > 0
        d = (a.got() - b.got()).abs()
        es = (d[..., 0][own] / (2 * cnt * 2.0 ** -53 * sa)[own]).max().item()
        eq = (d[..., 1][own] / (2 * cnt * 2.0 ** -53 * q)[own]).max().item()
        worst = [max(worst[0], es), max(worst[1], eq)]
        assert es <= 1 and eq <= 1, (what, "target", k, t, es, eq)
    return worst


def _run(case, probe=None):
    o = gc.operands(case, DEV)
    out = OutBuf(o.M, o.N, 2 if case.hilo else 1)
    sts = [StatBuf(o.B, t.G) for t in case.targets]
    _launch(case, o, out, sts, probe)
    out.check_guards()
    return o, out, sts


@pytest.mark.parametrize("case", gc.CASES, ids=repr)
def test_producer_statistics_against_fp64(case):
    o, out, sts = _run(case)
    p = out.planes_out()
    ref = o.ref
    fl = gc.bf16_floor(ref)
    assert bool(torch.isfinite(p.float()).all())
    e_hi = gc.rel_l2(p[0], ref)
    stored = p[0].double()
    e_hilo = float("nan")
    if case.hilo:
        stored = stored + p[1].double()
        e_hilo = gc.rel_l2(stored, ref)
    ws, wq = _check_stats(case, o, stored, sts, "first launch")
    if case.stands_for:
        print(f"gn-stats {case.name} stands for: {case.stands_for}")
    print(f"gn-stats {case.name}: kernel {case.expect[0]} tile {case.expect[1]}x{case.expect[2]}/{case.expect[3]} "
          f"M={o.M} N={o.N} hw={o.hw}: out / floor {e_hi / fl:.4f} (floor {fl:.3e}) hi+lo {e_hilo:.3e} "
          f"sum / bound {ws:.3e} sum^2 / bound {wq:.3e}")
    assert e_hi <= ONE_ROUNDING * fl, (e_hi, fl)
    if case.hilo:
        assert e_hilo <= HILO_TOL, e_hilo
    if case.expect[3] > 1:  # split-K: a second launch into zeroed statistics
        _, out2, sts2 = _run(case)
        assert torch.equal(out2.buf, out.buf), "a second split-K launch gave other output bits"
        _check_stats(case, o, stored, sts2, "second launch")
        d2 = _check_same_sums(case, o, stored, sts, sts2, "second launch against the first")
        print(f"  second launch: same bits, statistics against the first: sum {d2[0]:.3e} sum^2 {d2[1]:.3e} of the "
              f"summation bound")
    if case.listed_two_target:  # the listed feature set against the generic items loop
        _, out4, sts4 = _run(case, probe=4)
        assert torch.equal(out4.buf, out.buf), "the generic items loop gave other output bits than the listed set"
        _check_stats(case, o, stored, sts4, "generic loop")
        d4 = _check_same_sums(case, o, stored, sts, sts4, "generic loop against the listed set")
        print(f"  generic loop (probe = 4): same bits, statistics against the listed set: sum {d4[0]:.3e} sum^2 "
              f"{d4[1]:.3e} of the summation bound")


def _chain_tensors(C):
    """Both producers of the concat norm over C channels into one [M][C] buffer and one statistics slot (the skip
    producer also feeds its own norm, as target 0)."""
    ch, cs = gc.chain_cases(C)
    oh, os_ = gc.operands(ch, DEV), gc.operands(cs, DEV)
    assert (oh.B, oh.hw) == (os_.B, os_.hw) and oh.N + os_.N == C
    B, hw, M = oh.B, oh.hw, oh.M
    shared = StatBuf(B, gc.G)
    own = StatBuf(B, gc.G)
    cat = OutBuf(M, C, 1, ld=C)
    cat.N, cat.col0 = oh.N, 0
    _launch(ch, oh, cat, [shared])
    cat.N, cat.col0 = os_.N, oh.N
    _launch(cs, os_, cat, [own, shared])
    cat.N, cat.col0 = C, 0
    cat.check_guards()
    return ch, cs, oh, os_, cat, shared, own


@pytest.mark.parametrize("C", sorted(gc.CHAINS))
def test_concat_groupnorm_chain(C):
    L, _ = _L()
    ch, cs, oh, os_, cat, shared, own = _chain_tensors(C)
    B, hw, M = oh.B, oh.hw, oh.M
    x = cat.planes_out()[0]
    for o, lo in ((oh, 0), (os_, oh.N)):
        e, fl = gc.rel_l2(x[:, lo:lo + o.N], o.ref), gc.bf16_floor(o.ref)
        assert e <= ONE_ROUNDING * fl, (lo, e, fl)
    # the shared slot: n and the stored values of both producers
    xs = x.double()
    sums = [a + b for a, b in zip(gc.slot_sums(xs[:, :oh.N], B, hw, ch.targets[0]),
                                  gc.slot_sums(xs[:, oh.N:], B, hw, cs.targets[1]))]
    whole = gc.slot_sums(xs, B, hw, gc.Tgt(C // gc.G, gc.G, 0))
    assert all(torch.equal(a, b) for a, b in zip(sums[3:], whole[3:]))  # every group complete: hw * cg values
    es, eq, owned = gc.slot_errors(shared.got(), sums, hilo=False)
    shared.check_untouched(owned)
    assert bool(owned.all())
    assert es <= 1 and eq <= 1, (es, eq)
    es0, eq0, owned0 = gc.slot_errors(own.got(), gc.slot_sums(xs[:, oh.N:], B, hw, cs.targets[0]), hilo=False)
    own.check_untouched(owned0)
    assert es0 <= 1 and eq0 <= 1, (es0, eq0)
    # the consumer
    gamma, beta = gc.gn_params(C, DEV)
    y = OutBuf(M, C, 1, ld=C)
    assert L.tair_k_gn_apply_stats(x.data_ptr(), C, 0, B, hw, C, gc.G, gc.GN_EPS, gamma.data_ptr(), beta.data_ptr(), 0,
                                   shared.ptr(), shared.rs, y.buf.data_ptr(), C, 0, _stream()) == 0, L.tair_last_error()
    torch.cuda.synchronize()
    y.check_guards()
    ref = gc.gn_ref(x, B, hw, gamma, beta)
    r = gc.block_ratios(y.planes_out()[0], ref, B, hw)
    r_emu = gc.block_ratios(gc.gn_emulate(x, B, hw, gamma, beta), ref, B, hw)
    print(f"gn-stats chain C={C}: shared slot sum / bound {es:.3e} sum^2 / bound {eq:.3e}; apply worst block / floor "
          f"{r.max().item():.4f} (emulation with exact statistics on the same tensor {r_emu.max().item():.4f}), "
          f"shared group 21: {r[:, 21].tolist()}")
    assert float(r.max()) <= CHAIN_GATE, r.max().item()


def measure_chain_emulation():
    """The yardstick of CHAIN_GATE, on the CPU: python -c 'import test_gn_stats_gpu as t; t.measure_chain_emulation()'
    from tests/.  The producers' stored tensors are taken as bf16(fp64 reference)."""
    for C in sorted(gc.CHAINS):
        ch, cs = gc.chain_cases(C)
        oh, os_ = gc.operands(ch, "cpu"), gc.operands(cs, "cpu")
        x = torch.cat([oh.ref, os_.ref], 1).to(torch.bfloat16)
        gamma, beta = gc.gn_params(C)
        r = gc.block_ratios(gc.gn_emulate(x, oh.B, oh.hw, gamma, beta), gc.gn_ref(x, oh.B, oh.hw, gamma, beta), oh.B, oh.hw)
        print(f"C={C}: emulated apply, worst block / floor {r.max().item():.4f}, mean {r.mean().item():.4f}")
