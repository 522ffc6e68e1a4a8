"""Which GEMM plans does the split-precision VAE launch?  (host logic, no GPU)

HipVAEDecoder.decode and HipVAEEncoder.encode_mode run on the CPU with a stand-in for the loaded library whose
tair_k_gemm plans each descriptor with the real tair_k_gemm_plan and records it (tests/_vae_cases.py); every call at
the workload's shape (latent 64x64, image 512x512, B = 1 and 2) must reduce to a signature of _vae_cases.SIGNATURES,
the table tests/test_vae_kernels_gpu.py parametrises over.  A planner change that moves the VAE onto a plan no
per-kernel test runs fails here.

The same module pins, from the reference and a CPU emulation alone, what the GPU tests rely on: every table entry is
reached by a GEMM case at some shape, no case skips more than 1 % of its rows or columns, and the per-row /
per-column bound R_ROWCOL is at least 4 x the worst value the fp32 emulation reaches (and at most 1e-4).
"""
import pytest

import _vae_cases as vc


@pytest.fixture(scope="module")
def recorded():
    return {(w, B): vc.record_workload(w, B) for w in ("dec", "enc") for B in (1, 2)}


def test_every_vae_gemm_at_the_workload_shape_is_in_the_table(recorded):
    seen = set()
    for (which, B), calls in recorded.items():
        assert len(calls) >= 30, (which, B, len(calls))  # conv_in, 12-14 ResnetBlocks, the AttnBlock, conv_out
        for sig, (M, N, K, Kx, rc) in calls:
            assert rc == 0, (which, B, M, N, K, Kx)
            assert sig in vc.SIGNATURES, (f"{which} B={B}: GEMM M={M} N={N} K={K} Kx={Kx} plans to a signature no "
                                          f"per-kernel test covers: {dict(zip(vc.FIELDS, sig))}")
            seen.add(sig)
    # and the table holds nothing the workload does not launch (a stale row would pin a dead plan)
    assert seen == vc.SIGNATURES, [dict(zip(vc.FIELDS, s)) for s in vc.SIGNATURES - seen]


def test_the_check_notices_a_missing_table_row(recorded):
    """Each row of the table is needed: without it some recorded call is uncovered."""
    sigs = {sig for calls in recorded.values() for sig, _ in calls}
    for row in vc.SIGNATURES:
        assert not sigs <= (vc.SIGNATURES - {row}), row


def test_workload_exercises_the_paths_the_vae_alone_uses(recorded):
    sigs = {sig for calls in recorded.values() for sig, _ in calls}
    f = {n: i for i, n in enumerate(vc.FIELDS)}
    assert {s[f["out_split"]] for s in sigs} == {0, 1, 2}
    assert any(s[f["res_lo"]] and s[f["stats"]] for s in sigs)
    assert any(s[f["k_ext"]] for s in sigs) and any(s[f["s2_shift"]] for s in sigs)
    assert any(s[f["c_not_64"]] for s in sigs) and any(s[f["out_f32"]] and s[f["split_k"]] for s in sigs)


def test_every_table_row_is_run_by_a_gemm_case():
    """Each signature belongs to the kind of some case of the GPU tests, and some shape of that case takes the plan
    when forced (a plan the validator refuses at a shape moves to the next larger one, never out of the list)."""
    covered = set()
    for c in vc.CASES:
        kind = c.ops("cpu", c.shapes[0]).kind()
        for s in c.shapes + c.grow:
            assert c.ops("cpu", s).kind() == kind, (c.name, s)
        plans = vc.plans_of(kind)
        assert plans, c.name
        for plan in plans:
            shape, _ = vc.forced_shape(c, plan)
            assert shape is not None, (c.name, plan)
            covered.add((kind[0],) + tuple(plan) + kind[1:])
    assert covered == vc.SIGNATURES, vc.SIGNATURES - covered


def test_row_and_column_bound_from_the_fp32_emulation():
    """R_ROWCOL = 4 x the worst per-row / per-column rel-L2 of the CPU emulation (three plane products accumulated in
    fp32, fp32 epilogue, hi + lo storage) against fp64 over every input the GPU tests use, and at most 1e-4; the
    reference alone leaves at most 1 % of a case's rows or columns under the skip threshold."""
    worst = 0.0
    for run in vc.runs():
        o = vc.resolve(run)
        name, shape = run[0], (o.B, o.hw, o.M, o.N)
        er, ec, sr, sc = vc.rowcol_errors(o.emu, o.ref)
        assert sr <= vc.MAX_SKIPPED and sc <= vc.MAX_SKIPPED, (name, shape, sr, sc)
        e_all = ((o.emu - o.ref).norm() / o.ref.norm()).item()
        print(f"vae emulation {name} {shape}: whole {e_all:.3e} worst row {er:.3e} worst column {ec:.3e}")
        assert e_all <= vc.TOL_ALL
        worst = max(worst, er, ec)
    print(f"vae emulation: worst per-row / per-column rel-L2 {worst:.3e}, 4 x = {4 * worst:.3e}, R_ROWCOL {vc.R_ROWCOL:.3e}")
    # (the worst value moves a little with the summation order of the host's fp32 GEMM / conv: R stays 4 x it to 12 %)
    assert 3.5 * worst <= vc.R_ROWCOL <= 4.5 * worst and vc.R_ROWCOL <= 1e-4, (worst, vc.R_ROWCOL)
