"""tests/_mg_ref.py against the oracle, on the CPU: (1) the Python restatement of Initialize / Ascend / Descend / VCycle / FullCycle
returns the bits and the V-cycle count of dfo_solve_poisson_nonuniform / dfo_solve_poisson_uniform, and (2) every stop test of every
solve that tests/test_gpu_multigrid_ops.py demands bits for keeps |err / errorMin - 1| >= 1e-9, far above the n 2^-52 by which a
GPU sweep's norm may differ (argument in tests/_mg_ref.py).  Measured here: the smallest margin over all cases is 8.96e-6 (10 levels,
Z = 86, the 5-node level).  An input that does not keep the margin is replaced, not tolerated.
"""
import numpy as np
import pytest

import _mg_ref as M


def _id(case):
    return "%s-Z%d" % (M.grid_id(case[0]), case[1])


@pytest.mark.parametrize("case", M.solve_cases(), ids=_id)
def test_restatement_equals_oracle_and_keeps_the_margin(case):
    (levels, delta, Rmax), Z = case
    rho, src0, U, vc = M.oracle_case(levels, delta, Rmax, Z)
    assert np.all(np.isfinite(U)) and 1 <= vc <= 100
    got, got_vc, (margin, lvl, n) = M.solve_from_source(levels, delta, src0, Z)
    assert got_vc == vc
    assert np.array_equal(got.view(np.int64), U.view(np.int64))
    print("%s Z=%d: %d V-cycles, smallest margin %.3e (level %d, %d nodes)" % (M.grid_id(case[0]), Z, vc, margin, lvl, n))
    assert margin >= M.MARGIN, (margin, lvl, n)
    assert M.MARGIN > 30 * M.norm_bound(131073)          # what the margin is for


def test_restated_pieces_equal_the_oracle_drivers():
    """Initialize and one VCycle from a planted state, piece by piece: dfo_initialize / dfo_vcycle against the restatement"""
    levels, delta = 9, 1.6e-2
    rng = np.random.default_rng(5)
    a, b = M.MgRef(levels, delta), M.MgRef(levels, delta)
    try:
        for m in (a, b):
            m.set_boundaries(0.25, 3.0)
        src0 = 1e-2 * rng.standard_normal(a.n[0])
        a.Src[0][:] = src0
        b.Src[0][:] = src0
        a.o.dfo_initialize(a.ps, 1e-3)
        b.initialize(1e-3)
        for l in range(levels):
            assert np.array_equal(a.Phi[l], b.Phi[l]) and np.array_equal(a.Src[l], b.Src[l]), l
        for l in range(levels):
            phi = rng.standard_normal(a.n[l])
            a.Phi[l][:] = phi
            b.Phi[l][:] = phi
        ea = a.o.dfo_vcycle(a.ps, 1e-14, 3)
        eb = b.vcycle(1e-14, 3)
        assert ea == eb
        for l in range(levels):
            assert np.array_equal(a.Phi[l].view(np.int64), b.Phi[l].view(np.int64)), l
            assert np.array_equal(a.Src[l].view(np.int64), b.Src[l].view(np.int64)), l
    finally:
        a.close()
        b.close()
