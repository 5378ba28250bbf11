"""GPU suite (-m gpu): the exact multigrid's fused visits of the one-wave levels (129 ... 1025 nodes) with predicted start values, a
32-node warm-up and a bitwise hand-over check (poisson_kernels.inc: cs_predict3, cs_visit3).

A visit whose check passes in every lane IS the sequential result (induction over the lanes from the level's boundary), a visit whose
check fails is put back and repeated with the 112-node warm-up from old values -- so U, the V-cycle counts and the error norms are the
same bits with the prediction (default), without it (POISSON_NOPREDICT), with every prediction spoilt (POISSON_PREDICT_FUZZ: every
visit takes the redo path) and with the visits run sweep by sweep (POISSON_NOFUSE3_WAVE).  Tolerance 0 everywhere.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import dftatom_amd as D                 # noqa: E402
from _knobs import knobs as env          # noqa: E402  (DFTA_DEBUG entries for the duration of a block)

# 12 levels: the one-wave levels and their entry only; 17: the only size with the staged levels 4-6 of the resident kernel; a uniform grid
SIZES = [(12, 2e-3, 25.0), (14, 5e-4, 25.0), (17, 1e-4, 50.0), (12, None, 25.0)]


@pytest.fixture(scope="module")
def ctx(torch_first):
    c = D.Context(0)
    yield c
    c.close()


def _solve(ctx, grid, Z, rho, **kv):
    with env(**kv):
        ps = D.Poisson(ctx, grid, 1, D.POISSON_EXACT)
        U, vc, err = ps.solve([Z], rho)
        counts = ps.predict_counts()
        ps.close()
    return U, vc, err, counts


def _rho(grid, Z):
    return (Z * np.exp(-2 * grid.r()) / np.pi)[None, :]


@pytest.mark.parametrize("Z", [1, 18, 86])
@pytest.mark.parametrize("L,delta,R", SIZES)
def test_predicted_visits_return_the_unpredicted_bits(ctx, L, delta, R, Z):
    """U, V-cycle count and error norm of the default build against the 112-node warm-ups, the all-redo run and the sweep-by-sweep visits
    (Z = 1 ends visits early: restore and prediction together)"""
    grid = D.Grid(ctx, L, delta, R)
    rho = _rho(grid, Z)
    U, vc, err, (checked, repeated) = _solve(ctx, grid, Z, rho)
    assert checked > 0, "no visit ran with predicted start values"
    for kv in ({"DFTA_POISSON_NOPREDICT": "1"}, {"DFTA_POISSON_PREDICT_FUZZ": "1"}, {"DFTA_POISSON_NOFUSE3_WAVE": "1"}):
        U2, vc2, err2, (c2, r2) = _solve(ctx, grid, Z, rho, **kv)
        assert np.array_equal(U.view(np.int64), U2.view(np.int64)), (L, Z, kv, float(np.max(np.abs(U - U2))))
        assert np.array_equal(vc, vc2) and np.array_equal(err.view(np.int64), err2.view(np.int64)), (L, Z, kv, vc, vc2, err, err2)
        if "DFTA_POISSON_PREDICT_FUZZ" not in kv:
            assert (c2, r2) == (0, 0), (kv, c2, r2)        # neither run predicts anything
    grid.close()


@pytest.mark.parametrize("L,delta,R", SIZES)
def test_the_check_fires_on_spoilt_predictions_and_is_quiet_otherwise(ctx, L, delta, R):
    """POISSON_PREDICT_FUZZ moves every prediction by a relative 2^-20: every visit fails its check and is repeated (repeated = checked:
    the check works, and the redo path returns the same bits -- test above).  In the default run at most one visit in a thousand may be
    repeated (the cap is a condition of the design: a repeat costs a visit and a half).
    Measured on MI355X (checked visits per solve, Z = 1 / 18 / 86): 12 levels 48 / 800 / 800, 14 levels 48 / 800 / 800, 17 levels
    640 / 800 / 800, the uniform grid 56 / 800 / 800 -- 7 192 visits, none repeated; with the fuzz knob every one of them repeated."""
    grid = D.Grid(ctx, L, delta, R)
    checked = repeated = 0
    for Z in (1, 18, 86):
        rho = _rho(grid, Z)
        _, _, _, (c, r) = _solve(ctx, grid, Z, rho)
        _, _, _, (cf, rf) = _solve(ctx, grid, Z, rho, DFTA_POISSON_PREDICT_FUZZ="1")
        print("predict counts, %d levels, delta %s, Z %d: default %d checked / %d repeated, fuzz %d / %d" % (L, delta, Z, c, r, cf, rf))
        assert cf > 0 and rf == cf, (L, Z, cf, rf)
        assert c == cf, (L, Z, c, cf)             # the same visits either way
        checked += c
        repeated += r
    assert repeated * 1000 <= checked, (L, checked, repeated)
    grid.close()
