"""CPU suite: the model behind the predicted start values of the exact multigrid's short warm-ups (poisson_kernels.inc:
cs_predict3 / cs_visit3).

A Gauss-Seidel sweep is, in exact arithmetic, the affine recurrence x_i = a x_(i-1) + c_i with a = (1 + d/2) / 2 and
c_i = (S_i + (1 - d/2) Phi_(i+1)) / 2.  Chunk-local offsets (a lane's recurrence run from zero) combined by a log-depth scan over the
lanes give every node's new value to a few ulp of the level's scale without any warm-up; a lane that restarts the reference's own
expression W nodes in front of its chunk from that prediction (instead of from the old value, which is off by O(1) of itself on a
correction level) reaches the sequential sweep's bits after far fewer nodes of contraction a ~ 0.52 than the 95 / 112 the old-value
start needs.

Here: the 129- to 1025-node levels of an Ar solve at 14 levels (oracle: dfo_poisson_create, dfo_solve_poisson_nonuniform,
dfo_gauss_seidel and the struct's Phi / Src), 64 lanes; for every level forty consecutive sweeps from Phi = 0 (a correction level right
after the restriction: Phi changes by O(1) of itself in the first sweeps).  The sequential sweep in numpy is first held to
dfo_gauss_seidel bit for bit, so the model's reference expression is the oracle's.  Measured: 38 of 9 800 chunk boundaries differ at
W = 8, none of 9 480 at W = 16 and none of 8 880 at W = 32 (boundaries whose restart node lies inside the level); the largest prediction
error is 2.0 ulp of the level's largest |Phi|.
"""
import ctypes as C

import numpy as np
import pytest

import _oracle as O

LANES = 64
L14 = (14, 5e-4, 25.0)
SWEEPS = 40


def _seq_sweep(S, x, d):
    """PoissonSolver.cpp:48-61 in numpy scalars: the same expression in the same order, no contraction"""
    x = x.copy()
    for i in range(1, len(x) - 1):
        x[i] = 0.5 * (S[i] + x[i - 1] + x[i + 1] - d * (x[i + 1] - x[i - 1]) * 0.5)
    return x


def _predict(S, old, d):
    """every node's new value from chunk-local offsets and a Hillis-Steele scan over the 64 lanes (the arithmetic of cs_predict3's one
    stage, without FMA): lane t owns nodes t C .. t C + C - 1, node 0 is the boundary value"""
    n = len(old)
    Cn = (n - 1) // LANES
    a, omd = 0.5 * (1.0 + 0.5 * d), 1.0 - 0.5 * d
    c = np.zeros(n)
    c[1:n - 1] = 0.5 * (omd * old[2:] + S[1:n - 1])
    c = c[:LANES * Cn].reshape(LANES, Cn)
    z = np.zeros((LANES, Cn))
    run = np.zeros(LANES)
    for k in range(Cn):
        run = a * run + c[:, k]
        if k == 0:
            run[0] = old[0]
        z[:, k] = run
    pw = a ** np.arange(1, Cn + 1)
    v, ratio, off = run.copy(), pw[-1], 1
    while off < LANES:
        up = np.concatenate([np.zeros(off), v[:-off]])
        v = np.where(np.arange(LANES) >= off, ratio * up + v, v)
        ratio *= ratio
        off *= 2
    xin = np.concatenate([[0.0], v[:-1]])
    p = pw[None, :] * xin[:, None] + z
    p[0, 0] = old[0]
    return np.concatenate([p.reshape(-1), [old[-1]]])


def _restarted_boundaries(S, old, new, pred, d, W):
    """the value at node lo - 1 of every lane with lo - W - 1 >= 1, from the reference expression restarted at the predicted value of
    node lo - W - 1 (all lanes at once); returns (boundaries, boundaries whose value is not the sequential sweep's bits)"""
    n = len(old)
    Cn = (n - 1) // LANES
    lo = np.arange(1, LANES) * Cn
    lo = lo[lo - W - 1 >= 1]
    x = pred[lo - W - 1].copy()
    for j in range(W, 0, -1):
        i = lo - j
        x = 0.5 * (S[i] + x + old[i + 1] - d * (old[i + 1] - x) * 0.5)
    return len(lo), int(np.count_nonzero(x.view(np.int64) != new[lo - 1].view(np.int64)))


@pytest.fixture(scope="module")
def model():
    o = O.oracle()
    L, delta, R = L14
    g = O.make_grid(L, delta, R)
    r = O.grid_r(g)
    Z = 18
    rho = Z * np.exp(-2 * r) / np.pi
    U = np.zeros(g.N)
    p = o.dfo_poisson_create(L, delta)
    o.dfo_solve_poisson_nonuniform(p, Z, R, O.dp(rho), O.dp(U))
    ps = p.contents
    out = {"bounds": {8: 0, 16: 0, 32: 0}, "miss": {8: 0, 16: 0, 32: 0}, "ulp": 0.0, "levels": []}
    for lvl in range(ps.levels):
        n = ps.n[lvl]
        if n < 129 or n > 1025:
            continue
        out["levels"].append(n)
        d = ps.dlev[lvl]
        Phi = np.ctypeslib.as_array(ps.Phi[lvl], shape=(n,))
        S = np.ctypeslib.as_array(ps.Src[lvl], shape=(n,)).copy()
        Phi[1:n - 1] = 0.0
        for _ in range(SWEEPS):
            old = Phi.copy()
            o.dfo_gauss_seidel(p, lvl)
            new = Phi.copy()
            assert np.array_equal(_seq_sweep(S, old, d).view(np.int64), new.view(np.int64))
            pred = _predict(S, old, d)
            scale = np.spacing(np.max(np.abs(new)))
            out["ulp"] = max(out["ulp"], float(np.max(np.abs(pred - new)) / scale))
            for W in out["bounds"]:
                nb, miss = _restarted_boundaries(S, old, new, pred, d, W)
                out["bounds"][W] += nb
                out["miss"][W] += miss
    o.dfo_poisson_destroy(p)
    print("predict model: levels %s, boundaries %s, differing %s, largest prediction error %.2f ulp of the level's scale"
          % (out["levels"], out["bounds"], out["miss"], out["ulp"]))
    return out


def test_the_levels_are_the_one_wave_levels(model):
    assert model["levels"] == [1025, 513, 257, 129]


def test_predictions_are_within_16_ulp_of_the_levels_scale(model):
    assert model["ulp"] <= 16.0, model["ulp"]


def test_no_boundary_differs_after_32_nodes(model):
    assert model["bounds"][32] >= 8000 and model["miss"][32] == 0, model


def test_the_model_can_fail_after_8_nodes(model):
    assert model["miss"][8] > 0, model
