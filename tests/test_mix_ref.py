"""CPU suite of tests/_mix_ref.py, the stage-wise reference tests/test_gpu_mixing_kernels.py holds the mixing kernels to.

(a) Anchoring: the stage functions evaluated in float64 and chained (MixModel, one sum over all nodes) return the bits of
    tests/_anderson_ref.AndersonRef.anderson_mix over 12 steps, LDA and LSDA, on the generator's inputs; the grid tables of
    _mix_ref.log_tables are ScfRef's bit for bit.
(b) The generator gives, on the model alone, what the GPU tests rely on: an m = 8 run whose regularised systems reach condition
    numbers >= 1e10; in every case candidates that are clearly negative (cand_ext < -tol) and none inside the clamp's band
    |cand_ext| <= tol (the GPU test allows 0.1 % of a case's nodes); the failed solves of the batch on the planned steps and nowhere
    else; the duplicate pair exactly singular before the shift and solved after it.
Every test prints what it observed.
"""
import numpy as np
import pytest

import _anderson_ref as AR
import _mix_ref as M
import _scf_ref as SR
import dftatom_amd as D

GRID = dict(mg_levels=12, MaxR=25.0, delta=2e-3)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


@pytest.mark.parametrize("Z,lsda", [(10, False), (7, True)], ids=["lda", "lsda"])
def test_float64_stages_are_andersonref_bits(Z, lsda):
    a, b = SR.config_levels(D.ion_config(Z, 0, lsda), lsda)
    ref = AR.AndersonRef(Z, a, b, mix=0.5, **GRID)
    try:
        r, cnst, hstep = M.log_tables(ref.N, GRID["delta"], GRID["MaxR"])
        assert np.array_equal(bits(r[1:]), bits(ref.pos[1:])) and np.array_equal(bits(cnst[1:]), bits(ref.cnst[1:])) and hstep == 1.0
        model = M.MixModel(ref.pos, ref.cnst, 1.0, 2 if lsda else 1, ref.m, ref.warmup, chunked=False)
        used = 0
        for k in range(1, 13):
            x, acc = M.generate(ref.pos, lsda, 3, k)
            want = ref.anderson_mix(list(x), list(acc))
            got = model.step(0.5, x, acc)
            for c in range(len(want)):
                assert np.array_equal(bits(got[c]), bits(want[c])), (k, c)
            assert len(ref.hist) == model.state[1]
            used += model.last["use"]
            if model.last["use"]:
                assert not np.array_equal(bits(got[:, 1:]), bits(np.asarray(model.last["lin"])[:, 1:]))
        assert used == 9 and ref.accelerated == 9 and ref.cleared == 0
        newest = M.history_slots(model.state[0], model.state[1], model.m, model.state[1])[-1]
        assert np.array_equal(bits(np.concatenate(list(model.ring[:, newest, 1, 1:]))), bits(ref.hist[-1][1]))
    finally:
        ref.close()


def test_automaton():
    """m = 2, warmup = 2: two linear steps that record, accelerated steps on a ring that wraps, a failed solve that clears"""
    st, seen = (0, 0, 0), []
    for ok in (True, True, True, True, False, True, True):
        st, this = M.automaton(st, 2, 2, ok)
        seen.append(M.state_ints(st, this))
    assert seen == [[1, 1, 1, 0, 0, 0, 0, 0], [0, 2, 2, 1, 0, 0, 0, 0], [1, 2, 3, 0, 2, 1, 0, 0], [0, 2, 4, 1, 2, 1, 0, 0],
                    [0, 0, 5, 0, 0, 0, 0, 0], [1, 1, 6, 0, 0, 0, 0, 0], [0, 2, 7, 1, 1, 1, 0, 0]]
    assert M.history_slots(1, 2, 2, 2) == [1, 0] and M.history_slots(0, 3, 4, 3) == [1, 2, 3] and M.history_slots(2, 4, 4, 4) == [2, 3, 0, 1]


def tables(N, uniform=False):
    return M.uniform_tables(N, M.RMAX) if uniform else M.log_tables(N, M.LOG_GRIDS[N][1], M.RMAX)


def run_case(N, lsda, m, warmup, steps, inputs, uniform=False):
    """the model over a case: (largest condition number of A_r, clearly negative candidates, nodes in the band, nodes, failed steps)"""
    r, cnst, hstep = tables(N, uniform)
    model = M.MixModel(r, cnst, hstep, 2 if lsda else 1, m, warmup)
    cond, neg, band, nodes = 0.0, 0, 0, 0
    for k in range(1, steps + 1):
        x, acc = inputs(r, lsda, k)
        out = model.step(M.ALPHA, x, acc)
        L = model.last
        if not L["use"]:
            assert np.array_equal(bits(out[:, 1:]), bits(np.asarray(L["lin"])[:, 1:]))
            continue
        cond = max(cond, float(np.linalg.cond(M.regularised(L["A"])[0])))
        _, cand, T = M.candidate(M.ALPHA, 1. - M.ALPHA, x, L["g"], L["xh"], L["fh"], L["gamma"])
        tol = (L["H"] + 4) * M.EPS * T
        ok = np.isfinite(cand[:, 1:])
        assert ok.all()
        neg += int(np.sum(cand[:, 1:] < -tol[:, 1:]))
        band += int(np.sum(np.abs(cand[:, 1:]) <= tol[:, 1:]))
        nodes += cand[:, 1:].size
        assert np.all(x[:, 1:] > 0) and np.all(acc[:, 1:] >= 0) and acc[0, -1] == 0.0 and acc[0, N // 2] > 0
    return cond, neg, band, nodes, model.failed


def seeded(seed):
    return lambda r, lsda, k: M.generate(r, lsda, seed, k)


SIZES = [(N, lsda, 4, 3, False) for N in sorted(M.LOG_GRIDS) for lsda in (False, True)]
SIZES += [(1025, True, m, 1, False) for m in range(1, 9)] + [(1025, False, 3, 3, True)]


@pytest.mark.parametrize("N,lsda,m,warmup,uniform", SIZES)
def test_generator_exercises_the_clamp(N, lsda, m, warmup, uniform):
    cond, neg, band, nodes, failed = run_case(N, lsda, m, warmup, warmup + 2 * m + 2, seeded(N % 7 + m), uniform)
    print("N %5d %s m %d%s: cond(A_r) <= %.1e, %d clearly negative candidates, %d in the band, of %d; failed solves %s"
          % (N, "LSDA" if lsda else "LDA", m, " uniform" if uniform else "", cond, neg, band, nodes, failed))
    assert neg >= 5 and band == 0 and not failed
    if m == 8:
        assert cond >= 1e10


@pytest.mark.parametrize("lsda", [False, True], ids=["lda", "lsda"])
def test_batch_plan(lsda):
    """the five atoms of the batch: the planned failed solves on the planned steps, negative candidates in every atom"""
    for atom in range(M.BATCH_ATOMS):
        live = [k for k in range(1, M.BATCH_STEPS + 1) if not M.batch_input(tables(1025)[0], lsda, atom, k)[2]]
        assert live == (list(range(1, 6)) if atom == 1 else list(range(1, M.BATCH_STEPS + 1)))
        r, cnst, hstep = tables(1025)
        model = M.MixModel(r, cnst, hstep, 2 if lsda else 1, M.BATCH_M, M.BATCH_WARMUP)
        neg = band = 0
        for k in live:
            x, acc, _ = M.batch_input(r, lsda, atom, k)
            out = model.step(M.ALPHA, x, acc)
            L = model.last
            bad = ~np.isfinite(acc)
            assert np.all(np.isfinite(out[~bad])) and (not bad.any() or not L["use"])
            if L["use"]:
                _, cand, T = M.candidate(M.ALPHA, 1. - M.ALPHA, x, L["g"], L["xh"], L["fh"], L["gamma"])
                tol = (L["H"] + 4) * M.EPS * T
                neg += int(np.sum(cand[:, 1:] < -tol[:, 1:]))
                band += int(np.sum(np.abs(cand[:, 1:]) <= tol[:, 1:]))
        print("batch atom %d %s: failed solves %s, %d clearly negative candidates, %d in the band" % (atom, "LSDA" if lsda else "LDA", model.failed, neg, band))
        assert model.failed == M.BATCH_FAILURES[atom] and neg >= 5 and band == 0


@pytest.mark.parametrize("lsda", [False, True], ids=["lda", "lsda"])
def test_duplicate_pair_plan(lsda):
    r, cnst, hstep = tables(1025)
    model = M.MixModel(r, cnst, hstep, 2 if lsda else 1, M.DUP_M, M.DUP_WARMUP)
    for k in range(1, M.DUP_STEPS + 1):
        x, acc = M.dup_input(r, lsda, k)
        model.step(M.ALPHA, x, acc)
        L = model.last
        if k == 3:
            A, b = L["A"], L["b"]
            assert L["H"] == 2 and A[0, 0] == A[0, 1] == A[1, 1] > 0 and b[0] == b[1]
            assert L["use"] == 1 and np.all(np.isfinite(L["gamma"]))
            assert AR.cholesky_solve(A, b) is None                   # singular without the shift
            Ar, lam = M.regularised(A)
            exact = 2 * M.LD(b[0]) / (2 * M.LD(A[0, 0]) + M.LD(lam))
            dist = abs(M.LD(L["gamma"][0]) + M.LD(L["gamma"][1]) - exact) / abs(exact)
            print("duplicate pair %s: gamma %s, |gamma_0 + gamma_1 - exact| / |exact| = %.2f eps" % ("LSDA" if lsda else "LDA", L["gamma"], float(dist) / M.EPS))
        assert (k >= 3) == bool(L["use"]) and not model.failed
