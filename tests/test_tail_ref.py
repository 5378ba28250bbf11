"""CPU suite: tests/_tail_ref.py, the float64 restatement of the tail of an SCF step that tests/test_gpu_scf_tail.py replays the device
against.

* On the state of tests/_scf_ref.ScfRef (whose VWN steps are the bits of dfo_scf_step, tests/test_scf_ref.py) the restated potentials,
  integrands, Simpson 3/8 and assembly give ScfRef's energies bit for bit, LDA and LSDA.
* The model of k_integrate_simpson38_par's summation order shares the kernel's choices, so its five integrals are also held to
  Simpson 3/8 of the same integrands in np.longdouble:  |model - ext| <= c eps Sum |w_i v_i|,  c = _tail_ref.parallel_roundings(N)
  = ceil((N - 2) / 256) + 6 + 2 + 5 = 29 at 4097 nodes (a sum's error is at most the longest chain of roundings a term passes
  through, times the sum of the magnitudes).  Observed: below 0.05 of the bound.  A model that stops one node early (drops node
  N - 2) or sends i % 3 == 1 instead of i % 3 == 0 to the second sum misses the bound by factors above 1e8.
"""
import numpy as np
import pytest

import _scf_ref as SR
import _tail_ref as TR

LD = np.longdouble
EPS64 = float(np.finfo(np.float64).eps)
GRID = dict(mg_levels=12, delta=2e-3, MaxR=25.0)
CASES = {"Ne LDA": (10, [(0, 0, 2.0), (1, 0, 2.0), (1, 1, 6.0)], None),
         "N LSDA": (7, [(0, 0, 1.0), (1, 0, 1.0), (1, 1, 3.0)], [(0, 0, 1.0), (1, 0, 1.0)])}
_refs = {}


def stepped(name):
    """(ScfRef after two steps, the five energies of its second step)"""
    if name not in _refs:
        Z, a, b = CASES[name]
        ref = SR.ScfRef(Z, a, b, functional=SR.VWN, **GRID)
        ref.step()
        _refs[name] = (ref, ref.step())
    return _refs[name]


def tail(ref):
    potA, potB = TR.potentials(ref.Z, ref.lsda, ref.pos, ref.U, ref.Vexc, ref.va, ref.vb)
    return potA, potB, TR.integrands(ref.Z, ref.lsda, False, ref.pos, ref.cnst, ref.density, ref.dA, ref.dB, ref.U, ref.Vexc, ref.eexc,
                                     potA, potB)


@pytest.mark.parametrize("name", sorted(CASES))
def test_restated_tail_gives_the_reference_bits(name):
    ref, want = stepped(name)
    assert np.all(np.isfinite(want)) and ref.density[1] > 0
    potA, potB, F = tail(ref)
    assert np.array_equal(potA, ref.potA) and (not ref.lsda or np.array_equal(potB, ref.potB))
    occ = [f for _, _, f in ref.cfg[0] + ref.cfg[1]]
    E = list(ref.E[0]) + list(ref.E[1])
    e = TR.assemble(occ, E, [TR.quadrature(2, 1.0, f) for f in F])
    assert [e[k] for k in TR.FIELDS[:5]] == list(want)
    assert e["Ekinetic"] == e["Eelectronic"] - e["Epotential"] and e["Ecoul"] == -e["Ehartree"]
    assert np.array_equal(TR.log_cnst(ref.g.Rp, ref.delta, ref.N)[1:], ref.cnst[1:])


@pytest.mark.parametrize("name", sorted(CASES))
def test_parallel_sum_model_against_extended_simpson(name):
    ref, _ = stepped(name)
    N = ref.N
    c = TR.parallel_roundings(N)
    assert N == 4097 and c == 16 + 6 + 2 + 5
    worst = 0.0
    for k, f in enumerate(tail(ref)[2]):
        ext, mag = TR.simpson38_extended(f, 1.0)
        bound = c * EPS64 * mag
        got = TR.simpson38_parallel(f, 1.0)
        ratio = float(abs(LD(got) - ext) / bound)
        worst = max(worst, ratio)
        assert ratio <= 1, (name, k, ratio)
        ordered = TR.quadrature(2, 1.0, f)                                   # the reference's order: a chain of 2 (N - 2) / 3 additions
        assert abs(LD(ordered) - ext) <= (2 * (N - 2) // 3 + 5) * EPS64 * mag
        for wrong in (dict(last=N - 2), dict(second_class=1)):
            bad = float(abs(LD(TR.simpson38_parallel(f, 1.0, **wrong)) - ext) / bound)
            assert bad > 1e6, (name, k, wrong, bad)
    print("%s: parallel-sum model, |model - ext| / (%d eps Sum|w v|) max %.3f" % (name, c, worst))


def test_parallel_sum_model_on_short_and_ragged_vectors():
    """sizes around the thread count and the period of the rule: the model is Simpson 3/8 for every n = 3 m + 1"""
    rng = np.random.default_rng(3)
    for n in (4, 7, 256, 259, 514, 769, 1027):
        assert n % 3 == 1
        v = rng.standard_normal(n)
        ext, mag = TR.simpson38_extended(v, 0.37)
        assert abs(LD(TR.simpson38_parallel(v, 0.37)) - ext) <= TR.parallel_roundings(n) * EPS64 * mag, n


def test_stop_test_is_the_reference_one():
    """StopTest against ScfRef's own flags along a converging H run (the reference's rule needs two converged steps in a row)"""
    ref = SR.ScfRef(1, [(0, 0, 1.0)], None, functional=SR.VWN, **GRID)
    st = TR.StopTest()
    for step in range(60):
        en = ref.step()
        st.step(en[0], 1 if ref.finished else ref.lastTimeConverged)        # a finishing step had converged levels; else the flag is kept
        assert st.finished == ref.finished and (ref.finished or st.Eold == ref.Eold), step
        if ref.finished:
            break
    assert ref.finished and step > 5
    print("H meets the stop test in step %d" % (step + 1))
