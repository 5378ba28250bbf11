"""CPU anchors of tests/_scf_ref.py, the step reference that test_gpu_scf_ref.py holds the PW92 / PBE / fractional-occupation SCF
to: with VWN and integer occupations it returns the bits of _ion_ref.IonScf (which test_ion_ref.py pins to dfo_scf_step); its
Poisson restatement returns the bits of dfo_solve_poisson_nonuniform at integer boundaries and is linear in the boundary value; PW92
stays within 1 mHa per electron of VWN."""
import numpy as np
import pytest

import _gga_ref as R
import _ion_ref as IR
import _oracle as O
import _scf_ref as SR

GRID = dict(mg_levels=12, MaxR=25.0, delta=2e-3)
CASES = [("Ne LDA", 10, 0, False), ("N LSDA", 7, 0, True), ("Na+ LDA", 11, 1, False)]


def _floats(levels):
    return None if levels is None else [(n, l, float(f)) for n, l, f in levels]


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_vwn_integer_occupations_are_ionscf_bits(case):
    _, Z, q, lsda = case
    a, b = IR.ion_levels(Z, q, lsda)
    ion = IR.IonScf(Z, a, b, chained=3, **GRID)
    ref = SR.ScfRef(Z, _floats(a), _floats(b), functional=SR.VWN, **GRID)
    try:
        assert ref.Ne == ion.Ne
        assert np.array_equal(ref.U, ion.U) and np.array_equal(ref.potA, ion.potA) and np.array_equal(ref.potB, ion.potB)
        for _ in range(3):
            want, got = ion.step(), ref.step()
            assert got == want, (got, want)
            for sp in range(2 if lsda else 1):
                assert np.array_equal(ref.levels(sp), ion.levels(sp))
            for name in ("density", "dA", "dB", "U", "potA", "potB", "Vexc", "eexc"):
                assert np.array_equal(getattr(ref, name), getattr(ion, name)), name
            assert ref.finished == ion.finished
    finally:
        ion.close()
        ref.close()


def test_poisson_restatement():
    """the bits of dfo_solve_poisson_nonuniform at integer boundaries; U(rho, 17.5) = (U(rho, 17) + U(rho, 18)) / 2 within the
    project's Poisson gate 1e-10 Z (test_poisson_solve_vs_golden): the solve is linear in its boundary value"""
    o = O.oracle()
    L, d, Rm = 14, 5e-4, 25.0
    ref = SR.ScfRef(18, [(0, 0, 2.0)], None, mg_levels=L, MaxR=Rm, delta=d)
    try:
        r = ref.pos
        rho = R.neon_like(r) * 1.8
        rho[0] = 0.0
        U = {}
        for Ne in (17, 18):
            want = np.zeros(ref.N)
            ps = o.dfo_poisson_create(L, d)
            o.dfo_solve_poisson_nonuniform(ps, Ne, Rm, O.dp(rho), O.dp(want))
            o.dfo_poisson_destroy(ps)
            U[Ne] = ref.poisson(rho, float(Ne))
            assert np.array_equal(U[Ne], want), Ne
            assert U[Ne][-1] == Ne and U[Ne][0] == 0
        half = ref.poisson(rho, 17.5)
        assert half[-1] == 17.5
        assert np.max(np.abs(half - 0.5 * (U[17] + U[18]))) <= 1e-10 * 18
    finally:
        ref.close()


@pytest.mark.parametrize("Z,lsda", [(10, False), (7, True)], ids=["Ne LDA", "N LSDA"])
def test_pw92_first_step_close_to_vwn(Z, lsda):
    """the first step under PW92 differs from VWN's by less than 1 mHa per electron (the bound of test_pw92_close_to_vwn), and does differ"""
    a, b = IR.ion_levels(Z, 0, lsda)
    e = {}
    for fx in (SR.VWN, SR.PW92):
        ref = SR.ScfRef(Z, _floats(a), _floats(b), functional=fx, **GRID)
        e[fx] = ref.step()
        ref.close()
    for x, y in zip(e[SR.VWN], e[SR.PW92]):
        assert 0 < abs(x - y) < 1e-3 * Z, (e[SR.VWN], e[SR.PW92])


def test_fractional_occupation_weights():
    """a fractional configuration runs: Sum f Psi^2 integrates to N_e (every Psi is normalised by the same rule) and the Poisson
    boundary is N_e; moving half an electron between two shells at a fixed electron count changes the step by far more than any
    gate (a wrong weight that conserves the count is visible to this reference)"""
    Z = 18
    cfgs = {"3p5.5": [(0, 0, 2.0), (1, 0, 2.0), (1, 1, 6.0), (2, 0, 2.0), (2, 1, 5.5)],
            "3s1.5 3p6": [(0, 0, 2.0), (1, 0, 2.0), (1, 1, 6.0), (2, 0, 1.5), (2, 1, 6.0)]}
    out = {}
    for name, cfg in cfgs.items():
        ref = SR.ScfRef(Z, cfg, None, functional=SR.PBE, **GRID)
        assert ref.Ne == 17.5 and ref.U[-1] == 17.5
        E, acc, eel, conv = ref.solve_levels(ref.potA, cfg)
        assert conv and eel == sum(f * e for (_, _, f), e in zip(cfg, E))
        total = ref.o.dfo_simpson38(1, O.dp(np.ascontiguousarray(acc * ref.cnst)), ref.N)
        assert abs(total - 17.5) <= 1e-12 * 17.5, total
        out[name] = ref.step()
        assert np.array_equal(ref.levels(0), E)
        ref.close()
    assert abs(out["3p5.5"][0] - out["3s1.5 3p6"][0]) > 1e-3
