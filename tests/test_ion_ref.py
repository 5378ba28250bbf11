"""CPU check of the cation oracle tests/_ion_ref.py: at charge 0 its restatement of dfo_scf_step (Z and N_e kept apart) returns the
oracle's own bits -- energies, eigenvalues, density and U -- for Ne LDA and N LSDA over three steps."""
import ctypes as C

import numpy as np
import pytest

import _ion_ref as IR
import _oracle as O


@pytest.mark.parametrize("Z, lsda", [(10, False), (7, True)], ids=["Ne LDA", "N LSDA"])
def test_restatement_at_charge_zero_is_dfo_scf_step(Z, lsda):
    o = O.oracle()
    L, d, R = 12, 2e-3, 25.0
    s = o.dfo_scf_create(int(lsda), Z, L, 0.5, R, d, 3)
    a, b = IR.ion_levels(Z, 0, lsda)
    ion = IR.IonScf(Z, a, b, mg_levels=L, MaxR=R, delta=d, chained=3)
    N = ion.N
    try:
        for _ in range(3):
            e = O.Energies()
            o.dfo_scf_step(s, C.byref(e))
            got = ion.step()
            want = [e.Etotal, e.Ekinetic, e.Ecoul, e.Enuclear, e.Exc]
            assert np.array_equal(np.array(got), np.array(want)), (got, want)
            la = np.array([s.contents.la[k].E for k in range(s.contents.nla)])
            lb = np.array([s.contents.lb[k].E for k in range(s.contents.nlb)])
            assert np.array_equal(ion.levels(0), la)
            assert np.array_equal(ion.levels(1) if lsda else lb, lb)
            assert np.array_equal(np.ctypeslib.as_array(s.contents.density, (N,)), ion.density)
            assert np.array_equal(np.ctypeslib.as_array(s.contents.U, (N,)), ion.U)
            assert np.array_equal(np.ctypeslib.as_array(s.contents.potA, (N,)), ion.potA)
    finally:
        o.dfo_scf_destroy(s)
        ion.close()
