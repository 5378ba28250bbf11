"""CPU suite: tests/_orb_ref.py -- the longdouble reference of the orbital expectation values and r^k matrix elements -- against the
closed forms of hydrogen-like orbitals, on analytic u_nl evaluated in longdouble:

    <1/r> = Z / n^2,  <r> = (3 n^2 - l(l+1)) / (2 Z),  <r^2> = n^2 (5 n^2 + 1 - 3 l(l+1)) / (2 Z^2),
    <r^4> = n^4 (63 n^4 - 35 n^2 (2 l(l+1) - 3) + 5 l(l+1) (3 l(l+1) - 10) + 12) / (8 Z^4),
    <1/r^3> = Z^3 / (n^3 l (l + 1/2) (l + 1)),  T = Z^2 / (2 n^2),  <1s|2s> = 0,  <1s| r |2p> = 128 sqrt(6) / (243 Z)

(n: the principal quantum number).  The file MEASURES the distance of every quantity from its closed form on four grids and holds
each to the figure written into _orb_ref.MEASURED: not above it, and the figure not more than 1.2 x the measurement (or the
floor 1e-17 of the longdouble evaluation).  What the figures say: on the logarithmic grids the moments of the Z = 10 orbitals
sit at 1e-14 or below and T -- the five-point derivative -- at 2e-10 (4097 nodes), 2e-11 (8193), 3e-12 (16 385); the 3d orbital of
Z = 2 is limited by its truncation at Rmax = 25 (8e-9 in NORM, 2e-6 in <r^4>, the same on every grid); the uniform grid of 8193
nodes resolves the 1s orbital of Z = 10 with 30 nodes per bohr radius / Z: 5e-7 in NORM, 3e-5 in T.
"""
import numpy as np
import pytest

import _orb_ref as R

LD = R.LD


@pytest.fixture(scope="module")
def tables():
    assert np.finfo(LD).eps < 1.2e-19, "this reference needs an extended np.longdouble"
    return {name: R.grid(*spec) for name, spec in R.GRIDS.items()}


def _held(measured, figure, what):
    print("%-40s measured %.3e  figure %.1e" % (what, measured, figure))
    assert measured <= figure, (what, measured, figure)
    assert figure <= max(1.2 * measured, R.FLOOR), (what, measured, figure)


def test_weights_are_simpson38():
    """Integral::Simpson38's sums (Integral.h:50-73), term by term, on N = 10: end nodes 1, nodes 3 and 6 2, the others 3, times 3/8"""
    w = R.weights(10) * LD(8) / LD(3)
    assert [int(x) for x in w] == [1, 3, 3, 2, 3, 3, 2, 3, 3, 1]
    f = np.arange(10, dtype=LD) ** 3                     # the rule is exact for cubics where N - 1 is a multiple of 3
    assert abs(np.sum(R.weights(10) * f) - LD(9) ** 4 / 4) < 1e-15 * 9 ** 4


def test_closed_form_of_r4_against_quadrature_free_values():
    """Z = 1: u_1s^2 = 4 r^2 e^{-2r}, <r^4> = 4 * 6! / 2^7 = 22.5; u_2p^2 = r^4 e^{-r} / 24, <r^4> = 8! / 24 = 1680 (Int r^n e^{-ar} = n! / a^(n+1))"""
    assert R.closed_forms(1, 0, 1)[R.R4] == LD(45) / 2
    assert R.closed_forms(2, 1, 1)[R.R4] == LD(1680)


@pytest.mark.parametrize("name", sorted(R.GRIDS))
def test_properties_against_closed_forms(tables, name):
    r, s = tables[name]
    for nlZ in R.ORBITALS:
        n, l, Z = nlZ
        u = R.hydrogenic_u(n, l, Z, r)
        props, mag = R.properties(u, l, r, s)
        closed = R.closed_forms(n, l, Z)
        assert sorted(closed) == sorted(R.MEASURED[name][nlZ])
        for c, v in closed.items():
            _held(float(abs(props[c] - v) / abs(v)), R.MEASURED[name][nlZ][c], "%s %s %s" % (name, nlZ, R.COLUMNS[c]))
            assert mag[c] >= abs(props[c])
        if l == 0:
            assert props[R.RM3] == 0
        # RPEAK is a node: the one next to the analytic maximum of |u| (1s: r = 1 / Z)
        i = int(np.argmax(np.abs(u)))
        assert props[R.RPEAK] == r[i] and abs(u[i]) >= max(abs(u[i - 1]), abs(u[i + 1]))
        if (n, l) == (1, 0):
            assert r[i - 1] < LD(1) / Z < r[i + 1]


@pytest.mark.parametrize("name", sorted(R.GRIDS))
def test_overlap_and_dipole_against_closed_forms(tables, name):
    r, s = tables[name]
    U = np.array([R.hydrogenic_u(n, l, Z, r) for n, l, Z in R.PAIR])
    M0, mag0 = R.matrix(U, 0, r, s)
    M1, _ = R.matrix(U, 1, r, s)
    M2, _ = R.matrix(U, 2, r, s)
    d = R.DIPOLE_1S_2P(10)
    _held(float(abs(M0[0, 1])), R.MEASURED[name]["S12"], name + " <1s|2s>")
    _held(float(abs(M1[0, 2] - d) / d), R.MEASURED[name]["D"], name + " <1s|r|2p>")
    for M in (M0, M1, M2):
        assert np.array_equal(M, M.T)
    # the diagonals are the property columns: the same weighted terms, the same (longdouble) sum
    for a, (n, l, Z) in enumerate(R.PAIR):
        props, _ = R.properties(U[a], l, r, s)
        for M, c in ((M0, R.NORM), (M1, R.R1), (M2, R.R2)):
            assert abs(M[a, a] - props[c]) <= 1e-17 * abs(props[c])
    assert np.all(mag0 >= np.abs(M0))


def test_derivative_stencils():
    """du/di of the header: exact on cubics inside (five points), on quadratics at the four end nodes; D >= |du/di|"""
    i = np.arange(12, dtype=LD)
    du, D = R.du_di(2 + 3 * i - i * i)
    assert np.max(np.abs(du - (3 - 2 * i))) < 1e-17
    du3, _ = R.du_di(i ** 3)
    assert np.max(np.abs(du3[2:-2] - 3 * i[2:-2] ** 2)) < 1e-16
    assert np.all(D >= np.abs(du))


def test_rounding_counts():
    assert R.prop_roundings(4097) == 13 + 4 * 5 + 10 and R.prop_roundings(131073) == 13 + 4 * 129 + 10
    assert R.matrix_roundings(4097) == 8 + 512 + 9 + 1


def test_front_end_usage_names_the_orbital_table():
    """dftatom_cli without arguments (no GPU needed): the usage text names --orbital-table"""
    import os
    import subprocess
    compat = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "dftatom_amd", "compat")
    exe = os.path.join(compat, "dftatom_cli")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-C", compat])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "--orbital-table" in r.stderr
