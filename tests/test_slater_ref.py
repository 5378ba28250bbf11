"""CPU suite: tests/_slater_ref.py -- the longdouble reference of the Slater integrals R^k(ab,cd) -- against the closed forms of
hydrogen-like orbitals (in units of Z):

    F0(1s,1s) = 5/8      F0(1s,2s) = 17/81    G0(1s,2s) = 16/729   F0(2s,2s) = 77/512   F0(1s,2p) = 59/243
    G1(1s,2p) = 112/2187 F0(2s,2p) = 83/512   G1(2s,2p) = 45/512   F0(2p,2p) = 93/512   F2(2p,2p) = 45/512

The file MEASURES the reference's distance from each on four grids and holds it to the figure written into _slater_ref.MEASURED (not
above it, the figure not more than 1.2 x the measurement); the figures themselves may not exceed 1e-11 (4097 logarithmic nodes) and
4e-6 (8193 uniform nodes).  A float64 model of the reference -- sequential cumulative sums, the worst chain -- stays within the rounding
bound counted from the kernel's shape.  The host-only entries of the library (the angular factor, the job table) and the two energy
sums are checked here too: no GPU is needed for any of it.
"""
from fractions import Fraction

import numpy as np
import pytest

import _orb_ref as O
import _slater_ref as S
import dftatom_amd as D

LD, EPS = S.LD, S.EPS
GRIDS = ("log12", "log13", "log14", "uni13")


@pytest.fixture(scope="module")
def tables():
    assert np.finfo(LD).eps < 1.2e-19, "this reference needs an extended np.longdouble"
    out = {}
    for name in GRIDS:
        r, s = O.grid(*O.GRIDS[name])
        out[name] = (r, s, S.orbitals(r))
    return out


def _job(U, job, r, s, dtype=LD):
    a, b, c, d, k = job
    return S.rk(U[a], U[b], U[c], U[d], k, r, s, dtype=dtype)


@pytest.mark.parametrize("name", GRIDS)
def test_reference_against_closed_forms(tables, name):
    r, s, U = tables[name]
    assert sorted(S.MEASURED[name]) == sorted(nm for nm, _, _ in S.CLOSED)
    for nm, job, cf in S.CLOSED:
        val, mag = _job(U, job, r, s)
        closed = LD(S.ZREF) * LD(cf.numerator) / LD(cf.denominator)
        measured, figure = float(abs(val - closed) / closed), S.MEASURED[name][nm]
        print("%-6s %-10s measured %.3e  figure %.1e" % (name, nm, measured, figure))
        assert measured <= figure <= 1.2 * measured, (name, nm, measured, figure)
        assert mag >= abs(val)


def test_measured_figures_cannot_be_loosened():
    assert max(S.MEASURED["log12"].values()) <= 1e-11
    assert max(S.MEASURED["uni13"].values()) <= 4e-6
    assert S.MEASURED["hartree"][12] >= 8 * S.MEASURED["hartree"][14] > 0      # the multigrid is second order: 4x the nodes, 16x less


def test_symmetries_of_the_reference(tables):
    r, s, U = tables["log12"]
    a, b, c, d, k = S.P2, S.D3, S.D3, S.F4, 1
    base = S.rk(U[a], U[b], U[c], U[d], k, r, s)[0]
    for other in ((c, b, a, d), (a, d, c, b), (b, a, d, c)):
        v = S.rk(*(U[x] for x in other), k, r, s)[0]
        assert abs(v - base) <= 1e-17 * abs(base)


@pytest.mark.parametrize("name", ["log12", "log13", "uni13"])
def test_float64_model_within_the_counted_bound(tables, name):
    r, s, U = tables[name]
    U64 = U.astype(np.float64)
    c = S.rk_roundings(len(r))
    assert len(S.MODEL) == 9
    worst = 0.0
    for nm, job in S.MODEL:
        ref, mag = _job(U64, job, r, s)
        model, _ = _job(U64, job, r.astype(np.float64), s.astype(np.float64), dtype=np.float64)
        ratio = float(abs(LD(model) - ref) / (c * EPS * mag))
        worst = max(worst, ratio)
        assert ratio <= 1, (name, nm, ratio)
    print("%s: float64 model at %.3f of the bound (c = %d)" % (name, worst, c))


def test_rounding_counts():
    # inner 14, stencil 4, scan 15 + tiles, outer 19, tree 9 + 4 tiles at k = 8
    assert S.rk_roundings(4097) == 14 + 4 + (15 + 5) + 19 + (9 + 20) == 86
    assert S.rk_roundings(8193) == 106 and S.rk_roundings(5, k=0) == S.rk_roundings(5) - 16


def test_increment_stencils():
    """exact on cubics: the cumulative integral of i^3 over unit steps is i^4 / 4"""
    i = np.arange(12, dtype=LD)
    d, Dm = S.increments(i ** 3)
    assert np.max(np.abs(np.cumsum(d) - i ** 4 / 4)) < 1e-15 * 11 ** 4
    assert np.all(Dm >= np.abs(d))


# ---- the host-only entries of the library ---------------------------------------------------------------------------------------------
def test_gaunt_against_exact_rationals():
    exact = {(1, 2, 1): Fraction(2, 15), (2, 2, 2): Fraction(2, 35), (2, 4, 2): Fraction(2, 35), (1, 3, 2): Fraction(3, 35),
             (2, 1, 3): Fraction(3, 35), (3, 2, 3): Fraction(4, 105), (2, 3, 3): Fraction(4, 105), (3, 4, 3): Fraction(2, 77),
             (3, 6, 3): Fraction(100, 3003), (2, 5, 3): Fraction(10, 231)}
    for k in range(5):
        exact[(0, k, k)] = Fraction(1, 2 * k + 1)
    for (la, k, lb), v in exact.items():
        got = D.gaunt_3j2(la, k, lb)
        assert abs(got - float(v)) <= 2 * EPS * float(v), (la, k, lb, got, v)
        assert S.gaunt_3j2(la, k, lb) == v
    for la, k, lb in ((1, 1, 1), (2, 3, 2), (0, 1, 0)):          # parity
        assert D.gaunt_3j2(la, k, lb) == 0.0
    for la, k, lb in ((1, 4, 1), (0, 2, 0), (3, 0, 1), (4, 12, 4)):   # triangle
        assert D.gaunt_3j2(la, k, lb) == 0.0
    lib = D.load()
    import ctypes as C
    out = C.c_double(7.0)
    for la, k, lb in ((-1, 0, 1), (0, -2, 0), (1, 0, -1), (5, 0, 5), (0, 5, 5)):
        assert lib.dfta_gaunt_3j2(la, k, lb, C.byref(out)) == 1 and out.value == 7.0
    assert lib.dfta_gaunt_3j2(1, 0, 1, None) == 1


def test_gaunt_against_sympy():
    wigner = pytest.importorskip("sympy.physics.wigner")
    import sympy
    for la in range(5):
        for lb in range(5):
            for k in range(S.KMAX + 1):
                v = sympy.nsimplify(wigner.wigner_3j(la, k, lb, 0, 0, 0) ** 2)
                want = Fraction(int(v.p), int(v.q))
                assert S.gaunt_3j2(la, k, lb) == want, (la, k, lb)
                assert abs(D.gaunt_3j2(la, k, lb) - float(want)) <= 2 * EPS * float(want), (la, k, lb)


def _expected_jobs(l):
    rows, kinds = [], []
    n = len(l)
    for a in range(n):
        for b in range(a, n):
            for k in range(0, 2 * min(l[a], l[b]) + 1, 2):
                rows.append((a, b, a, b, k)); kinds.append(D.SLATER_F)
    for a in range(n):
        for b in range(a + 1, n):
            for k in S.exchange_ks(l[a], l[b]):
                rows.append((a, b, b, a, k)); kinds.append(D.SLATER_G)
    return rows, kinds


def test_fg_job_tables():
    lib = D.load()
    jobs, kinds = D.slater_fg_jobs([0])
    assert jobs.tolist() == [[0, 0, 0, 0, 0]] and kinds.tolist() == [D.SLATER_F]
    jobs, kinds = D.slater_fg_jobs([0, 0, 1])
    assert jobs.tolist() == [[0, 0, 0, 0, 0], [0, 1, 0, 1, 0], [0, 2, 0, 2, 0], [1, 1, 1, 1, 0], [1, 2, 1, 2, 0], [2, 2, 2, 2, 0],
                             [2, 2, 2, 2, 2], [0, 1, 1, 0, 0], [0, 2, 2, 0, 1], [1, 2, 2, 1, 1]]
    assert kinds.tolist() == [0] * 7 + [1] * 3
    # radon's levels (15 subshells) and, for a table of 19 levels with every l up to 3, oganesson's
    for Z, nlev in ((86, 15), (118, 19)):
        lz = [l for _, l, _ in D.get_subshells(Z)]
        assert len(lz) == nlev
        jobs, kinds = D.slater_fg_jobs(lz)
        rows, want_kinds = _expected_jobs(lz)
        assert [tuple(x) for x in jobs.tolist()] == rows and kinds.tolist() == want_kinds
        l32 = np.array(lz, np.int32)
        assert lib.dfta_slater_fg_jobs(nlev, l32.ctypes.data_as(D.c_ip), None, None) == len(rows)       # count only
        for (a, b, c, d, k), kind in zip(rows, want_kinds):             # every k admissible: F: (la k la)(lb k lb), G: (la k lb)
            la, lb = lz[a], lz[b]
            assert 0 <= k <= D.SLATER_KMAX
            assert (S.gaunt_3j2(la, k, lb) if kind else S.gaunt_3j2(la, k, la) * S.gaunt_3j2(lb, k, lb)) > 0
    assert lib.dfta_slater_fg_jobs(0, None, None, None) == 0
    bad = np.array([0, 5], np.int32)
    assert lib.dfta_slater_fg_jobs(2, bad.ctypes.data_as(D.c_ip), None, None) == -1
    assert lib.dfta_slater_fg_jobs(-1, bad.ctypes.data_as(D.c_ip), None, None) == -1
    with pytest.raises(D.DftaError):
        D.slater_fg_jobs([0, -1])


# ---- the energy sums ------------------------------------------------------------------------------------------------------------------
def test_energy_sums_one_electron_and_closed_1s(tables):
    r, s, U = tables["log12"]
    F0, G, _, _ = S.tables(U[:1], [0], r, s)
    eh, ex = S.energy_sums([0], [1.0], 1, True, F0, G, dtype=LD)              # one electron, one channel: no self-interaction
    assert eh > 0 and abs(ex + eh) <= 1e-18 * eh
    eh, ex = S.energy_sums([0], [2.0], 1, False, F0, G, dtype=LD)             # 1s2: exchange cancels half the Hartree energy
    assert abs(ex + eh / 2) <= 1e-18 * eh
    assert abs(eh - 2 * F0[0, 0]) <= 1e-18 * eh
    # the same closed shell as two LSDA channels
    U2 = np.array([U[0], U[0]])
    F0, G, _, _ = S.tables(U2, [0, 0], r, s, nA=1)
    eh2, ex2 = S.energy_sums([0, 0], [1.0, 1.0], 1, True, F0, G, dtype=LD)
    assert abs(eh2 - eh) <= 1e-18 * eh and abs(ex2 - ex) <= 1e-18 * eh


def test_closed_shell_reduction_of_the_exchange_sum():
    """Ne-like closed shells: E_x = -[F0(1s,1s) + F0(2s,2s) + 2 G0(1s,2s) + 2 G1(1s,2p) + 2 G1(2s,2p) + 3 F0(2p,2p) + 6/5 F2(2p,2p)],
    the textbook average-of-configuration coefficients (with the Hartree term 18 F0(2p,2p): 15 F0 - 30 F_2, F_2 = F2 / 25, for 2p6)"""
    l, occ = [0, 0, 1], [2.0, 2.0, 6.0]
    F0 = np.zeros((3, 3), dtype=LD)
    coef = {}
    for (a, b, k) in ((0, 0, 0), (1, 1, 0), (2, 2, 0), (2, 2, 2), (0, 1, 0), (0, 2, 1), (1, 2, 1)):
        G = np.zeros((S.KMAX + 1, 3, 3), dtype=LD)
        G[k, a, b] = G[k, b, a] = 1
        coef[(a, b, k)] = S.energy_sums(l, occ, 3, False, F0, G, dtype=LD)[1]
    want = {(0, 0, 0): -1, (1, 1, 0): -1, (2, 2, 0): -3, (2, 2, 2): LD(-6) / 5, (0, 1, 0): -2, (0, 2, 1): -2, (1, 2, 1): -2}
    for key, v in want.items():
        assert abs(coef[key] - v) <= 1e-18, (key, coef[key], v)


def test_hartree_gap_figures():
    """E_H from F^0 against 2 pi Q[r rho U s] with the oracle's multigrid on the hydrogenic 1s2 2s2 2p6 density of Z = 10: the stored
    figures hold the measured gap (discretisation of the second-order multigrid)"""
    import _scf_ref as SR
    for L, spec in S.HARTREE_GRIDS.items():
        r, s = O.grid(*spec)
        U, l, occ = S.orbitals(r)[:3], [0, 0, 1], [2.0, 2.0, 6.0]
        F0, G, _, _ = S.tables(U, l, r, s)
        eh = float(S.energy_sums(l, occ, 3, False, F0, G, dtype=LD)[0])
        ref = SR.ScfRef(10, [(0, 0, 2.0), (1, 0, 2.0), (1, 1, 6.0)], mg_levels=spec[0], MaxR=spec[2], delta=spec[1])
        try:
            e2 = S.hartree_from_density(U, occ, r, s, ref.poisson)
        finally:
            ref.close()
        gap, figure = abs(e2 - eh) / eh, S.MEASURED["hartree"][L]
        print("%d levels: E_H %.12f, from the multigrid %.12f, gap %.3e, figure %.1e" % (L, eh, e2, gap, figure))
        assert gap <= figure <= 1.2 * gap, (L, gap, figure)


def test_host_planner_stand_alone_under_sanitizers(tmp_path):
    """dftatom_amd/csrc/slater_plan.cpp is pure host code: a stand-alone program (tests/slater_plan_main.cpp) built with ASan + UBSan
    walks the angular factor's argument ranges, the job tables of 19 levels and the energy plans; its sums with every integral = 1:
    E_H = (Sum N)^2 / 2, E_x = -1/2 Sum_sigma Sum_ab n_a n_b Sum_k (la k lb)^2"""
    import os
    import shutil
    import subprocess
    here = os.path.dirname(os.path.abspath(__file__))
    csrc = os.path.join(here, "..", "dftatom_amd", "csrc")
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler is needed"
    exe = str(tmp_path / "slater_plan_main")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", csrc, "-o", exe,
                    os.path.join(here, "slater_plan_main.cpp"), os.path.join(csrc, "slater_plan.cpp")], check=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout, r.stderr)
    l = [x for _, x, _ in D.get_subshells(118)]
    first, second = (ln.split() for ln in r.stdout.strip().split("\n"))
    assert int(first[1]) == len(D.slater_fg_jobs(l)[0])
    occ = [1.5] * 19
    ones = np.ones((19, 19))
    G = np.ones((S.KMAX + 1, 19, 19))
    eh, ex = S.energy_sums(l, occ, 12, True, ones, G)
    assert float(first[4]) == eh and float(first[5]) == ex and eh == (19 * 1.5) ** 2 / 2
    eh, ex = S.energy_sums(l, occ, 19, False, ones, G)
    assert float(second[2]) == eh and float(second[3]) == ex


def test_front_end_usage_names_the_slater_table():
    """dftatom_cli without arguments (no GPU needed): the usage text names --slater-table"""
    import os
    import subprocess
    compat = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "dftatom_amd", "compat")
    exe = os.path.join(compat, "dftatom_cli")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-C", compat])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "--slater-table" in r.stderr
