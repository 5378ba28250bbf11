"""CPU suite: tests/_exchange_ref.py -- the longdouble reference of the screening functions y^k_xy = Y^k_xy / r and of the exchange
potentials built on them -- against the closed forms of hydrogen-like orbitals, which sympy derives from the definition

    y^k(r) = r^(-k-1) Int_0^r t^k P(t) dt + r^k Int_r^oo t^(-k-1) P(t) dt,      y^0_1s1s(r) = [1 - e^(-2Zr) (1 + Zr)] / r.

The file MEASURES the reference's distance from each closed form on two grids and holds it to the figure written into
_exchange_ref.MEASURED (not above it, the figure not more than 1.2 x the measurement).  A float64 model of the reference -- sequential
cumulative sums, the worst chain -- stays within the rounding bound counted from the kernel's shape, and two wrong reverse scans miss
that bound by orders of magnitude.  The identities of the header hold in longdouble at their rounding level -- but for Sum n vbarHF =
2 E_x, which compares two discretisations of one integral and is held to its measured gap.  The host planner is
checked against a Python statement, through the library and through a stand-alone program built with ASan + UBSan.  No GPU is needed.
"""
import os
import re

import numpy as np
import pytest

import _exchange_ref as X
import _orb_ref as O
import _slater_ref as S
import dftatom_amd as D

LD, EPS = X.LD, X.EPS
GRIDS = ("log13", "uni13")
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
NE = ([0, 0, 1], [1.0, 1.0, 3.0])        # the closed shells of neon as one LDA channel: l, channel occupations


@pytest.fixture(scope="module")
def tables():
    assert np.finfo(LD).eps < 1.2e-19, "this reference needs an extended np.longdouble"
    out = {}
    for name in GRIDS + ("log12",):
        r, s = O.grid(*O.GRIDS[name])
        out[name] = (r, s, S.orbitals(r))
    return out


@pytest.fixture(scope="module")
def neon(tables):
    """the reference's potentials of hydrogenic 1s 2s 2p (Z = 10) with neon's channel occupations, HOMO 2p, at 4097 nodes"""
    r, s, U = tables["log12"]
    return X.potentials(U[:3], NE[0], NE[1], 2, r, s)


# ---- the reference against the closed forms ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", GRIDS)
def test_reference_against_closed_forms(tables, name):
    r, s, U = tables[name]
    assert sorted(X.MEASURED[name]) == sorted(nm for nm, _, _ in X.CLOSED)
    for nm, (x, y, k), spec in X.CLOSED:
        val, mag = X.yk(U[x], U[y], k, r, s)
        closed = X.closed_yk(spec, S.ZREF, r)
        assert np.all(closed[1:] > 0) and np.all(mag >= np.abs(val))
        measured, figure = float(np.max(np.abs(val - closed)) / np.max(closed)), X.MEASURED[name][nm]
        print("%-6s %-10s measured %.3e  figure %.1e" % (name, nm, measured, figure))
        assert measured <= figure <= 1.2 * measured, (name, nm, measured, figure)


def test_measured_figures_cannot_be_loosened():
    assert max(X.MEASURED["log13"].values()) <= 2e-12 and max(X.MEASURED["uni13"].values()) <= 5e-5
    assert 0 < X.MEASURED["ex_identity"]["log12"] <= 1e-14
    assert 0 < X.MEASURED["hartree"][12] <= 1e-6 and all(0 < v <= 0.05 for v in X.MEASURED["tail"].values())


def test_sympy_route_reproduces_the_textbook_form(tables):
    r = tables["log13"][0]
    a, b = X.closed_yk(X.CLOSED[0][2], S.ZREF, r), X.y0_1s1s(S.ZREF, r)
    assert np.max(np.abs(a - b) / b) < 1e-17
    import sympy as sp
    expr, Z, rs = X.closed_expr(1, 0, 1, 0, 0)
    assert sp.simplify(expr - (1 - sp.exp(-2 * Z * rs) * (1 + Z * rs)) / rs) == 0


# ---- the counted bound: the float64 model inside it, two wrong scans far outside ---------------------------------------------------------
def _pairs(U):
    jobs = [j for _, j, _ in X.CLOSED] + [j for _, j in X.EXTRA]
    return [(nm, U[x], U[y], k) for (nm, (x, y, k)) in zip([c[0] for c in X.CLOSED] + [e[0] for e in X.EXTRA], jobs)]


@pytest.mark.parametrize("name", ["log12", "log13", "uni13"])
def test_float64_model_within_the_counted_bound(tables, name):
    r, s, U = tables[name]
    U64 = U.astype(np.float64)
    worst = 0.0
    for nm, ux, uy, k in _pairs(U64):
        c = X.yk_roundings(len(r), k)
        ref, mag = X.yk(ux, uy, k, r, s)
        model, _ = X.yk(ux, uy, k, r.astype(np.float64), s.astype(np.float64), dtype=np.float64)
        ok = mag > 0
        ratio = float(np.max(np.abs(model.astype(LD) - ref)[ok] / (c * EPS * mag[ok])))
        assert np.all(model[~ok] == 0)
        worst = max(worst, ratio)
        assert ratio <= 1, (name, nm, ratio)
    print("%s: float64 model at %.3f of the bound" % (name, worst))


@pytest.mark.parametrize("levels", [3, 4, 10, 11])
@pytest.mark.parametrize("model", ["no_end_stencil", "start_N2"])
def test_wrong_reverse_scans_miss_the_bound(levels, model):
    """the reverse scan's end: the end stencil of node N-1, and W_{N-1} = 0 with e_{N-1} inside W_{N-2}.  Orbitals that are not small at the
    outer end of a uniform grid: either mistake moves y by far more than the counted bound allows (which the right model meets)"""
    r, s = O.grid(levels, None, 10.0)
    u = X.smooth_orbitals(r)
    for x, y, k in ((0, 0, 0), (0, 1, 0), (2, 3, 1), (1, 1, 2)):
        c = X.yk_roundings(len(r), k)
        ref, mag = X.yk(u[x], u[y], k, r, s)
        good, _ = X.yk(u[x], u[y], k, r.astype(np.float64), s.astype(np.float64), dtype=np.float64)
        wrong, _ = X.yk(u[x], u[y], k, r.astype(np.float64), s.astype(np.float64), dtype=np.float64, model=model)
        rg = float(np.max(np.abs(good.astype(LD) - ref)[1:] / (c * EPS * mag[1:])))
        rw = float(np.max(np.abs(wrong.astype(LD) - ref)[1:] / (c * EPS * mag[1:])))
        assert rg <= 1 and rw >= 1e3, (levels, model, (x, y, k), rg, rw)


def test_rounding_counts():
    assert X.yk_roundings(4097, 0) == 29 + 5 and X.yk_roundings(4097) == 45 + 5 and X.yk_roundings(8193, 8) == 54
    assert X.yk_roundings(9, 0) == 30 and X.yk_roundings(1025, 0) == 31
    assert X.red_roundings(4097, X.HF) == 6 + 17 + 9 and X.red_roundings(4097, X.SL) == 33 == X.red_roundings(4097, X.KLI)
    assert X.red_roundings(4097, X.PAIR) == 35 and X.red_roundings(131073, X.PAIR) == 9 + 513 + 9


def test_symmetry_and_zero_rows_of_the_reference(tables):
    r, s, U = tables["log12"]
    a, _ = X.yk(U[S.P2], U[S.D3], 1, r, s)
    b, _ = X.yk(U[S.D3], U[S.P2], 1, r, s)
    assert np.array_equal(a, b)
    z, zm = X.yk(U[S.P2], np.zeros(len(r)), 1, r, s)
    assert not np.any(z) and not np.any(zm)
    assert a[0] == 0 and a[-1] == (np.cumsum(S.increments(r * (U[S.P2] * U[S.D3]) * s)[0])[-1]) / (r[-1] * r[-1])    # W_{N-1} = 0


# ---- against the Slater integrals ---------------------------------------------------------------------------------------------------------
def test_quadrature_of_the_screening_function_against_rk(tables):
    """Q[P_ac y^k_bd s] and _slater_ref.rk(a, b, c, d, k) discretise the same double integral in two ways (the reverse scan W on one side,
    the two regions swapped into forward scans on the other), so they differ by discretisation, not rounding.  The two bounds: each
    side's own measured distance from the exact value -- _slater_ref.MEASURED of the integral, relative, and _exchange_ref.MEASURED
    of the row (an error of y at every node, relative to the row's peak) times max |y| Q[|P| s]."""
    link = {"F0(1s,1s)": "y0(1s,1s)", "F0(2s,2s)": "y0(2s,2s)", "F0(2p,2p)": "y0(2p,2p)", "F2(2p,2p)": "y2(2p,2p)", "G1(1s,2p)": "y1(1s,2p)"}
    jobs = {nm: job for nm, job, _ in S.CLOSED}
    worst = 0.0
    for name in GRIDS:
        r, s, U = tables[name]
        for fname, yname in link.items():
            a, b, c, d, k = jobs[fname]
            y, _ = X.yk(U[b], U[d], k, r, s)
            P = U[a] * U[c]
            q, _ = X.quad(P * y * s)
            val, _ = S.rk(U[a], U[b], U[c], U[d], k, r, s)
            bound = S.MEASURED[name][fname] * abs(val) + X.MEASURED[name][yname] * np.max(np.abs(y)) * X.quad(P * s)[1]
            worst = max(worst, float(abs(q - val) / bound))
            assert abs(q - val) <= bound, (name, fname, float(q), float(val), float(abs(q - val) / bound))
    print("Q[P y s] against rk: %.3f of the two bounds" % worst)


# ---- the identities of the header, in longdouble ----------------------------------------------------------------------------------------------
def test_identities_in_longdouble(tables, neon):
    r, s, U = tables["log12"]
    l, occ = NE
    n = np.array(occ, dtype=LD)
    p = neon
    red = p["red"]
    tiny = 64 * np.finfo(LD).eps
    # Sum n vbarHF = 2 E_x of the channel: E_x of the LDA atom is twice the channel's, so Sum n vbarHF = E_x(LDA)
    F0, G, _, _ = S.tables(U[:3], l, r, s)
    _, ex = S.energy_sums(l, [2 * x for x in occ], 3, False, F0, G, dtype=LD)
    lhs = np.sum(n * p["vbar"][:, X.HF])
    mag = np.sum(n * red["HF"][1])
    # the two sides discretise the double integral differently (see test_quadrature_of_the_screening_function_against_rk): the gap is
    # the grid's, far below what either side is from the exact value, and is held to its measured figure
    gap, figure = float(abs(lhs - ex) / abs(ex)), X.MEASURED["ex_identity"]["log12"]
    print("Sum n vbarHF = %.15f, 2 E_x of the channel = %.15f, gap %.3e, figure %.1e" % (float(lhs), float(ex), gap, figure))
    assert gap <= figure <= 1.2 * gap
    # Sum n vbarS = Sum n vbarHF: node by node n u^2 vS = -n u X sums to the same integrand, so this one holds at rounding level
    assert abs(np.sum(n * p["vbar"][:, X.SL]) - lhs) <= tiny * mag
    # Sum_b M_ab = NORM_a
    norm = np.array([X.quad(U[a] * U[a] * s)[0] for a in range(3)])
    for a in range(3):
        assert abs(np.sum(p["M"][a]) - norm[a]) <= tiny * norm[a]
    # the rows that were kept: vbarKLI_a - vbarHF_a = c_a
    h = 2
    scale = np.sum(np.abs(p["vbar"][:, [X.HF, X.SL, X.KLI]])) + np.sum(np.abs(p["c"]))
    for a in range(2):
        assert abs(p["vbar"][a, X.KLI] - p["vbar"][a, X.HF] - p["c"][a]) <= tiny * scale
    # the dropped HOMO row: summing the kept rows with n_a and Sum_a n_a M_ab = n_b NORM_b gives
    # n_h (vbarKLI_h - vbarHF_h) = Sum_{b != h} n_b c_b (NORM_b - 1) -- the row holds as far as the orbitals are normalised under Q
    rest = sum(n[b] * p["c"][b] * (norm[b] - 1) for b in range(2))
    assert abs(n[h] * (p["vbar"][h, X.KLI] - p["vbar"][h, X.HF]) - rest) <= tiny * scale
    assert abs(p["vbar"][h, X.KLI] - p["vbar"][h, X.HF]) <= 2 * O.MEASURED["log12"][(1, 0, 10)][O.NORM] * np.sum(n * np.abs(p["c"])) / n[h]
    ok = p["D"] > 0
    assert p["c"][h] == 0 and np.all(p["vS"][ok] < 0) and not np.any(p["vKLI"][~ok]) and np.count_nonzero(ok) > 4000
    print("neon-like channel: vbar (HF, S, c, KLI) =", np.array2string(p["vbar"].astype(np.float64), precision=6))


def test_one_electron_and_closed_1s_shell(tables):
    r, s, U = tables["log12"]
    y0, _ = X.yk(U[0], U[0], 0, r, s)
    for occ in (1.0, 0.37):                           # one electron (or less) in one channel: vS = vKLI = -n y^0, no self-interaction for n = 1
        p = X.potentials(U[:1], [0], [occ], 0, r, s)
        ok = p["D"] > 0
        assert np.max(np.abs(p["vS"][ok] + LD(occ) * y0[ok]) / (LD(occ) * y0[ok])) <= 8 * np.finfo(LD).eps
        assert np.array_equal(p["vKLI"], p["vS"]) and p["c"][0] == 0          # an empty system: bit for bit
    # 1s2 as an LDA channel (n = 1) and as an LSDA channel: vS = vKLI = -y^0_1s1s
    p = X.potentials(U[:1], [0], [1.0], 0, r, s)
    ok = p["D"] > 0
    assert np.max(np.abs(p["vKLI"][ok] + y0[ok]) / y0[ok]) <= 8 * np.finfo(LD).eps
    assert abs(p["vbar"][0, X.HF] - p["vbar"][0, X.SL]) <= 1e-17 and p["vbar"][0, X.KLI] == p["vbar"][0, X.SL]


# ---- discretisation figures that the GPU suite gates on --------------------------------------------------------------------------------------
def test_hartree_potential_gap_figure(tables):
    """Sum_a N_a y^0_aa r against U of the oracle's multigrid on the hydrogenic 1s2 2s2 2p6 density of Z = 10 at 4097 nodes"""
    import _scf_ref as SR
    r, s, U = tables["log12"]
    occ = [2.0, 2.0, 6.0]
    tot = sum(LD(n) * X.yk(U[a], U[a], 0, r, s)[0] for a, n in enumerate(occ)) * r
    r64 = r.astype(np.float64)
    acc = np.einsum("k,ki->i", np.array(occ), U[:3].astype(np.float64) ** 2)
    rho = np.zeros(len(r))
    rho[1:] = acc[1:] / (4 * np.pi * r64[1:] * r64[1:])
    ref = SR.ScfRef(10, [(0, 0, 2.0), (1, 0, 2.0), (1, 1, 6.0)], mg_levels=12, MaxR=25.0, delta=2e-3)
    try:
        UH = ref.poisson(rho, 10.0)
    finally:
        ref.close()
    gap, figure = float(np.max(np.abs(tot - UH))) / 10.0, X.MEASURED["hartree"][12]
    print("Hartree potential: max |Sum N y0 r - U| / N_e = %.3e, figure %.1e" % (gap, figure))
    assert gap <= figure <= 1.2 * gap


def oracle_orbitals(Z, alpha, beta, steps=3):
    """the orbitals of the CPU oracle's step `steps` (eigenfunctions of that step's input potential) at 4097 nodes: per channel
    (l, occupations, eigenvalues, U)"""
    import _scf_ref as SR
    ref = SR.ScfRef(Z, alpha, beta, mg_levels=12, MaxR=25.0, delta=2e-3)
    try:
        for _ in range(steps):
            pots = (ref.potA.copy(), ref.potB.copy())
            ref.step()
        out = []
        for sp, cfg in enumerate(ref.cfg):
            if cfg:
                pot = pots[sp] if ref.lsda else pots[0]
                out.append(([l for _, l, _ in cfg], [f for _, _, f in cfg], ref.E[sp].copy(),
                            np.array([ref.orbital(pot, l, E) for (_, l, _), E in zip(cfg, ref.E[sp])])))
    finally:
        ref.close()
    return out


def tail_value(p, r):
    """(r vKLI at the outermost node with D > 0, that node)"""
    i = int(np.nonzero(np.asarray(p["D"]) > 0)[0][-1])
    return float(r[i] * p["vKLI"][i]), i


TAIL_CASES = {"Ne": (10, [(0, 0, 2.0), (1, 0, 2.0), (1, 1, 6.0)], None, 0, 0.5),
              "N_alpha": (7, [(0, 0, 1.0), (1, 0, 1.0), (1, 1, 3.0)], [(0, 0, 1.0), (1, 0, 1.0)], 0, 1.0)}


@pytest.mark.parametrize("case", sorted(TAIL_CASES))
def test_kli_tail_figures(tables, case):
    """r vKLI at the outermost node with D > 0, on the CPU oracle's orbitals: where only the HOMO is left vKLI = vS = -n_h Sum_k c_hhk y^k_hh,
    which tends to -n_h / (2 l_h + 1) / r = -1 / r for a full HOMO shell; the distance from -1 at r ~ 25 is what <r^2> / r^2 leaves"""
    r, s, _ = tables["log12"]
    Z, alpha, beta, spin, scale = TAIL_CASES[case]
    l, occ, E, U = oracle_orbitals(Z, alpha, beta)[spin]
    occ = [scale * f for f in occ]
    h = X.pick_homo(E, occ)
    assert l[h] == 1 and occ[h] == 3.0
    p = X.potentials(U, l, occ, h, r, s)
    v, i = tail_value(p, r)
    gap, figure = abs(v + 1), X.MEASURED["tail"][case]
    print("%s: HOMO %d, r vKLI = %.6f at node %d (r = %.3f), |.. + 1| = %.3e, figure %.1e" % (case, h, v, i, float(r[i]), gap, figure))
    assert gap <= figure <= 1.2 * gap


# ---- the host planner ------------------------------------------------------------------------------------------------------------------------
def test_job_tables_against_the_python_statement():
    lib = D.load()
    assert D.exchange_jobs([0]).tolist() == [[0, 0, 0]]
    assert D.exchange_jobs([0, 0, 1]).tolist() == [[0, 0, 0], [0, 1, 0], [0, 2, 1], [1, 1, 0], [1, 2, 1], [2, 2, 0], [2, 2, 2]]
    for Z, nlev, njobs in ((86, 15, 176), (118, 19, None)):
        lz = [l for _, l, _ in D.get_subshells(Z)]
        assert len(lz) == nlev
        jobs = D.exchange_jobs(lz)
        assert [tuple(x) for x in jobs.tolist()] == X.y_jobs(lz)
        assert njobs is None or len(jobs) == njobs
        l32 = np.array(lz, np.int32)
        assert lib.dfta_exchange_jobs(nlev, l32.ctypes.data_as(D.c_ip), None) == len(jobs)          # count only
        for x, y, k in jobs:
            assert x <= y and 0 <= k <= D.SLATER_KMAX and S.gaunt_3j2(lz[x], k, lz[y]) > 0
    assert lib.dfta_exchange_jobs(0, None, None) == 0
    bad = np.array([0, 5], np.int32)
    assert lib.dfta_exchange_jobs(2, bad.ctypes.data_as(D.c_ip), None) == -1
    assert lib.dfta_exchange_jobs(-1, bad.ctypes.data_as(D.c_ip), None) == -1
    assert lib.dfta_exchange_jobs(2, None, None) == -1
    with pytest.raises(D.DftaError):
        D.exchange_jobs([0, -1])


def test_homo_rule_statement():
    E = [-3.0, -1.0, -1.0, -0.5, -2.0]
    assert X.pick_homo(E, [1, 1, 1, 0, 1]) == 2 and X.pick_homo(E, [0] * 5) == -1 and X.pick_homo(E, [1] * 5) == 3
    assert X.pick_homo([], []) == -1 and X.pick_homo([-1.0, -1.0, -1.0], [1, 0.5, 0]) == 1


def test_host_planner_stand_alone_under_sanitizers(tmp_path):
    """dftatom_amd/csrc/exchange_plan.cpp is pure host code: a stand-alone program (tests/exchange_plan_main.cpp) built with ASan + UBSan
    makes the tables of 19 levels, validates good and bad tables and channels, applies the HOMO rule and solves a reduced system whose
    pivoting exchanges rows; what it prints equals the Python statement"""
    import shutil
    import subprocess
    here = os.path.dirname(os.path.abspath(__file__))
    csrc = os.path.join(here, "..", "dftatom_amd", "csrc")
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler is needed"
    exe = str(tmp_path / "exchange_plan_main")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", csrc, "-o", exe,
                    os.path.join(here, "exchange_plan_main.cpp"), os.path.join(csrc, "exchange_plan.cpp"),
                    os.path.join(csrc, "slater_plan.cpp")], check=True, timeout=300)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, (run.stdout, run.stderr)
    first, tab, homo, solve = (ln.split() for ln in run.stdout.strip().split("\n"))
    l = [x for _, x, _ in D.get_subshells(118)]
    occ = [0.5 + 0.25 * a for a in range(19)]
    entries = X.x_entries(l)
    assert int(first[1]) == len(X.y_jobs(l)) and int(first[3]) == sum(len(e) for e in entries)
    rows = {job: j for j, job in enumerate(X.y_jobs(l))}
    want = []
    for a in range(3):
        for b, k in entries[a]:
            c = S.gaunt_3j2(l[a], k, l[b])
            want.append("%d:%d:%d:%d:%.17g" % (a, b, k, rows[(min(a, b), max(a, b), k)], occ[b] * (c.numerator / c.denominator)))
    assert tab[1:] == want
    assert [int(x) for x in homo[1:]] == [2, -1, 3, -1]
    M = np.array([0.5, 0.1, 0.2, 0.2, 0.1, 0.4, 0.3, 0.2, 0.9, 0.0, 0.05, 0.05, 0.2, 0.3, 0.1, 0.4]).reshape(4, 4)
    vS, vHF = np.array([-1.0, -0.7, -0.4, -0.2]), np.array([-1.1, -0.65, -0.5, -0.1])
    c64 = X.solve_kli(M, vS, vHF, 1, dtype=np.float64)
    assert [float(x) for x in solve[1:]] == [float(x) for x in c64] and c64[1] == 0        # the stated order: bit for bit
    cld = X.solve_kli(M, vS, vHF, 1)
    idx = [0, 2, 3]
    A = np.eye(3) - M[np.ix_(idx, idx)]
    assert np.max(np.abs((np.eye(3, dtype=LD) - M[np.ix_(idx, idx)].astype(LD)) @ cld[idx] - (vS.astype(LD) - vHF.astype(LD))[idx])) < 1e-18


# ---- header and binding ----------------------------------------------------------------------------------------------------------------------
NEW = ("dfta_exchange_jobs", "dfta_screening_yk", "dfta_scf_screening_yk", "dfta_exchange_potentials", "dfta_scf_exchange_potentials")


def test_header_and_binding_agree_and_the_abi_stays():
    src = open(os.path.join(ROOT, "include", "dftatom_hip.h")).read()
    flat = re.sub(r"/\*.*?\*/", " ", src, flags=re.S)
    lib = D.load()
    for name in NEW:
        m = re.search(r"\bint\s+%s\s*\(([^;]*?)\)\s*;" % name, flat)
        assert m, "not declared: " + name
        assert name in D.SIGNATURES, "not bound: " + name
        res, args = D.SIGNATURES[name]
        assert len(args) == len(m.group(1).split(",")), name
        assert getattr(lib, name)
    assert "#define DFTA_ABI_VERSION 7" in src and lib.dfta_abi_version() == 7 == D.ABI_VERSION
    assert (D.XP_COLS, D.XP_HF, D.XP_S, D.XP_C, D.XP_KLI) == tuple(int(re.search(r"#define DFTA_XP_%s\s+(\d+)" % k, src).group(1))
                                                                  for k in ("COLS", "HF", "S", "C", "KLI"))
    assert "typedef struct" not in src[src.index("exchange potentials from orbitals"):src.index("Bessel transforms: X-ray")]


def test_front_end_usage_names_the_exchange_table():
    """dftatom_cli without arguments (no GPU needed): the usage text names --exchange-table"""
    import subprocess
    compat = os.path.join(ROOT, "dftatom_amd", "compat")
    exe = os.path.join(compat, "dftatom_cli")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-C", compat])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "--exchange-table" in r.stderr
