"""CPU suite: tests/_bessel_ref.py -- the longdouble reference of the spherical Bessel functions and of the Bessel transforms of
include/dftatom_hip.h -- against mpmath and against the closed forms of a hydrogen-like atom of charge Z:

    form factors of u^2 (spherical average):   1s 1 / (1 + a^2)^2, a = q / 2Z;   2s (1 - 3 a^2 + 2 a^4) / (1 + a^2)^4,
                                               2p (1 - a^2) / (1 + a^2)^4, a = q / Z
    momentum-space orbitals (Podolsky-Pauling), P = p / Z:
        R~_nl(p) = +- Z^(-3/2) sqrt((2/pi) (n-l-1)! / (n+l)!) n^2 2^(2l+2) l! (nP)^l / (n^2 P^2 + 1)^(l+2) C^(l+1)_(n-l-1)((n^2 P^2 - 1) / (n^2 P^2 + 1))

The file MEASURES (a) the error of a float64 model of the header's two branches of j_l on a dense ladder of arguments -- the check that
fixes the switch at x = 3 and the 14 series terms -- and (b) the distance of the reference's quadrature from the closed forms per grid,
orbital and q, and holds each to the figure written into _bessel_ref: not above it, and the figure not more than 1.2 x the measurement
(or the floor 1e-17).  It also holds the new symbols of the header to the binding, and runs the pure host planner
(dftatom_amd/csrc/bessel_plan.cpp) stand-alone under the sanitizers.
"""
import os
import re

import numpy as np
import pytest

import _bessel_ref as B

LD = B.LD
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("dfta_sph_bessel", "dfta_bessel_transform", "dfta_scf_form_factors", "dfta_scf_momentum_orbitals")


@pytest.fixture(scope="module")
def tables():
    assert np.finfo(LD).eps < 1.2e-19, "this reference needs an extended np.longdouble"
    return {name: B.grid(*B.GRIDS[name]) for name in B.CLOSED_GRIDS}


def _held(measured, figure, what):
    print("%-44s measured %.3e  figure %.1e" % (what, measured, figure))
    assert measured <= figure, (what, measured, figure)
    assert figure <= max(1.2 * measured, B.FLOOR), (what, measured, figure)


# ---- j_l --------------------------------------------------------------------------------------------------------------------------------
def test_special_arguments():
    for l in range(B.LMAX + 1):
        j, T = B.jl(l, np.array([0.0, -0.0]))
        assert np.all(j == (1 if l == 0 else 0)) and np.all(B.jl_bound(l, np.array([0.0, -0.0])) == 0)
        assert np.all(B.jl_model(l, np.array([0.0, -0.0])) == (1.0 if l == 0 else 0.0))
        assert B.jl_model(l, [1e-300])[0] == (1.0, 1e-300 / 3, 0.0, 0.0, 0.0)[l]
    x = B.ladder()
    assert x[0] == 1e-8 and x[-1] == 1e4 and {np.nextafter(3.0, 0), 3.0, np.nextafter(3.0, 4)} <= set(x)


def test_longdouble_jl_against_mpmath():
    """j_l = sqrt(pi / 2x) J_{l+1/2}(x) at 40 digits.  Gate 4 c eps_LD T_l(x) with c the device's count (jl_roundings): the reference runs
    the same recurrence with true divisions and a sin / cos good to 1 ulp (fewer roundings than counted), and its series of 30 terms,
    summed forward, puts at most 3 k + 30 <= 120 roundings on a term where the count is 69 or more."""
    mp = pytest.importorskip("mpmath")
    mp.mp.dps = 40
    eps_ld = float(np.finfo(LD).eps)
    x = B.ladder()
    worst = 0.0
    for l in range(B.LMAX + 1):
        j, T = B.jl(l, x)
        c = B.jl_roundings(l, x)
        for k in range(len(x)):
            xm = mp.mpf(float(x[k]))
            ref = mp.sqrt(mp.pi / (2 * xm)) * mp.besselj(l + mp.mpf(1) / 2, xm)
            err = abs(float(mp.mpf(str(j[k])) - ref))            # str of a longdouble: the shortest digits that give it back
            gate = 4 * c[k] * eps_ld * float(T[k]) + 1e-300
            worst = max(worst, err / gate)
            assert err <= gate, (l, x[k], float(j[k]), float(ref), err / gate)
    print("longdouble j_l against mpmath over %d arguments: %.3f of the gate" % (len(x), worst))


@pytest.mark.parametrize("l", range(B.LMAX + 1))
def test_float64_model_of_the_two_branches(l):
    x = B.ladder()
    j, T = B.jl(l, x)
    scale = B.EPS * B.e_l(l, x)
    err = np.abs(B.jl_model(l, x).astype(LD) - j).astype(np.float64) / scale
    below, above = x < B.SWITCH, x >= B.SWITCH
    _held(float(err[below].max()), B.MODEL_ERROR[l][0], "l = %d, x < 3 (series)" % l)
    _held(float(err[above].max()), B.MODEL_ERROR[l][1], "l = %d, x >= 3 (recurrence)" % l)
    # the counted bound of the device's j_l covers the model (the host's sin and cos are better than the 2 ulp counted)
    assert np.all(np.abs(B.jl_model(l, x).astype(LD) - j).astype(np.float64) <= B.jl_bound(l, x))
    assert np.all(T >= np.abs(j))
    if l == 0:
        return
    # what fixes the switch and the term count: the alternatives, in the same units
    alt = lambda sw, terms: np.abs(B.jl_model(l, x, sw, terms).astype(LD) - j).astype(np.float64) / scale       # noqa: E731
    more = alt(B.SWITCH, B.SERIES_TERMS + 2)
    assert more[below].max() == err[below].max(), "more terms change nothing"
    if l == 1:
        assert alt(B.SWITCH, 12)[below].max() > 5 * B.MODEL_ERROR[1][0], "12 terms are too few at x = 3"
        assert alt(4.0, B.SERIES_TERMS)[above].max() > 10 * B.MODEL_ERROR[1][1], "the series beyond 3 loses digits"
    if l == 4:
        assert alt(2.0, B.SERIES_TERMS)[below].max() > 50 * B.MODEL_ERROR[4][0], "the recurrence below 3 loses digits"
        lone = B.jl_model(4, [0.1], switch=0.0)[0]                        # the recurrence alone at x = 0.1
        assert abs(lone / float(B.jl(4, [0.1])[0][0]) - 1) > 1e-5


def test_derivative_term():
    """|x j_l'(x)| against a central difference of the longdouble j_l"""
    x = np.array([0.3, 2.9, 3.1, 17.0, 200.0])
    h = LD(1e-6)
    for l in range(B.LMAX + 1):
        d = (B.jl(l, x.astype(LD) + h)[0] - B.jl(l, x.astype(LD) - h)[0]) / (2 * h)
        assert np.all(np.abs(np.abs(x * d) - B.jl_prime_x(l, x)) < 1e-9 * (1 + np.abs(x)))


def test_rounding_counts():
    assert B.transform_roundings(B.BT_DENSITY, 9) == 8 + 4 + 11 and B.transform_roundings(B.BT_ORBITAL, 2049) == 7 + 12 + 11
    assert B.transform_roundings(B.BT_DENSITY, 131073) == 8 + 4 * 129 + 11
    x = np.array([0.0, 1.0, 2.999, 3.0, 50.0])
    assert B.jl_roundings(0, x).tolist() == [0, 3, 3, 3, 3]
    assert B.jl_roundings(1, x).tolist() == [0, 68, 68, 7, 7] and B.jl_roundings(4, x).tolist() == [0, 71, 71, 19, 19]


# ---- closed forms -----------------------------------------------------------------------------------------------------------------------
def test_closed_forms_at_known_points():
    """q = 0: every form factor is 1; R~_1s(p) = 4 sqrt(2/pi) Z^(-3/2) / (1 + P^2)^2; Int R~^2 p^2 dp = 1 (Parseval) by Simpson's rule"""
    for n, l in B.FORM_ORBITALS:
        assert B.form_factor_closed(n, l, 7, 0.0) == 1
    assert abs(B.momentum_closed(1, 0, 1, 1.0) - 4 * np.sqrt(2 / B.PI_LD) / 4) < 1e-18
    assert B.gegenbauer(2, 1, LD(0.5)) == 4 * LD(0.25) - 1 and B.gegenbauer(3, 2, LD(0.5)) == 32 * LD(0.125) - 12 * LD(0.5)
    p = np.linspace(0, 400, 2001).astype(LD)
    w = np.full(len(p), 2.0, dtype=LD)
    w[1::2] = 4
    w[0] = w[-1] = 1
    for n, l in B.MOMENTUM_ORBITALS:
        R = np.array([B.momentum_closed(n, l, B.ZREF, x) for x in p])
        norm = np.sum(w * R * R * p * p) * (p[1] - p[0]) / 3
        assert abs(norm - 1) < 2e-4, (n, l, float(norm))                                  # the tail beyond p = 400: (Z / p)^5 and less


def _distances(name, r, s):
    """the reference's quadrature on longdouble orbitals against the closed forms: {"F" / "M": {(n, l): [|ref - closed| per q]}}"""
    N = len(r)
    w = B.weights(N)
    out = {"F": {}, "M": {}}
    for n, l in B.FORM_ORBITALS:
        rho = B.density_row(B.hydrogenic_u(n, l, B.ZREF, r), r)
        g = w * rho * r * r * s * B.K_LD[B.BT_DENSITY]
        out["F"][(n, l)] = [float(abs(np.sum(g * B.jl(0, LD(q) * r)[0]) - B.form_factor_closed(n, l, B.ZREF, q))) for q in B.QS]
    for n, l in B.MOMENTUM_ORBITALS:
        g = w * B.hydrogenic_u(n, l, B.ZREF, r) * r * s * B.K_LD[B.BT_ORBITAL]
        vals = [np.sum(g * B.jl(l, LD(q) * r)[0]) for q in B.QS]
        closed = [B.momentum_closed(n, l, B.ZREF, q) for q in B.QS]
        sign = 1 if vals[0] * closed[0] > 0 else -1                                       # the convention, fixed at the smallest q
        out["M"][(n, l)] = [float(abs(v - sign * c)) for v, c in zip(vals, closed)]
    return out


@pytest.mark.parametrize("name", B.CLOSED_GRIDS)
def test_reference_against_closed_forms(tables, name):
    r, s = tables[name]
    got = _distances(name, r, s)
    for fam in ("F", "M"):
        assert sorted(got[fam]) == sorted(B.MEASURED[name][fam])
        for nl, dist in got[fam].items():
            for q, d, fig in zip(B.QS, dist, B.MEASURED[name][fam][nl]):
                _held(d, fig, "%s %s %s q = %g" % (name, fam, nl, q))


def test_hydrogen_lsda_distance_from_the_exact_1s():
    """the CPU oracle's converged H LSDA density on log12: its form factor against the exact 1s one, the figure the GPU test gates at"""
    import ctypes as C
    import _oracle as O
    o = O.oracle()
    L, d, Rm = B.GRIDS["log12"]
    s = o.dfo_scf_create(1, 1, L, 0.5, Rm, d, 0)
    try:
        e = O.Energies()
        for _ in range(150):
            o.dfo_scf_step(s, C.byref(e))
            if s.contents.finished:
                break
        assert s.contents.finished
        N = s.contents.g.N
        rho = np.ctypeslib.as_array(s.contents.density, (N,)).copy()
    finally:
        o.dfo_scf_destroy(s)
    r = O.grid_r(O.make_grid(L, d, Rm))
    sl = B.grid(L, d, Rm)[1]
    for q, fig in B.H_LSDA_DISTANCE.items():
        v, _ = B.transform(B.BT_DENSITY, 0, rho, r, sl, q)
        _held(float(abs(v - B.form_factor_closed(1, 0, 1, q))), fig, "H LSDA q = %g" % q)
    assert abs(B.transform(B.BT_DENSITY, 0, rho, r, sl, 0.0)[0] - 1) < 1e-12


def test_measured_figures_cannot_be_loosened():
    worst = lambda name: max(v for fam in B.MEASURED[name].values() for t in fam.values() for v in t)      # noqa: E731
    assert worst("log12") <= 3e-15 and worst("log13") <= 2e-16 and worst("uni13") <= 5.4e-7


def test_transform_of_the_reference_matches_its_parts(tables):
    """transform() on float64 input is the same weighted sum as _distances on longdouble input, up to the input's rounding; the bound is
    positive and the value of an all-zero row is exactly 0 with bound 2^-1022"""
    r, s = tables["log12"]
    r64 = r.astype(np.float64)
    u = B.hydrogenic_u(2, 1, B.ZREF, r64.astype(LD)).astype(np.float64)
    v, b = B.transform(B.BT_ORBITAL, 1, u, r64, s, 3.0)
    assert abs(abs(v) - abs(B.momentum_closed(2, 1, B.ZREF, 3.0))) < 1e-14 and 0 < b < 1e-12
    v0, b0 = B.transform(B.BT_DENSITY, 0, np.zeros(len(r)), r64, s, 3.0)
    assert v0 == 0 and b0 == B.TINY


# ---- the header, the binding, the planner, the front end -----------------------------------------------------------------------------------
def test_new_symbols_are_declared_and_bound():
    """every new entry is declared in include/dftatom_hip.h and bound in dftatom_amd.SIGNATURES with the header's number of arguments;
    the constants agree; the ABI version stays 7"""
    import dftatom_amd as D
    src = open(os.path.join(ROOT, "include", "dftatom_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in NEW_SYMBOLS:
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, src)
        assert m, "not declared in the header: " + name
        assert name in D.SIGNATURES, "not bound: " + name
        res, args = D.SIGNATURES[name]
        assert res is D.C.c_int and len(args) == len(m.group(1).split(",")), name
    defines = dict(re.findall(r"#define\s+(DFTA_\w+)\s+(\d+)", src))
    assert int(defines["DFTA_ABI_VERSION"]) == 7 == D.ABI_VERSION
    assert (int(defines["DFTA_BT_DENSITY"]), int(defines["DFTA_BT_ORBITAL"])) == (D.BT_DENSITY, D.BT_ORBITAL) == (B.BT_DENSITY, B.BT_ORBITAL)
    assert int(defines["DFTA_BESSEL_LMAX"]) == D.BESSEL_LMAX == B.LMAX
    lib = D.load()
    assert lib.dfta_abi_version() == 7 and all(hasattr(lib, n) for n in NEW_SYMBOLS)
    for f in (D.sph_bessel, D.bessel_transform, D.Scf.form_factors, D.Scf.momentum_orbitals):
        assert callable(f)
    # the device's constants are the reference's: switch, term count
    plan = open(os.path.join(ROOT, "dftatom_amd", "csrc", "bessel_plan.h")).read()
    assert "kSeriesTerms = %d;" % B.SERIES_TERMS in plan and "kSwitch = %.1f;" % B.SWITCH in plan


def test_host_planner_stand_alone_under_sanitizers(tmp_path):
    """dftatom_amd/csrc/bessel_plan.cpp is pure host code: a stand-alone program (tests/bessel_plan_main.cpp) built with ASan + UBSan
    walks the validation and the choice of q's per workgroup; its lines are checked here"""
    import shutil
    import subprocess
    here = os.path.dirname(os.path.abspath(__file__))
    csrc = os.path.join(here, "..", "dftatom_amd", "csrc")
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler is needed"
    exe = str(tmp_path / "bessel_plan_main")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", csrc, "-o", exe,
                    os.path.join(here, "bessel_plan_main.cpp"), os.path.join(csrc, "bessel_plan.cpp")], check=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout, r.stderr)
    rows = [ln.split() for ln in r.stdout.strip().split("\n")]
    picks = {(int(a), int(b), int(c), int(f)): int(qb) for tag, a, b, c, f, qb in rows if tag == "pick"}
    # 256 compute units: Rn's three LSDA rows with 256 q stay at 1 per workgroup (768 workgroups), a periodic table of 1000 rows
    # with 41 q takes 8 (6000 workgroups); the knob wins when it names 1, 2, 4 or 8 and is ignored otherwise
    assert picks[(1, 256, 256, 0)] == 1 and picks[(3, 256, 256, 0)] == 2 and picks[(1000, 41, 256, 0)] == 8
    assert picks[(64, 17, 256, 0)] == 4 and picks[(1, 1, 256, 0)] == 1 and picks[(19, 17, 256, 0)] == 1
    assert [picks[(1000, 41, 256, f)] for f in (1, 2, 4, 8, 3, 16, -1)] == [1, 2, 4, 8, 8, 8, 8]
    for (nrow, nq, cu, f), qb in picks.items():
        if f == 0 and qb > 1:
            assert nrow * -(-nq // qb) >= cu


def test_front_end_usage_names_the_form_factor_table():
    """dftatom_cli without arguments (no GPU needed): the usage text names --form-factor-table"""
    import subprocess
    compat = os.path.join(ROOT, "dftatom_amd", "compat")
    exe = os.path.join(compat, "dftatom_cli")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-C", compat])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "--form-factor-table" in r.stderr
