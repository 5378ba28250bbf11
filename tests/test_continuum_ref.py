"""CPU suite: the reference of the continuum block (tests/_continuum_ref.py) -- the header's arithmetic in longdouble against the closed
forms (free particle, Coulomb functions, hydrogen-like bound orbitals, the hydrogen 1s cross section), with the measured distances that
tests/test_gpu_continuum.py gates the device at; the calibration of the rounding gate 8 E + floor (a perturbed float64 model passes at
half the gate, two wrong models miss it by more than 10^3); the WKB normalisation against the Riccati matching on a short-range
potential; the header, the binding and the host planner (stand-alone, under ASan + UBSan).  No GPU."""
import math
import os
import re

import numpy as np
import pytest

import _continuum_ref as R

LD = np.longdouble
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("dfta_continuum", "dfta_scf_continuum", "dfta_scf_photoionization")


def _held(d, fig, what):
    """a measured figure holds: the distance is within it, and the figure is not loose (within 1.5 x of the distance, or at the floor)"""
    assert d <= fig, "%s: %.3g exceeds the recorded %.3g" % (what, d, fig)
    assert fig <= R.FLOOR or d >= fig / 1.5, "%s: the recorded %.3g is loose, measured %.3g" % (what, fig, d)


@pytest.mark.parametrize("name", R.CLOSED_GRIDS)
def test_reference_against_closed_forms(name):
    r, s, c, lam = R.tables(*R.GRIDS[name])
    seen = set()
    worst = 0.0
    for group in R.closed_groups(name):
        tag, V, l, E, m, mode, P, power, want_rows = group
        res = R.sweep(V, l, E, np.full(len(E), m), r, s, c, lam, mode, P, power, dtype=LD, want_rows=want_rows)
        assert not res["status"].any(), tag
        if tag[0] == "bound":
            assert res["nodes"][0] == 4 - l - 1 and res["scale"][0] == 0 and res["delta"][0] == 0       # E < 0: no normalisation
        for key, dist in R.closed_distance(name, group, res).items():
            seen.add(key)
            for k, d in enumerate(dist):
                _held(d, R.MEASURED[name][key][k], "%s %s #%d" % (name, key, k))
                worst = max(worst, d / R.MEASURED[name][key][k])
    assert seen == set(R.MEASURED[name])
    print("%s: largest distance / recorded figure %.3f" % (name, worst))


def test_measured_figures_cannot_be_loosened():
    """the figures of the issue: u'/u of the Coulomb problem within 4e-8 on log12 and 2e-9 on log13; free phase shifts about 1e-9
    at E <= 0.05 for every l (1.1e-9 for l = 0 on log12: capped at 2e-9); the WKB normalisation of H 1s within 7.5e-4 x 2 (sigma ~ S^2) at E = 0.01 and 1e-4 from E = 0.5 on"""
    for name, cap in (("log12", 4e-8), ("log13", 2e-9)):
        assert max(max(v) for k, v in R.MEASURED[name].items() if k[0] in ("coul_ld", "bound_ld")) <= cap
    for name in R.CLOSED_GRIDS:
        assert max(max(v[:2]) for k, v in R.MEASURED[name].items() if k[0] == "free_delta") <= 2e-9
        assert R.MEASURED[name][("H_sigma",)][0] <= 1.5e-3 and max(R.MEASURED[name][("H_sigma",)][1:]) <= 1e-4
    assert abs(R.hydrogen_1s_sigma(0.5 + 1e-9) * R.MB_PER_A02 - 6.30) < 0.01                 # the threshold value, megabarn


def test_hydrogen_cross_section_closed_form_against_mpmath_coulomb_functions():
    """the closed form the H 1s gate uses, against the dipole integral taken with mpmath's Coulomb functions (l = 1, Z = 1)"""
    import mpmath as mp
    mp.mp.dps = 25
    for omega in (0.51, 2.0):
        k = mp.sqrt(2 * (mp.mpf(omega) - mp.mpf(1) / 2))
        eta = -1 / k
        S = mp.sqrt(2 / (mp.pi * k)) * mp.quad(lambda x: 2 * x * mp.exp(-x) * x * mp.coulombf(1, eta, k * x), mp.linspace(0, 60, 31))
        sigma = 4 * mp.pi ** 2 * R.ALPHA_FS * omega / 3 * S ** 2
        assert abs(float(sigma) / R.hydrogen_1s_sigma(omega) - 1) < 1e-10, omega


def test_neon_orthogonality_figure_of_the_cpu_oracle():
    """Ne LDA on log12, 40 steps of the CPU oracle: the overlaps of eps s (in the potential the step leaves) with the step's 1s and 2s"""
    got = R.neon40_overlaps()
    for b in range(2):
        for k, e in enumerate(R.NE40_ENERGIES):
            _held(float(got[b][k]), R.NE40_OVERLAP[b][k], "Ne %s eps = %g" % (("1s", "2s")[b], e))


# ---- the rounding gate -----------------------------------------------------------------------------------------------------------------
def _yukawa_case():
    r, s, c, lam = R.tables(*R.GRIDS["log12"])
    N = len(r)
    V = np.zeros(N)
    V[1:] = -10.0 * np.exp(-r[1:]) / r[1:]
    P = np.array([R.hydrogenic_u(n, l, 10, r.astype(LD)).astype(np.float64) for n, l in ((1, 0), (2, 0))])
    E = np.geomspace(0.005, 8.0, 24)
    return V, E, N, r, s, c, lam, P


@pytest.fixture(scope="module")
def yukawa():
    V, E, N, r, s, c, lam, P = _yukawa_case()
    return {mode: R.gate(V, 1, E, N - 2, r, s, c, lam, mode, P, 1, want_rows=True) for mode in (R.FREE, R.WKB)}


@pytest.mark.parametrize("mode", (R.FREE, R.WKB))
def test_gate_passes_a_perturbed_model_and_fails_two_wrong_models(yukawa, mode):
    """8 E + floor: a float64 model whose every division is moved by +-1 ulp (a seed the floor has not seen) stays within half of it;
    the model without the delta^2 / 4 term and the model with 1/10 in place of 1/12 miss it by more than 10^3"""
    V, E, N, r, s, c, lam, P = _yukawa_case()
    ld, f64, gates = yukawa[mode]
    m = np.full(len(E), N - 2)
    pert = R.distances(R.sweep(V, 1, E, m, r, s, c, lam, mode, P, 1, perturb=R.Perturb(1234), want_rows=True), ld)
    worst = max(float(np.max(pert[q] / gates[q])) for q in R.QUANTITIES)
    print("mode %d: perturbed model / gate %.3f" % (mode, worst))
    assert worst <= 0.5
    assert np.array_equal(f64["nodes"], ld["nodes"])
    for wrong in ("noc", "tenth"):
        bad = R.distances(R.sweep(V, 1, E, m, r, s, c, lam, mode, P, 1, wrong=wrong, want_rows=True), ld)
        miss = max(float(np.max(bad[q] / gates[q])) for q in R.QUANTITIES)
        print("mode %d: wrong model %s / gate %.3g" % (mode, wrong, miss))
        assert miss > 1e3, (wrong, miss)
        for q in ("logderiv", "delta"):          # scale-free quantities see both mistakes at every energy
            assert float(np.min(bad[q] / gates[q])) > 1, (wrong, q)


def test_wkb_normalisation_agrees_with_the_riccati_matching_on_a_short_range_potential(yukawa):
    """at r_m = 25 the Yukawa potential is gone (1e-11) and the centrifugal term is all that separates kappa from k: the first-order WKB
    amplitude is off by |alpha'' / (2 alpha kappa^2)| ~ (3/2) L / (k r)^4, L = l (l + 1) = 2 -- the bound is twice that plus the two
    rounding gates"""
    V, E, N, r, s, c, lam, P = _yukawa_case()
    free, wkb = yukawa[R.FREE], yukawa[R.WKB]
    k = np.sqrt(2 * E)
    bound = 2 * 1.5 * 2 / (k * r[N - 2]) ** 4 + free[2]["scale"] + wkb[2]["scale"]
    ratio = np.abs((wkb[0]["scale"] / free[0]["scale"]).astype(np.float64) - 1)
    print("WKB / FREE scale: largest ratio to the bound %.3f" % float(np.max(ratio / bound)))
    assert np.all(ratio <= bound), (ratio, bound)
    big = np.max(np.abs(free[0]["sums"]), axis=1)
    assert np.all(np.max(np.abs(wkb[0]["sums"] - free[0]["sums"]), axis=1) <= (bound + free[2]["sums"] + wkb[2]["sums"]) * big)
    # where WKB is needed: on a pure -1/r tail the Riccati matching at r = 25 is 13 % wrong at E = 0.05 (l = 0)
    Vc = np.zeros(N)
    Vc[1:] = -1.0 / r[1:]
    fr = R.sweep(Vc, 0, [0.05], [N - 2], r, s, c, lam, R.FREE, dtype=LD)["scale"]
    wk = R.sweep(Vc, 0, [0.05], [N - 2], r, s, c, lam, R.WKB, dtype=LD)["scale"]
    assert abs(float(fr[0] / wk[0]) - 1) > 0.1


def test_status_bits_and_unnormalised_trials():
    r, s, c, lam = R.tables(*R.GRIDS["uni10"])
    N = len(r)
    V = np.zeros(N)
    out = R.sweep(V, 0, [-1.0, 0.0, 0.5], [N - 2] * 3, r, s, c, lam, R.FREE)
    assert list(out["scale"][:2]) == [0, 0] and list(out["delta"][:2]) == [0, 0] and out["scale"][2] > 0 and np.all(np.isfinite(out["logderiv"]))
    # u = sinh(kappa r) for E < 0, r for E = 0: u'/u = kappa / tanh(kappa R), 1 / R (Numerov's h^4: h = 0.0244)
    kap = math.sqrt(2.0)
    assert abs(out["logderiv"][0] / (kap / math.tanh(kap * r[N - 2])) - 1) < 1e-7 and abs(out["logderiv"][1] * r[N - 2] - 1) < 1e-9
    Vn = V.copy()
    Vn[500] = np.nan
    out = R.sweep(Vn, 0, [0.5, 0.5], [400, 600], r, s, c, lam, R.FREE)
    assert out["status"][0] == 0 and out["status"][1] & R.STEP and np.isnan(out["logderiv"][1]) and out["nodes"][1] == -1
    # a barrier at the end node: kappa^2 <= 0 there -- the WKB bit, u'/u and nodes stay
    Vb = V.copy()
    Vb[N - 4:] = 5.0
    out = R.sweep(Vb, 0, [0.5], [N - 2], r, s, c, lam, R.WKB)
    assert out["status"][0] == R.WKB_TAIL and np.isnan(out["scale"][0]) and np.isfinite(out["logderiv"][0]) and out["nodes"][0] >= 0
    # the free normalisation below double range, l = 4: at E = 1e-300 yh_4 ~ x^-4 overflows and a = inf - inf -- the NORM bit, u'/u and
    # nodes stand; at E = 1e-150 only yh'_4 overflows, hypot is inf and the scale is 0.0 (the replay's: 1.3e-340) without a bit
    P = np.array([r * np.exp(-r)])
    out = R.sweep(V, 4, [1e-300, 1e-150], [N - 2] * 2, r, s, c, lam, R.FREE, P, 1, want_rows=True)
    assert list(out["status"]) == [R.NORM, 0] and np.isnan(out["scale"][0]) and out["scale"][1] == 0.0
    assert np.all(np.isfinite(out["logderiv"])) and np.all(out["nodes"] >= 0)
    assert np.isnan(out["delta"][0]) and np.isnan(out["sums"][0, 0]) and np.all(np.isnan(out["rows"][0, 1:])) and out["rows"][0, 0] == 0
    assert not out["rows"][1].any() and out["sums"][1, 0] == 0
    ld = R.sweep(V, 4, [1e-300, 1e-150], [N - 2] * 2, r, s, c, lam, R.FREE, dtype=LD)
    assert not ld["status"].any() and np.all(np.isfinite(ld["scale"])) and 0 < ld["scale"][1] < 5e-324
    # gate() marks the replay where the float64 model carries the bit: the trial counts as one without a normalisation
    ld, f64, gates = R.gate(V, 4, [1e-300, 1e-150], N - 2, r, s, c, lam, R.FREE, P, 1, seeds=(0,), want_rows=True)
    assert list(ld["status"]) == [R.NORM, 0] and np.isnan(ld["scale"][0]) and np.all(np.isnan(ld["rows"][0])) and np.isfinite(ld["scale"][1])
    assert all(np.all(np.isfinite(gates[q])) for q in R.QUANTITIES)


def test_atan2_reconstruction_with_both_halves_of_pi():
    """the kernel's atan2 takes the library's value in the first octant only and puts the quadrant back with pi / 2 and pi as two doubles:
    against mpmath that is as good as a correctly rounded first octant allows (within 1 ulp, wrong in under 3 % of 4000 draws), where
    the reconstruction from the one nearest double is wrong in more than 10 %; the special values are np.arctan2's, sign included"""
    import mpmath as mp
    mp.mp.dps = 40
    rng = np.random.default_rng(2)
    n = 4000
    x = rng.standard_normal(n) * 10.0 ** rng.integers(-3, 3, n)
    y = rng.standard_normal(n) * 10.0 ** rng.integers(-6, 3, n)
    ref = np.array([float(mp.atan2(mp.mpf(float(a)), mp.mpf(float(b)))) for a, b in zip(y, x)])
    two, one = R.atan2_quadrants(y, x), R.atan2_quadrants(y, x, tails=False)
    assert np.all(np.abs(two - ref) <= np.spacing(np.abs(ref))) and np.mean(two != ref) < 0.03 and np.mean(one != ref) > 0.10
    # the case that showed it: Coulomb Z = 10, l = 1, uni10, E = 1e-4 -- the exact phase shift lies 0.38 ulp below the double nearest it,
    # the one-double pi is another 0.28 ulp short: 0.66 ulp, the neighbour below
    r, s, c, lam = R.tables(*R.GRIDS["uni10"])
    V = np.zeros(len(r))
    V[1:] = -10.0 / r[1:]
    ld = R.sweep(V, 1, [1e-4], [len(r) - 2], r, s, c, lam, R.FREE, dtype=LD)["delta"][0]
    f64 = R.sweep(V, 1, [1e-4], [len(r) - 2], r, s, c, lam, R.FREE)["delta"][0]
    assert f64 == np.float64(ld) and 0.3 < float((LD(f64) - ld) / LD(2.0 ** -51)) < 0.45
    inf, nan = np.inf, np.nan
    for yy, xx in ((0.0, -1.0), (-0.0, -1.0), (0.0, -0.0), (-0.0, -0.0), (0.0, 0.0), (-0.0, 0.0), (1.0, -0.0), (1.0, 0.0), (inf, -inf), (inf, inf),
                   (-1.0, -inf), (1.0, inf), (inf, 1.0), (-inf, -1.0), (1e-300, -1e300), (5e-324, -1.0), (nan, 1.0), (1.0, nan), (nan, -1.0)):
        got, want = R.atan2_quadrants(yy, xx), np.arctan2(yy, xx)
        assert (np.isnan(got) and np.isnan(want)) or (got == want and np.signbit(got) == np.signbit(want)), (yy, xx, got, want)


def test_energy_ladder_model_against_its_gate():
    """the premise of the GPU suite's energy ladder, E = 1e-100 .. 1e-4 (uni10, free particle and Coulomb Z = 10, l = 1 .. 4, FREE): no
    status bit in either format, a positive scale, finite gates.  Prints the model's own distance over its gate (at most 1/8 by the
    gate's construction; close to it when the floor adds little, i.e. the gate is about eight times the model's own error)"""
    r, s, c, lam = R.tables(*R.GRIDS["uni10"])
    N = len(r)
    V = np.zeros((2, N))
    V[1, 1:] = -10.0 / r[1:]
    worst = 0.0
    for v in range(2):
        for l in range(1, 5):
            ld, f64, gates = R.gate(V[v], l, R.LADDER_E, N - 2, r, s, c, lam, R.FREE)
            assert not f64["status"].any() and not ld["status"].any() and np.all(f64["scale"] > 0)
            own = R.distances(f64, ld)
            for q in ("logderiv", "delta", "scale"):
                assert np.all(own[q] <= gates[q]), (v, l, q)
                worst = max(worst, float(np.max(own[q] / np.where(gates[q] > 0, gates[q], 1))))
    print("ladder: the model's largest ratio to its gate %.3f" % worst)
    assert 0 < worst <= 0.125


# ---- the header, the binding, the planner ---------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_and_bound():
    import dftatom_amd as D
    src = open(os.path.join(ROOT, "include", "dftatom_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in NEW_SYMBOLS:
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, src)
        assert m, "not declared in the header: " + name
        res, args = D.SIGNATURES[name]
        assert res is D.C.c_int and len(args) == len(m.group(1).split(",")), name
    defines = dict(re.findall(r"#define\s+(DFTA_\w+)\s+(\d+)", src))
    assert int(defines["DFTA_ABI_VERSION"]) == D.ABI_VERSION          # entries were added, no struct grew
    assert (int(defines["DFTA_CONT_FREE"]), int(defines["DFTA_CONT_WKB"])) == (D.CONT_FREE, D.CONT_WKB) == (R.FREE, R.WKB)
    assert int(defines["DFTA_CONT_MAX_PARTNERS"]) == D.CONT_MAX_PARTNERS == R.MAX_PARTNERS
    assert tuple(int(defines["DFTA_CONT_" + n]) for n in ("NONFINITE", "STEP", "WKB_TAIL", "NORM")) == (R.NONFINITE, R.STEP, R.WKB_TAIL, R.NORM) \
        == (D.CONT_NONFINITE, D.CONT_STEP, D.CONT_WKB_TAIL, D.CONT_NORM) == (1, 2, 4, 8)
    lib = D.load()
    assert all(hasattr(lib, n) for n in NEW_SYMBOLS)
    for f in (D.continuum, D.Scf.continuum, D.Scf.photoionization):
        assert callable(f)
    plan = open(os.path.join(ROOT, "dftatom_amd", "csrc", "continuum_plan.h")).read()
    assert "kTile = %d;" % R.TILE in plan and "kMaxPartners = %d;" % R.MAX_PARTNERS in plan


def test_host_planner_stand_alone_under_sanitizers(tmp_path):
    """dftatom_amd/csrc/continuum_plan.cpp is pure host code: a stand-alone program (tests/continuum_plan_main.cpp) built with ASan +
    UBSan walks the validation, the grouping into waves, the instance and the chunking; its lines are checked here"""
    import shutil
    import subprocess
    here = os.path.dirname(os.path.abspath(__file__))
    csrc = os.path.join(here, "..", "dftatom_amd", "csrc")
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler is needed"
    exe = str(tmp_path / "continuum_plan_main")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", csrc, "-o", exe,
                    os.path.join(here, "continuum_plan_main.cpp"), os.path.join(csrc, "continuum_plan.cpp")], check=True, timeout=300)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, (run.stdout, run.stderr)
    lines = [ln.split() for ln in run.stdout.strip().split("\n")]
    plans = {(int(a), int(b)): (int(c), int(d), int(e), int(f)) for tag, a, b, c, d, e, f in lines}
    assert len(plans) == len(lines) == 7
    # (N, trials) -> (waves, padded positions, instance, waves per chunk of rows)
    assert plans[(4097, 1)] == (1, 64, 0, 0)
    assert plans[(4097, 192)] == (4, 256, 8, 4)             # groups of 63, 64 and 65 trials: 1 + 1 + 2 waves; 5 partners: instance 8
    assert plans[(4097, 129)] == (3, 192, 16, 0)
    assert plans[(131073, 1280)] == (20, 1280, 16, 3)       # 64 rows of 131 073 doubles: 64 MiB a wave, three fit 256 MiB
    assert plans[(9, 70000)] == (1094, 70016, 0, 1023)      # the scaling launch's grid caps a chunk
    # the two-chunk calls of tests/test_gpu_continuum.py, one trial per potential (every trial its own wave): 1023 + 77 waves by the
    # wave cap, 511 + 9 waves by the 256 MiB budget (64 rows of 1025 doubles: 524 800 bytes a wave)
    assert plans[(9, 1100)] == (1100, 70400, 4, 1023)
    assert plans[(1025, 520)] == (520, 33280, 4, 511)


def test_front_end_usage_names_the_continuum_tables():
    """dftatom_cli without arguments (no GPU needed): the usage text names both tables"""
    import subprocess
    compat = os.path.join(ROOT, "dftatom_amd", "compat")
    exe = os.path.join(compat, "dftatom_cli")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-C", compat])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "--phase-shift-table" in r.stderr and "--photo-table" in r.stderr
