"""CPU suite: the reference of the pseudization block (tests/_pseudo_ref.py) -- the header's arithmetic in float64 and in longdouble on
hydrogen-like Z = 10 2s, 2p, 3d (V' and V'' analytic: the stencils' distance from the truth) and on the CPU oracle's Ne, Ar and Fe LDA
orbitals: the properties of the scheme, every status bit, the end-to-end checks with no code of this block in the loop (the oracle's
level solver on V_ps returns eps; the restated outward sweep gives equal u'/u at r_c and equal E-differences), with the measured
distances that tests/test_gpu_pseudo.py gates the device at; the calibration of the rounding gate 8 E + floor; the header, the binding
and the host planner (stand-alone, under ASan + UBSan).  No GPU.

Two status bits are safety nets that no input built here reaches: DFTA_PS_CAP (reachable in principle: from the bracket [0, 1/4] a
root within 2^-70 of 0 needs more than 200 halvings, but g(0) is a difference of two logs with a granularity of 1e-16 and g' = O(1), so
a root is 0 or at least 1e-17 away and the search ends after about 3 + 57 + 53 evaluations; the cap is 200) and DFTA_PS_NOTPOSITIVE (an underflow of exp inside r_c: wild inputs end in
DFTA_PS_NOBRACKET first).  The model shows both with a lower cap and with an a2 handed to it."""
import os
import re

import numpy as np
import pytest

import _pseudo_ref as R

LD = R.LD
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("dfta_pseudize", "dfta_pseudo_ionic", "dfta_scf_pseudopotentials", "dfta_pseudo_default_valence", "dfta_pseudo_default_ic")


def _held(d, fig, what, floor=R.LD_FLOOR):
    """a measured figure holds: the distance is within it, and the figure is not loose (within 1.5 x of the distance, or at the floor)"""
    assert d <= max(fig, floor), "%s: %.3g exceeds the recorded %.3g" % (what, d, fig)
    assert fig <= floor or d >= fig / 1.5, "%s: the recorded %.3g is loose, measured %.3g" % (what, fig, d)


@pytest.fixture(scope="module")
def runs():
    """tag -> (inputs, float64 model, longdouble replay) on log12"""
    made = {}

    def get(tag):
        if tag not in made:
            V, u, l, eps, ic = R.case(tag)
            r, s, c, lam = R.tables(*R.GRIDS["log12"])
            made[tag] = ((V, u, l, eps, ic), R.pseudize(V, u, l, eps, ic, r, s, lam), R.pseudize(V, u, l, eps, ic, r, s, lam, dtype=LD))
        return made[tag]
    return get


# ---- the stencils against the truth ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(R.STENCIL))
def test_five_point_stencils_against_analytic_derivatives(name):
    r, s, c, lam = R.tables(*R.GRIDS[name])
    worst = 0.0
    for n, l in R.HYDROGENIC:
        V, u, eps = R.hydrogenic_channel(n, l, r)
        ic = R.default_ic(r, u, R.FACTOR)
        ld = R.pseudize(V, u, l, eps, ic, r, s, lam, dtype=LD)
        assert ld["status"] == 0
        an, mag = R.analytic_matching(n, l, r[ic])
        worst = max(worst, max(float(abs(ld["match"][k + 1] - an[k]) / mag[k]) for k in range(4)))
    print("%s: stencils' distance from the analytic P1 .. P4: %.3g" % (name, worst))
    _held(worst, R.STENCIL[name], name)


# ---- properties of the scheme -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", R.E2E_CASES)
def test_properties_of_a_pseudized_channel(runs, tag):
    (V, u, l, eps, ic), f64, ld = runs(tag)
    r = R.tables(*R.GRIDS["log12"])[0]
    for res, T, eps_T in ((f64, np.float64, R.EPS), (ld, LD, float(np.finfo(LD).eps))):
        assert res["status"] == 0 and 0 < res["iters"] <= 1 + 2 * R.BRACKET_STEPS + 90
        sigma = 1.0 if u[ic] > 0 else -1.0
        # the outside copies, bit for bit
        assert np.array_equal(res["u_ps"][ic:], (sigma * u[ic:]).astype(T)) and np.array_equal(res["V_ps"][ic:], V[ic:].astype(T))
        assert res["rc"] == r[ic]
        # norm conservation: |g| within the roundings of two evaluations -- a term's 16 (the exponent's |p| <= 8, the square, s, the
        # increment's five operations), the lane's chain of ic / 256 additions and the tree's 8; twice for the two logs' arguments, twice
        # for the neighbouring a2 whose g has the other sign
        g = float(res["match"][7])
        assert abs(g) <= 4 * (16 + ic / R.LANES + 8) * eps_T, (tag, g)
        assert abs(float(res["match"][6] / res["match"][5]) - 1) <= 4 * (16 + ic / R.LANES + 8) * eps_T
        # the five matching conditions: the polynomial's derivatives at x = 1 in longdouble against P0 .. P4, within the backward error
        # of a 5 x 5 elimination with partial pivoting, 32 eps Sum |A_kj| |a_j|
        c = res["coef"].astype(LD)
        n = np.arange(0, 13, 2)
        fall = np.ones(7, dtype=LD)
        for k in range(5):
            lhs, mag = np.sum(fall * c), np.sum(np.abs(fall * c))
            assert abs(lhs - res["match"][k]) <= 32 * eps_T * mag, (tag, k)
            fall = fall * (n - k)
        # zero curvature: one product and one division
        a2, a4 = c[1], c[2]
        assert abs(a2 * a2 + (2 * l + 5) * a4) <= 2 * eps_T * a2 * a2 * (1 + 1e-6), tag
        # u_ps positive inside, V_ps at the origin and continuous at r_c to the stencils' accuracy
        assert np.all(res["u_ps"][1:ic] > 0) and res["u_ps"][0] == 0
        assert abs(float(res["V_ps"][0] - (T(eps) + (2 * l + 3) * res["coef"][1] / (res["rc"] * res["rc"])))) <= 8 * eps_T * abs(float(res["V_ps"][0]))
        jump = float(abs(res["V_ps"][ic - 1] - (2 * V[ic] - V[ic + 1])))
        assert jump <= 1e-3 * abs(V[ic]), (tag, jump)
    print("%s: a2 %.6f, %d evaluations (float64), %d (longdouble), g %.2e" % (tag, f64["coef"][1], f64["iters"], ld["iters"], f64["match"][7]))


def test_every_status_bit():
    r, s, c, lam = R.tables(*R.GRIDS["log12"])
    V, u, eps = R.hydrogenic_channel(2, 0, r)
    ic = R.default_ic(r, u, R.FACTOR)

    def nans(res):
        return all(np.all(np.isnan(np.asarray(res[k], dtype=np.float64))) for k in ("u_ps", "V_ps", "coef", "rc", "match"))
    # a NaN node, an infinite eigenvalue
    Vn = V.copy()
    Vn[ic + 500] = np.nan
    for res in (R.pseudize(Vn, u, 0, eps, ic, r, s, lam), R.pseudize(V, u, 0, np.inf, ic, r, s, lam)):
        assert res["status"] == R.NONFINITE and nans(res) and res["iters"] == 0
    # the core node inside the node of 2s (r = 2 / Z = 0.2), and on an exact zero
    inner = int(np.argmin(np.abs(r - 0.1)))
    res = R.pseudize(V, u, 0, eps, inner, r, s, lam)
    assert res["status"] == R.NODES and nans(res)
    uz = u.copy()
    uz[ic] = 0.0
    assert R.pseudize(V, uz, 0, eps, ic, r, s, lam)["status"] == R.NODES
    # no bracket: an all-electron norm that overflows (its increments are inf - inf) makes g(0) NaN
    ub = u.copy()
    ub[5:ic - 10] = 1e200
    res = R.pseudize(V, ub, 0, eps, ic, r, s, lam)
    assert res["status"] == R.NOBRACKET and nans(res) and res["iters"] == 1
    # no bracket after the whole walk: an eigenvalue of -1e4 Ha leaves g of one sign at all 49 trial values
    res = R.pseudize(V, u, 0, -1e4, ic, r, s, lam)
    assert res["status"] == R.NOBRACKET and nans(res) and res["iters"] == 1 + 2 * R.BRACKET_STEPS
    # not positive: the guard of exp's underflow.  No input was found that ends the search and underflows (scans of eps over +-1e2 ..
    # 1e8 end in DFTA_PS_NOBRACKET first); an a2 handed to the model, -1e6, shows the bit and its NaNs
    res = R.pseudize(V, u, 0, eps, ic, r, s, lam, a2=-1e6)
    assert res["status"] == R.NOTPOSITIVE and nans(res)
    # the cap (no input built here reaches it: see the module's docstring), through the model's own constant
    keep = R.ITER_CAP
    try:
        R.ITER_CAP = 20
        res = R.pseudize(V, u, 0, eps, ic, r, s, lam)
    finally:
        R.ITER_CAP = keep
    assert res["status"] == R.CAP and nans(res) and res["iters"] == 20


# ---- end to end -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", R.E2E_CASES)
def test_end_to_end_with_the_oracles_level_solver_and_the_outward_sweep(runs, tag):
    (V, u, l, eps, ic), f64, ld = runs(tag)
    eig, ldv, dE = R.check_potential(V, f64["V_ps"], l, eps, ic)
    print("%s: |eps' - eps| %.2e Ha, u'/u %.2e, E-difference %.2e" % (tag, eig, ldv, dE))
    _held(eig, R.E2E[tag][0], tag + " eigenvalue", R.EIG_FLOOR)
    _held(ldv, R.E2E[tag][1], tag + " u'/u")
    _held(dE, R.E2E[tag][2], tag + " E-difference")


# ---- the rounding gate --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ("H2s", "Ne_p", "Fe_d"))
def test_gate_passes_a_perturbed_model_and_fails_two_wrong_models(tag):
    """8 E + floor: a float64 model whose every exp and log is moved by +-1 ulp (a seed the floor has not seen) stays within the gate;
    the model with the wrong sign in p''' and the model without the lam term of d2/dr2 miss it by more than 10^3"""
    V, u, l, eps, ic = R.case(tag)
    r, s, c, lam = R.tables(*R.GRIDS["log12"])
    ld, f64, gates = R.gate(V, u, l, eps, ic, r, s, lam)
    pert = R.distances(R.pseudize(V, u, l, eps, ic, r, s, lam, perturb=R.Perturb(1234)), ld)
    worst = max(pert[q] / gates[q] for q in R.GATED)
    print("%s: perturbed model / gate %.3f" % (tag, worst))
    assert worst <= 1.0
    for wrong in ("p3sign", "nolam"):
        bad = R.pseudize(V, u, l, eps, ic, r, s, lam, wrong=wrong)
        assert bad["status"] == 0
        miss = max(R.distances(bad, ld)[q] / gates[q] for q in ("a2", "a0", "u_ps"))
        print("%s: wrong model %s / gate %.3g" % (tag, wrong, miss))
        assert miss > 1e3, (wrong, miss)


# ---- unscreening ------------------------------------------------------------------------------------------------------------------------
def test_ionic_potential_has_the_valence_coulomb_tail():
    """Ne after 30 steps of the CPU oracle (_pseudo_ref.oracle_tail says what the figure is made of): r V_ion at the last node but one is -N_valence = -8 within the recorded figure"""
    d = float(R.oracle_tail("Ne"))
    print("Ne: |r V_ion + 8| = %.3g" % d)
    _held(d, R.TAIL["Ne"], "Ne tail")


def test_ionic_model_on_two_channels():
    """the pointwise model: rho_v's node 0 takes the l = 0 limit, the local channel is the highest l, its beta is zero, V_ion differs
    between channels only inside the larger core"""
    r, s, c, lam = R.tables(*R.GRIDS["log12"])
    chans = [R.case(t) for t in ("Ne_s", "Ne_p")]
    res = [R.pseudize(V, u, l, eps, ic, r, s, lam) for V, u, l, eps, ic in chans]
    U, Vps = np.array([x["u_ps"] for x in res]), np.array([x["V_ps"] for x in res])
    Y = np.ones_like(U)
    out = R.ionic(U, Vps, [x["coef"][0] for x in res], [0, 1], [2.0, 6.0], Y, np.zeros(len(r)), r)
    assert out["loc"] == 1 and not out["beta"][1].any()
    assert out["rho_v"][0] == 2.0 * (np.exp(2.0 * res[0]["coef"][0]) / R.FOURPI) and np.all(out["rho_v"] > 0)
    assert abs(out["rho_v"][1] / out["rho_v"][0] - 1) < 1e-3                   # continuous at the origin
    icmax = max(ch[4] for ch in chans)
    assert np.array_equal(out["V_ion"][0][icmax:], out["V_ion"][1][icmax:]) and not out["beta"][0][icmax:].any()
    assert R.ionic(U, Vps, [x["coef"][0] for x in res], [0, 1], [2.0, 6.0], Y, np.zeros(len(r)), r, l_loc=0)["loc"] == 0
    q1, q2, m1, m2 = R.kb_sums(out["beta"][0], U[0], s)
    assert q2 > 0 and abs(q1) > 0 and R.kb_roundings(len(r)) == 6 + 17 + 9


def test_upf_file_parses_back_to_the_arrays(tmp_path):
    """examples/write_upf.py: every array and the header of a written file come back through xml.etree, value for value"""
    import importlib.util
    spec = importlib.util.spec_from_file_location("write_upf", os.path.join(ROOT, "examples", "write_upf.py"))
    W = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(W)
    rng = np.random.default_rng(5)
    n = 37
    r = np.cumsum(rng.random(n))
    kw = dict(element="Ne", z_valence=8.0, functional="SLA VWN NOGX NOGC", r=r, rab=rng.random(n), v_local=-rng.random(n), l_local=1,
              betas=[(0, 21, rng.standard_normal(n))], dij=[-1.2345678901234567], pswfc=[("2S", 0, 2.0, rng.random(n)), ("2P", 1, 6.0, rng.random(n))],
              rho_atom=rng.random(n))
    path = str(tmp_path / "Ne.upf")
    W.write_upf(path, **kw)
    got = W.read_upf(path)
    for q in ("r", "rab", "v_local", "rho_atom"):
        assert np.array_equal(got[q], kw[q]), q
    assert got["header"]["element"] == "Ne" and float(got["header"]["z_valence"]) == 8.0 and got["header"]["l_local"] == "1"
    assert got["header"]["number_of_proj"] == "1" and got["header"]["number_of_wfc"] == "2" and got["header"]["mesh_size"] == str(n)
    assert len(got["betas"]) == 1 and got["betas"][0][:2] == (0, 21) and np.array_equal(got["betas"][0][2], kw["betas"][0][2])
    assert np.array_equal(got["dij"], np.array([[kw["dij"][0]]]))
    for a, b in zip(got["pswfc"], kw["pswfc"]):
        assert a[:3] == b[:3] and np.array_equal(a[3], b[3])
    tags = [e.tag for e in __import__("xml.etree.ElementTree").etree.ElementTree.parse(path).getroot().iter()]
    for t in ("PP_R", "PP_RAB", "PP_LOCAL", "PP_BETA.1", "PP_DIJ", "PP_PSWFC", "PP_RHOATOM"):
        assert t in tags, t


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
    assert int(defines["DFTA_ABI_VERSION"]) == D.ABI_VERSION == 7         # entries were added, no struct grew
    assert (int(defines["DFTA_PS_COEF"]), int(defines["DFTA_PS_MATCH"])) == (D.PS_COEF, D.PS_MATCH) == (R.COEF, R.MATCH)
    names = ("NOBRACKET", "CAP", "NODES", "NONFINITE", "NOTPOSITIVE")
    assert tuple(int(defines["DFTA_PS_" + n]) for n in names) == tuple(getattr(D, "PS_" + n) for n in names) \
        == (R.NOBRACKET, R.CAP, R.NODES, R.NONFINITE, R.NOTPOSITIVE)
    lib = D.load()
    assert all(hasattr(lib, n) for n in NEW_SYMBOLS)
    for f in (D.pseudize, D.pseudo_ionic, D.Scf.pseudopotentials, D.default_valence, D.default_ic):
        assert callable(f)
    plan = open(os.path.join(ROOT, "dftatom_amd", "csrc", "pseudo_plan.h")).read()
    for name, val in (("kLanes", R.LANES), ("kEdge", R.EDGE), ("kBracketSteps", R.BRACKET_STEPS), ("kIterCap", R.ITER_CAP), ("kCoef", R.COEF)):
        assert "%s = %d;" % (name, val) in plan, name


def test_front_end_usage_names_the_pseudo_table():
    """dftatom_cli without arguments (no GPU needed): the usage text names the table; a bad factor is refused before anything runs"""
    import subprocess
    compat = os.path.join(ROOT, "dftatom_amd", "compat")
    exe = os.path.join(compat, "dftatom_cli")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-C", compat])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "--pseudo-table" in r.stderr
    r = subprocess.run([exe, "10", "12", "0.5", "25", "0.002", "0", "--pseudo-table=-1"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "bad pseudo table" in r.stderr


def test_default_valence_of_the_library_is_the_rule():
    """host integers only: no device is needed"""
    import dftatom_amd as D
    import _oracle as O
    for Z in (1, 3, 10, 14, 18, 26, 29, 36, 46, 79, 86):
        n, l, occ = (list(x) for x in zip(*O.subshells(Z)))
        assert list(D.default_valence(n, l, occ)) == R.default_valence(n, l, occ), Z
    n, l, occ = (list(x) for x in zip(*O.subshells(26)))
    assert [(n[k] + 1, l[k]) for k in D.default_valence(n, l, occ)] == [(4, 0), (3, 2)]          # Fe: 4s, 3d
    n, l, occ = (list(x) for x in zip(*O.subshells(18)))
    assert [(n[k] + 1, l[k]) for k in D.default_valence(n, l, occ)] == [(3, 0), (3, 1)]          # Ar: 3s, 3p
    with pytest.raises(D.DftaError):
        D.default_valence([0, 1], [0, -1], [2, 1])


def test_host_planner_stand_alone_under_sanitizers(tmp_path):
    """dftatom_amd/csrc/pseudo_plan.cpp is pure host code: a stand-alone program (tests/pseudo_plan_main.cpp) built with ASan + UBSan
    walks the validation, the valence rule and the default core node; its lines are checked here"""
    import shutil
    import subprocess
    here = os.path.dirname(os.path.abspath(__file__))
    csrc = os.path.join(here, "..", "dftatom_amd", "csrc")
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler is needed"
    exe = str(tmp_path / "pseudo_plan_main")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", csrc, "-o", exe,
                    os.path.join(here, "pseudo_plan_main.cpp"), os.path.join(csrc, "pseudo_plan.cpp")], check=True, timeout=300)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, (run.stdout, run.stderr)
    lines = run.stdout.strip().split("\n")
    assert lines == ["valence Fe 2 6 5", "valence Ar 2 3 4", "valence H 1 0 -1", "valence Fe2+ 3 3 4 5", "ic 10 12 61 10", "ic0 61"], lines
    # the same core nodes from the restated rule
    r = 0.25 * np.arange(65)
    u = r * (2.0 - r) * np.exp(-r)
    assert [R.default_ic(r, u, f) for f in (1.5, 6.0, 1e3, 1e-3)] == [10, 12, 61, 10]
    u[10:] = 0
    assert R.default_ic(r, u, 1.5) == 61
