"""CPU suite: the reference of the Kleinman-Bylander block, tests/_kb_ref.py, held to what it must reproduce on its own -- no GPU.

  - with beta == 0 and q1 = 1 the model IS the continuum block's model, bit for bit (logderiv, rows), and B_h is its partner sum;
  - float64 against longdouble on analytic channels; the combination is continuous and the homogeneous freedom of u_p drops out;
  - the restated search finds the box states of hydrogen and closes every bracket to neighbouring doubles in about 9 rounds;
  - the figures of MEASURED (the gates of tests/test_gpu_kb.py) are what the CPU model gives on the CPU oracle's neon;
  - the planted ghost of (c): clean at A = 0, a ghost at A = GHOST_A with the stated margin, both verdicts agreeing;
  - the header declares the new entries and dftatom_amd binds them.
"""
import os
import re

import numpy as np
import pytest

import _continuum_ref as C
import _kb_ref as K

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
NEW_SYMBOLS = ("dfta_kb_sweep", "dfta_kb_bound_states", "dfta_kb_ghost_report")
LD = K.LD


@pytest.mark.parametrize("name", ["log12", "uni10", "uni3"])
def test_zero_projector_is_the_continuum_model(name):
    r, s, c, lam = K.tables(*K.GRIDS[name])
    N = len(r)
    V = K.hydrogen_like(r, 3.0, 0)[0]
    ends = [m for m in (3, 255, 256, 257, N - 2) if m <= N - 2]
    E = np.repeat([-2.0, 0.0, 0.7], len(ends))
    m = np.tile(ends, 3)
    for l in (0, 2, 4):
        a = K.sweep(V, l, np.zeros(N), 1.0, E, m, r, s, c, lam, want_rows=True)
        b = C.sweep(V, l, E, m, r, s, c, lam, want_rows=True)
        assert not a["status"].any() and np.all(a["D"] == 1) and np.all(a["Bh"] == 0) and np.all(a["Bp"] == 0)
        assert np.array_equal(a["logderiv"], b["logderiv"])
        assert np.array_equal(a["rows"] * np.where(E > 0, b["scale"], 1.0)[:, None], b["rows"])
    cut = min(200, N - 2)
    beta = K.hydrogen_like(r, 3.0, 1, cut)[1]
    ok = m >= cut
    a = K.sweep(V, 1, beta, 0.75, E[ok], m[ok], r, s, c, lam)
    b = C.sweep(V, 1, E[ok], m[ok], r, s, c, lam, P=beta[None, :], power=0)
    neg = E[ok] <= 0
    assert np.array_equal(a["Bh"][neg], b["sums"][neg, 0])


def test_float64_against_longdouble_and_the_freedom_of_the_particular_solution():
    r, s, c, lam = K.tables(*K.GRIDS["log12"])
    N = len(r)
    E = np.array([-1.5, -0.2, 0.0, 0.8])
    for l in range(5):
        V, beta, q1 = K.smooth_well(r, 4.0, l, 2600)
        f64 = K.sweep(V, l, beta, q1, E, 3000, r, s, c, lam)
        ld = K.sweep(V, l, beta, q1, E, 3000, r, s, c, lam, dtype=LD)
        assert np.max(np.abs((f64["logderiv"] - ld["logderiv"]) / ld["logderiv"])) < 1e-9
        # logderiv does not depend on q1's companion: scaling beta by t and q1 by t^2 leaves H, hence u'/u
        t = 1.7
        sc = K.sweep(V, l, t * beta, t * t * q1, E, 3000, r, s, c, lam, dtype=LD)
        assert np.max(np.abs((sc["logderiv"] - ld["logderiv"]) / ld["logderiv"])) < 1e-12
    # the model's status: a NaN node of beta or of V
    V, beta, q1 = K.hydrogen_like(r, 3.0, 1, 257)
    bn = beta.copy()
    bn[200] = np.nan
    assert K.last_nonzero(bn) == 256 and K.sweep(V, 1, bn, q1, [-1.0], [300], r, s, c, lam)["status"][0] != 0
    Vn = V.copy()
    Vn[300] = np.nan
    st = K.sweep(Vn, 1, beta, q1, [-1.0, -1.0], [298, 299], r, s, c, lam)["status"]
    assert st[0] == 0 and st[1] != 0


def test_search_finds_the_box_states_of_hydrogen():
    r, s, c, lam = K.tables(*K.GRIDS["uni11"])
    N = len(r)
    V = K.hydrogen_like(r, 1.0, 0)[0]
    zero = np.zeros(N)
    (en, rounds, status), = K.search(K.model_signs(V, 0, zero, 1.0, N - 2, r, s, c, lam), [(-1.0, -0.04)], 128)
    assert status == 0 and 8 <= rounds <= 11
    assert len(en) == 3 and np.max(np.abs(en[:2] - np.array([-0.5, -0.125]))) < 2e-4 and abs(en[2] + 1 / 18.0) < 5e-3, en      # (3s feels the box)
    sg = K.model_signs(V, 0, zero, 1.0, N - 2, r, s, c, lam)(0, np.array([en[0], np.nextafter(en[0], 0.0)]))
    assert sg[1][0] != sg[1][1]                                           # the state's bracket is a pair of neighbouring doubles
    # a repulsive projector on the 1s-like state pushes the lowest state up and leaves the count
    beta = K.hydrogen_like(r, 1.0, 0, 600)[1]
    (en2, _, st2), = K.search(K.model_signs(V, 0, beta, 0.75, N - 2, r, s, c, lam), [(-1.0, -0.04)], 128)
    assert st2 == 0 and len(en2) == 3 and en2[0] > en[0] + 1e-3


def test_measured_figures_of_neon():
    fig = K.measure(("Ne",))
    for where in ("rc", "end"):
        got, kept = fig["identity"][("Ne_s", where)], K.MEASURED["identity"][("Ne_s", where)]
        for g, k in zip(got, kept):
            assert k / 1.5 <= g <= k, (where, got, kept)
    assert K.MEASURED["lowest"]["Ne_s"] / 1.5 <= fig["lowest"]["Ne_s"] <= K.MEASURED["lowest"]["Ne_s"], fig["lowest"]
    assert set(K.MEASURED["lowest"]) == {"Ne_s", "Ar_s", "Fe_s"} and len(K.MEASURED["identity"]) == 6


def test_iron_has_a_ghost_on_the_cpu():
    """the 4s channel of iron with the d channel local: a state of H_KB 11.34 Ha below eps_ref, and GKS agrees"""
    at = K.atom_channels("Fe")
    r, s, c, lam = at["r"], at["s"], at["c"], at["lam"]
    N, loc = len(r), at["channels"][at["loc"]]
    (_, ch), = K.nonlocal_channels(at)
    assert loc["l"] == 2 and ch["l"] == 0 and ch["E_KB"] > 0
    en = K.search(K.model_signs(loc["V_ps"], 0, ch["beta"], ch["q1"], N - 2, r, s, c, lam), [(K.SEARCH_LO, 0.0)], 512)[0][0]
    e = K.local_levels(loc["V_ps"], 0, N - 2, -40.0, r, s, c, lam, nscan=1024)
    assert len(en) == 2 and abs(en[0] - K.MEASURED["lowest_E"]["Fe_s"]) < 1e-6 and abs(en[1] - ch["eps"]) < 1e-8
    assert K.MEASURED["lowest"]["Fe_s"] / 1.5 <= abs(en[0] - ch["eps"]) <= K.MEASURED["lowest"]["Fe_s"]
    assert e[1] < ch["eps"] and K.gks_verdict(ch["E_KB"], e[0], e[1], ch["eps"]) == 1 == K.MEASURED["ghost"]["Fe_s"]


def test_planted_ghost_on_the_cpu():
    clean, ghost = K.ghost_case(0.0), K.ghost_case()
    assert clean["gks"] == 0 and clean["direct"] == 0 and len(clean["states"]) == 1
    assert ghost["gks"] == 1 and ghost["direct"] == 1 and len(ghost["states"]) == 2
    assert abs(ghost["local"][1] - K.GHOST_E1) < 1e-3 and abs(ghost["eps"] - K.GHOST_EPS) < 1e-4
    assert ghost["local"][1] < ghost["eps"] - 1.3 and ghost["states"][0] < ghost["eps"] - 1.3        # the margin
    for case in (clean, ghost):
        assert abs(case["states"][-1] - case["eps"]) < 1e-9                                            # eps_ref stays a state


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
    assert (int(defines["DFTA_KB_MAX_STATES"]), int(defines["DFTA_KB_REPORT"])) == (D.KB_MAX_STATES, D.KB_REPORT) == (K.MAX_STATES, 10)
    names = ("NONFINITE", "FULL", "CAP")
    assert tuple(int(defines["DFTA_KB_SEARCH_" + n]) for n in names) == tuple(getattr(D, "KB_SEARCH_" + n) for n in names) \
        == (K.SEARCH_NONFINITE, K.SEARCH_FULL, K.SEARCH_CAP)
    assert (int(defines["DFTA_CONT_NONFINITE"]), int(defines["DFTA_CONT_STEP"])) == (K.NONFINITE, K.STEP)
    lib = D.load()
    assert all(hasattr(lib, n) for n in NEW_SYMBOLS)
    for f in (D.kb_sweep, D.kb_bound_states, D.kb_ghost_report, D.Scf.kb_ghost_report):
        assert callable(f)
