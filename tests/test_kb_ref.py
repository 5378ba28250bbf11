"""CPU suite: the reference of the Kleinman-Bylander block, tests/_kb_ref.py, held to what it must reproduce on its own -- no GPU.

  - with beta == 0 and q1 = 1 the model IS the continuum block's model, bit for bit (logderiv, rows), and B_h is its partner sum;
  - float64 against longdouble on analytic channels; the combination is continuous and the homogeneous freedom of u_p drops out;
  - the restated search finds the box states of hydrogen and closes every bracket to neighbouring doubles in about 9 rounds;
  - the figures of MEASURED (the gates of tests/test_gpu_kb.py) are what the CPU model gives on the CPU oracle's neon;
  - the planted ghost of (c): clean at A = 0, a ghost at A = GHOST_A with the stated margin, both verdicts agreeing;
  - dftatom_amd/csrc/kb_plan.cpp on its own in a stand-alone program under ASan + UBSan (tests/kb_plan_main.cpp): last_nonzero (zero rows,
    -0.0, NaN, the first and the last node), every refusal of check, plan (groups of 1, 63, 64, 65 and 129 trials of interleaved
    channels; the chunk of rows from the header's constants, forced, capped, when nothing fits), scan_energy / cut_energy /
    bracket_closed on ranges down to neighbouring doubles, open_brackets and cut_bracket called directly, and search on synthetic sign
    functions -- several channels and closing rounds in one call, 8 and 9 roots (FULL), windows that are not finite over a root, below
    and ABOVE the picked pair and over the low end of round 0, no root, a failing evaluation, the widest range, the cap --, equal to
    search() here in count, energies (bit for bit), rounds and status;
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


def _synthetic_signs(chans):
    """signs() of tests/kb_plan_main.cpp's searches: u(E) = Prod_j (E - root_j), the factors multiplied in order; inside a window the value
    is not finite (kind 0: NaN, 1: a status bit, 2: +inf, 3: -inf)"""
    def signs(k, E):
        _, _, roots, windows = chans[k]
        E = np.asarray(E, dtype=np.float64)
        u = E - roots[0]
        for root in roots[1:]:
            u = u * (E - root)
        fin = np.ones(len(E), bool)
        for lo, hi, kind in windows:
            inside = (lo < E) & (E < hi)
            fin &= ~inside
            if kind != 1:
                u = np.where(inside, {0: np.nan, 2: np.inf, 3: -np.inf}[kind], u)
        return fin & np.isfinite(u), u < 0
    return signs


def test_host_planner_stand_alone_under_sanitizers(tmp_path):
    """dftatom_amd/csrc/kb_plan.cpp is pure host code: a stand-alone program (tests/kb_plan_main.cpp) built with ASan + UBSan and without
    contraction walks last_nonzero, check, plan, the search's formulas, open_brackets, cut_bracket and the whole search on synthetic sign
    functions.  It holds its own expectations (exit status 0); every line that _kb_ref restates is compared here, doubles bit for bit."""
    import shutil
    import subprocess
    here = os.path.dirname(os.path.abspath(__file__))
    csrc = os.path.join(here, "..", "dftatom_amd", "csrc")
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler is needed"
    exe = str(tmp_path / "kb_plan_main")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off", "-I", csrc,
                    "-o", exe, os.path.join(here, "kb_plan_main.cpp"), os.path.join(csrc, "kb_plan.cpp")], check=True, timeout=300)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    lines = [ln.split() for ln in run.stdout.strip().split("\n")]
    hx = float.fromhex
    bits = lambda a: np.asarray(a, dtype=np.float64).view(np.uint64)      # noqa: E731

    # the searches first: where the program and the model part, that is the finding
    searches, at = {}, 0
    while at < len(lines):
        if lines[at][0] != "search":
            at += 1
            continue
        name, nscan, nch = lines[at][1], int(lines[at][2]), int(lines[at][3])
        chans, results = [], []
        for k in range(nch):
            w = lines[at + 1 + 2 * k]
            assert w[0] == "chan"
            nr = int(w[3])
            rest = w[4 + nr:]
            chans.append((hx(w[1]), hx(w[2]), [hx(x) for x in w[4:4 + nr]],
                          [(hx(rest[q]), hx(rest[q + 1]), int(rest[q + 2])) for q in range(0, len(rest), 3)]))
            w = lines[at + 2 + 2 * k]
            assert w[0] == "result" and len(w) == 4 + K.MAX_STATES
            results.append((int(w[1]), int(w[2]), int(w[3]), np.array([hx(x) for x in w[4:]])))
        searches[name] = (nscan, chans, results)
        at += 1 + 2 * nch
    for name, (nscan, chans, results) in searches.items():
        ref = K.search(_synthetic_signs(chans), [(c[0], c[1]) for c in chans], nscan)
        for k, ((count, rounds, status, en), (ren, rrounds, rstatus)) in enumerate(zip(results, ref)):
            assert (count, rounds, status) == (len(ren), rrounds, rstatus), (name, k, (count, rounds, status), (len(ren), rrounds, rstatus))
            assert np.array_equal(bits(en[:count]), bits(ren)) and np.all(np.isnan(en[count:])), (name, k, en, ren)
    assert run.returncode == 0, (run.stdout[-4000:], run.stderr[-4000:])
    want = {"two", "eight", "nine", "covered", "below0", "below1", "below2", "below3", "above", "above1", "lowend", "allbad", "none", "both",
            "widest", "cap"}
    assert set(searches) == want
    status = {name: [r[2] for r in s[2]] for name, s in searches.items()}
    assert status["two"] == [0] * 5 and [r[0] for r in searches["two"][2]] == [2, 3, 0, 1, 1] and searches["two"][2][2][1] == 1
    assert len({r[1] for r in searches["two"][2]}) >= 3                                      # the channels close in different rounds
    assert status["eight"] == [0] and status["nine"] == [K.SEARCH_FULL] and status["both"] == [K.SEARCH_FULL | K.SEARCH_NONFINITE, 0]
    assert all(status[n] == [K.SEARCH_NONFINITE] for n in ("below0", "below1", "below2", "below3", "above", "above1"))
    assert searches["above"][2][0][:2] == (3, 10)                                             # the reproducer: three states, ten rounds
    assert status["covered"] == status["lowend"] == status["allbad"] == status["none"] == [0]
    assert status["widest"] == [0, 0, 0, 0] and max(r[1] for r in searches["widest"][2]) <= 13
    assert status["cap"] == [K.SEARCH_CAP, 0] and searches["cap"][2][0][1] == K.MAX_ROUNDS

    # last_nonzero: the program's six rows
    N = 7
    rows = np.zeros((6, N))
    rows[1] = -0.0
    rows[2, 3] = np.nan
    rows[3, 0] = 2.0
    rows[4, N - 1] = -1e-300
    rows[5, 2], rows[5, 4] = 1.0, -0.0
    (got,) = [w[1:] for w in lines if w[0] == "lastnz"]
    assert [int(x) for x in got] == [K.last_nonzero(row) for row in rows] == [0, 0, 3, 0, N - 1, 2]
    assert [w for w in lines if w[0] == "check"] == [["check", "21"]]

    # plan: (N, trials, rows wanted, forced chunk) -> (waves, padded positions, waves per chunk of rows)
    plans = {tuple(int(x) for x in w[1:5]): tuple(int(x) for x in w[5:]) for w in lines if w[0] == "plan"}
    assert 2 * 8 * 64 * 4097 * 63 <= 256 << 20 < 2 * 8 * 64 * 4097 * 64 and 2 * 8 * 64 * 65537 * 3 <= 256 << 20 < 2 * 8 * 64 * 65537 * 4
    assert plans == {
        (4097, 322, 0, 0): (8, 512, 0),                    # groups of 1, 63, 64, 65 and 129 trials: 1 + 1 + 1 + 2 + 3 waves; no rows
        (4097, 322, 1, 0): (8, 512, 8),                    # fewer waves than fit: the wave count
        (4097, 322, 1, 1): (8, 512, 1), (4097, 322, 1, 2): (8, 512, 2), (4097, 322, 1, 3): (8, 512, 3), (4097, 322, 1, 100): (8, 512, 8),
        (4097, 4096, 1, 0): (64, 4096, 63),                # 2 x 8 x 64 x 4097 bytes a wave: 63 fit 256 MiB
        (65537, 320, 1, 0): (6, 384, 3),
        (131073, 66, 1, 0): (3, 192, 1),
        (9, 70000, 1, 0): (1094, 70016, 1023),             # the combining launch's grid caps a chunk
        (9, 70000, 1, 2): (1094, 70016, 2),
        (300000, 65, 1, 0): (2, 128, 1),                   # no wave fits: 1
        (9, 0, 1, 0): (0, 0, 1),
    }

    # the formulas
    scans = [w for w in lines if w[0] == "scan"]
    cuts = [w for w in lines if w[0] == "cut"]
    assert len(scans) == 5 and len(cuts) == 9
    for w in scans:
        lo, hi, nscan = hx(w[1]), hx(w[2]), int(w[3])
        assert len(w) == 4 + nscan and np.array_equal(bits([hx(x) for x in w[4:]]), bits(K.scan_energies(lo, hi, nscan))), w[:4]
    widths = set()
    for w in cuts:
        a, b = hx(w[1]), hx(w[2])
        e = np.array([hx(x) for x in w[4:]])
        assert len(e) == K.CUTS and np.array_equal(bits(e), bits(K.cut_energies(a, b))) and bool(int(w[3])) == bool(K.closed(a, b)), w[:4]
        assert np.all((e >= a) & (e <= b))
        if a < 0 and b < 0 and b - a < 1e-15:
            widths.add(int(bits(a) - bits(b)))                             # (negative doubles: the bits descend)
    assert widths == {1, 2, 3}                                              # neighbours, one double between, three ulps
    assert lines[-1] == ["done", "0"]


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
