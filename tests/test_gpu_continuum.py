"""GPU suite (-m gpu): continuum orbitals -- dftatom_amd/csrc/continuum.hip (k_partner_weight, k_continuum, k_continuum_scale),
include/dftatom_hip.h has the arithmetic, tests/_continuum_ref.py restates it in float64 (the model of the kernel) and in longdouble
(the replay) and holds the closed forms.

Two kinds of check.  Everything the device computes with + - * / sqrt alone -- u'/u, the node count, the status, and the sums and rows
of a trial with E <= 0 (factor 1) -- must equal the float64 model BIT FOR BIT.  Everything that passes through the normalisation (the
device's sin, cos, atan2, hypot) is held to the longdouble replay on the same float64 inputs at 8 E + floor (_continuum_ref.gate: E the
model's own distance from the replay, floor the model's change under +-1 ulp on every division, 8 seeds); against closed forms at twice
the replay's measured distance (_continuum_ref.MEASURED) plus that rounding gate.

a. shapes      uniform grids of 9, 1025 and 2049 nodes and log12; end nodes 3, 255, 256, 257, N-2; l = 0 .. 4 and three potentials in one
               call; partner lists of 0, 1, 4, 5 and 16 rows; E <= 0 and E > 0; rows; both normalisations.
b. closed      log13 and uni13: the free particle (delta_l = 0, rows = sqrt(2 / (pi k)) x j_l, overlaps with Z = 10 orbitals against
               the closed momentum orbitals AND against the device's own bessel_transform, dipole sums against sympy), Coulomb Z = 10
               (u'/u against mpmath's F_l at E = 0.5, 8 and against the n = 4 bound orbitals, nodes = n - l - 1, WKB-normalised rows
               against sqrt(2 / (pi k)) F_l), the hydrogen 1s cross section at omega = 0.51, 1, 2.
c. replay      Scf.continuum on Ne LDA, N LSDA and the batch [H, Ne, Fe] after three steps: == continuum() on Scf.array(3 / 4) and
               Scf.orbitals(), and every output against the replay.
d. bits        a trial alone == among 128 others at any position == in reversed order == a repeated call; rows asked for or not; the
               kernel's instance 4, 8 or 16; trial counts 1, 63, 64, 65, 129; frozen atoms keep their outputs while a live atom moves on.
e. edges       a NaN node poisons the trials of its potential that reach it, and no other; the error paths; zero trials.
f. physics     Ne after 40 steps: the overlaps of eps s with 1s and 2s at twice the CPU reference's figure; sigma_2p positive and falling.
g. front end   dftatom_cli --phase-shift-table and --photo-table: the figures of Scf.continuum / Scf.photoionization, nothing else changes.
h. chunks      rows in two chunks, cut by the 1023-wave cap (1100 one-trial waves on 9 nodes) and by the 256 MiB budget (520 on 1025
               nodes): block0 > 0, pos0, the host scatter, the row buffer's second use (second-chunk trials end early: a stale row
               shows), the timer; every trial == its like in a one-chunk call that is held to the model and the replay.
i. loops       the second pass of k_partner_weight's grid-stride loop (1100 rows x 2049 nodes, a list from both ends) and of
               k_continuum_scale's (16385 nodes: the last node of a full row).
j. exits       DFTA_CONT_NONFINITE without STEP (overflow behind a barrier, status exactly [1, 1, 0, 0], the finite lanes of the wave
               untouched); DFTA_CONT_NORM (l = 4 at E = 1e-300; E = 1e-150 gives scale 0.0 and no bit).
k. ranges      power 2, 3, 8; E = 1e-100 .. 1e-4 for l = 0 .. 4; Scf.continuum with end nodes given (inside c.).
l. photo rows  every row of Scf.photoionization for Yb LDA (4f, 5p, 4d) and LSDA [N, Cu] (open shells, beta rows, atom 1) rebuilt
               from Scf.continuum and Scf.levels in the header's order, bit for bit; sigma is NaN exactly under a status bit.

Every test prints the largest ratio to its gate that it observed.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import _continuum_ref as R               # noqa: E402
import dftatom_amd as D                  # noqa: E402

LD = R.LD
ALPHA = 0.5


@pytest.fixture(scope="module")
def ctx(torch_first):
    assert np.finfo(LD).eps < 1.2e-19, "the reference of this file needs an extended np.longdouble"
    c = D.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def grids(ctx):
    """name -> (grid, (r, s, c, lam) as the library holds them)"""
    made = {}

    def get(name):
        if name not in made:
            L, d, Rm = R.GRIDS[name]
            g = D.Grid(ctx, L, d, Rm)
            tab = R.tables(L, d, Rm)
            assert np.array_equal(g.r(), tab[0]), "the reference's r table is not the library's"
            made[name] = (g, tab)
        return made[name]
    yield get
    for g, _ in made.values():
        g.close()


def _potentials(r):
    """free, Coulomb Z = 10, Yukawa: (3, N)"""
    V = np.zeros((3, len(r)))
    V[1, 1:] = -10.0 / r[1:]
    V[2, 1:] = -10.0 * np.exp(-r[1:]) / r[1:]
    return V


def _partners(r, count):
    """`count` smooth made-up rows that vanish at the origin"""
    return np.array([r ** (1 + k % 3) * np.exp(-(0.6 + 0.15 * k) * r) * (1 - 0.1 * k * r) for k in range(count)])


def _bitwise(out, ref, sel, nb, what):
    """the scale-free outputs of the trials `sel` equal the model bit for bit; so do the sums and rows of its trials with E <= 0"""
    for q in ("logderiv", "nodes", "status"):
        assert np.array_equal(out[q][sel], ref[q], equal_nan=True), (what, q)
    raw = np.asarray(ref["scale"]) == 0
    assert np.array_equal(out["scale"][sel][raw], ref["scale"][raw]) and np.array_equal(out["delta"][sel][raw], ref["delta"][raw]), what
    if nb:
        assert np.array_equal(out["sums"][sel][raw][:, :nb], ref["sums"][raw], equal_nan=True), (what, "sums")
        assert not out["sums"][sel][:, nb:].any(), (what, "sums beyond the list")
    if "rows" in out and "rows" in ref:
        assert np.array_equal(out["rows"][sel][raw], ref["rows"][raw], equal_nan=True), (what, "rows")


def _gated(out, sel, nb, ld, gates, what):
    """every normalised output of the trials `sel` within the gate of the replay; returns the largest ratio"""
    got = {"logderiv": out["logderiv"][sel], "delta": out["delta"][sel], "scale": out["scale"][sel],
           "sums": out["sums"][sel][:, :nb] if nb else np.zeros((len(sel), 0))}
    if "rows" in out and "rows" in ld:
        got["rows"] = out["rows"][sel]
    dist = R.distances(got, ld)
    worst = 0.0
    ok = np.isfinite(np.asarray(ld["scale"], dtype=np.float64))
    for q in R.QUANTITIES:
        d, g = dist[q][ok], gates[q][ok]
        ratio = np.where(d == 0, 0.0, d / np.where(g > 0, g, 1e-300))        # (a quantity that is exact has gate 0)
        assert np.all(d <= g), (what, q, float(ratio.max()))
        if ok.any():
            worst = max(worst, float(ratio.max()))
    assert np.array_equal(np.isnan(out["scale"][sel]), np.isnan(np.asarray(ld["scale"], dtype=np.float64))), what
    return worst


# ---- a. shapes ----------------------------------------------------------------------------------------------------------------------------
LIST_OF_L = {0: -1, 1: 0, 2: 1, 3: 2, 4: 3}            # l -> its partner list: none, 1, 4, 5, 16 rows
LISTS = [[3], [0, 5, 9, 15], [1, 2, 4, 8, 14], list(range(16))]
PAIRS = ((0, 0), (0, 3), (1, 1), (1, 4), (2, 2))        # (potential, l): l = 0 .. 4 and three potentials in one call
ENERGIES = (-3.0, 0.0, 0.005, 0.5, 8.0)


@pytest.mark.parametrize("mode", (R.FREE, R.WKB))
@pytest.mark.parametrize("name", ("uni3", "uni10", "uni11", "log12"))
def test_small_and_awkward_shapes(ctx, grids, name, mode):
    grid, (r, s, c, lam) = grids(name)
    N = grid.N
    V, P = _potentials(r), _partners(r, 16)
    ends = [m for m in (3, 255, 256, 257, N - 2) if 3 <= m <= N - 2]
    trials = [(v, l, e, m) for v, l in PAIRS for m in ends for e in ENERGIES]
    vidx, l, E, m = (np.array(x) for x in zip(*trials))
    tl = np.array([LIST_OF_L[x] for x in l])
    out = D.continuum(ctx, grid, V, l, E, m, vidx, norm=mode, partners=P, power=1, lists=LISTS, trial_list=tl, want_rows=True)
    assert ctx.last_kernel_ms() > 0
    worst = 0.0
    for v, ll in PAIRS:
        sel = np.where((vidx == v) & (l == ll))[0]
        Pl = P[LISTS[LIST_OF_L[ll]]] if LIST_OF_L[ll] >= 0 else None
        nb = 0 if Pl is None else len(Pl)
        ld, f64, gates = R.gate(V[v], ll, E[sel], m[sel], r, s, c, lam, mode, Pl, 1, want_rows=True)
        _bitwise(out, f64, sel, nb, (name, v, ll))
        worst = max(worst, _gated(out, sel, nb, ld, gates, (name, v, ll)))
    print("%s mode %d: %d trials, largest ratio to the gate %.3f" % (name, mode, len(E), worst))


# ---- b. closed forms ----------------------------------------------------------------------------------------------------------------------
def _group_ids():
    return [(name, k) for name in ("log13", "uni13") for k in range(len(R.CLOSED_TAGS))]


@pytest.fixture(scope="module")
def closed_cache():
    return {}


@pytest.mark.parametrize("name,k", _group_ids())
def test_closed_forms(ctx, grids, closed_cache, name, k):
    grid, (r, s, c, lam) = grids(name)
    if name not in closed_cache:
        closed_cache[name] = R.closed_groups(name)
    group = closed_cache[name][k]
    tag, V, l, E, m, mode, P, power, want_rows = group
    E = np.array(E)
    out = D.continuum(ctx, grid, V, np.full(len(E), l), E, np.full(len(E), m), norm=mode, partners=P, power=power, want_rows=want_rows)
    assert not out["status"].any()
    ld, f64, gates = R.gate(V, l, E, m, r, s, c, lam, mode, P, power, want_rows=want_rows)
    nb = 0 if P is None else len(P)
    sel = np.arange(len(E))
    _bitwise(out, f64, sel, nb, tag)
    if tag[0] == "bound":
        assert out["nodes"][0] == 4 - l - 1
    dist = R.closed_distance(name, group, out)
    rounding = R.closed_gate(group, ld, gates)
    worst = 0.0
    for key, d in dist.items():
        for j, dj in enumerate(d):
            bound = 2 * R.MEASURED[name][key][j] + rounding[key][j]
            assert dj <= bound, (name, key, j, dj, bound)
            worst = max(worst, dj / bound)
    if tag[0] == "free" and nb:            # the cross-check of the two kernels: S = sqrt(k) R~_nl(k) of the device's own Bessel transform
        k_ = np.sqrt(2 * E)
        bt = D.bessel_transform(ctx, grid, D.BT_ORBITAL, [l] * nb, P, k_)
        for b in range(nb):
            got, want = out["sums"][:, b], np.sqrt(k_) * bt[b]
            key = ("overlap", [nl for nl in R.OVERLAP_ORBITALS if nl[1] == l][b])
            bound = 2 * np.array(R.MEASURED[name][key]) + np.array(rounding[key]) + 64 * R.EPS * np.abs(want)
            assert np.all(np.abs(got - want) <= bound), (name, key, np.abs(got - want), bound)
            worst = max(worst, float(np.max(np.abs(got - want) / bound)))
    print("%s %s: largest ratio to the gate %.3f" % (name, tag, worst))


# ---- c. the replay on SCF potentials ------------------------------------------------------------------------------------------------------
SCF_E = (-0.3, 0.01, 0.1, 0.7, 3.0, 8.0)


@pytest.mark.parametrize("Z,lsda,ls", [([10], False, (0, 1, 2)), ([7], True, (0, 1, 2)), ([1, 10, 26], False, (0, 1))])
def test_scf_entry_is_the_direct_entry_and_both_follow_the_replay(ctx, grids, Z, lsda, ls):
    grid, (r, s, c, lam) = grids("log12")
    N = grid.N
    scf = D.Scf(ctx, grid, Z, lsda=lsda, alpha=ALPHA)
    try:
        with pytest.raises(D.DftaError):
            scf.continuum([0], [0.5], power=1)                                   # no orbitals before the first step
        pre = scf.continuum([0, 1], [0.5, 0.5])                                  # ... but the start potential can be swept
        assert np.array_equal(pre["logderiv"], D.continuum(ctx, grid, scf.array(3, 0), [0, 1], [0.5, 0.5])["logderiv"])
        for _ in range(3):
            scf.step()
        chans = [(a, sp) for a in range(len(Z)) for sp in ((0, 1) if lsda else (0,))]
        trials = [(a, sp, l, e) for a, sp in chans for l in ls for e in SCF_E]
        atom, spin, l, E = (np.array(x) for x in zip(*trials))
        out = scf.continuum(l, E, atom=atom, spin=spin, norm="auto", power=1, want_rows=True)
        assert ctx.last_kernel_ms() > 0
        worst = 0.0
        for a, sp in chans:
            V, U = scf.array(4 if sp else 3, a), scf.orbitals(a, sp)
            lv = scf.levels(a, sp)["l"]
            for ll in ls:
                sel = np.where((atom == a) & (spin == sp) & (l == ll))[0]
                rows = [b for b in range(len(lv)) if abs(int(lv[b]) - ll) == 1]
                assert all(list(out["partner_index"][t][:len(rows)]) == rows and np.all(out["partner_index"][t][len(rows):] == -1) for t in sel)
                direct = D.continuum(ctx, grid, V, l[sel], E[sel], partners=U, power=1, lists=[rows], want_rows=True)
                for q in ("logderiv", "nodes", "delta", "scale", "status", "sums", "rows"):
                    assert np.array_equal(direct[q], out[q][sel], equal_nan=True), (Z, a, sp, ll, q)
                P = U[rows] if rows else None
                ld, f64, gates = R.gate(V, ll, E[sel], N - 2, r, s, c, lam, R.FREE, P, 1, want_rows=True)
                _bitwise(out, f64, sel, len(rows), (Z, a, sp, ll))
                worst = max(worst, _gated(out, sel, len(rows), ld, gates, (Z, a, sp, ll)))
        again = scf.continuum(l, E, atom=atom, spin=spin, norm="auto", power=1, want_rows=True)
        assert all(np.array_equal(again[q], out[q], equal_nan=True) for q in out)
        if Z == [10]:                                                            # the end nodes given per trial
            m2 = np.array([3, 257, 2500, N - 2])[np.arange(len(E)) % 4]
            out2 = scf.continuum(l, E, m=m2, atom=atom, spin=spin, norm="auto", power=1, want_rows=True)
            V, U, lv = scf.array(3, 0), scf.orbitals(0, 0), scf.levels(0, 0)["l"]
            for ll in ls:
                sel = np.where(l == ll)[0]
                assert len(set(m2[sel])) == 4
                rows = [b for b in range(len(lv)) if abs(int(lv[b]) - ll) == 1]
                direct = D.continuum(ctx, grid, V, l[sel], E[sel], m2[sel], partners=U, power=1, lists=[rows], want_rows=True)
                for q in ("logderiv", "nodes", "delta", "scale", "status", "sums", "rows"):
                    assert np.array_equal(direct[q], out2[q][sel], equal_nan=True), (Z, "m given", ll, q)
                ld, f64, gates = R.gate(V, ll, E[sel], m2[sel], r, s, c, lam, R.FREE, U[rows], 1, want_rows=True)
                _bitwise(out2, f64, sel, len(rows), (Z, "m given", ll))
                worst = max(worst, _gated(out2, sel, len(rows), ld, gates, (Z, "m given", ll)))
            assert np.all(out2["rows"][np.arange(N)[None, :] > (m2 + 1)[:, None]] == 0)
    finally:
        scf.close()
    print("Z = %s %s: largest ratio to the gate %.3f" % (Z, "LSDA" if lsda else "LDA", worst))


# ---- d. bits ------------------------------------------------------------------------------------------------------------------------------
def _same(a, b, ia, ib, what, keys=("logderiv", "nodes", "delta", "scale", "status", "sums", "rows")):
    for q in keys:
        if q in a and q in b:
            assert np.array_equal(a[q][ia], b[q][ib], equal_nan=True), (what, q)


def test_a_trial_does_not_depend_on_its_company(ctx, grids):
    grid, (r, s, c, lam) = grids("log12")
    N = grid.N
    V, P = _potentials(r), _partners(r, 16)
    rng = np.random.default_rng(7)
    probe = dict(vidx=2, l=2, E=0.37, m=2500)
    alone = D.continuum(ctx, grid, V, [probe["l"]], [probe["E"]], [probe["m"]], [probe["vidx"]], norm=R.WKB, partners=P, power=1,
                        lists=[[0, 5, 9]], want_rows=True)
    assert alone["status"][0] == 0 and np.all(alone["rows"][0, probe["m"] + 2:] == 0) and alone["rows"][0, 0] == 0
    for count in (1, 63, 64, 65, 129):
        vidx = rng.integers(0, 3, count)
        l = rng.integers(0, 5, count)
        E = rng.choice([-1.0, 0.02, 0.37, 2.0], count)
        m = rng.integers(3, N - 1, count)
        for at in sorted({0, count // 2, count - 1}):
            vidx[at], l[at], E[at], m[at] = probe["vidx"], probe["l"], probe["E"], probe["m"]
            tl = np.where(l == 2, 0, -1)
            out = D.continuum(ctx, grid, V, l, E, m, vidx, norm=R.WKB, partners=P, power=1, lists=[[0, 5, 9]], trial_list=tl, want_rows=True)
            _same(out, alone, [at], [0], ("position", count, at))
            rev = D.continuum(ctx, grid, V, l[::-1], E[::-1], m[::-1], vidx[::-1], norm=R.WKB, partners=P, power=1, lists=[[0, 5, 9]],
                              trial_list=tl[::-1], want_rows=True)
            _same(rev, out, slice(None), slice(None, None, -1), ("reversed", count))
            norows = D.continuum(ctx, grid, V, l, E, m, vidx, norm=R.WKB, partners=P, power=1, lists=[[0, 5, 9]], trial_list=tl)
            _same(norows, out, slice(None), slice(None), ("rows or not", count))
            again = D.continuum(ctx, grid, V, l, E, m, vidx, norm=R.WKB, partners=P, power=1, lists=[[0, 5, 9]], trial_list=tl, want_rows=True)
            _same(again, out, slice(None), slice(None), ("repeated", count))
    # the instance: the probe's list of 3 runs in the instance of 4; another trial's list of 8 or 16 raises the call's instance
    for other in (list(range(8)), list(range(16))):
        out = D.continuum(ctx, grid, V, [2, 1], [0.37, 1.0], [2500, 300], [2, 0], norm=R.WKB, partners=P, power=1, lists=[[0, 5, 9], other],
                          trial_list=[0, 1], want_rows=True)
        _same(out, alone, [0], [0], ("instance", len(other)))
        assert np.all(out["sums"][1, :len(other)] != 0)


def test_frozen_atoms_keep_their_outputs(ctx, grids):
    """the batch of test_gpu_orbitals.test_frozen_atoms_keep_their_orbitals: H and Ar freeze in step 33 while Cu is live"""
    grid, _ = grids("log12")
    scf = D.Scf(ctx, grid, [1, 18, 29], alpha=ALPHA)
    l, E = np.array([0, 1, 2] * 3), np.array([0.05, 0.5, 4.0] * 3)
    atom = np.repeat([0, 1, 2], 3)
    try:
        for _ in range(80):
            scf.step(want_stats=False)
            fin = scf.energies()[1]
            if fin[0] and fin[1]:
                break
        assert fin[0] and fin[1] and not fin[2], "the premise: hydrogen and argon finish while copper is live"
        one = scf.continuum(l, E, atom=atom, power=1)
        for _ in range(5):
            scf.step(want_stats=False)
        assert not scf.energies()[1][2]
        two = scf.continuum(l, E, atom=atom, power=1)
    finally:
        scf.close()
    _same(one, two, atom < 2, atom < 2, "frozen")
    assert np.all(one["logderiv"][atom == 2] != two["logderiv"][atom == 2])


# ---- e. edges -----------------------------------------------------------------------------------------------------------------------------
def test_nan_node_unnormalised_trials_and_error_paths(ctx, grids):
    grid, (r, s, c, lam) = grids("uni10")
    N = grid.N
    V = _potentials(r)
    V[1, 500] = np.nan
    vidx, m = np.array([0, 1, 1, 1, 2]), np.array([N - 2, 498, 499, N - 2, N - 2])
    out = D.continuum(ctx, grid, V, [1] * 5, [0.5] * 5, m, vidx, partners=_partners(r, 2), want_rows=True)
    assert [int(x) for x in out["status"] & R.STEP] == [0, 0, R.STEP, R.STEP, 0] and not out["status"][[0, 1, 4]].any()
    assert list(out["nodes"][2:4]) == [-1, -1] and np.all(out["nodes"][[0, 1, 4]] >= 0)
    for q in ("logderiv", "delta", "scale"):
        assert list(np.isnan(out[q])) == [False, False, True, True, False], q
    assert np.all(np.isnan(out["sums"][2:4, :2])) and not np.isnan(out["sums"][[0, 1, 4]]).any()
    assert np.all(np.isnan(out["rows"][2, 1:501])) and np.all(out["rows"][2, 501:] == 0) and not np.isnan(out["rows"][[0, 1, 4]]).any()
    # E <= 0: zeros for the normalisation, a valid u'/u (sinh, and u = r at E = 0)
    out = D.continuum(ctx, grid, V[0], [0, 0], [-1.0, 0.0])
    assert not out["scale"].any() and not out["delta"].any() and not out["status"].any()
    assert abs(out["logderiv"][0] / (np.sqrt(2) / np.tanh(np.sqrt(2) * r[N - 2])) - 1) < 1e-7 and abs(out["logderiv"][1] * r[N - 2] - 1) < 1e-9
    # zero trials
    assert D.continuum(ctx, grid, V[0], np.zeros(0, np.int32), np.zeros(0))["logderiv"].shape == (0,)
    # the error paths
    ok = dict(V=V[0], l=[0], E=[0.5])
    for bad in (dict(l=[5]), dict(l=[-1]), dict(m=[2]), dict(m=[N - 1]), dict(E=[np.nan]), dict(E=[np.inf]), dict(vidx=[1]), dict(norm=2),
                dict(partners=_partners(r, 17)), dict(partners=_partners(r, 2), lists=[[0, 2]]), dict(partners=_partners(r, 2), power=9),
                dict(partners=_partners(r, 2), lists=[[0]], trial_list=[1])):
        with pytest.raises(D.DftaError):
            D.continuum(ctx, grid, **{**ok, **bad})
    one = np.zeros(1)
    i1 = np.zeros(1, np.int32)
    rc = ctx.lib.dfta_continuum(ctx.h, grid.h, 0, 1, None, 1, None, D._ip(i1), D._dp(one), D._ip(i1 + 3), 0, None, 0, 0, None, None, None,
                                D._dp(one), None, None, None, None, None, None)
    assert rc == 1                                                               # DFTA_ERR_INVALID: V is NULL


# ---- f. physics ---------------------------------------------------------------------------------------------------------------------------
def test_neon_orthogonality_and_2p_cross_section(ctx, grids):
    grid, (r, s, c, lam) = grids("log12")
    scf = D.Scf(ctx, grid, [10], alpha=ALPHA)
    try:
        for _ in range(40):
            scf.step(want_stats=False)
        E = np.array(R.NE40_ENERGIES)
        out = scf.continuum([0] * len(E), E, power=0)
        lv = scf.levels(0, 0)
        assert [int(x) for x in out["partner_index"][0][:2]] == [0, 1] and list(lv["l"][:2]) == [0, 0]      # 1s, 2s
        worst = 0.0
        for b in range(2):
            bound = 2 * np.array(R.NE40_OVERLAP[b])
            assert np.all(np.abs(out["sums"][:, b]) <= bound), (b, out["sums"][:, b], bound)
            worst = max(worst, float(np.max(np.abs(out["sums"][:, b]) / bound)))
        eps = np.linspace(4.6, 12.0, 16)
        ph = scf.photoionization(eps)
        j2p = ph["jobs"].index((0, 1, 1))
        om, sg = ph["omega"][j2p], ph["sigma"][j2p]
        assert np.all(om > 5) and np.all(sg > 0) and np.all(np.diff(sg) < 0), (om, sg)
        assert np.allclose(om, eps - lv["E"][j2p], rtol=0, atol=1e-15)
        # the entry is the sums of Scf.continuum put together in the header's order
        S = scf.continuum([0] * 16 + [2] * 16, np.concatenate([eps, eps]), power=1)
        col = [list(S["partner_index"][k]).index(j2p) for k in (0, 16)]
        K = (4.0 * (np.pi * np.pi)) * (1.0 / 137.035999084)
        s0, s2 = S["sums"][:16, col[0]], S["sums"][16:, col[1]]
        want = (((K * om) / 3.0) * (6.0 / 3.0)) * ((1 * (s0 * s0)) + (2.0 * (s2 * s2)))
        assert np.array_equal(sg, want)
    finally:
        scf.close()
    print("Ne, 40 steps: overlaps of eps s with 1s, 2s at %.3f of twice the CPU figure; sigma_2p(%.2f Ha) = %.4f a0^2" % (worst, om[0], sg[0]))


# ---- g. the front end -----------------------------------------------------------------------------------------------------------------------
def test_cli_phase_shift_and_photo_tables(ctx, grids):
    """dftatom_cli --phase-shift-table=1.5:3 --photo-table=2:2: after Finished!, 15 + 6 lines whose figures are those of Scf.continuum and
    Scf.photoionization at six decimals; without the flags the output is byte for byte what it is with the tables taken out"""
    import os
    import subprocess
    exe = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "dftatom_amd", "compat", "dftatom_cli")
    args = [exe, "10", "12", "0.5", "25", "0.002", "0"]
    plain = subprocess.run(args, capture_output=True, text=True, timeout=120)
    table = subprocess.run(args + ["--phase-shift-table=1.5:3", "--photo-table=2:2"], capture_output=True, text=True, timeout=120)
    assert plain.returncode == 0 and table.returncode == 0, (plain.stderr, table.stderr)
    for bad in ("2:0", "2", "-1:5", "0:5", "2:5x"):                              # refused before anything runs
        for flag in ("--phase-shift-table=", "--photo-table="):
            assert subprocess.run(args + [flag + bad], capture_output=True, text=True, timeout=120).returncode == 2, (flag, bad)
    lines = table.stdout.split("\n")
    ps = [k for k, ln in enumerate(lines) if ln.startswith("PhaseShift ")]
    ph = [k for k, ln in enumerate(lines) if ln.startswith("Photo ")]
    assert len(ps) == 15 and ps == list(range(ps[0], ps[0] + 15)) and lines[ps[0] - 2] == "Finished!" and lines[ps[-1] + 1] == ""
    assert len(ph) == 6 and ph == list(range(ps[-1] + 2, ps[-1] + 8)) and lines[ph[-1] + 1] == ""
    assert "\n".join(lines[:ps[0]] + lines[ph[-1] + 2:]) == plain.stdout and "PhaseShift" not in plain.stdout and "Photo" not in plain.stdout
    grid, _ = grids("log12")
    scf = D.Scf(ctx, grid, [10], alpha=ALPHA)
    try:
        for _ in range(100):
            scf.step(want_stats=False)
            if scf.energies()[1][0]:
                break
        E = np.tile([1.5 * (k + 1) / 3 for k in range(3)], 5)
        l = np.repeat(np.arange(5), 3)
        out = scf.continuum(l, E)
        pi = scf.photoionization([1.0, 2.0])
    finally:
        scf.close()
    for k, row in enumerate(ps):
        want = "PhaseShift l = %d E = %.6f delta = %.6f dlog = %.6f nodes = %d status = 0" % (l[k], E[k], out["delta"][k], out["logderiv"][k], out["nodes"][k])
        assert lines[row] == want, (lines[row], want)
    names = ["1s", "2s", "2p"]
    for k, row in enumerate(ph):
        a, e = divmod(k, 2)
        want = "Photo %s eps = %.6f omega = %.6f sigma = %.6f Mb = %.6f" % (names[a], (1.0, 2.0)[e], pi["omega"][a][e], pi["sigma"][a][e],
                                                                          pi["sigma"][a][e] * 28.002852)
        assert lines[row] == want, (lines[row], want)


# ---- h. rows in more than one chunk ---------------------------------------------------------------------------------------------------------
CHUNK_E = (-3.0, 0.0, 0.005, 0.5, 8.0)


def _rows_in_two_chunks(ctx, grid, tab, count, first, late_m, what):
    """`count` trials, one per potential index t (so every trial is a wave of its own): potential t % 3 of _potentials, l = (t // 3) % 5,
    E by (potential + l) % 5, a 3-row partner list on the l = 2 trials.  The first `first` trials (the first chunk) end at N - 2, the
    later ones at the nodes late_m in turn: a row that chunk 1 left in the row buffer would show beyond their m + 1.  Every output must be
    the one of the same (potential, l, m) in a small call of one chunk, which is held to the model and the replay.  Returns the small
    call's largest ratio to the gate."""
    r, s, c, lam = tab
    N = grid.N
    V3, P = _potentials(r), _partners(r, 3)
    t = np.arange(count)
    v, l = t % 3, (t // 3) % 5
    E = np.array(CHUNK_E)[(v + l) % 5]
    m = np.where(t < first, N - 2, np.array(late_m)[(t - first) % len(late_m)])
    classes = sorted(set(zip(v.tolist(), l.tolist(), m.tolist())))
    sv, sl, sm = (np.array(x) for x in zip(*classes))
    sE = np.array(CHUNK_E)[(sv + sl) % 5]
    assert len(classes) <= 64 and {(a, b) for a, b, _ in classes} == {(a, b) for a in range(3) for b in range(5)}
    small = D.continuum(ctx, grid, V3, sl, sE, sm, sv, partners=P, power=1, lists=[[0, 1, 2]], trial_list=np.where(sl == 2, 0, -1), want_rows=True)
    worst = 0.0
    for vv in range(3):
        for ll in range(5):
            sel = np.where((sv == vv) & (sl == ll))[0]
            Pl, nb = (P, 3) if ll == 2 else (None, 0)
            ld, f64, gates = R.gate(V3[vv], ll, sE[sel], sm[sel], r, s, c, lam, R.FREE, Pl, 1, want_rows=True)
            _bitwise(small, f64, sel, nb, (what, "small", vv, ll))
            worst = max(worst, _gated(small, sel, nb, ld, gates, (what, "small", vv, ll)))
    V = np.tile(V3, ((count + 2) // 3, 1))
    tl = np.where(l == 2, 0, -1)
    big = D.continuum(ctx, grid, V, l, E, m, t, partners=P, power=1, lists=[[0, 1, 2]], trial_list=tl, want_rows=True)
    assert ctx.last_kernel_ms() > 0
    at = np.array([classes.index(k) for k in zip(v.tolist(), l.tolist(), m.tolist())])
    _same(big, small, slice(None), at, what)
    beyond = np.arange(N)[None, :] > (m + 1)[:, None]
    assert not big["rows"][:, 0].any() and not big["rows"][beyond].any(), (what, "zeros at node 0 and beyond m + 1")
    assert np.all(big["rows"][t, m + 1] != 0), (what, "the last node of a row")
    norows = D.continuum(ctx, grid, V, l, E, m, t, partners=P, power=1, lists=[[0, 1, 2]], trial_list=tl)
    assert "rows" not in norows
    _same(norows, big, slice(None), slice(None), (what, "rows or not"))
    return worst


def test_rows_in_two_chunks_capped_by_waves(ctx, grids):
    """1100 waves of one trial on 9 nodes: the scaling launch's grid caps a chunk at 1023 waves -- chunks of 1023 + 77 (the planner's
    line in tests/test_continuum_ref.py).  block0 > 0 in k_continuum<.., true>, pos0 in k_continuum_scale, the host scatter of the second
    chunk, the row buffer's second use and the timer's stop on the last chunk."""
    grid, tab = grids("uni3")
    worst = _rows_in_two_chunks(ctx, grid, tab, 1100, 1023, (3,), "waves")
    print("two chunks by waves: 1100 trials equal their small call; its largest ratio to the gate %.3f" % worst)


def test_rows_in_two_chunks_capped_by_bytes(ctx, grids):
    """520 waves of one trial on 1025 nodes: 64 rows a wave, 524 800 bytes; the 256 MiB budget holds 511 -- chunks of 511 + 9"""
    grid, tab = grids("uni10")
    worst = _rows_in_two_chunks(ctx, grid, tab, 520, 511, (3, 255, 257), "bytes")
    print("two chunks by bytes: 520 trials equal their small call; its largest ratio to the gate %.3f" % worst)


# ---- i. grid-stride loops ---------------------------------------------------------------------------------------------------------------------
def test_partner_weights_beyond_one_grid_pass(ctx, grids):
    """k_partner_weight runs 8192 x 256 threads: 1100 rows of 2049 nodes are 2 253 900 values, the rows from 1024 on (1030 on: whole
    rows) are formed in the loop's second pass.  Rows j = (made-up row j % 16) (1 + j / 2048): a value read from or written to another
    row shows.  One list of 16 rows from both ends."""
    grid, (r, s, c, lam) = grids("uni11")
    N = grid.N
    base = _partners(r, 16)
    P = np.array([base[j % 16] * (1.0 + j / 2048.0) for j in range(1100)])
    rows = [0, 1, 2, 1030, 1031, 1040, 1047, 1055, 1063, 1064, 1071, 1080, 1087, 1090, 1095, 1099]
    assert len(P) * N > 8192 * 256 and min(rows[3:]) * N >= 8192 * 256 and len(rows) == 16
    V = _potentials(r)[2]
    E = np.array([-3.0, -0.5, 0.0, 0.005, 0.05, 0.3, 0.5, 2.0, 4.0, 8.0])
    out = D.continuum(ctx, grid, V, np.ones(len(E), np.int32), E, partners=P, power=1, lists=[rows])
    ld, f64, gates = R.gate(V, 1, E, N - 2, r, s, c, lam, R.FREE, P[rows], 1)
    sel = np.arange(len(E))
    assert not out["status"].any() and np.all(out["sums"] != 0)
    _bitwise(out, f64, sel, 16, "weights")
    worst = _gated(out, sel, 16, ld, gates, "weights")
    print("partner weights beyond one pass: largest ratio to the gate %.3f" % worst)


def test_row_scaling_beyond_one_grid_pass(ctx, grids):
    """k_continuum_scale runs 64 x 256 threads a row: on 16385 nodes node 16384 = N - 1 is the loop's second pass, the last node of a row
    that ends at m = N - 2.  Rows of E <= 0 are the model's; a row of E > 0 is ONE multiplication of q y by the factor: the model's
    unscaled row times the device's own scale, bit for bit.  (The float64 model alone: no replay, no seeds.)"""
    grid, (r, s, c, lam) = grids("uni14")
    N = grid.N
    assert N == 16385 and N > 64 * 256
    V = _potentials(r)[2]
    l = np.repeat([0, 2], 3)
    E = np.tile([-1.0, 0.0, 0.5], 2)
    m = np.array([N - 2, 300, N - 2, 300, N - 2, 300])
    out = D.continuum(ctx, grid, V, l, E, m, want_rows=True)
    assert not out["status"].any()
    for ll in (0, 2):
        sel = np.where(l == ll)[0]
        f64 = R.sweep(V, ll, E[sel], m[sel], r, s, c, lam, R.FREE, want_rows=True)
        _bitwise(out, f64, sel, 0, ("uni14", ll))
        pos = sel[E[sel] > 0]
        assert np.all(out["scale"][pos] > 0)
        assert np.array_equal(out["rows"][pos], f64["rows_raw"][E[sel] > 0] * out["scale"][pos][:, None]), ("uni14", ll, "scaled rows")
    beyond = np.arange(N)[None, :] > (m + 1)[:, None]
    assert not out["rows"][:, 0].any() and not out["rows"][beyond].any() and np.all(out["rows"][np.arange(6), m + 1] != 0)


# ---- j. exits -------------------------------------------------------------------------------------------------------------------------------
def _raw_times_factor(out, f64, sel, E, m, N, nb, what):
    """sums and rows of the trials `sel` are the model's unscaled ones times ONE factor: NaN under NONFINITE or STEP, 1 for E <= 0, else
    the device's own scale; rows are 0.0 at node 0 and beyond m + 1"""
    bad = (out["status"][sel] & (R.NONFINITE | R.STEP)) != 0
    fac = np.where(bad, np.nan, np.where(E[sel] > 0, out["scale"][sel], 1.0))
    with np.errstate(all="ignore"):
        assert np.array_equal(out["sums"][sel][:, :nb], f64["sums_raw"] * fac[:, None], equal_nan=True), (what, "sums")
        inside = (np.arange(N)[None, :] >= 1) & (np.arange(N)[None, :] <= (m[sel] + 1)[:, None])
        want = np.where(inside, f64["rows_raw"] * fac[:, None], 0.0)
    assert np.array_equal(out["rows"][sel], want, equal_nan=True), (what, "rows")


def test_overflow_without_a_bad_step(ctx, grids):
    """DFTA_CONT_NONFINITE alone: V = 2e4 at every node but 0 on uni11 gives f ~ 6 a step, d = 0.5 > 0 throughout, and y grows 14-fold a
    node: past DBL_MAX after some 270 nodes.  The trials that end at N - 2 carry status 1 -- not 3 --, nodes -1 and NaN outputs; those
    of the same wave that end at 200 and at 3 are untouched.  A group of four healthy free-particle trials is interleaved."""
    grid, (r, s, c, lam) = grids("uni11")
    N = grid.N
    V = np.zeros((2, N))
    V[0, 1:] = 2.0e4
    P = _partners(r, 2)
    vidx = np.tile([0, 1], 4)
    E, m = np.empty(8), np.empty(8, np.int64)
    E[0::2], m[0::2] = (-1.0, 0.5, -1.0, 0.5), (N - 2, N - 2, 200, 3)
    E[1::2], m[1::2] = (-1.0, 0.0, 0.5, 0.5), (N - 2, 3, 200, N - 2)
    out = D.continuum(ctx, grid, V, np.ones(8, np.int32), E, m, vidx, partners=P, power=1, want_rows=True)
    barrier, free = np.arange(0, 8, 2), np.arange(1, 8, 2)
    assert [int(x) for x in out["status"][barrier]] == [R.NONFINITE, R.NONFINITE, 0, 0] and not out["status"][free].any()
    assert list(out["nodes"][barrier[:2]]) == [-1, -1] and np.all(np.isnan(out["logderiv"][barrier[:2]]))
    assert np.all(np.isnan(out["sums"][barrier[:2], :2])) and np.all(np.isnan(out["rows"][barrier[:2], 1:])) and not out["rows"][:, 0].any()
    worst = 0.0
    for sel, v, live in ((barrier, 0, barrier[2:]), (free, 1, free)):
        f64 = R.sweep(V[v], 1, E[sel], m[sel], r, s, c, lam, R.FREE, P, 1, want_rows=True)
        _bitwise(out, f64, sel, 2, ("overflow", v))
        _raw_times_factor(out, f64, sel, E, m, N, 2, ("overflow", v))
        ld, _, gates = R.gate(V[v], 1, E[live], m[live], r, s, c, lam, R.FREE, P, 1, want_rows=True)
        worst = max(worst, _gated(out, live, 2, ld, gates, ("overflow", v)))
    for t in barrier[2:]:
        alone = D.continuum(ctx, grid, V[0], [1], [E[t]], [m[t]], partners=P, power=1, want_rows=True)
        _same(out, alone, [t], [0], ("beside an overflowing lane", int(t)))
    print("overflow without a bad step: status [1, 1, 0, 0]; the finite trials' largest ratio to the gate %.3f" % worst)


@pytest.mark.parametrize("name", ("uni10", "log12"))
def test_normalisation_below_double_range(ctx, grids, name):
    """DFTA_CONT_NORM: the free particle, l = 4.  E = 1e-300: yh_4 ~ x^-4 overflows, a = inf - inf -- the bit, NaN scale, phase shift,
    sums and rows; u'/u and nodes stand.  E = 1e-150: yh'_4 alone overflows, hypot is inf, scale = 0.0 and no bit.  E = 0.5 beside them."""
    grid, (r, s, c, lam) = grids(name)
    N = grid.N
    V, P = np.zeros(N), _partners(r, 2)
    E = np.array([1e-300, 1e-150, 0.5])
    out = D.continuum(ctx, grid, V, [4] * 3, E, partners=P, power=1, want_rows=True)
    ld, f64, gates = R.gate(V, 4, E, N - 2, r, s, c, lam, R.FREE, P, 1, want_rows=True)
    assert list(f64["status"]) == [R.NORM, 0, 0] and D.CONT_NORM == R.NORM, "the premise"
    assert [int(x) for x in out["status"]] == [D.CONT_NORM, 0, 0]
    sel = np.arange(3)
    _bitwise(out, f64, sel, 2, (name, "norm"))
    assert np.all(np.isfinite(out["logderiv"])) and np.all(out["nodes"] >= 0)
    assert np.isnan(out["scale"][0]) and np.isnan(out["delta"][0]) and np.all(np.isnan(out["sums"][0, :2])) and np.all(np.isnan(out["rows"][0, 1:]))
    assert out["scale"][1] == 0.0 and not out["rows"][1].any() and not out["sums"][1].any() and not out["rows"][:, 0].any()
    worst = _gated(out, sel, 2, ld, gates, (name, "norm"))
    print("%s below double range: status [8, 0, 0]; largest ratio to the gate %.3f" % (name, worst))


# ---- k. powers and small energies -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("power", (2, 3, 8))
def test_partner_powers(ctx, grids, power):
    """k_partner_weight's r^p loop up to check()'s bound of 8 (9 is refused: the error paths above)"""
    grid, (r, s, c, lam) = grids("log12")
    N = grid.N
    V, P = _potentials(r), _partners(r, 4)
    E, vidx = np.tile([-0.5, 0.3, 2.0], 2), np.repeat([1, 2], 3)
    out = D.continuum(ctx, grid, V, np.ones(6, np.int32), E, None, vidx, partners=P, power=power)
    assert not out["status"].any() and np.all(out["sums"][:, :4] != 0)
    worst = 0.0
    for v in (1, 2):
        sel = np.where(vidx == v)[0]
        ld, f64, gates = R.gate(V[v], 1, E[sel], N - 2, r, s, c, lam, R.FREE, P, power)
        _bitwise(out, f64, sel, 4, ("power", power, v))
        worst = max(worst, _gated(out, sel, 4, ld, gates, ("power", power, v)))
    print("power %d: largest ratio to the gate %.3f" % (power, worst))


@pytest.mark.parametrize("l", range(5))
@pytest.mark.parametrize("v", (0, 1))
@pytest.mark.parametrize("name", ("uni10", "log12"))
def test_energy_ladder(ctx, grids, name, v, l):
    """E = 1e-100 .. 1e-4, the free particle and Coulomb Z = 10: the normalisation's sincos, j_l and yh_l at x = k r down to 3.5e-49.

    [uni10-1-1] (Coulomb, l = 1) is the case that found the one-ulp phase shift: its gate of delta is 0.0 at all five energies -- the
    float64 model equals the rounded replay and no seed moves it (pi to the last bit at E <= 1e-8, 3.128 at E = 1e-4) --, and a
    reconstruction pi - t from the one double nearest pi lands 0.66 ulp from the exact value at E = 1e-4.  continuum.hip's
    atan2_quadrants carries pi as two doubles (tests/test_continuum_ref.py restates it)."""
    grid, (r, s, c, lam) = grids(name)
    N = grid.N
    V, P = _potentials(r)[v], _partners(r, 2)
    E = np.array(R.LADDER_E)
    out = D.continuum(ctx, grid, V, np.full(len(E), l), E, partners=P, power=1)
    assert not out["status"].any() and np.all(out["scale"] > 0)
    sel = np.arange(len(E))
    ld, f64, gates = R.gate(V, l, E, N - 2, r, s, c, lam, R.FREE, P, 1)
    with np.errstate(all="ignore"):
        dist = R.distances({q: out[q] if q != "sums" else out[q][:, :2] for q in ("logderiv", "delta", "scale", "sums")}, ld)
    print("%s potential %d l = %d: distance / gate per quantity %s" % (name, v, l, {q: (float(np.max(dist[q])), float(np.max(gates[q]))) for q in R.QUANTITIES}))
    _bitwise(out, f64, sel, 2, (name, v, l))
    worst = _gated(out, sel, 2, ld, gates, (name, v, l))
    print("%s potential %d l = %d, E = 1e-100 .. 1e-4: largest ratio to the gate %.3f" % (name, v, l, worst))


# ---- l. every photoionization row -----------------------------------------------------------------------------------------------------------
PHOTO_EPS = (0.05, 0.2, 0.7, 2.0, 4.5, 8.0)


def _photo_rows(scf, a, eps, norm):
    """Scf.photoionization of atom a and, for every (spin, n, l) of its "jobs", omega and sigma rebuilt in the header's order from
    Scf.continuum (power 1, the same normalisation; the S column through partner_index) and Scf.levels; flagged: the rows' entries with
    a status bit in their l - 1 or l + 1 trial.  Returns (ph, omega, sigma, flagged)."""
    eps = np.asarray(eps, dtype=np.float64)
    ne = len(eps)
    ph = scf.photoionization(eps, atom=a, norm=norm)
    K = (4.0 * (np.pi * np.pi)) * (1.0 / 137.035999084)
    jobs, om, sg, flagged = [], [], [], []
    for sp in range(1 + max(j[0] for j in ph["jobs"])):
        lv = scf.levels(a, sp)
        S = scf.continuum(np.repeat(np.arange(5), ne), np.tile(eps, 5), atom=a, spin=sp, power=1, norm=norm)
        for k in range(len(lv["l"])):
            lb, occ = int(lv["l"][k]), float(lv["occupation"][k])
            side, bad = [], np.zeros(ne, bool)
            for lp in (lb - 1, lb + 1):
                if not 0 <= lp <= 4:
                    side.append(np.zeros(ne))                    # the absent term: exact 0
                    continue
                t = np.arange(lp * ne, (lp + 1) * ne)
                col = list(S["partner_index"][t[0]]).index(k)
                assert np.all(S["partner_index"][t, col] == k)
                st = S["status"][t] != 0
                side.append(np.where(st, np.nan, S["sums"][t, col]))
                bad |= st
            omega = eps - lv["E"][k]
            sigma = (((K * omega) / 3.0) * (occ / (2.0 * lb + 1.0))) * ((lb * (side[0] * side[0])) + ((lb + 1.0) * (side[1] * side[1])))
            jobs.append((sp, int(lv["n"][k]), lb))
            om.append(omega), sg.append(sigma), flagged.append(bad)
    assert jobs == ph["jobs"]
    return ph, np.array(om), np.array(sg), np.array(flagged)


@pytest.mark.parametrize("Z,lsda", [([70], False), ([7, 29], True)])
def test_every_photoionization_row(ctx, grids, Z, lsda):
    """Yb LDA (4f: l' = 2 and 4; 5p, 4d) and the LSDA batch [N, Cu] (open shells, beta rows, 3d, the atom of index 1) after three steps:
    every row of Scf.photoionization is the header's formula on the sums of Scf.continuum, bit for bit, omega included; Yb after 24
    steps with the WKB normalisation at eps = 0.012: the l' = 4 trial has no WKB tail at r = 25 (20 / r^2 > 2 (eps - V); l' = 3:
    12 / r^2 < 2 (eps - V)), and sigma is NaN exactly in the rows that need it -- 4f."""
    grid, _ = grids("log12")
    scf = D.Scf(ctx, grid, Z, lsda=lsda, alpha=ALPHA)
    try:
        for _ in range(3):
            scf.step()
        rows = 0
        for a in range(len(Z)):
            ph, om, sg, flagged = _photo_rows(scf, a, PHOTO_EPS, "auto")
            assert np.array_equal(ph["omega"], om), (Z, a, "omega")
            assert np.array_equal(ph["sigma"], sg, equal_nan=True), (Z, a, "sigma")
            assert not flagged.any() and np.all(np.isfinite(sg)) and np.all(sg >= 0) and np.any(sg > 0, axis=1).sum() >= 1
            rows += len(ph["jobs"])
            ls = {(sp, l) for sp, _, l in ph["jobs"]}
            if Z == [70]:
                assert {(0, 1), (0, 2), (0, 3)} <= ls
            else:
                assert (1, 0) in ls and ((1, 2) in ls) == (a == 1)
                occ = [scf.levels(a, sp)["occupation"] for sp in (0, 1)]
                assert len(occ[0]) != len(occ[1]) or not np.array_equal(occ[0], occ[1]), "the premise: an open shell"
        if Z == [70]:
            # the NaN rule needs the neutral atom's tail gone: after 3 steps V(25) = -0.070 and every l' has a WKB tail at any eps > 0;
            # after 24 it is -7e-4 (the CPU oracle's figures), and 2 (eps - V) = 0.0254 lies between 12 / r^2 = 0.0193 and 20 / r^2 = 0.0321
            for _ in range(21):
                scf.step(want_stats=False)
            eps = (0.012,) + PHOTO_EPS
            ph, om, sg, flagged = _photo_rows(scf, 0, eps, D.CONT_WKB)
            assert np.array_equal(ph["omega"], om) and np.array_equal(ph["sigma"], sg, equal_nan=True)
            assert np.array_equal(np.isnan(ph["sigma"]), flagged)
            assert flagged[:, 0].any() and not flagged[:, 0].all(), "the premise: at eps = 0.012 a row is NaN and a row is finite"
            f = [k for k, j in enumerate(ph["jobs"]) if j[2] == 3]
            assert np.all(flagged[f, 0]) and not flagged[[k for k in range(len(ph["jobs"])) if k not in f], 0].any()
    finally:
        scf.close()
    print("Z = %s %s: %d photoionization rows rebuilt bit for bit at %d energies" % (Z, "LSDA" if lsda else "LDA", rows, len(PHOTO_EPS)))
