"""GPU suite (-m gpu): the Kleinman-Bylander block -- dftatom_amd/csrc/kb.hip (k_kb, k_kb_combine) and the host loops of kb_plan.cpp;
include/dftatom_hip.h has the arithmetic, tests/_kb_ref.py restates it in float64 (the model of the kernel) and in longdouble, restates
the search, and holds the CPU figures the physics gates come from.

The sweep uses + - * / sqrt alone, so EVERY output must equal the float64 model BIT FOR BIT.

a. continuum   beta == 0, q1 = 1: logderiv and rows are continuum()'s on the same (potential, l, E, m), bit for bit (values compared with
               ==: the combination adds 0.0, which turns a -0.0 into 0.0 and changes nothing else).
b. model       hydrogen-like and smooth-well channels on log12 (4097), uni11 (2049) and uni3 (9 nodes): m = 255, 256, 257, N-2; beta cut
               at 255, 256, 257, N-2 and all zero; E < 0, = 0, > 0; l = 0 .. 4; a NaN node in Vloc and one in beta.
c. bits        a trial alone == among 63, 64, 65, 200 others at any position == with rows == a repeated call == one wave per chunk.
d. search      kb_bound_states == _kb_ref.search fed with the device's own signs, bit for bit.
e. physics     Ne, Ar, Fe after convergence: the eigenstate identity (gated by the model on the same channel), the lowest bound state, the
               planted ghost, continuity through D = 0.
f. edges       the DFTA_ERR_INVALID cases, zero trials.

Every gated test prints its figures before it asserts.
"""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import _kb_ref as K                      # noqa: E402
import dftatom_amd as D                  # noqa: E402

OUTS = ("u", "du", "logderiv", "Bh", "Bp", "D", "status")


@pytest.fixture(scope="module")
def ctx(torch_first):
    assert np.finfo(K.LD).eps < 1.2e-19, "the reference of this file needs an extended np.longdouble"
    c = D.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def grids(ctx):
    """name -> (grid, (r, s, c, lam) as the library holds them)"""
    made = {}

    def get(name):
        if name not in made:
            L, d, Rm = K.GRIDS[name]
            g = D.Grid(ctx, L, d, Rm)
            tab = K.tables(L, d, Rm)
            assert np.array_equal(g.r(), tab[0]), "the reference's r table is not the library's"
            made[name] = (g, tab)
        return made[name]
    yield get
    for g, _ in made.values():
        g.close()


def _ends(N):
    return sorted({m for m in (255, 256, 257, N - 2) if 3 <= m <= N - 2} | ({3} if N < 256 else set()))


def _channels(r):
    """ten channels: every l with both potentials, the cuts 255, 256, 257, N-2 and 0 (all zero) going round"""
    N = len(r)
    cuts = [c for c in (255, 256, 257) if c < N - 2] + [N - 2, 0]
    if N < 256:
        cuts = [3, 4, N - 2, 0]
    out = []
    for l in range(5):
        for q, make in enumerate((lambda cut: K.hydrogen_like(r, 3.0, l, cut), lambda cut: K.smooth_well(r, 4.0, l, cut))):
            cut = cuts[(2 * l + q) % len(cuts)]
            V, beta, q1 = make(cut)
            out.append((V, l, beta, q1))
    return out


def _trials(chans, N, energies=(-1.5, 0.0, 0.8)):
    chan, E, m = [], [], []
    for k, (_, _, beta, _) in enumerate(chans):
        for mm in _ends(N):
            if mm >= K.last_nonzero(beta):
                for e in energies:
                    chan.append(k); E.append(e); m.append(mm)
    return np.array(chan, np.int32), np.array(E), np.array(m, np.int32)


def _call(ctx, grid, chans, chan, E, m, want_rows=False):
    V = np.array([ch[0] for ch in chans])
    return D.kb_sweep(ctx, grid, V, [ch[1] for ch in chans], np.array([ch[2] for ch in chans]), [ch[3] for ch in chans], E, m, chan=chan,
                      vidx=np.arange(len(chans)), want_rows=want_rows)


def _model(chans, chan, E, m, tab, want_rows=False):
    r, s, c, lam = tab
    out = {q: np.zeros(len(E)) for q in OUTS}
    if want_rows:
        out["rows"] = np.zeros((len(E), len(r)))
    for k, (V, l, beta, q1) in enumerate(chans):
        sel = np.nonzero(chan == k)[0]
        if len(sel):
            res = K.sweep(V, l, beta, q1, E[sel], m[sel], r, s, c, lam, want_rows=want_rows)
            for q in out:
                out[q][sel] = res[q]
    return out


def _same(got, ref, what):
    for q in ref:
        assert np.array_equal(np.asarray(got[q], dtype=np.float64), np.asarray(ref[q], dtype=np.float64), equal_nan=True), (what, q)


# ---- a. against continuum() --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["log12", "uni11", "uni3"])
def test_zero_projector_is_continuum(ctx, grids, name):
    grid, (r, s, c, lam) = grids(name)
    N = grid.N
    V = np.array([K.hydrogen_like(r, 3.0, 0)[0], K.smooth_well(r, 4.0, 0)[0]])
    l, vi, E, m = [], [], [], []
    for ll in range(5):
        for v in range(2):
            for mm in _ends(N):
                for e in (-2.0, -0.3, 0.0, 0.7):
                    l.append(ll); vi.append(v); E.append(e); m.append(mm)
    l, vi, E, m = np.array(l, np.int32), np.array(vi, np.int32), np.array(E), np.array(m, np.int32)
    cont = D.continuum(ctx, grid, V, l, E, m, vidx=vi, want_rows=True)
    nch = 10                                                             # channel = (l, potential)
    kb = D.kb_sweep(ctx, grid, V, np.repeat(np.arange(5), 2), np.zeros((nch, N)), np.ones(nch), E, m, chan=2 * l + vi,
                    vidx=np.tile(np.arange(2), 5), want_rows=True)
    assert not kb["status"].any() and not cont["status"].any()
    assert np.all(kb["Bh"] == 0) and np.all(kb["Bp"] == 0) and np.all(kb["D"] == 1)
    assert np.array_equal(kb["logderiv"], cont["logderiv"])
    scale = np.where(E > 0, cont["scale"], 1.0)                          # continuum() normalises its rows for E > 0: the same product
    assert np.array_equal(kb["rows"] * scale[:, None], cont["rows"])
    # B_h is the continuum block's partner sum with beta as the partner, power 0 (E <= 0: factor 1)
    beta = K.hydrogen_like(r, 3.0, 1, min(257, N - 2))[1]
    sel = (l == 1) & (vi == 0) & (E <= 0) & (m >= K.last_nonzero(beta))
    a = D.kb_sweep(ctx, grid, V, [1], beta, [0.75], E[sel], m[sel])
    b = D.continuum(ctx, grid, V, l[sel], E[sel], m[sel], partners=beta[None, :], power=0)
    assert sel.any() and np.array_equal(a["Bh"], b["sums"][:, 0])


# ---- b. against the model -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["log12", "uni11", "uni3"])
def test_model_bits(ctx, grids, name):
    grid, tab = grids(name)
    chans = _channels(tab[0])
    chan, E, m = _trials(chans, grid.N)
    assert len(E) > (64 if grid.N > 256 else 10)
    got = _call(ctx, grid, chans, chan, E, m, want_rows=True)
    ref = _model(chans, chan, E, m, tab, want_rows=True)
    assert not ref["status"].any()
    _same(got, ref, name)
    assert np.all(got["rows"][:, 0] == 0) and all(not got["rows"][t, m[t] + 2:].any() for t in range(len(E)))
    print("   %s: %d trials of %d channels equal the float64 model bit for bit (largest |logderiv| %.3g)"
          % (name, len(E), len(chans), np.max(np.abs(got["logderiv"]))))


def test_nan_nodes_poison_their_own_trials(ctx, grids):
    grid, tab = grids("log12")
    r, N = tab[0], grid.N
    V, beta, q1 = K.hydrogen_like(r, 3.0, 1, 257)
    Vn, bn = V.copy(), beta.copy()
    Vn[300] = np.nan
    bn[200] = np.nan
    chans = [(Vn, 1, beta, q1), (V, 1, bn, q1), (V, 1, beta, q1)]
    chan, E, m = _trials(chans, N)
    chan, E, m = np.append(chan, [0, 0]).astype(np.int32), np.append(E, [-1.0, 0.3]), np.append(m, [298, 299]).astype(np.int32)
    got = _call(ctx, grid, chans, chan, E, m, want_rows=True)
    _same(got, _model(chans, chan, E, m, tab, want_rows=True), "nan")
    hit = ((chan == 0) & (m + 1 >= 300)) | (chan == 1)
    assert np.all(got["status"][hit] != 0) and not got["status"][~hit].any() and hit.any() and (~hit & (chan == 0)).any()
    assert np.all(np.isnan(got["logderiv"][hit])) and np.all(np.isfinite(got["logderiv"][~hit]))


# ---- c. a trial's bits are its own ------------------------------------------------------------------------------------------------------------
def test_a_trial_does_not_depend_on_the_call(ctx, grids, monkeypatch):
    grid, tab = grids("uni11")
    N = grid.N
    chans = _channels(tab[0])[:4]
    one = (np.array([1], np.int32), np.array([-0.7]), np.array([1000], np.int32))
    alone = _call(ctx, grid, chans, *one, want_rows=True)
    assert alone["status"][0] == 0
    rng = np.random.default_rng(5)
    for others in (63, 64, 65, 200):
        for at in (0, others // 2, others):
            ch = rng.integers(0, len(chans), others).astype(np.int32)
            E = rng.uniform(-2.0, 1.0, others)
            m = np.array([max(int(x), K.last_nonzero(chans[k][2])) for x, k in zip(rng.integers(3, N - 1, others), ch)], np.int32)
            ch, E, m = (np.insert(a, at, b[0]) for a, b in zip((ch, E, m), one))
            for rows in (False, True):
                got = _call(ctx, grid, chans, ch.astype(np.int32), E, m.astype(np.int32), want_rows=rows)
                for q in OUTS + (("rows",) if rows else ()):
                    assert np.array_equal(got[q][at], alone[q][0], equal_nan=True), (others, at, rows, q)
    again = _call(ctx, grid, chans, ch.astype(np.int32), E, m.astype(np.int32), want_rows=True)
    monkeypatch.setenv("DFTA_DEBUG", "KB_CHUNK_WAVES=1")                  # read by every call
    chunked = _call(ctx, grid, chans, ch.astype(np.int32), E, m.astype(np.int32), want_rows=True)
    monkeypatch.delenv("DFTA_DEBUG")
    for q in OUTS + ("rows",):
        assert np.array_equal(again[q], got[q], equal_nan=True) and np.array_equal(chunked[q], got[q], equal_nan=True), q


# ---- d. the search ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["log12", "uni11"])
def test_bound_states_are_the_restated_search(ctx, grids, name):
    grid, tab = grids(name)
    r, N = tab[0], grid.N
    chans = [K.hydrogen_like(r, 3.0, 0, 257), K.hydrogen_like(r, 3.0, 1, 256), K.smooth_well(r, 4.0, 0, 255), K.smooth_well(r, 4.0, 2, 0)]
    ls = [0, 1, 0, 2]
    V, beta, q1 = np.array([c[0] for c in chans]), np.array([c[1] for c in chans]), [c[2] for c in chans]
    mbox = int(np.searchsorted(r, 12.0))
    lo, hi = [-6.0, -3.0, -4.5, -4.0], [0.0, 0.0, 0.5, 0.0]
    got = D.kb_bound_states(ctx, grid, V, ls, beta, q1, lo, hi, m=mbox, vidx=np.arange(4), nscan=128)

    def signs(k, E):
        res = D.kb_sweep(ctx, grid, V[k], [ls[k]], beta[k], [q1[k]], E, mbox)
        return (res["status"] == 0) & np.isfinite(res["u"]), res["u"] < 0
    ref = K.search(signs, list(zip(lo, hi)), 128)
    for k in range(4):
        en, rounds, status = ref[k]
        assert got["count"][k] == len(en) and np.array_equal(got["energies"][k][:len(en)], en), (k, got["energies"][k], en)
        assert np.all(np.isnan(got["energies"][k][len(en):])) and got["rounds"][k] == rounds and got["status"][k] == status
    assert got["count"].sum() >= 4 and np.all(got["rounds"] <= 12)
    print("   %s: %s states, %s rounds" % (name, got["count"], got["rounds"]))


# ---- e. physics -----------------------------------------------------------------------------------------------------------------------------------
ATOMS = ("Ne", "Ar", "Fe")


@pytest.fixture(scope="module")
def atoms(ctx, grids):
    """the batch Ne, Ar, Fe on log12 run until every atom has converged: (ps with the highest l local, ps of Ar with l_loc = 0)"""
    grid, _ = grids("log12")
    scf = D.Scf(ctx, grid, [K.ATOMS[a] for a in ATOMS], alpha=0.5)
    try:
        for step in range(400):
            scf.step(want_stats=False)
            if all(scf.energies()[1]):
                break
        assert all(scf.energies()[1]), "the batch did not converge"
        ps = scf.pseudopotentials()
        ar = scf.pseudopotentials(atoms=[1], l_loc=[0])
    finally:
        scf.close()
    assert not ps["status"].any() and not ar["status"].any()
    return ps, ar


def _nonlocal(ps):
    """(k, the atom's local channel) of every non-local channel"""
    return [(k, int(np.nonzero((ps["atom"] == ps["atom"][k]) & np.isnan(ps["kb"][:, 2]))[0][0])) for k in range(len(ps["l"]))
            if not np.isnan(ps["kb"][k, 2])]


@pytest.mark.parametrize("where", ["rc", "end"])
@pytest.mark.parametrize("name", ATOMS)
def test_eigenstate_identity(ctx, grids, atoms, name, where):
    """(a): at E = eps_ref the KB logderiv is the semilocal one -- continuum() in V_ps,l --, at m = ic_max + 8 ("rc") and at N - 2
    ("end").  The gate is the issue's: twice the sum of (the longdouble model's KB logderiv from the longdouble semilocal one) and (the
    float64 model's distance from the longdouble model), _kb_ref.identity_distances, taken ON THE CHANNEL UNDER TEST as
    _continuum_ref.gate takes its gates on the trials under test: the second figure is a rounding error, one draw per input.  At N - 2
    the outward sweep at a bound state's energy has picked up the growing solution and that draw scatters by a factor of a few between
    two atoms that differ in the last digits -- neon: 1.1e-05 on the CPU oracle's atom (_kb_ref.MEASURED, kept for the record and
    held by tests/test_kb_ref.py), 3.3e-05 on the device's, whose distance was 3.35e-05 --, so the figures of another atom gate nothing.
    Observed on an MI355X, distance: rc 1.3e-12 / 7.2e-13 / 7.4e-13, end 3.3e-05 / 2.2e-05 / 1.3e-07 (Ne, Ar, Fe)."""
    grid, tab = grids("log12")
    ps, _ = atoms
    seen = 0
    for k, loc in _nonlocal(ps):
        if ATOMS[ps["atom"][k]] != name:
            continue
        seen += 1
        tag = "%s_%s" % (name, "spdf"[ps["l"][k]])
        icmax = int(ps["ic"][ps["atom"] == ps["atom"][k]].max())
        m = icmax + 8 if where == "rc" else grid.N - 2
        kb = D.kb_sweep(ctx, grid, ps["V_ps"][loc], [ps["l"][k]], ps["beta"][k], [ps["kb"][k, 0]], [ps["eps"][k]], [m])
        semi = D.continuum(ctx, grid, ps["V_ps"][k], [ps["l"][k]], [ps["eps"][k]], [m])
        assert kb["status"][0] == 0 and semi["status"][0] == 0
        dist = abs(kb["logderiv"][0] - semi["logderiv"][0]) / abs(semi["logderiv"][0])
        r, s, c, lam = tab
        fig = K.identity_distances(ps["V_ps"][loc], ps["V_ps"][k], int(ps["l"][k]), ps["beta"][k], float(ps["kb"][k, 0]), float(ps["eps"][k]), m,
                                   r, s, c, lam)
        gate = 2 * sum(fig)
        print("   %s at %s (m = %d): |KB - semilocal| / |semilocal| = %.3e, gate %.3e = 2 (%.3e + %.3e); on the CPU oracle's atom: 2 (%.3e + %.3e) "
              "(D = %.3e)" % ((tag, where, m, dist, gate) + fig + K.MEASURED["identity"][(tag, where)] + (kb["D"][0],)))
        assert dist <= gate, (tag, where, dist, gate)
    assert seen == 1


@pytest.mark.parametrize("name", ATOMS)
def test_lowest_bound_state_is_the_reference_level(ctx, grids, atoms, name):
    """(b): the lowest bound state of H_KB with the box at N - 2 against eps_ref; the gate is twice the CPU figure of
    _kb_ref.MEASURED["lowest"].  Neon and argon: the lowest state IS eps_ref.  IRON (d local) HAS A GHOST in its 4s channel, on the CPU
    model and on the device alike: the lowest state lies 11.34 Ha below eps_ref, so twice the CPU figure gates nothing there; what holds
    the device for iron is that both verdicts say ghost, as on the CPU, that the ghost sits where the CPU model finds it (1e-5 Ha:
    the two SCFs agree far better), and that eps_ref is still a state (1e-6 Ha: what the SCF's stop test leaves between the resident
    potential and the orbitals' own, measured 2.5e-10 on the CPU and 7.2e-10 on the device)."""
    grid, _ = grids("log12")
    ps, _ = atoms
    rep = D.kb_ghost_report(ctx, grid, ps)
    seen = 0
    for k, loc in _nonlocal(ps):
        if ATOMS[ps["atom"][k]] != name:
            continue
        seen += 1
        tag = "%s_%s" % (name, "spdf"[ps["l"][k]])
        assert len(rep["bound"][k]) >= 1 and rep["status"][k] == 0, (tag, rep["bound"][k], rep["status"][k])
        dist, gate = abs(rep["bound"][k][0] - ps["eps"][k]), 2 * K.MEASURED["lowest"][tag]
        near = float(np.min(np.abs(rep["bound"][k] - ps["eps"][k])))
        print("   %s: states %s, eps_ref %.12f, lowest at %.3e (gate %.3e), nearest at %.3e; e_loc %s, E_KB %.4f, verdicts %d %d"
              % (tag, rep["bound"][k], ps["eps"][k], dist, gate, near, rep["e_loc"][k], rep["E_KB"][k], rep["gks"][k], rep["direct"][k]))
        assert dist <= gate, (tag, dist, gate)
        want = K.MEASURED["ghost"][tag]
        assert rep["gks"][k] == want and rep["direct"][k] == want and (rep["ghosts"][k] > 0) == bool(want), tag
        assert near <= 1e-6, (tag, near)
        if want:
            assert abs(rep["bound"][k][0] - K.MEASURED["lowest_E"][tag]) <= 1e-5 and rep["e_loc"][k][1] < ps["eps"][k]
    assert seen == 1
    for k in set(range(len(ps["l"]))) - {k for k, _ in _nonlocal(ps)}:         # the local channels
        assert rep["gks"][k] == -1 and rep["direct"][k] == -1 and len(rep["bound"][k]) == 0 and rep["eps_ref"][k] == ps["eps"][k]


def _planted(grid, ar, A):
    """Ar's p channel on the s channel's potential with the well of depth A planted: a ps to hand to kb_ghost_report"""
    r, s = grid.r(), K.tables(*K.GRIDS["log12"])[1]
    ks, kp = int(np.nonzero(ar["l"] == 0)[0][0]), int(np.nonzero(ar["l"] == 1)[0][0])
    ch_s = {"V_ps": ar["V_ps"][ks]}
    ch_p = {"V_ps": ar["V_ps"][kp], "u_ps": ar["u_ps"][kp]}
    V_loc, beta = K.planted(ch_p, ch_s, A, r)
    ps = {q: np.array(ar[q], copy=True) for q in ("V_ps", "beta", "kb", "l", "eps", "atom")}
    ps["V_ps"][ks], ps["beta"][kp] = V_loc, beta
    q1, q2 = K.q1_of(beta, ar["u_ps"][kp], s), K.q1_of(beta, beta, s)
    ps["kb"][kp] = (q1, q2, q2 / q1)
    return ps, kp


def test_planted_ghost_is_found_and_the_clean_case_is_clean(ctx, grids, atoms):
    """(c): A = _kb_ref.GHOST_A puts the local potential's second p level 1.3 Ha below eps_ref (CPU): both verdicts say ghost, and agree;
    A = 0: both say clean"""
    grid, _ = grids("log12")
    _, ar = atoms
    for A, want in ((0.0, 0), (K.GHOST_A, 1)):
        ps, kp = _planted(grid, ar, A)
        rep = D.kb_ghost_report(ctx, grid, ps, l_loc=[0])
        print("   A = %g: E_KB %.4f, e_loc %s, states of H_KB %s, eps_ref %.6f, GKS %d, direct %d"
              % (A, rep["E_KB"][kp], rep["e_loc"][kp], rep["bound"][kp], ps["eps"][kp], rep["gks"][kp], rep["direct"][kp]))
        assert rep["status"][kp] == 0
        assert rep["gks"][kp] == rep["direct"][kp] == want
        assert (rep["ghosts"][kp] >= 1) == bool(want)
        if want:
            assert rep["bound"][kp][0] < ps["eps"][kp] - 1.0 and rep["e_loc"][kp][1] < ps["eps"][kp] - 1.0
        assert np.min(np.abs(rep["bound"][kp] - ps["eps"][kp])) < 1e-6         # the reference state itself stays


def test_continuity_through_the_zero_of_D(ctx, grids, atoms):
    """(d): u~_m(E) changes sign on a fine scan only at the states the search finds, although D = q1 - B_p crosses 0 in between"""
    grid, _ = grids("log12")
    _, ar = atoms
    ps, kp = _planted(grid, ar, K.GHOST_A)
    ks = int(np.nonzero(ar["l"] == 0)[0][0])
    m = int(np.searchsorted(grid.r(), 10.0))
    q1 = ps["kb"][kp, 0]
    st = D.kb_bound_states(ctx, grid, ps["V_ps"][ks], [1], ps["beta"][kp], [q1], K.GHOST_LO, 0.0, m=m, nscan=512)
    E = np.linspace(K.GHOST_LO, 0.0, 6001)
    fine = D.kb_sweep(ctx, grid, ps["V_ps"][ks], [1], ps["beta"][kp], [q1], E, m)
    assert not fine["status"].any() and np.all(np.isfinite(fine["u"]))
    flips = np.nonzero(np.signbit(fine["u"][1:]) != np.signbit(fine["u"][:-1]))[0]
    dflips = np.nonzero(np.signbit(fine["D"][1:]) != np.signbit(fine["D"][:-1]))[0]
    states = st["energies"][0][:st["count"][0]]
    print("   sign changes of u~_m at %s, states %s, zeros of D near %s" % (E[flips], states, E[dflips]))
    assert len(dflips) >= 1 and len(flips) == len(states) and st["status"][0] == 0
    for j, e in zip(flips, states):
        assert E[j] <= e <= E[j + 1]
    for j in dflips:                                                      # no jump where D = 0: the step of u~ across it is an ordinary one
        step = abs(fine["u"][j + 1] - fine["u"][j])
        around = np.abs(np.diff(fine["u"][max(j - 3, 0):j + 5]))
        assert step <= 4 * np.median(around) + 1e-300


# ---- the front end ------------------------------------------------------------------------------------------------------------------------------
def test_cli_kb_table(ctx, grids):
    """dftatom_cli --kb-table=-1.5:0.5:3 on argon: after Finished!, per valence channel a head line (the local channel says so) and three
    lines of u'/u; the figures are those of Scf.kb_ghost_report and kb_sweep at six decimals; without the flag the output is byte for
    byte what it is with the table taken out"""
    import subprocess
    exe = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "dftatom_amd", "compat", "dftatom_cli")
    args = [exe, "18", "12", "0.5", "25", "0.002", "0"]
    plain = subprocess.run(args, capture_output=True, text=True, timeout=120)
    table = subprocess.run(args + ["--kb-table=-1.5:0.5:3"], capture_output=True, text=True, timeout=120)
    assert plain.returncode == 0 and table.returncode == 0, (plain.stderr, table.stderr)
    for bad in ("1:0:3", "-1:1", "-1:1:1", "-1:1:3x"):
        assert subprocess.run(args + ["--kb-table=" + bad], capture_output=True, text=True, timeout=120).returncode == 2, bad
    lines = table.stdout.split("\n")
    kb = [k for k, ln in enumerate(lines) if ln.startswith("KB ")]
    assert len(kb) == 8 and kb == list(range(kb[0], kb[0] + 8)) and lines[kb[0] - 2] == "Finished!" and lines[kb[-1] + 1] == ""
    assert "\n".join(lines[:kb[0]] + lines[kb[-1] + 2:]) == plain.stdout and "KB " not in plain.stdout
    head_s, head_p = lines[kb[0]].split(), lines[kb[4]].split()
    assert head_s[:2] == ["KB", "3s"] and head_p == ["KB", "3p", "local"]
    val = lambda words, key: float(words[words.index(key, 2) + 2])        # noqa: E731   ("key = value", after the line's own "KB 3s")
    grid, _ = grids("log12")
    scf = D.Scf(ctx, grid, [18], alpha=0.5)
    try:
        for _ in range(100):
            scf.step(want_stats=False)
            if scf.energies()[1][0]:
                break
        rep, ps = scf.kb_ghost_report()
    finally:
        scf.close()
    assert abs(val(head_s, "EKB") - rep["E_KB"][0]) < 2e-6 and abs(val(head_s, "eps") - ps["eps"][0]) < 2e-6
    assert abs(float(head_s[head_s.index("states") + 2]) - rep["bound"][0][0]) < 2e-6
    assert int(val(head_s, "GKS")) == rep["gks"][0] == 0 and int(val(head_s, "direct")) == rep["direct"][0] == 0
    icmax = int(ps["ic"].max())
    E = np.array([-1.5, -0.5, 0.5])
    nl = D.kb_sweep(ctx, grid, ps["V_ps"][1], [0], ps["beta"][0], [ps["kb"][0, 0]], E, icmax)["logderiv"]
    sl = D.continuum(ctx, grid, ps["V_ps"][0], [0] * 3, E, icmax)["logderiv"]
    for j in range(3):
        w = lines[kb[1 + j]].split()
        assert abs(val(w, "E") - E[j]) < 1e-6 and abs(val(w, "KB") - nl[j]) < 2e-6 * max(1, abs(nl[j])) and abs(val(w, "semilocal") - sl[j]) < 2e-6 * max(1, abs(sl[j]))
        assert np.isfinite(val(w, "AE"))


def test_write_upf_refuses_a_ghost(ctx, tmp_path):
    """examples/write_upf.py writes argon (clean) with the report in PP_INFO, refuses iron -- whose 4s channel has the ghost of
    test_lowest_bound_state_is_the_reference_level[Fe], a real one where (c) plants one -- and writes it with --force"""
    import subprocess
    import sys
    exe = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "examples", "write_upf.py")
    ar, fe = str(tmp_path / "Ar.upf"), str(tmp_path / "Fe.upf")
    run = lambda *a: subprocess.run([sys.executable, exe] + list(a), capture_output=True, text=True, timeout=120)      # noqa: E731
    clean = run("--z", "18", "--out", ar)
    assert clean.returncode == 0 and os.path.exists(ar), clean.stderr
    text = open(ar).read()
    assert "Kleinman-Bylander ghost report" in text and "3S: eps_ref" in text and "ghost by count: 0, by Gonze-Kaeckell-Scheffler: 0" in text
    assert "3P: local" in text
    ghost = run("--z", "26", "--out", fe)
    assert ghost.returncode != 0 and not os.path.exists(fe) and "ghost" in ghost.stderr and "ghost by count: 1, by Gonze-Kaeckell-Scheffler: 1" in ghost.stdout
    forced = run("--z", "26", "--out", fe, "--force")
    assert forced.returncode == 0 and os.path.exists(fe) and "ghost by count: 1" in open(fe).read()


# ---- f. edges -----------------------------------------------------------------------------------------------------------------------------------
def test_invalid_calls(ctx, grids):
    grid, tab = grids("uni11")
    r, N = tab[0], grid.N
    V, beta, q1 = K.hydrogen_like(r, 3.0, 1, 257)
    ok = dict(V=V, l=[1], beta=beta, q1=[q1], E=[-1.0], m=[300])
    assert D.kb_sweep(ctx, grid, **ok)["status"][0] == 0
    for change in (dict(m=[255]), dict(m=[2]), dict(m=[N - 1]), dict(l=[5]), dict(l=[-1]), dict(q1=[0.0]), dict(q1=[np.nan]), dict(E=[np.inf]),
                   dict(chan=[1]), dict(vidx=[1])):
        with pytest.raises(D.DftaError):
            D.kb_sweep(ctx, grid, **dict(ok, **change))
    assert len(D.kb_sweep(ctx, grid, V, [1], beta, [q1], np.zeros(0))["u"]) == 0
    for bad in (dict(nscan=100), dict(nscan=0), dict(E_lo=0.0, E_hi=-1.0), dict(m=255)):
        with pytest.raises(D.DftaError):
            D.kb_bound_states(ctx, grid, V, [1], beta, [q1], **dict(dict(E_lo=-3.0, E_hi=0.0), **bad))
