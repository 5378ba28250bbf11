"""GPU suite (-m gpu): the Kleinman-Bylander block -- dftatom_amd/csrc/kb.hip (k_kb, k_kb_combine) and the host loops of kb_plan.cpp;
include/dftatom_hip.h has the arithmetic, tests/_kb_ref.py restates it in float64 (the model of the kernel) and in longdouble, restates
the search, and holds the CPU figures the physics gates come from.

The sweep uses + - * / sqrt alone, so EVERY output must equal the float64 model BIT FOR BIT.

a. continuum   beta == 0, q1 = 1: logderiv and rows are continuum()'s on the same (potential, l, E, m), bit for bit (values compared with
               ==: the combination adds 0.0, which turns a -0.0 into 0.0 and changes nothing else).
b. model       hydrogen-like and smooth-well channels on log12 (4097), uni11 (2049) and uni3 (9 nodes): m = 255, 256, 257, N-2; beta cut
               at 255, 256, 257, N-2 and all zero; E < 0, = 0, > 0; l = 0 .. 4; a NaN node in Vloc and one in beta.
b'. exits      the status words born mid-sweep from finite inputs: DFTA_CONT_STEP alone (uni3, E = -146), DFTA_CONT_NONFINITE by overflow
               (uni11, E = -1e4 and +1e6), both (E = -40 315): every output and the rows equal the model; flagged trials at lanes 0, 31, 32
               and 63 of a wave between clean ones, some of which end before a node whose step test would fail; a flagged row is NaN on
               1 .. m+1 and 0.0 elsewhere.
c. bits        a trial alone == among 63, 64, 65, 200 others at any position == with rows == a repeated call == rows in chunks of one, two
               and three waves (the last chunk shorter than the others).
d. search      kb_bound_states == _kb_ref.search fed with the device's own signs, bit for bit; DFTA_KB_SEARCH_FULL (nine sign changes and
               more on uni11); scan points that are not finite in round 0 (uni3, also against the model's search); four channels with their
               own potential, l, m, range and closing round in one call == each alone, one of them without a state.
d'. report     kb_ghost_report on a synthetic ps of five atoms held to its composition -- the bound of E_lo = NaN restated, the states of
               kb_bound_states, the ghosts below eps_ref - tol (at the state, one double above it, tol = 0), e_loc of dfta_solve_levels,
               both verdicts, status, rounds, the rows that stay NaN --: l = 3 non-local, l = 4 local and non-local, E_KB of both signs, a
               channel that was not pseudized, l_loc by default and given, two channels of the local l; a given range, E_hi below and
               above 0 and a shorter box; local channels only; every refusal.
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


# ---- b'. the status exits of k_kb -------------------------------------------------------------------------------------------------------------
# Ordinary arithmetic that the kernel answers with a status word: a step so long that d_i = 1 - f_i / 12 is not positive (STEP), a chain
# that overflows on the way out (NONFINITE), both.  (grid) -> the channels (V, l, beta, q1), the flagged energies with the bits the float64
# model gives them at m = N - 2, a range of clean energies.
def _status_case(name, r):
    """channels, [(flagged E, its bits at m = N - 2)], the clean energies' range, the channel of the shared wave, end nodes of its clean trials"""
    N = len(r)
    if name == "uni3":
        Vh, bh, qh = K.hydrogen_like(r, 3.0, 0, 4)
        Vw, bw, qw = K.smooth_well(r, 40.0, 1, N - 2)
        Vc, bc, qc = K.smooth_well(r, 40.0, 1, 4)
        # the third channel: between E = -122 and -118.4 d_i is positive up to node 5 and not at node 6: a trial that ends at m = 3 is clean
        # and shares its wave with lanes that march on through node 6
        return [(Vh, 0, bh, qh), (Vw, 1, bw, qw), (Vc, 1, bc, qc)], [(-146.0, K.STEP)], (-122.0, 1.0), 2, lambda e, j: 3 if e < -95.0 else (3, 5, N - 2)[j % 3]
    Vh, bh, qh = K.hydrogen_like(r, 3.0, 0, 257)
    return ([(Vh, 0, bh, qh)], [(-1e4, K.NONFINITE), (1e6, K.NONFINITE), (-40315.0, K.STEP | K.NONFINITE)], (-2.0, 1.0), 0,
            lambda e, j: (257, 1000, N - 2)[j % 3])


def _flagged_row_is_nan_inside(row, m):
    return np.all(np.isnan(row[1:m + 2])) and row[0] == 0 and not np.signbit(row[0]) and np.all(row[m + 2:] == 0) and not np.signbit(row[m + 2:]).any()


@pytest.mark.parametrize("name", ["uni3", "uni11"])
def test_status_exits_are_the_models(ctx, grids, name):
    """DFTA_CONT_STEP, DFTA_CONT_NONFINITE by overflow and both together, born mid-sweep from finite inputs: every output, rows included,
    is the float64 model's bit for bit, the model gives exactly the expected bits, and a flagged trial's row is NaN on 1 .. m+1"""
    grid, tab = grids(name)
    N = grid.N
    chans, flagged, _, _, _ = _status_case(name, tab[0])
    energies = [e for e, _ in flagged] + [-95.0 if name == "uni3" else -2.0]
    want = [bits for _, bits in flagged] + [0]
    chan = np.repeat(np.arange(len(chans)), len(energies)).astype(np.int32)
    E = np.tile(energies, len(chans))
    m = np.full(len(E), N - 2, np.int32)
    got = _call(ctx, grid, chans, chan, E, m, want_rows=True)
    ref = _model(chans, chan, E, m, tab, want_rows=True)
    print("   %s: E %s -> status %s (model %s)" % (name, E, got["status"], ref["status"].astype(int)))
    assert np.array_equal(ref["status"], np.tile(want, len(chans))), "the model does not take the exits this test is about"
    _same(got, ref, name)
    for t in range(len(E)):
        if got["status"][t]:
            assert all(np.isnan(got[q][t]) for q in OUTS[:-1]) and _flagged_row_is_nan_inside(got["rows"][t], m[t]), t
        else:
            assert all(np.isfinite(got[q][t]) for q in OUTS[:-1]) and np.all(np.isfinite(got["rows"][t])), t


@pytest.mark.parametrize("name", ["uni3", "uni11"])
def test_flagged_and_clean_trials_share_a_wave(ctx, grids, name):
    """one wave of 64 trials of one channel, flagged ones at lanes 0, 31, 32 and 63 between clean ones of other end nodes: the clean trials
    keep the bits they have in a call without the flagged ones, and alone; the whole wave is the model's"""
    grid, tab = grids(name)
    N = grid.N
    chans, flagged, clean, which, end_of = _status_case(name, tab[0])
    chans = chans[which:which + 1]
    lanes = (0, 31, 32, 63)
    E = np.zeros(64)
    m = np.zeros(64, np.int32)
    bits = np.zeros(64, np.int64)
    others = [t for t in range(64) if t not in lanes]
    E[others] = np.linspace(clean[0], clean[1], len(others))
    m[others] = [end_of(E[t], j) for j, t in enumerate(others)]
    for j, t in enumerate(lanes):
        E[t], bits[t] = flagged[j % len(flagged)]
        m[t] = N - 2
    chan = np.zeros(64, np.int32)
    got = _call(ctx, grid, chans, chan, E, m, want_rows=True)
    ref = _model(chans, chan, E, m, tab, want_rows=True)
    print("   %s: status by lane %s" % (name, got["status"]))
    assert np.array_equal(ref["status"], bits), "the model does not take the exits this test is about"
    if name == "uni3":                               # clean trials whose step test would fail beyond their own last node
        r, s, c, lam = tab
        V, l, beta, q1 = chans[0]
        beyond = K.sweep(V, l, beta, q1, E[others], N - 2, r, s, c, lam)["status"]
        print("   uni3: %d clean trials end before a node where d_i <= 0" % np.count_nonzero(beyond & K.STEP))
        assert np.count_nonzero(beyond & K.STEP) >= 2
    _same(got, ref, name)
    apart = _call(ctx, grid, chans, chan[others], E[others], m[others], want_rows=True)
    for q in OUTS + ("rows",):
        assert np.array_equal(got[q][others], apart[q], equal_nan=True), q
    for t in (1, 30, 33, 62):
        alone = _call(ctx, grid, chans, chan[t:t + 1], E[t:t + 1], m[t:t + 1], want_rows=True)
        for q in OUTS + ("rows",):
            assert np.array_equal(got[q][t], alone[q][0], equal_nan=True), (t, q)
    assert not got["status"][others].any() and all(np.all(np.isfinite(got[q][others])) for q in OUTS[:-1])
    for t in lanes:
        assert all(np.isnan(got[q][t]) for q in OUTS[:-1]) and _flagged_row_is_nan_inside(got["rows"][t], m[t]), t


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
    for q in OUTS + ("rows",):
        assert np.array_equal(again[q], got[q], equal_nan=True), q
    # the rows in chunks of 1, 2 and 3 waves: the call has four waves (one per channel), so chunks of 3 leave a last chunk of one
    waves_of_call = sum(-(-int(n) // 64) for n in np.bincount(ch.astype(np.int64)))
    assert waves_of_call % 3 != 0, waves_of_call
    for waves in (1, 2, 3):
        monkeypatch.setenv("DFTA_DEBUG", "KB_CHUNK_WAVES=%d" % waves)     # read by every call
        chunked = _call(ctx, grid, chans, ch.astype(np.int32), E, m.astype(np.int32), want_rows=True)
        monkeypatch.delenv("DFTA_DEBUG")
        for q in OUTS + ("rows",):
            assert np.array_equal(chunked[q], got[q], equal_nan=True), (waves, q)


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


def _device_signs(ctx, grid, V, ls, beta, q1, ms, seen=None):
    """signs() for _kb_ref.search from the device's own sweep, a channel at a time; seen[k] counts the scan points (the first call per
    channel) that were not finite"""
    def signs(k, E):
        res = D.kb_sweep(ctx, grid, V[k], [ls[k]], beta[k], [q1[k]], E, ms[k])
        fin = (res["status"] == 0) & np.isfinite(res["u"])
        if seen is not None and k not in seen:
            seen[k] = int(np.count_nonzero(~fin))
        return fin, res["u"] < 0
    return signs


def _same_search(got, ref, k, j=None):
    """channel k of kb_bound_states' output against entry j (default k) of _kb_ref.search's"""
    en, rounds, status = ref[k if j is None else j]
    assert got["count"][k] == len(en) and np.array_equal(got["energies"][k][:len(en)], en), (k, got["energies"][k], en)
    assert np.all(np.isnan(got["energies"][k][len(en):])) and got["rounds"][k] == rounds and got["status"][k] == status, (k, got, ref)


def test_search_reports_more_sign_changes_than_states(ctx, grids):
    """DFTA_KB_SEARCH_FULL: the box at N - 2 of uni11 and a range that reaches up to E = 3 hold more than eight sign changes; the lowest
    eight are kept and closed, the bit is set"""
    grid, tab = grids("uni11")
    r, N = tab[0], grid.N
    V, beta, q1 = K.hydrogen_like(r, 3.0, 0, 257)
    got = D.kb_bound_states(ctx, grid, V, [0], beta, [q1], -6.0, 3.0, m=N - 2, nscan=128)
    ref = K.search(_device_signs(ctx, grid, [V], [0], [beta], [q1], [N - 2]), [(-6.0, 3.0)], 128)
    print("   uni11: %d states %s, %d rounds, status %d" % (got["count"][0], got["energies"][0], got["rounds"][0], got["status"][0]))
    _same_search(got, ref, 0)
    assert got["count"][0] == K.MAX_STATES and got["status"][0] & K.SEARCH_FULL and not got["status"][0] & K.SEARCH_CAP
    assert np.all(np.diff(got["energies"][0]) > 0)


def test_search_steps_over_scan_points_that_are_not_finite(ctx, grids):
    """round 0 with points that are not finite (the low end of the range has DFTA_CONT_STEP on nine nodes): they open nothing and set
    nothing; the states above them are found.  Held to the restated search on the device's signs AND on the float64 model's."""
    grid, tab = grids("uni3")
    r, s, c, lam = tab
    N = grid.N
    chans, _, _, _, _ = _status_case("uni3", r)
    chans = chans[:2]
    V, ls, beta, q1 = [ch[0] for ch in chans], [ch[1] for ch in chans], [ch[2] for ch in chans], [ch[3] for ch in chans]
    got = D.kb_bound_states(ctx, grid, np.array(V), ls, np.array(beta), q1, -200.0, 0.0, m=N - 2, vidx=[0, 1], nscan=64)
    seen = {}
    ref = K.search(_device_signs(ctx, grid, V, ls, beta, q1, [N - 2] * 2, seen), [(-200.0, 0.0)] * 2, 64)
    print("   uni3: scan points that are not finite %s, states %s, rounds %s, status %s" % (seen, got["count"], got["rounds"], got["status"]))
    for k in range(2):
        _same_search(got, ref, k)
        model = K.search(K.model_signs(V[k], ls[k], beta[k], q1[k], N - 2, r, s, c, lam), [(-200.0, 0.0)], 64)
        _same_search(got, model, k, 0)
        assert 0 < seen[k] < 64
    assert got["count"].sum() >= 2


def test_four_channels_search_as_each_alone(ctx, grids):
    """one call with four channels that differ in potential, l, end node, range and closing round, one of them without a state: every
    channel's count, energies, rounds and status are those of the channel searched alone"""
    grid, tab = grids("log12")
    r, N = tab[0], grid.N
    chans = [K.hydrogen_like(r, 3.0, 0, 257), K.smooth_well(r, 4.0, 2, 0), K.hydrogen_like(r, 3.0, 1, 256), K.smooth_well(r, 4.0, 0, 255)]
    ls = [0, 2, 1, 0]
    V = np.array([chans[2][0], chans[1][0]])                              # the potentials, each once
    vidx = [0, 1, 0, 1]
    beta, q1 = np.array([c[1] for c in chans]), [c[2] for c in chans]
    ms = [int(np.searchsorted(r, 12.0)), N - 2, int(np.searchsorted(r, 8.0)), int(np.searchsorted(r, 5.0))]
    lo, hi = [-6.0, -4.0, -1.126, -4.5], [0.0, -3.5, -1.124, 0.5]          # (the third: a narrow range round the 2p-like state closes sooner)
    got = D.kb_bound_states(ctx, grid, V, ls, beta, q1, lo, hi, m=ms, vidx=vidx, nscan=128)
    print("   log12: states %s, rounds %s, status %s" % (got["count"], got["rounds"], got["status"]))
    for k in range(4):
        print("      channel %d: m = %d, (%g, %g): %s" % (k, ms[k], lo[k], hi[k], got["energies"][k][:got["count"][k]]))
        alone = D.kb_bound_states(ctx, grid, V[vidx[k]], [ls[k]], beta[k], [q1[k]], lo[k], hi[k], m=ms[k], nscan=128)
        for q in ("count", "rounds", "status"):
            assert got[q][k] == alone[q][0], (k, q, got[q], alone[q])
        assert np.array_equal(got["energies"][k], alone["energies"][0], equal_nan=True), k
    assert got["count"][1] == 0 and got["rounds"][1] == 1 and min(got["count"][k] for k in (0, 2, 3)) >= 1
    assert len(set(got["rounds"].tolist())) >= 3, got["rounds"]


# ---- d'. the ghost report is its own composition ----------------------------------------------------------------------------------------------------
REPORT_CUT = 3400                       # the projectors of the synthetic report end here (r = 6.2 on log12) ...
REPORT_M = 3600                         # ... and this is the shorter box (r = 9.3)
#              atom, l, maker ("h": hydrogen_like, Z; "w": smooth_well, depth), pseudized
REPORT_CHANNELS = [(0, 0, "h", 3.0, True), (0, 1, "w", 5.0, True), (0, 2, "h", 3.0, True), (0, 3, "w", 7.0, True), (0, 4, "w", 40.0, True),
                   (1, 0, "w", 30.0, True), (1, 4, "h", 3.0, True),
                   (2, 0, "h", 3.0, True), (2, 1, "w", 1.0, True), (2, 2, "w", 6.0, False),
                   (3, 2, "w", 10.0, True),
                   (4, 0, "h", 3.0, True), (4, 1, "w", 20.0, True), (4, 1, "w", 8.0, True)]
REPORT_L_LOC = [-1, 0, 1, -1, -1]       # atom 0: l = 4 is local and l = 3 is not; 1: l = 4 is NOT local; 2: l = 1; 3: its one channel; 4: the
#                                         first of its two l = 1 channels


def _report_ps(r, s):
    """a synthetic `ps`: V_ps and beta of the makers, kb = (q1, q2, q2 / q1) with q2 = <beta|beta>: E_KB > 0 for "h", < 0 for "w"; the
    channel that was not pseudized has kb = NaN; a local channel has kb = NaN as well (what pseudo_ionic leaves)"""
    V, beta, kb = [], [], []
    for atom, l, kind, par, pseudized in REPORT_CHANNELS:
        v, b, q1 = K.hydrogen_like(r, par, l, REPORT_CUT) if kind == "h" else K.smooth_well(r, par, l, REPORT_CUT)
        V.append(v); beta.append(b)
        kb.append((q1, K.q1_of(b, b, s), K.q1_of(b, b, s) / q1) if pseudized else (np.nan,) * 3)
    ps = {"V_ps": np.array(V), "beta": np.array(beta), "kb": np.array(kb), "l": np.array([c[1] for c in REPORT_CHANNELS], np.int32),
          "atom": np.array([c[0] for c in REPORT_CHANNELS], np.int32), "eps": np.full(len(V), -0.5)}
    for k in _report_local(ps, REPORT_L_LOC).values():
        ps["kb"][k] = np.nan
    return ps


def _report_atoms(ps):
    """the atoms numbered by their first channel, as the binding numbers them (and the rows of l_loc)"""
    seen = {}
    return np.array([seen.setdefault(int(a), len(seen)) for a in ps["atom"]])


def _report_local(ps, l_loc):
    """the header's rule: per atom the first channel of l_loc, or (l_loc < 0) the first channel of the atom's highest l"""
    atom, loc = _report_atoms(ps), {}
    for a in range(int(atom.max()) + 1):
        ks = [k for k in range(len(atom)) if atom[k] == a]
        want = l_loc[a] if l_loc[a] >= 0 else max(ps["l"][k] for k in ks)
        loc[a] = [k for k in ks if ps["l"][k] == want][0]
    return loc


def _levels_as_the_report(ctx, grid, V, levels, vidx):
    """dfta_solve_levels as the report calls it: LEVELS_BATCHED on every potential of `ps` with bottom min_{i >= 1} V - 1, no hints, no
    density, no orbitals; a level that did not converge is not an error here.  Returns E per level, NaN for an absent one."""
    V = D._f64(V)
    n, l, occ = (D._i32([lv[q] for lv in levels]) for q in range(3))
    vi, bottom = D._i32(vidx), D._f64(V[:, 1:].min(axis=1) - 1.0)
    res = (D.LevelResult * len(levels))()
    issued = D.C.c_long(0)
    rc = ctx.lib.dfta_solve_levels(ctx.h, grid.h, D.LEVELS_BATCHED, 0, V.shape[0], D._dp(V), D._dp(bottom), None, len(levels), D._ip(vi),
                                   D._ip(n), D._ip(l), D._ip(occ), res, None, None, None, D.C.byref(issued))
    assert rc in (D.OK, 5), rc                                            # (5: DFTA_ERR_NOT_CONVERGED, soft)
    return np.array([x.E if x.converged and np.isfinite(x.E) and x.E < 0 else np.nan for x in res])


def _report_expected(ctx, grid, ps, l_loc, m=None, E_lo=None, E_hi=0.0, nscan=512, tol=1e-5):
    """what include/dftatom_hip.h says dfta_kb_ghost_report returns, composed from kb_bound_states and dfta_solve_levels called directly"""
    r, N = grid.r(), grid.N
    nch = len(ps["l"])
    loc, atom = _report_local(ps, l_loc), _report_atoms(ps)
    nl = [k for k in range(nch) if k != loc[atom[k]] and np.isfinite(ps["kb"][k, 0]) and ps["kb"][k, 0] != 0]
    exp = {"eps_ref": ps["eps"].copy(), "E_KB": ps["kb"][:, 2].copy(), "bound": [np.zeros(0)] * nch, "ghosts": np.full(nch, -1),
           "e_loc": np.full((nch, 2), np.nan), "gks": np.full(nch, -1), "direct": np.full(nch, -1), "status": np.full(nch, -1),
           "rounds": np.full(nch, -1), "lo": np.full(nch, np.nan), "nl": nl, "loc": loc}
    if not nl:
        return exp
    vidx = [loc[atom[k]] for k in nl]
    for k, v in zip(nl, vidx):
        if E_lo is None:                             # min_{i >= 1} vl_i - max(0, -E_KB), the header's operations in its order
            L = float(ps["l"][k]) * (float(ps["l"][k]) + 1.0)
            exp["lo"][k] = np.min(ps["V_ps"][v][1:] + (L / (r[1:] * r[1:])) * 0.5) - max(0.0, -ps["kb"][k, 2])
        else:
            exp["lo"][k] = E_lo
    st = D.kb_bound_states(ctx, grid, ps["V_ps"], ps["l"][nl], ps["beta"][nl], ps["kb"][nl, 0], exp["lo"][nl], min(0.0, E_hi),
                           m=N - 2 if m is None else m, vidx=vidx, nscan=nscan)
    has = [j for j, k in enumerate(nl) if ps["l"][k] <= 3]
    levels = [(int(ps["l"][nl[j]]) + q, int(ps["l"][nl[j]]), 1) for j in has for q in range(2)]
    e = _levels_as_the_report(ctx, grid, ps["V_ps"], levels, [vidx[j] for j in has for q in range(2)])
    for at, j in enumerate(has):
        exp["e_loc"][nl[j]] = e[2 * at:2 * at + 2]
    for j, k in enumerate(nl):
        states = st["energies"][j][:st["count"][j]]
        exp["bound"][k] = states
        exp["ghosts"][k] = np.count_nonzero(states < ps["eps"][k] - tol)
        exp["direct"][k] = int(exp["ghosts"][k] > 0)
        exp["status"][k], exp["rounds"][k] = st["status"][j], st["rounds"][j]
        if ps["l"][k] <= 3 and ps["kb"][k, 2] != 0 and not np.isnan(ps["kb"][k, 2]):
            exp["gks"][k] = K.gks_verdict(ps["kb"][k, 2], exp["e_loc"][k, 0], exp["e_loc"][k, 1], ps["eps"][k])
    return exp


def _same_report(rep, exp, what):
    for k in range(len(exp["eps_ref"])):
        row = "%s channel %d: eps_ref %.17g E_KB %.6g lo %.6g states %s ghosts %d e_loc %s gks %d direct %d status %d rounds %d" % (
            what, k, rep["eps_ref"][k], rep["E_KB"][k], exp["lo"][k], rep["bound"][k], rep["ghosts"][k], rep["e_loc"][k], rep["gks"][k],
            rep["direct"][k], rep["status"][k], rep["rounds"][k])
        print("   " + row)
        for q in ("eps_ref", "E_KB", "e_loc"):
            assert np.array_equal(rep[q][k], exp[q][k], equal_nan=True), (row, q, exp[q][k])
        assert np.array_equal(rep["bound"][k], exp["bound"][k]), (row, exp["bound"][k])
        for q in ("ghosts", "gks", "direct", "status", "rounds"):
            assert rep[q][k] == exp[q][k], (row, q, exp[q][k])


@pytest.fixture(scope="module")
def report(ctx, grids):
    """the synthetic ps on log12, its first report (eps_ref = -0.5 everywhere) and what that report must be"""
    grid, tab = grids("log12")
    ps = _report_ps(tab[0], tab[1])
    rep = D.kb_ghost_report(ctx, grid, ps, l_loc=REPORT_L_LOC)
    return ps, rep, _report_expected(ctx, grid, ps, REPORT_L_LOC)


def test_ghost_report_is_its_composition(ctx, grids, report):
    """the bound of E_lo = NaN (E_KB of both signs), the states, the count of ghosts, e_loc, both verdicts, status and rounds of every
    channel of five atoms: l = 3 non-local, l = 4 local and non-local, a channel that was not pseudized, l_loc by default and given,
    two channels of the local l; the rows that stay NaN"""
    ps, rep, exp = report
    _same_report(rep, exp, "first")
    nl, loc = exp["nl"], exp["loc"]
    assert [loc[a] for a in range(5)] == [4, 5, 8, 10, 12] and nl == [0, 1, 2, 3, 6, 7, 11, 13]
    assert np.all(ps["kb"][nl, 2][[0, 2, 4, 5, 6]] > 0) and np.all(ps["kb"][nl, 2][[1, 3, 7]] < 0)      # E_KB of both signs
    for k in range(len(ps["l"])):
        if k not in nl:                              # local, or not pseudized: (eps, E_KB, NaN ...)
            assert len(rep["bound"][k]) == 0 and np.all(np.isnan(rep["e_loc"][k])), k
            assert (rep["ghosts"][k], rep["gks"][k], rep["direct"][k], rep["status"][k], rep["rounds"][k]) == (-1,) * 5, k
            assert np.isnan(rep["E_KB"][k]) and rep["eps_ref"][k] == ps["eps"][k]
    assert np.all(np.isnan(rep["e_loc"][6])) and rep["gks"][6] == -1 and rep["direct"][6] in (0, 1) and rep["rounds"][6] >= 1      # l = 4, non-local
    assert set(rep["gks"][[0, 1, 2, 3, 7, 11, 13]].tolist()) <= {0, 1} and len(rep["bound"][3]) >= 1                              # l = 3 has levels
    assert sum(len(rep["bound"][k]) >= 1 for k in nl) >= 4
    assert np.isfinite(rep["e_loc"][7, 0]) and np.isnan(rep["e_loc"][7, 1])      # atom 2's shallow local well has one s level: the second is absent
    assert np.all(np.isfinite(rep["e_loc"][[0, 1, 2, 3, 11, 13]]))


def test_ghost_report_at_the_edge_of_tol(ctx, grids, report):
    """eps_ref placed from the first report's states, tol = 1e-5: 1e-3 above the lowest state (a ghost), below every state (none),
    eps_ref - tol EQUAL to the lowest state (not a ghost: the count is of states BELOW it) and the next double above that (a ghost)"""
    grid, _ = grids("log12")
    ps, rep, exp = report
    tol = 1e-5
    with_states = [k for k in exp["nl"] if len(rep["bound"][k]) >= 1][:4]
    assert len(with_states) == 4
    ps2 = dict(ps, eps=ps["eps"].copy())
    lowest = [rep["bound"][k][0] for k in with_states]
    def at_the_state(e):                             # the largest double x with x - tol == e in float64
        x = e + tol
        for _ in range(8):
            x = np.nextafter(x, np.inf) if x - tol < e else (np.nextafter(x, -np.inf) if x - tol > e else x)
        while np.nextafter(x, np.inf) - tol == e:
            x = np.nextafter(x, np.inf)
        assert x - tol == e
        return x
    equal, above = at_the_state(lowest[2]), np.nextafter(at_the_state(lowest[3]), np.inf)
    assert equal - tol == lowest[2] and above - tol > lowest[3] and np.nextafter(above, -np.inf) - tol == lowest[3]
    ps2["eps"][with_states] = [lowest[0] + 1e-3, lowest[1] - 1.0, equal, above]
    rep2 = D.kb_ghost_report(ctx, grid, ps2, l_loc=REPORT_L_LOC, tol=tol)
    _same_report(rep2, _report_expected(ctx, grid, ps2, REPORT_L_LOC, tol=tol), "edge")
    print("   ghosts of channels %s: %s" % (with_states, rep2["ghosts"][with_states]))
    assert rep2["ghosts"][with_states[0]] >= 1 and rep2["direct"][with_states[0]] == 1
    assert rep2["ghosts"][with_states[1]] == 0 and rep2["direct"][with_states[1]] == 0
    assert rep2["ghosts"][with_states[2]] == 0 and rep2["direct"][with_states[2]] == 0
    assert rep2["ghosts"][with_states[3]] == 1 and rep2["direct"][with_states[3]] == 1
    for k in exp["nl"]:                              # the states do not depend on eps_ref
        assert np.array_equal(rep2["bound"][k], rep["bound"][k])
    # tol = 0: a state at eps_ref itself is not below it
    ps3 = dict(ps, eps=ps["eps"].copy())
    ps3["eps"][with_states] = lowest
    rep3 = D.kb_ghost_report(ctx, grid, ps3, l_loc=REPORT_L_LOC, tol=0.0)
    assert np.all(rep3["ghosts"][with_states] == 0) and np.all(rep3["direct"][with_states] == 0)


def test_ghost_report_with_a_given_range_and_box(ctx, grids, report):
    """E_lo given, E_hi = -0.5 below 0 and the box at a node below N - 2; a ps without a non-local channel returns its heads"""
    grid, _ = grids("log12")
    ps, _, _ = report
    kw = dict(m=REPORT_M, E_lo=-30.0, E_hi=-0.5, nscan=256)
    rep = D.kb_ghost_report(ctx, grid, ps, l_loc=REPORT_L_LOC, **kw)
    exp = _report_expected(ctx, grid, ps, REPORT_L_LOC, **kw)
    _same_report(rep, exp, "given")
    assert all(np.all((b > -30.0) & (b < -0.5)) for b in rep["bound"]) and sum(len(b) for b in rep["bound"]) >= 4
    # E_hi above 0: the range ends at 0
    rep0 = D.kb_ghost_report(ctx, grid, ps, l_loc=REPORT_L_LOC, m=REPORT_M, E_lo=-30.0, E_hi=2.0, nscan=256)
    _same_report(rep0, _report_expected(ctx, grid, ps, REPORT_L_LOC, m=REPORT_M, E_lo=-30.0, E_hi=2.0, nscan=256), "E_hi = 2")
    # local channels only: atom 3 alone, and the local channels of atoms 0 and 1 together
    for keep, l_loc in (([10], [-1]), ([4, 5], [-1, 0])):
        only = {q: ps[q][keep] for q in ps}
        rep1 = D.kb_ghost_report(ctx, grid, only, l_loc=l_loc)
        exp1 = _report_expected(ctx, grid, only, l_loc)
        assert not exp1["nl"]
        _same_report(rep1, exp1, "local only")
        assert np.array_equal(rep1["eps_ref"], only["eps"]) and np.all(rep1["rounds"] == -1)


def test_ghost_report_refusals(ctx, grids, report):
    grid, _ = grids("log12")
    ps, _, _ = report
    ok = dict(l_loc=REPORT_L_LOC, m=REPORT_M, E_lo=-30.0, nscan=64)
    for bad in (dict(tol=-1e-9), dict(tol=np.nan), dict(E_hi=np.inf), dict(E_hi=np.nan), dict(E_lo=-np.inf), dict(E_lo=np.inf),
                dict(l_loc=[-1, 0, 3, -1, -1]),                           # atom 2 has no l = 3 channel
                dict(E_lo=0.0), dict(E_lo=-0.5, E_hi=-0.5), dict(E_lo=-0.25, E_hi=-0.5), dict(E_lo=1.0, E_hi=2.0),      # E_lo >= min(0, E_hi)
                dict(l=np.where(np.arange(len(ps["l"])) == 6, 5, ps["l"])), dict(l=np.where(np.arange(len(ps["l"])) == 0, -1, ps["l"]))):
        with pytest.raises(D.DftaError):
            D.kb_ghost_report(ctx, grid, ps, **dict(ok, **bad))
    # an atom index out of range: the binding renumbers the atoms, so the entry is called as the binding calls it
    nch = len(ps["l"])
    rep, st = np.zeros((nch, D.KB_REPORT)), np.zeros((nch, D.KB_MAX_STATES))
    for atoms, natoms in ((ps["atom"], 4), (np.where(np.arange(nch) == 3, -1, ps["atom"]), 5)):
        atoms = D._i32(atoms)
        rc = ctx.lib.dfta_kb_ghost_report(ctx.h, grid.h, natoms, nch, D._ip(atoms), D._ip(D._i32(ps["l"])), D._dp(D._f64(ps["eps"])),
                                          D._dp(D._f64(ps["V_ps"])), D._dp(D._f64(ps["beta"])), D._dp(D._f64(ps["kb"])),
                                          D._ip(D._i32(REPORT_L_LOC)), REPORT_M, -30.0, 0.0, 64, 1e-5, D._dp(rep), D._dp(st))
        with pytest.raises(D.DftaError):
            ctx.check(rc)
    assert D.kb_ghost_report(ctx, grid, ps, **ok)["rounds"][0] >= 1       # the call the refusals were cut from is accepted


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
