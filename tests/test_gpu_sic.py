"""GPU suite (-m gpu): the self-interaction-corrected LSDA step -- DFTA_EXCHANGE_SIC_KLI of dfta_scf_set_exchange, the SIC kernels of
dftatom_amd/csrc/kli_stage.hip and the direct entry dfta_sic_channels; include/dftatom_hip.h states the rule, tests/_sic_ref.py is the CPU
reference and the float64 statement of every stage.

1. direct     smooth and hydrogen-like orbitals on 9, 1025, 2049 (uniform) and 4097 (logarithmic) nodes, orbitals cut at 1023 / 1024 / 1025,
              an all-zero orbital, a NaN node: y0 == screening_yk, v_a / eps_a == vwn_lsda on the float64 rho_a, X, D, vS, vKLI, tail, mix, c
              and E_SIC the float64 replay of the device's own rows -- all bit for bit; EH, EXC, vbar within the counted bounds of the
              longdouble quadrature on the device's integrands.  Twelve channels alone, reversed, repeated, one per chunk: the same bits.
2. switch     values 0 and 1 keep today's bits; the refusals.
3. stage      steps 1 - 3 of Ne LDA, N / Li / H LSDA, [H, He, Ne] (also chunked), Ne uniform, Ne with the scan sweeps: the SCF's stage ==
              sic_channels on Scf.orbitals(); the mix recurrence; the assemble launch and the nine energies replayed in float64.
4. batch      [H, He, Be]: every atom equals its run alone; the first frozen atom keeps every bit, the SIC table included.
5. reference  steps 1 and 2 and the converged H, He, Li, Be, Ne, Fe against tests/_sic_ref.py; H on -0.5 Ha; the -1 / r tail.

Observed on an MI355X: every bit-for-bit comparison holds; EH / EXC / vbar at most 0.042 / 0.038 / 0.042 of their counted bounds; steps 1
and 2 against the CPU reference: eigenvalues 5.3e-4 of the gate, energies 5.8e-12 relative; converged H / He / Li / Be / Ne / Fe 4.8e-12 /
7.4e-12 / 1.7e-12 / 4.1e-12 / 7.6e-13 / 2.0e-12 relative (gate 1e-9); H |E + 0.5| = 3.618e-8, |eps + 0.5| = 7.235e-8.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import _exchange_ref as X                # noqa: E402
import _kli_scf_ref as K                 # noqa: E402
import _orb_ref as OR                    # noqa: E402
import _sic_ref as R                     # noqa: E402
import _slater_ref as S                  # noqa: E402
import _tail_ref as TR                   # noqa: E402
import dftatom_amd as D                  # noqa: E402
from _knobs import knobs                 # noqa: E402

LD, EPS = X.LD, X.EPS
CAP = 60
SPEC = {"log12": R.GRID, "uni12": (12, None, 25.0), "uni11": (11, None, 10.0), "uni10": (10, None, 10.0), "uni3": (3, None, 10.0)}


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.int64)


def same(x, y):
    x, y = np.asarray(x), np.asarray(y)
    return x.shape == y.shape and np.array_equal(bits(x), bits(y))


@pytest.fixture(scope="module")
def ctx(torch_first):
    assert np.finfo(LD).eps < 1.2e-19, "the reference of this file needs an extended np.longdouble"
    c = D.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def grids(ctx):
    """name -> (grid, r as the library holds it, s = dr/di in longdouble)"""
    made = {}

    def get(name):
        if name not in made:
            g = D.Grid(ctx, *SPEC[name])
            made[name] = (g, g.r(), OR.grid(*SPEC[name])[1])
        return made[name]
    yield get
    for g, _, _ in made.values():
        g.close()


def nspin(lsda):
    return 2 if lsda else 1


# ---- 1. the direct entry -------------------------------------------------------------------------------------------------------------------
def check_channels(ctx, grid, r, s, norb, l, occ, E, u, out, what, first=True, alpha=0.5, vx0=None):
    """every stated order of the rule on the device's own rows; returns the largest ratios of EH, EXC, vbar to their counted bounds"""
    N = grid.N
    tot = int(np.sum(norb))
    worst = {"EH": 0.0, "EXC": 0.0, "vbar": 0.0}
    if tot:
        y = D.screening_yk(ctx, grid, u, [(a, a, 0) for a in range(tot)])
        assert same(out["y0"], y), (what, "y0")
        rho = np.stack([R.orbital_density(u[a], r) for a in range(tot)])
        res, va, _, e = D.vwn_lsda(ctx, rho, np.zeros_like(rho))
        assert same(out["vorb"], va) and same(out["eps"], res + e), (what, "orbital xc")
        assert same(out["X"], (out["y0"] + out["vorb"]) * u), (what, "X")
    o = 0
    for c, n in enumerate(norb):
        sl = slice(o, o + n)
        o += n
        if n == 0:
            assert not np.any(out["v_raw"][c]) and not np.any(out["vx"][c]) and out["homo"][c] == -1 and out["Esic"][c] == 0, (what, c)
            continue
        U, nn = u[sl], np.asarray(occ[sl], dtype=np.float64)
        if not np.all(np.isfinite(U)):
            continue                                         # a poisoned channel: the caller looks at it
        Dr, _, vS = R.density_and_slater(U, nn, out["X"][sl])
        assert same(out["D"][c], Dr) and same(out["vS"][c], vS), (what, c, "D / vS")
        homo = X.pick_homo(E[sl], nn)
        assert int(out["homo"][c]) == homo, (what, c, "homo")
        cc = K.solve(out["M"][c], out["vbarS"][sl], out["vbar"][sl], homo)
        assert same(out["c"][sl], cc), (what, c, "c")
        if n == 1:
            assert out["c"][sl][0] == 0
        vK = X.kli_potential(U, nn, homo, out["c"][sl], out["D"][c], out["vS"][c], dtype=np.float64)
        want = K.tail(vK, out["D"][c], r)
        assert same(out["v_raw"][c], want), (what, c, "vKLI / tail")
        assert same(out["vx"][c], K.mix(None if first else vx0[c], want, first, alpha)), (what, c, "mix")
        assert same(out["Esic"][c], R.esic_channel(nn, out["EH"][sl], out["EXC"][sl])), (what, c, "E_SIC")
        # the three quadratures against longdouble on the device's own integrands, counted bounds
        for a in range(n):
            ua = U[a].astype(LD)
            for key, term, kind, f in (("EH", ((ua * ua) * out["y0"][sl][a].astype(LD)) * s, X.SL, LD(0.5)),
                                       ("EXC", ((ua * ua) * out["eps"][sl][a].astype(LD)) * s, X.SL, LD(1)),
                                       ("vbar", (ua * out["X"][sl][a].astype(LD)) * s, X.HF, LD(-1))):
                v, mag = X.quad(term)
                bound = X.red_roundings(N, kind) * EPS * mag * abs(f)
                err = abs(LD(out[key][sl][a]) - f * v)
                assert err <= bound, (what, c, a, key, float(err), float(bound))
                if bound > 0:
                    worst[key] = max(worst[key], float(err / bound))
                else:
                    assert out[key][sl][a] == 0
    return worst


def smooth_case(r):
    """two channels of the four smooth orbitals: (0, 1, 2) and (3,), with a tie of the eigenvalues in the first"""
    u = X.smooth_orbitals(r)
    return [3, 1], [0, 1, 0, 2], np.array([1., 3., 0.5, 5.]), np.array([-2., -1., -1., -0.5]), u


@pytest.mark.parametrize("gname", ["uni3", "uni10", "uni11", "log12"])
def test_direct_every_order_bit_for_bit(ctx, grids, gname):
    """observed on an MI355X, ratios of EH / EXC / vbar to the counted bounds: 9 nodes 0.042 / 0.038 / 0.036, 1025 nodes 0.039 / 0.031 /
    0.042, 2049 nodes 0.032 / 0.009 / 0.016, 4097 logarithmic nodes 0.029 / 0.024 / 0.040"""
    grid, r, s = grids(gname)
    assert grid.N == {"uni3": 9, "uni10": 1025, "uni11": 2049, "log12": 4097}[gname]
    norb, l, occ, E, u = smooth_case(r)
    out = D.sic_channels(ctx, grid, norb, l, occ, E, u)
    worst = check_channels(ctx, grid, r, s, norb, l, occ, E, u, out, gname)
    print("%s: ratios to the bounds %s" % (gname, {k: round(v, 3) for k, v in worst.items()}))
    assert np.all(np.isfinite(out["v_raw"])) and np.all(out["Esic"] < 0) and int(out["homo"][0]) == 2
    vx0 = np.random.default_rng(grid.N).standard_normal((2, grid.N))
    m = D.sic_channels(ctx, grid, norb, l, occ, E, u, first_step=False, alpha=0.3, vx=vx0)
    check_channels(ctx, grid, r, s, norb, l, occ, E, u, m, gname + " mixed", first=False, alpha=0.3, vx0=vx0)
    assert same(m["v_raw"], out["v_raw"])


L6 = [l for _, l in S.ORBS]                                                  # 1s 2s 2p 3d 4f 4s of Z = 10
OCC6 = np.array([1., 1., 3., 5., 7., 1.])
E6 = np.array([-S.ZREF ** 2 / (2. * n * n) for n, _ in S.ORBS])


def hydrogenic(r):
    return S.orbitals(np.asarray(r, dtype=LD)).astype(np.float64)


@pytest.mark.parametrize("cut", [1023, 1024, 1025])
def test_direct_cut_orbitals(ctx, grids, cut):
    grid, r, s = grids("log12")
    u = hydrogenic(r)
    u[:, cut:] = 0
    out = D.sic_channels(ctx, grid, [6], L6, OCC6, E6, u)
    check_channels(ctx, grid, r, s, [6], L6, OCC6, E6, u, out, "cut %d" % cut)
    assert K.last_node(out["D"][0]) == cut - 1 and int(out["homo"][0]) == 5
    assert not np.any(out["X"][:, cut:]) and not np.any(out["vorb"][:, cut:]) and not np.any(out["eps"][:, cut:])
    assert np.all(out["v_raw"][0][cut:] != 0)                # the Coulomb tail


CHANNELS = [(0,), (0, 1), (0, 1, 2), (0, 1, 2, 3), (0, 1, 2, 3, 4), (0, 1, 2, 3, 4, 5), (2,), (1, 2), (0, 2, 3), (3, 4), (0, 5), (2, 3, 4, 5)]
KEYS_ROWS, KEYS_CH = ("y0", "vorb", "eps", "X", "vbar", "vbarS", "c", "EH", "EXC"), ("D", "vS", "v_raw", "vx", "Esic")


def run_channels(ctx, grid, u, chans):
    idx = [i for ch in chans for i in ch]
    return D.sic_channels(ctx, grid, [len(ch) for ch in chans], [L6[i] for i in idx], OCC6[idx], E6[idx], u[idx])


def channel_parts(out, chans):
    parts, o = [], 0
    for k, ch in enumerate(chans):
        parts.append([out[key][o:o + len(ch)] for key in KEYS_ROWS] + [out[key][k] for key in KEYS_CH]
                     + [out["M"][k], np.float64(out["homo"][k])])
        o += len(ch)
    return parts


def test_direct_channels_alone_anywhere_again_and_chunked(ctx, grids):
    grid, r, _ = grids("uni11")
    u = hydrogenic(r)
    whole = channel_parts(run_channels(ctx, grid, u, CHANNELS), CHANNELS)
    again = channel_parts(run_channels(ctx, grid, u, CHANNELS), CHANNELS)
    back = channel_parts(run_channels(ctx, grid, u, CHANNELS[::-1]), CHANNELS[::-1])[::-1]
    with knobs(KLI_Y_MB="0"):
        chunked = channel_parts(run_channels(ctx, grid, u, CHANNELS), CHANNELS)
    for k, ch in enumerate(CHANNELS):
        alone = channel_parts(run_channels(ctx, grid, u, [ch]), [ch])[0]
        for other, what in ((again[k], "again"), (back[k], "reversed"), (chunked[k], "chunked"), (alone, "alone")):
            assert all(same(x, y) for x, y in zip(whole[k], other)), (k, ch, what)
        assert np.all(np.isfinite(whole[k][11])) and whole[k][13] < 0


def test_direct_zero_and_nan_channels(ctx, grids):
    grid, r, s = grids("uni11")
    u = hydrogenic(r)
    N = grid.N
    rows = np.concatenate([u[[0, 1, 2]], np.zeros((1, N)), u[[0, 1, 2]], np.zeros((1, N)), u[[0]]])
    rows[5, 700] = np.nan                                    # the 2s of the third channel
    idx = [0, 1, 2, 0, 0, 1, 2, 1, 0]
    norb = [3, 1, 3, 2]
    out = D.sic_channels(ctx, grid, norb, [L6[i] for i in idx], OCC6[idx], E6[idx], rows)
    check_channels(ctx, grid, r, s, norb, [L6[i] for i in idx], OCC6[idx], E6[idx], rows, out, "zero / NaN")
    clean = channel_parts(run_channels(ctx, grid, u, [(0, 1, 2)]), [(0, 1, 2)])[0]
    got = channel_parts(out, [(0, 1, 2), (0,), (0, 1, 2), (1, 0)])
    assert all(same(x, y) for x, y in zip(got[0], clean))                   # the NaN of another channel does not reach it
    # an all-zero orbital: its X, v_a, eps and energies are exactly 0 -- alone in a channel, and beside a real one
    for g, a in ((got[1], 0), (got[3], 0)):
        assert all(not np.any(g[KEYS_ROWS.index(k)][a]) for k in ("y0", "vorb", "eps", "X", "vbar", "EH", "EXC")), a
    assert not np.any(got[1][11]) and got[1][13] == 0                        # v_raw, E_SIC of the all-zero channel
    assert np.all(np.isfinite(got[3][11])) and got[3][13] < 0
    assert np.isnan(got[2][11][600]) and np.isnan(got[2][13])               # the poisoned channel: every node with D > 0
    assert np.isnan(out["X"][5, 700]) and np.all(np.isfinite(out["X"][4])) and np.all(np.isfinite(out["X"][7:]))
    e = D.sic_channels(ctx, grid, [0, 1], [0], [1.], [-1.], u[:1])
    assert not np.any(e["v_raw"][0]) and e["homo"][0] == -1 and e["Esic"][0] == 0 and np.all(np.isfinite(e["v_raw"][1])) and e["Esic"][1] < 0
    with pytest.raises(D.DftaError, match="no HOMO"):
        D.sic_channels(ctx, grid, [1], [0], [0.], [-1.], u[:1])
    with pytest.raises(D.DftaError, match="outside 0 .. 4"):
        D.sic_channels(ctx, grid, [1], [5], [1.], [-1.], u[:1])


# ---- 2. the switch: values 0 and 1 keep their bits; the refusals ---------------------------------------------------------------------------
def snapshot(scf, a, lsda):
    e, fin = scf.energies()
    return {"arrays": [scf.array(w, a) for w in range(6)], "fin": int(fin[a]), "energies": [getattr(e[a], k) for k in TR.FIELDS],
            "E": [scf.levels(a, sp)["E"].copy() for sp in range(nspin(lsda))]}


def same_snapshot(s, t):
    return (s["fin"] == t["fin"] and same(s["energies"], t["energies"]) and all(same(x, y) for x, y in zip(s["arrays"], t["arrays"]))
            and all(same(x, y) for x, y in zip(s["E"], t["E"])))


def sic_state(scf, a, lsda):
    ex = [scf.exchange(a, sp) for sp in range(nspin(lsda))]
    tb = [scf.sic_table(a, sp) for sp in range(nspin(lsda))]
    return {"vx": [e["vx"] for e in ex], "v_raw": [e["v_raw"] for e in ex], "Ex": ex[0]["Ex"],
            "u": [scf.orbitals(a, sp) for sp in range(nspin(lsda))],
            "table": [np.concatenate([t[k] for k in ("EH", "EXC", "vbar", "c")] + [[t["homo"]]]) if t else np.zeros(0) for t in tb]}


def same_sic(s, t):
    return same(s["Ex"], t["Ex"]) and all(same(x, y) for k in ("vx", "v_raw", "u", "table") for x, y in zip(s[k], t[k]))


def test_values_0_and_1_keep_their_bits_and_refusals(ctx, grids):
    grid, _, _ = grids("log12")
    plain, touched = D.Scf(ctx, grid, [10]), D.Scf(ctx, grid, [10])
    touched.set_exchange(D.EXCHANGE_SIC_KLI)
    touched.set_exchange(D.EXCHANGE_FUNCTIONAL)              # back before the first step: nothing of it stays
    kli, rekli = D.Scf(ctx, grid, [10], exchange=D.EXCHANGE_KLI), D.Scf(ctx, grid, [10], exchange=D.EXCHANGE_SIC_KLI)
    rekli.set_exchange(D.EXCHANGE_KLI)                       # from the third value to the second: the exchange stage's own tables
    try:
        for _ in range(3):
            for scf in (plain, touched, kli, rekli):
                scf.step(want_stats=False)
            assert same_snapshot(snapshot(plain, 0, False), snapshot(touched, 0, False))
            assert same_snapshot(snapshot(kli, 0, False), snapshot(rekli, 0, False))
            a, b, xp = kli.exchange(), rekli.exchange(), kli.exchange_potentials()
            assert same(a["vx"], b["vx"]) and same(a["v_raw"], b["v_raw"]) and same(a["Ex"], b["Ex"])
            ok = xp["D"] > 0
            assert same(a["v_raw"][ok], xp["vKLI"][ok]) and same(a["v_raw"], K.tail(xp["vKLI"], xp["D"], grid.r()))
            assert same(a["Ex"], K.ex_atom(False, [K.ex_channel(xp["occ"], xp["vbar"][:, D.XP_HF])]))
        with pytest.raises(D.DftaError, match="not DFTA_EXCHANGE_SIC_KLI"):
            kli.sic_table()
        with pytest.raises(D.DftaError, match="not DFTA_EXCHANGE_KLI"):
            touched.exchange()
        with pytest.raises(D.DftaError, match="after the first step"):
            plain.set_exchange(D.EXCHANGE_SIC_KLI)
    finally:
        for scf in (plain, touched, kli, rekli):
            scf.close()
    fresh = D.Scf(ctx, grid, [10], exchange=D.EXCHANGE_SIC_KLI)
    with pytest.raises(D.DftaError, match="no SCF step has run"):
        fresh.sic_table()
    with pytest.raises(D.DftaError, match="DFTA_EXCHANGE_SIC_KLI"):
        fresh.set_exchange(3)
    fresh.close()
    with pytest.raises(D.DftaError, match="DFTA_EXCHANGE_SIC_KLI: functional must be DFTA_XC_VWN"):
        D.Scf(ctx, grid, [10], functional=D.XC_PW92, exchange=D.EXCHANGE_SIC_KLI)
    with pytest.raises(D.DftaError, match="DFTA_EXCHANGE_SIC_KLI: mixing must be DFTA_MIX_LINEAR"):
        D.Scf(ctx, grid, [10], mixing=D.MIX_ANDERSON, exchange=D.EXCHANGE_SIC_KLI)


# ---- 3. the stage inside the SCF, the assemble launch and the energies --------------------------------------------------------------------
STAGE = [
    ("Ne LDA", "log12", [10], False, {}, None),
    ("N LSDA", "log12", [7], True, {}, None),
    ("Li LSDA", "log12", [3], True, {}, None),
    ("H LSDA", "log12", [1], True, {}, None),
    ("H He Ne LDA", "log12", [1, 2, 10], False, {}, None),
    ("H He Ne LDA chunked", "log12", [1, 2, 10], False, {}, "0"),
    ("Ne LDA uniform", "uni12", [10], False, {}, None),
    ("Ne LDA scan sweeps", "log12", [10], False, {"sweep_mode": D.SWEEPS_TOLERANCE}, None),
]


def check_stage_and_step(ctx, grid, r, scf, Z, lsda, step, vx, o, stops, label, replay_energies):
    for a in range(len(Z)):
        es = []
        for sp in range(nspin(lsda)):
            got, tb = scf.exchange(a, sp), scf.sic_table(a, sp)
            if tb is None:
                assert not np.any(got["vx"]) and not np.any(got["v_raw"]), (label, a, sp)
                es.append(np.float64(0.))
                continue
            lv = scf.levels(a, sp)
            occ = lv["occupation"] if lsda else 0.5 * lv["occupation"]
            d = D.sic_channels(ctx, grid, [len(lv["l"])], lv["l"], occ, lv["E"], scf.orbitals(a, sp))
            assert same(d["v_raw"][0], got["v_raw"]), (label, a, sp, "v_raw")
            for k in ("EH", "EXC", "vbar", "c"):
                assert same(d[k], tb[k]), (label, a, sp, k)
            assert int(d["homo"][0]) == tb["homo"] == X.pick_homo(lv["E"], occ), (label, a, sp)
            vx[a][sp] = K.mix(vx[a][sp], got["v_raw"], step == 1, 0.5)
            assert same(got["vx"], vx[a][sp]), (label, a, sp, "mix")
            es.append(np.float64(d["Esic"][0]))
        esic = R.esic_atom(lsda, es)
        assert same(scf.exchange(a, 0)["Ex"], esic), (label, a, "E_SIC")
        if not replay_energies:
            continue
        # the functional's launch on the mixed densities, the assemble launch, the potential and the nine energies in float64
        rho, dA, dB, potA, potB, U = (scf.array(w, a) for w in range(6))
        if lsda:
            Vexc, va, vb, eexc = D.vwn_lsda(ctx, dA, dB)
        else:
            Vexc, eexc = D.vwn_lda(ctx, rho)
            va = vb = np.zeros(grid.N)
        Vexc, va, vb, eexc = R.assemble_sic(lsda, Vexc, va, vb, eexc, vx[a][0], vx[a][1], dA, dB, rho)
        wA, wB = TR.potentials(Z[a], lsda, r, U, Vexc, va, vb)
        assert same(potA, wA) and same(potB, wB if lsda else wA), (label, a, "V")
        focc, E, conv = [], [], True
        for sp in range(nspin(lsda)):
            lv = scf.levels(a, sp)
            focc += list(lv["occupation"])
            E += list(lv["E"])
            conv = conv and bool(np.all(lv["converged"] != 0))
        Eel = 0.0
        for f, e in zip(focc, E):
            Eel += float(f) * float(e)
        cnst = TR.log_cnst(grid.Rp, grid.delta, grid.N)
        want = K.energies9(o, Z[a], lsda, r, cnst, rho, dA, dB, U, Vexc, eexc, wA, wB, Eel, esic)
        en, fin = scf.energies()
        bad = [k for k in TR.FIELDS if not same(getattr(en[a], k), want[k])]
        assert not bad, (label, a, bad, [(getattr(en[a], k), want[k]) for k in bad])
        assert stops[a].step(want["Etotal"], conv) == fin[a]


@pytest.mark.parametrize("case", STAGE, ids=[c[0].replace(" ", "_") for c in STAGE])
def test_stage_equals_entry_and_step_replays(ctx, grids, case):
    label, gname, Z, lsda, kw, y_mb = case
    grid, r, _ = grids(gname)
    with knobs(**({"KLI_Y_MB": y_mb} if y_mb is not None else {})):
        scf = D.Scf(ctx, grid, Z, lsda=lsda, alpha=0.5, exchange=D.EXCHANGE_SIC_KLI, **kw)
    vx = [[np.zeros(grid.N), np.zeros(grid.N)] for _ in Z]
    stops = [TR.StopTest() for _ in Z]
    o = K.O.oracle()
    replay = gname == "log12" and not kw                     # the energy replay states the logarithmic grid's ordered sums
    try:
        for step in range(1, 4):
            scf.step(want_stats=False)
            check_stage_and_step(ctx, grid, r, scf, Z, lsda, step, vx, o, stops, "%s step %d" % (label, step), replay)
            assert scf.exchange_ms() > 0
            assert all(np.isfinite(x.Etotal) and x.Etotal < 0 for x in scf.energies()[0])
    finally:
        scf.close()


# ---- 4. a batch, its atoms alone, and the frozen atom ------------------------------------------------------------------------------------
def test_batch_equals_alone_and_frozen_atom_keeps_its_bits(ctx, grids):
    grid, _, _ = grids("log12")
    Z = [1, 2, 4]
    batch = D.Scf(ctx, grid, Z, exchange=D.EXCHANGE_SIC_KLI)
    alone = [D.Scf(ctx, grid, [z], exchange=D.EXCHANGE_SIC_KLI) for z in Z]
    try:
        steps, first = 0, None
        while first is None and steps < CAP:
            batch.step(want_stats=False)
            steps += 1
            fin = batch.energies()[1]
            if fin.any():
                first = int(np.nonzero(fin)[0][0])
        assert first is not None, "no atom of [H, He, Be] finished within %d steps" % CAP
        frozen = (snapshot(batch, first, False), sic_state(batch, first, False))
        batch.step(want_stats=False)
        steps += 1
        assert same_snapshot(frozen[0], snapshot(batch, first, False)) and same_sic(frozen[1], sic_state(batch, first, False))
        print("[H, He, Be]: Z = %d froze first, on step %d" % (Z[first], steps - 1))
        for a, one in enumerate(alone):
            for _ in range(steps):
                one.step(want_stats=False)
            assert same_snapshot(snapshot(batch, a, False), snapshot(one, 0, False)), ("alone", Z[a])
            assert same_sic(sic_state(batch, a, False), sic_state(one, 0, False)), ("alone, SIC", Z[a])
    finally:
        batch.close()
        for one in alone:
            one.close()


# ---- 5. against the CPU reference ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["Ne", "N"])
def test_first_steps_vs_reference(ctx, grids, name):
    """steps 1 and 2: eigenvalues within 1e-8 Ha + 2e-9 |E|, energies within 1e-9 relative"""
    grid, _, _ = grids("log12")
    Z, lsda = R.ATOMS[name]
    ref = R.make(name)
    scf = D.Scf(ctx, grid, [Z], lsda=lsda, exchange=D.EXCHANGE_SIC_KLI)
    try:
        for step in (1, 2):
            scf.step(want_stats=False)
            want_e = ref.step()
            got_e = scf.energies()[0][0].as_list()
            got = np.concatenate([scf.levels(0, sp)["E"] for sp in range(nspin(lsda))])
            want = np.concatenate([ref.levels(sp) for sp in range(nspin(lsda))])
            gate = 1e-8 + 2e-9 * np.abs(want)
            re = max(abs(a - b) / abs(b) for a, b in zip(got_e, want_e))
            print("%s step %d: eigenvalues %.1e of the gate, energies %.2e relative (gate 1e-9); E_SIC %.3e relative"
                  % (name, step, np.max(np.abs(got - want) / gate), re, abs(scf.exchange()["Ex"] - ref.Ex) / abs(ref.Ex)))
            assert np.all(np.abs(got - want) <= gate), (step, got, want)
            assert np.allclose(got_e, want_e, rtol=1e-9, atol=0), (step, got_e, want_e)
    finally:
        scf.close()
        ref.close()


_gpu_runs, _ref_runs = {}, {}


def converged_pair(ctx, grid, name):
    """(GPU energy, levels, r vx at the last node per channel, steps), the CPU reference run: both to their stop test, once per session"""
    if name not in _gpu_runs:
        Z, lsda = R.ATOMS[name]
        scf = D.Scf(ctx, grid, [Z], lsda=lsda, exchange=D.EXCHANGE_SIC_KLI)
        steps = 0
        while not scf.energies()[1][0] and steps < CAP:
            scf.step(want_stats=False)
            steps += 1
        _gpu_runs[name] = {"fin": int(scf.energies()[1][0]), "E": scf.energies()[0][0].Etotal, "eps": scf.levels(0, 0)["E"].copy(),
                           "tail": [float(grid.r()[-1] * scf.exchange(0, sp)["vx"][-1]) for sp in range(nspin(lsda))], "steps": steps,
                           "Esic": scf.exchange()["Ex"]}
        scf.close()
        ref = R.make(name)
        ref.run(CAP)
        _ref_runs[name] = ref
    return _gpu_runs[name], _ref_runs[name]


@pytest.mark.parametrize("name", ["H", "He", "Li", "Be", "Ne", "Fe"])
def test_converged_vs_reference(ctx, grids, name):
    """Fe (LSDA, Aufbau) finishes here; under EXCHANGE_KLI it oscillates"""
    grid, _, _ = grids("log12")
    gpu, ref = converged_pair(ctx, grid, name)
    assert gpu["fin"] and ref.finished, (name, gpu["steps"], ref.steps)
    rel = abs(gpu["E"] - ref.en["Etotal"]) / abs(ref.en["Etotal"])
    print("%s: GPU %d steps, reference %d; E %.12f vs %.12f, %.2e relative (gate 1e-9); E_SIC %.9f vs %.9f"
          % (name, gpu["steps"], ref.steps, gpu["E"], ref.en["Etotal"], rel, gpu["Esic"], ref.Ex))
    assert rel <= 1e-9


def test_hydrogen_and_the_tail(ctx, grids):
    grid, _, _ = grids("log12")
    h, _ = converged_pair(ctx, grid, "H")
    assert h["fin"]
    dE, de, dt = abs(h["E"] + 0.5), abs(h["eps"][0] + 0.5), abs(1 + h["tail"][0])
    print("H: |E + 0.5| = %.3e (CPU %.2e), |eps + 0.5| = %.3e (CPU %.2e), |1 + r vx| = %.3e"
          % (dE, R.MEASURED["H_E"], de, R.MEASURED["H_eps"], dt))
    assert dE <= 2 * R.MEASURED["H_E"] and de <= 2 * R.MEASURED["H_eps"]
    assert dt <= 2e-13                                       # CPU: round-off, held under 1e-13
    for name in ("Be", "Ne"):
        g, _ = converged_pair(ctx, grid, name)
        t = abs(1 + g["tail"][0])
        print("%s: |1 + r vx| = %.3e (CPU %.2e)" % (name, t, R.MEASURED["tail"][name][0]))
        assert t <= 2 * R.MEASURED["tail"][name][0]


def test_cli_exchange_sic():
    """dftatom_cli --exchange=sic: hydrogen (LSDA) ends on -0.5 Ha; --sic-table prints the per-shell table and changes nothing else"""
    import os
    import re
    import subprocess
    exe = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "dftatom_amd", "compat", "dftatom_cli")
    args = [exe, "1", "12", "0.5", "25", "0.002", "1", "--exchange=sic"]
    run = subprocess.run(args + ["--sic-table"], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and "Finished!" in run.stdout, run.stderr[-2000:]
    etot = float(re.findall(r"Etotal = (-?\d+\.\d+)", run.stdout)[-1])
    assert abs(etot + 0.5) <= 2 * R.MEASURED["H_E"] + 5e-7   # six printed decimals
    table = [ln for ln in run.stdout.split("\n") if ln.startswith("SIC ") or ln.startswith("ESIC ")]
    assert len(table) == 2 and " EH = " in table[0] and " EXC = " in table[0] and " vbar = " in table[0] and " c = " in table[0]
    assert abs(float(table[1].split("=")[1]) - R.MEASURED["E"]["H"][2]) < 2e-6
    bare = subprocess.run(args, capture_output=True, text=True, timeout=120)
    assert bare.returncode == 0
    assert [ln for ln in run.stdout.split("\n") if ln not in table and ln != ""] == [ln for ln in bare.stdout.split("\n") if ln != ""]
