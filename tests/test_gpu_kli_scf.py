"""GPU suite (-m gpu): the self-consistent exchange-only KLI step -- dfta_scf_set_exchange, the batched exchange stage of
dftatom_amd/csrc/kli_stage.hip and the direct entry dfta_kli_channels; include/dftatom_hip.h states the rule, tests/_kli_scf_ref.py is the
CPU reference and the float64 statement of every stage.

1. default    set_exchange(EXCHANGE_FUNCTIONAL) changes no bit of three Ne steps; the four refusals; functional = 5 keeps its old text.
2. stage      Steps 1 - 3 of Ne LDA, N LSDA, Li LSDA, H LSDA, [H, He, Ne] LDA (also with one channel per chunk), Ne on the uniform grid, Ne
              with the scan sweeps: v_raw at the nodes with D > 0, vbarHF, c and the HOMO equal Scf.exchange_potentials bit for bit, E_x the
              float64 sum in the stated order.
3. direct     Hydrogen-like orbitals cut to zero at 1023 .. 2048 of 4097 nodes: tail and mix equal the float64 replay bit for bit; twelve
              channels in one call equal each alone, reversed, repeated and with one channel per chunk; an all-zero channel; a NaN node.
4. mix        Steps 1 - 4: vx is the recurrence on the device's own v_raw; the potentials (arrays 3 / 4) the replay from U and vx.
5. energies   The nine energies and `finished` from the device's own arrays plus E_x, bit for bit.
6. batch      [H, He, Be] LDA to the first freeze plus three steps: every atom equals its run alone; the frozen atom keeps every bit.
7. reference  Steps 1 and 2 of Ne LDA and N LSDA against the CPU reference at the VWN path's gates; converged He, Be, Ne within 1e-9.
8. physics    H (LSDA) on -0.5 Ha, He on Hartree-Fock, each within twice the CPU reference's own distance; the -1 / r tail of Ne.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import _exchange_ref as X                # noqa: E402
import _kli_scf_ref as K                 # noqa: E402
import _slater_ref as S                  # noqa: E402
import _tail_ref as TR                   # noqa: E402
import dftatom_amd as D                  # noqa: E402
from _knobs import knobs                 # noqa: E402

LD = np.longdouble
LOG12 = K.GRID
CAP = 60


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.int64)


def same(x, y):
    x, y = np.asarray(x), np.asarray(y)
    return x.shape == y.shape and np.array_equal(bits(x), bits(y))


@pytest.fixture(scope="module")
def ctx(torch_first):
    c = D.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def grids(ctx):
    """name -> (grid, r as the library holds it)"""
    spec = {"log12": LOG12, "uni12": (12, None, 25.0), "uni11": (11, None, 10.0)}
    made = {}

    def get(name):
        if name not in made:
            g = D.Grid(ctx, *spec[name])
            made[name] = (g, g.r())
        return made[name]
    yield get
    for g, _ in made.values():
        g.close()


def nspin(lsda):
    return 2 if lsda else 1


def snapshot(scf, a, lsda):
    e, fin = scf.energies()
    out = {"arrays": [scf.array(w, a) for w in range(6)], "fin": int(fin[a]),
           "energies": [getattr(e[a], k) for k in TR.FIELDS],
           "E": [scf.levels(a, sp)["E"].copy() for sp in range(nspin(lsda))]}
    return out


def same_snapshot(s, t):
    return (s["fin"] == t["fin"] and same(s["energies"], t["energies"]) and all(same(x, y) for x, y in zip(s["arrays"], t["arrays"]))
            and all(same(x, y) for x, y in zip(s["E"], t["E"])))


def kli_state(scf, a, lsda):
    """vx, v_raw per channel, E_x and the orbitals of atom a"""
    ex = [scf.exchange(a, sp) for sp in range(nspin(lsda))]
    return {"vx": [e["vx"] for e in ex], "v_raw": [e["v_raw"] for e in ex], "Ex": ex[0]["Ex"],
            "u": [scf.orbitals(a, sp) for sp in range(nspin(lsda))]}


def same_kli(s, t):
    return (same(s["Ex"], t["Ex"]) and all(same(x, y) for k in ("vx", "v_raw", "u") for x, y in zip(s[k], t[k])))


# ---- 1. the default path is untouched; the refusals ----------------------------------------------------------------------------------
def test_default_untouched_and_refusals(ctx, grids):
    grid, _ = grids("log12")
    plain, touched = D.Scf(ctx, grid, [10]), D.Scf(ctx, grid, [10], exchange=D.EXCHANGE_FUNCTIONAL)
    touched.set_exchange(D.EXCHANGE_KLI)
    touched.set_exchange(D.EXCHANGE_FUNCTIONAL)              # back before the first step: nothing of it stays
    try:
        for _ in range(3):
            plain.step(want_stats=False)
            touched.step(want_stats=False)
            assert same_snapshot(snapshot(plain, 0, False), snapshot(touched, 0, False))
        with pytest.raises(D.DftaError, match="not DFTA_EXCHANGE_KLI"):
            touched.exchange()
        with pytest.raises(D.DftaError, match="no exchange stage"):
            touched.exchange_ms()
        with pytest.raises(D.DftaError, match="after the first step"):
            plain.set_exchange(D.EXCHANGE_KLI)
    finally:
        plain.close()
        touched.close()
    fresh = D.Scf(ctx, grid, [10])
    with pytest.raises(D.DftaError, match="DFTA_EXCHANGE_FUNCTIONAL or DFTA_EXCHANGE_KLI"):
        fresh.set_exchange(7)
    fresh.set_exchange(D.EXCHANGE_KLI)
    with pytest.raises(D.DftaError, match="no SCF step has run"):
        fresh.exchange()
    fresh.close()
    with pytest.raises(D.DftaError, match="functional must be DFTA_XC_VWN"):
        D.Scf(ctx, grid, [10], functional=D.XC_PW92, exchange=D.EXCHANGE_KLI)
    with pytest.raises(D.DftaError, match="mixing must be DFTA_MIX_LINEAR"):
        D.Scf(ctx, grid, [10], mixing=D.MIX_ANDERSON, exchange=D.EXCHANGE_KLI)
    with pytest.raises(D.DftaError, match=r"functional \(DFTA_XC_VWN \.\. DFTA_XC_PBE\)"):
        D.Scf(ctx, grid, [10], functional=5)


# ---- 2. the stage equals the existing entry ----------------------------------------------------------------------------------------------
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


def check_stage_against_entry(ctx, grid, scf, Z, lsda, label):
    """every channel of every atom: the SCF's stage == Scf.exchange_potentials, and == the direct entry on the same orbitals"""
    for a in range(len(Z)):
        exs = []
        for sp in range(nspin(lsda)):
            got = scf.exchange(a, sp)
            xp = scf.exchange_potentials(a, sp)
            if xp is None:
                assert not np.any(got["vx"]) and not np.any(got["v_raw"]), (label, a, sp)
                exs.append(np.float64(0.))
                continue
            ok = xp["D"] > 0
            assert ok.any() and same(got["v_raw"][ok], xp["vKLI"][ok]), (label, a, sp)
            assert same(got["v_raw"], K.tail(xp["vKLI"], xp["D"], grid.r())), (label, a, sp, "tail")
            lv = scf.levels(a, sp)
            d = D.kli_channels(ctx, grid, [len(lv["l"])], lv["l"], xp["occ"], lv["E"], scf.orbitals(a, sp))
            assert same(d["v_raw"][0], got["v_raw"]), (label, a, sp, "direct entry")
            assert same(d["vbarHF"], xp["vbar"][:, D.XP_HF]) and same(d["c"], xp["vbar"][:, D.XP_C]), (label, a, sp)
            assert int(d["homo"][0]) == xp["homo"] == X.pick_homo(lv["E"], xp["occ"]), (label, a, sp)
            # the device solve is the float64 statement of the header's elimination order on the same M and averages
            assert same(d["c"], K.solve(xp["M"], xp["vbar"][:, D.XP_S], xp["vbar"][:, D.XP_HF], xp["homo"])), (label, a, sp, "solve")
            exs.append(K.ex_channel(xp["occ"], xp["vbar"][:, D.XP_HF]))
            assert same(d["Ex"][0], exs[-1]), (label, a, sp)
        assert same(scf.exchange(a, 0)["Ex"], K.ex_atom(lsda, exs)), (label, a, "E_x")


@pytest.mark.parametrize("case", STAGE, ids=[c[0].replace(" ", "_") for c in STAGE])
def test_stage_equals_entry(ctx, grids, case):
    label, gname, Z, lsda, kw, y_mb = case
    grid, _ = grids(gname)
    with knobs(**({"KLI_Y_MB": y_mb} if y_mb is not None else {})):
        scf = D.Scf(ctx, grid, Z, lsda=lsda, exchange=D.EXCHANGE_KLI, **kw)
    try:
        for step in range(1, 4):
            scf.step(want_stats=False)
            check_stage_against_entry(ctx, grid, scf, Z, lsda, "%s step %d" % (label, step))
            assert scf.exchange_ms() > 0
            e = scf.energies()[0]
            assert all(np.isfinite(x.Etotal) and x.Etotal < 0 for x in e)
    finally:
        scf.close()


# ---- 3. the direct entry -------------------------------------------------------------------------------------------------------------------
L6 = [l for _, l in S.ORBS]                                                  # 1s 2s 2p 3d 4f 4s of Z = 10
OCC6 = np.array([1., 1., 3., 5., 7., 1.])
E6 = np.array([-S.ZREF ** 2 / (2. * n * n) for n, _ in S.ORBS])              # 4f and 4s tie: the HOMO is the higher index


def hydrogenic(r):
    return S.orbitals(np.asarray(r, dtype=LD)).astype(np.float64)


@pytest.mark.parametrize("cut", [1023, 1024, 1025, 2048])
def test_direct_tail_and_mix_on_cut_orbitals(ctx, grids, cut):
    grid, r = grids("log12")
    u = hydrogenic(r)
    u[:, cut:] = 0
    homo = X.pick_homo(E6, OCC6)
    assert homo == 5
    xp = D.exchange_potentials(ctx, grid, L6, OCC6, homo, u)
    assert K.last_node(xp["D"]) == cut - 1
    d = D.kli_channels(ctx, grid, [6], L6, OCC6, E6, u)
    want = K.tail(xp["vKLI"], xp["D"], r)
    assert same(d["v_raw"][0], want) and same(d["vx"][0], want)
    assert np.all(d["v_raw"][0][cut:] != 0) and same(d["v_raw"][0][:cut], xp["vKLI"][:cut])
    assert same(d["vbarHF"], xp["vbar"][:, D.XP_HF]) and same(d["c"], xp["vbar"][:, D.XP_C]) and int(d["homo"][0]) == homo
    assert same(d["Ex"][0], K.ex_channel(OCC6, xp["vbar"][:, D.XP_HF]))
    vx0 = np.random.default_rng(cut).standard_normal((1, grid.N))
    m = D.kli_channels(ctx, grid, [6], L6, OCC6, E6, u, first_step=False, alpha=0.3, vx=vx0)
    assert same(m["v_raw"], d["v_raw"]) and same(m["vx"][0], K.mix(vx0[0], want, False, 0.3))


CHANNELS = [(0,), (0, 1), (0, 1, 2), (0, 1, 2, 3), (0, 1, 2, 3, 4), (0, 1, 2, 3, 4, 5), (2,), (1, 2), (0, 2, 3), (3, 4), (0, 5), (2, 3, 4, 5)]


def run_channels(ctx, grid, u, chans):
    idx = [i for ch in chans for i in ch]
    return D.kli_channels(ctx, grid, [len(ch) for ch in chans], [L6[i] for i in idx], OCC6[idx], E6[idx], u[idx])


def channel_parts(out, chans):
    """per channel: (v_raw, vx, vbarHF, c, homo, Ex)"""
    parts, o = [], 0
    for k, ch in enumerate(chans):
        parts.append((out["v_raw"][k], out["vx"][k], out["vbarHF"][o:o + len(ch)], out["c"][o:o + len(ch)], np.float64(out["homo"][k]),
                      out["Ex"][k]))
        o += len(ch)
    return parts


def test_direct_channels_alone_anywhere_again_and_chunked(ctx, grids):
    grid, r = grids("uni11")
    assert grid.N == 2049
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
        assert np.all(np.isfinite(whole[k][0])) and whole[k][5] < 0


def test_direct_zero_and_nan_channels(ctx, grids):
    grid, r = grids("uni11")
    u = hydrogenic(r)
    N = grid.N
    chans = [(0, 1, 2), (0,), (0, 1, 2)]
    rows = np.concatenate([u[[0, 1, 2]], np.zeros((1, N)), u[[0, 1, 2]]])
    rows[5, 700] = np.nan                                    # the 2s of the last channel
    idx = [0, 1, 2, 0, 0, 1, 2]
    out = D.kli_channels(ctx, grid, [3, 1, 3], [L6[i] for i in idx], OCC6[idx], E6[idx], rows)
    clean = channel_parts(run_channels(ctx, grid, u, [chans[0]]), [chans[0]])[0]
    got = channel_parts(out, chans)
    assert all(same(x, y) for x, y in zip(got[0], clean))                   # the NaN of another channel does not reach it
    assert not np.any(got[1][0]) and not np.any(got[1][1]) and got[1][5] == 0 and got[1][3][0] == 0 and got[1][4] == 0     # all zeros
    assert np.isnan(got[2][0][600]) and np.isnan(got[2][5]) and np.all(np.isnan(got[2][3][:2]))      # c = NaN: every node with D > 0
    # channels without shells, and the refusals
    e = D.kli_channels(ctx, grid, [0, 1], [0], [1.], [-1.], u[:1])
    assert not np.any(e["v_raw"][0]) and e["homo"][0] == -1 and e["Ex"][0] == 0 and np.all(np.isfinite(e["v_raw"][1])) and e["Ex"][1] < 0
    with pytest.raises(D.DftaError, match="no HOMO"):
        D.kli_channels(ctx, grid, [1], [0], [0.], [-1.], u[:1])
    with pytest.raises(D.DftaError, match="outside 0 .. 4"):
        D.kli_channels(ctx, grid, [1], [5], [1.], [-1.], u[:1])


# ---- 4. the mix and the assembly, 5. the energies ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [("Ne LDA", [10], False), ("N LSDA", [7], True)], ids=["Ne_LDA", "N_LSDA"])
def test_mix_assembly_and_energies(ctx, grids, case):
    """steps 1 - 4: vx from the recurrence on the device's own v_raw; arrays 3 / 4 from U and vx; the nine energies and the stop flag from
    the device's own arrays plus E_x -- all bit for bit"""
    label, Z, lsda = case
    grid, r = grids("log12")
    cnst = TR.log_cnst(grid.Rp, grid.delta, grid.N)
    scf = D.Scf(ctx, grid, Z, lsda=lsda, alpha=0.5, exchange=D.EXCHANGE_KLI)
    stop = TR.StopTest()
    o = K.O.oracle()
    try:
        vx = [np.zeros(grid.N), np.zeros(grid.N)]
        for step in range(1, 5):
            scf.step(want_stats=False)
            st = kli_state(scf, 0, lsda)
            for sp in range(nspin(lsda)):
                vx[sp] = K.mix(vx[sp], st["v_raw"][sp], step == 1, 0.5)
                assert same(st["vx"][sp], vx[sp]), (label, step, sp, "mix")
            rho, dA, dB, potA, potB, U = (scf.array(w, 0) for w in range(6))
            Vexc, va, vb, eexc = K.assemble(lsda, vx[0], vx[1], dA, dB, rho)
            wA, wB = TR.potentials(Z[0], lsda, r, U, Vexc, va, vb)
            assert same(potA, wA) and same(potB, wB if lsda else wA), (label, step, "V")
            occ, E, conv = [], [], True
            for sp in range(nspin(lsda)):
                lv = scf.levels(0, sp)
                occ += list(lv["occupation"])
                E += list(lv["E"])
                conv = conv and bool(np.all(lv["converged"] != 0))
            Eel = 0.0
            for f, e in zip(occ, E):
                Eel += float(f) * float(e)
            want = K.energies9(o, Z[0], lsda, r, cnst, rho, dA, dB, U, Vexc, eexc, wA, wB, Eel, st["Ex"])
            en, fin = scf.energies()
            bad = [k for k in TR.FIELDS if not same(getattr(en[0], k), want[k])]
            assert not bad, (label, step, bad, [(getattr(en[0], k), want[k]) for k in bad])
            assert stop.step(want["Etotal"], conv) == fin[0]
            assert en[0].Exc == pytest.approx(st["Ex"], rel=1e-12)         # exchange only: Exc is E_x up to the two integrals' rounding
    finally:
        scf.close()


# ---- 6. a batch, its atoms alone, and the frozen atom ----------------------------------------------------------------------------------
def test_batch_equals_alone_and_frozen_atom_keeps_its_bits(ctx, grids):
    grid, _ = grids("log12")
    Z = [1, 2, 4]
    batch = D.Scf(ctx, grid, Z, exchange=D.EXCHANGE_KLI)
    alone = [D.Scf(ctx, grid, [z], exchange=D.EXCHANGE_KLI) for z in Z]
    try:
        steps, first = 0, None
        while first is None and steps < CAP:
            batch.step(want_stats=False)
            steps += 1
            fin = batch.energies()[1]
            if fin.any():
                first = int(np.nonzero(fin)[0][0])
        assert first is not None, "no atom of [H, He, Be] finished within %d steps" % CAP
        frozen = (snapshot(batch, first, False), kli_state(batch, first, False))
        for _ in range(3):
            batch.step(want_stats=False)
            steps += 1
        assert same_snapshot(frozen[0], snapshot(batch, first, False)) and same_kli(frozen[1], kli_state(batch, first, False))
        print("[H, He, Be]: Z = %d froze first, on step %d" % (Z[first], steps - 3))
        for a, one in enumerate(alone):
            for _ in range(steps):
                one.step(want_stats=False)
            assert same_snapshot(snapshot(batch, a, False), snapshot(one, 0, False)), ("alone", Z[a])
            assert same_kli(kli_state(batch, a, False), kli_state(one, 0, False)), ("alone, exchange", Z[a])
    finally:
        batch.close()
        for one in alone:
            one.close()


# ---- 7. against the CPU reference ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["Ne", "N"])
def test_first_steps_vs_reference(ctx, grids, name):
    """steps 1 and 2 at the VWN path's gates: eigenvalues 1e-8 Ha + 1e-10 |E| resp. 2e-9 |E|, energies 1e-9 relative"""
    grid, _ = grids("log12")
    Z, lsda = K.ATOMS[name]
    ref = K.make(name)
    scf = D.Scf(ctx, grid, [Z], lsda=lsda, exchange=D.EXCHANGE_KLI)
    try:
        for step, rel in ((1, 1e-10), (2, 2e-9)):
            scf.step(want_stats=False)
            want_e = ref.step()
            got_e = scf.energies()[0][0].as_list()
            got = np.concatenate([scf.levels(0, sp)["E"] for sp in range(nspin(lsda))])
            want = np.concatenate([ref.levels(sp) for sp in range(nspin(lsda))])
            gate = 1e-8 + rel * np.abs(want)
            re = max(abs(a - b) / abs(b) for a, b in zip(got_e, want_e))
            print("%s step %d: eigenvalues %.1e of the gate, energies %.2e relative (gate 1e-9); E_x %.3e relative"
                  % (name, step, np.max(np.abs(got - want) / gate), re, abs(scf.exchange()["Ex"] - ref.Ex) / abs(ref.Ex)))
            assert np.all(np.abs(got - want) <= gate), (step, got, want)
            assert np.allclose(got_e, want_e, rtol=1e-9, atol=0), (step, got_e, want_e)
    finally:
        scf.close()
        ref.close()


_gpu_runs, _ref_runs = {}, {}


def converged_pair(ctx, grid, name):
    """(GPU energies, levels, r vx at the last node, steps), the CPU reference run: both to their stop test, once per session"""
    if name not in _gpu_runs:
        Z, lsda = K.ATOMS[name]
        scf = D.Scf(ctx, grid, [Z], lsda=lsda, exchange=D.EXCHANGE_KLI)
        steps = 0
        while not scf.energies()[1][0] and steps < CAP:
            scf.step(want_stats=False)
            steps += 1
        _gpu_runs[name] = {"fin": int(scf.energies()[1][0]), "E": scf.energies()[0][0].Etotal, "eps": scf.levels(0, 0)["E"].copy(),
                           "tail": float(grid.r()[-1] * scf.exchange()["vx"][-1]), "steps": steps}
        scf.close()
        ref = K.make(name)
        ref.run(CAP)
        _ref_runs[name] = ref
    return _gpu_runs[name], _ref_runs[name]


@pytest.mark.parametrize("name", ["He", "Be", "Ne"])
def test_converged_vs_reference(ctx, grids, name):
    grid, _ = grids("log12")
    gpu, ref = converged_pair(ctx, grid, name)
    assert gpu["fin"] and ref.finished, (name, gpu["steps"], ref.steps)
    rel = abs(gpu["E"] - ref.en["Etotal"]) / abs(ref.en["Etotal"])
    print("%s: GPU %d steps, reference %d; E %.12f vs %.12f, %.2e relative (gate 1e-9)" % (name, gpu["steps"], ref.steps, gpu["E"],
                                                                                         ref.en["Etotal"], rel))
    assert rel <= 1e-9


# ---- 8. physics ------------------------------------------------------------------------------------------------------------------------
def test_hydrogen_helium_and_the_tail(ctx, grids):
    grid, _ = grids("log12")
    h, _ = converged_pair(ctx, grid, "H")
    assert h["fin"]
    dE, de = abs(h["E"] + 0.5), abs(h["eps"][0] + 0.5)
    print("H: |E + 0.5| = %.3e (CPU %.1e), |eps + 0.5| = %.3e (CPU %.1e)" % (dE, K.MEASURED["H_E"], de, K.MEASURED["H_eps"]))
    assert dE <= 2 * K.MEASURED["H_E"] and de <= 2 * K.MEASURED["H_eps"]
    he, _ = converged_pair(ctx, grid, "He")
    dHe = abs(he["E"] - K.E_HE_HF)
    print("He: |E - E_HF| = %.3e (CPU %.1e)" % (dHe, K.MEASURED["He_E"]))
    assert he["fin"] and dHe <= 2 * K.MEASURED["He_E"]
    ne, ref = converged_pair(ctx, grid, "Ne")
    want = float(ref.pos[-1] * ref.vx[0][-1])
    print("Ne: r vx at the last node %.9f (CPU %.9f)" % (ne["tail"], want))
    assert abs(ne["tail"] + 1) <= 2 * K.MEASURED["tail_Ne"]


def test_cli_exchange_kli():
    """dftatom_cli --exchange=kli: neon ends on the literature's -128.5448 Ha; --exchange-table works on top of it"""
    import os
    import re
    import subprocess
    exe = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "dftatom_amd", "compat", "dftatom_cli")
    run = subprocess.run([exe, "10", "12", "0.5", "25", "0.002", "0", "--exchange=kli", "--exchange-table"], capture_output=True, text=True,
                         timeout=120)
    assert run.returncode == 0 and "Finished!" in run.stdout, run.stderr[-2000:]
    etot = float(re.findall(r"Etotal = (-?\d+\.\d+)", run.stdout)[-1])
    assert "%.4f" % etot == "-128.5448", etot
    assert any(ln.startswith("Exchange ") for ln in run.stdout.split("\n"))
    bad = subprocess.run([exe, "10", "12", "0.5", "25", "0.002", "0", "--exchange=oep"], capture_output=True, text=True, timeout=120)
    assert bad.returncode != 0 and "unknown exchange" in bad.stderr
