"""GPU suite (-m gpu): SCF steps under PW92, PBE and fractional / non-Aufbau configurations against the CPU step reference
tests/_scf_ref.py (anchored bit for bit to the oracle in tests/test_scf_ref.py).  Grid (14, 5e-4, 25) throughout.

(a) free-running: steps 1 and 2 from the flat start density, every eigenvalue and the five energies, with the gates the project
    uses for a step against the oracle (test_reference_rounding_sensitivity_of_scf_steps): eigenvalues 1e-8 Ha + 1e-10 |E| at
    step 1 (a common potential), 1e-8 Ha + 2e-9 |E| at step 2 (one Poisson solve later), energies 1e-9 relative.

(b) replay at late steps: the GPU runs to step k, its rho_k and V_k are read, it takes one more step, and every stage of that
    step is checked against the CPU from the GPU's OWN input to that stage, so nothing compounds:
      eigenvalues from V_k                               1e-8 Ha + 1e-10 |E|
      rho_k+1 = alpha rho_k + (1 - alpha) Sum f Psi^2    twice the node-wise envelope measured on the reference: the change of
                                                         Sum f Psi^2 / (4 pi r^2) when every level's E moves by +-2e-12 Ha (the
                                                         bound of BASELINE.md section 3 on eigenvalues from a given potential),
                                                         running maximum over +-8 nodes, plus 4 eps rho for the mixing
      U_k+1 from the GPU's rho_k+1 and N_e               1e-10 Z
      v_xc = V_k+1 - (-Z + U_k+1) / r                    the measure of test_gpu_xc_radial.py, 8 E + 1e-11 T against the
                                                         extended-precision _gga_ref.radial on the GPU's rho_k+1, plus 2 eps |V|:
                                                         V is stored rounded and v_xc is recovered from it by a subtraction
      the five energies from the GPU's rho, U, V, eigenvalues and the configuration's occupations, Vexc / eexc of the
      reference on the GPU's rho_k+1                     1e-9 relative
    at k = 20 and on the step on which the atom finishes; and inside the batches [He, Ar, Ar 3p5.5, Ar+] (Ar+ finishes on step
    32, He on 34, the two others on 35) and [Fe, He, Na] (Fe finishes on step 25, He on 34, Na on 43): a frozen atom keeps every
    bit from step to step while the live atoms pass the replay.

Observed on an MI355X (largest ratio to the gate over all cases; every test prints its own): (a) eigenvalues 0.008, energies
6.1e-11 relative; (b) eigenvalues 5e-4 (mostly the oracle's bits), rho 0.081, U 0 (the oracle's bits), v_xc 0.25, energies 2.3e-6
of the gate.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import _gga_ref as R                     # noqa: E402
import _scf_ref as SR                    # noqa: E402
import dftatom_amd as D                  # noqa: E402

LD = np.longdouble
GRID = (14, 5e-4, 25.0)
EPS = np.finfo(float).eps


@pytest.fixture(scope="module")
def ctx(torch_first):
    c = D.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def grid(ctx):
    g = D.Grid(ctx, *GRID)
    yield g
    g.close()


def make(ctx, grid, Z, lsda, functional, config=None, charge=None):
    """(GPU Scf of one atom, its CPU reference)"""
    if config is not None:
        cfg = D.parse_config(Z, config, lsda)
    else:
        cfg = D.ion_config(Z, charge or 0, lsda)
    kw = {} if (config is None and not charge) else {"config": [cfg]}
    scf = D.Scf(ctx, grid, [Z], lsda=lsda, functional=functional, **kw)
    a, b = SR.config_levels(cfg, lsda)
    ref = SR.ScfRef(Z, a, b, functional=functional, mg_levels=GRID[0], delta=GRID[1], MaxR=GRID[2])
    return scf, ref


def assert_config(scf, atom, ref):
    """the GPU's level list is the reference's: n, l and the (fractional) occupations"""
    for sp in range(2 if ref.lsda else 1):
        lv = scf.levels(atom, sp)
        want = ref.cfg[sp]
        assert [(int(n), int(l), float(f)) for n, l, f in zip(lv["n"], lv["l"], lv["occupation"])] == want, (atom, sp)


# ---- (a) free-running --------------------------------------------------------------------------------------------------------
FREE = [
    ("PW92 LDA Ne", 10, False, D.XC_PW92, None, None),
    ("PW92 LSDA N", 7, True, D.XC_PW92, None, None),
    ("PBE LDA Ar", 18, False, D.XC_PBE, None, None),
    ("PBE LSDA N", 7, True, D.XC_PBE, None, None),
    ("PBE LSDA H", 1, True, D.XC_PBE, None, None),
    ("VWN LDA Ar 3p5.5", 18, False, D.XC_VWN, "[Ne] 3s2 3p5.5", None),
    ("PBE LDA Ar 3p5.5", 18, False, D.XC_PBE, "[Ne] 3s2 3p5.5", None),
    ("VWN LSDA N 2p2.5/0.5", 7, True, D.XC_VWN, "1s2 2s2 2p2.5/0.5", None),
    ("PBE LSDA N 2p2.5/0.5", 7, True, D.XC_PBE, "1s2 2s2 2p2.5/0.5", None),
    ("PBE LSDA Fe2+", 26, True, D.XC_PBE, None, 2),
]


@pytest.mark.parametrize("case", FREE, ids=[c[0].replace(" ", "_") for c in FREE])
def test_first_steps_vs_reference(ctx, grid, case):
    name, Z, lsda, fx, config, charge = case
    scf, ref = make(ctx, grid, Z, lsda, fx, config, charge)
    try:
        for step, rel in ((1, 1e-10), (2, 2e-9)):
            scf.step(want_stats=False)
            assert_config(scf, 0, ref)
            want_e = ref.step()
            got_e = scf.energies()[0][0].as_list()
            got = np.concatenate([scf.levels(0, sp)["E"] for sp in range(2 if lsda else 1)])
            want = np.concatenate([ref.levels(sp) for sp in range(2 if lsda else 1)])
            assert got.shape == want.shape
            gate = 1e-8 + rel * np.abs(want)
            re = max(abs(a - b) / abs(b) for a, b in zip(got_e, want_e))
            print("%-22s step %d: eigenvalues %.1e of the gate, energies %.2e relative (gate 1e-9)"
                  % (name, step, np.max(np.abs(got - want) / gate), re))
            assert np.all(np.abs(got - want) <= gate), (step, got, want)
            assert np.allclose(got_e, want_e, rtol=1e-9, atol=0), (step, got_e, want_e)
    finally:
        scf.close()
        ref.close()


# ---- (b) replay --------------------------------------------------------------------------------------------------------------
def snap(scf, atom, lsda):
    e, fin = scf.energies()
    s = {"rho": scf.array(0, atom), "U": scf.array(5, atom), "potA": scf.array(3, atom), "fin": int(fin[atom]),
         "energies": e[atom].as_list(), "E": [scf.levels(atom, sp)["E"].copy() for sp in range(2 if lsda else 1)]}
    if lsda:
        s.update(dA=scf.array(1, atom), dB=scf.array(2, atom), potB=scf.array(4, atom))
    return s


def same_bits(s, t):
    for k in s:
        if k in ("fin", "energies"):
            if s[k] != t[k]:
                return False
        elif k == "E":
            if not all(np.array_equal(a.view(np.int64), b.view(np.int64)) for a, b in zip(s[k], t[k])):
                return False
        elif not np.array_equal(s[k].view(np.int64), t[k].view(np.int64)):
            return False
    return True


def density_envelope(ref, pot, levels, E):
    """the change of Sum f Psi^2 / (4 pi r^2) when every eigenvalue moves by +-2e-12 Ha, as a running maximum over +-8 nodes"""
    env = np.zeros(ref.N)
    for (n, l, f), e in zip(levels, E):
        p0 = ref.orbital(pot, l, e) ** 2
        d = np.maximum(np.abs(ref.orbital(pot, l, e + 2e-12) ** 2 - p0), np.abs(ref.orbital(pot, l, e - 2e-12) ** 2 - p0))
        env += f * d
    env[1:] /= SR.FOURPI * ref.pos[1:] * ref.pos[1:]
    env[0] = env[-1] = 0.0
    return R.running_max(env)


def replay(ref, pre, post, label):
    """every stage of the GPU step pre -> post against the reference, each from the GPU's own input to it"""
    lsda, Z, N = ref.lsda, ref.Z, ref.N
    out = {}
    # 1. eigenvalues from V_k, 2. the new density from rho_k and V_k
    Eel = 0.0
    for sp in range(2 if lsda else 1):
        pot = pre["potB" if sp else "potA"]
        levels = ref.cfg[sp]
        E, acc, _, conv = ref.solve_levels(pot, levels)
        got = post["E"][sp]
        gate = 1e-8 + 1e-10 * np.abs(E)
        assert got.shape == E.shape and conv
        if len(E):
            out["eig"] = max(out.get("eig", 0.0), float(np.max(np.abs(got - E) / gate)))
        assert np.all(np.abs(got - E) <= gate), (label, sp, got, E)
        for (_, _, f), e in zip(levels, got):
            Eel += f * e
        key = ("dB" if sp else "dA") if lsda else "rho"
        want = ref.mix(pre[key], acc)
        bound = 2.0 * (density_envelope(ref, pot, levels, E) + 4.0 * EPS * np.abs(want))
        err = np.abs(post[key] - want)
        live = bound > 0
        assert np.all(err[~live] == 0.0), (label, key)
        if live.any():
            out["rho"] = max(out.get("rho", 0.0), float(np.max(err[live] / bound[live])))
        assert np.all(err <= bound), (label, key, out["rho"], int(np.argmax(err / np.where(live, bound, 1.0))))
    if lsda:
        assert np.array_equal(post["rho"][1:], post["dA"][1:] + post["dB"][1:])
    # 3. U from the GPU's new density and the electron count
    U = ref.poisson(post["rho"], ref.Ne)
    out["U"] = float(np.max(np.abs(post["U"] - U)) / (1e-10 * Z))
    assert np.max(np.abs(post["U"] - U)) <= 1e-10 * Z, (label, out["U"])
    assert post["U"][-1] == ref.Ne
    # 4. v_xc, recovered from the GPU's V, against the extended reference on the GPU's density
    r = ref.pos
    dens = (post["dA"], post["dB"]) if lsda else (post["rho"],)
    if ref.functional == SR.VWN:
        Vexc, va, vb, eexc = ref.xc(post["rho"], post.get("dA"), post.get("dB"))
        f64 = (Vexc, va, vb, eexc)
    else:
        ext, T = R.radial(ref.functional, r, ref.cnst_xc, *(x.astype(LD) for x in dens), scale=True)
        f64 = R.radial(ref.functional, r, ref.cnst_xc, *dens)
        idx = (1, 2) if lsda else (0,)
        u = np.zeros(N)
        u[1:] = (-Z + post["U"][1:]) / r[1:]
        for sp, i in enumerate(idx):
            V = post["potB" if sp else "potA"]
            v = V.astype(LD) - u.astype(LD)
            bound = 8.0 * R.running_max(np.abs(f64[i] - ext[i])) + 1e-11 * T[i] + 2.0 * EPS * np.abs(V)
            err = np.abs(v - ext[i])
            dead = (post["rho"] < 1e-18)
            dead[0] = True
            assert np.all(np.isfinite(V))
            assert np.all(np.abs(V[dead] - u[dead]) <= 2.0 * EPS * np.abs(V[dead])), (label, sp)     # the kernel wrote zeros there
            live = ~dead
            out["vxc"] = max(out.get("vxc", 0.0), float(np.max(err[live] / bound[live])))
            assert np.all(err[live] <= bound[live]), (label, sp, out["vxc"], int(np.argmax(np.where(live, err / np.where(bound > 0, bound, 1), 0))))
        Vexc, eexc = f64[0], f64[-1]
    # 5. the energies from the GPU's arrays, eigenvalues and the configuration's occupations
    en = ref.energies(post["rho"], post.get("dA"), post.get("dB"), post["U"], Vexc, eexc, post["potA"], post.get("potB"), Eel)
    out["energies"] = max(abs(a - b) / abs(b) for a, b in zip(post["energies"], en)) / 1e-9
    assert np.allclose(post["energies"], en, rtol=1e-9, atol=0), (label, post["energies"], en)
    print("%-50s ratios to the gates: %s" % (label, "  ".join("%s %.1e" % kv for kv in out.items())))
    return out


REPLAY = [
    ("PBE LDA Ar", 18, False, None),
    ("PBE LSDA N", 7, True, None),
    ("PBE LDA Ar 3p5.5", 18, False, "[Ne] 3s2 3p5.5"),
]


def steps_to_finish(ctx, grid, Z, lsda, config, cap=300):
    scf, ref = make(ctx, grid, Z, lsda, D.XC_PBE, config)
    ref.close()
    scf.step(want_stats=False)
    n = 1
    while not scf.energies()[1][0]:
        assert n < cap
        scf.step(want_stats=False)
        n += 1
    scf.close()
    return n


@pytest.mark.parametrize("case", REPLAY, ids=[c[0].replace(" ", "_") for c in REPLAY])
def test_replay_late_and_finishing_step(ctx, grid, case):
    name, Z, lsda, config = case
    nfin = steps_to_finish(ctx, grid, Z, lsda, config)
    assert nfin > 22, nfin
    scf, ref = make(ctx, grid, Z, lsda, D.XC_PBE, config)
    try:
        for _ in range(20):
            scf.step(want_stats=False)
        assert_config(scf, 0, ref)
        pre = snap(scf, 0, lsda)
        scf.step(want_stats=False)
        post = snap(scf, 0, lsda)
        assert not post["fin"]
        replay(ref, pre, post, "%s step 21" % name)
        for _ in range(nfin - 22):
            scf.step(want_stats=False)
        pre = snap(scf, 0, lsda)
        assert not pre["fin"]
        scf.step(want_stats=False)
        post = snap(scf, 0, lsda)
        assert post["fin"], "the run is deterministic: it finishes on the step the scout run finished on"
        replay(ref, pre, post, "%s finishing step %d" % (name, nfin))
        scf.step(want_stats=False)                      # a finished atom is frozen
        assert same_bits(post, snap(scf, 0, lsda))
    finally:
        scf.close()
        ref.close()


BATCHES = [
    ("He Ar Ar3p5.5 Ar+", [2, 18, 18, 18], ["1s2", "[Ar]", "[Ne] 3s2 3p5.5", "[Ne] 3s2 3p5"]),
    ("Fe He Na", [26, 2, 11], ["[Ar] 3d6 4s2", "1s2", "[Ne] 3s1"]),
]


@pytest.mark.parametrize("case", BATCHES, ids=[c[0].replace(" ", "_") for c in BATCHES])
def test_replay_in_batch_with_frozen_atoms(ctx, grid, case):
    """batches under PBE whose atoms finish on different steps (Ar+ on step 32, He on 34, Ar and Ar 3p5.5 on 35; Fe on 25, He on
    34, Na on 43): from the step after it has finished a frozen atom keeps every bit of rho, U, V, energies and eigenvalues from
    step to step (the fin return of k_pbe_radial, k_mix's freeze) while the live atoms still pass the replay -- on every
    atom's finishing step and on the first and the fifth step after the first freeze"""
    name, Z, texts = case
    cfgs = [D.parse_config(z, t, False) for z, t in zip(Z, texts)]
    scf = D.Scf(ctx, grid, Z, functional=D.XC_PBE, config=cfgs)
    refs = [SR.ScfRef(z, SR.config_levels(c, False)[0], None, functional=SR.PBE, mg_levels=GRID[0], delta=GRID[1], MaxR=GRID[2])
            for z, c in zip(Z, cfgs)]
    A = range(len(Z))
    try:
        scf.step(want_stats=False)
        n = 1
        for a, ref in enumerate(refs):
            assert_config(scf, a, ref)
        post = [snap(scf, a, False) for a in A]
        since, beside_frozen, frozen_steps = 0, 0, 0
        while not all(p["fin"] for p in post):
            assert n < 300
            pre = post
            scf.step(want_stats=False)
            n += 1
            post = [snap(scf, a, False) for a in A]
            nfrozen = sum(p["fin"] for p in pre)
            since += 1 if nfrozen else 0
            for a in A:
                if pre[a]["fin"]:
                    assert same_bits(pre[a], post[a]), (texts[a], n)
                    frozen_steps += 1
                elif post[a]["fin"] or since in (1, 5):
                    replay(refs[a], pre[a], post[a], "batch %s: %s step %d%s, %d frozen"
                           % (name, texts[a], n, " (finishing)" if post[a]["fin"] else "", nfrozen))
                    beside_frozen += 1 if nfrozen else 0
        assert beside_frozen >= 3 and frozen_steps >= 3, (beside_frozen, frozen_steps)
        pre = post
        scf.step(want_stats=False)
        assert all(same_bits(pre[a], snap(scf, a, False)) for a in A)
    finally:
        scf.close()
        for ref in refs:
            ref.close()
