"""GPU suite (-m gpu): cations and user-set, fractional electron configurations (Scf(config=...), Scf(charge=...),
dfta_scf_create_config).

The nuclear charge Z stays in the potential and the energies; the electron count N_e sets the flat start density and the multigrid's
outer boundary U(Rmax) = N_e.  A neutral Aufbau configuration given explicitly must run bit for bit as the default path; a cation
must carry N_e electrons and see the Coulomb tail -(Z - N_e)/r; fractional occupations must obey Janak's theorem dE/dn_i = eps_i.
The oracle (tests/_ion_ref.py) takes integer occupations; fractional ones are held step by step to tests/_scf_ref.py, which solves
every level with the oracle and weights it in NumPy, in test_gpu_scf_ref.py.
"""
import os
import re
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import _ion_ref as IR                    # noqa: E402
import dftatom_amd as D                  # noqa: E402

COMPAT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "dftatom_amd", "compat")

FOURPI = 4.0 * np.pi
HARTREE_EV = 27.211386245988


@pytest.fixture(scope="module")
def ctx(torch_first):
    c = D.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def grid14(ctx):
    g = D.Grid(ctx, 14, 5e-4, 25.0)
    yield g
    g.close()


@pytest.fixture(scope="module")
def grid17(ctx):
    g = D.Grid(ctx, 17, 1e-4, 50.0)
    yield g
    g.close()


def _aufbau_text(Z):
    return " ".join("%d%s%d" % (n + 1, "spdf"[l], o) for n, l, o in D.ion_config(Z, 0)["alpha"])


def _snapshot(scf):
    """every result of the last step: energies, finished flags, eigenvalues and occupations, rho and U of every atom"""
    en, fin = scf.energies()
    out = {"E": np.array([[getattr(e, f) for f, _ in D.Energies._fields_] for e in en]), "fin": fin}
    for a in range(scf.natoms):
        for sp in range(2 if scf.lsda else 1):
            lv = scf.levels(a, sp)
            out["lev%d_%d" % (a, sp)] = np.concatenate([lv["E"], lv["occupation"], lv["n"], lv["l"]])
        out["rho%d" % a] = scf.array(0, a)
        out["U%d" % a] = scf.array(5, a)
        out["V%d" % a] = scf.array(3, a)
    return out


def _same_bits(x, y):
    assert x.keys() == y.keys()
    for k in x:
        assert np.array_equal(np.asarray(x[k]).view(np.uint8), np.asarray(y[k]).view(np.uint8)), k


def _run(scf, steps):
    snaps = []
    for _ in range(steps):
        scf.step()
        snaps.append(_snapshot(scf))
    return snaps


def _converge(scf, cap=400):
    for _ in range(cap):
        scf.step(want_stats=False)
        if scf.energies()[1].all():
            return scf.energies()[0]
    raise AssertionError("not converged in %d steps" % cap)


# ---- 1. charge 0 / the Aufbau text is the default path, bit for bit --------------------------------------------------------------------
CASES = [("Ar LDA", [18], False, "grid14"), ("Ar LSDA", [18], True, "grid14"), ("N LSDA", [7], True, "grid14"),
         ("Z 1..24 LDA", list(range(1, 25)), False, "grid14"), ("Ne LDA uniform", [10], False, "ugrid")]


@pytest.mark.parametrize("nopersist", [False, True])
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_neutral_configuration_is_the_default_path(ctx, grid14, case, nopersist, monkeypatch):
    name, Z, lsda, gname = case
    if nopersist:
        monkeypatch.setenv("DFTA_DEBUG", "LEVELS_NOPERSIST")
    g = grid14 if gname == "grid14" else D.Grid(ctx, 14, None, 25.0)
    try:
        ref = D.Scf(ctx, g, Z, lsda=lsda)
        want = _run(ref, 5)
        ref.close()
        for kw in ({"config": [_aufbau_text(z) for z in Z]}, {"charge": 0}):
            s = D.Scf(ctx, g, Z, lsda=lsda, **kw)
            got = _run(s, 5)
            s.close()
            for a, b in zip(want, got):
                _same_bits(a, b)
    finally:
        if g is not grid14:
            g.close()


# ---- 3. boundary and charge --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lsda", [False, True])
@pytest.mark.parametrize("kw, ne", [({"charge": 1}, 17.0), ({"config": "[Ne] 3s2 3p5.5"}, 17.5)], ids=["Ar+", "Ar 3p5.5"])
def test_boundary_value_and_electron_count(ctx, grid17, kw, ne, lsda):
    s = D.Scf(ctx, grid17, [18], lsda=lsda, **kw)
    for _ in range(40):
        s.step(want_stats=False)
    r = grid17.r()
    U, rho, V = s.array(5), s.array(0), s.array(3)
    assert U[-1] == ne                                                  # U(Rmax) = N_e exactly (the Dirichlet value)
    lv = s.levels(0, 0)
    assert abs(lv["occupation"].sum() + (s.levels(0, 1)["occupation"].sum() if lsda else 0) - ne) < 1e-12
    # 4 pi int rho r^2 dr on the logarithmic grid (dr = Rp delta exp(i delta) di), Simpson 3/8 over the index
    Rp, delta = grid17.Rp, 1e-4
    f = FOURPI * rho * r * r * Rp * delta * np.exp(np.arange(grid17.N) * delta)
    n = grid17.N - 1
    w = np.ones(n + 1)
    w[1:n] = np.where(np.arange(1, n) % 3 == 0, 2.0, 3.0)
    q = 3.0 / 8.0 * np.dot(w, f)
    assert abs(q - ne) <= 1e-9 * ne, (q, ne)
    # A loose sanity check of the Coulomb tail, not the 1e-6 gate: r V(r) -> -(Z - N_e) far out (Rmax = 50 bohr) up to r v_xc of the
    # density there.  Linear mixing keeps 0.5^steps of the flat start density at every node the orbitals do not reach (~3e-17 after 40
    # steps: r v_xc ~ 3e-3), so r V cannot meet 1e-6 at any node; the boundary itself is pinned exactly by U[-1] == N_e above.  v_xc of
    # that density is bounded by twice its Slater exchange (3 rho / pi)^(1/3).
    xc_bound = 2.0 * r[-2] * (3.0 * rho[-2] / np.pi) ** (1.0 / 3.0)
    assert abs(r[-2] * V[-2] + (18 - ne)) < 1e-6 + xc_bound, (r[-2] * V[-2], xc_bound)
    assert xc_bound < 5e-3                                               # far below the charge offsets tested (0.5, 1)
    s.close()


def test_fractional_occupation_getters(ctx, grid14):
    s = D.Scf(ctx, grid14, [18], config="[Ne] 3s2 3p5.5")
    s.step()
    lv = s.levels(0, 0)
    assert lv["occ"] is None and list(lv["occupation"]) == [2, 2, 6, 2, 5.5]
    assert list(lv["n"]) == [0, 1, 1, 2, 2] and list(lv["l"]) == [0, 0, 1, 0, 1]
    s.close()
    with pytest.raises(D.DftaError):
        D.Scf(ctx, grid14, [9], config="[Ne]")                          # anion
    with pytest.raises(ValueError):
        D.Scf(ctx, grid14, [18], config="[Ar]", charge=0)


# ---- 4. Janak's theorem and Slater's transition state -----------------------------------------------------------------------------
@pytest.mark.parametrize("functional", [D.XC_VWN, D.XC_PBE], ids=["VWN", "PBE"])
def test_janak_theorem_ar_3p(ctx, grid17, functional):
    h = 0.01
    cfg = ["[Ne] 3s2 3p%.2f" % (5.5 + h), "[Ne] 3s2 3p%.2f" % (5.5 - h), "[Ne] 3s2 3p5.5"]
    s = D.Scf(ctx, grid17, [18, 18, 18], config=cfg, functional=functional)
    en = _converge(s)
    dE = (en[0].Etotal - en[1].Etotal) / (2 * h)
    eps = s.levels(2, 0)["E"][-1]
    assert abs(dE - eps) < 2e-5, (dE, eps)
    s.close()
    if functional == D.XC_VWN:                                          # Slater: E(Ar+) - E(Ar) ~ -eps_3p(3p^5.5)
        t = D.Scf(ctx, grid17, [18, 18], charge=[0, 1])
        e2 = _converge(t)
        ie = e2[1].Etotal - e2[0].Etotal
        assert abs(ie + eps) < 5e-3, (ie, -eps)
        t.close()


# ---- 5. batches: neutral atoms and cations mixed, each atom as when run alone ----------------------------------------------------
def _final(scf, cap=400):
    _converge(scf, cap)
    return _snapshot(scf)


@pytest.mark.parametrize("nopersist", [False, True])
def test_mixed_batch_equals_atoms_alone(ctx, grid14, nopersist, monkeypatch):
    """Z = 1..24 neutral and Z = 2..25 singly charged in ONE batch of 48, run until every atom has finished (finished atoms are frozen,
    the live atoms go to the smaller multigrid classes, down to the resident 15- and 7-atom groups): each atom ends with the bits it
    ends with alone"""
    if nopersist:
        monkeypatch.setenv("DFTA_DEBUG", "LEVELS_NOPERSIST")
    Z = list(range(1, 25)) + list(range(2, 26))
    q = [0] * 24 + [1] * 24
    b = D.Scf(ctx, grid14, Z, charge=q)
    layouts, groups = [], []
    for _ in range(400):
        st = b.step()
        layouts.append(st.levels_layout)
        groups.append(st.poisson_groups)
        if b.energies()[1].all():
            break
    assert b.energies()[1].all()
    batch = _snapshot(b)
    b.close()
    print("levels layouts", sorted(set(layouts)), "poisson groups per atom", sorted(set(groups)))
    # the paths the batch went through: the device-side search (layout 5) or only host rounds, and the multigrid classes of the live
    # atoms down to the resident group of <= 7 atoms (33 workgroups per atom)
    assert (5 in layouts) == (not nopersist), layouts
    assert 33 in groups and len(set(groups)) >= 3, groups
    for a in (1, 6, 17, 23, 24, 29, 40, 47):                            # He, N, Ar, Cr and He+, N+, Ar+, Mn+
        s = D.Scf(ctx, grid14, [Z[a]], charge=[q[a]])
        alone = _final(s)
        s.close()
        for key in ("rho", "U", "V"):
            assert np.array_equal(batch["%s%d" % (key, a)], alone["%s0" % key]), (a, key)
        assert np.array_equal(batch["E"][a], alone["E"][0]), a
        assert np.array_equal(batch["lev%d_0" % a], alone["lev0_0"]), a


@pytest.mark.parametrize("mode", ["sweeps", "poisson"])
def test_lsda_open_shell_cations_tolerance_modes(ctx, grid14, mode):
    """both tolerance modes run cations within the SCF gate of the multigrid's tolerance mode against the exact path after two steps:
    energies 1e-9 relative, eigenvalues 1e-8 Ha + 2e-9 |E|.  (The scan sweeps' own gate, 2e-11 |E| + 1e-11 Ha, is per level solve on a
    fixed potential; after a step the differences have passed through the density and the Poisson solve, so the SCF gate applies.)"""
    Z = [5, 7, 8, 13, 15, 17, 26]
    q = [0, 1, 1, 0, 1, 1, 2]
    kw = {"sweep_mode": D.SWEEPS_TOLERANCE} if mode == "sweeps" else {"poisson_mode": D.POISSON_TOLERANCE}
    ex = D.Scf(ctx, grid14, Z, lsda=True, charge=q)
    tol = D.Scf(ctx, grid14, Z, lsda=True, charge=q, **kw)
    for _ in range(2):
        ex.step(want_stats=False)
        tol.step(want_stats=False)
    e1, e2 = ex.energies()[0], tol.energies()[0]
    for a in range(len(Z)):
        for f in ("Etotal", "Ekinetic", "Ecoul", "Enuclear", "Exc"):
            x, y = getattr(e1[a], f), getattr(e2[a], f)
            assert abs(x - y) <= 1e-9 * abs(x), (a, f, x, y)
        for sp in (0, 1):
            x, y = ex.levels(a, sp)["E"], tol.levels(a, sp)["E"]
            assert np.all(np.abs(x - y) <= 1e-8 + 2e-9 * np.abs(x)), (a, sp, x, y)
    ex.close()
    tol.close()


# ---- 2. cations against the oracle (tests/_ion_ref.py: dfo_scf_step restated with Z and N_e apart, clamped un-chained brackets) -----
ORACLE_IONS = [("Na+ LDA", 11, 1, False), ("Ar+ LSDA", 18, 1, True), ("Fe2+ LSDA", 26, 2, True), ("Li+ LDA", 3, 1, False)]


@pytest.mark.parametrize("case", ORACLE_IONS, ids=[c[0] for c in ORACLE_IONS])
def test_cation_first_steps_vs_oracle(ctx, case):
    """the gates of test_open_shell_lsda_vs_oracle: eigenvalues 1e-8 Ha + 1e-10 |E|, the five energies rtol 1e-9, steps 1 and 2"""
    _, Z, q, lsda = case
    L, d, R = 14, 5e-4, 25.0
    grid = D.Grid(ctx, L, d, R)
    scf = D.Scf(ctx, grid, [Z], lsda=lsda, charge=[q], levels_mode=D.LEVELS_BATCHED)
    a, b = IR.ion_levels(Z, q, lsda)
    ref = IR.IonScf(Z, a, b, mg_levels=L, MaxR=R, delta=d, chained=3)
    assert ref.Ne == Z - q
    try:
        for _ in range(2):
            scf.step()
            want_e = ref.step()
            en, _ = scf.energies()
            got = np.concatenate([scf.levels(0, sp)["E"] for sp in range(2 if lsda else 1)])
            want = np.concatenate([ref.levels(sp) for sp in range(2 if lsda else 1)])
            assert got.shape == want.shape
            assert np.all(np.abs(got - want) <= 1e-8 + 1e-10 * np.abs(want)), (got, want)
            assert np.allclose(en[0].as_list(), want_e, rtol=1e-9, atol=0), (en[0].as_list(), want_e)
    finally:
        ref.close()
        scf.close()
        grid.close()


# ---- 7. the reference-shaped front end -------------------------------------------------------------------------------------------
def _cli(*args, timeout=900):
    exe = os.path.join(COMPAT, "dftatom_cli")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-C", COMPAT])
    return subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=timeout)


def test_cli_charge_and_config():
    r = _cli(18, 14, 0.5, 25, 0.0005, 1, "--charge=1")
    assert r.returncode == 0, r.stderr[-2000:]
    out = r.stdout
    assert out.startswith("Computing atom with Z=18 using LSDA with non-uniform grid") and "Step: 0" in out and "Finished!" in out
    assert re.search(r"Energy 3p: -?\d+\.\d{6} Num nodes: 1", out)
    assert re.search(r"Etotal = -?\d+\.\d{6} Ekin = ", out)
    tail = out[out.rindex("Finished!"):]
    assert "Alpha: " in tail and "3p3" in tail.split("Beta: ")[0] and "3p2" in tail.split("Beta: ")[1], tail
    f = _cli(18, 14, 0.5, 25, 0.0005, 0, "--config=[Ne] 3s2 3p5.5")
    assert f.returncode == 0 and "Finished!" in f.stdout, f.stderr[-2000:]
    assert "3p5.5 " in f.stdout[f.stdout.rindex("Finished!"):]
    bad = _cli(18, 14, 0.5, 25, 0.0005, 0, "--config=[Ne] 3s2 3p7")
    assert bad.returncode == 2 and "occupation 7" in bad.stderr


# ---- 6. physical sanity: LSDA Delta-SCF first ionization energies within 1 eV of experiment -----------------------------------------
IE_EXP = {3: 5.392, 11: 5.139, 19: 4.341, 10: 21.565, 18: 15.760, 36: 14.000}


def test_first_ionization_energies_lsda(ctx, grid17):
    Z = sorted(IE_EXP)
    s = D.Scf(ctx, grid17, Z + Z, lsda=True, charge=[0] * len(Z) + [1] * len(Z))
    en = _converge(s, cap=600)
    s.close()
    got = {z: (en[len(Z) + k].Etotal - en[k].Etotal) * HARTREE_EV for k, z in enumerate(Z)}
    print("Delta-SCF LSDA first ionization energies (eV):", {z: round(v, 3) for z, v in got.items()})
    for z in Z:
        assert abs(got[z] - IE_EXP[z]) < 1.0, (z, got[z], IE_EXP[z])
