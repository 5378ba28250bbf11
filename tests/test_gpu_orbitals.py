"""GPU suite (-m gpu): the orbitals the SCF exports (dfta_scf_get_orbitals), their expectation values (k_orbital_properties) and r^k
matrix elements (k_orbital_matrix) -- dftatom_amd/csrc/orbitals.hip, include/dftatom_hip.h has the definitions.

a. meaning   (The issue's batch for the frozen-atom case, [H, Ar], has no live atom left when H freezes: both meet the stop test in
             step 33 on this grid.  Cu, 60 steps, is added as the live one.)  The exported u and the occupations rebuild the step's density BIT FOR BIT: acc = Sum_levels (occ u) u over i < N-1 in
             level order, nd = acc / (4 pi r r), alpha rho_k + (1 - alpha) nd -- the arithmetic of k_accumulate_density and k_mix in
             float64 numpy -- equals array(0) (LSDA: arrays 1, 2 and their sum) at every node i >= 1.  The orbitals therefore belong to
             the step's INPUT potential.  A frozen atom keeps its orbitals and property rows bit for bit while the batch goes on.
b. rounding  Properties and matrices against tests/_orb_ref.py (longdouble) on the device's own exported u: every entry within
             c eps mag, mag the sum of the magnitudes of the weighted terms, c the counted roundings of the kernels' fixed-shape tree
             (_orb_ref.prop_roundings / matrix_roundings: 43 / 530 at 4097 nodes, 91 / 554 at 16 385).  RPEAK equals r[argmax |u|].
             M == M.T, batch == alone == repeated call, bit for bit.
c. accuracy  The direct entries on analytic hydrogen-like orbitals against the closed forms: gate = 2 x the distance
             tests/test_orb_ref.py measured for the reference on that grid (_orb_ref.MEASURED) + the rounding bound (with
             _orb_ref.INPUT_ROUNDINGS more for the float64 rounding of the input).  8193 nodes: N - 2 = 8191 is a prime, no multiple
             of a tile (1024 / 128 nodes) or of 3; norb = 1 and norb = 19; orbitals cut to zero at, before and after a tile boundary.
d. errors    DFTA_ERR_INVALID before the first step, for a bad atom / spin / k; norb = 0 writes nothing.

Every test prints the largest ratio to its bound that it observed.  On an MI355X: properties 0.035 / 0.019 / 0.026 of the bound (4097 /
16 385 nodes / uniform), |NORM - 1| <= 0.004, matrices 0.016 / 0.006 / 0.008, diagonal against column 0.014; analytic input at 8193
nodes: rounding 0.024, closed forms 0.48 of the gate (the reference's own distance: the gate is twice it), matrices 0.019.
"""

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import _orb_ref as R                     # noqa: E402
import dftatom_amd as D                  # noqa: E402

LD, EPS = R.LD, R.EPS
ALPHA = 0.5


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
            L, d, Rm = R.GRIDS.get(name) or {"uni12": (12, None, 15.0)}[name]
            g = D.Grid(ctx, L, d, Rm)
            made[name] = (g, g.r(), R.grid(L, d, Rm)[1])
        return made[name]
    yield get
    for g, _, _ in made.values():
        g.close()


# ---- a. what the exported orbitals mean ---------------------------------------------------------------------------------------------
def _density_in(scf, a, lsda):
    return [scf.array(w, a) for w in ((1, 2) if lsda else (0,))]


def _check_rebuild(scf, r, natoms, lsda, steps):
    N = len(r)
    fpr2 = 4 * np.pi * r * r                               # (4 pi r) r, as the grid's table
    for step in range(steps):
        before = [_density_in(scf, a, lsda) for a in range(natoms)]
        scf.step()
        for a in range(natoms):
            mixed = []
            for spin in range(2 if lsda else 1):
                u = scf.orbitals(a, spin)
                occ = scf.levels(a, spin)["occupation"]
                assert u.shape == (len(occ), N)
                acc = np.zeros(N)
                for k in range(len(occ)):
                    acc[:N - 1] += (occ[k] * u[k, :N - 1]) * u[k, :N - 1]
                nd = np.zeros(N)
                nd[1:] = acc[1:] / fpr2[1:]
                mixed.append(ALPHA * before[a][spin] + (1 - ALPHA) * nd)
            got = _density_in(scf, a, lsda)
            for spin in range(len(mixed)):
                assert np.array_equal(got[spin][1:], mixed[spin][1:]), (step, a, spin)
            if lsda:
                assert np.array_equal(scf.array(0, a)[1:], (mixed[0] + mixed[1])[1:]), (step, a)


@pytest.mark.parametrize("Z,lsda,sweep_mode", [([10], False, D.SWEEPS_EXACT), ([7], True, D.SWEEPS_EXACT), ([1, 10, 26], False, D.SWEEPS_EXACT),
                                               ([10], False, D.SWEEPS_TOLERANCE)])
def test_exported_orbitals_rebuild_the_density_bit_for_bit(ctx, grids, Z, lsda, sweep_mode):
    grid, r, _ = grids("log12")
    scf = D.Scf(ctx, grid, Z, lsda=lsda, alpha=ALPHA, sweep_mode=sweep_mode)
    try:
        _check_rebuild(scf, r, len(Z), lsda, 3)
    finally:
        scf.close()


def _scf_norm_bound(N):
    """|NORM - 1|: the property kernel's bound on a sum of positive terms, the SCF's own normalisation (Simpson 3/8 by ordered chains
    of at most 2 (N - 2) / 3 adds, the end sum, 1 / sqrt, the scaling, the square: 10) -- in units of eps"""
    return R.prop_roundings(N) + 2 * (N - 2) // 3 + 10


def test_uniform_grid_norm_and_shapes(ctx, grids):
    grid, r, _ = grids("uni12")
    scf = D.Scf(ctx, grid, [10], alpha=ALPHA)
    try:
        scf.step()
        u = scf.orbitals(0, 0)
        props, jobs = scf.orbital_properties()
        M = scf.orbital_matrix(0, 0, 0)
    finally:
        scf.close()
    assert u.shape == (3, grid.N) and props.shape == (3, D.ORB_PROPS) and M.shape == (3, 3)
    assert jobs == [(0, 0, 0, 0), (0, 0, 1, 0), (0, 0, 1, 1)]
    worst = np.max(np.abs(props[:, D.ORB_NORM] - 1)) / (_scf_norm_bound(grid.N) * EPS)
    print("uniform grid: |NORM - 1| / bound = %.3f" % worst)
    assert worst <= 1


def test_frozen_atoms_keep_their_orbitals(ctx, grids):
    """H and Ar in a batch with Cu: on this grid H and Ar meet the stop test in the same step, 33 (the CPU oracle's count; linear mixing
    sets the pace of both), so the atom that is still live while they are frozen is a third one -- Cu needs 60 steps.  Five steps
    beyond: the frozen atoms' orbitals and property rows keep every bit, the live atom's change."""
    grid, _, _ = grids("log12")
    scf = D.Scf(ctx, grid, [1, 18, 29], alpha=ALPHA)
    try:
        for _ in range(80):
            scf.step(want_stats=False)
            fin = scf.energies()[1]
            if fin[0] and fin[1]:
                break
        assert fin[0] and fin[1] and not fin[2], "the premise: hydrogen and argon finish while copper is live"
        u = [scf.orbitals(a, 0) for a in range(3)]
        props, jobs = scf.orbital_properties()
        for _ in range(5):
            scf.step(want_stats=False)
        assert not scf.energies()[1][2]
        u2 = [scf.orbitals(a, 0) for a in range(3)]
        props2 = scf.orbital_properties()[0]
    finally:
        scf.close()
    frozen = np.array([j[0] < 2 for j in jobs])
    assert frozen.sum() == 1 + 5 and (~frozen).sum() == len(u[2])
    for a in (0, 1):
        assert np.array_equal(u[a], u2[a]), a
    assert np.array_equal(props[frozen], props2[frozen])
    assert np.all(np.any(u[2] != u2[2], axis=1))                             # every orbital of the live atom has moved
    assert np.all(np.any(props[~frozen] != props2[~frozen], axis=1))


# ---- b. rounding: the kernels against the longdouble reference on the device's own orbitals -------------------------------------------
def _check_props(props, u, l, r, s, c, what):
    """every column of every row within c eps mag of the reference on the same u; RPEAK exact.  Returns (largest ratio, the mags)."""
    worst, mags = 0.0, []
    for k in range(len(l)):
        ref, mag = R.properties(u[k], int(l[k]), r, s)
        mags.append(mag)
        assert props[k, D.ORB_RPEAK] == r[int(np.argmax(np.abs(u[k])))], (what, k)
        for col in range(D.ORB_PROPS):
            if col == D.ORB_RPEAK:
                continue
            bound = c * EPS * float(mag[col])
            err = abs(float(LD(props[k, col]) - ref[col]))
            if bound == 0:
                assert err == 0, (what, k, col)
                continue
            worst = max(worst, err / bound)
            assert err <= bound, (what, k, R.COLUMNS[col], props[k, col], float(ref[col]), err / bound)
    return worst, mags


def _check_matrix(M, u, k, r, s, c, what):
    ref, mag = R.matrix(u, k, r, s)
    assert np.array_equal(M, M.T), what
    ratio = np.abs(M.astype(LD) - ref) / (c * EPS * mag)
    assert np.all(ratio <= 1), (what, k, float(np.max(ratio)))
    return float(np.max(ratio))


@pytest.mark.parametrize("name", ["log12", "log14", "uni12"])
def test_properties_and_matrices_of_scf_orbitals(ctx, grids, name):
    grid, r, s = grids(name)
    N = grid.N
    cp, cm = R.prop_roundings(N), R.matrix_roundings(N)
    Z = [10] if grid.uniform else [1, 10, 26]           # (the uniform SCF is exercised one atom at a time elsewhere in the suite too)
    last = len(Z) - 1
    scf = D.Scf(ctx, grid, Z, alpha=ALPHA)
    try:
        scf.step()
        scf.step()
        props, jobs = scf.orbital_properties()
        again = scf.orbital_properties()[0]
        U = [scf.orbitals(a, 0) for a in range(len(Z))]
        Ms = {(a, k): scf.orbital_matrix(a, 0, k) for a in range(len(Z)) for k in range(3)}
        Ms_again = scf.orbital_matrix(last, 0, 1)
    finally:
        scf.close()
    assert props.shape == (len(jobs), D.ORB_PROPS) and np.array_equal(props, again) and np.array_equal(Ms[(last, 1)], Ms_again)
    assert [j[0] for j in jobs] == sorted(j[0] for j in jobs) and len(jobs) == sum(len(x) for x in U)
    ls = np.array([j[3] for j in jobs])
    wp, mags = _check_props(props, np.concatenate(U), ls, r, s, cp, name)
    wn = np.max(np.abs(props[:, D.ORB_NORM] - 1)) / (_scf_norm_bound(N) * EPS)
    assert wn <= 1, wn
    wm = wd = 0.0
    off = 0
    for a in range(len(Z)):
        n = len(U[a])
        rows = props[off:off + n]
        for k, col in ((0, D.ORB_NORM), (1, D.ORB_R1), (2, D.ORB_R2)):
            M = Ms[(a, k)]
            wm = max(wm, _check_matrix(M, U[a], k, r, s, cm, (name, a)))
            # the diagonal is the property column: both lie within their bounds of the same exact sum
            for q in range(n):
                d = abs(M[q, q] - rows[q, col]) / ((cp + cm) * EPS * float(mags[off + q][col]))
                wd = max(wd, d)
                assert d <= 1, (name, a, k, q, d)
        # batch = alone: the atom's orbitals through the direct entries, as a batch of their own
        alone = D.orbital_properties(ctx, grid, ls[off:off + n], U[a])
        assert np.array_equal(alone, rows), (name, a)
        assert np.array_equal(D.orbital_matrix(ctx, grid, U[a], 2), Ms[(a, 2)]), (name, a)
        off += n
    print("%s: properties %.3f, |NORM - 1| %.3f, matrices %.3f, diagonal vs column %.3f of the bound" % (name, wp, wn, wm, wd))


# ---- c. accuracy: analytic hydrogen-like orbitals against the closed forms ----------------------------------------------------------
def _analytic_set(r):
    """19 orbitals: the four of the closed-form checks, 1s 2s 2p of Z = 10, three copies of 3p cut to zero at 1023, 1024 and 1025,
    and nine more levels of Z = 10.  Returns (u float64 (19, N), l, the (n, l, Z) of the first seven)."""
    rl = np.asarray(r, dtype=LD)
    spec = list(R.ORBITALS) + list(R.PAIR)
    u = [R.hydrogenic_u(n, l, Z, rl) for n, l, Z in spec]
    ls = [l for _, l, _ in spec]
    for cut in (1023, 1024, 1025):
        v = R.hydrogenic_u(3, 1, 10, rl)
        v[cut:] = 0
        u.append(v)
        ls.append(1)
    for n, l in ((3, 0), (3, 2), (4, 0), (4, 1), (4, 2), (5, 0), (5, 1), (5, 3), (5, 4)):
        u.append(R.hydrogenic_u(n, l, 10, rl))
        ls.append(l)
    assert len(u) == 19
    return np.array(u).astype(np.float64), np.array(ls, np.int32), spec


@pytest.mark.parametrize("name", ["log13", "uni13"])
def test_direct_entries_on_analytic_orbitals(ctx, grids, name):
    grid, r, s = grids(name)
    N = grid.N
    assert (N - 2) % 3 and (N - 2) % R.PROP_TILE and (N - 2) % 128
    cp, cm = R.prop_roundings(N), R.matrix_roundings(N)
    u, ls, spec = _analytic_set(r)
    props = D.orbital_properties(ctx, grid, ls, u)
    ms = ctx.last_kernel_ms()
    assert ms > 0
    # rounding: all 19 against the reference on the same float64 input
    wr, _ = _check_props(props, u, ls, r, s, cp, name)
    # accuracy: the first four against the closed forms
    wa = 0.0
    for k, nlZ in enumerate(R.ORBITALS):
        n, l, Z = nlZ
        _, mag = R.properties(u[k], l, r, s)
        for col, v in R.closed_forms(n, l, Z).items():
            gate = 2 * R.MEASURED[name][nlZ][col] * abs(float(v)) + (cp + R.INPUT_ROUNDINGS) * EPS * float(mag[col])
            err = abs(float(LD(props[k, col]) - v))
            wa = max(wa, err / gate)
            assert err <= gate, (name, nlZ, R.COLUMNS[col], props[k, col], float(v), err / gate)
        if l == 0:
            assert props[k, D.ORB_RM3] == 0.0
    # norb = 1: one orbital alone has the bits it has among nineteen
    for k in (0, 3, 8):
        assert np.array_equal(D.orbital_properties(ctx, grid, ls[k:k + 1], u[k:k + 1])[0], props[k]), k
    # matrices: 19 x 19 against the reference; <1s|2s> and <1s|r|2p> against their closed forms
    wm = 0.0
    M = {}
    for k in range(3):
        M[k] = D.orbital_matrix(ctx, grid, u, k)
        wm = max(wm, _check_matrix(M[k], u, k, r, s, cm, name))
        assert np.array_equal(D.orbital_matrix(ctx, grid, u, k), M[k])
    _, mag0 = R.matrix(u, 0, r, s)
    _, mag1 = R.matrix(u, 1, r, s)
    i1s, i2s, i2p = 4, 5, 6
    ce = (cm + R.INPUT_ROUNDINGS) * EPS
    assert abs(M[0][i1s, i2s]) <= 2 * R.MEASURED[name]["S12"] + ce * float(mag0[i1s, i2s])
    dip = float(R.DIPOLE_1S_2P(10))
    assert abs(M[1][i1s, i2p] - dip) <= 2 * R.MEASURED[name]["D"] * dip + ce * float(mag1[i1s, i2p])
    one = D.orbital_matrix(ctx, grid, u[2:3], 1)
    assert one.shape == (1, 1) and one[0, 0] == M[1][2, 2]
    print("%s: rounding %.3f, closed forms %.3f, matrices %.3f of the gate; property launch of 19 orbitals %.4f ms" % (name, wr, wa, wm, ms))


# ---- the front end ------------------------------------------------------------------------------------------------------------------
def test_cli_orbital_table(ctx, grids):
    """dftatom_cli --orbital-table: after Finished!, one line per level whose figures are those of Scf.orbital_properties() at six
    decimals; without the flag the output is byte for byte what it is with the table taken out"""
    import os
    import re
    import subprocess
    exe = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "dftatom_amd", "compat", "dftatom_cli")
    args = [exe, "10", "12", "0.5", "25", "0.002", "0"]
    plain = subprocess.run(args, capture_output=True, text=True, timeout=120)
    table = subprocess.run(args + ["--orbital-table"], capture_output=True, text=True, timeout=120)
    assert plain.returncode == 0 and table.returncode == 0, (plain.stderr, table.stderr)
    lines = table.stdout.split("\n")
    rows = [k for k, ln in enumerate(lines) if ln.startswith("Orbital ")]
    assert len(rows) == 3 and rows == list(range(rows[0], rows[0] + 3)) and lines[rows[0] - 2] == "Finished!" and lines[rows[-1] + 1] == ""
    assert "\n".join(lines[:rows[0]] + lines[rows[-1] + 2:]) == plain.stdout and "Orbital" not in plain.stdout
    grid, _, _ = grids("log12")
    scf = D.Scf(ctx, grid, [10], alpha=ALPHA)
    try:
        for _ in range(100):
            scf.step(want_stats=False)
            if scf.energies()[1][0]:
                break
        props, jobs = scf.orbital_properties()
        lv = scf.levels(0, 0)
    finally:
        scf.close()
    for k, row in enumerate(rows):
        want = "Orbital %d%s: n = %d l = %d occ = %d E = %.6f <r> = %.6f <r^2> = %.6f T = %.6f r_peak = %.6f" % (
            jobs[k][2] + 1, "spdf"[jobs[k][3]], jobs[k][2] + 1, jobs[k][3], lv["occ"][k], lv["E"][k], props[k, D.ORB_R1], props[k, D.ORB_R2],
            props[k, D.ORB_T], props[k, D.ORB_RPEAK])
        assert lines[row] == want, (lines[row], want)
    assert re.match(r"^Orbital 1s: n = 1 l = 0 occ = 2 E = -", lines[rows[0]])


# ---- d. error paths -----------------------------------------------------------------------------------------------------------------
def test_error_paths(ctx, grids):
    grid, r, _ = grids("log12")
    lib, N = ctx.lib, grid.N
    scf = D.Scf(ctx, grid, [10], alpha=ALPHA)
    try:
        buf = np.full(3 * N, 7.0)
        p = buf.ctypes.data_as(D.c_dp)
        # before the first step
        assert lib.dfta_scf_get_orbitals(scf.h, 0, 0, p) == 1
        assert lib.dfta_scf_orbital_properties(scf.h, p) == 1
        assert lib.dfta_scf_orbital_matrix(scf.h, 0, 0, 0, p) == 1
        assert np.all(buf == 7.0)
        with pytest.raises(D.DftaError):
            scf.orbitals()
        scf.step()
        for atom, spin in ((-1, 0), (1, 0), (0, 1), (0, -1), (0, 2)):
            assert lib.dfta_scf_get_orbitals(scf.h, atom, spin, p) == 1, (atom, spin)
            assert lib.dfta_scf_orbital_matrix(scf.h, atom, spin, 0, p) == 1, (atom, spin)
        for k in (-1, 3):
            assert lib.dfta_scf_orbital_matrix(scf.h, 0, 0, k, p) == 1
            assert lib.dfta_orbital_matrix(ctx.h, grid.h, 3, p, k, p) == 1
        assert np.all(buf == 7.0)
        assert lib.dfta_orbital_matrix(ctx.h, grid.h, 33, p, 0, p) == 1        # more orbitals than a channel can hold
        # norb = 0: OK, nothing written
        l = np.zeros(1, np.int32)
        assert lib.dfta_orbital_properties(ctx.h, grid.h, 0, l.ctypes.data_as(D.c_ip), p, p) == 0
        assert lib.dfta_orbital_matrix(ctx.h, grid.h, 0, p, 0, p) == 0
        assert lib.dfta_orbital_properties(ctx.h, grid.h, -1, l.ctypes.data_as(D.c_ip), p, p) == 1
        assert np.all(buf == 7.0)
        assert lib.dfta_scf_get_orbitals(scf.h, 0, 0, p) == 0 and not np.all(buf == 7.0)
    finally:
        scf.close()
