"""GPU suite (-m gpu): the Slater integrals R^k(ab,cd), the F^k / G^k tables and the Hartree / exact-exchange energies of orbitals --
dftatom_amd/csrc/slater.hip (k_slater_rk), include/dftatom_hip.h has the definitions, tests/_slater_ref.py the longdouble reference.

a. analytic   The direct entry on hydrogen-like orbitals of Z = 10 (1s 2s 2p 3d 4f 4s) at 8193 nodes (N - 2 = 8191, a prime: no multiple
              of a tile or of 3), logarithmic and uniform: the ten closed forms and F6(4f,4f), G5(3d,4f), R1(2p3d,3d4f).  Against the
              reference on the same float64 input: c eps mag (c = _slater_ref.rk_roundings(N), counted from the kernel's shape; mag the
              formula on |P| with the increments' coefficients positive).  Against the closed forms: 2 x the reference's own
              distance (_slater_ref.MEASURED) + that bound.
b. shapes     Uniform grids of 9, 17, 33, 1025 and 2049 nodes with made-up smooth orbitals, k = 0 and k = 8: one short tile; the last
              node as the FIRST node of a tile (its stencil reaches three nodes back across the boundary -- so it is on every grid of
              1025 nodes or more: the library's grids have 2^L + 1 nodes, L >= 3, which is why sizes such as 5 or 1026 .. 1029 cannot
              be built through the ABI and are not here).  4097 nodes with orbitals cut to zero at, one before and one after a tile
              boundary.  An all-zero orbital gives exactly 0.
c. bits       R^k(ab,cd) == R^k(cb,ad) == R^k(ad,cb) == R^k(ba,dc); a job alone == the job among 300 others at any position == a
              repeated call; slater_fg symmetric; F^k(a,a) of the table == the direct job.
d. SCF        Ne LDA, N LSDA, the batch [H, Ne, Fe] after three steps at 4097 nodes: every entry of slater_fg within the bound of the
              reference on the exported orbitals; cross-spin F^0 through Scf.slater_rk; coulomb_exchange == the header's host sums over
              these values in float64 NumPy, bit for bit; one electron: E_x = -E_H, 1s2: E_x = -E_H / 2; a frozen atom keeps its table.
e. Hartree    E_H from F^0 against 2 pi Q[r rho U s] with U from dfta_poisson_solve on the density rebuilt from the orbitals, Ne at 4097
              and 16 385 nodes: gate 2 x the gap measured on the CPU between the reference and the oracle's multigrid
              (_slater_ref.MEASURED["hartree"]: the discretisation of a second-order solver, not rounding).
f. front end  dftatom_cli --slater-table; the error paths.

Every test prints the largest ratio to its bound that it observed.
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import _orb_ref as O                     # noqa: E402
import _slater_ref as S                  # noqa: E402
import dftatom_amd as D                  # noqa: E402

LD, EPS = S.LD, S.EPS
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
    extra = {"uni3": (3, None, 10.0), "uni4": (4, None, 10.0), "uni5": (5, None, 10.0), "uni10": (10, None, 10.0), "uni11": (11, None, 10.0)}

    def get(name):
        if name not in made:
            L, d, Rm = O.GRIDS.get(name) or extra[name]
            g = D.Grid(ctx, L, d, Rm)
            made[name] = (g, g.r(), O.grid(L, d, Rm)[1])
        return made[name]
    yield get
    for g, _, _ in made.values():
        g.close()


def _ref(u, job, r, s):
    a, b, c, d, k = (int(x) for x in job)
    return S.rk(u[a], u[b], u[c], u[d], k, r, s)


def _check(R, u, jobs, r, s, what):
    """every result within rk_roundings(N) eps mag of the reference on the same u (exactly 0 where mag is 0); returns the largest ratio"""
    c = S.rk_roundings(len(r))
    worst = 0.0
    for j, job in enumerate(jobs):
        ref, mag = _ref(u, job, r, s)
        bound = c * EPS * float(mag)
        err = abs(float(LD(R[j]) - ref))
        if bound == 0:
            assert R[j] == 0, (what, job)
            continue
        worst = max(worst, err / bound)
        assert err <= bound, (what, tuple(job), R[j], float(ref), err / bound)
    return worst


# ---- a. the direct entry on analytic orbitals -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["log13", "uni13"])
def test_direct_entry_on_analytic_orbitals(ctx, grids, name):
    grid, r, s = grids(name)
    N = grid.N
    assert (N - 2) % 3 and (N - 2) % S.TILE
    u = S.orbitals(np.asarray(r, dtype=LD)).astype(np.float64)
    jobs = [job for _, job, _ in S.CLOSED] + [job for _, job in S.EXTRA]
    R = D.slater_rk(ctx, grid, u, jobs)
    ms = ctx.last_kernel_ms()
    assert ms > 0
    wr = _check(R, u, jobs, r, s, name)
    c = S.rk_roundings(N)
    wc = 0.0
    for j, (nm, job, cf) in enumerate(S.CLOSED):
        closed = LD(S.ZREF) * LD(cf.numerator) / LD(cf.denominator)
        _, mag = _ref(u, job, r, s)
        gate = 2 * S.MEASURED[name][nm] * float(closed) + c * EPS * float(mag)
        err = abs(float(LD(R[j]) - closed))
        wc = max(wc, err / gate)
        assert err <= gate, (name, nm, R[j], float(closed), err / gate)
    print("%s: rounding %.3f of the bound, closed forms %.3f of the gate; launch of %d jobs %.4f ms" % (name, wr, wc, len(jobs), ms))


# ---- b. small and awkward shapes ------------------------------------------------------------------------------------------------------
def _smooth(r):
    """four made-up smooth orbitals on [0, 10], one with a node, float64 (4, N)"""
    r = np.asarray(r, dtype=np.float64)
    return np.array([r * np.exp(-r), r * r * np.exp(-0.7 * r), r * (1 - 0.4 * r) * np.exp(-0.5 * r), r ** 3 * np.exp(-r)])


@pytest.mark.parametrize("name", ["uni3", "uni4", "uni5", "uni10", "uni11"])
def test_small_grids_and_the_last_node_on_a_tile_boundary(ctx, grids, name):
    grid, r, s = grids(name)
    N = grid.N
    assert N == {"uni3": 9, "uni4": 17, "uni5": 33, "uni10": 1025, "uni11": 2049}[name]
    u = np.vstack([_smooth(r), np.zeros((1, N))])
    jobs = [(0, 0, 0, 0, 0), (0, 1, 0, 1, 0), (0, 1, 1, 0, 8), (2, 3, 2, 3, 8), (0, 1, 2, 3, 1), (2, 2, 2, 2, 8), (3, 2, 1, 0, 4),
            (4, 0, 4, 0, 0), (0, 4, 1, 2, 3), (4, 4, 4, 4, 8)]
    R = D.slater_rk(ctx, grid, u, jobs)
    assert np.all(R[7:] == 0.0) and not np.any(np.signbit(R[7:]))           # an all-zero orbital: exactly 0
    assert np.all(np.isfinite(R)) and np.all(R[:7] != 0)
    w = _check(R, u, jobs, r, s, name)
    print("%s (%d nodes): %.3f of the bound" % (name, N, w))


def test_orbitals_cut_at_tile_boundaries(ctx, grids):
    grid, r, s = grids("log12")
    base = S.orbitals(np.asarray(r, dtype=LD)).astype(np.float64)
    rows = [base[S.S1], base[S.P2]]
    for cut in (1023, 1024, 1025, 2047, 2048, 2049):
        v = base[S.D3].copy()
        v[cut:] = 0
        rows.append(v)
    u = np.array(rows)
    jobs = []
    for q in range(2, 8):
        jobs += [(q, q, q, q, 0), (q, q, q, q, 4), (1, q, q, 1, 1), (1, q, 1, q, 2), (0, q, q, 0, 2), (q, 7 if q < 7 else 2, 1, 0, 8)]
    R = D.slater_rk(ctx, grid, u, jobs)
    w = _check(R, u, jobs, r, s, "cuts")
    print("orbitals cut at 1023 .. 2049 of 4097 nodes: %.3f of the bound" % w)


# ---- c. symmetry and independence, bit for bit ----------------------------------------------------------------------------------------
def test_symmetry_and_independence_bit_for_bit(ctx, grids):
    grid, r, s = grids("log12")
    u = S.orbitals(np.asarray(r, dtype=LD)).astype(np.float64)
    rng = np.random.default_rng(7)
    quads = [(S.P2, S.D3, S.D3, S.F4, 1), (S.S1, S.S2, S.P2, S.S4, 3), (S.F4, S.S1, S.D3, S.P2, 8), (S.S2, S.S2, S.S4, S.S1, 0)]
    for a, b, c, d, k in quads:
        R = D.slater_rk(ctx, grid, u, [(a, b, c, d, k), (c, b, a, d, k), (a, d, c, b, k), (b, a, d, c, k), (d, c, b, a, k), (c, d, a, b, k)])
        assert np.all(R == R[0]) and R[0] != 0, (a, b, c, d, k, R)
    job = (S.P2, S.D3, S.D3, S.F4, 1)
    alone = D.slater_rk(ctx, grid, u, [job])[0]
    others = np.column_stack([rng.integers(0, 6, size=(300, 4)), rng.integers(0, S.KMAX + 1, size=300)]).astype(np.int32)
    base = D.slater_rk(ctx, grid, u, others)
    for pos in (0, 1, 150, 299, 300):
        table = np.insert(others, pos, job, axis=0)
        R = D.slater_rk(ctx, grid, u, table)
        assert R[pos] == alone and np.array_equal(np.delete(R, pos), base), pos
    assert np.array_equal(D.slater_rk(ctx, grid, u, others), base)
    # the same job twice in one table, and among more orbitals (the indices shift, the bits stay)
    u2 = np.vstack([np.ones((2, grid.N)), u])
    shifted = tuple(x + 2 for x in job[:4]) + (job[4],)
    R = D.slater_rk(ctx, grid, u2, [shifted, (0, 1, 0, 1, 0), shifted])
    assert R[0] == alone and R[2] == alone


# ---- d. the orbitals of the SCF -------------------------------------------------------------------------------------------------------
def _atom_tables(scf, a, lsda):
    """what the SCF entries return for atom a: (l, occ, nA, U, F0 (norb, norb), G (KMAX + 1, norb, norb), the per-channel (F, G))"""
    chans = [0, 1] if lsda else [0]
    lv = [scf.levels(a, sp) for sp in chans]
    U = np.vstack([scf.orbitals(a, sp) for sp in chans])
    l = [int(x) for v in lv for x in v["l"]]
    occ = [float(x) for v in lv for x in v["occupation"]]
    nA, norb = len(lv[0]["l"]), len(l)
    F0 = np.zeros((norb, norb))
    G = np.zeros((S.KMAX + 1, norb, norb))
    per = []
    off = 0
    for sp in chans:
        F, Gc = scf.slater_fg(a, sp)
        n = F.shape[1]
        F0[off:off + n, off:off + n] = F[0]
        G[:, off:off + n, off:off + n] = Gc
        per.append((F, Gc, off, n))
        off += n
    if lsda and norb > nA > 0:                       # the cross-spin F^0: jobs over the atom's orbitals, alpha then beta
        jobs = [(i, j, i, j, 0) for i in range(nA) for j in range(nA, norb)]
        R = scf.slater_rk(a, jobs)
        for (i, j, _, _, _), v in zip(jobs, R):
            F0[i, j] = F0[j, i] = v
    return l, occ, nA, U, F0, G, per


def _check_atom(scf, a, lsda, r, s, what):
    """slater_fg and the cross-spin F^0 against the reference on the exported orbitals; coulomb_exchange against the host sums"""
    l, occ, nA, U, F0, G, per = _atom_tables(scf, a, lsda)
    norb = len(l)
    c = S.rk_roundings(len(r))
    worst = 0.0
    F0ref, Gref, F0mag, Gmag = S.tables(U, l, r, s, nA=nA)
    for F, Gc, off, n in per:
        lc = l[off:off + n]
        assert np.array_equal(F, F.transpose(0, 2, 1)) and np.array_equal(Gc, Gc.transpose(0, 2, 1)), what
        jobs, kinds = D.slater_fg_jobs(lc)
        have = {(int(kind), int(j[0]), int(j[1]), int(j[4])) for j, kind in zip(jobs, kinds)}
        for k in range(S.KMAX + 1):
            for x in range(n):
                for y in range(x, n):
                    if (D.SLATER_F, x, y, k) in have:
                        ref, mag = S.rk(U[off + x], U[off + y], U[off + x], U[off + y], k, r, s)
                        ratio = abs(float(LD(F[k, x, y]) - ref)) / (c * EPS * float(mag))
                        worst = max(worst, ratio)
                        assert ratio <= 1, (what, "F", k, x, y, ratio)
                    else:
                        assert F[k, x, y] == 0, (what, "F", k, x, y)
                    if x == y:
                        assert Gc[k, x, x] == F[k, x, x]
                    elif (D.SLATER_G, x, y, k) in have:
                        ratio = abs(float(LD(Gc[k, x, y]) - Gref[k, off + x, off + y])) / (c * EPS * float(Gmag[k, off + x, off + y]))
                        worst = max(worst, ratio)
                        assert ratio <= 1, (what, "G", k, x, y, ratio)
                    else:
                        assert Gc[k, x, y] == 0, (what, "G", k, x, y)
    ratio = np.abs(F0.astype(LD) - F0ref) / (c * EPS * F0mag)                  # the cross-spin block included
    assert np.all(ratio <= 1), (what, float(np.max(ratio)))
    worst = max(worst, float(np.max(ratio)))
    # the energies: the header's sums over these very values, bit for bit
    eh, ex = scf.coulomb_exchange(a)
    eh_np, ex_np = S.energy_sums(l, occ, nA, lsda, F0, G, dtype=np.float64)
    assert eh == float(eh_np) and ex == float(ex_np), (what, eh, float(eh_np), ex, float(ex_np))
    # ... and within the rounding bound of the reference's sums: the integrals' bound, one rounding per add and product of the sums
    eh_ref, ex_ref = S.energy_sums(l, occ, nA, lsda, F0ref, Gref, dtype=LD)
    mh, mx = S.energy_mags(l, occ, nA, lsda, F0mag, Gmag)
    cs = c + norb * norb * (S.KMAX // 2 + 4)
    assert abs(LD(eh) - eh_ref) <= cs * EPS * mh and abs(LD(ex) - ex_ref) <= cs * EPS * mx, what
    assert eh > 0 and ex < 0 and -ex < eh
    return worst, eh, ex


@pytest.mark.parametrize("Z,lsda", [([10], False), ([7], True), ([1, 10, 26], False)])
def test_tables_and_energies_of_scf_orbitals(ctx, grids, Z, lsda):
    grid, r, s = grids("log12")
    scf = D.Scf(ctx, grid, Z, lsda=lsda, alpha=ALPHA)
    try:
        for _ in range(3):
            scf.step()
        out = [_check_atom(scf, a, lsda, r, s, (Z, lsda, a)) for a in range(len(Z))]
        again = [scf.coulomb_exchange(a) for a in range(len(Z))]
        # F^k(a,a) of the table == the direct job on the exported orbitals
        a = len(Z) - 1
        F, _ = scf.slater_fg(a, 0)
        U = scf.orbitals(a, 0)
        lv = scf.levels(a, 0)["l"]
        q = int(np.argmax(lv))
        ks = list(range(0, 2 * int(lv[q]) + 1, 2))
        direct = D.slater_rk(ctx, grid, U, [(q, q, q, q, k) for k in ks])
        assert np.array_equal(direct, F[ks, q, q]) and np.array_equal(scf.slater_rk(a, [(q, q, q, q, k) for k in ks]), direct)
    finally:
        scf.close()
    assert [(eh, ex) for _, eh, ex in out] == again
    print("Z = %s %s: tables %.3f of the bound; E_H, E_x = %s" % (Z, "LSDA" if lsda else "LDA", max(w for w, _, _ in out),
                                                                   ["%.6f %.6f" % (eh, ex) for _, eh, ex in out]))


@pytest.mark.parametrize("Z,lsda,factor", [(1, True, 1.0), (2, False, 0.5)])
def test_one_electron_and_closed_1s_shell(ctx, grids, Z, lsda, factor):
    """H (LSDA, one electron): E_x = -E_H, no self-interaction; He (LDA, 1s2): E_x = -E_H / 2 -- within the rounding bound of the sums"""
    grid, r, s = grids("log12")
    scf = D.Scf(ctx, grid, [Z], lsda=lsda, alpha=ALPHA)
    try:
        for _ in range(3):
            scf.step()
        eh, ex = scf.coulomb_exchange(0)
        u = scf.orbitals(0, 0)
    finally:
        scf.close()
    _, mag = S.rk(u[0], u[0], u[0], u[0], 0, r, s)
    occ = 1.0 if lsda else 2.0
    bound = (S.rk_roundings(grid.N) + 8) * EPS * float(mag) * occ * occ
    print("Z = %d: E_H %.12f E_x %.12f, |E_x + %.1f E_H| = %.3e (bound %.3e)" % (Z, eh, ex, factor, abs(ex + factor * eh), bound))
    assert eh > 0 and abs(ex + factor * eh) <= bound


def test_frozen_atoms_keep_their_tables(ctx, grids):
    """the batch of test_gpu_orbitals.test_frozen_atoms_keep_their_orbitals: H and Ar freeze in step 33 while Cu is live"""
    grid, _, _ = grids("log12")
    scf = D.Scf(ctx, grid, [1, 18, 29], alpha=ALPHA)
    try:
        for _ in range(80):
            scf.step(want_stats=False)
            fin = scf.energies()[1]
            if fin[0] and fin[1]:
                break
        assert fin[0] and fin[1] and not fin[2], "the premise: hydrogen and argon finish while copper is live"
        t1 = [scf.slater_fg(a, 0) + scf.coulomb_exchange(a) for a in range(3)]
        for _ in range(5):
            scf.step(want_stats=False)
        assert not scf.energies()[1][2]
        t2 = [scf.slater_fg(a, 0) + scf.coulomb_exchange(a) for a in range(3)]
    finally:
        scf.close()
    for a in (0, 1):
        assert all(np.array_equal(x, y) for x, y in zip(t1[a], t2[a])), a
    assert not np.array_equal(t1[2][0], t2[2][0]) and t1[2][2:] != t2[2][2:]


# ---- e. the Hartree energy against the multigrid ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [12, 14])
def test_hartree_energy_against_the_multigrid(ctx, grids, L):
    grid, r, s = grids("log%d" % L)
    assert O.GRIDS["log%d" % L] == S.HARTREE_GRIDS[L]
    N = grid.N
    scf = D.Scf(ctx, grid, [10], alpha=ALPHA)
    try:
        for _ in range(3):
            scf.step()
        u = scf.orbitals(0, 0)
        occ = scf.levels(0, 0)["occupation"]
        eh, _ = scf.coulomb_exchange(0)
    finally:
        scf.close()
    acc = np.zeros(N)                                       # the step's output density before the mix, as k_accumulate_density forms it
    for k in range(len(occ)):
        acc[:N - 1] += (occ[k] * u[k, :N - 1]) * u[k, :N - 1]
    rho = np.zeros(N)
    rho[1:] = acc[1:] / (4 * np.pi * r[1:] * r[1:])
    ps = D.Poisson(ctx, grid, 1)
    try:
        UH = ps.solve([10], rho)[0][0]
    finally:
        ps.close()
    e2 = 2 * np.pi * float(np.sum(O.weights(N).astype(np.float64) * (r * rho * UH * s.astype(np.float64))))
    gap, gate = abs(e2 - eh) / eh, 2 * S.MEASURED["hartree"][L]
    print("%d nodes: E_H from F0 %.10f, from the multigrid %.10f, gap %.3e (gate %.1e)" % (N, eh, e2, gap, gate))
    assert gap <= gate


# ---- f. the front end and the error paths -----------------------------------------------------------------------------------------------
def test_cli_slater_table(ctx, grids):
    """dftatom_cli --slater-table: after Finished!, one line per F^k / G^k whose figures are those of Scf.slater_fg at six decimals, then
    E_H and E_x; without the flag the output is byte for byte what it is with the table taken out"""
    import os
    import subprocess
    exe = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "dftatom_amd", "compat", "dftatom_cli")
    args = [exe, "10", "12", "0.5", "25", "0.002", "0"]
    plain = subprocess.run(args, capture_output=True, text=True, timeout=120)
    table = subprocess.run(args + ["--slater-table"], capture_output=True, text=True, timeout=120)
    assert plain.returncode == 0 and table.returncode == 0, (plain.stderr, table.stderr)
    lines = table.stdout.split("\n")
    rows = [k for k, ln in enumerate(lines) if ln.startswith("Slater ")]
    assert len(rows) == 10 and rows == list(range(rows[0], rows[0] + 10)) and lines[rows[0] - 2] == "Finished!"
    assert lines[rows[-1] + 1].startswith("EHartree = ") and lines[rows[-1] + 2] == ""
    assert "\n".join(lines[:rows[0]] + lines[rows[-1] + 3:]) == plain.stdout and "Slater" not in plain.stdout and "EHartree" not in plain.stdout
    grid, _, _ = grids("log12")
    scf = D.Scf(ctx, grid, [10], alpha=ALPHA)
    try:
        for _ in range(100):
            scf.step(want_stats=False)
            if scf.energies()[1][0]:
                break
        F, G = scf.slater_fg(0, 0)
        eh, ex = scf.coulomb_exchange(0)
        lv = scf.levels(0, 0)
    finally:
        scf.close()
    jobs, kinds = D.slater_fg_jobs(lv["l"])
    name = lambda q: "%d%s" % (lv["n"][q] + 1, "spdf"[lv["l"][q]])               # noqa: E731
    for row, (a, b, _, _, k), kind in zip(rows, jobs, kinds):
        want = "Slater %s%d(%s,%s) = %.6f" % ("G" if kind else "F", k, name(a), name(b), (G if kind else F)[k, a, b])
        assert lines[row] == want, (lines[row], want)
    assert lines[rows[-1] + 1] == "EHartree = %.6f EXX = %.6f" % (eh, ex)
    assert lines[rows[0]].startswith("Slater F0(1s,1s) = ") and lines[rows[-1]].startswith("Slater G1(2s,2p) = ")


def test_error_paths(ctx, grids):
    grid, r, _ = grids("log12")
    lib, N = ctx.lib, grid.N
    ip, dp = D.c_ip, D.c_dp
    last = lambda: lib.dfta_last_error(ctx.h).decode()                           # noqa: E731
    u = np.full((3, N), 0.5)
    out = np.full(4 * 9 * 9, 7.0)
    po, pu = out.ctypes.data_as(dp), u.ctypes.data_as(dp)
    one = np.array([[0, 1, 2, 0, 2]], np.int32)
    scf = D.Scf(ctx, grid, [10], alpha=ALPHA)
    try:
        # before the first step
        assert lib.dfta_scf_slater_rk(scf.h, 0, 1, one.ctypes.data_as(ip), po) == 1 and "step" in last()
        assert lib.dfta_scf_slater_fg(scf.h, 0, 0, po, po) == 1 and "step" in last()
        eh, ex = C.c_double(7.0), C.c_double(7.0)
        assert lib.dfta_scf_coulomb_exchange(scf.h, 0, C.byref(eh), C.byref(ex)) == 1 and "step" in last()
        with pytest.raises(D.DftaError):
            scf.slater_fg()
        scf.step()
        # orbital index out of range, k outside 0 .. 8 -- on the SCF's orbitals and on the caller's
        for bad in ((3, 0, 0, 0, 0), (0, -1, 0, 0, 0), (0, 0, 3, 0, 0), (0, 0, 0, 7, 0), (0, 0, 0, 0, -1), (0, 0, 0, 0, 9)):
            tab = np.array([one[0], bad], np.int32)
            assert lib.dfta_scf_slater_rk(scf.h, 0, 2, tab.ctypes.data_as(ip), po) == 1 and "Slater job" in last(), bad
            assert lib.dfta_slater_rk(ctx.h, grid.h, 3, pu, 2, tab.ctypes.data_as(ip), po) == 1 and "Slater job" in last(), bad
        for atom, spin in ((-1, 0), (1, 0), (0, 1), (0, -1)):
            assert lib.dfta_scf_slater_fg(scf.h, atom, spin, po, po) == 1 and last(), (atom, spin)
        assert lib.dfta_scf_coulomb_exchange(scf.h, 1, C.byref(eh), C.byref(ex)) == 1
        # null pointers
        assert lib.dfta_slater_rk(ctx.h, grid.h, 3, None, 1, one.ctypes.data_as(ip), po) == 1 and last()
        assert lib.dfta_slater_rk(ctx.h, grid.h, 3, pu, 1, None, po) == 1
        assert lib.dfta_slater_rk(ctx.h, grid.h, 3, pu, 1, one.ctypes.data_as(ip), None) == 1
        assert lib.dfta_slater_rk(None, grid.h, 3, pu, 1, one.ctypes.data_as(ip), po) == 1
        assert lib.dfta_slater_rk(ctx.h, None, 3, pu, 1, one.ctypes.data_as(ip), po) == 1
        assert lib.dfta_slater_rk(ctx.h, grid.h, 3, pu, -1, one.ctypes.data_as(ip), po) == 1
        assert lib.dfta_scf_slater_rk(scf.h, 0, 1, None, po) == 1 and lib.dfta_scf_slater_rk(scf.h, 0, 1, one.ctypes.data_as(ip), None) == 1
        assert lib.dfta_scf_slater_rk(None, 0, 1, one.ctypes.data_as(ip), po) == 1
        assert lib.dfta_scf_slater_fg(scf.h, 0, 0, None, po) == 1 and lib.dfta_scf_slater_fg(scf.h, 0, 0, po, None) == 1
        assert lib.dfta_scf_coulomb_exchange(scf.h, 0, None, C.byref(ex)) == 1 and lib.dfta_scf_coulomb_exchange(scf.h, 0, C.byref(eh), None) == 1
        assert np.all(out == 7.0) and eh.value == 7.0 and ex.value == 7.0
        # njobs = 0: OK, nothing written (even with null tables)
        assert lib.dfta_slater_rk(ctx.h, grid.h, 3, pu, 0, None, None) == 0
        assert lib.dfta_scf_slater_rk(scf.h, 0, 0, None, None) == 0
        assert D.slater_rk(ctx, grid, u, np.zeros((0, 5), np.int32)).shape == (0,)
        assert np.all(out == 7.0)
        assert lib.dfta_scf_slater_rk(scf.h, 0, 1, one.ctypes.data_as(ip), po) == 0 and out[0] != 7.0 and np.all(out[1:] == 7.0)
    finally:
        scf.close()
