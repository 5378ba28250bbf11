"""GPU suite (-m gpu): the screening functions y^k_xy = Y^k_xy / r, the exchange operator applied to orbitals, Slater's potential and the
KLI potential -- dftatom_amd/csrc/exchange.hip, include/dftatom_hip.h has the definitions, tests/_exchange_ref.py the longdouble reference
and the counted bounds.

a. analytic   The direct entry on hydrogen-like orbitals of Z = 10 (1s 2s 2p 3d 4f 4s) at 8193 nodes, logarithmic and uniform: every node of
              every row within yk_roundings(N, k) eps mag_i of the reference on the same float64 input (mag: the formula on |P| with the
              stencils' coefficients positive); against the five closed forms 2 x the reference's own distance (_exchange_ref.MEASURED,
              relative to the row's peak) + that bound + the rounding of the orbitals to float64.
b. shapes     Uniform grids of 9, 17, 1025 and 2049 nodes, k = 0 and 8 (at 1025 and 2049 the last node is alone in the last tile: the
              reverse scan starts with a one-node tile); 4097 nodes with orbitals cut to zero at 1023 .. 1025 and 2047 .. 2049; an
              all-zero orbital gives exactly 0; a NaN node poisons the rows of the jobs that read its orbital and no other.
c. bits       y(x,y,k) == y(y,x,k); a job alone == among 200 others at any position == a repeated call; Scf.screening_yk == screening_yk
              on Scf.orbitals(); the batch [H, Ne, Fe] == each atom alone; a frozen atom keeps every bit.
d. orders     From the device's own y rows and u, float64 NumPy in the header's orders reproduces X, D, vS and (with the returned c) vKLI
              bit for bit; M == S n with S symmetric.
e. reductions vbarHF, vbarS, vbarKLI and S_ab n_b within their counted bounds of the longdouble quadratures of the device's own integrands;
              the returned c solves the reduced system on the returned M and vbar to the backward-error bound H (3H + 1) eps ||A|| ||c||;
              Sum n vbarS = Sum n vbarHF and the HOMO row within the bounds propagated from those of the parts.
f. physics    Ne LDA, N LSDA, [H, Ne, Fe] after three steps at 4097 nodes: 1/2 Sum n vbarHF == Scf.coulomb_exchange()'s E_x within the sum
              of the two counted bounds; H: vS == vKLI bit for bit and |vS + y^0| <= 3 eps |y^0|; Sum N y^0_aa r against U of
              dfta_poisson_solve, and r vKLI at the outermost node of the density against -1, each at 2 x the CPU figure.
g. front end  dftatom_cli --exchange-table; the error paths.

Every test prints the largest ratio to its bound that it observed.
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import _exchange_ref as X                # noqa: E402
import _orb_ref as O                     # noqa: E402
import _slater_ref as S                  # noqa: E402
import dftatom_amd as D                  # noqa: E402

LD, EPS = X.LD, X.EPS
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
    extra = {"uni3": (3, None, 10.0), "uni4": (4, None, 10.0), "uni10": (10, None, 10.0), "uni11": (11, None, 10.0)}

    def get(name):
        if name not in made:
            L, d, Rm = O.GRIDS.get(name) or extra[name]
            g = D.Grid(ctx, L, d, Rm)
            made[name] = (g, g.r(), O.grid(L, d, Rm)[1])
        return made[name]
    yield get
    for g, _, _ in made.values():
        g.close()


@pytest.fixture(scope="module")
def atoms(ctx, grids):
    """the three SCF runs of section f after three steps at 4097 nodes, made once: name -> (scf, Z list, lsda)"""
    grid, _, _ = grids("log12")
    made = {}
    for name, Z, lsda in (("Ne", [10], False), ("N", [7], True), ("batch", [1, 10, 26], False), ("H", [1], True)):
        scf = D.Scf(ctx, grid, Z, lsda=lsda, alpha=ALPHA)
        for _ in range(3):
            scf.step(want_stats=False)
        made[name] = (scf, Z, lsda)
    yield made
    for scf, _, _ in made.values():
        scf.close()


def _check_rows(Y, u, jobs, r, s, what):
    """every node of every row within yk_roundings(N, k) eps mag_i of the reference on the same u (exactly 0 where mag_i is 0); returns
    the largest ratio"""
    worst = 0.0
    for j, (x, y, k) in enumerate(jobs):
        ref, mag = X.yk(u[x], u[y], int(k), r, s)
        bound = X.yk_roundings(len(r), int(k)) * EPS * mag
        err = np.abs(Y[j].astype(LD) - ref)
        zero = bound == 0
        assert np.all(Y[j][zero] == 0) and not np.any(np.signbit(Y[j][zero])), (what, (x, y, k))
        assert np.all(np.isfinite(Y[j])), (what, (x, y, k))
        if np.all(zero):
            continue
        ratio = float(np.max(err[~zero] / bound[~zero]))
        worst = max(worst, ratio)
        assert ratio <= 1, (what, (x, y, k), int(np.argmax(np.where(zero, 0, err / np.where(zero, 1, bound)))), ratio)
    return worst


# ---- a. the direct entry on analytic orbitals -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["log13", "uni13"])
def test_rows_of_analytic_orbitals(ctx, grids, name):
    grid, r, s = grids(name)
    N = grid.N
    assert N == 8193 and (N - 2) % 3 and (N - 2) % X.TILE
    u = S.orbitals(np.asarray(r, dtype=LD)).astype(np.float64)
    jobs = [job for _, job, _ in X.CLOSED] + [job for _, job in X.EXTRA]
    Y = D.screening_yk(ctx, grid, u, jobs)
    ms = ctx.last_kernel_ms()
    assert ms > 0 and Y.shape == (len(jobs), N)
    wr = _check_rows(Y, u, jobs, r, s, name)
    wc = 0.0
    for j, (nm, (x, y, k), spec) in enumerate(X.CLOSED):
        closed = X.closed_yk(spec, S.ZREF, r)
        _, mag = X.yk(u[x], u[y], k, r, s)
        gate = 2 * X.MEASURED[name][nm] * np.max(closed) + (X.yk_roundings(N, k) + O.INPUT_ROUNDINGS) * EPS * mag
        ratio = float(np.max(np.abs(Y[j].astype(LD) - closed) / gate))
        wc = max(wc, ratio)
        assert ratio <= 1, (name, nm, ratio)
    print("%s: rounding %.3f of the bound, closed forms %.3f of the gate; launch of %d rows %.4f ms" % (name, wr, wc, len(jobs), ms))


# ---- b. small and awkward shapes ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["uni3", "uni4", "uni10", "uni11"])
def test_small_grids_and_a_one_node_last_tile(ctx, grids, name):
    grid, r, s = grids(name)
    N = grid.N
    assert N == {"uni3": 9, "uni4": 17, "uni10": 1025, "uni11": 2049}[name]
    u = np.vstack([X.smooth_orbitals(r), np.zeros((1, N))])
    jobs = [(0, 0, 0), (0, 1, 0), (0, 1, 8), (2, 3, 8), (2, 2, 8), (3, 1, 0), (2, 3, 0), (4, 0, 0), (4, 4, 8), (1, 4, 8)]
    Y = D.screening_yk(ctx, grid, u, jobs)
    assert not np.any(Y[7:]) and not np.any(np.signbit(Y[7:]))               # an all-zero orbital: exactly 0 everywhere
    assert np.all(Y[:7, 1:] != 0) and np.all(Y[[0, 1, 5, 6], 0] != 0) and not np.any(Y[[2, 3, 4], 0])       # y_0 = W_0 (k = 0), 0 (k > 0)
    w = _check_rows(Y, u, jobs, r, s, name)
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
        jobs += [(q, q, 0), (q, q, 4), (1, q, 1), (q, 0, 2), (q, q, 8), (q, 7 if q < 7 else 2, 0)]
    Y = D.screening_yk(ctx, grid, u, jobs)
    w = _check_rows(Y, u, jobs, r, s, "cuts")
    print("orbitals cut at 1023 .. 2049 of 4097 nodes: %.3f of the bound" % w)


def test_a_nan_node_poisons_only_its_rows(ctx, grids):
    grid, r, _ = grids("log12")
    u = S.orbitals(np.asarray(r, dtype=LD)).astype(np.float64)[:4]
    jobs = [(0, 0, 0), (0, 2, 1), (2, 2, 2), (1, 3, 2), (2, 3, 1), (1, 1, 0), (3, 2, 3)]
    clean = D.screening_yk(ctx, grid, u, jobs)
    bad = u.copy()
    bad[2, 1500] = np.nan
    Y = D.screening_yk(ctx, grid, bad, jobs)
    for j, (x, y, k) in enumerate(jobs):
        if 2 in (x, y):
            assert np.all(np.isnan(Y[j, 1:])) and Y[j, 0] == 0, (x, y, k)          # Z from the node on, W up to it; y_0 = 0 for k > 0
        else:
            assert np.array_equal(Y[j], clean[j]), (x, y, k)


# ---- c. symmetry and independence, bit for bit ----------------------------------------------------------------------------------------
def test_symmetry_and_independence_bit_for_bit(ctx, grids):
    grid, r, _ = grids("log12")
    u = S.orbitals(np.asarray(r, dtype=LD)).astype(np.float64)
    rng = np.random.default_rng(11)
    for x, y, k in ((S.P2, S.D3, 1), (S.S1, S.S4, 0), (S.F4, S.S2, 8)):
        Y = D.screening_yk(ctx, grid, u, [(x, y, k), (y, x, k)])
        assert np.array_equal(Y[0], Y[1]) and np.any(Y[0])
    job = (S.P2, S.D3, 1)
    alone = D.screening_yk(ctx, grid, u, [job])[0]
    others = np.column_stack([rng.integers(0, 6, size=(200, 2)), rng.integers(0, X.KMAX + 1, size=200)]).astype(np.int32)
    base = D.screening_yk(ctx, grid, u, others)
    for pos in (0, 1, 100, 199, 200):
        Y = D.screening_yk(ctx, grid, u, np.insert(others, pos, job, axis=0))
        assert np.array_equal(Y[pos], alone) and np.array_equal(np.delete(Y, pos, axis=0), base), pos
    assert np.array_equal(D.screening_yk(ctx, grid, u, others), base)
    u2 = np.vstack([np.ones((2, grid.N)), u])                                    # more orbitals: the indices shift, the bits stay
    Y = D.screening_yk(ctx, grid, u2, [(job[0] + 2, job[1] + 2, 1), (0, 1, 0), (job[1] + 2, job[0] + 2, 1)])
    assert np.array_equal(Y[0], alone) and np.array_equal(Y[2], alone)


def _channels(lsda):
    return (0, 1) if lsda else (0,)


def _same(p, q):
    return all(np.array_equal(p[key], q[key]) for key in ("X", "D", "vS", "vKLI", "vbar", "M")) and p["homo"] == q["homo"]


def test_scf_entries_read_the_exported_orbitals(ctx, grids, atoms):
    grid, _, _ = grids("log12")
    for name in ("N", "batch"):
        scf, Z, lsda = atoms[name]
        for a in range(len(Z)):
            U = np.vstack([scf.orbitals(a, sp) for sp in _channels(lsda)])
            norb = len(U)
            jobs = [(0, 0, 0), (norb - 1, 0, 1), (norb - 1, norb - 1, 2), (0, norb - 1, 0)]         # across the channels too
            assert np.array_equal(scf.screening_yk(a, jobs), D.screening_yk(ctx, grid, U, jobs)), (name, a)
            for sp in _channels(lsda):
                p = scf.exchange_potentials(a, sp)
                lv = scf.levels(a, sp)
                assert p["homo"] == X.pick_homo(lv["E"], p["occ"])
                q = D.exchange_potentials(ctx, grid, lv["l"], p["occ"], p["homo"], scf.orbitals(a, sp))
                assert _same(p, q), (name, a, sp)
                assert _same(p, scf.exchange_potentials(a, sp))                   # a repeated call


def test_batch_equals_each_atom_alone(ctx, grids, atoms):
    grid, _, _ = grids("log12")
    batch, Z, _ = atoms["batch"]
    for a, z in enumerate(Z):
        alone = atoms["Ne"][0] if z == 10 else D.Scf(ctx, grid, [z], alpha=ALPHA)
        try:
            if z != 10:
                for _ in range(3):
                    alone.step(want_stats=False)
            assert _same(batch.exchange_potentials(a, 0), alone.exchange_potentials(0, 0)), z
            jobs = D.exchange_jobs(batch.levels(a, 0)["l"])
            assert np.array_equal(batch.screening_yk(a, jobs), alone.screening_yk(0, jobs)), z
        finally:
            if z != 10:
                alone.close()


def test_frozen_atoms_keep_their_potentials(ctx, grids):
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
        t1 = [(scf.exchange_potentials(a, 0), scf.screening_yk(a, [(0, 0, 0)])) for a in range(3)]
        for _ in range(5):
            scf.step(want_stats=False)
        assert not scf.energies()[1][2]
        t2 = [(scf.exchange_potentials(a, 0), scf.screening_yk(a, [(0, 0, 0)])) for a in range(3)]
    finally:
        scf.close()
    for a in (0, 1):
        assert _same(t1[a][0], t2[a][0]) and np.array_equal(t1[a][1], t2[a][1]), a
    assert not np.array_equal(t1[2][0]["vKLI"], t2[2][0]["vKLI"]) and not np.array_equal(t1[2][1], t2[2][1])


# ---- d. the header's orders, bit for bit; e. the reductions and the solve -----------------------------------------------------------------
def _rows(ctx, grid, u, l):
    jobs = D.exchange_jobs(l)
    Y = D.screening_yk(ctx, grid, u, jobs)
    return {tuple(int(v) for v in job): Y[j] for j, job in enumerate(jobs)}


def _check_orders_bit_for_bit(p, u, l, occ, Y, what):
    Xr, Dr, _, vS = X.pointwise(u, l, occ, Y, dtype=np.float64)
    assert np.array_equal(Xr, p["X"]) and np.array_equal(Dr, p["D"]) and np.array_equal(vS, p["vS"]), what
    vK = X.kli_potential(u, occ, p["homo"], p["vbar"][:, X.CC], p["D"], p["vS"], dtype=np.float64)
    assert np.array_equal(vK, p["vKLI"]), what
    assert p["vbar"][p["homo"], X.CC] == 0 and not np.any(p["vS"][p["D"] <= 0]) and not np.any(p["vKLI"][p["D"] <= 0])
    n = np.asarray(occ, dtype=np.float64)
    for a in range(len(l)):                           # M_ab = S_ab n_b from one S_ab per pair: M_ab n_a and M_ba n_b are S n_a n_b twice
        for b in range(a + 1, len(l)):
            assert abs(LD(p["M"][a, b]) * LD(n[a]) - LD(p["M"][b, a]) * LD(n[b])) <= 1.01 * EPS * abs(p["M"][a, b] * n[a]), (what, a, b)


def _check_reductions(p, u, l, occ, r, s, what):
    """the quadratures against longdouble on the device's own X, D, vS, vKLI; the solve; the two identities.  Returns the largest ratios"""
    N, n = len(r), len(l)
    nl = np.array([LD(x) for x in occ], dtype=LD)
    red = X.reductions(u, occ, p["X"], p["D"], p["vS"], s, vKLI=p["vKLI"])
    worst = {}
    bnd = {}
    for key, col, kind in (("HF", X.HF, X.HF), ("S", X.SL, X.SL), ("KLI", X.KLI, X.KLI)):
        bnd[key] = X.red_roundings(N, kind) * EPS * red[key][1]
        err = np.abs(p["vbar"][:, col].astype(LD) - red[key][0])
        assert np.all(err <= bnd[key]), (what, key, (err / bnd[key]).astype(np.float64))
        worst[key] = float(np.max(err / bnd[key]))
    bM = (X.red_roundings(N, X.PAIR) + 1) * EPS * red["pair"][1] * nl[None, :]          # + 1: the product S_ab n_b
    err = np.abs(p["M"].astype(LD) - red["M"])
    assert np.all(err <= bM), (what, "M")
    worst["M"] = float(np.max(np.where(bM > 0, err / np.where(bM > 0, bM, 1), 0)))
    # the solve: residual of the reduced system formed in float64 from the returned M and vbar, evaluated in longdouble
    h = p["homo"]
    idx = [a for a in range(n) if a != h]
    H = len(idx)
    c = p["vbar"][:, X.CC].astype(LD)
    res = np.zeros(n, dtype=LD)
    if H:
        A = (np.eye(H) - p["M"][np.ix_(idx, idx)])
        b = p["vbar"][idx, X.SL] - p["vbar"][idx, X.HF]
        res[idx] = A.astype(LD) @ c[idx] - b.astype(LD)
        bound = H * (3 * H + 1) * EPS * np.linalg.norm(A, 2) * float(np.sqrt(np.sum(c * c)))
        worst["solve"] = float(np.sqrt(np.sum(res * res))) / bound
        assert worst["solve"] <= 1, (what, "solve", worst["solve"])
    # Sum n vbarS = Sum n vbarHF.  On the device's integrands, node by node, Sum_a n_a u_a^2 vS = D* vS with D* the exact sum (D holds
    # n + 2 roundings of it: two per term, the chain), vS = -(num / D) (1 rounding), num the device's sum of n_a u_a X_a (n + 2 roundings
    # of its magnitude): the two integrands differ by (2 n + 5) eps Sum_a n_a |u_a X_a|.  Then each side's counted bound.
    magHF = np.sum(nl * red["HF"][1])
    pw = (2 * n + 5) * EPS * magHF
    b_sum = np.sum(nl * (bnd["HF"] + bnd["S"])) + pw
    lhs = np.sum(nl * p["vbar"][:, X.SL].astype(LD)) - np.sum(nl * p["vbar"][:, X.HF].astype(LD))
    worst["sumS"] = float(abs(lhs) / b_sum)
    assert worst["sumS"] <= 1, (what, "Sum n vbarS", worst["sumS"])
    # the HOMO row.  With K, S*, HF*, P_ab the longdouble quadratures of the device's integrands: K_a = S*_a + Sum_b P_ab n_b c_b + dK_a
    # (dK: the n + 5 roundings of vKLI at a node -- three per term of its sum, the chain, the division, the sum with vS -- on
    # Q[u_a^2 (|vS| + Sum_b n_b u_b^2 |c_b| / D) s]).  Summed over a with n_a, Sum_a n_a P_ab = NORM_b (1 + the n + 2 roundings of D); for
    # the kept rows the solve gives S*_a - HF*_a + Sum_b P_ab n_b c_b = c_a up to its residual and the bounds of vbarS_a, vbarHF_a and
    # M_ab; their dK cancel.  What is left:
    #   n_h (K_h - HF*_h) = Sum_{b != h} n_b c_b (NORM_b - 1)  +  [Sum n S* - Sum n HF*: pw above]  +  n_h dK_h  +  those terms,
    # and vbarKLI_h, vbarHF_h are within their own bounds of K_h, HF*_h.
    norm = np.array([X.quad((u[a].astype(LD) * u[a]) * s)[0] for a in range(n)], dtype=LD)
    ca = np.abs(c)
    kmag_h = red["S"][1][h] + np.sum(red["pair"][0][h] * nl * ca)
    b_row = nl[h] * (bnd["KLI"][h] + bnd["HF"][h]) + pw + nl[h] * (n + 5) * EPS * kmag_h + (n + 2) * EPS * np.sum(nl * ca * norm)
    for a in idx:
        b_row = b_row + nl[a] * (abs(res[a]) + bnd["S"][a] + bnd["HF"][a] + np.sum(bM[a] * ca))
    lhs = nl[h] * (LD(p["vbar"][h, X.KLI]) - LD(p["vbar"][h, X.HF])) - sum(nl[b] * c[b] * (norm[b] - 1) for b in idx)
    worst["homo"] = float(abs(lhs) / b_row) if b_row > 0 else 0.0
    assert abs(lhs) <= b_row, (what, "HOMO row", worst["homo"], float(lhs))
    # ... and Sum_b M_ab = NORM_a within the bounds of the row and the roundings of D
    for a in range(n):
        assert abs(np.sum(p["M"][a].astype(LD)) - norm[a]) <= np.sum(bM[a]) + (n + 2) * EPS * norm[a], (what, "row sum", a)
    return worst


def test_orders_and_reductions_on_analytic_orbitals(ctx, grids):
    grid, r, s = grids("log12")
    u = S.orbitals(np.asarray(r, dtype=LD)).astype(np.float64)[:5]
    l = [0, 0, 1, 2, 3]
    worst = {}
    for occ, homo in (([1.0, 1.0, 3.0, 2.5, 0.75], 3), ([1.0] * 5, 4), ([0.5, 0.0, 3.0, 5.0, 7.0], 0)):
        p = D.exchange_potentials(ctx, grid, l, occ, homo, u)
        assert ctx.last_kernel_ms() > 0
        Y = _rows(ctx, grid, u, l)
        _check_orders_bit_for_bit(p, u, l, occ, Y, (occ, homo))
        if occ == [1.0] * 5:
            assert np.array_equal(p["M"], p["M"].T)                              # n = 1: M is S itself, symmetric bit for bit
        for key, v in _check_reductions(p, u, l, occ, r, s, (occ, homo)).items():
            worst[key] = max(worst.get(key, 0.0), v)
    # one shell: an empty system, vKLI = vS bit for bit
    p = D.exchange_potentials(ctx, grid, [1], [2.0], 0, u[2:3])
    assert np.array_equal(p["vKLI"], p["vS"]) and p["vbar"][0, X.CC] == 0 and p["vbar"][0, X.KLI] == p["vbar"][0, X.SL]
    print("analytic channel: ratios to the bounds %s" % {k: round(v, 3) for k, v in worst.items()})


@pytest.mark.parametrize("name", ["Ne", "N", "batch"])
def test_orders_and_reductions_on_scf_orbitals(ctx, grids, atoms, name):
    grid, r, s = grids("log12")
    scf, Z, lsda = atoms[name]
    worst = {}
    for a in range(len(Z)):
        for sp in _channels(lsda):
            p = scf.exchange_potentials(a, sp)
            u, l = scf.orbitals(a, sp), [int(v) for v in scf.levels(a, sp)["l"]]
            jobs = D.exchange_jobs(l)
            off = 0 if sp == 0 else scf.levels(a, 0)["l"].size                    # the atom's orbitals count alpha then beta
            Yd = scf.screening_yk(a, jobs + np.array([off, off, 0], np.int32))
            Y = {tuple(int(v) for v in job): Yd[j] for j, job in enumerate(jobs)}
            _check_orders_bit_for_bit(p, u, l, p["occ"], Y, (name, a, sp))
            for key, v in _check_reductions(p, u, l, p["occ"], r, s, (name, a, sp)).items():
                worst[key] = max(worst.get(key, 0.0), v)
    print("%s: ratios to the bounds %s" % (name, {k: round(v, 3) for k, v in worst.items()}))


# ---- f. physics on the orbitals of the SCF --------------------------------------------------------------------------------------------------
def _atom_exchange(scf, a, lsda, r, s):
    """(1/2 Sum n vbarHF over the channels -- LDA: twice the one channel's --, its counted bound).  The bound: vbarHF_a is within
    red_roundings eps of the quadrature of the device's own u_a X_a; X_a carries, relative to Sum |coef| Ymag |u_b|, the bound of a row
    (yk_roundings at the largest k of the channel), the angular factor and its product with n_b 2, the products y u and coef (..) 2,
    and the chain of its entries.  The sum over the shells is taken here in longdouble."""
    N = len(r)
    total, bound = LD(0), LD(0)
    for sp in _channels(lsda):
        p = scf.exchange_potentials(a, sp)
        if p is None:
            continue
        u, l = scf.orbitals(a, sp), [int(v) for v in scf.levels(a, sp)["l"]]
        occ = p["occ"]
        Ym = {job: X.yk(u[job[0]], u[job[1]], job[2], r, s)[1] for job in X.y_jobs(l)}
        fac = LD(0.5) if lsda else LD(1)
        for q, entries in enumerate(X.x_entries(l)):
            xm = sum(LD(occ[b]) * X.gaunt(l[q], k, l[b], LD) * (Ym[(min(q, b), max(q, b), k)] * np.abs(u[b])) for b, k in entries)
            c = X.red_roundings(N, X.HF) + X.yk_roundings(N, 2 * max(l)) + 4 + len(entries)
            total += fac * LD(occ[q]) * LD(p["vbar"][q, X.HF])
            bound += fac * LD(occ[q]) * c * EPS * X.quad(np.abs(u[q]) * xm * s)[0]
    return total, bound


@pytest.mark.parametrize("name", ["Ne", "N", "batch"])
def test_exchange_energy_from_the_fock_averages(ctx, grids, atoms, name):
    grid, r, s = grids("log12")
    scf, Z, lsda = atoms[name]
    worst = 0.0
    for a in range(len(Z)):
        mine, b1 = _atom_exchange(scf, a, lsda, r, s)
        eh, ex = scf.coulomb_exchange(a)
        lv = [scf.levels(a, sp) for sp in _channels(lsda)]
        U = np.vstack([scf.orbitals(a, sp) for sp in _channels(lsda)])
        l = [int(v) for w in lv for v in w["l"]]
        occ = [float(v) for w in lv for v in w["occupation"]]
        nA, norb = len(lv[0]["l"]), len(l)
        _, _, F0mag, Gmag = S.tables(U, l, r, s, nA=nA)
        _, mx = S.energy_mags(l, occ, nA, lsda, F0mag, Gmag)
        b2 = (S.rk_roundings(grid.N) + norb * norb * (S.KMAX // 2 + 4)) * EPS * mx          # the bound tests/test_gpu_slater.py holds E_x to
        ratio = float(abs(mine - LD(ex)) / (b1 + b2))
        worst = max(worst, ratio)
        print("Z = %d: 1/2 Sum n vbarHF = %.12f, E_x = %.12f, %.3f of the two bounds (%.2e + %.2e)" % (Z[a], float(mine), ex, ratio, float(b1), float(b2)))
        assert ratio <= 1, (name, a, float(mine), ex, ratio)
    assert worst > 0


def test_hydrogen_has_no_self_interaction(ctx, grids, atoms):
    """one electron: X = y^0 u, num = u X, D = u u, vS = -(num / D) -- four roundings of half an eps each -- and an empty KLI system"""
    scf, _, _ = atoms["H"]
    p = scf.exchange_potentials(0, 0)
    assert scf.exchange_potentials(0, 1) is None
    y0 = scf.screening_yk(0, [(0, 0, 0)])[0]
    u = scf.orbitals(0, 0)[0]
    assert np.array_equal(p["vS"], p["vKLI"]) and p["homo"] == 0 and p["vbar"][0, X.CC] == 0
    ok = u * u > 1e-290                               # above the subnormal range, where a product keeps its relative accuracy
    assert np.count_nonzero(ok) > 4000 and np.all(p["D"][ok] > 0)
    ratio = float(np.max(np.abs(p["vS"][ok] + y0[ok]) / (3 * EPS * np.abs(y0[ok]))))
    print("H: |vS + y0| at %.3f of 3 eps |y0|; vbarHF = %.12f" % (ratio, p["vbar"][0, X.HF]))
    both = X.red_roundings(len(u), X.HF) + X.red_roundings(len(u), X.SL) + 3          # the two quadratures of one positive integrand
    assert ratio <= 1 and abs(p["vbar"][0, X.HF] - p["vbar"][0, X.SL]) <= both * EPS * abs(p["vbar"][0, X.HF])


def test_hartree_potential_against_the_multigrid(ctx, grids, atoms):
    grid, r, _ = grids("log12")
    N = grid.N
    scf, _, _ = atoms["Ne"]
    u = scf.orbitals(0, 0)
    occ = scf.levels(0, 0)["occupation"]
    y0 = scf.screening_yk(0, [(a, a, 0) for a in range(len(occ))])
    tot = np.einsum("a,ai->i", occ, y0) * r
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
    gap, gate = float(np.max(np.abs(tot - UH))) / float(np.sum(occ)), 2 * X.MEASURED["hartree"][12]
    print("Ne: max |Sum N y0 r - U| / N_e = %.3e (gate %.1e)" % (gap, gate))
    assert gap <= gate


@pytest.mark.parametrize("case", ["Ne", "N_alpha"])
def test_kli_tail(ctx, grids, atoms, case):
    grid, r, _ = grids("log12")
    scf, _, _ = atoms["Ne" if case == "Ne" else "N"]
    p = scf.exchange_potentials(0, 0)
    i = int(np.nonzero(p["D"] > 0)[0][-1])
    v = r[i] * p["vKLI"][i]
    lv = scf.levels(0, 0)
    assert lv["l"][p["homo"]] == 1 and p["occ"][p["homo"]] == 3.0
    gate = 2 * X.MEASURED["tail"][case]
    print("%s: r vKLI = %.6f at node %d (r = %.3f), |.. + 1| = %.3e (gate %.1e)" % (case, v, i, r[i], abs(v + 1), gate))
    assert abs(v + 1) <= gate


# ---- g. the front end and the error paths -----------------------------------------------------------------------------------------------
def test_cli_exchange_table(ctx, grids):
    """dftatom_cli --exchange-table: after Finished!, one line per shell whose figures are those of Scf.exchange_potentials at six decimals,
    then E_x and the tail value; without the flag the output is byte for byte what it is with the table taken out"""
    import os
    import subprocess
    exe = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "dftatom_amd", "compat", "dftatom_cli")
    args = [exe, "10", "12", "0.5", "25", "0.002", "0"]
    plain = subprocess.run(args, capture_output=True, text=True, timeout=120)
    table = subprocess.run(args + ["--exchange-table"], capture_output=True, text=True, timeout=120)
    assert plain.returncode == 0 and table.returncode == 0, (plain.stderr, table.stderr)
    lines = table.stdout.split("\n")
    rows = [k for k, ln in enumerate(lines) if ln.startswith("Exchange ")]
    assert len(rows) == 3 and rows == list(range(rows[0], rows[0] + 3)) and lines[rows[0] - 2] == "Finished!"
    assert lines[rows[-1] + 1].startswith("EXX = ") and lines[rows[-1] + 2] == ""
    assert "\n".join(lines[:rows[0]] + lines[rows[-1] + 3:]) == plain.stdout and "Exchange" not in plain.stdout and "EXX" not in plain.stdout
    grid, r, _ = grids("log12")
    scf = D.Scf(ctx, grid, [10], alpha=ALPHA)
    try:
        for _ in range(100):
            scf.step(want_stats=False)
            if scf.energies()[1][0]:
                break
        p = scf.exchange_potentials(0, 0)
        lv = scf.levels(0, 0)
    finally:
        scf.close()
    ex = 0.0
    for a, row in enumerate(rows):
        v = p["vbar"][a]
        ex += p["occ"][a] * v[X.HF]
        want = "Exchange %d%s: E = %.6f vbarHF = %.6f vbarS = %.6f vbarKLI = %.6f c = %.6f" % (
            lv["n"][a] + 1, "spdf"[lv["l"][a]], lv["E"][a], v[X.HF], v[X.SL], v[X.KLI], v[X.CC])
        assert lines[row] == want, (lines[row], want)
    i = int(np.nonzero(p["D"] > 0)[0][-1])
    assert lines[rows[-1] + 1] == "EXX = %.6f r*vKLI = %.6f" % (ex, r[i] * p["vKLI"][i])


def test_error_paths(ctx, grids):
    grid, r, _ = grids("log12")
    lib, N = ctx.lib, grid.N
    ip, dp = D.c_ip, D.c_dp
    last = lambda: lib.dfta_last_error(ctx.h).decode()                           # noqa: E731
    u = np.full((3, N), 0.5)
    out = np.full(3 * N, 7.0)
    po, pu = out.ctypes.data_as(dp), u.ctypes.data_as(dp)
    one = np.array([[0, 2, 1]], np.int32)
    l3, occ3 = np.array([0, 0, 1], np.int32), np.array([1.0, 1.0, 3.0])
    pl, pocc = l3.ctypes.data_as(ip), occ3.ctypes.data_as(dp)
    homo = C.c_int(7)
    scf = D.Scf(ctx, grid, [10], alpha=ALPHA)
    try:
        # before the first step
        assert lib.dfta_scf_screening_yk(scf.h, 0, 1, one.ctypes.data_as(ip), po) == 1 and "step" in last()
        assert lib.dfta_scf_exchange_potentials(scf.h, 0, 0, po, None, None, None, None, None, C.byref(homo)) == 1 and "step" in last()
        with pytest.raises(D.DftaError):
            scf.exchange_potentials()
        scf.step()
        # orbital index out of range, k outside 0 .. 8 -- on the SCF's orbitals and on the caller's
        for bad in ((3, 0, 0), (0, -1, 0), (0, 3, 0), (0, 0, -1), (0, 0, 9)):
            tab = np.array([one[0], bad], np.int32)
            assert lib.dfta_scf_screening_yk(scf.h, 0, 2, tab.ctypes.data_as(ip), po) == 1 and "screening job" in last(), bad
            assert lib.dfta_screening_yk(ctx.h, grid.h, 3, pu, 2, tab.ctypes.data_as(ip), po) == 1 and "screening job" in last(), bad
        for atom, spin in ((-1, 0), (1, 0), (0, 1), (0, -1)):                     # LDA: spin 0 only
            assert lib.dfta_scf_exchange_potentials(scf.h, atom, spin, po, None, None, None, None, None, None) == 1 and last(), (atom, spin)
        assert lib.dfta_scf_screening_yk(scf.h, 1, 1, one.ctypes.data_as(ip), po) == 1
        # homo out of range, norb, l, a negative occupation
        for h in (-1, 3):
            assert lib.dfta_exchange_potentials(ctx.h, grid.h, 3, pl, pocc, h, pu, po, None, None, None, None, None) == 1 and "homo" in last()
        assert lib.dfta_exchange_potentials(ctx.h, grid.h, 0, pl, pocc, 0, pu, po, None, None, None, None, None) == 1 and "norb" in last()
        assert lib.dfta_exchange_potentials(ctx.h, grid.h, 33, pl, pocc, 0, pu, po, None, None, None, None, None) == 1
        lbad, obad = np.array([0, 5, 1], np.int32), np.array([1.0, -1.0, 3.0])
        assert lib.dfta_exchange_potentials(ctx.h, grid.h, 3, lbad.ctypes.data_as(ip), pocc, 0, pu, po, None, None, None, None, None) == 1
        assert lib.dfta_exchange_potentials(ctx.h, grid.h, 3, pl, obad.ctypes.data_as(dp), 0, pu, po, None, None, None, None, None) == 1
        # null pointers
        assert lib.dfta_screening_yk(ctx.h, grid.h, 3, None, 1, one.ctypes.data_as(ip), po) == 1 and last()
        assert lib.dfta_screening_yk(ctx.h, grid.h, 3, pu, 1, None, po) == 1
        assert lib.dfta_screening_yk(ctx.h, grid.h, 3, pu, 1, one.ctypes.data_as(ip), None) == 1
        assert lib.dfta_screening_yk(None, grid.h, 3, pu, 1, one.ctypes.data_as(ip), po) == 1
        assert lib.dfta_screening_yk(ctx.h, None, 3, pu, 1, one.ctypes.data_as(ip), po) == 1
        assert lib.dfta_screening_yk(ctx.h, grid.h, 3, pu, -1, one.ctypes.data_as(ip), po) == 1
        assert lib.dfta_scf_screening_yk(scf.h, 0, 1, None, po) == 1 and lib.dfta_scf_screening_yk(scf.h, 0, 1, one.ctypes.data_as(ip), None) == 1
        assert lib.dfta_scf_screening_yk(None, 0, 1, one.ctypes.data_as(ip), po) == 1
        assert lib.dfta_exchange_potentials(ctx.h, grid.h, 3, None, pocc, 0, pu, po, None, None, None, None, None) == 1
        assert lib.dfta_exchange_potentials(ctx.h, grid.h, 3, pl, None, 0, pu, po, None, None, None, None, None) == 1
        assert lib.dfta_exchange_potentials(ctx.h, grid.h, 3, pl, pocc, 0, None, po, None, None, None, None, None) == 1
        assert lib.dfta_exchange_potentials(None, grid.h, 3, pl, pocc, 0, pu, po, None, None, None, None, None) == 1
        assert lib.dfta_scf_exchange_potentials(None, 0, 0, po, None, None, None, None, None, None) == 1
        assert np.all(out == 7.0) and homo.value == 7
        # njobs = 0: OK, nothing written (even with null tables); every output NULL: OK
        assert lib.dfta_screening_yk(ctx.h, grid.h, 3, pu, 0, None, None) == 0
        assert lib.dfta_scf_screening_yk(scf.h, 0, 0, None, None) == 0
        assert D.screening_yk(ctx, grid, u, np.zeros((0, 3), np.int32)).shape == (0, N)
        assert lib.dfta_exchange_potentials(ctx.h, grid.h, 3, pl, pocc, 2, pu, None, None, None, None, None, None) == 0
        assert lib.dfta_scf_exchange_potentials(scf.h, 0, 0, None, None, None, None, None, None, C.byref(homo)) == 0
        lv = scf.levels(0, 0)
        assert homo.value == X.pick_homo(lv["E"], lv["occupation"]) and lv["l"][homo.value] == 1
        assert np.all(out == 7.0)
        assert lib.dfta_scf_screening_yk(scf.h, 0, 1, one.ctypes.data_as(ip), po) == 0 and np.all(out[:N] != 7.0) and np.all(out[N:] == 7.0)
    finally:
        scf.close()
