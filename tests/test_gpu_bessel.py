"""GPU suite (-m gpu): spherical Bessel functions and the Bessel transforms -- dftatom_amd/csrc/bessel.hip (k_sph_bessel,
k_bessel_transform), include/dftatom_hip.h has the definitions, tests/_bessel_ref.py the longdouble reference and the counted bounds.

a. j_l         dfta_sph_bessel against the longdouble j_l on the ladder 1e-8 .. 1e4 and at 0, -0, 1e-300 and the doubles on both sides of
               the switch x = 3: gate c eps T_l(x) + 2^-1022 (_bessel_ref.jl_bound: c counted from the kernel, 2 ulp for the device's sin
               and cos), exact at x == 0.
b. transform   dfta_bessel_transform against the longdouble transform on the device's own float64 inputs (f, Grid.r(), q; s in
               longdouble with the three roundings of its table counted): gate eps Sum_i |g_i| (c |j| + c_j T_l + |x j_l'|)
               (_bessel_ref.transform).  Uniform grids of 9, 1025 and 2049 nodes (one short pass, one node beyond a tile of 1024, two
               tiles) and log12; both kinds; l = 0 .. 4 in one call; nq = 1, 7, 8, 9, 17; q with 0, 1e-300, values that put x = 3 inside
               a tile, and 200.  Rows cut to zero at 1023, 1024, 1025 of 2049 nodes, an all-zero row (exactly 0), a NaN node (only that
               row is NaN).  The library's grids have 2^L + 1 nodes: a grid of 1027 nodes cannot be built through the ABI (as
               tests/test_gpu_slater.py notes for its shapes); a last pass of few lanes is what 9 and 1025 nodes and the cut rows give.
c. closed      log13 and uni13, analytic Z = 10 orbitals: form factors of 1s, 2s, 2p and the momentum orbitals 1s, 2s, 2p, 3d, 4f at
               q = 0.5, 3, 20, 60: gate 2 x the reference's stored distance (_bessel_ref.MEASURED) + the rounding bound (x (1 + 1 / c):
               the rounding of the analytic row to float64).
d. bits        a q alone == among 16 others at any position == a repeated call; a row alone == inside a batch of 19 rows;
               BESSEL_QBLOCK = 1, 2, 4, 8 == the planner's choice; Scf.form_factors == bessel_transform on Scf.array(0 / 1 / 2) and
               Scf.momentum_orbitals == bessel_transform on Scf.orbitals() for Ne LDA, N LSDA and the batch [1, 10, 26] after three
               steps on log12; frozen atoms keep every bit while a live atom moves on.
e. physics     f(0) within the rounding bound of Q[4 pi rho r^2 s] and within 1e-9 relative of the electron count (Ne, Ar 3p5.5,
               Fe2+); LSDA: f[rho] within the sum of the bounds of f[rho_a] + f[rho_b]; H LSDA converged against the exact 1s form
               factor at the CPU reference run's distance.
f. front end   dftatom_cli --form-factor-table; the error paths.

Every test prints the largest ratio to its bound that it observed.
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import _bessel_ref as B                  # noqa: E402
import _orb_ref as O                     # noqa: E402
import dftatom_amd as D                  # noqa: E402
from _knobs import knobs                 # noqa: E402

LD, EPS = B.LD, B.EPS
ALPHA = 0.5
# 17 momenta: 0, 1e-300, the switch x = 3 inside the grid (r = 3 / q between 0.1 and 10), 200
Q17 = np.array([0.0, 1e-300, 0.3, 0.5, 1.0, 3.0, 200.0, 0.05, 7.5, 20.0, 60.0, 2.0, 1e-8, 0.75, 12.0, 33.0, 100.0])


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
    extra = {"uni3": (3, None, 10.0), "uni10": (10, None, 10.0), "uni11": (11, None, 10.0)}

    def get(name):
        if name not in made:
            L, d, Rm = O.GRIDS.get(name) or extra[name]
            g = D.Grid(ctx, L, d, Rm)
            made[name] = (g, g.r(), O.grid(L, d, Rm)[1])
        return made[name]
    yield get
    for g, _, _ in made.values():
        g.close()


def _check(out, kind, l, F, r, s, q, what, ref=None):
    """every value within its bound of the reference on the same inputs (exactly 0 where the row is all zero); returns (worst ratio, ref)"""
    V, Bd = ref if ref is not None else B.transform_rows(kind, l, F, r, s, q)
    err = np.abs(out.astype(LD) - V).astype(np.float64)
    ratio = err / Bd
    assert np.all(err <= Bd), (what, float(ratio.max()), np.argwhere(err > Bd)[:4].tolist())
    return float(ratio.max()), (V, Bd)


def _smooth(r):
    """five made-up smooth rows for l = 0 .. 4 on [0, Rmax], one with a node, float64 (5, N)"""
    r = np.asarray(r, dtype=np.float64)
    return np.array([np.exp(-r) * (1 - 0.4 * r), r * np.exp(-0.7 * r), r * r * np.exp(-r), r ** 3 * np.exp(-1.3 * r) * (1 - 0.2 * r),
                     r ** 4 * np.exp(-1.1 * r)])


# ---- a. j_l -----------------------------------------------------------------------------------------------------------------------------
def test_sph_bessel_against_the_reference(ctx):
    x = np.concatenate([[0.0, -0.0, 1e-300], B.ladder()])
    worst = {}
    for l in range(B.LMAX + 1):
        got = D.sph_bessel(ctx, l, x)
        assert ctx.last_kernel_ms() > 0
        ref, _ = B.jl(l, x)
        bound = B.jl_bound(l, x)
        err = np.abs(got.astype(LD) - ref).astype(np.float64)
        assert np.all(got[:2] == (1.0 if l == 0 else 0.0)) and not np.any(np.signbit(got[:2]))
        live = bound > 0
        assert np.all(err[live] <= bound[live]), (l, x[live][np.argmax(err[live] / bound[live])], float((err[live] / bound[live]).max()))
        # the counted bound minus its 2^-1022: what the figure in the README is stated in
        rel = err[3:] / (bound[3:] - B.TINY)
        worst[l] = float(rel.max())
    print("sph_bessel, largest |gpu - ref| / (c eps T_l) per l: %s" % {l: "%.3f" % v for l, v in worst.items()})


# ---- b. the transform against the reference -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", [B.BT_DENSITY, B.BT_ORBITAL])
@pytest.mark.parametrize("name", ["uni3", "uni10", "uni11", "log12"])
def test_transform_on_small_and_awkward_grids(ctx, grids, name, kind):
    grid, r, s = grids(name)
    assert grid.N == {"uni3": 9, "uni10": 1025, "uni11": 2049, "log12": 4097}[name]
    F, l = _smooth(r), np.arange(5)
    ref = None
    worst = 0.0
    for nq in (17, 1, 7, 8, 9):
        out = D.bessel_transform(ctx, grid, kind, l, F, Q17[:nq])
        assert out.shape == (5, nq) and np.all(np.isfinite(out))
        if ref is None:
            w, ref = _check(out, kind, l, F, r, s, Q17, (name, kind, nq))
            full = out
        else:
            w, _ = _check(out, kind, l, F, r, s, Q17[:nq], (name, kind, nq), ref=(ref[0][:, :nq], ref[1][:, :nq]))
            assert np.array_equal(out, full[:, :nq])
        worst = max(worst, w)
    assert np.all(full[1:, 0] == 0) and np.all(full[0, :2] != 0)               # q = 0: only l = 0 survives
    print("%s (%d nodes) kind %d: %.3f of the bound" % (name, grid.N, kind, worst))


def test_cut_rows_zero_row_and_nan_node(ctx, grids):
    grid, r, s = grids("uni11")
    N = grid.N
    base = _smooth(r)[2]
    rows, l = [base], [2]
    for cut in (1023, 1024, 1025):
        v = base.copy()
        v[cut:] = 0
        rows.append(v)
        l.append(2)
    rows.append(np.zeros(N))
    l.append(1)
    bad = _smooth(r)[0].copy()
    bad[1500] = np.nan
    rows.append(bad)
    l.append(0)
    rows.append(_smooth(r)[4])
    l.append(4)
    F = np.array(rows)
    worst = 0.0
    for kind in (B.BT_DENSITY, B.BT_ORBITAL):
        out = D.bessel_transform(ctx, grid, kind, l, F, Q17)
        assert np.all(out[4] == 0.0) and not np.any(np.signbit(out[4]))          # an all-zero row: exactly 0 for every q
        assert np.all(np.isnan(out[5])) and np.all(np.isfinite(np.delete(out, 5, axis=0)))
        keep = [0, 1, 2, 3, 4, 6]
        w, _ = _check(out[keep], kind, [l[k] for k in keep], F[keep], r, s, Q17, ("cuts", kind))
        worst = max(worst, w)
    print("rows cut at 1023 .. 1025 of 2049 nodes, zero row, NaN node: %.3f of the bound" % worst)


# ---- c. closed forms ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["log13", "uni13"])
def test_closed_forms_of_hydrogen_like_orbitals(ctx, grids, name):
    grid, r, s = grids(name)
    rl = np.asarray(r, dtype=LD)
    q = np.array(B.QS)
    # form factors of 1s, 2s, 2p
    Fd = np.array([B.density_row(B.hydrogenic_u(n, l, B.ZREF, rl), rl) for n, l in B.FORM_ORBITALS]).astype(np.float64)
    out = D.bessel_transform(ctx, grid, D.BT_DENSITY, [0] * len(Fd), Fd, q)
    ms = ctx.last_kernel_ms()
    wr, (_, Bd) = _check(out, B.BT_DENSITY, [0] * len(Fd), Fd, r, s, q, name)
    cD = B.transform_roundings(B.BT_DENSITY, grid.N)
    wc = 0.0
    for a, (n, l) in enumerate(B.FORM_ORBITALS):
        for m, qm in enumerate(q):
            gate = 2 * B.MEASURED[name]["F"][(n, l)][m] + Bd[a, m] * (1 + 1 / cD)
            err = abs(float(LD(out[a, m]) - B.form_factor_closed(n, l, B.ZREF, qm)))
            wc = max(wc, err / gate)
            assert err <= gate, (name, "F", n, l, qm, out[a, m], err / gate)
    # momentum orbitals 1s .. 4f
    U = np.array([B.hydrogenic_u(n, l, B.ZREF, rl) for n, l in B.MOMENTUM_ORBITALS]).astype(np.float64)
    lo = [l for _, l in B.MOMENTUM_ORBITALS]
    out = D.bessel_transform(ctx, grid, D.BT_ORBITAL, lo, U, q)
    wr2, (_, Bo) = _check(out, B.BT_ORBITAL, lo, U, r, s, q, name)
    cO = B.transform_roundings(B.BT_ORBITAL, grid.N)
    for a, (n, l) in enumerate(B.MOMENTUM_ORBITALS):
        closed = [B.momentum_closed(n, l, B.ZREF, qm) for qm in q]
        sign = 1 if out[a, 0] * closed[0] > 0 else -1                            # the convention, fixed at the smallest q
        for m, qm in enumerate(q):
            gate = 2 * B.MEASURED[name]["M"][(n, l)][m] + Bo[a, m] * (1 + 1 / cO)
            err = abs(float(LD(out[a, m]) - sign * closed[m]))
            wc = max(wc, err / gate)
            assert err <= gate, (name, "M", n, l, qm, out[a, m], float(sign * closed[m]), err / gate)
    print("%s: rounding %.3f of the bound, closed forms %.3f of the gate; launch of %d x %d values %.4f ms" % (name, max(wr, wr2), wc, len(Fd), len(q), ms))


# ---- d. bit for bit ---------------------------------------------------------------------------------------------------------------------------
def _rows19(r):
    """19 rows with l cycling through 0 .. 4"""
    base = _smooth(r)
    rows = [base[k % 5] * (1.0 + 0.01 * k) for k in range(19)]
    return np.array(rows), np.array([k % 5 for k in range(19)])


def test_a_q_and_a_row_do_not_depend_on_their_company(ctx, grids):
    grid, r, _ = grids("log12")
    F, l = _rows19(r)
    for kind in (D.BT_DENSITY, D.BT_ORBITAL):
        row, lrow, qm = F[8], int(l[8]), 7.5
        alone = D.bessel_transform(ctx, grid, kind, [lrow], row, [qm])[0, 0]
        others = np.delete(Q17, 8)
        base = D.bessel_transform(ctx, grid, kind, [lrow], row, others)[0]
        for pos in (0, 1, 7, 8, 15, 16):
            out = D.bessel_transform(ctx, grid, kind, [lrow], row, np.insert(others, pos, qm))[0]
            assert out[pos] == alone and np.array_equal(np.delete(out, pos), base), (kind, pos)
        assert np.array_equal(D.bessel_transform(ctx, grid, kind, [lrow], row, others)[0], base)
        batch = D.bessel_transform(ctx, grid, kind, l, F, Q17)
        for a in (0, 8, 18):
            assert np.array_equal(D.bessel_transform(ctx, grid, kind, [int(l[a])], F[a], Q17)[0], batch[a]), (kind, a)
        assert np.array_equal(D.bessel_transform(ctx, grid, kind, l[::-1], F[::-1], Q17[::-1]), batch[::-1, ::-1])


def test_qblock_knob_changes_no_bit(ctx, grids):
    grid, r, _ = grids("log12")
    F, l = _rows19(r)
    for kind in (D.BT_DENSITY, D.BT_ORBITAL):
        own = D.bessel_transform(ctx, grid, kind, l, F, Q17)
        for qb in (1, 2, 4, 8):
            with knobs(BESSEL_QBLOCK=qb):
                assert np.array_equal(D.bessel_transform(ctx, grid, kind, l, F, Q17), own), (kind, qb)
                assert np.array_equal(D.bessel_transform(ctx, grid, kind, l[:1], F[:1], Q17[:9]), own[:1, :9]), (kind, qb)


def _channels(lsda):
    return [0, 1] if lsda else [0]


@pytest.mark.parametrize("Z,lsda", [([10], False), ([7], True), ([1, 10, 26], False)])
def test_scf_entries_are_the_direct_entry_on_the_exported_arrays(ctx, grids, Z, lsda):
    grid, r, s = grids("log12")
    q = Q17[:9]
    scf = D.Scf(ctx, grid, Z, lsda=lsda, alpha=ALPHA)
    try:
        f0 = scf.form_factors(q)                                                 # valid from creation on: the flat start density
        assert f0.shape == (len(Z), 3 if lsda else 1, len(q))
        for a in range(len(Z)):
            rows = np.array([scf.array(w, a) for w in ((0, 1, 2) if lsda else (0,))])
            assert np.array_equal(D.bessel_transform(ctx, grid, D.BT_DENSITY, [0] * len(rows), rows, q), f0[a]), ("start", a)
        for _ in range(3):
            scf.step()
        f = scf.form_factors(q)
        ms = ctx.last_kernel_ms()
        mo, jobs = scf.momentum_orbitals(q)
        assert ms > 0 and ctx.last_kernel_ms() > 0 and mo.shape == (scf.njobs, len(q)) and len(jobs) == scf.njobs
        row = 0
        worst = 0.0
        for a in range(len(Z)):
            rows = np.array([scf.array(w, a) for w in ((0, 1, 2) if lsda else (0,))])
            direct = D.bessel_transform(ctx, grid, D.BT_DENSITY, [0] * len(rows), rows, q)
            assert np.array_equal(direct, f[a]), a
            w, (V, Bd) = _check(f[a], B.BT_DENSITY, [0] * len(rows), rows, r, s, q, ("form factors", Z, a))
            worst = max(worst, w)
            if lsda:                                                             # f[rho] against f[rho_a] + f[rho_b]
                assert np.all(np.abs(f[a, 0] - (f[a, 1] + f[a, 2])) <= Bd[0] + Bd[1] + Bd[2] + EPS * np.abs(f[a, 0]))
            for sp in _channels(lsda):
                U = scf.orbitals(a, sp)
                lv = scf.levels(a, sp)["l"]
                direct = D.bessel_transform(ctx, grid, D.BT_ORBITAL, lv, U, q)
                assert np.array_equal(direct, mo[row:row + len(U)]), (a, sp)
                assert [j[:2] + (j[3],) for j in jobs[row:row + len(U)]] == [(a, sp, int(x)) for x in lv]
                row += len(U)
        assert row == scf.njobs
        assert np.array_equal(scf.form_factors(q), f) and np.array_equal(scf.momentum_orbitals(q)[0], mo)
    finally:
        scf.close()
    print("Z = %s %s: form factors %.3f of the bound" % (Z, "LSDA" if lsda else "LDA", worst))


def test_frozen_atoms_keep_their_transforms(ctx, grids):
    """the batch of test_gpu_orbitals.test_frozen_atoms_keep_their_orbitals: H and Ar freeze in step 33 while Cu is live"""
    grid, _, _ = grids("log12")
    q = Q17[:9]
    scf = D.Scf(ctx, grid, [1, 18, 29], alpha=ALPHA)
    try:
        for _ in range(80):
            scf.step(want_stats=False)
            fin = scf.energies()[1]
            if fin[0] and fin[1]:
                break
        assert fin[0] and fin[1] and not fin[2], "the premise: hydrogen and argon finish while copper is live"
        f1, (m1, jobs) = scf.form_factors(q), scf.momentum_orbitals(q)
        for _ in range(5):
            scf.step(want_stats=False)
        assert not scf.energies()[1][2]
        f2, m2 = scf.form_factors(q), scf.momentum_orbitals(q)[0]
    finally:
        scf.close()
    frozen = np.array([j[0] < 2 for j in jobs])
    assert np.array_equal(f1[:2], f2[:2]) and np.array_equal(m1[frozen], m2[frozen])
    assert np.any(f1[2] != f2[2]) and np.all(np.any(m1[~frozen] != m2[~frozen], axis=1))


# ---- e. physics ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Z,kw,ne,lsda", [(10, {}, 10.0, False), (18, {"config": "[Ne] 3s2 3p5.5"}, 17.5, False), (26, {"charge": 2}, 24.0, True)],
                         ids=["Ne", "Ar 3p5.5", "Fe2+"])
def test_form_factor_at_zero_is_the_electron_count(ctx, grids, Z, kw, ne, lsda):
    """40 steps, as the check of DESIGN.md 4.6 whose figure this is (tests/test_gpu_ions.py): the flat start density integrates to
    N_e (1 - 1.5e-3) on this grid, and linear mixing keeps 0.5^steps of it -- after 3 steps f(0) / N_e - 1 is -1.87e-4 for every atom"""
    grid, r, s = grids("log12")
    scf = D.Scf(ctx, grid, [Z], lsda=lsda, alpha=ALPHA, **kw)
    try:
        for _ in range(40):
            scf.step(want_stats=False)
        f = scf.form_factors([0.0])[0, :, 0]
        rho = scf.array(0)
    finally:
        scf.close()
    v, b = B.transform(B.BT_DENSITY, 0, rho, r, s, 0.0)                          # j_0(0) = 1: Q[4 pi rho r^2 s]
    print("Z = %d, %.1f electrons: f(0) = %.15f, |f(0) - Q| / bound %.3f, |f(0) / N_e - 1| = %.2e" % (Z, ne, f[0], abs(float(LD(f[0]) - v)) / b, abs(f[0] / ne - 1)))
    assert abs(float(LD(f[0]) - v)) <= b
    assert abs(f[0] - ne) <= 1e-9 * ne
    if lsda:
        assert abs(f[0] - (f[1] + f[2])) <= 3 * b + EPS * ne


def test_hydrogen_lsda_against_the_exact_1s_form_factor(ctx, grids):
    """H, LSDA, converged on log12: |f(q) - 1 / (1 + q^2 / 4)^2| <= 1.3e-2 at q = 0.5 and 6.0e-3 at q = 3 -- the distance the CPU
    reference run of the same atom has (1.265e-2, 5.965e-3: _bessel_ref.H_LSDA_DISTANCE, held by tests/test_bessel_ref.py); it is the
    self-interaction of the functional, not rounding.  One electron, all of it alpha: f_b = 0 exactly, f_a = f within the bounds."""
    grid, r, s = grids("log12")
    q = np.array(sorted(B.H_LSDA_DISTANCE))
    scf = D.Scf(ctx, grid, [1], lsda=True, alpha=ALPHA)
    try:
        for _ in range(150):
            scf.step(want_stats=False)
            if scf.energies()[1][0]:
                break
        assert scf.energies()[1][0]
        f = scf.form_factors(q)[0]
    finally:
        scf.close()
    for m, qm in enumerate(q):
        dist = abs(float(LD(f[0, m]) - B.form_factor_closed(1, 0, 1, qm)))
        print("H LSDA q = %g: f = %.12f, distance from the exact 1s %.4e (gate %.1e)" % (qm, f[0, m], dist, B.H_LSDA_DISTANCE[qm]))
        assert dist <= B.H_LSDA_DISTANCE[qm]
    assert np.all(f[2] == 0) and np.all(np.abs(f[0] - f[1]) <= 1e-13)


# ---- f. the front end and the error paths -------------------------------------------------------------------------------------------------
def test_cli_form_factor_table(ctx, grids):
    """dftatom_cli --form-factor-table: after Finished!, 41 lines whose figures are those of Scf.form_factors at six decimals; without
    the flag the output is byte for byte what it is with the table taken out; =smax:ns sets the table; LSDA adds f_a - f_b"""
    import os
    import subprocess
    exe = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "dftatom_amd", "compat", "dftatom_cli")
    args = [exe, "10", "12", "0.5", "25", "0.002", "0"]
    plain = subprocess.run(args, capture_output=True, text=True, timeout=120)
    table = subprocess.run(args + ["--form-factor-table"], capture_output=True, text=True, timeout=120)
    assert plain.returncode == 0 and table.returncode == 0, (plain.stderr, table.stderr)
    for bad in ("2:0", "2", "-1:5", "2:5x"):                                     # refused before anything runs
        assert subprocess.run(args + ["--form-factor-table=" + bad], capture_output=True, text=True, timeout=120).returncode == 2, bad
    lines = table.stdout.split("\n")
    rows = [k for k, ln in enumerate(lines) if ln.startswith("FormFactor ")]
    assert len(rows) == 41 and rows == list(range(rows[0], rows[0] + 41)) and lines[rows[0] - 2] == "Finished!" and lines[rows[-1] + 1] == ""
    assert "\n".join(lines[:rows[0]] + lines[rows[-1] + 2:]) == plain.stdout and "FormFactor" not in plain.stdout
    grid, _, _ = grids("log12")
    scf = D.Scf(ctx, grid, [10], alpha=ALPHA)
    try:
        for _ in range(100):
            scf.step(want_stats=False)
            if scf.energies()[1][0]:
                break
        sv = [2.0 * k / 40 for k in range(41)]
        qv = [((4.0 * np.pi) * x) * 0.529177210903 for x in sv]
        f = scf.form_factors(qv)[0, 0]
    finally:
        scf.close()
    for k, row in enumerate(rows):
        want = "FormFactor s = %.6f q = %.6f f = %.6f" % (sv[k], qv[k], f[k])
        assert lines[row] == want, (lines[row], want)
    assert lines[rows[0]] == "FormFactor s = 0.000000 q = 0.000000 f = 10.000000"
    # =smax:ns, and LSDA's extra column: hydrogen, one alpha electron, f_a - f_b = f
    lsda = subprocess.run([exe, "1", "12", "0.5", "25", "0.002", "1", "--form-factor-table=1.5:4"], capture_output=True, text=True, timeout=120)
    assert lsda.returncode == 0, lsda.stderr
    got = [ln.split() for ln in lsda.stdout.split("\n") if ln.startswith("FormFactor ")]
    s4 = [1.5 * k / 3 for k in range(4)]
    assert len(got) == 4 and " ".join(got[0]) == "FormFactor s = 0.000000 q = 0.000000 f = 1.000000 fa-fb = 1.000000"
    for k, t in enumerate(got):
        assert t[:7] == ("FormFactor s = %.6f q = %.6f" % (s4[k], ((4.0 * np.pi) * s4[k]) * 0.529177210903)).split() and t[9] == t[12], t


def test_error_paths(ctx, grids):
    grid, r, _ = grids("log12")
    lib, N = ctx.lib, grid.N
    ip, dp = D.c_ip, D.c_dp
    last = lambda: lib.dfta_last_error(ctx.h).decode()                           # noqa: E731
    F = np.full((2, N), 0.5)
    l = np.array([0, 4], np.int32)
    q = np.array([0.0, 1.0, 2.0])
    out = np.full(64, 7.0)
    pF, pl, pq, po = F.ctypes.data_as(dp), l.ctypes.data_as(ip), q.ctypes.data_as(dp), out.ctypes.data_as(dp)
    bt = lib.dfta_bessel_transform
    # null pointers
    assert bt(None, grid.h, 0, 2, pl, pF, 3, pq, po) == 1 and bt(ctx.h, None, 0, 2, pl, pF, 3, pq, po) == 1
    for args in ((None, pF, pq, po), (pl, None, pq, po), (pl, pF, None, po), (pl, pF, pq, None)):
        assert bt(ctx.h, grid.h, 0, 2, args[0], args[1], 3, args[2], args[3]) == 1 and last()
    # kind, l, q
    for kind in (-1, 2):
        assert bt(ctx.h, grid.h, kind, 2, pl, pF, 3, pq, po) == 1 and "kind" in last()
    for badl in (-1, 5):
        lb = np.array([0, badl], np.int32)
        assert bt(ctx.h, grid.h, 1, 2, lb.ctypes.data_as(ip), pF, 3, pq, po) == 1 and "l outside" in last()
        assert lib.dfta_sph_bessel(ctx.h, badl, 3, pq, po) == 1 and "l outside" in last()
    for badq in (-1.0, -1e-300, np.nan, np.inf, -np.inf):
        qb = np.array([0.0, badq, 2.0])
        assert bt(ctx.h, grid.h, 0, 2, pl, pF, 3, qb.ctypes.data_as(dp), po) == 1 and "q must be" in last(), badq
        assert lib.dfta_sph_bessel(ctx.h, 1, 3, qb.ctypes.data_as(dp), po) == 1 and "x must be" in last(), badq
    assert bt(ctx.h, grid.h, 0, -1, pl, pF, 3, pq, po) == 1 and bt(ctx.h, grid.h, 0, 2, pl, pF, -1, pq, po) == 1
    assert lib.dfta_sph_bessel(None, 1, 3, pq, po) == 1 and lib.dfta_sph_bessel(ctx.h, 1, 3, None, po) == 1 and lib.dfta_sph_bessel(ctx.h, 1, 3, pq, None) == 1
    assert np.all(out == 7.0)
    # nothing to do: OK, nothing written (even with null tables)
    assert bt(ctx.h, grid.h, 0, 0, None, None, 3, pq, po) == 0 and bt(ctx.h, grid.h, 1, 2, pl, pF, 0, None, None) == 0
    assert lib.dfta_sph_bessel(ctx.h, 2, 0, None, None) == 0
    assert D.bessel_transform(ctx, grid, 0, l, F, np.zeros(0)).shape == (2, 0) and D.sph_bessel(ctx, 3, np.zeros(0)).shape == (0,)
    assert np.all(out == 7.0)
    with pytest.raises(ValueError):
        D.bessel_transform(ctx, grid, 0, [0], F, q)
    scf = D.Scf(ctx, grid, [10], alpha=ALPHA)
    try:
        # momentum orbitals before the first step; form factors are valid from creation on
        assert lib.dfta_scf_momentum_orbitals(scf.h, 3, pq, po) == 1 and "step" in last()
        with pytest.raises(D.DftaError):
            scf.momentum_orbitals(q)
        assert np.all(out == 7.0)
        assert lib.dfta_scf_form_factors(scf.h, 3, pq, po) == 0 and np.all(out[:3] != 7.0) and np.all(out[3:] == 7.0)
        out[:] = 7.0
        scf.step()
        for fn in (lib.dfta_scf_form_factors, lib.dfta_scf_momentum_orbitals):
            assert fn(None, 3, pq, po) == 1
            assert fn(scf.h, 3, None, po) == 1 and last() and fn(scf.h, 3, pq, None) == 1 and fn(scf.h, -1, pq, po) == 1
            for badq in (-1.0, np.nan, np.inf):
                qb = np.array([0.0, badq, 2.0])
                assert fn(scf.h, 3, qb.ctypes.data_as(dp), po) == 1 and "q must be" in last(), badq
            assert fn(scf.h, 0, None, None) == 0
        assert np.all(out == 7.0)
        assert lib.dfta_scf_momentum_orbitals(scf.h, 3, pq, po) == 0 and np.all(out[:9] != 7.0) and np.all(out[9:] == 7.0)
    finally:
        scf.close()
