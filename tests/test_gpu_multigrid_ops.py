"""GPU suite (-m gpu): the exact multigrid against the CPU oracle's sequential sweep, operation by operation and solve by solve, at the
smallest grid of every layout the planner (dftatom_amd/csrc/poisson_plan.cpp) makes -- DESIGN.md section 2: "restrict, prolong, single
GS sweeps, V-cycle: bit-exact".  Tolerance 0 on every array; POISSON_EXACT everywhere.

Layouts and where they run (plan_poisson for 256 compute units):
  * sequential levels (< 129 nodes, one lane, LDS-resident)            every level of the 3 .. 6-level grids
  * one wave, 129 nodes, outside any coarse section                    level 0 at 7 levels (no production grid has it)
  * one wave, 129 .. 1025 nodes (the coarse section of a V-cycle)      8 .. 10 levels
  * LDS-staged, 2049 / 4097 / 8193 nodes (8, 16, 32 nodes per lane)    level 0 at 11, 12, 13 levels
  * global chunked, 16385 nodes (64 per lane: the fused global pass)   level 0 at 14 levels (the unit entries run ONE workgroup, the solve
                                                                        is resident: 33 workgroups, or 17 for a batch of 8)
  * global chunked, 64 .. 512 nodes per lane                           levels 0 .. 3 at 17 levels under POISSON_GROUP=0
  * shared by 4 workgroups (staged, 8 nodes per lane)                  level 0 at 13 levels in a batch of 40
  * shared by 16 workgroups (staged, 4 nodes per lane)                 level 0 at 14 levels under POISSON_RES=0; level 1 is the
                                                                        hand-over from the shared level to workgroup 0

A. one operation at a time from planted states: Phi = standard_normal(n), Src = 1e-2 standard_normal(n) on every level, the same on the
   device (set_level) and in the oracle's arrays.  Magnitudes are moderate ON PURPOSE: the kernels replace d x 0.5 by (d / 2) x and carry
   2x through a sweep (power-of-two rescalings), and the chunked sweeps start from warm-ups that forget their start values -- identities
   that hold for finite numbers of ordinary size, not across overflow, denormals or 60 orders of magnitude within one level.
   Norms are sums taken in another order: |e - e_ref| <= n 2^-52 e_ref (tests/_mg_ref.py), and e_ref == 0 implies e == 0.
B. whole cycles: full_cycle on the oracle's level-0 source, and solve on the device's own source, against the restatement of
   tests/_mg_ref.py -- bits of U and the V-cycle count, under the margin condition shown there (asserted again for the device's source).
   Source fill (the one place where the device's exp() enters): see test_source_fill_vs_oracle.
"""
import contextlib
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import _mg_ref as M                     # noqa: E402  (checker only)
import dftatom_amd as D                 # noqa: E402
from _knobs import knobs                # noqa: E402


@pytest.fixture(scope="module")
def ctx(torch_first):
    c = D.Context(0)
    yield c
    c.close()


class Case:
    """one solver: a grid of M.GRIDS, a batch size, DFTA_DEBUG entries, the workgroups per atom it must report, the levels section A runs"""

    def __init__(self, name, grid, batch=1, kn=None, group=1, run_levels=None):
        self.name, self.grid, self.batch, self.kn, self.group = name, grid, batch, kn or {}, group
        self.levels = grid[0]
        self.run_levels = list(range(self.levels)) if run_levels is None else run_levels

    def __repr__(self):
        return self.name


_G = {M.grid_id(g): g for g in M.GRIDS}
PLAIN = [Case(M.grid_id(g), g, group=33 if g[0] == 14 else 1) for g in M.GRIDS if g[0] != 17]
SHARED4 = Case("L13-batch40-G4", _G["L13"], batch=40, group=4)
SHARED16 = Case("L14-RES0-G16", _G["L14"], kn={"DFTA_POISSON_RES": "0"}, group=16)
RES16 = Case("L14-batch8-res16", _G["L14"], batch=8, group=17)
L17_ONE = Case("L17-GROUP0", _G["L17"], kn={"DFTA_POISSON_GROUP": "0"}, group=1, run_levels=[0, 1, 2, 3])
L17_RES = Case("L17-resident", _G["L17"], group=33)

OPS_CASES = PLAIN + [SHARED4, SHARED16, L17_ONE]          # A
CYCLE_CASES = PLAIN + [SHARED4, SHARED16]                 # A (vcycle), B.1
SOLVE_CASES = PLAIN + [SHARED4, SHARED16, RES16]          # B.2, B.4


@contextlib.contextmanager
def solver(ctx, case):
    levels, delta, Rmax = case.grid
    grid = D.Grid(ctx, levels, delta, Rmax)
    ps = None
    try:
        with knobs(case.kn):                               # read by dfta_poisson_create_ex
            ps = D.Poisson(ctx, grid, case.batch, D.POISSON_EXACT)
        assert ps.group_info()[0] == case.group, ps.group_info()
        yield grid, ps
    finally:
        if ps is not None:
            ps.close()
        grid.close()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def assert_level(ps, ref, lvl, tag):
    phi, src = ps.get_level(lvl)
    assert np.array_equal(bits(phi), bits(ref.Phi[lvl])), (tag, lvl, "Phi", int(np.sum(bits(phi) != bits(ref.Phi[lvl]))))
    assert np.array_equal(bits(src), bits(ref.Src[lvl])), (tag, lvl, "Src", int(np.sum(bits(src) != bits(ref.Src[lvl]))))


def assert_norm(e, e_ref, n, tag):
    if e_ref == 0:
        assert e == 0, (tag, e)
    else:
        assert abs(e - e_ref) <= M.norm_bound(n) * e_ref, (tag, e, e_ref)


class Planted:
    """the random state of every level, on both sides"""

    def __init__(self, ps, ref, seed):
        rng = np.random.default_rng(seed)
        self.ps, self.ref = ps, ref
        self.phi = [rng.standard_normal(n) for n in ref.n]
        self.src = [1e-2 * rng.standard_normal(n) for n in ref.n]

    def plant(self, lvl):
        self.ps.set_level(lvl, self.phi[lvl], self.src[lvl])
        self.ref.Phi[lvl][:] = self.phi[lvl]
        self.ref.Src[lvl][:] = self.src[lvl]


def _id(c):
    return c.name


# ---- A. one operation at a time -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", OPS_CASES, ids=_id)
def test_sweeps_vs_oracle(ctx, case):
    """gauss_seidel(lvl, k), k = 1, 2, 3 continuing from one call to the next, then iterate_gs(lvl, emin, 3) from the planted state for
    emin = 0 (three sweeps), 1e30 (one) and sqrt(e1 e2) (two: e1, e2 the oracle's first two norms; used where e1 >= 1.2 e2 > 0, which
    fails on the 3-node level alone, where e2 = 0): Phi and Src bits, sweep counts, norms within n 2^-52"""
    ref = M.MgRef(case.levels, case.grid[1])
    try:
        with solver(ctx, case) as (grid, ps):
            st = Planted(ps, ref, 100 + case.levels)
            for lvl in range(case.levels):
                st.plant(lvl)
            for lvl in case.run_levels:
                n = ref.n[lvl]
                assert ps.level_size(lvl) == n
                for k in (1, 2, 3):
                    e = ps.gauss_seidel(lvl, k)
                    for q in range(k):
                        assert_norm(e[q], ref.gauss_seidel(lvl), n, ("gs", lvl, k, q))
                    assert_level(ps, ref, lvl, ("gs", k))
                st.plant(lvl)
                e1, e2 = ref.gauss_seidel(lvl), ref.gauss_seidel(lvl)
                emins = [(0.0, 3), (1e30, 1)]                  # (errorMin, sweeps the reference runs)
                if e1 >= 1.2 * e2 > 0:
                    emins.append((float(np.sqrt(e1 * e2)), 2))
                else:
                    assert n == 3, (lvl, n, e1, e2)
                for emin, sweeps in emins:
                    st.plant(lvl)
                    er, nr = ref.iterate(lvl, emin, 3)
                    assert nr == sweeps, (lvl, emin, nr)
                    e, ns = ps.iterate_gs(lvl, emin, 3)
                    assert ns == nr, (lvl, emin, ns, nr)
                    assert_norm(e, er, n, ("iterate", lvl, emin))
                    assert_level(ps, ref, lvl, ("iterate", emin))
    finally:
        ref.close()


@pytest.mark.parametrize("case", OPS_CASES, ids=_id)
def test_transfers_vs_oracle(ctx, case):
    """restrict(lvl): level lvl gets zero Phi, the oracle's Src and zero ends, level lvl-1 is untouched; prolong(lvl): level lvl-1 gets the
    oracle's Phi, level lvl is untouched"""
    ref = M.MgRef(case.levels, case.grid[1])
    try:
        with solver(ctx, case) as (grid, ps):
            st = Planted(ps, ref, 200 + case.levels)
            for lvl in range(case.levels):
                st.plant(lvl)
            for lvl in case.run_levels:
                if lvl == 0:
                    continue
                ps.restrict(lvl)
                ref.restrict(lvl)
                assert_level(ps, ref, lvl, "restrict")
                phi, src = ps.get_level(lvl)
                assert not phi.any() and src[0] == 0 and src[-1] == 0
                assert np.array_equal(ref.Phi[lvl - 1], st.phi[lvl - 1]) and np.array_equal(ref.Src[lvl - 1], st.src[lvl - 1])
                assert_level(ps, ref, lvl - 1, "restrict: fine level")
                st.plant(lvl)
                ps.prolong(lvl)
                ref.prolong(lvl)
                assert_level(ps, ref, lvl - 1, "prolong")
                assert np.array_equal(ref.Phi[lvl], st.phi[lvl])
                assert_level(ps, ref, lvl, "prolong: coarse level")
                st.plant(lvl - 1)
    finally:
        ref.close()


@pytest.mark.parametrize("case", CYCLE_CASES, ids=_id)
def test_vcycle_vs_oracle(ctx, case):
    """one VCycle(1E-14, 3) from planted data on every level: Phi and Src of every level afterwards, the returned norm"""
    ref = M.MgRef(case.levels, case.grid[1])
    try:
        with solver(ctx, case) as (grid, ps):
            st = Planted(ps, ref, 300 + case.levels)
            for lvl in range(case.levels):
                st.plant(lvl)
            er = ref.vcycle(1e-14, 3)
            assert ref.min_margin()[0] >= M.MARGIN, ref.min_margin()
            e = ps.vcycle()
            assert_norm(e, er, ref.n[0], "vcycle")
            for lvl in range(case.levels):
                assert_level(ps, ref, lvl, "vcycle")
    finally:
        ref.close()


# ---- B. whole cycles ------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def oracle_solution(grid, Z):
    """(rho, the oracle's level-0 source, the restatement's U and V-cycle count on it) -- computed once per module run, never modified"""
    levels, delta, Rmax = grid
    rho, src0, _, _ = M.oracle_case(levels, delta, Rmax, Z)
    U, vc, margin = M.solve_from_source(levels, delta, src0, Z)
    assert margin[0] >= M.MARGIN, (grid, Z, margin)
    for a in (rho, src0, U):
        a.setflags(write=False)
    return rho, src0, U, vc


@pytest.mark.parametrize("case", CYCLE_CASES, ids=_id)
def test_full_cycle_vs_restatement(ctx, case):
    """B.1: the oracle's level-0 source planted with set_level, full_cycle(0, Z): Phi of level 0 and the V-cycle count"""
    with solver(ctx, case) as (grid, ps):
        for Z in M.ZS:
            rho, src0, U, vc = oracle_solution(case.grid, Z)
            ps.set_level(0, src=src0)
            err, n = ps.full_cycle(0.0, float(Z))
            phi, src = ps.get_level(0)
            assert np.array_equal(bits(src), bits(src0)), Z
            assert n == vc, (Z, n, vc)
            assert np.array_equal(bits(phi), bits(U)), (Z, int(np.sum(bits(phi) != bits(U))), float(np.max(np.abs(phi - U))))


_device = {}


def device_solve(ctx, case, Z):
    """solve([Z] * batch, rho) of a case: (U of every atom, V-cycle counts, the device's level-0 source of atom 0); one solve per module run"""
    key = (case.name, Z)
    if key not in _device:
        rho = oracle_solution(case.grid, Z)[0]
        with solver(ctx, case) as (grid, ps):
            U, vc, err = ps.solve([Z] * case.batch, np.tile(rho, (case.batch, 1)))
            _, src = ps.get_level(0)
            assert ps.group_info()[1:] == (False, 0), ps.group_info()       # the planned kernel ran: not degraded, nothing repeated
        _device[key] = (U, vc, src)
    return _device[key]


def assert_solve(case, Z, U, vc, src):
    levels, delta, _ = case.grid
    want, want_vc, margin = M.solve_from_source(levels, delta, src, Z)
    assert margin[0] >= M.MARGIN, (case.name, Z, "margin condition fails on the device's source", margin)
    for a in range(U.shape[0]):
        assert vc[a] == want_vc, (case.name, Z, a, int(vc[a]), want_vc)
        assert np.array_equal(bits(U[a]), bits(want)), (case.name, Z, a, int(np.sum(bits(U[a]) != bits(want))), float(np.max(np.abs(U[a] - want))))


@pytest.mark.parametrize("case", SOLVE_CASES, ids=_id)
def test_solve_vs_restatement(ctx, case):
    """B.2: solve([Z], rho), the device's level-0 source read back with get_level(0), the restatement run on THAT source (its margin
    condition asserted, not assumed): U and the V-cycle count bit for bit.  14 levels: the resident kernels (33 workgroups per atom, 17 in
    a batch of 8).  3 .. 6 levels: level 0 itself is sequential -- k_poisson_solve must put the source into the LDS block it is read from"""
    for Z in M.ZS:
        U, vc, src = device_solve(ctx, case, Z)
        assert_solve(case, Z, U, vc, src)


@pytest.mark.parametrize("case", [L17_RES, L17_ONE], ids=_id)
def test_solve_17_levels_vs_restatement(ctx, case):
    """B.3: 131073 nodes, Z = 86: the resident solve and the one-workgroup solve (POISSON_GROUP=0)"""
    U, vc, src = device_solve(ctx, case, 86)
    assert_solve(case, 86, U, vc, src)


def ulps(a, b):
    """distance in units of the last place between arrays of finite doubles of equal sign"""
    return np.abs(bits(a) - bits(b))


@pytest.mark.parametrize("case", SOLVE_CASES + [L17_RES, L17_ONE], ids=_id)
def test_source_fill_vs_oracle(ctx, case):
    """B.4: the device's level-0 source -- r_i (psrc_i rho_i), r and psrc tables the host fills with libm's exp, the product taken by the
    solve kernels -- against the oracle's Src[0], in ulps, maximum over the nodes and Z = 1, 18, 86 (Z = 86 at 17 levels).
    Measured on an MI355X: 0 ulp for every case (every grid of 3 .. 14 levels, both uniform grids, the groups of 4 and 16, both resident
    kernels, both 17-level solves), so equality is asserted"""
    worst = 0
    for Z in (M.ZS if case.levels != 17 else (86,)):
        src0 = oracle_solution(case.grid, Z)[1]
        src = device_solve(ctx, case, Z)[2]
        assert np.all(np.signbit(src) == np.signbit(src0)) and np.all(np.isfinite(src))
        worst = max(worst, int(np.max(ulps(src, src0))))
    print("source fill %s: %d ulp" % (case.name, worst))
    assert worst == 0, (case.name, worst)
