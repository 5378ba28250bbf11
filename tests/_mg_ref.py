"""CPU reference of the multigrid's cycle drivers: PoissonSolver's Initialize, Ascend, Descend, VCycle and FullCycle restated in Python
on the oracle's three primitives (dfo_gauss_seidel, dfo_restrict, dfo_prolong; tests/_oracle.py), in the style of tests/_scf_ref.py.

Why a restatement when the oracle has dfo_full_cycle: it can start from ANY level-0 source (the device's own, read back after a solve),
and it records every stop test `err < errorMin` the cycle takes, as (|err / errorMin - 1|, level, n).  A GPU sweep reproduces every
node's bits but adds the n terms of a norm in another order; two orders of a sum of n non-negative terms differ by at most about
2 (n - 2) 2^-53 relative, the square root halves that and adds one rounding: two norms differ by at most n 2^-52 relative (2.9e-11 at
131073 nodes).  While every recorded margin is >= MARGIN = 1e-9 no decision can differ, so the GPU must return the restatement's bits
and its V-cycle count -- tests/test_mg_ref.py shows the margins for the inputs of tests/test_gpu_multigrid_ops.py with the reference
alone, and that the restatement returns the bits of dfo_solve_poisson_nonuniform / _uniform.
"""
import math

import numpy as np

import _oracle as O

MARGIN = 1e-9

# (mg_levels, delta, Rmax); delta None: the uniform grid.  The smallest grid of every layout the planner makes (see the GPU test).
GRIDS = [(3, 0.3, 25.0), (4, 0.2, 25.0), (5, 0.1, 25.0), (6, 0.06, 25.0), (7, 0.05, 25.0),
         (8, 3.2e-2, 25.0), (9, 1.6e-2, 25.0), (10, 8e-3, 25.0), (11, 4e-3, 25.0),
         (12, 2e-3, 25.0), (13, 1e-3, 25.0), (14, 5e-4, 25.0), (17, 1e-4, 50.0),
         (9, None, 25.0), (12, None, 25.0)]
ZS = (1, 18, 86)


def grid_id(g):
    return "L%d%s" % (g[0], "u" if g[1] is None else "")


def solve_cases():
    """every (grid, Z) the GPU tests run a whole cycle on: all three atoms everywhere, Z = 86 alone at 17 levels"""
    return [(g, Z) for g in GRIDS for Z in ZS if g[0] != 17 or Z == 86]


def radii(levels, delta, Rmax):
    """node positions as the oracle's source fill computes them"""
    N = O.oracle().dfo_num_nodes(levels)
    if delta is None:
        i = np.arange(N, dtype=np.float64)
        return (0.0 * ((N - 1) - i) + Rmax * i) / (N - 1)
    return O.grid_r(O.make_grid(levels, delta, Rmax))


def density_1s(r, Z):
    return Z * np.exp(-2.0 * r) / np.pi


def norm_bound(n):
    """relative distance of two summation orders of a sweep's error norm over n nodes"""
    return n * 2.0 ** -52


class MgRef:
    """One oracle multigrid (dfo_poisson) with numpy views of its arrays: Phi[l], Src[l], n[l] -- plant any state on any level."""

    def __init__(self, levels, delta):
        self.o = O.oracle()
        self.levels = levels
        self.ps = self.o.dfo_poisson_create(levels, float(delta or 0.0))
        p = self.ps.contents
        self.n = [p.n[l] for l in range(levels)]
        self.Phi = [np.ctypeslib.as_array(p.Phi[l], (self.n[l],)) for l in range(levels)]
        self.Src = [np.ctypeslib.as_array(p.Src[l], (self.n[l],)) for l in range(levels)]
        self.tests = []                 # (|err / errorMin - 1|, level, n) of every stop test since the last clear
        self.vcycles = 0

    def close(self):
        if self.ps:
            self.Phi = self.Src = None
            self.o.dfo_poisson_destroy(self.ps)
            self.ps = None

    def set_boundaries(self, low, high):
        self.ps.contents.lowB, self.ps.contents.highB = float(low), float(high)

    # ---- the oracle's own solves (they build the level-0 source, which no cycle overwrites) ----------------------------------------
    def oracle_solve(self, Z, Rmax, density, uniform):
        """dfo_solve_poisson_nonuniform / _uniform: (U, V-cycles)"""
        U = np.zeros(self.n[0])
        before = self.ps.contents.n_vcycles
        rho = np.ascontiguousarray(density, dtype=np.float64)
        solve = self.o.dfo_solve_poisson_uniform if uniform else self.o.dfo_solve_poisson_nonuniform
        solve(self.ps, int(Z), float(Rmax), O.dp(rho), O.dp(U))
        return U, self.ps.contents.n_vcycles - before

    # ---- the three primitives -----------------------------------------------------------------------------------------------------
    def gauss_seidel(self, l):
        return self.o.dfo_gauss_seidel(self.ps, l)

    def restrict(self, l):
        """level l-1 -> level l"""
        self.o.dfo_restrict(self.ps, l)

    def prolong(self, l):
        """level l -> level l-1 (additive)"""
        p = self.ps.contents
        self.o.dfo_prolong(p.Phi[l], self.n[l], p.Phi[l - 1])

    # ---- the restated drivers -----------------------------------------------------------------------------------------------------
    def stop(self, err, error_min, l):
        """the cycle's only kind of decision"""
        if error_min > 0:
            self.tests.append((abs(err / error_min - 1.0), l, self.n[l]))
        return err < error_min

    def iterate(self, l, error_min, iterno):
        """IterateGaussSeidel: (err of the last sweep, sweeps executed)"""
        err, done = 1E10, 0
        for _ in range(iterno):
            err = self.gauss_seidel(l)
            done += 1
            if self.stop(err, error_min, l):
                break
        return err, done

    def initialize(self, error_min):
        self.Phi[0][:] = 0
        for l in range(1, self.levels):
            lim = self.n[l] - 1
            self.Src[l][1:lim] = 4 * self.Src[l - 1][2:2 * lim:2]
            self.Src[l][0] = self.Src[l][lim] = 0
            self.Phi[l][:] = 0
        c = self.levels - 1
        p = self.ps.contents
        self.Phi[c][0], self.Phi[c][self.n[c] - 1] = p.lowB, p.highB
        self.iterate(c, error_min, 15)

    def ascend(self, lo, hi, error_min, iterno):
        for l in range(lo, hi):
            self.iterate(l, error_min, iterno)
            self.restrict(l + 1)
        self.iterate(hi, error_min, iterno)

    def descend(self, hi, lo, error_min, iterno):
        err = 1E10
        for l in range(hi, lo, -1):
            self.prolong(l)
            err, _ = self.iterate(l - 1, error_min, iterno)
        return err

    def vcycle(self, error_min, iterno=3):
        last = self.levels - 1
        self.ascend(0, last, error_min, iterno)
        self.vcycles += 1
        return self.descend(last, 0, error_min, iterno)

    def full_cycle(self, low, high, error_min=1E-3, error_min_last=1E-14):
        """SetBoundaries + FullCycle on the level-0 source in place: (err, V-cycles); Phi[0] holds the solution"""
        self.set_boundaries(low, high)
        last, sweeps = self.levels - 1, 3
        self.vcycles = 0
        self.initialize(error_min)
        for l in range(self.levels - 2, 0, -1):
            self.descend(last, l, error_min, sweeps)
            self.ascend(l, last, error_min, sweeps)
        self.descend(last, 0, error_min_last, sweeps)
        err = 0.0
        for _ in range(100):
            err = self.vcycle(error_min_last, sweeps)
            if self.stop(err, error_min_last, 0):
                break
        return err, self.vcycles

    def min_margin(self):
        """(smallest |err / errorMin - 1|, level, n) over the recorded stop tests"""
        return min(self.tests) if self.tests else (math.inf, -1, 0)


def solve_from_source(levels, delta, src0, Z):
    """the restated FullCycle(1E-3, 1E-14) with boundaries (0, Z) on a given level-0 source: (U, V-cycles, smallest margin)"""
    m = MgRef(levels, delta)
    try:
        m.Src[0][:] = src0
        _, vc = m.full_cycle(0.0, float(Z))
        return m.Phi[0].copy(), vc, m.min_margin()
    finally:
        m.close()


def oracle_case(levels, delta, Rmax, Z):
    """the oracle's solve of the 1s density of charge Z on a grid: (rho, level-0 source, U, V-cycles)"""
    rho = density_1s(radii(levels, delta, Rmax), Z)
    m = MgRef(levels, delta)
    try:
        U, vc = m.oracle_solve(Z, Rmax, rho, delta is None)
        return rho, m.Src[0].copy(), U, vc
    finally:
        m.close()
