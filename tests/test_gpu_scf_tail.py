"""GPU suite (-m gpu): the tail of an SCF step, bit for bit -- k_tail, k_integrate over the batch's 5 natoms rows (and
k_integrate_simpson38_par in the sweeps' tolerance mode), k_energies with its stop test, and the start-up kernels k_init_density and
k_potential (scf.hip, reduce.hip).

The library is built with -ffp-contract=off and these kernels keep the reference's operation order and call no elementary function,
so after every step the device's own arrays -- Scf.array(0 .. 5), the eigenvalues, occupations and convergence flags of levels(), the
nine fields of energies() -- are recomputed in float64 NumPy (tests/_tail_ref.py) and compared BIT FOR BIT:

* the XC arrays come from D.vwn_lda / D.vwn_lsda / D.chachiyo_lda on the device's density: the same pointwise kernels as the step's,
  which give the same bits for the same value wherever it sits (test_gpu_vwn.py, position independence);
* V = (-Z + U) / r + v at i >= 1 and 0 at node 0 -- right after creation that is k_potential on k_init_density's flat start density
  (nE / volume, 0 at node 0, the LSDA split), after a step it is k_tail's first statement;
* the five integrands in k_tail's grouping (LDA, LSDA, and the LSDA grouping of the uniform grid), integrated by the oracle's
  dfo_simpson38 / dfo_trapezoid / dfo_simpson13 / dfo_boole / dfo_romberg(.., 1e-18, 3) with delta = 1 on the logarithmic grid and
  h on the uniform one;
* k_energies: Sum occ E over the atom's jobs (alpha levels, then beta levels, as the job layout has them), the five products with
  4 pi and -2 pi, the four combinations; then the reference's stop test from consecutive Etotal and the flags -- `finished` must flip
  on exactly the step the recomputation says, a frozen atom then keeps every bit while a live atom of the same batch still replays.

In the tolerance mode of the sweeps the quadrature is k_integrate_simpson38_par; its summation order is modelled
(_tail_ref.simpson38_parallel) and the nine energies must equal that model bit for bit.  A model of an order shares the kernel's choices,
so the model's integrals of the device's integrands are also held to Simpson 3/8 in np.longdouble within
parallel_roundings(N) eps Sum |w_i v_i| (29 at 4097 nodes, counted in _tail_ref; tests/test_tail_ref.py shows that a dropped node or a
wrong residue class misses it).  With the SCF_ORDERED_SUMS knob the same run must equal the ordered replay instead.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import _tail_ref as TR                   # noqa: E402
import dftatom_amd as D                  # noqa: E402
from _knobs import knobs                 # noqa: E402

LD = np.longdouble
EPS64 = float(np.finfo(np.float64).eps)
LOG12 = (12, 2e-3, 25.0)
UNIFORM = (14, None, 25.0)               # the uniform grid of test_gpu_uniform.py (tests/golden/uniform_meta.json)


@pytest.fixture(scope="module")
def ctx(torch_first):
    c = D.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def grids(ctx):
    """name -> (grid, r, dr/di table, quadrature step)"""
    made = {}

    def get(name):
        if name not in made:
            g = D.Grid(ctx, *(LOG12 if name == "log" else UNIFORM))
            r = g.r()
            if g.uniform:
                made[name] = (g, r, np.ones(g.N), float(r[1]))
            else:
                made[name] = (g, r, TR.log_cnst(g.Rp, g.delta, g.N), 1.0)
        return made[name]
    yield get
    for g, _, _, _ in made.values():
        g.close()


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.int64)


def same(x, y):
    return np.array_equal(bits(x), bits(y))


class Run:
    """an Scf and what the replay needs to know about it"""

    def __init__(self, ctx, grids, gname, Z, lsda=False, functional=D.XC_VWN, config=None, rule=D.INT_SIMPSON38, sweep_mode=D.SWEEPS_EXACT,
                 parallel=False):
        self.ctx, self.Z, self.lsda, self.functional, self.rule, self.parallel = ctx, list(Z), lsda, functional, rule, parallel
        self.grid, self.r, self.cnst, self.dq = grids(gname)
        self.scf = D.Scf(ctx, self.grid, self.Z, lsda=lsda, functional=functional, config=config, integrator=rule, sweep_mode=sweep_mode)
        self.stop = [TR.StopTest() for _ in self.Z]
        self.steps = 0

    def close(self):
        self.scf.close()

    def arrays(self, a):
        return [self.scf.array(w, a) for w in range(6)]

    def xc(self, rho, dA, dB):
        """(Vexc, va, vb, eexc) of the step's own pointwise kernel on the device's density"""
        if self.lsda:
            return D.vwn_lsda(self.ctx, dA, dB)
        if self.functional == D.XC_VWN:
            v, e = D.vwn_lda(self.ctx, rho)
        else:
            v, e = D.chachiyo_lda(self.ctx, rho, improved=self.functional == D.XC_CHACHIYO_IMPROVED)
        return v, None, None, e

    def occupations(self, a):
        return [self.scf.levels(a, spin) for spin in range(2 if self.lsda else 1)]

    def start_occupations(self, a, spin):
        """levels() has no eigenvalues to give before the first step; the occupations are there from creation"""
        lib, h = self.ctx.lib, self.scf.h
        occ = np.zeros(max(lib.dfta_scf_num_levels(h, a, spin), 1))
        self.ctx.check(lib.dfta_scf_get_occupations(h, a, spin, occ.ctypes.data_as(D.c_dp)))
        return occ

    def check_start(self):
        """k_init_density and k_potential, right after creation"""
        N = self.grid.N
        for a, Z in enumerate(self.Z):
            rho, dA, dB, potA, potB, U = self.arrays(a)
            nA = float(np.sum(self.start_occupations(a, 0)))              # whole numbers and halves: the sum is exact
            nB = float(np.sum(self.start_occupations(a, 1))) if self.lsda else 0.0
            want = TR.start_density(nA + nB, nA, nB, self.lsda, self.grid.Rmax, N)
            assert same(rho, want[0]) and rho[0] == 0.0 and rho[1] > 0
            if self.lsda:
                assert same(dA, want[1]) and same(dB, want[2])
            else:
                assert same(dA, rho) and same(dB, rho)                       # array(1 / 2) of an LDA run is the density
            Vexc, va, vb, _ = self.xc(rho, dA, dB)
            wA, wB = TR.potentials(Z, self.lsda, self.r, U, Vexc, va, vb)
            assert same(potA, wA) and same(potB, wB if self.lsda else wA), a
            assert potA[0] == 0.0 and np.all(np.isfinite(potA))

    def replay(self, a):
        """the nine energies of atom a recomputed from the device's arrays; V checked on the way; returns (energies, integrands)"""
        rho, dA, dB, potA, potB, U = self.arrays(a)
        Vexc, va, vb, eexc = self.xc(rho, dA, dB)
        wA, wB = TR.potentials(self.Z[a], self.lsda, self.r, U, Vexc, va, vb)
        assert same(potA, wA) and same(potB, wB if self.lsda else wA), ("V", a, self.steps)
        if self.lsda:
            assert same(rho[1:], (dA + dB)[1:])
        F = TR.integrands(self.Z[a], self.lsda, self.grid.uniform, self.r, self.cnst, rho, dA, dB, U, Vexc, eexc, wA, wB)
        if self.parallel:
            I = [TR.simpson38_parallel(f, self.dq) for f in F]
        else:
            I = [TR.quadrature(self.rule, self.dq, f) for f in F]
        occ, E = [], []
        for lv in self.occupations(a):
            occ += list(lv["occupation"])
            E += list(lv["E"])
        return TR.assemble(occ, E, I), F

    def converged(self, a):
        return all(bool(np.all(lv["converged"] != 0)) for lv in self.occupations(a))

    def step(self, check=None):
        """one step; every live atom (or those of `check`) replayed: nine energies and the stop test.  Returns the device's energies"""
        was = self.scf.energies()[1].copy()
        self.scf.step(want_stats=False)
        self.steps += 1
        en, fin = self.scf.energies()
        for a in range(len(self.Z)):
            if was[a] or (check is not None and a not in check):
                continue
            want, _ = self.replay(a)
            got = {k: getattr(en[a], k) for k in TR.FIELDS}
            bad = [k for k in TR.FIELDS if not same(got[k], want[k])]
            assert not bad, (self.steps, a, bad, [(got[k], want[k]) for k in bad])
            assert self.stop[a].step(want["Etotal"], self.converged(a)) == fin[a], ("stop test", self.steps, a)
        return en, fin

    def nine(self, a):
        e = self.scf.energies()[0][a]
        return [getattr(e, k) for k in TR.FIELDS]


SINGLE = [
    ("Ne LDA", "log", [10], False, D.XC_VWN, None),
    ("N LSDA", "log", [7], True, D.XC_VWN, None),
    ("Ne LDA uniform", "uniform", [10], False, D.XC_VWN, None),
    ("N LSDA uniform", "uniform", [7], True, D.XC_VWN, None),
    ("Ar 3p5.5 LDA", "log", [18], False, D.XC_VWN, "[Ne] 3s2 3p5.5"),
    ("N 2p2.5/0.5 LSDA", "log", [7], True, D.XC_VWN, "1s2 2s2 2p2.5/0.5"),
    ("Ne Chachiyo improved", "log", [10], False, D.XC_CHACHIYO_IMPROVED, None),
]


@pytest.mark.parametrize("case", SINGLE, ids=[c[0].replace(" ", "_").replace("/", "_") for c in SINGLE])
def test_start_and_first_steps(ctx, grids, case):
    """k_init_density / k_potential after creation, then steps 1 - 3 replayed"""
    name, gname, Z, lsda, fx, config = case
    run = Run(ctx, grids, gname, Z, lsda=lsda, functional=fx, config=config)
    try:
        run.check_start()
        for _ in range(3):
            en, fin = run.step()
            assert not fin[0] and np.isfinite(en[0].Etotal) and en[0].Etotal < 0
        if "uniform" in name:
            assert run.grid.uniform and run.dq == 25.0 / (run.grid.N - 1)
        if config:
            occ = np.concatenate([lv["occupation"] for lv in run.occupations(0)])
            assert np.any(occ != np.floor(occ))
    finally:
        run.close()


RULES = {"trapezoid": D.INT_TRAPEZOID, "simpson13": D.INT_SIMPSON13, "simpson38": D.INT_SIMPSON38, "boole": D.INT_BOOLE, "romberg": D.INT_ROMBERG}
_rule_energies = {}


@pytest.mark.parametrize("rule", sorted(RULES))
def test_live_integrator_bit_for_bit(ctx, grids, rule):
    """Ne LDA, three steps under each quadrature rule (test_live_integrator_switch compares the rules at 2e-5: this is the bit level)"""
    run = Run(ctx, grids, "log", [10], rule=RULES[rule])
    try:
        for _ in range(3):
            run.step()
        _rule_energies[rule] = run.nine(0)
    finally:
        run.close()
    for other, e in _rule_energies.items():
        assert other == rule or e != _rule_energies[rule]                    # the rules do differ


def test_batch_rows(ctx, grids):
    """[H, Ne, Fe], three steps: k_integrate with nvec = 15 and a row stride -- every row replays, and equals the atom run alone"""
    Z = [1, 10, 26]
    run = Run(ctx, grids, "log", Z)
    alone = [Run(ctx, grids, "log", [z]) for z in Z]
    try:
        run.check_start()
        for _ in range(3):
            run.step()
            for k, one in enumerate(alone):
                one.step()
                assert same(run.nine(k), one.nine(0)), (run.steps, k)
        assert len({tuple(run.nine(k)) for k in range(3)}) == 3
    finally:
        run.close()
        for one in alone:
            one.close()


def test_batch_to_its_first_freeze(ctx, grids):
    """[H, Ar, Cu]: the CPU reference (tests/_scf_ref.py, and test_tail_ref.py for H) has H and Ar meet the stop test in step 33 on this
    grid, Cu far later.  Every step of every live atom is replayed, so the recomputed stop test decides the step on which `finished`
    has to flip; on the step after it the frozen atoms keep every bit and Cu still replays."""
    run = Run(ctx, grids, "log", [1, 18, 29])
    try:
        frozen_at = {}
        snap = {}
        for step in range(1, 37):
            en, fin = run.step()
            for a in range(3):
                if fin[a] and a not in frozen_at:
                    frozen_at[a] = step
                    snap[a] = (run.arrays(a), run.nine(a), [lv["E"].copy() for lv in run.occupations(a)], step)
            if len(frozen_at) == 2 and step > max(frozen_at.values()):
                break
        print("stop test met in steps %s" % frozen_at)
        assert sorted(frozen_at) == [0, 1] and not fin[2], (frozen_at, list(fin))
        assert frozen_at[0] == 33 and frozen_at[1] == 33                       # the CPU reference's count
        assert run.steps == 34 and not run.stop[2].finished
        for a, (arr, nine, E, at) in snap.items():
            assert run.stop[a].finished
            for x, y in zip(arr, run.arrays(a)):
                assert same(x, y), a
            assert same(nine, run.nine(a))
            for x, lv in zip(E, run.occupations(a)):
                assert same(x, lv["E"])
    finally:
        run.close()


@pytest.mark.parametrize("Z", [[10], [1, 10, 26]], ids=["Ne", "H_Ne_Fe"])
@pytest.mark.parametrize("ordered", [False, True], ids=["parallel", "ordered_knob"])
def test_tolerance_mode_quadrature(ctx, grids, Z, ordered):
    """sweeps in tolerance mode: the energies equal the model of k_integrate_simpson38_par's order bit for bit (with SCF_ORDERED_SUMS:
    the ordered replay), and the model's integrals of the device's integrands sit within the counted bound of extended Simpson 3/8"""
    with knobs({"SCF_ORDERED_SUMS": "1"} if ordered else {}):
        run = Run(ctx, grids, "log", Z, sweep_mode=D.SWEEPS_TOLERANCE, parallel=not ordered)
        try:
            for _ in range(3):
                run.step()
            worst, differ = 0.0, False
            c = TR.parallel_roundings(run.grid.N)
            assert c == 29
            for a in range(len(Z)):
                _, F = run.replay(a)
                for f in F:
                    ext, mag = TR.simpson38_extended(f, run.dq)
                    par = TR.simpson38_parallel(f, run.dq)
                    worst = max(worst, float(abs(LD(par) - ext) / (c * EPS64 * mag)))
                    differ = differ or par != TR.quadrature(D.INT_SIMPSON38, run.dq, f)
            print("tolerance mode %s: |parallel model - ext| / (%d eps Sum|w v|) max %.3f" % (Z, c, worst))
            assert worst <= 1 and differ                                     # the two orders are told apart by these integrands
        finally:
            run.close()
