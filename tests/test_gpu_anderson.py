"""GPU suite (-m gpu): the opt-in Anderson density mixing (DFTA_MIX_ANDERSON, dftatom_amd/csrc/mixing.hip) against the CPU statement
of the rule, tests/_anderson_ref.AndersonRef (anchored to tests/_scf_ref.ScfRef bit for bit in tests/test_anderson_ref.py).
Grid (12, 2e-3, 25) = 4097 nodes unless stated.

Gates, the ones tests/test_gpu_scf_ref.py holds the linear path to from its second step on: energies 1e-9 relative, eigenvalues
1e-8 Ha + 2e-9 |E|.  (The accelerated trajectory is well conditioned: moving the level solver's output density by +-1 ulp at
random on every step moves the reference's energies of steps 1 .. 12 by at most 1.1e-11 relative and its eigenvalues by at most
1.5e-10 Ha.)  Step counts: the GPU's Anderson run finishes within AndersonRef's count + 2 and within 0.75 of the GPU's linear
count; its final Etotal is within 1e-9 relative of the GPU's linear one.  "Eigenvalues inside the gate" at the finishing step is
taken against AndersonRef at the SAME step number (the reference is stepped two steps past its own finish for that): the two
mixings stop at different distances from the fixed point, so their final eigenvalues are not comparable at 1e-8 Ha.

Every test prints what it observed.  The kernels themselves, stage by stage against an extended reference: tests/test_gpu_mixing_kernels.py.
"""
import ctypes as C
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import _anderson_ref as AR               # noqa: E402
import _scf_ref as SR                    # noqa: E402
import dftatom_amd as D                  # noqa: E402

GRID = (12, 2e-3, 25.0)
BIG = (14, 5e-4, 25.0)

# name, Z, lsda, functional, configuration text (None: Aufbau)
CASES = {
    "Ne LDA": (10, False, D.XC_VWN, None),
    "N LSDA": (7, True, D.XC_VWN, None),
    "Ar 3p5.5 LDA": (18, False, D.XC_VWN, "[Ne] 3s2 3p5.5"),
    "Ne PBE": (10, False, D.XC_PBE, None),
}
NAMES = list(CASES)
IDS = [n.replace(" ", "_") for n in NAMES]


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


def config_of(name):
    Z, lsda, _, text = CASES[name]
    return D.parse_config(Z, text, lsda) if text else D.ion_config(Z, 0, lsda)


def gpu(ctx, grid, name, **kw):
    Z, lsda, fx, text = CASES[name]
    if text:
        kw["config"] = [config_of(name)]
    return D.Scf(ctx, grid, [Z], lsda=lsda, functional=fx, **kw)


@functools.lru_cache(maxsize=None)
def reference(name, m=4, grid=GRID, steps=None):
    """AndersonRef's trajectory, computed once: (its step count to `finished` -- None when `steps` cuts the run short --, the five
    energies of every step, the eigenvalues of every step); it is stepped to two steps past its finish, or for `steps` steps"""
    Z, lsda, fx, _ = CASES[name]
    a, b = SR.config_levels(config_of(name), lsda)
    ref = AR.AndersonRef(Z, a, b, functional={D.XC_VWN: SR.VWN, D.XC_PBE: SR.PBE}[fx], mg_levels=grid[0], delta=grid[1], MaxR=grid[2], m=m)
    en, ev, nfin = [], [], None
    try:
        while len(en) < (steps if steps else (nfin + 2 if nfin else 100)):
            en.append(ref.step())
            ev.append(np.concatenate([ref.levels(sp) for sp in range(2 if lsda else 1)]))
            if ref.finished and nfin is None:
                nfin = len(en)
        assert steps or nfin
    finally:
        ref.close()
    return nfin, en, ev


def snap(scf, atom=0, arrays=range(6)):
    e, fin = scf.energies()
    out = {"energies": e[atom].as_list(), "fin": int(fin[atom]),
           "E": np.concatenate([scf.levels(atom, sp)["E"] for sp in range(2 if scf.lsda else 1)])}
    for w in arrays:
        out[w] = scf.array(w, atom)
    return out


def same_bits(s, t):
    for k in s:
        if k in ("energies", "fin"):
            if s[k] != t[k]:
                return False
        elif not np.array_equal(s[k].view(np.int64), t[k].view(np.int64)):
            return False
    return True


def finite(s):
    return all(np.all(np.isfinite(v)) for v in s.values())


def run(scf, cap=200):
    """steps to `finished` and the last snapshot (density only)"""
    n = 0
    while True:
        assert n < cap, n
        scf.step(want_stats=False)
        n += 1
        if scf.energies()[1][0]:
            return n, snap(scf, 0, arrays=(0,))


def against(got, want_en, want_ev):
    """(energies' largest relative difference / 1e-9, eigenvalues' largest difference / (1e-8 + 2e-9 |E|)), asserted <= 1"""
    re = max(abs(a - b) / abs(b) for a, b in zip(got["energies"], want_en)) / 1e-9
    assert got["E"].shape == want_ev.shape
    rv = float(np.max(np.abs(got["E"] - want_ev) / (1e-8 + 2e-9 * np.abs(want_ev))))
    assert re <= 1.0 and rv <= 1.0, (re, rv, got["energies"], want_en, got["E"], want_ev)
    return re, rv


# ---- 1. the default is untouched ------------------------------------------------------------------------------------------------
class OldOptions(C.Structure):            # dfta_scf_options as it was before the mixing members: 24 bytes
    _fields_ = [(n, C.c_int) for n in ("struct_size", "integrator", "functional", "aufbau", "poisson_mode", "sweep_mode")]


def test_linear_and_short_struct_are_the_default(ctx, grid):
    a = D.Scf(ctx, grid, [10])
    b = D.Scf(ctx, grid, [10], mixing=D.MIX_LINEAR)
    c = D.Scf.__new__(D.Scf)               # the same atom made through the C ABI with a 24-byte options struct
    c.ctx, c.grid, c.Z, c.natoms, c.lsda, c.h = ctx, grid, np.array([10], np.int32), 1, False, D.vp()
    opt = OldOptions(C.sizeof(OldOptions), D.INT_SIMPSON38, D.XC_VWN, D.AUFBAU_REFERENCE, D.POISSON_DEFAULT, D.SWEEPS_EXACT)
    assert C.sizeof(opt) == 24
    ctx.check(ctx.lib.dfta_scf_create_ex(ctx.h, grid.h, 0, 1, c.Z.ctypes.data_as(D.c_ip), 0.5, D.LEVELS_BATCHED, 0, C.cast(C.byref(opt), D.vp),
                                         C.byref(c.h)))
    try:
        for k in range(1, 5):
            for s in (a, b, c):
                s.step(want_stats=False)
            sa = snap(a)
            assert same_bits(sa, snap(b)) and same_bits(sa, snap(c)), k
    finally:
        for s in (a, b, c):
            s.close()


# ---- 2. warm-up ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES[:2], ids=IDS[:2])
def test_warmup_steps_are_the_linear_bits(ctx, grid, name):
    lin, on = gpu(ctx, grid, name), gpu(ctx, grid, name, mixing=D.MIX_ANDERSON)
    try:
        for k in range(1, 5):
            lin.step(want_stats=False)
            on.step(want_stats=False)
            sl, so = snap(lin), snap(on)
            if k <= 3:
                assert same_bits(sl, so), k
            else:
                assert not np.array_equal(sl[0], so[0]) and sl["energies"] != so["energies"]
                print("%s: step 4 moves Etotal by %.2e relative" % (name, abs(so["energies"][0] - sl["energies"][0]) / abs(sl["energies"][0])))
    finally:
        lin.close()
        on.close()


# ---- 3. the first ten steps against the reference --------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES, ids=IDS)
def test_first_ten_steps_vs_reference(ctx, grid, name):
    _, en, ev = reference(name)
    scf = gpu(ctx, grid, name, mixing=D.MIX_ANDERSON)
    worst = [0.0, 0.0]
    try:
        for k in range(10):
            scf.step(want_stats=False)
            s = snap(scf, arrays=(0,))
            assert finite(s) and np.all(s[0] >= 0.0)
            re, rv = against(s, en[k], ev[k])
            worst = [max(worst[0], re), max(worst[1], rv)]
    finally:
        scf.close()
    print("%-14s steps 1..10: energies %.1e of the gate (1e-9 relative), eigenvalues %.1e of the gate (1e-8 Ha + 2e-9 |E|)" % (name, *worst))


# ---- 4. to the stop test ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES, ids=IDS)
def test_finishes_sooner_on_the_same_energy(ctx, grid, name):
    nref, en, ev = reference(name)
    lin, on = gpu(ctx, grid, name), gpu(ctx, grid, name, mixing=D.MIX_ANDERSON)
    try:
        nl, sl = run(lin)
        na, sa = run(on)
        rel = abs(sa["energies"][0] - sl["energies"][0]) / abs(sl["energies"][0])
        print("%-14s linear %d steps, Anderson %d (reference %d), Etotal differs from the linear run's by %.1e relative, eigenvalues by %.1e Ha"
              % (name, nl, na, nref, rel, np.max(np.abs(sa["E"] - sl["E"]))))
        assert na <= nref + 2 and na <= 0.75 * nl, (na, nref, nl)
        assert rel <= 1e-9
        re, rv = against(sa, en[na - 1], ev[na - 1])
        print("%-14s finishing step %d vs the reference's step %d: energies %.1e, eigenvalues %.1e of the gates" % (name, na, na, re, rv))
        for sp in range(2 if on.lsda else 1):
            assert np.all(on.levels(0, sp)["converged"] == 1)
        on.step(want_stats=False)                      # a finished atom is frozen
        assert same_bits(sa, snap(on, 0, arrays=(0,)))
    finally:
        lin.close()
        on.close()


# ---- 5. ring wrap and the extremes of the history --------------------------------------------------------------------------------
def test_history_of_two_wraps(ctx, grid):
    _, en, ev = reference("Ne LDA", m=2, steps=10)
    scf = gpu(ctx, grid, "Ne LDA", mixing=D.MIX_ANDERSON, mix_history=2)
    worst = [0.0, 0.0]
    try:
        for k in range(10):
            scf.step(want_stats=False)
            re, rv = against(snap(scf, arrays=()), en[k], ev[k])
            worst = [max(worst[0], re), max(worst[1], rv)]
    finally:
        scf.close()
    assert max(abs(a - b) / abs(b) for a, b in zip(en[9], reference("Ne LDA")[1][9])) > 1e-9, "m = 2 and m = 4 are different trajectories"
    print("Ne LDA, history 2, steps 1..10: energies %.1e, eigenvalues %.1e of the gates" % tuple(worst))


@pytest.mark.parametrize("kw", [dict(mix_history=8), dict(mix_history=1, mix_warmup=1)], ids=["history8", "history1_warmup1"])
def test_history_extremes_converge_to_the_linear_result(ctx, grid, kw):
    lin, on = gpu(ctx, grid, "Ne LDA"), gpu(ctx, grid, "Ne LDA", mixing=D.MIX_ANDERSON, **kw)
    try:
        nl, sl = run(lin)
        na, sa = run(on)
        rel = abs(sa["energies"][0] - sl["energies"][0]) / abs(sl["energies"][0])
        print("Ne LDA %s: linear %d steps, Anderson %d, Etotal differs by %.1e relative" % (kw, nl, na, rel))
        assert rel <= 1e-9 and finite(sa)
        assert np.all(on.levels(0, 0)["converged"] == 1)
    finally:
        lin.close()
        on.close()


# ---- 6. a batch: every atom as if alone, frozen atoms untouched, runs repeat -----------------------------------------------------
BATCH_Z = [1, 10, 18, 26, 7]
BATCH_CFG = ["1s1", "[Ne]", "[Ne] 3s2 3p5.5", "[Ar] 3d6 4s2", "[He] 2s2 2p3"]


def trajectory(ctx, grid, Z, texts, cap=100):
    cfgs = [D.parse_config(z, t, False) for z, t in zip(Z, texts)]
    scf = D.Scf(ctx, grid, Z, config=cfgs, mixing=D.MIX_ANDERSON)
    steps = []
    try:
        while not steps or not all(s["fin"] for s in steps[-1]):
            assert len(steps) < cap
            scf.step(want_stats=False)
            steps.append([snap(scf, a, arrays=(0,)) for a in range(len(Z))])
        scf.step(want_stats=False)
        steps.append([snap(scf, a, arrays=(0,)) for a in range(len(Z))])
    finally:
        scf.close()
    return steps


def test_batch_atoms_are_bit_identical_to_single_runs(ctx, grid):
    batch = trajectory(ctx, grid, BATCH_Z, BATCH_CFG)
    again = trajectory(ctx, grid, BATCH_Z, BATCH_CFG)
    assert len(batch) == len(again) and all(same_bits(s, t) for p, q in zip(batch, again) for s, t in zip(p, q)), "two runs of the batch differ"
    nfin = []
    for a, (z, t) in enumerate(zip(BATCH_Z, BATCH_CFG)):
        alone = trajectory(ctx, grid, [z], [t])
        n = len(alone) - 1                                # its finishing step (one frozen step follows)
        nfin.append(n)
        assert alone[n - 1][0]["fin"] and (n == 1 or not alone[n - 2][0]["fin"])
        for k, step in enumerate(batch):                  # every step of the batch: the atom's own step, its finishing state afterwards
            assert same_bits(step[a], alone[min(k, n - 1)][0]), (t, k + 1)
    print("batch %s: finishing steps %s, %d steps of the batch" % (BATCH_CFG, nfin, len(batch) - 1))
    assert len(set(nfin)) > 1, "the atoms finish on different steps: frozen atoms sit beside live ones"
    assert len(batch) - 1 == max(nfin)


# ---- 7. several chunks and the odd last node -------------------------------------------------------------------------------------
def test_16385_nodes_vs_reference(ctx):
    _, en, ev = reference("Ne LDA", grid=BIG, steps=6)
    g = D.Grid(ctx, *BIG)
    assert g.N == 16385
    scf = gpu(ctx, g, "Ne LDA", mixing=D.MIX_ANDERSON)
    worst = [0.0, 0.0]
    try:
        for k in range(6):
            scf.step(want_stats=False)
            s = snap(scf, arrays=(0,))
            assert finite(s)
            re, rv = against(s, en[k], ev[k])
            worst = [max(worst[0], re), max(worst[1], rv)]
    finally:
        scf.close()
        g.close()
    print("Ne LDA, 16385 nodes, steps 1..6: energies %.1e, eigenvalues %.1e of the gates" % tuple(worst))


# ---- 8. uniform grid -------------------------------------------------------------------------------------------------------------
def test_uniform_grid(ctx):
    g = D.Grid(ctx, 12, None, 25.0)
    lin, on = D.Scf(ctx, g, [10]), D.Scf(ctx, g, [10], mixing=D.MIX_ANDERSON)
    try:
        for k in range(1, 4):
            lin.step(want_stats=False)
            on.step(want_stats=False)
            assert same_bits(snap(lin), snap(on)), k
        nl, sl = run(lin)
        na, sa = run(on)
        rel = abs(sa["energies"][0] - sl["energies"][0]) / abs(sl["energies"][0])
        print("Ne LDA, uniform grid: linear %d steps, Anderson %d, Etotal differs by %.1e relative" % (nl + 3, na + 3, rel))
        assert na < nl and rel <= 1e-9 and finite(sa)
    finally:
        lin.close()
        on.close()
        g.close()


# ---- 9. the tolerance modes ------------------------------------------------------------------------------------------------------
def test_tolerance_modes(ctx, grid):
    kw = dict(sweep_mode=D.SWEEPS_TOLERANCE, poisson_mode=D.POISSON_TOLERANCE)
    lin, on = gpu(ctx, grid, "Ne LDA", **kw), gpu(ctx, grid, "Ne LDA", mixing=D.MIX_ANDERSON, **kw)
    try:
        nl, sl = run(lin)
        na, sa = run(on)
        rel = abs(sa["energies"][0] - sl["energies"][0]) / abs(sl["energies"][0])
        print("Ne LDA, tolerance modes: linear %d steps, Anderson %d, Etotal differs by %.1e relative" % (nl, na, rel))
        assert na <= 0.75 * nl and rel <= 1e-9
    finally:
        lin.close()
        on.close()


# ---- 10. a failed solve, reached by ordinary input -------------------------------------------------------------------------------
def test_alpha_one_takes_the_linear_step(ctx, grid):
    """alpha = 1: the density never moves, every dF is zero, A = 0 and the first pivot is 0 -- the linear step, history cleared"""
    lin, on = gpu(ctx, grid, "Ne LDA", alpha=1.0), gpu(ctx, grid, "Ne LDA", alpha=1.0, mixing=D.MIX_ANDERSON)
    try:
        for k in range(1, 6):
            lin.step(want_stats=False)
            on.step(want_stats=False)
            sl, so = snap(lin), snap(on)
            assert finite(so) and same_bits(sl, so), k
    finally:
        lin.close()
        on.close()


# ---- 11. validation --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [dict(mixing=2), dict(mixing=-1), dict(mix_history=9), dict(mix_history=-1), dict(mix_warmup=-1), dict(mix_warmup=101)],
                         ids=lambda kw: "%s=%d" % next(iter(kw.items())))
def test_invalid_options_are_rejected(ctx, grid, kw):
    kw.setdefault("mixing", D.MIX_ANDERSON)
    with pytest.raises(D.DftaError):
        D.Scf(ctx, grid, [10], **kw)
    D.Scf(ctx, grid, [10], mixing=D.MIX_ANDERSON, mix_history=8, mix_warmup=100).close()
