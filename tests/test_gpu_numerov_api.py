"""GPU suite (-m gpu): the C ABI of the Numerov layer (dftatom_amd/csrc/numerov_api.cpp) against itself -- the resident potential
against the per-call entries, batches against one trial at a time, host against device boundary values -- and what every entry
refuses.  All comparisons are bit for bit: the entries differ in how the trials travel (grouping, staging blocks, resident tables),
never in what is computed.  Grids: the 16385-node logarithmic grid of the parity tests and the uniform grid of test_gpu_uniform.py;
the potential is golden.make_golden's screened18.
"""
import ctypes as C
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import dftatom_amd as D                 # noqa: E402
from golden.make_golden import GRIDS, screened_potential   # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
ERR_INVALID = 1                         # DFTA_ERR_INVALID (include/dftatom_hip.h)


@pytest.fixture(scope="module")
def ctx(torch_first):
    c = D.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def grid14(ctx):
    g = D.Grid(ctx, *GRIDS["L14"])
    yield g
    g.close()


@pytest.fixture(scope="module")
def ugrid(ctx):
    with open(os.path.join(HERE, "golden", "uniform_meta.json")) as f:
        m = json.load(f)["grid"]
    g = D.Grid(ctx, m["L"], None, m["Rmax"])
    assert g.uniform
    yield g
    g.close()


def _trials(n, seed, lmax=3):
    """n trials of mixed l: energies from -150 to -0.01 Ha in geometric steps (shuffled), node limits 0..5"""
    rng = np.random.RandomState(seed)
    E = -150.0 * (0.01 / 150.0) ** (rng.permutation(n) / max(n - 1, 1))
    return rng.randint(0, lmax + 1, n).astype(np.int32), E, (np.arange(n) % 6).astype(np.int32)


def _same_sweeps(got, want, kind, what):
    names = ("count", "start", "trip") if kind == D.SWEEP_COUNT else ("u0", "start", "trip")
    for k in names:
        assert np.array_equal(got[k], want[k]), (what, k, np.flatnonzero(got[k] != want[k])[:8])


def _resident_against_per_call(ctx, grid, sizes, match_sizes):
    V = screened_potential(grid.r(), 18.0)
    pot = D.Potential(ctx, grid, V)
    try:
        for kind in (D.SWEEP_COUNT, D.SWEEP_ZERO):
            for call, n in enumerate(sizes):             # the scratch grows, then is reused
                l, E, lim = _trials(n, 100 + call)
                _same_sweeps(pot.sweeps(kind, l, E, lim), D.numerov_sweeps(ctx, grid, kind, V, l, E, lim), kind, (kind, n))
        for call, n in enumerate(match_sizes):
            l, E, _ = _trials(n, 200 + call)
            E = np.maximum(E, -20.0)
            psi, mp = pot.match(l, E)
            psi_ref, mp_ref = D.numerov_match(ctx, grid, V, l, E)
            assert np.array_equal(mp, mp_ref) and np.array_equal(psi, psi_ref), n
    finally:
        pot.close()


def test_resident_equals_per_call_logarithmic(ctx, grid14):
    _resident_against_per_call(ctx, grid14, (5, 200, 5), (1, 3, 2))


def test_resident_equals_per_call_uniform(ctx, ugrid):
    _resident_against_per_call(ctx, ugrid, (65,), (3,))


@pytest.fixture(scope="module")
def singles(ctx, grid14):
    """129 trials of l = 1 on two potentials, every one computed by a call of its own (COUNT and ZERO): the reference of the batches"""
    rr = grid14.r()
    V = np.stack([screened_potential(rr, 18.0), screened_potential(rr, 30.0)])
    _, E, lim = _trials(129, 7)
    l = np.ones(129, np.int32)
    ref = {}
    for v in range(2):
        for kind in (D.SWEEP_COUNT, D.SWEEP_ZERO):
            rows = [D.numerov_sweeps(ctx, grid14, kind, V[v], l[t:t + 1], E[t:t + 1], lim[t:t + 1]) for t in range(129)]
            ref[v, kind] = {k: np.concatenate([r[k] for r in rows]) for k in rows[0]}
    return V, l, E, lim, ref


@pytest.mark.parametrize("n", [1, 64, 65, 129])
def test_per_call_batch_equals_single_trials(ctx, grid14, singles, n):
    V, l, E, lim, ref = singles
    vidx = (np.arange(n) * 7 % 3 == 0).astype(np.int32)          # two potentials, interleaved
    for kind in (D.SWEEP_COUNT, D.SWEEP_ZERO):
        one = D.numerov_sweeps(ctx, grid14, kind, V[0], l[:n], E[:n], lim[:n])             # full blocks of one l plus a remainder
        _same_sweeps(one, {k: a[:n] for k, a in ref[0, kind].items()}, kind, ("one potential", n))
        two = D.numerov_sweeps(ctx, grid14, kind, V, l[:n], E[:n], lim[:n], vidx=vidx)
        want = {k: np.where(vidx == 1, ref[1, kind][k][:n], ref[0, kind][k][:n]) for k in ref[0, kind]}
        _same_sweeps(two, want, kind, ("two potentials", n))


def test_host_and_device_boundary_give_the_same_start(ctx, grid14, singles):
    V, l, E, lim, _ = singles
    host = D.numerov_sweeps(ctx, grid14, D.SWEEP_COUNT, V[0], l, E, lim, boundary=D.BOUNDARY_HOST)
    dev = D.numerov_sweeps(ctx, grid14, D.SWEEP_COUNT, V[0], l, E, lim, boundary=D.BOUNDARY_DEVICE)
    assert np.array_equal(host["start"], dev["start"])


def _refused(ctx, call):
    with pytest.raises(D.DftaError, match="status %d:" % ERR_INVALID):
        call()


def test_invalid_l_is_refused_by_every_entry(ctx, grid14, torch_first):
    torch = torch_first
    V = screened_potential(grid14.r(), 18.0)
    l, E, lim = _trials(5, 3)
    bad = l.copy()
    bad[2] = 4
    pot = D.Potential(ctx, grid14, V)
    try:
        before = pot.sweeps(D.SWEEP_COUNT, l, E, lim)
        psi_before = pot.match(l[:2], np.maximum(E[:2], -20.0))
        _refused(ctx, lambda: D.numerov_sweeps(ctx, grid14, D.SWEEP_COUNT, V, bad, E, lim))
        _refused(ctx, lambda: D.numerov_match(ctx, grid14, V, bad, E))
        _refused(ctx, lambda: pot.sweeps(D.SWEEP_COUNT, bad, E, lim))
        _refused(ctx, lambda: pot.sweeps(D.SWEEP_ZERO, bad, E))
        _refused(ctx, lambda: pot.match(bad, E))
        # the device-pointer entry: one group of 5 trials with l = 4 (refused before any pointer is followed)
        dV = torch.tensor(V, dtype=torch.float64, device="cuda")
        dE = torch.tensor(E, dtype=torch.float64, device="cuda")
        dlim = torch.zeros(5, dtype=torch.int32, device="cuda")
        dcount = torch.zeros(5, dtype=torch.int32, device="cuda")
        off, gv, gl = (np.array(a, np.int32) for a in ([0, 5], [0], [4]))
        ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))      # noqa: E731
        rc = ctx.lib.dfta_numerov_sweeps_dev(ctx.h, grid14.h, D.SWEEP_COUNT, 1, dV.data_ptr(), 1, ip(off), ip(gv), ip(gl), dE.data_ptr(),
                                             dlim.data_ptr(), None, None, None, dcount.data_ptr(), None, None, None)
        assert rc == ERR_INVALID
        # the object still works, with the same results
        _same_sweeps(pot.sweeps(D.SWEEP_COUNT, l, E, lim), before, D.SWEEP_COUNT, "after the refusals")
        psi_after = pot.match(l[:2], np.maximum(E[:2], -20.0))
        assert np.array_equal(psi_after[0], psi_before[0]) and np.array_equal(psi_after[1], psi_before[1])
    finally:
        pot.close()


def test_empty_batches_are_ok(ctx, grid14):
    V = screened_potential(grid14.r(), 18.0)
    none_i, none_d = np.zeros(0, np.int32), np.zeros(0)
    pot = D.Potential(ctx, grid14, V)
    try:
        for kind in (D.SWEEP_COUNT, D.SWEEP_ZERO):
            assert len(D.numerov_sweeps(ctx, grid14, kind, V, none_i, none_d, none_i)["count"]) == 0
            assert len(pot.sweeps(kind, none_i, none_d, none_i)["count"]) == 0
        assert D.numerov_match(ctx, grid14, V, none_i, none_d)[0].shape == (0, grid14.N)
        assert pot.match(none_i, none_d)[0].shape == (0, grid14.N)
    finally:
        pot.close()
