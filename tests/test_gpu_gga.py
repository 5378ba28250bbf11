"""GPU suite (-m gpu): the PW92 and PBE functionals (gga.h, gga.hip, the PW92 kernels of xc.hip) and their SCF path.

The reference program has LDA only, so the compiled oracle does not cover these.  What stands in for it: the independent NumPy
reference tests/_gga_ref.py (energy density in the papers' variables, derivatives by complex steps) -- here for the pointwise
kernels, the functional-derivative identity, batch-against-single bit pins and, coarsely, published PBE totals; in
test_gpu_xc_radial.py, evaluated in extended precision, for the radial kernels at their edges; and in test_gpu_scf_ref.py, plugged
into the step reference tests/_scf_ref.py, for whole SCF steps.
"""
import os
import re
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import _gga_ref as R                     # noqa: E402
import dftatom_amd as D                  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
COMPAT = os.path.join(ROOT, "dftatom_amd", "compat")
README_GRID = (14, 5e-4, 25.0)           # the Ar grid of the reference's README
PBE_TOTALS = {2: -2.893, 10: -128.866, 18: -527.346}     # published PBE total energies (Ha), quoted, not measured here


@pytest.fixture(scope="module")
def ctx(torch_first):
    c = D.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def grid(ctx):
    g = D.Grid(ctx, *README_GRID)
    yield g
    g.close()


def _cnst(grid):
    i = np.arange(grid.N, dtype=float)
    return grid.Rp * grid.delta * np.exp(grid.delta * i)


def _run(scf, cap):
    steps = 0
    while steps < cap:
        scf.step(want_stats=False)
        steps += 1
        if scf.energies()[1].all():
            break
    return steps


def _state(scf, k, lsda):
    e, fin = scf.energies()
    arrays = [scf.array(w, k) for w in ((1, 2, 3, 4, 5) if lsda else (0, 3, 5))]
    levels = [scf.levels(k, s)["E"] for s in ((0, 1) if lsda else (0,))]
    return e[k].as_list(), int(fin[k]), [a.view(np.int64).copy() for a in arrays + levels]


def _sweep():
    rho = np.concatenate([np.logspace(-12, 6, 37), [1e-19, 0.0]])
    s = np.concatenate([[0.0], np.logspace(-2, 2, 21)])
    return np.meshgrid(rho, s, indexing="ij")


@pytest.mark.parametrize("functional", [D.XC_PW92, D.XC_PBE])
@pytest.mark.parametrize("zeta", [None, 0.0, 0.3, -0.3, 1.0, -1.0])
def test_pointwise_against_reference(ctx, functional, zeta):
    """e and every partial derivative within 1e-11 of the reference (relative to the sum of the terms' magnitudes); below 1e-18
    exact zeros; nothing non-finite; PBE at sigma = 0 is PW92"""
    RR, SS = _sweep()
    na, nb, saa, sab, sbb = (x.ravel() for x in R.sweep_inputs(RR, SS, 0.0 if zeta is None else zeta))
    if zeta is None:                                   # the unpolarised entry: n, sigma of the total density
        n, sig = na + nb, saa + 2 * sab + sbb
        got = D.xc_pointwise(ctx, functional, n, None, sig)
        ref = R.pointwise(functional, n, None, sig)
        scale = R.term_scale(functional, n, None, sig)
        keys, rho = ("e", "dn", "dsigma"), n
    else:
        got = D.xc_pointwise(ctx, functional, na, nb, saa, sab, sbb)
        ref = R.pointwise(functional, na, nb, saa, sab, sbb)
        scale = R.term_scale(functional, na, nb, saa, sab, sbb)
        keys, rho = ("e", "dna", "dnb", "dsaa", "dsab", "dsbb"), na + nb
    off = rho < 1e-18
    assert off.any() and (~off).any()
    for k in keys:
        assert np.all(np.isfinite(got[k])), k
        assert np.all(got[k][off] == 0.0), k
        err = np.abs(got[k] - ref[k])
        assert np.all(err <= 1e-11 * scale[k]), (k, np.max(err / np.where(scale[k] > 0, scale[k], 1.0)))
    if functional == D.XC_PBE:                          # sigma = 0: the gradient terms vanish
        flat = SS.ravel() == 0.0
        pw = D.xc_pointwise(ctx, D.XC_PW92, n, None) if zeta is None else D.xc_pointwise(ctx, D.XC_PW92, na, nb)
        for k in keys:
            if k.startswith("ds"):
                continue
            a, b = got[k][flat], pw[k][flat]
            assert np.all(np.abs(a - b) <= 1e-14 * np.abs(b)), k


def _vwn_density(ctx, grid, Z, lsda):
    scf = D.Scf(ctx, grid, [Z], lsda=lsda)
    for _ in range(5):
        scf.step(want_stats=False)
    out = (scf.array(1), scf.array(2)) if lsda else (scf.array(0),)
    scf.close()
    return out


@pytest.mark.parametrize("lsda", [False, True])
def test_radial_against_reference_and_identity(ctx, grid, lsda):
    """dfta_xc_radial on an Ar VWN density (5 steps) against the reference's radial scheme, and the functional-derivative identity
    on the GPU's potential"""
    r, cnst = grid.r(), _cnst(grid)
    dens = _vwn_density(ctx, grid, 18, lsda)
    got = D.xc_radial(ctx, grid, D.XC_PBE, *dens)
    ref = R.radial(R.PBE, r, cnst, *dens)
    for g, w in zip(got, ref):
        assert np.all(np.isfinite(g))
        assert np.all(np.abs(g - w) <= 1e-9 * np.abs(w) + 1e-12), np.max(np.abs(g - w) / (np.abs(w) + 1e-12))
    ms = ctx.last_kernel_ms()
    assert ms > 0
    # identity: dE/dh along a bump == 4 pi Int v dn r^2 dr, with v from the GPU
    dn = 0.05 * np.exp(-((r - 1.0) / 0.15) ** 2)
    h = 1e-3
    v = got[1] if lsda else got[0]
    nb = dens[1] if lsda else None
    lhs = (R.energy(R.PBE, r, cnst, dens[0] + h * dn, nb) - R.energy(R.PBE, r, cnst, dens[0] - h * dn, nb)) / (2 * h)
    rhs = R.potential_integral(r, cnst, v, dn)
    assert abs(lhs - rhs) <= 1e-8 * abs(rhs), (lhs, rhs)


@pytest.mark.parametrize("Z", [2, 10, 18])
def test_pbe_scf_literature(ctx, grid, Z):
    scf = D.Scf(ctx, grid, [Z], functional=D.XC_PBE)
    n = _run(scf, 100)
    e, fin = scf.energies()
    scf.close()
    assert fin[0], (Z, n)
    assert abs(e[0].Etotal - PBE_TOTALS[Z]) <= 5e-3, (Z, e[0].Etotal)


def test_pbe_lsda_hydrogen_and_closed_shell(ctx, grid):
    h = D.Scf(ctx, grid, [1], lsda=True, functional=D.XC_PBE)
    _run(h, 150)
    e, fin = h.energies()
    h.close()
    assert fin[0] and abs(e[0].Etotal + 0.500) <= 1e-3, e[0].Etotal
    lda = D.Scf(ctx, grid, [10], functional=D.XC_PBE)
    lsd = D.Scf(ctx, grid, [10], lsda=True, functional=D.XC_PBE)
    _run(lda, 100)
    _run(lsd, 150)
    ea, eb = lda.energies()[0][0].as_list(), lsd.energies()[0][0].as_list()
    assert lda.energies()[1][0] and lsd.energies()[1][0]
    for a, b in zip(ea, eb):
        assert abs(a - b) <= 1e-9 * abs(a), (ea, eb)
    la, lb = lda.levels(0, 0)["E"], lsd.levels(0, 0)["E"]
    assert np.max(np.abs(la - lb)) <= 1e-8 and np.max(np.abs(la - lsd.levels(0, 1)["E"])) <= 1e-8
    lda.close()
    lsd.close()


@pytest.mark.parametrize("Zs,lsda", [([2, 10, 18, 36], False), ([1, 7, 10], True)])
def test_batch_bits_equal_single_atoms(ctx, grid, Zs, lsda):
    """a PBE batch == each atom alone, bit for bit, at every step (energies, eigenvalues, densities, potentials, U, finished flags),
    the steps after an atom has finished (frozen) included"""
    cap = 150 if lsda else 100
    alone = []
    for Z in Zs:
        one = D.Scf(ctx, grid, [Z], lsda=lsda, functional=D.XC_PBE)
        hist = []
        for _ in range(cap):
            one.step(want_stats=False)
            hist.append(_state(one, 0, lsda))
            if hist[-1][1]:
                break
        one.close()
        assert hist[-1][1], Z
        alone.append(hist)
    batch = D.Scf(ctx, grid, Zs, lsda=lsda, functional=D.XC_PBE)
    nsteps = max(len(h) for h in alone)
    for step in range(nsteps):
        batch.step(want_stats=False)
        for k, hist in enumerate(alone):
            want = hist[min(step, len(hist) - 1)]
            got = _state(batch, k, lsda)
            assert got[0] == want[0] and got[1] == want[1], (Zs[k], step)
            assert all(np.array_equal(a, b) for a, b in zip(got[2], want[2])), (Zs[k], step)
    assert batch.energies()[1].all()
    batch.close()


@pytest.mark.parametrize("uniform", [False, True])
def test_pw92_scf(ctx, uniform):
    g = D.Grid(ctx, 16, None, 25.0) if uniform else D.Grid(ctx, *README_GRID)
    for Z in (10, 18):
        E = {}
        for fx in (D.XC_VWN, D.XC_PW92):
            scf = D.Scf(ctx, g, [Z], functional=fx)
            n = _run(scf, 100)
            e, fin = scf.energies()
            scf.close()
            assert fin[0], (Z, fx, n)
            E[fx] = e[0].Etotal
        d = abs(E[D.XC_PW92] - E[D.XC_VWN])
        assert 0 < d <= 5e-4 * Z, (Z, E)
    g.close()


def test_refusals(ctx):
    ug = D.Grid(ctx, 12, None, 25.0)
    with pytest.raises(D.DftaError, match="logarithmic grid"):
        D.Scf(ctx, ug, [10], functional=D.XC_PBE)
    with pytest.raises(D.DftaError, match="logarithmic grid"):
        D.xc_radial(ctx, ug, D.XC_PBE, np.ones(ug.N))
    with pytest.raises(D.DftaError, match="functional"):
        D.Scf(ctx, ug, [10], functional=5)
    with pytest.raises(D.DftaError, match="LDA only"):
        D.Scf(ctx, ug, [10], lsda=True, functional=D.XC_CHACHIYO)
    ug.close()


def _cli(*args, timeout=900):
    exe = os.path.join(COMPAT, "dftatom_cli")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-C", COMPAT])
    return subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=timeout)


def test_cli_xc():
    pbe = _cli(10, 14, 0.5, 25, 0.0005, 0, "--xc=pbe")
    assert pbe.returncode == 0, pbe.stderr[-2000:]
    assert "Finished!" in pbe.stdout
    etot = float(re.findall(r"Etotal = (-?\d+\.\d+)", pbe.stdout)[-1])
    assert abs(etot - PBE_TOTALS[10]) <= 5e-3, etot
    plain = _cli(10, 14, 0.5, 25, 0.0005, 0)
    vwn = _cli(10, 14, 0.5, 25, 0.0005, 0, "--xc=vwn")
    assert plain.returncode == 0 and vwn.returncode == 0
    assert vwn.stdout == plain.stdout
    bad = _cli(10, 14, 0.5, 25, 0.0005, 0, "--xc=bogus")
    assert bad.returncode != 0 and "usage" in bad.stderr
