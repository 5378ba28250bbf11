"""CPU suite: the NumPy reference of the PW92 / PBE functionals (tests/_gga_ref.py) on its own -- its analytic pieces against complex
steps, PW92 against the VWN fit of the oracle, the functional-derivative identity of the radial scheme -- and the public constants.

The reference program has no GGA, so there is no oracle for PBE.  What stands in for one: this NumPy reference, here checked on its
own and -- evaluated in np.longdouble -- used as the yardstick of the radial kernels in test_gpu_xc_radial.py; test_gpu_gga.py holds
the pointwise kernels and the SCF to it.  test_stencil_form_rounding records why the difference stencils are written differences
first."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import _gga_ref as R
import dftatom_amd as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cstep(f, x):
    h = 1e-20 * np.abs(x)
    return f(x + 1j * h).imag / h


def _rel(a, b):
    return np.max(np.abs(a - b) / np.abs(b))


def test_analytic_pieces_match_complex_steps():
    rs = np.logspace(-2, 2, 301)
    for fit in (R.PW92_PARA, R.PW92_FERRO, R.PW92_STIFF):
        assert _rel(R.pw92_dG(rs, fit), _cstep(lambda x: R.pw92_G(x, fit), rs)) <= 1e-12
    # Slater exchange potential -(3 n / pi)^(1/3), and through the whole pointwise path (PW92, sigma ignored)
    n = np.logspace(-12, 6, 181)
    assert _rel(-(3.0 * n / np.pi) ** (1.0 / 3.0), _cstep(lambda x: R.exchange_unpolarised(x, 0.0, False), n)) <= 1e-12
    rsn = (3.0 / (4.0 * np.pi * n)) ** (1.0 / 3.0)
    eps = R.pw92_G(rsn, R.PW92_PARA)
    v_analytic = -(3.0 * n / np.pi) ** (1.0 / 3.0) + eps - rsn / 3.0 * R.pw92_dG(rsn, R.PW92_PARA)
    assert _rel(R.pointwise(R.PW92, n)["dn"], v_analytic) <= 1e-12
    # PBE enhancement factor dF_x/ds^2 = mu / (1 + mu s^2 / kappa)^2
    s2 = np.logspace(-6, 4, 101)
    assert _rel(_cstep(R.pbe_Fx, s2), R.MU / (1.0 + R.MU * s2 / R.KAPPA) ** 2) <= 1e-12
    # spin interpolation f'(zeta) = 4/3 ((1+z)^(1/3) - (1-z)^(1/3)) / (2^(4/3) - 2)
    z = np.linspace(-0.95, 0.95, 39)
    z = z[z != 0]
    fp = 4.0 / 3.0 * (np.cbrt(1.0 + z) - np.cbrt(1.0 - z)) / R.FDEN
    h = 1e-20
    assert _rel(R.spin_f(z + 1j * h).imag / h, fp) <= 1e-12
    # f''(0) of the interpolation is the constant the PW92 form divides by
    assert abs(R.FZ0 - 4.0 / 9.0 * 2.0 / R.FDEN) <= 1e-15 * R.FZ0


def test_pw92_close_to_vwn():
    """PW92 and VWN fit the same Ceperley-Alder data: eps_xc differs by well under 1 mHa for rs in [0.01, 100], zeta = 0 and 1"""
    import _oracle as O
    o = O.oracle()
    rs = np.logspace(-2, 2, 401)
    n = 3.0 / (4.0 * np.pi * rs ** 3)
    sz = n.size
    v, e = np.zeros(sz), np.zeros(sz)
    o.dfo_vwn_vexc(O.dp(n), O.dp(v), sz)
    o.dfo_vwn_eexcdif(O.dp(n), O.dp(e), sz)
    pw = R.pointwise(R.PW92, n)["e"] / n
    d0 = np.max(np.abs(pw - (v + e)))
    zero = np.zeros(sz)
    res, va, vb, el = (np.zeros(sz) for _ in range(4))
    o.dfo_vwn_vexc_lsda(O.dp(n), O.dp(zero), O.dp(res), O.dp(va), O.dp(vb), sz)
    o.dfo_vwn_eexcdif_lsda(O.dp(n), O.dp(zero), O.dp(el), sz)
    pw1 = R.pointwise(R.PW92, n, zero)["e"] / n
    d1 = np.max(np.abs(pw1 - (res + el)))
    assert 0 < d0 < 1e-3 and 0 < d1 < 1e-3, (d0, d1)


def _bump(r, r0=1.0, w=0.15):
    return np.exp(-((r - r0) / w) ** 2)


@pytest.mark.parametrize("levels,delta", [(14, 5e-4), (17, 1e-4)])
def test_functional_derivative_identity(levels, delta):
    """dE/dh along a Gaussian bump equals 4 pi Int v drho r^2 dr for the reference's radial scheme (LDA and LSDA paths)"""
    r, cnst = R.log_grid(levels, delta, 25.0)
    rho = R.neon_like(r)
    dr = 0.05 * _bump(r)
    h = 1e-3
    for pol in (False, True):
        if pol:
            na, nb = 0.55 * rho, 0.45 * rho
            out = R.radial(R.PBE, r, cnst, na, nb)
            va = out[1]
            Ep = R.energy(R.PBE, r, cnst, na + h * dr, nb)
            Em = R.energy(R.PBE, r, cnst, na - h * dr, nb)
        else:
            va = R.radial(R.PBE, r, cnst, rho)[0]
            Ep = R.energy(R.PBE, r, cnst, rho + h * dr)
            Em = R.energy(R.PBE, r, cnst, rho - h * dr)
        lhs = (Ep - Em) / (2 * h)
        rhs = R.potential_integral(r, cnst, va, dr)
        assert abs(lhs - rhs) <= 1e-8 * abs(rhs), (pol, lhs, rhs)
        # without the 2F/r part of the divergence the identity fails by orders of magnitude
        if not pol:
            ga = R.d_index(rho) / cnst
            p = R.pointwise(R.PBE, rho, None, ga * ga)
            F = 2.0 * p["dsigma"] * ga
            wrong = va + 2.0 * F / np.where(r > 0, r, 1.0)
            assert abs(R.potential_integral(r, cnst, wrong, dr) - lhs) > 1e-5 * abs(rhs)


LD = np.longdouble
HEADLINE_GRIDS = [(14, 5e-4, 25.0), (17, 1e-4, 50.0), (20, 1.25e-5, 50.0)]


def _neon_lsda(levels, delta, Rmax):
    r, cnst = R.log_grid(levels, delta, Rmax)
    rho = R.neon_like(r)
    return r, cnst, 0.55 * rho, 0.45 * rho


@pytest.mark.parametrize("levels,delta,Rmax", HEADLINE_GRIDS)
def test_stencil_form_rounding(levels, delta, Rmax):
    """Why d_index (here and in gga.hip) takes differences first.  v_a of a Ne-like LSDA density, fp64 against np.longdouble, largest
    relative difference over the nodes with rho >= 1e-17 (in the last decade above the 1e-18 threshold v_a is a remainder of
    cancelling terms and a relative figure says nothing):
        differences first   1.4e-13 / 4.0e-12 / 3.6e-11   at 16 385 / 131 073 / 1 048 577 nodes   (gate 1e-10)
        summed by value     1.8e-10 / 6.0e-07 / 3.9e-05                                           (> 1e-7 from 131 073 nodes on)
    Summed by value, (f[k-2] - 8 f[k-1] + 8 f[k+1] - f[k+2]) / 12 goes through partial sums of size 7 |f| for a result of size
    delta |f|, and the divergence of the flux divides by delta once more."""
    assert np.finfo(LD).eps < 1.2e-19, "needs an extended np.longdouble"
    r, cnst, na, nb = _neon_lsda(levels, delta, Rmax)
    ext = R.radial(R.PBE, r, cnst, na.astype(LD), nb.astype(LD))[1]
    assert ext.dtype == LD
    m = (na + nb) >= 1e-17
    m[0] = False
    rel = lambda v: float(np.max(np.abs(v[m] - ext[m]) / np.abs(ext[m])))          # noqa: E731
    first = rel(R.radial(R.PBE, r, cnst, na, nb)[1])
    summed = rel(R.radial(R.PBE, r, cnst, na, nb, stencil=R.d_index_sums)[1])
    print("levels %d: differences first %.2e, summed by value %.2e" % (levels, first, summed))
    assert first <= 1e-10, first
    assert summed > 50 * first
    if levels >= 17:
        assert summed > 1e-7, summed


@pytest.mark.parametrize("levels,delta,Rmax", HEADLINE_GRIDS)
def test_input_noise_sensitivity_is_recorded(levels, delta, Rmax):
    """A measurement, no gate on its size: how far one ulp of noise on the input density moves v_a (extended arithmetic throughout, so
    this is conditioning, not rounding): about 1e-9 / 4e-6 / 2e-3 relative at the three sizes -- a second derivative on a grid
    of spacing delta amplifies by 1 / delta^2 whatever the stencil's form.  Taken on six windows of N / 16 nodes."""
    r, cnst, na, nb = _neon_lsda(levels, delta, Rmax)
    rng = np.random.default_rng(levels)
    N, worst = r.size, 0.0
    W = N // 16
    for start in np.linspace(0, N - W, 6).astype(int):
        w = slice(start, start + W)
        a, b = na[w], nb[w]
        if (a + b).min() < 1e-17:
            continue
        a1 = a + np.spacing(a) * rng.integers(-1, 2, a.size)
        v0 = R.radial(R.PBE, r[w], cnst[w], a.astype(LD), b.astype(LD))[1][8:-8]
        v1 = R.radial(R.PBE, r[w], cnst[w], a1.astype(LD), b.astype(LD))[1][8:-8]
        worst = max(worst, float(np.max(np.abs(v1 - v0) / np.abs(v0))))
    print("levels %d: one ulp of input noise moves v_a by %.1e relative" % (levels, worst))
    assert worst > 0 and np.isfinite(worst)


def test_public_constants():
    src = open(os.path.join(ROOT, "include", "dftatom_hip.h")).read()
    vals = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define\s+DFTA_(XC_\w+|ABI_VERSION)\s+(\d+)", src)}
    assert vals["XC_PW92"] == D.XC_PW92 == R.PW92 == 3
    assert vals["XC_PBE"] == D.XC_PBE == R.PBE == 4
    assert vals["ABI_VERSION"] == D.ABI_VERSION == 7
    for name in ("dfta_xc_pointwise", "dfta_xc_radial"):
        assert name in D.SIGNATURES
