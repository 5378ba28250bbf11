"""Independent NumPy reference of the PW92 and PBE functionals (dftatom_amd/csrc/gga.h, gga.hip).

Only the ENERGY density e(rho_a, rho_b, sigma_aa, sigma_ab, sigma_bb) is written out, in the papers' own variables (k_F, k_s, phi,
s, t, A, H); every derivative comes from complex-step differentiation, Im e(x + i h) / h with h = 1e-20 of the variable's scale,
so the reference shares no derivative algebra with the kernels.  The radial part (stencils, flux, divergence, output contract) is
the one of gga.hip, written again over whole arrays.

Thresholds as the library's: a total density below 1e-18 gives zeros; a spin channel below it has no exchange and zeta is then
the constant +-1.  Complex inputs are compared through their real parts.

Every function works in the floating type of its inputs: fp64 arrays give the fp64 reference, np.longdouble arrays (x87 80-bit
where the host has it) the extended one that tests/test_gpu_xc_radial.py measures the kernels and the fp64 reference against.
The irrational constants are formed in that type (consts()), cube roots go through np.cbrt and not through an fp64 exponent 1/3;
the fitted constants of the papers are the doubles the kernels hold.
"""
import types

import numpy as np

PI = np.pi
THRESHOLD = 1e-18
KAPPA = 0.804
BETA = 0.06672455060314922
MU = BETA * PI ** 2 / 3.0
GAMMA = (1.0 - np.log(2.0)) / PI ** 2
FDEN = 2.0 ** (4.0 / 3.0) - 2.0
FZ0 = 8.0 / (9.0 * FDEN)

PW92_PARA = (0.0310907, 0.21370, 7.5957, 3.5876, 1.6382, 0.49294)
PW92_FERRO = (0.01554535, 0.20548, 14.1189, 6.1977, 3.3662, 0.62517)
PW92_STIFF = (0.0168869, 0.11125, 10.357, 3.6231, 0.88026, 0.49671)      # G = -alpha_c

PW92, PBE = 3, 4                  # DFTA_XC_PW92, DFTA_XC_PBE

_CONSTS = {}


def real_type(x):
    """the real floating dtype of an array or dtype (the component type of a complex one)"""
    dt = np.dtype(getattr(x, "dtype", x))
    return np.zeros(0, dt).real.dtype if dt.kind == "c" else (dt if dt.kind == "f" else np.dtype(float))


def complex_type(dt):
    return np.result_type(real_type(dt), np.complex64)


def consts(x):
    """pi, mu, gamma, 2^(4/3) - 2 and f''(0) in the real type of x"""
    dt = real_type(x)
    if dt not in _CONSTS:
        one = dt.type(1)
        pi = 4 * np.arctan(one)
        gamma = (one - np.log(2 * one)) / (pi * pi)
        fden = 2 * np.cbrt(2 * one) - 2
        _CONSTS[dt] = types.SimpleNamespace(PI=pi, MU=BETA * pi * pi / 3, GAMMA=gamma, FDEN=fden, FZ0=8 * one / (9 * fden),
                                            eps=np.finfo(dt).eps)
    return _CONSTS[dt]


# ---- complex-safe elementary functions (accurate real parts, exact first-order imaginary parts) ----------------------------
def _log1p(z):
    z = np.asarray(z)
    if not np.iscomplexobj(z):
        return np.log1p(z)
    return np.log1p(z.real) + 1j * np.arctan2(z.imag, 1.0 + z.real)


def _expm1(z):
    z = np.asarray(z)
    if not np.iscomplexobj(z):
        return np.expm1(z)
    return np.expm1(z.real) * np.cos(z.imag) + (np.cos(z.imag) - 1.0) + 1j * np.exp(z.real) * np.sin(z.imag)


def _cbrt(x):
    """x^(1/3) for a real part >= 0; a complex step goes through to first order"""
    x = np.asarray(x)
    if not np.iscomplexobj(x):
        return np.cbrt(x)
    c = np.cbrt(x.real)
    with np.errstate(divide="ignore", invalid="ignore"):
        return c + 1j * np.where(c > 0, x.imag / (3.0 * c * c), 0.0)


def _p23(x):
    c = _cbrt(x)
    return c * c


def _p43(x):
    return x * _cbrt(x)


# ---- the functionals -------------------------------------------------------------------------------------------------------
def pw92_G(rs, fit):
    """G(rs) = -2A (1 + a1 rs) ln(1 + 1 / (2A (b1 rs^1/2 + b2 rs + b3 rs^3/2 + b4 rs^2)))"""
    A, a1, b1, b2, b3, b4 = fit
    q = b1 * np.sqrt(rs) + b2 * rs + b3 * rs * np.sqrt(rs) + b4 * rs * rs
    return -2.0 * A * (1.0 + a1 * rs) * _log1p(1.0 / (2.0 * A * q))


def pw92_dG(rs, fit):
    """analytic dG/drs (checked against complex steps in test_gga_reference.py)"""
    A, a1, b1, b2, b3, b4 = fit
    q = b1 * np.sqrt(rs) + b2 * rs + b3 * rs * np.sqrt(rs) + b4 * rs * rs
    dq = 0.5 * b1 / np.sqrt(rs) + b2 + 1.5 * b3 * np.sqrt(rs) + 2.0 * b4 * rs
    return -2.0 * A * a1 * np.log1p(1.0 / (2.0 * A * q)) + (1.0 + a1 * rs) * dq / (q * q + q / (2.0 * A))


def spin_f(z):
    return (_p43(1.0 + z) + _p43(1.0 - z) - 2.0) / consts(z).FDEN


def pw92_eps(rs, z):
    """PW92 correlation energy per particle"""
    e0, e1, mac = pw92_G(rs, PW92_PARA), pw92_G(rs, PW92_FERRO), pw92_G(rs, PW92_STIFF)
    f, z4 = spin_f(z), (z * z) * (z * z)
    return e0 - mac * f * (1.0 - z4) / consts(z).FZ0 + (e1 - e0) * f * z4


def pbe_Fx(s2):
    return 1.0 + KAPPA - KAPPA / (1.0 + consts(s2).MU * s2 / KAPPA)


def exchange_unpolarised(n, sigma, gga):
    """e_x of the unpolarised gas: n eps_x^unif(n) F_x(s), s = |grad n| / (2 k_F n)"""
    pi = consts(n).PI
    kf = _cbrt(3.0 * pi * pi * n)
    ex = -3.0 * kf / (4.0 * pi) * n
    if not gga:
        return ex
    return ex * pbe_Fx(sigma / (2.0 * kf * n) ** 2)


def pbe_H(rho, z, sigma, eps):
    k = consts(rho)
    phi = 0.5 * (_p23(1.0 + z) + _p23(1.0 - z))
    kf = _cbrt(3.0 * k.PI * k.PI * rho)
    ks = np.sqrt(4.0 * kf / k.PI)
    t2 = sigma / (2.0 * phi * ks * rho) ** 2
    gp3 = k.GAMMA * phi ** 3
    GAMMA = k.GAMMA
    A = (BETA / GAMMA) / _expm1(-eps / gp3)
    y = A * t2
    D = 1.0 + y + y * y
    # the paper's ratio, and for y > 1 its saturating form (b / A)(1 - 1/D): the same value, but a complex step through the plain
    # ratio of two growing terms loses ~y^2 of its imaginary part to cancellation
    with np.errstate(divide="ignore", invalid="ignore"):
        R = np.where(np.abs(y) > 1.0, BETA / GAMMA / A * (1.0 - 1.0 / D), BETA / GAMMA * t2 * (1.0 + y) / D)
    return gp3 * _log1p(R)


def energy_density(functional, na, nb=None, saa=None, sab=None, sbb=None, part="xlh"):
    """e per volume; nb None: unpolarised (rho = na, sigma = saa).  Arrays (real or complex) of one shape.
    part: the terms to sum -- "x" exchange, "l" local (PW92) correlation, "h" PBE's gradient correction H, "c" = "lh"; default all."""
    gga = functional == PBE
    na = np.asarray(na)
    pol = nb is not None
    dt = np.result_type(na, *(np.asarray(x) for x in (nb, saa, sab, sbb) if x is not None))
    z0 = np.zeros(na.shape, dt)
    nb = np.asarray(nb) + z0 if pol else z0
    saa = np.asarray(saa) + z0 if saa is not None else z0
    sab = np.asarray(sab) + z0 if sab is not None else z0
    sbb = np.asarray(sbb) + z0 if sbb is not None else z0
    na = na + z0
    rho = na + nb if pol else na
    e = np.zeros(na.shape, dt)
    on = rho.real >= THRESHOLD
    if not on.any():
        return e
    na, nb, saa, sab, sbb, rho = (x[on] for x in (na, nb, saa, sab, sbb, rho))
    if pol:
        ex = np.zeros(rho.shape, dt)
        for n, s in ((na, saa), (nb, sbb)):
            m = n.real >= THRESHOLD
            ex[m] += 0.5 * exchange_unpolarised(2.0 * n[m], 4.0 * s[m], gga)
        z = (na - nb) / rho
        z = np.where(nb.real < THRESHOLD, 1.0 + 0.0 * z, np.where(na.real < THRESHOLD, -1.0 + 0.0 * z, z))
        sigma = saa + 2.0 * sab + sbb
    else:
        ex = exchange_unpolarised(rho, saa, gga)
        z = np.zeros_like(rho)
        sigma = saa
    rs = _cbrt(3.0 / (4.0 * consts(rho).PI * rho))
    eps = pw92_eps(rs, z)
    part = part.replace("c", "lh")
    ec = rho * eps if "l" in part else 0.0
    if gga and "h" in part:
        ec = ec + rho * pbe_H(rho, z, sigma, eps)
    e[on] = (ex if "x" in part else 0.0) + ec
    return e


def sweep_inputs(rho, s, zeta):
    """pointwise test inputs: total density rho, reduced gradient s = |grad rho| / (2 k_F rho) of the total density, spin
    polarisation zeta, the gradients split like the densities.  Returns (na, nb, saa, sab, sbb) of the broadcast shape."""
    rho, s, zeta = np.broadcast_arrays(*(np.asarray(x, float) for x in (rho, s, zeta)))
    sigma = (2.0 * (3.0 * PI ** 2 * rho) ** (1.0 / 3.0) * rho * s) ** 2
    a, b = 0.5 * (1.0 + zeta), 0.5 * (1.0 - zeta)
    return rho * a, rho * b, sigma * a * a, sigma * a * b, sigma * b * b


def term_scale(functional, na, nb=None, saa=None, sab=None, sbb=None):
    """per output of pointwise(): |exchange term| + |local correlation term| + |gradient correction term| -- the scale of a
    comparison, since the terms cancel to a small sum in places (exchange against H in d/dsigma at s -> 0, PW92 against H at t -> oo)"""
    parts = [pointwise(functional, na, nb, saa, sab, sbb, part=p) for p in "xlh"]
    return {k: sum(np.abs(p[k]) for p in parts) for k in parts[0]}


def _step(x, scale):
    return 1e-20 * (np.abs(x) + scale)


def pointwise(functional, na, nb=None, saa=None, sab=None, sbb=None, part="xlh"):
    """e and its partial derivatives by complex steps.  Unpolarised: dict(e, dn, dsigma); polarised: dict(e, dna, dnb, dsaa, dsab, dsbb)."""
    pol = nb is not None
    rest = (nb, saa, sab, sbb) if pol else (saa,)
    dt = real_type(np.result_type(*(np.asarray(x) for x in (na,) + rest if x is not None)))
    na = np.asarray(na, dt)
    shape = na.shape
    args = [na] + [np.zeros(shape, dt) + (0.0 if x is None else np.asarray(x, dt)) for x in rest]
    rho = args[0] + (args[1] if pol else 0.0)
    sscale = np.maximum(rho, THRESHOLD) ** (8.0 / 3.0)           # the sigma of s ~ 1
    out = {"e": energy_density(functional, *(args if pol else [args[0], None, args[1]]), part=part).real}
    names = ("dna", "dnb", "dsaa", "dsab", "dsbb") if pol else ("dn", "dsigma")
    for k, name in enumerate(names):
        h = _step(args[k], np.maximum(rho, THRESHOLD) if (k < 2 if pol else k < 1) else sscale)
        pert = [a.astype(complex_type(dt)) for a in args]
        pert[k] = pert[k] + 1j * h
        e = energy_density(functional, *(pert if pol else [pert[0], None, pert[1]]), part=part)
        out[name] = e.imag / h
    return out


# ---- radial grid: the stencils and the output contract of gga.hip ----------------------------------------------------------
def log_grid(levels, delta, Rmax):
    N = 2 ** levels + 1
    i = np.arange(N, dtype=float)
    Rp = Rmax / (np.exp(delta * (N - 1)) - 1.0)
    return Rp * (np.exp(delta * i) - 1.0), Rp * delta * np.exp(delta * i)      # r, dr/di


def d_index(f):
    """df/di along the last axis: 5-point central, second-order one-sided at 0, 1, N-2, N-1.

    Differences first, as gga.hip: neighbouring nodes differ by delta |f|, their difference is (nearly) exact in fp64 and the
    result keeps its digits.  d_index_sums() is the same stencil summed value by value; its partial sums are of size 7 |f| for
    a result of size delta |f| (tests/test_gga_reference.py::test_stencil_form_rounding measures both)."""
    f = np.asarray(f)
    d = np.empty_like(f)
    d[..., 2:-2] = (8.0 * (f[..., 3:-1] - f[..., 1:-3]) - (f[..., 4:] - f[..., :-4])) / 12.0
    for j in (0, 1):
        d[..., j] = (4.0 * (f[..., j + 1] - f[..., j]) - (f[..., j + 2] - f[..., j])) * 0.5
    N = f.shape[-1]
    for j in (N - 2, N - 1):
        d[..., j] = (4.0 * (f[..., j] - f[..., j - 1]) - (f[..., j] - f[..., j - 2])) * 0.5
    return d


def d_index_sums(f):
    """the stencils of d_index in the form that cancels (the library's until the radial tests measured it): NOT the reference"""
    f = np.asarray(f)
    d = np.empty_like(f)
    d[..., 2:-2] = (f[..., :-4] - 8.0 * f[..., 1:-3] + 8.0 * f[..., 3:-1] - f[..., 4:]) / 12.0
    for j in (0, 1):
        d[..., j] = (-3.0 * f[..., j] + 4.0 * f[..., j + 1] - f[..., j + 2]) * 0.5
    N = f.shape[-1]
    for j in (N - 2, N - 1):
        d[..., j] = (3.0 * f[..., j] - 4.0 * f[..., j - 1] + f[..., j - 2]) * 0.5
    return d


def radial(functional, r, cnst, na, nb=None, scale=False, stencil=None):
    """LDA: (Vexc, eexc); LSDA: (res, va, vb, eexc) -- dfta_xc_radial's outputs for densities of shape (..., N), in the floating
    type of the densities.  PBE writes zeros at node 0 and below the threshold; PW92 is pointwise (k_pw92_*: zeros below the
    threshold only -- the SCF's density is 0 at node 0).
    scale=True: also the tuple T of the same layout, the sum of the magnitudes of the terms each output is made of
    (|de/drho| + |dF/dr| + 2 |F| / r, plus |e / rho| for eexc; res: the density-weighted mean of the two spins').
    stencil: d_index (default) or d_index_sums."""
    D = stencil or d_index
    pol = nb is not None
    dt = real_type(np.result_type(np.asarray(na), *([np.asarray(nb)] if pol else [])))
    na = np.asarray(na, dt)
    nb = np.asarray(nb, dt) if pol else None
    r, cnst = np.asarray(r, dt), np.asarray(cnst, dt)
    gga = functional == PBE
    rho = na + nb if pol else na
    fa = fb = None
    if gga:
        ga = D(na) / cnst
        if pol:
            gb = D(nb) / cnst
            p = pointwise(functional, na, nb, ga * ga, ga * gb, gb * gb)
            fa = 2.0 * p["dsaa"] * ga + p["dsab"] * gb
            fb = 2.0 * p["dsbb"] * gb + p["dsab"] * ga
        else:
            p = pointwise(functional, na, None, ga * ga)
            fa = 2.0 * p["dsigma"] * ga
    else:
        p = pointwise(functional, na, nb) if pol else pointwise(functional, na)
    off = rho < THRESHOLD
    if gga:
        off = off | (np.arange(na.shape[-1]) == 0)
    z = lambda x: np.where(off, 0.0, x)                                            # noqa: E731

    def potential(dn, F):
        if not gga:
            return dn, np.abs(dn)
        dF, c = D(F) / cnst, 2.0 * F / r
        return dn - (dF + c), np.abs(dn) + np.abs(dF) + np.abs(c)

    with np.errstate(divide="ignore", invalid="ignore"):
        va, ta = potential(p["dna"] if pol else p["dn"], fa)
        exc = p["e"] / rho
        if not pol:
            out, T = (z(va), z(exc - va)), (z(ta), z(ta + np.abs(exc)))
        else:
            vb, tb = potential(p["dnb"], fb)
            mean, tm = (va * na + vb * nb) / rho, (ta * na + tb * nb) / rho
            out, T = (z(mean), z(va), z(vb), z(exc - mean)), (z(tm), z(ta), z(tb), z(tm + np.abs(exc)))
    return (out, T) if scale else out


def running_max(x, w=8):
    """max of x over j-w .. j+w (a rounding error taken node by node is noise with zeros in it)"""
    out = x.copy()
    for k in range(1, w + 1):
        out[k:] = np.maximum(out[k:], x[:-k])
        out[:-k] = np.maximum(out[:-k], x[k:])
    return out


def energy(functional, r, cnst, na, nb=None):
    """E_xc = 4 pi Int e r^2 dr (trapezoid rule in the grid index)"""
    e = energy_density(functional, np.asarray(na), None if nb is None else np.asarray(nb), *_sigmas(functional, cnst, na, nb)).real
    return 4.0 * consts(e).PI * _trapezoid(e * r * r * cnst)


def potential_integral(r, cnst, v, dn):
    """4 pi Int v dn r^2 dr, same rule"""
    return 4.0 * consts(np.asarray(v)).PI * _trapezoid(v * dn * r * r * cnst)


def _sigmas(functional, cnst, na, nb):
    if functional != PBE:
        return None, None, None
    ga = d_index(np.asarray(na)) / cnst
    if nb is None:
        return ga * ga, None, None
    gb = d_index(np.asarray(nb)) / cnst
    return ga * ga, ga * gb, gb * gb


def _trapezoid(f):
    return np.sum(f, axis=-1) - 0.5 * (f[..., 0] + f[..., -1])


def neon_like(r):
    """a Ne-like density (per volume): 1s^2 and 2s^2 2p^6 Slater shells, exponents 9.64 and 2.88"""
    z1, z2 = 9.64, 2.88
    return 2.0 * z1 ** 3 / PI * np.exp(-2.0 * z1 * r) + 8.0 * (2.0 * z2) ** 5 * r * r * np.exp(-2.0 * z2 * r) / (96.0 * PI)
