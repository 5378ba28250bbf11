"""Reference for the spherical Bessel functions and the Bessel transforms of include/dftatom_hip.h (dfta_sph_bessel,
dfta_bessel_transform, dfta_scf_form_factors, dfta_scf_momentum_orbitals), in np.longdouble, with the magnitudes that the rounding
bounds of tests/test_gpu_bessel.py are stated in, a float64 model of the header's two branches of j_l, and the closed forms of
hydrogen-like atoms.  No GPU, no library.

    DENSITY  out = 4 pi      Q[f r^2 j_l(q r) s]        ORBITAL  out = sqrt(2/pi) Q[f r j_l(q r) s]       x_i = q r_i rounded once in double

j_l, 0 <= l <= 4, x >= 0 (the header's definition; the reference runs the same two branches in longdouble, the series with 30 terms):
    x == 0: 1 (l = 0), 0 (l >= 1);   l = 0: sin x / x;
    l >= 1, x < 3:  x^l / (2l+1)!! Sum_k t_k,  t_k = t_{k-1} (-x^2 / 2) / (k (2l + 2k + 1));
    l >= 1, x >= 3: j_0 = sin / x, j_1 = (j_0 - cos) / x, j_{k+1} = ((2k+1) / x) j_k - j_{k-1}.

T_l(x), the sum of the magnitudes of the terms of the branch taken: |sin x| / x (l = 0); x^l / (2l+1)!! Sum |t_k| (series);
T_0 = |sin| / x, T_1 = (T_0 + |cos|) / x, T_{k+1} = ((2k+1) / x) T_k + T_{k-1} (recurrence).

jl_roundings: c of the bound c eps T_l(x) of the DEVICE's j_l, counted from sph_bessel of dftatom_amd/csrc/bessel.hip (first order in eps).
    l = 0:       the device's sin 2 ulp, the division 1: 3.
    series:      term k is the prefactor times z_1 .. z_k, z_j = y c_j.  Per factor: c_j rounded 1, y = (x x)(-1/2) 1, the product y c_j 1;
                 per nesting level the product with h 1 and the addition 1: 5 k <= 5 (SERIES_TERMS - 1).  The prefactor: l - 1 products
                 for x^l, d_l rounded 1, the product 1, the product with h 1: l + 2.
    recurrence:  j_0 = sin rx: sin 2, rx 1, the product 1: 4 on T_0.  j_1 = (j_0 - cos) rx: 4 |sin| / x + 2 |cos| (cos: 2 ulp) + the
                 subtraction 1 on both, then rx 1 and the product 1: 7 on T_1.  A step up adds rx 1, (2k+1) rx 1, the product 1 on its
                 first term and the subtraction 1 on all: c_{k+1} = c_k + 4.
An absolute 2^-1022 is added per value: below the normal range of float64 a result has no relative precision (x = 1e-300, l >= 2: the
device's 0 against 1e-600 in longdouble).

transform_roundings: c of the transform's own arithmetic on a term g_i j_l(x_i), counted from k_bessel_transform: f r 1, r again 1
(DENSITY only), the table s (Rp delta, exp, product) 3, times s 1, the weight (2 or 3) 1, g j 1; the lane's chain: 4 adds per tile of
1024 nodes; six xor-shuffle levels, the tree (w0 + w1) + (w2 + w3) 2, the factor 3/8 1, the constant K rounded 1 and its product 1.
"""
import math

import numpy as np

from _orb_ref import GRIDS, grid, hydrogenic_u, weights          # noqa: F401  (re-exported for the tests)

LD = np.longdouble
EPS = 2.0 ** -52
TINY = 2.0 ** -1022
BT_DENSITY, BT_ORBITAL = 0, 1
LMAX = 4
SWITCH = 3.0                     # the header's switch between the two branches
SERIES_TERMS = 14                # the device's: k = 0 .. 13
SERIES_TERMS_LD = 30             # the reference's
DFACT = (1, 3, 15, 105, 945)     # (2l+1)!!
TILE = 1024

PI_LD = LD("3.14159265358979323846264338327950288419716939937510")
K_LD = {BT_DENSITY: 4 * PI_LD, BT_ORBITAL: np.sqrt(2 / PI_LD)}


# ---- j_l ------------------------------------------------------------------------------------------------------------------------------
def _branches(l, x):
    """(zero, series, rec): masks of the branch the header takes at each x (l >= 1; l = 0: rec stands for sin x / x)"""
    zero = x == 0
    if l == 0:
        return zero, np.zeros_like(zero), ~zero
    ser = ~zero & (x < SWITCH)
    return zero, ser, ~zero & ~ser


def jl(l, x):
    """(j_l(x), T_l(x)) in longdouble, elementwise; x: float64 or longdouble, >= 0"""
    x = np.atleast_1d(np.asarray(x, dtype=LD))
    j, T = np.zeros(x.shape, dtype=LD), np.zeros(x.shape, dtype=LD)
    zero, ser, rec = _branches(l, x)
    j[zero] = T[zero] = LD(1 if l == 0 else 0)
    if np.any(ser):
        xs = x[ser]
        y = -xs * xs / 2
        t = np.ones_like(xs)
        S, A = t.copy(), t.copy()
        for k in range(1, SERIES_TERMS_LD):
            t = t * y / LD(k * (2 * l + 2 * k + 1))
            S, A = S + t, A + np.abs(t)
        pref = xs ** l / LD(DFACT[l])
        j[ser], T[ser] = pref * S, pref * A
    if np.any(rec):
        xr = x[rec]
        s, c = np.sin(xr), np.cos(xr)
        jm, Tm = s / xr, np.abs(s) / xr
        if l == 0:
            j[rec], T[rec] = jm, Tm
        else:
            jk, Tk = (jm - c) / xr, (Tm + np.abs(c)) / xr
            for k in range(1, l):
                jm, jk = jk, LD(2 * k + 1) / xr * jk - jm
                Tm, Tk = Tk, LD(2 * k + 1) / xr * Tk + Tm
            j[rec], T[rec] = jk, Tk
    return j, T


def jl_prime_x(l, x):
    """|x j_l'(x)| in longdouble: j_0' = -j_1, j_l' = j_{l-1} - (l+1) j_l / x"""
    x = np.atleast_1d(np.asarray(x, dtype=LD))
    if l == 0:
        return np.abs(x * jl(1, x)[0])
    return np.abs(x * jl(l - 1, x)[0] - (l + 1) * jl(l, x)[0])


def jl_roundings(l, x):
    """c per argument (see the module's docstring); 0 at x == 0, where the value is exact"""
    x = np.atleast_1d(np.asarray(x, dtype=LD))
    zero, ser, rec = _branches(l, x)
    c = np.zeros(x.shape)
    c[ser] = 5 * (SERIES_TERMS - 1) + l + 2
    c[rec] = 3 if l == 0 else 7 + 4 * (l - 1)
    return c


def jl_bound(l, x):
    """the gate of the device's j_l per argument: c eps T_l(x) + 2^-1022 (0 at x == 0)"""
    x = np.atleast_1d(np.asarray(x, dtype=LD))
    b = jl_roundings(l, x) * EPS * jl(l, x)[1].astype(np.float64) + TINY
    b[x == 0] = 0.0
    return b


def e_l(l, x):
    """the scale the float64 model's error is recorded in: x^l / (2l+1)!! below the switch, 1 / x from it on"""
    x = np.asarray(x, dtype=np.float64)
    return np.where(x < SWITCH, x ** l / DFACT[l], 1 / np.where(x > 0, x, 1.0))


C64 = [[1.0 / DFACT[l]] + [1.0 / (k * (2.0 * l + 2.0 * k + 1.0)) for k in range(1, SERIES_TERMS)] for l in range(LMAX + 1)]


def jl_model(l, x, switch=SWITCH, terms=SERIES_TERMS):
    """the header's j_l in float64 NumPy, operation for operation as sph_bessel of bessel.hip (the host's sin and cos in place of the
    device's); switch / terms: other choices, for the test that fixes them"""
    x = np.atleast_1d(np.asarray(x, dtype=np.float64))
    out = np.zeros(x.shape)
    zero = x == 0
    out[zero] = 1.0 if l == 0 else 0.0
    if l == 0:
        out[~zero] = np.sin(x[~zero]) / x[~zero]
        return out
    ser = ~zero & (x < switch)
    rec = ~zero & ~ser
    c = [1.0 / DFACT[l]] + [1.0 / (k * (2.0 * l + 2.0 * k + 1.0)) for k in range(1, terms)]
    xs = x[ser]
    y = (xs * xs) * -0.5
    h = 1.0 + y * c[terms - 1]
    for k in range(terms - 2, 0, -1):
        h = 1.0 + (y * c[k]) * h
    p = xs.copy()
    for _ in range(1, l):
        p = p * xs
    with np.errstate(under="ignore"):
        out[ser] = (p * c[0]) * h
    xr = x[rec]
    s, co = np.sin(xr), np.cos(xr)
    rx = 1.0 / xr
    jm = s * rx
    jk = (jm - co) * rx
    for k in range(1, l):
        jm, jk = jk, (float(2 * k + 1) * rx) * jk - jm
    out[rec] = jk
    return out


def ladder():
    """the arguments of the j_l checks: 1e-8 .. 1e4 dense in the logarithm, the neighbourhood of the switch dense in x, the doubles on
    both sides of the switch"""
    lo, hi = np.nextafter(SWITCH, 0.0), np.nextafter(SWITCH, 10.0)
    return np.unique(np.concatenate([np.geomspace(1e-8, 1e4, 1201), np.linspace(2.0, 4.0, 401), [lo, SWITCH, hi]]))


# MEASURED largest error of jl_model against jl over ladder(), in units of eps e_l(x), per l: (below the switch, from the switch on),
# rounded up to two digits.  tests/test_bessel_ref.py holds each to [measured, 1.2 x measured]; it also shows what other switch points
# and term counts would give: a switch at 2 costs l = 4 two digits below it (the recurrence at x = 2: 286), a switch at 4 costs l = 1
# one above 3 (the series at x = 4: 21.5); 12 terms leave 9.6 for l = 1, 13 reach the figures below, the 14th is spare.  l = 0 has one
# branch (sin x / x on both sides).  In relative terms the model stays within 7e-15 of j_l over the whole ladder.
MODEL_ERROR = {0: (0.7, 0.6), 1: (1.3, 0.91), 2: (1.3, 2.0), 3: (1.6, 3.0), 4: (2.1, 4.8)}


# ---- the transform ----------------------------------------------------------------------------------------------------------------------
def transform_roundings(kind, N):
    tiles = (N + TILE - 1) // TILE
    return (8 if kind == BT_DENSITY else 7) + 4 * tiles + 6 + 2 + 3


def transform(kind, l, f, r, s, q):
    """(value, bound) of one (row, q): the transform in longdouble on float64 inputs f, r, q (s: longdouble), x = q r rounded once in
    float64, and the gate eps Sum_i |g_i| (c |j_l(x_i)| + c_j T_l(x_i) + |x_i j_l'(x_i)|) + 2^-1022 (Sum |g_i| + 1), with g_i the
    weighted term including 3/8 and the constant factor"""
    f64, r64 = np.asarray(f, dtype=np.float64), np.asarray(r, dtype=np.float64)
    with np.errstate(under="ignore"):
        x = (np.float64(q) * r64).astype(LD)
    fl, rl, s = f64.astype(LD), r64.astype(LD), np.asarray(s, dtype=LD)
    N = len(r64)
    t = fl * rl * rl * s if kind == BT_DENSITY else fl * rl * s
    g = weights(N) * t * K_LD[kind]
    j, T = jl(l, x)
    value = np.sum(g * j)
    ag = np.abs(g)
    c = transform_roundings(kind, N)
    per_node = c * np.abs(j) + jl_roundings(l, x) * T + jl_prime_x(l, x)
    bound = EPS * float(np.sum(ag * per_node)) + TINY * (float(np.sum(ag)) + 1.0)
    return value, bound


def transform_rows(kind, l, F, r, s, q):
    """values (nrow, nq) in longdouble and bounds (nrow, nq) in float64"""
    F = np.atleast_2d(F)
    V, B = np.zeros((F.shape[0], len(q)), dtype=LD), np.zeros((F.shape[0], len(q)))
    for a in range(F.shape[0]):
        for m, qm in enumerate(q):
            V[a, m], B[a, m] = transform(kind, int(l[a]), F[a], r, s, qm)
    return V, B


# ---- closed forms of a hydrogen-like atom of charge Z -----------------------------------------------------------------------------------
ZREF = 10
QS = (0.5, 3.0, 20.0, 60.0)
FORM_ORBITALS = ((1, 0), (2, 0), (2, 1))                           # (n, l), n the principal quantum number
MOMENTUM_ORBITALS = ((1, 0), (2, 0), (2, 1), (3, 2), (4, 3))


def form_factor_closed(n, l, Z, q):
    """Int u_nl^2 j_0(q r) dr, the spherically averaged form factor of one electron in (n, l): 1s, 2s, 2p"""
    q = LD(q)
    if (n, l) == (1, 0):
        a = q / (2 * LD(Z))
        return 1 / (1 + a * a) ** 2
    a = q / LD(Z)
    if (n, l) == (2, 0):
        return (1 - 3 * a ** 2 + 2 * a ** 4) / (1 + a * a) ** 4
    if (n, l) == (2, 1):
        return (1 - a * a) / (1 + a * a) ** 4
    raise ValueError((n, l))


def gegenbauer(m, a, x):
    """C_m^a(x) by its three-term recurrence"""
    x = LD(x)
    c0, c1 = LD(1), 2 * LD(a) * x
    if m == 0:
        return c0
    for k in range(2, m + 1):
        c0, c1 = c1, (2 * x * (k + a - 1) * c1 - (k + 2 * a - 2) * c0) / k
    return c1


def momentum_closed(n, l, Z, p):
    """Podolsky-Pauling: R~_nl(p) up to the orbital's overall sign (a convention: the tests fix it at the smallest q > 0)"""
    P = LD(p) / LD(Z)
    n2P2 = LD(n * n) * P * P
    pref = np.sqrt(LD(2) / PI_LD * LD(math.factorial(n - l - 1)) / LD(math.factorial(n + l))) * LD(n * n) * LD(2) ** (2 * l + 2) * LD(math.factorial(l))
    return LD(Z) ** LD(-1.5) * pref * (LD(n) * P) ** l / (n2P2 + 1) ** (l + 2) * gegenbauer(n - l - 1, l + 1, (n2P2 - 1) / (n2P2 + 1))


def density_row(u, r):
    """u^2 / (4 pi r^2) in longdouble (0 at r = 0, where the transform's factor r^2 is 0 anyway): the row whose DENSITY transform with
    l = 0 is Q[u^2 j_0 s]"""
    u, r = np.asarray(u, dtype=LD), np.asarray(r, dtype=LD)
    rho = np.zeros(len(r), dtype=LD)
    rho[1:] = u[1:] * u[1:] / (4 * PI_LD * r[1:] * r[1:])
    return rho


CLOSED_GRIDS = ("log12", "log13", "uni13")

# MEASURED distance of this reference (on longdouble orbitals) from the closed forms, |ref - closed| per grid, orbital and q of QS,
# rounded up to two digits (floor 1e-17: the noise of the longdouble evaluation itself).  "F": form factors, "M": momentum orbitals.
# tests/test_bessel_ref.py holds every entry to [measured, 1.2 x measured] (or the floor); tests/test_gpu_bessel.py gates the device's
# results on analytic input at twice these plus its rounding bound.  The logarithmic grids sit at the floor or within 1e-15; the uniform
# grid of 8193 nodes feels the cusp of the s orbitals (30 nodes per bohr radius / Z): Simpson's rule at 5e-7.
FLOOR = 1e-17
# Hydrogen, LSDA (VWN), converged on log12 by the CPU oracle (35 steps): |f(q) - 1 / (1 + q^2 / 4)^2| of its density at q = 0.5 and 3,
# rounded up to two digits -- the self-interaction of the functional (the LSDA density is more diffuse than the exact 1s), not rounding
H_LSDA_DISTANCE = {0.5: 1.3e-2, 3.0: 6.0e-3}
MEASURED = {
    "log12": {"F": {(1, 0): (3e-15, 3e-15, 3e-15, 3e-15), (2, 0): (3.8e-16, 3.8e-16, 3.8e-16, 3.8e-16), (2, 1): (1e-17, 1e-17, 1e-17, 1e-17)},
              "M": {(1, 0): (3.9e-17, 3.9e-17, 3.9e-17, 3.9e-17), (2, 0): (1.4e-17, 1.4e-17, 1.4e-17, 1.4e-17),
                    (2, 1): (1e-17, 1e-17, 1e-17, 1e-17), (3, 2): (1e-17, 1e-17, 1e-17, 1e-17), (4, 3): (1e-17, 1e-17, 1e-17, 1.6e-16)}},
    "log13": {"F": {(1, 0): (1.9e-16, 1.9e-16, 1.9e-16, 1.9e-16), (2, 0): (2.3e-17, 2.4e-17, 2.4e-17, 2.4e-17), (2, 1): (1e-17, 1e-17, 1e-17, 1e-17)},
              "M": {(1, 0): (1e-17, 1e-17, 1e-17, 1e-17), (2, 0): (1e-17, 1e-17, 1e-17, 1e-17), (2, 1): (1e-17, 1e-17, 1e-17, 1e-17),
                    (3, 2): (1e-17, 1e-17, 1e-17, 1e-17), (4, 3): (1e-17, 1e-17, 1e-17, 1e-17)}},
    "uni13": {"F": {(1, 0): (5.2e-07, 5.2e-07, 5.3e-07, 5.4e-07), (2, 0): (6.5e-08, 6.5e-08, 6.6e-08, 6.7e-08),
                    (2, 1): (1.3e-11, 1.3e-11, 1.3e-11, 1.3e-11)},
              "M": {(1, 0): (3.3e-09, 3.3e-09, 3.3e-09, 3.4e-09), (2, 0): (1.2e-09, 1.2e-09, 1.2e-09, 1.2e-09),
                    (2, 1): (1.3e-14, 7.5e-14, 5e-13, 1.6e-12), (3, 2): (1e-17, 1e-17, 5.3e-17, 4.9e-16), (4, 3): (1e-17, 1e-17, 1e-17, 1e-17)}},
}
