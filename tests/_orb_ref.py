"""Reference for the orbital expectation values and r^k matrix elements of include/dftatom_hip.h (dfta_orbital_properties,
dfta_orbital_matrix), in np.longdouble, with the sums of the magnitudes of the weighted terms that the rounding bounds of
tests/test_gpu_orbitals.py are stated in, analytic hydrogen-like orbitals and their closed forms.  No GPU, no library.

    Q[f] = (3/8) (f_0 + f_{N-1} + 3 Sum_{0<i<N-1, i%3 != 0} f_i + 2 Sum_{0<i<N-1, i%3 == 0} f_i)       (Integral::Simpson38)
    s_i  = dr/di: Rp delta exp(i delta) on the logarithmic grid r_i = Rp (exp(i delta) - 1), h on the uniform grid r_i = i h
"""
import math

import numpy as np

LD = np.longdouble
EPS = 2.0 ** -52
NORM, RM1, R1, R2, R4, T, RPEAK, RM3 = range(8)
COLUMNS = ("NORM", "<1/r>", "<r>", "<r^2>", "<r^4>", "T", "RPEAK", "<1/r^3>")

# tiling of the two kernels (dftatom_amd/csrc/orbitals.hip): what the counted rounding bounds depend on
PROP_TILE, PROP_PER_LANE = 1024, 4
MAT_CHUNK = 512


def weights(N):
    """Simpson 3/8 weights as Integral::Simpson38 applies them, the factor 3/8 included"""
    w = np.full(N, 3.0, dtype=LD)
    w[0::3] = 2.0
    w[0] = w[N - 1] = 1.0
    return w * LD(3) / LD(8)


def grid(levels, delta, Rmax):
    """(r, s) in longdouble; delta None / 0: the uniform grid"""
    N = 2 ** levels + 1
    i = np.arange(N, dtype=LD)
    if not delta:
        h = LD(Rmax) / LD(N - 1)
        return i * h, np.full(N, h, dtype=LD)
    d = LD(delta)
    Rp = LD(Rmax) / (np.exp(d * LD(N - 1)) - LD(1))
    return Rp * np.expm1(d * i), Rp * d * np.exp(d * i)


def du_di(u):
    """(du/di, D): the stencils of the header and the same stencils with every difference (end nodes: every term) taken in magnitude"""
    u = np.asarray(u, dtype=LD)
    N = len(u)
    du, D = np.zeros(N, dtype=LD), np.zeros(N, dtype=LD)
    a, b = u[3:N - 1] - u[1:N - 3], u[4:N] - u[0:N - 4]
    du[2:N - 2] = (8 * a - b) / 12
    D[2:N - 2] = (8 * np.abs(a) + np.abs(b)) / 12
    du[0] = (-3 * u[0] + 4 * u[1] - u[2]) / 2
    D[0] = (3 * abs(u[0]) + 4 * abs(u[1]) + abs(u[2])) / 2
    du[1], D[1] = (u[2] - u[0]) / 2, abs(u[2] - u[0]) / 2
    du[N - 2], D[N - 2] = (u[N - 1] - u[N - 3]) / 2, abs(u[N - 1] - u[N - 3]) / 2
    du[N - 1] = (3 * u[N - 1] - 4 * u[N - 2] + u[N - 3]) / 2
    D[N - 1] = (3 * abs(u[N - 1]) + 4 * abs(u[N - 2]) + abs(u[N - 3])) / 2
    return du, D


def properties(u, l, r, s):
    """(props, mag): the eight columns of one orbital and, per column, the sum of the magnitudes of the weighted terms (for T with
    D of du_di in place of du/di; RPEAK: 0).  u, r, s: N values each; everything is evaluated in longdouble."""
    u, r, s = (np.asarray(x, dtype=LD) for x in (u, r, s))
    N = len(u)
    w = weights(N)
    g = u * u * s
    inv = np.zeros(N, dtype=LD)
    inv[1:] = 1 / r[1:]
    du, D = du_di(u)
    cent = LD(l * (l + 1)) * u * u * inv * inv * s
    terms = {NORM: g, RM1: g * inv, R1: g * r, R2: g * r * r, R4: g * r ** 4, T: (du * du / s + cent) / 2,
             RM3: g * inv ** 3 if l >= 1 else np.zeros(N, dtype=LD)}
    props, mag = np.zeros(8, dtype=LD), np.zeros(8, dtype=LD)
    for c, t in terms.items():
        props[c] = np.sum(w * t)
        mag[c] = np.sum(w * np.abs(t))
    mag[T] = np.sum(w * (D * D / s + cent) / 2)
    props[RPEAK] = r[int(np.argmax(np.abs(u)))]          # argmax: the first of equal maxima
    return props, mag


def matrix(U, k, r, s):
    """(M, mag): M_ab = Q[u_a u_b r^k s] and the sums of the magnitudes of its weighted terms; U: (norb, N)"""
    U, r, s = (np.asarray(x, dtype=LD) for x in (U, r, s))
    f = weights(U.shape[1]) * s * r ** k
    M, mag = (U * f) @ U.T, (np.abs(U) * f) @ np.abs(U).T
    return np.triu(M) + np.triu(M, 1).T, np.triu(mag) + np.triu(mag, 1).T     # each pair once, mirrored


def prop_roundings(N):
    """c of the bound c eps mag for a column of k_orbital_properties: the roundings on a term's way into the result.
    The term itself, the longest path (T): the three differences and the division of du/di enter (du/di)^2 twice 6, the square
    and / s 2, the table s (Rp delta, exp, product) 3, the centrifugal term's five operations ride beside it, the add of the two 1,
    the weight 1: 13.  The lane's chain: PROP_PER_LANE adds per tile.  Six xor-shuffle levels, the tree (w0 + w1) + (w2 + w3) 2,
    the factors 3/8 and 1/2 2."""
    tiles = (N + PROP_TILE - 1) // PROP_TILE
    return 13 + PROP_PER_LANE * tiles + 6 + 2 + 2


def matrix_roundings(N):
    """c for an entry of k_orbital_matrix: s table 3, r^k 1, s r^k 1, the weight 1, u_a u_b 1, times the weight 1: 8; the lane's chain
    over the MAT_CHUNK nodes of a chunk; the chunks in order; the factor 3/8 1."""
    chunks = (N + MAT_CHUNK - 1) // MAT_CHUNK
    return 8 + MAT_CHUNK + chunks + 1


INPUT_ROUNDINGS = 2     # an analytic orbital rounded to float64 moves a product of two of its values by one eps, and (du/di)^2 by two


# ---- hydrogen-like orbitals (nuclear charge Z, principal quantum number n) -----------------------------------------------------------
def hydrogenic_u(n, l, Z, r):
    """u_nl(r) = r R_nl(r), normalised to Int u^2 dr = 1, in longdouble"""
    r = np.asarray(r, dtype=LD)
    rho = LD(2 * Z) * r / LD(n)
    a, kmax = 2 * l + 1, n - l - 1
    Lm, Lk = np.zeros_like(rho), np.ones_like(rho)             # generalised Laguerre L_k^a by its three-term recurrence
    for k in range(kmax):
        Lm, Lk = Lk, ((2 * k + 1 + a - rho) * Lk - (k + a) * Lm) / (k + 1)
    norm = np.sqrt(LD(2 * Z) / LD(n) * LD(math.factorial(n - l - 1)) / LD(2 * n * math.factorial(n + l)))
    return norm * rho ** (l + 1) * np.exp(-rho / 2) * Lk


def closed_forms(n, l, Z):
    """the columns that have a closed form for a hydrogen-like orbital (NORM = 1), as longdouble; RM3 only for l >= 1"""
    n_, l_, Z_ = LD(n), LD(l), LD(Z)
    ll = l_ * (l_ + 1)
    out = {NORM: LD(1), RM1: Z_ / n_ ** 2, R1: (3 * n_ ** 2 - ll) / (2 * Z_), R2: n_ ** 2 * (5 * n_ ** 2 + 1 - 3 * ll) / (2 * Z_ ** 2),
           R4: n_ ** 4 * (63 * n_ ** 4 - 35 * n_ ** 2 * (2 * ll - 3) + 5 * ll * (3 * ll - 10) + 12) / (8 * Z_ ** 4),
           T: Z_ ** 2 / (2 * n_ ** 2)}
    if l >= 1:
        out[RM3] = Z_ ** 3 / (n_ ** 3 * l_ * (l_ + LD(1) / 2) * (l_ + 1))
    return out


DIPOLE_1S_2P = lambda Z: LD(128) * np.sqrt(LD(6)) / (LD(243) * LD(Z))        # <1s| r |2p>

# the orbitals of the closed-form checks: decayed far inside Rmax = 25 (Z = 1, n = 2 there is truncation-limited near 1e-6)
ORBITALS = ((1, 0, 10), (3, 1, 10), (4, 3, 10), (3, 2, 2))                   # (n, l, Z)
PAIR = ((1, 0, 10), (2, 0, 10), (2, 1, 10))                                  # 1s, 2s, 2p of Z = 10: overlap and dipole
GRIDS = {"log12": (12, 2e-3, 25.0), "log14": (14, 5e-4, 25.0), "log13": (13, 1e-3, 25.0), "uni13": (13, None, 25.0)}

# MEASURED distance of this reference from the closed forms, |ref - closed| / |closed| per grid, orbital and column, rounded up to two
# digits (floor 1e-17: the noise of the longdouble evaluation itself); "S12": |<1s|2s>| (closed form 0: absolute), "D": the dipole
# integral <1s|r|2p>, relative.  Discretisation on the Z = 10 orbitals -- T, through the five-point derivative, is the column that
# feels it --; the 3d orbital of Z = 2 is limited by its truncation at Rmax = 25 instead (u^2 ~ 1e-8 of its peak there), the same
# 8e-9 in NORM on every grid.  tests/test_orb_ref.py holds every entry to [measured, 1.2 x measured] (or the floor);
# tests/test_gpu_orbitals.py gates the device's results on analytic input at twice these plus its rounding bound.
FLOOR = 1e-17
MEASURED = {
    "log12": {
        (1, 0, 10): {NORM: 3.2e-15, RM1: 2.2e-14, R1: 7.8e-17, R2: 1e-17, R4: 1e-17, T: 1.8e-10},
        (3, 1, 10): {NORM: 1e-17, RM1: 1e-17, R1: 1e-17, R2: 1e-17, R4: 1e-17, T: 2.3e-11, RM3: 7.4e-15},
        (4, 3, 10): {NORM: 1e-17, RM1: 1e-17, R1: 1e-17, R2: 1e-17, R4: 1e-17, T: 7.5e-12, RM3: 1e-17},
        (3, 2, 2): {NORM: 8.2e-09, RM1: 1.5e-09, R1: 4.1e-08, R2: 1.8e-07, R4: 2.4e-06, T: 5.8e-09, RM3: 2.5e-11},
        "S12": 1.2e-15, "D": 1e-17},
    "log14": {
        (1, 0, 10): {NORM: 1.3e-17, RM1: 8.5e-17, R1: 1e-17, R2: 1e-17, R4: 1e-17, T: 2.8e-12},
        (3, 1, 10): {NORM: 1e-17, RM1: 1e-17, R1: 1e-17, R2: 1e-17, R4: 1e-17, T: 9e-14, RM3: 2.9e-17},
        (4, 3, 10): {NORM: 1e-17, RM1: 1e-17, R1: 1e-17, R2: 1e-17, R4: 1e-17, T: 3e-14, RM3: 1e-17},
        (3, 2, 2): {NORM: 8.2e-09, RM1: 1.5e-09, R1: 4.1e-08, R2: 1.8e-07, R4: 2.4e-06, T: 5.7e-09, RM3: 2.4e-11},
        "S12": 1e-17, "D": 1e-17},
    "log13": {
        (1, 0, 10): {NORM: 2e-16, RM1: 1.4e-15, R1: 1e-17, R2: 1e-17, R4: 1e-17, T: 2.2e-11},
        (3, 1, 10): {NORM: 1e-17, RM1: 1e-17, R1: 1e-17, R2: 1e-17, R4: 1e-17, T: 1.5e-12, RM3: 4.7e-16},
        (4, 3, 10): {NORM: 1e-17, RM1: 1e-17, R1: 1e-17, R2: 1e-17, R4: 1e-17, T: 4.7e-13, RM3: 1e-17},
        (3, 2, 2): {NORM: 8.2e-09, RM1: 1.5e-09, R1: 4.1e-08, R2: 1.8e-07, R4: 2.4e-06, T: 5.8e-09, RM3: 2.4e-11},
        "S12": 7e-17, "D": 1e-17},
    "uni13": {
        (1, 0, 10): {NORM: 5.5e-07, RM1: 5.5e-07, R1: 1.9e-07, R2: 8.1e-10, R4: 9.5e-13, T: 3.7e-05},
        (3, 1, 10): {NORM: 4.5e-12, RM1: 9e-09, R1: 3.6e-13, R2: 2.2e-16, R4: 1e-17, T: 1.8e-07, RM3: 3.9e-08},
        (4, 3, 10): {NORM: 1e-17, RM1: 1e-17, R1: 1e-17, R2: 1e-17, R4: 1e-17, T: 3.4e-11, RM3: 4e-14},
        (3, 2, 2): {NORM: 8.1e-09, RM1: 1.5e-09, R1: 4e-08, R2: 1.8e-07, R4: 2.3e-06, T: 5.7e-09, RM3: 2.8e-11},
        "S12": 2e-07, "D": 1.5e-10},
}
