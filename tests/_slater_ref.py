"""Reference for the Slater integrals of include/dftatom_hip.h (dfta_slater_rk and the SCF entries on top of it), in np.longdouble, with
the measure `mag` that the rounding bounds of tests/test_gpu_slater.py are stated in, the counted roundings of k_slater_rk, the two
energy sums, and the closed forms of hydrogen-like orbitals.  No GPU, no library.

    R^k(ab,cd) = Q[ (P_ac Z_bd + P_bd Z_ac) / (r^k r) s ],  P_xy = u_x u_y,  Z_i = Sum_{j<=i} d_j,  g = r^k P s,
    d_1 = (9 g_0 + 19 g_1 - 5 g_2 + g_3) / 24,  d_i = (13 (g_{i-1} + g_i) - (g_{i-2} + g_{i+1})) / 24,
    d_{N-1} = (g_{N-4} - 5 g_{N-3} + 19 g_{N-2} + 9 g_{N-1}) / 24                 (Q, s: tests/_orb_ref.py)
"""
from fractions import Fraction
from math import factorial

import numpy as np

import _orb_ref as O

LD, EPS = O.LD, O.EPS
KMAX = 8
# shape of k_slater_rk (dftatom_amd/csrc/slater.hip): what the counted rounding bound depends on
TILE, PER_LANE = 1024, 4


def increments(g):
    """(d, D): the increments of the cumulative integral of g, and the same stencils with every coefficient positive on |g|"""
    g = np.asarray(g)
    a = np.abs(g)
    N = len(g)
    d, D = np.zeros(N, dtype=g.dtype), np.zeros(N, dtype=g.dtype)
    d[1] = (9 * g[0] + 19 * g[1] - 5 * g[2] + g[3]) / 24
    D[1] = (9 * a[0] + 19 * a[1] + 5 * a[2] + a[3]) / 24
    d[2:N - 1] = (13 * (g[1:N - 2] + g[2:N - 1]) - (g[0:N - 3] + g[3:N])) / 24
    D[2:N - 1] = (13 * (a[1:N - 2] + a[2:N - 1]) + (a[0:N - 3] + a[3:N])) / 24
    d[N - 1] = (g[N - 4] - 5 * g[N - 3] + 19 * g[N - 2] + 9 * g[N - 1]) / 24
    D[N - 1] = (a[N - 4] + 5 * a[N - 3] + 19 * a[N - 2] + 9 * a[N - 1]) / 24
    return d, D


def rk(ua, ub, uc, ud, k, r, s, dtype=LD):
    """(R^k(ab,cd), mag) of the discrete definition in `dtype`; mag: the same formula on |P| with the cumulative sums of the increments
    taken in magnitude.  dtype np.float64: the float64 model (sequential cumulative sums, the worst chain)."""
    ua, ub, uc, ud, r, s = (np.asarray(x, dtype=dtype) for x in (ua, ub, uc, ud, r, s))
    N = len(r)
    w = O.weights(N).astype(dtype)
    p = np.ones(N, dtype=dtype)
    for _ in range(k):
        p = p * r
    inv = np.zeros(N, dtype=dtype)
    inv[1:] = 1 / (p[1:] * r[1:])
    Pac, Pbd = ua * uc, ub * ud
    dac, Dac = increments(p * Pac * s)
    dbd, Dbd = increments(p * Pbd * s)
    Zac, Zbd, Mac, Mbd = (np.cumsum(x) for x in (dac, dbd, Dac, Dbd))
    val = np.cumsum(w * ((Pac * Zbd + Pbd * Zac) * inv * s))[-1]
    mag = np.cumsum(w * ((np.abs(Pac) * Mbd + np.abs(Pbd) * Mac) * inv * s))[-1]
    return val, mag


def rk_roundings(N, k=KMAX):
    """c of the bound c eps mag for a result of k_slater_rk: the roundings on a term's way into the result.
    The inner term g: the product P 1, the chain r^k k, p P 1, the table s (Rp delta, exp, product) 3, times s 1.  The increment
    stencil: two sums, the factor 13, the difference, / 24: 4 (the end stencils: 3 products ride beside 3 adds, / 24).  The scan: the
    lane's chain PER_LANE - 1, six shuffle levels, the waves' chain 3, wave offset + lane prefix 1, + the lane's chain 1, the carry
    chain of the earlier tiles, + the carry 1.  The outer term: P 1, P Z 1, the sum of the two 1, p r (k + 1), the reciprocal 1, times
    it 1, times s 1 (its table 3), the weight 1.  The lane's outer chain PER_LANE adds per tile, six xor-shuffle levels, the tree
    (w0 + w1) + (w2 + w3) 2, the factor 3/8 1."""
    tiles = (N + TILE - 1) // TILE
    inner = 1 + k + 1 + 3 + 1
    stencil = 4
    scan = (PER_LANE - 1) + 6 + 3 + 1 + 1 + tiles + 1
    outer = 1 + 1 + 1 + (k + 1) + 1 + 1 + 1 + 3 + 1
    tree = PER_LANE * tiles + 6 + 2 + 1
    return inner + stencil + scan + outer + tree


# ---- the angular factor and the two energy sums ---------------------------------------------------------------------------------------
def gaunt_3j2(la, k, lb):
    """(la k lb; 0 0 0)^2 as an exact Fraction"""
    J = la + k + lb
    if J % 2 or k > la + lb or k < abs(la - lb):
        return Fraction(0)
    g = J // 2
    f = factorial
    return Fraction(f(J - 2 * la) * f(J - 2 * k) * f(J - 2 * lb), f(J + 1)) * Fraction(f(g), f(g - la) * f(g - k) * f(g - lb)) ** 2


def exchange_ks(la, lb):
    return range(abs(la - lb), la + lb + 1, 2)


def energy_sums(l, occ, nA, lsda, F0, G, dtype=np.float64):
    """(E_H, E_x) in the order the header states.  l, occ: the atom's orbitals, alpha channel (nA of them; LDA: all) then beta; F0:
    (norb, norb) symmetric; G: (KMAX + 1, norb, norb), G^k(a,a) = F^k(a,a), only same-channel blocks are read."""
    norb = len(l)
    occ = [dtype(x) for x in occ]
    eh = dtype(0)
    for i in range(norb):
        for j in range(norb):
            eh = eh + (occ[i] * occ[j]) * dtype(F0[i, j])
    S = dtype(0)
    for c0, c1 in ((0, nA), (nA, norb)):
        for a in range(c0, c1):
            for b in range(c0, c1):
                T = dtype(0)
                for k in exchange_ks(l[a], l[b]):
                    c = gaunt_3j2(l[a], k, l[b])
                    T = T + dtype(c.numerator) / dtype(c.denominator) * dtype(G[k, a, b])
                na, nb = (occ[a], occ[b]) if lsda else (dtype(0.5) * occ[a], dtype(0.5) * occ[b])
                S = S + (na * nb) * T
    return dtype(0.5) * eh, (dtype(-0.5) * S if lsda else -S)


def energy_mags(l, occ, nA, lsda, F0mag, Gmag):
    """the two sums with every term in magnitude: what the rounding bounds of E_H and E_x are stated in"""
    eh, ex = energy_sums(l, occ, nA, lsda, np.abs(F0mag), np.abs(Gmag), dtype=LD)
    return eh, -ex


def tables(U, l, r, s, nA=None):
    """(F0, G, F0mag, Gmag) in longdouble for orbitals U (norb, N): every F^0(i,j); G^k(a,b) within a channel, G^k(a,a) = F^k(a,a)"""
    norb = len(l)
    nA = norb if nA is None else nA
    F0, F0m = np.zeros((norb, norb), dtype=LD), np.zeros((norb, norb), dtype=LD)
    G, Gm = np.zeros((KMAX + 1, norb, norb), dtype=LD), np.zeros((KMAX + 1, norb, norb), dtype=LD)
    for i in range(norb):
        for j in range(i, norb):
            F0[i, j], F0m[i, j] = F0[j, i], F0m[j, i] = rk(U[i], U[j], U[i], U[j], 0, r, s)
    for c0, c1 in ((0, nA), (nA, norb)):
        for a in range(c0, c1):
            for b in range(a, c1):
                for k in exchange_ks(l[a], l[b]):
                    G[k, a, b], Gm[k, a, b] = G[k, b, a], Gm[k, b, a] = rk(U[a], U[b], U[b], U[a], k, r, s)
    return F0, G, F0m, Gm


# ---- hydrogen-like orbitals of nuclear charge Z: closed forms in units of Z -------------------------------------------------------------
ZREF = 10
ORBS = ((1, 0), (2, 0), (2, 1), (3, 2), (4, 3), (4, 0))          # 1s 2s 2p 3d 4f 4s: (n, l), n the principal quantum number
S1, S2, P2, D3, F4, S4 = range(6)
# (name, (a, b, c, d, k) into ORBS, closed form / Z)
CLOSED = (
    ("F0(1s,1s)", (S1, S1, S1, S1, 0), Fraction(5, 8)),
    ("F0(1s,2s)", (S1, S2, S1, S2, 0), Fraction(17, 81)),
    ("G0(1s,2s)", (S1, S2, S2, S1, 0), Fraction(16, 729)),
    ("F0(2s,2s)", (S2, S2, S2, S2, 0), Fraction(77, 512)),
    ("F0(1s,2p)", (S1, P2, S1, P2, 0), Fraction(59, 243)),
    ("G1(1s,2p)", (S1, P2, P2, S1, 1), Fraction(112, 2187)),
    ("F0(2s,2p)", (S2, P2, S2, P2, 0), Fraction(83, 512)),
    ("G1(2s,2p)", (S2, P2, P2, S2, 1), Fraction(45, 512)),
    ("F0(2p,2p)", (P2, P2, P2, P2, 0), Fraction(93, 512)),
    ("F2(2p,2p)", (P2, P2, P2, P2, 2), Fraction(45, 512)),
)
# against the reference only
EXTRA = (
    ("F6(4f,4f)", (F4, F4, F4, F4, 6)),
    ("G5(3d,4f)", (D3, F4, F4, D3, 5)),
    ("R1(2p3d,3d4f)", (P2, D3, D3, F4, 1)),
)
# the nine integrals of the float64-model check: high k, three distinct orbitals, the nodal 4s
MODEL = (CLOSED[0][:2], CLOSED[2][:2], CLOSED[5][:2], CLOSED[9][:2]) + EXTRA + (
    ("F0(4s,4s)", (S4, S4, S4, S4, 0)), ("G3(4s,4f)", (S4, F4, F4, S4, 3)))


def orbitals(r, Z=ZREF):
    """the six orbitals of ORBS on r, longdouble (6, N)"""
    return np.array([O.hydrogenic_u(n, l, Z, r) for n, l in ORBS])


def hartree_from_density(U, occ, r, s, poisson):
    """2 pi Q[r rho U_H s] in float64: rho = Sum occ u^2 / (4 pi r^2), U_H = poisson(rho, N_e) (= r V_H)"""
    r, s = np.asarray(r, dtype=np.float64), np.asarray(s, dtype=np.float64)
    acc = np.einsum("k,ki->i", np.asarray(occ, dtype=np.float64), np.asarray(U, dtype=np.float64) ** 2)
    rho = np.zeros(len(r))
    rho[1:] = acc[1:] / (4 * np.pi * r[1:] * r[1:])
    UH = poisson(rho, float(np.sum(occ)))
    return 2 * np.pi * float(np.sum(O.weights(len(r)).astype(np.float64) * (r * rho * UH * s)))


# MEASURED distance of this reference (longdouble orbitals) from the closed forms, |ref - closed| / |closed| per grid of _orb_ref.GRIDS,
# rounded up to two digits; tests/test_slater_ref.py holds every entry to [measured, 1.2 x measured].  "hartree": the relative gap
# between E_H from F^0 (this file) and 2 pi Q[r rho U s] with U from the oracle's second-order multigrid, on the hydrogenic Z = 10
# density 1s2 2s2 2p6, at 4097 (12 levels, delta 2e-3) and 16 385 nodes (14 levels, delta 5e-4): discretisation, not rounding.
MEASURED = {
    "log12": {"F0(1s,1s)": 6.4e-13, "F0(1s,2s)": 5e-13, "G0(1s,2s)": 4.8e-12, "F0(2s,2s)": 2.6e-12, "F0(1s,2p)": 6e-13,
              "G1(1s,2p)": 2.6e-12, "F0(2s,2p)": 1.4e-12, "G1(2s,2p)": 8.6e-12, "F0(2p,2p)": 1.3e-12, "F2(2p,2p)": 8.9e-13},
    "log13": {"F0(1s,1s)": 4e-14, "F0(1s,2s)": 3.1e-14, "G0(1s,2s)": 3e-13, "F0(2s,2s)": 1.7e-13, "F0(1s,2p)": 3.8e-14,
              "G1(1s,2p)": 1.7e-13, "F0(2s,2p)": 8.4e-14, "G1(2s,2p)": 5.4e-13, "F0(2p,2p)": 8e-14, "F2(2p,2p)": 5.6e-14},
    "log14": {"F0(1s,1s)": 2.5e-15, "F0(1s,2s)": 2e-15, "G0(1s,2s)": 1.9e-14, "F0(2s,2s)": 1.1e-14, "F0(1s,2p)": 2.4e-15,
              "G1(1s,2p)": 1.1e-14, "F0(2s,2p)": 5.3e-15, "G1(2s,2p)": 3.4e-14, "F0(2p,2p)": 5e-15, "F2(2p,2p)": 3.5e-15},
    "uni13": {"F0(1s,1s)": 1.4e-06, "F0(1s,2s)": 7.7e-07, "G0(1s,2s)": 2.7e-06, "F0(2s,2s)": 1.9e-07, "F0(1s,2p)": 4.6e-07,
              "G1(1s,2p)": 7e-08, "F0(2s,2p)": 8.9e-08, "G1(2s,2p)": 3.3e-09, "F0(2p,2p)": 3.1e-09, "F2(2p,2p)": 1.5e-09},
    "hartree": {12: 1.2e-07, 14: 7.3e-09},
}
HARTREE_GRIDS = {12: (12, 2e-3, 25.0), 14: (14, 5e-4, 25.0)}
