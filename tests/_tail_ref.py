"""The tail of an SCF step -- k_tail, k_integrate / k_integrate_simpson38_par, k_energies (scf.hip, reduce.hip) and the start-up
kernels k_init_density, k_potential -- restated in float64 NumPy in the kernels' operation order.  The library is built with
-ffp-contract=off and these kernels call no elementary function, so the restatement gives the device's bits.  TEST INFRASTRUCTURE
of tests/test_gpu_scf_tail.py (GPU) and tests/test_tail_ref.py (CPU).
"""
import math

import numpy as np

import _oracle as O

LD = np.longdouble
FOURPI = 4. * math.pi
TOTAL_ENERGY_ERR = 1E-11                                   # DFTAtom.cpp:349
FIELDS = ("Etotal", "Ekinetic", "Ecoul", "Enuclear", "Exc", "Eelectronic", "Ehartree", "eExcDif", "Epotential")
RULES = ("dfo_trapezoid", "dfo_simpson13", "dfo_simpson38", "dfo_boole", "dfo_romberg")          # DFTA_INT_* 0 .. 4


def log_cnst(Rp, delta, N):
    """dr/di as dfta_grid_create tabulates it (DFTAtom.cpp:47,442): Rp delta exp(i delta), libm's exp"""
    return np.array([Rp * delta * math.exp(float(i) * delta) for i in range(N)])


def start_density(nE, nA, nB, lsda, MaxR, N):
    """k_init_density: (density, dA, dB), flat, 0 at node 0 (DFTAtom.cpp:371-376 / 874-884); LDA: dA, dB None"""
    volume = FOURPI / 3. * MaxR * MaxR * MaxR
    flat = lambda c: np.concatenate([[0.0], np.full(N - 1, c)])              # noqa: E731
    if not lsda:
        return flat(nE / volume), None, None
    cA, cB = nA / volume, nB / volume
    return flat(cA + cB), flat(cA), flat(cB)


def potentials(Z, lsda, r, U, Vexc, va, vb):
    """k_potential and the first statement of k_tail: (-Z + U) / r + v at i >= 1, 0 at node 0"""
    u = np.zeros_like(U)
    u[1:] = (float(-Z) + U[1:]) / r[1:]
    potA, potB = np.zeros_like(U), np.zeros_like(U)
    if not lsda:
        potA[1:] = u[1:] + Vexc[1:]
        return potA, None
    potA[1:] = u[1:] + va[1:]
    potB[1:] = u[1:] + vb[1:]
    return potA, potB


def integrands(Z, lsda, uniform, r, cnst, rho, dA, dB, U, Vexc, eexc, potA, potB):
    """k_tail: [nuclear, exccor, eexcDeriv, hartree, potentiale] (DFTAtom.cpp:437-457 LDA, 956-983 LSDA; the LSDA loop of the
    uniform grid groups potentiale differently, DFTAtom.cpp:799); node 0 is 0"""
    out = [np.zeros_like(rho) for _ in range(5)]
    p, c, d, u = r[1:], cnst[1:], rho[1:], U[1:]
    if not lsda:
        positiondensity = p * d * c
        position2density = p * p * d * c
        out[4][1:] = position2density * potA[1:]
    else:
        positioncnst = p * c
        positiondensity = positioncnst * d
        position2cnst = p * positioncnst
        position2density = position2cnst * d
        if uniform:
            out[4][1:] = (p * p) * (dA[1:] * potA[1:] + dB[1:] * potB[1:])
        else:
            out[4][1:] = (position2cnst * dA[1:]) * potA[1:] + (position2cnst * dB[1:]) * potB[1:]
    out[0][1:] = float(Z) * positiondensity
    out[1][1:] = position2density * Vexc[1:]
    out[2][1:] = position2density * eexc[1:]
    out[3][1:] = positiondensity * u
    return out


def quadrature(rule, delta, v):
    """Integral::<rule>(delta, v) in the reference's summation order: the oracle's"""
    o, v = O.oracle(), np.ascontiguousarray(v, dtype=np.float64)
    if rule == 4:
        return o.dfo_romberg(float(delta), O.dp(v), v.size, 1e-18, 3)
    return getattr(o, RULES[rule])(float(delta), O.dp(v), v.size)


def simpson38_parallel(v, delta, last=None, second_class=0):
    """k_integrate_simpson38_par's summation order: thread t of 256 adds the nodes 1 + t, 1 + t + 256, .. < n - 1 to s1, or to s2 where
    i % 3 == 0; the xor butterfly over the 64 lanes of each wave (32, 16, 8, 4, 2, 1); (red0 + red1) + (red2 + red3) over the four
    waves; sum = v[0] + v[n-1]; sum += 3 s1 + 2 s2; sum delta 3/8.
    last / second_class: deliberately wrong variants (the loop's end, the residue that goes to s2) for tests/test_tail_ref.py"""
    v = np.asarray(v, dtype=np.float64)
    n = v.size
    last = n - 1 if last is None else last
    t = np.arange(256)
    s1, s2 = np.zeros(256), np.zeros(256)
    for k in range((n + 255) // 256):
        i = 1 + t + 256 * k
        x = np.where(i < last, v[np.minimum(i, n - 1)], 0.0)             # adding 0.0 changes nothing
        two = i % 3 == second_class
        s1 = s1 + np.where(two, 0.0, x)
        s2 = s2 + np.where(two, x, 0.0)
    lane = np.arange(64)
    s1, s2 = s1.reshape(4, 64), s2.reshape(4, 64)
    for off in (32, 16, 8, 4, 2, 1):
        s1 = s1 + s1[:, lane ^ off]
        s2 = s2 + s2[:, lane ^ off]
    red1, red2 = s1[:, 0], s2[:, 0]
    sum1 = (red1[0] + red1[1]) + (red1[2] + red1[3])
    sum2 = (red2[0] + red2[1]) + (red2[2] + red2[3])
    total = v[0] + v[n - 1]
    total += 3. * sum1 + 2. * sum2
    return float(total * delta * (3. / 8.))


def parallel_roundings(n):
    """the roundings between a node's value and k_integrate_simpson38_par's result: the thread's chain ceil((n - 2) / 256), the
    butterfly 6, the two pair sums 2, then 3 s1, + 2 s2 (2 s2 itself is exact), sum +=, delta, 3/8: 5.  (An end node passes v[0] + v[n-1],
    sum +=, delta, 3/8: fewer.)"""
    return -(-(n - 2) // 256) + 6 + 2 + 5


def simpson38_extended(v, delta):
    """(Simpson 3/8 of v in np.longdouble, Sum |w_i v_i| delta 3/8)"""
    v = np.asarray(v).astype(LD)
    w = np.full(v.size, LD(3))
    w[::3] = 2
    w[0] = w[-1] = 1
    scale = LD(delta) * LD(3) / LD(8)
    return np.sum(w * v) * scale, np.sum(np.abs(w * v)) * abs(scale)


def assemble(occupations, eigenvalues, integrals):
    """k_energies: Sum occ E over the atom's jobs in job order (alpha levels, then beta), the five products, the four combinations"""
    Eel = 0.0
    for f, E in zip(occupations, eigenvalues):
        Eel += float(f) * float(E)
    I = [float(x) for x in integrals]
    Enuclear = -FOURPI * I[0]
    Exc = FOURPI * I[1]
    eExcDif = FOURPI * I[2]
    Exc += eExcDif
    Ehartree = -2 * math.pi * I[3]
    Epotential = FOURPI * I[4]
    Ekinetic = Eel - Epotential
    Etotal = Eel + Ehartree + eExcDif
    return dict(Etotal=Etotal, Ekinetic=Ekinetic, Ecoul=-Ehartree, Enuclear=Enuclear, Exc=Exc, Eelectronic=Eel, Ehartree=Ehartree,
                eExcDif=eExcDif, Epotential=Epotential)


class StopTest:
    """the reference's stop test (DFTAtom.cpp:474-479) as k_energies keeps it per atom"""

    def __init__(self):
        self.Eold, self.lastTimeConverged, self.finished = 0.0, 0, 0

    def step(self, Etotal, conv):
        with np.errstate(all="ignore"):
            small = abs(np.float64(self.Eold - Etotal) / np.float64(Etotal)) < TOTAL_ENERGY_ERR
        if small and conv and self.lastTimeConverged:
            self.finished = 1
        else:
            self.Eold, self.lastTimeConverged = Etotal, int(bool(conv))
        return self.finished
