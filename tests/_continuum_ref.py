"""Reference for the continuum block of include/dftatom_hip.h (dfta_continuum, dfta_scf_continuum, dfta_scf_photoionization): the
header's arithmetic restated ONCE, as sweep(), and run in two number formats -- np.float64, operation for operation in the header's order
(the model of the kernel), and np.longdouble on the same float64 inputs (the replay the gates are stated against) --, the closed forms
(free particle, Coulomb functions through mpmath, hydrogen-like bound orbitals, the hydrogen 1s cross section), the perturbed and the
two wrong models that the gates are calibrated with.  No GPU, no library.

The gate of a GPU quantity against the longdouble replay is 8 E + floor: E the float64 model's own distance from the replay (a running
maximum over the +-8 neighbouring energies of a ladder: the error of a single energy can sit in a zero crossing), floor the largest change
of the float64 model when every division result is moved by +-1 ulp, over 8 seeds (the device's division, sqrt and the table s are
correctly rounded; its sin, cos, atan2 and hypot are not -- 1 ulp on every division moves the result by more than they do.  Where no seed
moves a phase shift the gate is 0.0 and asks for the correctly rounded value: Coulomb Z = 10, l = 1 on uni10 at E <= 1e-4, which is why
the kernel puts the quadrant of its atan2 back with pi as two doubles, atan2_quadrants below).
"""
import math

import numpy as np

from _bessel_ref import jl as jl_ld, jl_model
from _orb_ref import GRIDS as _ORB_GRIDS, hydrogenic_u, weights      # noqa: F401  (re-exported for the tests)

LD = np.longdouble
EPS = 2.0 ** -52
FREE, WKB = 0, 1
NONFINITE, STEP, WKB_TAIL, NORM = 1, 2, 4, 8
MAX_PARTNERS = 16
TILE = 256
ALPHA_FS = 1 / 137.035999084
MB_PER_A02 = 28.002852                     # a_0^2 in megabarn
PI_LD = LD("3.14159265358979323846264338327950288419716939937510")

# (levels, delta, Rmax); delta None: uniform
GRIDS = {"uni3": (3, None, 2.0), "uni10": (10, None, 25.0), "uni11": (11, None, 25.0), "log12": (12, 2e-3, 25.0),
         "log13": (13, 1e-3, 25.0), "uni13": (13, None, 25.0), "uni14": (14, None, 25.0)}


def tables(levels, delta, Rmax):
    """(r, s, c, lam) in float64 exactly as the library's tables hold them (libm's exp through math.exp, the library's operation order)"""
    N = 2 ** levels + 1
    if not delta:
        h = Rmax / (N - 1)
        return np.array([h * i for i in range(N)]), np.full(N, 1.0 * h), 0.0, 0.0
    Rp = Rmax / (math.exp((float(N) - 1.0) * delta) - 1.0)
    e1 = np.array([math.exp(float(i) * delta) for i in range(N)])
    return Rp * (e1 - 1.0), Rp * delta * e1, (delta * delta) * 0.25, delta


class Perturb:
    """every division result moved by +-1 ulp, the direction drawn per element"""

    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)

    def __call__(self, q):
        q = np.asarray(q, dtype=np.float64)
        up = self.rng.integers(0, 2, size=q.shape).astype(bool)
        return np.where(up, np.nextafter(q, np.inf), np.nextafter(q, -np.inf))


def atan2_quadrants(y, x, tails=True):
    """the header's atan2 in float64 on top of np.arctan2 in the first octant: the quadrant put back with pi / 2 and pi as two doubles
    each (tails=False: with the one nearest double, the usual reconstruction) -- the operations of continuum.hip's atan2_quadrants"""
    h_hi, h_lo, p_hi, p_lo = np.float64(1.5707963267948966), np.float64(6.123233995736766e-17), np.float64(math.pi), np.float64(1.2246467991473532e-16)
    if not tails:
        h_lo = p_lo = np.float64(0.0)
    y, x = np.asarray(y, dtype=np.float64), np.asarray(x, dtype=np.float64)
    with np.errstate(all="ignore"):
        ay, ax = np.abs(y), np.abs(x)
        swap, neg = ay > ax, np.signbit(x)
        hi = np.arctan2(np.where(swap, ax, ay), np.where(swap, ay, ax))
        lo = np.zeros_like(hi)
        s = h_hi - hi
        e = (h_hi - s) - hi
        hi, lo = np.where(swap, s, hi), np.where(swap, (e + h_lo) - lo, lo)
        s = p_hi - hi
        e = (p_hi - s) - hi
        hi, lo = np.where(neg, s, hi), np.where(neg, (e + p_lo) - lo, lo)
        return np.copysign(hi + lo, y)


def _riccati(l, x, dtype):
    """(jh, jh', yh, yh') of the header at x > 0 (arrays)"""
    s, co = np.sin(x), np.cos(x)
    if dtype is LD:
        j = lambda ll: jl_ld(ll, x)[0]                                  # noqa: E731
    else:
        j = lambda ll: jl_model(ll, x)                                  # noqa: E731
    jh = x * j(l)
    if l == 0:
        return jh, co, -co, s
    jhp = x * j(l - 1) - (dtype(l) / x) * jh
    ym = -co
    y = ym / x - s
    for n in range(1, l):
        ym, y = y, (dtype(2 * n + 1) / x) * y - ym
    return jh, jhp, y, ym - (dtype(l) / x) * y


def sweep(V, l, E, m, r, s, c, lam, mode=FREE, P=None, power=0, dtype=np.float64, perturb=None, wrong=None, want_rows=False):
    """The header's arithmetic for the trials (E[t], m[t]) of ONE potential V and one l, vectorised over the trials; r, s: float64
    tables; P: (nb, N) partner rows.  dtype np.float64: the kernel's model; LD: the replay (inputs are converted, nothing else changes).
    perturb: a Perturb (float64 only); wrong: "noc" drops the delta^2 / 4 term, "tenth" uses 1/10 in place of 1/12.
    Returns logderiv, nodes, delta (phase shift or WKB phase), scale, status, sums (nt, nb) and, on request, rows (nt, N); sums_raw and
    rows_raw are the two before their one multiplication by the factor.  NORM is set
    by the header's rule in the sweep's own format; gate() marks the replay's trials where the float64 model carries it."""
    T = dtype
    div = (lambda a, b: perturb(a / b)) if perturb is not None else (lambda a, b: a / b)      # noqa: E731
    V, r, s = (np.asarray(x, dtype=np.float64).astype(T) for x in (V, r, s))
    E = np.atleast_1d(np.asarray(E, dtype=np.float64)).astype(T)
    m = np.atleast_1d(np.asarray(m, dtype=np.int64))
    nt, N = len(E), len(r)
    c, lam = T(0.0 if wrong == "noc" else c), T(lam)
    twelve = T(10 if wrong == "tenth" else 12)
    L = T(l) * (T(l) + T(1))
    with np.errstate(all="ignore"):
        s2, sq = s * s, np.sqrt(s)
        vl = V.copy()
        vl[1:] = V[1:] + div(L, r[1:] * r[1:]) * T(0.5)
        one = np.ones(nt, dtype=T)                   # (per trial, so that a Perturb moves every trial's divisions on its own)
        Zc = div(((V[2] - V[1]) * (r[1] * r[2])) * one, (r[2] - r[1]) * one)
        v0 = V[1] + div(Zc, r[1] * one)
        a = [one, div(-Zc, (T(l) + T(1)) * one)]
        for k in range(2, 5):
            a.append(div(((T(-2) * Zc) * a[k - 1]) + ((T(2) * (v0 - E)) * a[k - 2]), T(k * (k + 2 * l + 1)) * one))
        nb = 0 if P is None else len(P)
        if nb:
            Pm = np.asarray(P, dtype=np.float64).astype(T)
            rp = np.ones(N, dtype=T)
            for _ in range(power):
                rp = rp * r
            w38 = np.full(N, 3.0)
            w38[0::3] = 2.0
            w38[0] = w38[N - 1] = 1.0
            G = w38.astype(T) * ((Pm * rp) * s)
        mend = m + 1
        y_all = np.zeros((int(mend.max()) + 1, nt), dtype=T)
        f_all = np.zeros_like(y_all)
        status = np.zeros(nt, dtype=np.int64)
        nodes = np.zeros(nt, dtype=np.int64)
        tot, bs = np.zeros((nb, nt), dtype=T), np.zeros((nb, nt), dtype=T)
        w1 = w2 = y1 = f1 = np.zeros(nt, dtype=T)
        for i in range(1, int(mend.max()) + 1):
            on = i <= mend
            f = (T(2) * (vl[i] - E)) * s2[i] + c
            d = T(1) - div(f, twelve)
            if i <= 2:
                p = r[i]
                for _ in range(l):
                    p = p * r[i]
                u = p * ((((a[4] * r[i] + a[3]) * r[i] + a[2]) * r[i] + a[1]) * r[i] + a[0])
                y = div(u, sq[i])
                w = d * y
            else:
                w = ((T(2) * w1) - w2) + f1 * y1
                y = div(w, d)
                status[on & ~(d > 0)] |= STEP
            status[on & ~np.isfinite(y)] |= NONFINITE
            if i >= 2:
                nodes[(i <= m) & ((y < 0) != (y1 < 0))] += 1
            y_all[i], f_all[i] = y, f
            if nb:
                if i % TILE == 0:
                    bs[:] = 0
                acc = i <= m
                bs[:, acc] = bs[:, acc] + G[:, i][:, None] * (sq[i] * y[acc])[None, :]
                closing = acc & ((i % TILE == TILE - 1) | (i == m))
                tot[:, closing] = tot[:, closing] + bs[:, closing]
            w1, w2, y1, f1 = np.where(on, w, w1), np.where(on, w1, w2), np.where(on, y, y1), np.where(on, f, f1)
        t = np.arange(nt)
        ym1, fm1, ym, yp, fp = y_all[m - 1, t], f_all[m - 1, t], y_all[m, t], y_all[m + 1, t], f_all[m + 1, t]
        dy = (((T(1) - div(fp, T(6))) * yp) - ((T(1) - div(fm1, T(6))) * ym1)) * T(0.5)
        qm = sq[m]
        um = qm * ym
        dum = div(dy + (lam * T(0.5)) * ym, qm)
        logderiv = div(dum, um)
        pos = E > 0
        delta, scale, factor = np.zeros(nt, dtype=T), np.zeros(nt, dtype=T), np.ones(nt, dtype=T)
        Ep = np.where(pos, E, T(1))
        if mode == FREE:
            k = np.sqrt(T(2) * Ep)
            x, U = k * r[m], div(dum, k)
            jh, jhp, yh, yhp = _riccati(l, x, T)
            ca, cb = um * yhp - U * yh, U * jh - um * jhp
            pi = PI_LD if T is LD else T(math.pi)
            dl, fc = np.arctan2(-cb, ca), div(np.sqrt(div(T(2), pi * k)), np.hypot(ca, cb))
            formed, opa, opb = np.ones(nt, dtype=bool), ca, cb
        else:
            kap2 = [(T(2) * (Ep - V[m + q])) - div(L, r[m + q] * r[m + q]) for q in (-1, 0, 1)]
            ok = (kap2[0] > 0) & (kap2[1] > 0) & (kap2[2] > 0)
            status[pos & ~ok & (status == 0)] |= WKB_TAIL
            kap = [np.sqrt(x) for x in kap2]
            kp = div(kap[2] - kap[0], r[m + 1] - r[m - 1])
            sk = np.sqrt(kap[1])
            al = div(T(1), sk)
            alp = div(-kp, (T(2) * kap[1]) * sk)
            A, B = div(um, al), al * dum - alp * um
            c2 = np.sqrt(T(2) / PI_LD) if T is LD else T(0.7978845608028654)
            dl, fc = np.arctan2(A, B), div(c2, np.hypot(A, B))
            formed, opa, opb = ok, A, B
            dl, fc = np.where(ok, dl, T(np.nan)), np.where(ok, fc, T(np.nan))
        delta, scale, factor = np.where(pos, dl, delta), np.where(pos, fc, scale), np.where(pos, fc, factor)
        bad = (status & (NONFINITE | STEP)) != 0
        nan = T(np.nan)
        # NORM: the factor was formed (E > 0, no other exit) from a NaN operand of the hypot, or is not finite
        lost = pos & formed & ~bad & (np.isnan(opa) | np.isnan(opb) | ~np.isfinite(fc))
        status[lost] |= NORM
        delta, scale, factor = (np.where(lost, nan, x) for x in (delta, scale, factor))
        logderiv, delta, scale, factor = (np.where(bad, nan, x) for x in (logderiv, delta, scale, factor))
        nodes[bad] = -1
        out = {"logderiv": logderiv, "nodes": nodes, "delta": delta, "scale": scale, "status": status,
               "sums": ((tot * T(0.375)) * factor[None, :]).T, "sums_raw": (tot * T(0.375)).T}
        if want_rows:
            rows, raw = np.zeros((nt, N), dtype=T), np.zeros((nt, N), dtype=T)
            for tt in range(nt):
                raw[tt, 1:mend[tt] + 1] = sq[1:mend[tt] + 1] * y_all[1:mend[tt] + 1, tt]
                rows[tt, 1:mend[tt] + 1] = raw[tt, 1:mend[tt] + 1] * factor[tt]
            out["rows"], out["rows_raw"] = rows, raw
    return out


# ---- gates ------------------------------------------------------------------------------------------------------------------------------
SEEDS = tuple(range(8))
NEIGHBOURS = 8
LADDER_E = (1e-100, 1e-40, 1e-12, 1e-8, 1e-4)      # small positive energies: sincos, j_l and yh_l at tiny x = k r (FREE)


def running_max(x, half=NEIGHBOURS):
    """the maximum over the +-half neighbours along the first axis (the ladder of energies)"""
    x = np.nan_to_num(np.asarray(x, dtype=np.float64), nan=0.0)         # (a trial without a normalisation has no distance)
    out = np.empty_like(x)
    for k in range(len(x)):
        out[k] = np.max(x[max(0, k - half):k + half + 1], axis=0)
    return out


def phase_distance(a, b):
    """|a - b| of two angles, modulo 2 pi"""
    d = np.abs(np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64))
    return np.minimum(d, np.abs(2 * math.pi - d))


QUANTITIES = ("logderiv", "delta", "scale", "sums", "rows")


def distances(a, b):
    """per quantity the distance of two results of sweep(): logderiv and scale relative to the second, the phase modulo 2 pi, the sums
    relative to the largest sum of the trial's row in the second"""
    out = {}
    with np.errstate(all="ignore"):
        for q in ("logderiv", "scale"):
            ref = np.asarray(b[q], dtype=LD)
            out[q] = np.abs((np.asarray(a[q], dtype=LD) - ref) / np.where(ref == 0, LD(1), ref)).astype(np.float64)
        out["delta"] = phase_distance(a["delta"], b["delta"])
        ref = np.asarray(b["sums"], dtype=LD)
        if ref.size:
            big = np.max(np.abs(ref), axis=1, keepdims=True)
            out["sums"] = np.max(np.abs((np.asarray(a["sums"], dtype=LD) - ref) / np.where(big == 0, LD(1), big)), axis=1).astype(np.float64)
        else:
            out["sums"] = np.zeros(len(out["delta"]))
        if "rows" in a and "rows" in b:
            ref = np.asarray(b["rows"], dtype=LD)
            big = np.max(np.abs(ref), axis=1, keepdims=True)
            out["rows"] = np.max(np.abs((np.asarray(a["rows"], dtype=LD) - ref) / np.where(big == 0, LD(1), big)), axis=1).astype(np.float64)
        else:
            out["rows"] = np.zeros(len(out["delta"]))
    return out


def gate(V, l, E, m, r, s, c, lam, mode, P=None, power=0, seeds=SEEDS, want_rows=False):
    """(replay, model, gates): the longdouble replay and the float64 model of a ladder of energies E (ascending), and per quantity the
    gate 8 E + floor per trial.  The perturbed models of all seeds run as ONE sweep over len(seeds) copies of the ladder."""
    E = np.atleast_1d(np.asarray(E, dtype=np.float64))
    m = np.broadcast_to(m, E.shape)
    nt, ns = len(E), len(seeds)
    ld = sweep(V, l, E, m, r, s, c, lam, mode, P, power, dtype=LD, want_rows=want_rows)
    f64 = sweep(V, l, E, m, r, s, c, lam, mode, P, power, want_rows=want_rows)
    lost = (f64["status"] & NORM) != 0               # the float64 normalisation left double range: the trial's normalised outputs are NaN,
    if lost.any():                                   # and the replay (whose range is wider) has no say on them
        ld["status"] = np.where(lost, ld["status"] | NORM, ld["status"])
        for q in ("delta", "scale"):
            ld[q] = np.where(lost, LD(np.nan), ld[q])
        for q in ("sums", "rows"):
            if q in ld:
                ld[q] = np.where(lost[:, None], LD(np.nan), ld[q])
    own = distances(f64, ld)
    pert = sweep(V, l, np.tile(E, ns), np.tile(m, ns), r, s, c, lam, mode, P, power, perturb=Perturb(seeds), want_rows=want_rows)
    gates = {}
    for q in QUANTITIES:
        floor = np.zeros(nt)
        for k in range(ns):
            part = {key: val[k * nt:(k + 1) * nt] for key, val in pert.items()}
            floor = np.maximum(floor, distances(part, f64)[q])
        gates[q] = 8 * running_max(own[q]) + running_max(floor)
    return ld, f64, gates


# ---- closed forms -------------------------------------------------------------------------------------------------------------------------
def riccati_j(l, x):
    """x j_l(x) in longdouble"""
    x = np.asarray(x, dtype=LD)
    return x * jl_ld(l, x)[0]


def free_row(l, E, r):
    """the energy-normalised free solution sqrt(2 / (pi k)) x j_l(x), x = k r, in longdouble"""
    k = np.sqrt(2 * LD(E))
    return np.sqrt(2 / (PI_LD * k)) * riccati_j(l, k * np.asarray(r, dtype=LD))


def coulomb_F(l, Z, E, r, derivative=False):
    """F_l(eta, k r) of the attractive Coulomb potential -Z / r at E > 0 through mpmath (30 digits), as float; derivative: d/dr"""
    import mpmath as mp
    mp.mp.dps = 30
    k = mp.sqrt(2 * mp.mpf(float(E)))
    eta = -mp.mpf(Z) / k
    if derivative:
        return float(mp.diff(lambda rr: mp.coulombf(l, eta, k * rr), mp.mpf(float(r))))
    return float(mp.coulombf(l, eta, k * mp.mpf(float(r))))


def coulomb_row(l, Z, E, r):
    k = math.sqrt(2 * E)
    return math.sqrt(2 / (math.pi * k)) * np.array([coulomb_F(l, Z, E, x) for x in r])


def coulomb_logderiv(l, Z, E, r):
    return coulomb_F(l, Z, E, r, True) / coulomb_F(l, Z, E, r)


def hydrogenic_logderiv(n, l, Z, r):
    """u'/u of the hydrogen-like bound orbital (n, l) at r, through mpmath"""
    import mpmath as mp
    mp.mp.dps = 30
    Zm = mp.mpf(Z)
    u = lambda rr: rr ** (l + 1) * mp.exp(-Zm * rr / n) * mp.laguerre(n - l - 1, 2 * l + 1, 2 * Zm * rr / n)      # noqa: E731
    x = mp.mpf(float(r))
    return float(mp.diff(u, x) / u(x))


def hydrogen_1s_sigma(omega):
    """the photoionization cross section of H 1s in a_0^2 (Bethe and Salpeter, eq. 71.7): 2^9 pi^2 alpha / 3 (1 / (2 omega))^4
    exp(-4 arctan(k) / k) / (1 - exp(-2 pi / k)), k = sqrt(2 omega - 1); 6.30 Mb at threshold"""
    k = math.sqrt(2 * omega - 1)
    return 512 * math.pi ** 2 * ALPHA_FS / 3 * (1 / (2 * omega)) ** 4 * math.exp(-4 * math.atan(k) / k) / (1 - math.exp(-2 * math.pi / k))


def dipole_free_closed(which, Z, k):
    """Int_0^inf u_b(r) r^p (k r j_l(k r)) dr for hydrogen-like orbitals of charge Z, through sympy: "1s_p" (1s, l = 1, p = 1), "2p_s"
    (2p, l = 0), "2p_d" (2p, l = 2); without the normalisation sqrt(2 / (pi k))"""
    import sympy as sp
    r, kk, z = sp.symbols("r k z", positive=True)
    x = kk * r
    ric = {0: sp.sin(x), 1: sp.sin(x) / x - sp.cos(x), 2: (3 / x ** 2 - 1) * sp.sin(x) - 3 * sp.cos(x) / x}
    u1s = 2 * z ** sp.Rational(3, 2) * r * sp.exp(-z * r)
    u2p = z ** sp.Rational(5, 2) / (2 * sp.sqrt(6)) * r ** 2 * sp.exp(-z * r / 2)
    ub, l = {"1s_p": (u1s, 1), "2p_s": (u2p, 0), "2p_d": (u2p, 2)}[which]
    val = sp.integrate(ub * r * ric[l], (r, 0, sp.oo))
    return float(val.subs({z: Z, kk: sp.Float(k, 30)}).evalf(25))


# ---- the closed-form cases: one list for the CPU test (replay against closed forms) and the GPU test (device against closed forms) -----
ZREF = 10
FREE_E = (0.005, 0.05, 0.5, 2.0, 8.0)
COUL_E = (0.5, 8.0)
H_OMEGA = (0.51, 1.0, 2.0)
OVERLAP_ORBITALS = ((1, 0), (2, 0), (2, 1), (3, 2), (4, 3))          # (n, l) of Z = 10; the continuum l is the orbital's
DIPOLES = (("1s_p", (1, 0), 1), ("2p_s", (2, 1), 0), ("2p_d", (2, 1), 2))
CLOSED_GRIDS = ("log12", "log13", "uni13")
CLOSED_TAGS = tuple([("free", l) for l in range(5)] + [("dipole", d[0]) for d in DIPOLES]
                    + [(t, l) for l in range(3) for t in ("coul", "coul_row")] + [("bound", l) for l in range(4)] + [("H",)])
_closed_cache = {}


def _memo(key, fn):
    if key not in _closed_cache:
        _closed_cache[key] = fn()
    return _closed_cache[key]


def closed_groups(name):
    """the groups of a grid: (tag, V, l, E, m, mode, P, power, want_rows) -- one potential, one l, a ladder of energies each"""
    from _bessel_ref import momentum_closed                      # noqa: F401
    r, s, c, lam = tables(*GRIDS[name])
    N = len(r)
    rl = r.astype(LD)
    zero, coul, hyd = np.zeros(N), np.zeros(N), np.zeros(N)
    coul[1:], hyd[1:] = -ZREF / r[1:], -1.0 / r[1:]
    orb = {nl: hydrogenic_u(nl[0], nl[1], ZREF, rl).astype(np.float64) for nl in OVERLAP_ORBITALS}
    m2 = int(np.searchsorted(r, 2.0))
    groups = []
    for l in range(5):
        P = np.array([orb[nl] for nl in OVERLAP_ORBITALS if nl[1] == l])
        groups.append((("free", l), zero, l, FREE_E, N - 2, FREE, P, 0, True))
    for tag, nl, l in DIPOLES:
        groups.append((("dipole", tag), zero, l, FREE_E, N - 2, FREE, orb[nl][None, :], 1, False))
    for l in range(3):
        groups.append((("coul", l), coul, l, COUL_E, m2, WKB, None, 0, False))
        groups.append((("coul_row", l), coul, l, COUL_E, N - 2, WKB, None, 0, True))
    for l in range(4):
        groups.append((("bound", l), coul, l, (-ZREF ** 2 / 32.0,), m2, WKB, None, 0, False))
    u1s = hydrogenic_u(1, 0, 1, rl).astype(np.float64)
    groups.append((("H",), hyd, 1, tuple(w - 0.5 for w in H_OMEGA), N - 2, WKB, u1s[None, :], 1, False))
    assert tuple(g[0] for g in groups) == CLOSED_TAGS
    return groups


ROW_STRIDE = 256                # the Coulomb rows are compared at every 256th node (mpmath's F_l costs a millisecond per value)


def closed_distance(name, group, res):
    """{key: tuple over the group's energies} of |res - closed form|, res a result of sweep() (or the device's) for the group:
    phase shifts and sums absolute, rows relative to the closed row's largest value, u'/u and sigma relative"""
    from _bessel_ref import momentum_closed
    tag, V, l, E, m, mode, P, power, want_rows = group
    r = tables(*GRIDS[name])[0]
    out = {}
    f = lambda x: float(abs(x))                                         # noqa: E731
    if tag[0] == "free":
        out[("free_delta", l)] = tuple(f(d) for d in res["delta"])
        rows = [_memo((name, "free_row", l, e), lambda e=e: free_row(l, e, r)) for e in E]
        out[("free_row", l)] = tuple(f(np.max(np.abs(np.asarray(res["rows"][k], dtype=LD) - rows[k])) / np.max(np.abs(rows[k]))) for k in range(len(E)))
        for b, nl in enumerate(nl for nl in OVERLAP_ORBITALS if nl[1] == l):
            closed = [np.sqrt(np.sqrt(2 * LD(e))) * momentum_closed(nl[0], nl[1], ZREF, np.sqrt(2 * LD(e))) for e in E]
            out[("overlap", nl)] = tuple(f(abs(LD(res["sums"][k][b])) - abs(closed[k])) for k in range(len(E)))
    elif tag[0] == "dipole":
        closed = [_memo(("dip", tag[1], e), lambda e=e: math.sqrt(2 / (math.pi * math.sqrt(2 * e))) * dipole_free_closed(tag[1], ZREF, math.sqrt(2 * e)))
                  for e in E]
        out[("dipole", tag[1])] = tuple(f(LD(res["sums"][k][0]) - LD(closed[k])) for k in range(len(E)))
    elif tag[0] == "coul":
        closed = [_memo((name, "cld", l, e), lambda e=e: coulomb_logderiv(l, ZREF, e, r[m])) for e in E]
        out[("coul_ld", l)] = tuple(f(LD(res["logderiv"][k]) / LD(closed[k]) - 1) for k in range(len(E)))
    elif tag[0] == "coul_row":
        idx = np.arange(ROW_STRIDE, m + 1, ROW_STRIDE)
        rows = [_memo((name, "crow", l, e), lambda e=e: coulomb_row(l, ZREF, e, r[idx])) for e in E]
        out[("coul_row", l)] = tuple(f(np.max(np.abs(np.asarray(res["rows"][k], dtype=np.float64)[idx] - rows[k])) / np.max(np.abs(rows[k])))
                                     for k in range(len(E)))
    elif tag[0] == "bound":
        closed = _memo((name, "bld", l), lambda: hydrogenic_logderiv(4, l, ZREF, r[m]))
        out[("bound_ld", l)] = (f(LD(res["logderiv"][0]) / LD(closed) - 1),)
    elif tag[0] == "H":
        sig = [4 * math.pi ** 2 * ALPHA_FS * w / 3 * float(res["sums"][k][0]) ** 2 for k, w in enumerate(H_OMEGA)]
        out[("H_sigma",)] = tuple(f(sg / hydrogen_1s_sigma(w) - 1) for sg, w in zip(sig, H_OMEGA))
    return out


def closed_gate(group, res_ld, gates):
    """the rounding gates of gate() in the units of closed_distance, per key of the group"""
    tag, V, l, E, m, mode, P, power, want_rows = group
    out = {}
    big = (lambda k: float(np.max(np.abs(res_ld["sums"][k])))) if P is not None else None      # noqa: E731
    if tag[0] == "free":
        out[("free_delta", l)] = tuple(gates["delta"])
        out[("free_row", l)] = tuple(gates["rows"])
        for nl in (nl for nl in OVERLAP_ORBITALS if nl[1] == l):
            out[("overlap", nl)] = tuple(gates["sums"][k] * big(k) for k in range(len(E)))
    elif tag[0] == "dipole":
        out[("dipole", tag[1])] = tuple(gates["sums"][k] * big(k) for k in range(len(E)))
    elif tag[0] == "coul":
        out[("coul_ld", l)] = tuple(gates["logderiv"])
    elif tag[0] == "coul_row":
        out[("coul_row", l)] = tuple(gates["rows"])
    elif tag[0] == "bound":
        out[("bound_ld", l)] = tuple(gates["logderiv"])
    elif tag[0] == "H":
        out[("H_sigma",)] = tuple(2.5 * g for g in gates["sums"])       # sigma ~ S^2: twice the relative gate of S, and its square
    return out


# ---- neon after 40 SCF steps: what the gap between a step's input and output potential leaves of the orthogonality -------------------
NE40_ENERGIES = (0.05, 0.5, 2.0)


def neon40_overlaps():
    """|Int u_b u_eps dr|, b = 1s, 2s, eps s at NE40_ENERGIES (Riccati-normalised), from the CPU oracle on log12: the orbitals of step
    40 (eigenfunctions of its input potential) against continuum orbitals of the potential the step leaves -- what dfta_scf_continuum
    pairs.  Exact eigenfunctions of ONE potential would be orthogonal."""
    import ctypes as C
    import _oracle as O
    o = O.oracle()
    L, d, Rm = GRIDS["log12"]
    scf = o.dfo_scf_create(0, 10, L, 0.5, Rm, d, 1)
    try:
        e = O.Energies()
        N = scf.contents.g.N
        for _ in range(39):
            o.dfo_scf_step(scf, C.byref(e))
        Vin = np.ctypeslib.as_array(scf.contents.potA, (N,)).copy()
        o.dfo_scf_step(scf, C.byref(e))
        Vout = np.ctypeslib.as_array(scf.contents.potA, (N,)).copy()
        U = np.zeros((2, N))
        for b in range(2):
            lev = scf.contents.la[b]
            assert lev.l == 0
            o.dfo_match(C.byref(scf.contents.g), O.dp(Vin), 0, lev.E, O.dp(U[b]), None)
            o.dfo_normalize_nonuniform(C.byref(scf.contents.g), O.dp(U[b]))
    finally:
        o.dfo_scf_destroy(scf)
    r, s, c, lam = tables(L, d, Rm)
    res = sweep(Vout, 0, NE40_ENERGIES, [N - 2] * len(NE40_ENERGIES), r, s, c, lam, FREE, U, 0, dtype=LD)
    return np.abs(res["sums"].astype(np.float64)).T                # (2, energies)


# MEASURED by neon40_overlaps(), rounded up to two digits; tests/test_continuum_ref.py holds them, tests/test_gpu_continuum.py gates the
# device's overlaps at twice these
NE40_OVERLAP = ((8.0e-11, 7.7e-11, 7.9e-11), (6.3e-10, 6.1e-10, 6.3e-10))

# MEASURED distance of the longdouble replay from the closed forms, rounded up to two digits: what the discretisation (Numerov's h^4, the
# five-term start, the matching radius) leaves.  tests/test_continuum_ref.py holds every entry to [measured / 1.5, measured] (or the floor);
# tests/test_gpu_continuum.py gates the device at twice these plus the rounding gate.  Keys: (case, grid) -> figure.
FLOOR = 1e-14              # below it a figure is the noise of the evaluation (mpmath's values pass through float64)
MEASURED = {
    "log12": {
        ('free_delta', 0): (1.2e-11, 1.1e-09, 4.3e-08, 1.5e-06, 5.4e-05), ('free_row', 0): (2.2e-11, 3.5e-10, 9.8e-08, 2.2e-06, 6.1e-05),
        ('overlap', (1, 0)): (6.9e-13, 2e-11, 6.4e-09, 1.2e-07, 9e-07), ('overlap', (2, 0)): (3.9e-12, 1.1e-10, 3.2e-08, 3.9e-07, 5.6e-07),
        ('free_delta', 1): (1.6e-11, 2.1e-10, 1.1e-07, 2.8e-06, 8.1e-05), ('free_row', 1): (4.3e-12, 7.3e-10, 4.3e-08, 1.8e-06, 6.2e-05),
        ('overlap', (2, 1)): (2e-14, 1.6e-11, 3e-09, 5.8e-08, 1.2e-06), ('free_delta', 2): (7.7e-12, 5.4e-10, 5.2e-08, 1.6e-06, 5.4e-05),
        ('free_row', 2): (1.4e-11, 4.9e-10, 9.1e-08, 2e-06, 5.5e-05), ('overlap', (3, 2)): (1e-14, 6.3e-12, 1.2e-08, 3.9e-07, 1.5e-06),
        ('free_delta', 3): (3.3e-12, 6.9e-10, 8.1e-08, 2.7e-06, 8.1e-05), ('free_row', 3): (2.6e-11, 5e-10, 3.4e-08, 1.6e-06, 5.6e-05),
        ('overlap', (4, 3)): (1e-14, 4.5e-12, 8.7e-09, 1.9e-07, 4.2e-07), ('free_delta', 4): (1.6e-13, 7.8e-11, 7.5e-08, 1.7e-06, 5.3e-05),
        ('free_row', 4): (8.9e-12, 7.6e-11, 8.3e-08, 1.9e-06, 5.2e-05), ('dipole', '1s_p'): (1e-14, 4.8e-13, 1e-10, 2.5e-09, 9.7e-08),
        ('dipole', '2p_s'): (2.7e-12, 7.6e-11, 2.1e-08, 2.4e-07, 2.4e-07), ('dipole', '2p_d'): (1e-14, 8.5e-13, 1.9e-09, 9.6e-08, 9.6e-07),
        ('coul_ld', 0): (4.2e-11, 1.3e-09), ('coul_row', 0): (3.6e-05, 1.2e-05), ('coul_ld', 1): (3.1e-10, 2e-10),
        ('coul_row', 1): (3.2e-05, 2.1e-05), ('coul_ld', 2): (6.5e-10, 4.7e-09), ('coul_row', 2): (2e-05, 1.5e-05), ('bound_ld', 0): (1.3e-10,),
        ('bound_ld', 1): (7.9e-11,), ('bound_ld', 2): (3.3e-11,), ('bound_ld', 3): (5.5e-11,), ('H_sigma',): (0.0015, 2.3e-05, 4.3e-06),
    },
    "log13": {
        ('free_delta', 0): (7e-13, 6.4e-11, 2.9e-09, 9.8e-08, 3.4e-06), ('free_row', 0): (1.4e-12, 2.3e-11, 6.3e-09, 1.4e-07, 3.9e-06),
        ('overlap', (1, 0)): (4.3e-14, 1.3e-12, 4.2e-10, 8e-09, 8.3e-08), ('overlap', (2, 0)): (2.5e-13, 7e-12, 2.1e-09, 2.7e-08, 5.2e-08),
        ('free_delta', 1): (9.9e-13, 1.4e-11, 6.5e-09, 1.8e-07, 5.1e-06), ('free_row', 1): (2.7e-13, 4.6e-11, 2.7e-09, 1.1e-07, 3.8e-06),
        ('overlap', (2, 1)): (1e-14, 9.7e-13, 2e-10, 4.6e-09, 3e-08), ('free_delta', 2): (4.8e-13, 3.4e-11, 3.4e-09, 1.1e-07, 3.4e-06),
        ('free_row', 2): (8.4e-13, 3.1e-11, 5.8e-09, 1.3e-07, 3.5e-06), ('overlap', (3, 2)): (1e-14, 4e-13, 7.6e-10, 2.6e-08, 1.3e-07),
        ('free_delta', 3): (2.1e-13, 4.4e-11, 4.9e-09, 1.7e-07, 5e-06), ('free_row', 3): (1.6e-12, 3.1e-11, 2.2e-09, 9.6e-08, 3.5e-06),
        ('overlap', (4, 3)): (1e-14, 2.8e-13, 5.5e-10, 1.4e-08, 5.3e-09), ('free_delta', 4): (1e-14, 5e-12, 4.9e-09, 1.2e-07, 3.4e-06),
        ('free_row', 4): (5.6e-13, 5e-12, 5.2e-09, 1.2e-07, 3.3e-06), ('dipole', '1s_p'): (1e-14, 3e-14, 6.7e-12, 2e-10, 2.6e-09),
        ('dipole', '2p_s'): (1.7e-13, 4.9e-12, 1.4e-09, 1.6e-08, 2.2e-08), ('dipole', '2p_d'): (1e-14, 5.4e-14, 1.3e-10, 6.4e-09, 8.4e-08),
        ('coul_ld', 0): (2.6e-12, 8e-11), ('coul_row', 0): (3.5e-05, 1.5e-06), ('coul_ld', 1): (2e-11, 1.3e-11), ('coul_row', 1): (3.1e-05, 1.9e-06),
        ('coul_ld', 2): (4.1e-11, 3e-10), ('coul_row', 2): (1.8e-05, 9.4e-07), ('bound_ld', 0): (7.7e-12,), ('bound_ld', 1): (5e-12,),
        ('bound_ld', 2): (2.1e-12,), ('bound_ld', 3): (3.4e-12,), ('H_sigma',): (0.0015, 2.3e-05, 3e-06),
    },
    "uni13": {
        ('free_delta', 0): (1e-14, 1.2e-14, 4.4e-12, 1.4e-10, 4.5e-09), ('free_row', 0): (1e-14, 1e-14, 4.4e-12, 1.4e-10, 4.6e-09),
        ('overlap', (1, 0)): (1.1e-09, 1.9e-09, 3.3e-09, 4.7e-09, 6.7e-09), ('overlap', (2, 0)): (3.7e-10, 6.6e-10, 1.2e-09, 1.7e-09, 2.4e-09),
        ('free_delta', 1): (1e-14, 1.3e-14, 4.3e-12, 1.5e-10, 4.7e-09), ('free_row', 1): (1e-14, 1.5e-14, 3.6e-12, 1.3e-10, 4.2e-09),
        ('overlap', (2, 1)): (1e-14, 1e-14, 5.3e-14, 3e-13, 9.5e-12), ('free_delta', 2): (1e-14, 1e-14, 3.5e-12, 1.3e-10, 4.2e-09),
        ('free_row', 2): (1e-14, 1e-14, 3.2e-12, 1.1e-10, 3.9e-09), ('overlap', (3, 2)): (1e-14, 1e-14, 1.6e-13, 6.8e-12, 4e-11),
        ('free_delta', 3): (1e-14, 1e-14, 2.9e-12, 1.3e-10, 4.4e-09), ('free_row', 3): (1e-14, 1e-14, 2.4e-12, 1e-10, 3.7e-09),
        ('overlap', (4, 3)): (1e-14, 1e-14, 1.4e-13, 3.3e-12, 4.5e-12), ('free_delta', 4): (1e-14, 1e-14, 3e-12, 1.1e-10, 4e-09),
        ('free_row', 4): (1e-14, 1e-14, 2.5e-12, 9.3e-11, 3.4e-09), ('dipole', '1s_p'): (1e-14, 1e-14, 5.1e-14, 1.7e-13, 8.7e-13),
        ('dipole', '2p_s'): (2.4e-14, 4.2e-14, 4.5e-13, 5.4e-12, 6.4e-13), ('dipole', '2p_d'): (1e-14, 1e-14, 1.9e-14, 1.6e-12, 2.8e-11),
        ('coul_ld', 0): (7.9e-10, 6.8e-10), ('coul_row', 0): (3.4e-05, 4e-07), ('coul_ld', 1): (1.7e-08, 5.2e-10), ('coul_row', 1): (3e-05, 5.5e-07),
        ('coul_ld', 2): (1.8e-09, 7.2e-09), ('coul_row', 2): (1.6e-05, 8.9e-08), ('bound_ld', 0): (3.9e-10,), ('bound_ld', 1): (6.1e-09,),
        ('bound_ld', 2): (2.2e-09,), ('bound_ld', 3): (2.7e-11,), ('H_sigma',): (0.0015, 2.2e-05, 2.9e-06),
    },
}
