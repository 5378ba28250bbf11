"""The VWN and Chachiyo LDA / LSDA formulas of the reference (VWNExcCor.h:23-312, ExcCorBase.h:12-26, ExcCor.h:27-95, as restated in
oracle/dfta_oracle.c and in dftatom_amd/csrc/xc.hip), in plain NumPy, generic in the floating type like _gga_ref.py.  TEST
INFRASTRUCTURE: the reference of tests/test_vwn_ref.py (CPU) and tests/test_gpu_vwn.py (GPU).

    lda(n)            -> (Vexc, eexcDif)
    lsda(na, nb)      -> (res, va, vb, eexcDif)
    chachiyo(n, imp)  -> (Vexc, eexcDif)

With np.longdouble inputs every operation, pi, 1/3, (3 / 2 pi)^(2/3), 2^(1/3) and ln 2 are extended; the fit parameters are the
doubles the kernels hold (the decimal literals of VWNExcCor.h:23-41, rounded once), because those doubles define the function that
is computed.  The expressions keep the kernels' operation order, so that the same text evaluated in float64 is a model of the
kernel (Model below: its elementary functions can be moved by some ulps, its 1/3 and one fit constant can be replaced -- what
test_vwn_ref.py feeds the gate to show that it discriminates).

The threshold (VWNExcCor.h:82,160: total density < 1e-18 -> zeros) is a decision the reference takes in double: the inputs are
doubles, and the LSDA total is their double sum, whatever type the rest is evaluated in.  A NaN total is not below it.

scale=True returns T as well, per output the sum of the magnitudes of the terms it is assembled from:
    LDA  Vexc  |c_x / r_s| + |eps| + |slope / 3|                 eexcDif  |c_x / (4 r_s)| + |slope / 3|
    LSDA common = eps_P + alpha_c w - drs:  C = |eps_P| + |alpha_c w| + (|slope_P| + |slope_S w| + |alpha_c dw|) / 3
         res   C + |x_P| + |(x_F - x_P) g|          va, vb  |x_F(rho_a,b)| + C + |(1 -+ zeta) dzeta|
         eexc  |x_P / 4| + |(x_F - x_P) g / 4| + (|slope_P| + |slope_S w| + |alpha_c dw|) / 3
    Chachiyo  Vexc  |c_x / r_s| + |a ln(..)| + |tail|            eexcDif  |c_x / (4 r_s)| + |tail|
"""
import numpy as np

from _gga_ref import running_max

LD = np.longdouble
THRESHOLD = 1e-18
PARA = (0.0310907, -0.10498, 3.72744, 12.93532)                  # A, y0, b, c: VWNExcCor.h:23-41
FERRO = (0.01554535, -0.325, 7.06042, 18.0578)
STIFF = (None, -0.0047584, 1.13107, 13.0045)                     # A = -1 / (6 pi^2)
CHACHIYO_B = {False: 20.4562557, True: 21.7392245}               # ExcCor.h:16,24
C_LDA, C_LSDA, C_CHACHIYO = 33, 138, 19                          # the c of gate(), counted from the kernels in tests/test_gpu_vwn.py


class Model:
    """the arithmetic the formulas run in: floating type, constants, elementary functions.

    third / ferro_b: replace 1 / 3 or the b of the ferromagnetic fit (a deliberately wrong kernel);
    ulps > 0 (float64 only): every array-valued sqrt / pow / log / atan result is moved by a random whole number of ulps in
    -ulps .. +ulps -- another libm, within its documented error"""

    def __init__(self, dtype, third=None, ferro_b=None, ulps=0, seed=0):
        t = self.t = np.dtype(dtype).type
        self.pi = 4 * np.arctan(t(1))
        self.fourpi = 4 * self.pi
        self.third = t(1) / t(3) if third is None else t(third)
        self.cx = np.power(t(3) / (2 * self.pi), 2 * self.third)            # X1, VWNExcCor.h:75
        self.cbrt2 = np.power(t(2), self.third)                             # X2, VWNExcCor.h:140
        self.ln2 = np.log(t(2))
        fit = lambda p: tuple(t(x) for x in p)                               # noqa: E731
        self.para, self.ferro = fit(PARA), fit(FERRO)
        if ferro_b is not None:
            self.ferro = (self.ferro[0], self.ferro[1], t(ferro_b), self.ferro[3])
        self.stiff = (-1 / (6 * self.pi * self.pi),) + fit(STIFF[1:])
        self.ulps = int(ulps)
        self.rng = np.random.default_rng(seed) if ulps else None
        assert not ulps or t is np.float64

    def _moved(self, y):
        if not self.ulps:
            return y
        y = np.array(y, dtype=np.float64)
        ok = np.isfinite(y) & (np.abs(y) > 1e-300)
        k = self.rng.integers(-self.ulps, self.ulps + 1, size=y.shape)
        bits = y.view(np.int64).copy()
        bits[ok] += k[ok]
        return bits.view(np.float64)

    def sqrt(self, x):
        return self._moved(np.sqrt(x))

    def pow(self, x, p):
        return self._moved(np.power(x, p))

    def log(self, x):
        return self._moved(np.log(x))

    def atan(self, x):
        return self._moved(np.arctan(x))


def _model(model, *arrays):
    if model is not None:
        return model
    t = arrays[0].dtype.type
    assert all(a.dtype.type is t for a in arrays) and t in (np.float64, LD)
    return Model(t)


def _fit(m, p, y, nested):
    """(eps, slope) of one fit (VWNExcCor.h:43-55); nested: Y = y (y + b) + c as the LSDA routines round it, else y y + b y + c"""
    A, y0, b, c = p
    Y = y * (y + b) + c if nested else y * y + b * y + c
    Y0 = y0 * y0 + b * y0 + c
    dy = y - y0
    Q = np.sqrt(4 * c - b * b)
    at = m.atan(Q / (2 * y + b))
    eps = A * (m.log(y * y / Y) + 2 * b / Q * at - b * y0 / Y0 * (m.log(dy * dy / Y) + 2 * (b + 2 * y0) / Q * at))
    slope = A * (c * dy - b * y0 * y) / (dy * Y)
    return eps, slope


def _rs(m, rho):
    return m.pow(3 / (m.fourpi * rho), m.third)


def _out(live, values, scale, terms):
    zero = values[0].dtype.type(0)
    out = tuple(np.where(live, v, zero) for v in values)
    if not scale:
        return out
    return out, tuple(np.where(live, t, zero) for t in terms)


def lda(n, scale=False, model=None):
    n = np.asarray(n)
    m = _model(model, n)
    live = ~(n.astype(np.float64) < THRESHOLD)
    with np.errstate(all="ignore"):
        rs = _rs(m, np.where(live, n, 1))
        eps, slope = _fit(m, m.para, m.sqrt(rs), False)
        v = -m.cx / rs + eps - m.third * slope
        e = (0.25 * m.cx) / rs + m.third * slope
        third = abs(m.third * slope)
        T = (abs(m.cx / rs) + abs(eps) + third, abs(0.25 * m.cx / rs) + third)
    return _out(live, (v, e), scale, T)


def lsda(na, nb, scale=False, model=None):
    na, nb = np.asarray(na), np.asarray(nb)
    m = _model(model, na, nb)
    live = ~(na.astype(np.float64) + nb.astype(np.float64) < THRESHOLD)
    with np.errstate(all="ignore"):
        up, dn = np.where(live, na, 1), np.where(live, nb, 1)
        tot = up + dn
        gdd = 4 / (9 * (m.cbrt2 - 1))
        gscale, dgscale = 1 / (2 * (m.cbrt2 - 1)), 2 / (3 * (m.cbrt2 - 1))
        rs = _rs(m, tot)
        z = (up - dn) / tot
        z3 = z * z * z
        z4 = z3 * z
        g = gscale * (m.pow(1 + z, 4 * m.third) + m.pow(1 - z, 4 * m.third) - 2)
        dg = dgscale * (m.pow(1 + z, m.third) - m.pow(1 - z, m.third))
        y = m.sqrt(rs)
        Pe, Ps = _fit(m, m.para, y, True)
        Fe, Fs = _fit(m, m.ferro, y, True)
        Se, Ss = _fit(m, m.stiff, y, True)
        gap = Fe - Pe
        beta = gdd * gap / Se - 1
        env = 1 + beta * z4
        w = g / gdd * env
        dbeta = gdd / Se * (Fs - Ps - Ss * gap / Se)
        dw = g / gdd * z4 * dbeta
        drs = m.third * (Ps + Ss * w + Se * dw)
        dz = Se / gdd * (4 * beta * z3 * g + env * dg)
        xP = -m.cx / rs
        xF = m.cbrt2 * xP
        common = Pe + Se * w - drs
        xa, xb = -(m.cx * m.cbrt2) / _rs(m, up), -(m.cx * m.cbrt2) / _rs(m, dn)
        va = xa + common + (1 - z) * dz
        vb = xb + common - (1 + z) * dz
        res = common + (xP + (xF - xP) * g)
        xPd = (0.25 * m.cx) / rs
        e = xPd + (m.cbrt2 * xPd - xPd) * g + drs
        D = abs(m.third) * (abs(Ps) + abs(Ss * w) + abs(Se * dw))
        Cm = abs(Pe) + abs(Se * w) + D
        T = (Cm + abs(xP) + abs((xF - xP) * g), abs(xa) + Cm + abs((1 - z) * dz), abs(xb) + Cm + abs((1 + z) * dz),
             abs(xPd) + abs((m.cbrt2 * xPd - xPd) * g) + D)
    return _out(live, (res, va, vb, e), scale, T)


def chachiyo(n, improved, scale=False, model=None):
    n = np.asarray(n)
    m = _model(model, n)
    live = ~(n.astype(np.float64) < THRESHOLD)
    a = (m.ln2 - 1) / (2 * m.pi * m.pi)                                      # ExcCor.h:30
    b = m.t(CHACHIYO_B[bool(improved)])
    with np.errstate(all="ignore"):
        rs = _rs(m, np.where(live, n, 1))
        q1 = b / rs
        q2 = q1 / rs
        tail = a / (1 + q1 + q2) * (q1 + 2 * q2) * rs / 3
        ln = a * m.log(1 + q1 + q1 / rs)
        v = -m.cx / rs + ln - tail
        e = (0.25 * m.cx) / rs + tail
        T = (abs(m.cx / rs) + abs(ln) + abs(tail), abs(0.25 * m.cx / rs) + abs(tail))
    return _out(live, (v, e), scale, T)


# ---- the fp64 oracle on the same inputs --------------------------------------------------------------------------------------------
def oracle_lda(n):
    import _oracle as O
    o, n = O.oracle(), np.ascontiguousarray(n, dtype=np.float64)
    v, e = np.zeros_like(n), np.zeros_like(n)
    o.dfo_vwn_vexc(O.dp(n), O.dp(v), n.size)
    o.dfo_vwn_eexcdif(O.dp(n), O.dp(e), n.size)
    return v, e


def oracle_lsda(na, nb):
    import _oracle as O
    o, na, nb = O.oracle(), np.ascontiguousarray(na, dtype=np.float64), np.ascontiguousarray(nb, dtype=np.float64)
    res, va, vb, e = (np.zeros_like(na) for _ in range(4))
    o.dfo_vwn_vexc_lsda(O.dp(na), O.dp(nb), O.dp(res), O.dp(va), O.dp(vb), na.size)
    o.dfo_vwn_eexcdif_lsda(O.dp(na), O.dp(nb), O.dp(e), na.size)
    return res, va, vb, e


# ---- the inputs of tests/test_gpu_vwn.py (and of the CPU tests that show what its gate can tell apart) ---------------------------
def ladder(npts, lo=-18.0, hi=6.0):
    return np.logspace(lo, hi, npts)


def lda_input(npts=4097):
    """the density ladder 1e-18 .. 1e6 with the values below, on and just above the threshold in front of it (contiguous in rho, so
    that the running maximum E mixes neighbours of like conditioning) and NaN, +Inf, -1 behind it"""
    return np.concatenate([[0.0, -0.0, 1e-300, 9.99e-19, 1e-18, np.nextafter(1e-18, 1.0)], ladder(npts), [np.nan, np.inf, -1.0]])


ZETAS = (0.0, 1e-8, -1e-8, 0.3, -0.3, 0.77, -0.77, 1 - 1e-6, -(1 - 1e-6), 1 - 1e-12, -(1 - 1e-12), 1.0, -1.0)
IDLE = (0.0, -0.0, 1e-30, 1e-19)


def lsda_inputs(npts=1025):
    """name -> (na, nb): proportional channels for every zeta of ZETAS; one channel live along the ladder, the other one of IDLE (both
    ways round); totals that cross the threshold while one channel alone stays below it (cross_low) or above it (cross_high: the
    other channel slightly negative); rho_b = -1e-3 rho_a (zeta > 1)"""
    rho = ladder(npts)
    out = {}
    for z in ZETAS:
        out["zeta%+.12g" % z] = (rho * ((1 + z) / 2), rho * ((1 - z) / 2))
    for k, v in enumerate(IDLE):
        idle = np.full(npts, v)
        out["idle_b%d" % k] = (rho, idle)
        out["idle_a%d" % k] = (idle, rho)
    low = np.logspace(-19.0, -17.0, 257)
    out["cross_low"] = (low, np.full(257, 6e-19))
    out["cross_low_mirror"] = (np.full(257, 6e-19), low)
    out["cross_high"] = (np.full(257, 2e-18), -np.logspace(-19.0, -17.7, 257))
    out["negative_b"] = (rho, -1e-3 * rho)
    out["negative_a"] = (-1e-3 * rho, rho)
    return out


# ---- the measure -------------------------------------------------------------------------------------------------------------------
def gate(got, ext, T, oracle, c):
    """|got - ref_ext|(j) <= 8 E(j) + c eps T(j) along one ladder; E the running maximum over j-8 .. j+8 of |oracle64 - ref_ext|.
    Where ref_ext is not finite `got` has to be what the oracle has (NaN for NaN, the same infinity); where T is 0 (below the
    threshold) it has to be 0.  Returns (ok, largest ratio, its index)."""
    got, oracle = np.asarray(got, dtype=np.float64), np.asarray(oracle, dtype=np.float64)
    fin = np.isfinite(ext) & np.isfinite(T)
    dead = fin & (T == 0)
    live = fin & ~dead
    ok = np.array_equal(got[~fin], oracle[~fin], equal_nan=True) and bool(np.all(got[dead] == 0.0)) and bool(np.all(ext[dead] == 0))
    ok = ok and bool(np.all(np.isfinite(got[fin])))
    with np.errstate(all="ignore"):
        E = running_max(np.where(live & np.isfinite(oracle), np.abs(oracle.astype(LD) - ext), LD(0)))
        bound = 8 * E + c * np.finfo(np.float64).eps * T
        ratio = np.where(live, np.abs(got.astype(LD) - ext) / np.where(bound > 0, bound, LD(1)), LD(0))
    ratio = np.where(np.isnan(ratio), np.inf, ratio)
    j = int(np.argmax(ratio)) if ratio.size else 0
    worst = float(ratio[j]) if ratio.size else 0.0
    return ok and worst <= 1.0, worst, j


def old_gate(got, want):
    """test_vwn_vs_golden's: 5e-11 relative against the fp64 value"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    fin = np.isfinite(want)
    return bool(np.all(np.abs(got[fin] - want[fin]) <= 5e-11 * np.abs(want[fin]) + 1e-300)) and np.array_equal(got[~fin], want[~fin], equal_nan=True)
