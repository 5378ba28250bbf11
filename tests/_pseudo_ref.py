"""Reference for the pseudization block of include/dftatom_hip.h (dfta_pseudize): the header's arithmetic restated ONCE, as pseudize(),
and run in two number formats -- np.float64, operation for operation in the header's order (the model of k_pseudize), and np.longdouble
on the same float64 inputs (the replay the gates are stated against) --, the perturbed model (every exp and log moved by +-1 ulp) and two
wrong models that the gates are calibrated with, and the hydrogen-like test channels.  No GPU, no library.

The gate of a device quantity that passes through exp or log against the longdouble replay is 8 E + floor: E the float64 model's own
distance from the replay, floor the largest change of the float64 model when every exp and log result is moved by +-1 ulp, over 8 seeds
(the device's + - x / are correctly rounded and keep the header's order; its exp and log are not libm's).
"""
import math

import numpy as np

from _continuum_ref import GRIDS as _CGRIDS, tables      # noqa: F401  (re-exported for the tests)
from _orb_ref import hydrogenic_u

LD = np.longdouble
EPS = 2.0 ** -52
COEF, MATCH = 7, 8
NOBRACKET, CAP, NODES, NONFINITE, NOTPOSITIVE = 1, 2, 4, 8, 16
LANES = 256
EDGE = 3
BRACKET_STEPS = 24
ITER_CAP = 200
GRIDS = dict(_CGRIDS)
ROWS = ((1., 1., 1., 1., 1.), (0., 6., 8., 10., 12.), (0., 30., 56., 90., 132.), (0., 120., 336., 720., 1320.),
        (0., 360., 1680., 5040., 11880.))


class Perturb:
    """every result of the wrapped function moved by +-1 ulp, the direction drawn per call"""

    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)

    def __call__(self, q):
        q = np.asarray(q, dtype=np.float64)
        up = self.rng.integers(0, 2, size=q.shape).astype(bool)
        return np.where(up, np.nextafter(q, np.inf), np.nextafter(q, -np.inf))


def solve5(b, T):
    """the header's elimination on the augmented matrix; returns (a0, a6, a8, a10, a12)"""
    A = [[T(v) for v in row] + [T(b[k])] for k, row in enumerate(ROWS)]
    for k in range(5):
        for i in range(k + 1, 5):
            if abs(A[i][k]) > abs(A[k][k]):
                A[k], A[i] = A[i], A[k]
        for i in range(k + 1, 5):
            m = A[i][k] / A[k][k]
            for j in range(k + 1, 6):
                A[i][j] = A[i][j] - m * A[k][j]
    x = [T(0)] * 5
    for k in range(4, -1, -1):
        t = A[k][5]
        for j in range(k + 1, 5):
            t = t - A[k][j] * x[j]
        x[k] = t / A[k][k]
    return x


def coefficients(a2, l, P, T):
    """(a0, a2, .., a12) of a trial a2"""
    a2 = T(a2)
    a4 = -((a2 * a2) / T(2 * l + 5))
    b = (P[0] - (a2 + a4), P[1] - (T(2) * a2 + T(4) * a4), P[2] - (T(2) * a2 + T(12) * a4), P[3] - T(24) * a4, P[4] - T(24) * a4)
    x = solve5(b, T)
    return [x[0], a2, a4, x[1], x[2], x[3], x[4]]


def pseudo_u(r, rinv, l, c, exp):
    x = r * rinv
    t = x * x
    p = c[0] + t * (c[1] + t * (c[2] + t * (c[3] + t * (c[4] + t * (c[5] + t * c[6])))))
    rp = r.copy()
    for _ in range(l):
        rp = rp * r
    return rp * exp(p)


def pseudo_v(r, rinv, l, eps, c, rc, T):
    """V_ps inside the core: needs no exp, no log and not a0"""
    x = r * rinv
    t = x * x
    cq = [T(2 * k) * c[k] for k in range(1, 7)]
    cw = [T(2 * k * (2 * k - 1)) * c[k] for k in range(1, 7)]
    q = cq[0] + t * (cq[1] + t * (cq[2] + t * (cq[3] + t * (cq[4] + t * cq[5]))))
    w = cw[0] + t * (cw[1] + t * (cw[2] + t * (cw[3] + t * (cw[4] + t * cw[5]))))
    return eps + ((T(l + 1) * q) + ((w + t * (q * q)) * T(0.5))) / (rc * rc)


def tree_norm(f, ic):
    """the sum of the increments d_1 .. d_ic of the integrand f (nodes 0 .. ic + 1 at least) in the kernel's shape"""
    T = f.dtype.type
    d = np.zeros(((ic // LANES) + 1) * LANES, dtype=f.dtype)
    d[1] = (((T(9) * f[0] + T(19) * f[1]) - T(5) * f[2]) + f[3]) / T(24)
    i = np.arange(2, ic + 1)
    d[2:ic + 1] = (T(13) * (f[i - 1] + f[i]) - (f[i - 2] + f[i + 1])) / T(24)
    acc = np.zeros(LANES, dtype=f.dtype)
    for row in d.reshape(-1, LANES):
        acc = acc + row
    lane = np.arange(64)
    w = []
    for k in range(LANES // 64):
        v = acc[64 * k:64 * k + 64]
        for off in (32, 16, 8, 4, 2, 1):
            v = v + v[lane ^ off]
        w.append(v[0])
    return (w[0] + w[1]) + (w[2] + w[3])


def matching(V, su, l, eps, ic, r, s, lam, T, log, wrong=None):
    """(P0 .. P4) of the header at the core node; su = sigma u"""
    f = lambda a, k: a[ic + k]                                                       # noqa: E731
    D1 = lambda a: (T(8) * (f(a, 1) - f(a, -1)) - (f(a, 2) - f(a, -2))) / T(12)      # noqa: E731
    D2 = lambda a: ((T(16) * (f(a, 1) + f(a, -1)) - (f(a, 2) + f(a, -2))) - T(30) * f(a, 0)) / T(12)      # noqa: E731
    si, rc, L = s[ic], r[ic], T(l + 1)
    du = D1(su) / si
    dvi = D1(V)
    dv = dvi / si
    d2v = (D2(V) - (T(0) if wrong == "nolam" else T(lam)) * dvi) / (si * si)
    rcp = rc
    for _ in range(l):
        rcp = rcp * rc
    rc2 = rc * rc
    rc3, rc4, tl, fl = rc2 * rc, rc2 * rc2, T(2) * L, T(4) * L
    p0 = log(su[ic] / rcp)
    p1 = du / su[ic] - L / rc
    p2 = ((T(2) * (V[ic] - eps)) - (tl * p1) / rc) - p1 * p1
    if wrong == "p3sign":
        p3 = (((T(2) * dv) - (tl * p1) / rc2) - (tl * p2) / rc) - (T(2) * p1) * p2
    else:
        p3 = (((T(2) * dv) + (tl * p1) / rc2) - (tl * p2) / rc) - (T(2) * p1) * p2
    p4 = ((((T(2) * d2v) - (fl * p1) / rc3) + (fl * p2) / rc2) - (tl * p3) / rc) - (T(2) * (p2 * p2) + (T(2) * p1) * p3)
    return [p0, p1 * rc, p2 * rc2, p3 * rc3, p4 * rc4]


def _changes(u):
    """the nodes i >= 2 with u_i strictly opposite to u_{i-1} (to u_{i-2} where u_{i-1} is exactly zero)"""
    u = np.asarray(u, dtype=np.float64)
    b = np.where(u[1:-1] != 0, u[1:-1], u[:-2])
    return np.where(((u[2:] < 0) & (b > 0)) | ((u[2:] > 0) & (b < 0)))[0] + 2


def _sign(g):
    return 1 if g > 0 else (-1 if g < 0 else 0)


def pseudize(V, u, l, eps, ic, r, s, lam, dtype=np.float64, a2=None, perturb=None, wrong=None):
    """The header's arithmetic for ONE channel; V, u, r, s: float64 rows.  dtype np.float64: the kernel's model; LD: the replay (inputs
    are converted, nothing else changes).  a2: skip the root search and form everything from this a2 (the device's own).  perturb: a
    Perturb applied to every exp and log (float64 only).  wrong: "p3sign" / "nolam" -- the two wrong models.
    Returns u_ps, V_ps, coef, rc, match, iters, status (the keys of dftatom_amd.pseudize)."""
    T = dtype
    N = len(r)
    exp = (lambda x: perturb(np.exp(x))) if perturb is not None else np.exp          # noqa: E731
    log = (lambda x: T(perturb(np.log(x)))) if perturb is not None else np.log       # noqa: E731
    nan = T(np.nan)
    out = {"u_ps": np.full(N, nan), "V_ps": np.full(N, nan), "coef": np.full(COEF, nan), "rc": nan, "match": np.full(MATCH, nan),
           "iters": 0, "status": 0}
    V64, u64 = np.asarray(V, dtype=np.float64), np.asarray(u, dtype=np.float64)
    if not (np.isfinite(eps) and np.all(np.isfinite(V64)) and np.all(np.isfinite(u64))):
        out["status"] = NONFINITE
        return out
    ch = _changes(u64)
    last = int(ch[-1]) if len(ch) else 0
    if ic <= last or u64[ic] == 0:
        out["status"] = NODES
        return out
    V, u, r, s = (np.asarray(x, dtype=np.float64).astype(T) for x in (V, u, r, s))
    eps = T(eps)
    sigma = T(1) if u[ic] > 0 else T(-1)
    su = sigma * u
    rc = r[ic]
    rinv = T(1) / rc
    with np.errstate(all="ignore"):
        P = matching(V, su, l, eps, ic, r, s, lam, T, log, wrong)
        fae = (u[:ic + 2] * u[:ic + 2]) * s[:ic + 2]
        IAE = tree_norm(fae, ic)
        lnAE = log(IAE)
        state = {"iters": 0}

        def evaluate(x):
            state["iters"] += 1
            c = coefficients(x, l, P, T)
            f = fae.copy()
            ups = pseudo_u(r[:ic], rinv, l, c, exp)
            f[:ic] = (ups * ups) * s[:ic]
            Ips = tree_norm(f, ic)
            state.update(c=c, Ips=Ips, g=log(Ips) - lnAE)
            return state["g"]

        status = 0
        if a2 is not None:
            lo = T(a2)
        else:
            lo, hi = T(0), T(0)
            glo = ghi = evaluate(lo)
            s0 = _sign(glo)
            if glo != glo:
                status |= NOBRACKET
            if s0 != 0 and not status:
                found, ap, gp, am, gm, h = False, T(0), glo, T(0), glo, T(0.25)
                for _ in range(BRACKET_STEPS):
                    gq = evaluate(h)
                    if gq == gq and _sign(gq) != s0:
                        lo, glo, hi, ghi, found = ap, gp, h, gq, True
                        break
                    if gq == gq:
                        ap, gp = h, gq
                    gr = evaluate(-h)
                    if gr == gr and _sign(gr) != s0:
                        lo, glo, hi, ghi, found = am, gm, -h, gr, True
                        break
                    if gr == gr:
                        am, gm = -h, gr
                    h = h + h
                if not found:
                    status |= NOBRACKET
            if s0 != 0 and not status:
                while ghi != 0:
                    mid = lo + (hi - lo) * T(0.5)
                    if mid == lo or mid == hi:
                        break
                    if state["iters"] >= ITER_CAP:
                        status |= CAP
                        break
                    gmid = evaluate(mid)
                    if gmid != gmid:
                        status |= NOBRACKET
                        break
                    if _sign(gmid) == s0:
                        lo, glo = mid, gmid
                    else:
                        hi, ghi = mid, gmid
                if abs(ghi) < abs(glo):
                    lo = hi
        out["iters"] = state["iters"]
        if not status:
            evaluate(lo)
            out["iters"] = state["iters"]
            c = state["c"]
            ups = pseudo_u(r[:ic], rinv, l, c, exp)
            if not (np.all(ups[1:] > 0) and np.all(np.isfinite(ups[1:]))):
                status |= NOTPOSITIVE
        out["status"] = status
        if status:
            return out
        out["u_ps"] = np.concatenate([ups, su[ic:]])
        out["V_ps"] = np.concatenate([pseudo_v(r[:ic], rinv, l, eps, c, rc, T), V[ic:]])
        out["coef"] = np.array(c, dtype=T)
        out["rc"] = rc
        out["match"] = np.array(P + [IAE, state["Ips"], state["g"]], dtype=T)
    return out


def default_valence(n, l, occ):
    """the header's rule, restated: indices kept, ascending in l"""
    occd = [k for k in range(len(n)) if occ[k] > 0]
    if not occd:
        return []
    nmax = max(n[k] for k in occd)
    keep = []
    for ll in range(max(l[k] for k in occd) + 1):
        cand = [k for k in occd if l[k] == ll]
        if cand:
            best = max(cand, key=lambda k: (n[k], -k))
            if n[best] >= nmax - max(0, ll - 1):
                keep.append(best)
    return keep


def default_ic(r, u, factor):
    N = len(r)
    peak = int(np.argmax(np.abs(u)))
    ic = int(np.argmin(np.abs(r - factor * r[peak])))
    ch = _changes(u)
    ic = max(ic, (int(ch[-1]) if len(ch) else 0) + 1)
    while ic < N - 1 - EDGE and u[ic] == 0:
        ic += 1
    return min(max(ic, EDGE), N - 1 - EDGE)


# ---- hydrogen-like channels: V = -Z / r, where V' and V'' are analytic ------------------------------------------------------------------
ZREF = 10
HYDROGENIC = ((2, 0), (2, 1), (3, 2))                  # 2s, 2p, 3d of Z = 10: (principal n, l)


def hydrogenic_channel(n, l, r, Z=ZREF):
    """(V, u, eps) in float64 on the nodes r"""
    V = np.zeros(len(r))
    V[1:] = -float(Z) / r[1:]
    u = hydrogenic_u(n, l, Z, r.astype(LD)).astype(np.float64)
    return V, u, -0.5 * Z * Z / (n * n)


def analytic_matching(n, l, rc, Z=ZREF):
    """(P1 .. P4, their scales) of a hydrogen-like channel with V' = Z / r^2, V'' = -2 Z / r^3 analytic and u'/u by a longdouble central
    difference of the closed-form orbital (step 1e-5 r_c: error 1e-11).  The nodeless 2p and 3d have p = const - Z r / n: P2 = P3 = P4 = 0
    exactly, so a distance is taken relative to the scale of a value: the sum of the magnitudes of the terms it is made of."""
    rc = LD(rc)
    hh = rc * LD(1e-5)
    up, um, u0 = (hydrogenic_u(n, l, Z, np.array([x]))[0] for x in (rc + hh, rc - hh, rc))
    L, eps = LD(l + 1), -LD(Z * Z) / LD(2 * n * n)
    p1 = (up - um) / (2 * hh) / u0 - L / rc
    v, dv, d2v = -LD(Z) / rc, LD(Z) / rc ** 2, -2 * LD(Z) / rc ** 3
    t2 = (2 * (v - eps), -2 * L * p1 / rc, -p1 * p1)
    p2 = sum(t2)
    t3 = (2 * dv, 2 * L * p1 / rc ** 2, -2 * L * p2 / rc, -2 * p1 * p2)
    p3 = sum(t3)
    t4 = (2 * d2v, -4 * L * p1 / rc ** 3, 4 * L * p2 / rc ** 2, -2 * L * p3 / rc, -2 * p2 * p2, -2 * p1 * p3)
    p4 = sum(t4)
    mag = lambda t: sum(abs(x) for x in t)           # noqa: E731
    m2 = mag(t2)
    m3 = abs(t3[0]) + abs(t3[1]) + 2 * L * m2 / rc + 2 * abs(p1) * m2
    m4 = abs(t4[0]) + abs(t4[1]) + 4 * L * m2 / rc ** 2 + 2 * L * m3 / rc + 2 * m2 * m2 + 2 * abs(p1) * m3
    return [p1 * rc, p2 * rc ** 2, p3 * rc ** 3, p4 * rc ** 4], [(abs(p1 + L / rc) + L / rc) * rc, m2 * rc ** 2, m3 * rc ** 3, m4 * rc ** 4]


def oracle_atom(Z, steps=3, grid="log12"):
    """The CPU oracle's LDA atom after `steps` steps: (Vin, channels), Vin the last step's input potential and channels the default valence
    levels as (l, eps, u), u the normalised eigenfunction of Vin at the level's eigenvalue (what dfta_scf_get_orbitals holds)."""
    import ctypes as C
    import _oracle as O
    o = O.oracle()
    L, d, Rm = GRIDS[grid]
    scf = o.dfo_scf_create(0, Z, L, 0.5, Rm, d, 1)
    try:
        e = O.Energies()
        N = scf.contents.g.N
        for _ in range(steps - 1):
            o.dfo_scf_step(scf, C.byref(e))
        Vin = np.ctypeslib.as_array(scf.contents.potA, (N,)).copy()
        o.dfo_scf_step(scf, C.byref(e))
        lev = [scf.contents.la[k] for k in range(scf.contents.nla)]
        keep = default_valence([x.n for x in lev], [x.l for x in lev], [x.occ for x in lev])
        channels = []
        for k in keep:
            u = np.zeros(N)
            o.dfo_match(C.byref(scf.contents.g), O.dp(Vin), lev[k].l, lev[k].E, O.dp(u), None)
            o.dfo_normalize_nonuniform(C.byref(scf.contents.g), O.dp(u))
            channels.append((lev[k].l, lev[k].E, u))
    finally:
        o.dfo_scf_destroy(scf)
    return Vin, channels


def oracle_level(V, l, grid="log12"):
    """the CPU oracle's level solver on a caller potential: the eigenvalue of the nodeless level of angular momentum l"""
    import ctypes as C
    import _oracle as O
    o = O.oracle()
    g = O.make_grid(*GRIDS[grid])
    lv = O.levels_array([(l, l, 1)])
    dens = np.zeros(g.N)
    V = np.ascontiguousarray(V, dtype=np.float64)
    eel, bottom = C.c_double(0), C.c_double(float(np.min(V[1:])) - 1.0)
    o.dfo_loop_over_levels(C.byref(g), O.dp(V), lv, 1, O.dp(dens), C.byref(eel), C.byref(bottom), 1, None)
    return lv[0].E


GATED = ("a2", "a0", "Ips", "u_ps")                    # what passes through exp / log


def _gated_values(res):
    return {"a2": res["coef"][1], "a0": res["coef"][0], "Ips": res["match"][6], "u_ps": res["u_ps"]}


def distances(res, ld):
    """per gated quantity the distance of `res` from the replay `ld`, relative to the replay's magnitude (u_ps: to its largest value)"""
    a, b = _gated_values(res), _gated_values(ld)
    out = {}
    for q in GATED:
        scale = np.max(np.abs(b[q])) if q == "u_ps" else max(abs(b[q]), LD(1e-300))
        out[q] = float(np.max(np.abs(np.asarray(a[q], dtype=LD) - b[q])) / scale)
    return out


def gate(V, u, l, eps, ic, r, s, lam, seeds=range(8)):
    """(replay, model, gates): gates[q] = 8 E + floor of the header's docstring"""
    ld = pseudize(V, u, l, eps, ic, r, s, lam, dtype=LD)
    f64 = pseudize(V, u, l, eps, ic, r, s, lam)
    if ld["status"] or f64["status"]:
        return ld, f64, None
    E = distances(f64, ld)
    floor = {q: 0.0 for q in GATED}
    for seed in seeds:
        pert = pseudize(V, u, l, eps, ic, r, s, lam, perturb=Perturb(seed))
        dd = distances(pert, {k: np.asarray(v, dtype=LD) for k, v in f64.items()})
        floor = {q: max(floor[q], dd[q]) for q in GATED}
    return ld, f64, {q: 8 * E[q] + floor[q] for q in GATED}


# ---- end to end, with no code of this block in the loop ---------------------------------------------------------------------------------
FACTOR = 1.5                                           # the default core radius: 1.5 x the radius of the largest |u|
E2E_CASES = ("H2s", "H2p", "H3d", "H_s", "Ne_s", "Ne_p", "Ar_s", "Ar_p", "Fe_s", "Fe_d")
_ATOMS = {"H": 1, "Ne": 10, "Ar": 18, "Fe": 26}
_cache = {}


def case(tag, grid="log12"):
    """(V, u, l, eps, ic) of a named channel on `grid`: hydrogen-like Z = 10, or the CPU oracle's LDA atom after three steps (the third step's orbitals in its input potential)"""
    r = tables(*GRIDS[grid])[0]
    if tag[0] == "H" and "_" not in tag:
        n, l = int(tag[1]), "spdf".index(tag[2])
        V, u, eps = hydrogenic_channel(n, l, r)
    else:
        name, l = tag.split("_")[0], "spdf".index(tag[-1])
        if (name, grid) not in _cache:
            _cache[(name, grid)] = oracle_atom(_ATOMS[name], grid=grid)
        V, chans = _cache[(name, grid)]
        (eps, u), = [(e, uu) for ll, e, uu in chans if ll == l]
    return V, u, l, eps, default_ic(r, u, FACTOR)


def check_potential(V, Vps, l, eps, ic, grid="log12"):
    """(|eps' - eps| with eps' the CPU oracle's nodeless level of V_ps; the relative distance of u'/u at r_c in V_ps from that in V at
    E = eps; the relative distance of their central differences in E at +-0.05 Ha) -- the outward sweep of tests/_continuum_ref.py
    in longdouble: neither solver is part of this block"""
    from _continuum_ref import sweep
    r, s, c, lam = tables(*GRIDS[grid])
    E = [eps - 0.05, eps, eps + 0.05]
    a = sweep(V, l, E, [ic] * 3, r, s, c, lam, dtype=LD)["logderiv"]
    b = sweep(Vps, l, E, [ic] * 3, r, s, c, lam, dtype=LD)["logderiv"]
    return (abs(oracle_level(Vps, l, grid) - eps), float(abs(b[1] - a[1]) / abs(a[1])),
            float(abs((b[2] - b[0]) - (a[2] - a[0])) / abs(a[2] - a[0])))


def end_to_end(tag):
    V, u, l, eps, ic = case(tag)
    r, s, c, lam = tables(*GRIDS["log12"])
    return check_potential(V, pseudize(V, u, l, eps, ic, r, s, lam)["V_ps"], l, eps, ic)


# MEASURED on the CPU, rounded up to two digits; tests/test_pseudo_ref.py holds every entry to [measured / 1.5, measured], and
# tests/test_gpu_pseudo.py gates the device at twice these.
# STENCIL: the largest distance of the longdouble replay's P1 .. P4 from the analytic ones of the three hydrogen-like channels, relative to
# the scale of each value (analytic_matching), at ic = default_ic(1.5): what the five-point differences leave.
STENCIL = {"log12": 6.5e-11, "uni11": 1.7e-07}
# E2E: per channel on log12 (|eps' - eps| in Ha, u'/u at eps relative, its E-difference at +-0.05 Ha relative), the float64 model's V_ps.
# The last is the O(dE^2) remainder of the norm-conservation identity, not an error of the pseudization: Fe 4s at r_c = 3.6 has the most.
E2E = {
    "H2s": (7.3e-12, 3.2e-10, 9.8e-06),
    "H2p": (1.0e-10, 4.6e-10, 2.1e-06),
    "H3d": (4.1e-11, 4.5e-10, 4.4e-05),
    "H_s": (5.6e-12, 5.4e-10, 1.2e-04),
    "Ne_s": (2.4e-11, 4.1e-10, 2.6e-05),
    "Ne_p": (4.3e-11, 9.3e-10, 2.0e-05),
    "Ar_s": (6.8e-12, 4.0e-10, 2.1e-04),
    "Ar_p": (8.1e-12, 5.0e-11, 6.6e-05),
    "Fe_s": (4.4e-13, 3.4e-10, 1.5e-03),
    "Fe_d": (6.0e-11, 1.1e-09, 2.9e-05),
}
EIG_FLOOR = 1e-10          # below it an eigenvalue distance is the level solver's own stop (its bisection ends at 1e-10-ish brackets)
LD_FLOOR = 1e-14


# ---- unscreening and Kleinman-Bylander quantities (dfta_pseudo_ionic) ---------------------------------------------------------------------
FOURPI = 12.566370614359172                            # the double nearest 4 pi


def ionic(U, Vps, a0, l, occ, Y, vxc, r, l_loc=None, exp=np.exp):
    """The header's pointwise arithmetic for ONE atom in float64: U, Vps, Y (nch, N) -- the pseudo-orbitals, their potentials and their
    rows y^0_kk --, vxc (N) the functional's potential of rho_v.  Returns rho_v, vH, V_ion, beta, loc."""
    U, Vps, Y = (np.asarray(x, dtype=np.float64) for x in (U, Vps, Y))
    nch, N = U.shape
    rho, vH = np.zeros(N), np.zeros(N)
    for k in range(nch):
        t = np.zeros(N)
        t[1:] = (U[k, 1:] * U[k, 1:]) / ((FOURPI * r[1:]) * r[1:])
        t[0] = exp(2.0 * a0[k]) / FOURPI if l[k] == 0 else 0.0
        rho = rho + occ[k] * t
        vH = vH + occ[k] * Y[k]
    want = -1 if l_loc is None else int(l_loc)
    loc = [k for k in range(nch) if l[k] == (want if want >= 0 else max(l))][0]
    Vion = np.array([(Vps[k] - vH) - vxc for k in range(nch)])
    beta = np.array([(Vion[k] - Vion[loc]) * U[k] for k in range(nch)])
    return {"rho_v": rho, "vH": vH, "V_ion": Vion, "beta": beta, "loc": loc}


def kb_sums(beta, u, s):
    """(q1, q2, mag1, mag2) in longdouble: Q[(beta u) s], Q[(beta beta) s] and the sums of the magnitudes of their weighted terms"""
    from _orb_ref import weights
    b, u, s = (np.asarray(x, dtype=np.float64).astype(LD) for x in (beta, u, s))
    w = weights(len(s))
    t1, t2 = w * (b * u * s), w * (b * b * s)
    return np.sum(t1), np.sum(t2), np.sum(np.abs(t1)), np.sum(np.abs(t2))


def kb_roundings(N):
    """c of the bound c eps mag of a quadrature of k_ps_kb: the term's two products, the table s 3 and the weight 1: 6; the lane's chain
    of N / 256 additions; six shuffle levels, two joins, the factor 3/8: 9"""
    return 6 + (N + LANES - 1) // LANES + 9


TAIL_STEPS = 30


def oracle_tail(name, grid="log12"):
    """|r V_ion + N_valence| at node N - 2 of the CPU oracle's atom `name` after TAIL_STEPS steps, every channel.  What is left is v_xc of the
    flat start density's remnant in the linear mix, 2^-steps of 1.5e-4: it goes with the cube root, a factor 10 per 10 steps (-1.2 after
    three steps, 3.0e-2 after 20, 3.0e-3 after 30, 3.0e-4 after 40) -- a property of the unconverged potential, not of the
    unscreening.  30 steps: before the atom converges and freezes (the batched SCF freezes Ne after 35), so both sides mix alike: the float64 model's V_ps, y^0 by
    tests/_exchange_ref.py in longdouble, v_xc of rho_v by the oracle's own VWN.  What the y quadrature and the SCF's Poisson solve
    leave at the grid's end; the largest over the channels."""
    import _exchange_ref as X
    import _oracle as O
    r, s, c, lam = tables(*GRIDS[grid])
    Vin, found = oracle_atom(_ATOMS[name], steps=TAIL_STEPS, grid=grid)
    chans = [(Vin, u, l, eps, default_ic(r, u, FACTOR)) for l, eps, u in found]
    tags = ["x_" + "spdf"[ch[2]] for ch in chans]
    occ = {"s": 2.0, "p": 6.0, "d": 6.0}
    res = [pseudize(V, u, l, eps, ic, r, s, lam) for V, u, l, eps, ic in chans]
    U = np.array([x["u_ps"] for x in res])
    Y = np.array([X.yk(uu, uu, 0, r, s, dtype=LD)[0].astype(np.float64) for uu in U])
    ls = [ch[2] for ch in chans]
    oc = [1.0 if name == "H" else occ[t[-1]] for t in tags]
    a0 = [x["coef"][0] for x in res]
    first = ionic(U, [x["V_ps"] for x in res], a0, ls, oc, Y, np.zeros(len(r)), r)
    vxc = np.zeros(len(r))
    O.oracle().dfo_vwn_vexc(O.dp(np.ascontiguousarray(first["rho_v"])), O.dp(vxc), len(r))
    out = ionic(U, [x["V_ps"] for x in res], a0, ls, oc, Y, vxc, r)
    m = len(r) - 2
    return max(abs(r[m] * v[m] + sum(oc)) for v in out["V_ion"])


# MEASURED by oracle_tail(), rounded up to two digits; tests/test_pseudo_ref.py holds them, tests/test_gpu_pseudo.py gates the device at
# twice these
TAIL = {"Ne": 3.1e-03}
