"""Reference for the exchange potentials of include/dftatom_hip.h (dfta_screening_yk, dfta_exchange_potentials and the SCF entries on top
of them), in np.longdouble, with the measure `mag` that the rounding bounds of tests/test_gpu_exchange.py are stated in, the counted
roundings of the kernels of dftatom_amd/csrc/exchange.hip, and the closed forms of hydrogen-like orbitals.  No GPU, no library.

    y^k_xy,i = Z_i inv_i + p_i W_i,  Z_i = Sum_{j<=i} d_j(g),  W_i = Sum_{j>i} d_j(h),  g = (p P) s,  h = (P inv) s,  p = r^k,
    inv = 1 / (p r) (0 at node 0),  y_0 = W_0 (k = 0) or 0;   d_j: the three stencils of _slater_ref.increments
    X_a = Sum_b Sum_k (n_b c_abk) (y^k_ab u_b),  D = Sum n u^2,  vS = -(Sum n u X) / D,  vKLI = vS + (Sum_{a != h} n u^2 c) / D
"""
import numpy as np

import _orb_ref as O
import _slater_ref as S

LD, EPS = O.LD, O.EPS
KMAX = S.KMAX
HF, SL, CC, KLI = range(4)              # columns of a vbar row (DFTA_XP_*)
PAIR = 4                                # the quadrature S_ab (red_roundings)
# shape of the kernels (dftatom_amd/csrc/exchange.hip): what the counted rounding bounds depend on
TILE, PER_LANE, RED_LANES = 1024, 4, 256


def _powers(r, k, dtype):
    N = len(r)
    p = np.ones(N, dtype=dtype)
    for _ in range(k):
        p = p * r
    inv = np.zeros(N, dtype=dtype)
    inv[1:] = 1 / (p[1:] * r[1:])
    return p, inv


def _rcumsum(e):
    """W_i = Sum_{j > i} e_j, summed from the outside in"""
    return np.concatenate([np.cumsum(e[::-1])[::-1][1:], np.zeros(1, dtype=e.dtype)])


def yk(ux, uy, k, r, s, dtype=LD, model=None):
    """(y, mag): the screening function y^k_xy = Y^k_xy / r of the discrete definition in `dtype`, N values, and the same formula on |P|
    with every stencil coefficient positive and the sums in magnitude.  dtype np.float64: the float64 model (sequential cumulative
    sums, the worst chain).  model: None, or one of the two WRONG reverse scans that tests/test_exchange_ref.py shows to miss the
    bound -- "no_end_stencil": the increment of node N-1 by the inner stencil with g_N = 0; "start_N2": W starts at node N-2."""
    ux, uy, r, s = (np.asarray(x, dtype=dtype) for x in (ux, uy, r, s))
    N = len(r)
    p, inv = _powers(r, k, dtype)
    P = ux * uy
    d, Dg = S.increments(p * P * s)
    h = P * inv * s
    e, De = S.increments(h)
    if model == "no_end_stencil":
        e[N - 1] = (13 * (h[N - 2] + h[N - 1]) - h[N - 3]) / 24
    elif model == "start_N2":
        e[N - 1] = 0
    else:
        assert model is None
    Z, Zm, W, Wm = np.cumsum(d), np.cumsum(Dg), _rcumsum(e), _rcumsum(De)
    y, mag = Z * inv + p * W, Zm * inv + p * Wm
    y[0], mag[0] = (W[0], Wm[0]) if k == 0 else (0, 0)
    return y, mag


def yk_roundings(N, k=KMAX):
    """c of the bound c eps mag_i for a node of a row of k_screening_yk: the roundings on a term's way into y_i.
    Through Z: g -- the product P 1, the chain r^k k, p P 1, the table s (Rp delta, exp, product) 3, times s 1: k + 6.  The increment
    stencil: two sums, the factor 13, the difference, / 24: 4 (the end stencils: 3 products ride beside 3 adds, / 24).  The scan: the
    lane's chain PER_LANE - 1, six shuffle levels, the waves' chain 3, wave offset + lane prefix 1, + the lane's chain 1, the carry
    chain of the earlier tiles, + the carry 1: 15 + tiles.  The outer factor inv: p k, p r 1, the reciprocal 1, Z inv 1: k + 3.  The
    sum of the two products 1.
    Through W: h -- P 1, inv k + 2, P inv 1, the table s 3, times s 1: k + 8.  The stencil 4.  The mirrored scan 15 + tiles (the carry
    chain is that of the later tiles).  The outer factor: p k, p W 1: k + 1.  The sum 1.
    Both ways: 2 k + 29 + tiles."""
    tiles = (N + TILE - 1) // TILE
    via_z = (k + 6) + 4 + ((PER_LANE - 1) + 6 + 3 + 1 + 1 + tiles + 1) + (k + 3) + 1
    via_w = (k + 8) + 4 + ((PER_LANE - 1) + 6 + 3 + 1 + 1 + tiles + 1) + (k + 1) + 1
    assert via_z == via_w == 2 * k + 29 + tiles
    return via_z


def red_roundings(N, kind):
    """c of the bound c eps mag for a quadrature of k_exchange_reduce on the device's own integrands (u, X, D, vS, vKLI as the device holds
    them): the term -- HF: u X 1, times s 1, the table s 3, the weight 1: 6;  SL / KLI: u u 1, times v 1, times s 1, the table 3, the
    weight 1: 7;  PAIR: u_a u_a 1, u_b u_b 1, their product 1, / D 1, times s 1, the table 3, the weight 1: 9 --, the lane's chain
    ceil(N / RED_LANES) adds, six xor-shuffle levels, the tree (w0 + w1) + (w2 + w3) 2, the factor 3/8 1 (the sign of HF is exact)."""
    term = {HF: 6, SL: 7, KLI: 7, PAIR: 9}[kind]
    return term + (N + RED_LANES - 1) // RED_LANES + 6 + 2 + 1


def quad(term, dtype=LD):
    """(Q[term], Q[|term|]); term already carries s"""
    w = O.weights(len(term)).astype(dtype)
    return np.sum(w * term), np.sum(w * np.abs(term))


# ---- the tables of a channel: the Python statement of dftatom_amd/csrc/exchange_plan.cpp ---------------------------------------------
def y_jobs(l):
    """rows (x, y, k): a, then b >= a, then k of the exchange sum ascending"""
    return [(a, b, k) for a in range(len(l)) for b in range(a, len(l)) for k in S.exchange_ks(l[a], l[b])]


def x_entries(l):
    """for every a the entries (b, k) of X_a: b ascending over the whole channel, then k ascending"""
    return [[(b, k) for b in range(len(l)) for k in S.exchange_ks(l[a], l[b])] for a in range(len(l))]


def pick_homo(E, occ):
    """the highest eigenvalue among the shells with occ > 0, the higher index on ties; -1: none"""
    h = -1
    for a in range(len(E)):
        if occ[a] > 0 and (h < 0 or E[a] >= E[h]):
            h = a
    return h


def gaunt(la, k, lb, dtype):
    c = S.gaunt_3j2(la, k, lb)
    return dtype(c.numerator) / dtype(c.denominator)


def solve_kli(M, vS, vHF, homo, dtype=LD):
    """c with c[homo] = 0 and (I - M)_red c = (vS - vHF)_red, in the elimination order of the header"""
    n = len(vS)
    idx = [a for a in range(n) if a != homo]
    H = len(idx)
    c = np.zeros(n, dtype=dtype)
    if H == 0:
        return c
    A = np.array([[dtype(1 if i == j else 0) - dtype(M[idx[i], idx[j]]) for j in range(H)] for i in range(H)], dtype=dtype)
    b = np.array([dtype(vS[i]) - dtype(vHF[i]) for i in idx], dtype=dtype)
    for j in range(H):
        p = j
        for i in range(j + 1, H):
            if abs(A[i, j]) > abs(A[p, j]):
                p = i
        if p != j:
            A[[j, p]] = A[[p, j]]
            b[[j, p]] = b[[p, j]]
        for i in range(j + 1, H):
            f = A[i, j] / A[j, j]
            for m in range(j + 1, H):
                A[i, m] = A[i, m] - f * A[j, m]
            b[i] = b[i] - f * b[j]
    x = np.zeros(H, dtype=dtype)
    for i in range(H - 1, -1, -1):
        t = b[i]
        for m in range(i + 1, H):
            t = t - A[i, m] * x[m]
        x[i] = t / A[i, i]
    c[idx] = x
    return c


def pointwise(U, l, occ, Y, dtype=LD):
    """(X, D, num, vS) in the header's orders from the rows Y[(x, y, k)] (x <= y); dtype np.float64 on the device's own rows reproduces the
    device bit for bit (every operation is one IEEE operation per node)"""
    U = np.asarray(U, dtype=dtype)
    n, N = U.shape
    occ = [dtype(x) for x in occ]
    X = np.zeros((n, N), dtype=dtype)
    for a, entries in enumerate(x_entries(l)):
        acc = np.zeros(N, dtype=dtype)
        for b, k in entries:
            coef = occ[b] * gaunt(l[a], k, l[b], dtype)
            acc = acc + coef * (np.asarray(Y[(min(a, b), max(a, b), k)], dtype=dtype) * U[b])
        X[a] = acc
    D, num = np.zeros(N, dtype=dtype), np.zeros(N, dtype=dtype)
    for a in range(n):
        D = D + occ[a] * (U[a] * U[a])
        num = num + occ[a] * (U[a] * X[a])
    vS = np.zeros(N, dtype=dtype)
    ok = D > 0
    vS[ok] = -(num[ok] / D[ok])
    return X, D, num, vS


def kli_potential(U, occ, homo, c, D, vS, dtype=LD):
    U = np.asarray(U, dtype=dtype)
    acc = np.zeros(U.shape[1], dtype=dtype)
    for a in range(U.shape[0]):
        if a != homo:
            acc = acc + (dtype(occ[a]) * (U[a] * U[a])) * dtype(c[a])
    v = np.zeros(U.shape[1], dtype=dtype)
    ok = np.asarray(D) > 0
    v[ok] = np.asarray(vS, dtype=dtype)[ok] + acc[ok] / np.asarray(D, dtype=dtype)[ok]
    return v


def reductions(U, occ, X, D, vS, s, vKLI=None, dtype=LD):
    """the quadratures on GIVEN integrands: dict of (value, mag) arrays -- "HF", "S" (n each), "pair" (n x n, each pair once, mirrored), and
    with vKLI "KLI"; M = pair value times occ_b"""
    U, X, D, vS, s = (np.asarray(x, dtype=dtype) for x in (U, X, D, vS, s))
    n = U.shape[0]
    out = {"HF": np.zeros((2, n), dtype=dtype), "S": np.zeros((2, n), dtype=dtype), "pair": np.zeros((2, n, n), dtype=dtype)}
    ok = D != 0
    Dsafe = np.where(ok, D, 1)
    for a in range(n):
        v, m = quad((U[a] * X[a]) * s, dtype)
        out["HF"][:, a] = -v, m
        out["S"][:, a] = quad(((U[a] * U[a]) * vS) * s, dtype)
        for b in range(a, n):
            t = np.where(ok, ((U[a] * U[a]) * (U[b] * U[b])) / Dsafe, 0) * s
            out["pair"][:, a, b] = out["pair"][:, b, a] = quad(t, dtype)
    if vKLI is not None:
        vKLI = np.asarray(vKLI, dtype=dtype)
        out["KLI"] = np.zeros((2, n), dtype=dtype)
        for a in range(n):
            out["KLI"][:, a] = quad(((U[a] * U[a]) * vKLI) * s, dtype)
    out["M"] = out["pair"][0] * np.array([dtype(x) for x in occ], dtype=dtype)[None, :]
    return out


def potentials(U, l, occ, homo, r, s, dtype=LD):
    """everything dfta_exchange_potentials returns, from the discrete definitions in `dtype`: dict with Y (by job), Ymag, X, D, num, vS, c,
    vKLI, vbar (n x 4), M, and "red" (the reductions with their mags)"""
    U = np.asarray(U, dtype=dtype)
    Y, Ym = {}, {}
    for x, y, k in y_jobs(l):
        Y[(x, y, k)], Ym[(x, y, k)] = yk(U[x], U[y], k, r, s, dtype=dtype)
    X, D, num, vS = pointwise(U, l, occ, Y, dtype)
    red = reductions(U, occ, X, D, vS, s, dtype=dtype)
    c = solve_kli(red["M"], red["S"][0], red["HF"][0], homo, dtype)
    vKLI = kli_potential(U, occ, homo, c, D, vS, dtype)
    red = reductions(U, occ, X, D, vS, s, vKLI=vKLI, dtype=dtype)
    vbar = np.stack([red["HF"][0], red["S"][0], c, red["KLI"][0]], axis=1)
    return {"Y": Y, "Ymag": Ym, "X": X, "D": D, "num": num, "vS": vS, "c": c, "vKLI": vKLI, "vbar": vbar, "M": red["M"], "red": red}


# ---- closed forms on hydrogen-like orbitals of nuclear charge Z (sympy derives them, mpmath evaluates them at 40 digits) -----------------
# (name, (x, y, k) into _slater_ref.ORBS, ((n, l), (n, l), k))
CLOSED = (
    ("y0(1s,1s)", (S.S1, S.S1, 0), ((1, 0), (1, 0), 0)),
    ("y0(2s,2s)", (S.S2, S.S2, 0), ((2, 0), (2, 0), 0)),
    ("y0(2p,2p)", (S.P2, S.P2, 0), ((2, 1), (2, 1), 0)),
    ("y2(2p,2p)", (S.P2, S.P2, 2), ((2, 1), (2, 1), 2)),
    ("y1(1s,2p)", (S.S1, S.P2, 1), ((1, 0), (2, 1), 1)),
)
# against the reference only: high k, two distinct orbitals, the nodal 4s, and k above l_x + l_y (singular W integrand: grid-limited)
EXTRA = (
    ("y6(4f,4f)", (S.F4, S.F4, 6)), ("y5(3d,4f)", (S.D3, S.F4, 5)), ("y0(4s,4s)", (S.S4, S.S4, 0)), ("y3(4s,4f)", (S.S4, S.F4, 3)),
    ("y8(4f,4f)", (S.F4, S.F4, 8)), ("y1(2s,3d)", (S.S2, S.D3, 1)),
)
_closed_cache = {}


def closed_expr(na, la, nb, lb, k):
    """the sympy expression of y^k(r) for hydrogen-like orbitals (Z, r symbols): r^(-k-1) Int_0^r t^k P + r^k Int_r^oo t^(-k-1) P"""
    import sympy as sp
    key = (na, la, nb, lb, k)
    if key not in _closed_cache:
        Z, r, t = sp.symbols("Z r t", positive=True)

        def u(n, l):
            rho = 2 * Z * t / n
            norm = sp.sqrt(2 * Z / n * sp.factorial(n - l - 1) / (2 * n * sp.factorial(n + l)))
            return norm * rho ** (l + 1) * sp.exp(-rho / 2) * sp.assoc_laguerre(n - l - 1, 2 * l + 1, rho)
        P = sp.expand(u(na, la) * u(nb, lb))
        inner = sp.integrate(t ** k * P, (t, 0, r))
        outer = sp.integrate(sp.expand(t ** (-k - 1) * P), (t, r, sp.oo))
        _closed_cache[key] = (sp.simplify(inner / r ** (k + 1) + r ** k * outer), Z, r)
    return _closed_cache[key]


def closed_yk(spec, Zval, r):
    """the closed form at the nodes r (longdouble or float64), node 0 by its limit, as longdouble.  The form [1 - e^(-2Zr)(1 + Zr)] / r
    cancels near the origin: the nodes with Z r < 1 are evaluated with mpmath at 40 digits, the others in longdouble (where the forms
    lose three digits of nineteen at the most)"""
    import mpmath
    import sympy as sp
    (na, la), (nb, lb), k = spec
    expr, Z, rs = closed_expr(na, la, nb, lb, k)
    f = sp.lambdify(rs, expr.subs(Z, Zval), "mpmath")
    out = np.zeros(len(r), dtype=LD)
    rl = np.asarray(r, dtype=LD)
    far = Zval * rl >= 1
    num, den = sp.fraction(sp.together(expr.subs(Z, Zval)))
    cst = [x for x in sp.Mul.make_args(num) if not x.has(rs)]                      # irrational prefactors (sqrt 6): in longdouble, not float
    rest = sp.Mul(*[x for x in sp.Mul.make_args(num) if x.has(rs)]) / den
    scale = LD(1)
    for x in cst:
        v = sp.N(x, 40)
        a = float(v)
        scale = scale * (LD(a) + LD(float(v - a)))
    out[far] = scale * sp.lambdify(rs, rest, "numpy")(rl[far])
    with mpmath.workdps(40):
        for i in np.nonzero(~far)[0]:
            if i == 0:
                continue
            hi = float(r[i])
            x = mpmath.mpf(hi) + mpmath.mpf(float(LD(r[i]) - LD(hi)))
            v = f(x)
            a = float(v)
            out[i] = LD(a) + LD(float(v - mpmath.mpf(a)))
        out[0] = LD(float(sp.limit(expr.subs(Z, Zval), rs, 0))) if k == 0 else LD(0)
    return out


def y0_1s1s(Z, r):
    """the textbook form, for the test that the sympy route reproduces it"""
    r = np.asarray(r, dtype=LD)
    out = np.zeros(len(r), dtype=LD)
    out[1:] = -np.expm1(-2 * Z * r[1:]) / r[1:] - Z * np.exp(-2 * Z * r[1:])
    out[0] = Z
    return out


def smooth_orbitals(r):
    """four made-up smooth orbitals on [0, 10], one with a node, none small at the outer end; float64 (4, N)"""
    r = np.asarray(r, dtype=np.float64)
    return np.array([r * np.exp(-r), r * r * np.exp(-0.7 * r), r * (1 - 0.4 * r) * np.exp(-0.5 * r), r ** 3 * np.exp(-r)])


# MEASURED distance of this reference (longdouble orbitals) from the closed forms, max_i |ref_i - closed_i| / max_i |closed_i| over all
# nodes (node 0: the limit) per grid of _orb_ref.GRIDS, rounded up to two digits; tests/test_exchange_ref.py holds every entry to
# [measured, 1.2 x measured].  (Relative to the row's peak, not node by node: y^k ~ r^k at the origin for k > 0, and the first panel of
# the W integral carries a relative error of 1e-7 -- logarithmic -- to 1e-2 -- uniform -- at node 1 that no later node sees.)
# "ex_identity": |Sum n vbarHF - 2 E_x| / |2 E_x| of the neon-like channel of hydrogenic orbitals at 4097 nodes (log12) in longdouble:
# Q[P p W s] and Q[P Z inv s] are two discretisations of one integral, equal to the grid's order, not to rounding.
# "hartree": max_i |Sum_a N_a y^0_aa,i r_i - U_i| / N_e with U from the oracle's second-order multigrid on the hydrogenic Z = 10 density
# 1s2 2s2 2p6 at 4097 nodes (log12): discretisation of the multigrid, not rounding.  "tail": |r vKLI + 1| at the outermost node with D > 0
# on the CPU oracle's orbitals after three SCF steps at 4097 nodes (log12), from this reference: LDA neon and the alpha channel of LSDA
# nitrogen -- vKLI = -n_h Sum_k c_hhk y^k_hh there, -1 / r only up to <r^2> / r^2.
MEASURED = {
    "log13": {"y0(1s,1s)": 6.9e-14, "y0(2s,2s)": 2.7e-13, "y0(2p,2p)": 1.7e-13, "y2(2p,2p)": 1.3e-12, "y1(1s,2p)": 6.4e-13},
    "uni13": {"y0(1s,1s)": 4.5e-06, "y0(2s,2s)": 2.0e-06, "y0(2p,2p)": 8.7e-08, "y2(2p,2p)": 5.0e-06, "y1(1s,2p)": 4.0e-05},
    "ex_identity": {"log12": 4.5e-15},
    "hartree": {12: 2.6e-07},
    "tail": {"Ne": 6.2e-04, "N_alpha": 1.2e-03},
}
