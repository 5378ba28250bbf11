"""CPU suite: tests/_vwn_ref.py -- the extended-precision statement of VWN and Chachiyo that tests/test_gpu_vwn.py holds the kernels
to -- pinned three ways, and the gate of that file shown to tell a right kernel from a subtly wrong one.

1. The functional-derivative identity, in np.longdouble, independent of the oracle: Vexc = d(rho (Vexc + eexcDif)) / d rho, and
   va, vb the partial derivatives of (rho_a + rho_b)(res + eexcDif).  Central differences with the step d = h rho, h = eps^(1/3)
   (eps = 1.08e-19: h = 4.8e-7).  A term of the energy is a smooth function of ln rho_sigma (powers 4/3, -1/6, -1/3 .. and
   logarithms of them), for which the central difference is off by (p - 1)(p - 2) / 6 (d / rho_sigma)^2 < (h / f)^2 of the term,
   f = rho_sigma / rho the fraction of the channel that is moved (1 for the LDA); the two evaluations of the energy each carry
   K eps of the magnitude of their terms, K the number of roundings the cancellations amplify, taken from the fp64 oracle's own
   distance from the extended value on the same densities (K = max |oracle64 - ref_ext| / (eps64 T), Vexc plus eexcDif: 122 for
   the LDA, 128 .. 1590 for zeta = 0 .. 0.999).  So
       |quotient - V| <= ((h / f)^2 + 2 K eps / h) T.
   Chachiyo is left out on purpose: ExcCor.h:59-62 subtracts a (..) rs / 3 where the derivative of a ln(1 + b/rs + b/rs^2) adds
   a (..) / 3, so the reference's Vexc is not the derivative of its own energy (its call sites are commented out in the reference);
   the kernel follows the reference, and what holds -- Vexc + eexcDif = eps_xc -- is asserted.

2. Agreement with the fp64 oracle (dfo_vwn_*; for Chachiyo, which the oracle does not have, the golden vectors of the compiled
   reference) on the inputs of test_gpu_vwn.py: the zeros and the NaNs / infinities in the same places, and everywhere else
   E = |oracle64 - ref_ext|, printed.  Its maxima relative to |ref_ext|, measured here (glibc 2.x, x86-64 long double):
       LDA 4097 points: Vexc 3.0e-12 (at rho = 1.2e-18: ln(y^2 / Y) against the atan term at large r_s), eexcDif 1.0e-15;
       LSDA, proportional channels: res 2.7e-12, eexcDif 9.5e-16, majority channel 2.3e-12 .. 1.6e-12, minority channel
       3.2e-12 (zeta 0.3), 1.1e-11 (0.77), 6.3e-11 (1 - 1e-6 and 1), 4.6e-9 (1 - 1e-12: v of the minority channel is a difference
       of terms 1e4 times its size); an idle channel of 1e-30 or 1e-19: 3.4e-6 in that channel's v at the dilute end;
       Chachiyo on the golden ladder: 4.2e-15 / 3.7e-15 (original set), 2.1e-15 / 9.8e-16 (improved).
   These are what "8 E" in the gate is made of: measured, node by node, not chosen.

3. Discrimination.  Float64 models of the kernel (the same text, Model) through the gate |x - ref_ext| <= 8 E + c eps T:
   (a) elementary functions moved by random -2 .. +2 ulp: passes (largest ratio 0.19 LDA, 0.12 Chachiyo, 0.26 LSDA);
   (b) 1/3 truncated to 0.333333333333: passes test_vwn_vs_golden's 5e-11, fails here by a factor 950 in eexcDif (480 in Vexc);
   (c) the b of the ferromagnetic fit 7.06043 for 7.06042: fails on every ladder with zeta != 0 of the identity's set, by factors
       above 1e3, and passes at zeta = 0 (where the fit does not enter).
"""
import os

import numpy as np
import pytest

import _vwn_ref as V

LD = np.longdouble
EPS = float(np.finfo(LD).eps)
EPS64 = float(np.finfo(np.float64).eps)
HERE = os.path.dirname(os.path.abspath(__file__))
assert EPS < 1.2e-19, "the reference of this file needs an extended np.longdouble"

C_LDA, C_LSDA, C_CHACHIYO = V.C_LDA, V.C_LSDA, V.C_CHACHIYO
oracle_lda, oracle_lsda = V.oracle_lda, V.oracle_lsda


# ---- 1. the identity ---------------------------------------------------------------------------------------------------------------
RHO = np.logspace(-12, 4, 513)
H = LD(EPS) ** (LD(1) / 3)
IDENTITY_ZETAS = (0.0, 0.3, -0.3, 0.77, -0.77, 0.999, -0.999)


def amplification(ext, T, orc):
    """K: the fp64 oracle's distance from the extended value in units of eps64 T, Vexc-like output plus eexcDif"""
    return float(np.max(np.abs(orc[0] - ext[0]) / T[0] + np.abs(orc[-1] - ext[-1]) / T[0])) / EPS64


def test_identity_lda():
    rho = RHO.astype(LD)
    (v, e), T = V.lda(rho, scale=True)
    K = amplification((v, e), T, oracle_lda(RHO))
    F = lambda n: n * (V.lda(n)[0] + V.lda(n)[1])                              # noqa: E731
    up, dn = rho * (1 + H), rho * (1 - H)
    err = np.abs((F(up) - F(dn)) / (up - dn) - v) / T[0]
    bound = float(H * H + 2 * K * EPS / H)
    print("LDA: h %.2e, K %.1f, |quotient - Vexc| / T max %.2e, bound %.2e" % (H, K, err.max(), bound))
    assert 1 <= K < 1e3
    assert np.all(err <= bound)


@pytest.mark.parametrize("zeta", IDENTITY_ZETAS)
def test_identity_lsda(zeta):
    rho = RHO.astype(LD)
    a, b = rho * ((1 + LD(zeta)) / 2), rho * ((1 - LD(zeta)) / 2)
    (res, va, vb, e), T = V.lsda(a, b, scale=True)
    orc = oracle_lsda(a.astype(np.float64), b.astype(np.float64))
    K = max(amplification((x, e), (t,), (y, orc[3])) for x, t, y in ((va, T[1], orc[1]), (vb, T[2], orc[2])))

    def G(x, y):
        out = V.lsda(x, y)
        return (x + y) * (out[0] + out[3])
    d = rho * H
    qa = (G(a + d, b) - G(a - d, b)) / ((a + d) - (a - d))
    qb = (G(a, b + d) - G(a, b - d)) / ((b + d) - (b - d))
    for name, q, v, t, f in (("va", qa, va, T[1], (1 + zeta) / 2), ("vb", qb, vb, T[2], (1 - zeta) / 2)):
        err = np.abs(q - v) / t
        bound = float((H / f) ** 2 + 2 * K * EPS / H)
        print("zeta %+.3f %s: K %.1f, |quotient - v| / T max %.2e, bound %.2e" % (zeta, name, K, err.max(), bound))
        assert np.all(err <= bound), (zeta, name)
    # res is the density-weighted mean of the two potentials (VWNExcCor.h:236 against 233-234), to rounding
    mean = (va * a + vb * b) / (a + b)
    assert np.all(np.abs(res - mean) <= 16 * EPS * T[0])


@pytest.mark.parametrize("improved", [False, True])
def test_chachiyo_energy_density(improved):
    """Vexc + eexcDif = -3/4 c_x / rs + a ln(1 + b/rs + b/rs^2); and the statement of the module docstring about its derivative"""
    rho = RHO.astype(LD)
    m = V.Model(LD)
    (v, e), T = V.chachiyo(rho, improved, scale=True)
    rs = (3 / (4 * m.pi * rho)) ** (LD(1) / 3)
    b = LD(V.CHACHIYO_B[improved])
    exc = -LD(0.75) * m.cx / rs + (m.ln2 - 1) / (2 * m.pi * m.pi) * np.log(1 + b / rs + b / rs / rs)
    assert np.all(np.abs(v + e - exc) <= 8 * EPS * (T[0] + T[1]))
    F = lambda n: n * (V.chachiyo(n, improved)[0] + V.chachiyo(n, improved)[1])       # noqa: E731
    up, dn = rho * (1 + H), rho * (1 - H)
    err = np.abs((F(up) - F(dn)) / (up - dn) - v) / T[0]
    assert err.max() > 0.1                     # the reference's Vexc is not the derivative of its energy


# ---- 2. the oracle -------------------------------------------------------------------------------------------------------------------
def agreement(label, names, ext, T, orc):
    """patterns equal, E finite; prints and returns max E / |ref_ext| per output"""
    out = []
    for name, x, t, y in zip(names, ext, T, orc):
        fin = np.isfinite(x)
        assert np.array_equal(y[~fin], x[~fin].astype(np.float64), equal_nan=True), (label, name)          # NaN for NaN, inf for inf
        dead = fin & (t == 0)
        assert np.all(y[dead] == 0.0) and np.all(x[dead] == 0), (label, name)
        live = fin & ~dead
        assert np.all(y[live] != 0.0) and np.all(np.isfinite(y[live])), (label, name)
        E = np.abs(y[live] - x[live])
        assert np.all(np.isfinite(E))
        out.append(float(np.max(E / np.abs(x[live]))) if live.any() else 0.0)
    print("%-24s %s" % (label, "  ".join("%s %.2e" % (n, w) for n, w in zip(names, out))))
    return out


def test_oracle_agreement_lda():
    n = V.lda_input()
    ext, T = V.lda(n.astype(LD), scale=True)
    worst = agreement("LDA", ("Vexc", "eexcDif"), ext, T, oracle_lda(n))
    assert ext[0][0] == 0 and ext[0][3] == 0 and ext[0][4] != 0 and np.isnan(ext[0][-3]) and ext[0][-2] == -np.inf and ext[0][-1] == 0
    assert worst[0] < 1e-10 and worst[1] < 1e-14           # sanity only: the figures of the docstring are 3.0e-12 and 1.0e-15


def test_oracle_agreement_lsda():
    for name, (na, nb) in V.lsda_inputs().items():
        ext, T = V.lsda(na.astype(LD), nb.astype(LD), scale=True)
        agreement("LSDA " + name, ("res", "va", "vb", "eexcDif"), ext, T, oracle_lsda(na, nb))
        if name.startswith("negative") or name == "cross_high":
            total = na + nb
            assert np.all(np.isnan(ext[0][~(total < 1e-18)])) and np.all(ext[0][total < 1e-18] == 0)


def test_golden_agreement_chachiyo():
    data = np.load(os.path.join(HERE, "golden", "uniform.npz"))
    n = data["chachiyo_n"]
    for imp in (0, 1):
        ext, T = V.chachiyo(n.astype(LD), bool(imp), scale=True)
        worst = agreement("Chachiyo %d (golden)" % imp, ("Vexc", "eexcDif"), ext, T, data["chachiyo_%d" % imp])
        f64 = V.chachiyo(n, bool(imp))
        for k in range(2):                       # the float64 text of _vwn_ref is what test_gpu_vwn.py takes E from: as close as the golden
            live = T[k] > 0
            mine = float(np.max(np.abs(f64[k][live] - ext[k][live]) / np.abs(ext[k][live])))
            print("    float64 model: %.2e" % mine)
            assert mine <= 4 * max(worst[k], EPS64)


# ---- 3. discrimination ---------------------------------------------------------------------------------------------------------------
def through_gate(model_out, ext, T, orc, c):
    return [V.gate(g, x, t, y, c) for g, x, t, y in zip(model_out, ext, T, orc)]


@pytest.fixture(scope="module")
def lda_case():
    n = V.lda_input()
    ext, T = V.lda(n.astype(LD), scale=True)
    return n, ext, T, oracle_lda(n)


def test_gate_passes_another_libm_lda(lda_case):
    n, ext, T, orc = lda_case
    for seed in range(4):
        res = through_gate(V.lda(n, model=V.Model(np.float64, ulps=2, seed=seed)), ext, T, orc, C_LDA)
        print("LDA +-2 ulp, seed %d: ratios %.2f %.2f" % (seed, res[0][1], res[1][1]))
        assert all(ok for ok, _, _ in res)
    for imp in (False, True):
        e2, T2 = V.chachiyo(n.astype(LD), imp, scale=True)
        res = through_gate(V.chachiyo(n, imp, model=V.Model(np.float64, ulps=2, seed=5)), e2, T2, V.chachiyo(n, imp), C_CHACHIYO)
        print("Chachiyo %d +-2 ulp: ratios %.2f %.2f" % (imp, res[0][1], res[1][1]))
        assert all(ok for ok, _, _ in res)


def test_gate_passes_another_libm_lsda():
    worst = 0.0
    for name, (na, nb) in V.lsda_inputs().items():
        ext, T = V.lsda(na.astype(LD), nb.astype(LD), scale=True)
        res = through_gate(V.lsda(na, nb, model=V.Model(np.float64, ulps=2, seed=1)), ext, T, oracle_lsda(na, nb), C_LSDA)
        assert all(ok for ok, _, _ in res), (name, res)
        worst = max(worst, max(r for _, r, _ in res))
    print("LSDA +-2 ulp: largest ratio %.2f" % worst)


def test_gate_rejects_truncated_third(lda_case):
    n, ext, T, orc = lda_case
    out = V.lda(n, model=V.Model(np.float64, third=0.333333333333))
    assert V.old_gate(out[0], orc[0]) and V.old_gate(out[1], orc[1])               # what test_vwn_vs_golden asks
    res = through_gate(out, ext, T, orc, C_LDA)
    print("1/3 -> 0.333333333333: ratios %.0f (Vexc) %.0f (eexcDif)" % (res[0][1], res[1][1]))
    assert not res[1][0] and res[1][1] > 100


@pytest.mark.parametrize("zeta", IDENTITY_ZETAS)
def test_gate_rejects_changed_fit_constant(zeta):
    rho = V.ladder(1025)
    na, nb = rho * ((1 + zeta) / 2), rho * ((1 - zeta) / 2)
    ext, T = V.lsda(na.astype(LD), nb.astype(LD), scale=True)
    res = through_gate(V.lsda(na, nb, model=V.Model(np.float64, ferro_b=7.06043)), ext, T, oracle_lsda(na, nb), C_LSDA)
    print("kFerro.b 7.06043, zeta %+.3f: ratios %s" % (zeta, " ".join("%.3g" % r for _, r, _ in res)))
    if zeta == 0.0:
        assert all(ok for ok, _, _ in res)
    else:
        assert not any(ok for ok, _, _ in res) and min(r for _, r, _ in res) > 100
