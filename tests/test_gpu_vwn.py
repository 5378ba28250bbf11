"""GPU suite (-m gpu): k_vwn_lda, k_vwn_lsda and k_chachiyo_lda (xc.hip) on their own, through dfta_vwn_lda / dfta_vwn_lsda /
dfta_chachiyo_lda, against tests/_vwn_ref.py evaluated in EXTENDED precision (np.longdouble).  This file states the VWN gate; the
header of xc.hip and the header of test_gpu_parity.py point here.

The measure is the one of test_gpu_xc_radial.py, per output and point j of a ladder that is contiguous in rho:

    |gpu - ref_ext|(j)  <=  8 E(j) + c eps T(j)                                    (_vwn_ref.gate)

E(j): |oracle64 - ref_ext| of the fp64 oracle (dfo_vwn_*; Chachiyo, which the oracle does not have: the float64 evaluation of
      _vwn_ref.chachiyo, which test_vwn_ref.py holds to the golden vectors of the compiled reference), as a running maximum over
      j-8 .. j+8 within the ladder: what fp64 arithmetic costs these formulas at this density -- the cancellation of ln(y^2 / Y)
      against the atan term at large r_s, the rounded 1/3 in pow, zeta near +-1 -- measured, not chosen (maxima in test_vwn_ref.py);
      the factor 8 is that file's, for device elementary functions that differ from the host's;
T(j): the sum of the magnitudes of the terms the output is assembled from (_vwn_ref, scale=True); eps = 2^-52;
c:    counted from the kernel, one per rounding between the elementary-function results and the output, plus the bounds the HIP
      math API reference gives for the double-precision device functions (sqrt, pow, log, atan: 1 ulp each):
      k_vwn_lda      Y 4 (y y, b y, two sums), dy 1, the atan argument 2, the two log arguments 2 + 2, eps 7 (2b/Q at, +, the
                     second product, +, b y0 / Y0 (..), -, A (..)), slope 6, the output 4 (c_x / r_s, + eps, slope / 3, -)  = 28
                     roundings; pow, sqrt, atan, 2 log = 5 ulp:                                                       c = 33
      k_chachiyo_lda the tail 10 (q1, q2, two sums, a / (..), q1 + 2 q2, three products / quotients), the log argument 3, a log 1,
                     c_x / r_s 1, the two sums of the output 2 = 17 roundings; pow, log = 2 ulp:                       c = 19
      k_vwn_lsda     three fits of 3 (Y nested) + 1 + 2 + 4 + 7 + 6 = 23: 69; total, zeta, zeta^3, zeta^4 6; g 5, dg 2; gap, beta,
                     env, w, dbeta, dw, drs, dzeta 1 + 3 + 2 + 2 + 6 + 3 + 5 + 7 = 29; x_P, x_F 2; common 2; the channel's own
                     exchange 3; the output 4 = 122 roundings; 3 atan, 6 log, sqrt, 6 pow = 16 ulp:                   c = 138
      (the largest count of the four outputs, used for all of them).
Below the threshold (total density < 1e-18, -0.0 and a negative total included) every output is exactly 0; where the extended
reference is NaN or infinite (a NaN density, rho = +Inf, a negative channel: zeta outside [-1, 1]) the kernel has what the oracle has.

Observed maxima of |gpu - ref_ext| / (8 E + c eps T) on an MI355X (every test prints its own): LDA Vexc 0.14, eexcDif 0.07; Chachiyo
0.09 / 0.08 (both sets); LSDA with proportional channels res / va / vb 0.14, eexcDif 0.03, with an idle channel 0.18, with totals
crossing the threshold 0.13; vwn_lsda(n / 2, n / 2) against the LDA reference 0.24.  No zero, NaN or infinity out of place.

Position independence: the launches are min(ceil(sz / 256), 2048) blocks of 256 threads with a grid-stride loop, which no ladder
above enters; an input of 2048 * 256 + 257 points that repeats a 1021-point piece (1021 is prime: every value meets many lanes
and both trips of the loop) must give, point by point, the bits of the 1021-point call.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import _vwn_ref as V                     # noqa: E402
import dftatom_amd as D                  # noqa: E402

LD = np.longdouble
LDA_NAMES = ("Vexc", "eexcDif")
LSDA_NAMES = ("res", "va", "vb", "eexcDif")
LSDA_CASES = V.lsda_inputs()


@pytest.fixture(scope="module")
def ctx(torch_first):
    assert np.finfo(LD).eps < 1.2e-19, "the reference of this file needs an extended np.longdouble"
    c = D.Context(0)
    yield c
    c.close()


def bits(x):
    return np.ascontiguousarray(x).view(np.int64)


def check(label, names, got, ext, T, orc, c):
    """the module docstring's assertions for every output; prints and returns the largest ratio"""
    worst = 0.0
    for name, g, x, t, y in zip(names, got, ext, T, orc):
        ok, ratio, j = V.gate(g, x, t, y, c)
        print("%-28s %-7s max |gpu - ref_ext| / (8 E + %d eps T) = %.3f at point %d" % (label, name, c, ratio, j))
        assert ok, (label, name, ratio, j, g[j], float(x[j]))
        worst = max(worst, ratio)
    return worst


def test_lda_ladder(ctx):
    n = V.lda_input()
    got = D.vwn_lda(ctx, n)
    ext, T = V.lda(n.astype(LD), scale=True)
    check("VWN LDA", LDA_NAMES, got, ext, T, V.oracle_lda(n), V.C_LDA)
    for g in got:
        assert np.all(bits(g[:4]) == 0) and g[-1] == 0.0 and bits(g[-1:])[0] == 0      # 0, -0, 1e-300, 9.99e-19, -1: +0.0
        assert g[4] != 0.0 and g[5] != 0.0 and np.isnan(g[-3]) and np.isinf(g[-2])     # 1e-18 itself is live


@pytest.mark.parametrize("improved", [False, True], ids=["original", "improved"])
def test_chachiyo_ladder(ctx, improved):
    n = V.lda_input()
    got = D.chachiyo_lda(ctx, n, improved=improved)
    ext, T = V.chachiyo(n.astype(LD), improved, scale=True)
    check("Chachiyo %d" % improved, LDA_NAMES, got, ext, T, V.chachiyo(n, improved), V.C_CHACHIYO)
    for g in got:
        assert np.all(bits(g[:4]) == 0) and bits(g[-1:])[0] == 0 and g[4] != 0.0 and np.isnan(g[-3]) and np.isnan(g[-2])      # rho = +Inf: a / Inf * Inf * 0


@pytest.mark.parametrize("name", sorted(LSDA_CASES))
def test_lsda_ladder(ctx, name):
    """proportional channels for every zeta, independent channels (one idle: 0, -0, 1e-30, 1e-19), totals that cross the threshold
    with one channel below / above it, a negative channel: the measure, the zeros and the oracle's NaN pattern; and the channels
    exchanged: va <-> vb, res and eexcDif unchanged, bit for bit"""
    na, nb = LSDA_CASES[name]
    got = D.vwn_lsda(ctx, na, nb)
    ext, T = V.lsda(na.astype(LD), nb.astype(LD), scale=True)
    orc = V.oracle_lsda(na, nb)
    check("VWN LSDA " + name, LSDA_NAMES, got, ext, T, orc, V.C_LSDA)
    total = na + nb
    dead = total < 1e-18
    for g, y in zip(got, orc):
        assert np.all(bits(g[dead]) == 0)
        assert np.array_equal(np.isnan(g), np.isnan(y))
    if name.startswith("cross"):
        assert dead.any() and not dead.all()
    res, va, vb, ee = got
    res2, va2, vb2, ee2 = D.vwn_lsda(ctx, nb, na)
    for x, y, n in ((res, res2, "res"), (va, vb2, "va"), (vb, va2, "vb"), (ee, ee2, "eexcDif")):
        assert np.array_equal(bits(x), bits(y)), (name, n, int(np.sum(bits(x) != bits(y))))


def test_lsda_of_equal_channels_is_lda(ctx):
    """vwn_lsda(n / 2, n / 2) against the LDA reference of n, in the same measure (n / 2 + n / 2 = n exactly): the two kernels
    round Y(y) differently on purpose (VWNExcCor.h:89 against 182), so their bits may differ and the extended value decides.
    Without rho = +Inf, where zeta = (Inf - Inf) / Inf is NaN and the LDA value is -Inf"""
    n = np.concatenate([V.lda_input()[:-3], [np.nan, -1.0]])
    res, va, vb, ee = D.vwn_lsda(ctx, n / 2, n / 2)
    (v, e), (Tv, Te) = V.lda(n.astype(LD), scale=True)
    ov, oe = V.oracle_lda(n)
    check("VWN LSDA(n/2, n/2) vs LDA", LSDA_NAMES, (res, va, vb, ee), (v, v, v, e), (Tv, Tv, Tv, Te), (ov, ov, ov, oe), V.C_LSDA)
    ok = np.isfinite(va)                          # (1 - z) dz and -(1 + z) dz of a NaN density: NaNs of either sign
    assert np.array_equal(bits(va[ok]), bits(vb[ok])) and np.array_equal(np.isnan(va), np.isnan(vb)) and not ok.all()


PIECE = 1021
BIG = 2048 * 256 + 257


def lda_piece():
    n = V.lda_input()
    return np.concatenate([n[:6], n[6:-3][np.linspace(0, n.size - 10, PIECE - 9).astype(int)], n[-3:]])


def lsda_piece():
    parts_a, parts_b = [], []
    for name in ("zeta+0.3", "zeta-0.77", "zeta+1", "idle_a2", "idle_b1", "cross_low", "cross_high", "negative_b"):
        na, nb = LSDA_CASES[name]
        parts_a.append(na[::8])
        parts_b.append(nb[::8])
    na, nb = np.concatenate(parts_a), np.concatenate(parts_b)
    return np.resize(na, PIECE), np.resize(nb, PIECE)


@pytest.mark.parametrize("kernel", ["lda", "lsda", "chachiyo"])
def test_position_independence(ctx, kernel):
    """the grid-stride path: one launch of 2048 * 256 + 257 points, every output the bits of the same value in the 1021-point call"""
    if kernel == "lsda":
        pa, pb = lsda_piece()
        small = D.vwn_lsda(ctx, pa, pb)
        big = D.vwn_lsda(ctx, np.resize(pa, BIG), np.resize(pb, BIG))
    else:
        p = lda_piece()
        f = D.vwn_lda if kernel == "lda" else (lambda c, x: D.chachiyo_lda(c, x, improved=True))
        small = f(ctx, p)
        big = f(ctx, np.resize(p, BIG))
    assert small[0].size == PIECE and big[0].size == BIG and BIG > 2048 * 256 and BIG % PIECE != 0
    live = 0
    for s, b in zip(small, big):
        assert np.isnan(s).any() and (s == 0).any()
        live += int(np.sum(np.isfinite(s) & (s != 0)))
        diff = bits(b) != bits(np.resize(s, BIG))
        assert not diff.any(), (kernel, int(diff.sum()), int(np.argmax(diff)))
    assert live > PIECE
