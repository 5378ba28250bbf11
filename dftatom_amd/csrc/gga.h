// gga.h -- Perdew-Wang 1992 correlation and the PBE exchange-correlation energy density, with all partial derivatives, as device
// functions shared by the pointwise PW92 kernels (xc.hip) and the fused PBE kernels (gga.hip).
//
// Everything is per volume and in Hartree atomic units.  xc_point<POL, GGA> returns e(rho_a, rho_b, s_aa, s_ab, s_bb) and
// de/drho_a, de/drho_b, de/ds_aa, de/ds_ab, de/ds_bb (s_xy = grad rho_x . grad rho_y).  Unpolarised (POL = false): rho = rho_a,
// sigma = s_aa, and only e, da and dsaa are meaningful.  GGA = false is Slater exchange + PW92 (the sigmas are ignored).
//
// Thresholds (1e-18, the VWN one, VWNExcCor.h:82): a total density below it gives all zeros; a spin channel below it has no
// exchange and pins zeta to +-1 exactly, and zeta is then a constant (no de/dzeta term), so every output stays finite.
#pragma once
#include <hip/hip_runtime.h>

namespace dfta_gga {

constexpr double kPi = 3.14159265358979323846;
constexpr double kThreshold = 1E-18;
constexpr double kRsc = 0.23873241463784300365;        // 3 / (4 pi): rs = cbrt(kRsc / rho)
constexpr double kCx = 0.73855876638202240588;         // (3/4) (3/pi)^(1/3): e_x^LDA = -kCx rho^(4/3)
constexpr double kCs = 0.026121172985233599568;        // s^2 = kCs sigma / rho^(8/3)          (1 / (4 (3 pi^2)^(2/3)))
constexpr double kCt = 0.063468206097703704202;        // t^2 = kCt sigma / (phi^2 rho^(7/3))  (pi / (16 (3 pi^2)^(1/3)))
constexpr double kFden = 0.51984209978974632953;       // 2^(4/3) - 2
constexpr double kFz0 = 1.7099209341613656176;         // f''(0) = 8 / (9 (2^(4/3) - 2))
// PBE (Perdew, Burke, Ernzerhof, PRL 77, 3865 (1996))
constexpr double kKappa = 0.804;
constexpr double kBeta = 0.06672455060314922;
constexpr double kMu = kBeta * kPi * kPi / 3.;
constexpr double kGamma = (1. - 0.69314718055994530942) / (kPi * kPi);
constexpr double kBg = kBeta / kGamma;

// G(rs) = -2A (1 + a1 rs) ln(1 + 1 / (2A (b1 rs^1/2 + b2 rs + b3 rs^3/2 + b4 rs^2))) (Perdew, Wang, PRB 45, 13244 (1992), with the
// constants of the PBE reference code / libxc lda_c_pw_mod)
struct Pw92Fit { double A, a1, b1, b2, b3, b4; };
constexpr Pw92Fit kPw92Para{0.0310907, 0.21370, 7.5957, 3.5876, 1.6382, 0.49294};
constexpr Pw92Fit kPw92Ferro{0.01554535, 0.20548, 14.1189, 6.1977, 3.3662, 0.62517};
constexpr Pw92Fit kPw92Stiff{0.0168869, 0.11125, 10.357, 3.6231, 0.88026, 0.49671};   // G = -alpha_c

struct Pw92Value { double g, drs; };      // G and dG/drs
__device__ __forceinline__ Pw92Value pw92_G(const Pw92Fit p, double rs, double srs)
{
    const double Q = srs * (p.b1 + srs * (p.b2 + srs * (p.b3 + srs * p.b4)));
    const double dQ = p.b1 / (2. * srs) + p.b2 + 1.5 * p.b3 * srs + 2. * p.b4 * rs;
    const double L = log1p(1. / (2. * p.A * Q));
    Pw92Value v;
    v.g = -2. * p.A * (1. + p.a1 * rs) * L;
    v.drs = -2. * p.A * p.a1 * L + (1. + p.a1 * rs) * dQ / (Q * (Q + 1. / (2. * p.A)));
    return v;
}

// eps_c(rs, zeta) = eps_0 + alpha_c f (1 - z^4) / f''(0) + (eps_1 - eps_0) f z^4 and its rs- and zeta-derivatives
struct Pw92Spin { double ec, drs, dz; };
template <bool POL>
__device__ __forceinline__ Pw92Spin pw92(double rs, double z, double cp, double cm)      // cp, cm: cbrt(1 + z), cbrt(1 - z)
{
    const double srs = sqrt(rs);
    const Pw92Value P = pw92_G(kPw92Para, rs, srs);
    if (!POL) return {P.g, P.drs, 0.};
    const Pw92Value F = pw92_G(kPw92Ferro, rs, srs), S = pw92_G(kPw92Stiff, rs, srs);
    const double f = ((1. + z) * cp + (1. - z) * cm - 2.) / kFden;
    const double df = 4. / 3. * (cp - cm) / kFden;
    const double z3 = z * z * z, z4 = z3 * z;
    const double gap = F.g - P.g;
    Pw92Spin c;
    c.ec = P.g - S.g * f * (1. - z4) / kFz0 + gap * f * z4;
    c.drs = P.drs - S.drs * f * (1. - z4) / kFz0 + (F.drs - P.drs) * f * z4;
    c.dz = -S.g * (df * (1. - z4) - 4. * z3 * f) / kFz0 + gap * (df * z4 + 4. * z3 * f);
    return c;
}

// exchange of the unpolarised gas of density n > 0 and gradient square s: e = -kCx n^(4/3) F_x(p), p = s^2 of the paper
struct XValue { double e, dn, ds; };
template <bool GGA>
__device__ __forceinline__ XValue x_unpolarised(double n, double s)
{
    const double n13 = cbrt(n);
    const double elda = -kCx * n * n13;
    if (!GGA) return {elda, -4. / 3. * kCx * n13, 0.};
    const double pden = kCs / (n13 * n13 * n * n);           // dp/ds
    const double p = s * pden;
    const double den = kKappa + kMu * p;
    const double F = 1. + kKappa - kKappa * kKappa / den;
    const double dF = kKappa * kKappa * kMu / (den * den);
    return {elda * F, -kCx * n13 * (4. / 3. * F - 8. / 3. * p * dF), elda * dF * pden};
}

struct XcPoint { double e, da, db, dsaa, dsab, dsbb; };

template <bool POL, bool GGA>
__device__ __forceinline__ XcPoint xc_point(double na, double nb, double saa, double sab, double sbb)
{
    XcPoint o{0., 0., 0., 0., 0., 0.};
    const double rho = POL ? na + nb : na;
    if (rho < kThreshold || !(rho == rho)) return o;
    // exchange: E_x[a, b] = (E_x[2a] + E_x[2b]) / 2
    if (!POL) {
        const XValue x = x_unpolarised<GGA>(na, saa);
        o.e = x.e; o.da = x.dn; o.dsaa = x.ds;
    } else {
        if (!(na < kThreshold)) {
            const XValue x = x_unpolarised<GGA>(2. * na, 4. * saa);
            o.e += 0.5 * x.e; o.da = x.dn; o.dsaa = 2. * x.ds;
        }
        if (!(nb < kThreshold)) {
            const XValue x = x_unpolarised<GGA>(2. * nb, 4. * sbb);
            o.e += 0.5 * x.e; o.db = x.dn; o.dsbb = 2. * x.ds;
        }
    }
    // correlation
    double z = 0.;
    bool pinned = false;
    if (POL) {
        z = (na - nb) / rho;
        if (nb < kThreshold) { z = 1.; pinned = true; }
        else if (na < kThreshold) { z = -1.; pinned = true; }
    }
    const double cp = POL ? cbrt(1. + z) : 1., cm = POL ? cbrt(1. - z) : 1.;
    const double rs = cbrt(kRsc / rho);
    const Pw92Spin c = pw92<POL>(rs, z, cp, cm);
    double ec = rho * c.ec;
    double dedrho = c.ec - rs / 3. * c.drs;            // d(rho eps_c)/drho at fixed zeta
    double dedz = rho * c.dz;                          // d(rho eps_c)/dzeta at fixed rho
    double dsig = 0.;
    if (GGA) {
        const double sigma = POL ? (saa + sbb) + 2. * sab : saa;     // in this order: exchanging the spins exchanges the outputs' bits
        double phi = 1., dphi = 0.;
        if (POL) {
            phi = 0.5 * (cp * cp + cm * cm);
            dphi = ((cp > 0. ? 1. / cp : 0.) - (cm > 0. ? 1. / cm : 0.)) / 3.;
        }
        const double gphi3 = kGamma * phi * phi * phi;
        const double r13 = cbrt(rho);
        const double qs = kCt / (phi * phi * rho * rho * r13);     // dt^2/dsigma
        const double q = sigma * qs;                               // t^2
        const double w = expm1(-c.ec / gphi3);
        const double A = kBg / w;
        const double y = A * q;
        const double den = 1. + y * (1. + y);
        const double R = kBg * q * (1. + y) / den;
        const double H = gphi3 * log1p(R);
        const double HR = gphi3 / (1. + R);
        const double Hq = HR * kBg * (1. + 2. * y) / (den * den);
        const double HA = -HR * kBg * q * q * y * (2. + y) / (den * den);
        const double Aec = A * A * (w + 1.) / (kBg * gphi3);                 // dA/deps_c
        const double Aphi = -3. * c.ec / phi * Aec;                           // dA/dphi
        const double Hec = HA * Aec;
        const double Hphi = 3. * H / phi + HA * Aphi - 2. * q * Hq / phi;
        ec += rho * H;
        dedrho += H - rs / 3. * Hec * c.drs - 7. / 3. * q * Hq;
        dedz += rho * (Hec * c.dz + Hphi * dphi);
        dsig = rho * Hq * qs;
    }
    o.e += ec;
    if (!POL) {
        o.da += dedrho;
        o.dsaa += dsig;
    } else {
        o.da += pinned ? dedrho : dedrho + dedz * (1. - z) / rho;
        o.db += pinned ? dedrho : dedrho - dedz * (1. + z) / rho;
        o.dsaa += dsig;
        o.dsab = 2. * dsig;
        o.dsbb += dsig;
    }
    return o;
}

}  // namespace dfta_gga
