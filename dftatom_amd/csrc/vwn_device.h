// vwn_device.h -- the node arithmetic of the Vosko-Wilk-Nusair kernels as device functions, shared by xc.hip (k_vwn_lda, k_vwn_lsda) and
// by the orbital xc of the self-interaction correction (kli_stage.hip: k_sic_pointwise): one statement of each order of operations, so
// that v_up[rho_a, 0] of an orbital density is bit for bit what dfta_vwn_lsda returns on (rho_a, 0).  Expressions are written in the
// reference's operation order (VWNExcCor.h); pow / log / atan come from the ROCm device library.
#pragma once
#include <hip/hip_runtime.h>

namespace dfta_vwn_dev {

constexpr double kPi = 3.14159265358979323846;
constexpr double kFourPi = 4. * kPi;
constexpr double kThird = 1. / 3.;                                  // ExcCorBase.h:12

// One Pade-like fit of VWN: eps(y) = A { ln(y^2/Y) + 2b/Q atan(Q/(2y+b)) - b y0/Y0 [ ln((y-y0)^2/Y) + 2(b+2y0)/Q atan(Q/(2y+b)) ] },
// y = sqrt(rs), Y(y) = y^2 + b y + c, Q = sqrt(4c - b^2).  Three parameter sets (VWNExcCor.h:23-41): paramagnetic,
// ferromagnetic, and the spin stiffness alpha_c.
struct VwnFit { double A, y0, b, c; };
constexpr VwnFit kPara{0.0310907, -0.10498, 3.72744, 12.93532};
constexpr VwnFit kFerro{0.01554535, -0.325, 7.06042, 18.0578};
constexpr VwnFit kStiff{-1. / (6. * kPi * kPi), -0.0047584, 1.13107, 13.0045};
constexpr double poly_at(const VwnFit& p, double y) { return y * y + p.b * y + p.c; }

struct FitValue { double eps, slope; };     // eps: the fit itself (VWNExcCor.h:43-50); slope: its rs-derivative term (VWNExcCor.h:52-55)

// NESTED selects how Y(y) is rounded: the LDA routines write y*y + b*y + c (VWNExcCor.h:89,119), the LSDA ones y*(y + b) + c
// (VWNExcCor.h:182,187,192) -- both kept so that each path rounds like the reference's
template <bool NESTED>
__device__ __forceinline__ FitValue eval_fit(const VwnFit p, double y)
{
    const double Y = NESTED ? y * (y + p.b) + p.c : y * y + p.b * y + p.c;
    const double Y0 = poly_at(p, p.y0);
    const double dy = y - p.y0;
    const double Q = sqrt(4 * p.c - p.b * p.b);
    const double at = atan(Q / (2. * y + p.b));
    FitValue v;
    v.eps = p.A * (log(y * y / Y) + 2. * p.b / Q * at - p.b * p.y0 / Y0 * (log(dy * dy / Y) + 2. * (p.b + 2. * p.y0) / Q * at));
    v.slope = p.A * (p.c * dy - p.b * p.y0 * y) / (dy * Y);
    return v;
}

__device__ __forceinline__ double wigner_seitz(double rho) { return pow(3. / (kFourPi * rho), kThird); }   // rs, eq 2 of the NIST note

// the constants k_vwn_lsda forms from cbrt2 = 2^(1/3) before its loop
struct LsdaConsts { double cx, cbrt2, gdd, gscale, dgscale; };
__device__ __forceinline__ LsdaConsts lsda_consts(double cx, double cbrt2)
{
    LsdaConsts k;
    k.cx = cx; k.cbrt2 = cbrt2;
    k.gdd = 4. / (9. * (cbrt2 - 1.));
    k.gscale = 1. / (2. * (cbrt2 - 1.)); k.dgscale = 2. / (3. * (cbrt2 - 1.));               // ExcCorBase.h:16,23
    return k;
}

struct LsdaPoint { double common, vup, vdn, e; };                   // res, va, vb, eexc of dfta_vwn_lsda at one node

// LSDA at one node (VWNExcCor.h:134-312).  With g(zeta) the spin interpolation of ExcCorBase.h:14-19, g''(0) = gdd and
//     w(zeta) = g / gdd * (1 + beta zeta^4),   beta = gdd (eps_F - eps_P) / alpha_c - 1
// the correlation energy is eps_P + alpha_c w (eqs 7-10 of the NIST note); its rs-derivative (`drs`) and its zeta-derivative (`dz`)
// give the common term and the two spin potentials.
__device__ __forceinline__ LsdaPoint lsda_point(const LsdaConsts k, double up, double dn)
{
    const double cx = k.cx, cbrt2 = k.cbrt2, gdd = k.gdd, gscale = k.gscale, dgscale = k.dgscale;
    const double tot = up + dn;
    double common = 0., vup = 0., vdn = 0., e = 0.;
    if (!(tot < 1E-18)) {                                         // VWNExcCor.h:160,260
        const double rs = wigner_seitz(tot);
        const double z = (up - dn) / tot;
        const double z3 = z * z * z, z4 = z3 * z;
        const double g = gscale * (pow(1. + z, 4. * kThird) + pow(1. - z, 4. * kThird) - 2.);
        const double dg = dgscale * (pow(1. + z, kThird) - pow(1. - z, kThird));
        const double y = sqrt(rs);
        const FitValue P = eval_fit<true>(kPara, y), F = eval_fit<true>(kFerro, y), S = eval_fit<true>(kStiff, y);

        const double gap = F.eps - P.eps;                                             // VWNExcCor.h:202
        const double beta = gdd * gap / S.eps - 1.;
        const double env = 1. + beta * z4;
        const double w = g / gdd * env;
        const double dbeta = gdd / S.eps * (F.slope - P.slope - S.slope * gap / S.eps);   // VWNExcCor.h:208
        const double dw = g / gdd * z4 * dbeta;
        const double drs = kThird * (P.slope + S.slope * w + S.eps * dw);             // VWNExcCor.h:212-213
        const double dz = S.eps / gdd * (4. * beta * z3 * g + env * dg);               // VWNExcCor.h:216

        const double xP = -cx / rs;                                                    // exchange of the unpolarised gas ...
        const double xF = cbrt2 * xP;                                                  // ... and of the fully polarised one
        common = P.eps + S.eps * w - drs;                                              // VWNExcCor.h:219-231
        vup = -(cx * cbrt2) / wigner_seitz(up) + common + (1. - z) * dz;               // VWNExcCor.h:233
        vdn = -(cx * cbrt2) / wigner_seitz(dn) + common - (1. + z) * dz;               // VWNExcCor.h:234
        common += (xP + (xF - xP) * g);                                                // VWNExcCor.h:236

        const double xPd = (0.25 * cx) / rs;                                           // VWNExcCor.h:271-272
        e = xPd + (cbrt2 * xPd - xPd) * g + drs;                                       // VWNExcCor.h:306-308
    }
    LsdaPoint p;
    p.common = common; p.vup = vup; p.vdn = vdn; p.e = e;
    return p;
}

}  // namespace dfta_vwn_dev
