// bessel_device.h -- the device's spherical Bessel function j_l, 0 <= l <= 4, as include/dftatom_hip.h states it: one statement, used by
// bessel.hip (the pointwise entry and the transforms) and by continuum.hip (the matching to the Riccati functions), so that both return
// the same bits by construction.  DESIGN.md 4.10 has the two branches and the rounding count.
#pragma once
#include <hip/hip_runtime.h>

#include "bessel_plan.h"

namespace dfta_bessel {

// row l: 1 / (2l+1)!!, then c_k = 1 / (k (2l + 2k + 1)), k = 1 .. kSeriesTerms - 1, each the double nearest the quotient
#define DFTA_BC(l, k) (1. / ((k) * (2. * (l) + 2. * (k) + 1.)))
#define DFTA_BROW(d, l)                                                                                                                   \
    {d, DFTA_BC(l, 1), DFTA_BC(l, 2), DFTA_BC(l, 3), DFTA_BC(l, 4), DFTA_BC(l, 5), DFTA_BC(l, 6), DFTA_BC(l, 7), DFTA_BC(l, 8), DFTA_BC(l, 9), \
     DFTA_BC(l, 10), DFTA_BC(l, 11), DFTA_BC(l, 12), DFTA_BC(l, 13)}
static_assert(kSeriesTerms == 14, "the rows of kSeries have kSeriesTerms entries");
static __constant__ double kSeries[kLmax + 1][kSeriesTerms] = {DFTA_BROW(1., 0), DFTA_BROW(1. / 3., 1), DFTA_BROW(1. / 15., 2),
                                                               DFTA_BROW(1. / 105., 3), DFTA_BROW(1. / 945., 4)};
#undef DFTA_BROW
#undef DFTA_BC

// j_l(x), x >= 0, as the header states it; l is the same in every lane
__device__ __forceinline__ double sph_bessel(int l, double x)
{
    if (x == 0.) return l == 0 ? 1. : 0.;
    if (l == 0) return sin(x) / x;
    if (x < kSwitch) {
        // x^l / (2l+1)!! (1 + z_1 (1 + z_2 (... (1 + z_13)))),  z_k = (-x^2 / 2) c_k
        const double* __restrict__ c = kSeries[l];
        const double y = (x * x) * -0.5;
        double h = 1. + y * c[kSeriesTerms - 1];
#pragma unroll
        for (int k = kSeriesTerms - 2; k >= 1; --k) h = 1. + (y * c[k]) * h;
        double p = x;
        for (int m = 1; m < l; ++m) p = p * x;
        return (p * c[0]) * h;
    }
    double s, co;
    sincos(x, &s, &co);
    const double rx = 1. / x;
    double jm = s * rx;                              // j_0
    double j = (jm - co) * rx;                       // j_1
    for (int k = 1; k < l; ++k) {                    // j_{k+1} = ((2k+1) / x) j_k - j_{k-1}
        const double jn = (((double)(2 * k + 1)) * rx) * j - jm;
        jm = j;
        j = jn;
    }
    return j;
}

}  // namespace dfta_bessel
