// pseudo_plan.cpp -- see pseudo_plan.h.  Pure host code (no HIP include).
#include "pseudo_plan.h"

#include <algorithm>
#include <cmath>

#include "../../include/dftatom_hip.h"

namespace dfta_pseudo_plan {

static_assert(kCoef == DFTA_PS_COEF, "pseudo_plan.h and the header disagree");
static_assert(kMatch == DFTA_PS_MATCH, "pseudo_plan.h and the header disagree");
static_assert(kLmax == DFTA_BESSEL_LMAX, "pseudo_plan.h and the header disagree");

const char* check(const Call& c)
{
    if (c.N < 8) return "pseudize: the grid needs 8 nodes";
    if (c.nch < 0) return "pseudize: nch";
    if (c.nch > 0 && (!c.l || !c.ic)) return "pseudize: l, ic";
    for (int k = 0; k < c.nch; ++k) {
        if (c.l[k] < 0 || c.l[k] > kLmax) return "pseudize: l outside 0 .. 4";
        if (c.ic[k] < kEdge || c.ic[k] > c.N - 1 - kEdge) return "pseudize: a core node closer than 3 nodes to an end of the grid";
    }
    return nullptr;
}

int default_valence(int nlev, const int* n, const int* l, const int* occ, int* pick, int cap)
{
    if (nlev < 0 || (nlev > 0 && (!n || !l || !occ)) || !pick) return -1;
    int nmax = -1, lmax = -1;
    for (int k = 0; k < nlev; ++k) {
        if (l[k] < 0) return -1;
        if (occ[k] > 0) { nmax = std::max(nmax, n[k]); lmax = std::max(lmax, l[k]); }
    }
    int cnt = 0;
    for (int ll = 0; ll <= lmax; ++ll) {
        int best = -1;
        for (int k = 0; k < nlev; ++k)
            if (occ[k] > 0 && l[k] == ll && (best < 0 || n[k] > n[best])) best = k;
        if (best < 0 || n[best] < nmax - std::max(0, ll - 1)) continue;
        if (cnt >= cap) return -1;
        pick[cnt++] = best;
    }
    return cnt;
}

int default_ic(int N, const double* r, const double* u, double factor)
{
    if (!r || !u || N < 8 || !(factor > 0.) || !std::isfinite(factor)) return -1;
    int peak = 0;
    for (int i = 1; i < N; ++i)
        if (std::fabs(u[i]) > std::fabs(u[peak])) peak = i;
    const double target = factor * r[peak];
    int ic = 0;
    for (int i = 1; i < N; ++i)
        if (std::fabs(r[i] - target) < std::fabs(r[ic] - target)) ic = i;
    int last = 0;                                    // the last sign change of u: between last - 1 and last
    for (int i = 2; i < N; ++i) {
        const double b = u[i - 1] != 0. ? u[i - 1] : u[i - 2];      // (through one exact zero)
        if ((u[i] < 0. && b > 0.) || (u[i] > 0. && b < 0.)) last = i;
    }
    ic = std::max(ic, last + 1);
    while (ic < N - 1 - kEdge && u[ic] == 0.) ++ic;
    return std::min(std::max(ic, kEdge), N - 1 - kEdge);
}

}  // namespace dfta_pseudo_plan
