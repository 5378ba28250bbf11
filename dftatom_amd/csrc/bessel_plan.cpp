// bessel_plan.cpp -- see bessel_plan.h.  Pure host code (no HIP include).
#include "bessel_plan.h"

#include <cmath>

#include "../../include/dftatom_hip.h"

namespace dfta_bessel {

static_assert(DFTA_BT_DENSITY == 0 && DFTA_BT_ORBITAL == 1, "bessel_plan.cpp and the header disagree");
static_assert(kLmax == DFTA_BESSEL_LMAX, "bessel_plan.h and the header disagree");

const char* check_transform(int kind, int nrow, const int* l, int nq, const double* q)
{
    if (kind != DFTA_BT_DENSITY && kind != DFTA_BT_ORBITAL) return "Bessel transform: kind (DFTA_BT_DENSITY or DFTA_BT_ORBITAL)";
    for (int a = 0; a < nrow; ++a)
        if (l[a] < 0 || l[a] > kLmax) return "Bessel transform: l outside 0 .. 4";
    for (int m = 0; m < nq; ++m)
        if (!(q[m] >= 0.) || std::isinf(q[m])) return "Bessel transform: q must be finite and >= 0";
    return nullptr;
}

long num_blocks(int nrow, int nq, int qb) { return (long)nrow * ((nq + qb - 1) / qb); }

int pick_qblock(int nrow, int nq, int num_cu, int forced)
{
    if (forced == 1 || forced == 2 || forced == 4 || forced == 8) return forced;
    for (int qb = kQBlockMax; qb > 1; qb >>= 1)
        if (num_blocks(nrow, nq, qb) >= num_cu) return qb;
    return 1;
}

}  // namespace dfta_bessel
