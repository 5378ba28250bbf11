// bessel_plan.h -- the host side of the Bessel transforms (bessel.hip): what a call accepts, and how many q's a workgroup takes.
// Host-only and pure: no HIP call, no environment.  include/dftatom_hip.h has the definitions; DESIGN.md 4.10 the shape.
#pragma once

#include <cstddef>

namespace dfta_bessel {

constexpr int kLmax = 4;                 // order of j_l: the l range of the Slater block
constexpr int kSeriesTerms = 14;         // terms t_0 .. t_13 of the ascending series (below kSwitch)
constexpr double kSwitch = 3.0;          // x < kSwitch: series; x >= kSwitch: sincos and the upward recurrence
constexpr int kQBlockMax = 8;            // q's per workgroup: 8, 4, 2 or 1

// null, or what is wrong with the table of a transform (kind outside {0, 1}, an l outside 0 .. kLmax, a q that is negative, NaN or
// infinite).  The pointers are non-null where their count is positive.
const char* check_transform(int kind, int nrow, const int* l, int nq, const double* q);

// q's per workgroup of k_bessel_transform: the largest of 8, 4, 2, 1 for which nrow * ceil(nq / QB) workgroups still fill num_cu
// compute units (1 where none does); forced = 1, 2, 4 or 8 (the knob BESSEL_QBLOCK) is taken as it is, any other value is ignored.
// A q's bits do not depend on the choice: every q has its own accumulator and its own tree.
int pick_qblock(int nrow, int nq, int num_cu, int forced);

// workgroups of the launch: nrow * ceil(nq / qb)
long num_blocks(int nrow, int nq, int qb);

}  // namespace dfta_bessel
