// pseudo_plan.h -- the host side of the Troullier-Martins pseudization (pseudo.hip): what a call accepts, the default choice of the
// valence levels and of the core node.  Host-only and pure: no HIP call, no environment.  include/dftatom_hip.h has the arithmetic;
// DESIGN.md 4.15 the shape.
#pragma once

#include <cstddef>

namespace dfta_pseudo_plan {

constexpr int kLmax = 4;                 // l of a channel
constexpr int kLanes = 256;              // lanes of a channel's workgroup: lane t adds the norm's increments of the nodes t, t + 256, ..
constexpr int kCoef = 7;                 // a0, a2, .., a12
constexpr int kMatch = 8;                // P0 .. P4, I_AE, I_ps, g
constexpr int kEdge = 3;                 // nodes that the core node keeps from either end
constexpr int kBracketSteps = 24;        // expansions of the bracketing search
constexpr int kIterCap = 200;            // evaluations of g in a channel, the bracketing included (a root within 2^-70 of 0 would need more)

struct Call {                            // the arguments of dfta_pseudize that the planner reads (host pointers)
    int N, nch;
    const int* l;
    const int* ic;
};

// null, or what is wrong with the call: N < 8, nch < 0, a null l or ic with nch > 0, an l outside 0 .. 4, a core node outside
// 3 .. N-4 (the five-point stencils at ic and the increment of node ic read ic-2 .. ic+2)
const char* check(const Call& c);

// the valence levels of a configuration: for each l the occupied level (occ[k] > 0) of largest n, kept if n >= n_max - max(0, l - 1),
// n_max the largest n of an occupied level.  pick: the kept indices, ascending in l; returns their number, -1 if cap is too small or
// an argument is null / an l is negative.
int default_valence(int nlev, const int* n, const int* l, const int* occ, int* pick, int cap);

// the default core node of an orbital u on the nodes r (N each): the node whose r is nearest to factor x r_peak, r_peak = r at the
// first largest |u| (the lower node on a tie of distances), then moved outwards until it lies beyond the last sign change of u and
// u is non-zero there, and clamped to 3 .. N-4.  -1: null pointers, N < 8, a factor that is not finite and positive.
int default_ic(int N, const double* r, const double* u, double factor);

}  // namespace dfta_pseudo_plan
