// exchange_plan.h -- the host side of the exchange potentials (exchange.hip): the job table of the screening functions y^k_ab of a spin
// channel, the pointwise table of the exchange operator, the table of the reductions, the HOMO rule, the validation of a caller's
// tables and the reduced linear solve of the KLI constants.  Host-only and pure: no HIP call, no environment.
// include/dftatom_hip.h has the definitions and the orders stated here.
#pragma once

#include <vector>

namespace dfta_exchange {

constexpr int kKmax = 8;         // DFTA_SLATER_KMAX
constexpr int kLmax = 4;         // l of a shell of a channel: 2 l <= kKmax
constexpr int kJobInts = 3;      // a row of a y-job table: x, y, k
constexpr int kTabInts = 4;      // a row of the pointwise table: a, b, k, row of y^k_ab among the channel's y jobs
constexpr int kRedInts = 3;      // a row of the reduction table: kind, a, b
constexpr int kShellsMax = 32;   // shells of a channel (plan_scf_config allows 32)
enum { kRedHF = 0, kRedS = 1, kRedPair = 2, kRedKLI = 3 };

// the y jobs of a channel with angular momenta l: rows a, then b >= a, then k = |la - lb|, |la - lb| + 2 .. la + lb ascending (b == a:
// the F-type jobs k = 0, 2 .. 2 la; b > a: the G-type jobs).  jobs may be null (count only).  Returns the number of jobs, or -1:
// norb < 0, a null l, an l outside 0 .. kLmax.
int y_jobs(int norb, const int* l, int* jobs);

// null, or what is wrong with a caller's y-job table (indices outside 0 .. norb-1, k outside 0 .. kKmax)
const char* check_jobs(int norb, int njobs, const int* jobs);

// null, or what is wrong with a channel (norb outside 1 .. kShellsMax, an l outside 0 .. kLmax, a negative or non-finite occupation, homo
// outside 0 .. norb-1)
const char* check_channel(int norb, const int* l, const double* occ, int homo);

// the HOMO of a channel: the highest eigenvalue among the shells with occ > 0, ties to the higher index; -1: no occupied shell
int pick_homo(int norb, const double* E, const double* occ);

// Everything the launches of one channel need.  tab / coef: for every a ascending the entries of X_a -- b ascending (every b of the
// channel), then k ascending --, coef = occ_b * (la k lb; 0 0 0)^2 (one product), row the y job of (min(a,b), max(a,b), k);
// first[a] .. first[a+1]: the entries of X_a.  red1: vbarHF_a (a ascending), vbarS_a, then S_ab of every pair a <= b row by row;
// red2: vbarKLI_a.
struct ChannelPlan {
    int norb = 0;
    std::vector<int> jobs;       // kJobInts per y job
    std::vector<int> first;      // norb + 1
    std::vector<int> tab;        // kTabInts per entry
    std::vector<double> coef;    // per entry
    std::vector<int> red1, red2; // kRedInts per reduction
    int njobs() const { return (int)(jobs.size() / kJobInts); }
    int nred1() const { return (int)(red1.size() / kRedInts); }
    int nred2() const { return (int)(red2.size() / kRedInts); }
};
int plan_channel(int norb, const int* l, const double* occ, ChannelPlan* plan);      // 0, or -1 (check_channel fails without the homo)

// The KLI constants: c[homo] = 0, the others solve (I - M)_red c = (vbarS - vbarHF)_red, rows and columns `homo` removed, M row-major
// norb x norb.  Gaussian elimination with partial pivoting in double, in this order: for every column j ascending the pivot is the row
// p >= j of largest |A_pj| (the lowest on ties), rows j and p are exchanged; for every row i > j ascending f = A_ij / A_jj, then for m > j
// ascending A_im = A_im - f A_jm, then b_i = b_i - f b_j.  Back substitution for i descending: t = b_i, for m > i ascending
// t = t - A_im x_m, x_i = t / A_ii.  Returns 0, or -1: a pivot that is zero or not finite (c is then all zeros).
int solve_kli(int norb, int homo, const double* M, const double* vbarS, const double* vbarHF, double* c);

}  // namespace dfta_exchange
