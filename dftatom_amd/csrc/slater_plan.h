// slater_plan.h -- the host side of the Slater integrals (slater.hip): the angular factor (l k l'; 0 0 0)^2, the job tables of the
// F^k / G^k table and of the Hartree / exact-exchange energies, the validation of a caller's table and the two energy sums.
// Host-only and pure: no HIP call, no environment.  include/dftatom_hip.h has the definitions and the orders stated here.
#pragma once

#include <vector>

namespace dfta_slater {

constexpr int kKmax = 8;         // DFTA_SLATER_KMAX
constexpr int kLmax = 4;         // l of an orbital of a table: 2 l <= kKmax
constexpr int kJobInts = 5;      // a row of a job table: a, b, c, d, k
constexpr int kKindF = 0, kKindG = 1;

// (la k lb; 0 0 0)^2 from the factorial closed form, one rounding (the reduced fraction is formed in integers); 0 / non-zero status
int gaunt_3j2(int la, int k, int lb, double* out);

// rows a,b,c,d,k of the F^k(a,b) = R^k(ab,ab), a <= b, k = 0, 2 .. 2 min(la, lb) -- rows a, then b, then k ascending -- followed by the
// G^k(a,b) = R^k(ab,ba), a < b, k = |la - lb|, |la - lb| + 2 .. la + lb in the same order.  jobs / kinds may be null (count only).
// Returns the number of jobs, or -1: norb < 0, a null l, an l outside 0 .. kLmax.
int fg_jobs(int norb, const int* l, int* jobs, int* kinds);

// null, or what is wrong with the table (indices outside 0 .. norb-1, k outside 0 .. kKmax)
const char* check_jobs(int norb, int njobs, const int* jobs);

// The one launch of dfta_scf_coulomb_exchange.  Orbitals 0 .. nA-1 are the alpha channel (LDA: the only one), nA .. nA+nB-1 the beta
// channel.  jobs: F^0(i,j) of every pair i <= j of the atom (rows i, then j); then per channel, alpha first, rows a, then b >= a, then k
// ascending: F^k(a,a), k = 2 .. 2 la (b == a) and G^k(a,b) (b > a).
struct EnergyPlan {
    int norb = 0, nA = 0;
    std::vector<int> l;
    std::vector<int> jobs;       // kJobInts per job
    std::vector<int> f0;         // norb x norb: the job of F^0(i,j), mirrored
    std::vector<int> gk;         // (kKmax + 1) x norb x norb: the job of G^k(a,b) (a == b: F^k(a,a)), mirrored; -1: none
    int njobs() const { return (int)(jobs.size() / kJobInts); }
};
int plan_energy(int nA, int nB, const int* l, EnergyPlan* plan);     // 0, or -1 (an l outside 0 .. kLmax)

// E_H = 1/2 Sum_i Sum_j (N_i N_j) F^0(i,j): rows i, then j, one accumulator from 0.  E_x = -1/2 Sum_sigma Sum_a Sum_b (n_a n_b) T_ab,
// T_ab = Sum_k (la k lb; 0 0 0)^2 G^k(a,b), k ascending from 0: one accumulator S over the channels (alpha first), rows a, then b (all
// b of the channel, the mirrored value below the diagonal).  lsda: n = N, E_x = -0.5 S; LDA: n = 0.5 N in two equal channels, E_x = -S.
void energy_sums(const EnergyPlan& plan, const double* occ, int lsda, const double* R, double* EH, double* EXX);

}  // namespace dfta_slater
