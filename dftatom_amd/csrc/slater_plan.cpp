// slater_plan.cpp -- see slater_plan.h.  Pure host code (no HIP include): the two host-only entries of the C ABI live here too.
#include "slater_plan.h"

#include <algorithm>
#include <cstdlib>

#include "../../include/dftatom_hip.h"

namespace dfta_slater {

static_assert(kKmax == DFTA_SLATER_KMAX, "slater_plan.h and the header disagree");

namespace {
constexpr int kPrimes[] = {2, 3, 5, 7, 11, 13, 17};          // (J + 1)! with J <= 2 kLmax + kKmax = 16
constexpr int kNumPrimes = sizeof(kPrimes) / sizeof(kPrimes[0]);

// e[q] += sign * (exponent of kPrimes[q] in n!)   (Legendre)
void add_factorial(int n, int sign, int* e)
{
    for (int q = 0; q < kNumPrimes; ++q)
        for (int m = n / kPrimes[q]; m > 0; m /= kPrimes[q]) e[q] += sign * m;
}
}  // namespace

int gaunt_3j2(int la, int k, int lb, double* out)
{
    if (!out || la < 0 || k < 0 || lb < 0 || la > kLmax || lb > kLmax) return DFTA_ERR_INVALID;
    *out = 0.;
    const int J = la + k + lb;
    if (J % 2 || k > la + lb || k < std::abs(la - lb)) return DFTA_OK;       // parity, triangle
    // (J-2la)! (J-2k)! (J-2lb)! / (J+1)!  x  (g! / ((g-la)! (g-k)! (g-lb)!))^2,  g = J / 2
    const int g = J / 2;
    int e[kNumPrimes] = {0};
    add_factorial(J - 2 * la, 1, e); add_factorial(J - 2 * k, 1, e); add_factorial(J - 2 * lb, 1, e);
    add_factorial(J + 1, -1, e);
    add_factorial(g, 2, e);
    add_factorial(g - la, -2, e); add_factorial(g - k, -2, e); add_factorial(g - lb, -2, e);
    unsigned long long num = 1, den = 1;                                      // the reduced fraction: both far below 2^53
    for (int q = 0; q < kNumPrimes; ++q) {
        for (int m = 0; m < e[q]; ++m) num *= kPrimes[q];
        for (int m = 0; m < -e[q]; ++m) den *= kPrimes[q];
    }
    *out = (double)num / (double)den;
    return DFTA_OK;
}

int fg_jobs(int norb, const int* l, int* jobs, int* kinds)
{
    if (norb < 0 || (norb > 0 && !l)) return -1;
    for (int a = 0; a < norb; ++a)
        if (l[a] < 0 || l[a] > kLmax) return -1;
    int n = 0;
    auto put = [&](int a, int b, int c, int d, int k, int kind) {
        if (jobs) { int* row = jobs + (size_t)kJobInts * n; row[0] = a; row[1] = b; row[2] = c; row[3] = d; row[4] = k; }
        if (kinds) kinds[n] = kind;
        ++n;
    };
    for (int a = 0; a < norb; ++a)
        for (int b = a; b < norb; ++b)
            for (int k = 0; k <= 2 * std::min(l[a], l[b]); k += 2) put(a, b, a, b, k, kKindF);
    for (int a = 0; a < norb; ++a)
        for (int b = a + 1; b < norb; ++b)
            for (int k = std::abs(l[a] - l[b]); k <= l[a] + l[b]; k += 2) put(a, b, b, a, k, kKindG);
    return n;
}

const char* check_jobs(int norb, int njobs, const int* jobs)
{
    for (int j = 0; j < njobs; ++j) {
        const int* row = jobs + (size_t)kJobInts * j;
        for (int m = 0; m < 4; ++m)
            if (row[m] < 0 || row[m] >= norb) return "Slater job: orbital index out of range";
        if (row[4] < 0 || row[4] > kKmax) return "Slater job: k outside 0 .. DFTA_SLATER_KMAX";
    }
    return nullptr;
}

int plan_energy(int nA, int nB, const int* l, EnergyPlan* plan)
{
    const int norb = nA + nB;
    for (int a = 0; a < norb; ++a)
        if (l[a] < 0 || l[a] > kLmax) return -1;
    plan->norb = norb; plan->nA = nA;
    plan->l.assign(l, l + norb);
    plan->jobs.clear();
    plan->f0.assign((size_t)norb * norb, -1);
    plan->gk.assign((size_t)(kKmax + 1) * norb * norb, -1);
    auto put = [&](int a, int b, int c, int d, int k) {
        const int row[kJobInts] = {a, b, c, d, k};
        plan->jobs.insert(plan->jobs.end(), row, row + kJobInts);
        return plan->njobs() - 1;
    };
    for (int i = 0; i < norb; ++i)
        for (int j = i; j < norb; ++j) plan->f0[(size_t)i * norb + j] = plan->f0[(size_t)j * norb + i] = put(i, j, i, j, 0);
    for (int ch = 0; ch < 2; ++ch) {
        const int c0 = ch ? nA : 0, c1 = ch ? norb : nA;
        for (int a = c0; a < c1; ++a)
            for (int b = a; b < c1; ++b)
                for (int k = std::abs(l[a] - l[b]); k <= l[a] + l[b]; k += 2) {
                    const int job = a != b ? put(a, b, b, a, k) : (k == 0 ? plan->f0[(size_t)a * norb + a] : put(a, a, a, a, k));
                    plan->gk[((size_t)k * norb + a) * norb + b] = plan->gk[((size_t)k * norb + b) * norb + a] = job;
                }
    }
    return 0;
}

void energy_sums(const EnergyPlan& plan, const double* occ, int lsda, const double* R, double* EH, double* EXX)
{
    const int norb = plan.norb;
    double eh = 0.;
    for (int i = 0; i < norb; ++i)
        for (int j = 0; j < norb; ++j) eh += (occ[i] * occ[j]) * R[plan.f0[(size_t)i * norb + j]];
    *EH = 0.5 * eh;
    double S = 0.;
    for (int ch = 0; ch < 2; ++ch) {
        const int c0 = ch ? plan.nA : 0, c1 = ch ? norb : plan.nA;
        for (int a = c0; a < c1; ++a)
            for (int b = c0; b < c1; ++b) {
                double T = 0.;
                for (int k = std::abs(plan.l[a] - plan.l[b]); k <= plan.l[a] + plan.l[b]; k += 2) {
                    double c3j = 0.;
                    (void)gaunt_3j2(plan.l[a], k, plan.l[b], &c3j);
                    T += c3j * R[plan.gk[((size_t)k * norb + a) * norb + b]];
                }
                const double na = lsda ? occ[a] : 0.5 * occ[a], nb = lsda ? occ[b] : 0.5 * occ[b];
                S += (na * nb) * T;
            }
    }
    *EXX = lsda ? -0.5 * S : -S;
}

}  // namespace dfta_slater

extern "C" {

int dfta_gaunt_3j2(int la, int k, int lb, double* out) { return dfta_slater::gaunt_3j2(la, k, lb, out); }

int dfta_slater_fg_jobs(int norb, const int* l, int* jobs, int* kinds) { return dfta_slater::fg_jobs(norb, l, jobs, kinds); }

}  // extern "C"
