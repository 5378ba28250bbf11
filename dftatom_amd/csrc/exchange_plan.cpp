// exchange_plan.cpp -- see exchange_plan.h.  Pure host code (no HIP include): the host-only entry of the C ABI lives here too.
#include "exchange_plan.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>

#include "../../include/dftatom_hip.h"
#include "slater_plan.h"

namespace dfta_exchange {

static_assert(kKmax == DFTA_SLATER_KMAX && kKmax == dfta_slater::kKmax && kLmax == dfta_slater::kLmax, "exchange_plan.h, slater_plan.h and the header disagree");
static_assert(kRedHF == DFTA_XP_HF && kRedS == DFTA_XP_S && kRedKLI == DFTA_XP_KLI, "the columns of vbar");

int y_jobs(int norb, const int* l, int* jobs)
{
    if (norb < 0 || (norb > 0 && !l)) return -1;
    for (int a = 0; a < norb; ++a)
        if (l[a] < 0 || l[a] > kLmax) return -1;
    int n = 0;
    for (int a = 0; a < norb; ++a)
        for (int b = a; b < norb; ++b)
            for (int k = std::abs(l[a] - l[b]); k <= l[a] + l[b]; k += 2) {
                if (jobs) { int* row = jobs + (size_t)kJobInts * n; row[0] = a; row[1] = b; row[2] = k; }
                ++n;
            }
    return n;
}

const char* check_jobs(int norb, int njobs, const int* jobs)
{
    for (int j = 0; j < njobs; ++j) {
        const int* row = jobs + (size_t)kJobInts * j;
        if (row[0] < 0 || row[0] >= norb || row[1] < 0 || row[1] >= norb) return "screening job: orbital index out of range";
        if (row[2] < 0 || row[2] > kKmax) return "screening job: k outside 0 .. DFTA_SLATER_KMAX";
    }
    return nullptr;
}

const char* check_channel(int norb, const int* l, const double* occ, int homo)
{
    if (norb < 1 || norb > kShellsMax) return "exchange potentials: norb outside 1 .. 32";
    for (int a = 0; a < norb; ++a) {
        if (l[a] < 0 || l[a] > kLmax) return "exchange potentials: an l outside 0 .. 4";
        if (!(occ[a] >= 0.) || !std::isfinite(occ[a])) return "exchange potentials: an occupation that is negative or not finite";
    }
    if (homo < 0 || homo >= norb) return "exchange potentials: homo out of range";
    return nullptr;
}

int pick_homo(int norb, const double* E, const double* occ)
{
    int h = -1;
    for (int a = 0; a < norb; ++a)
        if (occ[a] > 0. && (h < 0 || E[a] >= E[h])) h = a;
    return h;
}

int plan_channel(int norb, const int* l, const double* occ, ChannelPlan* plan)
{
    if (check_channel(norb, l, occ, 0)) return -1;
    plan->norb = norb;
    plan->jobs.assign((size_t)kJobInts * y_jobs(norb, l, nullptr), 0);
    y_jobs(norb, l, plan->jobs.data());
    std::vector<int> row((size_t)(kKmax + 1) * norb * norb, -1);      // the y job of (k, a, b), mirrored
    for (int j = 0; j < plan->njobs(); ++j) {
        const int a = plan->jobs[(size_t)kJobInts * j], b = plan->jobs[(size_t)kJobInts * j + 1], k = plan->jobs[(size_t)kJobInts * j + 2];
        row[((size_t)k * norb + a) * norb + b] = row[((size_t)k * norb + b) * norb + a] = j;
    }
    plan->first.assign(1, 0);
    plan->tab.clear(); plan->coef.clear();
    for (int a = 0; a < norb; ++a) {
        for (int b = 0; b < norb; ++b)
            for (int k = std::abs(l[a] - l[b]); k <= l[a] + l[b]; k += 2) {
                double c3j = 0.;
                (void)dfta_slater::gaunt_3j2(l[a], k, l[b], &c3j);
                const int e[kTabInts] = {a, b, k, row[((size_t)k * norb + a) * norb + b]};
                plan->tab.insert(plan->tab.end(), e, e + kTabInts);
                plan->coef.push_back(occ[b] * c3j);
            }
        plan->first.push_back((int)plan->coef.size());
    }
    plan->red1.clear(); plan->red2.clear();
    auto put = [](std::vector<int>& t, int kind, int a, int b) { const int e[kRedInts] = {kind, a, b}; t.insert(t.end(), e, e + kRedInts); };
    for (int a = 0; a < norb; ++a) put(plan->red1, kRedHF, a, a);
    for (int a = 0; a < norb; ++a) put(plan->red1, kRedS, a, a);
    for (int a = 0; a < norb; ++a)
        for (int b = a; b < norb; ++b) put(plan->red1, kRedPair, a, b);
    for (int a = 0; a < norb; ++a) put(plan->red2, kRedKLI, a, a);
    return 0;
}

int solve_kli(int norb, int homo, const double* M, const double* vbarS, const double* vbarHF, double* c)
{
    for (int a = 0; a < norb; ++a) c[a] = 0.;
    const int H = norb - 1;
    if (H <= 0) return 0;
    std::vector<int> idx;
    for (int a = 0; a < norb; ++a)
        if (a != homo) idx.push_back(a);
    std::vector<double> A((size_t)H * H), b(H), x(H);
    for (int i = 0; i < H; ++i) {
        for (int j = 0; j < H; ++j) A[(size_t)i * H + j] = (i == j ? 1. : 0.) - M[(size_t)idx[i] * norb + idx[j]];
        b[i] = vbarS[idx[i]] - vbarHF[idx[i]];
    }
    for (int j = 0; j < H; ++j) {
        int p = j;
        for (int i = j + 1; i < H; ++i)
            if (std::fabs(A[(size_t)i * H + j]) > std::fabs(A[(size_t)p * H + j])) p = i;
        if (p != j) {
            for (int m = 0; m < H; ++m) std::swap(A[(size_t)j * H + m], A[(size_t)p * H + m]);
            std::swap(b[j], b[p]);
        }
        const double piv = A[(size_t)j * H + j];
        if (piv == 0. || !std::isfinite(piv)) return -1;
        for (int i = j + 1; i < H; ++i) {
            const double f = A[(size_t)i * H + j] / piv;
            for (int m = j + 1; m < H; ++m) A[(size_t)i * H + m] = A[(size_t)i * H + m] - f * A[(size_t)j * H + m];
            b[i] = b[i] - f * b[j];
        }
    }
    for (int i = H - 1; i >= 0; --i) {
        double t = b[i];
        for (int m = i + 1; m < H; ++m) t = t - A[(size_t)i * H + m] * x[m];
        x[i] = t / A[(size_t)i * H + i];
    }
    for (int i = 0; i < H; ++i) c[idx[i]] = x[i];
    return 0;
}

}  // namespace dfta_exchange

extern "C" {

int dfta_exchange_jobs(int norb, const int* l, int* jobs) { return dfta_exchange::y_jobs(norb, l, jobs); }

}  // extern "C"
