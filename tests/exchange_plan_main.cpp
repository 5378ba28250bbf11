// exchange_plan_main.cpp -- stand-alone driver of dftatom_amd/csrc/exchange_plan.cpp (pure host code) for tests/test_exchange_ref.py,
// which builds it with -fsanitize=address,undefined: the y-job table and the channel plan of 19 levels, the validation of tables and
// channels, the HOMO rule and the reduced solve.  Prints what the test compares with its Python statement; exit status 0 when every
// table validates.
#include <cmath>
#include <cstdio>
#include <vector>

#include "exchange_plan.h"

using namespace dfta_exchange;

int main()
{
    int bad = 0;
    const int l[19] = {0, 0, 1, 0, 1, 2, 0, 1, 2, 3, 0, 1, 2, 3, 0, 1, 2, 0, 1};      // Z = 118
    std::vector<double> occ(19);
    for (int a = 0; a < 19; ++a) occ[a] = 0.5 + 0.25 * a;
    const int n = y_jobs(19, l, nullptr);
    std::vector<int> jobs((size_t)kJobInts * n);
    bad += y_jobs(19, l, jobs.data()) != n;
    bad += check_jobs(19, n, jobs.data()) != nullptr;
    bad += check_jobs(18, n, jobs.data()) == nullptr;
    const int badk[3] = {0, 0, 9}, negk[3] = {0, 0, -1};
    bad += check_jobs(19, 1, badk) == nullptr;
    bad += check_jobs(19, 1, negk) == nullptr;
    bad += y_jobs(-1, l, nullptr) != -1;
    bad += y_jobs(2, nullptr, nullptr) != -1;
    const int l5[2] = {0, 5};
    bad += y_jobs(2, l5, nullptr) != -1;
    bad += y_jobs(0, nullptr, nullptr) != 0;
    ChannelPlan p;
    bad += plan_channel(19, l, occ.data(), &p) != 0;
    bad += p.njobs() != n || (int)p.first.size() != 20 || p.first[19] != (int)p.coef.size() || p.tab.size() != kTabInts * p.coef.size();
    bad += p.nred1() != 2 * 19 + 19 * 20 / 2 || p.nred2() != 19;
    std::printf("jobs %d entries %d\n", n, (int)p.coef.size());
    for (size_t e = 0; e < p.coef.size(); ++e) {     // every entry points at the y job of its pair
        const int a = p.tab[kTabInts * e], b = p.tab[kTabInts * e + 1], k = p.tab[kTabInts * e + 2], row = p.tab[kTabInts * e + 3];
        bad += row < 0 || row >= n;
        if (row < 0 || row >= n) continue;
        bad += jobs[kJobInts * row] != (a < b ? a : b) || jobs[kJobInts * row + 1] != (a < b ? b : a) || jobs[kJobInts * row + 2] != k;
    }
    std::printf("tab");
    for (int a = 0; a < 3; ++a)
        for (int e = p.first[a]; e < p.first[a + 1]; ++e) std::printf(" %d:%d:%d:%d:%.17g", p.tab[kTabInts * e], p.tab[kTabInts * e + 1], p.tab[kTabInts * e + 2], p.tab[kTabInts * e + 3], p.coef[e]);
    std::printf("\n");
    // channels that must be refused
    std::vector<double> neg(occ);
    neg[3] = -1.;
    bad += check_channel(19, l, neg.data(), 0) == nullptr;
    neg[3] = std::nan("");
    bad += check_channel(19, l, neg.data(), 0) == nullptr;
    bad += check_channel(19, l, occ.data(), 19) == nullptr || check_channel(19, l, occ.data(), -1) == nullptr;
    bad += check_channel(0, l, occ.data(), 0) == nullptr || check_channel(33, l, occ.data(), 0) == nullptr;
    bad += check_channel(2, l5, occ.data(), 0) == nullptr;
    bad += check_channel(19, l, occ.data(), 18) != nullptr;
    bad += plan_channel(2, l5, occ.data(), &p) != -1;
    // the HOMO rule
    const double E[5] = {-3., -1., -1., -0.5, -2.};
    const double o1[5] = {1., 1., 1., 0., 1.}, o0[5] = {0., 0., 0., 0., 0.}, o2[5] = {1., 1., 1., 1., 1.};
    std::printf("homo %d %d %d %d\n", pick_homo(5, E, o1), pick_homo(5, E, o0), pick_homo(5, E, o2), pick_homo(0, E, o2));
    // the reduced solve: a 4 x 4 matrix, homo 1 removed; then the one-shell channel and a singular system
    const double M[16] = {0.5, 0.1, 0.2, 0.2, 0.1, 0.4, 0.3, 0.2, 0.9, 0.0, 0.05, 0.05, 0.2, 0.3, 0.1, 0.4};
    const double vS[4] = {-1.0, -0.7, -0.4, -0.2}, vHF[4] = {-1.1, -0.65, -0.5, -0.1};
    double c[4] = {7., 7., 7., 7.};
    bad += solve_kli(4, 1, M, vS, vHF, c) != 0;
    std::printf("solve %.17g %.17g %.17g %.17g\n", c[0], c[1], c[2], c[3]);
    double c1[1] = {7.};
    bad += solve_kli(1, 0, M, vS, vHF, c1) != 0 || c1[0] != 0.;
    const double I2[4] = {1., 0., 0., 1.};
    double c2[2] = {7., 7.};
    bad += solve_kli(2, 0, I2, vS, vHF, c2) != -1 || c2[0] != 0. || c2[1] != 0.;
    return bad;
}
