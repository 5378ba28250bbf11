// slater_plan_main.cpp -- stand-alone driver of dftatom_amd/csrc/slater_plan.cpp (pure host code) for tests/test_slater_ref.py, which
// builds it with -fsanitize=address,undefined: every argument range of the angular factor, the job tables of 19 levels, the energy plan
// and its sums for an LSDA and an LDA atom.  Prints the counts and sums; exit status 0 when every table validates.
#include <cstdio>
#include <vector>

#include "slater_plan.h"

using namespace dfta_slater;

int main()
{
    double v = 0;
    int bad = 0;
    for (int a = -1; a <= 5; ++a)
        for (int k = -1; k <= 12; ++k)
            for (int b = -1; b <= 5; ++b) gaunt_3j2(a, k, b, &v);
    const int l[19] = {0, 0, 1, 0, 1, 2, 0, 1, 2, 3, 0, 1, 2, 3, 0, 1, 2, 0, 1};      // Z = 118
    const int n = fg_jobs(19, l, nullptr, nullptr);
    std::vector<int> jobs(5 * (size_t)n), kinds(n);
    bad += fg_jobs(19, l, jobs.data(), kinds.data()) != n;
    bad += check_jobs(19, n, jobs.data()) != nullptr;
    bad += check_jobs(18, n, jobs.data()) == nullptr;
    EnergyPlan p;
    bad += plan_energy(12, 7, l, &p) != 0;
    bad += check_jobs(19, p.njobs(), p.jobs.data()) != nullptr;
    std::vector<double> R(p.njobs(), 1.0), occ(19, 1.5);
    double eh = 0, ex = 0;
    energy_sums(p, occ.data(), 1, R.data(), &eh, &ex);
    std::printf("fg %d lsda %d %.17g %.17g\n", n, p.njobs(), eh, ex);
    bad += plan_energy(19, 0, l, &p) != 0;
    R.assign(p.njobs(), 1.0);
    energy_sums(p, occ.data(), 0, R.data(), &eh, &ex);
    std::printf("lda %d %.17g %.17g\n", p.njobs(), eh, ex);
    return bad;
}
