// Stand-alone check of dftatom_amd/csrc/pseudo_plan.cpp (pure host code), built with ASan + UBSan by tests/test_pseudo_ref.py.
// Prints one line per case; the test reads them.
#include <cmath>
#include <cstdio>
#include <vector>

#include "pseudo_plan.h"

namespace pp = dfta_pseudo_plan;

static int fails = 0;
static void expect(bool ok, const char* what)
{
    if (!ok) { std::printf("FAIL %s\n", what); ++fails; }
}

int main()
{
    // validation
    {
        const int N = 1025;
        std::vector<int> l = {0, 1, 2, 3, 4}, ic = {3, 255, 256, 257, N - 4};
        pp::Call c{N, 5, l.data(), ic.data()};
        expect(pp::check(c) == nullptr, "valid call");
        c.nch = 0; c.l = nullptr; c.ic = nullptr;
        expect(pp::check(c) == nullptr, "no channels");
        c.nch = 5; c.l = l.data();
        expect(pp::check(c) != nullptr, "null ic");
        c.ic = ic.data();
        for (int bad : {2, N - 3, -1, N}) {
            ic[2] = bad;
            expect(pp::check(c) != nullptr, "core node near an end");
        }
        ic[2] = 256;
        l[4] = 5;
        expect(pp::check(c) != nullptr, "l = 5");
        l[4] = -1;
        expect(pp::check(c) != nullptr, "l = -1");
        l[4] = 4;
        c.N = 7;
        expect(pp::check(c) != nullptr, "N = 7");
        c.N = N; c.nch = -1;
        expect(pp::check(c) != nullptr, "nch = -1");
    }
    // the default valence: Fe 1s2 2s2 2p6 3s2 3p6 3d6 4s2 (n as the library counts: principal - 1), Ar, H, and an empty 4s
    {
        const int n[] = {0, 1, 1, 2, 2, 2, 3}, l[] = {0, 0, 1, 0, 1, 2, 0}, occ[] = {2, 2, 6, 2, 6, 6, 2};
        int pick[8];
        int cnt = pp::default_valence(7, n, l, occ, pick, 8);
        std::printf("valence Fe %d %d %d\n", cnt, cnt > 0 ? pick[0] : -1, cnt > 1 ? pick[1] : -1);
        cnt = pp::default_valence(5, n, l, occ, pick, 8);
        std::printf("valence Ar %d %d %d\n", cnt, cnt > 0 ? pick[0] : -1, cnt > 1 ? pick[1] : -1);
        cnt = pp::default_valence(1, n, l, occ, pick, 8);
        std::printf("valence H %d %d %d\n", cnt, cnt > 0 ? pick[0] : -1, -1);
        const int occ0[] = {2, 2, 6, 2, 6, 6, 0};
        cnt = pp::default_valence(7, n, l, occ0, pick, 8);
        std::printf("valence Fe2+ %d %d %d %d\n", cnt, pick[0], pick[1], cnt > 2 ? pick[2] : -1);
        expect(pp::default_valence(7, n, l, occ, pick, 1) == -1, "cap too small");
        expect(pp::default_valence(7, n, l, occ, nullptr, 8) == -1, "null pick");
        expect(pp::default_valence(0, nullptr, nullptr, nullptr, pick, 8) == 0, "no levels");
        const int lneg[] = {0, -1};
        expect(pp::default_valence(2, n, lneg, occ, pick, 8) == -1, "negative l");
    }
    // the default core node: u = r (2 - r) exp(-r) on a uniform grid of 65 nodes to r = 16: peak at r = 2 - sqrt(2), sign change at r = 2
    {
        const int N = 65;
        std::vector<double> r(N), u(N);
        for (int i = 0; i < N; ++i) { r[i] = 0.25 * i; u[i] = r[i] * (2. - r[i]) * std::exp(-r[i]); }
        std::printf("ic %d %d %d %d\n", pp::default_ic(N, r.data(), u.data(), 1.5), pp::default_ic(N, r.data(), u.data(), 6.),
                    pp::default_ic(N, r.data(), u.data(), 1e3), pp::default_ic(N, r.data(), u.data(), 1e-3));
        for (int i = 10; i < N; ++i) u[i] = 0.;      // a cut-off orbital: the node moves past the zeros, and stops at N - 4
        std::printf("ic0 %d\n", pp::default_ic(N, r.data(), u.data(), 1.5));
        expect(pp::default_ic(N, r.data(), u.data(), 0.) == -1, "factor 0");
        expect(pp::default_ic(N, r.data(), u.data(), NAN) == -1, "factor NaN");
        expect(pp::default_ic(N, r.data(), u.data(), INFINITY) == -1, "factor inf");
        expect(pp::default_ic(N, nullptr, u.data(), 1.5) == -1, "null r");
        expect(pp::default_ic(7, r.data(), u.data(), 1.5) == -1, "N = 7");
    }
    return fails != 0;
}
