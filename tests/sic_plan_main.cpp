// sic_plan_main.cpp -- stand-alone driver of plan_channels_sic (dftatom_amd/csrc/kli_plan.cpp, pure host code) for tests/test_sic_ref.py,
// which builds it with -fsanitize=address,undefined: the tables of a batch of four channels (one without shells), the refusals, the
// chunks under several budgets and with a channel that is not live, and the buffer sizes.  Prints what the test compares with its Python
// statement; exit status 0 when every check holds.
#include <cmath>
#include <cstdio>
#include <vector>

#include "kli_plan.h"

using namespace dfta_kli;

static void print_chunks(const char* name, const std::vector<int>& b)
{
    std::printf("%s", name);
    for (size_t k = 0; k + 1 < b.size(); k += 2) std::printf(" %d:%d", b[k], b[k + 1]);
    std::printf("\n");
}

int main()
{
    int bad = 0;
    // channels: Ne-like (1s 2s 2p), none, Ar-like (1s 2s 2p 3s 3p), one shell
    const int norb[4] = {3, 0, 5, 1};
    const int l[9] = {0, 0, 1, 0, 0, 1, 0, 1, 0};
    const double occ[9] = {1., 1., 3., 1., 1., 3., 1., 3., 0.5};
    const int atom[4] = {0, 0, 1, 2};
    Plan p;
    bad += plan_channels_sic(4, norb, l, occ, atom, &p) != 0;
    bad += p.nch() != 4 || p.norb_total != 9 || p.njobs() != 9;
    bad += !p.first.empty() || !p.tab.empty() || !p.coef.empty();
    std::printf("channels");
    for (const Channel& c : p.ch)
        std::printf(" %d:%d:%d:%d:%d:%d:%d:%d:%d:%d", c.u0, c.norb, c.job0, c.njobs, c.first0, c.tab0, c.ntab, c.red0, c.nred, c.atom);
    std::printf("\njobs");
    for (int j = 0; j < p.njobs(); ++j) std::printf(" %d:%d:%d", p.jobs[kJobInts * j], p.jobs[kJobInts * j + 1], p.jobs[kJobInts * j + 2]);
    std::printf("\nred");
    for (int q = 0; q < p.nred(); ++q)
        std::printf(" %d:%d:%d:%d", p.red[kRedInts * q], p.red[kRedInts * q + 1], p.red[kRedInts * q + 2], p.red[kRedInts * q + 3]);
    std::printf("\n");
    // the part of a channel's reductions that the solve reads is the exchange stage's own, entry for entry
    Plan kli;
    bad += plan_channels(4, norb, l, occ, atom, &kli) != 0;
    for (int c = 0; c < 4; ++c) {
        const Channel& a = p.ch[c];
        const Channel& b = kli.ch[c];
        bad += a.u0 != b.u0 || a.norb != b.norb || a.atom != b.atom || a.nred != b.nred + 2 * a.norb || a.njobs != a.norb;
        for (int q = 0; q < b.nred; ++q)
            for (int m = 0; m < kRedInts; ++m) bad += p.red[(size_t)kRedInts * (a.red0 + q) + m] != kli.red[(size_t)kRedInts * (b.red0 + q) + m];
        for (int q = b.nred; q < a.nred; ++q) {
            const int* r = p.red.data() + (size_t)kRedInts * (a.red0 + q);
            const int want = q < b.nred + a.norb ? kRedSicH : kRedSicXC;
            bad += r[0] != want || r[1] != (q - b.nred) % a.norb || r[2] != r[1] || r[3] != c;
        }
    }
    // refusals: those of plan_channels
    const int n33[1] = {33};
    std::vector<int> l33(33, 0);
    std::vector<double> o33(33, 1.);
    bad += plan_channels_sic(1, n33, l33.data(), o33.data(), nullptr, &p) != -1;
    const int l5[9] = {0, 0, 5, 0, 0, 1, 0, 1, 0};
    bad += plan_channels_sic(4, norb, l5, occ, nullptr, &p) != -1;
    std::vector<double> o(occ, occ + 9);
    o[4] = std::nan("");
    bad += plan_channels_sic(4, norb, l, o.data(), nullptr, &p) != -1;
    o[4] = 1.; o[8] = 0.;                           // the one-shell channel has no occupied shell
    bad += plan_channels_sic(4, norb, l, o.data(), nullptr, &p) != -1;
    bad += plan_channels_sic(0, nullptr, nullptr, nullptr, nullptr, &p) != 0 || p.nch() != 0;
    bad += plan_channels_sic(4, norb, l, occ, nullptr, &p) != 0 || p.ch[2].atom != -1;
    // budgets and chunks: a channel costs one y row per shell
    std::vector<int> b;
    plan_chunks(p, nullptr, 1000, &b); print_chunks("all", b);
    plan_chunks(p, nullptr, 0, &b); print_chunks("each", b);
    plan_chunks(p, nullptr, p.ch[0].njobs + p.ch[2].njobs, &b); print_chunks("two", b);
    const unsigned char live[4] = {1, 1, 0, 1};
    plan_chunks(p, live, 1000, &b); print_chunks("frozen", b);
    const unsigned char none[4] = {0, 0, 0, 0};
    plan_chunks(p, none, 1000, &b); print_chunks("none", b);
    const Caps c0 = capacities(p, 0), c1 = capacities(p, 1000);
    std::printf("caps %ld:%ld:%ld %ld:%ld:%ld\n", c0.yrows, c0.xrows, c0.chans, c1.yrows, c1.xrows, c1.chans);
    return bad;
}
