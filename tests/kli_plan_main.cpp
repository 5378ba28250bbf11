// kli_plan_main.cpp -- stand-alone driver of dftatom_amd/csrc/kli_plan.cpp (pure host code) for tests/test_kli_scf_ref.py, which builds
// it with -fsanitize=address,undefined: the tables of a batch of four channels (one without shells), the refusals, the chunks under
// several budgets and with a channel that is not live, and the buffer sizes.  Prints what the test compares with its Python statement;
// exit status 0 when every check holds.
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
    bad += plan_channels(4, norb, l, occ, atom, &p) != 0;
    bad += p.nch() != 4 || p.norb_total != 9;
    std::printf("channels");
    for (const Channel& c : p.ch)
        std::printf(" %d:%d:%d:%d:%d:%d:%d:%d:%d:%d", c.u0, c.norb, c.job0, c.njobs, c.first0, c.tab0, c.ntab, c.red0, c.nred, c.atom);
    std::printf("\njobs");
    for (int j = 0; j < p.njobs(); ++j) std::printf(" %d:%d:%d", p.jobs[kJobInts * j], p.jobs[kJobInts * j + 1], p.jobs[kJobInts * j + 2]);
    std::printf("\n");
    // every channel's part equals exchange_plan's own plan of that channel
    for (int c = 0, u0 = 0; c < 4; u0 += norb[c], ++c) {
        if (!norb[c]) { bad += p.ch[c].njobs != 0 || p.ch[c].nred != 0 || p.ch[c].ntab != 0; continue; }
        dfta_exchange::ChannelPlan one;
        bad += dfta_exchange::plan_channel(norb[c], l + u0, occ + u0, &one) != 0;
        const Channel& ch = p.ch[c];
        bad += ch.njobs != one.njobs() || ch.ntab != (int)one.coef.size() || ch.nred != one.nred1();
        for (int a = 0; a <= norb[c]; ++a) bad += p.first[ch.first0 + a] != one.first[a];
        for (int e = 0; e < ch.ntab; ++e) {
            bad += p.coef[ch.tab0 + e] != one.coef[e];
            for (int m = 0; m < kTabInts; ++m) bad += p.tab[(size_t)kTabInts * (ch.tab0 + e) + m] != one.tab[(size_t)kTabInts * e + m];
            const int row = p.tab[(size_t)kTabInts * (ch.tab0 + e) + 3];
            bad += row < 0 || row >= ch.njobs;
        }
        for (int q = 0; q < ch.nred; ++q) {
            const int* r = p.red.data() + (size_t)kRedInts * (ch.red0 + q);
            bad += r[3] != c || r[1] < 0 || r[1] >= norb[c] || r[2] < 0 || r[2] >= norb[c];
            for (int m = 0; m < 3; ++m) bad += r[m] != one.red1[(size_t)dfta_exchange::kRedInts * q + m];
        }
        for (int j = 0; j < ch.njobs; ++j) {
            const int* r = p.jobs.data() + (size_t)kJobInts * (ch.job0 + j);
            bad += r[0] < u0 || r[0] >= u0 + norb[c] || r[1] < r[0] || r[1] >= u0 + norb[c];
        }
    }
    // refusals
    const int n33[1] = {33}, nneg[1] = {-1};
    std::vector<int> l33(33, 0);
    std::vector<double> o33(33, 1.);
    bad += check_channels(1, n33, l33.data(), o33.data()) == nullptr || check_channels(1, nneg, l, occ) == nullptr;
    bad += check_channels(-1, norb, l, occ) == nullptr || check_channels(1, nullptr, l, occ) == nullptr;
    const int l5[9] = {0, 0, 5, 0, 0, 1, 0, 1, 0};
    bad += check_channels(4, norb, l5, occ) == nullptr;
    std::vector<double> o(occ, occ + 9);
    o[4] = -1.;
    bad += check_channels(4, norb, l, o.data()) == nullptr;
    o[4] = std::nan("");
    bad += check_channels(4, norb, l, o.data()) == nullptr;
    o[4] = 1.; o[8] = 0.;                           // the one-shell channel has no occupied shell
    bad += check_channels(4, norb, l, o.data()) == nullptr;
    bad += plan_channels(4, norb, l, o.data(), nullptr, &p) != -1;
    bad += check_channels(0, nullptr, nullptr, nullptr) != nullptr;
    bad += plan_channels(4, norb, l, occ, nullptr, &p) != 0 || p.ch[2].atom != -1;
    // budgets and chunks
    std::printf("rows %ld %ld %ld %ld\n", budget_rows(1., 4097), budget_rows(0., 4097), budget_rows(-3., 4097), budget_rows(185., 131073));
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
