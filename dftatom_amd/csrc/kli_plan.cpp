// kli_plan.cpp -- see kli_plan.h.  Pure host code (no HIP include).
#include "kli_plan.h"

#include <algorithm>
#include <cmath>

namespace dfta_kli {

const char* check_channels(int nch, const int* norb, const int* l, const double* occ)
{
    if (nch < 0 || (nch > 0 && !norb)) return "KLI channels: nch / norb";
    int off = 0;
    for (int c = 0; c < nch; ++c) {
        const int n = norb[c];
        if (n < 0 || n > dfta_exchange::kShellsMax) return "KLI channels: a channel's norb outside 0 .. 32";
        if (n == 0) continue;
        if (!l || !occ) return "KLI channels: l / occ";
        bool occupied = false;
        for (int a = 0; a < n; ++a) {
            if (l[off + a] < 0 || l[off + a] > dfta_exchange::kLmax) return "KLI channels: an l outside 0 .. 4";
            if (!(occ[off + a] >= 0.) || !std::isfinite(occ[off + a])) return "KLI channels: an occupation that is negative or not finite";
            occupied = occupied || occ[off + a] > 0.;
        }
        if (!occupied) return "KLI channels: a channel without an occupied shell has no HOMO";
        off += n;
    }
    return nullptr;
}

int plan_channels(int nch, const int* norb, const int* l, const double* occ, const int* atom, Plan* plan)
{
    if (check_channels(nch, norb, l, occ)) return -1;
    *plan = Plan();
    int u0 = 0;
    for (int c = 0; c < nch; ++c) {
        Channel ch = {};
        ch.u0 = u0; ch.norb = norb[c];
        ch.job0 = plan->njobs(); ch.first0 = (int)plan->first.size(); ch.tab0 = (int)plan->coef.size(); ch.red0 = plan->nred();
        ch.atom = atom ? atom[c] : -1;
        if (ch.norb > 0) {
            dfta_exchange::ChannelPlan one;
            if (dfta_exchange::plan_channel(ch.norb, l + u0, occ + u0, &one)) return -1;
            for (int j = 0; j < one.njobs(); ++j) {        // the batch's orbital rows
                plan->jobs.push_back(u0 + one.jobs[(size_t)kJobInts * j]);
                plan->jobs.push_back(u0 + one.jobs[(size_t)kJobInts * j + 1]);
                plan->jobs.push_back(one.jobs[(size_t)kJobInts * j + 2]);
            }
            plan->first.insert(plan->first.end(), one.first.begin(), one.first.end());
            plan->tab.insert(plan->tab.end(), one.tab.begin(), one.tab.end());
            plan->coef.insert(plan->coef.end(), one.coef.begin(), one.coef.end());
            for (int q = 0; q < one.nred1(); ++q) {
                const int* row = one.red1.data() + (size_t)dfta_exchange::kRedInts * q;
                const int e[kRedInts] = {row[0], row[1], row[2], c};
                plan->red.insert(plan->red.end(), e, e + kRedInts);
            }
            ch.njobs = one.njobs(); ch.ntab = (int)one.coef.size(); ch.nred = one.nred1();
        }
        plan->ch.push_back(ch);
        u0 += ch.norb;
    }
    plan->norb_total = u0;
    return 0;
}

int plan_channels_sic(int nch, const int* norb, const int* l, const double* occ, const int* atom, Plan* plan)
{
    if (check_channels(nch, norb, l, occ)) return -1;
    *plan = Plan();
    int u0 = 0;
    auto put = [&](int kind, int a, int b, int c) {
        const int e[kRedInts] = {kind, a, b, c};
        plan->red.insert(plan->red.end(), e, e + kRedInts);
    };
    for (int c = 0; c < nch; ++c) {
        Channel ch = {};
        const int n = norb[c];
        ch.u0 = u0; ch.norb = n;
        ch.job0 = plan->njobs(); ch.red0 = plan->nred();
        ch.atom = atom ? atom[c] : -1;
        for (int a = 0; a < n; ++a) {
            const int e[kJobInts] = {u0 + a, u0 + a, 0};
            plan->jobs.insert(plan->jobs.end(), e, e + kJobInts);
        }
        for (int a = 0; a < n; ++a) put(dfta_exchange::kRedHF, a, a, c);
        for (int a = 0; a < n; ++a) put(dfta_exchange::kRedS, a, a, c);
        for (int a = 0; a < n; ++a)
            for (int b = a; b < n; ++b) put(dfta_exchange::kRedPair, a, b, c);
        for (int a = 0; a < n; ++a) put(kRedSicH, a, a, c);
        for (int a = 0; a < n; ++a) put(kRedSicXC, a, a, c);
        ch.njobs = n; ch.nred = plan->nred() - ch.red0;
        plan->ch.push_back(ch);
        u0 += n;
    }
    plan->norb_total = u0;
    return 0;
}

long budget_rows(double mb, int N)
{
    if (!(mb > 0.) || N <= 0) return 0;
    const double rows = std::floor(mb * 1048576. / (8. * N));
    return rows > 2e9 ? 2000000000L : (long)rows;
}

void plan_chunks(const Plan& plan, const unsigned char* live, long max_rows, std::vector<int>* bounds)
{
    bounds->clear();
    int c0 = -1;
    long rows = 0;
    auto close = [&](int c1) {
        if (c0 >= 0 && rows > 0) { bounds->push_back(c0); bounds->push_back(c1); }
        c0 = -1; rows = 0;
    };
    for (int c = 0; c < plan.nch(); ++c) {
        if (live && !live[c]) { close(c); continue; }
        const long n = plan.ch[c].njobs;
        if (c0 >= 0 && rows > 0 && rows + n > max_rows) close(c);
        if (c0 < 0) c0 = c;
        rows += n;
    }
    close(plan.nch());
}

Caps capacities(const Plan& plan, long max_rows)
{
    long most = 0;
    for (const Channel& c : plan.ch) most = std::max<long>(most, c.njobs);
    Caps caps;
    caps.yrows = std::min<long>(plan.njobs(), std::max(most, max_rows));
    caps.xrows = std::min<long>(plan.norb_total, caps.yrows);      // every shell a has its job (a, a, 0): a chunk has no more shells than jobs
    caps.chans = plan.nch();
    return caps;
}

}  // namespace dfta_kli
