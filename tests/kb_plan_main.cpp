// kb_plan_main.cpp -- stand-alone driver of dftatom_amd/csrc/kb_plan.cpp (pure host code) for tests/test_kb_ref.py, which builds it with
// -fsanitize=address,undefined -ffp-contract=off: the last non-zero node of a projector, the validation of a call, the grouping of its
// trials into waves and the chunking of the rows, the search's three formulas, open_brackets and cut_bracket called directly, and the
// whole search on a synthetic sign function u(E) = Prod_j (E - root_j) with windows in which the value is not finite.  Exit status 0:
// every expectation the program holds itself was met.  What tests/_kb_ref.py restates is printed, doubles as %a, and compared there bit
// for bit: the lines "lastnz", "plan", "scan", "cut" and, per search, its definition ("search", "chan") and its "result".
//
// DFTA_KB_SEARCH_CAP: a bracket's width shrinks 65-fold a round and the bracket is closed once the width is an ulp of the state, so a
// state E* inside a bracket of width W takes about log65(W / ulp(E*)) rounds: 9 to 11 for any state of the size of its range, the widest
// range that the scan's formula admits -- (hi - lo) (nscan - 1) must stay finite -- included; the searches "widest" hold that.  Through
// these formulas the cap is out of reach of every state that is not 65^22 = 8e39 times nearer to E = 0 than its scan interval is wide.
// What is left is a zero of u~_m AT E = 0 inside a range that straddles 0: the bracket then shrinks around 0 for hundreds of rounds.  No
// physical channel is known to do that; the search "cap" takes the exit with u(E) = E, so that code and model agree there as well.
#include <cmath>
#include <cstdio>
#include <limits>
#include <string>
#include <vector>

#include "../include/dftatom_hip.h"
#include "kb_plan.h"

using namespace dfta_kb_plan;

static const double kInf = std::numeric_limits<double>::infinity();
static const double kNan = std::numeric_limits<double>::quiet_NaN();
static int bad = 0;

#define EXPECT(cond) do { if (!(cond)) { ++bad; std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); } } while (0)

// ---- last_nonzero ------------------------------------------------------------------------------------------------------------------------
static void run_last_nonzero()
{
    const int N = 7;
    std::vector<double> beta((size_t)6 * N, 0.);
    for (int i = 0; i < N; ++i) beta[(size_t)1 * N + i] = -0.;         // row 0: all zero; row 1: all -0.0
    beta[(size_t)2 * N + 3] = kNan;                                       // a NaN node is not 0.0
    beta[(size_t)3 * N + 0] = 2.;                                         // a lone non-zero at node 0 ...
    beta[(size_t)4 * N + N - 1] = -1e-300;                                // ... and at N-1
    beta[(size_t)5 * N + 2] = 1.; beta[(size_t)5 * N + 4] = -0.;
    const std::vector<int> got = last_nonzero(6, N, beta.data());
    const int want[6] = {0, 0, 3, 0, N - 1, 2};
    EXPECT(got.size() == 6);
    std::printf("lastnz");
    for (size_t k = 0; k < got.size(); ++k) { EXPECT(got[k] == want[k]); std::printf(" %d", got[k]); }
    std::printf("\n");
    EXPECT(last_nonzero(0, N, beta.data()).empty());
    EXPECT(last_nonzero(0, N, nullptr).empty());
}

// ---- check ---------------------------------------------------------------------------------------------------------------------------------
static void run_check()
{
    const int N = 300, nV = 2, nch = 2;
    std::vector<double> beta((size_t)nch * N, 0.);
    for (int i = 1; i <= 200; ++i) beta[i] = 1.;                         // channel 0 ends at node 200, channel 1 is all zero
    const std::vector<int> lastnz = last_nonzero(nch, N, beta.data());
    EXPECT(lastnz[0] == 200 && lastnz[1] == 0);
    const std::vector<int> vidx = {1, 0}, l = {0, 4}, chan = {0, 1, 0}, m = {200, 3, N - 2};
    const std::vector<double> q1 = {0.75, -0.4}, E = {-3., 0., 1e6};
    Call c;
    c.N = N; c.nV = nV; c.nch = nch; c.ntrials = 3;
    c.vidx = vidx.data(); c.l = l.data(); c.beta = beta.data(); c.q1 = q1.data(); c.chan = chan.data(); c.E = E.data(); c.m = m.data();
    int refused = 0;
    auto refuse = [&](const Call& w) { const bool r = check(w, lastnz) != nullptr; EXPECT(r); refused += r; };
    EXPECT(check(c, lastnz) == nullptr);                                  // m = lastnz itself is accepted (trial 0)
    { Call w = c; w.vidx = nullptr; EXPECT(check(w, lastnz) == nullptr); }
    { Call w = c; w.N = 4; refuse(w); }
    { Call w = c; w.N = 5; const std::vector<int> m5 = {3, 3, 3}; w.m = m5.data(); const std::vector<int> z = {0, 0}; EXPECT(check(w, z) == nullptr); }
    { Call w = c; w.nV = 0; refuse(w); }
    { Call w = c; w.nch = 0; refuse(w); }
    for (int wrong : {-1, nV}) { std::vector<int> v = vidx; v[1] = wrong; Call w = c; w.vidx = v.data(); refuse(w); }
    for (int wrong : {-1, 5}) { std::vector<int> v = l; v[0] = wrong; Call w = c; w.l = v.data(); refuse(w); }
    for (double wrong : {0., -0., kNan, kInf, -kInf}) { std::vector<double> v = q1; v[1] = wrong; Call w = c; w.q1 = v.data(); refuse(w); }
    for (int wrong : {-1, nch}) { std::vector<int> v = chan; v[2] = wrong; Call w = c; w.chan = v.data(); refuse(w); }
    for (double wrong : {kNan, kInf, -kInf}) { std::vector<double> v = E; v[1] = wrong; Call w = c; w.E = v.data(); refuse(w); }
    for (int wrong : {2, N - 1}) { std::vector<int> v = m; v[1] = wrong; Call w = c; w.m = v.data(); refuse(w); }
    { std::vector<int> v = m; v[0] = 199; Call w = c; w.m = v.data(); refuse(w); }                     // m = lastnz - 1
    { std::vector<int> v = m; v[2] = 199; Call w = c; w.m = v.data(); refuse(w); }
    EXPECT(refused == 21);
    // chan null puts every trial into channel 0, whose projector ends at 200: trial 1 (m = 3) is then below it
    { std::vector<int> v = {200, 201, N - 2}; Call w = c; w.chan = nullptr; w.m = v.data(); EXPECT(check(w, lastnz) == nullptr); }
    { Call w = c; w.ntrials = 0; w.chan = nullptr; w.E = nullptr; w.m = nullptr; EXPECT(check(w, lastnz) == nullptr); }
    std::printf("check %d\n", refused);
}

// ---- plan ----------------------------------------------------------------------------------------------------------------------------------
// groups[k] trials of channel k, interleaved round robin; prints: plan N ntrials want_rows force blocks positions blocks_per_chunk
static void run_plan(int N, const std::vector<int>& groups, bool want_rows, int force)
{
    std::vector<int> chan;
    std::vector<int> left = groups;
    const int nch = (int)groups.size();
    for (bool any = true; any;) {                    // channel nch-1 first: the order of first appearance is not the channel's number
        any = false;
        for (int k = nch - 1; k >= 0; --k)
            if (left[k] > 0) { chan.push_back(k); --left[k]; any = true; }
    }
    Call c = {};
    c.N = N; c.nV = 1; c.nch = nch; c.ntrials = (int)chan.size(); c.chan = chan.data();
    const Plan p = plan(c, want_rows, force);
    std::vector<int> seen(chan.size(), 0), first_seen;
    int last_first = -kWave;
    for (const Block& b : p.blocks) {
        EXPECT(b.first % kWave == 0 && b.first == last_first + kWave && b.cnt >= 1 && b.cnt <= kWave);
        last_first = b.first;
        if (first_seen.empty() || first_seen.back() != b.chan) first_seen.push_back(b.chan);
        int prev = -1;
        for (int j = 0; j < kWave; ++j) {
            const int t = p.order[(size_t)b.first + j];
            if (j < b.cnt) {
                EXPECT(t >= 0 && t < c.ntrials && chan[t] == b.chan && t > prev);      // one channel a block, trials in call order
                if (t >= 0 && t < c.ntrials) ++seen[t];
                prev = t;
            } else EXPECT(t == -1);
        }
    }
    EXPECT(p.order.size() == p.blocks.size() * (size_t)kWave);
    for (int s : seen) EXPECT(s == 1);
    // channels in the order of first appearance: nch-1, nch-2, ..., each once; a channel's blocks are full but the last
    EXPECT((int)first_seen.size() == nch);
    for (int k = 0; k < (int)first_seen.size(); ++k) EXPECT(first_seen[k] == nch - 1 - k);
    size_t at = 0;
    for (int k = nch - 1; k >= 0; --k)
        for (int left_k = groups[k]; left_k > 0; left_k -= kWave, ++at) EXPECT(at < p.blocks.size() && p.blocks[at].cnt == std::min(left_k, kWave));
    EXPECT(at == p.blocks.size());
    std::printf("plan %d %zu %d %d %zu %zu %d\n", N, chan.size(), (int)want_rows, force, p.blocks.size(), p.order.size(), p.blocks_per_chunk);
}

static void run_plans()
{
    const std::vector<int> mixed = {1, 63, 64, 65, 129};                 // 1 + 1 + 1 + 2 + 3 = 8 waves
    run_plan(4097, mixed, false, 0);                                      // no rows: 0
    run_plan(4097, mixed, true, 0);                                       // fewer waves than fit: the wave count, 8
    run_plan(4097, mixed, true, 1);
    run_plan(4097, mixed, true, 2);
    run_plan(4097, mixed, true, 3);
    run_plan(4097, mixed, true, 100);                                     // a forced chunk above the wave count: 8
    run_plan(4097, {4096}, true, 0);                                      // 64 waves, 63 fit 256 MiB
    run_plan(65537, {200, 120}, true, 0);                                 // 4 + 2 waves, 3 fit
    run_plan(131073, {65, 1}, true, 0);                                   // 1 fits
    run_plan(9, {70000}, true, 0);                                        // 1094 waves: the combining launch's grid caps a chunk at 1023
    run_plan(9, {70000}, true, 2);
    run_plan(300000, {65}, true, 0);                                      // no wave fits 256 MiB: 1
    run_plan(9, {}, true, 0);                                             // no trial: no block, 1
    Call c = {};                                                          // chan null: one channel, 0
    c.N = 9; c.nV = 1; c.nch = 1; c.ntrials = 65;
    const Plan p = plan(c, true, 0);
    EXPECT(p.blocks.size() == 2 && p.blocks[0].chan == 0 && p.blocks[1].cnt == 1 && p.order[64] == 64 && p.order[65] == -1 && p.blocks_per_chunk == 2);
}

// ---- the formulas --------------------------------------------------------------------------------------------------------------------------
static void run_formulas()
{
    struct Scan { double lo, hi; int nscan; };
    const Scan scans[] = {{-1., 0., 64}, {-6., 3., 128}, {-200., 0., 64}, {-0.3, 0.7, 192}, {-1.0000000000000002, -1., 64}};
    for (const Scan& s : scans) {
        std::printf("scan %a %a %d", s.lo, s.hi, s.nscan);
        for (int k = 0; k < s.nscan; ++k) std::printf(" %a", scan_energy(s.lo, s.hi, s.nscan, k));
        std::printf("\n");
        EXPECT(scan_energy(s.lo, s.hi, s.nscan, 0) == s.lo);
    }
    const double x = -0.4748100000000001, y = 3.0e-7;
    const double pairs[][2] = {{-1., 0.}, {-0.5079365079365079, -0.4920634920634921}, {-0.1, 0.2},
                               {x, std::nextafter(x, kInf)},                                                        // two neighbouring doubles
                               {x, std::nextafter(std::nextafter(x, kInf), kInf)},                                  // one double between
                               {x, std::nextafter(std::nextafter(std::nextafter(x, kInf), kInf), kInf)},            // three ulps wide
                               {y, std::nextafter(std::nextafter(std::nextafter(y, kInf), kInf), kInf)},
                               {-std::numeric_limits<double>::denorm_min(), std::numeric_limits<double>::denorm_min()},
                               {-std::numeric_limits<double>::max() / 128., std::numeric_limits<double>::max() / 128.}};
    for (const auto& p : pairs) {
        std::printf("cut %a %a %d", p[0], p[1], (int)bracket_closed(p[0], p[1]));
        for (int j = 0; j < kCuts; ++j) {
            const double e = cut_energy(p[0], p[1], j);
            EXPECT(e >= p[0] && e <= p[1] && (j == 0 || e >= cut_energy(p[0], p[1], j - 1)));     // the clamp: no cut leaves [a, b]
            std::printf(" %a", e);
        }
        std::printf("\n");
    }
    EXPECT(bracket_closed(x, std::nextafter(x, kInf)) && !bracket_closed(x, std::nextafter(std::nextafter(x, kInf), kInf)));
    EXPECT(bracket_closed(1., 1.) && bracket_closed(-0., 0.) && !bracket_closed(-1., 0.));
}

// ---- open_brackets and cut_bracket, called directly ------------------------------------------------------------------------------------------
static void run_brackets()
{
    {   // nine sign changes open eight brackets, ascending
        const int n = 16;
        std::vector<double> E(n);
        std::vector<unsigned char> fin(n, 1), neg(n);
        for (int k = 0; k < n; ++k) { E[k] = -2. + 0.125 * k; neg[k] = k < 10 ? (k % 2 == 0) : 0; }      // changes at k = 0 .. 8
        const std::vector<Bracket> br = open_brackets(n, E.data(), fin.data(), neg.data());
        EXPECT(br.size() == (size_t)kMaxStates);
        for (size_t q = 0; q < br.size(); ++q) EXPECT(br[q].a == E[q] && br[q].b == E[q + 1] && br[q].neg_a == (q % 2 == 0));
        // a non-finite neighbour opens nothing: the changes at k = 2 (2, 3) and k = 3 (3, 4) go
        fin[3] = 0;
        const std::vector<Bracket> b2 = open_brackets(n, E.data(), fin.data(), neg.data());
        EXPECT(b2.size() == 7 && b2[1].a == E[1] && b2[2].a == E[4] && b2[6].a == E[8]);
        std::vector<unsigned char> none(n, 0);
        EXPECT(open_brackets(n, E.data(), none.data(), neg.data()).empty());
        std::vector<unsigned char> same(n, 1);
        EXPECT(open_brackets(n, E.data(), fin.data(), same.data()).empty());
    }
    std::vector<double> e(kCuts);
    for (int j = 0; j < kCuts; ++j) e[j] = cut_energy(-1., 0., j);
    for (int neg_a = 0; neg_a < 2; ++neg_a) {
        const unsigned char sa = (unsigned char)neg_a, sb = (unsigned char)!neg_a;
        std::vector<unsigned char> fin(kCuts, 1), neg(kCuts, sa);
        Bracket br = {-1., 0., neg_a != 0};
        EXPECT(!cut_bracket(&br, e.data(), fin.data(), neg.data()) && br.a == e[63] && br.b == 0. && br.neg_a == (neg_a != 0));      // no cut of b's sign
        std::fill(neg.begin(), neg.end(), sb);
        br = {-1., 0., neg_a != 0};
        EXPECT(!cut_bracket(&br, e.data(), fin.data(), neg.data()) && br.a == -1. && br.b == e[0]);                                  // the first cut has it
        std::fill(neg.begin(), neg.end(), sa);
        for (int j = 20; j < kCuts; ++j) neg[j] = sb;
        neg[40] = sa;                                                                                                              // the FIRST pair
        br = {-1., 0., neg_a != 0};
        EXPECT(!cut_bracket(&br, e.data(), fin.data(), neg.data()) && br.a == e[19] && br.b == e[20]);
        // a non-finite cut takes a's sign, whatever its own: below the pair ...
        fin[5] = 0; neg[5] = sb;
        br = {-1., 0., neg_a != 0};
        EXPECT(cut_bracket(&br, e.data(), fin.data(), neg.data()) && br.a == e[19] && br.b == e[20]);
        // ... at the pair: cut 20 no longer ends it
        fin[5] = 1; neg[5] = sa; fin[20] = 0;
        br = {-1., 0., neg_a != 0};
        EXPECT(cut_bracket(&br, e.data(), fin.data(), neg.data()) && br.a == e[20] && br.b == e[21]);
        // ... and ABOVE the pair: the bracket is the same, the flag is raised all the same (the header: a value that is not finite sets it)
        fin[20] = 1; fin[50] = 0;
        br = {-1., 0., neg_a != 0};
        EXPECT(cut_bracket(&br, e.data(), fin.data(), neg.data()) && br.a == e[19] && br.b == e[20]);
        fin[50] = 1; fin[63] = 0;
        br = {-1., 0., neg_a != 0};
        EXPECT(cut_bracket(&br, e.data(), fin.data(), neg.data()) && br.a == e[19] && br.b == e[20]);
        // all 64 not finite: (e_63, b)
        std::fill(fin.begin(), fin.end(), 0);
        br = {-1., 0., neg_a != 0};
        EXPECT(cut_bracket(&br, e.data(), fin.data(), neg.data()) && br.a == e[63] && br.b == 0.);
    }
}

// ---- the search on a synthetic sign function -----------------------------------------------------------------------------------------------
struct Window { double lo, hi; int kind; };          // lo < E < hi: 0 u = NaN, 1 a status bit (u stays finite), 2 u = +inf, 3 u = -inf
struct Channel {
    double lo, hi;
    std::vector<double> roots;
    std::vector<Window> windows;
};

static int g_launches;

static Evaluate evaluator(const std::vector<Channel>& chs)
{
    return [&chs](const std::vector<int>& chan, const std::vector<double>& E, const std::vector<int>& m, std::vector<double>* u,
                  std::vector<int>* st) -> int {
        ++g_launches;
        EXPECT(chan.size() == E.size() && chan.size() == m.size() && chan.size() % kWave == 0 && !chan.empty());
        u->assign(E.size(), 0.); st->assign(E.size(), 0);
        for (size_t t = 0; t < E.size(); ++t) {
            EXPECT(chan[t] >= 0 && chan[t] < (int)chs.size() && m[t] == 100 + chan[t]);
            EXPECT(t % kWave == 0 || chan[t] == chan[t - 1]);            // a wave of trials is of one channel
            const Channel& c = chs[(size_t)chan[t]];
            double v = E[t] - c.roots[0];
            for (size_t j = 1; j < c.roots.size(); ++j) v = v * (E[t] - c.roots[j]);
            for (const Window& w : c.windows)
                if (w.lo < E[t] && E[t] < w.hi) {
                    if (w.kind == 0) v = kNan;
                    if (w.kind == 1) (*st)[t] = DFTA_CONT_NONFINITE;
                    if (w.kind == 2) v = kInf;
                    if (w.kind == 3) v = -kInf;
                }
            (*u)[t] = v;
        }
        return DFTA_OK;
    };
}

// prints the search's definition and its result; returns the result
static SearchResult run_search(const char* name, const std::vector<Channel>& chs, int nscan)
{
    std::vector<SearchChannel> sc;
    for (size_t k = 0; k < chs.size(); ++k) sc.push_back({100 + (int)k, chs[k].lo, chs[k].hi});
    SearchResult res;
    g_launches = 0;
    EXPECT(search(sc, nscan, evaluator(chs), &res) == DFTA_OK);
    std::printf("search %s %d %zu\n", name, nscan, chs.size());
    int most = 0;
    for (size_t k = 0; k < chs.size(); ++k) {
        std::printf("chan %a %a %zu", chs[k].lo, chs[k].hi, chs[k].roots.size());
        for (double r : chs[k].roots) std::printf(" %a", r);
        for (const Window& w : chs[k].windows) std::printf(" %a %a %d", w.lo, w.hi, w.kind);
        std::printf("\n");
        std::printf("result %d %d %d", res.count[k], res.rounds[k], res.status[k]);
        for (int q = 0; q < kMaxStates; ++q) std::printf(" %a", res.energies[k * kMaxStates + q]);
        std::printf("\n");
        EXPECT(res.count[k] >= 0 && res.count[k] <= kMaxStates);
        for (int q = 0; q < kMaxStates; ++q) {
            const double e = res.energies[k * kMaxStates + q];
            EXPECT(q < res.count[k] ? (e >= chs[k].lo && e < chs[k].hi && (q == 0 || e > res.energies[k * kMaxStates + q - 1])) : std::isnan(e));
        }
        most = std::max(most, res.rounds[k]);
    }
    EXPECT(g_launches == most);                      // one launch a round, whatever the channels and their brackets
    return res;
}

static void run_searches()
{
    const int NF = DFTA_KB_SEARCH_NONFINITE, FULL = DFTA_KB_SEARCH_FULL, CAP = DFTA_KB_SEARCH_CAP;
    SearchResult r;
    // two channels with different ranges (and closing rounds) in one call
    r = run_search("two", {{-1., 0., {-0.5, -0.2}, {}}, {-4., -0.5, {-3.3, -1.7, -0.9}, {}}, {-0.4, 0., {-0.5}, {}}, {-2., 2., {0.25}, {}},
                            {-0.2500001, -0.2499999, {-0.25}, {}}}, 64);
    EXPECT(r.count[0] == 2 && r.count[1] == 3 && r.count[2] == 0 && r.count[3] == 1 && r.count[4] == 1 && r.rounds[2] == 1 && r.status == std::vector<int>(5, 0));
    EXPECT(r.energies[3 * kMaxStates] == std::nextafter(0.25, -kInf) || r.energies[3 * kMaxStates] == 0.25);
    // 8 roots: not FULL; 9: FULL, the lowest 8 kept
    r = run_search("eight", {{-1., 0., {-0.9, -0.8, -0.7, -0.6, -0.5, -0.4, -0.3, -0.2}, {}}}, 64);
    EXPECT(r.count[0] == 8 && r.status[0] == 0);
    r = run_search("nine", {{-1., 0., {-0.9, -0.8, -0.7, -0.6, -0.5, -0.4, -0.3, -0.2, -0.1}, {}}}, 64);
    EXPECT(r.count[0] == 8 && r.status[0] == FULL && r.energies[7] < -0.15);
    // a window that covers a root: the scan points in it open nothing, the root is lost, nothing is flagged (round 0 flags nothing)
    r = run_search("covered", {{-1., 0., {-0.6, -0.3}, {{-0.31, -0.29, 0}}}}, 64);
    EXPECT(r.count[0] == 1 && r.status[0] == 0);
    // a window inside a bracket BELOW the pair the cut picks, each kind of "not finite"
    for (int kind = 0; kind < 4; ++kind) {
        r = run_search(("below" + std::to_string(kind)).c_str(), {{-1., 0., {-0.5}, {{-0.5070, -0.5060, kind}}}}, 64);
        EXPECT(r.count[0] == 1 && r.status[0] == NF);
    }
    // ... and ABOVE it: u(E) = (E + 0.1)(E + 0.47481)(E + 0.85924), not finite for -0.4701 < E < -0.46999
    r = run_search("above", {{-1., 0., {-0.1, -0.47481, -0.85924}, {{-0.4701, -0.46999, 0}}}}, 64);
    EXPECT(r.count[0] == 3 && r.rounds[0] == 10 && r.status[0] == NF);
    r = run_search("above1", {{-1., 0., {-0.1, -0.47481, -0.85924}, {{-0.4701, -0.46999, 1}}}}, 64);
    EXPECT(r.count[0] == 3 && r.status[0] == NF);
    // a window over the low end of round 0
    r = run_search("lowend", {{-1., 0., {-0.5}, {{-1.1, -0.9, 0}}}}, 64);
    EXPECT(r.count[0] == 1 && r.status[0] == 0);
    r = run_search("allbad", {{-1., 0., {-0.5}, {{-2., 1., 2}}}}, 64);
    EXPECT(r.count[0] == 0 && r.rounds[0] == 1 && r.status[0] == 0);
    // a range with no root
    r = run_search("none", {{-0.4, 0., {-0.5}, {}}}, 128);
    EXPECT(r.count[0] == 0 && r.rounds[0] == 1 && r.status[0] == 0);
    // FULL and NONFINITE together, beside a clean channel
    r = run_search("both", {{-1., 0., {-0.9, -0.8, -0.7, -0.6, -0.5, -0.4, -0.3, -0.2, -0.1}, {{-0.5070, -0.5060, 3}}}, {-1., 0., {-0.5}, {}}}, 64);
    EXPECT(r.count[0] == 8 && r.status[0] == (NF | FULL) && r.count[1] == 1 && r.status[1] == 0);
    // the cap: the widest range the scan admits closes in far fewer than 32 rounds wherever the state is of the range's size ...
    const double big = std::numeric_limits<double>::max() / 128.;
    r = run_search("widest", {{-big, big, {big / 3.}, {}}, {-big, big, {-big * 0.99}, {}}, {-big, big, {big * 1e-3}, {}}, {-1e-300, 1e-300, {3e-301}, {}}}, 64);
    for (int k = 0; k < 4; ++k) EXPECT(r.count[k] == 1 && r.status[k] == 0 && r.rounds[k] <= 13);
    // ... and is reached only by a zero 65^22 times nearer to E = 0 than the scan interval is wide: u(E) = E
    r = run_search("cap", {{-1., 1., {0.}, {}}, {-1., 1., {0.3}, {}}}, 64);
    EXPECT(r.count[0] == 1 && r.rounds[0] == kMaxRounds && r.status[0] == CAP && r.energies[0] < 0. && r.energies[0] > -1e-50);
    EXPECT(r.count[1] == 1 && r.rounds[1] <= 12 && r.status[1] == 0);

    // an evaluation that fails: its code comes back, from round 0 and from a later round
    for (int fail_at = 1; fail_at <= 3; fail_at += 2) {
        int calls = 0;
        const std::vector<Channel> chs = {{-1., 0., {-0.5}, {}}};
        const Evaluate inner = evaluator(chs);
        const Evaluate failing = [&](const std::vector<int>& chan, const std::vector<double>& E, const std::vector<int>& m, std::vector<double>* u,
                                     std::vector<int>* st) -> int {
            if (++calls == fail_at) return DFTA_ERR_HIP;
            return inner(chan, E, m, u, st);
        };
        SearchResult res;
        EXPECT(search({{100, -1., 0.}}, 64, failing, &res) == DFTA_ERR_HIP && calls == fail_at);
    }
    SearchResult empty;
    // no channel: one (empty) evaluation of round 0 is still asked for; nothing to report
    const Evaluate nothing = [](const std::vector<int>& chan, const std::vector<double>&, const std::vector<int>&, std::vector<double>* u,
                                std::vector<int>* st) -> int { u->assign(chan.size(), 0.); st->assign(chan.size(), 0); return DFTA_OK; };
    EXPECT(search({}, 64, nothing, &empty) == DFTA_OK && empty.count.empty() && empty.energies.empty());
}

int main()
{
    run_last_nonzero();
    run_check();
    run_plans();
    run_formulas();
    run_brackets();
    run_searches();
    std::printf("done %d\n", bad);
    return bad ? 1 : 0;
}
