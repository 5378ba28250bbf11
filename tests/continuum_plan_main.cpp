// continuum_plan_main.cpp -- stand-alone driver of dftatom_amd/csrc/continuum_plan.cpp (pure host code) for tests/test_continuum_ref.py,
// which builds it with -fsanitize=address,undefined: the validation of a call, the grouping of its trials into waves, the partner-count
// instance and the chunking of the rows.  Prints one line per plan; exit status 0 when every validation answers as it should.
#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>

#include "continuum_plan.h"

using namespace dfta_continuum_plan;

static Call base(int N, int nV, const std::vector<int>& v, const std::vector<int>& l, const std::vector<double>& E, const std::vector<int>& m)
{
    Call c;
    c.norm_mode = 0; c.N = N; c.nV = nV; c.ntrials = (int)l.size();
    c.vidx = v.empty() ? nullptr : v.data(); c.l = l.data(); c.E = E.data(); c.m = m.data();
    c.npartner_rows = 0; c.power = 0; c.nlists = 0;
    c.list_off = c.list_rows = c.trial_list = nullptr;
    return c;
}

int main()
{
    int bad = 0;
    const int N = 4097;
    std::vector<int> v = {0, 1, 2, 0}, l = {0, 4, 2, 0}, m = {3, N - 2, 255, 256};
    std::vector<double> E = {-3., 0., 1e-3, 8.};
    Call c = base(N, 3, v, l, E, m);
    bad += check(c) != nullptr;
    c.norm_mode = 1;
    bad += check(c) != nullptr;
    c.norm_mode = 2;
    bad += check(c) == nullptr;
    c.norm_mode = 0;
    c.N = 4;
    bad += check(c) == nullptr;
    c.N = N;
    for (int wrong : {-1, 5}) { std::vector<int> lw = l; lw[1] = wrong; Call w = c; w.l = lw.data(); bad += check(w) == nullptr; }
    for (int wrong : {2, -1, N - 1, N}) { std::vector<int> mw = m; mw[2] = wrong; Call w = c; w.m = mw.data(); bad += check(w) == nullptr; }
    for (double wrong : {std::nan(""), std::numeric_limits<double>::infinity(), -std::numeric_limits<double>::infinity()}) {
        std::vector<double> Ew = E; Ew[3] = wrong; Call w = c; w.E = Ew.data(); bad += check(w) == nullptr;
    }
    for (int wrong : {-1, 3}) { std::vector<int> vw = v; vw[0] = wrong; Call w = c; w.vidx = vw.data(); bad += check(w) == nullptr; }
    for (int wrong : {-1, 9}) { Call w = c; w.power = wrong; bad += check(w) == nullptr; }
    {   // partner lists: 17 in a list, a row out of range, offsets that descend, a trial's list out of range
        std::vector<int> rows(17);
        for (int j = 0; j < 17; ++j) rows[j] = j;
        std::vector<int> off = {0, 16, 17}, tl = {0, 1, -1, 0};
        Call w = c;
        w.npartner_rows = 17; w.nlists = 2; w.list_off = off.data(); w.list_rows = rows.data(); w.trial_list = tl.data();
        bad += check(w) != nullptr;
        std::vector<int> off17 = {0, 17, 17};
        w.list_off = off17.data();
        bad += check(w) == nullptr;
        w.list_off = off.data();
        w.npartner_rows = 16;
        bad += check(w) == nullptr;
        w.npartner_rows = 17;
        std::vector<int> offd = {0, 5, 3};
        w.list_off = offd.data();
        bad += check(w) == nullptr;
        w.list_off = off.data();
        std::vector<int> tlw = {0, 2, -1, 0};
        w.trial_list = tlw.data();
        bad += check(w) == nullptr;
        tlw[1] = -2;
        bad += check(w) == nullptr;
    }
    bad += instance_for(0) != 0 || instance_for(1) != 4 || instance_for(4) != 4 || instance_for(5) != 8 || instance_for(9) != 16 || instance_for(16) != 16;

    // plans: (trials per group ...) -> blocks, padded positions, instance, chunk
    // a group is an l of potential 0, or (by_potential) a potential of its own with l = group % 5: more than five groups
    struct Shape { int N; std::vector<int> groups; int partners; bool rows; bool by_potential; };
    const Shape shapes[] = {{4097, {1}, 0, false, false}, {4097, {63, 64, 65}, 5, true, false}, {4097, {129}, 16, false, false},
                            {131073, {256, 256, 256, 256, 256}, 11, true, false}, {9, {70000}, 0, true, false},
                            {9, std::vector<int>(1100, 1), 3, true, true}, {1025, std::vector<int>(520, 1), 3, true, true}};
    for (const Shape& sh : shapes) {
        std::vector<int> vv, ll, mm, tl, off = {0}, rows;
        std::vector<double> EE;
        for (size_t gi = 0; gi < sh.groups.size(); ++gi)
            for (int t = 0; t < sh.groups[gi]; ++t) {
                vv.push_back(sh.by_potential ? (int)gi : 0); ll.push_back(sh.by_potential ? (int)gi % 5 : (int)gi);
                mm.push_back(3); EE.push_back(1.); tl.push_back(0);
            }
        // interleave: the trials of a group need not be adjacent in the call
        if (vv.size() > 2) { std::swap(ll[0], ll[vv.size() - 1]); }
        for (int j = 0; j < sh.partners; ++j) rows.push_back(j);
        off.push_back(sh.partners);
        Call w = base(sh.N, sh.by_potential ? (int)sh.groups.size() : 1, vv, ll, EE, mm);
        if (sh.partners) { w.npartner_rows = sh.partners; w.nlists = 1; w.list_off = off.data(); w.list_rows = rows.data(); w.trial_list = tl.data(); }
        bad += check(w) != nullptr;
        const Plan p = plan(w, sh.rows);
        // every trial exactly once, every block of one group
        std::vector<int> seen(vv.size(), 0);
        for (const Block& b : p.blocks)
            for (int j = 0; j < kWave; ++j) {
                const int t = p.order[b.first + j];
                if (j < b.cnt) { bad += t < 0 || ll[t] != b.l || vv[t] != b.v || b.first % kWave != 0; if (t >= 0) ++seen[t]; }
                else bad += t != -1;
            }
        for (int sgn : seen) bad += sgn != 1;
        std::printf("plan %d %zu %zu %zu %d %d\n", sh.N, vv.size(), p.blocks.size(), p.order.size(), p.instance, p.blocks_per_chunk);
    }
    return bad;
}
