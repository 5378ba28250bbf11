// plan_main.cpp -- the multigrid's layout planner (dftatom_amd/csrc/poisson_plan.cpp) as a stand-alone program, built with the
// sanitizers (make -C oracle plan); tests/test_poisson_plan.py runs it.
//
//   plan_main           one case per line on stdin, as key=value tokens (the members of PlanInputs and PoissonKnobs, plus occ_res /
//                       occ_res16 / occ_solve: what the occupancy queries answer); prints each plan as one JSON line, in the layout
//                       of tests/golden/poisson_plans.json, followed by its property violations
//   plan_main --sweep   batch 1..256 x four grids x three modes x num_cu {64, 128, 256, 304} x occupancies {0, 1, 2}^2: prints the
//                       property violations and the number of plans made
//
// Properties (of every plan that has no error):
//   (a) more than one workgroup per atom => batch * workgroups per atom <= occupancy * num_cu (all of them co-resident)
//   (b) level offsets start at kPad and are contiguous, n halves, logC + logT == log2(n - 1) on every level that is not sequential
//   (c) the coarse section's arrays and the rc_src slots lie inside 2 kStageArr - 64 doubles and do not overlap
//   (d) resident => logG == 0, res16 => resident
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <map>
#include <sstream>
#include <string>
#include <utility>
#include <vector>

#include "../dftatom_amd/csrc/poisson_plan.h"

using namespace dfta_mg;

struct Case {
    PlanInputs in;
    int occ_res = 0, occ_res16 = 0, occ_solve = 0;
};

static void bind_occupancy(Case& c)
{
    const int r = c.occ_res, r16 = c.occ_res16, s = c.occ_solve;
    c.in.occupancy = [r, r16, s](PlanKernel k) { return k == kKernelSolve ? s : (k == kKernelSolveRes16 ? r16 : r); };
}

static bool parse_case(const std::string& line, Case* c)
{
    std::map<std::string, std::string> kv;
    std::istringstream ss(line);
    for (std::string tok; ss >> tok;) {
        const size_t eq = tok.find('=');
        if (eq == std::string::npos) return false;
        kv[tok.substr(0, eq)] = tok.substr(eq + 1);
    }
    auto num = [&](const char* k, int dflt) { auto it = kv.find(k); return it == kv.end() ? dflt : atoi(it->second.c_str()); };
    PlanInputs& in = c->in;
    PoissonKnobs& K = in.knobs;
    in.N = num("N", 0); in.levels = num("levels", 0); in.uniform = num("uniform", 0); in.batch = num("batch", 1);
    in.delta = kv.count("delta") ? strtod(kv["delta"].c_str(), nullptr) : 0.0;      // (hex floats: exact)
    in.force_logG = num("force_logG", -1); in.mode = num("mode", 0); in.num_cu = num("num_cu", 0);
    c->occ_res = num("occ_res", 0); c->occ_res16 = num("occ_res16", 0); c->occ_solve = num("occ_solve", 0);
    K.group_set = num("group_set", 0); K.group = num("group", -1); K.res = num("res", -1); K.res16 = num("res16", -1);
    K.nostage = num("nostage", 0); K.nostage_wave = num("nostage_wave", 0); K.nostage_shared = num("nostage_shared", 0);
    K.nocoarse = num("nocoarse", 0); K.noxw = num("noxw", 0); K.norc = num("norc", 0);
    K.nofuse3 = num("nofuse3", 0); K.nofuse3_wave = num("nofuse3_wave", 0); K.nohalf129 = num("nohalf129", 0);
    K.nofold = num("nofold", 0); K.nofold_lds = num("nofold_lds", 0); K.nofuse_coop = num("nofuse_coop", 0);
    K.fuse_min_logc = num("fuse_min_logc", kFuseMinLogC); K.dbg = num("dbg", 0);
    K.plain_launch = num("plain_launch", 0); K.fault = num("fault", 0);
    bind_occupancy(*c);
    return in.N > 1 && in.levels >= 1 && in.levels <= kMaxLevels;
}

static void print_plan(const PoissonPlan& P)
{
    const MgDesc& D = P.D;
    if (P.error) { printf("{\"error\": \"%s\"}\n", P.error); return; }
    printf("{\"occ_res\": %d, \"occ_solve\": %d, ", P.occ_res, P.occ_solve);
    printf("\"flags\": {\"resident\": %d, \"res16\": %d, \"plain_launch\": %d, \"fault\": %d, \"tol\": %d, \"adaptive\": %d}, ",
           (int)P.resident, (int)P.res16, (int)P.plain_launch, P.fault, (int)P.tol, (int)P.adaptive);
    printf("\"alloc\": {\"level_store\": %zu, \"cur\": %zu, \"group_ctr\": %zu, \"group_part\": %zu, \"res_slots\": %zu, \"res_spill\": %zu}, ",
           P.n_level_store, P.n_cur, P.n_group_ctr, P.n_group_part, P.n_res_slots, P.n_res_spill);
    printf("\"soff\": %ld, \"desc\": {\"levels\": %d, \"G\": %d, \"logG\": %d, \"dbg\": %d, \"res_kres\": %d, \"res_logC0\": %d, \"fuse_min_logc\": %d, "
           "\"fuse_coop\": %d, \"fuse3\": %d, \"fuse3w\": %d, \"nofold\": %d, \"fold_lds\": %d, \"kcoop\": %d, \"spin_max\": %d, \"per_atom\": %ld, "
           "\"cs_top\": %d, \"xw_top\": %d, \"adaptive\": %d, \"rc_top\": %d, ",
           P.seq_doubles, D.levels, D.G, D.logG, D.dbg, D.res_kres, D.res_logC0, D.fuse_min_logc, D.fuse_coop, D.fuse3, D.fuse3w, D.nofold, D.fold_lds,
           D.kcoop, D.spin_max, D.per_atom, D.cs_top, D.xw_top, D.adaptive, D.rc_top);
    printf("\"rc_src\": [");
    for (int j = 0; j < 6; ++j) printf("%s%d", j ? ", " : "", D.rc_top >= 0 ? D.rc_src[j] : 0);
    printf("], \"cs\": [");      // [phi, src, lc] of levels cs_top .. levels-1
    for (int l = D.cs_top < 0 ? D.levels : D.cs_top; l < D.levels; ++l) printf("%s[%d, %d, %d]", l > D.cs_top ? ", " : "", D.cs_phi[l], D.cs_src[l], D.cs_lc[l]);
    printf("], \"lv\": [");
    for (int l = 0; l < D.levels; ++l) {
        const Lvl& L = D.lv[l];
        printf("%s{\"n\": %d, \"logC\": %d, \"logT\": %d, \"seq\": %d, \"stage\": %d, \"off\": %ld, \"soff\": %ld, \"d\": \"%a\"}", l ? ", " : "",
               L.n, L.logC, L.logT, L.seq, L.stage, L.off, L.soff, L.d);
    }
    printf("]}}\n");
}

// (c): [begin, end) of everything the plan places in the staging memory
static void staging_ranges(const MgDesc& D, std::vector<std::pair<int, int>>* cs, std::vector<std::pair<int, int>>* rc)
{
    for (int l = D.cs_top < 0 ? D.levels : D.cs_top; l < D.levels; ++l) {
        const Lvl& L = D.lv[l];
        if (D.rc_top >= 0 && l >= D.rc_top && L.n > 129) continue;      // run from registers: the section keeps no copy of them
        for (int at : {D.cs_phi[l], D.cs_src[l]}) {
            if (D.cs_lc[l] >= 0) cs->push_back({at - kStagePad, at + std::max(L.n, (64 << D.cs_lc[l]) + 1) + 8});
            else cs->push_back({at, at + L.n + 1});
        }
    }
    for (int j = 0; D.rc_top >= 0 && j < 6 && D.rc_top + j < D.levels; ++j)
        if (D.lv[D.rc_top + j].n >= 257) rc->push_back({D.rc_src[j], D.rc_src[j] + D.lv[D.rc_top + j].n - 1});
}

static int check_properties(const Case& c, const PoissonPlan& P, const char* label)
{
    const PlanInputs& in = c.in;
    const MgDesc& D = P.D;
    int bad = 0;
    auto fail = [&](const char* what) { printf("VIOLATION %s: %s (N %d batch %d mode %d num_cu %d occ %d/%d/%d)\n", label, what, in.N, in.batch, in.mode, in.num_cu, c.occ_res, c.occ_res16, c.occ_solve); ++bad; };
    const int wg = P.resident ? P.res_wg() : D.G;
    const int occ = P.resident ? std::max(P.occ_res, 0) : (P.occ_solve < 0 ? 1 : P.occ_solve);
    if (wg > 1 && (long)in.batch * wg > (long)occ * in.num_cu) fail("(a) a group's launch is not co-resident");
    if (D.G != 1 << D.logG) fail("(a) G != 2^logG");
    long off = kPad;
    int n = in.N;
    for (int l = 0; l < D.levels; ++l) {
        const Lvl& L = D.lv[l];
        if (L.off != off || L.n != n) fail("(b) level offsets / sizes");
        if (!L.seq && (1 << (L.logC + L.logT)) != L.n - 1) fail("(b) logC + logT != log2(n - 1)");
        off += L.n;
        n = (n + 1) / 2;
    }
    if (D.per_atom != off) fail("(b) per_atom");
    std::vector<std::pair<int, int>> cs, rc, all;
    staging_ranges(D, &cs, &rc);
    all = cs;
    all.insert(all.end(), rc.begin(), rc.end());
    std::sort(all.begin(), all.end());
    for (size_t i = 0; i < all.size(); ++i) {
        if (all[i].first < 0 || all[i].second > 2 * kStageArr - 64) fail("(c) outside the staging memory");
        if (i && all[i].first < all[i - 1].second) fail("(c) overlap");
    }
    if (P.resident && D.logG != 0) fail("(d) resident with logG != 0");
    if (P.res16 && !P.resident) fail("(d) res16 without resident");
    return bad;
}

static int sweep()
{
    const int grids[4][2] = {{4097, 12}, {16385, 14}, {131073, 17}, {1048577, 20}};
    const double deltas[4] = {2e-3, 5e-4, 1e-4, 1.25e-5};
    long plans = 0, bad = 0;
    Case c;
    for (int gi = 0; gi < 4; ++gi)
        for (int mode = 0; mode < 3; ++mode)
            for (int num_cu : {64, 128, 256, 304})
                for (int occ_r = 0; occ_r < 3; ++occ_r)
                    for (int occ_s = 0; occ_s < 3; ++occ_s)
                        for (int batch = 1; batch <= 256; ++batch) {
                            c.in.N = grids[gi][0]; c.in.levels = grids[gi][1]; c.in.delta = deltas[gi];
                            c.in.batch = batch; c.in.mode = mode; c.in.num_cu = num_cu;
                            c.occ_res = c.occ_res16 = occ_r; c.occ_solve = occ_s;
                            bind_occupancy(c);
                            PoissonPlan P;
                            if (plan_poisson(c.in, &P)) { printf("VIOLATION sweep: %s\n", P.error); ++bad; continue; }
                            bad += check_properties(c, P, "sweep");
                            ++plans;
                        }
    printf("sweep: %ld plans, %ld violations\n", plans, bad);
    return bad ? 1 : 0;
}

int main(int argc, char** argv)
{
    if (argc > 1 && !strcmp(argv[1], "--sweep")) return sweep();
    int bad = 0, lineno = 0;
    for (std::string line; std::getline(std::cin, line);) {
        ++lineno;
        if (line.empty()) continue;
        Case c;
        if (!parse_case(line, &c)) { fprintf(stderr, "plan_main: line %d: bad case\n", lineno); return 2; }
        PoissonPlan P;
        const int rc = plan_poisson(c.in, &P);
        print_plan(P);
        if (!rc) bad += check_properties(c, P, std::to_string(lineno).c_str());
    }
    return bad ? 1 : 0;
}
