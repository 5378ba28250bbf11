// poisson_plan.cpp -- the multigrid's layout decisions, in the order they depend on each other (see poisson_plan.h).
#include "poisson_plan.h"

#include <algorithm>
#include <cmath>

namespace dfta_mg {
namespace {

// Workgroups per atom: a solve is bound by ONE compute unit's vector-memory path, so while the batch leaves compute
// units idle the fine levels of every atom are shared by a group of G workgroups (all of them must be resident:
// batch * G <= 256 CUs).  A level is shared when every lane of the group still owns >= 8 nodes (>= 4 for G = 16: the
// same four levels at 131073 nodes, with 32 nodes per lane on the finest one -- the most that is staged in LDS).
// round 3, re-measured with the fused visits in place (131073 nodes, ms per solve): 8 atoms 39.8 (G = 16) / 48.7 (8); 12: 42.4 / 50.5;
// 16: 45.0 / 51.4; 32: 59.2 (8) / 71.6 (4); 64: 99.6 (4) / 124 (2) / 149 (1); 96: 150 (2) / 156 (1); 128: 184 (2) / 171 (1).
// End of round 3, with fused visits on the global levels too (gs_fused3, also on shared levels): 16 atoms 45.1 (16) / 50.1 (8);
// 32: 53.6 (8) / 64.7 (4); 64: 77.3 (4) / 99.5 (2) / 137 (1); 96: 113 (2) / 145 (1); 112: 118 / 154; 128: 129 (2) / 153 (1)
int choose_group_size(const PlanInputs& in)
{
    const int batch = in.batch;
    int logG = batch <= 16 ? 4 : (batch <= 32 ? 3 : (batch <= 64 ? 2 : ((batch <= 128 && 2 * batch <= std::max(in.num_cu, 1)) ? 1 : 0)));
    // 1 048 577 nodes, up to four atoms: 32 workgroups per atom (measured: 95.3 -> 84.0 ms for one atom, 99.5 -> 92.0 for four; 64 workgroups
    // 88.5; at eight atoms, and at 131 073 nodes, 16 remain faster: the barrier of a larger group costs more than the shorter chunks save)
    if (batch <= 4 && in.N - 1 >= (1 << 20)) logG = 5;
    if (in.knobs.group >= 0) logG = in.knobs.group;      // measurements: force log2 of the group size
    if (in.force_logG >= 0) logG = in.force_logG;
    return logG;
}

// Resident group (k_poisson_solve_res): where the batch leaves 33 compute units per atom (up to 7 atoms) and level 0 gives every
// lane of kResG x kResNT lanes 4 .. 32 nodes (16385 .. 131073 nodes); the knob POISSON_RES = 0 / 1 switches it off / on, a forced
// group size (POISSON_GROUP, force_logG) selects the staged groups.  Sets res16, D.res_kres and D.res_logC0 (0: no resident layout).
void choose_resident(const PlanInputs& in, PoissonPlan& P)
{
    const PoissonKnobs& K = in.knobs;
    const int batch = in.batch;
    const bool free_choice = in.force_logG < 0 && !K.nostage;     // (the hand-over needs the first coarse level staged)
    // every atom of the batch gets its 33 workgroups at once: up to 7 atoms on 256 compute units (measured: 28.6 .. 29.0 ms per
    // 131073-node solve for 5 .. 7 atoms against 46 .. 48 ms with staged groups of 8)
    bool want = batch * kResWG <= in.num_cu && free_choice && !K.group_set;
    if (K.res >= 0) want = K.res != 0 && free_choice && batch * kResWG <= 256;
    // 8 .. 15 atoms: 17 workgroups per atom, 16 members of 256 lanes whose level 0 takes turns with their other shared levels in
    // LDS (mg_exact16 / mg_tol16); POISSON_RES16 = 0 / 1 switches it off / on (1: for any batch of up to 15 atoms)
    bool want16 = !want && batch * kRes16WG <= in.num_cu && free_choice && !K.group_set && K.res < 0;
    if (K.res16 >= 0) want16 = K.res16 != 0 && free_choice && batch * kRes16WG <= in.num_cu;
    if (want16) { want = true; P.res16 = true; }
    const int lanes = kResG * kResNT;          // (the same 4096 lanes in both configurations)
    if (want && (in.N - 1) % lanes == 0) {
        const int C0 = (in.N - 1) / lanes;
        int lc = 0;
        while ((1 << lc) < C0) ++lc;
        if ((1 << lc) == C0 && lc >= 2 && lc <= 5 && in.levels >= lc + 4) { P.D.res_logC0 = lc; P.D.res_kres = lc - 1; }
    }
}

// Every workgroup of a launch must be resident at once (the members wait for each other): the resident layout is dropped, and a
// staged group halved, until the launch fits what the occupancy queries say.  Returns logG; sets resident, res16, kcoop.
int fit_to_occupancy(const PlanInputs& in, PoissonPlan& P, int logG)
{
    MgDesc& D = P.D;
    if (D.res_kres > 0) {
        P.occ_res = in.occupancy(P.res16 ? kKernelSolveRes16 : kKernelSolveRes);
        const int per_cu = std::max(P.occ_res, 0);
        if (in.batch * P.res_wg() > per_cu * in.num_cu) D.res_kres = 0;
    }
    if (D.res_kres > 0) { logG = 0; P.resident = true; }
    else P.res16 = false;
    P.occ_solve = in.occupancy(kKernelSolve);
    const int per_cu = P.occ_solve < 0 ? 1 : P.occ_solve;
    while (logG > 0 && (in.batch << logG) > per_cu * in.num_cu) --logG;
    D.kcoop = 0;
    int n = in.N;
    for (int l = 0; l < D.levels; ++l, n = (n + 1) / 2)
        if (logG > 0 && (n - 1) >= (kThreads << logG) * (logG >= 4 ? 4 : 8)) D.kcoop = l + 1;
    return D.kcoop == 0 ? 0 : logG;
}

// sizes, offsets and lane split of every level, finest first; returns the LDS doubles of the sequential ones
long lay_out_levels(const PlanInputs& in, MgDesc& D)
{
    long off = kPad, soff = 0;
    double d = in.delta;                       // PoissonSolver.cpp:21-26 (0 on a uniform grid: PoissonSolver(levels), DFTAtom.cpp:89)
    int n = in.N;
    for (int l = 0; l < D.levels; ++l) {
        Lvl& L = D.lv[l];
        L.n = n; L.off = off; L.d = d;
        int lg = 0;
        while ((1 << lg) < n - 1) ++lg;        // n - 1 == 2^lg
        L.stage = 0;
        if (n < kSeqBelow) { L.seq = 1; L.logT = 0; L.logC = lg; L.soff = soff; soff += n; }
        else { L.seq = 0; L.logT = std::min(lg, l < D.kcoop ? 8 + D.logG : 8); L.logC = lg - L.logT; L.soff = -1; }
        off += n;
        n = (n + 1) / 2;
        d *= 2;
    }
    D.per_atom = off;
    return soff;
}

// which chunked levels are swept from a copy in LDS
void classify_staging(const PoissonKnobs& K, MgDesc& D)
{
    if (K.nostage) return;
    for (int l = 0; l < D.levels; ++l) {
        Lvl& L = D.lv[l];
        if (L.seq) continue;
        // (round 6: 2 049 nodes tried -- level 6 inside the coarse section, 32 nodes per lane: the solve got 0.5 ms slower)
        if (l >= D.kcoop && L.n <= kWaveMaxN && L.n >= 129 && !K.nostage_wave) L.stage = 3;
        else if (l >= D.kcoop && L.logT == 8 && L.logC <= kStageMaxLogC) L.stage = 1;
        else if (l < D.kcoop && D.G > 1 && L.logT == 8 + D.logG && L.logC >= 2 && L.logC <= kStageMaxLogC && !K.nostage_shared) L.stage = 2;
    }
}

// coarse section: from the first one-wave level down, if everything below is one-wave or sequential and fits the staging memory
void plan_coarse_section(const PoissonKnobs& K, bool tol, MgDesc& D)
{
    D.cs_top = -1;
    if (K.nocoarse) return;
    int top = -1;
    for (int l = 1; l < D.levels; ++l)
        if (D.lv[l].stage == 3) { top = l; break; }
    bool ok = top >= 1 && top >= D.kcoop + 1 && top <= D.levels - 2;
    int at = 0;
    for (int l = top; ok && l < D.levels; ++l) {
        const Lvl& L = D.lv[l];
        if (L.stage == 3) {
            int lc = 0;
            while ((64 << lc) < L.n - 1) ++lc;                 // n - 1 == 64 * 2^lc
            if (lc < 1 || lc > 4) { ok = false; break; }
            // exact mode: the 129-node level is laid out 4 nodes per lane on 32 lanes (rows of 64 all the same: its last node sits behind
            // the four rows, cs_idx) so that its visits run as the fused three-sweep pass too (gs_lds3 needs >= 4 nodes per lane)
            if (lc == 1 && !tol && !K.nofuse3 && !K.nofuse3_wave && !K.nohalf129) lc = 2;
            const int span = std::max(L.n, (64 << lc) + 1);    // the last node's slot: (2^lc) << 6
            D.cs_lc[l] = lc;
            D.cs_phi[l] = at + kStagePad; at += kStagePad + span + 8;
            D.cs_src[l] = at + kStagePad; at += kStagePad + span + 8;
        } else if (L.seq) {
            D.cs_lc[l] = -1;
            D.cs_phi[l] = at; at += L.n + 1;
            D.cs_src[l] = at; at += L.n + 1;
        } else ok = false;
    }
    if (ok && at <= 2 * kStageArr - 64) D.cs_top = top;
}

// exact mode: the six coarsest levels of the coarse section in registers (poisson_kernels.inc: xw_section), entered from the 129-node level
void plan_xw(const PoissonKnobs& K, bool tol, MgDesc& D)
{
    D.xw_top = -1;
    if (tol || K.noxw || D.cs_top <= 0 || D.levels < 8 || D.levels - 6 <= D.cs_top) return;
    const int l65 = D.levels - 6, l129 = D.levels - 7;
    if (D.lv[l65].n == 65 && D.lv[D.levels - 1].n == 3 && D.cs_lc[l65] < 0 && (D.cs_lc[l129] == 1 || D.cs_lc[l129] == 2) && D.lv[l129].n == 129)
        D.xw_top = l65;
}

// the sources of rc's six register levels live in the staging memory around the coarse section's arrays of the levels it
// still runs (129 nodes and below): 8192 + 4096 behind them, 2048 + 1024 + 512 + 256 in front (where the section's own
// copies of the 1025 .. 257-node levels would be)
bool place_rc_sources(MgDesc& D, int k8193, int sft)
{
    int first10 = 1 << 30, end_cs = 0;
    for (int l = k8193 + 6; l < D.levels; ++l) {
        first10 = std::min(first10, std::min(D.cs_phi[l], D.cs_src[l]) - (D.cs_lc[l] >= 0 ? kStagePad : 0));
        end_cs = std::max(end_cs, std::max(D.cs_phi[l], D.cs_src[l]) + D.lv[l].n + 8);
    }
    const int cap = 2 * kStageArr - 64;
    if (!(first10 >= 3840 && end_cs + 12288 <= cap)) return false;
    const int slot[6] = {end_cs, end_cs + 8192, 0, 2048, 3072, 3584};      // by level: 8193, 4097, 2049, 1025, 513, 257 nodes
    for (int j = 0; j < 6; ++j) D.rc_src[j] = j + sft < 6 ? slot[j + sft] : 0;          // index: level - rc_top
    return true;
}

// tolerance mode: the sub-cycle from the 8193-node level down in registers (poisson_kernels.inc: coarse_resident_cycle) -- 32 nodes per
// thread on its first level, the levels down to 257 nodes halve the chunk, the 129-node level and below run in one wave.  Resident
// groups: the coarse workgroup's levels; staged groups and one workgroup per atom: workgroup 0's, from the first level it does not share
// (8193 nodes for groups of 8 and 16 and for a lone workgroup, 4097 / 2049 nodes -- 16 / 8 per thread -- for groups of 4 / 2)
void plan_rc(const PoissonKnobs& K, bool tol, MgDesc& D)
{
    D.rc_top = -1;
    int k8193 = -1;
    for (int l = 0; l < D.levels; ++l) if (D.lv[l].n == 8193) k8193 = l;
    int sft = 0;                                    // the cycle starts `sft` levels below the 8193-node level
    if (k8193 > 0 && D.res_kres == 0) while (sft < 2 && k8193 + sft < D.kcoop) ++sft;
    if (!tol || K.norc || k8193 <= 0 || D.cs_top <= 0 || !(D.res_kres > 0 ? k8193 == D.res_kres : k8193 + sft >= D.kcoop)) return;
    const int kt = k8193 + sft;
    const Lvl& Lk = D.lv[kt];
    bool ok = !Lk.seq && Lk.logT == 8 && Lk.logC == 5 - sft && k8193 + 6 < D.levels && D.lv[k8193 + 5].n == 257 &&
              D.lv[k8193 + 6].n == 129 && k8193 + 6 >= D.cs_top && D.cs_lc[k8193 + 6] == 1;
    // a wave's scan end value goes to the next wave without what entered the wave itself: a^(64 C) of it, largest on the 257-node level
    // (C = 1, a = (1 + delta_l / 2) / 2) -- 3e-19 on the grids of BASELINE.md; a grid coarse enough to make it matter stays level by level
    if (ok) ok = std::pow(0.5 * (1.0 + 0.5 * D.lv[k8193 + 5].d), 64.0) < 1e-16;
    if (ok && place_rc_sources(D, k8193, sft)) D.rc_top = kt;
}

void count_allocations(const PlanInputs& in, PoissonPlan& P)
{
    const size_t batch = (size_t)in.batch;
    P.n_level_store = (size_t)P.D.per_atom * batch;
    P.n_group_ctr = batch;
    P.n_group_part = batch * group_part_doubles(P.D.G);
    if (P.resident) P.n_res_slots = batch * res_slot_doubles();
    if (P.res16) {
        // per member: Phi and source of level 0 as they lie in LDS (C0 rows of H0 + 256 + 1 columns each)
        const int C0 = 1 << P.D.res_logC0, RS0 = ((P.tol ? kWarm3Tol : kWarm3Exact) + 3 + C0 - 1) / C0 + kRes16NT + 1;
        P.n_res_spill = batch * kRes16G * 2 * C0 * RS0;
    }
}

}  // namespace

int plan_poisson(const PlanInputs& in, PoissonPlan* plan)
{
    *plan = PoissonPlan();
    PoissonPlan& P = *plan;
    MgDesc& D = P.D;
    const PoissonKnobs& K = in.knobs;
    D.levels = in.levels;
    P.tol = in.mode == 1 || in.mode == 2;
    P.adaptive = in.mode == 2;
    P.fault = K.fault;
    // rocprofiler-sdk (ROCm 7.2) crashes in an exit handler of a process that has made a cooperative launch -- after its
    // output is written, but the profiled command returns 139.  Under the profiler (rocprofv3 exports ROCP_TOOL_LIBRARIES), or
    // when DFTA_POISSON_PLAIN_LAUNCH is set, the groups are therefore started with an ordinary launch: same kernel, same
    // results and timing; co-residency then rests on fit_to_occupancy, the bounded spins and the abort flag
    // (dfta_poisson_finish) as in round 1.
    P.plain_launch = K.plain_launch;
    D.spin_max = P.fault ? (1 << 12) : (1 << 23);
    int logG = choose_group_size(in);
    choose_resident(in, P);
    D.logG = fit_to_occupancy(in, P, logG);
    D.G = 1 << D.logG;
    D.nofold = K.nofold ? 1 : 0;
    D.fold_lds = K.nofold_lds ? 0 : 1;
    D.fuse3 = K.nofuse3 ? 0 : 1;
    D.fuse3w = (D.fuse3 && !K.nofuse3_wave) ? 1 : 0;
    D.predict = (D.fuse3w && !P.tol && !K.nopredict) ? (K.predict_fuzz ? 2 : 1) : 0;
    D.fuse_min_logc = K.fuse_min_logc;
    D.fuse_coop = K.nofuse_coop ? 0 : 1;
    D.dbg = K.dbg;
    D.adaptive = P.adaptive ? 1 : 0;
    P.seq_doubles = lay_out_levels(in, D);
    classify_staging(K, D);
    plan_coarse_section(K, P.tol, D);
    plan_xw(K, P.tol, D);
    plan_rc(K, P.tol, D);
    if (P.seq_doubles > kSeqCap) { P.error = "sequential levels exceed LDS budget"; return 1; }
    count_allocations(in, P);
    return 0;
}

}  // namespace dfta_mg
