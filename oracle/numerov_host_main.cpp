// numerov_host_main.cpp -- the pure host logic of the Numerov layer (dftatom_amd/csrc/numerov_host.cpp) as a stand-alone program, built
// with the sanitizers (make -C oracle numerov_host) and linked with the oracle; tests/test_numerov_host.py runs it.
//
//   numerov_host_main boundary   host_boundary / host_boundary_uniform against dfo_max_radius_index, dfo_far and dfo_ucount_nodes
//   numerov_host_main grouping   properties of make_grouping; make_grouping_of_groups against the loop it replaced
//   numerov_host_main staging    properties of stage_layout for 1..300 trials and both calls
//   numerov_host_main persist    properties of plan_persist, and its output against the loop it replaced (kept below, verbatim)
//
// Every check that fails prints a line "VIOLATION ..."; every mode ends with one summary line that says how many cases it ran.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../dftatom_amd/csrc/numerov_host.h"
#include "dfta_oracle.h"

using namespace dfta_nh;

static int g_violations = 0;
#define CHECK(cond, ...)                                                      \
    do {                                                                      \
        if (!(cond)) {                                                        \
            ++g_violations;                                                   \
            printf("VIOLATION %s:%d %s: ", __func__, __LINE__, #cond);        \
            printf(__VA_ARGS__);                                              \
            printf("\n");                                                     \
        }                                                                     \
    } while (0)

// the tests' fixed generator (a 64-bit LCG, its high bits)
struct Rng {
    unsigned long long s;
    explicit Rng(unsigned long long seed) : s(seed) {}
    int below(int n) { s = s * 6364136223846793005ull + 1442695040888963407ull; return static_cast<int>((s >> 33) % static_cast<unsigned long long>(n)); }
};

static bool same_bits(double a, double b) { return memcmp(&a, &b, sizeof(double)) == 0; }

// ---- boundary values ----------------------------------------------------------------------------------------------------------
static std::vector<double> energies()      // 200 values from -4000 to -1e-4 in geometric steps
{
    std::vector<double> E;
    for (int k = 0; k < 200; ++k) E.push_back(-4000. * pow(1e-4 / 4000., k / 199.));
    return E;
}

static void boundary_log(int N, double delta, double Rmax)
{
    dfo_grid og;
    dfo_grid_init(&og, N, delta, Rmax);
    std::vector<double> r(N);
    for (int i = 0; i < N; ++i) r[i] = dfo_position(&og, i);
    GridView gv;
    gv.N = N; gv.uniform = 0; gv.delta = delta; gv.Rmax = Rmax; gv.h = 1; gv.r = r.data();
    int kept = 0;
    for (double E : energies()) {
        const long ostart = dfo_max_radius_index(&og, E, N - 1);
        if (ostart <= 0) continue;           // the oracle alone has no value here
        ++kept;
        int start = -1;
        double us = 0, us1 = 0;
        host_boundary(gv, E, &start, &us, &us1);
        CHECK(start == ostart, "N=%d E=%a: start %d, oracle %ld", N, E, start, ostart);
        CHECK(same_bits(us, dfo_far(&og, static_cast<double>(ostart), E)), "N=%d E=%a: us %a", N, E, us);
        CHECK(same_bits(us1, dfo_far(&og, static_cast<double>(ostart - 1), E)), "N=%d E=%a: us1 %a", N, E, us1);
        // the dispatching entry is the same function on this grid
        int s2 = -1;
        double a = 0, b = 0, uz = -7;
        host_boundary_of(gv, E, 2, true, &s2, &a, &b, &uz);
        CHECK(s2 == start && same_bits(a, us) && same_bits(b, us1) && uz == -7, "N=%d E=%a: host_boundary_of differs", N, E);
    }
    CHECK(kept >= 150, "N=%d: %d energies kept", N, kept);
    printf("boundary log N=%d: %d energies\n", N, kept);
}

static void boundary_uniform(int N, double Rmax)
{
    dfo_ugrid ug;
    ug.N = N; ug.Rmax = Rmax; ug.h = Rmax / (N - 1);
    GridView gv;
    gv.N = N; gv.uniform = 1; gv.delta = 0; gv.Rmax = Rmax; gv.h = ug.h; gv.r = nullptr;
    const std::vector<double> V(N, 0.0);
    int kept = 0;
    for (double E : energies()) {
        long ostart = -1;
        dfo_ucount_nodes(&ug, V.data(), 0, E, 0, &ostart);
        if (ostart <= 0) continue;
        ++kept;
        for (int for_match = 0; for_match < 2; ++for_match) {
            int start = -1;
            double us = 0, us1 = 0, uz = 0;
            host_boundary_uniform(gv, E, 1, for_match != 0, &start, &us, &us1, &uz);
            CHECK(start == ostart, "uniform E=%a for_match=%d: start %d, oracle %ld", E, for_match, start, ostart);
        }
    }
    CHECK(kept >= 150, "uniform: %d energies kept", kept);
    printf("boundary uniform N=%d: %d energies\n", N, kept);
}

// ---- grouping ---------------------------------------------------------------------------------------------------------------------
static void grouping_case(int ntrials, int nV, bool with_vidx, Rng& rng)
{
    std::vector<int> l(ntrials), vidx(ntrials);
    for (int t = 0; t < ntrials; ++t) { l[t] = rng.below(4); vidx[t] = rng.below(nV); }
    const int* vp = with_vidx ? vidx.data() : nullptr;
    auto key = [&](int t) { return (vp ? vp[t] : 0) * 4 + l[t]; };
    Grouping G;
    CHECK(make_grouping(ntrials, vp, l.data(), nV, G) == DFTA_OK, "ntrials=%d", ntrials);
    // order: a permutation, sorted by key, stable within a key
    std::vector<int> seen(ntrials, 0);
    CHECK((int)G.order.size() == ntrials, "order size");
    for (int t : G.order) { CHECK(t >= 0 && t < ntrials && !seen[t], "order repeats %d", t); if (t >= 0 && t < ntrials) seen[t] = 1; }
    for (int s = 1; s < ntrials; ++s) {
        CHECK(key(G.order[s - 1]) <= key(G.order[s]), "not sorted at %d", s);
        if (key(G.order[s - 1]) == key(G.order[s])) CHECK(G.order[s - 1] < G.order[s], "not stable at %d", s);
    }
    // blocks: 1..64 trials of one slot, tiling [0, ntrials) without gaps; trial_slot agrees; no more blocks than trials
    const size_t nb = G.blk_slot.size();
    CHECK(nb == G.blk_first.size() && nb == G.blk_cnt.size() && (int)nb <= ntrials && (int)G.trial_slot.size() == ntrials, "sizes");
    CHECK(G.slot_v.size() == G.slot_l.size(), "slot sizes");
    int next = 0;
    for (size_t b = 0; b < nb; ++b) {
        CHECK(G.blk_first[b] == next, "block %zu starts at %d, expected %d", b, G.blk_first[b], next);
        CHECK(G.blk_cnt[b] >= 1 && G.blk_cnt[b] <= 64, "block %zu has %d trials", b, G.blk_cnt[b]);
        const int slot = G.blk_slot[b];
        CHECK(slot >= 0 && slot < (int)G.slot_v.size(), "block %zu slot %d", b, slot);
        for (int s = G.blk_first[b]; s < G.blk_first[b] + G.blk_cnt[b] && s < ntrials; ++s) {
            CHECK(G.trial_slot[s] == slot, "trial %d: slot %d, its block's %d", s, G.trial_slot[s], slot);
            CHECK(G.slot_v[slot] * 4 + G.slot_l[slot] == key(G.order[s]), "trial %d is not of its block's slot", s);
        }
        next += G.blk_cnt[b];
    }
    CHECK(next == ntrials, "blocks cover %d of %d", next, ntrials);
    // out-of-range l or vidx
    for (int bad : {-1, 4}) {
        std::vector<int> l2 = l;
        l2[rng.below(ntrials)] = bad;
        Grouping G2;
        CHECK(make_grouping(ntrials, vp, l2.data(), nV, G2) == DFTA_ERR_INVALID, "l=%d accepted", bad);
    }
    if (with_vidx)
        for (int bad : {-1, nV}) {
            std::vector<int> v2 = vidx;
            v2[rng.below(ntrials)] = bad;
            Grouping G2;
            CHECK(make_grouping(ntrials, v2.data(), l.data(), nV, G2) == DFTA_ERR_INVALID, "vidx=%d accepted", bad);
        }
}

static void grouping_of_groups()
{
    const int group_off[] = {0, 1, 65, 65, 200};        // the third group is empty
    const int ngroups = 4, nV = 2;
    const int gv[] = {0, 1, 1, 0}, gl[] = {0, 3, 1, 2};
    // the loop of dfta_numerov_sweeps_dev this entry replaced
    std::vector<int> bs, bf, bc;
    for (int k = 0; k < ngroups; ++k)
        for (int s = group_off[k]; s < group_off[k + 1]; s += 64) {
            bs.push_back(k); bf.push_back(s); bc.push_back(std::min(64, group_off[k + 1] - s));
        }
    Grouping G;
    CHECK(make_grouping_of_groups(ngroups, group_off, gv, gl, nV, G) == DFTA_OK, "groups refused");
    CHECK(G.blk_slot == bs && G.blk_first == bf && G.blk_cnt == bc, "blocks differ from the replaced loop");
    CHECK(G.slot_v == std::vector<int>(gv, gv + ngroups) && G.slot_l == std::vector<int>(gl, gl + ngroups), "slots differ");
    CHECK(std::find(bs.begin(), bs.end(), 2) == bs.end() && bs.size() == 5, "the empty group has a block");
    const int bad_l[] = {0, 4, 1, 2}, bad_v[] = {0, 2, 1, 0};
    Grouping G2, G3;
    CHECK(make_grouping_of_groups(ngroups, group_off, gv, bad_l, nV, G2) == DFTA_ERR_INVALID, "l=4 accepted");
    CHECK(make_grouping_of_groups(ngroups, group_off, bad_v, gl, nV, G3) == DFTA_ERR_INVALID, "vidx=nV accepted");
}

static void grouping()
{
    Rng rng(20240229);
    int cases = 0;
    for (int ntrials : {1, 63, 64, 65, 129, 257})
        for (int nV : {1, 3})
            for (int with_vidx = 0; with_vidx < 2; ++with_vidx) { grouping_case(ntrials, nV, with_vidx != 0, rng); ++cases; }
    grouping_of_groups();
    printf("grouping: %d cases\n", cases);
}

// ---- staging layout -------------------------------------------------------------------------------------------------------------
static void staging()
{
    int cases = 0;
    for (int call = 0; call < 2; ++call)
        for (int nt = 1; nt <= 300; ++nt) {
            StageLayout L;
            CHECK(stage_layout(nt, static_cast<StageCall>(call), &L) == DFTA_OK, "nt=%d call=%d refused", nt, call);
            const size_t block[2] = {L.in_bytes, L.out_bytes};
            const size_t cap = 64 * static_cast<size_t>(std::max(nt, 64));
            CHECK(L.in_bytes <= cap && L.out_bytes <= cap && stage_scratch_bytes(nt) == cap, "nt=%d call=%d: blocks %zu / %zu of %zu", nt, call, L.in_bytes, L.out_bytes, cap);
            CHECK(L.in_bytes <= 64 * static_cast<size_t>(nt) && L.out_bytes <= 64 * static_cast<size_t>(nt), "nt=%d call=%d: more than 64 bytes per trial", nt, call);
            int used = 0;
            for (int a = 0; a < kNumStageFields; ++a) {
                const StageField& fa = kStageFields[a];
                const size_t oa = L.*(fa.off);
                if (!(fa.calls & (1u << call))) { CHECK(oa == kStageNone, "%s has an offset in call %d", fa.name, call); continue; }
                ++used;
                const size_t ea = oa + static_cast<size_t>(fa.elem_bytes) * nt;
                CHECK(oa != kStageNone && oa % fa.elem_bytes == 0, "nt=%d %s: offset %zu not aligned to %d", nt, fa.name, oa, fa.elem_bytes);
                CHECK(ea <= block[fa.out], "nt=%d %s ends at %zu, block of %zu", nt, fa.name, ea, block[fa.out]);
                for (int b = a + 1; b < kNumStageFields; ++b) {
                    const StageField& fb = kStageFields[b];
                    if (!(fb.calls & (1u << call)) || fb.out != fa.out) continue;
                    const size_t ob = L.*(fb.off), eb = ob + static_cast<size_t>(fb.elem_bytes) * nt;
                    CHECK(ea <= ob || eb <= oa, "nt=%d: %s and %s overlap", nt, fa.name, fb.name);
                }
            }
            CHECK(used == (call == kStageSweeps ? 13 : 8), "call %d uses %d arrays", call, used);
            ++cases;
        }
    StageLayout L;
    CHECK(stage_layout(0, kStageSweeps, &L) == DFTA_ERR_INVALID, "0 trials accepted");
    printf("staging: %d layouts\n", cases);
}

// ---- control-block plan ---------------------------------------------------------------------------------------------------------
// The reference: the loop of dfta_launch_levels_persist as it stood before the planner existed (numerov.hip of commit 784e19f),
// verbatim, on stand-ins for its control-block structs.
namespace ref {
constexpr int kPersistMaxBlocks = 512;
constexpr int kPersistMaxJobs = 256;
enum { kCmdPlan = 2 };
struct PersistJob { int nown, base, job; unsigned short blocks[kPersistMaxBlocks]; };
struct PersistCtl { unsigned long long pool[kPersistMaxBlocks / 64]; };
static unsigned long long persist_msg(int cmd, int level, int idx)
{
    return (static_cast<unsigned long long>(cmd) << 56) | (static_cast<unsigned long long>(level & 0xffffff) << 32) | static_cast<unsigned>(idx);
}
// hm has room for 2 * kPersistMaxBlocks words: the loop writes before it checks
static int plan(int nblocks, const int* live, int nlive, const int* share, PersistCtl* hc, unsigned long long* hm, PersistJob* hj)
{
    const int base = nblocks / nlive;
    if (base < 1) return DFTA_ERR_INVALID;
    int next = 0;
    for (int k = 0; k < nlive; ++k) {
        // (a level never starts with more than an equal share -- except where that share is ONE workgroup: the caller hands the rest out as second ones)
        const int mine = share ? (base == 1 ? std::min(std::max(share[k], 1), 2) : std::max(2, std::min(share[k], base))) : base;      // (a level never starts with more than an equal share)
        hj[k].job = live[k];
        hj[k].base = mine;
        hj[k].nown = mine;
        for (int q = 0; q < mine; ++q) hj[k].blocks[q] = static_cast<unsigned short>(next + q);
        hm[next] = persist_msg(kCmdPlan, k, 0);
        next += mine;
    }
    if (next > nblocks) return DFTA_ERR_INVALID;
    for (int q = next; q < nblocks; ++q) hc->pool[q >> 6] |= 1ull << (q & 63);
    return DFTA_OK;
}
}  // namespace ref

static void persist_case(int nblocks, int nlive, const int* share)
{
    std::vector<int> live(nlive);
    for (int k = 0; k < nlive; ++k) live[k] = 3 * k + 1;
    ref::PersistCtl hc;
    memset(&hc, 0, sizeof(hc));
    std::vector<unsigned long long> hm(2 * ref::kPersistMaxBlocks, 0ull);
    std::vector<ref::PersistJob> hj(nlive);
    memset(hj.data(), 0, sizeof(ref::PersistJob) * nlive);
    const int want = ref::plan(nblocks, live.data(), nlive, share, &hc, hm.data(), hj.data());
    PersistPlan P;
    const int got = plan_persist(nblocks, nlive, share, &P);
    CHECK(got == want, "nblocks=%d nlive=%d share=%d: status %d, the replaced loop's %d", nblocks, nlive, share != nullptr, got, want);
    if (got != DFTA_OK || want != DFTA_OK) return;
    const int equal = nblocks / nlive;
    CHECK((int)P.base.size() == nlive && (int)P.nown.size() == nlive && (int)P.first.size() == nlive && (int)P.plan_level.size() == nblocks
              && (int)P.pool.size() == (nblocks + 63) / 64, "sizes");
    std::vector<int> owner(nblocks, -1);
    int next = 0, mailboxes = 0;
    for (int k = 0; k < nlive; ++k) {
        CHECK(P.nown[k] >= 1 && P.base[k] == P.nown[k], "level %d owns %d (base %d)", k, P.nown[k], P.base[k]);
        CHECK(P.nown[k] <= (equal == 1 ? 2 : equal), "level %d owns %d of an equal share of %d", k, P.nown[k], equal);
        CHECK(P.first[k] == next, "level %d starts at %d, expected %d", k, P.first[k], next);      // disjoint and contiguous from 0
        for (int q = 0; q < P.nown[k]; ++q) {
            const int b = P.blocks[P.first[k] + q];
            CHECK(b == next + q && b < nblocks, "level %d workgroup %d is %d", k, q, b);
            if (b >= 0 && b < nblocks) owner[b] = k;
            CHECK(b == hj[k].blocks[q], "level %d workgroup %d: %d, the replaced loop's %d", k, q, b, hj[k].blocks[q]);
        }
        CHECK(P.base[k] == hj[k].base && P.nown[k] == hj[k].nown, "level %d: base/nown differ from the replaced loop", k);
        CHECK(P.plan_level[P.first[k]] == k, "level %d has no plan mailbox on its first workgroup", k);
        next += P.nown[k];
    }
    CHECK((int)P.blocks.size() == next, "blocks size");
    for (int b = 0; b < nblocks; ++b) {
        const bool pooled = (P.pool[b >> 6] >> (b & 63)) & 1ull;
        CHECK(pooled == (owner[b] < 0), "workgroup %d: pooled %d, owner %d", b, pooled, owner[b]);
        mailboxes += P.plan_level[b] >= 0;
        const unsigned long long msg = P.plan_level[b] >= 0 ? ref::persist_msg(ref::kCmdPlan, P.plan_level[b], 0) : 0ull;
        CHECK(msg == hm[b], "mailbox %d differs from the replaced loop", b);
    }
    CHECK(mailboxes == nlive, "%d plan mailboxes for %d levels", mailboxes, nlive);
    for (size_t w = 0; w < sizeof(hc.pool) / sizeof(hc.pool[0]); ++w)
        CHECK((w < P.pool.size() ? P.pool[w] : 0ull) == hc.pool[w], "pool word %zu differs from the replaced loop", w);
}

static void persist()
{
    Rng rng(777);
    int cases = 0;
    for (int nblocks : {2, 37, 64, 256})
        for (int nlive = 1; nlive <= nblocks; ++nlive) {
            persist_case(nblocks, nlive, nullptr);
            // shares as the level solver makes them (the equal share, half of it, second workgroups) and beyond (0, more than equal)
            std::vector<int> share(nlive);
            const int equal = nblocks / nlive;
            for (int k = 0; k < nlive; ++k) share[k] = rng.below(equal + 3);
            persist_case(nblocks, nlive, share.data());
            cases += 2;
        }
    PersistPlan P;
    CHECK(plan_persist(4, 5, nullptr, &P) == DFTA_ERR_INVALID && plan_persist(4, 0, nullptr, &P) == DFTA_ERR_INVALID, "less than a workgroup per level accepted");
    const int two[] = {2, 2, 2};
    CHECK(plan_persist(4, 3, two, &P) == DFTA_ERR_INVALID, "more workgroups than the machine has accepted");
    printf("persist: %d plans\n", cases);
}

int main(int argc, char** argv)
{
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "boundary") {
        boundary_log(4097, 2e-3, 25.);
        boundary_log(16385, 5e-4, 25.);
        boundary_uniform(4097, 25.);
    } else if (mode == "grouping") grouping();
    else if (mode == "staging") staging();
    else if (mode == "persist") persist();
    else { printf("usage: numerov_host_main boundary | grouping | staging | persist\n"); return 2; }
    printf("%d violations\n", g_violations);
    return g_violations ? 1 : 0;
}
