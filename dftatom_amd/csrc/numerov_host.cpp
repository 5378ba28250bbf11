// numerov_host.cpp -- see numerov_host.h.  Host-only and pure; built with -ffp-contract=off (the boundary values).
#include "numerov_host.h"

#include <algorithm>
#include <cmath>
#include <numeric>

namespace dfta_nh {

namespace {
// the sorted trials [p, q) belong to table slot `slot`: blocks of up to 64
void add_blocks(Grouping& G, int slot, int p, int q)
{
    for (int s = p; s < q; s += 64) {
        G.blk_slot.push_back(slot);
        G.blk_first.push_back(s);
        G.blk_cnt.push_back(std::min(64, q - s));
    }
}
}  // namespace

int make_grouping(int ntrials, const int* vidx, const int* l, int nV, Grouping& G)
{
    G.order.resize(ntrials);
    std::iota(G.order.begin(), G.order.end(), 0);
    auto key = [&](int t) { return (vidx ? vidx[t] : 0) * 4 + l[t]; };
    for (int t = 0; t < ntrials; ++t) {
        const int v = vidx ? vidx[t] : 0;
        if (v < 0 || v >= nV || l[t] < 0 || l[t] > 3) return DFTA_ERR_INVALID;
    }
    std::stable_sort(G.order.begin(), G.order.end(), [&](int a, int b) { return key(a) < key(b); });
    G.trial_slot.resize(ntrials);
    int p = 0;
    while (p < ntrials) {
        const int k = key(G.order[p]);
        int q = p;
        while (q < ntrials && key(G.order[q]) == k) ++q;
        const int slot = static_cast<int>(G.slot_v.size());
        G.slot_v.push_back(k / 4);
        G.slot_l.push_back(k % 4);
        add_blocks(G, slot, p, q);
        for (int s = p; s < q; ++s) G.trial_slot[s] = slot;
        p = q;
    }
    return DFTA_OK;
}

int make_grouping_of_groups(int ngroups, const int* group_off, const int* group_vidx, const int* group_l, int nV, Grouping& G)
{
    G.slot_v.assign(group_vidx, group_vidx + ngroups);
    G.slot_l.assign(group_l, group_l + ngroups);
    for (int k = 0; k < ngroups; ++k) {
        if (G.slot_v[k] < 0 || G.slot_v[k] >= nV || G.slot_l[k] < 0 || G.slot_l[k] > 3) return DFTA_ERR_INVALID;
        add_blocks(G, k, group_off[k], group_off[k + 1]);
    }
    return DFTA_OK;
}

// uniform grid: cut-off and start values exactly as the reference evaluates them (libm), Numerov.h:32-41,274-296
void host_boundary_uniform(const GridView& g, double E, unsigned l, bool for_match, int* start, double* us, double* us1, double* uz)
{
    const double s = sqrt(2. * fabs(E));
    const double mr = 200. / s;
    const double sp = mr < g.Rmax ? mr : g.Rmax;
    const long steps = static_cast<long>(sp / g.h);
    const double hh = for_match ? sp / steps : g.h;
    *start = static_cast<int>(steps);
    *us = exp(-sp * s);
    *us1 = exp(-(sp - hh) * s);
    if (uz) *uz = pow(hh, static_cast<double>(l) + 1.);
}

// boundary values exactly as the reference evaluates them (libm exp)
void host_boundary(const GridView& g, double E, int* start, double* us, double* us1)
{
    const double s = sqrt(2. * fabs(E));
    auto far = [&](int i) { return exp(-g.r[i] * s - static_cast<double>(i) * g.delta * 0.5); };
    size_t maxIndex = static_cast<size_t>(g.N - 1), minIndex = 1;
    while (maxIndex - minIndex > 1) {
        const size_t mid = (maxIndex + minIndex) / 2;
        if (far(static_cast<int>(mid)) < 1E-200) maxIndex = mid; else minIndex = mid;
    }
    *start = static_cast<int>(maxIndex);
    *us = far(static_cast<int>(maxIndex));
    *us1 = far(static_cast<int>(maxIndex) - 1);
}

// ---- staging layout ------------------------------------------------------------------------------------------------------------
// The arrays of the two calls in the order they lie in their block.  (The scan sweeps' trial slots are the blk_slot array.)
constexpr unsigned kS = 1u << kStageSweeps, kM = 1u << kStageMatch;
constexpr StageField kStageFields[] = {
    {"E", &StageLayout::E, 8, 0, kS | kM},
    {"us", &StageLayout::us, 8, 0, kS | kM},
    {"us1", &StageLayout::us1, 8, 0, kS | kM},
    {"uz", &StageLayout::uz, 8, 0, kM},
    {"limit", &StageLayout::limit, 4, 0, kS},
    {"start", &StageLayout::start, 4, 0, kS | kM},
    {"blk_slot", &StageLayout::blk_slot, 4, 0, kS},
    {"blk_first", &StageLayout::blk_first, 4, 0, kS},
    {"blk_cnt", &StageLayout::blk_cnt, 4, 0, kS},
    {"l", &StageLayout::l, 4, 0, kM},
    {"trial_slot", &StageLayout::trial_slot, 4, 0, kM},
    {"u0", &StageLayout::u0, 8, 1, kS},
    {"count", &StageLayout::count, 4, 1, kS},
    {"trip", &StageLayout::trip, 4, 1, kS},
    {"start_out", &StageLayout::start_out, 4, 1, kS},
    {"bad", &StageLayout::bad, 4, 1, kS},
    {"match_point", &StageLayout::match_point, 4, 1, kM},
};
constexpr int kNumStageFieldsC = static_cast<int>(sizeof(kStageFields) / sizeof(kStageFields[0]));
const int kNumStageFields = kNumStageFieldsC;

namespace {
// every block of every call: within the per-trial budget, and no double behind an int (alignment for every ntrials)
constexpr bool stage_fields_fit()
{
    for (int call = 0; call < 2; ++call)
        for (int out = 0; out < 2; ++out) {
            size_t per_trial = 0;
            bool seen_int = false;
            for (int k = 0; k < kNumStageFieldsC; ++k) {
                const StageField& f = kStageFields[k];
                if (f.out != out || !(f.calls & (1u << call))) continue;
                if (f.elem_bytes == 8 && seen_int) return false;
                seen_int = seen_int || f.elem_bytes == 4;
                per_trial += static_cast<size_t>(f.elem_bytes);
            }
            if (per_trial > kStageBytesPerTrial) return false;
        }
    return true;
}
static_assert(stage_fields_fit(), "the staging arrays of dfta_potential_* exceed their per-trial budget or break alignment");
}  // namespace

size_t stage_scratch_bytes(int ntrials) { return static_cast<size_t>(std::max(ntrials, 64)) * kStageBytesPerTrial; }

int stage_layout(int ntrials, StageCall call, StageLayout* L)
{
    if (ntrials < 1 || (call != kStageSweeps && call != kStageMatch)) return DFTA_ERR_INVALID;
    size_t end[2] = {0, 0};
    for (int k = 0; k < kNumStageFieldsC; ++k) {
        const StageField& f = kStageFields[k];
        const bool used = (f.calls & (1u << call)) != 0;
        L->*(f.off) = used ? end[f.out] : kStageNone;
        if (used) end[f.out] += static_cast<size_t>(f.elem_bytes) * static_cast<size_t>(ntrials);
    }
    L->in_bytes = end[0];
    L->out_bytes = end[1];
    return DFTA_OK;
}

// ---- control block of the device-side search -------------------------------------------------------------------------------------
int plan_persist(int nblocks, int nlive, const int* share, PersistPlan* P)
{
    *P = PersistPlan();
    if (nlive < 1 || nblocks < 1) return DFTA_ERR_INVALID;
    const int base = nblocks / nlive;
    if (base < 1) return DFTA_ERR_INVALID;
    P->plan_level.assign(static_cast<size_t>(nblocks), -1);
    P->pool.assign(static_cast<size_t>(nblocks + 63) / 64, 0ull);
    int next = 0;
    for (int k = 0; k < nlive; ++k) {
        // (a level never starts with more than an equal share -- except where that share is ONE workgroup: the caller hands the rest out as second ones)
        const int mine = share ? (base == 1 ? std::min(std::max(share[k], 1), 2) : std::max(2, std::min(share[k], base))) : base;
        P->base.push_back(mine);
        P->nown.push_back(mine);
        P->first.push_back(next);
        if (next + mine > nblocks) return DFTA_ERR_INVALID;      // (checked here: plan_level and blocks stay inside the machine)
        for (int q = 0; q < mine; ++q) P->blocks.push_back(static_cast<unsigned short>(next + q));
        P->plan_level[static_cast<size_t>(next)] = k;
        next += mine;
    }
    for (int q = next; q < nblocks; ++q) P->pool[static_cast<size_t>(q >> 6)] |= 1ull << (q & 63);
    return DFTA_OK;
}

}  // namespace dfta_nh
