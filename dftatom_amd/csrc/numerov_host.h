// numerov_host.h -- the pure host logic of the Numerov layer: grouping of trials into 64-trial blocks, the boundary values as the
// reference's libm evaluates them, the staging layout of the resident potential's calls and the control-block plan of the device-side
// level search.  Plain C++17: no HIP header, no HIP call, no environment -- numerov_api.cpp and numerov.hip pass in numbers,
// tests/test_numerov_host.py (oracle/numerov_host_main.cpp) does the same without a GPU.
// Compiled with -ffp-contract=off wherever it is built: the boundary values must equal the reference's bit for bit.
#pragma once

#include <cstddef>
#include <vector>

#include "../../include/dftatom_hip.h"      // DFTA_OK / DFTA_ERR_INVALID (plain C)

namespace dfta_nh {

// ---- trials -> (table slot, 64-trial blocks) ------------------------------------------------------------------------------------
struct Grouping {
    std::vector<int> order;       // sorted trial -> original trial
    std::vector<int> slot_v, slot_l;
    std::vector<int> blk_slot, blk_first, blk_cnt;
    std::vector<int> trial_slot;  // per sorted trial
};
// group trials by (vidx, l) so every wave shares its per-point inputs; vidx null: potential 0.  DFTA_ERR_INVALID: a vidx outside
// [0, nV) or an l outside 0..3
int make_grouping(int ntrials, const int* vidx, const int* l, int nV, Grouping& G);
// the caller's trials are grouped already: group k = trials [group_off[k], group_off[k + 1]) of slot k (an empty group keeps its slot
// and gets no block); `order` and `trial_slot` stay empty -- nothing is sorted
int make_grouping_of_groups(int ngroups, const int* group_off, const int* group_vidx, const int* group_l, int nV, Grouping& G);

// ---- boundary values (GetMaxRadiusIndex / GetBoundaryValueFar, Numerov.h:32-41,103-136,274-296) ----------------------------------
struct GridView {
    int N, uniform;
    double delta, Rmax, h;
    const double* r;              // N radii (logarithmic grid)
};
void host_boundary(const GridView& g, double E, int* start, double* us, double* us1);
// for_match: the match solve re-derives its step from the truncated step count; uz (may be null): GetBoundaryValueZero(h', l)
void host_boundary_uniform(const GridView& g, double E, unsigned l, bool for_match, int* start, double* us, double* us1, double* uz);
// whichever of the two the grid asks for (logarithmic grid: l, for_match unused, *uz untouched)
inline void host_boundary_of(const GridView& g, double E, int l, bool for_match, int* start, double* us, double* us1, double* uz)
{
    if (g.uniform) host_boundary_uniform(g, E, static_cast<unsigned>(l), for_match, start, us, us1, uz);
    else host_boundary(g, E, start, us, us1);
}

// ---- staging blocks of dfta_potential_sweeps / _match: one block in, one out, every array ntrials long ----------------------------
// The scratch holds kStageBytesPerTrial bytes per trial either way (at least 64 trials), so the arrays of a block must add up to no more
// than that per trial (checked at compile time, numerov_host.cpp); doubles come first, so everything is aligned for every ntrials.
constexpr size_t kStageBytesPerTrial = 64;
constexpr size_t kStageNone = ~static_cast<size_t>(0);
enum StageCall { kStageSweeps = 0, kStageMatch = 1 };
struct StageLayout {              // byte offsets into the block (kStageNone: not part of this call)
    // in: both calls
    size_t E, us, us1, start;
    // in: sweeps (blk_* hold one entry per block, blocks <= trials; the scan sweeps read blk_slot as the trials' slots)
    size_t limit, blk_slot, blk_first, blk_cnt;
    // in: match
    size_t uz, l, trial_slot;
    // out: sweeps / match
    size_t u0, count, trip, start_out, bad, match_point;
    size_t in_bytes, out_bytes;
};
struct StageField {
    const char* name;
    size_t StageLayout::*off;
    int elem_bytes;               // 8: double, 4: int
    int out;                      // 0: in-block, 1: out-block
    unsigned calls;               // bit kStageSweeps / kStageMatch
};
extern const StageField kStageFields[];
extern const int kNumStageFields;
size_t stage_scratch_bytes(int ntrials);      // of each of the two blocks
int stage_layout(int ntrials, StageCall call, StageLayout* L);
template <typename T> inline T* stage_ptr(void* block, size_t off) { return reinterpret_cast<T*>(static_cast<char*>(block) + off); }

// ---- control block of the device-side level search (persist.inc) -----------------------------------------------------------------
// Level k owns the workgroups blocks[first[k] .. first[k] + nown[k]): never more than an equal share base = nblocks / nlive -- except
// where that share is ONE workgroup, where `share` may hand out second ones; the first workgroup of a level finds the command "plan
// the level's first round" in its mailbox, and what is left over forms the pool.
struct PersistPlan {
    std::vector<int> base, nown, first;        // per level
    std::vector<unsigned short> blocks;         // the levels' workgroups, level after level
    std::vector<int> plan_level;                // per workgroup: the level whose first round it plans, or -1 (empty mailbox)
    std::vector<unsigned long long> pool;       // (nblocks + 63) / 64 words: the workgroups that belong to nobody
};
// share: workgroups wanted per level (nlive), or null: the equal share.  DFTA_ERR_INVALID: no level, less than one workgroup per
// level, or more workgroups handed out than there are
int plan_persist(int nblocks, int nlive, const int* share, PersistPlan* P);

}  // namespace dfta_nh
