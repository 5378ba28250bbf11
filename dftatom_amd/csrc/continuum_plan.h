// continuum_plan.h -- the host side of the outward sweeps (continuum.hip): what a call accepts, how its trials are grouped into waves,
// which partner-count instance of the kernel runs and how the rows are chunked.  Host-only and pure: no HIP call, no environment.
// include/dftatom_hip.h has the arithmetic; DESIGN.md 4.14 the shape.
#pragma once

#include <cstddef>
#include <vector>

namespace dfta_continuum_plan {

constexpr int kLmax = 4;                 // l of a trial: the range of sph_bessel
constexpr int kWave = 64;                // trials of a wave: one lane each, one (potential, l, partner list) per wave
constexpr int kTile = 256;               // nodes of a staged tile = nodes of a block of the partner sums
constexpr int kMaxPartners = 16;         // partners of a list
constexpr int kMaxPower = 8;             // r^p in the partner sums
constexpr size_t kRowBudgetBytes = size_t(256) << 20;     // device memory of a chunk's rows
constexpr int kMaxChunkBlocks = 1023;    // ... and its waves: the scaling launch has one grid row per trial (65 535 at most)

struct Call {                            // the arguments of dfta_continuum that the planner reads (host pointers)
    int norm_mode, N, nV, ntrials;
    const int *vidx, *l;
    const double* E;
    const int* m;
    int npartner_rows, power, nlists;
    const int *list_off, *list_rows, *trial_list;
};

// null, or what is wrong with the call: a mode outside {FREE, WKB}, N < 5, a potential index outside 0 .. nV-1, an l outside 0 .. 4, a
// non-finite E, an m outside 3 .. N-2, a power outside 0 .. 8, offsets that do not ascend from 0, more than 16 partners in a list, a
// partner row outside 0 .. npartner_rows-1, a trial's list outside -1 .. nlists-1.  vidx, trial_list may be null (potential 0, no list);
// l, E, m are non-null where ntrials > 0.
const char* check(const Call& c);

struct Block {                           // one wave: cnt <= 64 trials of one group at the padded positions first .. first + cnt - 1
    int v, l, list;                      // list: -1 none
    int first, cnt;
};

struct Plan {
    std::vector<Block> blocks;
    std::vector<int> order;              // padded position (64 per block) -> trial of the call, -1: padding
    int instance = 0;                    // partner accumulators of the kernel: 0, 4, 8 or 16 -- the least that holds the longest list in use
    int blocks_per_chunk = 0;            // rows requested: waves whose rows (64 N doubles each) fit kRowBudgetBytes, at least 1
};

// groups in the order of their first trial, a group's trials in the order of the call; a trial's results do not depend on any of it
Plan plan(const Call& c, bool want_rows);

// the instance for a list of n partners (0 .. 16)
int instance_for(int n);

}  // namespace dfta_continuum_plan
