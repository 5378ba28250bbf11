// kb_plan.h -- the host side of the Kleinman-Bylander solves (kb.hip): what a call accepts, the last non-zero node of every projector,
// how the trials are grouped into waves and the rows chunked, and the bound-state search on the sign of u~_m(E) as a loop over a
// caller-given evaluation (kb.hip passes the launch of the sweep).  Host-only and pure: no HIP call, no environment.
// include/dftatom_hip.h has the arithmetic and the search's formulas; DESIGN.md 4.16 the shape.
#pragma once

#include <cstddef>
#include <functional>
#include <vector>

namespace dfta_kb_plan {

constexpr int kLmax = 4;                 // l of a channel
constexpr int kWave = 64;                // trials of a wave: one lane each, one channel per wave
constexpr int kTile = 256;               // nodes of a staged tile = nodes of a block of the projector sums
constexpr size_t kRowBudgetBytes = size_t(256) << 20;     // device memory of a chunk's rows (two raw chains per trial)
constexpr int kMaxChunkBlocks = 1023;    // ... and its waves: the combining launch has one grid row per trial (65 535 at most)
constexpr int kMaxStates = 8;            // brackets (bound states) of a channel
constexpr int kCuts = 64;                // interior energies of a bracket per round: one wave
constexpr int kMaxRounds = 32;           // of the search (a bracket closes in about 9)

struct Call {                            // the arguments of dfta_kb_sweep that the planner reads (host pointers)
    int N, nV, nch, ntrials;
    const int *vidx, *l;                 // per channel (vidx null: 0)
    const double *beta, *q1;             // nch x N; nch
    const int* chan;                     // per trial (null: 0)
    const double* E;
    const int* m;
};

// the last node of each projector row whose value is not 0.0 (a NaN is not 0.0); 0: the row is all zero
std::vector<int> last_nonzero(int nch, int N, const double* beta);

// null, or what is wrong with the call: N < 5, nV or nch < 1, a potential index outside 0 .. nV-1, an l outside 0 .. 4, a q1 that is 0
// or not finite, a channel outside 0 .. nch-1, a non-finite E, an m outside 3 .. N-2 or below the last non-zero node of the
// channel's projector (lastnz: last_nonzero of the call)
const char* check(const Call& c, const std::vector<int>& lastnz);

struct Block {                           // one wave: cnt <= 64 trials of one channel at the padded positions first .. first + cnt - 1
    int chan, first, cnt;
};

struct Plan {
    std::vector<Block> blocks;
    std::vector<int> order;              // padded position (64 per block) -> trial of the call, -1: padding
    int blocks_per_chunk = 0;            // rows requested: waves whose raw chains (2 x 64 N doubles each) fit kRowBudgetBytes, at least 1
};

// channels in the order of their first trial, a channel's trials in the order of the call; a trial's results do not depend on any of
// it.  force_chunk > 0 (DFTA_DEBUG KB_CHUNK_WAVES): that many waves per chunk
Plan plan(const Call& c, bool want_rows, int force_chunk);

// ---- the search (the header states these formulas) ----
double scan_energy(double lo, double hi, int nscan, int k);        // k = 0 .. nscan-1
double cut_energy(double a, double b, int j);                      // j = 0 .. 63
bool bracket_closed(double a, double b);                           // no double lies between a and b

struct Bracket { double a, b; bool neg_a; };

// round 0 of a channel: neighbouring finite values of opposite sign, ascending, at most kMaxStates
std::vector<Bracket> open_brackets(int nscan, const double* E, const unsigned char* finite, const unsigned char* neg);
// a further round: the 64 cuts of br and their values; br becomes the first pair of neighbours of opposite sign among a, cuts, b.  A
// non-finite value takes the sign of a; returns whether any of the 64 cuts had one (below, at or above the new bracket)
bool cut_bracket(Bracket* br, const double* E, const unsigned char* finite, const unsigned char* neg);

struct SearchChannel { int m; double lo, hi; };
struct SearchResult {
    std::vector<int> count, rounds, status;          // per channel
    std::vector<double> energies;                    // nch x kMaxStates, NaN beyond count
};
// evaluate(chan, E, m, u, status): one launch of the sweep on ntrials = chan.size() trials; returns a DFTA_ code
typedef std::function<int(const std::vector<int>& chan, const std::vector<double>& E, const std::vector<int>& m, std::vector<double>* u,
                          std::vector<int>* status)> Evaluate;
int search(const std::vector<SearchChannel>& ch, int nscan, const Evaluate& evaluate, SearchResult* out);

}  // namespace dfta_kb_plan
