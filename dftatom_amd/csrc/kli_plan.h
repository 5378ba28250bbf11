// kli_plan.h -- the host side of the batched exchange stage (kli_stage.hip): the tables of every spin channel of a batch laid end to end,
// the partition of the live channels into chunks under a budget of y rows, and the buffer sizes that partition needs.  Host-only and
// pure: no HIP call, no environment.  A channel's own tables are exchange_plan.h's (plan_channel), entry for entry.
#pragma once

#include <vector>

#include "exchange_plan.h"

namespace dfta_kli {

constexpr int kJobInts = dfta_exchange::kJobInts;   // a row of the y-job table: x, y, k -- x, y count the orbital rows of the WHOLE batch
constexpr int kTabInts = dfta_exchange::kTabInts;   // a row of the pointwise table: a, b, k, y row -- all counted inside the channel
constexpr int kRedInts = 4;                         // a row of the reduction table: kind, a, b (inside the channel), channel
constexpr int kSolveMax = dfta_exchange::kShellsMax - 1;    // unknowns of the reduced system

// where a channel's orbitals, tables and results lie (counts of rows / entries from the start of the batch's arrays)
struct Channel {
    int u0, norb;        // orbital rows
    int job0, njobs;     // y jobs
    int first0;          // the norb + 1 entries of `first` (their values count from tab0)
    int tab0, ntab;      // pointwise entries (tab, coef)
    int red0, nred;      // reductions: vbarHF_a (a ascending), vbarS_a, then S_ab of every pair a <= b row by row
    int atom;            // the atom of an SCF channel, -1: none
};

struct Plan {
    int norb_total = 0;
    std::vector<Channel> ch;
    std::vector<int> jobs, first, tab, red;
    std::vector<double> coef;
    int nch() const { return (int)ch.size(); }
    int njobs() const { return (int)(jobs.size() / kJobInts); }
    int nred() const { return (int)(red.size() / kRedInts); }
};

// null, or what is wrong with a batch of channels: norb[c] outside 0 .. 32, an l outside 0 .. 4, an occupation that is negative or not
// finite, a channel with shells but no occupied one (it has no HOMO).  l, occ: the channels' shells end to end.
const char* check_channels(int nch, const int* norb, const int* l, const double* occ);

// the tables of the batch; atom may be null (-1 everywhere).  0, or -1: check_channels fails
int plan_channels(int nch, const int* norb, const int* l, const double* occ, const int* atom, Plan* plan);

// The tables of the self-interaction-corrected stage (SIC-KLI): per channel the y jobs are the diagonals (a, a, 0) alone, a ascending --
// y row a of a channel is the Hartree potential of one electron in shell a --, there are no pointwise entries (first0 = tab0 = ntab = 0;
// first, tab, coef stay empty), and the reductions are those of plan_channels (vbar_a, vbarS_a, S_ab: the solve reads the same layout)
// followed by EH_a (kRedSicH, a ascending) and EXC_a (kRedSicXC).  Same refusals as plan_channels.
enum { kRedSicH = 4, kRedSicXC = 5 };               // kinds of the reduction table beyond dfta_exchange's
int plan_channels_sic(int nch, const int* norb, const int* l, const double* occ, const int* atom, Plan* plan);

// y rows of N doubles that fit `mb` MiB, at least 0
long budget_rows(double mb, int N);

// The chunks of a step: consecutive channels [c0, c1) as pairs, every channel of a pair live (live null: all are), whole channels only,
// a chunk's y jobs <= max_rows unless it is one channel.  A channel that is not live ends a chunk and is in none; a live channel without
// shells may lie inside a chunk (it costs nothing).
void plan_chunks(const Plan& plan, const unsigned char* live, long max_rows, std::vector<int>* bounds);

// what any chunk plan_chunks can return under max_rows needs at the most: y rows, orbital rows (X), channels (D and vS rows)
struct Caps { long yrows, xrows, chans; };
Caps capacities(const Plan& plan, long max_rows);

}  // namespace dfta_kli
