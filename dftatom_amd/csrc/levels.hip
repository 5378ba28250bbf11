// levels.hip -- device-side eigenvalue search for a batch of (potential, n, l) levels.
//
// Replaces DFTAtom::LoopOverLevels, LocateInterval, NormalizeNonUniform and the accumulation
// newDensity += occ * Psi^2 (DFTAtom.cpp:36-56, 493-604).
//
// The reference finds each eigenvalue with three sequential bisections (node count > n: top of the band;
// node count < n: bottom of the band; sign of u(0): the eigenvalue), ~140 sweeps per level, each sweep a
// sequential O(N) recurrence.  Here every bisection is a SPECULATIVE TREE: in one round the 2^d - 1
// possible midpoints of the next d bisection steps of every level are integrated concurrently (one lane
// per trial, numerov.hip), then one thread per chain walks its tree with the reference's predicates.
// The midpoints are generated with the reference's expression (toe + boe) / 2 along the same paths, so the
// walk reproduces the reference's decision sequence; ~53 sequential sweeps per phase become ceil(53/d) rounds.
// A tree may hang at the end of a SPINE, a predicted decision path that costs one trial per decision; predictions come
// from the previous SCF step, from the sibling level (the second bisection evaluates the predicate of the sibling's
// first one), from the position of the sign change of u(0) (upper end of the band for l = 0, scouted for l > 0).
// They select which midpoints are integrated speculatively and never enter a decision (k_plan, plan_round).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "internal.h"
#include "levels.h"
#include "ordered_sum.h"

namespace {

#include "levels_device.inc"

// ---- expand: trial energies of the current round of every job, plus their far boundary values ----------------------
// qctl / qlist (may be null): the round's work queue for the balanced launch of the fused sweeps (numerov.hip:k_sweep_queue).  Every
// 64-trial block with an active trial is entered into one of kSweepQueueClasses lists by its expected length -- the cut-off index of
// its outermost trial, halved where CountNodes will stop at an inner turning point (l > 0) -- so that the launch's waves take the
// longest blocks first; blocks without an active trial are not entered at all.
__global__ __launch_bounds__(256) void k_expand(const dfta::Job* __restrict__ jobs, const int* __restrict__ wave_job, int wshift, int ntrials, const double* __restrict__ r,
                                                int N, double delta, double far_thr, double* __restrict__ E,
                                                int* __restrict__ limit, int* __restrict__ start, double* __restrict__ us,
                                                double* __restrict__ us1, int* __restrict__ wave_kind,
                                                unsigned long long* __restrict__ issued, int uniform, double Rmax, double hstep,
                                                int* __restrict__ qctl, int* __restrict__ qlist, int qcap)
{
    const int gt = blockIdx.x * blockDim.x + threadIdx.x;
    if (gt >= ntrials) return;       // ntrials is a multiple of 64: whole waves leave
    const int job = wave_job[gt >> wshift];   // one entry per 64-trial block (wshift 6) or per trial (packed rounds: wshift 0)
    bool active = false, zero_kind = true;
    int st = 0, key = 0;
    if (job < 0) {                    // slots that no job owns this round
        E[gt] = 0; limit[gt] = 0; start[gt] = 0;
    } else {
        const dfta::Job j = jobs[job];
        const TrialSpec ts = trial_spec<false>(j, jobs, gt - j.tbase);
        const double e = ts.e;
        active = ts.active;
        zero_kind = ts.zero_kind;
        E[gt] = e;
        limit[gt] = j.nodes;
        if (active && uniform) {
            // uniform grid (Numerov.h:32-35,43-56,274-296): start at min(Rmax, 200 / sqrt(2|E|)), index (long)(startPoint / h)
            const double s = sqrt(2. * fabs(e));
            const double mr = 200. / s;
            const double sp = mr < Rmax ? mr : Rmax;
            st = static_cast<int>(static_cast<long>(sp / hstep));
            us[gt] = exp(-sp * s);
            us1[gt] = exp(-(sp - hstep) * s);
        } else if (active) {
            double a, b;
            st = trial_boundary(e, r, N, delta, far_thr, a, b);
            us[gt] = a;
            us1[gt] = b;
        }
        start[gt] = st;
        key = active ? ((zero_kind || j.l == 0) ? st : st / 2) : 0;
    }
    // the block's kind: its first trial's (a block of the static / latency layouts has one owner, a packed block one (slot, kind) group)
    const int kind0 = __shfl(zero_kind ? 1 : 0, 0);
    if ((gt & 63) == 0) wave_kind[gt >> 6] = kind0 ? DFTA_SWEEP_ZERO : DFTA_SWEEP_COUNT;
    const unsigned long long m = __ballot(active);
    if (issued && (threadIdx.x & 63) == 0 && m) atomicAdd(issued, (unsigned long long)__popcll(m));
    if (qctl) {
        for (int off = 32; off > 0; off >>= 1) key = max(key, __shfl_xor(key, off));
        if ((gt & 63) == 0 && m) {
            int cls = kSweepQueueClasses - 1 - static_cast<int>((static_cast<long long>(key) * kSweepQueueClasses) / N);
            cls = cls < 0 ? 0 : (cls >= kSweepQueueClasses ? kSweepQueueClasses - 1 : cls);
            const int pos = atomicAdd(&qctl[cls], 1);
            qlist[(size_t)cls * qcap + pos] = gt >> 6;
        }
    }
}

__global__ __launch_bounds__(64) void k_scout(dfta::Job* __restrict__ jobs, const double* __restrict__ E,
                                              const int* __restrict__ start, const double* __restrict__ u0)
{
    scout_job(jobs + blockIdx.x, threadIdx.x, E, start, u0);
}

__global__ void k_walk(dfta::Job* __restrict__ jobs, const int* __restrict__ chain_off, int nchains,
                       const int* __restrict__ count, const double* __restrict__ u0, const double* __restrict__ phi,
                       const int* __restrict__ istop, const int* __restrict__ trip, const double2* __restrict__ tab, int N,
                       int* __restrict__ ndone)
{
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= nchains) return;
    int done = 0;
    for (int k = chain_off[c]; k < chain_off[c + 1]; ++k) {
        dfta::Job j = jobs[k];
        if (j.phase == PH_DONE) { ++done; continue; }
        if (j.phase == PH_WAIT) {
            // DFTAtom.cpp:541: BottomEnergy = level.E - 3 handed to the next level of the chain
            const double bot = (k == chain_off[c]) ? j.bottom0 : jobs[k - 1].E - 3;
            j.bottom0 = bot;
            j.toe = 50;                                             // DFTAtom.cpp:499
            j.boe = bot;
            j.phase = PH_TOP;
            j.phase_done = 0;
            j.miss = 0;
            j.capz = 0;
            j.se_state = 0;
            j.se_stop = 0;
            j.se_tok = 0;
            j.sc_is[0] = j.sc_is[1] = j.sc_is[2] = -1;
            j.sc_ok = 0;
            jobs[k] = j;
            break;                                                  // its trials are generated next round
        }
        walk_job(j, count, u0, phi, istop, trip, tab + (size_t)j.slot * N);
        jobs[k] = j;
        if (j.phase == PH_DONE) { ++done; continue; }
        break;
    }
    if (done) atomicAdd(ndone, done);
}

// spines of the next round, after every walk of this one (a job reads its sibling's first-bisection result)
__global__ void k_plan(dfta::Job* __restrict__ jobs, int njobs, int nopredict, int tpj_override)
{
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= njobs) return;
    dfta::Job j = jobs[k];
    if (j.phase != PH_TOP && j.phase != PH_BOTTOM && j.phase != PH_ZERO) return;
    const int tpj = tpj_override > 0 ? tpj_override : j.tcap;   // packed rounds: "with room to spare", k_pack cuts it to size
    plan_round(j, jobs, tpj);
    if (nopredict) { j.spine = 0; j.capz = tpj; j.use_sp = 0; j.sp_len = 0; j.sp_bits = 0; }     // plain trees only (DFTA_LEVELS_NOPREDICT)
    jobs[k].spine = j.spine;
    jobs[k].capz = j.capz;
    jobs[k].use_sp = j.use_sp;
    jobs[k].sp_bits = j.sp_bits;
    jobs[k].sp_len = j.sp_len;
}

// ---- packed rounds: many jobs (batches of atoms) -- the trials of a round laid out job after job, no 64-slot block per job ----
// A 64-trial block of the sweep kernels has ONE table slot (potential, l) and ONE kind (CountNodes / SolutionInZero); its
// lanes are independent otherwise.  With a block per job (the static layout) a job cannot have fewer than 64 trials, and the
// work of a step is the number of blocks: a depth-5 tree behind a 10-decision spine integrates 42 trials for 15 decisions
// and pays for 64.  Here the jobs of a round are grouped by (slot, kind) -- 1s..6s of one atom share a table, 2p..6p the
// next -- and laid out back to back inside their group, a job taking exactly probe + spine + 2^d - 1 trials; only the end
// of a group is padded to a block.  The depth d is the same for every job of a round and is chosen from what is still
// searching: the largest one whose trials fit the launch that fills the machine (latency regime: ~1.5 passes of one block
// per compute unit, the pipelined kernel; else two waves per SIMD of the fused one), never below dmin.  As jobs finish, the
// rest get deeper trees.  Which midpoints are integrated changes; the decisions do not (the walk follows the reference's
// predicates on whatever nodes it finds).
constexpr int kPackThreads = 1024;
constexpr int kMaxRounds = 4096;       // host rounds of one solve
constexpr int kPackSpineCap = 40;      // decisions of one round's spine (the tree behind it adds d more)


__global__ __launch_bounds__(kPackThreads) void k_pack(dfta::Job* __restrict__ jobs, int njobs, int nslots, const int* __restrict__ slot_off,
                                                       const int* __restrict__ slot_jobs, int lanes_small, int dsmall, int lanes_large, int dmin, int dmax,
                                                       int* __restrict__ gsz, int* __restrict__ goff, int* __restrict__ lane_job,
                                                       int* __restrict__ wave_slot, int* __restrict__ out)
{
    __shared__ long long s_sum[kPackThreads / 64];
    __shared__ int s_cnt[kPackThreads / 64];
    __shared__ int s_scan[kPackThreads];
    __shared__ int s_d;
    const int tid = threadIdx.x;
    // (1) what is still searching, and how long its spines are
    long long ss = 0;
    int a = 0;
    for (int k = tid; k < njobs; k += kPackThreads) {
        if (!job_searching(jobs[k].phase)) continue;
        int S = jobs[k].spine;
        if (S > kPackSpineCap) { S = kPackSpineCap; jobs[k].spine = S; }
        ss += S;
        ++a;
    }
    for (int off = 32; off > 0; off >>= 1) { ss += __shfl_xor(ss, off); a += __shfl_xor(a, off); }
    if ((tid & 63) == 0) { s_sum[tid >> 6] = ss; s_cnt[tid >> 6] = a; }
    __syncthreads();
    if (tid == 0) {
        long long S = 0;
        long long A = 0;
        for (int w = 0; w < kPackThreads / 64; ++w) { S += s_sum[w]; A += s_cnt[w]; }
        auto fit = [&](long long T) { int d = dmin; while (d < dmax && S + (A << (d + 1)) <= T) ++d; return d; };
        int d = fit(lanes_small);
        if (d < dsmall) d = fit(lanes_large);
        s_d = d;
        out[1] = d;
        out[2] = (int)A;
    }
    __syncthreads();
    const int d = s_d;
    // (2) size of every (slot, kind) group, padded to whole blocks
    for (int s = tid; s < nslots; s += kPackThreads) {
        int nc = 0, nz = 0;
        for (int q = slot_off[s]; q < slot_off[s + 1]; ++q) {
            const int k = slot_jobs[q];
            const int ph = jobs[k].phase;
            if (!job_searching(ph)) continue;
            const int t = jobs[k].spine + (1 << d);
            if (ph == PH_ZERO) nz += t; else nc += t;
        }
        gsz[2 * s] = (nc + 63) & ~63;
        gsz[2 * s + 1] = (nz + 63) & ~63;
    }
    __syncthreads();
    // (3) exclusive scan of the group sizes: consecutive chunks per thread, scan of the chunk sums in LDS
    const int n2 = 2 * nslots;
    const int chunk = (n2 + kPackThreads - 1) / kPackThreads;
    const int c0 = min(tid * chunk, n2), c1 = min(c0 + chunk, n2);
    int local = 0;
    for (int i = c0; i < c1; ++i) local += gsz[i];
    s_scan[tid] = local;
    __syncthreads();
    for (int off = 1; off < kPackThreads; off <<= 1) {
        const int v = tid >= off ? s_scan[tid - off] : 0;
        __syncthreads();
        s_scan[tid] += v;
        __syncthreads();
    }
    int run = s_scan[tid] - local;
    for (int i = c0; i < c1; ++i) { goff[i] = run; run += gsz[i]; }
    if (tid == kPackThreads - 1) out[0] = s_scan[tid];       // trials of the round (a multiple of 64)
    __syncthreads();
    // (4) the jobs of a group back to back.  What the padding of the group's last block leaves free goes to deeper trees, a
    // level at a time, to the job with the shallowest tree (among equals: the one furthest behind -- earlier bisection, wider
    // interval); only what is left after that belongs to nobody.
    for (int s = tid; s < nslots; s += kPackThreads) {
        const int q0 = slot_off[s], q1 = slot_off[s + 1];
        int used[2] = {0, 0};
        for (int q = q0; q < q1; ++q) {
            const int k = slot_jobs[q];
            const int ph = jobs[k].phase;
            if (!job_searching(ph)) { jobs[k].tbase = 0; jobs[k].tcap = 0; continue; }
            jobs[k].tcap = d;                                      // depth of the job's tree, for now
            used[ph == PH_ZERO] += jobs[k].spine + (1 << d);
        }
        for (int kind = 0; kind < 2; ++kind) {
            int room = gsz[2 * s + kind] - used[kind];
            while (room >= (1 << d)) {
                int best = -1, bd = 1 << 30, bph = 0;
                double bw = 0;
                for (int q = q0; q < q1; ++q) {
                    const int k = slot_jobs[q];
                    const int ph = jobs[k].phase;
                    if (!job_searching(ph) || (ph == PH_ZERO) != (kind == 1)) continue;
                    const int dj = jobs[k].tcap;
                    const double w = jobs[k].toe - jobs[k].boe;
                    if (dj < bd || (dj == bd && (ph < bph || (ph == bph && w > bw)))) { best = k; bd = dj; bph = ph; bw = w; }
                }
                if (best < 0 || (1 << bd) > room || bd >= dmax) break;
                room -= 1 << bd;
                jobs[best].tcap = bd + 1;
            }
        }
        int c = goff[2 * s], z = goff[2 * s + 1];
        const int cend = c + gsz[2 * s], zend = z + gsz[2 * s + 1];
        for (int b = c >> 6; b < (cend >> 6); ++b) wave_slot[b] = s;
        for (int b = z >> 6; b < (zend >> 6); ++b) wave_slot[b] = s;
        for (int q = q0; q < q1; ++q) {
            const int k = slot_jobs[q];
            const int ph = jobs[k].phase;
            if (!job_searching(ph)) continue;
            const int t = jobs[k].spine + (1 << jobs[k].tcap);
            jobs[k].tcap = t;
            jobs[k].capz = t;
            if (ph == PH_ZERO) { jobs[k].tbase = z; z += t; } else { jobs[k].tbase = c; c += t; }
        }
        for (; c < cend; ++c) lane_job[c] = -1;
        for (; z < zend; ++z) lane_job[z] = -1;
    }
}

// owner of every trial slot of a packed round (one wave per job)
__global__ __launch_bounds__(256) void k_pack_lanes(const dfta::Job* __restrict__ jobs, int njobs, int* __restrict__ lane_job)
{
    const int k = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (k >= njobs) return;
    if (!job_searching(jobs[k].phase)) return;
    const int base = jobs[k].tbase, cap = jobs[k].tcap;
    for (int i = lane; i < cap; i += 64) lane_job[base + i] = k;
}

// ---- latency mode: the trial slots of a round are re-allotted among the jobs that are still searching -----------------
// With a handful of jobs (one atom) a round is one pass of at most `budget / 64` blocks over the compute units whatever
// the blocks do, and the number of rounds is set by the slowest job: the levels whose last decisions cannot be predicted
// (the count / the sign of u(0) are not monotonic in E below ~1e-11 |E|: 7 decisions for an outer level, 14-16 for 2s / 1s)
// need one tree of that depth or several rounds of shallower ones.  So each round every active job asks for what it can
// use -- probe + spine + a tree as deep as the decisions that remain after the spine (6 .. kMaxTreeDepth), twice that when
// it also scouts -- and the requests are cut back, deepest tree first, until they fit.  Which midpoints are integrated
// changes, the decisions taken do not (the walk follows the reference's predicates on whatever nodes it finds).
__global__ __launch_bounds__(64) void k_allot(dfta::Job* __restrict__ jobs, int njobs, int budget, int nopredict, int* __restrict__ wave_job,
                                              int* __restrict__ wave_slot, const int* __restrict__ live)
{
    // `live` (may be null): the njobs <= 64 jobs of a larger list that are still to be solved (the rest are frozen: finished atoms
    // of an SCF batch); lane k then stands for job live[k]
    __shared__ int s_S[64], s_base[64], s_cap[64], s_id[64];
    const int k = threadIdx.x;            // njobs <= 64 in this mode
    const int kk = (live && k < njobs) ? live[k] : k;
    s_id[k] = kk;
    bool act = false;
    int S = 0, r = 0, sc = 0, rem = 0, left = 0;
    if (k < njobs) {
        dfta::Job j = jobs[kk];
        act = (j.phase == PH_TOP || j.phase == PH_BOTTOM || j.phase == PH_ZERO);
        if (act) {
            plan_round(j, jobs, 1 << 14);                      // what would it do with room to spare?
            if (nopredict) { j.spine = 0; j.capz = 1 << 14; }
            S = j.spine;
            sc = j.capz < (1 << 14);
            // a tree that ends the phase if ten levels can (1024 trials: what a job's share of a pass affords), else equal shares
            // of the rounds it takes anyway; deeper phase-ending trees are handed out below, from what the others leave
            left = decisions_left(j) - S;
            if (left <= 10) r = left < 6 ? 6 : left;
            else { const int nr = (left + 9) / 10; r = (left + nr - 1) / nr; if (r < 6) r = 6; }
            // rounds this job still has in front of it (a level's three bisections take about 3 + 2 + 2 rounds): the slots go to
            // the jobs that are furthest behind, because the round count of a step is theirs
            rem = (left + 9) / 10 + (j.phase == PH_TOP ? 4 : (j.phase == PH_BOTTOM ? 2 : 0));
        }
    }
    // One lane per job from here on (the kernel is one wave): selections are wave-wide maxima of a key, sums are wave sums.
    auto wave_max = [](int v) { for (int off = 32; off > 0; off >>= 1) v = max(v, __shfl_xor(v, off)); return v; };
    auto wave_sum = [](int v) { for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off); return v; };
    auto slots_at = [&](int depth) { const int t = 1 + S + (1 << depth); const int u = (t + 127) & ~127; return sc ? 2 * u : u; };
    int tot = wave_sum(act ? slots_at(r) : 0);
    // What the modest requests leave goes, furthest-behind job first, to deeper trees that SAVE A ROUND of the phase: the
    // smallest depth with ceil(left / depth) one less than now, up to kMaxTreeDepth levels.  (Round 2 first let every job ask
    // for its phase-ending tree outright: a level with 14 undecided decisions then asked for the whole pass, was cut to 13 --
    // two rounds all the same -- and the cuts took the ninth level from a job that needed exactly nine: an extra round for a
    // single decision.  And a level with 23 decisions left got three rounds of 8 where 12 + 11 were affordable.)
    {
        bool stuck = !act;
        for (int guard = 0; guard < 256; ++guard) {
            // furthest behind first (largest rem), then the fewest decisions left, then the lowest job
            const bool cand = act && !stuck && r < left;
            const int key = cand ? (((rem & 0x3fff) << 16) | ((255 - min(left, 255)) << 8) | (63 - k)) : -1;
            const int best = wave_max(key);
            if (best < 0) break;
            const int lane_pick = 63 - (best & 0xff);
            const int nr = (left + max(r, 1) - 1) / max(r, 1);                   // rounds of this phase at the present depth
            const int target = nr > 1 ? (left + nr - 2) / (nr - 1) : left;
            const int cost = (target <= kMaxTreeDepth && target > r) ? slots_at(target) - slots_at(r) : (1 << 29);
            const int c = __shfl(cost, lane_pick);
            const bool ok = tot + c <= budget;                                   // wave-uniform
            if (k == lane_pick) { if (ok) { r = target; --rem; } else stuck = true; }
            if (ok) tot += c;
        }
    }
    // still too much: cut the job that is least behind (then the deepest tree among equals), down to 8 levels first, then to 6
    for (int floor = 8; floor >= 6 && tot > budget; floor -= 2) {
        for (int guard = 0; guard < 1024 && tot > budget; ++guard) {
            const bool cand = act && r > floor;
            const int key = cand ? ((((0x3fff - (rem & 0x3fff))) << 16) | (r << 8) | (63 - k)) : -1;
            const int best = wave_max(key);
            if (best < 0) break;
            const int lane_pick = 63 - (best & 0xff);
            const int delta = slots_at(r) - slots_at(max(r - 1, 0));
            tot -= __shfl(delta, lane_pick);
            if (k == lane_pick) --r;
        }
    }
    // slots in job order; what does not fit any more (cuts exhausted) is clamped exactly as a sequential pass would
    {
        int cap = act ? slots_at(r) : 0;
        int base = cap;                                                          // inclusive prefix sum
        for (int off = 1; off < 64; off <<= 1) { const int v = __shfl_up(base, off); if (k >= off) base += v; }
        base -= cap;
        if (tot > budget) {                                                      // rare: sequential semantics by one lane
            s_S[k] = cap;
            __syncthreads();
            if (k == 0) {
                int b = 0;
                for (int q = 0; q < njobs; ++q) {
                    int cq = s_S[q];
                    if (b + cq > budget) cq = ((budget - b) / 128) * 128;
                    s_base[q] = b;
                    s_cap[q] = cq;
                    b += cq;
                }
            }
            __syncthreads();
        } else {
            s_base[k] = base;
            s_cap[k] = cap;
            __syncthreads();
        }
    }
    // the block table of the round, by all lanes (a lone thread pays a memory round trip per entry)
    const int my_slot = k < njobs ? jobs[kk].slot : 0;
    s_S[k] = my_slot;                                          // (the spine lengths are not needed any more)
    __syncthreads();
    for (int w = k; w < (budget >> 6); w += 64) {
        int q = -1;
        for (int t = 0; t < njobs; ++t)
            if (w * 64 >= s_base[t] && w * 64 < s_base[t] + s_cap[t]) q = t;
        wave_job[w] = q >= 0 ? s_id[q] : -1;
        wave_slot[w] = q >= 0 ? s_S[q] : 0;
    }
    if (k < njobs) { jobs[kk].tbase = s_base[k]; jobs[kk].tcap = s_cap[k]; }
    if (k < njobs && act) {                                    // the plan for the slots the job really got
        dfta::Job j = jobs[kk];
        j.tbase = s_base[k];
        j.tcap = s_cap[k];
        if (j.tcap < 128) {                                    // nothing left for it this round (cannot happen while budget >= 128 njobs)
            jobs[kk].spine = 0; jobs[kk].capz = j.tcap; jobs[kk].use_sp = 0; jobs[kk].sp_bits = 0; jobs[kk].sp_len = 0;
            return;
        }
        plan_round(j, jobs, j.tcap);
        if (nopredict) { j.spine = 0; j.capz = j.tcap; j.use_sp = 0; j.sp_len = 0; j.sp_bits = 0; }
        jobs[kk].spine = j.spine;
        jobs[kk].capz = j.capz;
        jobs[kk].use_sp = j.use_sp;
        jobs[kk].sp_bits = j.sp_bits;
        jobs[kk].sp_len = j.sp_len;
    }
}

// ---- normalise (DFTAtom.cpp:36-56) ------------------------------------------------------------------------------
// one block per job; the first two waves perform the Simpson 3/8 sum in the reference's order (the other rules: the first wave)
constexpr int kNormThreads = 1024;     // the two pointwise passes are chains of memory round trips of a single block
__global__ __launch_bounds__(kNormThreads) void k_normalize(double* __restrict__ Psi, double* __restrict__ G, int N,
                                                            const double* __restrict__ eh, const double* __restrict__ cnst,
                                                            const int* __restrict__ jstart, double step, int rule)
{
    __shared__ __attribute__((aligned(16))) double lds[dfta::kTile];
    __shared__ double rtab[64];
    __shared__ double s_unorm;
    if (jstart && jstart[blockIdx.x] < 0) return;     // frozen job: its normalised Psi stands
    double* P = Psi + (size_t)blockIdx.x * N;
    double* g = G + (size_t)blockIdx.x * N;
    for (int i = threadIdx.x; i < N; i += kNormThreads) {
        const double p = P[i] * eh[i];            // Psi[i] *= exp(i * deltaGrid * 0.5)
        P[i] = p;
        double r2 = p * p;
        r2 *= cnst[i];                            // result2[i] *= Rp * deltaGrid * exp(deltaGrid * i)
        g[i] = r2;
    }
    __syncthreads();
    // Simpson38(1, .) on the logarithmic grid, Simpson38(h, .) on the uniform one (DFTAtom.cpp:27,51)
    if (rule == DFTA_INT_SIMPSON38) {
        const double integral = dfta::block_simpson38(g, N, step, lds, rtab);
        if (threadIdx.x == 0) s_unorm = 1. / sqrt(integral);
    } else if (threadIdx.x < 64) {
        const double integral = dfta::wave_integrate(rule, g, N, step, lds, rtab);
        if (threadIdx.x == 0) s_unorm = 1. / sqrt(integral);
    }
    __syncthreads();
    const double unorm = s_unorm;
    for (int i = threadIdx.x; i < N; i += kNormThreads) P[i] *= unorm;
}

// newDensity[v][i] += occ * Psi[i] * Psi[i] for i < N-1, levels of a potential in their order (DFTAtom.cpp:558-559); occ: per job,
// (double)Job::occ for an Aufbau configuration (the same product as the int operand converted), fractional ones beside it
__global__ void k_accumulate_density(const double* __restrict__ Psi, const double* __restrict__ occ,
                                     const int* __restrict__ v_off, int N, double* __restrict__ newDensity)
{
    const int v = blockIdx.y;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < N; i += gridDim.x * blockDim.x) {
        double acc = newDensity[(size_t)v * N + i];
        if (i < N - 1)
            for (int k = v_off[v]; k < v_off[v + 1]; ++k) {
                const double p = Psi[(size_t)k * N + i];
                acc += occ[k] * p * p;
            }
        newDensity[(size_t)v * N + i] = acc;
    }
}

// min_i Veff_l(i), i = 1..N-1, of every table slot (one block per slot; NaN entries are ignored)
__global__ __launch_bounds__(1024) void k_slot_min(const double2* __restrict__ tab, int N, double* __restrict__ slot_min)
{
    __shared__ double red[16];
    const double2* T = tab + (size_t)blockIdx.x * N;
    double m = INFINITY;
    for (int i = 1 + threadIdx.x; i < N; i += 1024) {
        const double v = T[i].x;
        if (v < m) m = v;
    }
    for (int off = 32; off > 0; off >>= 1) {
        const double o = __shfl_xor(m, off);
        if (o < m) m = o;
    }
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        double r = red[0];
        for (int w = 1; w < 16; ++w) r = fmin(r, red[w]);
        slot_min[blockIdx.x] = r;
    }
}

// BATCHED: every level starts un-chained from max(-Z^2-1, min Veff_l): no eigenvalue lies below the minimum of
// the effective potential, and below it the node count of l >= 1 misfires
__global__ void k_clamp_bottoms(dfta::Job* __restrict__ jobs, int njobs, const double* __restrict__ slot_min)
{
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= njobs) return;
    const double vmin = slot_min[jobs[k].slot];
    const double b = (vmin > jobs[k].bottom0) ? vmin : jobs[k].bottom0;
    jobs[k].bottom0 = b;
    jobs[k].boe = b;
}

__global__ void k_job_energies(const dfta::Job* __restrict__ jobs, int njobs, double* __restrict__ E, int* __restrict__ slot,
                               int* __restrict__ l)
{
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= njobs) return;
    E[k] = jobs[k].E;
    slot[k] = jobs[k].slot;
    l[k] = jobs[k].l;
}

__global__ void k_store_match(dfta::Job* __restrict__ jobs, int njobs, const int* __restrict__ mp, const int* __restrict__ jstart)
{
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k < njobs && !jobs[k].frozen) {
        jobs[k].matchPoint = mp[k];
        jobs[k].n_points += jstart[k];        // inward from the cut-off to the match point + outward up to it
    }
}

// Early match solves run on a SECOND stream while the next round runs on the first, whose k_walk rewrites the job records.  What the
// second stream needs of them is therefore SNAPSHOT on the first stream, in order with the round -- right after k_walk, before the
// event the second stream waits for: the eigenvalue of every job and whether its search has ended.  (Before round 4 the second stream
// read jobs[k].E and, two kernels later, jobs[k].phase: a level that finished in the NEXT round between those two reads would have
// been matched with a stale energy.  Unlikely -- a sweep outlasts three small kernels -- but not ordered.)
__global__ void k_snapshot_done(const dfta::Job* __restrict__ jobs, int njobs, double* __restrict__ snapE, int* __restrict__ snapReady)
{
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= njobs) return;
    snapE[k] = jobs[k].E;
    snapReady[k] = jobs[k].phase == PH_DONE && !jobs[k].frozen;
}
// second stream: the snapshot's finished jobs that have not been matched yet take their energy; the others keep what they had
__global__ void k_take_ready(const double* __restrict__ snapE, const int* __restrict__ snapReady, const int* __restrict__ matched, int njobs,
                             double* __restrict__ jE, int* __restrict__ take)
{
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= njobs) return;
    const int t = snapReady[k] && !matched[k];
    take[k] = t;
    if (t) jE[k] = snapE[k];
    else if (!(jE[k] == jE[k])) jE[k] = -1.;         // never written yet: any finite energy (its cut-off index is masked out below)
}
// of the jobs whose cut-off indices were just computed, keep the taken ones (the others get -1: skipped by k_match); remember the kept
// ones' cut-off index for the statistics and the final passes
__global__ void k_mask_ready(const int* __restrict__ take, int njobs, int* __restrict__ jstart, int* __restrict__ matched,
                             int* __restrict__ jstart_keep)
{
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= njobs) return;
    if (take[k]) { matched[k] = 1; jstart_keep[k] = jstart[k]; }
    else jstart[k] = -1;
}
// slot and l of every job (they never change during a run)
__global__ void k_job_slots(const dfta::Job* __restrict__ jobs, int njobs, int* __restrict__ slot, int* __restrict__ l)
{
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= njobs) return;
    slot[k] = jobs[k].slot;
    l[k] = jobs[k].l;
}
// the final pass: every job that is neither frozen nor matched already
__global__ void k_mask_rest(const dfta::Job* __restrict__ jobs, int njobs, int* __restrict__ jstart, const int* __restrict__ matched,
                            int* __restrict__ jstart_keep)
{
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= njobs) return;
    if (jobs[k].frozen) { jstart[k] = -1; jstart_keep[k] = -1; }
    else if (matched[k]) jstart[k] = -1;
    else jstart_keep[k] = jstart[k];
}

// TopEnergy of every live level as the scan search found it (scan.hip, on a copy of the records) becomes the centre of the bracket from
// which plan_round lays the first spine of the exact search's FIRST bisection -- speculation only.  Half width = `factor` (1.5) x the
// scan's asserted distance from the exact path, 6e-11 |T| + 6e-10 Ha (tests/test_gpu_scan.py), less the 1e-10 |T| that plan_round adds
// for brackets from SCF histories.  Measured (Rn, steps 5 - 24): factor 1.5 / 1 / 3 alike, 0.5 and 0.25 lose rounds to missed spines.
__global__ void k_inject_scan_top(dfta::Job* __restrict__ jobs, const dfta::Job* __restrict__ scanned, const int* __restrict__ live, int nlive,
                                  const unsigned long long* __restrict__ scan_counters, double factor, double shift)
{
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= nlive || scan_counters[3] != 0ull) return;          // a sweep the scan could not decide / a lost member: no prediction
    const int k = live[q];
    if (jobs[k].phase != PH_TOP || jobs[k].frozen) return;
    const double T = scanned[k].top * (1.0 + shift);             // (shift: tests -- a recklessly wrong prediction changes rounds, never results)
    if (!(fabs(T) < 1e300)) return;
    // (scanned.bottom: the half width the scan itself left around T -- 0 from the group search, which bisects to the end)
    const double w = factor * (6e-11 * fabs(T) + 6e-10) + scanned[k].bottom - 1e-10 * fabs(T);
    jobs[k].hist_c[0] = T;
    jobs[k].hist_w[0] = w;
    jobs[k].hist_d[0] = 0.0;
    if (jobs[k].hist_ok < 2) jobs[k].hist_ok = 2;
}

// frozen jobs are skipped by the match / normalise kernels: their cut-off index is replaced by -1
__global__ void k_mask_frozen(const dfta::Job* __restrict__ jobs, int njobs, int* __restrict__ jstart)
{
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k < njobs && jobs[k].frozen) jstart[k] = -1;
}

}  // namespace

namespace dfta {

// What one run() has decided and what its phases hand to each other: built once at the top of run(), passed to every phase.
// It OWNS every host buffer that is the source or the target of an asynchronous copy (jobs, live, plive, scan_live, pack_out): such a
// buffer must live until the synchronisation that follows its copy, and the plan lives in run()'s frame, to the end of the solve.
struct RunPlan {
    const double* dV = nullptr;
    double* dNewDensity = nullptr;
    bool stats = false;                // the caller wants LevelStats: event pairs around the sweeps, the trip counters
    bool chained = false;
    const int* d_chains = nullptr;     // the chain table of this run and its length
    int run_chains = 0;
    std::vector<Job> jobs;             // the records of this run as the host prepared them (uploaded; uploaded again by a fall-back)
    std::vector<int> live;             // the live jobs of a batch with frozen atoms
    std::vector<int> plive, plevel;    // the levels of the device-side / own-pace search, and each job's index among them (-1: none)
    std::vector<int> second_share;     // more than nblocks / 2 live levels: the levels that get a second workgroup of their own (the others have one)
    std::vector<int> scan_live;        // live jobs of the tolerance-mode scan
    // this run's layout: the solver's own, or -- a batch most of whose atoms have finished (sw) -- latency mode over the live jobs
    bool sw = false, dyn = false, pk = false, early = false, wide = false, use_persist = false, use_own = false;
    int own_W = 1, nfrozen = 0;
    bool carry_cand_hist = true;       // LEVELS_PERSIST_NOBUDGET: off
    bool scan_wanted = false;          // a live level whose history bracket is still wide (or missing): the batch predictor runs
    int scan_match_mode = 0;           // the tolerance-mode scan matches (1) and normalises (2) in its own kernel
    int pack_out[4] = {0, 0, 0, 0};    // k_pack's report on the round it has laid out
    // what the engine that ran leaves behind for the tail and the statistics
    bool searched = false;             // an engine has taken every live level to its eigenvalue
    LevelLayout layout = LAYOUT_STATIC;
    int rounds = 0;
    float ms_sweep = 0;
    bool early_pending = false;        // early match solves are under way on the second stream
};

namespace {

// setup(): allocate / allocate and upload on the context's stream; false: setup() reports the HIP error
template <typename T> bool dev_alloc(DevBuf<T>& buf, size_t count) { return buf.alloc(count) == hipSuccess; }
template <typename T> bool dev_upload(hipStream_t st, DevBuf<T>& buf, const std::vector<T>& vec)
{
    return dev_alloc(buf, vec.size()) && hipMemcpyAsync(buf.p, vec.data(), sizeof(T) * vec.size(), hipMemcpyHostToDevice, st) == hipSuccess;
}

// $DFTA_DEBUG LEVELS_PERSIST_TRACE: one line per closed round of the device-side search, in the order of the closings: time since the
// first record [us], level, rounds taken, then what was planned
void print_persist_trace(const std::vector<unsigned long long>& trace, float ms_kernel)
{
    const size_t n = trace.size() / 4;
    std::vector<size_t> order(n);
    for (size_t q = 0; q < n; ++q) order[q] = q;
    std::sort(order.begin(), order.end(), [&](size_t x, size_t y) { return trace[4 * x] < trace[4 * y]; });
    const unsigned long long t0 = n ? trace[4 * order[0]] : 0;
    fprintf(stderr, "persist trace: %zu records, kernel %.3f ms\n", n, ms_kernel);
    for (size_t q : order) {
        const unsigned long long *w = &trace[4 * q];
        const int ph = (int)(w[2] >> 56);
        if (ph == PH_DONE + 1) fprintf(stderr, "  %9.1f us  job %2d round %2d  search ended\n", (w[0] - t0) * 0.01, (int)(w[1] >> 32), (int)(w[1] & 0xffffffff));
        else if (ph == PH_DONE) fprintf(stderr, "  %9.1f us  job %2d round %2d  DONE (matched, start %llu, candidate %d)\n", (w[0] - t0) * 0.01, (int)(w[1] >> 32), (int)(w[1] & 0xffffffff), w[3] & 0xffffffffull, (int)(signed char)((w[3] >> 32) & 0xff));
        else fprintf(stderr, "  %9.1f us  job %2d round %2d  next: phase %d done %2d blocks %3d spine %2d capz %5d tcap %5d cand %d/%d\n", (w[0] - t0) * 0.01, (int)(w[1] >> 32),
                     (int)(w[1] & 0xffffffff), ph, (int)((w[2] >> 32) & 0xff), (int)((w[2] >> 16) & 0xffff), (int)(w[2] & 0xffff), (int)((w[3] >> 32) & 0xffff), (int)(w[3] & 0xffffffff),
                     (int)((w[3] >> 56) & 0xff), (int)(signed char)((w[3] >> 48) & 0xff));
    }
}

// $DFTA_DEBUG DEBUG_ROUNDS: census of the jobs after a host round (phase / decisions taken), stderr
void print_census(const std::vector<Job>& dbg, int rounds, int debug_rounds)
{
    const int njobs = (int)dbg.size();
    fprintf(stderr, "round %2d |", rounds);
    for (int q = 0; q < njobs; ++q)
        if (dbg[q].phase != PH_DONE) fprintf(stderr, " %d:%d/%d", q, dbg[q].phase, dbg[q].phase_done);
    fprintf(stderr, "\n");
    if (debug_rounds >= 3)
        for (int q = 0; q < njobs; ++q) {
            const Job& J = dbg[q];
            fprintf(stderr, "   J %2d ph %d done %d l %d boe %.17g toe %.17g top %.17g sc_ok %d sc_lo %.17g sc_hi %.17g spine %d use_sp %d miss %d tcap %d\n",
                    q, J.phase, J.phase_done, J.l, J.boe, J.toe, J.top, J.sc_ok, J.sc_lo, J.sc_hi, J.spine, J.use_sp, J.miss, J.tcap);
        }
    if (debug_rounds >= 2)
        for (int q = 0; q < njobs; ++q) {
            const Job& J = dbg[q];
            if (J.phase != PH_TOP) continue;
            fprintf(stderr, "   job %2d l=%d w=%.3e ok=%d spine=%d use_sp=%d miss=%d | a: is=%d phi=%.4e  b: is=%s%d phi=%.4e  c: de=%.3e is=%s%d phi=%.4e | pred w/e=%.3e\n",
                    q, J.l, J.toe - J.boe, J.sc_ok, J.spine, J.use_sp, J.miss, J.sc_is[0], J.sc_phi[0],
                    (J.sc_is[1] >= 0 && (J.sc_is[1] & kStopOver)) ? "o" : "", J.sc_is[1] < 0 ? -1 : (J.sc_is[1] & ~kStopOver), J.sc_phi[1],
                    J.sc_e[2] - J.sc_e[0], (J.sc_is[2] >= 0 && (J.sc_is[2] & kStopOver)) ? "o" : "", J.sc_is[2] < 0 ? -1 : (J.sc_is[2] & ~kStopOver), J.sc_phi[2],
                    J.sc_ok ? (J.toe - J.boe) / (J.sc_hi - J.sc_lo) : 0.0);
        }
}

}  // namespace

// Once per solver.  jobs must be ordered by potential index v (levels of one potential contiguous, in the reference's (N,L) order)
int LevelSolver::setup(dfta_ctx* c, const dfta_grid* grid, int mode_, int tree_depth, int nV_, const std::vector<JobSpec>& specs)
{
    ctx = c; g = grid; mode = mode_; nV = nV_;
    use_prediction = dfta_knob("LEVELS_NOPREDICT") == nullptr;   // measurements / tests: every spine and scout off
    {   // tuning of the predictions (never of a result): the defaults, or what the environment says, every time a solver is made
        if (const char* e = dfta_knob("LEVELS_NOISE")) sscanf(e, "%lf:%lf:%lf", &tuning[0], &tuning[1], &tuning[2]);   // "rel:abs:secant" of the noise band (':' -- the knob list itself is comma-separated)
        hist_extrapolate = dfta_knob("LEVELS_NOEXTRAP") == nullptr;
        if (const char* e = dfta_knob("LEVELS_EXTRAP")) sscanf(e, "%lf:%lf", &hist_kA, &hist_kB);
        if (const char* e = dfta_knob("LEVELS_SECANT_KAPPA")) tuning[3] = atof(e);                              // trust in the parabolic correction
        (void)hipMemcpyToSymbol(HIP_SYMBOL(g_noise_rel), &tuning[0], sizeof(double));
        (void)hipMemcpyToSymbol(HIP_SYMBOL(g_noise_abs), &tuning[1], sizeof(double));
        (void)hipMemcpyToSymbol(HIP_SYMBOL(g_secant_noise), &tuning[2], sizeof(double));
        (void)hipMemcpyToSymbol(HIP_SYMBOL(g_secant_kappa), &tuning[3], sizeof(double));
        fixed_point = dfta_knob("LEVELS_NOFIXEDPOINT") ? 0 : 1;
        (void)hipMemcpyToSymbol(HIP_SYMBOL(g_fixed_point), &fixed_point, sizeof(int));
    }
    debug_rounds = dfta_knob("DEBUG_ROUNDS") ? atoi(dfta_knob("DEBUG_ROUNDS")) : 0;
    njobs = static_cast<int>(specs.size());
    if (njobs == 0) return DFTA_OK;
    const int N = g->N;
    // chains: CHAINED -> one chain per potential; BATCHED -> one chain per job.  Both layouts are kept on the
    // device so that a BATCHED solver can run a CHAINED solve (first SCF step, when there are no hints yet).
    std::vector<int> chain_off, chain_off_b, v_off(nV + 1, 0);
    for (int k = 0; k < njobs; ++k) {
        if (specs[k].v < 0 || specs[k].v >= nV || specs[k].l < 0 || specs[k].l > 3) return DFTA_ERR_INVALID;
        if (k > 0 && specs[k].v < specs[k - 1].v) return DFTA_ERR_INVALID;
        v_off[specs[k].v + 1]++;
    }
    for (int v = 0; v < nV; ++v) v_off[v + 1] += v_off[v];
    for (int v = 0; v < nV; ++v) if (v_off[v + 1] > v_off[v]) chain_off.push_back(v_off[v]);
    chain_off.push_back(njobs);
    for (int k = 0; k <= njobs; ++k) chain_off_b.push_back(k);
    nchains_chained = static_cast<int>(chain_off.size()) - 1;
    nchains = (mode == DFTA_LEVELS_CHAINED) ? nchains_chained : njobs;
    // tree depth.  Few jobs (a handful of atoms): the pipelined sweep kernel runs one 64-trial block per compute unit at
    // ~1/4 of the fused kernel's time per point, so the best depth keeps the blocks of a round within ~1.5 passes over
    // the 256 CUs (measured on Rn: depth 10 = 384 blocks beats 9 and 11).  Many jobs: fill the machine with the fused
    // kernel (one wave per SIMD = 65536 lanes).
    int d = tree_depth;
    if (d <= 0) {
        const long active = std::max(1, mode == DFTA_LEVELS_CHAINED ? nchains : njobs);
        d = 6;
        if (active <= 768) { while (d < 14 && ((active << (d + 1)) >> 6) <= 384) ++d; }
        else               { while (d < 14 && (active << (d + 1)) <= 131072L) ++d; }   // up to two waves per SIMD: measured optimum at 960 jobs
        if (const char* e = dfta_knob("LEVELS_DEPTH")) d = atoi(e);                    // measurements: the automatic layout with another tree depth
    }
    d = std::min(std::max(d, 6), 16);
    depth = d;
    tpj = 1 << d;
    ntrials = static_cast<long>(njobs) * tpj;
    // latency mode (the pipelined kernel's regime: at most ~1.5 passes of one block per compute unit): the slots of a
    // round are re-allotted among the active jobs (k_allot); the budget is one full pass at least
    dynamic = (tree_depth <= 0) && njobs <= 64 && ntrials / 64 <= 384 && dfta_knob("LEVELS_STATIC") == nullptr;
    static_trials = ntrials;
    // A larger job list whose atoms finish one by one (SCF batches: finished atoms are frozen) ends up in that regime too: once at
    // most 64 jobs are live, run() hands the rounds to k_allot through the list of live jobs (room for one pass is kept for it).
    can_switch = (tree_depth <= 0) && !dynamic && mode == DFTA_LEVELS_BATCHED && dfta_knob("LEVELS_STATIC") == nullptr && dfta_knob("LEVELS_NOSWITCH") == nullptr;
    if (dynamic || can_switch) {
        long blocks = std::max(ctx->num_cu, 1);
        if (const char* e = dfta_knob("LEVELS_BUDGET_BLOCKS")) blocks = std::max(64, atoi(e));     // measurements
        budget_trials = 64L * blocks;
        ntrials = std::max<long>(ntrials, budget_trials);
    }
    if (dynamic) budget_trials = ntrials;
    // packed rounds (k_pack): batches whose static layout would have 64-trial trees (up to 192 jobs it has 128 trials per job and
    // the upper half scouts the third bisection: measured on a 12-atom shard, 98 jobs, that is worth 1.6 rounds a step, and the
    // packed layout has no whole blocks of kind ZERO to give to a job that is still counting nodes), unless a depth was asked for
    {
        int min_jobs = 193;
        if (const char* e = dfta_knob("LEVELS_PACK_MIN_JOBS")) min_jobs = atoi(e);              // measurements
        packed = (tree_depth <= 0) && !dynamic && njobs >= min_jobs && dfta_knob("LEVELS_NOPACK") == nullptr;
    }
    // table slots: one per distinct (v, l)
    std::vector<int> slot_v, slot_l;
    std::vector<Job> jobs(njobs);
    {
        std::vector<int> last_of_v(4, -1);          // jobs are ordered by v: only the slots of the current potential can match
        int cur_v = -1;
        for (int k = 0; k < njobs; ++k) {
            if (specs[k].v != cur_v) { cur_v = specs[k].v; std::fill(last_of_v.begin(), last_of_v.end(), -1); }
            int& slot = last_of_v[specs[k].l];
            if (slot < 0) { slot = (int)slot_v.size(); slot_v.push_back(specs[k].v); slot_l.push_back(specs[k].l); }
            Job& j = jobs[k];
            memset(&j, 0, sizeof(Job));
            j.v = specs[k].v; j.n = specs[k].n; j.l = specs[k].l; j.occ = specs[k].occ; j.nodes = specs[k].n - specs[k].l;
            j.slot = slot;
        }
        // sibling: the level of the same potential and l with one node less (its end points bracket this one's, plan_round)
        for (int k = 0, v0 = 0; k < njobs; ++k) {
            if (jobs[k].v != jobs[v0].v) v0 = k;
            jobs[k].sib = -1;
            for (int q = v0; q < njobs && jobs[q].v == jobs[k].v; ++q)
                if (jobs[q].l == jobs[k].l && jobs[q].nodes == jobs[k].nodes - 1) jobs[k].sib = q;
        }
    }
    h_jobs_template = jobs;
    nslots = static_cast<int>(slot_v.size());
    if (packed) {
        pack_lanes_small = std::max(ctx->num_cu, 64) * 64;   // one pass of one block per compute unit: the pipelined kernel's regime
        pack_dsmall = 3;                                     // ... as long as that leaves every job a tree of this depth
        pack_lanes_large = 131072;                   // two waves per SIMD of the fused kernel
        if (const char* e = dfta_knob("LEVELS_PACK_DMIN")) pack_dmin = std::min(std::max(atoi(e), 1), 8);
        if (const char* e = dfta_knob("LEVELS_PACK_LANES")) pack_lanes_large = std::max(4096, atoi(e));
        if (const char* e = dfta_knob("LEVELS_PACK_LANES_SMALL")) pack_lanes_small = std::max(4096, atoi(e));
        if (const char* e = dfta_knob("LEVELS_PACK_DSMALL")) pack_dsmall = atoi(e);
        depth = pack_dmin;
        tpj = 0;                                     // no fixed share: k_pack lays the trials of a round out
        ntrials = std::max<long>(std::max(pack_lanes_large, pack_lanes_small), static_cast<long>(njobs) * (kPackSpineCap + (1L << pack_dmin))) + 128L * nslots;
        ntrials = (ntrials + 63) & ~63L;
    }
    // the own-pace search of a batch (own.inc: one workgroup of W waves per live level, one launch): more than 64 live levels of an
    // un-chained solve on the logarithmic grid; the host rounds remain for everything else ($DFTA_DEBUG LEVELS_NOOWN, LEVELS_NOPERSIST: host rounds)
    own_ok = (tree_depth <= 0) && !dynamic && !g->uniform && mode == DFTA_LEVELS_BATCHED && ctx->sweep_kernel != DFTA_SWEEP_PIPELINED &&
             dfta_knob("LEVELS_OWN") != nullptr && dfta_knob("LEVELS_NOPERSIST") == nullptr && dfta_knob("LEVELS_STATIC") == nullptr;
    if (own_ok) {
        own_waves = 2048;                            // two waves per SIMD: what the sweep's registers (177 VGPRs) leave resident
        if (const char* e = dfta_knob("LEVELS_OWN_WAVES")) own_waves = std::max(64, atoi(e));      // measurements
        if (const char* e = dfta_knob("LEVELS_OWN_WMAX")) own_wmax = std::min(8, std::max(1, atoi(e)));
        if (const char* e = dfta_knob("LEVELS_OWN_SPINE_CAP")) own_spine_cap = atoi(e);
        ntrials = std::max<long>(ntrials, 64L * std::max<long>(own_waves, njobs));
    }
    nwaves = static_cast<int>(ntrials / 64);
    early_match = (dynamic || can_switch) && !g->uniform && dfta_knob("LEVELS_NOEARLYMATCH") == nullptr;
    // the device-side search serves the latency regime (one atom, or the last live atoms of a batch) on the logarithmic grid
    persist_ok = (dynamic || can_switch) && !g->uniform && ctx->sweep_kernel != DFTA_SWEEP_FUSED && dfta_knob("LEVELS_NOPERSIST") == nullptr;

    std::vector<int> wave_slot(nwaves), wave_first(nwaves), wave_cnt(nwaves, 64), wave_job(nwaves);
    for (int w = 0; w < nwaves; ++w) {
        const int q = packed ? njobs : (w * 64) / tpj;
        wave_job[w] = q < njobs ? q : -1;
        wave_slot[w] = q < njobs ? jobs[q].slot : 0;
        wave_first[w] = w * 64;
    }
    h_wave_job = wave_job;
    h_wave_slot = wave_slot;

    hipStream_t st = ctx->stream;
    auto no_memory = [&]() { snprintf(ctx->err, sizeof(ctx->err), "level solver: device buffers -> %s", hipGetErrorString(hipGetLastError())); return (int)DFTA_ERR_HIP; };
    h_occ.resize(njobs);
    for (int k = 0; k < njobs; ++k) h_occ[k] = specs[k].docc;
    const size_t nt = (size_t)ntrials;
    bool ok = dev_alloc(d_jobs, njobs) && dev_upload(st, d_occ, h_occ) && dev_upload(st, d_chain_off, chain_off) && dev_upload(st, d_chain_off_b, chain_off_b) &&
              dev_upload(st, d_v_off, v_off) && dev_upload(st, d_slot_v, slot_v) && dev_upload(st, d_slot_l, slot_l) && dev_alloc(d_tab, (size_t)nslots * N) &&
              dev_alloc(d_E, nt) && dev_alloc(d_limit, nt) && dev_alloc(d_start, nt) && dev_alloc(d_us, nt) && dev_alloc(d_us1, nt) &&
              dev_alloc(d_count, nt) && dev_alloc(d_u0, nt) && dev_alloc(d_phi, nt) && dev_alloc(d_istop, nt) && dev_alloc(d_trip, nt) &&
              dev_alloc(d_wave_kind, nwaves) && dev_upload(st, d_wave_slot, wave_slot) && dev_upload(st, d_wave_first, wave_first) &&
              dev_upload(st, d_wave_cnt, wave_cnt) && dev_upload(st, d_wave_job, wave_job);
    if (ok && packed) {
        std::vector<int> slot_off(nslots + 1, 0), slot_jobs(njobs);
        for (int k = 0; k < njobs; ++k) slot_off[jobs[k].slot + 1]++;
        for (int q = 0; q < nslots; ++q) slot_off[q + 1] += slot_off[q];
        std::vector<int> fill(slot_off.begin(), slot_off.end() - 1);
        for (int k = 0; k < njobs; ++k) slot_jobs[fill[jobs[k].slot]++] = k;
        ok = dev_upload(st, d_slot_off, slot_off) && dev_upload(st, d_slot_jobs, slot_jobs) && dev_alloc(d_gsz, 2 * (size_t)nslots) &&
             dev_alloc(d_goff, 2 * (size_t)nslots) && dev_alloc(d_lane_job, nt) && dev_alloc(d_pack_out, 4);
        if (ok) DFTA_HIP(ctx, hipStreamSynchronize(st));     // the vectors above are the sources of the copies
    }
    if (!ok || !dev_alloc(d_counters, 4)) return no_memory();
    // the device-side search takes up to 256 live levels: one workgroup per level and compute unit, two for as many levels as there are
    // compute units left (all of them up to 128 levels), the rest in the pool; LEVELS_PERSIST_WIDE=n: up to 64 <= n <= 256 levels (64: one
    // atom's worth, round 5 -- larger batches then run host rounds)
    if (const char* e = dfta_knob("LEVELS_PERSIST_WIDE")) persist_cap = std::min(256, std::max(64, atoi(e)));
    if (persist_ok) { const int prc = dfta_persist_create(ctx, g, std::min(njobs, persist_cap), &pb); if (prc) return prc; }
    ok = (!can_switch || dev_alloc(d_live, 64)) &&
         (g->uniform || dfta_knob("LEVELS_NOQUEUE") != nullptr || dev_alloc(d_queue, kSweepQueueClasses + 1 + (size_t)kSweepQueueClasses * nwaves)) &&
         (!own_ok || dev_alloc(d_own_live, njobs)) && dev_alloc(d_Psi, (size_t)njobs * N) && dev_alloc(d_Q, (size_t)njobs * N) &&
         dev_alloc(d_jE, njobs) && dev_alloc(d_jslot, njobs) && dev_alloc(d_jl, njobs) && dev_alloc(d_jstart, njobs) &&
         dev_alloc(d_jmatched, njobs) && dev_alloc(d_jstart_keep, njobs) && dev_alloc(d_snapE, njobs) && dev_alloc(d_snapReady, njobs) &&
         dev_alloc(d_jtake, njobs);
    if (!ok) return no_memory();
    if (early_match) {
        DFTA_HIP(ctx, hipStreamCreateWithFlags(&st2.s, hipStreamNonBlocking));
        DFTA_HIP(ctx, hipEventCreateWithFlags(&ev_walk.e, hipEventDisableTiming));
        DFTA_HIP(ctx, hipEventCreateWithFlags(&ev_early.e, hipEventDisableTiming));
        DFTA_HIP(ctx, hipEventCreateWithFlags(&ev_taken.e, hipEventDisableTiming));
    }
    ok = dev_alloc(d_jus, njobs) && dev_alloc(d_jus1, njobs) && dev_alloc(d_jmp, njobs) && dev_alloc(d_slot_min, nslots) &&
         dev_alloc(d_bounds, (size_t)nslots * dfta_bounds_stride(g));
    if (!ok) return no_memory();
    // Round 6: the scan search (scan.hip: 40 - 60 us per sweep instead of 4 ms) runs the FIRST bisection of every live level ahead of the
    // device-side exact search and hands its end point to plan_round as the bracket of the exact search's first spine -- speculation only,
    // as the history bracket it replaces: the exact sweeps at the reference's midpoints take every decision.  One atom / a few atoms
    // (<= 64 jobs: the solver whose every run is the device-side search); $DFTA_DEBUG LEVELS_NOSCANPREDICT: off.
    // Batches (host rounds): the same with one workgroup per level (k_scan_levels, which stops at a quarter of the band); the scan tables of
    // all the batch's slots must be affordable (<= 2 GB).
    scan_predict = (sweep_mode != DFTA_SWEEPS_TOLERANCE && dfta_scan_supported(g) && dfta_knob("LEVELS_NOSCANPREDICT") == nullptr && use_prediction &&
                    mode == DFTA_LEVELS_BATCHED && tree_depth <= 0 &&
                    ((persist_ok && dynamic) || (!dynamic && (size_t)nslots * N * sizeof(double) <= ((size_t)2 << 30) && dfta_knob("LEVELS_NOSCANPREDICT_BATCH") == nullptr))) ? 1 : 0;
    if (const char* e = dfta_knob("LEVELS_SCAN_PREDICT_W")) scan_predict_factor = atof(e);
    if (const char* e = dfta_knob("LEVELS_SCAN_PREDICT_SHIFT")) scan_predict_shift = atof(e);
    if (scan_predict && !(dev_alloc(d_jobs_scan, njobs) && dev_alloc(d_counters_scan, 4))) return no_memory();
    if ((sweep_mode == DFTA_SWEEPS_TOLERANCE || scan_predict) && dfta_scan_supported(g)) {      // scan.hip: interleaved tables + per-lane {min, max}
        const int trc = dfta_scan_tables_create(ctx, g, nslots, &scan_tb);
        if (trc) return trc;
        if (!(dev_alloc(d_scan_live, njobs) && dev_alloc(d_scan_xch, 32 * (size_t)njobs))) return no_memory();
    }
    DFTA_HIP(ctx, hipEventCreate(&ev[0].e));
    DFTA_HIP(ctx, hipEventCreate(&ev[1].e));
    DFTA_HIP(ctx, hipMemsetAsync(d_count, 0, sizeof(int) * ntrials, st));
    DFTA_HIP(ctx, hipMemsetAsync(d_u0, 0, sizeof(double) * ntrials, st));
    DFTA_HIP(ctx, hipMemsetAsync(d_trip, 0, sizeof(int) * ntrials, st));
    DFTA_HIP(ctx, hipStreamSynchronize(st));
    return DFTA_OK;
}

// What this run does: the layout of its host rounds and the engines that may run ahead of them (no HIP call)
void LevelSolver::make_plan(RunPlan& p, int run_mode, const unsigned char* frozen) const
{
    p.chained = (run_mode == DFTA_LEVELS_CHAINED);
    p.d_chains = p.chained ? d_chain_off : d_chain_off_b;
    p.run_chains = p.chained ? nchains_chained : njobs;
    const bool have_last = h_last.size() == (size_t)njobs;
    // this run's layout: the solver's own, or -- a batch most of whose atoms have finished -- latency mode over the live jobs
    if (frozen && have_last)
        for (int k = 0; k < njobs; ++k) if (!frozen[k]) p.live.push_back(k);
    p.sw = can_switch && !p.chained && frozen && have_last && !p.live.empty() && p.live.size() <= 64;
    p.dyn = dynamic || p.sw;
    p.pk = packed && !p.sw;
    p.early = early_match && p.dyn;
    p.layout = p.sw ? LAYOUT_LATENCY_LIVE : (dynamic ? LAYOUT_LATENCY : (p.pk ? LAYOUT_PACKED : LAYOUT_STATIC));      // of the host rounds; an engine that runs instead says so
    // the live levels of a latency-mode run search on the device, each at its own pace (persist.inc), when every one of them can have two
    // 64-trial blocks of its own; the host rounds are the fallback
    if (p.sw) p.plive = p.live;
    else for (int k = 0; k < njobs; ++k) if (!(frozen && frozen[k] && have_last)) p.plive.push_back(k);
    const int nplive = (int)p.plive.size();
    // (wide: 65 .. persist_cap live levels of a batch whose host rounds -- the fallback -- are the solver's own static / packed layout)
    p.wide = !p.dyn && !own_ok && persist_cap > 64 && nplive > 64;          // (LEVELS_OWN: that search was asked for)
    p.use_persist = persist_ok && (p.dyn || p.wide) && !p.chained && sweep_mode != DFTA_SWEEPS_TOLERANCE && nplive > 0 && nplive <= pb.nlive_cap &&
                    pb.nblocks / nplive >= (persist_cap > 128 ? 1 : 2) && debug_rounds == 0;
    // more than 64 live levels: every level at its own pace all the same, one workgroup of W waves each in ONE ordinary launch (own.inc)
    p.use_own = own_ok && !p.dyn && !p.chained && sweep_mode != DFTA_SWEEPS_TOLERANCE && nplive > 0 && debug_rounds == 0;
    if (p.use_own) { while (p.own_W < own_wmax && (long)nplive * p.own_W * 2 <= own_waves) p.own_W *= 2; }
    p.plevel.assign(njobs, -1);
    if (p.use_persist || p.use_own) for (int q = 0; q < nplive; ++q) p.plevel[p.plive[q]] = q;
    p.carry_cand_hist = dfta_knob("LEVELS_PERSIST_NOBUDGET") == nullptr;
    // the match solve and the normalisation in the scan's own kernel (SCAN_NOMATCH: the exact k_match / k_normalize follow, measurements)
    p.scan_match_mode = dfta_knob("SCAN_NOMATCH") ? 0 : (integ_rule == DFTA_INT_SIMPSON38 ? 2 : 1);
}

// Trial slots of job k in the host rounds: its own static block; packed rounds: k_pack lays the trials out (latency mode: k_allot)
void LevelSolver::host_round_slots(const RunPlan& p, int k, Job& j) const
{
    j.tbase = (p.pk || p.sw) ? 0 : k * tpj;
    j.tcap = (p.pk || p.sw) ? 0 : tpj;
}

// The records of this run (p.jobs) from the template, the frozen mask, the previous solve's records (h_last) and the bracket bottoms:
// path predictions, history brackets, scan_wanted, the candidate budget.  Host arithmetic only.
void LevelSolver::prepare_jobs(RunPlan& p, const double* job_bottom, const unsigned char* frozen) const
{
    std::vector<Job>& jobs = p.jobs;
    jobs = h_jobs_template;
    const bool have_last = h_last.size() == jobs.size();
    for (int k = 0; k < njobs; ++k) {
        Job& j = jobs[k];
        if (frozen && frozen[k] && have_last) {
            j = h_last[k];             // E, interval, convergence flag, match point, history: as the last solve left them
            j.phase = PH_DONE;
            j.frozen = 1;
            j.spine = 0;
            j.capz = 0;
            ++p.nfrozen;
            continue;
        }
        j.frozen = 0;
        host_round_slots(p, k, j);
        if (p.use_persist) { j.tbase = p.plevel[k] * pb.tmax; j.tcap = 0; }      // its own region of the device-side search's trial arrays
        if (p.use_own) { j.tbase = p.plevel[k] * 64 * p.own_W; j.tcap = 64 * p.own_W; }
        j.rounds = 0;
        j.t_end_us = 0;
        j.deep = -1;
        j.cand_hist = (use_prediction && have_last && p.carry_cand_hist) ? h_last[k].cand_hist : 0;
        j.bottom0 = job_bottom[k];
        const bool first = (k == 0 || jobs[k].v != jobs[k - 1].v);
        if (!p.chained || first) { j.phase = PH_TOP; j.toe = 50; j.boe = j.bottom0; }   // DFTAtom.cpp:499
        else j.phase = PH_WAIT;
        // path prediction from the previous solve of the same job list (speculation only)
        if (use_prediction && have_last) {
            for (int ph = 0; ph < 3; ++ph) {
                j.pred_bits[ph] = h_last[k].cur_bits[ph];
                j.pred_len[ph] = h_last[k].cur_len[ph];
                j.trust[ph] = h_last[k].trust[ph];
                // the very first comparison has no history: trust what a one-step-old prediction typically gives
                // (no spine from it: a miss forfeits the whole tree of a round, three predicted bits are not worth that)
                if (h_last[k].pred_len[ph] == 0) j.trust[ph] = 0;
            }
            const Job& h = h_last[k];
            const double T[3] = {h.top, h.bottom, h.E};
            for (int ph = 0; ph < 3; ++ph) {
                constexpr double kHistSafety = 2.0;
                const double d = h.hist_ok >= 1 ? T[ph] - h.hist_T[ph] : 0.0;
                j.hist_T[ph] = T[ph];
                j.hist_s[ph] = d;
                j.hist_d[ph] = h.hist_ok >= 1 ? fabs(d) : -1.0;
                const double q = (h.hist_ok >= 2 && h.hist_s[ph] != 0.0) ? d / h.hist_s[ph] : NAN;
                j.hist_q[ph] = q;
                j.hist_c[ph] = T[ph];
                j.hist_w[ph] = kHistSafety * fabs(d);
                // geometric convergence: extrapolate with the last ratio; the bracket is as wide as the ratio has been unsteady
                if (hist_extrapolate && h.hist_ok >= 3 && std::isfinite(q) && std::isfinite(h.hist_q[ph]) && fabs(q) <= 1.0 && fabs(h.hist_q[ph]) <= 1.0) {
                    const double u = (hist_kA + hist_kB * fabs(q - h.hist_q[ph])) * fabs(d);
                    if (u < j.hist_w[ph]) { j.hist_c[ph] = T[ph] + q * d; j.hist_w[ph] = u; }
                }
            }
            j.hist_ok = std::min(h.hist_ok + 1, 3);
        } else {
            j.hist_ok = 0;
        }
        {   // does this level still want the scan predictor of its first spine?  (scan.hip:k_scan_levels: the same rule, per level)
            const double T = j.hist_c[0], band = 6e-11 * fabs(T) + 6e-10;
            if (!(j.hist_ok >= 2 && j.hist_d[0] >= 0 && j.hist_w[0] + 1e-10 * fabs(T) + 64e-12 <= 4096. * band)) p.scan_wanted = true;
        }
        j.miss = j.capz = j.se_state = j.se_stop = j.se_sl = j.se_tok = j.sc_ok = j.use_sp = j.sp_len = j.phase_done = 0;
        j.se_plo = j.se_phi = NAN;
        j.sc_is[0] = j.sc_is[1] = j.sc_is[2] = -1;
        j.sp_bits = 0;
        j.spine = 0;           // planned on the device (k_plan), after the bottoms have been clamped
    }
}

// Feedback of the device-side search (speculation only): the levels whose search ended last in the previous step get first call on the pool
// (persist_plan, deep = 2: as many as the pool can give a second share to), those within 15 % of the last one may match candidate
// eigenvalues (deep = 1), the rest have time to spare (deep = 0)
// (ranked by the maximum over the last three steps: a level that gets its deeper trees ends earlier, and a one-step memory would take
// them away again in the next step)
void LevelSolver::rank_feedback(RunPlan& p)
{
    persist_deep_reserve = 0;
    std::vector<Job>& jobs = p.jobs;
    const std::vector<int>& plive = p.plive;
    if (!(p.use_persist && h_last.size() == jobs.size() && !pb.equal_shares)) return;
    if (persist_tend.size() != 3 * jobs.size()) persist_tend.assign(3 * jobs.size(), 0);
    for (int k : plive) {
        int* h = &persist_tend[3 * (size_t)k];
        if (h_last[k].t_end_us > 0) { h[2] = h[1]; h[1] = h[0]; h[0] = h_last[k].t_end_us; }
    }
    auto score = [&](int k) { const int* h = &persist_tend[3 * (size_t)k]; return std::max(h[0], std::max(h[1], h[2])); };
    std::vector<int> order;
    for (int k : plive) if (score(k) > 0) order.push_back(k);
    if (order.size() != plive.size()) return;
    std::sort(order.begin(), order.end(), [&](int x, int y) { return score(x) > score(y); });
    const int equal = pb.nblocks / (int)plive.size();
    if (equal == 1) p.second_share.assign(order.begin(), order.begin() + std::min<size_t>(order.size(), pb.nblocks - (int)plive.size()));
    int pool = pb.nblocks - equal * (int)plive.size();
    for (int k : plive) if (jobs[k].nodes == 0 && equal >= 8) pool += equal / 2;
    const int ndeep = std::min<int>((int)order.size(), pool / std::max(equal - 1, 1));
    persist_deep_reserve = ndeep * (equal - 1);
    const int tmax_us = score(order[0]);
    for (size_t q = 0; q < order.size(); ++q)
        jobs[order[q]].deep = (int)q < ndeep ? 2 : (score(order[q]) > 0.85 * tmax_us ? 1 : 0);
    if (pb.want_trace) {
        fprintf(stderr, "persist feedback: pool %d, reserve %d; search ends of the previous step [us]:", pool, persist_deep_reserve);
        for (size_t q = 0; q < order.size(); ++q) fprintf(stderr, " %d:%d%s", order[q], score(order[q]), jobs[order[q]].deep == 2 ? "*" : "");
        fprintf(stderr, "\n");
    }
}

// Back to the host rounds after an engine gave the solve up: the records as they were uploaded, in the host rounds' own trial slots, the
// counters zeroed, the bottoms clamped again.  (The scan search hands back records whose slots ARE the host rounds' -- use_persist and
// use_own are false in tolerance mode, and nothing writes p.jobs after prepare_jobs / rank_feedback -- so setting them is a no-op there.)
int LevelSolver::restore_jobs_for_rounds(RunPlan& p)
{
    hipStream_t st = ctx->stream;
    for (int k = 0; k < njobs; ++k) if (!p.jobs[k].frozen) host_round_slots(p, k, p.jobs[k]);
    DFTA_HIP(ctx, hipMemcpyAsync(d_jobs, p.jobs.data(), sizeof(Job) * njobs, hipMemcpyHostToDevice, st));
    DFTA_HIP(ctx, hipMemsetAsync(d_counters, 0, sizeof(unsigned long long) * 4, st));
    return clamp_job_bottoms(p);
}

int LevelSolver::clamp_job_bottoms(const RunPlan& p)
{
    if (p.chained || !clamp_bottoms) return DFTA_OK;
    hipLaunchKernelGGL(k_clamp_bottoms, dim3((njobs + 63) / 64), dim3(64), 0, ctx->stream, d_jobs.p, njobs, d_slot_min.p);
    DFTA_CHECK_LAUNCH(ctx);
    return DFTA_OK;
}

// TOLERANCE MODE of the sweeps (scan.hip, opt-in): every level's three bisections by one workgroup, start to end on the device --
// no rounds, no speculation.  A sweep the scan cannot decide (non-finite values, f >= 12 in a step row: never seen for the
// potential of an SCF) sends the whole solve to the exact kernels: the host rounds.
int LevelSolver::search_scan(RunPlan& p)
{
    hipStream_t st = ctx->stream;
    int rc = dfta_launch_scan_build_tab(ctx, g, scan_tb, p.dV, d_slot_v, d_slot_l);
    if (rc) return rc;
    // a handful of levels leave compute units idle: K = 15, 7 or 3 workgroups per level take a depth-4, 3 or 2 bisection tree per round
    std::vector<int>& live_jobs = p.scan_live;
    for (int k = 0; k < njobs; ++k) if (!p.jobs[k].frozen) live_jobs.push_back(k);
    int K = 1;
    if (!p.chained && !live_jobs.empty()) {
        for (int cand : {15, 7, 3}) if ((long)live_jobs.size() * cand <= ctx->num_cu) { K = cand; break; }
        if (const char* e = dfta_knob("SCAN_GROUP")) { const int f = atoi(e); K = (f == 15 || f == 7 || f == 3) && (long)live_jobs.size() * f <= ctx->num_cu ? f : 1; }
    }
    DFTA_HIP(ctx, hipEventRecord(ev[0], st));
    rc = DFTA_ERR_NOT_CONVERGED;
    if (K > 1) {
        DFTA_HIP(ctx, hipMemcpyAsync(d_scan_live, live_jobs.data(), sizeof(int) * live_jobs.size(), hipMemcpyHostToDevice, st));
        DFTA_HIP(ctx, hipMemsetAsync(d_jstart_keep, 0xff, sizeof(int) * njobs, st));      // -1: frozen (the live jobs write their cut-off index)
        rc = dfta_launch_scan_levels_group(ctx, g, d_jobs, d_scan_live, (int)live_jobs.size(), K, scan_tb, dfta_knob("LEVELS_NOFIXEDPOINT") ? 0 : 1, d_counters,
                                           d_scan_xch, p.scan_match_mode, d_Psi, d_jstart_keep);
        if (rc && rc != DFTA_ERR_NOT_CONVERGED) return rc;
    }
    if (rc == DFTA_ERR_NOT_CONVERGED) {
        K = 1;
        rc = dfta_launch_scan_levels(ctx, g, d_jobs, p.d_chains, p.run_chains, p.chained ? 1 : 0, scan_tb, dfta_knob("LEVELS_NOFIXEDPOINT") ? 0 : 1, d_counters,
                                     p.scan_match_mode, d_Psi, d_jstart_keep);
    }
    if (rc) return rc;
    scan_group = K;
    DFTA_HIP(ctx, hipEventRecord(ev[1], st));
    unsigned long long flag = 0;
    DFTA_HIP(ctx, hipMemcpyAsync(&flag, d_counters + 3, sizeof(flag), hipMemcpyDeviceToHost, st));
    DFTA_HIP(ctx, hipStreamSynchronize(st));
    if (p.stats) DFTA_HIP(ctx, hipEventElapsedTime(&p.ms_sweep, ev[0], ev[1]));
    if (flag) {                  // back to the exact kernels with the job records as they were uploaded (a trial the scan could not decide, or a lost group member)
        ++scan_fallbacks;
        return restore_jobs_for_rounds(p);
    }
    p.searched = true;
    p.layout = LAYOUT_SCAN;
    p.rounds = 1;
    return DFTA_OK;
}

// The scan search of the first bisection as a predictor of the exact search's first spines (speculation only): a group of workgroups per
// level ahead of the device-side search, one workgroup per level ahead of the host rounds of a batch
int LevelSolver::predict_scan(RunPlan& p)
{
    const std::vector<int>& plive = p.plive;
    if (!(!p.chained && scan_predict && scan_tb.tabv != nullptr && !plive.empty() && debug_rounds == 0 && ((p.use_persist && !p.wide) || p.scan_wanted))) return DFTA_OK;
    hipStream_t st = ctx->stream;
    int K = 1;
    if (p.use_persist) for (int cand : {15, 7, 3}) if ((long)plive.size() * cand <= ctx->num_cu) { K = cand; break; }
    const bool grouped = p.use_persist && K > 1;             // (a wide device-side search: one workgroup per level, as for the host rounds)
    if (!(grouped || !p.use_persist || p.wide)) return DFTA_OK;
    const int rc = dfta_launch_scan_build_tab(ctx, g, scan_tb, p.dV, d_slot_v, d_slot_l);
    if (rc) return rc;
    DFTA_HIP(ctx, hipMemcpyAsync(d_jobs_scan, d_jobs, sizeof(Job) * njobs, hipMemcpyDeviceToDevice, st));
    DFTA_HIP(ctx, hipMemcpyAsync(d_scan_live, plive.data(), sizeof(int) * plive.size(), hipMemcpyHostToDevice, st));
    DFTA_HIP(ctx, hipMemsetAsync(d_counters_scan, 0, sizeof(unsigned long long) * 4, st));
    const int prc = grouped
        ? dfta_launch_scan_levels_group(ctx, g, d_jobs_scan, d_scan_live, (int)plive.size(), K, scan_tb, fixed_point, d_counters_scan, d_scan_xch, -1, nullptr, nullptr)
        : dfta_launch_scan_levels(ctx, g, d_jobs_scan, d_chain_off_b, njobs, 0, scan_tb, fixed_point, d_counters_scan, -1, nullptr, nullptr);
    if (prc == DFTA_OK) {
        hipLaunchKernelGGL(k_inject_scan_top, dim3(((int)plive.size() + 63) / 64), dim3(64), 0, st, d_jobs.p, d_jobs_scan.p, d_scan_live.p, (int)plive.size(), d_counters_scan.p, scan_predict_factor, scan_predict_shift);
        DFTA_CHECK_LAUNCH(ctx);
    } else if (prc != DFTA_ERR_NOT_CONVERGED) return prc;
    return DFTA_OK;
}

// The device-side search (persist.inc): sweeps, walk, match and normalisation of every live level in one persistent kernel.  A lost
// worker (or a grid that cannot be co-resident) sends the whole solve to the host rounds, from the records as they were.
int LevelSolver::search_persist(RunPlan& p)
{
    hipStream_t st = ctx->stream;
    const std::vector<int>& plive = p.plive;
    dfta_range r_p("dfta: level search on the device (persistent kernel: sweeps, walk, match, normalisation)");
    DFTA_HIP(ctx, hipMemsetAsync(d_jstart_keep, 0xff, sizeof(int) * njobs, st));      // -1: frozen (the live levels write their cut-off index)
    if (p.stats) DFTA_HIP(ctx, hipEventRecord(ev[0], st));
    float ms_persist = 0;
    const bool want_trace = pb.want_trace;
    // A level without nodes has no second bisection (walk_job takes it without a sweep): a third of the search less, so half of its equal
    // share goes to the pool, from which the levels whose phases need one decision more than their trees hold take deeper ones
    std::vector<int> share(plive.size());
    const int equal = pb.nblocks / (int)plive.size();
    const bool float_shares = !pb.equal_shares && equal >= 8;
    for (size_t q = 0; q < plive.size(); ++q) share[q] = (float_shares && p.jobs[plive[q]].nodes == 0) ? equal - equal / 2 : equal;
    if (equal == 1 && !pb.equal_shares) {
        // one workgroup per level leaves nblocks - nlive over: second workgroups (scouts, a tree one level deeper) for the levels whose
        // search ended last in the previous steps; without that feedback, for the first ones of the list
        if (p.second_share.empty()) for (size_t q = 0; q < plive.size() && (int)q < pb.nblocks - (int)plive.size(); ++q) share[q] = 2;
        else for (int k : p.second_share) share[p.plevel[k]] = 2;
    }
    PersistRun run;
    run.Psi = d_Psi; run.Q = d_Q; run.jstart_keep = d_jstart_keep; run.counters = d_counters;
    run.stats = p.stats; run.nopredict = use_prediction ? 0 : 1; run.integ_rule = integ_rule; run.tuning = tuning; run.fixed_point = fixed_point;
    run.share = share.data(); run.deep_reserve = persist_deep_reserve; run.want_trace = want_trace;
    PersistResult res;
    const int rc = dfta_launch_levels_persist(ctx, g, &pb, d_jobs, plive.data(), (int)plive.size(), tables(), run, &res);
    if (rc) return rc;
    if (p.stats) { DFTA_HIP(ctx, hipEventRecord(ev[1], st)); DFTA_HIP(ctx, hipEventSynchronize(ev[1])); DFTA_HIP(ctx, hipEventElapsedTime(&ms_persist, ev[0], ev[1])); }
    ++persist_runs;
    if (!res.aborted) {
        if (want_trace) { persist_trace.swap(res.trace); print_persist_trace(persist_trace, ms_persist); }
        p.searched = true;            // every live level was matched and normalised by the workgroup that closed its search
        p.layout = LAYOUT_PERSIST;
        p.rounds = res.rounds;
        p.ms_sweep = ms_persist;
        return DFTA_OK;
    }
    ++persist_fallbacks;
    {   // said once per process: the results are the same, the step is slower (dfta_step_stats::levels_fallbacks counts them)
        static bool told = false;
        if (!told) {
            told = true;
            fprintf(stderr, "dftatom_hip: the device-side level search did not finish (a workgroup of its cooperative launch was not scheduled -- "
                            "another process on the device, masked compute units -- or timed out); this solve and any later one that fails the "
                            "same way run with host-synchronised rounds instead: same results, slower steps\n");
        }
    }
    return restore_jobs_for_rounds(p);
}

// The own-pace search of a batch (own.inc): one workgroup of W waves per live level, sweeps + walk in one ordinary launch
int LevelSolver::search_own(RunPlan& p)
{
    hipStream_t st = ctx->stream;
    dfta_range r_o("dfta: level search on the device (own pace: one workgroup per level, sweeps + walk)");
    DFTA_HIP(ctx, hipMemcpyAsync(d_own_live, p.plive.data(), sizeof(int) * p.plive.size(), hipMemcpyHostToDevice, st));
    if (p.stats) DFTA_HIP(ctx, hipEventRecord(ev[0], st));
    OwnLevels lv;
    lv.jobs = d_jobs; lv.live = d_own_live; lv.nlive = (int)p.plive.size(); lv.W = p.own_W;
    OwnOptions opt;
    opt.stats = p.stats; opt.nopredict = use_prediction ? 0 : 1; opt.spine_cap = own_spine_cap;
    const int rc = dfta_launch_levels_own(ctx, g, lv, tables(), blocks(lv.nlive * lv.W), trials(p.stats), d_counters, opt);
    if (rc) return rc;
    if (p.stats) DFTA_HIP(ctx, hipEventRecord(ev[1], st));
    tables_dirty = true;             // the kernel wrote its blocks' table slots
    own_last_W = p.own_W;
    p.searched = true;
    p.layout = LAYOUT_OWN;           // (rounds and sweep time: read with the counters, fill_stats)
    return DFTA_OK;
}

// spines (and, in latency mode, the slots) of the next host round
int LevelSolver::plan_round(const RunPlan& p)
{
    hipStream_t st = ctx->stream;
    if (p.dyn)
        hipLaunchKernelGGL(k_allot, dim3(1), dim3(64), 0, st, d_jobs.p, p.sw ? (int)p.live.size() : njobs, (int)budget_trials, use_prediction ? 0 : 1, d_wave_job.p,
                           d_wave_slot.p, p.sw ? d_live.p : nullptr);
    else
        hipLaunchKernelGGL(k_plan, dim3((njobs + 63) / 64), dim3(64), 0, st, d_jobs.p, njobs, use_prediction ? 0 : 1, p.pk ? (1 << 14) : 0);
    DFTA_CHECK_LAUNCH(ctx);
    if (p.pk) {
        hipLaunchKernelGGL(k_pack, dim3(1), dim3(kPackThreads), 0, st, d_jobs.p, njobs, nslots, d_slot_off.p, d_slot_jobs.p, pack_lanes_small,
                           pack_dsmall, pack_lanes_large, pack_dmin, pack_dmax, d_gsz.p, d_goff.p, d_lane_job.p, d_wave_slot.p, d_pack_out.p);
        DFTA_CHECK_LAUNCH(ctx);
        hipLaunchKernelGGL(k_pack_lanes, dim3((njobs + 3) / 4), dim3(256), 0, st, d_jobs.p, njobs, d_lane_job.p);
        DFTA_CHECK_LAUNCH(ctx);
    }
    return DFTA_OK;
}

// Match solves of the levels whose search has ended while others still search: on the second stream, under the next round's sweeps
// (two waves and 8 KB of LDS per level fit next to a sweep block)
int LevelSolver::early_match_solves(RunPlan& p)
{
    DFTA_HIP(ctx, hipStreamWaitEvent(st2, ev_walk, 0));
    hipLaunchKernelGGL(k_take_ready, dim3((njobs + 63) / 64), dim3(64), 0, st2.s, d_snapE.p, d_snapReady.p, d_jmatched.p, njobs, d_jE.p, d_jtake.p);
    DFTA_CHECK_LAUNCH(ctx);
    DFTA_HIP(ctx, hipEventRecord(ev_taken, st2));
    int erc = dfta_launch_boundary(ctx, g, job_boundary(), st2);
    if (!erc) {
        hipLaunchKernelGGL(k_mask_ready, dim3((njobs + 63) / 64), dim3(64), 0, st2.s, d_jtake.p, njobs, d_jstart.p, d_jmatched.p, d_jstart_keep.p);
        DFTA_CHECK_LAUNCH(ctx);
        erc = dfta_launch_match(ctx, g, tables(), job_match(), st2);
    }
    if (erc) return erc;
    DFTA_HIP(ctx, hipEventRecord(ev_early, st2));
    p.early_pending = true;
    return DFTA_OK;
}

// The host rounds: expand, sweeps, scout, walk, plan -- one host synchronisation per round, all levels in lock step
int LevelSolver::search_rounds(RunPlan& p)
{
    const int N = g->N;
    hipStream_t st = ctx->stream;
    const bool pk = p.pk, early = p.early, stats = p.stats;
    int rc = plan_round(p);
    if (rc) return rc;
    // trials of the coming round: the whole static / latency-mode layout, or what k_pack has just laid out
    long round_trials = p.dyn ? budget_trials : static_trials;
    int* pack_out = p.pack_out;
    if (pk) {
        DFTA_HIP(ctx, hipMemcpyAsync(pack_out, d_pack_out, sizeof(p.pack_out), hipMemcpyDeviceToHost, st));
        DFTA_HIP(ctx, hipStreamSynchronize(st));
        round_trials = pack_out[0];
    }
    if (early) {
        hipLaunchKernelGGL(k_job_slots, dim3((njobs + 63) / 64), dim3(64), 0, st, d_jobs.p, njobs, d_jslot.p, d_jl.p);
        DFTA_CHECK_LAUNCH(ctx);
        DFTA_HIP(ctx, hipMemsetAsync(d_jE, 0xff, sizeof(double) * njobs, st));      // NaN: "no energy yet" (k_take_ready)
    }
    int* d_ndone = reinterpret_cast<int*>(d_counters + 2);
    int done_seen = p.nfrozen;
    while (p.rounds < kMaxRounds) {
        dfta_range r_round("dfta: level-search round (expand, sweeps, scout, walk, plan)");
        if (round_trials <= 0 || round_trials > ntrials) { snprintf(ctx->err, sizeof(ctx->err), "level solver: packed round of %ld trials (room for %ld)", round_trials, ntrials); return DFTA_ERR_HIP; }
        const int round_waves = static_cast<int>(round_trials / 64);
        // the fused sweeps of a batch are launched as a queue of blocks, longest first (numerov.hip:k_sweep_queue)
        // (the pipelined kernel likewise once a round has more blocks than compute units: its second pass is then made of the short blocks)
        const bool queued = d_queue.p != nullptr && !g->uniform && (dfta_sweep_is_fused(ctx, round_waves) || round_waves > ctx->num_cu);
        if (queued) DFTA_HIP(ctx, hipMemsetAsync(d_queue, 0, sizeof(int) * (kSweepQueueClasses + 1), st));
        hipLaunchKernelGGL(k_expand, dim3((unsigned)((round_trials + 255) / 256)), dim3(256), 0, st, d_jobs.p, pk ? d_lane_job.p : d_wave_job.p, pk ? 0 : 6,
                           (int)round_trials, g->d_r, N, g->delta, g->far_arg_threshold, d_E.p, d_limit.p, d_start.p, d_us.p, d_us1.p, d_wave_kind.p, d_counters.p, g->uniform,
                           g->Rmax, g->h, queued ? d_queue.p : nullptr, queued ? d_queue + kSweepQueueClasses + 1 : nullptr, nwaves);
        DFTA_CHECK_LAUNCH(ctx);
        if (stats) DFTA_HIP(ctx, hipEventRecord(ev[0], st));
        rc = dfta_launch_sweep(ctx, g, DFTA_SWEEP_COUNT, tables(), blocks(round_waves).view(d_wave_kind), trials(stats).sweep(), stats ? d_counters + 1 : nullptr,
                               queued ? d_queue.p : nullptr, nwaves);
        if (rc) return rc;
        if (stats) DFTA_HIP(ctx, hipEventRecord(ev[1], st));
        if (!pk) {          // packed rounds have no scouts (capz == tcap)
            hipLaunchKernelGGL(k_scout, dim3(njobs), dim3(64), 0, st, d_jobs.p, d_E.p, d_start.p, d_u0.p);
            DFTA_CHECK_LAUNCH(ctx);
        }
        DFTA_HIP(ctx, hipMemsetAsync(d_ndone, 0, sizeof(int), st));
        hipLaunchKernelGGL(k_walk, dim3((p.run_chains + 63) / 64), dim3(64), 0, st, d_jobs.p, p.d_chains, p.run_chains, d_count.p, d_u0.p, d_phi.p, d_istop.p, stats ? d_trip.p : nullptr, d_tab.p, N, d_ndone);
        DFTA_CHECK_LAUNCH(ctx);
        if (early) {
            DFTA_HIP(ctx, hipStreamWaitEvent(st, ev_taken, 0));      // the second stream has consumed the previous snapshot (no-op if none was taken)
            hipLaunchKernelGGL(k_snapshot_done, dim3((njobs + 63) / 64), dim3(64), 0, st, d_jobs.p, njobs, d_snapE.p, d_snapReady.p);
            DFTA_CHECK_LAUNCH(ctx);
            DFTA_HIP(ctx, hipEventRecord(ev_walk, st));
        }
        rc = plan_round(p);
        if (rc) return rc;
        int ndone = 0;
        DFTA_HIP(ctx, hipMemcpyAsync(&ndone, d_ndone, sizeof(int), hipMemcpyDeviceToHost, st));
        if (pk) DFTA_HIP(ctx, hipMemcpyAsync(pack_out, d_pack_out, sizeof(p.pack_out), hipMemcpyDeviceToHost, st));
        DFTA_HIP(ctx, hipStreamSynchronize(st));
        const long this_round = round_trials;
        if (pk) round_trials = pack_out[0];
        if (early && ndone > done_seen && ndone < njobs) {     // some levels have their eigenvalue while others still search
            done_seen = ndone;
            rc = early_match_solves(p);
            if (rc) return rc;
        }
        if (stats) {
            float ms = 0;
            DFTA_HIP(ctx, hipEventElapsedTime(&ms, ev[0], ev[1]));
            p.ms_sweep += ms;
            if (debug_rounds && pk)
                fprintf(stderr, "   packed round %d: %ld trials in %.3f ms; next: %d trials, depth %d, %d jobs searching\n", p.rounds + 1, this_round, ms, pack_out[0], pack_out[1], pack_out[2]);
        }
        ++p.rounds;
        if (debug_rounds) {
            std::vector<Job> dbg(njobs);
            DFTA_HIP(ctx, hipMemcpy(dbg.data(), d_jobs, sizeof(Job) * njobs, hipMemcpyDeviceToHost));
            print_census(dbg, p.rounds, debug_rounds);
        }
        if (ndone >= njobs) break;
    }
    return DFTA_OK;
}

// Wavefunctions: match (the levels that were not matched while the others searched), normalise, accumulate the density
int LevelSolver::finish_wavefunctions(RunPlan& p)
{
    const int N = g->N;
    hipStream_t st = ctx->stream;
    bool normalise = true;
    const int* keep = d_jstart_keep;       // the cut-off index of every job that was matched in this run (-1: frozen, its Psi stands)
    if (p.layout == LAYOUT_PERSIST) normalise = false;       // every live level was matched and normalised by the workgroup that closed its search
    else if (p.layout == LAYOUT_SCAN && p.scan_match_mode) normalise = p.scan_match_mode == 1;     // k_scan_levels has matched (and, with Simpson 3/8, normalised) every live level
    else {
        if (p.early_pending) DFTA_HIP(ctx, hipStreamWaitEvent(st, ev_early, 0));       // the early solves use the same per-job scratch arrays
        hipLaunchKernelGGL(k_job_energies, dim3((njobs + 63) / 64), dim3(64), 0, st, d_jobs.p, njobs, d_jE.p, d_jslot.p, d_jl.p);
        DFTA_CHECK_LAUNCH(ctx);
        int rc = dfta_launch_boundary(ctx, g, job_boundary(), nullptr);
        if (rc) return rc;
        // cut-off index -1 = skipped by k_match: frozen jobs (the result of their last solve stands) and jobs matched already;
        // d_jstart_keep: the cut-off index of every job that was matched in this run (-1: frozen)
        hipLaunchKernelGGL(k_mask_rest, dim3((njobs + 63) / 64), dim3(64), 0, st, d_jobs.p, njobs, d_jstart.p, d_jmatched.p, d_jstart_keep.p);
        DFTA_CHECK_LAUNCH(ctx);
        rc = dfta_launch_match(ctx, g, tables(), job_match(), nullptr);
        if (rc) return rc;
        hipLaunchKernelGGL(k_store_match, dim3((njobs + 63) / 64), dim3(64), 0, st, d_jobs.p, njobs, d_jmp.p, d_jstart_keep.p);
        DFTA_CHECK_LAUNCH(ctx);
        if (!p.nfrozen) keep = nullptr;
    }
    if (normalise) {
        hipLaunchKernelGGL(k_normalize, dim3(njobs), dim3(kNormThreads), 0, st, d_Psi.p, d_Q.p, N, g->d_eh, g->d_cnst, keep, dfta_hstep(g), integ_rule);
        DFTA_CHECK_LAUNCH(ctx);
    }
    if (p.dNewDensity) {
        hipLaunchKernelGGL(k_accumulate_density, dim3(std::min(256, (N + 255) / 256), nV), dim3(256), 0, st, d_Psi.p, d_occ.p, d_v_off.p,
                           N, p.dNewDensity);
        DFTA_CHECK_LAUNCH(ctx);
    }
    return DFTA_OK;
}

int LevelSolver::fill_stats(RunPlan& p, LevelStats* stats)
{
    hipStream_t st = ctx->stream;
    unsigned long long cnt[3];
    DFTA_HIP(ctx, hipMemcpyAsync(cnt, d_counters, sizeof(cnt), hipMemcpyDeviceToHost, st));
    DFTA_HIP(ctx, hipStreamSynchronize(st));
    if (p.layout == LAYOUT_OWN) {
        p.rounds = (int)(cnt[2] & 0xffffffffull);                 // the most rounds a level took
        DFTA_HIP(ctx, hipEventElapsedTime(&p.ms_sweep, ev[0], ev[1]));
    }
    stats->rounds = p.rounds;
    stats->sweeps_issued = static_cast<long>(cnt[0]) + 2L * (njobs - p.nfrozen);    // + inward/outward halves of the match solve
    stats->points_traversed = static_cast<long>(cnt[1]);
    stats->ms_sweep = p.ms_sweep;
    stats->layout = p.layout;
    return DFTA_OK;
}

// Solve all levels for the potentials dV (device, nV*N).
//   job_bottom (host, njobs): BottomEnergy at entry of LocateInterval for every job.  CHAINED uses only the entry
//   of the first job of each potential (-Z^2-1, DFTAtom.cpp:407) and hands E-3 from level to level (DFTAtom.cpp:541);
//   BATCHED starts every level from its own entry (the caller's hint: E_{k-1} of the previous SCF step - 3).
// The engines are tried in order; each either takes every live level to its eigenvalue (p.searched) or leaves the records ready for the
// next one: the scan search (tolerance mode), [the scan predictor,] the device-side search, the own-pace search, the host rounds.
int LevelSolver::run(const double* dV, const double* job_bottom, int run_mode, double* dNewDensity, LevelStats* stats,
                     const unsigned char* frozen)
{
    if (njobs == 0) return DFTA_OK;
    hipStream_t st = ctx->stream;
    RunPlan p;                         // lives to the end of the solve: its vectors are the sources of asynchronous copies
    p.dV = dV; p.dNewDensity = dNewDensity; p.stats = stats != nullptr;
    make_plan(p, run_mode, frozen);
    if (p.sw) {
        DFTA_HIP(ctx, hipMemcpyAsync(d_live, p.live.data(), sizeof(int) * p.live.size(), hipMemcpyHostToDevice, st));
        tables_dirty = true;
    } else if (tables_dirty && !p.use_own) {           // back from latency mode / the own-pace search: the solver's own block tables
        DFTA_HIP(ctx, hipMemcpyAsync(d_wave_job, h_wave_job.data(), sizeof(int) * h_wave_job.size(), hipMemcpyHostToDevice, st));
        DFTA_HIP(ctx, hipMemcpyAsync(d_wave_slot, h_wave_slot.data(), sizeof(int) * h_wave_slot.size(), hipMemcpyHostToDevice, st));
        tables_dirty = false;
    }
    prepare_jobs(p, job_bottom, frozen);
    rank_feedback(p);
    DFTA_HIP(ctx, hipMemcpyAsync(d_jobs, p.jobs.data(), sizeof(Job) * njobs, hipMemcpyHostToDevice, st));
    DFTA_HIP(ctx, hipMemsetAsync(d_counters, 0, sizeof(unsigned long long) * 4, st));
    DFTA_HIP(ctx, hipMemsetAsync(d_jmatched, 0, sizeof(int) * njobs, st));
    if (p.nfrozen == njobs) {          // nothing to solve: Psi, density contributions and job records stand
        DFTA_HIP(ctx, hipStreamSynchronize(st));      // p.jobs is the source of the copy above
        if (stats) *stats = LevelStats();
        return DFTA_OK;
    }
    int rc = dfta_launch_build_tab(ctx, g, d_tab, dV, d_slot_v, d_slot_l, nslots, d_bounds);
    if (rc) return rc;
    if (!p.chained && clamp_bottoms) {
        hipLaunchKernelGGL(k_slot_min, dim3(nslots), dim3(1024), 0, st, d_tab.p, g->N, d_slot_min.p);
        DFTA_CHECK_LAUNCH(ctx);
    }
    rc = clamp_job_bottoms(p);
    if (rc) return rc;

    if (sweep_mode == DFTA_SWEEPS_TOLERANCE && scan_tb.tabv != nullptr) rc = search_scan(p);
    if (!rc && !p.searched) rc = predict_scan(p);
    if (!rc && !p.searched && p.use_persist) rc = search_persist(p);
    if (!rc && !p.searched && p.use_own) rc = search_own(p);
    if (!rc && !p.searched) rc = search_rounds(p);
    if (rc) return rc;
    if (p.rounds >= kMaxRounds) { snprintf(ctx->err, sizeof(ctx->err), "level solver did not terminate"); return DFTA_ERR_NOT_CONVERGED; }

    rc = finish_wavefunctions(p);
    if (rc) return rc;
    return stats ? fill_stats(p, stats) : DFTA_OK;
}

int LevelSolver::fetch_jobs(std::vector<Job>& out)
{
    out.resize(njobs);
    if (njobs == 0) return DFTA_OK;
    DFTA_HIP(ctx, hipMemcpyAsync(out.data(), d_jobs, sizeof(Job) * njobs, hipMemcpyDeviceToHost, ctx->stream));
    DFTA_HIP(ctx, hipStreamSynchronize(ctx->stream));
    h_last = out;            // decision strings of this solve predict the paths of the next one
    return DFTA_OK;
}

}  // namespace dfta

extern "C" int dfta_solve_levels(dfta_ctx* ctx, const dfta_grid* g, int mode, int tree_depth, int nV, const double* V,
                                 const double* bottom0, const double* bottom_hint, int nlevels, const int* vidx, const int* n,
                                 const int* l, const int* occ,
                                 dfta_level_result* results, double* newDensity, double* Eelectronic, double* Psi_out,
                                 long* issued_sweeps)
{
    if (!ctx || !g) return DFTA_ERR_INVALID;
    DFTA_ENTER(ctx);
    DFTA_REQUIRE(ctx, V && bottom0 && n && l && occ && results && nV > 0 && nlevels > 0, "null input");
    const bool scan_sweeps = (mode & DFTA_LEVELS_SCAN_SWEEPS) != 0;
    mode &= ~DFTA_LEVELS_SCAN_SWEEPS;
    DFTA_REQUIRE(ctx, mode == DFTA_LEVELS_CHAINED || mode == DFTA_LEVELS_BATCHED, "mode");
    DFTA_REQUIRE(ctx, !scan_sweeps || dfta_scan_supported(g), "the tolerance mode of the sweeps needs a logarithmic grid of 12 .. 20 multigrid levels");
    const int N = g->N;
    std::vector<dfta::JobSpec> specs(nlevels);
    for (int k = 0; k < nlevels; ++k) specs[k] = {vidx ? vidx[k] : 0, n[k], l[k], occ[k], static_cast<double>(occ[k])};
    dfta::LevelSolver solver;
    solver.sweep_mode = scan_sweeps ? DFTA_SWEEPS_TOLERANCE : DFTA_SWEEPS_EXACT;
    int rc = solver.setup(ctx, g, mode, tree_depth, nV, specs);
    if (rc) { if (rc == DFTA_ERR_INVALID) snprintf(ctx->err, sizeof(ctx->err), "levels must be grouped by potential, l in 0..3"); return rc; }
    hipStream_t st = ctx->stream;
    DevBuf<double> dV, dND;
    DFTA_HIP(ctx, dV.alloc((size_t)nV * N));
    DFTA_HIP(ctx, hipMemcpyAsync(dV.p, V, sizeof(double) * (size_t)nV * N, hipMemcpyHostToDevice, st));
    if (newDensity) {
        DFTA_HIP(ctx, dND.alloc((size_t)nV * N));
        DFTA_HIP(ctx, hipMemcpyAsync(dND.p, newDensity, sizeof(double) * (size_t)nV * N, hipMemcpyHostToDevice, st));
    }
    dfta::LevelStats stats;
    std::vector<double> job_bottom(nlevels);
    for (int k = 0; k < nlevels; ++k) job_bottom[k] = bottom_hint ? bottom_hint[k] : bottom0[specs[k].v];
    solver.clamp_bottoms = (bottom_hint == nullptr);    // explicit hints are taken as given
    rc = solver.run(dV.p, job_bottom.data(), mode, dND.p, &stats);
    if (rc) return rc;
    std::vector<dfta::Job> jobs;
    rc = solver.fetch_jobs(jobs);
    if (rc) return rc;
    if (Eelectronic) for (int v = 0; v < nV; ++v) Eelectronic[v] = 0;
    for (int k = 0; k < nlevels; ++k) {
        const dfta::Job& j = jobs[k];
        results[k].E = j.E; results[k].top = j.top; results[k].bottom = j.bottom; results[k].n_count = j.n_count;
        results[k].n_zero = j.n_zero; results[k].converged = j.converged; results[k].matchPoint = j.matchPoint;
        results[k].status = j.status;
        if (Eelectronic) Eelectronic[j.v] += solver.h_occ[k] * j.E;  // DFTAtom.cpp:561 (h_occ[k] == (double)j.occ)
    }
    if (newDensity) DFTA_HIP(ctx, hipMemcpyAsync(newDensity, dND.p, sizeof(double) * (size_t)nV * N, hipMemcpyDeviceToHost, st));
    if (Psi_out) DFTA_HIP(ctx, hipMemcpyAsync(Psi_out, solver.d_Psi, sizeof(double) * (size_t)nlevels * N, hipMemcpyDeviceToHost, st));
    DFTA_HIP(ctx, hipStreamSynchronize(st));
    if (issued_sweeps) *issued_sweeps = stats.sweeps_issued;
    return DFTA_OK;
}
