// levels.h -- device-resident eigenvalue search shared by dfta_solve_levels and the SCF driver.
#pragma once
#include <vector>

#include "common.h"
#include "internal.h"
#include "scf_config.h"     // JobSpec

namespace dfta {

// state of one (potential, level) eigenvalue search; lives in device memory
struct Job {
    double toe, boe;        // current interval of the running bisection (Top / Bottom)
    double bottom0;         // BottomEnergy at entry of LocateInterval
    double top, bottom;     // interval returned by LocateInterval
    double E;               // eigenvalue
    int v, n, l, occ, nodes, slot;
    int phase;
    int haveSgn, sgnBottom, iter3, converged;
    int n_count, n_zero, matchPoint;
    // path prediction (speculation only, never changes a decision): the decision strings of the three bisections in
    // the previous SCF step and how many of their leading bits held in the step before -- the next round evaluates
    // that many nodes along the predicted path (a "spine") and hangs the full speculative tree at its end
    unsigned long long pred_bits[3], cur_bits[3];
    int pred_len[3], cur_len[3], trust[3];
    int phase_done;         // decisions already taken in the running phase
    int spine;              // spine length of the trial layout of the current round
    // Predictions from the structure of the problem (speculation only).  A node enters the inward solution through
    // r = 0 exactly when u(0) changes sign, i.e. at an eigenvalue.  Hence (i) the energy at which the count reaches
    // `nodes` -- the end point of the SECOND bisection -- is where the count of the level with one node less (same
    // potential and l: job `sib`) exceeds nodes-1, which is the end point of ITS first bisection; (ii) the sign change
    // of the THIRD bisection lies at the upper end of its interval, the end point of the job's own first bisection.
    int sib;                // job of (v, n-1, l), or -1
    unsigned long long sp_bits;      // predicted decisions of the running phase (bit k = decision k of the phase) ...
    int sp_len;                      // ... valid for decisions < sp_len
    int use_sp;                      // the spine of this round follows sp_bits instead of pred_bits
    int miss;                        // a spine of the running phase mispredicted: no more spines in this phase
    // l > 0: the sign change of u(0) lies INSIDE the band between the two count thresholds (the count stops at the inner
    // turning point).  While the first two bisections run, the upper half of the job's trials (indices >= capz, whole
    // 64-trial blocks of kind ZERO) samples u(0) inside the part of the band that is already certain, then inside the
    // bracket of the sign change; the third bisection is predicted from that bracket.
    int capz;                        // trials [0, capz) = probe + spine + tree, [capz, tpj) = scouts (0: all tpj)
    double se_lo, se_hi;
    int se_state, se_sl, se_stop;    // bracketed? / sign of u(0) at se_lo / no longer shrinking
    double se_plo, se_phi;           // u(0) at se_lo / se_hi (NaN: unknown)
    double se_tlo, se_thi;           // secant estimate of the sign change inside the bracket, with its error bound
    int se_tok;
    // First bisection: every counted trial also reports where it stopped and how far the nearest zero of u was from that
    // point (SweepArgs::phi / istop, numerov.hip) -- a smooth function of E that crosses 0 where the count changes.  The
    // last sample on either side of the running bisection and the most recently replaced one give a secant estimate of
    // the end point with an error bound from the second divided difference: the next round's spine follows it.
    double sc_e[3], sc_phi[3];       // [0]: count <= nodes side (boe), [1]: count > nodes side (toe), [2]: replaced sample
    int sc_is[3];                    // istop of the samples (-1: none)
    double sc_lo, sc_hi;             // predicted bracket of the end point
    int sc_ok;
    // History: the end points of the three bisections in the previous SCF step (top, bottom, E) and how far each had moved
    // against the step before.  The potential changes by about half as much every step (mixing), so this step's end
    // point lies within a few times that distance of the last one: the spine follows the bisection while its midpoints
    // stay outside that bracket.  (Replaces the bit-prefix rule -- "as many leading decisions as matched last time" --
    // once two steps of history exist: a level close to a coarse bisection boundary flips an early decision now and then,
    // and a miss on the spine forfeits the round's tree.)
    double hist_T[3], hist_d[3];
    // Round 5: with linear mixing the end points converge geometrically -- the movement of one step is a nearly constant multiple q of the
    // previous one (Rn: q = 0.47 .. 0.49 from step 10 on, the extrapolated point T + q d is off by < 0.01 |d|; Cu LSDA alternates, q = -0.7).
    // hist_s: signed last movement, hist_q: its ratio to the one before (NaN: unknown); hist_c +- hist_w: the bracket the spine is
    // planned from -- T +- 2 |d| without ratios, T + q d +- (0.2 + 4 |q - q_prev|) |d| with them (levels.hip; 2 - 3 more predicted
    // decisions per first round than the two-step rule, profiles/history_brackets.py).
    double hist_s[3], hist_q[3], hist_c[3], hist_w[3];
    int hist_ok;                     // 0: none, 1: end points only, 2: end points and distances (3: and ratios)
    int frozen;                      // the job's atom has finished its SCF: the result of its last solve stands, nothing is integrated
    // Trial slots of the job in the current round: [tbase, tbase + tcap).  Static (k * tpj, tpj) when the launch fills the
    // machine; re-allotted every round by k_allot when a handful of jobs leave compute units idle (levels.hip).
    int tbase, tcap;
    int n_fixed;                     // iterations of the third bisection counted in n_zero but not integrated: the bisection stood on a fixed point (walk_job)
    int status;                      // DFTA_LEVEL_* bits: how the third bisection ended (DFTAtom.cpp:517-539)
    // device-side search (persist.inc): the certain part of the band (count == nodes) as the planner of the round saw it -- the scouts'
    // grid; the workers of a round must not read a sibling's record while it moves -- and the rounds this job has taken
    double sb_lo, sb_hi;
    int rounds;
    // feedback from one SCF step to the next (device-side search): when the level's search ended, in microseconds after the kernel's first
    // workgroup started; the host gives the levels that ended last in the previous step first call on the pool's workgroups (deep = 1)
    int t_end_us, deep;
    int cand_hist;                   // hit-rate budget of the level's candidate wavefunctions (persist.inc: cand_allowed), carried over by the host
    long long n_points;              // grid points traversed by the sweeps ON the bisection path (n_count + n_zero executed ones) + the match solve
};

// how the levels of a run were searched (LevelStats::layout, dfta_step_stats::levels_layout: the values are part of the ABI)
enum LevelLayout {
    LAYOUT_STATIC = 0,         // host rounds: one static block of trials per job
    LAYOUT_LATENCY = 1,        // host rounds: latency mode (k_allot re-allots the trial slots among the active jobs)
    LAYOUT_PACKED = 2,         // host rounds: packed (k_pack)
    LAYOUT_LATENCY_LIVE = 3,   // host rounds: latency mode over the live jobs of a batch
    LAYOUT_SCAN = 4,           // the scan search (tolerance mode of the sweeps)
    LAYOUT_PERSIST = 5,        // the device-side search (persist.inc)
    LAYOUT_OWN = 6,            // the own-pace search (own.inc)
};

struct LevelStats {
    int rounds = 0;
    long sweeps_issued = 0;
    long points_traversed = 0;
    float ms_sweep = 0;          // HIP-event time summed over the sweep launches
    int layout = 0;              // LevelLayout: 0 static blocks, 1 latency mode, 2 packed rounds, 3 latency mode over the live jobs of a batch,
                                 // 4 scan search, 5 device-side search, 6 own-pace search
};

struct RunPlan;                  // levels.hip: what one run() has decided, handed from phase to phase

struct LevelSolver {
    dfta_ctx* ctx = nullptr;
    const dfta_grid* g = nullptr;
    int mode = 0, nV = 0, njobs = 0, nchains = 0, nchains_chained = 0, depth = 0, tpj = 0, nwaves = 0, nslots = 0;
    long ntrials = 0;
    bool clamp_bottoms = true;     // BATCHED runs: bracket bottoms clamped to max(bottom, min Veff_l)
    std::vector<Job> h_jobs_template;
    std::vector<Job> h_last;       // job records of the previous solve (source of the path predictions)
    bool use_prediction = true;
    int debug_rounds = 0;          // $DFTA_DEBUG_ROUNDS, read once in setup()
    int integ_rule = DFTA_INT_SIMPSON38;   // quadrature of the normalisation integral (the reference calls Simpson38: DFTAtom.cpp:27,51)
    DevBuf<Job> d_jobs;
    std::vector<double> h_occ;     // per job: JobSpec::docc (Job keeps its int occ: persist.inc / own.inc copy Job as 8-byte words)
    DevBuf<double> d_occ;
    DevBuf<int> d_chain_off, d_chain_off_b, d_v_off, d_slot_v, d_slot_l;
    DevBuf<double2> d_tab;
    DevBuf<double> d_E, d_us, d_us1, d_u0, d_phi;
    DevBuf<int> d_limit, d_start, d_count, d_istop, d_trip;
    DevBuf<int> d_wave_kind, d_wave_slot, d_wave_first, d_wave_cnt, d_wave_job;
    bool dynamic = false;          // trial slots re-allotted among the active jobs every round (few jobs: latency mode)
    // a static / packed solver whose live jobs have dropped to <= 64 (frozen atoms) runs its rounds in latency mode (k_allot over d_live)
    bool can_switch = false, tables_dirty = false;
    long static_trials = 0, budget_trials = 0;
    DevBuf<int> d_live;
    std::vector<int> h_wave_job, h_wave_slot;
    // packed rounds (batches): the trials of a round laid out job after job inside their (table slot, kind) group by k_pack
    bool packed = false;
    int pack_dmin = 3, pack_dmax = 12, pack_lanes_small = 0, pack_dsmall = 3, pack_lanes_large = 0;
    DevBuf<int> d_lane_job, d_slot_off, d_slot_jobs, d_gsz, d_goff, d_pack_out;
    DevBuf<unsigned long long> d_counters;      // [0] issued trials, [1] traversed points, [2] scratch
    DevBuf<double> d_Psi, d_Q;                   // njobs*N each
    DevBuf<double> d_jE, d_jus, d_jus1;
    DevBuf<int> d_jslot, d_jl, d_jstart, d_jmp;
    DevBuf<double> d_slot_min;      // per table slot: min_i Veff_l(i)
    DevBuf<double2> d_bounds;       // per table slot: fast-division range bounds (numerov.hip)
    DevEvent ev[2];
    // Early match solves (latency mode): a level whose search has ended is matched on a second stream while the remaining levels'
    // last rounds run -- the outer levels, whose outward streams are the long ones, end a round or two before the core levels.
    DevStream st2;
    DevEvent ev_walk, ev_early, ev_taken;
    DevBuf<int> d_jmatched, d_jstart_keep;
    DevBuf<double> d_snapE;             // snapshot of the jobs' eigenvalues / "search ended" flags, taken on the first stream after every walk
    DevBuf<int> d_snapReady, d_jtake;
    bool early_match = false;
    // Tolerance mode of the sweeps (scan.hip; DFTA_SWEEPS_TOLERANCE, set before setup()): interleaved tables per slot, per-lane {min, max}
    int sweep_mode = DFTA_SWEEPS_EXACT;
    dfta_scan_tables scan_tb;
    DevBuf<int> d_scan_live;                      // live jobs of a grouped scan search
    DevBuf<unsigned long long> d_scan_xch;        // 32 words per job: the members' results of a round, two parities
    int scan_group = 1;             // workgroups per level of the last scan search (1, 3, 7 or 15)
    int scan_predict = 0;           // $DFTA_DEBUG LEVELS_SCAN_PREDICT (measurements): the scan's first bisection predicts the exact search's first spines
    double scan_predict_factor = 1.5, scan_predict_shift = 0.0;
    DevBuf<Job> d_jobs_scan;        // ... on a copy of the records
    DevBuf<unsigned long long> d_counters_scan;
    int scan_fallbacks = 0;         // solves the scan handed back to the exact kernels (a trial it could not decide)
    // Device-side exact search (persist.inc): up to 64 live levels of an un-chained solve on the logarithmic grid run their three bisections in ONE
    // persistent kernel, every level at its own pace; the host rounds of run() remain for everything else and as the fallback
    bool persist_ok = false;        // the solver's shape allows it (decided in setup(); $DFTA_DEBUG LEVELS_NOPERSIST switches it off)
    dfta_persist_buffers pb;
    int persist_fallbacks = 0;      // solves repeated with host rounds after a lost worker
    int persist_deep_reserve = 0;   // workgroups of the pool kept for the levels that ended last in the previous steps
    std::vector<int> persist_tend;  // per job: 3 x the search-end times of the last three device-side solves [us] (0: none) -- the feedback ranks by their maximum
    int persist_runs = 0;
    // Own-pace search of a batch (own.inc): more than 64 live levels, one workgroup of W waves per level, one ordinary launch
    bool own_ok = false;
    int own_waves = 2048, own_wmax = 8, own_spine_cap = -1, own_last_W = 0;
    DevBuf<int> d_own_live;
    // balanced launch of the fused sweeps (numerov.hip:k_sweep_queue): [0, C) entries per length class, [C] the ticket counter, then C lists of nwaves blocks
    DevBuf<int> d_queue;
    double tuning[4] = {1e-11, 16e-12, 1.5e-11, 0.25};     // noise band (rel, abs, secant) and the secant's kappa, as set in setup()
    int fixed_point = 1;
    // history bracket of the first spines (Job::hist_c / hist_w): extrapolation with the last movement ratio ($DFTA_DEBUG LEVELS_NOEXTRAP: the
    // two-step rule only; LEVELS_EXTRAP="a:b": half width (a + b |q - q_prev|) |d|)
    bool hist_extrapolate = true;
    double hist_kA = 0.2, hist_kB = 4.0;
    std::vector<unsigned long long> persist_trace;          // $DFTA_DEBUG LEVELS_PERSIST_TRACE: 4 words per closed round of the last run

    LevelSolver() = default;    // the device buffers, the stream, the events, scan_tb and pb own themselves
    LevelSolver(const LevelSolver&) = delete;
    LevelSolver& operator=(const LevelSolver&) = delete;
    int persist_cap = 256;      // live levels the device-side search takes (LEVELS_PERSIST_WIDE=n: 64 .. 256)
    // once per solver
    int setup(dfta_ctx* c, const dfta_grid* grid, int mode, int tree_depth, int nV, const std::vector<JobSpec>& specs);
    // frozen (host, njobs, may be null): jobs whose result of the previous run() stands (finished atoms of an SCF batch)
    int run(const double* dV, const double* job_bottom, int run_mode, double* dNewDensity, LevelStats* stats,
            const unsigned char* frozen = nullptr);
    int fetch_jobs(std::vector<Job>& out);

    // views of the solver's buffers for the launch helpers (internal.h): every buffer is named here, once
    SlotTables tables() const
    {
        SlotTables t;
        t.tab = d_tab; t.bounds = g->uniform ? nullptr : d_bounds.p; t.slot_l = d_slot_l;
        return t;
    }
    WaveBlocksRW blocks(int n) const
    {
        WaveBlocksRW b;
        b.slot = d_wave_slot; b.first = d_wave_first; b.cnt = d_wave_cnt; b.n = n;
        return b;
    }
    TrialArrays trials(bool with_trips) const          // (the loop iterations per trial are diagnostics: written with the statistics only)
    {
        TrialArrays t;
        t.E = d_E; t.us = d_us; t.us1 = d_us1; t.u0 = d_u0; t.phi = d_phi;
        t.limit = d_limit; t.start = d_start; t.count = d_count; t.istop = d_istop; t.trip = with_trips ? d_trip.p : nullptr;
        return t;
    }
    // the match solves' per-job arrays (uniform grid: the start value at the first node, one per job, lies in d_Q)
    BoundaryTrials job_boundary() const
    {
        BoundaryTrials t;
        t.E = d_jE; t.n = njobs; t.start = d_jstart; t.us = d_jus; t.us1 = d_jus1; t.for_match = 1; t.l = d_jl; t.uz = d_Q;
        return t;
    }
    MatchTrials job_match() const
    {
        MatchTrials t;
        t.slot = d_jslot; t.E = d_jE; t.start = d_jstart; t.us = d_jus; t.us1 = d_jus1; t.l = d_jl; t.uz = d_Q;
        t.Psi = d_Psi; t.Q = d_Q; t.match_point = d_jmp; t.n = njobs;
        return t;
    }

private:
    // the phases of run(), in their order (levels.hip)
    void make_plan(RunPlan& p, int run_mode, const unsigned char* frozen) const;
    void host_round_slots(const RunPlan& p, int k, Job& j) const;
    void prepare_jobs(RunPlan& p, const double* job_bottom, const unsigned char* frozen) const;
    void rank_feedback(RunPlan& p);
    int clamp_job_bottoms(const RunPlan& p), restore_jobs_for_rounds(RunPlan& p);
    int search_scan(RunPlan& p), predict_scan(RunPlan& p), search_persist(RunPlan& p), search_own(RunPlan& p);
    int plan_round(const RunPlan& p), early_match_solves(RunPlan& p), search_rounds(RunPlan& p);
    int finish_wavefunctions(RunPlan& p), fill_stats(RunPlan& p, LevelStats* stats);
};

}  // namespace dfta

// scan.hip: LocateInterval + the u(0) bisection of every chain of jobs by one workgroup each; counters[0] += executed sweeps,
// counters[1] += traversed points, counters[3] |= 1 when a sweep could not be decided by the scan
int dfta_launch_scan_levels(dfta_ctx* ctx, const dfta_grid* g, dfta::Job* d_jobs, const int* d_chain_off, int nchains, int chained,
                            const dfta_scan_tables& tb, int fixed_point, unsigned long long* d_counters,
                            int match_mode /* 0 none, 1 match, 2 match + Simpson-3/8 normalisation */, double* d_Psi, int* d_jstart_keep);
// K = 3, 7 or 15 workgroups per live job (un-chained brackets); DFTA_ERR_NOT_CONVERGED: the grid cannot be co-resident (use the one above)
int dfta_launch_scan_levels_group(dfta_ctx* ctx, const dfta_grid* g, dfta::Job* d_jobs, const int* d_live, int nlive, int K, const dfta_scan_tables& tb,
                                  int fixed_point, unsigned long long* d_counters, unsigned long long* d_xch, int match_mode, double* d_Psi, int* d_jstart_keep);
