// internal.h -- launch helpers shared between the translation units of libdftatom_hip (not part of the ABI).
#pragma once
#include "common.h"

// numerov.hip
// doubles2 per table slot in a `bounds` buffer: the fast-division bounds of the slot + { min, max } of veff per block of points
int dfta_bounds_stride(const dfta_grid* g);
int dfta_launch_build_tab(dfta_ctx* ctx, const dfta_grid* g, double2* tab, const double* dV, const int* d_slot_v,
                          const int* d_slot_l, int nslots, double2* bounds /* nslots, may be null */);
// Views the launch helpers take: device pointers only, nothing owned; filled member by member at the call site.
struct SlotTables {                // the tables of the slots
    const double2* tab;
    const double2* bounds;         // per slot (dfta_bounds_stride), may be null
    const int* slot_l;             // l per table slot (the uniform grid's sweeps need it)
};
struct WaveBlocks {                // the 64-trial blocks of a launch
    const int* slot; const int* first; const int* cnt;
    const int* kind;               // per block DFTA_SWEEP_COUNT / _ZERO, or null: the launch's kind
    int n;
};
struct WaveBlocksRW {              // ... of the searches that write them on the device (own pace: the slots; device-side: all three)
    int* slot; int* first; int* cnt;
    int n;
    WaveBlocks view(const int* kind = nullptr) const { WaveBlocks b; b.slot = slot; b.first = first; b.cnt = cnt; b.kind = kind; b.n = n; return b; }
};
struct SweepTrials {               // per trial, as a sweep launch uses them: inputs read, results written (u0, phi, istop, trip may be null)
    const double *E, *us, *us1; const int *limit, *start;
    double *u0, *phi; int *count, *istop, *trip;
};
struct TrialArrays {               // per trial, all writable: the own-pace and device-side searches fill the inputs themselves
    double *E, *us, *us1, *u0, *phi;
    int *limit, *start, *count, *istop, *trip;
    SweepTrials sweep() const
    {
        SweepTrials t;
        t.E = E; t.us = us; t.us1 = us1; t.limit = limit; t.start = start;
        t.u0 = u0; t.phi = phi; t.count = count; t.istop = istop; t.trip = trip;
        return t;
    }
};
// uniform grid only: for_match, l and uz -- the match solve re-derives its step from the truncated step count, so its second start value
// differs from a sweep's, and it needs GetBoundaryValueZero(h', l) per trial (Numerov.h:430,475); l and uz null: none
struct BoundaryTrials {
    const double* E; int n;
    int* start; double *us, *us1;
    int for_match; const int* l; double* uz;
};
struct MatchTrials {
    const int* slot; const double* E; const int* start; const double *us, *us1; const int* l;
    const double* uz;              // uniform grid: start value at the first node per trial
    double *Psi, *Q; int* match_point;
    int n;
};
// stream: nullptr = the context's stream (the early match solves of levels.hip run on a second one)
int dfta_launch_boundary(dfta_ctx* ctx, const dfta_grid* g, const BoundaryTrials& t, hipStream_t stream);
int dfta_launch_match(dfta_ctx* ctx, const dfta_grid* g, const SlotTables& tables, const MatchTrials& t, hipStream_t stream);
// flag in SweepArgs::istop (numerov.hip): the sweep left CountNodes because the count exceeded the limit
constexpr int kStopOver = 0x40000000;
// Balanced launch of the fused sweeps: the blocks of a round are entered into kSweepQueueClasses lists by expected length, and the launch's
// waves (two per SIMD, all resident) take them longest first through one ticket counter -- see k_sweep_queue
constexpr int kSweepQueueClasses = 16;
// total_trips: optional global counter (points traversed); queue: the round's work queue (k_expand of levels.hip), lists of qcap blocks, or null
int dfta_launch_sweep(dfta_ctx* ctx, const dfta_grid* g, int kind, const SlotTables& tables, const WaveBlocks& blocks, const SweepTrials& trials,
                      unsigned long long* total_trips, const int* queue, int qcap);
bool dfta_sweep_is_fused(const dfta_ctx* ctx, int nblocks);

// persist.inc (compiled with numerov.hip): the exact level search of up to 64 levels on the device, every level at its own pace
namespace dfta { struct Job; }
struct dfta_persist_buffers {
    DevBuf<unsigned char> d_ctl;   // control block, mailboxes, per-level workgroup lists, trace
    size_t ctl_bytes = 0;
    DevBuf<double> E, us, us1, u0, phi;            // trial arrays: nlive_cap x tmax
    DevBuf<int> limit, start, count, istop, trip;
    DevBuf<double> candP, candQ;   // per workgroup: wavefunction + scratch of a speculative match (null: none)
    DevBuf<int> blk;               // per workgroup: table slot, first trial, trial count of its running block
    int nblocks = 0, tmax = 0, nlive_cap = 0, trace_cap = 0;
    // $DFTA_DEBUG knobs, read when the buffers are made (as every other knob of a solver)
    int fault_block = -1;          // FAULT_PERSIST_WORKER: this workgroup drops its first block (tests)
    double timeout_ms = 0;         // LEVELS_PERSIST_TIMEOUT_MS (0: from the grid size)
    bool plain_launch = false;     // LEVELS_PERSIST_PLAIN_LAUNCH: no cooperative launch
    bool equal_shares = false;     // LEVELS_PERSIST_EQUAL: node-less levels keep their whole share
    bool want_trace = false;       // LEVELS_PERSIST_TRACE
    std::vector<unsigned char> h_stage;
    void reset()                   // frees the buffers; sizes and knobs as constructed
    {
        for (DevBuf<double>* b : {&E, &us, &us1, &u0, &phi, &candP, &candQ}) b->reset();
        for (DevBuf<int>* b : {&limit, &start, &count, &istop, &trip, &blk}) b->reset();
        d_ctl.reset();
        ctl_bytes = 0; nblocks = tmax = nlive_cap = trace_cap = 0;
        fault_block = -1; timeout_ms = 0; plain_launch = equal_shares = want_trace = false;
        h_stage.clear();
    }
    TrialArrays trials() const
    {
        TrialArrays t;
        t.E = E; t.us = us; t.us1 = us1; t.u0 = u0; t.phi = phi;
        t.limit = limit; t.start = start; t.count = count; t.istop = istop; t.trip = trip;
        return t;
    }
    WaveBlocksRW blocks() const;   // the three parts of blk (numerov.hip)
};
int dfta_persist_create(dfta_ctx* ctx, const dfta_grid* g, int nlive_cap, dfta_persist_buffers* pb);     // (re)creates: frees what pb held
struct PersistRun {
    double *Psi, *Q; int* jstart_keep;
    unsigned long long* counters;
    bool stats; int nopredict, integ_rule;
    const double* tuning;          // host: noise rel, abs, secant, kappa
    int fixed_point;
    const int* share;              // host, nlive: workgroups per level (null: equal shares)
    int deep_reserve;              // workgroups the pool keeps for the levels marked Job::deep == 2
    bool want_trace;
};
struct PersistResult {
    int rounds = 0;
    int aborted = 0;               // 1: a worker was lost (time-out) -- nothing is valid, the caller repeats the solve with host rounds
    std::vector<unsigned long long> trace;      // want_trace: 4 words per closed round
};
// live (host): indices into jobs, whose records carry phase = first bisection, tbase = position in `live` x pb->tmax
int dfta_launch_levels_persist(dfta_ctx* ctx, const dfta_grid* g, dfta_persist_buffers* pb, dfta::Job* jobs, const int* live, int nlive,
                               const SlotTables& tables, const PersistRun& run, PersistResult* out);

// own.inc (compiled with numerov.hip): the exact level search of a batch on the device, one workgroup of W waves per live level, one
// ordinary launch; counters[0] += issued trials, [1] += traversed points (stats), [2] = max rounds of a level (as unsigned int)
struct OwnOptions { bool stats; int nopredict, spine_cap; };
struct OwnLevels {
    dfta::Job* jobs;
    const int* live;               // device, may be null: level q = job q; the records carry phase = first bisection, tbase = q * 64 W
    int nlive, W;
};
// the trial arrays are the level solver's own (room for nlive * 64 W trials; blocks.first[b] = 64 b, blocks.cnt[b] = 64)
int dfta_launch_levels_own(dfta_ctx* ctx, const dfta_grid* g, const OwnLevels& levels, const SlotTables& tables, const WaveBlocksRW& blocks,
                           const TrialArrays& trials, unsigned long long* counters, const OwnOptions& opt);

// scan.hip: the tolerance mode of the sweeps (transfer-matrix scan: one workgroup per trial)
struct dfta_scan_tables {
    double* tabv = nullptr;    // nslots * N: veff = V + c_l per slot, lane-interleaved (row i = t C + k at k 512 + t, row N-1 at N-1)
    DevBuf<double2> mm;        // nslots * 512: {min, max} of veff over a lane's rows
    DevBuf<double> Atop;       // 513: A = 2 Rp^2 delta^2 exp(2 i delta) of every lane's top row (and of row N-1)
    double* T = nullptr;       // C: exp(-2 delta (C-1-k))
    // tabv and T point kScanPadRows rows / 8 entries INTO their allocations: the row loops issue the loads of the next batches
    // unconditionally (rows below row 0 of slot 0, entries below T[0]: read, never used) -- no clamps, no branches in the loops
    DevBuf<double> tabv_alloc, T_alloc;
    int nslots = 0;
    void reset() { tabv_alloc.reset(); T_alloc.reset(); mm.reset(); Atop.reset(); tabv = T = nullptr; nslots = 0; }
};
int dfta_scan_supported(const dfta_grid* g);
int dfta_scan_tables_create(dfta_ctx* ctx, const dfta_grid* g, int nslots, dfta_scan_tables* tb);     // tb: empty (as constructed)
int dfta_launch_scan_build_tab(dfta_ctx* ctx, const dfta_grid* g, const dfta_scan_tables& tb, const double* dV, const int* d_slot_v, const int* d_slot_l);
int dfta_launch_scan_sweeps(dfta_ctx* ctx, const dfta_grid* g, int kind, int ntrials, const dfta_scan_tables& tb, const int* d_trial_slot,
                            const double* dE, const int* dLimit, int* dCount, double* dU0, int* dStart, int* dTrip, int* dBad);

// reduce.hip: Integral::{Trapezoid,SimpsonOneThird,Simpson38,Boole,Romberg} (Integral.h:11-155) with the reference's
// sequential summation order, one wave per vector: out[k] = rule(delta, vals + k*stride) for k < nvec
int dfta_launch_integrate_ordered(dfta_ctx* ctx, int rule /* DFTA_INT_* */, double delta, const double* dVals, int n, int nvec,
                                  size_t stride, double* dOut);
// Simpson 3/8 (Integral.h:50-73) with its two sums taken in parallel (tolerance mode of the sweeps: the normalisation integral of
// scan_match is summed that way too); same weights, a different order of additions
int dfta_launch_integrate_simpson38_parallel(dfta_ctx* ctx, double delta, const double* dVals, int n, int nvec, size_t stride, double* dOut);
int dfta_integral_shape_ok(int rule, int sz);

// mixing.hip: Anderson density mixing (dfta_scf_options::mixing), three ordinary launches in place of k_mix
constexpr int kAndersonMaxHistory = 8;
constexpr int kAndersonDots = kAndersonMaxHistory * (kAndersonMaxHistory + 1) / 2 + kAndersonMaxHistory;   // A's upper triangle, then b
constexpr int kAndersonChunk = 1024;       // nodes per workgroup of k_anderson_gram: the chunking is a function of N alone
constexpr int kAndersonStateInts = 8;      // per atom: ring head, length, steps taken | this step's head, length, use flag
constexpr int kAndersonCoefDoubles = kAndersonMaxHistory;
struct dfta_anderson {
    int m = 0, warmup = 0;                 // pairs kept per atom, linear steps before the first accelerated one
    DevBuf<double> ring;                   // [potential][slot < m][x, f][N]
    DevBuf<double> slab;                   // [atom][chunk][kAndersonDots]: the chunks' partial dot products
    DevBuf<double> gamma;                  // [atom][kAndersonCoefDoubles]
    DevBuf<int> state;                     // [atom][kAndersonStateInts]
};
inline int dfta_anderson_chunks(int N) { return (N + kAndersonChunk - 1) / kAndersonChunk; }
int dfta_anderson_create(dfta_ctx* ctx, const dfta_grid* g, int natoms, int nspin, int history, int warmup, dfta_anderson* an);
// newDensity: the level search's Sum f Psi^2 of every potential (in), the output density g (out); density / dA / dB: the step's input
// density (in), the mixed one (out); fin: per atom, finished (skipped)
int dfta_launch_anderson_mix(dfta_ctx* ctx, const dfta_grid* g, dfta_anderson* an, int lsda, int natoms, double alpha, double oneMinusAlpha,
                             double* newDensity, double* density, double* dA, double* dB, const int* fin);
// orbitals.hip: expectation values and r^k matrix elements of orbitals u = r R (device pointers; include/dftatom_hip.h has the definitions)
constexpr int kOrbitalMatrixMax = 32;      // orbitals of one matrix: the levels of a spin channel (plan_scf_config allows 32)
struct dfta_orbital_scratch {              // of dfta_launch_orbital_matrix, for up to norb_max orbitals
    int norb_max = 0;
    DevBuf<double> slab;                   // [chunk][pair a <= b]: the chunks' partial sums
    DevBuf<double> M;                      // norb x norb
    DevBuf<unsigned> ticket;               // 0 between launches
};
int dfta_orbital_scratch_create(dfta_ctx* ctx, const dfta_grid* g, int norb_max, dfta_orbital_scratch* sc);
// props: norb x DFTA_ORB_PROPS; records the launch's time for dfta_ctx_last_kernel_ms
int dfta_launch_orbital_properties(dfta_ctx* ctx, const dfta_grid* g, int norb, const int* dL, const double* dU, double* dProps);
int dfta_launch_orbital_matrix(dfta_ctx* ctx, const dfta_grid* g, int norb, const double* dU, int k, double* dSlab, unsigned* dTicket, double* dM);
// slater.hip: Slater integrals R^k(ab,cd) of orbitals u = r R (device pointers; jobs: rows a,b,c,d,k, validated by the caller --
// slater_plan.h: check_jobs); records the launch's time for dfta_ctx_last_kernel_ms
int dfta_launch_slater_rk(dfta_ctx* ctx, const dfta_grid* g, const double* dU, int njobs, const int* dJobs, double* dR);
struct dfta_slater_scratch {               // job table and results on the device: empty until the first run, grown as needed
    DevBuf<int> d_jobs;
    DevBuf<double> d_R;
    // uploads the table (host), launches, copies the njobs results to R (host) and synchronises
    int run(dfta_ctx* ctx, const dfta_grid* g, const double* dU, int njobs, const int* jobs, double* R);
};
// exchange.hip: screening functions y^k_xy and the exchange potentials of a spin channel (device pointers; jobs: rows x,y,k, validated
// by the caller -- exchange_plan.h: check_jobs)
namespace dfta_exchange { struct ChannelPlan; }
int dfta_launch_screening_yk(dfta_ctx* ctx, const dfta_grid* g, const double* dU, int njobs, const int* dJobs, double* dY);
struct dfta_exchange_scratch {             // tables, y rows and the channel's rows on the device: empty until the first run, grown as needed
    DevBuf<int> d_jobs, d_first, d_tab, d_red;
    DevBuf<double> d_y;                    // njobs x N: 1 MB per job at 131 073 nodes
    DevBuf<double> d_X, d_rows;            // norb x N; D, vS, vKLI
    DevBuf<double> d_occ, d_coef, d_redout;
    int upload_jobs(dfta_ctx* ctx, const dfta_grid* g, int njobs, const int* jobs);
    // uploads the table (host), launches, copies the njobs x N rows to y (host) and synchronises; records the launch's time
    int run_yk(dfta_ctx* ctx, const dfta_grid* g, const double* dU, int njobs, const int* jobs, double* y);
    // the whole sequence of dfta_exchange_potentials for a planned channel (occ, outputs: host; any output may be null); the events of
    // dfta_ctx_last_kernel_ms bracket it
    int run_potentials(dfta_ctx* ctx, const dfta_grid* g, const double* dU, const dfta_exchange::ChannelPlan& plan, const double* occ, int homo,
                       double* X, double* D, double* vS, double* vKLI, double* vbar, double* M);
};
// bessel.hip: Bessel transforms of radial arrays (device pointers; dRows: nrow device addresses of N doubles each; kind, l and q
// validated by the caller -- bessel_plan.h: check_transform); dOut: nrow x nq; records the launch's time for dfta_ctx_last_kernel_ms
int dfta_launch_bessel_transform(dfta_ctx* ctx, const dfta_grid* g, int kind, int nrow, const int* dL, const double* const* dRows, int nq,
                                 const double* dQ, double* dOut);
struct dfta_bessel_scratch {               // the tables of a transform and its results on the device: empty until the first run, grown as needed
    DevBuf<int> d_l;
    DevBuf<const double*> d_rows;
    DevBuf<double> d_q, d_out;
    // uploads l, the rows' device addresses and q (host arrays), launches, copies the nrow x nq results to out (host) and synchronises
    int run(dfta_ctx* ctx, const dfta_grid* g, int kind, int nrow, const int* l, const double* const* rows, int nq, const double* q, double* out);
};
// continuum.hip: the outward sweeps of a validated call (continuum_plan.h: check) on potentials dV (nV x N) and partner rows dP
// (npartner_rows x N) that are on the device; the call's arrays and every output are host pointers (any output may be null).  Plans,
// launches, copies the results back in the order of the call and synchronises; records the launches' time for dfta_ctx_last_kernel_ms
namespace dfta_continuum_plan { struct Call; }
struct dfta_continuum_out {
    double* logderiv; int* nodes; double *delta_or_phase, *scale; int* status;
    double *sums, *rows;           // ntrials x 16; ntrials x N
};
int dfta_continuum_run(dfta_ctx* ctx, const dfta_grid* g, const dfta_continuum_plan::Call& c, const double* dV, const double* dP,
                       const dfta_continuum_out& out);
// pseudo.hip: the pseudization of nch validated channels (pseudo_plan.h: check) whose rows dV, dU and tables dL, dEps,
// dIc are on the device; every output is a host pointer and may be null.  One launch; copies the results back and synchronises;
// records the launch's time for dfta_ctx_last_kernel_ms
struct dfta_pseudize_out {
    double *u_ps, *V_ps;           // nch x N
    double *coef, *rc, *match;     // nch x DFTA_PS_COEF, nch, nch x DFTA_PS_MATCH
    int *iters, *status;
};
// dVrow, dUrow (device, may be null): per channel the row of dV and of dU that it reads -- resident rows are read in place
int dfta_pseudize_run(dfta_ctx* ctx, const dfta_grid* g, int nch, const double* dV, const int* dVrow, const double* dU, const int* dUrow,
                      const int* dL, const double* dEps, const int* dIc, const dfta_pseudize_out& out);
// kli_stage.hip: the budget of a chunk's y rows in MiB: DFTA_DEBUG KLI_Y_MB, or the default
double dfta_kli_budget_mb();
// scf.hip: the k_mix launch (DFTA_MIX_LINEAR), same arguments
int dfta_launch_linear_mix(dfta_ctx* ctx, const dfta_grid* g, int lsda, int natoms, double alpha, double oneMinusAlpha, double* newDensity,
                           double* density, double* dA, double* dB, const int* fin);
