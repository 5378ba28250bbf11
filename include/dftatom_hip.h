/*
 * dftatom_hip.h -- C ABI of the MI355X (gfx950) radial-DFT inner loop.
 *
 * Drop-in boundary for the numerical core of aromanro/DFTAtom.  The reference has no FFI; its seam is
 * the public C++ surface of DFT::Numerov / DFT::PoissonSolver / DFT::VWNExchCor / DFT::Integral /
 * DFT::DFTAtom.  Every entry point below names the reference interface it replaces
 * (file:line under /root/reference/DFTAtom).  dftatom_amd/compat/ holds C++ classes with the reference's
 * names and signatures that forward to this ABI.
 *
 * Conventions
 *   - plain C types only; every function returns an int status (DFTA_OK == 0) and never throws;
 *   - all floating point is IEEE fp64; kernels are built with -ffp-contract=off and use only + - * / sqrt on
 *     values, with exp() tables built on the host exactly as the reference evaluates them (the Bessel transforms, which the
 *     reference does not have, also call the device's sin and cos; the continuum block's normalisation also atan2 and hypot);
 *   - `_dev` functions take DEVICE pointers and are asynchronous on the context's stream;
 *     functions without the suffix take HOST pointers, copy, run the same kernels and synchronise;
 *   - one in-flight call per context (the reference is single threaded: DFTAtomFrame.cpp:176-198);
 *   - there is NO CPU fallback: without a usable HIP device every call fails with DFTA_ERR_NO_DEVICE.
 */
#ifndef DFTATOM_HIP_H
#define DFTATOM_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DFTA_OK              0
#define DFTA_ERR_INVALID     1   /* bad argument */
#define DFTA_ERR_NO_DEVICE   2   /* no HIP device / HIP runtime failure at start-up */
#define DFTA_ERR_HIP         3   /* HIP runtime error, see dfta_last_error() */
#define DFTA_ERR_NOMEM       4
#define DFTA_ERR_NOT_CONVERGED 5 /* soft: DFTAtom.cpp:538-539 `didNotConverge` */

typedef struct dfta_ctx     dfta_ctx;      /* device + stream + scratch                              */
typedef struct dfta_grid    dfta_grid;     /* device-resident tables of one logarithmic radial grid   */
typedef struct dfta_poisson dfta_poisson;  /* multigrid level storage for a batch of atoms            */
typedef struct dfta_scf     dfta_scf;      /* device-resident SCF state of a batch of atoms           */

/* ---- context -------------------------------------------------------------------------------------- */
/* hip_stream: a hipStream_t to launch on (e.g. torch.cuda.current_stream().cuda_stream), or NULL for a
 * stream owned by the context. */
int         dfta_ctx_create(int device, void* hip_stream, dfta_ctx** out);
void        dfta_ctx_destroy(dfta_ctx* ctx);
int         dfta_ctx_synchronize(dfta_ctx* ctx);
const char* dfta_last_error(const dfta_ctx* ctx);
const char* dfta_version(void);
/* HIP-event duration (ms, on the context's stream) of the dominant kernel of the last host-pointer call */
int         dfta_ctx_last_kernel_ms(dfta_ctx* ctx, float* ms);
/* Which of the two (bit-identical) Numerov sweep kernels dfta_numerov_sweeps / dfta_solve_levels / dfta_scf_step launch:
 * AUTO picks the pipelined kernel (one workgroup per block of 64 trials) while a launch has few blocks and the fused
 * one-wave-per-block kernel when the machine is full.  Initial value: AUTO, or $DFTA_SWEEP_KERNEL = fused | pipe. */
#define DFTA_SWEEP_AUTO      0
#define DFTA_SWEEP_FUSED     1
#define DFTA_SWEEP_PIPELINED 2
int         dfta_ctx_set_sweep_kernel(dfta_ctx* ctx, int which);
/* number of compute units / name of the device behind the context (reporting only) */
int         dfta_ctx_device_info(const dfta_ctx* ctx, int* num_cu, char* name, int name_cap);
/* Measurement aid (no counterpart in the reference): attainable HBM bandwidth of the device, GB/s, from a copy (c = a) and a
 * triad (a = b + s c) kernel over arrays of `doubles_per_array` fp64 each (>= 2^20, even; use >= 2^27 to defeat the 256 MB
 * Infinity Cache), best of `reps` timed repetitions after one warm-up.  bench.py quotes it next to the 8 TB/s spec figure. */
int         dfta_ctx_measure_hbm(dfta_ctx* ctx, size_t doubles_per_array, int reps, double* copy_gbs, double* triad_gbs);

/* ---- grid ------------------------------------------------------------------------------------------
 * Replaces NumerovFunctionNonUniformGrid's constructor and position/exp evaluations (Numerov.h:76-101,
 * 181-184), PoissonSolver::GetNumberOfNodes (PoissonSolver.h:127-135) and FillRNonuniformR
 * (PoissonSolver.cpp:212-223).  N = 2^mg_levels + 1.  Tables exp(i d), exp(2 i d), exp(i d / 2), r_i and
 * l(l+1)/(r_i r_i)*0.5 are evaluated once on the host with libm in the reference's operation order and
 * uploaded, so device kernels never call exp() on grid quantities. */
int    dfta_grid_create(dfta_ctx* ctx, int mg_levels, double delta, double Rmax, dfta_grid** out);
/* Uniform grid r_i = i h, h = Rmax / (N - 1): replaces NumerovFunctionRegularGrid (Numerov.h:16-70), the h of
 * DFTAtom.cpp:66-68 and PoissonSolver::FillR (PoissonSolver.cpp:200-210).  Every entry point below accepts either kind
 * of grid: sweeps then follow the IsUniform() branches of Numerov.h:274-291,353-370,408-425 (cut-off radius
 * 200/sqrt(2|E|), recurrence with h^2), the Poisson solver runs with deltaGrid = 0 (SolvePoissonUniform,
 * PoissonSolver.h:20-49) and the SCF is CalculateUniformLDA / LSDA (DFTAtom.cpp:60-210, 646-844). */
int    dfta_grid_create_uniform(dfta_ctx* ctx, int mg_levels, double Rmax, dfta_grid** out);
int    dfta_grid_is_uniform(const dfta_grid* g);
void   dfta_grid_destroy(dfta_grid* g);
int    dfta_grid_num_nodes(const dfta_grid* g);
double dfta_grid_rp(const dfta_grid* g);
int    dfta_grid_get_r(const dfta_grid* g, double* r_host);           /* N doubles */
int    dfta_num_nodes(int mg_levels);                                  /* PoissonSolver.h:127-135 */

/* ---- batched Numerov sweeps ------------------------------------------------------------------------
 * One trial = one call of
 *   DFTA_SWEEP_COUNT  Numerov<NonUniform>::SolveSchrodingerCountNodes     (Numerov.h:272-349)
 *   DFTA_SWEEP_ZERO   Numerov<NonUniform>::SolveSchrodingerSolutionInZero (Numerov.h:351-401)
 * for (potential index, l, E[, nodesLimit]).  All trials of a call are integrated concurrently, one lane
 * per trial, lanes of a wavefront marching the grid index together.
 *
 * boundary values (GetMaxRadiusIndex / GetBoundaryValueFar, Numerov.h:103-136):
 *   DFTA_BOUNDARY_DEVICE  cut-off index and the two start values are computed on the device (device exp());
 *   DFTA_BOUNDARY_HOST    they are computed on the host with libm exactly as the reference does and
 *                         uploaded -- sweeps are then bit-identical to the reference's.
 * The _dev variant always uses DFTA_BOUNDARY_DEVICE unless start/us/us1 are given (non-NULL). */
#define DFTA_SWEEP_COUNT 0
#define DFTA_SWEEP_ZERO  1
/* how a sweep is integrated: EXACT = the reference's rounding sequence (numerov.hip); TOLERANCE = transfer-matrix scan (scan.hip) */
#define DFTA_SWEEPS_EXACT     0
#define DFTA_SWEEPS_TOLERANCE 1
#define DFTA_BOUNDARY_DEVICE 0
#define DFTA_BOUNDARY_HOST   1

int dfta_numerov_sweeps(dfta_ctx* ctx, const dfta_grid* g, int kind, int boundary,
                        int nV, const double* V,            /* nV potentials, nV*N doubles (host)      */
                        int ntrials, const int* vidx,       /* potential index per trial (NULL -> 0)   */
                        const int* l, const double* E, const int* nodesLimit /* COUNT only */,
                        int* count_out,                     /* COUNT: node count per trial             */
                        double* u0_out,                     /* ZERO: extrapolated u(0); COUNT: optional */
                        int* start_out, int* trip_out);     /* optional diagnostics: cut-off index, loop trips */

/* device-pointer form; trials must be grouped: `ngroups` groups, group k covers trials
 * [group_off[k], group_off[k+1]) which share (group_vidx[k], group_l[k]).  All pointers are device
 * pointers except the small group_* arrays (host). */
int dfta_numerov_sweeps_dev(dfta_ctx* ctx, const dfta_grid* g, int kind,
                            int nV, const double* dV,
                            int ngroups, const int* group_off, const int* group_vidx, const int* group_l,
                            const double* dE, const int* dLimit,
                            const int* dStart, const double* dUs, const double* dUs1,   /* NULL -> device boundary */
                            int* dCount, double* dU0, int* dStartOut, int* dTrip);

/* TOLERANCE MODE of the same two sweeps (opt-in; logarithmic grids of 12 .. 20 multigrid levels): the recurrence of Numerov.h:309-321
 * is linear in w, w_{i-1} = (2 + f_i/(1 - f_i/12)) w_i - w_{i+1}, so ONE trial is integrated by the 512 lanes of a workgroup as a
 * transfer-matrix scan (segment products, log-depth combine, a second pass for the sign changes) in ~25 us at 131 073 points instead
 * of 4 ms as a dependent chain.  Same cut-off index, start values (device exp) and exit rules as above; a different order of roundings:
 * node counts equal the exact kernels' except inside the round-off band of a count transition (a few 1e-12 |E| wide), u(0) agrees to
 * ~1e-9 relative away from its zeros.  count_out holds CountNodes' decision value min(count, nodesLimit + 1); trip_out the loop trips up
 * to the classical-turning-point exit (not the early return at count > nodesLimit).  fallback_out[t] != 0 (optional): the scan met a
 * non-finite value or f >= 12 -- the exact kernels must decide that trial (never the case for potentials of an SCF). */
int dfta_numerov_sweeps_scan(dfta_ctx* ctx, const dfta_grid* g, int kind, int nV, const double* V, int ntrials, const int* vidx,
                             const int* l, const double* E, const int* nodesLimit, int* count_out, double* u0_out,
                             int* start_out, int* trip_out, int* fallback_out);

/* Numerov<NonUniform>::SolveSchrodingerMatchSolutionCompletely (Numerov.h:403-504) for a batch of
 * (vidx, l, E); Psi_out: ntrials*N doubles; matchPoint_out: ntrials. */
int dfta_numerov_match(dfta_ctx* ctx, const dfta_grid* g, int boundary, int nV, const double* V,
                       int ntrials, const int* vidx, const int* l, const double* E,
                       double* Psi_out, long* matchPoint_out);

/* ---- a potential resident on the device ------------------------------------------------------------------------------------------
 * The reference's Numerov keeps a REFERENCE to the caller's Potential and re-reads it on every call (Numerov.h:69,186), and its L3 makes
 * ~2100 calls on one Numerov object per SCF step.  dfta_numerov_sweeps / _match copy the potential and build the slot tables on every
 * call; a dfta_potential does both once (tables for l = 0..3), so that a call costs its sweep.  dfta_potential_update keeps the
 * "re-read on every call" semantics: a host memcmp against the resident copy, re-upload and rebuild only when the caller's values changed.
 * sweep_mode: DFTA_SWEEPS_EXACT (host boundary values: bit-identical to the reference) or DFTA_SWEEPS_TOLERANCE (scan sweeps,
 * ~0.1 ms per call at 131 073 points instead of 4 ms; a trial the scan cannot decide is repeated on the exact kernels).
 * dftatom_amd/compat/Numerov.h holds one per DFT::Numerov object. */
typedef struct dfta_potential dfta_potential;
int  dfta_potential_create(dfta_ctx* ctx, const dfta_grid* g, const double* V /* N, host */, dfta_potential** out);
int  dfta_potential_update(dfta_potential* p, const double* V /* N, host */);
void dfta_potential_destroy(dfta_potential* p);
int  dfta_potential_sweeps(dfta_potential* p, int kind, int sweep_mode, int ntrials, const int* l, const double* E, const int* nodesLimit,
                           int* count_out, double* u0_out, int* start_out, int* trip_out);
int  dfta_potential_match(dfta_potential* p, int ntrials, const int* l, const double* E, double* Psi_out, long* matchPoint_out);

/* ---- eigenvalue search for a batch of (atom,spin) potentials -----------------------------------------
 * Replaces DFTAtom::LoopOverLevels + LocateInterval + NormalizeNonUniform + the density update of
 * CalculateNonUniformDensity (DFTAtom.cpp:36-56, 328-343, 493-604).  All bisections run on the device as
 * speculative bisection trees of depth `tree_depth` that reproduce the reference's midpoint sequence.
 *   mode DFTA_LEVELS_CHAINED : BottomEnergy handed from level to level as DFTAtom.cpp:541 (E-3); levels of one
 *                              potential run one after the other (bit-for-bit the reference's bisection path)
 *   mode DFTA_LEVELS_BATCHED : all levels run concurrently and un-chained; level (v, l) starts from
 *                              max(bottom0[v], min_i Veff_l(i)) -- no eigenvalue lies below the minimum of the
 *                              effective potential, and below it the node-count predicate of l >= 1 misfires
 *                              (SURVEY C.12), which is why plain -Z^2-1 is not safe for f levels.  Documented
 *                              deviation from DFTAtom.cpp:541: the bisection paths differ, eigenvalues agree with
 *                              the chained path to ~1e-10 relative (tests).  bottom_hint, if given, is used as is. */
#define DFTA_LEVELS_CHAINED 0
#define DFTA_LEVELS_BATCHED 1
/* OR-ed into `mode` of dfta_solve_levels: the TOLERANCE MODE of the sweeps (see dfta_numerov_sweeps_scan).  The same three bisections
 * with the same midpoints, every trial integrated by the transfer-matrix scan: one workgroup runs LocateInterval and the u(0)
 * bisection of its level from start to end on the device -- no rounds, no speculation.  Eigenvalues agree with the exact path to the
 * width of the round-off band of the reference's own predicates (gate 2e-11 |E| + 1e-11 Ha; sweeps_reference counts stay
 * the reference's except for decisions inside that band).  Grids of 12 .. 20 multigrid levels; dfta_scf_options::sweep_mode for the SCF. */
#define DFTA_LEVELS_SCAN_SWEEPS 0x10

typedef struct dfta_level_result {
    double E;            /* eigenvalue (level.E, DFTAtom.cpp:534)                       */
    double top, bottom;  /* interval returned by LocateInterval                          */
    int    n_count;      /* reference-equivalent CountNodes sweeps on the bisection path */
    int    n_zero;       /* reference-equivalent SolutionInZero sweeps                   */
    int    converged;    /* !didNotConverge                                              */
    int    matchPoint;
    int    status;       /* DFTA_LEVEL_* bits: HOW the u(0) bisection ended (below)      */
} dfta_level_result;
/* The reference folds every way its u(0) bisection (DFTAtom.cpp:517-539) can fail to meet `Top - Bottom < 1e-12 && |u(0)| < 1e15` into
 * one flag, didNotConverge.  status tells them apart:
 *   CONVERGED       the stop test was met (converged != 0, no other bit);
 *   ITERATION_CAP   the 500-iteration cap ended the loop;
 *   FIXED_POINT     ... and the interval had collapsed long before: a step left (Top, Bottom) as they were, i.e. the same midpoint, sweep and
 *                   decision repeated to the cap -- |u(0)| never came below 1e15 (the case at 1 048 577 nodes from the seventh SCF step on;
 *                   those repeats are counted in n_zero but not integrated);
 *   U0_NONFINITE    u(0) of the last trial was NaN or infinite (overflow of the inward solution). */
#define DFTA_LEVEL_CONVERGED     1
#define DFTA_LEVEL_ITERATION_CAP 2
#define DFTA_LEVEL_FIXED_POINT   4
#define DFTA_LEVEL_U0_NONFINITE  8

int dfta_solve_levels(dfta_ctx* ctx, const dfta_grid* g, int mode, int tree_depth,
                      int nV, const double* V, const double* bottom0 /* nV */,
                      const double* bottom_hint /* BATCHED: per level bracket start, NULL -> bottom0[v] */,
                      int nlevels, const int* vidx, const int* n, const int* l, const int* occ,
                      dfta_level_result* results,           /* nlevels */
                      double* newDensity /* nV*N, accumulated occ*Psi^2 (i < N-1), may be NULL */,
                      double* Eelectronic /* nV, may be NULL */,
                      double* Psi_out /* nlevels*N normalised, may be NULL */,
                      long* issued_sweeps /* optional: sweeps actually launched */);

/* ---- multigrid Poisson -------------------------------------------------------------------------------
 * Replaces DFT::PoissonSolver (PoissonSolver.h:15-171, PoissonSolver.cpp).  `batch` independent atoms are
 * solved concurrently, one workgroup per atom. */
int  dfta_poisson_create(dfta_ctx* ctx, const dfta_grid* g, int batch, dfta_poisson** out);  /* PoissonSolver.cpp:8-27 */
/* Smoother mode.  EXACT (default): every Gauss-Seidel sweep (PoissonSolver.cpp:40-64) equals the reference's sequential sweep bit
 * for bit (lanes start 96 / 112 nodes early).  TOLERANCE (opt-in): 32-node warm-ups -- a lane's start value then
 * carries ~1e-9 of the change its start node undergoes in that sweep; the cycle converges to the same discrete solution and
 * round-off floor (gates: U within 2e-9 Z of the exact solve -- observed 4e-10 .. 9e-10 Z, what the reference itself moves by
 * under FMA contraction --, SCF energies 1e-9 relative, eigenvalues 1e-8 Ha + 2e-9 |E|), at about 75 % of the time.
 * dfta_poisson_create takes the mode from the knob list, DFTA_DEBUG="POISSON_MODE=tolerance" (or adaptive); default EXACT. */
#define DFTA_POISSON_EXACT     0
#define DFTA_POISSON_TOLERANCE 1
/* DFTA_POISSON_ADAPTIVE: the tolerance mode's kernels, and the V-cycles stop where the cycle has reached its round-off floor -- the norm of
 * the last level-0 sweep has not fallen below 0.7 x the previous cycle's twice in a row (and is below 1e-3 of the first cycle's) -- instead
 * of at the reference's cap of 100 (PoissonSolver.cpp:185-197: its test ||dPhi|| < 1e-14 lies below that floor, so the reference always
 * runs to the cap; the floor is reached after 6 .. 8 cycles).  Opt-in, never the default.  Gates against the exact 100-cycle
 * solve (tests/test_gpu_resident.py): U within 2e-9 Z on the logarithmic grids of the BASELINE configurations (the tolerance mode's gate),
 * 1e-8 Z on the uniform and nearly uniform grid, 2e-8 Z at 2^20+1 nodes (the conditioning of those solves: the reference's own solve moves
 * by 1.4e-8 relative under a 1e-12 perturbation there); the end residual is the exact solve's in every case. */
#define DFTA_POISSON_ADAPTIVE 2
int  dfta_poisson_create_ex(dfta_ctx* ctx, const dfta_grid* g, int batch, int mode, dfta_poisson** out);
int  dfta_poisson_mode(const dfta_poisson* p);
void dfta_poisson_destroy(dfta_poisson* p);
/* SolvePoissonNonUniform (PoissonSolver.h:51-81): density batch*N (host) -> U batch*N (host).
 * vcycles_out/err_out (optional, per atom): V-cycles executed (<=100) and last ||dPhi||_2. */
int  dfta_poisson_solve(dfta_poisson* p, const int* Z, const double* density, double* U,
                        int* vcycles_out, double* err_out);
/* device-pointer form; SYNCHRONISES: see dfta_poisson_group_info */
int  dfta_poisson_solve_dev(dfta_poisson* p, const int* dZ, const double* dDensity, double* dU);
/* While the batch leaves compute units idle, the fine levels of an atom are swept by a group of G workgroups that wait
 * for each other: the solve is launched cooperatively (the runtime refuses a grid that cannot be co-resident), the
 * barriers' spins are bounded, and after EVERY solve (dfta_poisson_solve, _solve_dev, dfta_scf_create, dfta_scf_step)
 * the groups' abort flag is inspected.  A refused launch or an aborted solve is repeated in the same process with one
 * workgroup per atom (bit-identical results), and the solver stays `degraded` to that path; `aborts` counts the solves
 * that had to be repeated.  $DFTA_FAULT_POISSON_MEMBER=1 (tests) makes the last member of every group return at once. */
int  dfta_poisson_group_info(const dfta_poisson* p, int* G, int* degraded, int* aborts);
/* Exact mode: the fused three-sweep visits of the 129 .. 1025-node levels start 32 nodes in front of a lane's chunk from PREDICTED values
 * (affine scan of the sweep's recurrence) and every lane's state is compared bit for bit with what the lane in front computed for the
 * same nodes; a visit with a mismatch is put back and repeated with the 112-node warm-up from old values, so results
 * never depend on a prediction.  `checked`: visits that ran that way since the solver was created, `repeated`: those that had to be run
 * again (either may be NULL).  $DFTA_DEBUG POISSON_NOPREDICT: off (both stay 0); POISSON_PREDICT_FUZZ: every visit repeated. */
int  dfta_poisson_predict_counts(dfta_poisson* p, unsigned long long* checked, unsigned long long* repeated);
/* unit-parity hooks on level storage of atom 0 (GaussSeidel / Restrict / Prolong / VCycle,
 * PoissonSolver.cpp:40-64, 110-157; PoissonSolver.h:155-159) */
int  dfta_poisson_level_size(const dfta_poisson* p, int lvl);
int  dfta_poisson_set_level(dfta_poisson* p, int lvl, const double* Phi, const double* Src);
int  dfta_poisson_get_level(dfta_poisson* p, int lvl, double* Phi, double* Src);
int  dfta_poisson_gauss_seidel(dfta_poisson* p, int lvl, int sweeps, double* err_out /* per sweep */);
/* IterateGaussSeidel (PoissonSolver.cpp:66-77): up to iterno sweeps, stops after a sweep with err < errorMin;
 * three sweeps of a chunked level run as one fused pass (same arithmetic, one third of the memory traffic) */
int  dfta_poisson_iterate_gs(dfta_poisson* p, int lvl, double errorMin, int iterno, double* err_out, int* sweeps_out);
int  dfta_poisson_restrict(dfta_poisson* p, int lvl);
int  dfta_poisson_prolong(dfta_poisson* p, int lvl_src);
int  dfta_poisson_vcycle(dfta_poisson* p, double* err_out);
/* PoissonSolver::SetBoundaries + FullCycle (PoissonSolver.cpp:29-33, PoissonSolver.h:89-124) on atom 0's level storage: the
 * level-0 source is the one the last solve (or dfta_poisson_set_level) left there */
int  dfta_poisson_full_cycle(dfta_poisson* p, double lowBoundary, double highBoundary, double errorMin, double errorMinLast,
                             double* err_out, int* vcycles_out);

/* ---- VWN exchange-correlation ---------------------------------------------------------------------------
 * VWNExchCor::Vexc / eexcDif, LDA (VWNExcCor.h:73-128) and LSDA (VWNExcCor.h:134-312). Host pointers. */
int dfta_vwn_lda(dfta_ctx* ctx, const double* n, size_t sz, double* vexc, double* eexcdif);
int dfta_vwn_lsda(dfta_ctx* ctx, const double* na, const double* nb, size_t sz,
                  double* vexc, double* va, double* vb, double* eexcdif);

/* Chachiyo's correlation functional with Dirac exchange, LDA: ChachiyoExchCor<Param>::Vexc / eexcDif (ExcCor.h:27-95);
 * improved != 0 selects ChachiyoExchCorImprovedParam (ExcCor.h:21-26).  The reference keeps it beside VWN with every
 * call site commented out (DFTAtom.cpp:383,412,421). */
int dfta_chachiyo_lda(dfta_ctx* ctx, int improved, const double* n, size_t sz, double* vexc, double* eexcdif);

/* ---- PW92 and PBE (beyond the reference, which has LDA only) ------------------------------------------------
 * DFTA_XC_PW92: Slater exchange + Perdew-Wang 1992 correlation (constants of the PBE reference code, libxc lda_c_pw_mod).
 * DFTA_XC_PBE: Perdew-Burke-Ernzerhof 1996 exchange and correlation on top of PW92; the spin-polarised exchange follows the
 * spin-scaling relation E_x[a, b] = (E_x[2a] + E_x[2b]) / 2.  Densities per volume, sigma_xy = grad rho_x . grad rho_y.  A total
 * density below 1e-18 (the VWN threshold, VWNExcCor.h:82) gives zeros; a spin channel below it has no exchange and pins zeta to +-1.
 * Host pointers; both record the kernel time for dfta_ctx_last_kernel_ms. */
/* pointwise e (per volume) and its partial derivatives; nb == NULL: unpolarised (n = na, sigma = saa; dnb, dsab, dsbb not written);
   functional: DFTA_XC_PW92 (sigma ignored, d/dsigma = 0) or DFTA_XC_PBE */
int dfta_xc_pointwise(dfta_ctx* ctx, int functional, size_t sz, const double* na, const double* nb,
                      const double* saa, const double* sab, const double* sbb,
                      double* e, double* dna, double* dnb, double* dsaa, double* dsab, double* dsbb);
/* the SCF's evaluation on a grid for natoms x N densities (atom-major); nb == NULL: LDA outputs (res = Vexc, va / vb not written).
 * PBE: rho' by 5-point central differences in the grid index over dr/di (second-order one-sided at nodes 0, 1, N-2, N-1),
 * v = de/drho - (dF/dr + 2F/r) with the flux F_a = 2 e_saa rho_a' + e_sab rho_b'; node 0 is 0.  Logarithmic grids only for PBE.
 * Outputs as the VWN pair: LDA Vexc = v, eexc = e/rho - v; LSDA res = (v_a rho_a + v_b rho_b)/rho, va, vb, eexc = e/rho - res. */
int dfta_xc_radial(dfta_ctx* ctx, const dfta_grid* g, int functional, int natoms, const double* na, const double* nb,
                   double* res, double* va, double* vb, double* eexc);

/* ---- quadrature --------------------------------------------------------------------------------------------
 * Integral::{Trapezoid,SimpsonOneThird,Simpson38,Boole,Romberg} (Integral.h:11-155); values: host. */
#define DFTA_INT_TRAPEZOID 0
#define DFTA_INT_SIMPSON13 1
#define DFTA_INT_SIMPSON38 2
#define DFTA_INT_BOOLE     3
#define DFTA_INT_ROMBERG   4
int dfta_integrate(dfta_ctx* ctx, int rule, double delta, const double* values, int sz, double* result);

/* ---- SCF on a batch of atoms ---------------------------------------------------------------------------------
 * Replaces the body of DFTAtom::CalculateNonUniformLDA / LSDA (DFTAtom.cpp:346-491, 847-1022): state lives
 * in HBM between steps; one call advances every atom of the batch by one SCF iteration. */
typedef struct dfta_energies {
    double Etotal, Ekinetic, Ecoul, Enuclear, Exc;     /* as printed at DFTAtom.cpp:472 */
    double Eelectronic, Ehartree, eExcDif, Epotential;
} dfta_energies;

typedef struct dfta_step_stats {
    int    struct_size;          /* IN: sizeof(dfta_step_stats) of the CALLER's header (set it before every dfta_scf_step); the library
                                    fills no more than that many bytes, and rejects a value smaller than the version-6 prefix */
    int    levels_fallbacks;     /* solves of this step's level search that were repeated on another path: a sweep the scan could not decide or a
                                    lost worker of the device-side search (both: host rounds on the exact kernels, same results) */
    long   sweeps_issued;        /* Numerov sweeps launched (speculative trees)            */
    long   sweeps_reference;     /* sweeps on the reference's bisection path (count+zero+match) */
    long   points_traversed;     /* grid points traversed by issued sweeps                  */
    long   vcycles;              /* Poisson V-cycles executed over the batch                */
    int    rounds;               /* bisection rounds (= launches of the sweep kernel)       */
    float  ms_levels, ms_poisson, ms_tail;   /* HIP-event times of the three phases       */
    float  ms_sweep_kernels;     /* HIP-event time summed over the sweep-kernel launches only */
    float  ms_poisson_kernel;    /* HIP-event time of the persistent multigrid kernel        */
    long   sweeps_reference_executed; /* sweeps_reference minus the CountNodes calls of node-less levels' second
                                    bisection ("count < 0": decided without integrating, levels.hip) */
    long   points_reference;     /* grid points traversed by the executed sweeps on the reference's path */
    int    levels_layout;        /* trial layout of this step's level search: 0 one block of 2^depth trials per job, 1 latency mode
                                    (slots re-allotted every round, <= 64 jobs), 2 packed rounds (batches), 3 latency mode over the
                                    live jobs of a batch most of whose atoms have finished, 4 scan search (tolerance mode of the sweeps), 5 device-side exact
                                    search (one persistent kernel, every level at its own pace, up to 256 live levels: persist.inc), 6 own-pace search of a batch (one
                                    workgroup per level in one launch: own.inc, opt-in $DFTA_DEBUG LEVELS_OWN) -- never changes a result */
    int    poisson_groups;       /* workgroups per atom of the multigrid solve of this step (33 / 17: resident groups of up to 7 / 15 atoms); the live atoms of
                                    a batch are solved by a solver of their size class (128 / 64 / 32 / 16 / 15 / 7 atoms) once that is smaller
                                    than the batch's own */
} dfta_step_stats;

int  dfta_scf_create(dfta_ctx* ctx, const dfta_grid* g, int lsda, int natoms, const int* Z,
                     double alpha, int levels_mode, int tree_depth, dfta_scf** out);   /* DFTAtom.cpp:351-394 / 852-906 */
/* The reference's compile-time alternatives as run-time options (NULL = what the reference runs). */
#define DFTA_XC_VWN               0   /* VWNExchCor (live in the reference)                                  */
#define DFTA_XC_CHACHIYO          1   /* ChachiyoExchCor<ChachiyoExchCorParam>, LDA only (ExcCor.h)           */
#define DFTA_XC_CHACHIYO_IMPROVED 2   /* ChachiyoExchCor<ChachiyoExchCorImprovedParam> (DFTAtom.cpp:383)      */
#define DFTA_XC_PW92              3   /* Slater exchange + PW92 correlation, LDA and LSDA, both grids (not in the reference) */
#define DFTA_XC_PBE               4   /* PBE GGA, LDA and LSDA, logarithmic grid only (not in the reference)  */
/* Density mixing.  The reference mixes linearly, rho <- alpha rho + (1 - alpha) rho_out (DFTAtom.cpp:332-342): DFTA_MIX_LINEAR, the
 * default, keeps that bit for bit.  DFTA_MIX_ANDERSON goes beyond the reference: per atom, on the atom's own step count k = 1, 2, ...,
 * the (x_j, f_j = g_j - x_j) pairs of the newest mix_history previous steps (x the input density of a step -- LSDA: both spin
 * densities as one vector --, g its output density) are kept on the device; steps k <= mix_warmup and steps with no history are
 * the linear mix, bit for bit; otherwise, with dX_j = x - x_j, dF_j = f - f_j and <u,v> = Sum_{i>=1} 4 pi r_i^2 (dr/di)_i u_i v_i,
 *   (A + 1e-14 trace(A) I) gamma = b,  A_jk = <dF_j, dF_k>,  b_j = <dF_j, f>          (Cholesky)
 *   x+ = lin - Sum_j gamma_j (dX_j + (1 - alpha) dF_j), node by node and per spin channel only where that is >= 0, lin elsewhere.
 * A pivot <= 0 or a non-finite gamma (alpha = 1: nothing moves, A = 0): x+ = lin and the atom's history is cleared.  Stop test,
 * energies and everything downstream are unchanged; a frozen atom's history is untouched; an atom's bits do not depend on its batch.
 * Costs 2 mix_history doubles per node and spin channel of device memory.  A typical atom finishes in 17-21 steps instead of 28-36. */
#define DFTA_MIX_LINEAR   0
#define DFTA_MIX_ANDERSON 1
/* The mixing launches on their own (tests and tools; dfta_scf_step does not go through this).  A dfta_mixer owns what the SCF owns for its
 * mixing stage -- device copies of newDensity (natoms x nspin x N), density, dA, dB (natoms x N) and, with DFTA_MIX_ANDERSON, the atoms'
 * history -- and one dfta_mixer_step issues exactly the launches dfta_scf_step issues at that stage for the same `mixing`.  Host pointers.
 * step: acc is Sum f Psi^2 of every potential (in) and the output density g as the kernels store it (out); density / dA / dB are the
 * step's input density (in; LDA: dA = dB = NULL) and the mixed one (out); fin: per atom, != 0: frozen.  The caller supplies the input
 * density of every step.  get, Anderson only, any pointer may be NULL: state[8] = ring head, length, steps taken | the last step's head,
 * pairs used, use flag, 0, 0; gamma[8]; slab[chunks of 1024 nodes][44]: the chunks' shares of A's upper triangle row by row (the newest 8
 * pairs: 36), then b (8), of the last step; ring[nspin][history][2][N]: the (x, f) pairs by slot. */
typedef struct dfta_mixer dfta_mixer;
int  dfta_mixer_create(dfta_ctx* ctx, const dfta_grid* g, int lsda, int natoms, int mixing, int history, int warmup, dfta_mixer** out);
int  dfta_mixer_step(dfta_mixer* mx, double alpha, double* acc, double* density, double* dA, double* dB, const int* fin);
int  dfta_mixer_get(dfta_mixer* mx, int atom, int* state, double* gamma, double* slab, double* ring);
void dfta_mixer_destroy(dfta_mixer* mx);
typedef struct dfta_scf_options {
    int struct_size;  /* sizeof(dfta_scf_options) of the CALLER's header: members beyond it keep their defaults, a value that is no valid
                         size of this struct (0, or what an older header had in this place) is rejected with DFTA_ERR_INVALID          */
    int integrator;   /* DFTA_INT_*: quadrature of the energy integrals and of the normalisation (default SIMPSON38) */
    int functional;   /* DFTA_XC_*                                                                                */
    int aufbau;       /* DFTA_AUFBAU_*                                                                            */
    int poisson_mode; /* DFTA_POISSON_EXACT (0, default) / DFTA_POISSON_TOLERANCE / DFTA_POISSON_ADAPTIVE; -1: as dfta_poisson_create (DFTA_DEBUG POISSON_MODE=...) */
    int sweep_mode;   /* DFTA_SWEEPS_EXACT (0, default) / DFTA_SWEEPS_TOLERANCE (scan sweeps, see DFTA_LEVELS_SCAN_SWEEPS)                */
    int mixing;       /* DFTA_MIX_LINEAR (0, default: the reference's mixing) / DFTA_MIX_ANDERSON                                       */
    int mix_history;  /* Anderson: pairs kept per atom, 1 .. 8; 0: the default, 4                                                       */
    int mix_warmup;   /* Anderson: linear steps before the first accelerated one, 1 .. 100; 0: the default, 3                           */
} dfta_scf_options;
/* The option and statistics structs start with struct_size (since version 6) and grow at the END between versions of this header:
 * zero-initialise them, set struct_size = sizeof(...) -- every other member's 0 is the reference's behaviour -- and the library reads /
 * writes no more than the caller's struct holds.  dfta_abi_version() returns the DFTA_ABI_VERSION the library was built with. */
#define DFTA_ABI_VERSION 7
int  dfta_abi_version(void);
int  dfta_scf_create_ex(dfta_ctx* ctx, const dfta_grid* g, int lsda, int natoms, const int* Z, double alpha, int levels_mode,
                        int tree_depth, const dfta_scf_options* options, dfta_scf** out);
void dfta_scf_destroy(dfta_scf* s);
int  dfta_scf_step(dfta_scf* s, dfta_step_stats* stats);                               /* DFTAtom.cpp:396-484 / 908-1009 */
/* An atom that has met the reference's stop test (DFTAtom.cpp:474-479: |dE/E| < 1e-11 and all levels converged in two
 * consecutive steps) is FROZEN: later steps of the batch leave its density, potential, eigenvalues, energies, step count
 * and record untouched, exactly as if it had been run alone, and cost nothing for it.
 * results of the last step (host copies): per atom energies; finished flag (the reference's Finished! test) */
int  dfta_scf_get_energies(dfta_scf* s, dfta_energies* e /* natoms */, int* finished /* natoms */);
/* geometry of the level search: bisection-tree depth, number of (atom,spin,n,l) jobs, trial lanes per round */
int  dfta_scf_info(const dfta_scf* s, int* tree_depth, int* njobs, long* trials_per_round);
int  dfta_scf_poisson_info(const dfta_scf* s, int* G, int* degraded, int* aborts);
/* Quadrature rule (DFTA_INT_*) of the live path: the five energy integrals of a step and the normalisation of every
 * orbital.  The reference calls Integral::Simpson38 at all 22 sites (DFTAtom.cpp:27,51,459-467,...) although its README
 * names Romberg (README.md:81); Simpson38 is the default, the other rules of Integral.h:11-155 are a switch away. */
int  dfta_scf_set_integrator(dfta_scf* s, int rule);   /* dfta_poisson_group_info of the SCF's solver */
int  dfta_scf_num_levels(const dfta_scf* s, int atom, int spin);
int  dfta_scf_get_levels(dfta_scf* s, int atom, int spin, int* n, int* l, int* occ, double* E, int* converged);
/* DFTA_LEVEL_* bits of every level of (atom, spin) after the last step, and the reference-equivalent sweep counts (any pointer may be NULL) */
int  dfta_scf_get_level_status(dfta_scf* s, int atom, int spin, int* status, int* n_count, int* n_zero);
int  dfta_scf_get_array(dfta_scf* s, int atom, int which, double* out /* N */);  /* 0 density,1 densityA,2 densityB,3 potA,4 potB,5 U */
/* fixed-size per-atom record for the periodic-table gather: 64 doubles */
#define DFTA_RECORD_DOUBLES 64
int  dfta_scf_get_records_dev(dfta_scf* s, double* dRecords /* natoms*64, device */);

/* ---- orbitals of the SCF, their expectation values and r^k matrix elements (beyond the reference, which prints eigenvalues only) ----
 * An orbital is the array u[i] = r_i R_nl(r_i), N doubles, exactly as the level search holds it after the step: normalised so that the
 * SCF's quadrature of u^2 (dr/di) is 1 (DFTAtom.cpp:36-56), with the sign the match solve left, zero beyond the level's cut-off index;
 * Sum_levels occ u^2 over the nodes i < N-1 is the step's output density times 4 pi r^2 (DFTAtom.cpp:558-559, 332-342).  The orbitals
 * of an atom are those of the LAST STEP IN WHICH IT WAS LIVE: eigenfunctions of that step's INPUT potential, not of the potential
 * dfta_scf_get_array(.., 3 / 4) returns after the step (that one is the next step's input).  A frozen atom keeps its orbitals.  Before
 * the first dfta_scf_step every dfta_scf_* call of this block returns DFTA_ERR_INVALID.
 *
 * Quadrature: with s_i = dr/di (Rp delta exp(i delta) on the logarithmic grid, h on the uniform one),
 *   Q[f] = (3/8) (f_0 + f_{N-1} + 3 Sum_{0<i<N-1, i%3 != 0} f_i + 2 Sum_{0<i<N-1, i%3 == 0} f_i),
 * the weights of Integral::Simpson38 (Integral.h:50-73) -- whatever dfta_scf_options::integrator the SCF runs with (NORM shows the
 * difference).  Columns of a property row:
 *   NORM = Q[u^2 s];  <r^m> = Q[u^2 r^m s], m = -1, 1, 2, 4 and, for l >= 1, m = -3 (0.0 for l = 0); negative powers add 0 at r_0 = 0;
 *   T = 1/2 Q[(du/di)^2 / s + l(l+1) u^2 / r^2 s] (second term 0 at node 0): the kinetic energy from the orbital alone; du/di is
 *       (8 (u_{i+1} - u_{i-1}) - (u_{i+2} - u_{i-2})) / 12 inside and (-3 u_0 + 4 u_1 - u_2) / 2, (u_2 - u_0) / 2,
 *       (u_{N-1} - u_{N-3}) / 2, (3 u_{N-1} - 4 u_{N-2} + u_{N-3}) / 2 at the nodes 0, 1, N-2, N-1;
 *   RPEAK = r at the node of largest |u| (lowest index on ties; no interpolation).
 * M^(k)_ab = Q[u_a u_b r^k s], k = 0, 1, 2: computed once per pair and mirrored, symmetric bit for bit.
 * In the closed forms of a hydrogen-like atom (<r> = (3 n^2 - l(l+1)) / (2 Z), ...) n is the principal quantum number; the level
 * arrays of this header hold the reference's m_N = n - 1.  Sums have a fixed shape that depends on N alone (no floating-point
 * atomics): an orbital's values do not depend on the batch it sits in, nor on the run. */
#define DFTA_ORB_PROPS 8
#define DFTA_ORB_NORM  0
#define DFTA_ORB_RM1   1   /* <1/r>   */
#define DFTA_ORB_R1    2   /* <r>     */
#define DFTA_ORB_R2    3   /* <r^2>   */
#define DFTA_ORB_R4    4   /* <r^4>   */
#define DFTA_ORB_T     5
#define DFTA_ORB_RPEAK 6
#define DFTA_ORB_RM3   7   /* <1/r^3>, l >= 1 */
/* u: nlev x N (host), levels in the order of dfta_scf_get_levels */
int  dfta_scf_get_orbitals(dfta_scf* s, int atom, int spin, double* u);
/* props: njobs x DFTA_ORB_PROPS (host), every orbital of the batch in one launch; jobs atom-major, an atom's alpha levels then its
 * beta levels (njobs of dfta_scf_info).  Records the launch's time for dfta_ctx_last_kernel_ms. */
int  dfta_scf_orbital_properties(dfta_scf* s, double* props);
/* M: nlev x nlev, row-major (host); k = 0, 1 or 2 */
int  dfta_scf_orbital_matrix(dfta_scf* s, int atom, int spin, int k, double* M);
/* the same two launches on caller-supplied orbitals (tests and tools); host pointers.  u: norb x N; props: norb x DFTA_ORB_PROPS;
 * M: norb x norb, norb <= 32.  norb == 0: DFTA_OK, nothing is written. */
int  dfta_orbital_properties(dfta_ctx* ctx, const dfta_grid* g, int norb, const int* l, const double* u, double* props);
int  dfta_orbital_matrix(dfta_ctx* ctx, const dfta_grid* g, int norb, const double* u, int k, double* M);

/* ---- Slater integrals R^k, F^k, G^k and the exact-exchange energy of orbitals (beyond the reference) ---------------------------------
 * With the orbitals u, s_i = dr/di and the quadrature Q[f] of the block above, and P_xy,i = u_x,i u_y,i,
 *   R^k(ab,cd) = Int Int u_a(r) u_c(r) r_<^k / r_>^(k+1) u_b(r') u_d(r') dr dr'
 *              = Int r^(-k-1) [P_ac(r) Z^k_bd(r) + P_bd(r) Z^k_ac(r)] dr,   Z^k_xy(r) = Int_0^r t^k P_xy(t) dt
 * (the regions r' < r and r' > r swapped into one form: forward cumulative integrals only).  What the library computes, node by node:
 *   g_i = (p_i P_xy,i) s_i with p_i = r_i^k formed as p = 1, then k times p = p * r_i;
 *   d_1 = (((9 g_0 + 19 g_1) - 5 g_2) + g_3) / 24,  d_i = (13 (g_{i-1} + g_i) - (g_{i-2} + g_{i+1})) / 24 for 2 <= i <= N-2,
 *   d_{N-1} = (((g_{N-4} - 5 g_{N-3}) + 19 g_{N-2}) + 9 g_{N-1}) / 24;   Z_0 = 0, Z_i = Sum_{j <= i} d_j;
 *   R^k = Q[ ((P_X,i Z_Y,i + P_Y,i Z_X,i) (1 / (p_i r_i))) s_i ], the term of node 0 (r_0 = 0) being 0,
 * where X = (min(a,c), max(a,c)) and Y = (min(b,d), max(b,d)) are exchanged if Y < X (first index, then second), a product is its
 * lower-indexed orbital times the other, and X == Y is one stream.  R^k is therefore bit-identical under a <-> c, b <-> d and
 * (a,c) <-> (b,d).  F^k(a,b) = R^k(ab,ab), G^k(a,b) = R^k(ab,ba).  0 <= k <= DFTA_SLATER_KMAX, N >= 5.  The sums have a fixed shape
 * that depends on N alone (no atomics): a job's value depends on its orbitals, k and N -- not on the other jobs of the
 * call, its position among them, or the run.  Nodes beyond an orbital's cut-off are zeros like any others.
 *
 * A job table is njobs rows of five ints a, b, c, d, k.  Energies, with N_i the occupation of shell i in its channel
 * (dfta_scf_get_occupations) and n_a = N_a for LSDA, N_a / 2 in each of two equal channels for LDA:
 *   E_H = 1/2 Sum_i Sum_j (N_i N_j) F^0(i,j) over all shells of the atom, both channels: rows i, then j, one accumulator;
 *   E_x = -1/2 Sum_sigma Sum_{a,b in sigma} (n_a n_b) T_ab,  T_ab = Sum_k (l_a k l_b; 0 0 0)^2 G^k(a,b),  G^k(a,a) = F^k(a,a),
 *         |l_a - l_b| <= k <= l_a + l_b, k = l_a + l_b (mod 2), ascending: one accumulator S over the channels, alpha first, rows a,
 *         then b (every b of the channel); LSDA: E_x = -0.5 S; LDA: S of the one channel with n = 0.5 N, E_x = -S.
 * This is the spherically averaged exchange: valid for fractional occupations; for closed shells the average-of-configuration
 * formula.  Both sums are host arithmetic in double on the integrals of ONE launch. */
#define DFTA_SLATER_KMAX 8
/* host-only: (la k lb; 0 0 0)^2 from the factorial closed form, correctly rounded; 0.0 where parity or the triangle rule fails.
 * DFTA_ERR_INVALID: a negative argument, la or lb > 4, out NULL. */
int  dfta_gaunt_3j2(int la, int k, int lb, double* out);
/* host-only: the job table of the F^k / G^k of norb orbitals with angular momenta l (0 .. 4).  First the F^k(a,b), a <= b, k = 0, 2 ..
 * 2 min(l_a, l_b), rows a,b,a,b,k ordered by a, then b, then k (kinds[j] = 0); then the G^k(a,b), a < b, k of the exchange sum, rows
 * a,b,b,a,k in the same order (kinds[j] = 1).  G^k(a,a) = F^k(a,a) is no job of its own.  Returns the number of jobs (jobs, kinds may be
 * NULL: count only), or -1 for norb < 0, l NULL or an l outside 0 .. 4. */
int  dfta_slater_fg_jobs(int norb, const int* l, int* jobs, int* kinds);
/* every job in one launch, on caller-supplied orbitals; host pointers.  u: norb x N; R: njobs.  njobs == 0: DFTA_OK, nothing is
 * written.  Records the launch's time for dfta_ctx_last_kernel_ms. */
int  dfta_slater_rk(dfta_ctx* ctx, const dfta_grid* g, int norb, const double* u, int njobs, const int* jobs, double* R);
/* ... on the orbitals of an atom of the SCF, read in place; indices count the atom's orbitals as dfta_scf_orbital_properties lists
 * them: alpha levels, then beta levels.  Before the first dfta_scf_step: DFTA_ERR_INVALID.  The job table and the results are kept
 * on the device from the first such call on (grown when a longer table comes). */
int  dfta_scf_slater_rk(dfta_scf* s, int atom, int njobs, const int* jobs, double* R);
/* F, G: (DFTA_SLATER_KMAX + 1) x nlev x nlev each, k-major (host): the table of dfta_slater_fg_jobs for the levels of (atom, spin)
 * from one launch, each value computed once and mirrored (symmetric bit for bit), G^k(a,a) = F^k(a,a), 0.0 where there is no job. */
int  dfta_scf_slater_fg(dfta_scf* s, int atom, int spin, double* F, double* G);
/* E_H and E_x of an atom from one launch: the F^0 of all its shell pairs, the G^k of each channel, then the host sums above */
int  dfta_scf_coulomb_exchange(dfta_scf* s, int atom, double* EH, double* EXX);

/* ---- exchange potentials from orbitals: screening functions y^k, the Fock operator, Slater's and the KLI potential (beyond the reference)
 * In the notation of the Slater block (s_i = dr/di, P_xy,i = u_x,i u_y,i with the lower-indexed orbital first, p_i = r_i^k formed as
 * p = 1, then k times p = p * r_i, the increments d_i(g) of the three stencils there, Q[.] with the Simpson 3/8 weights), and with
 * inv_i = 1 / (p_i r_i) for i >= 1, inv_0 = 0:
 *
 * Screening function of a pair x <= y, 0 <= k <= DFTA_SLATER_KMAX:
 *   y^k_xy(r) = Y^k_xy(r) / r = r^(-k-1) Z^k_xy(r) + r^k W^k_xy(r),  Z(r) = Int_0^r t^k P(t) dt,  W(r) = Int_r^inf t^(-k-1) P(t) dt
 *   Z_i exactly as in the Slater block: g_i = (p_i P_i) s_i, Z_0 = 0, Z_i = Sum_{j <= i} d_j(g);
 *   h_i = (P_i inv_i) s_i (so h_0 = 0), e_j = d_j(h) with the same three stencils, W_{N-1} = 0, W_i = Sum_{j > i} e_j: a REVERSE
 *   cumulative sum taken from the outside in, never "total minus prefix";
 *   y_i = Z_i inv_i + p_i W_i for i >= 1 (two products, one sum);  y_0 = W_0 for k = 0 and 0 for k > 0.
 * Y^0_aa / r is the Hartree potential of the density of one electron in orbital a.  Both scans have a fixed shape that depends on N alone
 * (no atomics): a row's bits depend on its two orbitals, k and N -- not on the other jobs of the call, its position
 * among them, or the run; a job (x, y, k) is computed under x <= y, so (y, x, k) returns the same bits.  Nodes beyond an orbital's
 * cut-off are zeros like any others; an all-zero pair gives exactly 0 everywhere.  Any k in 0 .. 8 is accepted; for k > l_x + l_y the
 * integrand of W is singular at the origin (P ~ r^(l_x + l_y + 2)) and the values near the origin are only as good as the grid.  N >= 5.
 *
 * Exchange operator of ONE spin channel with shells a = 0 .. n-1 (n <= 32), angular momenta l_a (0 .. 4), channel occupations n_a >= 0
 * (LSDA: N_a; LDA: N_a / 2) and c_abk = (l_a k l_b; 0 0 0)^2 = dfta_gaunt_3j2, k over the exchange sum of the Slater block:
 *   X_a,i = Sum_b Sum_k (n_b c_abk) (y^k_ab,i u_b,i)     one accumulator from 0.0, b ascending (every b of the channel), then k ascending
 *   D_i   = Sum_a n_a (u_a,i u_a,i)                      one accumulator from 0.0, a ascending       (= 4 pi r^2 rho_sigma)
 *   num_i = Sum_a n_a (u_a,i X_a,i)                      the same
 *   vS_i  = -(num_i / D_i) where D_i > 0, else 0.0       Slater's averaged exchange potential
 *   vbarHF_a = -Q[(u_a X_a) s]                           <a| v_x^HF,a |a>
 *   vbarS_a  = Q[((u_a u_a) vS) s]
 *   S_ab     = Q[(((u_a u_a) (u_b u_b)) / D) s]          the term is 0 where D_i = 0; computed once per a <= b and mirrored
 *   M_ab     = S_ab n_b
 * (u_a X_a is the radial part of u_a times the Fock exchange operator applied to orbital a, sign included in vbarHF.)
 * KLI (Krieger, Li, Iafrate): with h the HOMO of the channel, c_h = 0 and the other c solve (I - M)_red c = (vbarS - vbarHF)_red, rows and
 * columns h removed: host arithmetic in double, Gaussian elimination with partial pivoting -- for every column j ascending the pivot is
 * the row p >= j of largest |A_pj| (the lowest on ties), rows j and p are exchanged; for every row i > j ascending f = A_ij / A_jj, for
 * m > j ascending A_im = A_im - f A_jm, then b_i = b_i - f b_j; back substitution for i descending: t = b_i, for m > i ascending
 * t = t - A_im x_m, x_i = t / A_ii.  Then
 *   vKLI_i = vS_i + (Sum_{a != h} (n_a (u_a,i u_a,i)) c_a) / D_i     one accumulator from 0.0, a ascending; 0.0 where D_i is not > 0
 *   vbarKLI_a = Q[((u_a u_a) vKLI) s]
 * A channel of one shell has an empty system: vKLI = vS bit for bit.  The spherical average treats a shell as a unit (one orbital per
 * shell, occupation n_a), the convention of E_x above.  Up to rounding: Sum_a n_a vbarS_a = Sum_a n_a vbarHF_a; Sum_b M_ab = NORM_a;
 * n_h (vbarKLI_h - vbarHF_h) = Sum_{b != h} n_b c_b (NORM_b - 1), the row that was dropped: vbarKLI_h = vbarHF_h for orbitals normalised
 * under Q.  Sum_a n_a vbarHF_a = 2 E_x of the channel up to the grid's order: Q[P p W s] here and Q[P Z inv s] of the Slater block are two
 * discretisations of one integral (4.5e-15 apart, relative, for a neon-like channel at 4097 logarithmic nodes).  The HOMO of an SCF
 * channel is the shell of highest eigenvalue among those with n_a > 0, the higher index on ties.
 * Q's sums have the fixed shape of the orbital block: lane t of 256 adds the terms of the nodes t, t + 256, ..., then the tree. */
#define DFTA_XP_COLS 4
#define DFTA_XP_HF   0   /* columns of a vbar row: vbarHF_a */
#define DFTA_XP_S    1   /* vbarS_a  */
#define DFTA_XP_C    2   /* the KLI constant c_a (0 for the HOMO) */
#define DFTA_XP_KLI  3   /* vbarKLI_a */
/* host-only: the y jobs of a channel with angular momenta l (0 .. 4), rows x, y, k of three ints: a, then b >= a, then k = |l_a - l_b|,
 * |l_a - l_b| + 2 .. l_a + l_b ascending (b == a: k = 0, 2 .. 2 l_a).  Returns the number of jobs (jobs may be NULL: count only), or -1
 * for norb < 0, l NULL or an l outside 0 .. 4. */
int  dfta_exchange_jobs(int norb, const int* l, int* jobs);
/* every job (x, y, k) of the table in one launch, on caller-supplied orbitals; host pointers.  u: norb x N; y: njobs x N.  njobs == 0:
 * DFTA_OK, nothing is written.  Records the launch's time for dfta_ctx_last_kernel_ms. */
int  dfta_screening_yk(dfta_ctx* ctx, const dfta_grid* g, int norb, const double* u, int njobs, const int* jobs, double* y);
/* ... on the orbitals of an atom of the SCF, read in place; indices count the atom's orbitals, alpha levels then beta levels, as in
 * dfta_scf_slater_rk.  Before the first dfta_scf_step: DFTA_ERR_INVALID.  The job table and the y rows are kept on the device from the
 * first such call on, grown when a longer table comes: njobs x N doubles (at 131 073 nodes 1 MB per job). */
int  dfta_scf_screening_yk(dfta_scf* s, int atom, int njobs, const int* jobs, double* y);
/* the potentials of one channel on caller-supplied orbitals; host pointers.  l, occ: norb; homo: 0 .. norb-1; u: norb x N.  Outputs, any
 * of which may be NULL: X norb x N; D, vS, vKLI N each; vbar norb x DFTA_XP_COLS; M norb x norb, row-major.  Launches: the y jobs of
 * dfta_exchange_jobs, the pointwise pass, the reductions; after the host solve the KLI pass and its reductions.  The events of
 * dfta_ctx_last_kernel_ms bracket the whole sequence.  DFTA_ERR_INVALID: a NULL input, norb outside 1 .. 32, an l outside 0 .. 4, a
 * negative occupation, homo out of range, N < 5, a singular system. */
int  dfta_exchange_potentials(dfta_ctx* ctx, const dfta_grid* g, int norb, const int* l, const double* occ, int homo, const double* u,
                              double* X, double* D, double* vS, double* vKLI, double* vbar, double* M);
/* ... of channel (atom, spin) of the SCF, orbitals read in place, n_a = N_a (LSDA) or N_a / 2 (LDA: spin 0 only), the HOMO by the rule
 * above from the level's eigenvalues (homo, may be NULL: its index).  A channel without levels: DFTA_OK, nothing is written (homo: -1).
 * Before the first dfta_scf_step: DFTA_ERR_INVALID.  A frozen atom keeps its orbitals, hence its potentials.  Device scratch from the
 * first such call on, grown as needed: the y rows of the channel (Rn LDA: 176 jobs, 1 MB each at 131 073 nodes), X (norb x N) and five
 * rows of N. */
int  dfta_scf_exchange_potentials(dfta_scf* s, int atom, int spin, double* X, double* D, double* vS, double* vKLI, double* vbar,
                                  double* M, int* homo);

/* ---- self-consistent exchange-only KLI (beyond the reference) ---------------------------------------------------------------------------
 * A switch on a created SCF, on the model of dfta_scf_set_integrator: with DFTA_EXCHANGE_KLI a step takes its exchange potential from its
 * own orbitals -- the KLI potential of the block above, per spin channel -- instead of v_xc of dfta_scf_options::functional, and adds no
 * correlation.  DFTA_ERR_INVALID (text in dfta_last_error): after the first dfta_scf_step; an unknown value; functional != DFTA_XC_VWN;
 * mixing != DFTA_MIX_LINEAR.  Both kinds of grid.  Creation is unchanged: the start potential is VWN's on the flat start density.  With
 * the switch untouched (or DFTA_EXCHANGE_FUNCTIONAL) every launch and every bit of a step is what it was, and nothing is allocated.
 *
 * A step under DFTA_EXCHANGE_KLI, per live atom:
 *  1. level search and density mix as ever; the orbitals u_a are those of the step's input potential.
 *  2. exchange stage, for every live channel (atom, sigma) with at least one level: occupations and HOMO rule of
 *     dfta_scf_exchange_potentials (LSDA n_a = N_a; LDA spin 0, n_a = N_a / 2); y rows, X_a, D, vS, the quadratures, the reduced system, c
 *     and vKLI as the block above defines them: v_raw, vbarHF and c are bit for bit what dfta_scf_exchange_potentials(s, atom, sigma, ..)
 *     returns on the same state (vKLI; the columns DFTA_XP_HF and DFTA_XP_C of vbar), except:
 *     tail: with i_last the largest node with D > 0, v_raw,i = (v_raw,i_last r_i_last) / r_i for i > i_last -- the Coulomb tail, continuous
 *       at i_last, in place of the 0.0 of vKLI there (one product, one quotient); node 0 and every node i < i_last with D = 0 keep 0.0;
 *     mix: on the first step vx_sigma = v_raw; later vx_sigma,i = alpha vx_sigma,i + (1 - alpha) v_raw,i with the two doubles alpha and
 *       1 - alpha of the density mix, the products rounded separately;
 *     energy: E_x,sigma = 0.5 (Sum_a n_a vbarHF_a), a ascending, one accumulator from 0.0; E_x = 2 E_x,0 (LDA), E_x,alpha + E_x,beta
 *       (LSDA); a channel without levels contributes 0.
 *     A pivot of the reduced system that is zero or not finite: dfta_scf_step returns DFTA_ERR_INVALID.
 *  3. Poisson as ever.
 *  4. in place of the functional's launch: LDA Vexc = vx_0; LSDA va = vx_alpha, vb = vx_beta (a channel without levels: 0),
 *     Vexc = (dA va + dB vb) / rho where rho > 0, else 0 (two products, one sum, one quotient); both: eexc = -Vexc.  The potential and
 *     the integrands follow as ever.
 *  5. energies as ever with eExcDif = 4 pi I[2] + E_x, so that Exc = E_x and Etotal = Eelectronic + Ehartree + eExcDif.
 * A frozen atom is skipped by every kernel of the stage and keeps vx, v_raw and E_x.  All live channels of a step go through one sequence
 * of launches per chunk -- whole channels whose y rows fit a budget (DFTA_DEBUG KLI_Y_MB, MiB, default 1024, read at creation; at least
 * one channel per chunk) -- with no host synchronisation inside the stage; the solve runs on the device and repeats the host solve of
 * the block above operation by operation.  Shapes depend on N alone, no floating-point atomics: a channel's bits do not depend on the
 * batch, its position in it, the chunking or the run.
 * Limits: exchange only (no correlation is added); open-shell atoms whose Aufbau configuration puts a level near zero may not converge
 * (Fe LSDA oscillates). */
#define DFTA_EXCHANGE_FUNCTIONAL 0   /* default: v_xc of dfta_scf_options::functional */
#define DFTA_EXCHANGE_KLI        1   /* exchange-only KLI from the step's orbitals, no correlation */
int  dfta_scf_set_exchange(dfta_scf* s, int exchange);
/* vx, v_raw (N each) of channel (atom, spin) and E_x of the atom after the last step in which the atom was live; any pointer may be NULL.
 * A channel without levels: zeros.  DFTA_ERR_INVALID before the first step or without the switch. */
int  dfta_scf_get_exchange(dfta_scf* s, int atom, int spin, double* vx, double* v_raw, double* Ex);
/* HIP-event time of the last step's exchange stage (all chunks), ms */
int  dfta_scf_exchange_ms(dfta_scf* s, float* ms);
/* the same stage on caller-supplied channels; host pointers.  norb: nch shell counts (0 .. 32; a channel of 0 shells gives zeros, homo -1);
 * l, occ (the channel occupations n_a), E (the eigenvalues the HOMO rule reads): the channels' shells end to end; u: their orbitals end
 * to end, N each.  Every channel with shells needs an occupied one.  first_step != 0: vx = v_raw, vx_inout is written only; otherwise
 * vx_inout (nch x N) is mixed with alpha and 1 - alpha.  Outputs, any of which may be NULL: v_raw nch x N; vbarHF, c per shell; homo and
 * Ex (E_x,sigma) per channel.  A channel whose reduced system has a pivot that is zero or not finite gets c = NaN (hence v_raw = NaN);
 * the other channels are not touched by it.  Chunks as in the SCF (DFTA_DEBUG KLI_Y_MB, read by the call).  The events of
 * dfta_ctx_last_kernel_ms bracket the stage. */
int  dfta_kli_channels(dfta_ctx* ctx, const dfta_grid* g, int nch, const int* norb, const int* l, const double* occ, const double* E,
                       const double* u, int first_step, double alpha, double* vx_inout, double* v_raw, double* vbarHF, double* c, int* homo,
                       double* Ex);

/* ---- self-interaction-corrected LSDA: Perdew-Zunger SIC through KLI (beyond the reference) ----------------------------------------------
 * A third value of the switch above: with DFTA_EXCHANGE_SIC_KLI a step keeps the functional's v_xc (VWN) and adds to it ONE local potential
 * per spin channel that stands for the orbital-dependent Perdew-Zunger corrections v_a^SIC = -(v_H[rho_a] + v_xc[rho_a, 0]), folded together
 * by the KLI construction of the exchange block.  The potential has the -1/r tail and the HOMO eigenvalue approaches -IP; a one-electron
 * atom is free of self-interaction (H: -0.5 Ha).  Refusals as DFTA_EXCHANGE_KLI: after the first dfta_scf_step; functional != DFTA_XC_VWN;
 * mixing != DFTA_MIX_LINEAR.  Both kinds of grid.  Creation is unchanged.  With the switch at 0 or 1 every launch and every bit of a step
 * is what it was.
 *
 * Per live channel (atom, sigma) with shells a = 0 .. n-1, channel occupations n_a (LSDA N_a; LDA spin 0, N_a / 2) and the HOMO rule of
 * the exchange block, in the notation of that block (s_i = dr/di, Q[.] with the Simpson 3/8 weights and the fixed 256-lane shape):
 *   rho_a,i = (u_a,i u_a,i) / ((K r_i) r_i) for i >= 1, K the double nearest 4 pi (one product, then the two products of the divisor,
 *             one quotient); rho_a,0 = 0.0                       the density of ONE electron in shell a
 *   y0_a    = y^0_aa: the row of job (a, a, 0) of dfta_screening_yk, bit for bit              (its Hartree potential)
 *   v_a,i   = va of dfta_vwn_lsda at (rho_a,i, 0.0); eps_a,i = vexc + eexcdif of dfta_vwn_lsda there (one sum): the fully polarised LSDA
 *             potential and energy density per electron of the orbital density, the kernel's own arithmetic (one device function)
 *   X_a,i   = (y0_a,i + v_a,i) u_a,i                             one sum, one product
 *   D, num, vS, vbar_a = -Q[(u_a X_a) s] (the column DFTA_XP_HF: now <a| v_a^SIC |a>), vbarS_a, S_ab, M, the reduced system, c, vKLI, the
 *   Coulomb tail beyond the last node with D > 0 and the mix into vx: exactly those of the exchange block and of DFTA_EXCHANGE_KLI, the
 *   same kernels for the solve and the update.  vS = -(num / D) is the density-weighted average of the v_a^SIC.
 *   EH_a    = 0.5 Q[((u_a u_a) y0_a) s]                          (the factor applied to the finished quadrature)
 *   EXC_a   = Q[((u_a u_a) eps_a) s]
 *   E_SIC,sigma = -(Sum_a n_a (EH_a + EXC_a))                    one accumulator from 0.0, a ascending
 *   E_SIC   = 2 E_SIC,0 (LDA), E_SIC,alpha + E_SIC,beta (LSDA); a channel without levels contributes 0.
 * The step: level search, mix, Poisson and the functional's launch on the mixed densities as ever; then one more launch adds the SIC
 * potential for every atom that has not finished:
 *   LDA:  Vexc = Vexc + vx_0, eexc = eexc - vx_0;
 *   LSDA: va = va + vx_alpha, vb = vb + vx_beta; t = (dA vx_alpha + dB vx_beta) / rho where rho > 0, else 0.0 (two products, one sum, one
 *         quotient); Vexc = Vexc + t, eexc = eexc - t.
 * The potential and the integrands follow as ever; the energies with eExcDif = 4 pi I[2] + E_SIC.  A frozen atom is in no launch of the
 * stage and keeps vx, v_raw, E_SIC and its per-shell table.  A pivot that is zero or not finite: as DFTA_EXCHANGE_KLI.  Chunks: whole
 * channels whose y rows (one per shell) fit the budget of DFTA_EXCHANGE_KLI (DFTA_DEBUG KLI_Y_MB); no host synchronisation inside the
 * stage, no floating-point atomics, shapes depend on N alone: a channel's bits do not depend on the batch, its position, the chunking or
 * the run.  dfta_scf_get_exchange and dfta_scf_exchange_ms work under this value (the E_x slot holds E_SIC).
 * Limits: VWN only (no SIC of PW92 / PBE); spherically averaged shells as the orbitals (one orbital density per shell, no unitary
 * optimisation of the orbitals); linear mixing only. */
#define DFTA_EXCHANGE_SIC_KLI    2   /* v_xc of VWN plus the Perdew-Zunger self-interaction correction as one KLI potential per channel */
/* per shell of channel (atom, spin) after the last step in which the atom was live: EH_a, EXC_a, vbar_a = <a| v_a^SIC |a>, c_a (cnt doubles
 * each, cnt = dfta_scf_num_levels), homo: the HOMO's index (-1: no levels).  Any pointer may be NULL.  DFTA_ERR_INVALID before the first
 * step or without DFTA_EXCHANGE_SIC_KLI. */
int  dfta_scf_sic_table(dfta_scf* s, int atom, int spin, double* EH, double* EXC, double* vbar, double* c, int* homo);
/* the stage on caller-supplied channels, arguments as dfta_kli_channels.  Further outputs, any of which may be NULL: y0, vorb, eps, X
 * (shells x N each: y0_a, v_a, eps_a, X_a); D, vS (nch x N, before the tail: vS of a node with D = 0 is 0.0); EH, EXC and vbarS per
 * shell; M: the channels' matrices end to end, norb x norb row-major each, M_ab = S_ab n_b formed on the host from the one S_ab of a pair;
 * Esic (E_SIC,sigma) per channel. */
int  dfta_sic_channels(dfta_ctx* ctx, const dfta_grid* g, int nch, const int* norb, const int* l, const double* occ, const double* E,
                       const double* u, int first_step, double alpha, double* vx_inout, double* y0, double* vorb, double* eps, double* X,
                       double* D, double* vS, double* v_raw, double* vbar, double* c, double* EH, double* EXC, int* homo, double* Esic,
                       double* vbarS, double* M);

/* ---- Bessel transforms: X-ray form factors and momentum-space orbitals (beyond the reference) -------------------------------------------
 * With Q[.], s_i = dr/di and the weights of the orbital block, a row f of N doubles, x_i = q r_i (one product, rounded once) and w_i the
 * weight of node i WITHOUT the factor 3/8 (1 at the two end nodes, 2 where i % 3 == 0, 3 elsewhere):
 *   DFTA_BT_DENSITY  out = 4 pi Q[f r^2 j_l(q r) s]:        g_i = w_i (((f_i r_i) r_i) s_i),   out = ((Sum_i g_i j_l(x_i)) (3/8)) K_D
 *   DFTA_BT_ORBITAL  out = sqrt(2/pi) Q[f r j_l(q r) s]:    g_i = w_i ((f_i r_i) s_i),         out = ((Sum_i g_i j_l(x_i)) (3/8)) K_O
 * K_D and K_O are the doubles nearest 4 pi and sqrt(2 / pi); both constant factors are applied once, to the finished sum.  A node whose
 * g_i is zero adds nothing (its Bessel values are not formed): nodes beyond an orbital's cut-off index, an underflowed density tail.
 * With f = rho and l = 0 the first is the X-ray form factor f(q) = 4 pi Int rho(r) j_0(q r) r^2 dr (f(0): the electron count; with a
 * spin density the magnetic form factor), with f = u_nl = r R_nl and l the orbital's the second is the momentum-space radial function
 * R~_nl(p) = sqrt(2/pi) Int R_nl(r) j_l(p r) r^2 dr (sign as u's, no factor (-i)^l).
 *
 * j_l(x), 0 <= l <= DFTA_BESSEL_LMAX, x >= 0, as the device evaluates it:
 *   x == 0 (q = 0 or node 0; -0 too): exactly 1 for l = 0, exactly 0 for l >= 1;
 *   l = 0: sin(x) / x;
 *   l >= 1, x < 3: the ascending series x^l / (2l+1)!! Sum_k t_k, t_0 = 1, t_k = t_{k-1} (-x^2 / 2) / (k (2l + 2k + 1)), 14 terms
 *       (k = 0 .. 13), nested: with y = (x x) (-1/2), c_k the double nearest 1 / (k (2l + 2k + 1)) and d_l the double nearest
 *       1 / (2l+1)!!:  h = 1 + y c_13;  h = 1 + (y c_k) h for k = 12 .. 1;  p = x, then l - 1 times p = p x;  j_l = (p d_l) h;
 *   l >= 1, x >= 3: one sincos, rx = 1 / x, j_0 = sin rx, j_1 = (j_0 - cos) rx, and upward j_{k+1} = ((2k+1) rx) j_k - j_{k-1}.
 * (At x = 3 both branches are within a few 1e-16 of j_l; the recurrence alone is 3e-4 wrong at x = 0.1 for l = 4, the series alone
 * loses three digits by x = 6: tests/test_bessel_ref.py measures both on a dense ladder.)
 *
 * Sums have a fixed shape that depends on N alone (no floating-point atomics): a (row, q) value depends on that row's
 * N numbers, its l, the kind, q and the grid -- not on the other rows or q's of the call, their number or order, or the run.  A NaN
 * inside a row makes that row's outputs NaN and no other's.  The grid samples f j_l: q (r_{i+1} - r_i) << 1 is needed where f lives
 * (a diffuse orbital at large q aliases -- a property of the grid, not of the sum).
 * DFTA_ERR_INVALID: a NULL pointer, kind outside {0, 1}, an l outside 0 .. 4, a q (or x) that is negative, NaN or infinite, N < 5.
 * nq == 0 or nrow == 0: DFTA_OK, nothing is written.  All four entries record the launch's time for dfta_ctx_last_kernel_ms. */
#define DFTA_BT_DENSITY 0
#define DFTA_BT_ORBITAL 1
#define DFTA_BESSEL_LMAX 4
/* pointwise j_l(x) of n arguments (tests and tools); host pointers */
int  dfta_sph_bessel(dfta_ctx* ctx, int l, size_t n, const double* x, double* out);
/* every (row, q) in one launch, on caller-supplied rows; host pointers.  l: nrow; f: nrow x N; q: nq; out: nrow x nq */
int  dfta_bessel_transform(dfta_ctx* ctx, const dfta_grid* g, int kind, int nrow, const int* l, const double* f, int nq, const double* q,
                           double* out);
/* form factors of the densities of every atom of the batch, read in place, one launch: out natoms x nchan x nq (host), nchan = 1 for
 * LDA (rho), 3 for LSDA (rho, rho_a, rho_b) -- the arrays dfta_scf_get_array(.., 0 / 1 / 2) returns at the time of the call (after a
 * step: the mixed density, the next step's input).  Valid from creation on: the start density has a form factor too. */
int  dfta_scf_form_factors(dfta_scf* s, int nq, const double* q, double* out);
/* R~_nl(q) of every orbital of the batch, read in place, one launch: out njobs x nq (host), rows as dfta_scf_orbital_properties lists
 * them, each with its own l.  Before the first dfta_scf_step: DFTA_ERR_INVALID. */
int  dfta_scf_momentum_orbitals(dfta_scf* s, int nq, const double* q, double* out);

/* ---- continuum orbitals: outward sweeps, phase shifts, photoionization (beyond the reference's live code) -------------------------------
 * The outward integration of the radial equation from the nucleus to a caller-given end node, at ANY finite energy: logarithmic
 * derivatives u'/u, node counts, scattering phase shifts, energy-normalised continuum orbitals and their overlap / dipole sums with
 * bound orbitals.  The reference's own outward sweep, Numerov::SolveSchrodingerCountNodesFromNucleus (Numerov.h:204-270), is dormant
 * there; this block keeps its transformation (Numerov.h:96-101) and replaces its start (u_1 = r^(l+1), w_0 = 0) by a power series.
 * One trial = (potential, l, E, end node m), 0 <= l <= 4, 3 <= m <= N-2; one lane per trial, the 64 lanes of a wave marching the node
 * index together.
 *
 * Tables: r_i and s_i = dr/di of the orbital block (logarithmic grid: (Rp delta) exp(i delta), uniform grid: h); c = delta^2 / 4 and
 * lam = delta on the logarithmic grid, c = lam = 0 on the uniform one.  Per node i >= 1 of a (potential, l), the same in every trial:
 *   s2_i = s_i s_i;  q_i = sqrt(s_i);  vl_i = V_i + ((L / (r_i r_i)) 0.5) with L = l (l + 1.) (l = 0: vl_i = V_i + 0.0).
 * Per trial, with y_i = u(r_i) / q_i:
 *   f_i = (2 (vl_i - E)) s2_i + c        (the equation is y'' = f y in the index)
 *   d_i = 1 - f_i / 12
 * Start, nodes 1 and 2, from the fit V_i = -Zc / r_i + v0 at those two nodes:
 *   Zc = ((V_2 - V_1) (r_1 r_2)) / (r_2 - r_1);  v0 = V_1 + Zc / r_1;
 *   a_0 = 1;  a_1 = -Zc / (l + 1);  a_k = (((-2 Zc) a_{k-1}) + ((2 (v0 - E)) a_{k-2})) / (k (k + 2l + 1)), k = 2, 3, 4 (the divisor exact);
 *   u_i = p_i ((((a_4 r_i + a_3) r_i + a_2) r_i + a_1) r_i + a_0),  p_i = r_i^(l+1) by l products from r_i;
 *   y_i = u_i / q_i;  w_i = d_i y_i.          (V = 0 gives Zc = v0 = 0; the Coulomb cusp of l = 0 is right.)
 * Recurrence, i = 3 .. m+1:
 *   w_i = ((2 w_{i-1}) - w_{i-2}) + f_{i-1} y_{i-1};  y_i = w_i / d_i.
 * End node m:
 *   y'_m = (((1 - f_{m+1} / 6) y_{m+1}) - ((1 - f_{m-1} / 6) y_{m-1})) 0.5          (Numerov's O(h^4) derivative)
 *   u_m = q_m y_m;  u'_m = (y'_m + (lam 0.5) y_m) / q_m;  logderiv = u'_m / u_m;
 *   nodes = the number of i in 2 .. m with (y_i < 0) != (y_{i-1} < 0).
 * status (0: fine): DFTA_CONT_NONFINITE -- a y_i, 1 <= i <= m+1, was not finite; DFTA_CONT_STEP -- d_i > 0 failed for an i in 3 .. m+1
 * (a NaN node of the potential does that).  With either bit every floating-point output of the trial is NaN and nodes is -1.
 *
 * Normalisation, E > 0 only: k = sqrt(2 E), x = k r_m, U = u'_m / k.  E <= 0: factor = 1 and delta_or_phase = scale = 0.0; logderiv,
 * nodes, sums and rows stay valid (unnormalised).  scale = factor.
 *   DFTA_CONT_FREE (short-range potentials: neutral atoms under an LDA or GGA): matching to the Riccati functions jh_l = x j_l(x), with
 *     j_l the device's (the Bessel block), and yh_l: yh_0 = -cos x, yh_1 = yh_0 / x - sin x, yh_{n+1} = ((2n+1) / x) yh_n - yh_{n-1};
 *     jh'_l = x j_{l-1}(x) - (l / x) jh_l, yh'_l = yh_{l-1} - (l / x) yh_l; l = 0: jh' = cos x, yh' = sin x.
 *     a = u_m yh' - U yh;  b = U jh - u_m jh';  delta_l = atan2(-b, a) in (-pi, pi];  factor = sqrt(2 / (pi k)) / hypot(a, b).
 *   DFTA_CONT_WKB (any tail: ions, KLI, SIC-KLI): kap2_i = (2 (E - V_i)) - L / (r_i r_i) at i = m-1, m, m+1; all three must be > 0,
 *     otherwise status has DFTA_CONT_WKB_TAIL, logderiv and nodes stay and the normalised outputs are NaN.  kap_i = sqrt(kap2_i);
 *     kp = (kap_{m+1} - kap_{m-1}) / (r_{m+1} - r_{m-1});  al = 1 / sqrt(kap_m);  alp = -kp / ((2 kap_m) kap_m^(1/2));
 *     A = u_m / al;  B = al u'_m - alp u_m;  factor = sqrt(2 / pi) / hypot(A, B);  phase = atan2(A, B): the phase of the WKB form
 *     u = C al sin(phase) at r_m -- no phase shift (that needs Coulomb functions), but the amplitude is the energy-normalised one.
 *   atan2(y, x) in both modes: t = the device's atan2(min(|y|, |x|), max(|y|, |x|)), the first octant only; |y| > |x|: t <- pi/2 - t;
 *     the sign bit of x set: t <- pi - t; the result takes the sign of y.  Both subtractions carry the constant as two doubles
 *     (s = hi - t and its exact error, then the tails), so the reconstruction adds one rounding: a phase near pi/2 or pi is not off
 *     by the 0.28 ulp that the one double nearest pi is short.
 *   DFTA_CONT_NORM (E > 0, either mode): an operand of the hypot (a or b, A or B) is NaN, or the computed factor is not finite.  Then
 *     delta_or_phase, scale, the sums and the rows are NaN; logderiv and nodes stand.  The floor: for l >= 3 the free normalisation
 *     leaves double range below roughly E ~ 1e-150 .. 1e-200 (yh_l ~ x^-l overflows and a = inf - inf).  Before that yh'_l alone
 *     overflows (l = 4, r_m = 25: from E ~ 4e-126 on), hypot is inf and factor = scale = 0.0 WITHOUT a bit: an underflow, although the
 *     true factor is a normal double (1e-286 .. 1e-307) down to E ~ 1e-135.  Treat scale == 0.0 at E > 0 as "below double range".
 * Normalised, u_E(r) -> sqrt(2 / (pi k)) sin(k r - l pi / 2 + delta_l): Int u_E u_E' dr = delta(E - E').
 *
 * Partner sums (overlap and dipole integrals with bound orbitals), fused into the sweep.  Partner rows P_b (N doubles each), a power
 * 0 <= p <= 8: g_b,i = w_i ((P_b,i rp_i) s_i) with w_i the weight of node i without 3/8 (the Bessel block's) and rp_i = r_i^p by p
 * products from 1;  S_t,b = ((Sum_{1 <= i <= m} g_b,i (q_i y_i)) (3/8)) factor_t.  The sum is taken sequentially inside blocks of 256
 * nodes (256 k .. 256 k + 255), and the blocks' sums are added in order: the shape depends on m alone.  Every trial names one partner
 * list (or none); a list holds at most DFTA_CONT_MAX_PARTNERS rows.  Rows: u_t,i = (q_i y_i) factor_t for 1 <= i <= m+1, 0.0 at node 0
 * and beyond m+1.
 * The first steps of the recurrence at high l on the logarithmic grid (f_i ~ l (l+1) / i^2) admix the irregular solution, which dies
 * as (r_1 / r)^(2l+1): the SCALE of the unnormalised solution carries that error (1e-4 for l = 4 at 4097 nodes), so compare only
 * scale-free (logderiv, nodes, delta) and normalised quantities.
 * A trial's bits depend on its potential, l, E, m, its partners and the grid -- not on the other trials of the call, their number or
 * order, the instance of the kernel (0, 4, 8 or 16 partner accumulators), whether rows were asked for, or the run.  No atomics.
 * DFTA_ERR_INVALID: a NULL pointer, a mode outside {0, 1}, an l outside 0 .. 4, an m outside 3 .. N-2, a non-finite E, more than 16
 * partners in a list, an index out of range, N < 5.  ntrials == 0: DFTA_OK, nothing is written.  Every entry records the sweep's
 * time for dfta_ctx_last_kernel_ms. */
#define DFTA_CONT_FREE 0
#define DFTA_CONT_WKB  1
#define DFTA_CONT_MAX_PARTNERS 16
#define DFTA_CONT_NONFINITE 1
#define DFTA_CONT_STEP      2
#define DFTA_CONT_WKB_TAIL  4
#define DFTA_CONT_NORM      8
/* on caller-supplied potentials and partner rows; host pointers.  V: nV x N; vidx (NULL: 0), l, E, m: ntrials; P: npartner_rows x N
 * (NULL with 0 rows); list k holds the rows list_rows[list_off[k] .. list_off[k+1] - 1], trial_list[t] (NULL: none) is the list of trial
 * t or -1.  Outputs per trial, any of which may be NULL: logderiv, nodes, delta_or_phase, scale, status; sums ntrials x 16 (entries
 * beyond the trial's list: 0.0); rows ntrials x N. */
int  dfta_continuum(dfta_ctx* ctx, const dfta_grid* g, int norm_mode, int nV, const double* V, int ntrials, const int* vidx, const int* l,
                    const double* E, const int* m, int npartner_rows, const double* P, int power, int nlists, const int* list_off,
                    const int* list_rows, const int* trial_list, double* logderiv, int* nodes, double* delta_or_phase, double* scale,
                    int* status, double* sums, double* rows);
/* ... on the batch's resident potentials, read in place: trial t runs in the potential of (atom[t], spin[t]), the array
 * dfta_scf_get_array(.., 3 / 4) returns at the time of the call.  power < 0: no partners.  Otherwise the partners of a trial are the
 * orbitals of its channel, in the order of dfta_scf_get_levels, with l_b = l - 1 or l + 1 for power == 1 and l_b = l for any other
 * power; partner_index (may be NULL): ntrials x 16, the level index of each column of sums within the channel, -1 beyond the list.
 * Mind the orbital block: the orbitals belong to the last step's INPUT potential, the resident potential is the NEXT step's input; at
 * convergence the two agree to the SCF's tolerance.  Before the first dfta_scf_step a call with power >= 0 returns DFTA_ERR_INVALID. */
int  dfta_scf_continuum(dfta_scf* s, int norm_mode, int ntrials, const int* atom, const int* spin, const int* l, const double* E,
                        const int* m, int power, double* logderiv, int* nodes, double* delta_or_phase, double* scale, int* status,
                        double* sums, int* partner_index, double* rows);
/* Photoionization cross sections of every subshell of an atom on a common grid of photoelectron energies eps (neps values > 0), in
 * a_0^2, from ONE launch: the trials (spin, l' = 0 .. 4, eps) with end node N-2 and the dipole sums (power 1) of dfta_scf_continuum.
 * For the subshell of job j of the atom (alpha levels, then beta levels: the order of dfta_scf_orbital_properties) with eigenvalue E_j,
 * angular momentum l and occupation occ (dfta_scf_get_occupations), omega = eps - E_j and, host arithmetic in double in this order,
 *   sigma = (((K omega) / 3) (occ / (2l + 1))) ((l (S_{l-1} S_{l-1})) + ((l + 1) (S_{l+1} S_{l+1}))),  K = (4 (pi pi)) alpha,
 * alpha = 1 / 137.035999084, S_{l'} the subshell's sum in the trial (its spin, l', eps); the S_{l-1} term is absent for l = 0, the
 * S_{l+1} term for l = 4.  omega_out, sigma_out: njobs_of_the_atom x neps.  A trial with a status bit makes its sigma NaN. */
int  dfta_scf_photoionization(dfta_scf* s, int atom, int neps, const double* eps, int norm_mode, double* omega_out, double* sigma_out);

/* ---- Troullier-Martins pseudization of valence orbitals (beyond the reference) ------------------------------------------------------------
 * N. Troullier and J. L. Martins, Phys. Rev. B 43, 1993 (1991).  One channel = a valence level (l, eps, u = r R of N doubles) in a
 * screened all-electron potential V (N doubles, Hartree: -u''/2 + [l(l+1)/2r^2 + V] u = eps u) and a core node ic, 3 <= ic <= N-4,
 * r_c = r_ic; 0 <= l <= 4.  Tables s_i = dr/di and lam of the continuum block.  sigma = 1 if u_ic > 0, else -1.
 *   outside, i >= ic:  u_ps,i = sigma u_i,  V_ps,i = V_i                                   (copies: bit for bit)
 *   inside,  i <  ic:  x_i = r_i rinv, rinv = 1 / r_c;  t = x_i x_i;
 *                      p = a0 + t (a2 + t (a4 + t (a6 + t (a8 + t (a10 + t a12)))));
 *                      u_ps,i = rp_i exp(p), rp_i = r_i^(l+1) by l products from r_i       (u_ps,0 = 0)
 *                      q = cq_1 + t (cq_2 + t (.. + t cq_6)), cq_k = (2k) a_2k;   w likewise with cw_k = (2k (2k-1)) a_2k;
 *                      V_ps,i = eps + (((l + 1) q) + ((w + t (q q)) 0.5)) / (r_c r_c)      (q = (p'/r) r_c^2, w = p'' r_c^2: no division
 *                      by r; node 0: eps + (2l + 3) a2 / r_c^2)
 * Matching values at r_c, with su_k = sigma u_{ic+k} and the five-point differences in the index
 *   D1[f] = (8 (f_1 - f_-1) - (f_2 - f_-2)) / 12,   D2[f] = ((16 (f_1 + f_-1) - (f_2 + f_-2)) - 30 f_0) / 12,   s = s_ic:
 *   u' = D1[su] / s;  V' = D1[V] / s;  V'' = (D2[V] - lam D1[V]) / (s s);  L = l + 1;  rcp = r_c^(l+1) by l products;
 *   p0 = log(su_0 / rcp);  p1 = u' / su_0 - L / r_c;
 *   p2 = ((2 (V_ic - eps)) - ((2 L) p1) / r_c) - p1 p1;
 *   p3 = (((2 V') + ((2 L) p1) / rc2) - ((2 L) p2) / r_c) - (2 p1) p2;
 *   p4 = ((((2 V'') - ((4 L) p1) / rc3) + ((4 L) p2) / rc2) - ((2 L) p3) / r_c) - (2 (p2 p2) + (2 p1) p3);
 *   rc2 = r_c r_c, rc3 = rc2 r_c, rc4 = rc2 rc2;   P0 = p0, P1 = p1 r_c, P2 = p2 rc2, P3 = p3 rc3, P4 = p4 rc4    (derivatives in x).
 * Coefficients of a trial a2:  a4 = -((a2 a2) / (2l + 5))        (zero curvature of V_ps at the origin: a2^2 + (2l+5) a4 = 0)
 *   b = (P0 - (a2 + a4), P1 - (2 a2 + 4 a4), P2 - (2 a2 + 12 a4), P3 - 24 a4, P4 - 24 a4); the unknowns (a0, a6, a8, a10, a12) solve
 *   the rows (1 1 1 1 1), (0 6 8 10 12), (0 30 56 90 132), (0 120 336 720 1320), (0 360 1680 5040 11880) = b by Gaussian elimination
 *   on the augmented matrix: for column k = 0 .. 4, each row i = k+1 .. 4 in turn changes places with row k if |A_ik| > |A_kk|; then
 *   m = A_ik / A_kk, A_ij = A_ij - m A_kj for j = k+1 .. 5; back substitution x_k = (A_k5 - A_k,k+1 x_k+1 - .. ) / A_kk, the products
 *   subtracted in ascending j.
 * Norm: f_i = (u_i u_i) s_i with u the all-electron orbital (I_AE) or u_ps below ic and u from ic on (I_ps); d_i the increment of the
 *   cumulative integral of the screening block (1 <= i <= ic: it reads f_{i-2} .. f_{i+1}; i = 1: f_0 .. f_3); lane t of 256 adds d_i of
 *   the nodes i = t, t + 256, .. in order from 0.0, then the tree of the orbital block (xor shuffles 32 .. 1, (w0 + w1) + (w2 + w3)).
 *   g(a2) = log(I_ps(a2)) - log(I_AE).
 * Root search, sgn(g) in {-1, 0, 1}, a NaN g is no sign:  g(0) NaN: DFTA_PS_NOBRACKET.  sgn g(0) = 0: a2 = 0.  Otherwise bracket: for
 *   h = 1/4, 1/2, 1, .. (24 values) evaluate g(h), then g(-h); the first value that is not NaN and whose sign differs from g(0)'s closes
 *   the bracket: hi = that a2, lo = the last a2 of the same side whose g was not NaN (0 at the start).  None: DFTA_PS_NOBRACKET.
 *   Bisection while g(hi) != 0: mid = lo + (hi - lo) 0.5; stop if mid == lo or mid == hi (no double between the ends); stop with
 *   DFTA_PS_CAP if 200 evaluations were made; a NaN g(mid): DFTA_PS_NOBRACKET; mid replaces lo if sgn g(mid) = sgn g(0), else hi.  The
 *   end of smaller |g| is kept (lo on a tie); one more evaluation there gives the coefficients, I_ps and g that are returned.  iters
 *   counts every evaluation.
 * status (0: fine): DFTA_PS_NOBRACKET, DFTA_PS_CAP; DFTA_PS_NODES -- ic is not beyond the last i >= 2 where u_i and b are of strictly
 *   opposite sign, b = u_{i-1}, or u_{i-2} where u_{i-1} is exactly zero; or u_ic = 0; DFTA_PS_NONFINITE -- eps or a node of u or V is not finite (the only bit then); DFTA_PS_NOTPOSITIVE --
 *   u_ps,i > 0 and finite failed for an i in 1 .. ic-1.  With any bit set every floating-point output of the channel is NaN.
 * match (DFTA_PS_MATCH doubles per channel): P0 .. P4, I_AE, I_ps, g.  coef: a0, a2, .., a12.
 * One workgroup of 256 lanes per channel, one launch per call, no atomics: a channel's bits depend on its own rows, l, eps, ic and
 * the grid -- not on the other channels, their number or order, or the run.  DFTA_ERR_INVALID: a NULL input, an l outside 0 .. 4, an ic
 * outside 3 .. N-4, N < 8.  nch == 0: DFTA_OK, nothing is written.  Records the launch's time for dfta_ctx_last_kernel_ms. */
#define DFTA_PS_COEF  7
#define DFTA_PS_MATCH 8
#define DFTA_PS_NOBRACKET   1
#define DFTA_PS_CAP         2
#define DFTA_PS_NODES       4
#define DFTA_PS_NONFINITE   8
#define DFTA_PS_NOTPOSITIVE 16
/* host pointers.  V, u: nch x N (a row of each per channel); l, eps, ic: nch.  Outputs, any of which may be NULL: u_ps, V_ps nch x N;
 * coef nch x 7; rc nch; match nch x 8; iters, status nch. */
int  dfta_pseudize(dfta_ctx* ctx, const dfta_grid* g, int nch, const double* V, const double* u, const int* l, const double* eps,
                   const int* ic, double* u_ps, double* V_ps, double* coef, double* rc, double* match, int* iters, int* status);
/* Unscreening and Kleinman-Bylander quantities of pseudized channels; host pointers.  Channel k belongs to atom[k] (0 .. natoms-1) with
 * occupation occ[k] > 0; u_ps, V_ps: nch x N (the rows of dfta_pseudize); a0: its first coefficient per channel.  K the double nearest
 * 4 pi; sums over the channels of an atom in the order of the call, one accumulator from 0.0, every product rounded on its own:
 *   rho_v,i = Sum occ ((u u) / ((K r_i) r_i)) for i >= 1;  node 0: the term is exp(2 a0) / K for l = 0 and 0.0 otherwise
 *   y_k     = y^0_kk: the row of job (k, k, 0) of dfta_screening_yk on the pseudo-orbitals, bit for bit;  vH,i = Sum occ y_k,i
 *   vxc     = Vexc of the functional's own launcher on rho_v (natoms x N): DFTA_XC_VWN, DFTA_XC_PW92, or DFTA_XC_PBE (logarithmic grid)
 *   V_ion,k = (V_ps,k - vH) - vxc              no nonlinear core correction
 *   local channel of an atom: the first channel with l = l_loc[atom]; l_loc NULL or negative: the first channel of its highest l
 *   beta_k  = (V_ion,k - V_ion,loc) u_ps,k     (V_ion,loc formed again from the local channel's V_ps: the same bits)
 *   q1 = <u|dV|u> = Q[(beta u) s], q2 = <u|dV^2|u> = Q[(beta beta) s] with the weights and the fixed 256-lane tree of the orbital block;
 *   kb (3 doubles per channel): q1, q2, E_KB = q2 / q1 (the local channel: 0, 0, NaN).  The normalised projector is beta / sqrt(q2).
 * Outputs, any of which may be NULL: rho_v, vH, vxc natoms x N; V_ion, beta nch x N; kb nch x 3.  Launches: the y jobs, the density, the
 * functional, the pointwise pass, the quadratures; no atomics, shapes depend on N alone.  An atom's bits do not depend on the other
 * atoms of the call.  DFTA_ERR_INVALID: a NULL input, an atom index out of range, an l outside 0 .. 4, an occupation that is not
 * positive (an unoccupied level), an atom without channels or without a channel of its l_loc, another functional, N < 8. */
int  dfta_pseudo_ionic(dfta_ctx* ctx, const dfta_grid* g, int functional, int natoms, int nch, const int* atom, const int* l, const double* occ,
                       const double* a0, const double* u_ps, const double* V_ps, const int* l_loc, double* rho_v, double* vH, double* vxc,
                       double* V_ion, double* beta, double* kb);
/* ... of levels of the batch, orbitals and potentials read in place on the device: channel k is level level[k] (the index within
 * dfta_scf_get_levels(atom[k], 0)) of atom[k]; l, eps and the occupation are the level's.  WHICH POTENTIAL: the resident one, the array
 * dfta_scf_get_array(.., 3) returns at the time of the call -- after a step that is the NEXT step's input, while the orbitals are
 * eigenfunctions of the last step's input potential (the orbital block's warning), which the SCF does not keep; at convergence the two
 * agree to the SCF's tolerance, and the mismatch enters V_ps inside r_c through p''.  The result is bit for bit dfta_pseudize on
 * dfta_scf_get_orbitals and dfta_scf_get_array(.., 3), then dfta_pseudo_ionic with the SCF's functional.  A frozen atom keeps its
 * orbitals and its potential, hence every bit of its channels.  ic NULL: the core nodes of dfta_pseudo_default_ic(factor); ic_used
 * (may be NULL): the core nodes used.  The atoms in use are numbered in the order of their first channel: l_loc (NULL: the highest l)
 * and the rows of rho_v, vH, vxc follow that numbering.  Any output may be NULL; without an output of dfta_pseudo_ionic only the
 * pseudization runs.  DFTA_ERR_INVALID: an LSDA batch, an exchange mode other than DFTA_EXCHANGE_FUNCTIONAL, a functional other than
 * VWN, PW92, PBE, a call before the first dfta_scf_step, an atom or level out of range, an unoccupied level, and what dfta_pseudize and
 * dfta_pseudo_ionic refuse (l > 4, ic closer than 3 nodes to an end). */
int  dfta_scf_pseudopotentials(dfta_scf* s, int nch, const int* atom, const int* level, const int* ic, double factor, const int* l_loc,
                               int* ic_used, double* u_ps, double* V_ps, double* coef, double* rc, double* match, int* iters, int* status,
                               double* rho_v, double* vH, double* vxc, double* V_ion, double* beta, double* kb);
/* the valence levels of a configuration (host integers only): for each l the level with occ > 0 of largest n, kept if
 * n >= n_max - max(0, l - 1), n_max the largest n with occ > 0 (Fe: 3d 4s; Ar: 3s 3p).  pick: the kept indices into the list, ascending
 * in l; npick: their number.  DFTA_ERR_INVALID: a NULL pointer, a negative l, more than cap levels kept. */
int  dfta_pseudo_default_valence(int nlev, const int* n, const int* l, const int* occ, int cap, int* pick, int* npick);
/* the default core node of each of nch orbitals u (nch x N, host): the node whose r is nearest to factor x r_peak (r_peak: DFTA_ORB_RPEAK's
 * definition, the lower node on a tie), moved outwards until it lies beyond the last sign change of u and u is non-zero there, clamped
 * to 3 .. N-4.  Host only.  DFTA_ERR_INVALID: a NULL pointer, a factor that is not finite and positive, N < 8. */
int  dfta_pseudo_default_ic(const dfta_grid* g, int nch, const double* u, double factor, int* ic);

/* ---- Kleinman-Bylander form: nonlocal radial solves, bound states of H_KB, ghost states (beyond the reference) -------------------------
 * L. Kleinman and D. M. Bylander, Phys. Rev. Lett. 48, 1425 (1982); X. Gonze, P. Kaeckell and M. Scheffler, Phys. Rev. B 41, 12264 (1990).
 * One channel = a local potential Vloc (N doubles), 0 <= l <= 4, a projector row beta (N doubles) and q1 != 0:
 *   H = -1/2 d^2/dr^2 + l(l+1)/2r^2 + Vloc + |beta><beta| / q1.
 * One trial = (channel, E, end node m), 3 <= m <= N-2 and m at or beyond the last node where beta is not 0.0 (so that the sums below
 * are complete; a NaN is not 0.0).  One lane per trial marches TWO solutions of the local equation outwards, both regular at the nucleus:
 *   u_h: (H_loc - E) u_h = 0       every operation of the continuum block on (Vloc, l, E): s2_i, q_i, vl_i, f_i, d_i, the start, the
 *                                  recurrence; written yh_i = u_h,i / q_i, wh_i here;
 *   u_p: (H_loc - E) u_p = -beta   in the index variable yp'' = f yp + G with G_i = ((2 beta_i) s_i) q_i and G12_i = G_i / 12:
 *     Numerov's form is wp_i = d_i yp_i - G12_i with wp_{i+1} - 2 wp_i + wp_{i-1} = f_i yp_i + G_i.
 *     Start, nodes i = 1 and 2, from the leading term of the series, u_p = 2 B r^(l+3) / (4l + 6) where beta = B r^(l+1):
 *       B = beta_1 / p_1;  u_p,i = (((2 B) p_i) (r_i r_i)) / (4l + 6)   (p_i = r_i^(l+1) by l products from r_i, the divisor exact);
 *       yp_i = u_p,i / q_i;  wp_i = d_i yp_i - G12_i.
 *     Recurrence, i = 3 .. m+1:  wp_i = ((2 wp_{i-1}) - wp_{i-2}) + (f_{i-1} yp_{i-1} + G_{i-1});  yp_i = (wp_i + G12_i) / d_i.
 *     (Any regular particular solution serves: two of them differ by a multiple of u_h, which the combination below removes.)
 * Projector sums, in the partner-sum shape of the continuum block at power 0: gb_i = w_i ((beta_i 1.) s_i), w_i the weight of node i
 * without 3/8;  B_h = (Sum_{1 <= i <= m} gb_i (q_i yh_i)) (3/8), B_p likewise with yp: sequential inside blocks of 256 nodes
 * (256 k .. 256 k + 255), the blocks' sums added in order.  (B_h is bit for bit the sum of dfta_continuum with the partner beta at E <= 0.)
 * End node m, per chain as the continuum block, the source's term kept:
 *   yh'_m = (((1 - f_{m+1} / 6) yh_{m+1}) - ((1 - f_{m-1} / 6) yh_{m-1})) 0.5
 *   yp'_m = ((((1 - f_{m+1} / 6) yp_{m+1}) - G_{m+1} / 6) - (((1 - f_{m-1} / 6) yp_{m-1}) - G_{m-1} / 6)) 0.5
 *   u_x,m = q_m yx_m;  u_x'_m = (yx'_m + (lam 0.5) yx_m) / q_m     for x = h, p.
 * The combination, continuous in E (the solution u_h + c u_p with c = B_h / D of (H - E) u = 0, multiplied through by D):
 *   D = q1 - B_p;   u~_m = (D u_h,m) + (B_h u_p,m);   u~'_m = (D u_h'_m) + (B_h u_p'_m);   logderiv = u~'_m / u~_m.
 * Rows: u~_i = (D (q_i yh_i)) + (B_h (q_i yp_i)) for 1 <= i <= m+1, 0.0 at node 0 and beyond m+1.
 * With beta == 0 and q1 = 1: B_h = B_p = 0, D = 1, every yp_i = 0 and G_i = 0 -- the additions of 0.0 change no bit, so logderiv and the
 * rows are those of dfta_continuum (its rows before the normalisation) wherever u_h,i is not -0.0.
 * status (0: fine): DFTA_CONT_NONFINITE -- a yh_i or yp_i, 1 <= i <= m+1, was not finite; DFTA_CONT_STEP as in the continuum block.  With
 * either bit every floating-point output of the trial is NaN.
 * A trial's bits depend on its channel, E, m and the grid -- not on the other trials of the call, their number or order, whether rows
 * were asked for, the chunking of the rows (DFTA_DEBUG KB_CHUNK_WAVES) or the run.  No atomics.
 * DFTA_ERR_INVALID: a NULL input, an l outside 0 .. 4, a q1 that is 0 or not finite, an m outside 3 .. N-2 or below the last non-zero
 * node of the channel's beta, a non-finite E, an index out of range, N < 5.  ntrials == 0: DFTA_OK, nothing is written.  Records the
 * launches' time for dfta_ctx_last_kernel_ms. */
#define DFTA_KB_MAX_STATES 8
#define DFTA_KB_SEARCH_NONFINITE 1
#define DFTA_KB_SEARCH_FULL      2
#define DFTA_KB_SEARCH_CAP       4
#define DFTA_KB_REPORT 10
/* host pointers.  V: nV x N; per channel vidx (NULL: 0), l, q1 and a row of beta (nch x N); per trial chan (NULL: 0), E, m.  Outputs per
 * trial, any of which may be NULL: u = u~_m, du = u~'_m, logderiv, Bh, Bp, D, status; rows ntrials x N. */
int  dfta_kb_sweep(dfta_ctx* ctx, const dfta_grid* g, int nV, const double* V, int nch, const int* vidx, const int* l, const double* beta,
                   const double* q1, int ntrials, const int* chan, const double* E, const int* m, double* u, double* du, double* logderiv,
                   double* Bh, double* Bp, double* D, int* status, double* rows);
/* Bound states of H_KB in a box that ends at node m[k] (u(r_m) = 0), E_lo[k] < E < E_hi[k], per channel: the zeros of u~_m(E).  The
 * nonlocal operator breaks the node theorem, so the search walks the sign of u~_m: a value is negative if u~_m < 0 and finite if the
 * trial has no status bit and u~_m is finite.  A host loop whose only device work is launches of the sweep:
 *   round 0: E_k = E_lo + ((E_hi - E_lo) k) / (nscan - 1), k = 0 .. nscan-1 (nscan a multiple of 64, 64 .. 65536); neighbours k, k+1 that
 *     are both finite and of opposite sign open a bracket (a, b) = (E_k, E_k+1), in ascending E, at most DFTA_KB_MAX_STATES per channel
 *     (more sign changes: status DFTA_KB_SEARCH_FULL);
 *   every further round cuts every open bracket of every channel in ONE launch, a wave per bracket: e_j = a + ((b - a) (j + 1)) / 65,
 *     j = 0 .. 63, moved to a or b if rounding left [a, b]; among p_0 = a, p_1 = e_0, .., p_64 = e_63, p_65 = b the first pair of
 *     neighbours of opposite sign is the new bracket; a value that is not finite takes the sign of a and sets DFTA_KB_SEARCH_NONFINITE
 *     (an outward sweep far below a state overflows at a large box: the caller's choice of m);
 *   a bracket is closed when no double lies between its ends (about 9 rounds); its state is a, the lower end.  32 rounds at most
 *     (DFTA_KB_SEARCH_CAP).
 * Outputs per channel, any of which may be NULL: count; energies nch x 8, ascending, NaN beyond count; rounds (round 0 included);
 * status.  The events of dfta_ctx_last_kernel_ms bracket the whole search, the host's work between the launches included. */
int  dfta_kb_bound_states(dfta_ctx* ctx, const dfta_grid* g, int nV, const double* V, int nch, const int* vidx, const int* l,
                          const double* beta, const double* q1, const int* m, const double* E_lo, const double* E_hi, int nscan, int* count,
                          double* energies, int* rounds, int* status);
/* Ghost-state report of Kleinman-Bylander channels; host code that composes dfta_kb_bound_states and dfta_solve_levels.  Inputs as
 * dfta_pseudo_ionic / dfta_scf_pseudopotentials return them: per channel atom, l, eps (the reference eigenvalue), the SCREENED V_ps
 * (nch x N), beta (nch x N) and kb (nch x 3); l_loc as dfta_pseudo_ionic (the same rule finds the local channel of each atom).  A
 * non-local channel k runs with Vloc = V_ps of its atom's local channel, beta_k and q1 = kb[3k].  report, DFTA_KB_REPORT doubles per
 * channel (the local channel: eps, NaN, then NaN):
 *   0 eps_ref;  1 E_KB;  2 the number of bound states of H_KB in [E_lo, min(0, E_hi)] with the box at node m (E_lo NaN: per channel
 *   min_{i >= 1} vl_i - max(0, -E_KB), below which H_KB has no state: H_loc >= min vl and the projector's norm is |E_KB|);  3 how many of them lie
 *   below eps_ref - tol: each is a ghost;  4, 5 the two lowest eigenvalues e~_0, e~_1 of the local potential at the channel's l from
 *   dfta_solve_levels (levels n = l, l + 1; a level that is not found -- not converged, or not below 0 -- is absent: NaN; l = 4: NaN, the
 *   level search ends at l = 3);  6 the verdict of Gonze, Kaeckell and Scheffler, 1 ghost / 0 clean: E_KB > 0: e~_1 < eps_ref, E_KB < 0:
 *   e~_0 < eps_ref (an absent level is not below; NaN where E_KB is 0 or NaN or l = 4);  7 the direct verdict: 1 if entry 3 is not 0;
 *   8 the search's status bits;  9 its rounds.
 * Both verdicts are returned as they come out; the report never reconciles them.  states (may be NULL): nch x 8, the bound states. */
int  dfta_kb_ghost_report(dfta_ctx* ctx, const dfta_grid* g, int natoms, int nch, const int* atom, const int* l, const double* eps,
                          const double* V_ps, const double* beta, const double* kb, const int* l_loc, int m, double E_lo, double E_hi,
                          int nscan, double tol, double* report, double* states);

/* ---- Aufbau -------------------------------------------------------------------------------------------------
 * AufbauPrinciple::GetSubshells + sort (AufbauPrinciple.h:36-75, DFTAtom.cpp:367); integer-only host code. */
int dfta_get_subshells(int Z, int* n, int* l, int* occ, int cap);
int dfta_split_spin(int Z, int* nA, int* nB, int* an, int* al, int* aocc, int* bn, int* bl, int* bocc, int cap); /* DFTAtom.cpp:611-638 */
/* aufbau: DFTA_AUFBAU_REFERENCE = what the reference runs (Madelung order + the f-block exceptions: Cr 3d4 4s2, Cu 3d9 4s2);
 * DFTA_AUFBAU_TRANSITION_METALS additionally applies AufbauPrinciple::AdjustForTransitionMetals (AufbauPrinciple.h:78-99),
 * which the reference defines but never calls (Cr 3d5 4s1, Cu 3d10 4s1, Pd 4d10, Pt 5d9 6s1 ...). */
#define DFTA_AUFBAU_REFERENCE          0
#define DFTA_AUFBAU_TRANSITION_METALS  1
int dfta_get_subshells_ex(int Z, int aufbau, int* n, int* l, int* occ, int cap);
int dfta_split_spin_ex(int Z, int aufbau, int* nA, int* nB, int* an, int* al, int* aocc, int* bn, int* bl, int* bocc, int cap);

/* ---- electron configurations: cations, holes, excited and fractional occupations (beyond the reference) --------------------
 * A configuration is a list of occupied levels per spin channel: LDA fills the alpha arrays only (nB = 0); LSDA lists the alpha
 * levels, then the beta levels.  n counts as in dfta_get_subshells (the reference's m_N: principal quantum number - 1; the text
 * uses the principal quantum number).  Levels are sorted by (n, l) as DFTAtom.cpp:367 sorts them.  Rules (DFTA_ERR_INVALID otherwise,
 * reason in dfta_config_last_error()): 1 <= Z <= 118; 0 <= l < n, l <= 3; no (n, l) twice in one channel; 0 < occ <= 2(2l+1)
 * (LDA) or <= 2l+1 (one LSDA channel); 0 < N_e = sum occ <= Z (no anions).
 *
 * dfta_config_parse: blank-separated tokens.  `[He]` .. `[Rn]`: that noble gas's Aufbau configuration; `<n><spdf><occ>` (occ may
 * be fractional: `3p5.5`) sets a subshell, replacing what the core holds there, occ 0 removes it; LSDA only: `<n><spdf><a>/<b>`
 * gives the alpha / beta split explicitly, otherwise the split of dfta_split_spin_ex applies (alpha = min(occ, 2l+1)).
 * dfta_ion_config: the Aufbau configuration of Z (option `aufbau`) with `charge` electrons removed from the subshell of highest n,
 * ties to the highest l (Fe+: 3d6 4s1), then the split of dfta_split_spin_ex; charge 0 gives exactly dfta_get_subshells_ex /
 * dfta_split_spin_ex.  Both are host-only. */
int dfta_config_parse(int Z, int lsda, int aufbau, const char* text, int cap, int* nA, int* nB, int* an, int* al, double* aocc,
                      int* bn, int* bl, double* bocc);
int dfta_ion_config(int Z, int charge, int lsda, int aufbau, int cap, int* nA, int* nB, int* an, int* al, double* aocc,
                    int* bn, int* bl, double* bocc);
/* reason of the last DFTA_ERR_INVALID of dfta_config_parse / dfta_ion_config / dfta_scf_create_config on the calling thread */
const char* dfta_config_last_error(void);
/* dfta_scf_create_ex for explicit configurations.  nlev: natoms x 2 level counts (alpha, beta; LDA: beta 0), NULL -> exactly
 * dfta_scf_create_ex (Aufbau configurations of Z); n, l, occ: atom-major, the alpha levels of an atom then its beta levels.  The
 * nuclear charge stays Z (potential, energies, bracket bottoms); the electron count N_e = sum occ sets the flat start density
 * N_e / volume and the multigrid's outer boundary U(Rmax) = N_e.  Neutral integer configurations run bit for bit as
 * dfta_scf_create_ex. */
int  dfta_scf_create_config(dfta_ctx* ctx, const dfta_grid* g, int lsda, int natoms, const int* Z, const int* nlev, const int* n,
                            const int* l, const double* occ, double alpha, int levels_mode, int tree_depth,
                            const dfta_scf_options* options, dfta_scf** out);
/* occupations of (atom, spin) as doubles (dfta_scf_get_levels reports them as int and refuses a channel with a fractional one) */
int  dfta_scf_get_occupations(dfta_scf* s, int atom, int spin, double* occ);

#ifdef __cplusplus
}
#endif
#endif
