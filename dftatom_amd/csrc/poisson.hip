// poisson.hip -- DFT::PoissonSolver (PoissonSolver.h:15-171, PoissonSolver.cpp) on gfx950.
//
// One PERSISTENT 256-thread workgroup (one wave per SIMD of a CU) owns one atom and runs the whole
// FullCycle (Initialize, FMG ramp, up to 100 V-cycles: ~10^4 smoother sweeps over 17 levels) in a single
// launch; the batch dimension (atoms) is the grid.  A launch per sweep would cost ~3*10^4 launches per solve.
//
// Gauss-Seidel is a first-order recurrence in i (PoissonSolver.cpp:48-61):
//     x_i = 0.5 * (S_i + x_{i-1} + x_{i+1}^old - d*(x_{i+1}^old - x_{i-1})*0.5),     |dx_i/dx_{i-1}| = (1+d/2)/2
// Lanes own contiguous chunks of C points; each lane starts W = 96 points early from the OLD values, so the
// error of its start value has decayed by ((1+d/2)/2)^96 < 2^-90 before its first owned point and its chunk
// equals what the sequential sweep computes.  Levels with fewer than 257 nodes (where d grows towards and
// beyond 2) are swept sequentially by one lane -- exactly the reference's loop.
//
// Layout.  A level with n = C*T + 1 nodes is stored lane-interleaved: node i = t*C + k lives at k*T + t
// (node n-1 at C*T), so that at step k the T lanes touch consecutive addresses -- the warm-up, restriction
// and prolongation accesses are coalesced too.  Phi is double-buffered (the sweep reads old right
// neighbours while other lanes overwrite them).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <memory>
#include <type_traits>
#include <vector>

#include "internal.h"
#include "poisson_plan.h"
#include "xc.h"

using namespace dfta_mg;     // Lvl, MgDesc and the layout constants: shared with the planner (poisson_plan.h)

namespace {

#ifndef DFTA_KWARM
#define DFTA_KWARM 96
#endif
// kWarm (the chunked sweeps' warm-up) and kWarm3 (the fused visit's) are set per inclusion of poisson_kernels.inc:
//   mg_exact: 96 / 112 nodes -- start-value error decays by <= 0.52^96 < 2^-90: chunked sweep == sequential sweep bit for bit
//   mg_tol  : 32 / 32 nodes  -- the opt-in tolerance mode (DFTA_POISSON_TOLERANCE): start values good to 1e-9 of a sweep's change
constexpr int kPF = 8;           // register prefetch depth of the chunked sweep

// storage index of node i RELATIVE to the start of its level
__host__ __device__ __forceinline__ int addr(const Lvl& L, int i)
{
    if (i == L.n - 1) return L.n - 1;
    return ((i & ((1 << L.logC) - 1)) << L.logT) + (i >> L.logC);
}
// inverse: storage index -> node
__device__ __forceinline__ int node_of(const Lvl& L, int idx)
{
    if (idx == L.n - 1) return idx;
    return ((idx & ((1 << L.logT) - 1)) << L.logC) + (idx >> L.logT);
}

// Level storage of one atom.  The chunked levels live in global memory (L2-resident: 6.3 MB per atom at 17
// levels); the sequential levels (n < 257, 261 nodes in total) live in LDS for the whole solve -- they are visited
// 6 times per V-cycle by a single lane and would otherwise pay a global-memory round trip per node.
constexpr unsigned long long kFastSentinel = 0x7FF8DEAD7FF8DEADull;

}  // namespace

namespace {
namespace mg_exact {
#define DFTA_MG_KWARM DFTA_KWARM
#define DFTA_MG_KWARM3 112
#include "poisson_kernels.inc"
#undef DFTA_MG_KWARM
#undef DFTA_MG_KWARM3
}  // namespace mg_exact
// The resident group's second configuration (exact mode): 16 members of 256 lanes + the coarse workgroup per atom, level 0 and the other
// shared levels taking turns in the members' LDS -- up to 15 atoms per launch (poisson_kernels.inc: DFTA_MG_RES16)
namespace mg_exact16 {
#define DFTA_MG_KWARM DFTA_KWARM
#define DFTA_MG_KWARM3 112
#define DFTA_MG_RES16 1
#include "poisson_kernels.inc"
#undef DFTA_MG_RES16
#undef DFTA_MG_KWARM
#undef DFTA_MG_KWARM3
}  // namespace mg_exact16
// Tolerance mode (opt-in, DFTA_POISSON_TOLERANCE): the same kernels with 32-node warm-ups.  A lane's start value then carries
// 0.52^32 ~ 1e-9 of the change its start node undergoes in that sweep -- a perturbation of the ITERATION, not of its fixed point:
// the cycle still converges to the solution of the same discrete equations, to the same round-off floor (tests: U within
// 2e-9 Z of the exact solve, SCF energies within 1e-9 of the reference's), but a sweep is no longer the sequential sweep bit for bit.
namespace mg_tol {
#define DFTA_MG_KWARM 32
#define DFTA_MG_KWARM3 32
#ifndef DFTA_MG_NO_SCAN_COARSE
#define DFTA_MG_SCAN_COARSE 1      // the coarse section's sweeps as affine scans (poisson_kernels.inc: cs_sweep_scan)
#endif
#include "poisson_kernels.inc"
#undef DFTA_MG_KWARM
#undef DFTA_MG_KWARM3
}  // namespace mg_tol
namespace mg_tol16 {               // tolerance mode, the resident group's second configuration (8 .. 15 atoms)
#define DFTA_MG_KWARM 32
#define DFTA_MG_KWARM3 32
#define DFTA_MG_RES16 1
#include "poisson_kernels.inc"
#undef DFTA_MG_RES16
#undef DFTA_MG_KWARM
#undef DFTA_MG_KWARM3
}  // namespace mg_tol16
}  // namespace

static_assert(mg_exact::kWarm3 == kWarm3Exact && mg_exact16::kWarm3 == kWarm3Exact && mg_tol::kWarm3 == kWarm3Tol && mg_tol16::kWarm3 == kWarm3Tol &&
              mg_exact16::kResNT == kRes16NT && mg_exact16::kResG == kRes16G && mg_tol16::kResNT == kRes16NT && mg_tol16::kResG == kRes16G,
              "poisson_plan.h sizes the spill buffer and the launches from these");

// The kernels of one solver, chosen once at creation from (tolerance mode, second resident configuration).  k_poisson_solve and k_unit
// exist once per mode: a res16 solver's are those of mg_exact / mg_tol.
struct KernelSet {
    decltype(&mg_exact::k_poisson_solve) solve;
    decltype(&mg_exact::k_poisson_solve_res) solve_res;
    decltype(&mg_exact::k_unit) unit;
#ifdef DFTA_POISSON_RPROF
    const void* rprof;       // its g_rprof, for hipMemcpyFromSymbol / hipMemcpyToSymbol
#define DFTA_RPROF_OF(ns) , &ns::g_rprof
#else
#define DFTA_RPROF_OF(ns)
#endif
};
static const KernelSet kKernels[2][2] = {      // [tol][res16]
    {{mg_exact::k_poisson_solve, mg_exact::k_poisson_solve_res, mg_exact::k_unit DFTA_RPROF_OF(mg_exact)},
     {mg_exact::k_poisson_solve, mg_exact16::k_poisson_solve_res, mg_exact::k_unit DFTA_RPROF_OF(mg_exact16)}},
    {{mg_tol::k_poisson_solve, mg_tol::k_poisson_solve_res, mg_tol::k_unit DFTA_RPROF_OF(mg_tol)},
     {mg_tol::k_poisson_solve, mg_tol16::k_poisson_solve_res, mg_tol::k_unit DFTA_RPROF_OF(mg_tol16)}}};
#undef DFTA_RPROF_OF

struct PoissonDestroy { void operator()(dfta_poisson* p) const { dfta_poisson_destroy(p); } };

struct dfta_poisson : PoissonPlan {      // the plan it was built from (D, resident, res16, plain_launch, fault, tol, adaptive) + what it owns
    dfta_ctx* ctx = nullptr;
    const dfta_grid* g = nullptr;
    int batch = 0;
    const KernelSet* K = nullptr;
    DevBuf<MgDesc> d_desc;          // device copy of D (read with scalar loads)
    DevBuf<double> d_phi0, d_phi1, d_src;
    DevBuf<int> d_cur;              // unit hooks: current buffer per level (atom 0)
    std::vector<int> h_cur;
    DevBuf<unsigned long long> d_total_vcycles;
    DevBuf<unsigned> d_group_ctr;   // per atom: arrival counter of its group of workgroups (zeroed before every launch)
    DevBuf<double> d_group_part;    // per atom: 6 G + 2 doubles (partial sums of the members, published state)
    // Groups of workgroups wait for each other, so every workgroup of a launch has to be resident: the launch is a
    // COOPERATIVE one (the runtime refuses it when the grid cannot be co-resident), the barriers' spins are bounded, and
    // dfta_poisson_finish() inspects the abort flag after every solve.  If a launch is refused or a group gives up, the
    // solve is repeated by `fallback` -- the same solver with one workgroup per atom (no cross-workgroup waits, results
    // bit-identical) -- and this solver stays degraded to it.
    std::unique_ptr<dfta_poisson, PoissonDestroy> fallback;
    bool degraded = false;
    int aborts = 0;                 // solves that had to be repeated
    DevBuf<double> d_res_slots;     // resident: per atom res_slot_doubles() exchange slots (sentinel-filled before every launch)
    DevBuf<double> d_res_spill;     // res16: per member the two LDS images of level 0
    DevBuf<unsigned long long> d_pred_ctr;   // fused visits with predicted start values: [0] checked, [1] repeated (D.pred_ctr)
    bool grouped() const { return D.G > 1 || resident; }
};

constexpr int kModeFromKnob = -1;    // poisson_create_impl: the mode $DFTA_DEBUG POISSON_MODE names (dfta_poisson_create)
static int poisson_create_impl(dfta_ctx* ctx, const dfta_grid* g, int batch, int force_logG, int mode, dfta_poisson** out);

static int degrade(dfta_poisson* p)
{
    if (!p->fallback) {
        dfta_poisson* fb = nullptr;
        int rc = poisson_create_impl(p->ctx, p->g, p->batch, 0, dfta_poisson_mode(p), &fb);
        if (rc) return rc;
        p->fallback.reset(fb);
    }
    p->degraded = true;
    return DFTA_OK;
}

// Starts `kernel` on `grid` workgroups of kThreads: ordinarily, or -- groups of workgroups that wait for each other -- cooperatively
// (the runtime refuses the launch when the grid cannot be co-resident).
static hipError_t launch(dfta_ctx* ctx, const void* kernel, int grid, void** args, bool cooperative)
{
    if (cooperative) return hipLaunchCooperativeKernel(kernel, dim3(grid), dim3(kThreads), args, 0, ctx->stream);
    const hipError_t e = hipLaunchKernel(kernel, dim3(grid), dim3(kThreads), args, 0, ctx->stream);
    return e != hipSuccess ? e : hipGetLastError();
}

// dNe (device, per atom): electron count, the outer boundary U(Rmax) of the solve (DFTAtom's Z for a neutral atom)
// dSkip (device, per atom, may be null): atoms with a non-zero entry are left untouched (frozen atoms of an SCF batch)
int dfta_poisson_solve_launch(dfta_poisson* p, const double* dNe, const double* dDensity, double* dU, int* dVcycles, double* dErr,
                              const int* dSkip)
{
    dfta_ctx* ctx = p->ctx;
    if (p->degraded) return dfta_poisson_solve_launch(p->fallback.get(), dNe, dDensity, dU, dVcycles, dErr, dSkip);
    DFTA_HIP(ctx, hipMemsetAsync(p->d_group_ctr, 0, sizeof(unsigned) * p->batch, ctx->stream));
    DFTA_HIP(ctx, hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(p->d_group_part.p), 0x7FF8DEAD, (size_t)p->batch * group_part_doubles(p->D.G) * 2, ctx->stream));   // group_sum_fast's sentinel
    if (p->resident)
        DFTA_HIP(ctx, hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(p->d_res_slots.p), 0x7FF8DEAD, (size_t)p->batch * res_slot_doubles() * 2, ctx->stream));
    const int wg = p->resident ? p->res_wg() : p->D.G;           // workgroups per atom
    const void* kernel = p->resident ? reinterpret_cast<const void*>(p->K->solve_res) : reinterpret_cast<const void*>(p->K->solve);
    const MgDesc* desc = p->d_desc;
    const double *r = p->g->d_rsrc, *psrc = p->g->d_psrc;
    int fault = wg == 1 ? 0 : p->fault, src_all = p->g->uniform;
    // the two kernels differ in their 14th argument (partial sums / exchange slots); the 18th is the resident kernel's alone
    double** group_mem = p->resident ? &p->d_res_slots.p : &p->d_group_part.p;
    void* args[] = {&desc, &p->d_phi0.p, &p->d_phi1.p, &p->d_src.p, &dNe, &dDensity, &r, &psrc, &dU, &dVcycles, &dErr, &p->d_total_vcycles.p,
                    &p->d_group_ctr.p, group_mem, &dSkip, &fault, &src_all, &p->d_res_spill.p};
    if (wg == 1 || p->plain_launch) {        // plain_launch: under a profiler (see plan_poisson): same kernel, ordinary launch
        DFTA_HIP(ctx, launch(ctx, kernel, p->batch * wg, args, false));
        return DFTA_OK;
    }
    if (launch(ctx, kernel, p->batch * wg, args, true) == hipSuccess) return DFTA_OK;
    // the grid cannot be co-resident right now (or cooperative launches are unavailable): one workgroup per atom instead
    (void)hipGetLastError();
    int rc = degrade(p);
    if (rc) return rc;
    ++p->aborts;
    return dfta_poisson_solve_launch(p->fallback.get(), dNe, dDensity, dU, dVcycles, dErr, dSkip);
}

// after a solve has completed: did a group of workgroups give up on one of its barriers (a member was never scheduled)?
static int check_groups(dfta_poisson* p)
{
    dfta_ctx* ctx = p->ctx;
    if (!p->grouped() || p->degraded) return DFTA_OK;
    std::vector<unsigned> h(p->batch);
    DFTA_HIP(ctx, hipMemcpyAsync(h.data(), p->d_group_ctr, sizeof(unsigned) * p->batch, hipMemcpyDeviceToHost, ctx->stream));
    DFTA_HIP(ctx, hipStreamSynchronize(ctx->stream));
    for (unsigned v : h)
        if (v & 0x80000000u) {
            const int G = p->resident ? p->res_wg() : p->D.G;
            snprintf(ctx->err, sizeof(ctx->err), "poisson: a group of %d workgroups lost a member at a barrier (the %d workgroups of "
                     "the launch were not all resident)", G, p->batch * G);
            return DFTA_ERR_HIP;
        }
    return DFTA_OK;
}

// Completes the solve launched last (synchronises the stream).  If a group of workgroups gave up, the solve is repeated
// with one workgroup per atom, in this process and on the same stream, and every later solve of `p` takes that path.
int dfta_poisson_finish(dfta_poisson* p, const double* dNe, const double* dDensity, double* dU, int* dVcycles, double* dErr,
                        const int* dSkip)
{
    dfta_ctx* ctx = p->ctx;
    if (!p->grouped() || p->degraded) { DFTA_HIP(ctx, hipStreamSynchronize(ctx->stream)); return DFTA_OK; }
    if (check_groups(p) == DFTA_OK) return DFTA_OK;
    ++p->aborts;
    DFTA_HIP(ctx, hipMemsetAsync(p->d_total_vcycles, 0, sizeof(unsigned long long), ctx->stream));   // the aborted solve's count
    int rc = degrade(p);
    if (rc) return rc;
    rc = dfta_poisson_solve_launch(p->fallback.get(), dNe, dDensity, dU, dVcycles, dErr, dSkip);
    if (rc) return rc;
    DFTA_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return DFTA_OK;
}

int dfta_poisson_take_vcycles(dfta_poisson* p, unsigned long long* out)   // reads and clears the V-cycle counter
{
    dfta_ctx* ctx = p->ctx;
    unsigned long long a = 0, b = 0;
    DFTA_HIP(ctx, hipMemcpyAsync(&a, p->d_total_vcycles, sizeof(unsigned long long), hipMemcpyDeviceToHost, ctx->stream));
    if (p->fallback) DFTA_HIP(ctx, hipMemcpyAsync(&b, p->fallback->d_total_vcycles, sizeof(unsigned long long), hipMemcpyDeviceToHost, ctx->stream));
    DFTA_HIP(ctx, hipStreamSynchronize(ctx->stream));
    DFTA_HIP(ctx, hipMemsetAsync(p->d_total_vcycles, 0, sizeof(unsigned long long), ctx->stream));
    if (p->fallback) DFTA_HIP(ctx, hipMemsetAsync(p->fallback->d_total_vcycles, 0, sizeof(unsigned long long), ctx->stream));
    *out = a + b;
    return DFTA_OK;
}

int dfta_poisson_group_state(const dfta_poisson* p, int* G, int* degraded, int* aborts)
{
    if (!p) return DFTA_ERR_INVALID;
    if (G) *G = p->resident ? p->res_wg() : p->D.G;
    if (degraded) *degraded = p->degraded ? 1 : 0;
    if (aborts) *aborts = p->aborts;
    return DFTA_OK;
}

extern "C" {

int dfta_poisson_create_ex(dfta_ctx* ctx, const dfta_grid* g, int batch, int mode, dfta_poisson** out)
{
    if (!ctx || !g || !out) return DFTA_ERR_INVALID;
    DFTA_ENTER(ctx);
    DFTA_REQUIRE(ctx, mode == DFTA_POISSON_EXACT || mode == DFTA_POISSON_TOLERANCE || mode == DFTA_POISSON_ADAPTIVE, "poisson mode");
    return poisson_create_impl(ctx, g, batch, -1, mode, out);
}

int dfta_poisson_create(dfta_ctx* ctx, const dfta_grid* g, int batch, dfta_poisson** out)
{
    // DFTA_DEBUG="POISSON_MODE=tolerance" (or adaptive): measurements and tests of the opt-in modes through callers that do not pass a mode
    if (!ctx || !g || !out) return DFTA_ERR_INVALID;
    DFTA_ENTER(ctx);
    return poisson_create_impl(ctx, g, batch, -1, kModeFromKnob, out);
}

int dfta_poisson_mode(const dfta_poisson* p) { return p ? (p->adaptive ? DFTA_POISSON_ADAPTIVE : (p->tol ? DFTA_POISSON_TOLERANCE : DFTA_POISSON_EXACT)) : -1; }

}  // extern "C"

// every $DFTA_DEBUG knob (and the profiler's environment variable) the multigrid's host code looks at, once per creation
static PoissonKnobs read_knobs(int batch)
{
    auto set = [](const char* value) { return value != nullptr; };
    auto on_off = [](const char* value) { return value ? (atoi(value) != 0 ? 1 : 0) : -1; };
    PoissonKnobs K;
    if (const char* e = dfta_knob("POISSON_GROUP")) {      // measurements: force log2 of the group size
        const int v = atoi(e);
        K.group_set = true;
        if (v >= 0 && v <= 6 && (batch << v) <= 256) K.group = v;
    }
    if (const char* e = dfta_knob("FAULT_POISSON_MEMBER")) K.fault = atoi(e) != 0;
    K.res = on_off(dfta_knob("POISSON_RES"));
    K.res16 = on_off(dfta_knob("POISSON_RES16"));
    K.nostage = set(dfta_knob("POISSON_NOSTAGE"));
    K.nostage_wave = set(dfta_knob("POISSON_NOSTAGE_WAVE"));
    K.nostage_shared = set(dfta_knob("POISSON_NOSTAGE_SHARED"));
    K.nocoarse = set(dfta_knob("POISSON_NOCOARSE"));
    K.noxw = set(dfta_knob("POISSON_NOXW"));
    K.norc = set(dfta_knob("POISSON_NORC"));
    K.nofuse3 = set(dfta_knob("POISSON_NOFUSE3"));
    K.nofuse3_wave = set(dfta_knob("POISSON_NOFUSE3_WAVE"));
    K.nohalf129 = set(dfta_knob("POISSON_NOHALF129"));
    K.nopredict = set(dfta_knob("POISSON_NOPREDICT"));
    K.predict_fuzz = set(dfta_knob("POISSON_PREDICT_FUZZ"));
    K.nofold = set(dfta_knob("POISSON_NOFOLD"));
    K.nofold_lds = set(dfta_knob("POISSON_NOFOLD_LDS"));
    K.nofuse_coop = set(dfta_knob("POISSON_NOFUSE_COOP"));
    if (const char* e = dfta_knob("POISSON_FUSE_MIN_LOGC")) K.fuse_min_logc = std::max(kFuseMinLogC, atoi(e));   // measurements (99: never; staged levels -- <= 32 nodes per lane -- have their own fused pass)
    if (const char* e = dfta_knob("POISSON_DBG")) K.dbg = atoi(e);
    K.plain_launch = set(dfta_knob("POISSON_PLAIN_LAUNCH")) || getenv("ROCP_TOOL_LIBRARIES") != nullptr;
    const char* m = dfta_knob("POISSON_MODE");
    K.mode = (m && m[0] == 't') ? DFTA_POISSON_TOLERANCE : ((m && m[0] == 'a') ? DFTA_POISSON_ADAPTIVE : DFTA_POISSON_EXACT);
    return K;
}

#define TRY_HIP(call) do { const hipError_t e_ = (call); if (e_ != hipSuccess) return e_; } while (0)
// the solver's device memory, sized by the plan; level storage, unit-hook state and the V-cycle counter start as zeros
static hipError_t allocate(dfta_poisson* p)
{
    const PoissonPlan& P = *p;
    hipStream_t st = p->ctx->stream;
    TRY_HIP(p->d_phi0.alloc(P.n_level_store));
    TRY_HIP(p->d_phi1.alloc(P.n_level_store));
    TRY_HIP(p->d_src.alloc(P.n_level_store));
    TRY_HIP(p->d_cur.alloc(P.n_cur));
    TRY_HIP(p->d_pred_ctr.alloc(2));
    TRY_HIP(hipMemsetAsync(p->d_pred_ctr, 0, 2 * sizeof(unsigned long long), st));
    p->D.pred_ctr = p->d_pred_ctr.p;
    TRY_HIP(p->d_desc.alloc(1));
    TRY_HIP(hipMemcpyAsync(p->d_desc, &p->D, sizeof(MgDesc), hipMemcpyHostToDevice, st));
    TRY_HIP(p->d_total_vcycles.alloc(1));
    TRY_HIP(p->d_group_ctr.alloc(P.n_group_ctr));
    TRY_HIP(p->d_group_part.alloc(P.n_group_part));
    TRY_HIP(p->d_res_slots.alloc(P.n_res_slots));
    TRY_HIP(p->d_res_spill.alloc(P.n_res_spill));
    TRY_HIP(hipMemsetAsync(p->d_phi0, 0, P.n_level_store * sizeof(double), st));
    TRY_HIP(hipMemsetAsync(p->d_phi1, 0, P.n_level_store * sizeof(double), st));
    TRY_HIP(hipMemsetAsync(p->d_src, 0, P.n_level_store * sizeof(double), st));
    TRY_HIP(hipMemsetAsync(p->d_cur, 0, P.n_cur * sizeof(int), st));
    TRY_HIP(hipMemsetAsync(p->d_total_vcycles, 0, sizeof(unsigned long long), st));
    // every atom's barrier counter: a unit launch clears atom 0's alone, and check_groups reads the abort flag of all of them
    TRY_HIP(hipMemsetAsync(p->d_group_ctr, 0, P.n_group_ctr * sizeof(unsigned), st));
    return hipStreamSynchronize(st);
}
#undef TRY_HIP

// workgroups of kThreads a compute unit holds at once, for the planner; -1: the query failed
static int blocks_per_cu(const void* kernel)
{
    int per_cu = 0;
    return hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, kThreads, 0) == hipSuccess ? per_cu : -1;
}

// force_logG >= 0: that many doublings of the workgroups per atom (0: one workgroup per atom); -1: chosen from the batch size
static int poisson_create_impl(dfta_ctx* ctx, const dfta_grid* g, int batch, int force_logG, int mode, dfta_poisson** out)
{
    DFTA_REQUIRE(ctx, batch >= 1 && g->levels <= kMaxLevels, "poisson batch/levels");
    PlanInputs in;
    in.knobs = read_knobs(batch);
    if (mode == kModeFromKnob) mode = in.knobs.mode;
    in.N = g->N; in.levels = g->levels; in.delta = g->delta; in.uniform = g->uniform;
    in.batch = batch; in.force_logG = force_logG; in.mode = mode; in.num_cu = ctx->num_cu;
    const bool tol = mode != DFTA_POISSON_EXACT;
    in.occupancy = [tol](PlanKernel k) {
        const KernelSet& K = kKernels[tol][k == kKernelSolveRes16];
        return blocks_per_cu(k == kKernelSolve ? reinterpret_cast<const void*>(K.solve) : reinterpret_cast<const void*>(K.solve_res));
    };
    std::unique_ptr<dfta_poisson, PoissonDestroy> p(new dfta_poisson());
    if (plan_poisson(in, p.get())) { snprintf(ctx->err, sizeof(ctx->err), "%s", p->error); return DFTA_ERR_INVALID; }
    p->ctx = ctx; p->g = g; p->batch = batch;
    p->K = &kKernels[p->tol][p->res16];
    const hipError_t e = allocate(p.get());
    if (e != hipSuccess) { snprintf(ctx->err, sizeof(ctx->err), "poisson alloc: %s", hipGetErrorString(e)); return DFTA_ERR_HIP; }
    p->h_cur.assign(kMaxLevels, 0);
    *out = p.release();
    return DFTA_OK;
}

extern "C" {

void dfta_poisson_destroy(dfta_poisson* p)
{
    if (!p) return;
    p->fallback.reset();
#ifdef DFTA_POISSON_PROF
    {
        unsigned long long h[8 * 24];
        if (hipMemcpyFromSymbol(h, HIP_SYMBOL(mg_exact::g_prof), sizeof(h)) == hipSuccess) {
            const char* names[8] = {"restrict", "prolong ", "iterate ", "grp_sum ", "gs_lds  ", "copy_in ", "copy_out", "sweeps1 "};
            unsigned long long tot = 0;
            for (int c = 0; c < 8; ++c) {
                fprintf(stderr, "[poisson prof] %s:", names[c]);
                for (int l = 0; l < 22; ++l) { fprintf(stderr, " %llu", h[c * 24 + l]); tot += h[c * 24 + l]; }
                fprintf(stderr, "\n");
            }
            fprintf(stderr, "[poisson prof] total ticks %llu\n", tot);
            unsigned long long hm[64 * 4];
            if (hipMemcpyFromSymbol(hm, HIP_SYMBOL(mg_exact::g_prof_member), sizeof(hm)) == hipSuccess) {
                for (int m = 0; m < 16; ++m) fprintf(stderr, "[poisson prof] member %2d: exchange %llu  sweeps %llu  copy-in %llu\n", m, hm[m * 4], hm[m * 4 + 1], hm[m * 4 + 2]);
                unsigned long long zz[64 * 4] = {0};
                (void)hipMemcpyToSymbol(HIP_SYMBOL(mg_exact::g_prof_member), zz, sizeof(zz));
            }
            unsigned long long z[8 * 24] = {0};
            (void)hipMemcpyToSymbol(HIP_SYMBOL(mg_exact::g_prof), z, sizeof(z));
        }
    }
#endif
#ifdef DFTA_POISSON_RPROF
    {
        unsigned long long hr[2 * 8 * 8];
        if (p->resident && hipMemcpyFromSymbol(hr, p->K->rprof, sizeof(hr)) == hipSuccess) {
            const char* mn[8] = {"pass    ", "publish ", "exchange", "commit  ", "restrict", "prolong ", "handover", "redo    "};
            const char* cn[8] = {"passive ", "cs sweep", "iterate ", "coarsesc", "restrict", "prolong ", "handover", "cs r/p/xw/enter/leave"};
            for (int role = 0; role < 2; ++role)
                for (int c = 0; c < 8; ++c) {
                    unsigned long long t = 0;
                    fprintf(stderr, "[res prof] %s %s:", role ? "coarse wg" : "member 0 ", role ? cn[c] : mn[c]);
                    for (int l = 0; l < 8; ++l) { fprintf(stderr, " %llu", hr[(role * 8 + c) * 8 + l]); t += hr[(role * 8 + c) * 8 + l]; }
                    fprintf(stderr, "  = %llu\n", t);
                }
            unsigned long long zz[2 * 8 * 8] = {0};
            (void)hipMemcpyToSymbol(p->K->rprof, zz, sizeof(zz));
        }
    }
#endif
    delete p;
}

int dfta_poisson_solve(dfta_poisson* p, const int* Z, const double* density, double* U, int* vcycles_out, double* err_out)
{
    if (!p) return DFTA_ERR_INVALID;
    dfta_ctx* ctx = p->ctx;
    DFTA_ENTER(ctx);
    DFTA_REQUIRE(ctx, Z && density && U, "null input");
    const int N = p->g->N, B = p->batch;
    hipStream_t st = ctx->stream;
    DevBuf<int> dVc;
    DevBuf<double> dZ, dRho, dU, dErr;
    std::vector<double> ne(Z, Z + B);                    // the outer boundary of a neutral atom: (double)Z
    DFTA_HIP(ctx, dZ.alloc(B)); DFTA_HIP(ctx, dVc.alloc(B)); DFTA_HIP(ctx, dErr.alloc(B));
    DFTA_HIP(ctx, dRho.alloc((size_t)B * N)); DFTA_HIP(ctx, dU.alloc((size_t)B * N));
    DFTA_HIP(ctx, hipMemcpyAsync(dZ.p, ne.data(), sizeof(double) * B, hipMemcpyHostToDevice, st));
    DFTA_HIP(ctx, hipMemcpyAsync(dRho.p, density, sizeof(double) * (size_t)B * N, hipMemcpyHostToDevice, st));
    DFTA_HIP(ctx, dfta_timer_start(ctx));
    int rc = dfta_poisson_solve_launch(p, dZ.p, dRho.p, dU.p, dVc.p, dErr.p, nullptr);
    if (rc) return rc;
    DFTA_HIP(ctx, dfta_timer_stop(ctx));
    rc = dfta_poisson_finish(p, dZ.p, dRho.p, dU.p, dVc.p, dErr.p, nullptr);
    if (rc) return rc;
    DFTA_HIP(ctx, hipMemcpyAsync(U, dU.p, sizeof(double) * (size_t)B * N, hipMemcpyDeviceToHost, st));
    if (vcycles_out) DFTA_HIP(ctx, hipMemcpyAsync(vcycles_out, dVc.p, sizeof(int) * B, hipMemcpyDeviceToHost, st));
    if (err_out) DFTA_HIP(ctx, hipMemcpyAsync(err_out, dErr.p, sizeof(double) * B, hipMemcpyDeviceToHost, st));
    DFTA_HIP(ctx, hipStreamSynchronize(st));
    return DFTA_OK;
}

}  // extern "C"

static __global__ void k_int_to_double(const int* __restrict__ in, int n, double* __restrict__ out)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = in[i];
}

extern "C" {

int dfta_poisson_solve_dev(dfta_poisson* p, const int* dZ, const double* dDensity, double* dU)
{
    if (!p) return DFTA_ERR_INVALID;
    DFTA_REQUIRE(p->ctx, dZ && dDensity && dU, "null input");
    DFTA_ENTER(p->ctx);
    DevBuf<double> dNe;                                  // (double)Z: the outer boundary of a neutral atom
    DFTA_HIP(p->ctx, dNe.alloc(p->batch));
    hipLaunchKernelGGL(k_int_to_double, dim3((p->batch + 255) / 256), dim3(256), 0, p->ctx->stream, dZ, p->batch, dNe.p);
    DFTA_CHECK_LAUNCH(p->ctx);
    // synchronises: the group barriers' abort flag is inspected after every solve (and the solve repeated with one
    // workgroup per atom if it was raised), so a DFTA_OK always means a completed solve
    int rc = dfta_poisson_solve_launch(p, dNe.p, dDensity, dU, nullptr, nullptr, nullptr);
    if (rc) return rc;
    return dfta_poisson_finish(p, dNe.p, dDensity, dU, nullptr, nullptr, nullptr);
}

int dfta_poisson_group_info(const dfta_poisson* p, int* G, int* degraded, int* aborts)
{
    return dfta_poisson_group_state(p, G, degraded, aborts);
}

// fused visits of the one-wave levels that ran with predicted start values (checked) and those whose hand-over check failed and that
// were run again with the full warm-up (repeated), since the solver was created; the one-workgroup fallback's visits included
int dfta_poisson_predict_counts(dfta_poisson* p, unsigned long long* checked, unsigned long long* repeated)
{
    if (!p) return DFTA_ERR_INVALID;
    dfta_ctx* ctx = p->ctx;
    DFTA_ENTER(ctx);
    unsigned long long a[2] = {0, 0}, b[2] = {0, 0};
    DFTA_HIP(ctx, hipMemcpyAsync(a, p->d_pred_ctr, sizeof(a), hipMemcpyDeviceToHost, ctx->stream));
    if (p->fallback) DFTA_HIP(ctx, hipMemcpyAsync(b, p->fallback->d_pred_ctr, sizeof(b), hipMemcpyDeviceToHost, ctx->stream));
    DFTA_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (checked) *checked = a[0] + b[0];
    if (repeated) *repeated = a[1] + b[1];
    return DFTA_OK;
}

int dfta_poisson_level_size(const dfta_poisson* p, int lvl)
{
    if (!p || lvl < 0 || lvl >= p->D.levels) return -1;
    return p->D.lv[lvl].n;
}

// one level of atom 0 between the host (natural node order) and the device (lane-interleaved): Phi's current copy and / or the source
static int copy_level(dfta_poisson* p, int lvl, double* Phi, double* Src, bool to_device)
{
    if (p->degraded) return copy_level(p->fallback.get(), lvl, Phi, Src, to_device);     // the solves run on the fallback's storage
    dfta_ctx* ctx = p->ctx;
    DFTA_ENTER(ctx);
    DFTA_REQUIRE(ctx, lvl >= 0 && lvl < p->D.levels, "level");
    const Lvl& L = p->D.lv[lvl];
    std::vector<double> tmp(L.n);
    double* const host[2] = {Phi, Src};
    double* const dev[2] = {(p->h_cur[lvl] ? p->d_phi1 : p->d_phi0) + L.off, p->d_src + L.off};
    for (int a = 0; a < 2; ++a) {
        if (!host[a]) continue;
        if (to_device) for (int i = 0; i < L.n; ++i) tmp[addr(L, i)] = host[a][i];
        DFTA_HIP(ctx, hipMemcpyAsync(to_device ? dev[a] : tmp.data(), to_device ? tmp.data() : dev[a], sizeof(double) * L.n,
                                      to_device ? hipMemcpyHostToDevice : hipMemcpyDeviceToHost, ctx->stream));
        DFTA_HIP(ctx, hipStreamSynchronize(ctx->stream));
        if (!to_device) for (int i = 0; i < L.n; ++i) host[a][i] = tmp[addr(L, i)];
    }
    return DFTA_OK;
}
int dfta_poisson_set_level(dfta_poisson* p, int lvl, const double* Phi, const double* Src)
{
    return p ? copy_level(p, lvl, const_cast<double*>(Phi), const_cast<double*>(Src), true) : DFTA_ERR_INVALID;
}
int dfta_poisson_get_level(dfta_poisson* p, int lvl, double* Phi, double* Src) { return p ? copy_level(p, lvl, Phi, Src, false) : DFTA_ERR_INVALID; }

// One unit launch on atom 0 with the solver's own group of G workgroups (cooperative, like the solve; a refused launch is an error):
// uploads h_cur, clears the group's counter and sentinel-fills its partial sums, runs `op`, brings h_cur and the first `nout` doubles
// of dOut back.  The caller ends with check_groups: a member lost at a barrier of a unit launch is an error, not a silent wrong answer.
static int run_unit(dfta_poisson* p, int op, int lvl, int sweeps, double* dOut, double* out_host, int nout)
{
    dfta_ctx* ctx = p->ctx;
    hipStream_t st = ctx->stream;
    DFTA_HIP(ctx, hipMemcpyAsync(p->d_cur, p->h_cur.data(), sizeof(int) * kMaxLevels, hipMemcpyHostToDevice, st));
    DFTA_HIP(ctx, hipMemsetAsync(p->d_group_ctr, 0, sizeof(unsigned), st));
    DFTA_HIP(ctx, hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(p->d_group_part.p), 0x7FF8DEAD, (size_t)group_part_doubles(p->D.G) * 2, st));
    const MgDesc* desc = p->d_desc;
    void* args[] = {&desc, &p->d_phi0.p, &p->d_phi1.p, &p->d_src.p, &p->d_cur.p, &op, &lvl, &sweeps, &dOut, &p->d_group_ctr.p, &p->d_group_part.p};
    DFTA_HIP(ctx, launch(ctx, reinterpret_cast<const void*>(p->K->unit), p->D.G, args, p->D.G > 1 && !p->plain_launch));
    DFTA_HIP(ctx, hipMemcpyAsync(p->h_cur.data(), p->d_cur, sizeof(int) * kMaxLevels, hipMemcpyDeviceToHost, st));
    if (out_host && nout > 0) DFTA_HIP(ctx, hipMemcpyAsync(out_host, dOut, sizeof(double) * nout, hipMemcpyDeviceToHost, st));
    DFTA_HIP(ctx, hipStreamSynchronize(st));
    return DFTA_OK;
}

static int unit_op(dfta_poisson* p, int op, int lvl, int sweeps, double* out_host, int nout)
{
    if (p->degraded) return unit_op(p->fallback.get(), op, lvl, sweeps, out_host, nout);
    dfta_ctx* ctx = p->ctx;
    DFTA_ENTER(ctx);
    DevBuf<double> dOut;
    DFTA_HIP(ctx, dOut.alloc(std::max(nout, 1)));
    if (int rc = run_unit(p, op, lvl, sweeps, dOut, out_host, nout)) return rc;
    return check_groups(p);
}

int dfta_poisson_gauss_seidel(dfta_poisson* p, int lvl, int sweeps, double* err_out)
{
    if (!p) return DFTA_ERR_INVALID;
    DFTA_REQUIRE(p->ctx, lvl >= 0 && lvl < p->D.levels && sweeps >= 1 && sweeps <= 1024, "level/sweeps");
    return unit_op(p, 0, lvl, sweeps, err_out, err_out ? sweeps : 0);
}
int dfta_poisson_iterate_gs(dfta_poisson* p, int lvl, double errorMin, int iterno, double* err_out, int* sweeps_out)
{
    if (!p) return DFTA_ERR_INVALID;
    if (p->degraded) return dfta_poisson_iterate_gs(p->fallback.get(), lvl, errorMin, iterno, err_out, sweeps_out);
    dfta_ctx* ctx = p->ctx;
    DFTA_ENTER(ctx);
    DFTA_REQUIRE(ctx, lvl >= 0 && lvl < p->D.levels && iterno >= 1 && iterno <= 1024, "level/iterno");
    DevBuf<double> dOut;
    DFTA_HIP(ctx, dOut.alloc(2));
    DFTA_HIP(ctx, hipMemcpyAsync(dOut.p, &errorMin, sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    double out[2] = {0, 0};
    if (int rc = run_unit(p, 4, lvl, iterno, dOut, out, 2)) return rc;
    if (err_out) *err_out = out[0];
    if (sweeps_out) *sweeps_out = (int)out[1];
    return check_groups(p);
}
// PoissonSolver::FullCycle (PoissonSolver.h:89-124) on atom 0's level storage: Initialize from the level-0 source that
// the last solve (or dfta_poisson_set_level) left there and from the boundary values, FMG ramp, up to 100 V-cycles
int dfta_poisson_full_cycle(dfta_poisson* p, double lowBoundary, double highBoundary, double errorMin, double errorMinLast,
                            double* err_out, int* vcycles_out)
{
    if (!p) return DFTA_ERR_INVALID;
    if (p->degraded) return dfta_poisson_full_cycle(p->fallback.get(), lowBoundary, highBoundary, errorMin, errorMinLast, err_out, vcycles_out);
    dfta_ctx* ctx = p->ctx;
    DFTA_ENTER(ctx);
    DevBuf<double> dOut;
    DFTA_HIP(ctx, dOut.alloc(4));
    double io[4] = {errorMin, errorMinLast, lowBoundary, highBoundary};
    DFTA_HIP(ctx, hipMemcpyAsync(dOut.p, io, sizeof(io), hipMemcpyHostToDevice, ctx->stream));
    std::fill(p->h_cur.begin(), p->h_cur.end(), 0);       // Initialize starts from copy 0 of every level
    if (int rc = run_unit(p, 5, 0, 0, dOut, io, 2)) return rc;
    if (err_out) *err_out = io[0];
    if (vcycles_out) *vcycles_out = (int)io[1];
    return check_groups(p);
}

int dfta_poisson_restrict(dfta_poisson* p, int lvl)
{
    if (!p) return DFTA_ERR_INVALID;
    DFTA_REQUIRE(p->ctx, lvl >= 1 && lvl < p->D.levels, "level");
    return unit_op(p, 1, lvl, 0, nullptr, 0);
}
int dfta_poisson_prolong(dfta_poisson* p, int lvl_src)
{
    if (!p) return DFTA_ERR_INVALID;
    DFTA_REQUIRE(p->ctx, lvl_src >= 1 && lvl_src < p->D.levels, "level");
    return unit_op(p, 2, lvl_src, 0, nullptr, 0);
}
int dfta_poisson_vcycle(dfta_poisson* p, double* err_out)
{
    if (!p) return DFTA_ERR_INVALID;
    return unit_op(p, 3, 0, 0, err_out, err_out ? 1 : 0);
}

}  // extern "C"
