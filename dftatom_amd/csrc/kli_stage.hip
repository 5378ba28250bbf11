// kli_stage.hip -- the exchange stage of a self-consistent KLI step: every live spin channel of a batch through one sequence of launches
// per chunk of whole channels, no host synchronisation in between (include/dftatom_hip.h states the rule; DESIGN.md 4.12 the shapes).
//
//   y launch            k_screening_yk of exchange.hip itself, one workgroup per job, the jobs of every channel of the chunk in one launch
//                       (the job table counts the batch's orbital rows).
//   k_kli_pointwise     grid (node tile, channel): X_a, D, vS -- the node arithmetic of k_exchange_pointwise (exchange_device.h).
//   k_kli_reduce        grid (quadrature of the chunk): vbarHF_a, vbarS_a, S_ab -- the lane chains and trees of k_exchange_reduce.
//   k_kli_solve         one wave per channel: the HOMO from the eigenvalues and occupations, the reduced system (I - M) c = vbarS - vbarHF in
//                       LDS, Gaussian elimination with partial pivoting in the header's order -- row i of an elimination step is lane i's,
//                       an element's operations do not depend on that --, back substitution by lane 0; then E_x of the channel, the last
//                       node with D > 0 and v_raw r there.
//   k_kli_update        grid (node tile, channel): the KLI pass, the Coulomb tail beyond the last node with D > 0, the mix into vx.
//   k_kli_assemble<false>  grid (node tile, atom), once per step: Vexc / va / vb / eexc from vx and the mixed densities; E_x of the atom.
// Under DFTA_EXCHANGE_SIC_KLI (dfta_kli_stage::sic) the builder of X_a differs and the rest is shared:
//   y launch            the diagonal jobs (a, a, 0) alone: one row per shell.
//   k_sic_pointwise     grid (node tile, channel): rho_a, v_a and eps_a (vwn_device.h: k_vwn_lsda's own arithmetic at (rho_a, 0)),
//                       X_a = (y0_a + v_a) u_a, D, vS.
//   k_kli_reduce<true, SicRows>  k_kli_reduce<false> plus the two quadratures EH_a and EXC_a, the same lane chains and trees.
//   k_kli_solve, then k_sic_energy (one thread per channel: E_SIC of the channel in place of E_x, the per-shell table), k_kli_update.
//   k_kli_assemble<true>  once per step AFTER the functional's launch: adds vx to Vexc / va / vb, takes it from eexc; E_SIC of the atom.
// Every shape is a function of N alone; no floating-point atomics; no workgroup waits for another: a channel's bits do not depend on the
// batch, its position in it, the chunking or the run.  Built, as everything here, without FMA contraction: the solve repeats the host
// solve of exchange_plan.cpp operation by operation.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <vector>

#include "exchange_device.h"
#include "internal.h"
#include "kli_stage.h"
#include "vwn_device.h"
#include "xc.h"

namespace {

using dfta_exchange_dev::kPwThreads;
using dfta_exchange_dev::kRedThreads;
using dfta_kli::Channel;
constexpr int kSolveThreads = 64;
constexpr int kSolveLd = 32;                 // row stride of the system in LDS

// X, D, vS of the chunk's channels [c0, c0 + gridDim.y); chunk rows: Y from job j0, X from orbital row u0, D / vS from channel c0
__global__ __launch_bounds__(kPwThreads) void k_kli_pointwise(int N, int c0, int j0, int u0, const Channel* __restrict__ chs,
                                                              const double* __restrict__ U, const double* __restrict__ occ,
                                                              const int* __restrict__ first, const int* __restrict__ tab,
                                                              const double* __restrict__ coef, const double* __restrict__ Y,
                                                              double* __restrict__ X, double* __restrict__ D, double* __restrict__ vS)
{
    const Channel ch = chs[c0 + blockIdx.y];
    const int i = blockIdx.x * kPwThreads + threadIdx.x;
    if (ch.norb == 0 || i >= N) return;
    double den, v;
    dfta_exchange_dev::pointwise_node(N, i, ch.norb, U + (size_t)ch.u0 * N, occ + ch.u0, first + ch.first0,
                                      tab + (size_t)dfta_kli::kTabInts * ch.tab0, coef + ch.tab0, Y + (size_t)(ch.job0 - j0) * N,
                                      X + (size_t)(ch.u0 - u0) * N, &den, &v);
    D[(size_t)blockIdx.y * N + i] = den;
    vS[(size_t)blockIdx.y * N + i] = v;
}

// the constants c of channel c0 + blockIdx.x, its HOMO, E_x, last node with D > 0 and v_raw r there
__global__ __launch_bounds__(kSolveThreads) void k_kli_solve(int N, int c0, const Channel* __restrict__ chs, const double* __restrict__ occ,
                                                             const char* __restrict__ Ebase, size_t Estride, const double* __restrict__ redout,
                                                             const double* __restrict__ r, const double* __restrict__ U,
                                                             const double* __restrict__ D, const double* __restrict__ vS,
                                                             double* __restrict__ cOut, double* __restrict__ vbarHF, int* __restrict__ homoOut,
                                                             double* __restrict__ ExCh, int* __restrict__ ilastOut, double* __restrict__ tailOut,
                                                             int* __restrict__ status)
{
    __shared__ double A[dfta_kli::kSolveMax * kSolveLd], rhs[kSolveLd], sol[kSolveLd], sOcc[kSolveLd], sE[kSolveLd], sC[kSolveLd];
    __shared__ int idx[kSolveLd];
    const int lane = threadIdx.x, c = c0 + blockIdx.x;
    const Channel ch = chs[c];
    const int n = ch.norb;
    if (n == 0) return;                      // homo, E_x, ilast keep what creation wrote: -1, 0, -1
    if (lane < n) {
        sOcc[lane] = occ[ch.u0 + lane];
        sE[lane] = *reinterpret_cast<const double*>(Ebase + (size_t)(ch.u0 + lane) * Estride);
    }
    __syncthreads();
    int h = -1;                              // every lane alike: the highest eigenvalue among the occupied shells, ties to the higher index
    for (int a = 0; a < n; ++a)
        if (sOcc[a] > 0. && (h < 0 || sE[a] >= sE[h])) h = a;
    const int H = n - 1;
    const double* vHF = redout + ch.red0;
    const double* vSb = vHF + n;
    const double* S = vSb + n;               // pair (a <= b) at a n - a (a - 1) / 2 + (b - a)
    if (lane < H) {
        const int a = lane < h ? lane : lane + 1;
        idx[lane] = a;
        rhs[lane] = vSb[a] - vHF[a];
    }
    if (lane < n) sC[lane] = 0.;
    __syncthreads();
    for (int e = lane; e < H * H; e += kSolveThreads) {
        const int i = e / H, j = e % H, a = idx[i], b = idx[j];
        const int lo = a < b ? a : b, hi = a < b ? b : a;
        const double M = S[lo * n - lo * (lo - 1) / 2 + (hi - lo)] * sOcc[b];
        A[i * kSolveLd + j] = (i == j ? 1. : 0.) - M;
    }
    __syncthreads();
    bool bad = false;
    for (int j = 0; j < H; ++j) {
        int p = j;                           // every lane alike
        for (int i = j + 1; i < H; ++i)
            if (fabs(A[i * kSolveLd + j]) > fabs(A[p * kSolveLd + j])) p = i;
        __syncthreads();
        if (p != j) {
            if (lane < H) { const double t = A[j * kSolveLd + lane]; A[j * kSolveLd + lane] = A[p * kSolveLd + lane]; A[p * kSolveLd + lane] = t; }
            if (lane == kSolveThreads - 1) { const double t = rhs[j]; rhs[j] = rhs[p]; rhs[p] = t; }
        }
        __syncthreads();
        const double piv = A[j * kSolveLd + j];
        if (piv == 0. || !isfinite(piv)) { bad = true; break; }
        if (lane > j && lane < H) {
            const double f = A[lane * kSolveLd + j] / piv;
            for (int m = j + 1; m < H; ++m) A[lane * kSolveLd + m] = A[lane * kSolveLd + m] - f * A[j * kSolveLd + m];
            rhs[lane] = rhs[lane] - f * rhs[j];
        }
        __syncthreads();
    }
    if (lane == 0) {
        if (!bad)
            for (int i = H - 1; i >= 0; --i) {
                double t = rhs[i];
                for (int m = i + 1; m < H; ++m) t = t - A[i * kSolveLd + m] * sol[m];
                sol[i] = t / A[i * kSolveLd + i];
            }
        for (int i = 0; i < H; ++i) sC[idx[i]] = bad ? nan("") : sol[i];
        double acc = 0.;
        for (int a = 0; a < n; ++a) acc += sOcc[a] * vHF[a];
        ExCh[c] = 0.5 * acc;
        homoOut[c] = h;
        status[c] = bad ? 1 : 0;
    }
    __syncthreads();
    if (lane < n) {
        cOut[ch.u0 + lane] = sC[lane];
        vbarHF[ch.u0 + lane] = vHF[lane];
    }
    const double* Dc = D + (size_t)blockIdx.x * N;
    int il = -1;
    for (int i = lane; i < N; i += kSolveThreads)
        if (Dc[i] > 0.) il = i;              // ascending: the lane's last one stays
    for (int off = 32; off > 0; off >>= 1) il = max(il, __shfl_xor(il, off));
    if (lane == 0) {
        ilastOut[c] = il;
        double tail = 0.;
        if (il >= 0) {
            const double v = dfta_exchange_dev::kli_node(N, il, n, h, U + (size_t)ch.u0 * N, sOcc, sC, Dc[il], vS[(size_t)blockIdx.x * N + il]);
            tail = v * r[il];
        }
        tailOut[c] = tail;
    }
}

// v_raw and vx of the chunk's channels
__global__ __launch_bounds__(kPwThreads) void k_kli_update(int N, int c0, const Channel* __restrict__ chs, const double* __restrict__ occ,
                                                           const double* __restrict__ U, const double* __restrict__ cArr,
                                                           const int* __restrict__ homo, const double* __restrict__ D,
                                                           const double* __restrict__ vS, const int* __restrict__ ilast,
                                                           const double* __restrict__ tail, const double* __restrict__ r, int first, double alpha,
                                                           double oneMinusAlpha, double* __restrict__ vx, double* __restrict__ vraw)
{
    const int c = c0 + blockIdx.y;
    const Channel ch = chs[c];
    const int i = blockIdx.x * kPwThreads + threadIdx.x;
    if (ch.norb == 0 || i >= N) return;
    const size_t o = (size_t)blockIdx.y * N + i, oc = (size_t)c * N + i;
    double v = dfta_exchange_dev::kli_node(N, i, ch.norb, homo[c], U + (size_t)ch.u0 * N, occ + ch.u0, cArr + ch.u0, D[o], vS[o]);
    const int il = ilast[c];
    if (il >= 0 && i > il) v = tail[c] / r[i];           // the Coulomb tail, continuous at il
    vraw[oc] = v;
    vx[oc] = first ? v : alpha * vx[oc] + oneMinusAlpha * v;
}

// ---- the self-interaction correction: the builder of X_a, the two energy quadratures, E_SIC and the additive assembly --------------------
// rho_a, v_a, eps_a, X_a, D, vS of the chunk's channels [c0, c0 + gridDim.y); chunk rows: Y from job j0; vorb, eps, X from orbital row u0
__global__ __launch_bounds__(kPwThreads) void k_sic_pointwise(int N, int c0, int j0, int u0, const Channel* __restrict__ chs,
                                                              const double* __restrict__ U, const double* __restrict__ occ,
                                                              const double* __restrict__ r, const double* __restrict__ Y, double cx,
                                                              double cbrt2, double* __restrict__ vorb, double* __restrict__ eps,
                                                              double* __restrict__ X, double* __restrict__ D, double* __restrict__ vS)
{
    const Channel ch = chs[c0 + blockIdx.y];
    const int i = blockIdx.x * kPwThreads + threadIdx.x;
    if (ch.norb == 0 || i >= N) return;
    const dfta_vwn_dev::LsdaConsts k = dfta_vwn_dev::lsda_consts(cx, cbrt2);
    const double* Uc = U + (size_t)ch.u0 * N;
    const double* Yc = Y + (size_t)(ch.job0 - j0) * N;
    const size_t row0 = (size_t)(ch.u0 - u0) * N;
    const double ri = r[i];
    const double fpr2 = (dfta_vwn_dev::kFourPi * ri) * ri;
    double den = 0., num = 0.;
    for (int a = 0; a < ch.norb; ++a) {
        const double ua = Uc[(size_t)a * N + i];
        const double rho = i >= 1 ? (ua * ua) / fpr2 : 0.;
        const dfta_vwn_dev::LsdaPoint p = dfta_vwn_dev::lsda_point(k, rho, 0.);
        const double x = (Yc[(size_t)a * N + i] + p.vup) * ua;
        const size_t o = row0 + (size_t)a * N + i;
        vorb[o] = p.vup;
        eps[o] = p.common + p.e;
        X[o] = x;
        den += occ[ch.u0 + a] * (ua * ua);
        num += occ[ch.u0 + a] * (ua * x);
    }
    D[(size_t)blockIdx.y * N + i] = den;
    vS[(size_t)blockIdx.y * N + i] = den > 0. ? -(num / den) : 0.;
}

// what the SIC quadratures read beyond the KLI ones: the chunk's y rows from job j0 and eps rows (from orbital row u0)
struct SicRows { int j0; const double* Y; const double* eps; };

// quadrature q0 + blockIdx.x of the batch's table: vbarHF_a, vbarS_a, S_ab; kSic: also EH_a / EXC_a as the kRedS chain on y0_a / eps_a.
// Rows is one SicRows under kSic and nothing otherwise: the KLI instance has the thirteen arguments it uses and compiles to the code it
// had (three unused arguments measured 0.5 us on the stage of a Ne step)
template <bool kSic, typename... Rows>
__global__ __launch_bounds__(kRedThreads) void k_kli_reduce(int N, double hstep, int q0, int c0, int u0, const Channel* __restrict__ chs,
                                                            const int* __restrict__ red, const double* __restrict__ cnst,
                                                            const double* __restrict__ U, const double* __restrict__ X,
                                                            const double* __restrict__ D, const double* __restrict__ vS,
                                                            double* __restrict__ out, Rows... rows)
{
    __shared__ double part[kRedThreads / 64];
    const int* row = red + (size_t)dfta_kli::kRedInts * (q0 + blockIdx.x);
    const int kind = row[0], a = row[1], b = row[2], c = row[3];
    const Channel ch = chs[c];
    const double* Uc = U + (size_t)ch.u0 * N;
    const double* v = vS + (size_t)(c - c0) * N;
    int shape = kind;
    if constexpr (kSic) {
        const SicRows sic = (rows, ...);
        if (kind == dfta_kli::kRedSicH) { v = sic.Y + (size_t)(ch.job0 - sic.j0 + a) * N; shape = dfta_exchange::kRedS; }
        else if (kind == dfta_kli::kRedSicXC) { v = sic.eps + (size_t)(ch.u0 - u0 + a) * N; shape = dfta_exchange::kRedS; }
    }
    double q = dfta_exchange_dev::reduce_block(N, hstep, cnst, Uc + (size_t)a * N, Uc + (size_t)b * N, X + (size_t)(ch.u0 - u0 + a) * N,
                                               D + (size_t)(c - c0) * N, v, shape, part);
    if (kSic && kind == dfta_kli::kRedSicH) q = 0.5 * q;
    if (threadIdx.x == 0) out[q0 + blockIdx.x] = q;
}

// E_SIC of the channels [c0, c0 + nc) in place of the E_x k_kli_solve wrote, and their per-shell table; one thread per channel
__global__ void k_sic_energy(int c0, int nc, const Channel* __restrict__ chs, const double* __restrict__ occ, const double* __restrict__ redout,
                             double* __restrict__ EH, double* __restrict__ EXC, double* __restrict__ ExCh)
{
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= nc) return;
    const Channel ch = chs[c0 + k];
    const int n = ch.norb;
    if (n == 0) return;
    const double* eh = redout + ch.red0 + 2 * n + n * (n + 1) / 2;
    const double* exc = eh + n;
    double acc = 0.;
    for (int a = 0; a < n; ++a) {
        acc += occ[ch.u0 + a] * (eh[a] + exc[a]);
        EH[ch.u0 + a] = eh[a];
        EXC[ch.u0 + a] = exc[a];
    }
    ExCh[c0 + k] = -acc;
}

// once per step, grid (node tile, atom): vx and E_x of the atom into the SCF's arrays.  kAdd false (KLI, in place of the functional's
// launch): Vexc / va / vb = the potential, eexc = -Vexc.  kAdd true (SIC, after the functional's launch): added to Vexc / va / vb, taken
// from eexc
template <bool kAdd>
__global__ __launch_bounds__(kPwThreads) void k_kli_assemble(int N, int lsda, const int* __restrict__ fin, const double* __restrict__ vx,
                                                             const double* __restrict__ ExCh, const double* __restrict__ density,
                                                             const double* __restrict__ dA, const double* __restrict__ dB,
                                                             double* __restrict__ Vexc, double* __restrict__ va, double* __restrict__ vb,
                                                             double* __restrict__ eexc, double* __restrict__ ExAtom)
{
    const int a = blockIdx.y;
    if (fin[a]) return;                      // a finished atom keeps its potential and its E_x / E_SIC
    const int i = blockIdx.x * kPwThreads + threadIdx.x;
    if (i == 0) ExAtom[a] = lsda ? ExCh[2 * a] + ExCh[2 * a + 1] : 2. * ExCh[a];
    if (i >= N) return;
    const size_t o = (size_t)a * N + i;
    double t;
    if (!lsda) t = vx[o];
    else {
        const double x = vx[((size_t)2 * a) * N + i], y = vx[((size_t)2 * a + 1) * N + i];
        const double rho = density[o];
        va[o] = kAdd ? va[o] + x : x;
        vb[o] = kAdd ? vb[o] + y : y;
        t = rho > 0. ? (dA[o] * x + dB[o] * y) / rho : 0.;
    }
    Vexc[o] = kAdd ? Vexc[o] + t : t;
    eexc[o] = kAdd ? eexc[o] - t : -t;
}

}  // namespace

void dfta_kli_stage::reset()
{
    plan = dfta_kli::Plan();
    max_rows = 0; caps = {0, 0, 0}; N = 0; natoms = 0; timed = false; sic = false;
    d_ch.reset();
    for (DevBuf<int>* b : {&d_jobs, &d_first, &d_tab, &d_red, &d_homo, &d_ilast, &d_status}) b->reset();
    for (DevBuf<double>* b : {&d_coef, &d_occ, &d_y, &d_X, &d_DvS, &d_redout, &d_vx, &d_vraw, &d_vbarHF, &d_c, &d_tail, &d_ExCh, &d_ExAtom, &d_vorb, &d_eps, &d_EH,
                          &d_EXC}) b->reset();
    h_status.clear(); bounds.clear();
}

int dfta_kli_stage::create(dfta_ctx* ctx, const dfta_grid* g, int nch, const int* norb, const int* l, const double* occ, const int* atom,
                           int natoms_, double y_mb, bool sic_)
{
    reset();
    if (const char* msg = dfta_kli::check_channels(nch, norb, l, occ)) DFTA_REQUIRE(ctx, false, msg);
    DFTA_REQUIRE(ctx, g->N >= 5, "KLI channels: the grid needs 5 nodes");
    DFTA_REQUIRE(ctx, nch >= 1 && nch <= 65535, "KLI channels: 1 .. 65535 channels");
    DFTA_REQUIRE(ctx, (sic_ ? dfta_kli::plan_channels_sic(nch, norb, l, occ, atom, &plan) : dfta_kli::plan_channels(nch, norb, l, occ, atom, &plan)) == 0,
                 "KLI channels: the tables");
    hipStream_t st = ctx->stream;
    const size_t n = g->N, no = std::max(plan.norb_total, 1);
    max_rows = dfta_kli::budget_rows(y_mb, g->N);
    caps = dfta_kli::capacities(plan, max_rows);
    hipError_t e = hipSuccess;
    auto al = [&](auto& buf, size_t cnt) { if (e == hipSuccess) e = buf.alloc(std::max<size_t>(cnt, 1)); };
    al(d_ch, nch); al(d_jobs, plan.jobs.size()); al(d_first, plan.first.size()); al(d_tab, plan.tab.size()); al(d_red, plan.red.size());
    al(d_coef, plan.coef.size()); al(d_occ, no);
    al(d_y, (size_t)caps.yrows * n); al(d_X, (size_t)caps.xrows * n); al(d_DvS, 2 * (size_t)caps.chans * n); al(d_redout, plan.nred());
    al(d_vx, (size_t)nch * n); al(d_vraw, (size_t)nch * n); al(d_vbarHF, no); al(d_c, no); al(d_tail, nch); al(d_ExCh, nch);
    al(d_ExAtom, natoms_); al(d_homo, nch); al(d_ilast, nch); al(d_status, nch);
    if (sic_) { al(d_vorb, (size_t)caps.xrows * n); al(d_eps, (size_t)caps.xrows * n); al(d_EH, no); al(d_EXC, no); }
    for (auto& v : ev) if (e == hipSuccess && !v.e) e = hipEventCreate(&v.e);
    if (e != hipSuccess) {
        snprintf(ctx->err, sizeof(ctx->err), "KLI stage alloc: %s", hipGetErrorString(e));
        reset();
        (void)hipGetLastError();
        return e == hipErrorOutOfMemory ? DFTA_ERR_NOMEM : DFTA_ERR_HIP;
    }
    auto up = [&](auto& buf, const auto& vec) {
        if (e == hipSuccess && !vec.empty()) e = hipMemcpyAsync(buf.p, vec.data(), sizeof(vec[0]) * vec.size(), hipMemcpyHostToDevice, st);
    };
    up(d_ch, plan.ch); up(d_jobs, plan.jobs); up(d_first, plan.first); up(d_tab, plan.tab); up(d_red, plan.red); up(d_coef, plan.coef);
    if (e == hipSuccess && plan.norb_total > 0) e = hipMemcpyAsync(d_occ.p, occ, sizeof(double) * plan.norb_total, hipMemcpyHostToDevice, st);
    auto zero = [&](auto& buf, int byte) { if (e == hipSuccess) e = hipMemsetAsync(buf.p, byte, sizeof(*buf.p) * buf.n, st); };
    zero(d_vx, 0); zero(d_vraw, 0); zero(d_vbarHF, 0); zero(d_c, 0); zero(d_tail, 0); zero(d_ExCh, 0); zero(d_ExAtom, 0); zero(d_status, 0);
    zero(d_homo, 0xff); zero(d_ilast, 0xff);
    if (sic_) { zero(d_EH, 0); zero(d_EXC, 0); }
    if (e == hipSuccess) e = hipStreamSynchronize(st);                   // occ is the caller's; the plan's vectors stay
    if (e != hipSuccess) {
        snprintf(ctx->err, sizeof(ctx->err), "KLI stage tables: %s", hipGetErrorString(e));
        reset();
        return DFTA_ERR_HIP;
    }
    N = g->N; natoms = natoms_; sic = sic_;
    h_status.assign(nch, 0);
    return DFTA_OK;
}

int dfta_kli_stage::run(dfta_ctx* ctx, const dfta_grid* g, const double* dU, const void* Ebase, size_t Estride, const unsigned char* live,
                        bool first, double alpha, double oneMinusAlpha, const Dump* dump)
{
    hipStream_t st = ctx->stream;
    const double hstep = dfta_hstep(g);
    const int nblk = (N + kPwThreads - 1) / kPwThreads;
    double* dD = d_DvS.p;
    double* dvS = d_DvS.p + (size_t)caps.chans * N;
    dfta_kli::plan_chunks(plan, live, max_rows, &bounds);
    DFTA_HIP(ctx, hipEventRecord(ev[0], st));
    for (size_t k = 0; k + 1 < bounds.size(); k += 2) {
        const int c0 = bounds[k], c1 = bounds[k + 1], nc = c1 - c0;
        const dfta_kli::Channel& a = plan.ch[c0];
        const dfta_kli::Channel& z = plan.ch[c1 - 1];
        const int njobs = z.job0 + z.njobs - a.job0, nred = z.red0 + z.nred - a.red0, norb = z.u0 + z.norb - a.u0;
        DFTA_REQUIRE(ctx, njobs <= caps.yrows && norb <= caps.xrows && nc <= caps.chans, "KLI stage: a chunk beyond its buffers");
        int rc = dfta_launch_screening_yk(ctx, g, dU, njobs, d_jobs.p + (size_t)dfta_kli::kJobInts * a.job0, d_y.p);
        if (rc) return rc;
        if (!sic) {
            hipLaunchKernelGGL(k_kli_pointwise, dim3(nblk, nc), dim3(kPwThreads), 0, st, N, c0, a.job0, a.u0, d_ch.p, dU, d_occ.p, d_first.p, d_tab.p,
                               d_coef.p, d_y.p, d_X.p, dD, dvS);
            DFTA_CHECK_LAUNCH(ctx);
        } else {
            hipLaunchKernelGGL(k_sic_pointwise, dim3(nblk, nc), dim3(kPwThreads), 0, st, N, c0, a.job0, a.u0, d_ch.p, dU, d_occ.p, g->d_r.p, d_y.p,
                               dfta_vwn_cx(), dfta_vwn_cbrt2(), d_vorb.p, d_eps.p, d_X.p, dD, dvS);
            DFTA_CHECK_LAUNCH(ctx);
        }
        if (!sic)
            hipLaunchKernelGGL(k_kli_reduce<false>, dim3(nred), dim3(kRedThreads), 0, st, N, hstep, a.red0, c0, a.u0, d_ch.p, d_red.p, g->d_cnst.p, dU,
                               d_X.p, dD, dvS, d_redout.p);
        else
            hipLaunchKernelGGL((k_kli_reduce<true, SicRows>), dim3(nred), dim3(kRedThreads), 0, st, N, hstep, a.red0, c0, a.u0, d_ch.p, d_red.p, g->d_cnst.p, dU,
                               d_X.p, dD, dvS, d_redout.p, SicRows{a.job0, d_y.p, d_eps.p});
        DFTA_CHECK_LAUNCH(ctx);
        hipLaunchKernelGGL(k_kli_solve, dim3(nc), dim3(kSolveThreads), 0, st, N, c0, d_ch.p, d_occ.p, static_cast<const char*>(Ebase), Estride,
                           d_redout.p, g->d_r.p, dU, dD, dvS, d_c.p, d_vbarHF.p, d_homo.p, d_ExCh.p, d_ilast.p, d_tail.p, d_status.p);
        DFTA_CHECK_LAUNCH(ctx);
        if (sic) {
            hipLaunchKernelGGL(k_sic_energy, dim3((nc + 63) / 64), dim3(64), 0, st, c0, nc, d_ch.p, d_occ.p, d_redout.p, d_EH.p, d_EXC.p, d_ExCh.p);
            DFTA_CHECK_LAUNCH(ctx);
        }
        hipLaunchKernelGGL(k_kli_update, dim3(nblk, nc), dim3(kPwThreads), 0, st, N, c0, d_ch.p, d_occ.p, dU, d_c.p, d_homo.p, dD, dvS, d_ilast.p,
                           d_tail.p, g->d_r.p, first ? 1 : 0, alpha, oneMinusAlpha, d_vx.p, d_vraw.p);
        DFTA_CHECK_LAUNCH(ctx);
        if (dump) {                              // the chunk's rows into the caller's whole-batch arrays (device to device, on the stream)
            auto keep = [&](double* dst, size_t row, const double* src, size_t rows) {
                return dst && rows ? hipMemcpyAsync(dst + row * N, src, sizeof(double) * rows * N, hipMemcpyDeviceToDevice, st) : hipSuccess;
            };
            DFTA_HIP(ctx, keep(dump->y, a.job0, d_y.p, njobs));
            DFTA_HIP(ctx, keep(dump->X, a.u0, d_X.p, norb));
            DFTA_HIP(ctx, keep(dump->vorb, a.u0, d_vorb.p, sic ? norb : 0));
            DFTA_HIP(ctx, keep(dump->eps, a.u0, d_eps.p, sic ? norb : 0));
            DFTA_HIP(ctx, keep(dump->D, c0, dD, nc));
            DFTA_HIP(ctx, keep(dump->vS, c0, dvS, nc));
        }
    }
    DFTA_HIP(ctx, hipEventRecord(ev[1], st));
    timed = true;
    DFTA_HIP(ctx, hipMemcpyAsync(h_status.data(), d_status.p, sizeof(int) * plan.nch(), hipMemcpyDeviceToHost, st));
    return DFTA_OK;
}

int dfta_kli_stage::assemble(dfta_ctx* ctx, const dfta_grid* g, int lsda, const double* density, const double* dA, const double* dB,
                             const int* fin, double* Vexc, double* va, double* vb, double* eexc)
{
    hipLaunchKernelGGL(sic ? k_kli_assemble<true> : k_kli_assemble<false>, dim3((N + kPwThreads - 1) / kPwThreads, natoms), dim3(kPwThreads), 0,
                       ctx->stream, N, lsda, fin, d_vx.p, d_ExCh.p, density, dA, dB, Vexc, va, vb, eexc, d_ExAtom.p);
    DFTA_CHECK_LAUNCH(ctx);
    return DFTA_OK;
}

double dfta_kli_budget_mb()
{
    const char* v = dfta_knob("KLI_Y_MB");
    return v && *v ? atof(v) : kKliDefaultYMB;
}

// ---- the stage on caller-supplied channels (host pointers) ---------------------------------------------------------------------------
namespace {

// what dfta_sic_channels returns beyond dfta_kli_channels (any may be null): y0, vorb, eps, X of every shell (rows of N), D and vS of every
// channel, EH and EXC per shell, vbarS per shell and M per channel from the quadratures
struct SicOutputs { double *y0, *vorb, *eps, *X, *D, *vS, *EH, *EXC, *vbarS, *M; };

// both entries: the checks, one stage made for the call, the uploads, the run between the events of dfta_ctx_last_kernel_ms (the whole
// stage), the downloads.  sic: null for dfta_kli_channels
int run_channels(dfta_ctx* ctx, const dfta_grid* g, int nch, const int* norb, const int* l, const double* occ, const double* E, const double* u,
                 int first_step, double alpha, double* vx_inout, double* v_raw, double* vbarHF, double* c, int* homo, double* Ex,
                 const SicOutputs* sic)
{
    if (!ctx || !g) return DFTA_ERR_INVALID;
    DFTA_ENTER(ctx);
    DFTA_REQUIRE(ctx, nch >= 0, sic ? "dfta_sic_channels: nch" : "dfta_kli_channels: nch");
    if (nch == 0) return DFTA_OK;
    DFTA_REQUIRE(ctx, norb, sic ? "dfta_sic_channels: norb" : "dfta_kli_channels: norb");
    DFTA_REQUIRE(ctx, alpha >= 0 && alpha <= 1, sic ? "dfta_sic_channels: alpha" : "dfta_kli_channels: alpha");
    long total = 0;
    for (int k = 0; k < nch; ++k) total += norb[k] > 0 ? norb[k] : 0;
    DFTA_REQUIRE(ctx, total == 0 || (l && occ && E && u), sic ? "dfta_sic_channels: l / occ / E / u" : "dfta_kli_channels: l / occ / E / u");
    DFTA_REQUIRE(ctx, first_step || vx_inout,
                 sic ? "dfta_sic_channels: a later step mixes into vx_inout" : "dfta_kli_channels: a later step mixes into vx_inout");
    dfta_kli_stage stage;
    int rc = stage.create(ctx, g, nch, norb, l, occ, nullptr, 0, dfta_kli_budget_mb(), sic != nullptr);
    if (rc) return rc;
    hipStream_t st = ctx->stream;
    const size_t N = g->N, no = stage.plan.norb_total;
    DevBuf<double> dU, dE, dRows[4], dChan[2];       // rows: y0, vorb, eps, X of every shell; D, vS of every channel
    DFTA_HIP(ctx, dU.alloc(std::max<size_t>(no * N, 1)));
    DFTA_HIP(ctx, dE.alloc(std::max<size_t>(no, 1)));
    double* hostRows[4] = {nullptr, nullptr, nullptr, nullptr};
    double* hostChan[2] = {nullptr, nullptr};
    if (sic) { hostRows[0] = sic->y0; hostRows[1] = sic->vorb; hostRows[2] = sic->eps; hostRows[3] = sic->X; hostChan[0] = sic->D; hostChan[1] = sic->vS; }
    for (int k = 0; k < 4; ++k)
        if (hostRows[k] && no) DFTA_HIP(ctx, dRows[k].alloc(no * N));
    for (int k = 0; k < 2; ++k)
        if (hostChan[k]) {
            DFTA_HIP(ctx, dChan[k].alloc((size_t)nch * N));
            DFTA_HIP(ctx, hipMemsetAsync(dChan[k].p, 0, sizeof(double) * nch * N, st));      // a channel without shells: zeros
        }
    if (no) {
        DFTA_HIP(ctx, hipMemcpyAsync(dU.p, u, sizeof(double) * no * N, hipMemcpyHostToDevice, st));
        DFTA_HIP(ctx, hipMemcpyAsync(dE.p, E, sizeof(double) * no, hipMemcpyHostToDevice, st));
    }
    if (!first_step) DFTA_HIP(ctx, hipMemcpyAsync(stage.d_vx.p, vx_inout, sizeof(double) * nch * N, hipMemcpyHostToDevice, st));
    const dfta_kli_stage::Dump dump = {dRows[0].p, dRows[1].p, dRows[2].p, dRows[3].p, dChan[0].p, dChan[1].p};
    DFTA_HIP(ctx, dfta_timer_start(ctx));
    rc = stage.run(ctx, g, dU.p, dE.p, sizeof(double), nullptr, first_step != 0, alpha, 1. - alpha, sic ? &dump : nullptr);
    if (rc) return rc;
    DFTA_HIP(ctx, dfta_timer_stop(ctx));
    auto down = [&](auto* host, const auto* dev, size_t count) {
        return host && count ? hipMemcpyAsync(host, dev, sizeof(*host) * count, hipMemcpyDeviceToHost, st) : hipSuccess;
    };
    for (int k = 0; k < 4; ++k) DFTA_HIP(ctx, down(dRows[k].p ? hostRows[k] : nullptr, dRows[k].p, no * N));
    for (int k = 0; k < 2; ++k) DFTA_HIP(ctx, down(hostChan[k], dChan[k].p, (size_t)nch * N));
    DFTA_HIP(ctx, down(vx_inout, stage.d_vx.p, (size_t)nch * N));
    DFTA_HIP(ctx, down(v_raw, stage.d_vraw.p, (size_t)nch * N));
    DFTA_HIP(ctx, down(vbarHF, stage.d_vbarHF.p, no));
    DFTA_HIP(ctx, down(c, stage.d_c.p, no));
    DFTA_HIP(ctx, down(homo, stage.d_homo.p, (size_t)nch));
    DFTA_HIP(ctx, down(Ex, stage.d_ExCh.p, (size_t)nch));
    std::vector<double> red;
    if (sic) {
        DFTA_HIP(ctx, down(sic->EH, stage.d_EH.p, no));
        DFTA_HIP(ctx, down(sic->EXC, stage.d_EXC.p, no));
        red.assign((sic->vbarS || sic->M) ? stage.plan.nred() : 0, 0.);
        DFTA_HIP(ctx, down(red.data(), stage.d_redout.p, red.size()));
    }
    DFTA_HIP(ctx, hipStreamSynchronize(st));
    if (!red.empty()) {
        double* vbarS = sic->vbarS;
        double* M = sic->M;
        size_t m0 = 0;
        for (const dfta_kli::Channel& ch : stage.plan.ch) {
            const int n = ch.norb;
            const double* S = red.data() + ch.red0 + 2 * n;     // pair (a <= b) at a n - a (a - 1) / 2 + (b - a)
            for (int a = 0; a < n; ++a) {
                if (vbarS) vbarS[ch.u0 + a] = red[ch.red0 + n + a];
                for (int b = 0; M && b < n; ++b) {
                    const int lo = a < b ? a : b, hi = a < b ? b : a;
                    M[m0 + (size_t)a * n + b] = S[lo * n - lo * (lo - 1) / 2 + (hi - lo)] * occ[ch.u0 + b];
                }
            }
            m0 += (size_t)n * n;
        }
    }
    return DFTA_OK;
}

}  // namespace

extern "C" {

int dfta_kli_channels(dfta_ctx* ctx, const dfta_grid* g, int nch, const int* norb, const int* l, const double* occ, const double* E,
                      const double* u, int first_step, double alpha, double* vx_inout, double* v_raw, double* vbarHF, double* c, int* homo,
                      double* Ex)
{
    return run_channels(ctx, g, nch, norb, l, occ, E, u, first_step, alpha, vx_inout, v_raw, vbarHF, c, homo, Ex, nullptr);
}

int dfta_sic_channels(dfta_ctx* ctx, const dfta_grid* g, int nch, const int* norb, const int* l, const double* occ, const double* E,
                      const double* u, int first_step, double alpha, double* vx_inout, double* y0, double* vorb, double* eps, double* X,
                      double* D, double* vS, double* v_raw, double* vbar, double* c, double* EH, double* EXC, int* homo, double* Esic,
                      double* vbarS, double* M)
{
    const SicOutputs sic = {y0, vorb, eps, X, D, vS, EH, EXC, vbarS, M};
    return run_channels(ctx, g, nch, norb, l, occ, E, u, first_step, alpha, vx_inout, v_raw, vbar, c, homo, Esic, &sic);
}

}  // extern "C"
