// exchange.hip -- exchange potentials from radial orbitals u_i = r_i R_nl(r_i): the screening functions y^k_xy = Y^k_xy / r, the exchange
// operator applied to the orbitals of a spin channel, Slater's averaged potential and the KLI potential (include/dftatom_hip.h has the
// definitions and the stated orders; DESIGN.md 4.11 the scans' shape and the rounding bounds).  Beyond the reference.
//
//   k_screening_yk      one workgroup of 256 lanes per job (x, y, k), every job of a call in one launch, no communication between
//                       workgroups.  Two passes over the tiles of kYkTile nodes.  Forward, tile 0 upwards: g = (r^k P) s is staged with
//                       its halo, lane t chains the four increments of the nodes tile * kYkTile + 4 t .. + 3, the lanes' totals are
//                       scanned across the wave by shuffles (six levels), the four waves' totals chained through LDS, the carry of the
//                       earlier tiles added last -- k_slater_rk's scan -- and Z_i inv_i goes to the row.  Backward, last tile downwards:
//                       the mirror image on h = (P inv) s, with E_i = e_{i+1} held at node i: the lane's chain runs from its last node
//                       down, the wave scan takes lane t + off, the waves chain from wave 3 down, the carry is that of the later tiles;
//                       W_i = Sum_{j >= i} E_j, and the lane that wrote Z_i inv_i reads it back and adds p_i W_i.
//   k_exchange_pointwise  one lane per node: X_a of every shell from the y rows through the channel's table, D, num, vS.
//   k_exchange_kli        one lane per node: vKLI from vS, D and the constants c.
//   k_exchange_reduce     one workgroup per quadrature (vbarHF_a, vbarS_a, vbarKLI_a, S_ab): lane t adds the weighted terms of the nodes
//                         t, t + 256, ... to one accumulator; the end is k_orbital_properties' tree.
// The per-node and per-quadrature arithmetic of the last three is exchange_device.h's, shared with the batched stage of kli_stage.hip.
// Every shape is a function of N alone.  No floating-point atomics; no workgroup waits for another.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "exchange_device.h"
#include "exchange_plan.h"
#include "internal.h"
#include "radial_device.h"

namespace {

constexpr int kYkThreads = 256;
constexpr int kYkPer = 4;                            // consecutive nodes per lane
constexpr int kYkTile = kYkThreads * kYkPer;         // nodes per tile
constexpr int kYkHalo = 3;                           // nodes staged in front of and behind a tile: the reach of the end stencils
constexpr int kYkSlots = kYkTile + 2 * kYkHalo;      // slot q of the running tile [t0, t0 + kYkTile) holds node t0 - kYkHalo + q
using dfta_exchange_dev::kPwThreads;
using dfta_exchange_dev::kRedThreads;
using namespace dfta_radial;

__global__ __launch_bounds__(kYkThreads) void k_screening_yk(int N, double hstep, const double* __restrict__ r, const double* __restrict__ cnst,
                                                             const double* __restrict__ U, const int* __restrict__ jobs, double* Y)
{
    __shared__ double sg[kYkSlots];                  // the scanned integrand: g forward, h backward
    __shared__ double sf[kYkSlots];                  // the outer factor: inv forward, p backward
    __shared__ double wtot[kYkThreads / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int* __restrict__ job = jobs + (size_t)dfta_exchange::kJobInts * blockIdx.x;
    const int x = min(job[0], job[1]), y = max(job[0], job[1]), k = job[2];
    const double* __restrict__ ux = U + (size_t)x * N;
    const double* __restrict__ uy = U + (size_t)y * N;
    double* out = Y + (size_t)blockIdx.x * N;

    // stages the nodes t0 - kYkHalo .. t0 + kYkTile + kYkHalo - 1 (zeros outside the grid)
    auto stage = [&](int t0, bool forward) {
        for (int q = tid; q < kYkSlots; q += kYkThreads) {
            const int i = t0 - kYkHalo + q;
            double vg = 0., vf = 0.;
            if (i >= 0 && i < N) {
                const double a0 = ux[i];
                const double P = a0 * (y == x ? a0 : uy[i]);
                const NodeFactors f = node_factors(k, r[i], cnst[i], hstep, i);
                vg = forward ? (f.p * P) * f.sc : (P * f.inv) * f.sc;
                vf = forward ? f.inv : f.p;
            }
            sg[q] = vg;
            sf[q] = vf;
        }
    };

    const int q0 = kYkHalo + kYkPer * tid;
    // ---- forward: Z_i inv_i -------------------------------------------------------------------------------------------------------
    double carry = 0.;
    for (int t0 = 0; t0 < N; t0 += kYkTile) {
        stage(t0, true);                             // the tile before was read (into registers) ahead of its second barrier
        __syncthreads();
        const int i0 = t0 + kYkPer * tid;
        // radial_device.h's scan of a tile, with chain_up and waves_chain_up written out: called as functions they give this kernel
        // another instruction schedule, 0.7 us (0.8 %) slower on 300 jobs at 8193 nodes; written out it compiles to the code it had
        double lx[kYkPer], f[kYkPer];
        double tx = 0.;
#pragma unroll
        for (int j = 0; j < kYkPer; ++j) {
            const int i = i0 + j;
            const double d = (i >= 1 && i < N) ? increment(sg, q0 + j, i, N) : 0.;
            tx = j == 0 ? d : tx + d;
            lx[j] = tx;
            f[j] = sf[q0 + j];
        }
        const LanePrefix px = wave_prefix_up(tx, lane);
        if (lane == 63) wtot[wave] = px.inc;
        __syncthreads();
        const double off = wave == 0 ? 0. : (wave == 1 ? wtot[0] : (wave == 2 ? wtot[0] + wtot[1] : (wtot[0] + wtot[1]) + wtot[2]));
        const double tot = ((wtot[0] + wtot[1]) + wtot[2]) + wtot[3];
        const double b = off + px.ex;
#pragma unroll
        for (int j = 0; j < kYkPer; ++j) {
            const int i = i0 + j;
            if (i < N) out[i] = (carry + (b + lx[j])) * f[j];
        }
        carry = carry + tot;
    }
    // ---- backward: + p_i W_i, W_i = Sum_{j >= i} E_j, E_j = e_{j+1} -----------------------------------------------------------------
    carry = 0.;
    for (int t0 = ((N - 1) / kYkTile) * kYkTile; t0 >= 0; t0 -= kYkTile) {
        stage(t0, false);
        __syncthreads();
        const int i0 = t0 + kYkPer * tid;
        double lw[kYkPer], f[kYkPer];                // chain_down and waves_chain_down written out, for the same reason
        double tw = 0.;
#pragma unroll
        for (int j = kYkPer - 1; j >= 0; --j) {
            const int i = i0 + j;
            const double e = i < N - 1 ? increment(sg, q0 + j + 1, i + 1, N) : 0.;
            tw = j == kYkPer - 1 ? e : tw + e;
            lw[j] = tw;
            f[j] = sf[q0 + j];
        }
        const LanePrefix pw = wave_prefix_down(tw, lane);
        if (lane == 0) wtot[wave] = pw.inc;
        __syncthreads();
        const double off = wave == 3 ? 0. : (wave == 2 ? wtot[3] : (wave == 1 ? wtot[3] + wtot[2] : (wtot[3] + wtot[2]) + wtot[1]));
        const double tot = ((wtot[3] + wtot[2]) + wtot[1]) + wtot[0];
        const double b = off + pw.ex;
#pragma unroll
        for (int j = 0; j < kYkPer; ++j) {
            const int i = i0 + j;
            if (i >= N) continue;
            const double W = carry + (b + lw[j]);
            out[i] = i > 0 ? out[i] + f[j] * W : (k == 0 ? W : 0.);      // this lane wrote out[i] in the forward pass
        }
        carry = carry + tot;
    }
}

// X_a of every shell, D, num and vS at one node per lane
__global__ __launch_bounds__(kPwThreads) void k_exchange_pointwise(int N, int norb, const double* __restrict__ U, const double* __restrict__ occ,
                                                                   const int* __restrict__ first, const int* __restrict__ tab,
                                                                   const double* __restrict__ coef, const double* __restrict__ Y,
                                                                   double* __restrict__ X, double* __restrict__ D, double* __restrict__ vS)
{
    const int i = blockIdx.x * kPwThreads + threadIdx.x;
    if (i >= N) return;
    double den, v;
    dfta_exchange_dev::pointwise_node(N, i, norb, U, occ, first, tab, coef, Y, X, &den, &v);
    D[i] = den;
    vS[i] = v;
}

__global__ __launch_bounds__(kPwThreads) void k_exchange_kli(int N, int norb, int homo, const double* __restrict__ U, const double* __restrict__ occ,
                                                             const double* __restrict__ c, const double* __restrict__ D,
                                                             const double* __restrict__ vS, double* __restrict__ vKLI)
{
    const int i = blockIdx.x * kPwThreads + threadIdx.x;
    if (i >= N) return;
    vKLI[i] = dfta_exchange_dev::kli_node(N, i, norb, homo, U, occ, c, D[i], vS[i]);
}

// one quadrature per workgroup: red rows kind, a, b
__global__ __launch_bounds__(kRedThreads) void k_exchange_reduce(int N, double hstep, const double* __restrict__ cnst, const double* __restrict__ U,
                                                                 const double* __restrict__ X, const double* __restrict__ D,
                                                                 const double* __restrict__ vS, const double* __restrict__ vKLI,
                                                                 const int* __restrict__ red, double* __restrict__ out)
{
    __shared__ double part[kRedThreads / 64];
    const int kind = red[dfta_exchange::kRedInts * blockIdx.x], a = red[dfta_exchange::kRedInts * blockIdx.x + 1],
              b = red[dfta_exchange::kRedInts * blockIdx.x + 2];
    const double q = dfta_exchange_dev::reduce_block(N, hstep, cnst, U + (size_t)a * N, U + (size_t)b * N, X + (size_t)a * N, D,
                                                     kind == dfta_exchange::kRedKLI ? vKLI : vS, kind, part);
    if (threadIdx.x == 0) out[blockIdx.x] = q;
}

}  // namespace

int dfta_launch_screening_yk(dfta_ctx* ctx, const dfta_grid* g, const double* dU, int njobs, const int* dJobs, double* dY)
{
    if (njobs <= 0) return DFTA_OK;
    hipLaunchKernelGGL(k_screening_yk, dim3(njobs), dim3(kYkThreads), 0, ctx->stream, g->N, dfta_hstep(g), g->d_r.p, g->d_cnst.p, dU,
                       dJobs, dY);
    DFTA_CHECK_LAUNCH(ctx);
    return DFTA_OK;
}

int dfta_exchange_scratch::upload_jobs(dfta_ctx* ctx, const dfta_grid* g, int njobs, const int* jobs)
{
    DFTA_HIP(ctx, d_jobs.reserve((size_t)njobs * dfta_exchange::kJobInts));   // first use, a longer table than any before (or a larger grid)
    DFTA_HIP(ctx, d_y.reserve((size_t)njobs * g->N));
    DFTA_HIP(ctx, hipMemcpyAsync(d_jobs.p, jobs, sizeof(int) * dfta_exchange::kJobInts * njobs, hipMemcpyHostToDevice, ctx->stream));
    return DFTA_OK;
}

int dfta_exchange_scratch::run_yk(dfta_ctx* ctx, const dfta_grid* g, const double* dU, int njobs, const int* jobs, double* y)
{
    if (njobs <= 0) return DFTA_OK;
    hipStream_t st = ctx->stream;
    int rc = upload_jobs(ctx, g, njobs, jobs);
    if (rc) return rc;
    DFTA_HIP(ctx, dfta_timer_start(ctx));
    rc = dfta_launch_screening_yk(ctx, g, dU, njobs, d_jobs.p, d_y.p);
    if (rc) return rc;
    DFTA_HIP(ctx, dfta_timer_stop(ctx));
    DFTA_HIP(ctx, hipMemcpyAsync(y, d_y.p, sizeof(double) * njobs * (size_t)g->N, hipMemcpyDeviceToHost, st));
    DFTA_HIP(ctx, hipStreamSynchronize(st));
    return DFTA_OK;
}

int dfta_exchange_scratch::run_potentials(dfta_ctx* ctx, const dfta_grid* g, const double* dU, const dfta_exchange::ChannelPlan& plan,
                                          const double* occ, int homo, double* X, double* D, double* vS, double* vKLI, double* vbar, double* M)
{
    using namespace dfta_exchange;
    hipStream_t st = ctx->stream;
    const int norb = plan.norb, N = g->N, ntab = (int)plan.coef.size(), nred1 = plan.nred1(), nred2 = plan.nred2();
    const double hstep = dfta_hstep(g);
    int rc = upload_jobs(ctx, g, plan.njobs(), plan.jobs.data());
    if (rc) return rc;
    DFTA_HIP(ctx, d_X.reserve((size_t)norb * N));    // the channel's own rows and tables
    DFTA_HIP(ctx, d_rows.reserve((size_t)3 * N));    // D, vS, vKLI
    DFTA_HIP(ctx, d_occ.reserve(2 * (size_t)norb));  // occ, then c
    DFTA_HIP(ctx, d_first.reserve((size_t)norb + 1));
    DFTA_HIP(ctx, d_red.reserve((size_t)kRedInts * (norb * (norb + 1) / 2 + 3 * norb)));
    DFTA_HIP(ctx, d_redout.reserve((size_t)norb * (norb + 1) / 2 + 3 * norb));
    DFTA_HIP(ctx, d_tab.reserve((size_t)kTabInts * ntab));
    DFTA_HIP(ctx, d_coef.reserve(ntab));
    double* dD = d_rows.p;
    double* dvS = d_rows.p + N;
    double* dvK = d_rows.p + 2 * (size_t)N;
    double* dC = d_occ.p + norb;
    int* dRed2 = d_red.p + (size_t)kRedInts * nred1;
    double* dOut2 = d_redout.p + nred1;
    DFTA_HIP(ctx, hipMemcpyAsync(d_occ.p, occ, sizeof(double) * norb, hipMemcpyHostToDevice, st));
    DFTA_HIP(ctx, hipMemcpyAsync(d_first.p, plan.first.data(), sizeof(int) * (norb + 1), hipMemcpyHostToDevice, st));
    DFTA_HIP(ctx, hipMemcpyAsync(d_tab.p, plan.tab.data(), sizeof(int) * kTabInts * ntab, hipMemcpyHostToDevice, st));
    DFTA_HIP(ctx, hipMemcpyAsync(d_coef.p, plan.coef.data(), sizeof(double) * ntab, hipMemcpyHostToDevice, st));
    DFTA_HIP(ctx, hipMemcpyAsync(d_red.p, plan.red1.data(), sizeof(int) * kRedInts * nred1, hipMemcpyHostToDevice, st));
    DFTA_HIP(ctx, hipMemcpyAsync(dRed2, plan.red2.data(), sizeof(int) * kRedInts * nred2, hipMemcpyHostToDevice, st));
    const int nblk = (N + kPwThreads - 1) / kPwThreads;
    DFTA_HIP(ctx, dfta_timer_start(ctx));
    rc = dfta_launch_screening_yk(ctx, g, dU, plan.njobs(), d_jobs.p, d_y.p);
    if (rc) return rc;
    hipLaunchKernelGGL(k_exchange_pointwise, dim3(nblk), dim3(kPwThreads), 0, st, N, norb, dU, d_occ.p, d_first.p, d_tab.p, d_coef.p, d_y.p, d_X.p,
                       dD, dvS);
    DFTA_CHECK_LAUNCH(ctx);
    hipLaunchKernelGGL(k_exchange_reduce, dim3(nred1), dim3(kRedThreads), 0, st, N, hstep, g->d_cnst.p, dU, d_X.p, dD, dvS, dvK, d_red.p, d_redout.p);
    DFTA_CHECK_LAUNCH(ctx);
    std::vector<double> h1(nred1), h2(nred2), hM((size_t)norb * norb), c(norb);
    DFTA_HIP(ctx, hipMemcpyAsync(h1.data(), d_redout.p, sizeof(double) * nred1, hipMemcpyDeviceToHost, st));
    DFTA_HIP(ctx, hipStreamSynchronize(st));
    const double* vHF = h1.data();
    const double* vSb = h1.data() + norb;
    int p = 2 * norb;
    for (int a = 0; a < norb; ++a)
        for (int b = a; b < norb; ++b, ++p) {        // S_ab once, mirrored; M_ab = S_ab n_b
            hM[(size_t)a * norb + b] = h1[p] * occ[b];
            hM[(size_t)b * norb + a] = h1[p] * occ[a];
        }
    DFTA_REQUIRE(ctx, solve_kli(norb, homo, hM.data(), vSb, vHF, c.data()) == 0, "exchange potentials: the KLI system is singular");
    DFTA_HIP(ctx, hipMemcpyAsync(dC, c.data(), sizeof(double) * norb, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_exchange_kli, dim3(nblk), dim3(kPwThreads), 0, st, N, norb, homo, dU, d_occ.p, dC, dD, dvS, dvK);
    DFTA_CHECK_LAUNCH(ctx);
    hipLaunchKernelGGL(k_exchange_reduce, dim3(nred2), dim3(kRedThreads), 0, st, N, hstep, g->d_cnst.p, dU, d_X.p, dD, dvS, dvK, dRed2, dOut2);
    DFTA_CHECK_LAUNCH(ctx);
    DFTA_HIP(ctx, dfta_timer_stop(ctx));
    DFTA_HIP(ctx, hipMemcpyAsync(h2.data(), dOut2, sizeof(double) * nred2, hipMemcpyDeviceToHost, st));
    if (X) DFTA_HIP(ctx, hipMemcpyAsync(X, d_X.p, sizeof(double) * norb * (size_t)N, hipMemcpyDeviceToHost, st));
    if (D) DFTA_HIP(ctx, hipMemcpyAsync(D, dD, sizeof(double) * N, hipMemcpyDeviceToHost, st));
    if (vS) DFTA_HIP(ctx, hipMemcpyAsync(vS, dvS, sizeof(double) * N, hipMemcpyDeviceToHost, st));
    if (vKLI) DFTA_HIP(ctx, hipMemcpyAsync(vKLI, dvK, sizeof(double) * N, hipMemcpyDeviceToHost, st));
    DFTA_HIP(ctx, hipStreamSynchronize(st));
    if (vbar)
        for (int a = 0; a < norb; ++a) {
            double* row = vbar + (size_t)DFTA_XP_COLS * a;
            row[DFTA_XP_HF] = vHF[a]; row[DFTA_XP_S] = vSb[a]; row[DFTA_XP_C] = c[a]; row[DFTA_XP_KLI] = h2[a];
        }
    if (M) std::copy(hM.begin(), hM.end(), M);
    return DFTA_OK;
}

// ---- the launches on caller-supplied orbitals (host pointers) ------------------------------------------------------------------------
extern "C" {

int dfta_screening_yk(dfta_ctx* ctx, const dfta_grid* g, int norb, const double* u, int njobs, const int* jobs, double* y)
{
    if (!ctx || !g) return DFTA_ERR_INVALID;
    DFTA_ENTER(ctx);
    DFTA_REQUIRE(ctx, norb >= 0 && njobs >= 0, "dfta_screening_yk: norb, njobs");
    if (njobs == 0) return DFTA_OK;
    DFTA_REQUIRE(ctx, u && jobs && y, "dfta_screening_yk arguments");
    DFTA_REQUIRE(ctx, g->N >= 5, "dfta_screening_yk: the grid needs 5 nodes");
    if (const char* msg = dfta_exchange::check_jobs(norb, njobs, jobs)) DFTA_REQUIRE(ctx, false, msg);
    DevBuf<double> dU;
    dfta_exchange_scratch sc;
    if (const int rc = dfta_upload_rows(ctx, u, (size_t)norb * g->N, &dU)) return rc;
    return sc.run_yk(ctx, g, dU.p, njobs, jobs, y);
}

int dfta_exchange_potentials(dfta_ctx* ctx, const dfta_grid* g, int norb, const int* l, const double* occ, int homo, const double* u,
                             double* X, double* D, double* vS, double* vKLI, double* vbar, double* M)
{
    if (!ctx || !g) return DFTA_ERR_INVALID;
    DFTA_ENTER(ctx);
    DFTA_REQUIRE(ctx, l && occ && u, "dfta_exchange_potentials arguments");
    DFTA_REQUIRE(ctx, g->N >= 5, "dfta_exchange_potentials: the grid needs 5 nodes");
    if (const char* msg = dfta_exchange::check_channel(norb, l, occ, homo)) DFTA_REQUIRE(ctx, false, msg);
    dfta_exchange::ChannelPlan plan;
    DFTA_REQUIRE(ctx, dfta_exchange::plan_channel(norb, l, occ, &plan) == 0, "dfta_exchange_potentials: the channel");
    DevBuf<double> dU;
    dfta_exchange_scratch sc;
    if (const int rc = dfta_upload_rows(ctx, u, (size_t)norb * g->N, &dU)) return rc;
    return sc.run_potentials(ctx, g, dU.p, plan, occ, homo, X, D, vS, vKLI, vbar, M);
}

}  // extern "C"
