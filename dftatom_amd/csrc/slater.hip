// slater.hip -- Slater integrals R^k(ab,cd) of radial orbitals u_i = r_i R_nl(r_i) (include/dftatom_hip.h has the definitions; DESIGN.md
// 4.9 the scan's shape and its rounding bound).  Beyond the reference.
//
//   R^k(ab,cd) = Q[ (P_X Z_Y + P_Y Z_X) (1 / (r^k r)) s ],  P_X = u_a u_c,  P_Y = u_b u_d,  Z_i = Sum_{j <= i} d_j(g),  g = (r^k P) s
//
// -- the double integral with its two regions r' < r and r' > r swapped into one form that needs forward cumulative integrals only.
//   k_slater_rk   one workgroup of 256 lanes per job (a, b, c, d, k), every job of a call in one launch, no communication between
//                 workgroups.  The job's distinct orbitals pass through LDS once, in tiles of kSlTile nodes: g_X, g_Y, P_X, P_Y, 1/(r^k r)
//                 and s are formed at the node when it is staged; three nodes before the tile and one after it (the increment
//                 stencils' reach) are carried over inside LDS, so every node is read from HBM exactly once.  Lane t owns the nodes
//                 tile * kSlTile + 4 t .. + 3: its four increments of both streams are chained, the lanes' totals scanned across the
//                 wave by shuffles (six levels), the four waves' totals chained through LDS, the carry of the earlier tiles added last.
//                 The lane adds its weighted outer terms to one accumulator; the end is k_orbital_properties' tree.
// The shape is a function of N alone: a job's bits depend on its orbitals, k and N, not on the launch it sits in.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "internal.h"
#include "radial_device.h"
#include "slater_plan.h"

namespace {

constexpr int kSlThreads = 256;
constexpr int kSlPer = 4;                            // consecutive nodes per lane
constexpr int kSlTile = kSlThreads * kSlPer;         // nodes per tile
constexpr int kSlBefore = 3;                         // nodes kept in front of a tile: the stencil of node N-1 reaches node N-4
constexpr int kSlSlots = kSlTile + kSlBefore + 1;    // slot q of the running tile [t0, t0 + kSlTile) holds node t0 - kSlBefore + q
constexpr int kSlArrays = 6;
enum { kGX, kGY, kPX, kPY, kInv, kSc };
using namespace dfta_radial;

__global__ __launch_bounds__(kSlThreads) void k_slater_rk(int N, double hstep, const double* __restrict__ r, const double* __restrict__ cnst,
                                                          const double* __restrict__ U, const int* __restrict__ jobs,
                                                          double* __restrict__ R)
{
    __shared__ double s[kSlArrays][kSlSlots];
    __shared__ double wtot[2][kSlThreads / 64];
    __shared__ double red[kSlThreads / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int* __restrict__ job = jobs + (size_t)dfta_slater::kJobInts * blockIdx.x;
    const int ja = job[0], jb = job[1], jc = job[2], jd = job[3], k = job[4];
    // the two products, each from its lower-indexed orbital first, the pair of lower (min, max) index as X
    int x0 = min(ja, jc), x1 = max(ja, jc), y0 = min(jb, jd), y1 = max(jb, jd);
    if (y0 < x0 || (y0 == x0 && y1 < x1)) { int t = x0; x0 = y0; y0 = t; t = x1; x1 = y1; y1 = t; }
    const bool same = x0 == y0 && x1 == y1;          // one product: G^k(a,b), F^k(a,a)
    const double* __restrict__ ux0 = U + (size_t)x0 * N;
    const double* __restrict__ ux1 = U + (size_t)x1 * N;
    const double* __restrict__ uy0 = U + (size_t)y0 * N;
    const double* __restrict__ uy1 = U + (size_t)y1 * N;

    // the six values of node i (zeros beyond the grid); every distinct orbital is read once
    auto stage = [&](int i, double* v) {
        if (i >= N) {
#pragma unroll
            for (int m = 0; m < kSlArrays; ++m) v[m] = 0.;
            return;
        }
        const double a0 = ux0[i];
        const double a1 = x1 == x0 ? a0 : ux1[i];
        const double px = a0 * a1;
        double py = px;
        if (!same) {
            const double b0 = y0 == x0 ? a0 : (y0 == x1 ? a1 : uy0[i]);
            const double b1 = y1 == y0 ? b0 : (y1 == x0 ? a0 : (y1 == x1 ? a1 : uy1[i]));
            py = b0 * b1;
        }
        const NodeFactors f = node_factors(k, r[i], cnst[i], hstep, i);
        v[kGX] = (f.p * px) * f.sc;
        v[kGY] = (f.p * py) * f.sc;
        v[kPX] = px;
        v[kPY] = py;
        v[kInv] = f.inv;
        v[kSc] = f.sc;
    };

    if (tid < kSlBefore)
        for (int m = 0; m < kSlArrays; ++m) s[m][tid] = 0.;          // nodes -3 .. -1: never used by a stencil
    for (int q = tid; q < kSlTile + 1; q += kSlThreads) {            // nodes 0 .. kSlTile
        double v[kSlArrays];
        stage(q, v);
#pragma unroll
        for (int m = 0; m < kSlArrays; ++m) s[m][kSlBefore + q] = v[m];
    }
    __syncthreads();

    double carryX = 0., carryY = 0., acc = 0.;
    for (int t0 = 0; t0 < N; t0 += kSlTile) {
        const int q0 = kSlBefore + kSlPer * tid, i0 = t0 + kSlPer * tid;
        // the scan of the tile (radial_device.h), both streams through one barrier
        double lx[kSlPer], ly[kSlPer];
        const double tx = chain_up(s[kGX], q0, i0, N, true, lx), ty = chain_up(s[kGY], q0, i0, N, !same, ly);
        const LanePrefix px = wave_prefix_up(tx, lane), py = wave_prefix_up(ty, lane);
        if (lane == 63) { wtot[0][wave] = px.inc; wtot[1][wave] = py.inc; }      // read before the next tile's: two barriers lie between
        __syncthreads();
        const TileSums wx = waves_chain_up(wtot[0], wave), wy = waves_chain_up(wtot[1], wave);
        const double bx = wx.off + px.ex, by = wy.off + py.ex;
#pragma unroll
        for (int j = 0; j < kSlPer; ++j) {
            const int i = i0 + j, q = q0 + j;
            if (i < 1 || i >= N) continue;
            const double zx = carryX + (bx + lx[j]);
            const double zy = same ? zx : carryY + (by + ly[j]);
            const double S = s[kPX][q] * zy + s[kPY][q] * zx;
            acc += simpson38_weight(i, N) * ((S * s[kInv][q]) * s[kSc][q]);
        }
        carryX = carryX + wx.tot;
        carryY = carryY + wy.tot;
        const int t1 = t0 + kSlTile;
        if (t1 < N) {
            double keep[kSlArrays];
            if (tid < kSlBefore + 1)                 // nodes t1 - 3 .. t1: the next tile's first four slots
                for (int m = 0; m < kSlArrays; ++m) keep[m] = s[m][kSlTile + tid];
            double nxt[kSlPer][kSlArrays];
#pragma unroll
            for (int j = 0; j < kSlPer; ++j) stage(t1 + 1 + tid + j * kSlThreads, nxt[j]);   // nodes t1 + 1 .. t1 + kSlTile
            __syncthreads();
            if (tid < kSlBefore + 1)
                for (int m = 0; m < kSlArrays; ++m) s[m][tid] = keep[m];
#pragma unroll
            for (int j = 0; j < kSlPer; ++j)
#pragma unroll
                for (int m = 0; m < kSlArrays; ++m) s[m][kSlBefore + 1 + tid + j * kSlThreads] = nxt[j][m];
            __syncthreads();
        }
    }
    acc = wave_tree_sum(acc);                        // the tree of radial_device.h
    if (lane == 0) red[wave] = acc;
    __syncthreads();
    if (tid == 0) R[blockIdx.x] = simpson38_finish(waves_join(red[0], red[1], red[2], red[3]));
}

}  // namespace

int dfta_launch_slater_rk(dfta_ctx* ctx, const dfta_grid* g, const double* dU, int njobs, const int* dJobs, double* dR)
{
    if (njobs <= 0) return DFTA_OK;
    DFTA_HIP(ctx, dfta_timer_start(ctx));
    hipLaunchKernelGGL(k_slater_rk, dim3(njobs), dim3(kSlThreads), 0, ctx->stream, g->N, dfta_hstep(g), g->d_r.p, g->d_cnst.p, dU, dJobs, dR);
    DFTA_CHECK_LAUNCH(ctx);
    DFTA_HIP(ctx, dfta_timer_stop(ctx));
    return DFTA_OK;
}

int dfta_slater_scratch::run(dfta_ctx* ctx, const dfta_grid* g, const double* dU, int njobs, const int* jobs, double* R)
{
    if (njobs <= 0) return DFTA_OK;
    hipStream_t st = ctx->stream;
    DFTA_HIP(ctx, d_jobs.reserve((size_t)njobs * dfta_slater::kJobInts));     // first use, or a longer table than any before
    DFTA_HIP(ctx, d_R.reserve(njobs));
    DFTA_HIP(ctx, hipMemcpyAsync(d_jobs.p, jobs, sizeof(int) * dfta_slater::kJobInts * njobs, hipMemcpyHostToDevice, st));
    const int rc = dfta_launch_slater_rk(ctx, g, dU, njobs, d_jobs.p, d_R.p);
    if (rc) return rc;
    DFTA_HIP(ctx, hipMemcpyAsync(R, d_R.p, sizeof(double) * njobs, hipMemcpyDeviceToHost, st));
    DFTA_HIP(ctx, hipStreamSynchronize(st));
    return DFTA_OK;
}

// ---- the launch on caller-supplied orbitals (host pointers) --------------------------------------------------------------------------
extern "C" {

int dfta_slater_rk(dfta_ctx* ctx, const dfta_grid* g, int norb, const double* u, int njobs, const int* jobs, double* R)
{
    if (!ctx || !g) return DFTA_ERR_INVALID;
    DFTA_ENTER(ctx);
    DFTA_REQUIRE(ctx, norb >= 0 && njobs >= 0, "dfta_slater_rk: norb, njobs");
    if (njobs == 0) return DFTA_OK;
    DFTA_REQUIRE(ctx, u && jobs && R, "dfta_slater_rk arguments");
    DFTA_REQUIRE(ctx, g->N >= 5, "dfta_slater_rk: the grid needs 5 nodes");
    if (const char* msg = dfta_slater::check_jobs(norb, njobs, jobs)) DFTA_REQUIRE(ctx, false, msg);
    DevBuf<double> dU;
    dfta_slater_scratch sc;
    if (const int rc = dfta_upload_rows(ctx, u, (size_t)norb * g->N, &dU)) return rc;
    return sc.run(ctx, g, dU.p, njobs, jobs, R);
}

}  // extern "C"
