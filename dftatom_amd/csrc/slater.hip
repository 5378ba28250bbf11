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
#include "slater_plan.h"

namespace {

constexpr int kSlThreads = 256;
constexpr int kSlPer = 4;                            // consecutive nodes per lane
constexpr int kSlTile = kSlThreads * kSlPer;         // nodes per tile
constexpr int kSlBefore = 3;                         // nodes kept in front of a tile: the stencil of node N-1 reaches node N-4
constexpr int kSlSlots = kSlTile + kSlBefore + 1;    // slot q of the running tile [t0, t0 + kSlTile) holds node t0 - kSlBefore + q
constexpr int kSlArrays = 6;
enum { kGX, kGY, kPX, kPY, kInv, kSc };

// Simpson 3/8 weight of node i without the factor 3/8 (Integral.h:50-73)
__device__ __forceinline__ double simpson38_weight(int i, int N) { return (i == 0 || i == N - 1) ? 1. : (i % 3 == 0 ? 2. : 3.); }

// the increment d_i of Z at node i, 1 <= i <= N-1, from the slots around q (the header states these orders)
__device__ __forceinline__ double increment(const double* g, int q, int i, int N)
{
    if (i == 1) return (((9. * g[q - 1] + 19. * g[q]) - 5. * g[q + 1]) + g[q + 2]) / 24.;
    if (i == N - 1) return (((g[q - 3] - 5. * g[q - 2]) + 19. * g[q - 1]) + 9. * g[q]) / 24.;
    return (13. * (g[q - 1] + g[q]) - (g[q - 2] + g[q + 1])) / 24.;
}

// inclusive scan of v over the 64 lanes of a wave: six levels, lane t takes lane t - off
__device__ __forceinline__ double wave_scan(double v, int lane)
{
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const double o = __shfl_up(v, off);
        if (lane >= off) v += o;
    }
    return v;
}

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
        const double ri = r[i], sc = cnst[i] * hstep;
        double p = 1.;
        for (int m = 0; m < k; ++m) p = p * ri;      // r^k: k multiplications from 1
        v[kGX] = (p * px) * sc;
        v[kGY] = (p * py) * sc;
        v[kPX] = px;
        v[kPY] = py;
        v[kInv] = i > 0 ? 1. / (p * ri) : 0.;        // r_0 = 0: the outer term is 0 there
        v[kSc] = sc;
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
        // the lane's chain of increments, both streams
        double lx[kSlPer], ly[kSlPer];
        double tx = 0., ty = 0.;
#pragma unroll
        for (int j = 0; j < kSlPer; ++j) {
            const int i = i0 + j;
            const bool in = i >= 1 && i < N;
            const double dx = in ? increment(s[kGX], q0 + j, i, N) : 0.;
            const double dy = (in && !same) ? increment(s[kGY], q0 + j, i, N) : 0.;
            tx = j == 0 ? dx : tx + dx;
            ty = j == 0 ? dy : ty + dy;
            lx[j] = tx;
            ly[j] = ty;
        }
        // the lanes' totals across the wave, the waves' totals through LDS
        const double ix = wave_scan(tx, lane), iy = wave_scan(ty, lane);
        double ex = __shfl_up(ix, 1), ey = __shfl_up(iy, 1);
        if (lane == 0) ex = ey = 0.;
        if (lane == 63) { wtot[0][wave] = ix; wtot[1][wave] = iy; }      // read before the next tile's: two barriers lie between
        __syncthreads();
        const double* wx = wtot[0];
        const double* wy = wtot[1];
        const double offx = wave == 0 ? 0. : (wave == 1 ? wx[0] : (wave == 2 ? wx[0] + wx[1] : (wx[0] + wx[1]) + wx[2]));
        const double offy = wave == 0 ? 0. : (wave == 1 ? wy[0] : (wave == 2 ? wy[0] + wy[1] : (wy[0] + wy[1]) + wy[2]));
        const double totx = ((wx[0] + wx[1]) + wx[2]) + wx[3], toty = ((wy[0] + wy[1]) + wy[2]) + wy[3];
        const double bx = offx + ex, by = offy + ey;
#pragma unroll
        for (int j = 0; j < kSlPer; ++j) {
            const int i = i0 + j, q = q0 + j;
            if (i < 1 || i >= N) continue;
            const double zx = carryX + (bx + lx[j]);
            const double zy = same ? zx : carryY + (by + ly[j]);
            const double S = s[kPX][q] * zy + s[kPY][q] * zx;
            acc += simpson38_weight(i, N) * ((S * s[kInv][q]) * s[kSc][q]);
        }
        carryX = carryX + totx;
        carryY = carryY + toty;
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
    // the tree: lanes of a wave by xor shuffles 32 .. 1, then the four waves as (w0 + w1) + (w2 + w3)
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off);
    if (lane == 0) red[wave] = acc;
    __syncthreads();
    if (tid == 0) {
        const double sum = (red[0] + red[1]) + (red[2] + red[3]);
        constexpr double coef = 3. / 8.;
        R[blockIdx.x] = sum * coef;
    }
}

}  // namespace

int dfta_launch_slater_rk(dfta_ctx* ctx, const dfta_grid* g, const double* dU, int njobs, const int* dJobs, double* dR)
{
    if (njobs <= 0) return DFTA_OK;
    hipStream_t st = ctx->stream;
    DFTA_HIP(ctx, hipEventRecord(ctx->ev[0], st));
    hipLaunchKernelGGL(k_slater_rk, dim3(njobs), dim3(kSlThreads), 0, st, g->N, g->uniform ? g->h : 1.0, g->d_r.p, g->d_cnst.p, dU, dJobs, dR);
    DFTA_CHECK_LAUNCH(ctx);
    DFTA_HIP(ctx, hipEventRecord(ctx->ev[1], st));
    ctx->have_kernel_time = true;
    return DFTA_OK;
}

int dfta_slater_scratch::run(dfta_ctx* ctx, const dfta_grid* g, const double* dU, int njobs, const int* jobs, double* R)
{
    if (njobs <= 0) return DFTA_OK;
    hipStream_t st = ctx->stream;
    if (cap < njobs) {                               // first use, or a longer table than any before
        cap = 0;
        DFTA_HIP(ctx, d_jobs.alloc((size_t)njobs * dfta_slater::kJobInts));
        DFTA_HIP(ctx, d_R.alloc(njobs));
        cap = njobs;
    }
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
    const size_t sz = (size_t)norb * g->N;
    DevBuf<double> dU;
    dfta_slater_scratch sc;
    DFTA_HIP(ctx, dU.alloc(sz));
    DFTA_HIP(ctx, hipMemcpyAsync(dU.p, u, sizeof(double) * sz, hipMemcpyHostToDevice, ctx->stream));
    return sc.run(ctx, g, dU.p, njobs, jobs, R);
}

}  // extern "C"
