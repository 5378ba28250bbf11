// orbitals.hip -- expectation values and r^k matrix elements of radial orbitals u_i = r_i R_nl(r_i) (include/dftatom_hip.h has the
// definitions; DESIGN.md 4.8 the summation shape and its rounding bound).  Beyond the reference, which prints eigenvalues only.
//
// Both kernels take Simpson's 3/8 weights as Integral::Simpson38 applies them (Integral.h:50-73) -- 1 at the two end nodes, 2 at the
// inner nodes i % 3 == 0, 3 elsewhere, times 3/8 -- whatever rule the SCF integrates with, and s_i = dr/di (cnst[i] on the logarithmic
// grid, h on the uniform one).  Each weighted term is formed at its node and the terms are added in a FIXED-SHAPE TREE that depends on
// N alone: no floating-point atomics, and an orbital's bits depend neither on the batch it sits in nor on the run.
//   k_orbital_properties  one workgroup per orbital, every orbital of the batch in one launch.  The orbital passes through LDS once, in
//                         tiles of kPropTile nodes with a 2-node halo for the derivative stencil (the halo of the next tile is carried
//                         over inside LDS: every node is read from HBM exactly once).  Lane t of 256 adds the terms of the nodes
//                         tile * kPropTile + t + 256 q, q = 0 .. 3, tile after tile; then xor shuffles 32 .. 1 and (w0 + w1) + (w2 + w3).
//   k_orbital_matrix      one workgroup per chunk of kMatChunk nodes; tiles of kMatTile nodes of ALL orbitals staged in LDS once and
//                         shared by every pair a <= b; a lane owns whole pairs and adds its pair's terms node after node.  The chunks'
//                         partial sums go to a slab; the workgroup that finishes last (an integer ticket) adds them in chunk order
//                         and writes M[a][b] and M[b][a] from the one value.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "internal.h"
#include "radial_device.h"

namespace {

constexpr int kPropThreads = 256;
constexpr int kPropTile = 1024;                      // nodes per tile: 4 per lane
constexpr int kPropPer = kPropTile / kPropThreads;
constexpr int kProps = DFTA_ORB_PROPS;

constexpr int kMatThreads = 256;
constexpr int kMatTile = 128;                        // nodes of every orbital in LDS at a time: 32 orbitals x 128 nodes = 32 KB
constexpr int kMatChunk = 512;                       // nodes per workgroup: the chunking is a function of N alone

using namespace dfta_radial;

__global__ __launch_bounds__(kPropThreads) void k_orbital_properties(int N, double hstep, const double* __restrict__ r,
                                                                     const double* __restrict__ cnst, const int* __restrict__ l,
                                                                     const double* __restrict__ U, double* __restrict__ props)
{
    // s[k] holds node t0 - 2 + k of the running tile [t0, t0 + kPropTile)
    __shared__ double s[kPropTile + 4];
    __shared__ double red[kPropThreads / 64][kProps];
    __shared__ int redi[kPropThreads / 64];
    const int orb = blockIdx.x, tid = threadIdx.x;
    const double* __restrict__ u = U + (size_t)orb * N;
    const int lq = l[orb];
    const double ll1 = (double)lq * (double)(lq + 1);
    double acc[7] = {0., 0., 0., 0., 0., 0., 0.};    // NORM, <1/r>, <r>, <r^2>, <r^4>, 2 T, <1/r^3>
    double best = -1.;
    int besti = 0;
    if (tid < 2) s[tid] = 0.;                        // nodes -2, -1: never used by a stencil
    for (int k = tid; k < kPropTile + 2; k += kPropThreads) s[2 + k] = k < N ? u[k] : 0.;     // nodes 0 .. kPropTile + 1
    __syncthreads();
    for (int t0 = 0; t0 < N; t0 += kPropTile) {
#pragma unroll
        for (int q = 0; q < kPropPer; ++q) {
            const int k = 2 + tid + q * kPropThreads, i = t0 - 2 + k;
            if (i >= N) continue;
            const double ui = s[k];
            double du;
            if (i == 0) du = ((4. * s[k + 1] - 3. * ui) - s[k + 2]) * 0.5;
            else if (i == N - 1) du = ((3. * ui - 4. * s[k - 1]) + s[k - 2]) * 0.5;
            else if (i == 1 || i == N - 2) du = (s[k + 1] - s[k - 1]) * 0.5;
            else du = (8. * (s[k + 1] - s[k - 1]) - (s[k + 2] - s[k - 2])) / 12.;
            const double ri = r[i], sc = cnst[i] * hstep, w = simpson38_weight(i, N);
            const double uu = ui * ui, g = uu * sc, r2 = ri * ri;
            const bool in = i > 0;                   // r_0 = 0: the negative powers contribute 0 there
            acc[0] += w * g;
            acc[1] += w * (in ? g / ri : 0.);
            acc[2] += w * (g * ri);
            acc[3] += w * (g * r2);
            acc[4] += w * (g * (r2 * r2));
            acc[5] += w * (du * du / sc + (in ? ll1 * uu / r2 * sc : 0.));
            acc[6] += w * ((in && lq >= 1) ? g / (r2 * ri) : 0.);
            const double au = fabs(ui);
            if (au > best) { best = au; besti = i; }     // a lane's nodes come in increasing order: the lowest index stays on ties
        }
        const int t1 = t0 + kPropTile;
        if (t1 < N) {
            double keep = 0.;
            if (tid < 4) keep = s[kPropTile + tid];  // nodes t1 - 2 .. t1 + 1: the next tile's first four entries
            double nxt[kPropPer];
#pragma unroll
            for (int q = 0; q < kPropPer; ++q) {     // nodes t1 + 2 .. t1 + kPropTile + 1
                const int i = t1 + 2 + tid + q * kPropThreads;
                nxt[q] = i < N ? u[i] : 0.;
            }
            __syncthreads();
            if (tid < 4) s[tid] = keep;
#pragma unroll
            for (int q = 0; q < kPropPer; ++q) s[4 + tid + q * kPropThreads] = nxt[q];
            __syncthreads();
        }
    }
    // the tree of radial_device.h, per quantity
#pragma unroll
    for (int c = 0; c < 7; ++c) {
        const double v = wave_tree_sum(acc[c]);
        if ((tid & 63) == 0) red[tid >> 6][c] = v;
    }
    for (int off = 32; off > 0; off >>= 1) {
        const double ob = __shfl_xor(best, off);
        const int oi = __shfl_xor(besti, off);
        if (ob > best || (ob == best && oi < besti)) { best = ob; besti = oi; }
    }
    if ((tid & 63) == 0) { red[tid >> 6][7] = best; redi[tid >> 6] = besti; }
    __syncthreads();
    double* __restrict__ out = props + (size_t)orb * kProps;
    if (tid < 7) {
        const double q = simpson38_finish(waves_join(red[0][tid], red[1][tid], red[2][tid], red[3][tid]));
        out[tid == 5 ? DFTA_ORB_T : (tid == 6 ? DFTA_ORB_RM3 : tid)] = tid == 5 ? 0.5 * q : q;
    } else if (tid == 7) {
        double b = red[0][7];
        int bi = redi[0];
        for (int wv = 1; wv < kPropThreads / 64; ++wv)
            if (red[wv][7] > b || (red[wv][7] == b && redi[wv] < bi)) { b = red[wv][7]; bi = redi[wv]; }
        out[DFTA_ORB_RPEAK] = r[bi];
    }
}

template <int K>
__global__ __launch_bounds__(kMatThreads) void k_orbital_matrix(int N, int norb, double hstep, const double* __restrict__ r,
                                                                const double* __restrict__ cnst, const double* __restrict__ U,
                                                                double* __restrict__ slab, unsigned* __restrict__ ticket,
                                                                double* __restrict__ M)
{
    extern __shared__ double lds[];                  // [kMatTile][norb] orbital values, node-major; then kMatTile weights
    __shared__ int s_last;
    double* __restrict__ su = lds;
    double* __restrict__ sw = lds + (size_t)kMatTile * norb;
    const int tid = threadIdx.x, chunk = blockIdx.x, nchunks = gridDim.x;
    const int npair = norb * (norb + 1) / 2;
    constexpr int kOwn = 3;                          // pairs per lane: 32 orbitals are 528 pairs <= 3 x 256
    int pa[kOwn], pb[kOwn];
    double acc[kOwn];
#pragma unroll
    for (int q = 0; q < kOwn; ++q) {                 // pair p = tid + 256 q -> (a, b), a <= b, row by row of the upper triangle
        int p = tid + q * kMatThreads, a = 0;
        if (p >= npair) p = 0;
        while (p >= norb - a) { p -= norb - a; ++a; }
        pa[q] = a;
        pb[q] = a + p;
        acc[q] = 0.;
    }
    const int c0 = chunk * kMatChunk, c1 = min(N, c0 + kMatChunk);
    for (int t0 = c0; t0 < c1; t0 += kMatTile) {
        const int nt = min(kMatTile, c1 - t0);
        for (int e = tid; e < nt * norb; e += kMatThreads) {
            const int o = e / nt, k = e - o * nt;    // consecutive lanes read consecutive nodes of one orbital
            su[k * norb + o] = U[(size_t)o * N + t0 + k];
        }
        if (tid < nt) {
            const int i = t0 + tid;
            const double ri = r[i], sc = cnst[i] * hstep;
            const double f = K == 0 ? sc : (K == 1 ? sc * ri : sc * (ri * ri));
            sw[tid] = simpson38_weight(i, N) * f;
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < kOwn; ++q) {
            if (tid + q * kMatThreads >= npair) continue;
            double v = acc[q];
            for (int k = 0; k < nt; ++k) v += (su[k * norb + pa[q]] * su[k * norb + pb[q]]) * sw[k];
            acc[q] = v;
        }
        __syncthreads();
    }
#pragma unroll
    for (int q = 0; q < kOwn; ++q) {
        const int p = tid + q * kMatThreads;
        if (p < npair) slab[(size_t)chunk * npair + p] = acc[q];
    }
    // the workgroup that takes the last ticket adds the chunks' shares in chunk order (every share is visible device-wide by then)
    __threadfence();
    __syncthreads();
    if (tid == 0) s_last = atomicAdd(ticket, 1u) == (unsigned)(nchunks - 1);
    __syncthreads();
    if (!s_last) return;
    __threadfence();
    const volatile double* vs = slab;
#pragma unroll
    for (int q = 0; q < kOwn; ++q) {
        const int p = tid + q * kMatThreads;
        if (p >= npair) continue;
        double sum = 0.;
        for (int c = 0; c < nchunks; ++c) sum += vs[(size_t)c * npair + p];
        const double m = simpson38_finish(sum);
        M[(size_t)pa[q] * norb + pb[q]] = m;
        M[(size_t)pb[q] * norb + pa[q]] = m;
    }
    if (tid == 0) *ticket = 0u;                      // ready for the next launch on this stream
}

}  // namespace

int dfta_launch_orbital_properties(dfta_ctx* ctx, const dfta_grid* g, int norb, const int* dL, const double* dU, double* dProps)
{
    if (norb <= 0) return DFTA_OK;
    DFTA_HIP(ctx, dfta_timer_start(ctx));
    hipLaunchKernelGGL(k_orbital_properties, dim3(norb), dim3(kPropThreads), 0, ctx->stream, g->N, dfta_hstep(g), g->d_r.p, g->d_cnst.p, dL, dU,
                       dProps);
    DFTA_CHECK_LAUNCH(ctx);
    DFTA_HIP(ctx, dfta_timer_stop(ctx));
    return DFTA_OK;
}

int dfta_orbital_matrix_chunks(int N) { return (N + kMatChunk - 1) / kMatChunk; }

int dfta_launch_orbital_matrix(dfta_ctx* ctx, const dfta_grid* g, int norb, const double* dU, int k, double* dSlab, unsigned* dTicket, double* dM)
{
    if (norb <= 0) return DFTA_OK;
    const int N = g->N, nchunks = dfta_orbital_matrix_chunks(N);
    const size_t lds = sizeof(double) * ((size_t)kMatTile * norb + kMatTile);
    const double hstep = dfta_hstep(g);
    hipStream_t st = ctx->stream;
    if (k == 0) hipLaunchKernelGGL(k_orbital_matrix<0>, dim3(nchunks), dim3(kMatThreads), lds, st, N, norb, hstep, g->d_r.p, g->d_cnst.p, dU, dSlab, dTicket, dM);
    else if (k == 1) hipLaunchKernelGGL(k_orbital_matrix<1>, dim3(nchunks), dim3(kMatThreads), lds, st, N, norb, hstep, g->d_r.p, g->d_cnst.p, dU, dSlab, dTicket, dM);
    else hipLaunchKernelGGL(k_orbital_matrix<2>, dim3(nchunks), dim3(kMatThreads), lds, st, N, norb, hstep, g->d_r.p, g->d_cnst.p, dU, dSlab, dTicket, dM);
    DFTA_CHECK_LAUNCH(ctx);
    return DFTA_OK;
}

int dfta_orbital_scratch_create(dfta_ctx* ctx, const dfta_grid* g, int norb_max, dfta_orbital_scratch* sc)
{
    const size_t npair = (size_t)norb_max * (norb_max + 1) / 2;
    hipError_t e = sc->slab.alloc((size_t)dfta_orbital_matrix_chunks(g->N) * npair);
    if (e == hipSuccess) e = sc->M.alloc((size_t)norb_max * norb_max);
    if (e == hipSuccess) e = sc->ticket.alloc(1);
    if (e == hipSuccess) e = hipMemsetAsync(sc->ticket.p, 0, sizeof(unsigned), ctx->stream);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        sc->slab.reset(); sc->M.reset(); sc->ticket.reset();
        snprintf(ctx->err, sizeof(ctx->err), "orbital matrix scratch: %s", hipGetErrorString(e));
        return e == hipErrorOutOfMemory ? DFTA_ERR_NOMEM : DFTA_ERR_HIP;
    }
    sc->norb_max = norb_max;
    return DFTA_OK;
}

// ---- the two launches on caller-supplied orbitals (host pointers) ------------------------------------------------------------------
extern "C" {

int dfta_orbital_properties(dfta_ctx* ctx, const dfta_grid* g, int norb, const int* l, const double* u, double* props)
{
    if (!ctx || !g) return DFTA_ERR_INVALID;
    DFTA_ENTER(ctx);
    DFTA_REQUIRE(ctx, norb >= 0, "dfta_orbital_properties: norb");
    if (norb == 0) return DFTA_OK;
    DFTA_REQUIRE(ctx, l && u && props && g->N >= 5, "dfta_orbital_properties arguments");
    for (int k = 0; k < norb; ++k) DFTA_REQUIRE(ctx, l[k] >= 0, "dfta_orbital_properties: l < 0");
    hipStream_t st = ctx->stream;
    DevBuf<double> dU, dP;
    DevBuf<int> dL;
    DFTA_HIP(ctx, dP.alloc((size_t)norb * kProps));
    int rc = dfta_upload_rows(ctx, u, (size_t)norb * g->N, &dU);
    if (!rc) rc = dfta_upload_rows(ctx, l, (size_t)norb, &dL);
    if (!rc) rc = dfta_launch_orbital_properties(ctx, g, norb, dL.p, dU.p, dP.p);
    if (rc) return rc;
    DFTA_HIP(ctx, hipMemcpyAsync(props, dP.p, sizeof(double) * norb * kProps, hipMemcpyDeviceToHost, st));
    DFTA_HIP(ctx, hipStreamSynchronize(st));
    return DFTA_OK;
}

int dfta_orbital_matrix(dfta_ctx* ctx, const dfta_grid* g, int norb, const double* u, int k, double* M)
{
    if (!ctx || !g) return DFTA_ERR_INVALID;
    DFTA_ENTER(ctx);
    DFTA_REQUIRE(ctx, norb >= 0 && norb <= kOrbitalMatrixMax, "dfta_orbital_matrix: norb (0 .. 32)");
    DFTA_REQUIRE(ctx, k >= 0 && k <= 2, "dfta_orbital_matrix: k (0, 1 or 2)");
    if (norb == 0) return DFTA_OK;
    DFTA_REQUIRE(ctx, u && M, "dfta_orbital_matrix arguments");
    hipStream_t st = ctx->stream;
    DevBuf<double> dU;
    dfta_orbital_scratch sc;
    int rc = dfta_orbital_scratch_create(ctx, g, norb, &sc);
    if (!rc) rc = dfta_upload_rows(ctx, u, (size_t)norb * g->N, &dU);
    if (!rc) rc = dfta_launch_orbital_matrix(ctx, g, norb, dU.p, k, sc.slab.p, sc.ticket.p, sc.M.p);
    if (rc) return rc;
    DFTA_HIP(ctx, hipMemcpyAsync(M, sc.M.p, sizeof(double) * norb * norb, hipMemcpyDeviceToHost, st));
    DFTA_HIP(ctx, hipStreamSynchronize(st));
    return DFTA_OK;
}

}  // extern "C"
