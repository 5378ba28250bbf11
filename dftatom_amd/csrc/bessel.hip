// bessel.hip -- spherical Bessel functions j_l, 0 <= l <= 4, and the Bessel (Hankel) transforms of radial arrays: X-ray form factors of
// densities and momentum-space radial functions of orbitals (include/dftatom_hip.h has the definitions; DESIGN.md 4.10 the summation
// shape, the two branches of j_l and the rounding count).  Beyond the reference, which has no q-space quantity.
//
//   k_sph_bessel         pointwise j_l(x), grid-stride: the test entry of the device's j_l.
//   k_bessel_transform   every (row, q) of a call in one launch, no communication between workgroups.  One workgroup of 256 lanes per
//                        (row, block of QB consecutive q's): the row passes once, lane t taking the nodes t, t + 256, t + 512, ... in that
//                        order (k_orbital_properties' order: node tile * 1024 + t + 256 j, j = 0 .. 3, tile after tile).  At a node the
//                        weighted term g_i is formed once, then the QB Bessel values, each added into its own register accumulator; a node
//                        whose g_i is zero adds nothing (an orbital beyond its cut-off index, an underflowed density tail).  The end is
//                        k_orbital_properties' tree, per q: xor shuffles 32 .. 1, then (w0 + w1) + (w2 + w3).
// Every q has its own accumulator and its own tree of a shape that depends on N alone: a (row, q) value depends on the row, its l, the
// kind, q and the grid -- not on QB, the other rows or q's of the call, their order, or the run.  No floating-point atomics.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <vector>

#include "bessel_device.h"
#include "bessel_plan.h"
#include "internal.h"
#include "radial_device.h"

namespace {

using dfta_bessel::sph_bessel;         // bessel_device.h: the one statement of j_l
using namespace dfta_radial;

constexpr int kBtThreads = 256;

__global__ __launch_bounds__(256) void k_sph_bessel(int l, size_t n, const double* __restrict__ x, double* __restrict__ out)
{
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) out[i] = sph_bessel(l, x[i]);
}

template <int QB>
__global__ __launch_bounds__(kBtThreads) void k_bessel_transform(int N, double hstep, const double* __restrict__ r,
                                                                 const double* __restrict__ cnst, int kind, double scale,
                                                                 const int* __restrict__ l, const double* const* __restrict__ rows, int nq,
                                                                 const double* __restrict__ q, double* __restrict__ out)
{
    __shared__ double red[kBtThreads / 64][QB];
    const int tid = threadIdx.x;
    const int nqb = (nq + QB - 1) / QB;
    const int row = blockIdx.x / nqb, q0 = (blockIdx.x - row * nqb) * QB;
    const int nv = min(QB, nq - q0);                 // q's of this workgroup (the last block of a row may be short)
    const double* __restrict__ f = dfta_as_global(rows[row]);
    const int lq = l[row];
    double qv[QB], acc[QB];
#pragma unroll
    for (int m = 0; m < QB; ++m) {
        qv[m] = m < nv ? q[q0 + m] : 0.;
        acc[m] = 0.;
    }
    // the node after the one being worked on is loaded ahead of its use
    int i = tid;
    double fi = 0., ri = 0., ci = 0.;
    if (i < N) { fi = f[i]; ri = r[i]; ci = cnst[i]; }
    while (i < N) {
        const int in = i + kBtThreads;
        double fn = 0., rn = 0., cn = 0.;
        if (in < N) { fn = f[in]; rn = r[in]; cn = cnst[in]; }
        const double sc = ci * hstep;
        const double fr = fi * ri;
        const double g = simpson38_weight(i, N) * ((kind == DFTA_BT_DENSITY ? fr * ri : fr) * sc);
        if (g != 0.) {                               // (NaN != 0: a NaN node reaches every q of its row)
#pragma unroll
            for (int m = 0; m < QB; ++m)
                if (m < nv) acc[m] += g * sph_bessel(lq, qv[m] * ri);
        }
        i = in; fi = fn; ri = rn; ci = cn;
    }
    // the tree of radial_device.h, per q
#pragma unroll
    for (int m = 0; m < QB; ++m) {
        const double v = wave_tree_sum(acc[m]);
        if ((tid & 63) == 0) red[tid >> 6][m] = v;
    }
    __syncthreads();
    if (tid < nv) out[(size_t)row * nq + q0 + tid] = simpson38_finish(waves_join(red[0][tid], red[1][tid], red[2][tid], red[3][tid])) * scale;
}

// the doubles nearest 4 pi and sqrt(2 / pi)
constexpr double kFourPi = 12.566370614359172;
constexpr double kSqrtTwoOverPi = 0.7978845608028654;

}  // namespace

int dfta_launch_bessel_transform(dfta_ctx* ctx, const dfta_grid* g, int kind, int nrow, const int* dL, const double* const* dRows, int nq,
                                 const double* dQ, double* dOut)
{
    if (nrow <= 0 || nq <= 0) return DFTA_OK;
    int forced = 0;
    if (const char* e = dfta_knob("BESSEL_QBLOCK")) forced = atoi(e);        // measurements / tests: q's per workgroup
    const int qb = dfta_bessel::pick_qblock(nrow, nq, ctx->num_cu, forced);
    DFTA_REQUIRE(ctx, dfta_bessel::num_blocks(nrow, nq, qb) <= 0x7fffffffL, "Bessel transform: too many (row, q) pairs for one launch");
    const dim3 grid((unsigned)dfta_bessel::num_blocks(nrow, nq, qb)), block(kBtThreads);
    const double hstep = dfta_hstep(g), scale = kind == DFTA_BT_DENSITY ? kFourPi : kSqrtTwoOverPi;
    hipStream_t st = ctx->stream;
    DFTA_HIP(ctx, dfta_timer_start(ctx));
    switch (qb) {
    case 8: hipLaunchKernelGGL(k_bessel_transform<8>, grid, block, 0, st, g->N, hstep, g->d_r.p, g->d_cnst.p, kind, scale, dL, dRows, nq, dQ, dOut); break;
    case 4: hipLaunchKernelGGL(k_bessel_transform<4>, grid, block, 0, st, g->N, hstep, g->d_r.p, g->d_cnst.p, kind, scale, dL, dRows, nq, dQ, dOut); break;
    case 2: hipLaunchKernelGGL(k_bessel_transform<2>, grid, block, 0, st, g->N, hstep, g->d_r.p, g->d_cnst.p, kind, scale, dL, dRows, nq, dQ, dOut); break;
    default: hipLaunchKernelGGL(k_bessel_transform<1>, grid, block, 0, st, g->N, hstep, g->d_r.p, g->d_cnst.p, kind, scale, dL, dRows, nq, dQ, dOut); break;
    }
    DFTA_CHECK_LAUNCH(ctx);
    DFTA_HIP(ctx, dfta_timer_stop(ctx));
    return DFTA_OK;
}

int dfta_bessel_scratch::run(dfta_ctx* ctx, const dfta_grid* g, int kind, int nrow, const int* l, const double* const* rows, int nq,
                             const double* q, double* out)
{
    if (nrow <= 0 || nq <= 0) return DFTA_OK;
    hipStream_t st = ctx->stream;
    DFTA_HIP(ctx, d_l.reserve(nrow));                // first use, or more rows / q's than any call before
    DFTA_HIP(ctx, d_rows.reserve(nrow));
    DFTA_HIP(ctx, d_q.reserve(nq));
    DFTA_HIP(ctx, d_out.reserve((size_t)nrow * nq));
    DFTA_HIP(ctx, hipMemcpyAsync(d_l.p, l, sizeof(int) * nrow, hipMemcpyHostToDevice, st));
    DFTA_HIP(ctx, hipMemcpyAsync(d_rows.p, rows, sizeof(const double*) * nrow, hipMemcpyHostToDevice, st));
    DFTA_HIP(ctx, hipMemcpyAsync(d_q.p, q, sizeof(double) * nq, hipMemcpyHostToDevice, st));
    const int rc = dfta_launch_bessel_transform(ctx, g, kind, nrow, d_l.p, d_rows.p, nq, d_q.p, d_out.p);
    if (rc) return rc;
    DFTA_HIP(ctx, hipMemcpyAsync(out, d_out.p, sizeof(double) * nrow * nq, hipMemcpyDeviceToHost, st));
    DFTA_HIP(ctx, hipStreamSynchronize(st));
    return DFTA_OK;
}

// ---- the two launches on caller-supplied arrays (host pointers) ---------------------------------------------------------------------
extern "C" {

int dfta_sph_bessel(dfta_ctx* ctx, int l, size_t n, const double* x, double* out)
{
    if (!ctx) return DFTA_ERR_INVALID;
    DFTA_ENTER(ctx);
    DFTA_REQUIRE(ctx, l >= 0 && l <= dfta_bessel::kLmax, "dfta_sph_bessel: l outside 0 .. 4");
    if (n == 0) return DFTA_OK;
    DFTA_REQUIRE(ctx, x && out, "dfta_sph_bessel arguments");
    for (size_t i = 0; i < n; ++i) DFTA_REQUIRE(ctx, x[i] >= 0. && !std::isinf(x[i]), "dfta_sph_bessel: x must be finite and >= 0");
    hipStream_t st = ctx->stream;
    DevBuf<double> dX, dO;
    DFTA_HIP(ctx, dO.alloc(n));
    if (const int rc = dfta_upload_rows(ctx, x, n, &dX)) return rc;
    const unsigned blocks = (unsigned)std::min<size_t>((n + 255) / 256, 4096);
    DFTA_HIP(ctx, dfta_timer_start(ctx));
    hipLaunchKernelGGL(k_sph_bessel, dim3(blocks), dim3(256), 0, st, l, n, dX.p, dO.p);
    DFTA_CHECK_LAUNCH(ctx);
    DFTA_HIP(ctx, dfta_timer_stop(ctx));
    DFTA_HIP(ctx, hipMemcpyAsync(out, dO.p, sizeof(double) * n, hipMemcpyDeviceToHost, st));
    DFTA_HIP(ctx, hipStreamSynchronize(st));
    return DFTA_OK;
}

int dfta_bessel_transform(dfta_ctx* ctx, const dfta_grid* g, int kind, int nrow, const int* l, const double* f, int nq, const double* q,
                          double* out)
{
    if (!ctx || !g) return DFTA_ERR_INVALID;
    DFTA_ENTER(ctx);
    DFTA_REQUIRE(ctx, nrow >= 0 && nq >= 0, "dfta_bessel_transform: nrow, nq");
    DFTA_REQUIRE(ctx, kind == DFTA_BT_DENSITY || kind == DFTA_BT_ORBITAL, "dfta_bessel_transform: kind (DFTA_BT_DENSITY or DFTA_BT_ORBITAL)");
    if (nrow == 0 || nq == 0) return DFTA_OK;
    DFTA_REQUIRE(ctx, l && f && q && out, "dfta_bessel_transform arguments");
    DFTA_REQUIRE(ctx, g->N >= 5, "dfta_bessel_transform: the grid needs 5 nodes");
    if (const char* msg = dfta_bessel::check_transform(kind, nrow, l, nq, q)) DFTA_REQUIRE(ctx, false, msg);
    const size_t N = g->N;
    DevBuf<double> dF;
    dfta_bessel_scratch sc;
    if (const int rc = dfta_upload_rows(ctx, f, (size_t)nrow * N, &dF)) return rc;
    std::vector<const double*> rows(nrow);
    for (int a = 0; a < nrow; ++a) rows[a] = dF.p + (size_t)a * N;
    return sc.run(ctx, g, kind, nrow, l, rows.data(), nq, q, out);
}

}  // extern "C"
