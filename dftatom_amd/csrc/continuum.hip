// continuum.hip -- outward Numerov sweeps at any finite energy: logarithmic derivatives, node counts, phase shifts, energy-normalised
// continuum orbitals and their overlap / dipole sums with bound orbitals (include/dftatom_hip.h has the arithmetic, DESIGN.md 4.14 the
// shape and the choice of staging).  Beyond the reference's live code: its SolveSchrodingerCountNodesFromNucleus (Numerov.h:204-270) is
// dormant there.
//
//   k_partner_weight     g_b,i = w_i ((P_b,i r_i^p) s_i) of every partner row, grid-stride: formed once per call, not once per wave.
//   k_continuum<NP, ROWS> one workgroup of ONE wave per block of 64 trials of a (potential, l, partner list); one lane per trial, the
//                        lanes march the node index together.  What is the same in every lane -- vl_i, s_i^2, sqrt(s_i) and the NP
//                        weighted partner values of a node -- is staged per tile of 256 nodes in LDS by the wave itself (lane t forms
//                        the nodes t, t + 64, t + 128, t + 192) and read back as broadcasts; the tile is also the block of the partner
//                        sums.  A lane is live while i <= m + 1 of ITS trial; the wave runs to the largest m + 1 among its lanes.
//                        ROWS: the unscaled q_i y_i of 64 nodes x 64 trials go through a padded LDS square so that each store
//                        instruction writes 64 consecutive nodes of one trial's row.
//   k_continuum_scale    rows: u = (q y) factor for 1 <= i <= m + 1, 0.0 elsewhere -- the factor is known only at m.
// A trial has its own registers and accumulators from start to end and reads only staged values that do not depend on the other
// lanes: its bits do not depend on the other trials, their number or order, NP, ROWS, the chunking of the rows or the run.  No atomics;
// every result leaves through ordinary vector stores.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstring>
#include <vector>

#include "bessel_device.h"
#include "continuum_plan.h"
#include "internal.h"
#include "radial_device.h"

namespace {

using dfta_bessel::sph_bessel;
using dfta_radial::simpson38_weight;
namespace cp = dfta_continuum_plan;

constexpr int kTile = cp::kTile;
constexpr int kBlkInts = 4 + cp::kMaxPartners;      // per block: potential, l, first position, trials, then the rows of its list (-1: none)
constexpr int kPad = 65;                            // row pitch of the transposition square
// the doubles nearest pi and sqrt(2 / pi)
constexpr double kPi = 3.141592653589793;
constexpr double kSqrtTwoOverPi = 0.7978845608028654;

struct ContArgs {
    int N, mode;
    double hstep, c, lam;
    const double *r, *cnst, *V, *G;                 // V: nV x N; G: the weighted partner rows
    const int* blk;                                 // kBlkInts per block
    const double* E;                                // per padded position
    const int* m;                                   // ... (-1: padding)
    double *logderiv, *dop, *scale, *sums;          // sums: 16 per position
    int *nodes, *status;
    double* rows;                                   // ROWS: the chunk's rows, position - 64 block0 first
};

__global__ __launch_bounds__(256) void k_partner_weight(int N, double hstep, int power, size_t total, const double* __restrict__ r,
                                                        const double* __restrict__ cnst, const double* __restrict__ P, double* __restrict__ G)
{
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x; k < total; k += stride) {
        const int i = (int)(k % (size_t)N);
        const double ri = r[i];
        double rp = 1.;
        for (int q = 0; q < power; ++q) rp = rp * ri;
        G[k] = simpson38_weight(i, N) * ((P[k] * rp) * (cnst[i] * hstep));
    }
}

// yh_l(x) and yh'_l(x) of the header
__device__ __forceinline__ void riccati_y(int l, double x, double s, double co, double* yh, double* yhp)
{
    if (l == 0) { *yh = -co; *yhp = s; return; }
    double ym = -co;                                 // yh_0
    double y = ym / x - s;                           // yh_1
    for (int n = 1; n < l; ++n) {
        const double yn = (((double)(2 * n + 1)) / x) * y - ym;
        ym = y;
        y = yn;
    }
    *yh = y;
    *yhp = ym - (((double)l) / x) * y;
}

// atan2 of the header: the library's atan2 only in the octant 0 <= min / max <= 1, the quadrant put back with both halves of pi / 2 and
// of pi.  (The library's own reconstruction subtracts from the ONE double nearest pi, 0.28 ulp short before its rounding: one ulp off in
// a phase near pi.)  s and e: the exact sum of the constant's head and -hi (the head is at least twice hi).
__device__ __forceinline__ double atan2_quadrants(double y, double x)
{
    const double kHalfPiHi = 1.5707963267948966, kHalfPiLo = 6.123233995736766e-17, kPiLo = 1.2246467991473532e-16;
    const double ay = fabs(y), ax = fabs(x);
    double hi = atan2(ay > ax ? ax : ay, ay > ax ? ay : ax), lo = 0.;      // (a NaN stays in place and comes out of the library)
    if (ay > ax) {
        const double s = kHalfPiHi - hi, e = (kHalfPiHi - s) - hi;
        lo = (e + kHalfPiLo) - lo;
        hi = s;
    }
    if (signbit(x)) {
        const double s = kPi - hi, e = (kPi - s) - hi;
        lo = (e + kPiLo) - lo;
        hi = s;
    }
    return copysign(hi + lo, y);
}

// DFTA_CONT_NORM: the normalisation left double range -- an operand of the hypot is NaN (inf - inf in the matching) or the factor is
// not finite.  (An infinite operand alone gives factor 0.0 and no bit: the header counts that as an underflow.)
__device__ __forceinline__ bool norm_finite(double a, double b, double factor) { return a == a && b == b && fabs(factor) <= DBL_MAX; }

template <int NP, bool ROWS>
__global__ __launch_bounds__(64) void k_continuum(ContArgs a, int block0)
{
    __shared__ double s_vl[kTile], s_s2[kTile], s_sq[kTile];
    __shared__ double s_g[NP > 0 ? NP : 1][kTile];
    __shared__ double s_t[ROWS ? 64 * kPad : 1];
    const int lane = threadIdx.x, b = blockIdx.x + block0, N = a.N;
    const int* __restrict__ bk = a.blk + (size_t)b * kBlkInts;
    const int l = bk[1], first = bk[2], cnt = bk[3];
    const double* __restrict__ V = a.V + (size_t)bk[0] * N;
    const double L = (double)l * ((double)l + 1.);
    const bool mine = lane < cnt;
    const double E = mine ? a.E[first + lane] : 0.;
    const int m = mine ? a.m[first + lane] : -1;
    const int mend = m + 1;                          // the lane's last node (0: none)
    int wave_end = mend;
    for (int off = 32; off > 0; off >>= 1) wave_end = max(wave_end, __shfl_xor(wave_end, off));

    // the start: the fit at nodes 1 and 2 and the series' coefficients
    const double r1 = a.r[1], r2 = a.r[2], V1 = V[1], V2 = V[2];
    const double Zc = ((V2 - V1) * (r1 * r2)) / (r2 - r1);
    const double v0 = V1 + Zc / r1;
    double ak[5];
    ak[0] = 1.;
    ak[1] = -Zc / ((double)l + 1.);
#pragma unroll
    for (int k = 2; k <= 4; ++k) ak[k] = (((-2. * Zc) * ak[k - 1]) + ((2. * (v0 - E)) * ak[k - 2])) / (double)(k * (k + 2 * l + 1));

    double w1 = 0., w2 = 0., y1 = 0., f1 = 0.;
    double ym1 = 0., fm1 = 0., ym = 0., yp = 0., fp = 0.;
    int nodes = 0, status = 0;
    double tot[NP > 0 ? NP : 1], bs[NP > 0 ? NP : 1];
#pragma unroll
    for (int q = 0; q < (NP > 0 ? NP : 1); ++q) tot[q] = 0.;

    for (int tile0 = 0; tile0 <= wave_end; tile0 += kTile) {
        // stage what every lane shares at the tile's nodes
#pragma unroll
        for (int k = 0; k < kTile / 64; ++k) {
            const int j = lane + 64 * k, i = tile0 + j;
            double vl = 0., s2 = 1., sq = 1.;
            if (i < N) {
                const double ri = a.r[i], si = a.cnst[i] * a.hstep;
                s2 = si * si;
                sq = sqrt(si);
                vl = V[i] + ((L / (ri * ri)) * 0.5);
            }
            s_vl[j] = vl; s_s2[j] = s2; s_sq[j] = sq;
            if (NP > 0) {
#pragma unroll
                for (int q = 0; q < NP; ++q) {
                    const int row = bk[4 + q];
                    s_g[q][j] = (row >= 0 && i < N) ? a.G[(size_t)row * N + i] : 0.;
                }
            }
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < (NP > 0 ? NP : 1); ++q) bs[q] = 0.;
        for (int sub = 0; sub < kTile / 64; ++sub) {
            const int i0 = tile0 + 64 * sub;
            if (i0 > wave_end) break;
            for (int jj = 0; jj < 64; ++jj) {
                const int i = i0 + jj, j = 64 * sub + jj;
                const double vl = s_vl[j], s2 = s_s2[j], sq = s_sq[j];
                const bool on = i >= 1 && i <= mend;
                const double f = (2. * (vl - E)) * s2 + a.c;
                const double d = 1. - f / 12.;
                double y, w;
                if (i <= 2) {                        // (the same in every lane)
                    const double ri = a.r[i];
                    double p = ri;
                    for (int q = 0; q < l; ++q) p = p * ri;
                    const double u = p * ((((ak[4] * ri + ak[3]) * ri + ak[2]) * ri + ak[1]) * ri + ak[0]);
                    y = u / sq;
                    w = d * y;
                } else {
                    w = ((2. * w1) - w2) + f1 * y1;
                    y = w / d;
                    if (on && !(d > 0.)) status |= DFTA_CONT_STEP;
                }
                if (on) {
                    if (!(fabs(y) <= DBL_MAX)) status |= DFTA_CONT_NONFINITE;
                    if (i >= 2 && i <= m && ((y < 0.) != (y1 < 0.))) ++nodes;
                    if (i == m - 1) { ym1 = y; fm1 = f; }
                    if (i == m) ym = y;
                    if (i == mend) { yp = y; fp = f; }
                    if (NP > 0 && i <= m) {
                        const double u = sq * y;
#pragma unroll
                        for (int q = 0; q < NP; ++q) bs[q] += s_g[q][j] * u;
                    }
                    w2 = w1; w1 = w; y1 = y; f1 = f;
                }
                if (ROWS) s_t[lane * kPad + jj] = on ? sq * y : 0.;
            }
            if (ROWS) {
                __syncthreads();
                const int i = i0 + lane;
                if (i < N)
                    for (int tt = 0; tt < cnt; ++tt) a.rows[((size_t)(b - block0) * 64 + tt) * N + i] = s_t[tt * kPad + lane];
                __syncthreads();
            }
        }
        if (NP > 0 && tile0 <= m) {
#pragma unroll
            for (int q = 0; q < NP; ++q) tot[q] = tot[q] + bs[q];
        }
        __syncthreads();
    }
    if (!mine) return;

    // the end node
    const double nan = __builtin_nan("");
    double logderiv = nan, dop = nan, scale = nan, factor = nan;
    if (!(status & (DFTA_CONT_NONFINITE | DFTA_CONT_STEP))) {
        const double dy = (((1. - fp / 6.) * yp) - ((1. - fm1 / 6.) * ym1)) * 0.5;
        const double qm = sqrt(a.cnst[m] * a.hstep);
        const double um = qm * ym;
        const double dum = (dy + (a.lam * 0.5) * ym) / qm;
        logderiv = dum / um;
        if (!(E > 0.)) {
            dop = 0.; scale = 0.; factor = 1.;
        } else if (a.mode == DFTA_CONT_FREE) {
            const double k = sqrt(2. * E), x = k * a.r[m], U = dum / k;
            double s, co, jh, jhp, yh, yhp;
            sincos(x, &s, &co);
            jh = x * sph_bessel(l, x);
            jhp = l == 0 ? co : x * sph_bessel(l - 1, x) - (((double)l) / x) * jh;
            riccati_y(l, x, s, co, &yh, &yhp);
            const double ca = um * yhp - U * yh, cb = U * jh - um * jhp;
            dop = atan2_quadrants(-cb, ca);
            factor = sqrt(2. / (kPi * k)) / hypot(ca, cb);
            scale = factor;
            if (!norm_finite(ca, cb, factor)) { status |= DFTA_CONT_NORM; dop = nan; scale = nan; factor = nan; }
        } else {
            double kap[3];
            bool ok = true;
#pragma unroll
            for (int q = 0; q < 3; ++q) {
                const int i = m - 1 + q;
                const double ri = a.r[i];
                const double k2 = (2. * (E - V[i])) - L / (ri * ri);
                ok = ok && k2 > 0.;
                kap[q] = sqrt(k2);
            }
            if (ok) {
                const double kp = (kap[2] - kap[0]) / (a.r[m + 1] - a.r[m - 1]);
                const double sk = sqrt(kap[1]);
                const double al = 1. / sk;
                const double alp = -kp / ((2. * kap[1]) * sk);
                const double A = um / al, B = al * dum - alp * um;
                factor = kSqrtTwoOverPi / hypot(A, B);
                dop = atan2_quadrants(A, B);
                scale = factor;
                if (!norm_finite(A, B, factor)) { status |= DFTA_CONT_NORM; dop = nan; scale = nan; factor = nan; }
            } else {
                status |= DFTA_CONT_WKB_TAIL;
            }
        }
    } else {
        nodes = -1;
    }
    const size_t pos = (size_t)first + lane;
    a.logderiv[pos] = logderiv; a.dop[pos] = dop; a.scale[pos] = scale;
    a.nodes[pos] = nodes; a.status[pos] = status;
    if (NP > 0) {
#pragma unroll
        for (int q = 0; q < NP; ++q) a.sums[pos * cp::kMaxPartners + q] = dfta_radial::simpson38_finish(tot[q]) * factor;
    }
}

// rows of a chunk: npos positions from pos0 on; one row per blockIdx.y
__global__ __launch_bounds__(256) void k_continuum_scale(int N, size_t pos0, const double* __restrict__ E, const int* __restrict__ m,
                                                         const double* __restrict__ scale, const int* __restrict__ status,
                                                         double* __restrict__ rows)
{
    const size_t pos = pos0 + blockIdx.y;
    const int mt = m[pos];
    if (mt < 0) return;                              // padding
    const double factor = (status[pos] & (DFTA_CONT_NONFINITE | DFTA_CONT_STEP)) ? __builtin_nan("") : (E[pos] > 0. ? scale[pos] : 1.);
    double* __restrict__ row = rows + (size_t)blockIdx.y * N;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < N; i += gridDim.x * blockDim.x) row[i] = (i >= 1 && i <= mt + 1) ? row[i] * factor : 0.;
}

template <bool ROWS>
void launch_instance(int instance, dim3 grid, hipStream_t st, const ContArgs& a, int block0)
{
    switch (instance) {
    case 16: hipLaunchKernelGGL((k_continuum<16, ROWS>), grid, dim3(64), 0, st, a, block0); break;
    case 8: hipLaunchKernelGGL((k_continuum<8, ROWS>), grid, dim3(64), 0, st, a, block0); break;
    case 4: hipLaunchKernelGGL((k_continuum<4, ROWS>), grid, dim3(64), 0, st, a, block0); break;
    default: hipLaunchKernelGGL((k_continuum<0, ROWS>), grid, dim3(64), 0, st, a, block0); break;
    }
}

}  // namespace

int dfta_continuum_run(dfta_ctx* ctx, const dfta_grid* g, const dfta_continuum_plan::Call& c, const double* dV, const double* dP,
                       const dfta_continuum_out& out)
{
    if (c.ntrials <= 0) return DFTA_OK;
    const cp::Plan plan = cp::plan(c, out.rows != nullptr);
    const size_t N = (size_t)g->N, npos = plan.order.size();
    const int nblocks = (int)plan.blocks.size();
    hipStream_t st = ctx->stream;

    std::vector<double> hE(npos, 0.);
    std::vector<int> hm(npos, -1), hblk((size_t)nblocks * kBlkInts, -1);
    for (size_t p = 0; p < npos; ++p)
        if (plan.order[p] >= 0) { hE[p] = c.E[plan.order[p]]; hm[p] = c.m[plan.order[p]]; }
    for (int b = 0; b < nblocks; ++b) {
        const cp::Block& bl = plan.blocks[b];
        int* bk = &hblk[(size_t)b * kBlkInts];
        bk[0] = bl.v; bk[1] = bl.l; bk[2] = bl.first; bk[3] = bl.cnt;
        if (bl.list >= 0)
            for (int j = c.list_off[bl.list]; j < c.list_off[bl.list + 1]; ++j) bk[4 + j - c.list_off[bl.list]] = c.list_rows[j];
    }
    DevBuf<double> dE, dLog, dDop, dScale, dSums, dG, dRows;
    DevBuf<int> dM, dBlk, dNodes, dStatus;
    if (const int rc = dfta_upload_rows(ctx, hE.data(), npos, &dE)) return rc;
    if (const int rc = dfta_upload_rows(ctx, hm.data(), npos, &dM)) return rc;
    if (const int rc = dfta_upload_rows(ctx, hblk.data(), hblk.size(), &dBlk)) return rc;
    DFTA_HIP(ctx, dLog.alloc(npos));
    DFTA_HIP(ctx, dDop.alloc(npos));
    DFTA_HIP(ctx, dScale.alloc(npos));
    DFTA_HIP(ctx, dNodes.alloc(npos));
    DFTA_HIP(ctx, dStatus.alloc(npos));
    if (plan.instance > 0) {
        DFTA_HIP(ctx, dSums.alloc(npos * cp::kMaxPartners));
        DFTA_HIP(ctx, dG.alloc((size_t)c.npartner_rows * N));
    }
    const int per_chunk = out.rows ? plan.blocks_per_chunk : nblocks;
    if (out.rows) DFTA_HIP(ctx, dRows.alloc((size_t)per_chunk * 64 * N));

    ContArgs a;
    a.N = g->N; a.mode = c.norm_mode;
    a.hstep = dfta_hstep(g);
    a.c = g->uniform ? 0. : g->delta2p4;
    a.lam = g->uniform ? 0. : g->delta;
    a.r = g->d_r.p; a.cnst = g->d_cnst.p; a.V = dV; a.G = dG.p;
    a.blk = dBlk.p; a.E = dE.p; a.m = dM.p;
    a.logderiv = dLog.p; a.dop = dDop.p; a.scale = dScale.p; a.sums = dSums.p;
    a.nodes = dNodes.p; a.status = dStatus.p; a.rows = dRows.p;

    std::vector<double> stage;
    DFTA_HIP(ctx, dfta_timer_start(ctx));
    if (plan.instance > 0) {
        const size_t total = (size_t)c.npartner_rows * N;
        const unsigned blocks = (unsigned)std::min<size_t>((total + 255) / 256, 8192);
        hipLaunchKernelGGL(k_partner_weight, dim3(blocks), dim3(256), 0, st, g->N, a.hstep, c.power, total, g->d_r.p, g->d_cnst.p, dP, dG.p);
        DFTA_CHECK_LAUNCH(ctx);
    }
    for (int block0 = 0; block0 < nblocks; block0 += per_chunk) {
        const int nb = std::min(per_chunk, nblocks - block0);
        if (out.rows) launch_instance<true>(plan.instance, dim3(nb), st, a, block0);
        else launch_instance<false>(plan.instance, dim3(nb), st, a, block0);
        DFTA_CHECK_LAUNCH(ctx);
        if (!out.rows) continue;
        const unsigned gx = (unsigned)std::min<size_t>((N + 255) / 256, 64);
        hipLaunchKernelGGL(k_continuum_scale, dim3(gx, (unsigned)nb * 64), dim3(256), 0, st, g->N, (size_t)block0 * 64, dE.p, dM.p, dScale.p,
                           dStatus.p, dRows.p);
        DFTA_CHECK_LAUNCH(ctx);
        if (block0 + nb >= nblocks) DFTA_HIP(ctx, dfta_timer_stop(ctx));      // the events bracket every launch (and the chunks' copies between them)
        stage.resize((size_t)nb * 64 * N);
        DFTA_HIP(ctx, hipMemcpyAsync(stage.data(), dRows.p, sizeof(double) * stage.size(), hipMemcpyDeviceToHost, st));
        DFTA_HIP(ctx, hipStreamSynchronize(st));
        for (size_t p = 0; p < (size_t)nb * 64; ++p) {
            const int t = plan.order[(size_t)block0 * 64 + p];
            if (t >= 0) memcpy(out.rows + (size_t)t * N, stage.data() + p * N, sizeof(double) * N);
        }
    }
    if (!out.rows) DFTA_HIP(ctx, dfta_timer_stop(ctx));

    std::vector<double> h1(npos), h2(npos), h3(npos), hs;
    std::vector<int> i1(npos), i2(npos);
    DFTA_HIP(ctx, hipMemcpyAsync(h1.data(), dLog.p, sizeof(double) * npos, hipMemcpyDeviceToHost, st));
    DFTA_HIP(ctx, hipMemcpyAsync(h2.data(), dDop.p, sizeof(double) * npos, hipMemcpyDeviceToHost, st));
    DFTA_HIP(ctx, hipMemcpyAsync(h3.data(), dScale.p, sizeof(double) * npos, hipMemcpyDeviceToHost, st));
    DFTA_HIP(ctx, hipMemcpyAsync(i1.data(), dNodes.p, sizeof(int) * npos, hipMemcpyDeviceToHost, st));
    DFTA_HIP(ctx, hipMemcpyAsync(i2.data(), dStatus.p, sizeof(int) * npos, hipMemcpyDeviceToHost, st));
    if (plan.instance > 0 && out.sums) {
        hs.resize(npos * cp::kMaxPartners);
        DFTA_HIP(ctx, hipMemcpyAsync(hs.data(), dSums.p, sizeof(double) * hs.size(), hipMemcpyDeviceToHost, st));
    }
    DFTA_HIP(ctx, hipStreamSynchronize(st));
    for (size_t p = 0; p < npos; ++p) {
        const int t = plan.order[p];
        if (t < 0) continue;
        if (out.logderiv) out.logderiv[t] = h1[p];
        if (out.delta_or_phase) out.delta_or_phase[t] = h2[p];
        if (out.scale) out.scale[t] = h3[p];
        if (out.nodes) out.nodes[t] = i1[p];
        if (out.status) out.status[t] = i2[p];
        if (out.sums) {
            const int list = c.trial_list ? c.trial_list[t] : -1;
            const int np = list >= 0 ? c.list_off[list + 1] - c.list_off[list] : 0;
            for (int q = 0; q < cp::kMaxPartners; ++q) out.sums[(size_t)t * cp::kMaxPartners + q] = q < np ? hs[p * cp::kMaxPartners + q] : 0.;
        }
    }
    return DFTA_OK;
}

extern "C" {

int dfta_continuum(dfta_ctx* ctx, const dfta_grid* g, int norm_mode, int nV, const double* V, int ntrials, const int* vidx, const int* l,
                   const double* E, const int* m, int npartner_rows, const double* P, int power, int nlists, const int* list_off,
                   const int* list_rows, const int* trial_list, double* logderiv, int* nodes, double* delta_or_phase, double* scale,
                   int* status, double* sums, double* rows)
{
    if (!ctx || !g) return DFTA_ERR_INVALID;
    DFTA_ENTER(ctx);
    DFTA_REQUIRE(ctx, ntrials >= 0, "dfta_continuum: ntrials");
    if (ntrials == 0) return DFTA_OK;
    DFTA_REQUIRE(ctx, V && l && E && m, "dfta_continuum arguments");
    DFTA_REQUIRE(ctx, npartner_rows == 0 || P, "dfta_continuum: P");
    cp::Call c;
    c.norm_mode = norm_mode; c.N = g->N; c.nV = nV; c.ntrials = ntrials;
    c.vidx = vidx; c.l = l; c.E = E; c.m = m;
    c.npartner_rows = npartner_rows; c.power = power; c.nlists = nlists;
    c.list_off = list_off; c.list_rows = list_rows; c.trial_list = nlists > 0 ? trial_list : nullptr;
    if (const char* msg = cp::check(c)) DFTA_REQUIRE(ctx, false, msg);
    DevBuf<double> dV, dP;
    if (const int rc = dfta_upload_rows(ctx, V, (size_t)nV * g->N, &dV)) return rc;
    if (const int rc = dfta_upload_rows(ctx, P, (size_t)npartner_rows * g->N, &dP)) return rc;
    dfta_continuum_out out;
    out.logderiv = logderiv; out.nodes = nodes; out.delta_or_phase = delta_or_phase; out.scale = scale; out.status = status;
    out.sums = sums; out.rows = rows;
    return dfta_continuum_run(ctx, g, c, dV.p, dP.p, out);
}

}  // extern "C"
