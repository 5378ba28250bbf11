// mixing.hip -- Anderson density mixing of the batched SCF (dfta_scf_options::mixing == DFTA_MIX_ANDERSON; include/dftatom_hip.h has the rule).
//
// The reference mixes linearly (DFTAtom.cpp:332-342, k_mix of scf.hip); this goes beyond it.  Three ordinary launches on the context's
// stream take k_mix's place, with no host synchronisation between them:
//   k_anderson_gram    grid (chunks of kAndersonChunk nodes, atoms): g = newDensity / (4 pi r^2) exactly as k_mix divides, stored back;
//                      f = g - x; the chunk's share of A_jk = <dF_j, dF_k> (j <= k) and b_j = <dF_j, f> into the slab [atom][chunk][44]
//   k_anderson_solve   one wave per atom: the slab summed in chunk order, (A + 1e-14 trace(A) I) gamma = b by Cholesky, the use flag,
//                      the ring's head / length / step count advanced (cleared on a failed solve)
//   k_anderson_update  lin with k_mix's expression, cand = lin - Sum_j gamma_j (dX_j + (1 - alpha) dF_j) oldest to newest, the clamp, and
//                      this step's (x, f) into the ring slot -- written here, node by node AFTER the node's history has been read, because
//                      with a full ring that slot is the oldest pair's
// Every sum has a fixed order that depends on N alone (per thread: channel, then node; wave: xor shuffles 32 .. 1; workgroup: (w0 + w1) +
// (w2 + w3); atom: chunk 0, 1, ...), there are no floating-point atomics, and every per-atom quantity is indexed by the atom: an atom's
// bits depend neither on the batch it is in nor on the run.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "internal.h"
#include "radial_device.h"

namespace {

constexpr int kGramThreads = 256;
constexpr int kGramPerThread = kAndersonChunk / kGramThreads;

// pairs of this step's accelerated mix: none while the atom warms up (the steps k <= warmup are the linear mix)
__device__ __forceinline__ int history_in_use(const int* __restrict__ st, int warmup) { return (st[2] + 1 <= warmup) ? 0 : st[1]; }

template <int H>
__device__ __forceinline__ void gram_chunk(int lsda, int N, int a, int chunk, int nchunks, int m, int head, double hstep,
                                           const double* __restrict__ fpr2, const double* __restrict__ cnst, double* __restrict__ newDensity,
                                           const double* __restrict__ density, const double* __restrict__ dA, const double* __restrict__ dB,
                                           const double* __restrict__ ring, double* __restrict__ slab, double* lds)
{
    constexpr int nA = H * (H + 1) / 2, nd = nA + H;
    double acc[nd > 0 ? nd : 1];
#pragma unroll
    for (int d = 0; d < nd; ++d) acc[d] = 0.;
    const int nch = lsda ? 2 : 1;
    for (int ch = 0; ch < nch; ++ch) {
        const size_t v = (size_t)nch * a + ch;                       // the potential index of this channel
        const double* __restrict__ xin = !lsda ? density : (ch ? dB : dA);
#pragma unroll
        for (int q = 0; q < kGramPerThread; ++q) {
            const int i = chunk * kAndersonChunk + q * kGramThreads + (int)threadIdx.x;
            if (i == 0 || i >= N) continue;                          // node 0 is excluded throughout, as in k_mix
            double g = newDensity[v * N + i];
            g /= fpr2[i];
            newDensity[v * N + i] = g;
            if (H == 0) continue;
            const double x = xin[(size_t)a * N + i];
            const double f = g - x;
            const double w = fpr2[i] * (cnst[i] * hstep);            // 4 pi r^2 dr/di
            double dF[H > 0 ? H : 1];
#pragma unroll
            for (int j = 0; j < H; ++j) {                            // oldest to newest
                const int slot = (head + m - H + j) % m;
                dF[j] = f - ring[((v * m + slot) * 2 + 1) * N + i];
            }
            int d = 0;
#pragma unroll
            for (int j = 0; j < H; ++j) {
                const double wj = w * dF[j];
#pragma unroll
                for (int k = j; k < H; ++k) acc[d++] += wj * dF[k];
                acc[nA + j] += wj * f;
            }
        }
    }
    if (H == 0) return;
#pragma unroll
    for (int d = 0; d < nd; ++d) {
        const double s = dfta_radial::wave_tree_sum(acc[d]);         // the tree of radial_device.h, per dot product
        if ((threadIdx.x & 63) == 0) lds[(threadIdx.x >> 6) * kAndersonDots + d] = s;
    }
    __syncthreads();
    if ((int)threadIdx.x < nd) {
        const int d = threadIdx.x;
        slab[((size_t)a * nchunks + chunk) * kAndersonDots + d] =
            dfta_radial::waves_join(lds[d], lds[kAndersonDots + d], lds[2 * kAndersonDots + d], lds[3 * kAndersonDots + d]);
    }
}

__global__ __launch_bounds__(kGramThreads) void k_anderson_gram(int lsda, int N, int m, int warmup, double hstep, const double* __restrict__ fpr2,
                                                                const double* __restrict__ cnst, double* __restrict__ newDensity,
                                                                const double* __restrict__ density, const double* __restrict__ dA,
                                                                const double* __restrict__ dB, const double* __restrict__ ring,
                                                                double* __restrict__ slab, const int* __restrict__ state, const int* __restrict__ fin)
{
    __shared__ double lds[(kGramThreads / 64) * kAndersonDots];
    const int a = blockIdx.y, chunk = blockIdx.x, nchunks = gridDim.x;
    if (fin[a]) return;                                              // a finished atom is frozen, its history untouched
    const int* __restrict__ st = state + (size_t)a * kAndersonStateInts;
    const int head = st[0], H = history_in_use(st, warmup);          // the same for every thread of the workgroup
#define DFTA_GRAM_CASE(h) \
    case h: gram_chunk<h>(lsda, N, a, chunk, nchunks, m, head, hstep, fpr2, cnst, newDensity, density, dA, dB, ring, slab, lds); break
    switch (H) {
        DFTA_GRAM_CASE(0); DFTA_GRAM_CASE(1); DFTA_GRAM_CASE(2); DFTA_GRAM_CASE(3); DFTA_GRAM_CASE(4);
        DFTA_GRAM_CASE(5); DFTA_GRAM_CASE(6); DFTA_GRAM_CASE(7); DFTA_GRAM_CASE(8);
    default: break;
    }
#undef DFTA_GRAM_CASE
}

// one wave per atom: lane d sums dot product d over the chunks, lane 0 solves
__global__ __launch_bounds__(64) void k_anderson_solve(int nchunks, int m, int warmup, const double* __restrict__ slab, double* __restrict__ gamma,
                                                       int* __restrict__ state, const int* __restrict__ fin)
{
    __shared__ double dots[kAndersonDots];
    const int a = blockIdx.x;
    if (fin[a]) return;
    int* __restrict__ st = state + (size_t)a * kAndersonStateInts;
    const int head = st[0], len = st[1], k = st[2] + 1, H = history_in_use(st, warmup);
    const int nA = H * (H + 1) / 2, nd = nA + H;
    if ((int)threadIdx.x < nd) {
        double s = 0.;
        for (int c = 0; c < nchunks; ++c) s += slab[((size_t)a * nchunks + c) * kAndersonDots + threadIdx.x];
        dots[threadIdx.x] = s;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    bool ok = H > 0;
    double L[kAndersonMaxHistory][kAndersonMaxHistory], y[kAndersonMaxHistory];
    if (ok) {
        double trace = 0.;
        for (int j = 0, d = 0; j < H; ++j)
            for (int i = j; i < H; ++i, ++d) {
                L[i][j] = dots[d];                                   // A's lower triangle (A is symmetric)
                if (i == j) trace += dots[d];
            }
        const double lambda = 1e-14 * trace;
        for (int j = 0; j < H; ++j) L[j][j] += lambda;
        for (int j = 0; j < H && ok; ++j) {                          // Cholesky, column by column, in place
            double p = L[j][j];
            for (int q = 0; q < j; ++q) p -= L[j][q] * L[j][q];
            if (!(p > 0.)) { ok = false; break; }                    // a pivot <= 0 (or a NaN)
            const double piv = sqrt(p);
            L[j][j] = piv;
            for (int i = j + 1; i < H; ++i) {
                double s = L[i][j];
                for (int q = 0; q < j; ++q) s -= L[i][q] * L[j][q];
                L[i][j] = s / piv;
            }
        }
    }
    if (ok) {
        for (int i = 0; i < H; ++i) {                                // L y = b
            double s = dots[nA + i];
            for (int q = 0; q < i; ++q) s -= L[i][q] * y[q];
            y[i] = s / L[i][i];
        }
        for (int i = H - 1; i >= 0; --i) {                           // L^T gamma = y
            double s = y[i];
            for (int q = i + 1; q < H; ++q) s -= L[q][i] * y[q];
            y[i] = s / L[i][i];
            ok = ok && isfinite(y[i]);
        }
    }
    double* __restrict__ gm = gamma + (size_t)a * kAndersonCoefDoubles;
    for (int j = 0; j < kAndersonMaxHistory; ++j) gm[j] = (ok && j < H) ? y[j] : 0.;
    st[3] = head;                                                    // this step, for k_anderson_update
    st[4] = ok ? H : 0;
    st[5] = ok ? 1 : 0;
    if (H > 0 && !ok) { st[0] = 0; st[1] = 0; }                      // a failed solve: linear step, the history is cleared (this step's pair too)
    else { st[0] = (head + 1) % m; st[1] = len < m ? len + 1 : m; }
    st[2] = k;
}

__device__ __forceinline__ double mixed(double alpha, double oneMinusAlpha, double x, double g, int N, int i, int m, int head, int H, int use,
                                        const double* __restrict__ gm, double* __restrict__ ringv /* the potential's m slots */)
{
    const double lin = alpha * x + oneMinusAlpha * g;                // k_mix's expression
    const double f = g - x;
    double out = lin;
    if (use) {
        double s = 0.;
        for (int j = 0; j < H; ++j) {                                // oldest to newest
            const int slot = (head + m - H + j) % m;
            const double xj = ringv[((size_t)slot * 2) * N + i], fj = ringv[((size_t)slot * 2 + 1) * N + i];
            s += gm[j] * ((x - xj) + oneMinusAlpha * (f - fj));
        }
        const double cand = lin - s;
        out = cand >= 0. ? cand : lin;
    }
    ringv[((size_t)head * 2) * N + i] = x;
    ringv[((size_t)head * 2 + 1) * N + i] = f;
    return out;
}

__global__ void k_anderson_update(int lsda, int N, int m, double alpha, double oneMinusAlpha, const double* __restrict__ newDensity,
                                  double* __restrict__ density, double* __restrict__ dA, double* __restrict__ dB, double* __restrict__ ring,
                                  const double* __restrict__ gamma, const int* __restrict__ state, const int* __restrict__ fin)
{
    const int a = blockIdx.y;
    if (fin[a]) return;
    const int* __restrict__ st = state + (size_t)a * kAndersonStateInts;
    const int head = st[3], H = st[4], use = st[5];
    const double* __restrict__ gm = gamma + (size_t)a * kAndersonCoefDoubles;
    const size_t slots = (size_t)m * 2 * N;                          // doubles of one potential's ring
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < N; i += gridDim.x * blockDim.x) {
        if (i == 0) continue;
        const size_t o = (size_t)a * N + i;
        if (!lsda) {
            density[o] = mixed(alpha, oneMinusAlpha, density[o], newDensity[o], N, i, m, head, H, use, gm, ring + (size_t)a * slots);
        } else {
            const size_t va = (size_t)2 * a, vb = (size_t)2 * a + 1;
            const double x = mixed(alpha, oneMinusAlpha, dA[o], newDensity[va * N + i], N, i, m, head, H, use, gm, ring + va * slots);
            const double y = mixed(alpha, oneMinusAlpha, dB[o], newDensity[vb * N + i], N, i, m, head, H, use, gm, ring + vb * slots);
            dA[o] = x;
            dB[o] = y;
            density[o] = x + y;
        }
    }
}

}  // namespace

int dfta_anderson_create(dfta_ctx* ctx, const dfta_grid* g, int natoms, int nspin, int history, int warmup, dfta_anderson* an)
{
    DFTA_REQUIRE(ctx, history >= 1 && history <= kAndersonMaxHistory && warmup >= 1, "Anderson mixing: history / warm-up");
    an->m = history;
    an->warmup = warmup;
    const size_t N = g->N, nV = (size_t)natoms * nspin;
    hipError_t e = an->ring.alloc(2 * (size_t)history * nV * N);
    if (e == hipSuccess) e = an->slab.alloc((size_t)natoms * dfta_anderson_chunks(g->N) * kAndersonDots);
    if (e == hipSuccess) e = an->gamma.alloc((size_t)natoms * kAndersonCoefDoubles);
    if (e == hipSuccess) e = an->state.alloc((size_t)natoms * kAndersonStateInts);
    if (e == hipSuccess) e = hipMemsetAsync(an->state, 0, sizeof(int) * natoms * kAndersonStateInts, ctx->stream);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        snprintf(ctx->err, sizeof(ctx->err), "Anderson mixing: %zu bytes of history: %s", 2 * (size_t)history * nV * N * sizeof(double), hipGetErrorString(e));
        return e == hipErrorOutOfMemory ? DFTA_ERR_NOMEM : DFTA_ERR_HIP;
    }
    return DFTA_OK;
}

int dfta_launch_anderson_mix(dfta_ctx* ctx, const dfta_grid* g, dfta_anderson* an, int lsda, int natoms, double alpha, double oneMinusAlpha,
                             double* newDensity, double* density, double* dA, double* dB, const int* fin)
{
    const int N = g->N, nchunks = dfta_anderson_chunks(N);
    hipStream_t st = ctx->stream;
    hipLaunchKernelGGL(k_anderson_gram, dim3(nchunks, natoms), dim3(kGramThreads), 0, st, lsda, N, an->m, an->warmup, dfta_hstep(g),
                       g->d_fpr2, g->d_cnst, newDensity, density, dA, dB, an->ring.p, an->slab.p, an->state.p, fin);
    DFTA_CHECK_LAUNCH(ctx);
    hipLaunchKernelGGL(k_anderson_solve, dim3(natoms), dim3(64), 0, st, nchunks, an->m, an->warmup, an->slab.p, an->gamma.p, an->state.p, fin);
    DFTA_CHECK_LAUNCH(ctx);
    hipLaunchKernelGGL(k_anderson_update, dim3(std::min(64, (N + 255) / 256), natoms), dim3(256), 0, st, lsda, N, an->m, alpha, oneMinusAlpha,
                       newDensity, density, dA, dB, an->ring.p, an->gamma.p, an->state.p, fin);
    DFTA_CHECK_LAUNCH(ctx);
    return DFTA_OK;
}

// ---- the mixing stage on its own (include/dftatom_hip.h: dfta_mixer) --------------------------------------------------------------
// No second implementation: a step uploads the caller's arrays into buffers laid out as dfta_scf's and calls the launch function
// dfta_scf_step calls for the same `mixing`.
struct dfta_mixer {
    dfta_ctx* ctx = nullptr;
    const dfta_grid* g = nullptr;
    int lsda = 0, natoms = 0, nspin = 1, mixing = DFTA_MIX_LINEAR;
    dfta_anderson anderson;
    DevBuf<double> newDensity, density, dA, dB;
    DevBuf<int> fin;
};

extern "C" {

void dfta_mixer_destroy(dfta_mixer* mx) { delete mx; }

int dfta_mixer_create(dfta_ctx* ctx, const dfta_grid* g, int lsda, int natoms, int mixing, int history, int warmup, dfta_mixer** out)
{
    if (!ctx || !g || !out) return DFTA_ERR_INVALID;
    DFTA_ENTER(ctx);
    DFTA_REQUIRE(ctx, natoms >= 1 && natoms <= 65535, "dfta_mixer_create: natoms");
    DFTA_REQUIRE(ctx, mixing == DFTA_MIX_LINEAR || mixing == DFTA_MIX_ANDERSON, "mixing (DFTA_MIX_LINEAR / DFTA_MIX_ANDERSON)");
    dfta_mixer* mx = new dfta_mixer();
    mx->ctx = ctx;
    mx->g = g;
    mx->lsda = lsda ? 1 : 0;
    mx->natoms = natoms;
    mx->nspin = lsda ? 2 : 1;
    mx->mixing = mixing;
    const size_t sz = (size_t)natoms * g->N;
    hipError_t e = mx->newDensity.alloc(sz * mx->nspin);
    if (e == hipSuccess) e = mx->density.alloc(sz);
    if (e == hipSuccess && lsda) e = mx->dA.alloc(sz);
    if (e == hipSuccess && lsda) e = mx->dB.alloc(sz);
    if (e == hipSuccess) e = mx->fin.alloc(natoms);
    int rc = DFTA_OK;
    if (e != hipSuccess) {
        (void)hipGetLastError();
        snprintf(ctx->err, sizeof(ctx->err), "dfta_mixer_create: %s", hipGetErrorString(e));
        rc = e == hipErrorOutOfMemory ? DFTA_ERR_NOMEM : DFTA_ERR_HIP;
    } else if (mixing == DFTA_MIX_ANDERSON) {
        rc = dfta_anderson_create(ctx, g, natoms, mx->nspin, history, warmup, &mx->anderson);
        if (rc == DFTA_OK && hipStreamSynchronize(ctx->stream) != hipSuccess) rc = DFTA_ERR_HIP;
    }
    if (rc) { delete mx; return rc; }
    *out = mx;
    return DFTA_OK;
}

int dfta_mixer_step(dfta_mixer* mx, double alpha, double* acc, double* density, double* dA, double* dB, const int* fin)
{
    if (!mx) return DFTA_ERR_INVALID;
    dfta_ctx* ctx = mx->ctx;
    DFTA_ENTER(ctx);
    DFTA_REQUIRE(ctx, acc && density && fin && (!mx->lsda || (dA && dB)), "dfta_mixer_step arguments");
    hipStream_t st = ctx->stream;
    const size_t row = sizeof(double) * (size_t)mx->natoms * mx->g->N;
    DFTA_HIP(ctx, hipMemcpyAsync(mx->newDensity.p, acc, row * mx->nspin, hipMemcpyHostToDevice, st));
    DFTA_HIP(ctx, hipMemcpyAsync(mx->density.p, density, row, hipMemcpyHostToDevice, st));
    if (mx->lsda) {
        DFTA_HIP(ctx, hipMemcpyAsync(mx->dA.p, dA, row, hipMemcpyHostToDevice, st));
        DFTA_HIP(ctx, hipMemcpyAsync(mx->dB.p, dB, row, hipMemcpyHostToDevice, st));
    }
    DFTA_HIP(ctx, hipMemcpyAsync(mx->fin.p, fin, sizeof(int) * mx->natoms, hipMemcpyHostToDevice, st));
    int rc;
    if (mx->mixing == DFTA_MIX_ANDERSON)
        rc = dfta_launch_anderson_mix(ctx, mx->g, &mx->anderson, mx->lsda, mx->natoms, alpha, 1. - alpha, mx->newDensity.p, mx->density.p, mx->dA.p,
                                      mx->dB.p, mx->fin.p);
    else
        rc = dfta_launch_linear_mix(ctx, mx->g, mx->lsda, mx->natoms, alpha, 1. - alpha, mx->newDensity.p, mx->density.p, mx->dA.p, mx->dB.p,
                                    mx->fin.p);
    if (rc) return rc;
    DFTA_HIP(ctx, hipMemcpyAsync(acc, mx->newDensity.p, row * mx->nspin, hipMemcpyDeviceToHost, st));
    DFTA_HIP(ctx, hipMemcpyAsync(density, mx->density.p, row, hipMemcpyDeviceToHost, st));
    if (mx->lsda) {
        DFTA_HIP(ctx, hipMemcpyAsync(dA, mx->dA.p, row, hipMemcpyDeviceToHost, st));
        DFTA_HIP(ctx, hipMemcpyAsync(dB, mx->dB.p, row, hipMemcpyDeviceToHost, st));
    }
    DFTA_HIP(ctx, hipStreamSynchronize(st));
    return DFTA_OK;
}

int dfta_mixer_get(dfta_mixer* mx, int atom, int* state, double* gamma, double* slab, double* ring)
{
    if (!mx) return DFTA_ERR_INVALID;
    dfta_ctx* ctx = mx->ctx;
    DFTA_ENTER(ctx);
    DFTA_REQUIRE(ctx, mx->mixing == DFTA_MIX_ANDERSON, "dfta_mixer_get: a DFTA_MIX_LINEAR mixer keeps no history");
    DFTA_REQUIRE(ctx, atom >= 0 && atom < mx->natoms, "dfta_mixer_get: atom");
    hipStream_t st = ctx->stream;
    const dfta_anderson& an = mx->anderson;
    const size_t a = atom, nslab = (size_t)dfta_anderson_chunks(mx->g->N) * kAndersonDots, nring = (size_t)mx->nspin * an.m * 2 * mx->g->N;
    if (state) DFTA_HIP(ctx, hipMemcpyAsync(state, an.state.p + a * kAndersonStateInts, sizeof(int) * kAndersonStateInts, hipMemcpyDeviceToHost, st));
    if (gamma) DFTA_HIP(ctx, hipMemcpyAsync(gamma, an.gamma.p + a * kAndersonCoefDoubles, sizeof(double) * kAndersonCoefDoubles, hipMemcpyDeviceToHost, st));
    if (slab) DFTA_HIP(ctx, hipMemcpyAsync(slab, an.slab.p + a * nslab, sizeof(double) * nslab, hipMemcpyDeviceToHost, st));
    if (ring) DFTA_HIP(ctx, hipMemcpyAsync(ring, an.ring.p + a * nring, sizeof(double) * nring, hipMemcpyDeviceToHost, st));
    DFTA_HIP(ctx, hipStreamSynchronize(st));
    return DFTA_OK;
}

}  // extern "C"
