// kb.hip -- radial solves with a Kleinman-Bylander (separable) pseudopotential: the outward Numerov sweep with a source term, the
// bound states of H_KB by the sign of u~_m(E) and the ghost-state report (include/dftatom_hip.h has the arithmetic and the search's
// formulas, DESIGN.md 4.16 the shape).  The first inhomogeneous radial solve of the library.
//
//   k_kb<ROWS>     one workgroup of ONE wave per block of 64 trials of a channel (local potential, l, projector, q1); one lane per
//                  trial, the lanes march the node index together, each with TWO chains: the homogeneous solution u_h (the
//                  arithmetic of k_continuum, start included) and the particular solution u_p of the source -beta, and the two
//                  projector sums <beta|u_h>, <beta|u_p> in the partner-sum shape of k_continuum.  What is the same in every lane
//                  -- vl_i, s_i^2, sqrt(s_i), the weighted beta_i, G_i and G_i / 12 -- is staged per tile of 256 nodes in LDS by
//                  the wave itself and read back as broadcasts.  ROWS: the raw q_i y_i of both chains, 32 nodes x 64 trials each,
//                  go through one padded LDS square so that each store instruction writes 32 consecutive nodes of a trial's u_h
//                  row and 32 of its u_p row.
//   k_kb_combine   rows: u~_i = (D u_h,i) + (B_h u_p,i) for 1 <= i <= m + 1, 0.0 elsewhere -- D and B_h are known only at m.
// A trial has its own registers and accumulators from start to end and reads only staged values that do not depend on the other
// lanes: its bits do not depend on the other trials, their number or order, ROWS, the chunking of the rows or the run.  No atomics;
// every result leaves through ordinary vector stores.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstring>
#include <limits>
#include <vector>

#include "internal.h"
#include "kb_plan.h"
#include "radial_device.h"

namespace {

using dfta_radial::simpson38_weight;
namespace kp = dfta_kb_plan;

constexpr int kTile = kp::kTile;
constexpr int kBlkInts = 5;                         // per block: potential row, channel, l, first position, trials
constexpr int kPad = 65;                            // row pitch of the transposition square

struct KbArgs {
    int N;
    double hstep, c, lam;
    const double *r, *cnst, *V, *beta;              // V: nV x N; beta: nch x N
    const double* q1;                               // per channel
    const int* blk;                                 // kBlkInts per block
    const double* E;                                // per padded position
    const int* m;                                   // ... (-1: padding)
    double *u, *du, *logderiv, *Bh, *Bp, *D;
    int* status;
    double* rows;                                   // ROWS: the chunk's raw chains, u_h rows then u_p rows, position - 64 block0 first
    size_t chunk_rows;                              // rows of a chain in the chunk's buffer
};

template <bool ROWS>
__global__ __launch_bounds__(64) void k_kb(KbArgs a, int block0)
{
    __shared__ double s_vl[kTile], s_s2[kTile], s_sq[kTile], s_gb[kTile], s_G[kTile], s_G12[kTile];
    __shared__ double s_t[ROWS ? 64 * kPad : 1];
    const int lane = threadIdx.x, b = blockIdx.x + block0, N = a.N;
    const int* __restrict__ bk = a.blk + (size_t)b * kBlkInts;
    const int ch = bk[1], l = bk[2], first = bk[3], cnt = bk[4];
    const double* __restrict__ V = a.V + (size_t)bk[0] * N;
    const double* __restrict__ beta = a.beta + (size_t)ch * N;
    const double L = (double)l * ((double)l + 1.);
    const bool mine = lane < cnt;
    const double E = mine ? a.E[first + lane] : 0.;
    const int m = mine ? a.m[first + lane] : -1;
    const int mend = m + 1;                          // the lane's last node (0: none)
    int wave_end = mend;
    for (int off = 32; off > 0; off >>= 1) wave_end = max(wave_end, __shfl_xor(wave_end, off));

    // the start of u_h: the fit at nodes 1 and 2 and the series' coefficients (k_continuum's)
    const double r1 = a.r[1], r2 = a.r[2], V1 = V[1], V2 = V[2];
    const double Zc = ((V2 - V1) * (r1 * r2)) / (r2 - r1);
    const double v0 = V1 + Zc / r1;
    double ak[5];
    ak[0] = 1.;
    ak[1] = -Zc / ((double)l + 1.);
#pragma unroll
    for (int k = 2; k <= 4; ++k) ak[k] = (((-2. * Zc) * ak[k - 1]) + ((2. * (v0 - E)) * ak[k - 2])) / (double)(k * (k + 2 * l + 1));
    // the start of u_p: B of beta = B r^(l+1) at node 1
    double p1 = r1;
    for (int q = 0; q < l; ++q) p1 = p1 * r1;
    const double twoB = 2. * (beta[1] / p1);
    const double lead = (double)(4 * l + 6);

    double wh1 = 0., wh2 = 0., yh1 = 0., wp1 = 0., wp2 = 0., yp1 = 0., f1 = 0., g1 = 0.;
    double yhm1 = 0., yhm = 0., yhp = 0., ypm1 = 0., ypm = 0., ypp = 0., fm1 = 0., fp = 0., gm1 = 0., gp = 0.;
    int status = 0;
    double toth = 0., totp = 0., bsh = 0., bsp = 0.;

    for (int tile0 = 0; tile0 <= wave_end; tile0 += kTile) {
        // stage what every lane shares at the tile's nodes
#pragma unroll
        for (int k = 0; k < kTile / 64; ++k) {
            const int j = lane + 64 * k, i = tile0 + j;
            double vl = 0., s2 = 1., sq = 1., gb = 0., G = 0.;
            if (i < N) {
                const double ri = a.r[i], si = a.cnst[i] * a.hstep, bi = beta[i];
                s2 = si * si;
                sq = sqrt(si);
                vl = V[i] + ((L / (ri * ri)) * 0.5);
                gb = simpson38_weight(i, N) * ((bi * 1.) * si);
                G = ((2. * bi) * si) * sq;
            }
            s_vl[j] = vl; s_s2[j] = s2; s_sq[j] = sq; s_gb[j] = gb; s_G[j] = G; s_G12[j] = G / 12.;
        }
        __syncthreads();
        bsh = 0.; bsp = 0.;
        for (int sub = 0; sub < kTile / 32; ++sub) {
            const int i0 = tile0 + 32 * sub;
            if (i0 > wave_end) break;
            for (int jj = 0; jj < 32; ++jj) {
                const int i = i0 + jj, j = 32 * sub + jj;
                const double vl = s_vl[j], s2 = s_s2[j], sq = s_sq[j], G = s_G[j], G12 = s_G12[j];
                const bool on = i >= 1 && i <= mend;
                const double f = (2. * (vl - E)) * s2 + a.c;
                const double d = 1. - f / 12.;
                double yh, wh, yp, wp;
                if (i <= 2) {                        // (the same in every lane)
                    const double ri = a.r[i];
                    double p = ri;
                    for (int q = 0; q < l; ++q) p = p * ri;
                    const double uh = p * ((((ak[4] * ri + ak[3]) * ri + ak[2]) * ri + ak[1]) * ri + ak[0]);
                    yh = uh / sq;
                    wh = d * yh;
                    const double up = ((twoB * p) * (ri * ri)) / lead;
                    yp = up / sq;
                    wp = d * yp - G12;
                } else {
                    wh = ((2. * wh1) - wh2) + f1 * yh1;
                    yh = wh / d;
                    wp = ((2. * wp1) - wp2) + (f1 * yp1 + g1);
                    yp = (wp + G12) / d;
                    if (on && !(d > 0.)) status |= DFTA_CONT_STEP;
                }
                if (on) {
                    if (!(fabs(yh) <= DBL_MAX) || !(fabs(yp) <= DBL_MAX)) status |= DFTA_CONT_NONFINITE;
                    if (i == m - 1) { yhm1 = yh; ypm1 = yp; fm1 = f; gm1 = G; }
                    if (i == m) { yhm = yh; ypm = yp; }
                    if (i == mend) { yhp = yh; ypp = yp; fp = f; gp = G; }
                    if (i <= m) {
                        const double gb = s_gb[j];
                        bsh += gb * (sq * yh);
                        bsp += gb * (sq * yp);
                    }
                    wh2 = wh1; wh1 = wh; yh1 = yh; wp2 = wp1; wp1 = wp; yp1 = yp; f1 = f;
                }
                g1 = G;
                if (ROWS) {
                    s_t[lane * kPad + jj] = on ? sq * yh : 0.;
                    s_t[lane * kPad + 32 + jj] = on ? sq * yp : 0.;
                }
            }
            if (ROWS) {
                __syncthreads();
                const int i = i0 + (lane & 31);
                double* __restrict__ dst = a.rows + ((size_t)(lane >> 5) * a.chunk_rows + (size_t)(b - block0) * 64) * N;
                if (i < N)
                    for (int tt = 0; tt < cnt; ++tt) dst[(size_t)tt * N + i] = s_t[tt * kPad + lane];
                __syncthreads();
            }
        }
        if (tile0 <= m) { toth = toth + bsh; totp = totp + bsp; }
        __syncthreads();
    }
    if (!mine) return;

    // the end node
    const double nan = __builtin_nan("");
    double u = nan, du = nan, logderiv = nan, Bh = nan, Bp = nan, D = nan;
    if (!(status & (DFTA_CONT_NONFINITE | DFTA_CONT_STEP))) {
        const double dyh = (((1. - fp / 6.) * yhp) - ((1. - fm1 / 6.) * yhm1)) * 0.5;
        const double dyp = ((((1. - fp / 6.) * ypp) - gp / 6.) - (((1. - fm1 / 6.) * ypm1) - gm1 / 6.)) * 0.5;
        const double qm = sqrt(a.cnst[m] * a.hstep);
        const double uh = qm * yhm, up = qm * ypm;
        const double duh = (dyh + (a.lam * 0.5) * yhm) / qm;
        const double dup = (dyp + (a.lam * 0.5) * ypm) / qm;
        Bh = dfta_radial::simpson38_finish(toth);
        Bp = dfta_radial::simpson38_finish(totp);
        D = a.q1[ch] - Bp;
        u = (D * uh) + (Bh * up);
        du = (D * duh) + (Bh * dup);
        logderiv = du / u;
    }
    const size_t pos = (size_t)first + lane;
    a.u[pos] = u; a.du[pos] = du; a.logderiv[pos] = logderiv;
    a.Bh[pos] = Bh; a.Bp[pos] = Bp; a.D[pos] = D;
    a.status[pos] = status;
}

// rows of a chunk: positions from pos0 on; one row per blockIdx.y; rows: the u_h rows, combined in place; rows + chunk_rows N: the u_p rows
__global__ __launch_bounds__(256) void k_kb_combine(int N, size_t pos0, size_t chunk_rows, const int* __restrict__ m, const double* __restrict__ D,
                                                    const double* __restrict__ Bh, double* __restrict__ rows)
{
    const size_t pos = pos0 + blockIdx.y;
    const int mt = m[pos];
    if (mt < 0) return;                              // padding
    const double Dt = D[pos], Bt = Bh[pos];          // NaN with a status bit
    double* __restrict__ rh = rows + (size_t)blockIdx.y * N;
    const double* __restrict__ rp = rows + (chunk_rows + blockIdx.y) * (size_t)N;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < N; i += gridDim.x * blockDim.x)
        rh[i] = (i >= 1 && i <= mt + 1) ? (Dt * rh[i]) + (Bt * rp[i]) : 0.;
}

struct KbOut {
    double *u, *du, *logderiv, *Bh, *Bp, *D;
    int* status;
    double* rows;                                   // ntrials x N
};

// the sweeps of a validated call on potentials dV (nV x N) and projectors dBeta (nch x N) that are on the device; the call's arrays and
// every output are host pointers (any output may be null).  timed: the events of dfta_ctx_last_kernel_ms bracket the launches
int kb_run(dfta_ctx* ctx, const dfta_grid* g, const kp::Call& c, const double* dV, const double* dBeta, const double* dQ1, const KbOut& out,
           bool timed)
{
    if (c.ntrials <= 0) return DFTA_OK;
    int force = 0;
    if (const char* v = dfta_knob("KB_CHUNK_WAVES")) force = atoi(v);
    const kp::Plan plan = kp::plan(c, out.rows != nullptr, force);
    const size_t N = (size_t)g->N, npos = plan.order.size();
    const int nblocks = (int)plan.blocks.size();
    hipStream_t st = ctx->stream;

    std::vector<double> hE(npos, 0.);
    std::vector<int> hm(npos, -1), hblk((size_t)nblocks * kBlkInts, 0);
    for (size_t p = 0; p < npos; ++p)
        if (plan.order[p] >= 0) { hE[p] = c.E[plan.order[p]]; hm[p] = c.m[plan.order[p]]; }
    for (int b = 0; b < nblocks; ++b) {
        const kp::Block& bl = plan.blocks[b];
        int* bk = &hblk[(size_t)b * kBlkInts];
        bk[0] = c.vidx ? c.vidx[bl.chan] : 0; bk[1] = bl.chan; bk[2] = c.l[bl.chan]; bk[3] = bl.first; bk[4] = bl.cnt;
    }
    DevBuf<double> dE, dRes, dRows;
    DevBuf<int> dM, dBlk, dStatus;
    if (const int rc = dfta_upload_rows(ctx, hE.data(), npos, &dE)) return rc;
    if (const int rc = dfta_upload_rows(ctx, hm.data(), npos, &dM)) return rc;
    if (const int rc = dfta_upload_rows(ctx, hblk.data(), hblk.size(), &dBlk)) return rc;
    DFTA_HIP(ctx, dRes.alloc(6 * npos));
    DFTA_HIP(ctx, dStatus.alloc(npos));
    const int per_chunk = out.rows ? plan.blocks_per_chunk : nblocks;
    const size_t chunk_rows = (size_t)per_chunk * 64;
    if (out.rows) DFTA_HIP(ctx, dRows.alloc(2 * chunk_rows * N));

    KbArgs a;
    a.N = g->N;
    a.hstep = dfta_hstep(g);
    a.c = g->uniform ? 0. : g->delta2p4;
    a.lam = g->uniform ? 0. : g->delta;
    a.r = g->d_r.p; a.cnst = g->d_cnst.p; a.V = dV; a.beta = dBeta; a.q1 = dQ1;
    a.blk = dBlk.p; a.E = dE.p; a.m = dM.p;
    a.u = dRes.p; a.du = dRes.p + npos; a.logderiv = dRes.p + 2 * npos; a.Bh = dRes.p + 3 * npos; a.Bp = dRes.p + 4 * npos;
    a.D = dRes.p + 5 * npos;
    a.status = dStatus.p; a.rows = dRows.p; a.chunk_rows = chunk_rows;

    std::vector<double> stage;
    if (timed) DFTA_HIP(ctx, dfta_timer_start(ctx));
    for (int block0 = 0; block0 < nblocks; block0 += per_chunk) {
        const int nb = std::min(per_chunk, nblocks - block0);
        if (out.rows) hipLaunchKernelGGL(k_kb<true>, dim3(nb), dim3(64), 0, st, a, block0);
        else hipLaunchKernelGGL(k_kb<false>, dim3(nb), dim3(64), 0, st, a, block0);
        DFTA_CHECK_LAUNCH(ctx);
        if (!out.rows) continue;
        const unsigned gx = (unsigned)std::min<size_t>((N + 255) / 256, 64);
        hipLaunchKernelGGL(k_kb_combine, dim3(gx, (unsigned)nb * 64), dim3(256), 0, st, g->N, (size_t)block0 * 64, chunk_rows, dM.p, a.D, a.Bh,
                           dRows.p);
        DFTA_CHECK_LAUNCH(ctx);
        if (timed && block0 + nb >= nblocks) DFTA_HIP(ctx, dfta_timer_stop(ctx));      // the events bracket every launch (and the chunks' copies between them)
        stage.resize((size_t)nb * 64 * N);
        DFTA_HIP(ctx, hipMemcpyAsync(stage.data(), dRows.p, sizeof(double) * stage.size(), hipMemcpyDeviceToHost, st));
        DFTA_HIP(ctx, hipStreamSynchronize(st));
        for (size_t p = 0; p < (size_t)nb * 64; ++p) {
            const int t = plan.order[(size_t)block0 * 64 + p];
            if (t >= 0) memcpy(out.rows + (size_t)t * N, stage.data() + p * N, sizeof(double) * N);
        }
    }
    if (timed && !out.rows) DFTA_HIP(ctx, dfta_timer_stop(ctx));

    std::vector<double> h(6 * npos);
    std::vector<int> hs(npos);
    DFTA_HIP(ctx, hipMemcpyAsync(h.data(), dRes.p, sizeof(double) * h.size(), hipMemcpyDeviceToHost, st));
    DFTA_HIP(ctx, hipMemcpyAsync(hs.data(), dStatus.p, sizeof(int) * npos, hipMemcpyDeviceToHost, st));
    DFTA_HIP(ctx, hipStreamSynchronize(st));
    double* const dst[6] = {out.u, out.du, out.logderiv, out.Bh, out.Bp, out.D};
    for (size_t p = 0; p < npos; ++p) {
        const int t = plan.order[p];
        if (t < 0) continue;
        for (int q = 0; q < 6; ++q)
            if (dst[q]) dst[q][t] = h[(size_t)q * npos + p];
        if (out.status) out.status[t] = hs[p];
    }
    return DFTA_OK;
}

// the channels of a call on the device
struct KbChannels {
    DevBuf<double> dV, dBeta, dQ1;
    std::vector<int> lastnz;
    int upload(dfta_ctx* ctx, const dfta_grid* g, int nV, const double* V, int nch, const double* beta, const double* q1)
    {
        lastnz = kp::last_nonzero(nch, g->N, beta);
        if (const int rc = dfta_upload_rows(ctx, V, (size_t)nV * g->N, &dV)) return rc;
        if (const int rc = dfta_upload_rows(ctx, beta, (size_t)nch * g->N, &dBeta)) return rc;
        return dfta_upload_rows(ctx, q1, (size_t)nch, &dQ1);
    }
};

}  // namespace

extern "C" {

int dfta_kb_sweep(dfta_ctx* ctx, const dfta_grid* g, int nV, const double* V, int nch, const int* vidx, const int* l, const double* beta,
                  const double* q1, int ntrials, const int* chan, const double* E, const int* m, double* u, double* du, double* logderiv,
                  double* Bh, double* Bp, double* D, int* status, double* rows)
{
    if (!ctx || !g) return DFTA_ERR_INVALID;
    DFTA_ENTER(ctx);
    DFTA_REQUIRE(ctx, ntrials >= 0, "dfta_kb_sweep: ntrials");
    if (ntrials == 0) return DFTA_OK;
    DFTA_REQUIRE(ctx, V && l && beta && q1 && E && m, "dfta_kb_sweep arguments");
    DFTA_REQUIRE(ctx, nV >= 1 && nch >= 1, "dfta_kb_sweep: nV, nch");
    kp::Call c;
    c.N = g->N; c.nV = nV; c.nch = nch; c.ntrials = ntrials;
    c.vidx = vidx; c.l = l; c.beta = beta; c.q1 = q1; c.chan = chan; c.E = E; c.m = m;
    KbChannels chn;
    chn.lastnz = kp::last_nonzero(nch, g->N, beta);
    if (const char* msg = kp::check(c, chn.lastnz)) DFTA_REQUIRE(ctx, false, msg);
    if (const int rc = chn.upload(ctx, g, nV, V, nch, beta, q1)) return rc;
    KbOut out;
    out.u = u; out.du = du; out.logderiv = logderiv; out.Bh = Bh; out.Bp = Bp; out.D = D; out.status = status; out.rows = rows;
    return kb_run(ctx, g, c, chn.dV.p, chn.dBeta.p, chn.dQ1.p, out, true);
}

int dfta_kb_bound_states(dfta_ctx* ctx, const dfta_grid* g, int nV, const double* V, int nch, const int* vidx, const int* l,
                         const double* beta, const double* q1, const int* m, const double* E_lo, const double* E_hi, int nscan, int* count,
                         double* energies, int* rounds, int* status)
{
    if (!ctx || !g) return DFTA_ERR_INVALID;
    DFTA_ENTER(ctx);
    DFTA_REQUIRE(ctx, nch >= 0, "dfta_kb_bound_states: nch");
    if (nch == 0) return DFTA_OK;
    DFTA_REQUIRE(ctx, V && l && beta && q1 && m && E_lo && E_hi, "dfta_kb_bound_states arguments");
    DFTA_REQUIRE(ctx, nV >= 1, "dfta_kb_bound_states: nV");
    DFTA_REQUIRE(ctx, nscan >= 64 && nscan % 64 == 0 && nscan <= 65536, "dfta_kb_bound_states: nscan must be a multiple of 64 in 64 .. 65536");
    std::vector<kp::SearchChannel> chs((size_t)nch);
    std::vector<int> tc((size_t)nch), tm((size_t)nch);
    std::vector<double> tE((size_t)nch);
    for (int k = 0; k < nch; ++k) {
        DFTA_REQUIRE(ctx, std::isfinite(E_lo[k]) && std::isfinite(E_hi[k]) && E_lo[k] < E_hi[k], "dfta_kb_bound_states: E_lo < E_hi, both finite");
        chs[k].m = m[k]; chs[k].lo = E_lo[k]; chs[k].hi = E_hi[k];
        tc[k] = k; tm[k] = m[k]; tE[k] = E_lo[k];
    }
    kp::Call c;                                      // one trial per channel: the checks of the sweep
    c.N = g->N; c.nV = nV; c.nch = nch; c.ntrials = nch;
    c.vidx = vidx; c.l = l; c.beta = beta; c.q1 = q1; c.chan = tc.data(); c.E = tE.data(); c.m = tm.data();
    KbChannels chn;
    chn.lastnz = kp::last_nonzero(nch, g->N, beta);
    if (const char* msg = kp::check(c, chn.lastnz)) DFTA_REQUIRE(ctx, false, msg);
    if (const int rc = chn.upload(ctx, g, nV, V, nch, beta, q1)) return rc;

    const kp::Evaluate evaluate = [&](const std::vector<int>& chan, const std::vector<double>& E, const std::vector<int>& mm, std::vector<double>* u,
                                      std::vector<int>* st) -> int {
        kp::Call cc = c;
        cc.ntrials = (int)chan.size(); cc.chan = chan.data(); cc.E = E.data(); cc.m = mm.data();
        u->assign(chan.size(), 0.); st->assign(chan.size(), 0);
        KbOut out = {};
        out.u = u->data(); out.status = st->data();
        return kb_run(ctx, g, cc, chn.dV.p, chn.dBeta.p, chn.dQ1.p, out, false);
    };
    kp::SearchResult res;
    DFTA_HIP(ctx, dfta_timer_start(ctx));            // the events bracket the whole search: its launches and the host's work between them
    if (const int rc = kp::search(chs, nscan, evaluate, &res)) return rc;
    DFTA_HIP(ctx, dfta_timer_stop(ctx));
    DFTA_HIP(ctx, hipStreamSynchronize(ctx->stream));
    for (int k = 0; k < nch; ++k) {
        if (count) count[k] = res.count[k];
        if (rounds) rounds[k] = res.rounds[k];
        if (status) status[k] = res.status[k];
        if (energies)
            for (int q = 0; q < kp::kMaxStates; ++q) energies[(size_t)k * kp::kMaxStates + q] = res.energies[(size_t)k * kp::kMaxStates + q];
    }
    return DFTA_OK;
}

int dfta_kb_ghost_report(dfta_ctx* ctx, const dfta_grid* g, int natoms, int nch, const int* atom, const int* l, const double* eps,
                         const double* V_ps, const double* beta, const double* kb, const int* l_loc, int m, double E_lo, double E_hi,
                         int nscan, double tol, double* report, double* states)
{
    if (!ctx || !g) return DFTA_ERR_INVALID;
    DFTA_ENTER(ctx);
    DFTA_REQUIRE(ctx, nch >= 0 && natoms >= 0, "dfta_kb_ghost_report: natoms, nch");
    if (nch == 0) return DFTA_OK;
    DFTA_REQUIRE(ctx, atom && l && eps && V_ps && beta && kb && report, "dfta_kb_ghost_report arguments");
    DFTA_REQUIRE(ctx, std::isfinite(tol) && tol >= 0., "dfta_kb_ghost_report: tol");
    DFTA_REQUIRE(ctx, !std::isinf(E_lo) && std::isfinite(E_hi), "dfta_kb_ghost_report: E_lo, E_hi");
    const int N = g->N;
    const double nan = std::numeric_limits<double>::quiet_NaN();
    // the local channel of every atom: pseudo_ionic's rule
    std::vector<int> loc((size_t)natoms, -1);
    for (int k = 0; k < nch; ++k) {
        DFTA_REQUIRE(ctx, atom[k] >= 0 && atom[k] < natoms, "dfta_kb_ghost_report: an atom index out of range");
        DFTA_REQUIRE(ctx, l[k] >= 0 && l[k] <= kp::kLmax, "dfta_kb_ghost_report: l outside 0 .. 4");
    }
    for (int a = 0; a < natoms; ++a) {
        const int want = l_loc ? l_loc[a] : -1;
        for (int k = 0; k < nch; ++k) {
            if (atom[k] != a) continue;
            if (want >= 0 ? (l[k] == want && loc[a] < 0) : (loc[a] < 0 || l[k] > l[loc[a]])) loc[a] = k;
        }
    }
    // the non-local channels
    std::vector<int> nl, vidx, ll, mm;
    std::vector<double> q1, lo, hi;
    for (int k = 0; k < nch; ++k) {
        const int a = atom[k];
        DFTA_REQUIRE(ctx, loc[a] >= 0, "dfta_kb_ghost_report: an atom without a channel of its l_loc");
        if (k == loc[a]) continue;
        if (!std::isfinite(kb[3 * k]) || kb[3 * k] == 0.) continue;     // a channel that was not pseudized: its report stays NaN
        nl.push_back(k); vidx.push_back(loc[a]); ll.push_back(l[k]); mm.push_back(m); q1.push_back(kb[3 * k]);
        double bound = E_lo;                         // NaN: no state of H_KB lies below min vl_i - max(0, -E_KB) (the projector's norm is |E_KB|)
        if (std::isnan(E_lo)) {
            const double* Vl = V_ps + (size_t)loc[a] * N;
            const double L = (double)l[k] * ((double)l[k] + 1.);
            bound = std::numeric_limits<double>::infinity();
            for (int i = 1; i < N; ++i) bound = std::min(bound, Vl[i] + ((L / (g->h_r[i] * g->h_r[i])) * 0.5));
            bound = bound - std::max(0., -kb[3 * k + 2]);
        }
        DFTA_REQUIRE(ctx, std::isfinite(bound) && bound < std::min(0., E_hi), "dfta_kb_ghost_report: no energy range below min(0, E_hi)");
        lo.push_back(bound); hi.push_back(std::min(0., E_hi));
    }
    for (int k = 0; k < nch; ++k) {
        double* rp = report + (size_t)k * DFTA_KB_REPORT;
        for (int q = 0; q < DFTA_KB_REPORT; ++q) rp[q] = nan;
        rp[0] = eps[k]; rp[1] = kb[3 * k + 2];
        if (states)
            for (int q = 0; q < kp::kMaxStates; ++q) states[(size_t)k * kp::kMaxStates + q] = nan;
    }
    const int nnl = (int)nl.size();
    if (nnl == 0) return DFTA_OK;
    std::vector<double> b((size_t)nnl * N);
    for (int j = 0; j < nnl; ++j) memcpy(&b[(size_t)j * N], beta + (size_t)nl[j] * N, sizeof(double) * N);
    std::vector<int> count((size_t)nnl), rounds((size_t)nnl), sstat((size_t)nnl);
    std::vector<double> en((size_t)nnl * kp::kMaxStates);
    if (const int rc = dfta_kb_bound_states(ctx, g, nch, V_ps, nnl, vidx.data(), ll.data(), b.data(), q1.data(), mm.data(), lo.data(), hi.data(),
                                            nscan, count.data(), en.data(), rounds.data(), sstat.data()))
        return rc;
    // the two lowest levels of the local potential at the channel's l (l <= 3: the level search's tables end there)
    std::vector<int> lv_of, lv_v, lv_n, lv_l, lv_occ;
    for (int j = 0; j < nnl; ++j) {
        if (ll[j] > 3) continue;
        for (int q = 0; q < 2; ++q) { lv_of.push_back(2 * j + q); lv_v.push_back(vidx[j]); lv_n.push_back(ll[j] + q); lv_l.push_back(ll[j]); lv_occ.push_back(1); }
    }
    std::vector<double> eloc((size_t)2 * nnl, nan);
    if (!lv_of.empty()) {
        std::vector<double> bottom((size_t)nch, 0.);
        for (int k = 0; k < nch; ++k) {
            double mn = V_ps[(size_t)k * N + 1];
            for (int i = 1; i < N; ++i) mn = std::min(mn, V_ps[(size_t)k * N + i]);
            bottom[k] = mn - 1.;
        }
        std::vector<dfta_level_result> res(lv_of.size());
        long issued = 0;
        const int rc = dfta_solve_levels(ctx, g, DFTA_LEVELS_BATCHED, 0, nch, V_ps, bottom.data(), nullptr, (int)lv_of.size(), lv_v.data(),
                                         lv_n.data(), lv_l.data(), lv_occ.data(), res.data(), nullptr, nullptr, nullptr, &issued);
        if (rc != DFTA_OK && rc != DFTA_ERR_NOT_CONVERGED) return rc;
        for (size_t q = 0; q < lv_of.size(); ++q)
            if (res[q].converged && std::isfinite(res[q].E) && res[q].E < 0.) eloc[lv_of[q]] = res[q].E;      // not found: absent
    }
    for (int j = 0; j < nnl; ++j) {
        double* rp = report + (size_t)nl[j] * DFTA_KB_REPORT;
        const double eref = rp[0], ekb = rp[1];
        int ghosts = 0;
        for (int q = 0; q < count[j]; ++q) ghosts += en[(size_t)j * kp::kMaxStates + q] < eref - tol;
        rp[2] = count[j]; rp[3] = ghosts; rp[4] = eloc[2 * j]; rp[5] = eloc[2 * j + 1];
        rp[6] = ll[j] > 3 ? nan : (ekb > 0. ? (eloc[2 * j + 1] < eref ? 1. : 0.) : (ekb < 0. ? (eloc[2 * j] < eref ? 1. : 0.) : nan));
        rp[7] = ghosts > 0 ? 1. : 0.;
        rp[8] = sstat[j]; rp[9] = rounds[j];
        if (states)
            for (int q = 0; q < kp::kMaxStates; ++q) states[(size_t)nl[j] * kp::kMaxStates + q] = en[(size_t)j * kp::kMaxStates + q];
    }
    return DFTA_OK;
}

}  // extern "C"
