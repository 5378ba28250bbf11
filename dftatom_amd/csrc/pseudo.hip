// pseudo.hip -- Troullier-Martins norm-conserving pseudization of valence orbitals (include/dftatom_hip.h has the arithmetic, DESIGN.md
// 4.15 the shape and the rounding bounds).  Beyond the reference, which generates no pseudopotentials.
//
//   k_pseudize   one workgroup of 256 lanes per channel, every channel of a call in one launch.  Inside the kernel: the check of the
//                channel's rows and the last sign change of u (one pass over its N nodes), the five matching values at the core node
//                (every lane forms them, from the same ten loads), the all-electron norm, the root search in a2 -- each evaluation the
//                5 x 5 solve in every lane, a pass over the tiles of 1024 nodes up to the core node and one tree sum -- and the write
//                of u_ps and V_ps.  Every branch on the search's state is uniform over the workgroup: every lane holds the same
//                coefficients and the same bracket.
// The integrand of a tile of 1024 nodes goes through LDS with a halo of two nodes below and one above (the increment of node i reads
// i-2 .. i+1); lane t adds the increments of the nodes t, t + 256, ... in order, then the tree of radial_device.h.  No atomics, no workgroup waits for
// another, and a channel reads only its own rows: its bits do not depend on the other channels, their number or order, or the run.
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cmath>
#include <vector>

#include "internal.h"
#include "pseudo_plan.h"
#include "radial_device.h"
#include "xc.h"

namespace {

namespace pp = dfta_pseudo_plan;
using namespace dfta_radial;

constexpr int kLanes = pp::kLanes;
constexpr int kTile = 4 * kLanes;                    // nodes of the integrand in LDS between two barriers: four per lane
constexpr int kCoef = pp::kCoef;
constexpr int kMatch = pp::kMatch;

struct PseudoArgs {
    int N;
    double hstep, lam;
    const double *r, *cnst;
    const double *V, *U;                             // rows of N
    const int *vrow, *urow;                          // per channel, the row of V and of U that it reads (null: its own number)
    const int *l, *ic;
    const double* eps;
    double *ups, *vps;                               // nch x N each, may be null
    double *coef, *rc, *match;                       // nch x 7, nch, nch x 8
    int *iters, *status;
};

__device__ __forceinline__ int sign_of(double g) { return g > 0. ? 1 : (g < 0. ? -1 : 0); }

// the 5 x 5 system of the header: unknowns (a0, a6, a8, a10, a12), right-hand side b; Gaussian elimination with partial pivoting
// (the first row of largest magnitude in the column), then back substitution -- c[0], c[3] .. c[6] are written
__device__ __forceinline__ void solve5(const double (&b)[5], double (&c)[kCoef])
{
    double A[5][6] = {{1., 1., 1., 1., 1., b[0]},
                      {0., 6., 8., 10., 12., b[1]},
                      {0., 30., 56., 90., 132., b[2]},
                      {0., 120., 336., 720., 1320., b[3]},
                      {0., 360., 1680., 5040., 11880., b[4]}};
#pragma unroll
    for (int k = 0; k < 5; ++k) {
#pragma unroll
        for (int i = k + 1; i < 5; ++i) {            // a larger entry further down comes up: rows k and i change places
            const bool sw = fabs(A[i][k]) > fabs(A[k][k]);
#pragma unroll
            for (int j = k; j < 6; ++j) {
                const double t = A[k][j];
                A[k][j] = sw ? A[i][j] : t;
                A[i][j] = sw ? t : A[i][j];
            }
        }
#pragma unroll
        for (int i = k + 1; i < 5; ++i) {
            const double m = A[i][k] / A[k][k];
#pragma unroll
            for (int j = k + 1; j < 6; ++j) A[i][j] = A[i][j] - m * A[k][j];
        }
    }
    double x[5];
#pragma unroll
    for (int k = 4; k >= 0; --k) {
        double t = A[k][5];
#pragma unroll
        for (int j = k + 1; j < 5; ++j) t = t - A[k][j] * x[j];
        x[k] = t / A[k][k];
    }
    c[0] = x[0]; c[3] = x[1]; c[4] = x[2]; c[5] = x[3]; c[6] = x[4];
}

// the coefficients of a trial a2 from the five matching values P
__device__ __forceinline__ void coefficients(double a2, double lfive, const double (&P)[5], double (&c)[kCoef])
{
    const double a4 = -((a2 * a2) / lfive);
    const double b[5] = {P[0] - (a2 + a4), P[1] - (2. * a2 + 4. * a4), P[2] - (2. * a2 + 12. * a4), P[3] - 24. * a4, P[4] - 24. * a4};
    c[1] = a2; c[2] = a4;
    solve5(b, c);
}

// u_ps at a node inside the core: r^(l+1) exp(p(x)), x = r / r_c through the one reciprocal rinv
__device__ __forceinline__ double pseudo_u(double ri, double rinv, int l, const double (&c)[kCoef])
{
    const double x = ri * rinv, t = x * x;
    const double p = c[0] + t * (c[1] + t * (c[2] + t * (c[3] + t * (c[4] + t * (c[5] + t * c[6])))));
    double rp = ri;
    for (int q = 0; q < l; ++q) rp = rp * ri;
    return rp * exp(p);
}

__global__ __launch_bounds__(kLanes) void k_pseudize(PseudoArgs a)
{
    __shared__ double s_f[kTile + 3];                // slot k: node tile0 - 2 + k
    __shared__ double s_red[kLanes / 64];
    __shared__ int s_last[kLanes / 64];
    const int tid = threadIdx.x, ch = blockIdx.x, N = a.N;
    const double* __restrict__ V = a.V + (size_t)(a.vrow ? a.vrow[ch] : ch) * N;
    const double* __restrict__ U = a.U + (size_t)(a.urow ? a.urow[ch] : ch) * N;
    const int l = a.l[ch], ic = a.ic[ch];
    const double eps = a.eps[ch];
    const double nan = __builtin_nan("");
    int status = 0, iters = 0;

    // the rows: finite everywhere, and the last sign change of u
    int bad = !(fabs(eps) <= DBL_MAX), last = 0;
    for (int i = tid; i < N; i += kLanes) {
        const double ui = U[i], vi = V[i];
        bad |= !(fabs(ui) <= DBL_MAX) || !(fabs(vi) <= DBL_MAX);
        if (i >= 2) {
            const double u1 = U[i - 1], um = u1 != 0. ? u1 : U[i - 2];      // (through one exact zero)
            if ((ui < 0. && um > 0.) || (ui > 0. && um < 0.)) last = i;
        }
    }
    for (int off = 32; off > 0; off >>= 1) last = max(last, __shfl_xor(last, off));
    if ((tid & 63) == 0) s_last[tid >> 6] = last;
    bad = __syncthreads_or(bad);
    last = max(max(s_last[0], s_last[1]), max(s_last[2], s_last[3]));
    const double uc = U[ic];
    if (bad) status |= DFTA_PS_NONFINITE;
    else if (ic <= last || uc == 0.) status |= DFTA_PS_NODES;

    double c[kCoef] = {nan, nan, nan, nan, nan, nan, nan}, P[5] = {nan, nan, nan, nan, nan};
    double rc = nan, IAE = nan, Ips = nan, g = nan, sigma = 1., rinv = 0.;

    // g's integral over the nodes 1 .. ic: `ps` the pseudo-orbital below ic, otherwise u itself
    auto norm = [&](bool ps) -> double {
        double acc = 0.;
        for (int tile0 = 0; tile0 <= ic; tile0 += kTile) {
            for (int k = tid; k < kTile + 3; k += kLanes) {
                const int i = tile0 - 2 + k;
                double f = 0.;
                if (i >= 0 && i <= ic + 1) {
                    const double ui = (ps && i < ic) ? pseudo_u(a.r[i], rinv, l, c) : U[i];
                    f = (ui * ui) * (a.cnst[i] * a.hstep);
                }
                s_f[k] = f;
            }
            __syncthreads();
#pragma unroll
            for (int q = 0; q < kTile / kLanes; ++q) {   // the lane's nodes in ascending order: the sum's shape does not depend on kTile
                const int j = tid + q * kLanes, i = tile0 + j;
                if (i >= 1 && i <= ic) acc += increment(s_f, j + 2, i, N);
            }
            __syncthreads();
        }
        const double w = wave_tree_sum(acc);
        if ((tid & 63) == 0) s_red[tid >> 6] = w;
        __syncthreads();
        return waves_join(s_red[0], s_red[1], s_red[2], s_red[3]);
    };

    if (!status) {
        sigma = uc > 0. ? 1. : -1.;
        rc = a.r[ic];
        rinv = 1. / rc;
        const double lp = (double)l + 1., lfive = (double)(2 * l + 5);
        const double s = a.cnst[ic] * a.hstep, s2 = s * s;
        const double um2 = sigma * U[ic - 2], um1 = sigma * U[ic - 1], u0 = sigma * uc, up1 = sigma * U[ic + 1], up2 = sigma * U[ic + 2];
        const double vm2 = V[ic - 2], vm1 = V[ic - 1], v0 = V[ic], vp1 = V[ic + 1], vp2 = V[ic + 2];
        const double du = ((8. * (up1 - um1) - (up2 - um2)) / 12.) / s;
        const double dvi = (8. * (vp1 - vm1) - (vp2 - vm2)) / 12.;
        const double d2vi = ((16. * (vp1 + vm1) - (vp2 + vm2)) - 30. * v0) / 12.;
        const double dv = dvi / s, d2v = (d2vi - a.lam * dvi) / s2;
        double rcp = rc;
        for (int q = 0; q < l; ++q) rcp = rcp * rc;
        const double rc2 = rc * rc, rc3 = rc2 * rc, rc4 = rc2 * rc2, tl = 2. * lp, fl = 4. * lp;
        const double p0 = log(u0 / rcp);
        const double p1 = du / u0 - lp / rc;
        const double p2 = ((2. * (v0 - eps)) - (tl * p1) / rc) - p1 * p1;
        const double p3 = (((2. * dv) + (tl * p1) / rc2) - (tl * p2) / rc) - (2. * p1) * p2;
        const double p4 = ((((2. * d2v) - (fl * p1) / rc3) + (fl * p2) / rc2) - (tl * p3) / rc) - (2. * (p2 * p2) + (2. * p1) * p3);
        P[0] = p0; P[1] = p1 * rc; P[2] = p2 * rc2; P[3] = p3 * rc3; P[4] = p4 * rc4;

        IAE = norm(false);
        const double lnAE = log(IAE);
        auto eval = [&](double a2) -> double {
            ++iters;
            coefficients(a2, lfive, P, c);
            Ips = norm(true);
            return log(Ips) - lnAE;
        };

        // the bracket: from a2 = 0 outwards, +h then -h, h = 1/4, 1/2, 1, ...
        // lo keeps the sign of g(0), hi has the other sign or g = 0
        double lo = 0., glo = eval(0.), hi = 0., ghi = glo;
        const int s0 = sign_of(glo);
        if (glo != glo) status |= DFTA_PS_NOBRACKET;
        if (s0 != 0 && !status) {
            bool found = false;
            double ap = 0., gp = glo, am = 0., gm = glo, h = 0.25;
            for (int k = 0; k < pp::kBracketSteps; ++k, h = h + h) {
                const double gq = eval(h);
                if (gq == gq && sign_of(gq) != s0) { lo = ap; glo = gp; hi = h; ghi = gq; found = true; break; }
                if (gq == gq) { ap = h; gp = gq; }
                const double gr = eval(-h);
                if (gr == gr && sign_of(gr) != s0) { lo = am; glo = gm; hi = -h; ghi = gr; found = true; break; }
                if (gr == gr) { am = -h; gm = gr; }
            }
            if (!found) status |= DFTA_PS_NOBRACKET;
        }
        // bisection until no double lies between the ends, or an end is a root
        if (s0 != 0 && !status) {
            while (ghi != 0.) {
                const double mid = lo + (hi - lo) * 0.5;
                if (mid == lo || mid == hi) break;
                if (iters >= pp::kIterCap) { status |= DFTA_PS_CAP; break; }
                const double gmid = eval(mid);
                if (gmid != gmid) { status |= DFTA_PS_NOBRACKET; break; }
                if (sign_of(gmid) == s0) { lo = mid; glo = gmid; }
                else { hi = mid; ghi = gmid; }
            }
            if (fabs(ghi) < fabs(glo)) lo = hi;      // the end of smaller |g| is kept
        }
        if (!status) g = eval(lo);                   // the coefficients and the norm of the end that is kept
    }

    // the rows: pseudo inside, copies outside; a pseudo-orbital that is not positive and finite inside takes the channel
    int neg = 0;
    if (!status)
        for (int i = tid; i < ic; i += kLanes)
            if (i >= 1) {
                const double ui = pseudo_u(a.r[i], rinv, l, c);
                neg |= !(ui > 0.) || !(ui <= DBL_MAX);
            }
    neg = __syncthreads_or(neg);
    if (neg) status |= DFTA_PS_NOTPOSITIVE;
    const bool ok = status == 0;
    double cq[6], cw[6];
#pragma unroll
    for (int k = 1; k <= 6; ++k) {
        cq[k - 1] = (double)(2 * k) * c[k];
        cw[k - 1] = (double)(2 * k * (2 * k - 1)) * c[k];
    }
    const double lp = (double)l + 1., rc2 = rc * rc;
    for (int i = tid; i < N; i += kLanes) {
        double uo = nan, vo = nan;
        if (ok) {
            if (i >= ic) {
                uo = sigma * U[i];
                vo = V[i];
            } else {
                const double ri = a.r[i];
                const double x = ri * rinv, t = x * x;
                const double q = cq[0] + t * (cq[1] + t * (cq[2] + t * (cq[3] + t * (cq[4] + t * cq[5]))));
                const double w = cw[0] + t * (cw[1] + t * (cw[2] + t * (cw[3] + t * (cw[4] + t * cw[5]))));
                uo = pseudo_u(ri, rinv, l, c);
                vo = eps + ((lp * q) + ((w + t * (q * q)) * 0.5)) / rc2;
            }
        }
        if (a.ups) a.ups[(size_t)ch * N + i] = uo;
        if (a.vps) a.vps[(size_t)ch * N + i] = vo;
    }
    if (tid == 0) {
        for (int k = 0; k < kCoef; ++k) a.coef[(size_t)ch * kCoef + k] = ok ? c[k] : nan;
        double* __restrict__ m = a.match + (size_t)ch * kMatch;
        for (int k = 0; k < 5; ++k) m[k] = ok ? P[k] : nan;
        m[5] = ok ? IAE : nan; m[6] = ok ? Ips : nan; m[7] = ok ? g : nan;
        a.rc[ch] = ok ? rc : nan;
        a.iters[ch] = iters;
        a.status[ch] = status;
    }
}

// ---- unscreening and the Kleinman-Bylander quantities (the header's second half of the block) -----------------------------------------
constexpr double kFourPi = 12.566370614359172;       // the double nearest 4 pi

struct IonicArgs {
    int N, nch;
    double hstep;
    const double *r, *cnst;
    const int *atom, *l, *loc;                       // per channel; loc: per atom, the channel of its local potential
    const double *occ, *a0;
    const double *U, *Vps, *Y;                       // nch x N
    double *rho, *vH;                                // natoms x N
    const double* vxc;
    double *Vion, *beta;                             // nch x N
    double* kb;                                      // nch x 3
};

// grid (node tiles, atoms): rho_v and v_H of an atom, its channels added in the order of the call from 0.0
__global__ __launch_bounds__(256) void k_ps_density(IonicArgs a)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x, A = blockIdx.y;
    if (i >= a.N) return;
    const double ri = a.r[i];
    double rho = 0., vh = 0.;
    for (int ch = 0; ch < a.nch; ++ch) {
        if (a.atom[ch] != A) continue;
        const double ui = a.U[(size_t)ch * a.N + i];
        const double t = i > 0 ? (ui * ui) / ((kFourPi * ri) * ri) : (a.l[ch] == 0 ? exp(2. * a.a0[ch]) / kFourPi : 0.);
        rho = rho + a.occ[ch] * t;
        vh = vh + a.occ[ch] * a.Y[(size_t)ch * a.N + i];
    }
    a.rho[(size_t)A * a.N + i] = rho;
    a.vH[(size_t)A * a.N + i] = vh;
}

// grid (node tiles, channels): V_ion of the channel, its difference from the atom's local channel and beta
__global__ __launch_bounds__(256) void k_ps_ionic(IonicArgs a)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x, ch = blockIdx.y;
    if (i >= a.N) return;
    const int A = a.atom[ch], lc = a.loc[A];
    const double vh = a.vH[(size_t)A * a.N + i], vx = a.vxc[(size_t)A * a.N + i];
    const double vion = (a.Vps[(size_t)ch * a.N + i] - vh) - vx;
    const double vloc = (a.Vps[(size_t)lc * a.N + i] - vh) - vx;
    a.Vion[(size_t)ch * a.N + i] = vion;
    a.beta[(size_t)ch * a.N + i] = (vion - vloc) * a.U[(size_t)ch * a.N + i];
}

// one workgroup per channel: <u|dV|u> and <u|dV^2|u> in the shape of the orbital block, and E_KB
__global__ __launch_bounds__(kLanes) void k_ps_kb(IonicArgs a)
{
    __shared__ double red[kLanes / 64][2];
    const int tid = threadIdx.x, ch = blockIdx.x, N = a.N;
    double q1 = 0., q2 = 0.;
    for (int i = tid; i < N; i += kLanes) {
        const double b = a.beta[(size_t)ch * N + i], ui = a.U[(size_t)ch * N + i], sc = a.cnst[i] * a.hstep, w = simpson38_weight(i, N);
        q1 += w * ((b * ui) * sc);
        q2 += w * ((b * b) * sc);
    }
    q1 = wave_tree_sum(q1);
    q2 = wave_tree_sum(q2);
    if ((tid & 63) == 0) { red[tid >> 6][0] = q1; red[tid >> 6][1] = q2; }
    __syncthreads();
    if (tid == 0) {
        const double s1 = simpson38_finish(waves_join(red[0][0], red[1][0], red[2][0], red[3][0]));
        const double s2 = simpson38_finish(waves_join(red[0][1], red[1][1], red[2][1], red[3][1]));
        a.kb[ch * 3] = s1; a.kb[ch * 3 + 1] = s2; a.kb[ch * 3 + 2] = s2 / s1;
    }
}

}  // namespace

int dfta_pseudize_run(dfta_ctx* ctx, const dfta_grid* g, int nch, const double* dV, const int* dVrow, const double* dU, const int* dUrow,
                      const int* dL, const double* dEps, const int* dIc, const dfta_pseudize_out& out)
{
    if (nch <= 0) return DFTA_OK;
    const size_t N = (size_t)g->N;
    hipStream_t st = ctx->stream;
    DevBuf<double> dUps, dVps, dCoef, dRc, dMatch;
    DevBuf<int> dIters, dStatus;
    if (out.u_ps) DFTA_HIP(ctx, dUps.alloc((size_t)nch * N));
    if (out.V_ps) DFTA_HIP(ctx, dVps.alloc((size_t)nch * N));
    DFTA_HIP(ctx, dCoef.alloc((size_t)nch * kCoef));
    DFTA_HIP(ctx, dMatch.alloc((size_t)nch * kMatch));
    DFTA_HIP(ctx, dRc.alloc(nch));
    DFTA_HIP(ctx, dIters.alloc(nch));
    DFTA_HIP(ctx, dStatus.alloc(nch));

    PseudoArgs a;
    a.N = g->N;
    a.hstep = dfta_hstep(g);
    a.lam = g->uniform ? 0. : g->delta;
    a.r = g->d_r.p; a.cnst = g->d_cnst.p;
    a.V = dV; a.U = dU; a.vrow = dVrow; a.urow = dUrow; a.l = dL; a.ic = dIc; a.eps = dEps;
    a.ups = dUps.p; a.vps = dVps.p; a.coef = dCoef.p; a.rc = dRc.p; a.match = dMatch.p;
    a.iters = dIters.p; a.status = dStatus.p;
    DFTA_HIP(ctx, dfta_timer_start(ctx));
    hipLaunchKernelGGL(k_pseudize, dim3((unsigned)nch), dim3(kLanes), 0, st, a);
    DFTA_CHECK_LAUNCH(ctx);
    DFTA_HIP(ctx, dfta_timer_stop(ctx));

    if (out.u_ps) DFTA_HIP(ctx, hipMemcpyAsync(out.u_ps, dUps.p, sizeof(double) * nch * N, hipMemcpyDeviceToHost, st));
    if (out.V_ps) DFTA_HIP(ctx, hipMemcpyAsync(out.V_ps, dVps.p, sizeof(double) * nch * N, hipMemcpyDeviceToHost, st));
    if (out.coef) DFTA_HIP(ctx, hipMemcpyAsync(out.coef, dCoef.p, sizeof(double) * nch * kCoef, hipMemcpyDeviceToHost, st));
    if (out.match) DFTA_HIP(ctx, hipMemcpyAsync(out.match, dMatch.p, sizeof(double) * nch * kMatch, hipMemcpyDeviceToHost, st));
    if (out.rc) DFTA_HIP(ctx, hipMemcpyAsync(out.rc, dRc.p, sizeof(double) * nch, hipMemcpyDeviceToHost, st));
    if (out.iters) DFTA_HIP(ctx, hipMemcpyAsync(out.iters, dIters.p, sizeof(int) * nch, hipMemcpyDeviceToHost, st));
    if (out.status) DFTA_HIP(ctx, hipMemcpyAsync(out.status, dStatus.p, sizeof(int) * nch, hipMemcpyDeviceToHost, st));
    DFTA_HIP(ctx, hipStreamSynchronize(st));
    return DFTA_OK;
}

extern "C" {

int dfta_pseudize(dfta_ctx* ctx, const dfta_grid* g, int nch, const double* V, const double* u, const int* l, const double* eps,
                  const int* ic, double* u_ps, double* V_ps, double* coef, double* rc, double* match, int* iters, int* status)
{
    if (!ctx || !g) return DFTA_ERR_INVALID;
    DFTA_ENTER(ctx);
    DFTA_REQUIRE(ctx, nch >= 0, "dfta_pseudize: nch");
    if (nch == 0) return DFTA_OK;
    DFTA_REQUIRE(ctx, V && u && l && eps && ic, "dfta_pseudize arguments");
    pp::Call c;
    c.N = g->N; c.nch = nch; c.l = l; c.ic = ic;
    if (const char* msg = pp::check(c)) DFTA_REQUIRE(ctx, false, msg);
    DevBuf<double> dV, dU, dEps;
    DevBuf<int> dL, dIc;
    if (const int rc_ = dfta_upload_rows(ctx, V, (size_t)nch * g->N, &dV)) return rc_;
    if (const int rc_ = dfta_upload_rows(ctx, u, (size_t)nch * g->N, &dU)) return rc_;
    if (const int rc_ = dfta_upload_rows(ctx, eps, (size_t)nch, &dEps)) return rc_;
    if (const int rc_ = dfta_upload_rows(ctx, l, (size_t)nch, &dL)) return rc_;
    if (const int rc_ = dfta_upload_rows(ctx, ic, (size_t)nch, &dIc)) return rc_;
    dfta_pseudize_out out;
    out.u_ps = u_ps; out.V_ps = V_ps; out.coef = coef; out.rc = rc; out.match = match; out.iters = iters; out.status = status;
    return dfta_pseudize_run(ctx, g, nch, dV.p, nullptr, dU.p, nullptr, dL.p, dEps.p, dIc.p, out);
}

int dfta_pseudo_ionic(dfta_ctx* ctx, const dfta_grid* g, int functional, int natoms, int nch, const int* atom, const int* l, const double* occ,
                      const double* a0, const double* u_ps, const double* V_ps, const int* l_loc, double* rho_v, double* vH, double* vxc,
                      double* V_ion, double* beta, double* kb)
{
    if (!ctx || !g) return DFTA_ERR_INVALID;
    DFTA_ENTER(ctx);
    DFTA_REQUIRE(ctx, nch >= 0 && natoms >= 0, "dfta_pseudo_ionic: nch, natoms");
    if (nch == 0 || natoms == 0) return DFTA_OK;
    DFTA_REQUIRE(ctx, atom && l && occ && a0 && u_ps && V_ps && g->N >= 8 && natoms <= 65535 && nch <= 65535, "dfta_pseudo_ionic arguments");
    DFTA_REQUIRE(ctx, functional == DFTA_XC_VWN || functional == DFTA_XC_PW92 || (functional == DFTA_XC_PBE && !g->uniform),
                 "dfta_pseudo_ionic: functional (VWN, PW92, or PBE on the logarithmic grid)");
    std::vector<int> loc(natoms, -1), jobs((size_t)nch * 3);
    for (int k = 0; k < nch; ++k) {
        DFTA_REQUIRE(ctx, atom[k] >= 0 && atom[k] < natoms, "dfta_pseudo_ionic: an atom index outside 0 .. natoms-1");
        DFTA_REQUIRE(ctx, l[k] >= 0 && l[k] <= pp::kLmax, "dfta_pseudo_ionic: l outside 0 .. 4");
        DFTA_REQUIRE(ctx, occ[k] > 0. && std::isfinite(occ[k]), "dfta_pseudo_ionic: an unoccupied level");
        jobs[3 * k] = k; jobs[3 * k + 1] = k; jobs[3 * k + 2] = 0;
        const int A = atom[k], want = l_loc ? l_loc[A] : -1;
        if (want >= 0) { if (l[k] == want && loc[A] < 0) loc[A] = k; }
        else if (loc[A] < 0 || l[k] > l[loc[A]]) loc[A] = k;
    }
    for (int A = 0; A < natoms; ++A) DFTA_REQUIRE(ctx, loc[A] >= 0, "dfta_pseudo_ionic: an atom without channels, or without a channel of l_loc");
    const size_t N = (size_t)g->N;
    hipStream_t st = ctx->stream;
    DevBuf<double> dU, dV, dOcc, dA0, dY, dRho, dVH, dVxc, dE, dVa, dVb, dVion, dBeta, dKb;
    DevBuf<int> dAtom, dL, dLoc, dJobs;
    int rc = dfta_upload_rows(ctx, u_ps, nch * N, &dU);
    if (!rc) rc = dfta_upload_rows(ctx, V_ps, nch * N, &dV);
    if (!rc) rc = dfta_upload_rows(ctx, occ, (size_t)nch, &dOcc);
    if (!rc) rc = dfta_upload_rows(ctx, a0, (size_t)nch, &dA0);
    if (!rc) rc = dfta_upload_rows(ctx, atom, (size_t)nch, &dAtom);
    if (!rc) rc = dfta_upload_rows(ctx, l, (size_t)nch, &dL);
    if (!rc) rc = dfta_upload_rows(ctx, loc.data(), (size_t)natoms, &dLoc);
    if (!rc) rc = dfta_upload_rows(ctx, jobs.data(), jobs.size(), &dJobs);
    if (rc) return rc;
    DFTA_HIP(ctx, dY.alloc(nch * N));
    DFTA_HIP(ctx, dVion.alloc(nch * N));
    DFTA_HIP(ctx, dBeta.alloc(nch * N));
    DFTA_HIP(ctx, dKb.alloc((size_t)nch * 3));
    for (DevBuf<double>* b : {&dRho, &dVH, &dVxc, &dE, &dVa, &dVb}) DFTA_HIP(ctx, b->alloc(natoms * N));
    IonicArgs a;
    a.N = g->N; a.nch = nch; a.hstep = dfta_hstep(g);
    a.r = g->d_r.p; a.cnst = g->d_cnst.p;
    a.atom = dAtom.p; a.l = dL.p; a.loc = dLoc.p; a.occ = dOcc.p; a.a0 = dA0.p;
    a.U = dU.p; a.Vps = dV.p; a.Y = dY.p; a.rho = dRho.p; a.vH = dVH.p; a.vxc = dVxc.p;
    a.Vion = dVion.p; a.beta = dBeta.p; a.kb = dKb.p;
    const unsigned tiles = (unsigned)((N + 255) / 256);
    const auto launches = [&]() -> int {             // (its own function: an error inside still reaches the timer's stop below)
        if (const int e = dfta_launch_screening_yk(ctx, g, dU.p, nch, dJobs.p, dY.p)) return e;
        hipLaunchKernelGGL(k_ps_density, dim3(tiles, (unsigned)natoms), dim3(256), 0, st, a);
        DFTA_CHECK_LAUNCH(ctx);
        int e;
        if (functional == DFTA_XC_PBE) e = dfta_launch_pbe_radial(ctx, g, natoms, dRho.p, nullptr, dVxc.p, dVa.p, dVb.p, dE.p, nullptr);
        else if (functional == DFTA_XC_PW92) e = dfta_launch_pw92_lda(ctx, dRho.p, natoms * N, dVxc.p, dE.p);
        else e = dfta_launch_vwn_lda(ctx, dRho.p, natoms * N, dVxc.p, dE.p);
        if (e) return e;
        hipLaunchKernelGGL(k_ps_ionic, dim3(tiles, (unsigned)nch), dim3(256), 0, st, a);
        DFTA_CHECK_LAUNCH(ctx);
        hipLaunchKernelGGL(k_ps_kb, dim3((unsigned)nch), dim3(kLanes), 0, st, a);
        DFTA_CHECK_LAUNCH(ctx);
        return DFTA_OK;
    };
    DFTA_HIP(ctx, dfta_timer_start(ctx));
    rc = launches();
    const hipError_t stopped = dfta_timer_stop(ctx);
    if (rc) return rc;
    DFTA_HIP(ctx, stopped);
    if (rho_v) DFTA_HIP(ctx, hipMemcpyAsync(rho_v, dRho.p, sizeof(double) * natoms * N, hipMemcpyDeviceToHost, st));
    if (vH) DFTA_HIP(ctx, hipMemcpyAsync(vH, dVH.p, sizeof(double) * natoms * N, hipMemcpyDeviceToHost, st));
    if (vxc) DFTA_HIP(ctx, hipMemcpyAsync(vxc, dVxc.p, sizeof(double) * natoms * N, hipMemcpyDeviceToHost, st));
    if (V_ion) DFTA_HIP(ctx, hipMemcpyAsync(V_ion, dVion.p, sizeof(double) * nch * N, hipMemcpyDeviceToHost, st));
    if (beta) DFTA_HIP(ctx, hipMemcpyAsync(beta, dBeta.p, sizeof(double) * nch * N, hipMemcpyDeviceToHost, st));
    if (kb) DFTA_HIP(ctx, hipMemcpyAsync(kb, dKb.p, sizeof(double) * nch * 3, hipMemcpyDeviceToHost, st));
    DFTA_HIP(ctx, hipStreamSynchronize(st));
    return DFTA_OK;
}

int dfta_pseudo_default_valence(int nlev, const int* n, const int* l, const int* occ, int cap, int* pick, int* npick)
{
    if (!npick) return DFTA_ERR_INVALID;
    const int cnt = pp::default_valence(nlev, n, l, occ, pick, cap);
    if (cnt < 0) return DFTA_ERR_INVALID;
    *npick = cnt;
    return DFTA_OK;
}

int dfta_pseudo_default_ic(const dfta_grid* g, int nch, const double* u, double factor, int* ic)
{
    if (!g || nch < 0 || (nch > 0 && (!u || !ic))) return DFTA_ERR_INVALID;
    for (int k = 0; k < nch; ++k) {
        ic[k] = pp::default_ic(g->N, g->h_r.data(), u + (size_t)k * g->N, factor);
        if (ic[k] < 0) return DFTA_ERR_INVALID;
    }
    return DFTA_OK;
}

}  // extern "C"
