// gga.hip -- the PBE gradient-corrected functional on the logarithmic radial grid: one fused launch per evaluation.
//
// Grid: (tiles of an atom's N nodes) x (atoms).  A workgroup of 256 lanes owns kTile = 252 consecutive output nodes:
//   1. loads rho (rho_a, rho_b under LSDA) of its tile plus a 4-node halo on each side into LDS;
//   2. every lane forms rho' at one node of the tile plus a 2-node halo (5-point central differences in the index i divided by
//      dr/di = Rp delta exp(delta i), second-order one-sided differences at nodes 0, 1, N-2, N-1) and evaluates the pointwise PBE
//      terms there (gga.h) -- the halo nodes are recomputed, not exchanged -- and puts the flux
//          F_a = 2 e_saa rho_a' + e_sab rho_b'   (F_b likewise; LDA: F = 2 e_s rho')
//      into LDS;
//   3. writes v = de/drho - (dF/dr + 2 F / r) at the tile's nodes, with the same stencils for dF/di.
// Output contract (what k_tail, the energies and the records expect):
//   LDA:  Vexc = v,  eexc = e / rho - v
//   LSDA: res = (v_a rho_a + v_b rho_b) / rho, v_a, v_b, eexc = e / rho - res
// so that 4 pi Int (Vexc + eexc) rho r^2 dr = Int e and Etotal = Sum f eps + E_H + eExcDif hold as for VWN.  Node 0 and nodes whose
// total density is below 1e-18 write zeros.  Every atom's bits depend on its own density only (no cross-atom tile, no reduction).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "gga.h"
#include "internal.h"
#include "xc.h"

namespace {

using namespace dfta_gga;

constexpr int kLanes = 256;
constexpr int kTile = kLanes - 4;          // outputs per workgroup: the pointwise pass covers the tile + 2 nodes on each side

// d f / d i at node j from f[k-2 .. k+2] (f[k] is node j's value).  Differences first: neighbouring nodes differ by delta |f|, so
// f[k+1] - f[k-1] is (nearly) exact in fp64 and the result keeps its digits; summing the weighted values instead goes through
// partial sums of size 7 |f| and loses a factor 1 / delta to cancellation -- twice, since the divergence differentiates the flux
// again (4e-5 relative in v_xc at 1 048 577 nodes; tests/test_gga_reference.py::test_stencil_form_rounding holds both figures).
__device__ __forceinline__ double d_index(const double* f, int k, int j, int N)
{
    if (j < 2) return (4. * (f[k + 1] - f[k]) - (f[k + 2] - f[k])) * 0.5;
    if (j >= N - 2) return (4. * (f[k] - f[k - 1]) - (f[k] - f[k - 2])) * 0.5;
    return (8. * (f[k + 1] - f[k - 1]) - (f[k + 2] - f[k - 2])) / 12.;
}

template <bool POL>
__global__ __launch_bounds__(kLanes) void k_pbe_radial(int N, const double* __restrict__ r, const double* __restrict__ cnst,
                                                      const double* __restrict__ na, const double* __restrict__ nb,
                                                      double* __restrict__ res, double* __restrict__ va, double* __restrict__ vb,
                                                      double* __restrict__ eexc, const int* __restrict__ fin)
{
    const int a = blockIdx.y;
    if (fin && fin[a]) return;                         // frozen atom: its outputs stay those of its last step
    __shared__ double sA[kLanes + 4], sB[POL ? kLanes + 4 : 1], sFa[kLanes], sFb[POL ? kLanes : 1];
    const size_t base = (size_t)a * N;
    const int i0 = blockIdx.x * kTile;
    const int lane = threadIdx.x;
    for (int k = lane; k < kLanes + 4; k += kLanes) {  // nodes i0 - 4 .. i0 + kTile + 3
        const int j = i0 - 4 + k;
        const bool in = j >= 0 && j < N;
        sA[k] = in ? na[base + j] : 0.;
        if (POL) sB[k] = in ? nb[base + j] : 0.;
    }
    __syncthreads();
    const int j = i0 - 2 + lane;                       // this lane's node of the pointwise pass
    const bool live = j >= 0 && j < N;
    double rhoA = 0., rhoB = 0., fa = 0., fb = 0.;
    XcPoint p{0., 0., 0., 0., 0., 0.};
    if (live) {
        const double c = cnst[j];
        rhoA = sA[lane + 2];
        const double ga = d_index(sA, lane + 2, j, N) / c;
        if (POL) {
            rhoB = sB[lane + 2];
            const double gb = d_index(sB, lane + 2, j, N) / c;
            p = xc_point<true, true>(rhoA, rhoB, ga * ga, ga * gb, gb * gb);
            fa = 2. * p.dsaa * ga + p.dsab * gb;
            fb = 2. * p.dsbb * gb + p.dsab * ga;
        } else {
            p = xc_point<false, true>(rhoA, 0., ga * ga, 0., 0.);
            fa = 2. * p.dsaa * ga;
        }
    }
    sFa[lane] = fa;
    if (POL) sFb[lane] = fb;
    __syncthreads();
    if (lane < 2 || lane >= kLanes - 2 || !live) return;
    const size_t o = base + j;
    const double rho = POL ? rhoA + rhoB : rhoA;
    if (j == 0 || rho < kThreshold || !(rho == rho)) {
        res[o] = 0.;
        if (POL) { va[o] = 0.; vb[o] = 0.; }
        eexc[o] = 0.;
        return;
    }
    const double c = cnst[j], rj = r[j];
    const double vA = p.da - (d_index(sFa, lane, j, N) / c + 2. * fa / rj);
    const double exc = p.e / rho;
    if (!POL) {
        res[o] = vA;
        eexc[o] = exc - vA;
    } else {
        const double vB = p.db - (d_index(sFb, lane, j, N) / c + 2. * fb / rj);
        const double mean = (vA * rhoA + vB * rhoB) / rho;
        res[o] = mean;
        va[o] = vA;
        vb[o] = vB;
        eexc[o] = exc - mean;
    }
}

// e and its partial derivatives at independent points (dfta_xc_pointwise)
template <bool POL, bool GGA>
__global__ void k_xc_pointwise(size_t sz, const double* __restrict__ na, const double* __restrict__ nb, const double* __restrict__ saa,
                               const double* __restrict__ sab, const double* __restrict__ sbb, double* __restrict__ e,
                               double* __restrict__ dna, double* __restrict__ dnb, double* __restrict__ dsaa, double* __restrict__ dsab,
                               double* __restrict__ dsbb)
{
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < sz; i += (size_t)gridDim.x * blockDim.x) {
        const XcPoint p = xc_point<POL, GGA>(na[i], POL ? nb[i] : 0., GGA ? saa[i] : 0., GGA && POL ? sab[i] : 0.,
                                             GGA && POL ? sbb[i] : 0.);
        if (e) e[i] = p.e;
        if (dna) dna[i] = p.da;
        if (dsaa) dsaa[i] = p.dsaa;
        if (POL) {
            if (dnb) dnb[i] = p.db;
            if (dsab) dsab[i] = p.dsab;
            if (dsbb) dsbb[i] = p.dsbb;
        }
    }
}

}  // namespace

int dfta_launch_pbe_radial(dfta_ctx* ctx, const dfta_grid* g, int natoms, const double* dNa, const double* dNb, double* dRes,
                           double* dVa, double* dVb, double* dEexc, const int* dFin)
{
    const dim3 grid((g->N + kTile - 1) / kTile, natoms), block(kLanes);
    if (dNb)
        hipLaunchKernelGGL(k_pbe_radial<true>, grid, block, 0, ctx->stream, g->N, g->d_r, g->d_cnst, dNa, dNb, dRes, dVa, dVb, dEexc, dFin);
    else
        hipLaunchKernelGGL(k_pbe_radial<false>, grid, block, 0, ctx->stream, g->N, g->d_r, g->d_cnst, dNa, nullptr, dRes, nullptr, nullptr,
                           dEexc, dFin);
    DFTA_CHECK_LAUNCH(ctx);
    return DFTA_OK;
}

extern "C" int dfta_xc_pointwise(dfta_ctx* ctx, int functional, size_t sz, const double* na, const double* nb, const double* saa,
                                 const double* sab, const double* sbb, double* e, double* dna, double* dnb, double* dsaa, double* dsab,
                                 double* dsbb)
{
    if (!ctx) return DFTA_ERR_INVALID;
    DFTA_ENTER(ctx);
    DFTA_REQUIRE(ctx, functional == DFTA_XC_PW92 || functional == DFTA_XC_PBE, "dfta_xc_pointwise: functional must be DFTA_XC_PW92 or DFTA_XC_PBE");
    const bool pol = nb != nullptr, gga = functional == DFTA_XC_PBE;
    DFTA_REQUIRE(ctx, na && (!gga || (saa && (!pol || (sab && sbb)))), "null input");
    if (sz == 0) return DFTA_OK;
    hipStream_t st = ctx->stream;
    DevBuf<double> in[5], out[6];
    const double* hin[5] = {na, nb, saa, sab, sbb};
    double* hout[6] = {e, dna, dnb, dsaa, dsab, dsbb};
    const double* din[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    double* dout[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    for (int k = 0; k < 5; ++k) if (hin[k] && (gga || k < 2)) {
        DFTA_HIP(ctx, in[k].alloc(sz));
        DFTA_HIP(ctx, hipMemcpyAsync(in[k].p, hin[k], sizeof(double) * sz, hipMemcpyHostToDevice, st));
        din[k] = in[k].p;
    }
    for (int k = 0; k < 6; ++k) if (hout[k]) { DFTA_HIP(ctx, out[k].alloc(sz)); dout[k] = out[k].p; }
    const int blocks = (int)std::min<size_t>((sz + 255) / 256, 2048);
    DFTA_HIP(ctx, dfta_timer_start(ctx));
    if (pol && gga) hipLaunchKernelGGL((k_xc_pointwise<true, true>), dim3(blocks), dim3(256), 0, st, sz, din[0], din[1], din[2], din[3], din[4], dout[0], dout[1], dout[2], dout[3], dout[4], dout[5]);
    else if (pol) hipLaunchKernelGGL((k_xc_pointwise<true, false>), dim3(blocks), dim3(256), 0, st, sz, din[0], din[1], din[2], din[3], din[4], dout[0], dout[1], dout[2], dout[3], dout[4], dout[5]);
    else if (gga) hipLaunchKernelGGL((k_xc_pointwise<false, true>), dim3(blocks), dim3(256), 0, st, sz, din[0], din[1], din[2], din[3], din[4], dout[0], dout[1], dout[2], dout[3], dout[4], dout[5]);
    else hipLaunchKernelGGL((k_xc_pointwise<false, false>), dim3(blocks), dim3(256), 0, st, sz, din[0], din[1], din[2], din[3], din[4], dout[0], dout[1], dout[2], dout[3], dout[4], dout[5]);
    DFTA_CHECK_LAUNCH(ctx);
    DFTA_HIP(ctx, dfta_timer_stop(ctx));
    for (int k = 0; k < 6; ++k) if (hout[k] && (pol || (k != 2 && k < 4)))
        DFTA_HIP(ctx, hipMemcpyAsync(hout[k], dout[k], sizeof(double) * sz, hipMemcpyDeviceToHost, st));
    DFTA_HIP(ctx, hipStreamSynchronize(st));
    return DFTA_OK;
}

extern "C" int dfta_xc_radial(dfta_ctx* ctx, const dfta_grid* g, int functional, int natoms, const double* na, const double* nb,
                              double* res, double* va, double* vb, double* eexc)
{
    if (!ctx || !g) return DFTA_ERR_INVALID;
    DFTA_ENTER(ctx);
    DFTA_REQUIRE(ctx, functional == DFTA_XC_PW92 || functional == DFTA_XC_PBE, "dfta_xc_radial: functional must be DFTA_XC_PW92 or DFTA_XC_PBE");
    DFTA_REQUIRE(ctx, functional != DFTA_XC_PBE || !g->uniform, "the PBE functional needs a logarithmic grid (no GGA on the uniform grid)");
    DFTA_REQUIRE(ctx, natoms >= 1 && natoms <= 65535 && na, "dfta_xc_radial arguments");
    hipStream_t st = ctx->stream;
    const size_t sz = (size_t)natoms * g->N;
    const bool pol = nb != nullptr;
    DevBuf<double> dA, dB, dR, dVa, dVb, dE;
    DFTA_HIP(ctx, dA.alloc(sz)); DFTA_HIP(ctx, dR.alloc(sz)); DFTA_HIP(ctx, dE.alloc(sz));
    DFTA_HIP(ctx, hipMemcpyAsync(dA.p, na, sizeof(double) * sz, hipMemcpyHostToDevice, st));
    if (pol) {
        DFTA_HIP(ctx, dB.alloc(sz)); DFTA_HIP(ctx, dVa.alloc(sz)); DFTA_HIP(ctx, dVb.alloc(sz));
        DFTA_HIP(ctx, hipMemcpyAsync(dB.p, nb, sizeof(double) * sz, hipMemcpyHostToDevice, st));
    }
    DFTA_HIP(ctx, dfta_timer_start(ctx));
    int rc;
    if (functional == DFTA_XC_PBE) rc = dfta_launch_pbe_radial(ctx, g, natoms, dA.p, dB.p, dR.p, dVa.p, dVb.p, dE.p, nullptr);
    else if (pol) rc = dfta_launch_pw92_lsda(ctx, dA.p, dB.p, sz, dR.p, dVa.p, dVb.p, dE.p);
    else rc = dfta_launch_pw92_lda(ctx, dA.p, sz, dR.p, dE.p);
    if (rc) return rc;
    DFTA_HIP(ctx, dfta_timer_stop(ctx));
    if (res) DFTA_HIP(ctx, hipMemcpyAsync(res, dR.p, sizeof(double) * sz, hipMemcpyDeviceToHost, st));
    if (eexc) DFTA_HIP(ctx, hipMemcpyAsync(eexc, dE.p, sizeof(double) * sz, hipMemcpyDeviceToHost, st));
    if (pol && va) DFTA_HIP(ctx, hipMemcpyAsync(va, dVa.p, sizeof(double) * sz, hipMemcpyDeviceToHost, st));
    if (pol && vb) DFTA_HIP(ctx, hipMemcpyAsync(vb, dVb.p, sizeof(double) * sz, hipMemcpyDeviceToHost, st));
    DFTA_HIP(ctx, hipStreamSynchronize(st));
    return DFTA_OK;
}
