// xc.hip -- Vosko-Wilk-Nusair exchange-correlation, LDA and LSDA, as coalesced pointwise kernels (and the PW92 / Chachiyo alternatives).
//
// Replaces VWNExchCor::Vexc / eexcDif (VWNExcCor.h:73-128, LDA) and the spin-polarised pair
// (VWNExcCor.h:134-312, LSDA) with ExcCorBase::f / df (ExcCorBase.h:14-26).  Expressions are written in the
// reference's operation order; pow/log/atan come from the ROCm device library, so results agree with the
// glibc-based reference to rounding of those functions (the gate and its measure: tests/test_gpu_vwn.py).
// HBM-bound by construction: LDA reads 8 B and writes 16 B per point, LSDA reads 16 B and writes 32 B.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "gga.h"
#include "internal.h"
#include "vwn_device.h"
#include "xc.h"

namespace {

using dfta_vwn_dev::eval_fit;
using dfta_vwn_dev::FitValue;
using dfta_vwn_dev::kPara;
using dfta_vwn_dev::kPi;
using dfta_vwn_dev::kThird;
using dfta_vwn_dev::wigner_seitz;

// LDA (VWNExcCor.h:73-128): v_xc and the double-counting term eps_xc - v_xc, both from one evaluation of the paramagnetic fit
__global__ void k_vwn_lda(const double* __restrict__ n, size_t sz, double* __restrict__ vexc, double* __restrict__ eexc, double cx)
{
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < sz; i += (size_t)gridDim.x * blockDim.x) {
        const double rho = n[i];
        double v = 0., e = 0.;
        if (!(rho < 1E-18)) {                                         // VWNExcCor.h:82,112
            const double rs = wigner_seitz(rho);
            const FitValue c = eval_fit<false>(kPara, sqrt(rs));
            v = -cx / rs + c.eps - kThird * c.slope;                  // VWNExcCor.h:94-97
            e = (0.25 * cx) / rs + kThird * c.slope;                  // VWNExcCor.h:123-124
        }
        if (vexc) vexc[i] = v;
        if (eexc) eexc[i] = e;
    }
}

// LSDA (VWNExcCor.h:134-312): the node arithmetic is dfta_vwn_dev::lsda_point (vwn_device.h), which the orbital xc of the
// self-interaction correction shares
__global__ void k_vwn_lsda(const double* __restrict__ na, const double* __restrict__ nb, size_t sz, double* __restrict__ res,
                           double* __restrict__ va, double* __restrict__ vb, double* __restrict__ eexc, double cx, double cbrt2)
{
    const dfta_vwn_dev::LsdaConsts k = dfta_vwn_dev::lsda_consts(cx, cbrt2);
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < sz; i += (size_t)gridDim.x * blockDim.x) {
        const dfta_vwn_dev::LsdaPoint p = dfta_vwn_dev::lsda_point(k, na[i], nb[i]);
        if (res) res[i] = p.common;
        if (va) va[i] = p.vup;
        if (vb) vb[i] = p.vdn;
        if (eexc) eexc[i] = p.e;
    }
}

// Chachiyo's one-line correlation (ExcCor.h:27-95; the reference keeps it next to VWN, all its call sites commented out:
// DFTAtom.cpp:383,412,421): eps_c = a ln(1 + b/rs + b/rs^2), a = (ln 2 - 1) / (2 pi^2).  LDA only, as in the reference.
__global__ void k_chachiyo_lda(const double* __restrict__ n, size_t sz, double* __restrict__ vexc, double* __restrict__ eexc, double cx,
                               double a, double b)
{
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < sz; i += (size_t)gridDim.x * blockDim.x) {
        const double rho = n[i];
        double v = 0., e = 0.;
        if (!(rho < 1E-18)) {                                         // ExcCor.h:50,79
            const double rs = wigner_seitz(rho);
            const double q1 = b / rs, q2 = q1 / rs;
            const double tail = a / (1. + q1 + q2) * (q1 + 2. * q2) * rs / 3.;
            v = -cx / rs + a * log(1. + q1 + q1 / rs) - tail;         // ExcCor.h:60-63
            e = (0.25 * cx) / rs + tail;                              // ExcCor.h:89-91
        }
        if (vexc) vexc[i] = v;
        if (eexc) eexc[i] = e;
    }
}

// Slater exchange + Perdew-Wang 1992 correlation (gga.h, the same G(rs) as the PBE kernel).  Outputs as k_vwn_lda / k_vwn_lsda:
// LDA Vexc = v, eexc = eps_xc - v; LSDA res = (v_a rho_a + v_b rho_b) / rho, v_a, v_b, eexc = eps_xc - res.
__global__ void k_pw92_lda(const double* __restrict__ n, size_t sz, double* __restrict__ vexc, double* __restrict__ eexc)
{
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < sz; i += (size_t)gridDim.x * blockDim.x) {
        const double rho = n[i];
        const dfta_gga::XcPoint p = dfta_gga::xc_point<false, false>(rho, 0., 0., 0., 0.);
        const bool on = !(rho < dfta_gga::kThreshold) && rho == rho;
        if (vexc) vexc[i] = p.da;
        if (eexc) eexc[i] = on ? p.e / rho - p.da : 0.;
    }
}

__global__ void k_pw92_lsda(const double* __restrict__ na, const double* __restrict__ nb, size_t sz, double* __restrict__ res,
                            double* __restrict__ va, double* __restrict__ vb, double* __restrict__ eexc)
{
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < sz; i += (size_t)gridDim.x * blockDim.x) {
        const double up = na[i], dn = nb[i];
        const double tot = up + dn;
        const dfta_gga::XcPoint p = dfta_gga::xc_point<true, false>(up, dn, 0., 0., 0.);
        const bool on = !(tot < dfta_gga::kThreshold) && tot == tot;
        const double mean = on ? (p.da * up + p.db * dn) / tot : 0.;
        if (res) res[i] = mean;
        if (va) va[i] = p.da;
        if (vb) vb[i] = p.db;
        if (eexc) eexc[i] = on ? p.e / tot - mean : 0.;
    }
}

}  // namespace

// the two irrational constants are evaluated once on the host with libm, as the reference does (VWNExcCor.h:75,139-140)
static double host_X1() { return pow(3. / (2. * kPi), 2. * kThird); }
static double host_X2() { return pow(2., kThird); }
double dfta_vwn_cx() { return host_X1(); }
double dfta_vwn_cbrt2() { return host_X2(); }

int dfta_launch_chachiyo_lda(dfta_ctx* ctx, int improved, const double* dN, size_t sz, double* dVexc, double* dEexc)
{
    const double a = (M_LN2 - 1.) / (2. * kPi * kPi);                 // ExcCor.h:32
    const double b = improved ? 21.7392245 : 20.4562557;              // ExcCor.h:16,24
    const int blocks = (int)std::min<size_t>((sz + 255) / 256, 2048);
    hipLaunchKernelGGL(k_chachiyo_lda, dim3(blocks), dim3(256), 0, ctx->stream, dN, sz, dVexc, dEexc, host_X1(), a, b);
    DFTA_CHECK_LAUNCH(ctx);
    return DFTA_OK;
}

int dfta_launch_vwn_lda(dfta_ctx* ctx, const double* dN, size_t sz, double* dVexc, double* dEexc)
{
    const int blocks = (int)std::min<size_t>((sz + 255) / 256, 2048);
    hipLaunchKernelGGL(k_vwn_lda, dim3(blocks), dim3(256), 0, ctx->stream, dN, sz, dVexc, dEexc, host_X1());
    DFTA_CHECK_LAUNCH(ctx);
    return DFTA_OK;
}

int dfta_launch_vwn_lsda(dfta_ctx* ctx, const double* dNa, const double* dNb, size_t sz, double* dRes, double* dVa, double* dVb,
                         double* dEexc)
{
    const int blocks = (int)std::min<size_t>((sz + 255) / 256, 2048);
    hipLaunchKernelGGL(k_vwn_lsda, dim3(blocks), dim3(256), 0, ctx->stream, dNa, dNb, sz, dRes, dVa, dVb, dEexc, host_X1(), host_X2());
    DFTA_CHECK_LAUNCH(ctx);
    return DFTA_OK;
}

int dfta_launch_pw92_lda(dfta_ctx* ctx, const double* dN, size_t sz, double* dVexc, double* dEexc)
{
    const int blocks = (int)std::min<size_t>((sz + 255) / 256, 2048);
    hipLaunchKernelGGL(k_pw92_lda, dim3(blocks), dim3(256), 0, ctx->stream, dN, sz, dVexc, dEexc);
    DFTA_CHECK_LAUNCH(ctx);
    return DFTA_OK;
}

int dfta_launch_pw92_lsda(dfta_ctx* ctx, const double* dNa, const double* dNb, size_t sz, double* dRes, double* dVa, double* dVb,
                          double* dEexc)
{
    const int blocks = (int)std::min<size_t>((sz + 255) / 256, 2048);
    hipLaunchKernelGGL(k_pw92_lsda, dim3(blocks), dim3(256), 0, ctx->stream, dNa, dNb, sz, dRes, dVa, dVb, dEexc);
    DFTA_CHECK_LAUNCH(ctx);
    return DFTA_OK;
}

extern "C" int dfta_vwn_lda(dfta_ctx* ctx, const double* n, size_t sz, double* vexc, double* eexcdif)
{
    if (!ctx) return DFTA_ERR_INVALID;
    DFTA_ENTER(ctx);
    DFTA_REQUIRE(ctx, n && (vexc || eexcdif), "null input");
    if (sz == 0) return DFTA_OK;
    hipStream_t st = ctx->stream;
    DevBuf<double> dN, dV, dE;
    DFTA_HIP(ctx, dN.alloc(sz)); DFTA_HIP(ctx, dV.alloc(sz)); DFTA_HIP(ctx, dE.alloc(sz));
    DFTA_HIP(ctx, hipMemcpyAsync(dN.p, n, sizeof(double) * sz, hipMemcpyHostToDevice, st));
    DFTA_HIP(ctx, dfta_timer_start(ctx));
    int rc = dfta_launch_vwn_lda(ctx, dN.p, sz, dV.p, dE.p);
    if (rc) return rc;
    DFTA_HIP(ctx, dfta_timer_stop(ctx));
    if (vexc) DFTA_HIP(ctx, hipMemcpyAsync(vexc, dV.p, sizeof(double) * sz, hipMemcpyDeviceToHost, st));
    if (eexcdif) DFTA_HIP(ctx, hipMemcpyAsync(eexcdif, dE.p, sizeof(double) * sz, hipMemcpyDeviceToHost, st));
    DFTA_HIP(ctx, hipStreamSynchronize(st));
    return DFTA_OK;
}

extern "C" int dfta_vwn_lsda(dfta_ctx* ctx, const double* na, const double* nb, size_t sz, double* vexc, double* va, double* vb,
                             double* eexcdif)
{
    if (!ctx) return DFTA_ERR_INVALID;
    DFTA_ENTER(ctx);
    DFTA_REQUIRE(ctx, na && nb, "null input");
    if (sz == 0) return DFTA_OK;
    hipStream_t st = ctx->stream;
    DevBuf<double> dA, dB, dR, dVa, dVb, dE;
    DFTA_HIP(ctx, dA.alloc(sz)); DFTA_HIP(ctx, dB.alloc(sz)); DFTA_HIP(ctx, dR.alloc(sz));
    DFTA_HIP(ctx, dVa.alloc(sz)); DFTA_HIP(ctx, dVb.alloc(sz)); DFTA_HIP(ctx, dE.alloc(sz));
    DFTA_HIP(ctx, hipMemcpyAsync(dA.p, na, sizeof(double) * sz, hipMemcpyHostToDevice, st));
    DFTA_HIP(ctx, hipMemcpyAsync(dB.p, nb, sizeof(double) * sz, hipMemcpyHostToDevice, st));
    DFTA_HIP(ctx, dfta_timer_start(ctx));
    int rc = dfta_launch_vwn_lsda(ctx, dA.p, dB.p, sz, dR.p, dVa.p, dVb.p, dE.p);
    if (rc) return rc;
    DFTA_HIP(ctx, dfta_timer_stop(ctx));
    if (vexc) DFTA_HIP(ctx, hipMemcpyAsync(vexc, dR.p, sizeof(double) * sz, hipMemcpyDeviceToHost, st));
    if (va) DFTA_HIP(ctx, hipMemcpyAsync(va, dVa.p, sizeof(double) * sz, hipMemcpyDeviceToHost, st));
    if (vb) DFTA_HIP(ctx, hipMemcpyAsync(vb, dVb.p, sizeof(double) * sz, hipMemcpyDeviceToHost, st));
    if (eexcdif) DFTA_HIP(ctx, hipMemcpyAsync(eexcdif, dE.p, sizeof(double) * sz, hipMemcpyDeviceToHost, st));
    DFTA_HIP(ctx, hipStreamSynchronize(st));
    return DFTA_OK;
}

extern "C" int dfta_chachiyo_lda(dfta_ctx* ctx, int improved, const double* n, size_t sz, double* vexc, double* eexcdif)
{
    if (!ctx) return DFTA_ERR_INVALID;
    DFTA_ENTER(ctx);
    DFTA_REQUIRE(ctx, n && (vexc || eexcdif), "null input");
    if (sz == 0) return DFTA_OK;
    hipStream_t st = ctx->stream;
    DevBuf<double> dN, dV, dE;
    DFTA_HIP(ctx, dN.alloc(sz)); DFTA_HIP(ctx, dV.alloc(sz)); DFTA_HIP(ctx, dE.alloc(sz));
    DFTA_HIP(ctx, hipMemcpyAsync(dN.p, n, sizeof(double) * sz, hipMemcpyHostToDevice, st));
    int rc = dfta_launch_chachiyo_lda(ctx, improved, dN.p, sz, dV.p, dE.p);
    if (rc) return rc;
    if (vexc) DFTA_HIP(ctx, hipMemcpyAsync(vexc, dV.p, sizeof(double) * sz, hipMemcpyDeviceToHost, st));
    if (eexcdif) DFTA_HIP(ctx, hipMemcpyAsync(eexcdif, dE.p, sizeof(double) * sz, hipMemcpyDeviceToHost, st));
    DFTA_HIP(ctx, hipStreamSynchronize(st));
    return DFTA_OK;
}
