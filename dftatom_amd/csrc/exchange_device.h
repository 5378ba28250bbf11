// exchange_device.h -- the per-node and per-quadrature arithmetic of the exchange potentials as device functions, shared by the kernels of
// exchange.hip (one channel per call) and kli_stage.hip (every channel of a batch in one sequence of launches): one statement of each
// order of operations, so that the two paths return the same bits by construction.  include/dftatom_hip.h states the orders.
#pragma once
#include <hip/hip_runtime.h>

#include "exchange_plan.h"
#include "radial_device.h"

namespace dfta_exchange_dev {

constexpr int kPwThreads = 256;
constexpr int kRedThreads = 256;

// node i of a channel: X_a of every shell (written), D and vS (returned).  U, X: the channel's rows; Y: the rows of its y jobs
__device__ __forceinline__ void pointwise_node(int N, int i, int norb, const double* __restrict__ U, const double* __restrict__ occ,
                                               const int* __restrict__ first, const int* __restrict__ tab, const double* __restrict__ coef,
                                               const double* __restrict__ Y, double* __restrict__ X, double* den_out, double* vS_out)
{
    double den = 0., num = 0.;
    for (int a = 0; a < norb; ++a) {
        double acc = 0.;
        for (int e = first[a]; e < first[a + 1]; ++e) {
            const int b = tab[dfta_exchange::kTabInts * e + 1], row = tab[dfta_exchange::kTabInts * e + 3];
            acc += coef[e] * (Y[(size_t)row * N + i] * U[(size_t)b * N + i]);
        }
        X[(size_t)a * N + i] = acc;
        const double ua = U[(size_t)a * N + i];
        den += occ[a] * (ua * ua);
        num += occ[a] * (ua * acc);
    }
    *den_out = den;
    *vS_out = den > 0. ? -(num / den) : 0.;
}

// vKLI at node i from vS, D and the constants c
__device__ __forceinline__ double kli_node(int N, int i, int norb, int homo, const double* __restrict__ U, const double* __restrict__ occ,
                                           const double* __restrict__ c, double den, double vS)
{
    double acc = 0.;
    for (int a = 0; a < norb; ++a) {
        if (a == homo) continue;
        const double ua = U[(size_t)a * N + i];
        acc += (occ[a] * (ua * ua)) * c[a];
    }
    return den > 0. ? vS + acc / den : 0.;
}

// one quadrature by a workgroup of kRedThreads lanes: lane t adds the weighted terms of the nodes t, t + 256, ... to one accumulator, then
// the tree of radial_device.h.  The value (sign of HF included) in lane 0.
__device__ __forceinline__ double reduce_block(int N, double hstep, const double* __restrict__ cnst, const double* __restrict__ ua,
                                               const double* __restrict__ ub, const double* __restrict__ xa, const double* __restrict__ D,
                                               const double* __restrict__ v, int kind, double* part /* LDS, kRedThreads / 64 */)
{
    const int tid = threadIdx.x;
    double acc = 0.;
    for (int i = tid; i < N; i += kRedThreads) {
        const double sc = cnst[i] * hstep, w = dfta_radial::simpson38_weight(i, N), u = ua[i];
        double t;
        if (kind == dfta_exchange::kRedHF) t = (u * xa[i]) * sc;
        else if (kind == dfta_exchange::kRedPair) {
            const double den = D[i], u2 = ub[i];
            t = den == 0. ? 0. : (((u * u) * (u2 * u2)) / den) * sc;
        } else t = ((u * u) * v[i]) * sc;
        acc += w * t;
    }
    acc = dfta_radial::wave_tree_sum(acc);
    if ((tid & 63) == 0) part[tid >> 6] = acc;
    __syncthreads();
    double q = 0.;
    if (tid == 0) {
        q = dfta_radial::simpson38_finish(dfta_radial::waves_join(part[0], part[1], part[2], part[3]));
        if (kind == dfta_exchange::kRedHF) q = -q;
    }
    return q;
}

}  // namespace dfta_exchange_dev
