// radial_device.h -- the orders of operations that the radial-integral kernels share, as device functions: Simpson's 3/8 weights, the
// factors of a node, the increments of a cumulative integral, the scan of a tile of 256 lanes x kPer nodes (upwards and mirrored) and
// the summation tree of a workgroup of four waves.  One statement of each, used by orbitals.hip, slater.hip, bessel.hip, exchange.hip,
// exchange_device.h and kli_stage.hip, so that the kernels return the same bits by construction.  include/dftatom_hip.h states the
// orders; DESIGN.md 4.8 (the tree) and 4.9 (the scan) their shapes and rounding bounds.  (k_screening_yk writes chain_* and
// waves_chain_* out: DESIGN.md 4.11 says why.)
//
// The scan of a tile, for a workgroup of 256 lanes (4 waves), lane t owning the kPer consecutive nodes i0 .. i0 + kPer - 1 at the LDS
// slots q0 ..:
//     chain_up           l_j = d_{i0} + ... + d_{i0+j}, left to right; returns the lane's total l_{kPer-1}
//     wave_prefix_up     the inclusive scan of the totals across the wave (six levels): inc, and ex = the sum of the lanes below this
//                        one in its wave (0 in lane 0)
//     -- the kernel: lane 63 posts inc, the wave's total, to wtot[wave] in LDS (every stream of the tile under ONE condition: a post per
//        helper call measured 2 % slower in k_slater_rk); then its __syncthreads(), which several streams may share --
//     waves_chain_up     off = the totals of the waves below this one, tot = the tile's total, both chained from wave 0
//     Z_i = carry + ((off + ex) + l_j);  carry = carry + tot after the tile.
// The mirror image (chain_down, wave_prefix_down, waves_chain_down) runs from the lane's last node, the wave's last lane and wave 3
// downwards; lane 0 posts.  The barrier is the kernel's own: nothing here synchronises or writes LDS, so a kernel keeps its count of
// barriers per tile.
// Built, as everything here, without FMA contraction: the source order is the order of the roundings.
#pragma once
#include <hip/hip_runtime.h>

namespace dfta_radial {

// Simpson 3/8 weight of node i without the factor 3/8 (Integral.h:50-73)
__device__ __forceinline__ double simpson38_weight(int i, int N) { return (i == 0 || i == N - 1) ? 1. : (i % 3 == 0 ? 2. : 3.); }

// the factor 3/8 that the weights leave out, applied once to the finished sum
__device__ __forceinline__ double simpson38_finish(double sum)
{
    constexpr double coef = 3. / 8.;
    return sum * coef;
}

// the factors of node i in a job of order k: p = r_i^k by k multiplications from 1, inv = 1 / (p r_i) with inv_0 = 0 (r_0 = 0: the outer
// term is 0 there), sc = cnst_i hstep = dr/di
struct NodeFactors { double p, inv, sc; };
__device__ __forceinline__ NodeFactors node_factors(int k, double ri, double ci, double hstep, int i)
{
    NodeFactors f;
    f.sc = ci * hstep;
    double p = 1.;
    for (int m = 0; m < k; ++m) p = p * ri;
    f.p = p;
    f.inv = i > 0 ? 1. / (p * ri) : 0.;
    return f;
}

// the increment d_i of a cumulative integral at node i, 1 <= i <= N-1, from the slots around q (the header states these orders)
__device__ __forceinline__ double increment(const double* g, int q, int i, int N)
{
    if (i == 1) return (((9. * g[q - 1] + 19. * g[q]) - 5. * g[q + 1]) + g[q + 2]) / 24.;
    if (i == N - 1) return (((g[q - 3] - 5. * g[q - 2]) + 19. * g[q - 1]) + 9. * g[q]) / 24.;
    return (13. * (g[q - 1] + g[q]) - (g[q - 2] + g[q + 1])) / 24.;
}

// inclusive scans of v over the 64 lanes of a wave, six levels: upwards lane t takes lane t - off, downwards lane t + off
__device__ __forceinline__ double wave_scan_up(double v, int lane)
{
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const double o = __shfl_up(v, off);
        if (lane >= off) v += o;
    }
    return v;
}
__device__ __forceinline__ double wave_scan_down(double v, int lane)
{
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const double o = __shfl_down(v, off);
        if (lane + off < 64) v += o;
    }
    return v;
}

// the lane's chain of increments d_i of the nodes i0 + j at the slots q0 + j (0 outside 1 .. N-1, or with `on` false), left to right
template <int kPer>
__device__ __forceinline__ double chain_up(const double* g, int q0, int i0, int N, bool on, double (&l)[kPer])
{
    double t = 0.;
#pragma unroll
    for (int j = 0; j < kPer; ++j) {
        const int i = i0 + j;
        const double d = (on && i >= 1 && i < N) ? increment(g, q0 + j, i, N) : 0.;
        t = j == 0 ? d : t + d;
        l[j] = t;
    }
    return t;
}
// mirrored: node i holds E_i = d_{i+1} (0 from N-1 on), chained from the lane's last node down
template <int kPer>
__device__ __forceinline__ double chain_down(const double* g, int q0, int i0, int N, double (&l)[kPer])
{
    double t = 0.;
#pragma unroll
    for (int j = kPer - 1; j >= 0; --j) {
        const int i = i0 + j;
        const double e = i < N - 1 ? increment(g, q0 + j + 1, i + 1, N) : 0.;
        t = j == kPer - 1 ? e : t + e;
        l[j] = t;
    }
    return t;
}

// before the barrier: the lanes' totals across the wave: inc up to and with this lane, ex the lanes before it (0 in the first); the kernel
// posts inc of the wave's last lane to LDS as the wave's total
struct LanePrefix { double inc, ex; };
__device__ __forceinline__ LanePrefix wave_prefix_up(double t, int lane)
{
    LanePrefix p;
    p.inc = wave_scan_up(t, lane);
    p.ex = __shfl_up(p.inc, 1);
    if (lane == 0) p.ex = 0.;
    return p;
}
__device__ __forceinline__ LanePrefix wave_prefix_down(double t, int lane)
{
    LanePrefix p;
    p.inc = wave_scan_down(t, lane);
    p.ex = __shfl_down(p.inc, 1);
    if (lane == 63) p.ex = 0.;
    return p;
}

// after the barrier: the four waves' totals chained, off for this wave and tot for the tile
struct TileSums { double off, tot; };
__device__ __forceinline__ TileSums waves_chain_up(const double* w, int wave)
{
    TileSums s;
    s.off = wave == 0 ? 0. : (wave == 1 ? w[0] : (wave == 2 ? w[0] + w[1] : (w[0] + w[1]) + w[2]));
    s.tot = ((w[0] + w[1]) + w[2]) + w[3];
    return s;
}
__device__ __forceinline__ TileSums waves_chain_down(const double* w, int wave)
{
    TileSums s;
    s.off = wave == 3 ? 0. : (wave == 2 ? w[3] : (wave == 1 ? w[3] + w[2] : (w[3] + w[2]) + w[1]));
    s.tot = ((w[3] + w[2]) + w[1]) + w[0];
    return s;
}

// the tree of a quadrature: the lanes of a wave by xor shuffles 32 .. 1 (every lane ends with the wave's sum), then the four waves'
// sums joined as (w0 + w1) + (w2 + w3)
__device__ __forceinline__ double wave_tree_sum(double v)
{
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}
__device__ __forceinline__ double waves_join(double w0, double w1, double w2, double w3) { return (w0 + w1) + (w2 + w3); }

}  // namespace dfta_radial
