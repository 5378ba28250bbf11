// poisson_kernels.inc -- the device code of poisson.hip (Atom, sweeps, transfers, cycle drivers, kernels), included twice:
// namespace mg_exact (DFTA_MG_KWARM = 96, DFTA_MG_KWARM3 = 112: every sweep equals the sequential one bit for bit) and
// namespace mg_tol (32 / 32: tolerance mode).  Not a translation unit of its own.
constexpr int kWarm = DFTA_MG_KWARM;
struct Atom {
    double* phi0;     // two copies of every level (global)
    double* phi1;
    double* src;
    double* lds;      // shared memory: [phi copy 0 | phi copy 1 | src], kSeqCap doubles each
    double* stage;    // shared memory: two arrays of kStageArr doubles (Phi, S) for the staged sweeps of one level visit
    unsigned cur;     // bit l: which copy of level l is current (identical in all threads)
    // group of G workgroups that share the fine levels of this atom (G == 1: none of this is touched)
    int g, G;               // member index, group size
    unsigned* ctr;          // monotonic arrival counter of the group (zeroed before the launch)
    unsigned bar;           // barriers passed so far
    double* part;           // [2][3][G] partial sums of the members (double-buffered by barrier parity) + [1] published `cur`
    double* fslot;          // [kGrpBuf][G] slots of the fast sum (group_sum_fast), sentinel-filled before the launch
    unsigned fseq;          // fast sums taken so far
    double* xchg;           // [kGrpBuf][G][kXchg] boundary nodes of the fast exchange, sentinel-filled before the launch
    int pend;               // > 0: the prolongation from this level is folded into the staged copy-in of the level below it
    int pend_r;             // > 0: the restriction TO this level is folded into its staged copy-in
    int pend_z;             // > 0: this level's Phi is zero and its source complete in global memory (written by the members of a resident group): staged as such
    int lds_holds;          // >= 0: the staging memory still holds this level as its last staged visit (stage 1) left it -- Phi equal to the current global copy, and the source
    int spin_max;           // polls of a group barrier before the waiting member gives up and raises the abort flag
    bool gave_up;           // this thread has timed out on a slot of group_sum_fast: it does not wait for that member again
    __device__ __forceinline__ int lane() const { return g * kThreads + static_cast<int>(threadIdx.x); }
    // pointer to storage element 0 of the level (generic address space: LDS for sequential levels, global otherwise)
    __device__ __forceinline__ double* cur_phi(int l, const Lvl& L) const
    {
        const unsigned c = (cur >> l) & 1u;
        return L.seq ? lds + c * kSeqCap + L.soff : (c ? phi1 : phi0) + L.off;
    }
    __device__ __forceinline__ double* other_phi(int l, const Lvl& L) const
    {
        const unsigned c = ((cur >> l) & 1u) ^ 1u;
        return L.seq ? lds + c * kSeqCap + L.soff : (c ? phi1 : phi0) + L.off;
    }
    __device__ __forceinline__ double* src_of(const Lvl& L) const { return L.seq ? lds + 2 * kSeqCap + L.soff : src + L.off; }
};

// Barrier of the G workgroups of an atom: every store made before it by any member is visible to every member after it
// (agent-scope release before the arrival, acquire after the last one; MI355X_MICROARCH.md: the per-XCD L2s are not
// coherent).  ~2 us for 8 members (profiles/microbench).  The spin is bounded so that a lost member cannot hang the GPU.
__device__ __forceinline__ void group_sync(Atom& A)
{
    if (A.G == 1) { __syncthreads(); return; }
    __syncthreads();
    ++A.bar;
    if (threadIdx.x == 0) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        __hip_atomic_fetch_add(A.ctr, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const unsigned target = A.bar * static_cast<unsigned>(A.G);
        // a member that never arrives (its workgroup was not scheduled: the group does not fit the free compute units)
        // must not hang the GPU: after ~1 s the waiting member raises the group's abort flag (the counter's top bit),
        // which releases every later barrier at once; the host sees the flag and reports the failure
        int spins = 0;
        unsigned seen;
        while ((seen = __hip_atomic_load(A.ctr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) < target) {
            __builtin_amdgcn_s_sleep(1);
            if (++spins > A.spin_max) { __hip_atomic_fetch_or(A.ctr, 0x80000000u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); break; }
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    }
    __syncthreads();
}

// Sum over the 64 lanes of a wave, returned in every lane: five DPP adds inside the rows of 16, two across them, a scalar broadcast of
// lane 63 (~150 cycles).  The `__shfl_xor` butterfly it replaces is twelve dependent ds_bpermute round trips for a double (~700 cycles) --
// paid once per sweep on the coarse levels and once per visit by every member.  The order of the additions differs from the butterfly's; it
// is the same for every caller, so all participants still take the same decisions (the norms only gate `err < errorMin`).
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ double wt_dpp(const double src)
{
    const long long x = __builtin_bit_cast(long long, src);
    const int lo = __builtin_amdgcn_update_dpp(0, (int)x, CTRL, ROW_MASK, 0xf, false);
    const int hi = __builtin_amdgcn_update_dpp(0, (int)(x >> 32), CTRL, ROW_MASK, 0xf, false);
    return __builtin_bit_cast(double, ((long long)hi << 32) | (unsigned)lo);
}
__device__ __forceinline__ double wave_total(double v)
{
    v += wt_dpp<0x111, 0xf>(v);      // row_shr:1
    v += wt_dpp<0x112, 0xf>(v);      // row_shr:2
    v += wt_dpp<0x114, 0xf>(v);      // row_shr:4
    v += wt_dpp<0x118, 0xf>(v);      // row_shr:8
    v += wt_dpp<0x142, 0xa>(v);      // row_bcast:15 into rows 1 and 3
    v += wt_dpp<0x143, 0xc>(v);      // row_bcast:31 into rows 2 and 3
    const long long x = __builtin_bit_cast(long long, v);
    const int lo = __builtin_amdgcn_readlane((int)x, 63), hi = __builtin_amdgcn_readlane((int)(x >> 32), 63);
    return __builtin_bit_cast(double, ((long long)hi << 32) | (unsigned)lo);
}

__device__ __forceinline__ double block_sum(double v, double* red)
{
    v = wave_total(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}

// Sum over all lanes of the group (cooperative levels): the members' block sums are exchanged through global memory around
// a group barrier and added in member order by everybody, so that every member takes the same decisions.
// `which` = 0..2 selects one of three concurrent sums (the fused three-sweep pass is never cooperative, kept for symmetry).
__device__ __forceinline__ double group_sum(Atom& A, double v, double* red)
{
    const double mine = block_sum(v, red);
    if (A.G == 1) return mine;
    double* slot = A.part + ((A.bar + 1) & 1u) * 3 * A.G;      // parity of the barrier that follows
    if (threadIdx.x == 0) slot[A.g] = mine;
    group_sync(A);
    double tot = 0;
    for (int m = 0; m < A.G; ++m) tot += slot[m];
    return tot;
}

// -DDFTA_POISSON_PROF: time (s_memtime ticks of workgroup 0) per operation kind and level, printed when the solver is destroyed
#ifdef DFTA_POISSON_PROF
#ifndef DFTA_PROF_BLOCK
#define DFTA_PROF_BLOCK 0          // the workgroup whose ticks are recorded (32: the coarse workgroup of atom 0 of the resident groups)
#endif
__device__ unsigned long long g_prof[8 * 24];
#define PROF_T0() const long long prof_t0 = clock64()
__device__ unsigned long long g_prof_member[64 * 4];     // per member of atom 0: ticks in the exchange / in the LDS sweeps (all shared levels)
#define PROF_ADD(cat, lvl) do { if (threadIdx.x == 0) { const unsigned long long dt_ = clock64() - prof_t0; \
        if (blockIdx.x == DFTA_PROF_BLOCK) g_prof[(cat) * 24 + (lvl)] += dt_; \
        if (blockIdx.x < 64 && ((cat) == 3 || (cat) == 4 || (cat) == 5)) g_prof_member[blockIdx.x * 4 + (cat) - 3] += dt_; } } while (0)
#else
#define PROF_T0()
#define PROF_ADD(cat, lvl)
#endif

// Sum over the group for the sweeps in the middle of a staged visit, where the members exchange only a partial sum and the
// <= 97 nodes next to their parts' boundaries.  Everything travels through agent-scope atomic stores into slots that hold a
// sentinel (a NaN with a payload no arithmetic produces) and is polled with agent-scope atomic loads until the sentinel is
// gone: coherent without cache maintenance, and every datum validates itself -- an agent-scope store can overtake an earlier
// one on its way to another XCD (measured), so "the sum has arrived" says nothing about the nodes.  One round trip for
// everything: while the first wave polls the G sums, the second and third poll the left neighbour's nodes straight into
// the halo columns and the fourth the right neighbour's first node (round 1: arrival counter, poll, read of the sums, then
// the nodes: three trips and two fences).  Three buffers rotate: when the sums of exchange s are complete everybody has
// read what it needed of exchange s-1 (they have all published s), so each member resets its part of that buffer; it is
// used again in exchange s+2, a whole sweep later.  Sums are added in member order, as in group_sum.
__device__ __forceinline__ double exchange_poll(Atom& A, const double* p)
{
    int spins = A.gave_up ? A.spin_max : 0;
    while (true) {
        const double x = __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (static_cast<unsigned long long>(__double_as_longlong(x)) != kFastSentinel) return x;
        if (++spins > A.spin_max) {      // a lost member must not hang the GPU: raise the group's abort flag
            __hip_atomic_fetch_or(A.ctr, 0x80000000u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            A.gave_up = true;
            return 0.0;
        }
        // somebody else has already given up on this group (the abort bit of the arrival counter): do not spin out the
        // whole bound again in every thread at every later exchange
        if ((spins & 1023) == 0 && (__hip_atomic_load(A.ctr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & 0x80000000u)) {
            A.gave_up = true;
            return 0.0;
        }
        __builtin_amdgcn_s_sleep(1);
    }
}
// this member's node `idx` of the exchange that travels with the next fast sum
__device__ __forceinline__ void exchange_store(Atom& A, int idx, double v)
{
    __hip_atomic_store(A.xchg + (static_cast<size_t>(A.fseq % kGrpBuf) * A.G + A.g) * kXchg + idx, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// PP: the staged part (element 0 = its first node); nhalo = Hc << logC nodes of the left neighbour go to the halo columns
// (node idx: row idx & (C-1), column -Hc + (idx >> logC)), the right neighbour's first node to PP[C * RS]
// FENCED: the sum that ends a visit, after the member has written its part out with plain stores -- a release before the sum
// is published and an acquire after the last one has arrived make those stores visible to every member (the next operation
// reads other members' columns with plain loads); no nodes travel with it.  One trip instead of the three of group_sum
// (arrival counter, poll, read of the slots).
template <int RS, bool FENCED = false>
__device__ __forceinline__ double group_sum_fast(Atom& A, double v, double* red, double* PP, int logC, int Hc)
{
    const double mine = block_sum(v, red);      // its barriers wait for every store of this member issued so far
    if (A.G == 1) return mine;
    const unsigned s = A.fseq++;
    const int tid = threadIdx.x, C = 1 << logC;
    if (tid < 64) {
        double* cur = A.fslot + (s % kGrpBuf) * A.G;
        if (FENCED && tid == 0) __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        if (tid == 0) __hip_atomic_store(cur + A.g, mine, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        double x = 0;
        if (tid < A.G) x = exchange_poll(A, cur + tid);
        double tot = 0;
        for (int m = 0; m < A.G; ++m) tot += __shfl(x, m);
        if (tid == 0) {
            if (FENCED) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            red[18] = tot;
            __hip_atomic_store(A.fslot + ((s + kGrpBuf / 2) % kGrpBuf) * A.G + A.g, __longlong_as_double(static_cast<long long>(kFastSentinel)),
                               __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    } else if (FENCED) {
    } else if (tid < 192) {
        const int idx = tid - 64;
        if (A.g > 0 && idx < (Hc << logC))
            PP[(idx & (C - 1)) * RS + (idx >> logC) - Hc] = exchange_poll(A, A.xchg + (static_cast<size_t>(s % kGrpBuf) * A.G + A.g - 1) * kXchg + idx);
    } else if (tid == 192) {
        if (A.g < A.G - 1) PP[C * RS] = exchange_poll(A, A.xchg + (static_cast<size_t>(s % kGrpBuf) * A.G + A.g + 1) * kXchg + kXchg - 1);
    }
    __syncthreads();
    if (tid < kXchg)
        __hip_atomic_store(A.xchg + (static_cast<size_t>((s + kGrpBuf / 2) % kGrpBuf) * A.G + A.g) * kXchg + tid,
                           __longlong_as_double(static_cast<long long>(kFastSentinel)), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return red[18];
}

__device__ __forceinline__ double gs_point(double s, double xm, double xp, double dh)
{
    // PoissonSolver.cpp:56-57; d * t * 0.5 == (0.5 d) * t exactly
    return 0.5 * (s + xm + xp - dh * (xp - xm));
}

// The same update with the recurrence carried as y = 2x: 0.5*y is exact, so fma(y, 0.5, s) = fl(s + x) and
// fma(y, -0.5, xp) = fl(xp - x) are the reference's roundings, and the dependent chain per node is three fp64 operations
// instead of four (the sweeps that run out of LDS are bound by exactly that latency: ~16 cycles per dependent operation).
// Returns 2 * gs_point(s, 0.5*y, xp, dh) before its (exact) halving.
__device__ __forceinline__ double gs_point2(double s, double y, double xp, double dh)
{
    const double t1 = __builtin_fma(y, 0.5, s);
    const double t2 = __builtin_fma(y, -0.5, xp);
    return (t1 + xp) - dh * t2;
}

// Chunked sweep of one level (S, pin, pout: storage element 0 of the level's source / current / other copy, in global
// memory or in LDS); LOGT = log2(lanes) as a compile-time constant (row strides become instruction offsets) or -1 for any
// value.  Returns this thread's share of sum dPhi^2.
template <int LOGT>
__device__ __forceinline__ double gs_chunked(const Lvl& L, const double* __restrict__ S, const double* __restrict__ pin,
                                             double* __restrict__ pout, const int tid, const double dh)
{
    double err2 = 0;
    {
        // chunked sweep: lane t owns nodes [t*C, t*C + C), all lanes step through their chunk in lockstep.  With
        // m = step number (m - W < 0: warm-up inside the previous lanes' chunks) the node of lane t is
        //     i = t*C + (m - W) = (t + tu)*C + ku,   ku = (m - W) & (C-1),  tu = (m - W) >> logC   (both wave-uniform)
        // so its storage index is ku*T + tu + t: a uniform base plus the lane id -- no per-lane address arithmetic.
        // Loads run kPF steps ahead of the recurrence in registers (two buffers), all of them unconditional: lanes
        // whose node index is still < 1 read in-bounds padding (kPad) and skip the update.
        const int logT = LOGT >= 0 ? LOGT : L.logT;
        const int T = 1 << logT, C = 1 << L.logC, logC = L.logC;
        if (tid < T) {
            const int lo = tid << logC;
            const int one_minus_lo = 1 - lo;
            // first node of this lane's run and its left neighbour (old value; the exact boundary value for node 0)
            const int i0 = (lo - kWarm) > 1 ? (lo - kWarm) : 1;
            double xm, old;
            {
                const int a0 = i0 - 1, a1 = i0;
                xm = pin[((a0 & (C - 1)) << logT) + (a0 >> logC)];
                old = pin[((a1 & (C - 1)) << logT) + (a1 >> logC)];
            }
            // right neighbour of the last owned node: node (t+1)*C, which is node n-1 (stored at C*T) for the last lane
            const double xp_end = pin[(tid == T - 1) ? (C << logT) : (tid + 1)];
            const int Cm1 = C - 1;
            const unsigned tu = static_cast<unsigned>(tid);
            // Every access is "wave-uniform row pointer + lane id" (scalar base register + 32-bit lane offset in the
            // load/store instruction): no per-lane address arithmetic on the VALU.
            auto row = [&](const double* base, int r) -> const double* {
                return base + (static_cast<long>((r & Cm1)) << logT) + (r >> logC);
            };
            // loads of step r (= m - W): S at node i(r), Phi_old at node i(r) + 1 = i(r+1); indices clamped to r <= C-1
            auto load8 = [&](double (&X)[kPF], double (&SV)[kPF], int rbase) {
                // a batch that neither wraps into the neighbouring lane's column nor runs past the chunk is 9 consecutive
                // rows: one base pointer per array, the row strides are instruction offsets
                if (LOGT >= 0 && C >= kPF && rbase + kPF <= Cm1 && ((rbase + kPF) & Cm1) != 0) {
                    const double* __restrict__ bs = row(S, rbase);
                    const double* __restrict__ bp = row(pin, rbase) + T;
#pragma unroll
                    for (int q = 0; q < kPF; ++q) {
                        SV[q] = bs[(q << logT) + tu];
                        X[q] = bp[(q << logT) + tu];
                    }
                    return;
                }
#pragma unroll
                for (int q = 0; q < kPF; ++q) {
                    int r0 = rbase + q;
                    r0 = r0 < Cm1 ? r0 : Cm1;
                    SV[q] = row(S, r0)[tu];
                    X[q] = row(pin, r0 + 1)[tu];
                }
            };
            // Only the first lanes of the workgroup ever see a node index < 1 (lo + r < 1: during the warm-up, and lane 0
            // at r = 0).  Their wave takes the `careful` variants, which keep xm with a select instead of an exec-mask
            // branch per node (a mask that depends on a compare costs a VALU -> SGPR -> EXEC round trip per step).
            const bool careful = __builtin_amdgcn_readfirstlane(lo) <= kWarm;
            // warm-up steps (r < 0): recurrence only
            auto warm8 = [&](auto CAREFUL, const double (&X)[kPF], const double (&SV)[kPF], int rbase) {
#pragma unroll
                for (int q = 0; q < kPF; ++q) {
                    const double x = gs_point(SV[q], xm, X[q], dh);
                    if (decltype(CAREFUL)::value) xm = (rbase + q >= one_minus_lo) ? x : xm;   // node index lo + r >= 1
                    else xm = x;
                }
            };
            // owned steps (0 <= r < C): recurrence, error norm, store.  FIRST: the batch that holds r = 0 (node 0 of lane 0
            // is a boundary value, not an unknown); LAST: the batch whose last node has xp_end as right neighbour
            auto main8 = [&](auto FIRST, auto LAST, const double (&X)[kPF], const double (&SV)[kPF], int rbase) {
                double* __restrict__ bo = pout + (static_cast<long>(rbase) << logT);   // rows rbase .. rbase+7 of the own chunk
#pragma unroll
                for (int q = 0; q < kPF; ++q) {
                    const int r0 = rbase + q;
                    const double xp = (decltype(LAST)::value && q == kPF - 1) ? xp_end : X[q];
                    const double x = gs_point(SV[q], xm, xp, dh);
                    double dif = old - x;
                    if (decltype(FIRST)::value && q == 0) {
                        const bool live = r0 >= one_minus_lo;
                        dif = live ? dif : 0.0;
                        xm = live ? x : xm;
                    } else {
                        xm = x;
                    }
                    err2 += dif * dif;
                    if (LOGT >= 0) bo[(q << logT) + tu] = x;             // node 0 (lane 0, r = 0) is rewritten below
                    else const_cast<double*>(row(pout, r0))[tu] = x;     // tu == 0 inside the own chunk
                    old = xp;
                }
            };
            using std::true_type;
            using std::false_type;
            double ax[kPF], as[kPF], bx[kPF], bs[kPF];
            static_assert(kWarm % (2 * kPF) == 0, "warm-up must be a whole number of A/B rounds");
            load8(ax, as, -kWarm);
            if (careful) {
                for (int r = -kWarm; r < 0; r += 2 * kPF) {
                    load8(bx, bs, r + kPF);
                    warm8(true_type{}, ax, as, r);
                    load8(ax, as, r + 2 * kPF);                          // the last one already fetches r = 0 .. kPF-1
                    warm8(true_type{}, bx, bs, r + kPF);
                }
            } else {
                for (int r = -kWarm; r < 0; r += 2 * kPF) {
                    load8(bx, bs, r + kPF);
                    warm8(false_type{}, ax, as, r);
                    load8(ax, as, r + 2 * kPF);
                    warm8(false_type{}, bx, bs, r + kPF);
                }
            }
            // Phi_old at the first owned node (the last warm-up step's right neighbour); lane 0 keeps the value loaded above
            if (lo >= 1) old = bx[kPF - 1];
            if (C >= 2 * kPF) {
                for (int r = 0; r < C; r += 2 * kPF) {
                    load8(bx, bs, r + kPF);
                    if (r == 0) main8(true_type{}, false_type{}, ax, as, r);
                    else        main8(false_type{}, false_type{}, ax, as, r);
                    load8(ax, as, r + 2 * kPF);
                    if (r + 2 * kPF >= C) main8(false_type{}, true_type{}, bx, bs, r + kPF);
                    else                  main8(false_type{}, false_type{}, bx, bs, r + kPF);
                }
            } else {
                // C = 1, 2, 4 or 8 owned nodes: ax/as hold r = 0 .. min(C, kPF) - 1 (clamped beyond)
                for (int r0 = 0; r0 < C; ++r0) {
                    if (r0 >= one_minus_lo) {
                        const int r1 = r0 + 1;
                        const double sv = S[(r0 << logT) + tid];
                        const double xp = (r0 == Cm1) ? xp_end : pin[(r1 << logT) + tid];
                        const double x = gs_point(sv, xm, xp, dh);
                        const double dif = old - x;
                        err2 += dif * dif;
                        pout[(r0 << logT) + tid] = x;
                        xm = x;
                        old = xp;
                    }
                }
            }
        }
        if (tid == 0) {
            pout[0] = pin[0];                                   // node 0
            pout[C << logT] = pin[C << logT];                   // node n-1
        }
    }
    return err2;
}

// Chunked sweep, IN PLACE, of (a workgroup's part of) a level staged in LDS: NT lanes, C = 2^LOGC nodes per lane; node
// t*C + k of the part lives at k*RS + t relative to SSbase / PPbase, lanes t < 0 (the 96 nodes in front of the part: the
// previous lanes' columns for RS == 256, halo columns otherwise) included; Phi of the node behind the part at C*RS.  Same
// arithmetic as gs_chunked.  A lone wave on a SIMD issues one instruction of any kind per ~4.5 cycles, so the step is
// priced in instructions: with C a compile-time constant every LDS access of a 16-step block is "per-lane base register +
// immediate offset" (the uniform part of the index, (q & (C-1))*RS + (q >> LOGC), is known at compile time; the base
// advances by 16/C per block) -- 2 reads + 6 flops per warm-up step, nothing else.  Everything a lane reads from other
// lanes' nodes (warm-up, start values, right neighbour of its last node) is read before the barrier in the middle, the
// owned nodes are overwritten after it.  lo_g = index of the lane's first node within the level.
// NT = lanes that sweep (256: the workgroup; 64: its first wave alone -- the barrier is then a wave-level fence).
template <int LOGC, int RS, int NT = kThreads>
__device__ __forceinline__ double gs_lds(const double* __restrict__ SSbase, double* __restrict__ PPbase, const int tid,
                                         const int lo_g, const double dh)
{
    constexpr int C = 1 << LOGC, Cm1 = C - 1, kH = 8;
    auto uoff = [](int q) constexpr -> int { return (q & Cm1) * RS + (q >> LOGC); };    // q >= 0
    // explicit LDS pointers, each pinned in its own register: otherwise the compiler rebuilds every address from one
    // base plus a literal (the arrays are > 64 KB apart, beyond the instruction offset) -- one VALU add per access
    typedef __attribute__((address_space(3))) double lds_f64;
    typedef __attribute__((address_space(3))) const double lds_cf64;
    lds_cf64* ps = (lds_cf64*)(SSbase) + tid;
    lds_f64* pp = (lds_f64*)(PPbase) + tid;
    asm volatile("" : "+v"(ps), "+v"(pp));
    // The warm-up covers the 95 nodes lo-95 .. lo-1, in blocks of BS = max(16, C) steps; step q of the block with base
    // node lo + Rb (Rb = -96, -96+BS, ..: multiples of C) handles node lo + Rb + q + 1.  It starts from the old value of
    // node lo-96.  Lanes whose run would begin below node 1 (the first 96/C lanes of the level) restart from the exact
    // boundary value at node 1: with the blocks shifted by one node against the chunk rows that can only happen at steps
    // with (q % C) == 0 -- one select per C steps instead of one per step.
    const int neg_lo = -lo_g;
    const double Y0 = 2.0 * PPbase[0];          // node 0 of the level (meaningful where a restart can happen at all)
    double y = 2.0 * pp[-(kWarm >> LOGC)];      // the recurrence is carried as y = 2x (gs_point2)
    const double xp_end = (tid == NT - 1) ? PPbase[C * RS] : pp[1];
    const double node0 = pp[0];
    lds_cf64* bs = ps - (kWarm >> LOGC);
    lds_cf64* bp = pp - (kWarm >> LOGC);
    double ax[kH], as[kH], bx[kH], bv[kH];
    constexpr int BS = C > 2 * kH ? C : 2 * kH;
    static_assert(kWarm % BS == 0, "warm-up must be a whole number of blocks");
    static_assert(BS <= 4 * kH, "chunks of more than 32 nodes are not staged");
    using std::integral_constant;
    auto load = [&](double (&X)[kH], double (&SV)[kH], auto HH) {
        constexpr int h = decltype(HH)::value;
#pragma unroll
        for (int q = 0; q < kH; ++q) { SV[q] = bs[uoff(h * kH + q + 1)]; X[q] = bp[uoff(h * kH + q + 2)]; }
    };
    auto load_own = [&](double (&X)[kH], double (&SV)[kH]) {     // rows 0 .. 7 of the own chunk (bs == ps, bp == pp by then)
#pragma unroll
        for (int q = 0; q < kH; ++q) { SV[q] = bs[uoff(q)]; X[q] = bp[uoff(q + 1)]; }
    };
    auto warm = [&](const double (&X)[kH], const double (&SV)[kH], int Rb, auto HH, auto NSTEPS) {
        constexpr int h = decltype(HH)::value;
#pragma unroll
        for (int q = 0; q < decltype(NSTEPS)::value; ++q) {
            if ((h * kH + q) % C == 0) y = (Rb + (h * kH + q) == neg_lo) ? Y0 : y;      // this step is node 1
            y = gs_point2(SV[q], y, X[q], dh);
        }
    };
    auto block = [&](int Rb, auto LAST) {
        // halves 0, 2 in A, 1, 3 in B; the reads stay a whole half block ahead of their use
        constexpr bool last = decltype(LAST)::value;
        auto pair = [&](auto H0) {
            constexpr int h = decltype(H0)::value;
            constexpr bool wraps = (h + 2) * kH >= BS;
            load(bx, bv, integral_constant<int, h + 1>{});
            __builtin_amdgcn_sched_barrier(0);
            warm(ax, as, Rb, integral_constant<int, h>{}, integral_constant<int, kH>{});
            if constexpr (!wraps) {
                load(ax, as, integral_constant<int, h + 2>{});
            } else {
                bs += BS >> LOGC;
                bp += BS >> LOGC;
                asm volatile("" : "+v"(bs), "+v"(bp));
                if constexpr (last) load_own(ax, as);
                else load(ax, as, integral_constant<int, 0>{});
            }
            __builtin_amdgcn_sched_barrier(0);
            warm(bx, bv, Rb, integral_constant<int, h + 1>{}, integral_constant<int, (last && wraps) ? kH - 1 : kH>{});
        };
        pair(integral_constant<int, 0>{});
        if constexpr (BS > 2 * kH) pair(integral_constant<int, 2>{});
    };
    load(ax, as, integral_constant<int, 0>{});
    for (int Rb = -kWarm; Rb < -BS; Rb += BS) block(Rb, std::false_type{});
    block(-BS, std::true_type{});
    double old = bx[kH - 2];                    // Phi_old at the first owned node: the right neighbour of the last warm-up step
    // node 1 as a lane's FIRST node (C == 1, lane 1): its restart falls on the step that the warm-up leaves to the owned part
    if constexpr (C == 1) y = (lo_g == 1) ? Y0 : y;
    // all reads of other lanes' old values are done
    if constexpr (NT == kThreads) __syncthreads();
    else { __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront"); __builtin_amdgcn_wave_barrier(); }
    double err2 = 0;
    auto own = [&](const double (&X)[kH], const double (&SV)[kH], int r0) {
#pragma unroll
        for (int q = 0; q < (C < kH ? C : kH); ++q) {
            const int r = r0 + q;
            const double xp = (r == Cm1) ? xp_end : X[q];
            const double yn = gs_point2(SV[q], y, xp, dh);
            const double x = 0.5 * yn;
            double dif = old - x;
            if (r == 0) {
                const bool live = lo_g >= 1;    // node 0 is a boundary value, not an unknown
                dif = live ? dif : 0.0;
                y = live ? yn : Y0;             // the lane of node 0 continues from the boundary value
            } else {
                y = yn;
            }
            err2 += dif * dif;
            pp[r * RS] = x;                     // node 0 is restored below
            old = xp;
        }
    };
    if constexpr (C <= kH) {
        own(ax, as, 0);
    } else {
        // rows r .. r+7 in A (fetched by the last warm-up block for r = 0), r+8 .. r+15 in B
#pragma unroll
        for (int r = 0; r < C; r += 2 * kH) {
#pragma unroll
            for (int q = 0; q < kH; ++q) { bv[q] = ps[(r + kH + q) * RS]; bx[q] = pp[((r + kH + q + 1) & Cm1) * RS]; }
            __builtin_amdgcn_sched_barrier(0);
            own(ax, as, r);
            if (r + 2 * kH < C) {
#pragma unroll
                for (int q = 0; q < kH; ++q) { as[q] = ps[(r + 2 * kH + q) * RS]; ax[q] = pp[(r + 2 * kH + q + 1) * RS]; }
            }
            __builtin_amdgcn_sched_barrier(0);
            own(bx, bv, r + kH);
        }
    }
    if (lo_g == 0) pp[0] = node0;
    return err2;
}

// ---- fused visit -------------------------------------------------------------------------------------------------
// The three sweeps of IterateGaussSeidel(level, errorMin, 3) (PoissonSolver.cpp:66-77) in ONE in-place pass over a part staged in
// LDS.  Sweep k+1 at node j needs sweep k at node j+1, so the three sweeps run as a software pipeline: at the step with stage-1
// node tau the lane computes
//     x1[tau]   = gs(S[tau],   x1[tau-1], x0[tau+1])
//     x2[tau-1] = gs(S[tau-1], x2[tau-2], x1[tau])
//     x3[tau-2] = gs(S[tau-2], x3[tau-3], x2[tau-1])
// with the arithmetic of gs_point2, i.e. exactly what three sequential sweeps compute.  All three stages start kWarm3 nodes in front
// of the lane's chunk from old values: a start-value error e decays as e b^j in stage 1, (1 + j/4) e b^j in stage 2 (which also
// feeds on stage 1's error) and (1 + j/4 + j^2/32) e b^j in stage 3, b = (1 + d/2)/2; at j = 112 the third factor is 2^8.7 and
// b^(112-95) <= 2^-16: a wider margin than the single sweep's 95 nodes.  The lane runs two nodes past its chunk (x1, x2 of the right
// neighbour's first nodes, from old values read before the barrier).  One LDS read pair per step instead of three, no barrier and --
// for a part shared by a group -- no exchange between the sweeps.  KST = which sweep's values are stored (3; 1 or 2 when the
// reference would have stopped early: the caller restores the old values and repeats the pass).
// Layout as gs_lds: node lo + r of lane tid at (r & (C-1)) * RS + (r >> LOGC) relative to the lane's column; the three nodes
// behind the chunk of lane NT-1 are rows 0..2 of column NT (a right halo column) unless `last_lane`: then the chunk ends at the
// level's last node, whose value is xN.  Returns the lane's shares of the three sums of dPhi^2.
constexpr int kWarm3 = DFTA_MG_KWARM3;
// gs_point2 with the right neighbour given as yp = 2 xp as well (stages 2 and 3 of the fused pass, which take it from the stage in
// front of them): halving commutes with every rounding involved -- fl(xp - x) = fl(yp - y) / 2, fl(t1 + xp) = fma(yp, 0.5, t1),
// dh fl(xp - x) = (dh / 2) fl(yp - y) -- so the result is gs_point2(s, y, yp / 2, dh) bit for bit, one instruction less.
__device__ __forceinline__ double gs_point2y(double s, double y, double yp, double dh2)
{
    const double t1 = __builtin_fma(y, 0.5, s);
    const double u = yp - y;
    const double a = __builtin_fma(yp, 0.5, t1);
    return a - dh2 * u;
}
// RIGHT: the part has no halo column behind it (a member's staged part of a shared level): lane NT-1 takes the old values of the three
// nodes behind its chunk and the sources of the first two from rightP[0..2] / rightS[0..1] instead.
// WARM: the warm-up's length.  PRED (cs_visit3, with a WARM shorter than kWarm3): the stages start from hs[0..2] -- predictions of twice
// x1[lo-W-1], x2[lo-W-2], x3[lo-W-3] -- instead of from old values, and the lane reports its pipeline state (y1, y2, y3) as it enters its
// chunk (hs[3..5]: twice x1[lo-1], x2[lo-2], x3[lo-3], from its warm-up) and as it leaves it (hs[6..8]: the same nodes of the lane
// behind it, from its own chunk) for the caller's hand-over check.
template <int LOGC, int RS, int NT, int KST, bool CAREFUL, bool RIGHT = false, int WARM = kWarm3, bool PRED = false>
__device__ __forceinline__ void gs_lds3(const double* __restrict__ SSbase, double* __restrict__ PPbase, const int tid, const int lo_g,
                                        const bool last_lane, const double xN, const double dh, double& e1, double& e2, double& e3,
                                        const double* rightP = nullptr, const double* rightS = nullptr, double* hs = nullptr)
{
    constexpr int C = 1 << LOGC, Cm1 = C - 1, kH = 8, W = WARM;
    static_assert(C >= 4 && C <= 32 && W % (2 * kH) == 0, "fused pass: 4..32 nodes per lane");
    typedef __attribute__((address_space(3))) double lds_f64;
    typedef __attribute__((address_space(3))) const double lds_cf64;
    const bool active = tid < NT;
    lds_cf64* ps = (lds_cf64*)(SSbase) + tid;
    lds_f64* pp = (lds_f64*)(PPbase) + tid;
    asm volatile("" : "+v"(ps), "+v"(pp));
    auto off = [](int r) constexpr -> int { return (r & Cm1) * RS + (r >> LOGC); };       // any r (arithmetic shift = floor)
    const int neg_lo = -lo_g;
    const double dh2 = 0.5 * dh;
    const double Y0 = 2.0 * PPbase[0];          // node 0 of the level (meaningful where a restart can happen at all)
    double a1 = 0, a2 = 0, a3 = 0;              // a2, a3 are accumulated on doubled differences: four times the sums (exactly)
    double y1 = 0, y2 = 0, y3 = 0, sA = 0, sB = 0, o0 = 0, y1p = 0, y2p = 0;
    double xr0 = 0, xr1 = 0, xr2 = 0, sr0 = 0, sr1 = 0;
    double ax[kH], as[kH], bx[kH], bv[kH];
    // loads of the batch of 8 steps whose stage-1 nodes are lo + r0 .. lo + r0 + 7 (r0 a multiple of 8): S at the node, old Phi at
    // the node behind it.  r0 is wave-uniform: one base per array and batch, the rows are instruction offsets.
    auto load = [&](double (&X)[kH], double (&SV)[kH], const int r0) {
        const int col = r0 >> LOGC;
        if constexpr (C <= kH) {
            lds_cf64* bs = ps + col;
            lds_cf64* bp = (lds_cf64*)pp + col;
#pragma unroll
            for (int q = 0; q < kH; ++q) { SV[q] = bs[off(q)]; X[q] = bp[off(q + 1)]; }
        } else {
            const int k0 = r0 & Cm1;
            lds_cf64* bs = ps + (k0 * RS + col);
            lds_cf64* bp = (lds_cf64*)pp + (k0 * RS + col);
#pragma unroll
            for (int q = 0; q < kH; ++q) SV[q] = bs[q * RS];
#pragma unroll
            for (int q = 0; q < kH - 1; ++q) X[q] = bp[(q + 1) * RS];
            lds_cf64* bw = (k0 + kH == C) ? (lds_cf64*)pp + (col + 1) : bp + kH * RS;     // the next column's first row
            X[kH - 1] = *bw;
        }
    };
    // warm-up batch: recurrences only (15 instructions per step)
    auto warm = [&](const double (&X)[kH], const double (&SV)[kH], const int r0) {
#pragma unroll
        for (int q = 0; q < kH; ++q) {
            double t = gs_point2(SV[q], y1, X[q], dh);
            if (CAREFUL && ((q & (C < kH ? Cm1 : kH - 1)) == 0)) t = (r0 + q == neg_lo) ? Y0 : t;           // stage 1 stands on node 0
            double u = gs_point2y(sA, y2, t, dh2);
            if (CAREFUL && (((q - 1) & (C < kH ? Cm1 : kH - 1)) == 0)) u = (r0 + q - 1 == neg_lo) ? Y0 : u;
            double v = gs_point2y(sB, y3, u, dh2);
            if (CAREFUL && (((q - 2) & (C < kH ? Cm1 : kH - 1)) == 0)) v = (r0 + q - 2 == neg_lo) ? Y0 : v;
            y1 = t; y2 = u; y3 = v;
            sB = sA; sA = SV[q];
        }
        o0 = X[kH - 1];
    };
    // own batch: recurrences, error norms, the store of sweep KST's values
    auto own = [&](auto FIRST, const double (&X)[kH], const double (&SV)[kH], const int r0) {
        constexpr bool first = decltype(FIRST)::value;
        constexpr int nq = C < kH ? C : kH;
        lds_f64* po = pp + r0 * RS;
#pragma unroll
        for (int q = 0; q < nq; ++q) {
            const double xn = (q == nq - 1) ? ((r0 + nq == C) ? xr0 : X[q]) : X[q];
            double t = gs_point2(SV[q], y1, xn, dh);
            if (CAREFUL && first && q == 0) t = (lo_g == 0) ? Y0 : t;
            { const double d = __builtin_fma(t, -0.5, o0); a1 = __builtin_fma(d, d, a1); }
            double u = gs_point2y(sA, y2, t, dh2);
            if (CAREFUL && first && q == 1) u = (lo_g == 0) ? Y0 : u;
            if (!(first && q == 0)) { const double d = y1p - u; a2 = __builtin_fma(d, d, a2); }
            double v = gs_point2y(sB, y3, u, dh2);
            if (CAREFUL && first && q == 2) v = (lo_g == 0) ? Y0 : v;
            if (!(first && q < 2)) { const double d = y2p - v; a3 = __builtin_fma(d, d, a3); }
            if (KST == 1) po[q * RS] = 0.5 * t;
            if (KST == 2 && !(first && q == 0)) po[(q - 1) * RS] = 0.5 * u;
            if (KST == 3 && !(first && q < 2)) po[(q - 2) * RS] = 0.5 * v;
            y1 = t; y2 = u; y3 = v;
            sB = sA; sA = SV[q];
            o0 = xn; y1p = t; y2p = u;
        }
    };
    if (active) {
        if constexpr (PRED) { y1 = hs[0]; y2 = hs[1]; y3 = hs[2]; }
        else { y1 = 2.0 * pp[off(-W - 1)]; y2 = 2.0 * pp[off(-W - 2)]; y3 = 2.0 * pp[off(-W - 3)]; }
        sA = ps[off(-W - 1)]; sB = ps[off(-W - 2)];
        load(ax, as, -W);
        for (int r0 = -W; r0 < 0; r0 += 2 * kH) {
            load(bx, bv, r0 + kH);
            __builtin_amdgcn_sched_barrier(0);
            warm(ax, as, r0);
            load(ax, as, r0 + 2 * kH);                  // the last one fetches the first own batch (still old values)
            __builtin_amdgcn_sched_barrier(0);
            warm(bx, bv, r0 + kH);
        }
        y1p = y1; y2p = y2;
        if constexpr (PRED) { hs[3] = y1; hs[4] = y2; hs[5] = y3; }
        // old values behind the chunk: the right neighbour overwrites them after the barrier
        xr0 = last_lane ? xN : pp[off(C)];
        xr1 = pp[off(C + 1)]; xr2 = pp[off(C + 2)];
        sr0 = ps[off(C)]; sr1 = ps[off(C + 1)];
        if (RIGHT && tid == NT - 1 && !last_lane) { xr0 = rightP[0]; xr1 = rightP[1]; xr2 = rightP[2]; sr0 = rightS[0]; sr1 = rightS[1]; }
    }
    // all reads of other lanes' old values are done
    if constexpr (NT <= 64) { __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront"); __builtin_amdgcn_wave_barrier(); }
    else __syncthreads();
    if (active) {
        if constexpr (C <= kH) {
            own(std::true_type{}, ax, as, 0);
        } else {
            for (int r0 = 0; r0 < C; r0 += 2 * kH) {
                load(bx, bv, r0 + kH);
                __builtin_amdgcn_sched_barrier(0);
                if (r0 == 0) own(std::true_type{}, ax, as, 0); else own(std::false_type{}, ax, as, r0);
                if (r0 + 2 * kH < C) load(ax, as, r0 + 2 * kH);
                __builtin_amdgcn_sched_barrier(0);
                own(std::false_type{}, bx, bv, r0 + kH);
            }
        }
        if constexpr (PRED) { hs[6] = y1; hs[7] = y2; hs[8] = y3; }
        if (KST >= 2) {
            // two steps behind the chunk: x1 (x2) of the right neighbour's first node(s) from the old values read above; a chunk that
            // ends at the level's last node finds the boundary value there
            const double Y_N = 2.0 * xN;
            double t = gs_point2(sr0, y1, xr1, dh);
            t = last_lane ? Y_N : t;
            double u = gs_point2y(sA, y2, t, dh2);
            { const double d = y1p - u; a2 = __builtin_fma(d, d, a2); }
            if (KST == 2) pp[Cm1 * RS] = 0.5 * u;
            if (KST == 3) {
                double v = gs_point2y(sB, y3, u, dh2);
                { const double d = y2p - v; a3 = __builtin_fma(d, d, a3); }
                pp[(C - 2) * RS] = 0.5 * v;
                y1 = t; y2 = u; y3 = v; sB = sA; sA = sr0; y2p = u;
                t = gs_point2(sr1, y1, xr2, dh);
                u = gs_point2y(sA, y2, t, dh2);
                u = last_lane ? Y_N : u;
                v = gs_point2y(sB, y3, u, dh2);
                { const double d = y2p - v; a3 = __builtin_fma(d, d, a3); }
                pp[Cm1 * RS] = 0.5 * v;
            }
        }
    }
    e1 = a1; e2 = 0.25 * a2; e3 = 0.25 * a3;
}

// ---- predicted start values of the one-wave levels' fused visits (exact mode; the argument stands above cs_visit3) ----------------
constexpr int kPredW = 32;                         // the warm-up of a visit that starts from predictions
constexpr bool kPredict = kWarm3 > kPredW;         // the tolerance kernels start from old values 32 nodes ahead by design

// lane t <- v of lane t-1 (DPP wave_shr:1 on both halves), lane 0 keeps `keep`
__device__ __forceinline__ double lane_shr1(double keep, double v)
{
    const long long k = __builtin_bit_cast(long long, keep), x = __builtin_bit_cast(long long, v);
    const int lo = __builtin_amdgcn_update_dpp((int)k, (int)x, 0x138, 0xf, 0xf, false);
    const int hi = __builtin_amdgcn_update_dpp((int)(k >> 32), (int)(x >> 32), 0x138, 0xf, 0xf, false);
    return __builtin_bit_cast(double, ((long long)hi << 32) | (unsigned)lo);
}
// lane t <- v of lane t+1 (DPP wave_shl:1 on both halves), lane 63 keeps `keep`
__device__ __forceinline__ double lane_shl1(double keep, double v)
{
    const long long k = __builtin_bit_cast(long long, keep), x = __builtin_bit_cast(long long, v);
    const int lo = __builtin_amdgcn_update_dpp((int)k, (int)x, 0x130, 0xf, 0xf, false);
    const int hi = __builtin_amdgcn_update_dpp((int)(k >> 32), (int)(x >> 32), 0x130, 0xf, 0xf, false);
    return __builtin_bit_cast(double, ((long long)hi << 32) | (unsigned)lo);
}

// One sweep of an LDS-resident level by ONE thread, in the reference's order.  The loads of a batch (right neighbours,
// sources) are independent of the recurrence: they are issued together ahead of it, so that the chain is not one LDS
// round trip per node.  Returns sum dPhi^2.
__device__ __forceinline__ double seq_sweep(const double* __restrict__ S, const double* __restrict__ pin, double* __restrict__ pout,
                                            const int n, const double dh)
{
    double err2 = 0;
    const double x0 = pin[0];
    pout[0] = x0;
    double y = 2.0 * x0;                // the recurrence is carried as y = 2x (gs_point2: a shorter dependent chain)
    const int limit = n - 1;
    double old = pin[1];
    constexpr int kB = 8;
    int i = 1;
    for (; i + kB <= limit; i += kB) {
        double xp[kB], sv[kB], xo[kB];
#pragma unroll
        for (int q = 0; q < kB; ++q) { xp[q] = pin[i + q + 1]; sv[q] = S[i + q]; }
#pragma unroll
        for (int q = 0; q < kB; ++q) {
            y = gs_point2(sv[q], y, xp[q], dh);
            const double x = 0.5 * y;
            const double dif = old - x;
            err2 += dif * dif;
            xo[q] = x;
            old = xp[q];
        }
#pragma unroll
        for (int q = 0; q < kB; ++q) pout[i + q] = xo[q];
    }
    for (; i < limit; ++i) {
        const double xp = pin[i + 1];
        y = gs_point2(S[i], y, xp, dh);
        const double x = 0.5 * y;
        const double dif = old - x;
        err2 += dif * dif;
        pout[i] = x;
        old = xp;
    }
    pout[limit] = pin[limit];
    return err2;
}

// one lexicographic Gauss-Seidel sweep of level l: PoissonSolver::GaussSeidel (PoissonSolver.cpp:40-64).
// returns ||dPhi||_2 (same value in every thread)
__device__ __forceinline__ double gauss_seidel(const MgDesc& D, Atom& A, int l, double* red)
{
    const Lvl L = D.lv[l];
    const double dh = L.d * 0.5;
    double err2 = 0;
    const bool coop = l < D.kcoop;         // swept by the whole group: lane ids run over all members
    const int tid = coop ? A.lane() : static_cast<int>(threadIdx.x);
    if (L.seq) {
        if (tid == 0) err2 = seq_sweep(A.src_of(L), A.cur_phi(l, L), A.other_phi(l, L), L.n, dh);
    } else {
        const double* S = A.src + L.off;
        const double* pin = (((A.cur >> l) & 1u) ? A.phi1 : A.phi0) + L.off;
        double* pout = (((A.cur >> l) & 1u) ? A.phi0 : A.phi1) + L.off;
        err2 = gs_chunked<-1>(L, S, pin, pout, tid, dh);
    }
    A.cur ^= (1u << l);
    // also orders the writes of this sweep before the next phase (group barrier inside for cooperative levels)
    const double tot = coop ? group_sum(A, err2, red) : block_sum(err2, red);
    return sqrt(tot);
}

// Three consecutive Gauss-Seidel sweeps of a chunked level in ONE pass over memory (the smoother is bound by the
// CU's vector-memory pipe: fusing cuts its traffic to a third).  Sweep k+1 at node j needs sweep k at node j+1, so the
// three sweeps run as a software pipeline: at step tau the lane computes
//     x1[tau]   = gs(S[tau],   x1[tau-1], x0[tau+1])
//     x2[tau-1] = gs(S[tau-1], x2[tau-2], x1[tau])
//     x3[tau-2] = gs(S[tau-2], x3[tau-3], x2[tau-1])
// i.e. exactly the arithmetic of three sequential sweeps.  Each lane starts kWarm3 nodes before its chunk, all three stages at
// once from old values (the error analysis of gs_lds3 below: a start-value error e is down to (1 + j/4 + j^2/32) e b^j in the
// third stage after j nodes, b = (1 + d/2)/2 -- 112 nodes leave a wider margin than the single sweep's 95; rounds 1-2 started
// 3 x 96 nodes ahead, which made the pass pay only from 512 nodes per lane on) and runs 2 nodes past it (recomputing what its
// right neighbour computes).  The input copy stays untouched (the result goes to the other
// copy), so when the reference would have stopped after the first or second sweep (err < errorMin) the caller redoes
// the visit with single sweeps.  Returns the three error norms of PoissonSolver::GaussSeidel.
#ifndef DFTA_MG_PF3
#define DFTA_MG_PF3 16
#endif
constexpr int kPF3 = DFTA_MG_PF3;           // register prefetch depth of the fused global pass (steps per batch, two batches in flight)
// the three norms of a fused visit over the group: the members' partial sums (the same value in every thread of a member), added in
// member order by everybody (as group_sum does); the barrier also orders the pass's writes before the next phase
__device__ __forceinline__ void group_norms3(Atom& A, double s1, double s2, double s3, double& e1, double& e2, double& e3)
{
    double* slot = A.part + ((A.bar + 1) & 1u) * 3 * A.G;
    if (threadIdx.x == 0) { slot[A.g] = s1; slot[A.G + A.g] = s2; slot[2 * A.G + A.g] = s3; }
    group_sync(A);
    double t1 = 0, t2 = 0, t3 = 0;
    for (int m = 0; m < A.G; ++m) { t1 += slot[m]; t2 += slot[A.G + m]; t3 += slot[2 * A.G + m]; }
    e1 = sqrt(t1); e2 = sqrt(t2); e3 = sqrt(t3);
}
constexpr int kWarm3g = DFTA_MG_KWARM3;      // = kWarm3 (defined with gs_lds3 further down)
// COOP: a level shared by the G workgroups of an atom (lanes run over all members): the pass reads only OLD values of other lanes and
// writes the other copy, so the members need nothing from each other until the three norms -- one group barrier per visit instead of three.
template <bool COOP>
__device__ __forceinline__ void gs_fused3(const MgDesc& D, Atom& A, int l, double* red, double& e1, double& e2, double& e3)
{
    const Lvl L = D.lv[l];
    const double dh = L.d * 0.5;
    const int tid = COOP ? A.lane() : static_cast<int>(threadIdx.x);
    const int T = 1 << L.logT, C = 1 << L.logC, logC = L.logC, logT = L.logT, Cm1 = C - 1;
    const int n = L.n;
    const double* __restrict__ S = A.src + L.off;
    const double* __restrict__ pin = (((A.cur >> l) & 1u) ? A.phi1 : A.phi0) + L.off;
    double* __restrict__ pout = (((A.cur >> l) & 1u) ? A.phi0 : A.phi1) + L.off;
    double a1 = 0, a2 = 0, a3 = 0;
    if (tid < T) {
        const int lo = tid << logC;
        const int nsteps = (C + kWarm3g + 2 + kPF3 - 1) / kPF3 * kPF3;        // whole prefetch batches; extra steps = extra warm-up
        const int rstart = (C + 1) - (nsteps - 1);                           // stage-1 node offset of the first step (<= -3W)
        const double b0 = pin[0], bN = pin[C << logT];                        // fixed values at node 0 and node n-1
        auto old_at = [&](int j) -> double {
            if (j <= 0) return b0;
            if (j >= n - 1) return bN;
            return pin[((j & Cm1) << logT) + (j >> logC)];
        };
        auto src_at = [&](int j) -> double {
            if (j <= 0 || j >= n - 1) return 0.0;
            return S[((j & Cm1) << logT) + (j >> logC)];
        };
        // pipeline state: left neighbours = values of the previous step; old values and sources of the last three nodes
        const int t0 = lo + rstart;                         // stage-1 node of the first step
        double x1m = old_at(t0 - 1), x2m = old_at(t0 - 2), x3m = old_at(t0 - 3);
        double o0 = old_at(t0), o1 = old_at(t0 - 1), o2 = old_at(t0 - 2);
        double sA = src_at(t0 - 1), sB = src_at(t0 - 2);
        // Fixed nodes.  Left: a stage is inactive (its value stays b0) while its node index is < 1, i.e. while
        // r - (k-1) < rs with rs = 1 - lo; only lanes whose warm-up reaches below node 1 are concerned and only in the
        // first batches of their wave.  Right: only the last lane, in the last two steps (nodes n-1, n).  Batches that
        // touch neither run the unguarded step.
        const int rs = 1 - lo;
        if (t0 - 1 < 1) { x1m = b0; }                       // stage values at nodes <= 0 are the boundary value
        if (t0 - 2 < 1) { x2m = b0; }
        if (t0 - 3 < 1) { x3m = b0; }
        const int wave_first_lo = (tid & ~63) << logC;
        const int rs_wave = 1 - wave_first_lo;             // largest rs in this wave
        const bool wave_has_last = ((tid | 63) >= T - 1) && ((tid & ~63) <= T - 1);

        // loads of the step with stage-1 offset r: S at node lo+r, old Phi at node lo+r+1 (rows are wave-uniform)
        auto load8 = [&](double (&X)[kPF3], double (&SV)[kPF3], int rbase) {
#pragma unroll
            for (int q = 0; q < kPF3; ++q) {
                int r0 = rbase + q;
                r0 = r0 < C + 1 ? r0 : C + 1;
                const int r1 = r0 + 1;
                SV[q] = S[(((r0 & Cm1) << logT) + (r0 >> logC)) + tid];
                X[q] = pin[(((r1 & Cm1) << logT) + (r1 >> logC)) + tid];
            }
        };
        // MODE 0: no fixed node in this batch; 1: left end only (stage activation by predicate); 2: anything (selects)
        auto step8 = [&](const double (&X)[kPF3], const double (&SV)[kPF3], int rbase, const int mode) {
#pragma unroll
            for (int q = 0; q < kPF3; ++q) {
                const int r = rbase + q;               // stage-1 node offset (wave-uniform)
                double xn = X[q];                      // old value at node tau + 1
                const double s0 = SV[q];
                double x1, x2, x3;
                bool u1 = true, u2 = true, u3 = true;
                if (mode == 0) {
                    x1 = gs_point(s0, x1m, xn, dh);
                    x2 = gs_point(sA, x2m, x1, dh);
                    x3 = gs_point(sB, x3m, x2, dh);
                } else if (mode == 1) {
                    u1 = (r >= rs); u2 = (r - 1 >= rs); u3 = (r - 2 >= rs);
                    x1 = x1m; x2 = x2m; x3 = x3m;      // == b0 while the stage has not started
                    if (u1) x1 = gs_point(s0, x1m, xn, dh);
                    if (u2) x2 = gs_point(sA, x2m, x1, dh);
                    if (u3) x3 = gs_point(sB, x3m, x2, dh);
                } else {
                    const int tau = lo + r;
                    if (tau + 1 >= n - 1) xn = bN;
                    if (tau + 1 <= 0) xn = b0;
                    u1 = (tau >= 1) && (tau <= n - 2);
                    u2 = (tau - 1 >= 1) && (tau - 1 <= n - 2);
                    u3 = (tau - 2 >= 1) && (tau - 2 <= n - 2);
                    x1 = u1 ? gs_point(s0, x1m, xn, dh) : ((tau <= 0) ? b0 : ((tau >= n - 1) ? bN : o0));
                    x2 = u2 ? gs_point(sA, x2m, x1, dh) : ((tau - 1 <= 0) ? b0 : ((tau - 1 >= n - 1) ? bN : o1));
                    x3 = u3 ? gs_point(sB, x3m, x2, dh) : ((tau - 2 <= 0) ? b0 : ((tau - 2 >= n - 1) ? bN : o2));
                }
                // error norms and the store, own nodes only (wave-uniform ranges); x1m / x2m still hold the stage values
                // of the previous step, which are x1[tau-1] and x2[tau-2]
                if (r >= 0 && r <= Cm1) { if (u1) { const double dd = o0 - x1; a1 = __builtin_fma(dd, dd, a1); } }
                if (r >= 1 && r <= C) { if (u2) { const double dd = x1m - x2; a2 = __builtin_fma(dd, dd, a2); } }
                if (r >= 2 && r <= C + 1) {
                    if (u3) { const double dd = x2m - x3; a3 = __builtin_fma(dd, dd, a3); pout[(((r - 2) & Cm1) << logT) + tid] = x3; }
                }
                x1m = x1; x2m = x2; x3m = x3;
                sB = sA; sA = s0;
                o2 = o1; o1 = o0; o0 = xn;
            }
        };
        auto mode_of = [&](int rbase) -> int {
            const bool left = (rbase - 2 < rs_wave);                          // some stage of some lane below node 1
            const bool right = wave_has_last && (rbase + kPF3 - 1 >= Cm1);      // last lane at / beyond node n-2
            return right ? 2 : (left ? 1 : 0);
        };
        double ax[kPF3], as[kPF3], bx[kPF3], bs[kPF3];
        load8(ax, as, rstart);
        for (int r = rstart; r <= C + 1; r += 2 * kPF3) {
            load8(bx, bs, r + kPF3);
            {
                const int m = mode_of(r);
                if (m == 0) step8(ax, as, r, 0); else if (m == 1) step8(ax, as, r, 1); else step8(ax, as, r, 2);
            }
            if (r + kPF3 > C + 1) break;
            load8(ax, as, r + 2 * kPF3);
            {
                const int m = mode_of(r + kPF3);
                if (m == 0) step8(bx, bs, r + kPF3, 0); else if (m == 1) step8(bx, bs, r + kPF3, 1); else step8(bx, bs, r + kPF3, 2);
            }
        }
    }
    if (tid == 0) {
        pout[0] = pin[0];                                   // node 0
        pout[(1 << L.logC) << L.logT] = pin[(1 << L.logC) << L.logT];   // node n-1
    }
    // one block reduction for the three norms (also orders this pass's writes before the next phase)
    a1 = wave_total(a1); a2 = wave_total(a2); a3 = wave_total(a3);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) { red[threadIdx.x >> 6] = a1; red[4 + (threadIdx.x >> 6)] = a2; red[8 + (threadIdx.x >> 6)] = a3; }
    __syncthreads();
    const double s1 = (red[0] + red[1]) + (red[2] + red[3]);
    const double s2 = (red[4] + red[5]) + (red[6] + red[7]);
    const double s3 = (red[8] + red[9]) + (red[10] + red[11]);
    if (!COOP || A.G == 1) { e1 = sqrt(s1); e2 = sqrt(s2); e3 = sqrt(s3); return; }
    group_norms3(A, s1, s2, s3, e1, e2, e3);
}

// Copy C rows of 256 lanes between global memory and LDS (row strides in doubles).  The loads of up to 8 rows are issued
// together: a row-by-row loop pays one memory round trip per row.
template <typename Dst, typename Src>
__device__ __forceinline__ void copy_rows(Dst* dst, int dstride, const Src* src, int sstride, int C)
{
    const int tid = threadIdx.x;
    int k = 0;
    for (; k + 8 <= C; k += 8) {
        double v[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) v[q] = src[(k + q) * sstride + tid];
#pragma unroll
        for (int q = 0; q < 8; ++q) dst[(k + q) * dstride + tid] = v[q];
    }
    for (; k < C; ++k) dst[k * dstride + tid] = src[k * sstride + tid];
}

// Two arrays at once, 16 rows of each in flight: the copy into the staging memory is a chain of round trips to L2 / the
// Infinity Cache (the level was last written by this or by another compute unit), not a bandwidth problem -- 32 loads per
// lane and trip instead of 8 cut a 32-row copy from eight trips to two.
template <typename DA, typename SA>
__device__ __forceinline__ void copy_rows2(DA* dstA, DA* dstB, int dstride, const SA* srcA, const SA* srcB, int sstride, int C)
{
    const int tid = threadIdx.x;
    int k = 0;
    for (; k + 16 <= C; k += 16) {
        double a[16], b[16];
#pragma unroll
        for (int q = 0; q < 16; ++q) { a[q] = srcA[(k + q) * sstride + tid]; b[q] = srcB[(k + q) * sstride + tid]; }
#pragma unroll
        for (int q = 0; q < 16; ++q) { dstA[(k + q) * dstride + tid] = a[q]; dstB[(k + q) * dstride + tid] = b[q]; }
    }
    for (; k + 4 <= C; k += 4) {
        double a[4], b[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) { a[q] = srcA[(k + q) * sstride + tid]; b[q] = srcB[(k + q) * sstride + tid]; }
#pragma unroll
        for (int q = 0; q < 4; ++q) { dstA[(k + q) * dstride + tid] = a[q]; dstB[(k + q) * dstride + tid] = b[q]; }
    }
    for (; k < C; ++k) { dstA[k * dstride + tid] = srcA[k * sstride + tid]; dstB[k * dstride + tid] = srcB[k * sstride + tid]; }
}

// PoissonSolver::IterateGaussSeidel (PoissonSolver.cpp:66-77)
// GF = false: the caller has no global-memory level with a long chunk (the resident kernel's coarse workgroup: levels of <= 8193 nodes,
// all staged) -- the fused global pass is not even compiled in (its registers would count against that kernel's budget)
template <bool GF = true>
__device__ __forceinline__ double iterate_gs(const MgDesc& D, Atom& A, int l, double errorMin, int iterno, double* red, long* nsweeps)
{
    const int held = A.lds_holds;             // what the staging memory holds from the last staged visit (anything else below gives it up)
    A.lds_holds = -1;
    // the fused pass (a third of the sweeps' memory traffic) wherever a lane owns at least 2^fuse_min_logc nodes
    if (GF && iterno == 3 && !D.lv[l].seq && D.lv[l].logC >= D.fuse_min_logc && (l >= D.kcoop || (D.lv[l].stage == 0 && D.fuse_coop))) {
        double e1, e2, e3;
        if (l < D.kcoop) gs_fused3<true>(D, A, l, red, e1, e2, e3);
        else gs_fused3<false>(D, A, l, red, e1, e2, e3);
        if (!(e1 < errorMin) && !(e2 < errorMin)) {          // the reference runs all three sweeps
            A.cur ^= (1u << l);
            *nsweeps += 3;
            return e3;
        }
        __syncthreads();                                      // rare: it stops early -- redo from the untouched input copy
    }
    if (D.lv[l].seq) {
        // LDS-resident level: the sweeps of the visit by one thread, no workgroup barrier between them; the others wait
        // for the result (the error norm of one thread's partial sums equals the workgroup sum: the others add zeros)
        const Lvl L = D.lv[l];
        if (threadIdx.x == 0) {
            const double dh = L.d * 0.5;
            unsigned cur = A.cur;
            double err = 1E10;
            int done = 0;
            for (int i = 0; i < iterno; ++i) {
                const unsigned c = (cur >> l) & 1u;
                const double err2 = seq_sweep(A.lds + 2 * kSeqCap + L.soff, A.lds + c * kSeqCap + L.soff,
                                              A.lds + (c ^ 1u) * kSeqCap + L.soff, L.n, dh);
                cur ^= (1u << l);
                err = sqrt(err2);
                ++done;
                if (err < errorMin) break;
            }
            red[16] = err;
            red[17] = done;
        }
        __syncthreads();
        const double err = red[16];
        const int done = static_cast<int>(red[17]);
        if (done & 1) A.cur ^= (1u << l);
        *nsweeps += done;
        __syncthreads();
        return err;
    }
    if (D.lv[l].stage == 3) {
        // A small level of one workgroup (129 ... 1025 nodes): staged like the others but laid out over 64 lanes and swept
        // by the first wave alone -- a quarter of the LDS traffic per warm-up step, no workgroup barrier between the
        // sweeps.  All four waves copy in and out.
        const Lvl L = D.lv[l];
        const double dh = L.d * 0.5;
        const int tid = threadIdx.x;
        const unsigned c0 = (A.cur >> l) & 1u;
        double* G0 = (c0 ? A.phi1 : A.phi0) + L.off;
        double* G1 = (c0 ? A.phi0 : A.phi1) + L.off;
        const double* Sg = A.src + L.off;
        double* PP = A.stage + kStagePad;
        double* SS = PP + kStageArr;
        const int lc = L.logC + L.logT - 6;                   // log2(nodes per lane) with 64 lanes
        const int nm1 = L.n - 1;
        const int Cg1 = (1 << L.logC) - 1;
        // LDS index j = k*64 + t <-> node i = t*2^lc + k <-> global storage index (i & (C-1))*T + (i >> logC)
        auto gidx = [&](int j) { const int i = ((j & 63) << lc) + (j >> 6); return ((i & Cg1) << L.logT) + (i >> L.logC); };
        for (int j0 = 0; j0 < nm1; j0 += 4 * kThreads) {       // (129 ... 1 025 nodes: one pass; 2 049: two)
            double a[4], b[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int j = j0 + tid + q * kThreads;
                if (j < nm1) { const int gi = gidx(j); a[q] = G0[gi]; b[q] = Sg[gi]; }
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int j = j0 + tid + q * kThreads;
                if (j < nm1) { PP[j] = a[q]; SS[j] = b[q]; }
            }
        }
        if (tid == 0) PP[nm1] = G0[nm1];
        __syncthreads();
        if (tid < 64) {
            const int lo_g = tid << lc;
            double err = 1E10;
            int done = 0;
            for (int i = 0; i < iterno; ++i) {
                double err2;
                switch (lc) {
                    case 1:  err2 = gs_lds<1, 64, 64>(SS, PP, tid, lo_g, dh); break;
                    case 2:  err2 = gs_lds<2, 64, 64>(SS, PP, tid, lo_g, dh); break;
                    case 3:  err2 = gs_lds<3, 64, 64>(SS, PP, tid, lo_g, dh); break;
                    default: err2 = gs_lds<4, 64, 64>(SS, PP, tid, lo_g, dh); break;
                }
                err2 = wave_total(err2);
                err = sqrt(err2);
                ++done;
                if (err < errorMin) break;
                __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
                __builtin_amdgcn_wave_barrier();
            }
            if (tid == 0) { red[16] = err; red[17] = done; }
        }
        __syncthreads();
        const double err = red[16];
        const int done = static_cast<int>(red[17]);
        *nsweeps += done;
        double* Gout = (done & 1) ? G1 : G0;
        for (int j = tid; j < nm1; j += kThreads) Gout[gidx(j)] = PP[j];
        if (tid == 0) Gout[nm1] = PP[nm1];
        if (done & 1) A.cur ^= (1u << l);
        __syncthreads();
        return err;
    }
    if (D.lv[l].stage == 1) {
        // A level of one workgroup with <= 8193 nodes: the current copy and the source are copied to LDS once per visit
        // (same interleaved layout), the sweeps of the visit run there in place, the result goes back once.  A smoother
        // step then costs LDS issue slots instead of the 12 vector-memory instructions that bound it in HBM/L2.
        const Lvl L = D.lv[l];
        const double dh = L.d * 0.5;
        const int tid = threadIdx.x;
        const unsigned c0 = (A.cur >> l) & 1u;
        double* G0 = (c0 ? A.phi1 : A.phi0) + L.off;
        double* G1 = (c0 ? A.phi0 : A.phi1) + L.off;
        const double* Sg = A.src + L.off;
        double* PP = A.stage + kStagePad;
        double* SS = PP + kStageArr;
        const int C1 = 1 << L.logC;
        const bool fold = (A.pend == l + 1);                  // prolongation from level l+1 taken in while staging (do_prolong)
        const bool fold_r = (l > 0 && A.pend_r == l);         // restriction from level l-1 computed while staging (do_restrict)
        const bool fold_z = (l > 0 && A.pend_z == l);                  // resident group: the members have written the source, Phi = 0
        // round 6: the restriction folded into the copy-in reads level l-1 where its visit has just left it -- in this very staging
        // memory (same rows and columns) -- instead of from its global copy one round trip away; coarse row k is written after fine
        // rows 2k, 2k+1 have been read (k <= 2k), the only other column read is the left neighbour's LAST fine row, which no coarse
        // row reaches.  A second staging of the same visit (the early-stop path below) finds the memory overwritten: global then.
        bool r_lds = fold_r && held == l - 1 && D.fold_lds;
        A.pend = 0;
        A.pend_r = 0;
        A.pend_z = 0;
        auto stage_in = [&]() { PROF_T0();
        // (Every branch below is a chain of round trips to L2 / the Infinity Cache, not a bandwidth problem: the loads of as many rows as
        // the registers hold -- 16, or 32 where a row is one load -- are issued together, then the arithmetic and the LDS stores follow.
        // Round 6: batches of 4 / 8 rows became 16 / 32: the coarse workgroup's levels 4 - 6 spent 1.9 of their 7.4 ms per solve here.)
        if (fold_z) {
            int k0 = 0;
            for (; k0 + 32 <= C1; k0 += 32) {
                double b[32];
#pragma unroll
                for (int q = 0; q < 32; ++q) b[q] = Sg[(k0 + q) * kThreads + tid];
#pragma unroll
                for (int q = 0; q < 32; ++q) { SS[(k0 + q) * kThreads + tid] = b[q]; PP[(k0 + q) * kThreads + tid] = 0; }
            }
            for (; k0 < C1; k0 += 8) {
                double b[8];
#pragma unroll
                for (int q = 0; q < 8; ++q) b[q] = Sg[(k0 + q) * kThreads + tid];
#pragma unroll
                for (int q = 0; q < 8; ++q) { SS[(k0 + q) * kThreads + tid] = b[q]; PP[(k0 + q) * kThreads + tid] = 0; }
            }
            if (tid == 0) PP[L.n - 1] = 0;
        } else if (fold_r) {
            // PoissonSolver::Restrict (PoissonSolver.cpp:126-157) from level l-1 (same workgroup, same lane columns: coarse node
            // (t, k) sits under the fine nodes (t, 2k-1 .. 2k+1)) straight into the staging memory: Phi starts from 0, the
            // source also goes to the level's global array for the visit on the way back up.  Arithmetic of restrict_to.
            const Lvl Lf = D.lv[l - 1];
            const int logT = L.logT, Cf = 1 << Lf.logC;
            const double* pf = r_lds ? PP : (((A.cur >> (l - 1)) & 1u) ? A.phi1 : A.phi0) + Lf.off;      // (logT == 8: a row is kThreads doubles in both)
            const double* sf = r_lds ? SS : A.src + Lf.off;
            r_lds = false;
            double* __restrict__ sc = A.src + L.off;
            const double dc = L.d;
            double pm = pf[((Cf - 1) << logT) + (tid > 0 ? tid - 1 : 0)];
            auto rows = [&](auto NB, const int k0) {
                constexpr int nb = decltype(NB)::value;
                double p0[nb], pp[nb], s0[nb];
#pragma unroll
                for (int q = 0; q < nb; ++q) {
                    const int k = k0 + q;
                    p0[q] = pf[((2 * k) << logT) + tid];
                    pp[q] = pf[((2 * k + 1) << logT) + tid];
                    s0[q] = sf[((2 * k) << logT) + tid];
                }
#pragma unroll
                for (int q = 0; q < nb; ++q) {
                    const int k = k0 + q;
                    double sv = 4. * (s0[q] + pm - 2. * p0[q] + pp[q]) - dc * (pp[q] - pm);
                    if (k == 0 && tid == 0) sv = 0;                // coarse node 0
                    sc[(k << logT) + tid] = sv;
                    SS[k * kThreads + tid] = sv;
                    PP[k * kThreads + tid] = 0;
                    pm = pp[q];
                }
            };
            int k = 0;
            for (; k + 16 <= C1; k += 16) rows(std::integral_constant<int, 16>{}, k);
            for (; k + 4 <= C1; k += 4) rows(std::integral_constant<int, 4>{}, k);
            for (; k < C1; ++k) rows(std::integral_constant<int, 1>{}, k);
            if (tid == 0) { sc[C1 << logT] = 0; PP[L.n - 1] = 0; }  // coarse node n-1
        } else if (fold) {
            // PoissonSolver::Prolong (PoissonSolver.cpp:110-123) from level l+1 added to what is staged (arithmetic of
            // prolong_from: fine(2j) += coarse(j), fine(2j-1) += 0.5 (coarse(j-1) + coarse(j))); the level's global copy is
            // brought up to date by the write-out at the end of the visit
            const Lvl Lc = D.lv[l + 1];
            const double* __restrict__ Pc = A.cur_phi(l + 1, Lc);
            auto corr = [&](int i, bool odd) -> double {
                if (!odd) return Pc[addr(Lc, i >> 1)];
                return 0.5 * (Pc[addr(Lc, (i - 1) >> 1)] + Pc[addr(Lc, (i + 1) >> 1)]);
            };
            auto rows = [&](auto NB, const int k0) {
                constexpr int nb = decltype(NB)::value;
                double a[nb], b[nb], cadd[nb];
#pragma unroll
                for (int q = 0; q < nb; ++q) {
                    const int k = k0 + q;
                    a[q] = G0[k * kThreads + tid];
                    b[q] = Sg[k * kThreads + tid];
                    cadd[q] = corr((tid << L.logC) + k, (q & 1) != 0);
                }
#pragma unroll
                for (int q = 0; q < nb; ++q) {
                    PP[(k0 + q) * kThreads + tid] = a[q] + cadd[q];
                    SS[(k0 + q) * kThreads + tid] = b[q];
                }
            };
            int k0 = 0;                                              // C1 >= 8 on these levels (a multiple of 4)
            for (; k0 + 16 <= C1; k0 += 16) rows(std::integral_constant<int, 16>{}, k0);
            for (; k0 + 8 <= C1; k0 += 8) rows(std::integral_constant<int, 8>{}, k0);       // (the 2 049-node level: one trip, not two)
            for (; k0 < C1; k0 += 4) rows(std::integral_constant<int, 4>{}, k0);
            if (tid == 0) PP[L.n - 1] = G0[L.n - 1] + corr(L.n - 1, false);
        } else {
            copy_rows2(PP, SS, kThreads, G0, Sg, kThreads, C1);
            if (tid == 0) PP[L.n - 1] = G0[L.n - 1];
        }
        __syncthreads();
        PROF_ADD(5, l); };
        stage_in();
        const int lo_g = tid << L.logC;
        double err = 1E10;
        int done = 0;
        PROF_T0();
        bool fused_done = false;
        if (D.fuse3 && iterno == 3 && L.logC >= 2) {
            // the whole visit as one fused pass (gs_lds3); if the reference would have stopped after the first or the second sweep
            // (rare: err < errorMin), the level is staged again and the visit runs sweep by sweep below
            double f1, f2, f3;
            const bool lastl = tid == kThreads - 1;
            const double xN = PP[L.n - 1];
            const bool careful = (__builtin_amdgcn_readfirstlane(lo_g) <= kWarm3);
#define DFTA_GS3(LC) do { if (careful) gs_lds3<LC, kThreads, kThreads, 3, true>(SS, PP, tid, lo_g, lastl, xN, dh, f1, f2, f3); \
                          else gs_lds3<LC, kThreads, kThreads, 3, false>(SS, PP, tid, lo_g, lastl, xN, dh, f1, f2, f3); } while (0)
            switch (L.logC) {
                case 2:  DFTA_GS3(2); break;
                case 3:  DFTA_GS3(3); break;
                case 4:  DFTA_GS3(4); break;
                default: DFTA_GS3(5); break;
            }
#undef DFTA_GS3
            f1 = wave_total(f1); f2 = wave_total(f2); f3 = wave_total(f3);
            __syncthreads();
            if ((tid & 63) == 0) { red[tid >> 6] = f1; red[4 + (tid >> 6)] = f2; red[8 + (tid >> 6)] = f3; }
            __syncthreads();
            const double e1 = sqrt((red[0] + red[1]) + (red[2] + red[3]));
            const double e2 = sqrt((red[4] + red[5]) + (red[6] + red[7]));
            const double e3 = sqrt((red[8] + red[9]) + (red[10] + red[11]));
            if (!(e1 < errorMin) && !(e2 < errorMin)) {
                err = e3;
                done = 3;
                *nsweeps += 3;
                fused_done = true;
            } else {
                __syncthreads();
                stage_in();
            }
        }
        if (!fused_done)
        for (int i = 0; i < iterno; ++i) {
            double err2;
            switch (L.logC) {
                case 0:  err2 = gs_lds<0, kThreads>(SS, PP, tid, lo_g, dh); break;
                case 1:  err2 = gs_lds<1, kThreads>(SS, PP, tid, lo_g, dh); break;
                case 2:  err2 = gs_lds<2, kThreads>(SS, PP, tid, lo_g, dh); break;
                case 3:  err2 = gs_lds<3, kThreads>(SS, PP, tid, lo_g, dh); break;
                case 4:  err2 = gs_lds<4, kThreads>(SS, PP, tid, lo_g, dh); break;
                default: err2 = gs_lds<5, kThreads>(SS, PP, tid, lo_g, dh); break;
            }
            err = sqrt(block_sum(err2, red));
            ++done;
            ++*nsweeps;
            if (err < errorMin) break;
        }
        PROF_ADD(7, l);
        // after `done` sweeps the current copy is G1 for odd counts, G0 for even ones
        double* Gout = (done & 1) ? G1 : G0;
        { PROF_T0();
        copy_rows(Gout, kThreads, PP, kThreads, C1);
        if (tid == 0) Gout[L.n - 1] = PP[L.n - 1];
        if (done & 1) A.cur ^= (1u << l);
        __syncthreads();
        PROF_ADD(6, l); }
        A.lds_holds = l;
        return err;
    }
    if (D.lv[l].stage == 2) {
        // A level shared by the G workgroups of the atom (lane ids run over the group: member g owns the columns
        // g*256 .. g*256+255 of every row): each member stages its columns plus kStageH halo columns in front of them (the
        // previous member's last lanes: the warm-up reads up to 96 nodes = 96/C lanes back) and Phi of the first node of
        // the next member.  After every sweep the members exchange the new values of those boundary nodes through the
        // level's other global copy (exactly where the unstaged sweep would have put them) around the group barrier that
        // the error norm needs anyway; the last sweep of the visit writes the whole part out instead.
        const Lvl L = D.lv[l];
        const double dh = L.d * 0.5;
        const int tid = threadIdx.x;
        const int C = 1 << L.logC, logT = L.logT, g = A.g;
        const int Hc = kWarm >> L.logC;                       // lanes in the halo that the warm-up touches
        const unsigned c0 = (A.cur >> l) & 1u;
        double* Gin = (c0 ? A.phi1 : A.phi0) + L.off;
        double* Gout = (c0 ? A.phi0 : A.phi1) + L.off;
        const double* Sg = A.src + L.off;
        double* PP = A.stage + kStageH;
        double* SS = PP + kStageArr;
        const int col0 = g * kThreads;
        const int end_g = (g == A.G - 1) ? (C << logT) : (col0 + kThreads);     // node behind this member's part
        const bool fold = (A.pend == l + 1);
        const bool fold_r = (l > 0 && A.pend_r == l);
        A.pend = 0;
        A.pend_r = 0;
        // the fused visit (below) takes everything it needs of the neighbours from the level's global copy, which is complete and
        // visible since the last barrier: 112 + 3 nodes in front of the part (halo columns), three behind it
        const bool want3 = D.fuse3 && D.fuse_coop && iterno == 3 && L.logC >= 3;       // 115 nodes <= kStageH lanes
        auto stage_in2 = [&]() {
        PROF_T0();
        if (fold_r) {
            // PoissonSolver::Restrict (PoissonSolver.cpp:126-157) from level l-1 folded into the copy: the source of every
            // staged node -- own columns and halo columns -- comes straight from the fine level (complete and visible since
            // its last barrier), Phi starts from 0.  The own columns of the source also go to the level's global array, where
            // the later visits of this V-cycle and the next restriction read them (after this visit's barriers).
            const Lvl Lf = D.lv[l - 1];
            const double* __restrict__ Pf = (((A.cur >> (l - 1)) & 1u) ? A.phi1 : A.phi0) + Lf.off;
            const double* __restrict__ Sf = A.src + Lf.off;
            double* __restrict__ Sgw = A.src + L.off;
            const int lim = L.n - 1;
            const double dc = L.d;
            auto src_of_node = [&](int i) -> double {
                if (i <= 0 || i >= lim) return 0.0;
                const int twoi = 2 * i;
                const double pm = Pf[addr(Lf, twoi - 1)], p0 = Pf[addr(Lf, twoi)], pp = Pf[addr(Lf, twoi + 1)];
                return 4. * (Sf[addr(Lf, twoi)] + pm - 2. * p0 + pp) - dc * (pp - pm);
            };
            const int lane0 = col0 + tid;
            for (int k0 = 0; k0 < C; k0 += 4) {
                double b[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) b[q] = src_of_node((lane0 << L.logC) + k0 + q);
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    PP[(k0 + q) * kStageRS + tid] = 0;
                    SS[(k0 + q) * kStageRS + tid] = b[q];
                    Sgw[((k0 + q) << logT) + lane0] = b[q];
                }
            }
            for (int idx = tid; idx < C * kStageH; idx += kThreads) {
                const int k = idx / kStageH, c = idx % kStageH - kStageH;
                const int lanec = col0 + c;
                PP[k * kStageRS + c] = 0;
                SS[k * kStageRS + c] = lanec >= 0 ? src_of_node((lanec << L.logC) + k) : 0.0;
            }
            if (tid == 0) {
                PP[C * kStageRS] = 0;
                if (g == A.G - 1) Sgw[C << logT] = 0;          // source of node n-1
            }
            if (want3 && tid < 2 && g < A.G - 1) {              // the fused pass also wants the next two nodes behind the part
                const int i_end = (col0 + kThreads) << L.logC;
                PP[C * kStageRS + 1 + tid] = 0;
                SS[C * kStageRS + tid] = src_of_node(i_end + tid);
            }
        } else if (!fold) {
            copy_rows2(PP, SS, kStageRS, Gin + col0, Sg + col0, 1 << logT, C);
            for (int idx = tid; idx < C * kStageH; idx += kThreads) {       // halo columns (member 0: in-bounds padding / the
                const int k = idx / kStageH, c = idx % kStageH - kStageH;   // previous level's tail, never used)
                PP[k * kStageRS + c] = Gin[(k << logT) + col0 + c];
                SS[k * kStageRS + c] = Sg[(k << logT) + col0 + c];
            }
            if (tid == 0) PP[C * kStageRS] = Gin[end_g];
            if (want3 && tid < 2 && g < A.G - 1) {              // nodes end + 1, end + 2 (rows 1, 2 of the next member's first lane)
                PP[C * kStageRS + 1 + tid] = Gin[((1 + tid) << logT) + col0 + kThreads];
                SS[C * kStageRS + tid] = Sg[(tid << logT) + col0 + kThreads];
            }
        } else {
            // PoissonSolver::Prolong (PoissonSolver.cpp:110-123) from level l+1 folded into the copy: every member adds the
            // correction to what it stages -- its own columns, the halo columns and the node behind its part -- from the
            // coarse level, which is complete and visible since that level's last barrier.  The separate pass over the fine
            // level and the group barrier after it are gone; the level's global copy is brought up to date by the write-out
            // at the end of this visit.
            const Lvl Lc = D.lv[l + 1];
            const double* __restrict__ Pc = (((A.cur >> (l + 1)) & 1u) ? A.phi1 : A.phi0) + Lc.off;
            auto corr = [&](int i, bool odd) -> double {               // fine node i (odd-ness known to the caller)
                if (!odd) return Pc[addr(Lc, i >> 1)];                  // fine(2j) += coarse(j)
                return 0.5 * (Pc[addr(Lc, (i - 1) >> 1)] + Pc[addr(Lc, (i + 1) >> 1)]);   // fine(2j-1) += 0.5 (coarse(j-1) + coarse(j))
            };
            const int lane0 = col0 + tid;
            for (int k0 = 0; k0 < C; k0 += 4) {                         // C >= 4, a multiple of 4
                double a[4], b[4], cadd[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int k = k0 + q, gi = (k << logT) + lane0;
                    a[q] = Gin[gi];
                    b[q] = Sg[gi];
                    cadd[q] = corr((lane0 << L.logC) + k, (q & 1) != 0);
                }
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    PP[(k0 + q) * kStageRS + tid] = a[q] + cadd[q];
                    SS[(k0 + q) * kStageRS + tid] = b[q];
                }
            }
            for (int idx = tid; idx < C * kStageH; idx += kThreads) {
                const int k = idx / kStageH, c = idx % kStageH - kStageH;
                const int lanec = col0 + c, gi = (k << logT) + lanec;
                double v = Gin[gi];
                if (lanec >= 0) v += corr((lanec << L.logC) + k, (k & 1) != 0);
                PP[k * kStageRS + c] = v;
                SS[k * kStageRS + c] = Sg[gi];
            }
            if (tid == 0) {
                const int i_end = (g == A.G - 1) ? (L.n - 1) : ((col0 + kThreads) << L.logC);
                PP[C * kStageRS] = Gin[end_g] + corr(i_end, false);    // even node in both cases
            }
            if (want3 && tid < 2 && g < A.G - 1) {
                const int i_end = (col0 + kThreads) << L.logC, k = 1 + tid;
                PP[C * kStageRS + k] = Gin[(k << logT) + col0 + kThreads] + corr(i_end + k, (k & 1) != 0);
                SS[C * kStageRS + tid] = Sg[(tid << logT) + col0 + kThreads];
            }
        }
        __syncthreads();
        PROF_ADD(5, l); };
        stage_in2();
        auto write_out = [&]() {
            copy_rows(Gout + col0, 1 << logT, PP, kStageRS, C);
            if (g == A.G - 1 && tid == 0) Gout[C << logT] = PP[C * kStageRS];
        };
        const int lo_g = (col0 + tid) << L.logC;
        double err = 1E10;
        int done = 0;
        if (want3) {
            // ONE fused pass (gs_lds3) on the staged part, the write-out and ONE group barrier carrying the three norms, instead of three
            // sweeps with an exchange of boundary nodes and a barrier each.  If the reference would have stopped after the first or the
            // second sweep (rare), the part is staged again -- the input copy is untouched -- and the visit runs sweep by sweep below.
            double f1, f2, f3;
            const bool lastl = (g == A.G - 1) && tid == kThreads - 1;
            const double xN = PP[C * kStageRS];
            const bool careful = (__builtin_amdgcn_readfirstlane(lo_g) <= kWarm3);
            const double* rP = PP + C * kStageRS;
            const double* rS = SS + C * kStageRS;
            { PROF_T0();
#define DFTA_GS3S(LC) do { if (careful) gs_lds3<LC, kStageRS, kThreads, 3, true, true>(SS, PP, tid, lo_g, lastl, xN, dh, f1, f2, f3, rP, rS); \
                           else gs_lds3<LC, kStageRS, kThreads, 3, false, true>(SS, PP, tid, lo_g, lastl, xN, dh, f1, f2, f3, rP, rS); } while (0)
            switch (L.logC) {
                case 3:  DFTA_GS3S(3); break;
                case 4:  DFTA_GS3S(4); break;
                default: DFTA_GS3S(5); break;
            }
#undef DFTA_GS3S
            PROF_ADD(4, l); }
            f1 = wave_total(f1); f2 = wave_total(f2); f3 = wave_total(f3);
            __syncthreads();
            if ((tid & 63) == 0) { red[tid >> 6] = f1; red[4 + (tid >> 6)] = f2; red[8 + (tid >> 6)] = f3; }
            { PROF_T0(); write_out(); PROF_ADD(6, l); }
            __syncthreads();
            double e1, e2, e3;
            { PROF_T0();
            group_norms3(A, (red[0] + red[1]) + (red[2] + red[3]), (red[4] + red[5]) + (red[6] + red[7]), (red[8] + red[9]) + (red[10] + red[11]), e1, e2, e3);
            PROF_ADD(3, l); }
            if (!(e1 < errorMin) && !(e2 < errorMin)) {
                *nsweeps += 3;
                A.cur ^= (1u << l);
                return e3;
            }
            stage_in2();
        }
        for (int i = 0; i < iterno; ++i) {
            double err2;
            { PROF_T0();
            switch (L.logC) {
                case 2:  err2 = gs_lds<2, kStageRS>(SS, PP, tid, lo_g, dh); break;
                case 3:  err2 = gs_lds<3, kStageRS>(SS, PP, tid, lo_g, dh); break;
                case 4:  err2 = gs_lds<4, kStageRS>(SS, PP, tid, lo_g, dh); break;
                default: err2 = gs_lds<5, kStageRS>(SS, PP, tid, lo_g, dh); break;
            }
            PROF_ADD(4, l); }
            ++done;
            ++*nsweeps;
            const bool last = (i == iterno - 1);
            __syncthreads();
            if (last) { PROF_T0(); write_out(); PROF_ADD(6, l); }
            else {
                // into the sentinel-filled slots of the exchange that travels with the fast sum (group_sum_fast)
                if (tid < (Hc << L.logC)) {                    // the last Hc lanes' nodes: what the next member's warm-up reads
                    const int k = tid & (C - 1), c = kThreads - Hc + (tid >> L.logC);
                    exchange_store(A, tid, PP[k * kStageRS + c]);
                }
                if (tid == 0) exchange_store(A, kXchg - 1, PP[0]);   // the first node: right neighbour of the previous member's last one
            }
            { PROF_T0(); err = sqrt(last ? group_sum_fast<kStageRS, true>(A, err2, red, PP, L.logC, Hc) : group_sum_fast<kStageRS>(A, err2, red, PP, L.logC, Hc)); PROF_ADD(3, l); }
            if (last) break;
            if (err < errorMin) {                              // the reference stops here: publish everything, meet once more
                write_out();
                group_sync(A);
                break;
            }
            // (the neighbours' nodes arrived with the sum: halo columns and PP[C * kStageRS] are up to date)
            { double* t = Gin; Gin = Gout; Gout = t; }
        }
        if (done & 1) A.cur ^= (1u << l);
        return err;
    }
    double err = 1E10;
    for (int i = 0; i < iterno; ++i) {
        err = gauss_seidel(D, A, l, red);
        ++*nsweeps;
        if (err < errorMin) break;
    }
    return err;
}

// PoissonSolver::Restrict(lvl) (PoissonSolver.cpp:126-157): fine = lvl-1 -> coarse = lvl
__device__ __forceinline__ void restrict_to(const MgDesc& D, Atom& A, int lvl)
{
    const Lvl Lc = D.lv[lvl], Lf = D.lv[lvl - 1];
    const double* Pf = A.cur_phi(lvl - 1, Lf);
    double* Pc = A.cur_phi(lvl, Lc);
    const double* Sf = A.src_of(Lf);
    double* Sc = A.src_of(Lc);
    const int lim = Lc.n - 1;
    const bool coop = lvl < D.kcoop;       // both levels are shared by the group
    if (!Lc.seq && !Lf.seq && Lc.logT == Lf.logT && Lc.logC >= 1) {
        // both levels chunked over the same lanes: coarse node (t, k) sits under fine nodes (t, 2k-1 .. 2k+1), so lane t
        // streams its own column -- all rows are wave-uniform, every access is coalesced, 4 rows per batch in flight
        const int T = 1 << Lc.logT, Cc = 1 << Lc.logC, Cf = 1 << Lf.logC, logT = Lc.logT;
        const int t = coop ? A.lane() : static_cast<int>(threadIdx.x);
        const double* __restrict__ pf = (((A.cur >> (lvl - 1)) & 1u) ? A.phi1 : A.phi0) + Lf.off;
        const double* __restrict__ sf = A.src + Lf.off;
        double* __restrict__ pc = (((A.cur >> lvl) & 1u) ? A.phi1 : A.phi0) + Lc.off;
        double* __restrict__ sc = A.src + Lc.off;
        const double dc = Lc.d;
        if (t < T) {
            // row -1 of lane t is the last row of lane t-1 (node t*Cf - 1); lane 0 never uses it (coarse node 0 is fixed)
            double pm = pf[((Cf - 1) << logT) + (t > 0 ? t - 1 : 0)];
#pragma unroll 4
            for (int k = 0; k < Cc; ++k) {
                const double p0 = pf[((2 * k) << logT) + t];
                const double pp = pf[((2 * k + 1) << logT) + t];
                const double s0 = sf[((2 * k) << logT) + t];
                double s = 4. * (s0 + pm - 2. * p0 + pp) - dc * (pp - pm);
                if (k == 0 && t == 0) s = 0;                       // coarse node 0
                sc[(k << logT) + t] = s;
                pc[(k << logT) + t] = 0;
                pm = pp;
            }
        }
        if (t == 0) { sc[Cc << logT] = 0; pc[Cc << logT] = 0; }    // coarse node n-1
        if (coop) group_sync(A); else __syncthreads();
        return;
    }
    // the fine level is shared but the coarse one is workgroup 0's (lvl == kcoop): the members compute it together all the
    // same (their copy of the coarse level's `cur` bit dates from the last prolongation out of it and is still valid)
    const bool share = coop || (lvl - 1 < D.kcoop && A.G > 1);
    for (int idx = share ? A.lane() : static_cast<int>(threadIdx.x); idx < Lc.n; idx += share ? kThreads * A.G : kThreads) {
        const int i = node_of(Lc, idx);
        Pc[idx] = 0;
        double s = 0;
        if (i > 0 && i < lim) {
            const int twoi = 2 * i;
            const double pm = Pf[addr(Lf, twoi - 1)], p0 = Pf[addr(Lf, twoi)], pp = Pf[addr(Lf, twoi + 1)];
            s = 4. * (Sf[addr(Lf, twoi)] + pm - 2. * p0 + pp) - Lc.d * (pp - pm);
        }
        Sc[idx] = s;
    }
    if (share) group_sync(A); else __syncthreads();
}

// PoissonSolver::Prolong (PoissonSolver.cpp:110-123): coarse = lvl -> fine = lvl-1 (additive)
__device__ __forceinline__ void prolong_from(const MgDesc& D, Atom& A, int lvl)
{
    const Lvl Lc = D.lv[lvl], Lf = D.lv[lvl - 1];
    const double* Pc = A.cur_phi(lvl, Lc);
    double* Pf = A.cur_phi(lvl - 1, Lf);
    const bool coop = lvl - 1 < D.kcoop;   // the fine level is shared by the group (the coarse one may be workgroup 0's)
    if (!Lc.seq && !Lf.seq && Lc.logT == Lf.logT && Lc.logC >= 1) {
        // same lane-column structure as in restrict_to: fine (t, 2k) += coarse (t, k); fine (t, 2k-1) += 0.5 (coarse (t, k-1) + coarse (t, k))
        const int T = 1 << Lc.logT, Cc = 1 << Lc.logC, Cf = 1 << Lf.logC, logT = Lc.logT;
        const int t = coop ? A.lane() : static_cast<int>(threadIdx.x);
        const double* __restrict__ pc = (((A.cur >> lvl) & 1u) ? A.phi1 : A.phi0) + Lc.off;
        double* __restrict__ pf = (((A.cur >> (lvl - 1)) & 1u) ? A.phi1 : A.phi0) + Lf.off;
        if (t < T) {
            // coarse value left of this lane's first node: last row of lane t-1 (unused by lane 0: fine node -1 does not exist)
            double cm = pc[((Cc - 1) << logT) + (t > 0 ? t - 1 : 0)];
#pragma unroll 4
            for (int k = 0; k < Cc; ++k) {
                const double c = pc[(k << logT) + t];
                pf[((2 * k) << logT) + t] += c;
                if (k > 0) pf[((2 * k - 1) << logT) + t] += 0.5 * (cm + c);
                else if (t > 0) pf[((Cf - 1) << logT) + t - 1] += 0.5 * (cm + c);      // fine node t*Cf - 1 lives in lane t-1's column
                cm = c;
            }
            if (t == T - 1) {                                                            // coarse node n-1 and the fine node below it
                const double cN = pc[Cc << logT];
                pf[Cf << logT] += cN;
                pf[((Cf - 1) << logT) + t] += 0.5 * (cm + cN);
            }
        }
        if (coop) group_sync(A); else __syncthreads();
        return;
    }
    for (int idx = coop ? A.lane() : static_cast<int>(threadIdx.x); idx < Lc.n; idx += coop ? kThreads * A.G : kThreads) {
        const int i = node_of(Lc, idx);
        const double c = Pc[idx];
        Pf[addr(Lf, 2 * i)] += c;
        if (i > 0) Pf[addr(Lf, 2 * i - 1)] += 0.5 * (Pc[addr(Lc, i - 1)] + c);
    }
    if (coop) group_sync(A); else __syncthreads();
}

struct Counters { long sweeps, vcycles; };

// PoissonSolver::Initialize without its final smoothing (PoissonSolver.cpp:80-103)
__device__ __forceinline__ void initialize(const MgDesc& D, Atom& A, double lowB, double highB)
{
    A.cur = 0;
    {
        const Lvl L0 = D.lv[0];
        double* P0 = A.cur_phi(0, L0);
        const bool coop = D.kcoop > 0;
        if (coop || A.g == 0)
            for (int idx = coop ? A.lane() : static_cast<int>(threadIdx.x); idx < L0.n; idx += coop ? kThreads * A.G : kThreads) P0[idx] = 0;
    }
    for (int l = 1; l < D.levels; ++l) {
        const Lvl L = D.lv[l], Lf = D.lv[l - 1];
        const bool coop = l < D.kcoop;
        // the source of level l-1 must be complete: it was written by the whole group for l <= kcoop
        if (A.G > 1 && l <= D.kcoop) group_sync(A); else __syncthreads();
        if (!coop && A.g != 0) continue;
        for (int idx = coop ? A.lane() : static_cast<int>(threadIdx.x); idx < L.n; idx += coop ? kThreads * A.G : kThreads) {
            const int p = node_of(L, idx);
            double s = 0;
            if (p > 0 && p < L.n - 1) s = 4 * A.src_of(Lf)[addr(Lf, 2 * p)];
            A.src_of(L)[idx] = s;
            A.cur_phi(l, L)[idx] = 0;
        }
    }
    __syncthreads();
    const int cl = D.levels - 1;
    if (threadIdx.x == 0 && A.g == 0) {
        double* Pc = A.cur_phi(cl, D.lv[cl]);
        Pc[addr(D.lv[cl], 0)] = lowB;
        Pc[addr(D.lv[cl], D.lv[cl].n - 1)] = highB;
    }
    __syncthreads();
}

// The whole cycle structure of PoissonSolver::FullCycle (PoissonSolver.h:89-124) as ONE loop over "legs", so that
// the smoother, restriction and prolongation are each inlined exactly once:
//   step 0                      : the 15 sweeps on the coarsest level that end Initialize (PoissonSolver.cpp:105)
//   steps 1 .. 2*nramp          : for i = levels-2 .. 1: Descend(last -> i), Ascend(i -> last)     (FMG ramp)
//   step 2*nramp+1              : Descend(last -> 0, errorMinLast)
//   then pairs                  : VCycle = Ascend(0 -> last), Descend(last -> 0); stop on err < errorMinLast or 100 cycles
// Ascend(from,to): { GS(from); Restrict(from+1); GS(from+1); ... ; GS(to) }      (PoissonSolver.cpp:162-171)
// Descend(from,to): { Prolong(from); GS(from-1); ... ; GS(to) }                  (PoissonSolver.cpp:173-186)
// The operations as the members of a group execute them: levels below kcoop by everybody, the others by workgroup 0
// alone (the other members skip them and meet workgroup 0 again at the barrier in front of the first shared operation).
// may_fold: the caller visits level lvl next (the V-cycle driver); a staged shared level then computes its source -- own
// columns and halo -- while it is copied to LDS (iterate_gs), and the pass and the group barrier below are skipped
__device__ __forceinline__ void do_restrict(const MgDesc& D, Atom& A, int lvl, bool may_fold = false)
{
    if (may_fold && lvl < D.kcoop && D.lv[lvl].stage == 2 && !D.nofold) { A.pend_r = lvl; return; }
    // both levels workgroup 0's, staged, on the same lane columns: folded into the copy-in likewise (iterate_gs, stage 1)
    if (may_fold && lvl - 1 >= D.kcoop && D.lv[lvl].stage == 1 && D.lv[lvl - 1].stage == 1 && D.lv[lvl].logT == D.lv[lvl - 1].logT &&
        D.lv[lvl].logC >= 2 && !D.nofold) {
        if (A.g == 0) A.pend_r = lvl;
        return;
    }
    if (lvl - 1 < D.kcoop || A.g == 0) restrict_to(D, A, lvl);
}

// may_fold: the caller visits level lvl-1 next (the V-cycle driver); a staged shared level then takes the correction in
// while it is copied to LDS (iterate_gs) and the pass below is skipped
__device__ __forceinline__ void do_prolong(const MgDesc& D, Atom& A, int lvl, bool may_fold = false)
{
    if (lvl - 1 < D.kcoop) {
        if (lvl >= D.kcoop && A.G > 1) {
            // the coarse level is workgroup 0's: wait for it, and learn which of its two copies is current
            unsigned* pub = reinterpret_cast<unsigned*>(A.part + 6 * A.G);
            if (A.g == 0 && threadIdx.x == 0) *pub = A.cur;
            group_sync(A);
            const unsigned shared = (1u << D.kcoop) - 1u;
            A.cur = (A.cur & shared) | (*pub & ~shared);
        }
        if (may_fold && D.lv[lvl - 1].stage == 2 && !D.nofold) { A.pend = lvl; return; }
        prolong_from(D, A, lvl);
    } else if (may_fold && D.lv[lvl - 1].stage == 1 && D.lv[lvl - 1].logC >= 2 && !D.lv[lvl].seq && !D.nofold) {
        if (A.g == 0) A.pend = lvl;                            // workgroup 0's own staged level: folded into its copy-in
    } else if (A.g == 0) prolong_from(D, A, lvl);
}

__device__ __forceinline__ double do_iterate(const MgDesc& D, Atom& A, int l, double errorMin, int iterno, double* red, long* nsweeps)
{
    if (l < D.kcoop || A.g == 0) return iterate_gs(D, A, l, errorMin, iterno, red, nsweeps);
    return 1E10;
}

// ---- coarse section -----------------------------------------------------------------------------------------------
// The levels with <= 1025 nodes cost a V-cycle more in waiting than in arithmetic: every visit pays a copy-in from global
// memory, workgroup barriers and a copy-out for ~1 us of sweeps.  From the first V-cycle on, the part of a cycle below
// level cs_top -- restrict .. iterate down to the coarsest level and prolong .. iterate back up -- therefore runs in the
// first wave of workgroup 0 alone, on copies that stay in LDS (the staging memory is idle meanwhile): no barrier, no
// global round trip until the wave hands level cs_top back.  Same operations in the same order on the same values as the
// level-by-level code (the error norms are summed in a different order, as everywhere).  Nothing on these levels
// carries over from one V-cycle to the next: the restriction rewrites the sources and zeroes Phi on the way down.
__device__ __forceinline__ void wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// index of node i inside the LDS copy of a level (n nodes, lc as in MgDesc::cs_lc)
__device__ __forceinline__ int cs_idx(int n, int lc, int i)
{
    if (lc < 0) return i;
    if (i == n - 1) return (1 << lc) << 6;          // behind the rows: n - 1 itself for 64 lanes x 2^lc nodes; 256 for the 129-node level on 32 lanes x 4
    return ((i & ((1 << lc) - 1)) << 6) + (i >> lc);
}

// One in-place sweep of a level in natural order by ONE thread (PoissonSolver.cpp:40-64); returns sum dPhi^2.  Explicit LDS
// pointers; the loads of a batch are issued together ahead of the recurrence (the right neighbours are read before the
// batch overwrites them).
__device__ __forceinline__ double seq_sweep_inplace(const double* __restrict__ Sg, double* __restrict__ Pg, const int n, const double dh)
{
    typedef __attribute__((address_space(3))) double lds_f64;
    typedef __attribute__((address_space(3))) const double lds_cf64;
    lds_cf64* S = (lds_cf64*)(Sg);
    lds_f64* P = (lds_f64*)(Pg);
    double err2 = 0;
    double y = 2.0 * P[0];
    const int limit = n - 1;
    double old = P[1];
    constexpr int kB = 8;
    int i = 1;
    for (; i + kB <= limit; i += kB) {
        double xp[kB], sv[kB], xo[kB];
#pragma unroll
        for (int q = 0; q < kB; ++q) { xp[q] = P[i + q + 1]; sv[q] = S[i + q]; }
#pragma unroll
        for (int q = 0; q < kB; ++q) {
            y = gs_point2(sv[q], y, xp[q], dh);
            const double x = 0.5 * y;
            const double dif = old - x;
            err2 += dif * dif;
            xo[q] = x;
            old = xp[q];
        }
#pragma unroll
        for (int q = 0; q < kB; ++q) P[i + q] = xo[q];
    }
    for (; i < limit; ++i) {
        const double xp = P[i + 1];
        y = gs_point2(S[i], y, xp, dh);
        const double x = 0.5 * y;
        const double dif = old - x;
        err2 += dif * dif;
        P[i] = x;
        old = xp;
    }
    return err2;
}

// The same sweep (n <= 65 nodes, natural order) by the 64 lanes of a wave: lane t keeps S, the old right neighbour and the
// old value of node t + 1 in registers and recomputes its node in every step from the candidate of lane t - 1, handed on
// through a DPP lane shift (lane 0: from the boundary value).  The candidate of node i is final from step i on -- its
// left neighbour's is final one step earlier and its other inputs never change -- so after n - 2 steps every lane holds
// exactly what the sequential loop computes: the same n - 2 dependent updates, but 7 instructions each (5 flops, 2 lane
// shifts) instead of a scalar loop with its LDS traffic (~46 ns per node).  Returns this lane's share of sum dPhi^2.
__device__ __forceinline__ double seq_sweep_wave(const double* __restrict__ Sg, double* __restrict__ Pg, const int n, const double dh)
{
    typedef __attribute__((address_space(3))) double lds_f64;
    typedef __attribute__((address_space(3))) const double lds_cf64;
    lds_cf64* S = (lds_cf64*)(Sg);
    lds_f64* P = (lds_f64*)(Pg);
    const int i = (threadIdx.x & 63) + 1;             // this lane's node
    const bool mine = i < n - 1;
    const double s = mine ? S[i] : 0.0;
    const double xp = mine ? P[i + 1] : 0.0;
    const double old = mine ? P[i] : 0.0;
    double yin = 2.0 * P[0];                          // stays the boundary value in lane 0
    double cand = 0;
    // (extra steps are harmless -- the candidates are at their fixed point -- so the trip count is rounded up to the unroll)
    for (int k = 0; k < n - 2; k += 4) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            cand = gs_point2(s, yin, xp, dh);
            yin = lane_shr1(yin, cand);
        }
    }
    const double x = 0.5 * cand;
    const double dif = old - x;
    if (mine) P[i] = x;
    return mine ? dif * dif : 0.0;
}

#ifdef DFTA_MG_SCAN_COARSE
// TOLERANCE MODE: a Gauss-Seidel sweep of the coarse section as an affine scan.  The sweep is the first-order recurrence
//     x_i = a x_{i-1} + c_i,   a = (1 + dh) / 2,   c_i = (S_i + (1 - dh) xold_{i+1}) / 2          (PoissonSolver.cpp:56-57, dh = delta_l / 2)
// with a constant ratio a ~ 0.5: lane t runs it over its own C nodes from 0 (z_k), the lanes' end values are combined by a
// Hillis-Steele scan with ratio a^C (6 shuffles + fma: x_end(t) = sum_j a^(C j) z_end(t - j), exact to rounding -- nothing is cut off), and
// the carry of the lane in front is added with precomputed powers, x_k = z_k + a^(k+1) x_end(t - 1).  2 C + 6 dependent steps per sweep
// instead of C + 32 (tolerance mode's chunked sweep) or n - 2 (the lane-shift sweep of the levels with <= 65 nodes); the same fixed point,
// a different order of roundings (gates: tests/test_gpu_resident.py).
template <int LOGC>
__device__ __forceinline__ double cs_sweep_scan(const double* __restrict__ Sg, double* __restrict__ Pg, const int n, const double dh)
{
    typedef __attribute__((address_space(3))) double lds_f64;
    typedef __attribute__((address_space(3))) const double lds_cf64;
    lds_cf64* S = (lds_cf64*)(Sg);
    lds_f64* P = (lds_f64*)(Pg);
    constexpr int C = 1 << LOGC;
    const int t = threadIdx.x & 63;
    const double a = 0.5 * (1.0 + dh), omd = 1.0 - dh;
    // old values of the lane's nodes and of the node behind them; node i = t C + k sits at (k << 6) + t, node n - 1 = 64 C at 64 C
    double old[C + 1], sv[C];
#pragma unroll
    for (int k = 0; k < C; ++k) { old[k] = P[(k << 6) + t]; sv[k] = S[(k << 6) + t]; }
    old[C] = (t == 63) ? P[C << 6] : P[t + 1];
    wave_sync();
    double z[C];
    double run = 0;
#pragma unroll
    for (int k = 0; k < C; ++k) {
        const double c = 0.5 * __builtin_fma(omd, old[k + 1], sv[k]);
        run = (t == 0 && k == 0) ? old[0] : __builtin_fma(a, run, c);      // node 0 is the boundary value
        z[k] = run;
    }
    // powers a^(k+1), k < C, and the scan ratios (a^C)^(2^s)
    double pw[C];
    pw[0] = a;
#pragma unroll
    for (int k = 1; k < C; ++k) pw[k] = pw[k - 1] * a;
    double ratio = pw[C - 1];
    double v = run;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const double up = __shfl_up(v, off, 64);
        if (t >= off) v = __builtin_fma(ratio, up, v);
        ratio *= ratio;
    }
    double xin = __shfl_up(v, 1, 64);
    if (t == 0) xin = 0.0;
    double err2 = 0;
#pragma unroll
    for (int k = 0; k < C; ++k) {
        const double x = (t == 0 && k == 0) ? old[0] : __builtin_fma(pw[k], xin, z[k]);
        const double dif = old[k] - x;
        if (!(t == 0 && k == 0)) { err2 += dif * dif; P[(k << 6) + t] = x; }
    }
    (void)n;
    return err2;
}

// the levels with <= 65 nodes in natural order: one node per lane
__device__ __forceinline__ double cs_sweep_scan_small(const double* __restrict__ Sg, double* __restrict__ Pg, const int n, const double dh)
{
    typedef __attribute__((address_space(3))) double lds_f64;
    typedef __attribute__((address_space(3))) const double lds_cf64;
    lds_cf64* S = (lds_cf64*)(Sg);
    lds_f64* P = (lds_f64*)(Pg);
    const int t = threadIdx.x & 63, i = t + 1;
    const bool mine = i < n - 1;
    const double a = 0.5 * (1.0 + dh), omd = 1.0 - dh;
    const double old = mine ? P[i] : 0.0;
    double c = mine ? 0.5 * __builtin_fma(omd, P[i + 1], S[i]) : 0.0;
    if (t == 0) c = __builtin_fma(a, P[0], c);                              // the boundary value enters through node 1
    wave_sync();
    double v = c, ratio = a;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const double up = __shfl_up(v, off, 64);
        if (t >= off) v = __builtin_fma(ratio, up, v);
        ratio *= ratio;
    }
    const double dif = old - v;
    if (mine) P[i] = v;
    return mine ? dif * dif : 0.0;
}
#endif

#ifndef DFTA_MG_SCAN_COARSE
// The three sweeps of a visit of a one-wave level with 4 .. 16 nodes per lane (257 .. 1025 nodes) as ONE fused pass on the level's LDS
// copy (gs_lds3: the software pipeline of the members' fused visit, here with the 64 lanes of the wave): 112 + C + 2 dependent steps and
// one prologue / norm / wave fence instead of 3 x (95 + C) steps and three of each.  Same arithmetic per node (gs_point2 / gs_point2y), so
// the values are those of three single sweeps bit for bit; the three norms are summed in another order -- they only gate the stop rule.
// When the reference would have stopped after the first or the second sweep (||dPhi|| < errorMin: PoissonSolver.cpp:66-77) the lane
// puts its nodes back as they were and the caller runs the visit sweep by sweep.  Returns true when the visit is done.
// (NT: the lanes that hold nodes -- 64, or 32 for the 129-node level, which is laid out 4 nodes per lane for this pass)
//
// Predicted start values (exact mode; POISSON_NOPREDICT: off).  The 112-node warm-up is 75 .. 95 % of the pass, and it is that long only
// because the stages start from OLD values, which on a correction level are off by O(1) of themselves: 2^53 ulp to contract away at
// b ~ 0.52 per node.  In exact arithmetic a sweep is the affine recurrence x_i = a x_(i-1) + c_i, a = (1 + dh) / 2,
// c_i = (S_i + (1 - dh) x_old(i+1)) / 2 (dh = d / 2), so the new values can be PREDICTED to a few ulp of the level's scale without any
// warm-up: every lane runs the recurrence over its chunk from zero (its offset), a log-depth scan over the lanes with the powers of a^C
// gives the value entering each chunk, and one more multiply-add per node the values inside it (cs_predict3: three such stages, each
// feeding on the one before -- ~12 C + 90 cheap instructions).  The fused pass then starts kPredW = 32 nodes in front of the chunk from
// the predictions: an error of a few ulp is gone after ~10 nodes of contraction (the pipeline amplifies it by <= 2^5.4 on the way).
// The prediction never reaches a result, because every visit is CHECKED: just before its first own step a lane's pipeline state must be,
// bit for bit, what the lane in front of it has computed for those nodes inside its own chunk (x1[lo-1], x2[lo-2], x3[lo-3]).  Lane 0
// starts on the level's boundary and the lanes up to node kPredW restart there, so by induction over the lanes a visit whose checks all
// pass is the sequential result exactly -- a stronger statement than the statistical 96 / 112-node argument.  On any mismatch the lanes
// put their nodes back and the visit is repeated with the full warm-up from old values; the error norms are the accepted pass's.

// Predictions of the three sweeps of a visit at the nodes where the lanes' short warm-ups start.  old[0..C-1]: the lane's nodes, sv: their
// sources (node lane * C + k), xN: the level's last node.  hs[0..2] = twice the predicted x1[lo-W-1], x2[lo-W-2], x3[lo-W-3], W = kPredW
// (W is a multiple of C: they are the last three nodes of lane - W/C - 1).  fuzz: every prediction off by a relative 2^-20 (tests).
template <int LOGC, int NT>
__device__ __forceinline__ void cs_predict3(const double (&old)[1 << LOGC], const double (&sv)[1 << LOGC], const double xN, const double dh,
                                            const int lane, const bool fuzz, double* hs)
{
    constexpr int C = 1 << LOGC;
    static_assert(kPredW % C == 0 && C >= 4, "the start nodes are the last three of one lane");
    const double a = 0.5 * (1.0 + dh), omd = 1.0 - dh;
    // a^(k+1), k < C; the scan's ratios (a^C)^(2^s) inside a row of 16 lanes, and (a^C)^(j+1) for the lane j lanes behind a row's / a
    // half-wave's last lane (the two steps across the rows)
    double pw[C];
    pw[0] = a;
#pragma unroll
    for (int k = 1; k < C; ++k) pw[k] = pw[k - 1] * a;
    const double A1 = pw[C - 1], A2 = A1 * A1, A4 = A2 * A2, A8 = A4 * A4, A16 = A8 * A8, A32 = A16 * A16;
    const int j31 = (lane & 31) + 1;
    double P15 = (j31 & 1) ? A1 : 1.0;
    P15 = (j31 & 2) ? P15 * A2 : P15;
    P15 = (j31 & 4) ? P15 * A4 : P15;
    P15 = (j31 & 8) ? P15 * A8 : P15;
    double P31 = (j31 & 16) ? P15 * A16 : P15;
    P31 = (j31 & 32) ? A32 : P31;
    P15 = ((lane & 15) == 15) ? A16 : P15;          // j15 = (lane & 15) + 1 = 16 where j31 = 16 or 32
    // one sweep: in[k] = the previous sweep's value of the lane's node k, in[C] = of the node behind the chunk
    auto stage = [&](const double (&in)[C + 1], double (&out)[C]) {
        double z[C];
        double run = 0;
#pragma unroll
        for (int k = 0; k < C; ++k) {
            const double c = 0.5 * __builtin_fma(omd, in[k + 1], sv[k]);
            run = (k == 0 && lane == 0) ? in[0] : __builtin_fma(a, run, c);       // node 0 is the boundary value
            z[k] = run;
        }
        double v = run;
        v = __builtin_fma(A1, wt_dpp<0x111, 0xf>(v), v);      // row_shr:1 (lanes without a source get 0: no contribution)
        v = __builtin_fma(A2, wt_dpp<0x112, 0xf>(v), v);      // row_shr:2
        v = __builtin_fma(A4, wt_dpp<0x114, 0xf>(v), v);      // row_shr:4
        v = __builtin_fma(A8, wt_dpp<0x118, 0xf>(v), v);      // row_shr:8
        v = __builtin_fma(P15, wt_dpp<0x142, 0xa>(v), v);     // row_bcast:15 into rows 1 and 3
        v = __builtin_fma(P31, wt_dpp<0x143, 0xc>(v), v);     // row_bcast:31 into rows 2 and 3
        const double xin = lane_shr1(0.0, v);
#pragma unroll
        for (int k = 0; k < C; ++k) out[k] = (k == 0 && lane == 0) ? in[0] : __builtin_fma(pw[k], xin, z[k]);
    };
    double in[C + 1], x1[C], x2[C];
#pragma unroll
    for (int k = 0; k < C; ++k) in[k] = old[k];
    in[C] = lane_shl1(xN, old[0]);
    in[C] = (lane == NT - 1) ? xN : in[C];
    stage(in, x1);
#pragma unroll
    for (int k = 0; k < C; ++k) in[k] = x1[k];
    in[C] = lane_shl1(xN, x1[0]);
    in[C] = (lane == NT - 1) ? xN : in[C];
    stage(in, x2);
#pragma unroll
    for (int k = 0; k < C; ++k) in[k] = x2[k];
    in[C] = lane_shl1(xN, x2[0]);
    in[C] = (lane == NT - 1) ? xN : in[C];
    double x3[C];
    stage(in, x3);
    constexpr int back = kPredW / C + 1;
    const double g = fuzz ? 2.0 * (1.0 + 0x1p-20) : 2.0;
    hs[0] = g * __shfl_up(x1[C - 1], back, 64);
    hs[1] = g * __shfl_up(x2[C - 2], back, 64);
    hs[2] = g * __shfl_up(x3[C - 3], back, 64);
}

// (predict: MgDesc::predict; ctr: the solver's counters of checked / repeated visits)
template <int LOGC, int NT = 64>
__device__ __forceinline__ bool cs_visit3(const double* __restrict__ S, double* __restrict__ P, const double dh, const double errorMin, double& err,
                                          const int predict, unsigned long long* ctr)
{
    constexpr int C = 1 << LOGC;
    typedef __attribute__((address_space(3))) double lds_f64;
    typedef __attribute__((address_space(3))) const double lds_cf64;
    lds_f64* pl = (lds_f64*)(P);
    const int lane = threadIdx.x & 63;
    double keep[C];
#pragma unroll
    for (int k = 0; k < C; ++k) keep[k] = pl[(k << 6) + lane];
    const double xN = pl[C << 6];                   // the level's last node (cs_idx)
    double f1, f2, f3;
    bool accepted = false;
    if constexpr (kPredict) {
        if (predict) {
            double sv[C], hs[9] = {};
#pragma unroll
            for (int k = 0; k < C; ++k) sv[k] = ((lds_cf64*)(S))[(k << 6) + lane];
            cs_predict3<LOGC, NT>(keep, sv, xN, dh, lane, predict == 2, hs);
            gs_lds3<LOGC, 64, NT, 3, true, false, kPredW, true>(S, P, lane, lane << LOGC, lane == NT - 1, xN, dh, f1, f2, f3, nullptr, nullptr, hs);
            // hand-over: what the lane in front left its chunk with (lane 0 has nobody in front: it compares with itself)
            bool bad = false;
#pragma unroll
            for (int q = 0; q < 3; ++q) {
                const double front = lane_shr1(hs[3 + q], hs[6 + q]);
                bad |= __builtin_bit_cast(long long, front) != __builtin_bit_cast(long long, hs[3 + q]);
            }
            const bool redo = __any(bad && lane < NT) != 0;
            if (lane == 0) {
                __hip_atomic_fetch_add(ctr, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (redo) __hip_atomic_fetch_add(ctr + 1, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            accepted = !redo;
            if (redo) {
                wave_sync();
                if (lane < NT) {
#pragma unroll
                    for (int k = 0; k < C; ++k) pl[(k << 6) + lane] = keep[k];
                }
                wave_sync();
            }
        }
    }
    if (!accepted) gs_lds3<LOGC, 64, NT, 3, true>(S, P, lane, lane << LOGC, lane == NT - 1, xN, dh, f1, f2, f3);
    const double e1 = sqrt(wave_total(f1)), e2 = sqrt(wave_total(f2)), e3 = sqrt(wave_total(f3));
    wave_sync();
    if (!(e1 < errorMin) && !(e2 < errorMin)) { err = e3; return true; }
    if (lane < NT) {
#pragma unroll
        for (int k = 0; k < C; ++k) pl[(k << 6) + lane] = keep[k];
    }
    wave_sync();
    return false;
}
#endif

// IterateGaussSeidel on the LDS copy of level l; all 64 lanes of the wave call
__device__ __forceinline__ double cs_iterate(const MgDesc& D, Atom& A, int l, double errorMin, int iterno, long* nsweeps)
{
    const Lvl L = D.lv[l];
    const double dh = L.d * 0.5;
    const int lane = threadIdx.x;
    double* P = A.stage + D.cs_phi[l];
    const double* S = A.stage + D.cs_src[l];
    const int lc = D.cs_lc[l];
    double err = 1E10;
#ifndef DFTA_MG_SCAN_COARSE
    const bool half = lc == 2 && L.n == 129;           // the 129-node level on 32 lanes x 4 nodes (poisson_plan.cpp, plan_coarse_section: exact mode)
    if (D.fuse3w && iterno == 3 && lc >= 2 && lc <= 4) {
        bool done;
        switch (lc) {
            case 2:  done = half ? cs_visit3<2, 32>(S, P, dh, errorMin, err, D.predict, D.pred_ctr) : cs_visit3<2>(S, P, dh, errorMin, err, D.predict, D.pred_ctr); break;
            case 3:  done = cs_visit3<3>(S, P, dh, errorMin, err, D.predict, D.pred_ctr); break;
            default: done = cs_visit3<4>(S, P, dh, errorMin, err, D.predict, D.pred_ctr); break;
        }
        if (done) { *nsweeps += 3; return err; }
    }
#else
    const bool half = false;
#endif
    for (int i = 0; i < iterno; ++i) {
        double err2 = 0;
#ifdef DFTA_MG_SCAN_COARSE
        if (lc >= 0) {
            switch (lc) {
                case 1:  err2 = cs_sweep_scan<1>(S, P, L.n, dh); break;
                case 2:  err2 = cs_sweep_scan<2>(S, P, L.n, dh); break;
                case 3:  err2 = cs_sweep_scan<3>(S, P, L.n, dh); break;
                default: err2 = cs_sweep_scan<4>(S, P, L.n, dh); break;
            }
            err2 = wave_total(err2);
        } else if (true) {
            err2 = cs_sweep_scan_small(S, P, L.n, dh);
            err2 = wave_total(err2);
        } else
#endif
        if (lc >= 0) {
            switch (lc) {
                case 1:  err2 = gs_lds<1, 64, 64>(S, P, lane, lane << lc, dh); break;
                case 2:  err2 = half ? ((lane & 63) < 32 ? gs_lds<2, 64, 32>(S, P, lane, lane << lc, dh) : 0.0) : gs_lds<2, 64, 64>(S, P, lane, lane << lc, dh); break;
                case 3:  err2 = gs_lds<3, 64, 64>(S, P, lane, lane << lc, dh); break;
                default: err2 = gs_lds<4, 64, 64>(S, P, lane, lane << lc, dh); break;
            }
            err2 = wave_total(err2);
        } else {
#ifdef DFTA_POISSON_SEQ_ONE_LANE
            if (lane == 0) err2 = seq_sweep_inplace(S, P, L.n, dh);
            err2 = __shfl(err2, 0);
#else
            err2 = seq_sweep_wave(S, P, L.n, dh);
            err2 = wave_total(err2);
#endif
        }
        err = sqrt(err2);
        ++*nsweeps;
        wave_sync();
        if (err < errorMin) break;
    }
    return err;
}

// PoissonSolver::Restrict into the LDS copy of level lc; the fine level is read through `fine(i)` / `fsrc(i)` (node index)
template <int NT, typename FP, typename FS>
__device__ __forceinline__ void cs_restrict(const MgDesc& D, Atom& A, int lvl, FP fine, FS fsrc)
{
    const Lvl Lc = D.lv[lvl];
    double* P = A.stage + D.cs_phi[lvl];
    double* S = A.stage + D.cs_src[lvl];
    const int lc = D.cs_lc[lvl], lim = Lc.n - 1;
    // four nodes per thread and pass, all their loads in flight together
    for (int i0 = threadIdx.x; i0 < Lc.n; i0 += 4 * NT) {
        double pm[4], p0[4], pp[4], s0[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int i = i0 + q * NT;
            if (i > 0 && i < lim) { pm[q] = fine(2 * i - 1); p0[q] = fine(2 * i); pp[q] = fine(2 * i + 1); s0[q] = fsrc(2 * i); }
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int i = i0 + q * NT;
            if (i < Lc.n) {
                double sv = 0;
                if (i > 0 && i < lim) sv = 4. * (s0[q] + pm[q] - 2. * p0[q] + pp[q]) - Lc.d * (pp[q] - pm[q]);
                const int idx = cs_idx(Lc.n, lc, i);
                S[idx] = sv;
                P[idx] = 0;
            }
        }
    }
    if (NT == 64) wave_sync();
}

// The whole part of a V-cycle below level cs_top (first wave of workgroup 0; the level above it, cs_top-1, is current in
// global memory on entry, and level cs_top is current in global memory on return).
// entry, by the whole workgroup: the restriction from level cs_top-1 (global) into the LDS copy of level cs_top
__device__ __forceinline__ void coarse_section_enter(const MgDesc& D, Atom& A)
{
    const int top = D.cs_top;
    const Lvl Lf = D.lv[top - 1];
    const int held = A.lds_holds;
    A.lds_holds = -1;
    if (held == top - 1 && D.fold_lds && Lf.logT == 8 && D.lv[top].n - 1 <= 4 * kThreads) {
        // round 6: level cs_top-1 lies in the staging memory as its visit has just left it (iterate_gs, stage 1: row k, column t =
        // storage index (k << 8) + t, the last node at n - 1: the global layout) -- read there instead of a round trip away.  The
        // coarse section's arrays share that memory: every thread takes its (up to four) values into registers, barrier, then stores.
        const Lvl Lc = D.lv[top];
        const double* Pf = A.stage + kStagePad;
        const double* Sf = Pf + kStageArr;
        double* P = A.stage + D.cs_phi[top];
        double* S = A.stage + D.cs_src[top];
        const int lc = D.cs_lc[top], lim = Lc.n - 1;
        const int tid = threadIdx.x;
        double sv[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int i = tid + q * kThreads;
            sv[q] = 0;
            if (i > 0 && i < lim) {
                const double pm = Pf[addr(Lf, 2 * i - 1) ], p0 = Pf[addr(Lf, 2 * i)], pp = Pf[addr(Lf, 2 * i + 1)], s0 = Sf[addr(Lf, 2 * i)];
                sv[q] = 4. * (s0 + pm - 2. * p0 + pp) - Lc.d * (pp - pm);       // the expression of cs_restrict
            }
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int i = tid + q * kThreads;
            if (i < lim) { const int idx = cs_idx(Lc.n, lc, i); S[idx] = sv[q]; P[idx] = 0; }
        }
        if (tid == 0) { const int idx = cs_idx(Lc.n, lc, lim); S[idx] = 0; P[idx] = 0; }
        return;
    }
    const double* __restrict__ Pf = (((A.cur >> (top - 1)) & 1u) ? A.phi1 : A.phi0) + Lf.off;
    const double* __restrict__ Sf = A.src + Lf.off;
    cs_restrict<kThreads>(D, A, top, [&](int i) { return Pf[addr(Lf, i)]; }, [&](int i) { return Sf[addr(Lf, i)]; });
}

// exit, by the whole workgroup: level cs_top goes back to its current global copy
__device__ __forceinline__ void coarse_section_leave(const MgDesc& D, Atom& A)
{
    const int top = D.cs_top;
    const Lvl L = D.lv[top];
    double* __restrict__ G = (((A.cur >> top) & 1u) ? A.phi1 : A.phi0) + L.off;
    const double* P = A.stage + D.cs_phi[top];
    const int lc = D.cs_lc[top];
    for (int i = threadIdx.x; i < L.n; i += kThreads) G[addr(L, i)] = P[cs_idx(L.n, lc, i)];
}

#ifndef DFTA_MG_SCAN_COARSE
// ---- EXACT mode: the six coarsest levels (65, 33, 17, 9, 5, 3 nodes) of the coarse section with Phi and S in REGISTERS ---------------
// Node t of a level sits in lane t of the wave (node 0 and the last node are the zero boundary values of a correction level: lane 0 holds
// 0, and what a shift from the right delivers behind the last lane in use is 0).  A sweep is the lane-shift form of seq_sweep_wave -- the
// candidate of node t, carried as y = 2x (gs_point2), is recomputed in every step from the candidate of node t-1 handed on by a DPP
// wave_shr:1, and is final from step t on: after n - 2 steps every lane holds what the sequential loop of PoissonSolver.cpp:40-64
// computes -- without the LDS loads, stores and wave fences between the sweeps of a visit and between the levels.  Restriction
// (PoissonSolver.cpp:126-157: the reference's expression at every fine node, the even ones move to lane t / 2) and prolongation
// (PoissonSolver.cpp:110-123) are lane arithmetic; IterateGaussSeidel's stop rule (PoissonSolver.cpp:66-77) as cs_iterate: the norm of
// every sweep, sqrt, compare.  Same operations on the same values in the same order as the level-by-level code (POISSON_NOXW: that code;
// tests/test_gpu_resident.py compares the two bit for bit).
__device__ __forceinline__ double xw_from_left(const double v) { return wt_dpp<0x138, 0xf>(v); }     // wave_shr:1: lane t <- lane t-1 (lane 0: 0)
__device__ __forceinline__ double xw_from_right(const double v) { return wt_dpp<0x130, 0xf>(v); }    // wave_shl:1: lane t <- lane t+1 (lane 63: 0)

struct XwCtx { double emin; int iterno, lane; long nsw; };

template <int NL>       // the level has NL + 1 nodes: unknowns in lanes 1 .. NL-1
__device__ __forceinline__ void xw_iterate(XwCtx& X, double& p, const double s, const double dh)
{
    const bool act = X.lane > 0 && X.lane < NL;
    for (int i = 0; i < X.iterno; ++i) {
        double xp = xw_from_right(p);                 // the OLD right neighbour (0 behind the last unknown)
        if (X.lane == 0) xp = 0.0;                    // lane 0 is the boundary node: s = 0, xp = 0 keep its candidate at exactly 0
        const double old = p;
        double c = 0.0;                               // candidates as y = 2 x; lane 0 stays 0 = twice the boundary value
#pragma unroll
        for (int k = 0; k < NL - 1; ++k) {
            const double yin = xw_from_left(c);
            c = gs_point2(s, yin, xp, dh);
        }
        const double x = 0.5 * c;
        const double dif = old - x;
        p = act ? x : 0.0;
        // (node t's share one lane down: the lane order of seq_sweep_wave, hence the same tree of additions and the same bits of the norm)
        const double err2 = wave_total(xw_from_right(act ? dif * dif : 0.0));
        ++X.nsw;
        if (sqrt(err2) < X.emin) break;
    }
}

template <int NL>
__device__ __forceinline__ void xw_level(const MgDesc& D, XwCtx& X, const int lvl, double& p, const double s)
{
    const double dh = D.lv[lvl].d * 0.5;
    xw_iterate<NL>(X, p, s, dh);
    if constexpr (NL > 2) {
        // Restrict (PoissonSolver.cpp:126-157): the combination at every fine node, the even ones move to lane t / 2
        const double pm = xw_from_left(p), pr = xw_from_right(p);
        const double r = 4. * (s + pm - 2. * p + pr) - D.lv[lvl + 1].d * (pr - pm);
        double sc = __shfl(r, (2 * X.lane) & 63, 64);
        if (X.lane == 0 || X.lane >= NL / 2) sc = 0.0;
        double pc = 0.0;
        xw_level<NL / 2>(D, X, lvl + 1, pc, sc);
        // Prolong (PoissonSolver.cpp:110-123)
        const double e = __shfl(pc, X.lane >> 1, 64);
        const double er = xw_from_right(e);
        const double add = (X.lane & 1) ? 0.5 * (e + er) : e;
        if (X.lane > 0 && X.lane < NL) p += add;
        xw_iterate<NL>(X, p, s, dh);
    }
}

// wave 0 of the coarse section: level `lvl` (65 nodes) and everything below it, entered from and left into the LDS copy of the 129-node
// level lvl - 1 (lane-interleaved: cs_idx with lc = 1, or lc = 2 on 32 lanes)
__device__ __forceinline__ void xw_section(const MgDesc& D, Atom& A, const int lvl, const double errorMin, const int iterno, long* nsweeps)
{
    const int lane = threadIdx.x & 63;
    const int nf = D.lv[lvl - 1].n, lcf = D.cs_lc[lvl - 1];
    double* Pf = A.stage + D.cs_phi[lvl - 1];
    const double* Sf = A.stage + D.cs_src[lvl - 1];
    // Restrict into lane t = coarse node t (cs_restrict's expression; node 0 and node 64 are boundary values: 0)
    double sc = 0.0;
    if (lane > 0) {
        const double pm = Pf[cs_idx(nf, lcf, 2 * lane - 1)], p0 = Pf[cs_idx(nf, lcf, 2 * lane)], pp = Pf[cs_idx(nf, lcf, 2 * lane + 1)];
        const double s0 = Sf[cs_idx(nf, lcf, 2 * lane)];
        sc = 4. * (s0 + pm - 2. * p0 + pp) - D.lv[lvl].d * (pp - pm);
    }
    XwCtx X;
    X.emin = errorMin; X.iterno = iterno; X.lane = lane; X.nsw = 0;
    double pc = 0.0;
    xw_level<64>(D, X, lvl, pc, sc);
    // Prolong into the 129-node level (PoissonSolver.cpp:110-123): Pf[2 i] += c_i, Pf[2 i - 1] += (c_{i-1} + c_i) / 2, i = 0 .. 64 (c_0 = c_64 = 0)
    const double cl = xw_from_left(pc);
    if (lane > 0) {
        Pf[cs_idx(nf, lcf, 2 * lane)] += pc;
        Pf[cs_idx(nf, lcf, 2 * lane - 1)] += 0.5 * (cl + pc);
    }
    if (lane == 63) Pf[cs_idx(nf, lcf, 127)] += 0.5 * (pc + 0.0);      // i = 64: the node under the last boundary value
    *nsweeps += X.nsw;
    wave_sync();
}
#endif

// (-DDFTA_POISSON_RPROF: csprof = the coarse workgroup's timer rows -- row 1: the sweeps of every one-wave level [level & 7], row 7: [0] the
// restrictions, [1] the prolongations, [2] the register levels (xw_section))
#ifdef DFTA_POISSON_RPROF
#define CS_T0() const long long cs_t0 = clock64()
#define CS_ADD(row, col) do { if (csprof && threadIdx.x == 0) csprof[(row) * 8 + ((col) & 7)] += clock64() - cs_t0; } while (0)
#else
#define CS_T0()
#define CS_ADD(row, col)
#endif
__device__ __forceinline__ void coarse_section(const MgDesc& D, Atom& A, double errorMin, int iterno, long* nsweeps, int top_level = -1, unsigned long long* csprof = nullptr)
{
    (void)csprof;
    const int top = top_level >= 0 ? top_level : D.cs_top;
#ifndef DFTA_MG_SCAN_COARSE
    // exact mode: the levels from 65 nodes down run in registers (xw_section), the loops below end on the 129-node level
    const bool xw = D.xw_top > top;
    const int last = xw ? D.xw_top - 1 : D.levels - 1;
#else
    const int last = D.levels - 1;
#endif
    // down: iterate, then restrict / iterate
    { CS_T0(); cs_iterate(D, A, top, errorMin, iterno, nsweeps); CS_ADD(1, top); }
    for (int l = top + 1; l <= last; ++l) {
        const int nf = D.lv[l - 1].n, lcf = D.cs_lc[l - 1];
        const double* Pf = A.stage + D.cs_phi[l - 1];
        const double* Sf = A.stage + D.cs_src[l - 1];
        { CS_T0(); cs_restrict<64>(D, A, l, [&](int i) { return Pf[cs_idx(nf, lcf, i)]; }, [&](int i) { return Sf[cs_idx(nf, lcf, i)]; }); CS_ADD(7, 0); }
        { CS_T0(); cs_iterate(D, A, l, errorMin, iterno, nsweeps); CS_ADD(1, l); }
    }
#ifndef DFTA_MG_SCAN_COARSE
    if (xw) {
        // the 129-node level has been iterated on the way down; the six levels below it in registers; its second visit follows
        { CS_T0(); xw_section(D, A, D.xw_top, errorMin, iterno, nsweeps); CS_ADD(7, 2); }
        { CS_T0(); cs_iterate(D, A, last, errorMin, iterno, nsweeps); CS_ADD(1, last); }
    }
#endif
    // up: prolong (PoissonSolver.cpp:110-123), iterate
    for (int l = last - 1; l >= top; --l) {
        const int nc = D.lv[l + 1].n, lcc = D.cs_lc[l + 1], nf = D.lv[l].n, lcf = D.cs_lc[l];
        const double* Pc = A.stage + D.cs_phi[l + 1];
        double* Pf = A.stage + D.cs_phi[l];
        { CS_T0();
        for (int i = threadIdx.x; i < nc; i += 64) {
            const double c = Pc[cs_idx(nc, lcc, i)];
            Pf[cs_idx(nf, lcf, 2 * i)] += c;
            if (i > 0) Pf[cs_idx(nf, lcf, 2 * i - 1)] += 0.5 * (Pc[cs_idx(nc, lcc, i - 1)] + c);
        }
        wave_sync();
        CS_ADD(7, 1); }
        { CS_T0(); cs_iterate(D, A, l, errorMin, iterno, nsweeps); CS_ADD(1, l); }
    }
}

#ifdef DFTA_MG_SCAN_COARSE
// ---- TOLERANCE MODE, resident groups: the coarse workgroup's part of a V-cycle with its levels in REGISTERS -------------------------
// Between the members' hand-over of the first coarse level's source (level rc_top = kres: 8193 nodes, Phi = 0) and the hand-over of
// its Phi, the coarse workgroup runs  iterate, restrict, ..., iterate (coarsest), prolong, iterate, ...  over 13 levels.  Level by level
// that costs a staging copy in and out of LDS, workgroup barriers and a warm-up per visit (27 % + 34 % of a solve, DESIGN.md 4.3c).  Here
// thread t of the workgroup's 256 owns the nodes [t C, t C + C) of EVERY level down to 257 nodes (C = 32, 16, 8, 4, 2, 1) and keeps
// their Phi in registers through the recursion (the sources in LDS, written and read by their owner only): restriction and prolongation
// are thread-local up to one neighbour value (DPP lane shifts; across the four waves through 8 doubles of LDS), and a Gauss-Seidel sweep
// is the affine scan of cs_sweep_scan: the chunk's recurrence from zero, a wave scan of the chunk ends with ratio r = a^C in DPP steps, the
// value in front of the wave (the end of the wave in front: r^64 of anything further back is < 1e-18, poisson_plan.cpp: plan_rc checks) added to lane t's
// input with r^t, the carry into the chunk with running powers of a -- 2 C + 6 dependent steps and ONE workgroup barrier per sweep (rc_iterate).
// The levels with <= 129 nodes run in one wave, every level in registers (rw_cycle).  Same operations, stop rules and sweep counts as the
// level-by-level code, a different order of roundings (tolerance mode; gates: tests/test_gpu_resident.py -- the uniform grid, where only
// the coarsest levels remove the smooth error, is the sensitive case).  Also run by workgroup 0 of a staged group (from its first own
// level: 8193, 4097 or 2049 nodes) and by the one workgroup of an atom (run_cycles).
typedef __attribute__((address_space(3))) double rc_lds;     // LDS through ds_ instructions (a generic pointer costs a flat access)
struct RcCtx {
    rc_lds* sc;        // LDS scratch: first[2][4], last[2][4], carry[2][4], norm[2][4]
    unsigned par;
    int lane, wv, tid;
    double emin;
    int iterno;
    long nsw;
#ifdef DFTA_POISSON_RPROF
    unsigned long long* prof;
#endif
};
#ifdef DFTA_POISSON_RPROF
#define RC_T0() const long long rc_t0 = clock64()
#define RC_ADD(cat, col) do { if (X.tid == 0 && X.prof) X.prof[(cat) * 8 + ((col) & 7)] += clock64() - rc_t0; } while (0)
#else
#define RC_T0()
#define RC_ADD(cat, col)
#endif
__device__ __forceinline__ rc_lds* rc_first(const RcCtx& X, unsigned par) { return X.sc + par * 4; }
__device__ __forceinline__ rc_lds* rc_last(const RcCtx& X, unsigned par) { return X.sc + 8 + par * 4; }
__device__ __forceinline__ rc_lds* rc_carry(const RcCtx& X, unsigned par) { return X.sc + 16 + par * 4; }
__device__ __forceinline__ rc_lds* rc_norm(const RcCtx& X, unsigned par) { return X.sc + 24 + par * 4; }

// lane shifts and the wave scan through DPP (a `__shfl` of a double is two ds_bpermute round trips: ~150 cycles per dependent step)
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ double rc_dpp(const double src)
{
    const long long x = __builtin_bit_cast(long long, src);
    const int lo = __builtin_amdgcn_update_dpp(0, (int)x, CTRL, ROW_MASK, 0xf, false);
    const int hi = __builtin_amdgcn_update_dpp(0, (int)(x >> 32), CTRL, ROW_MASK, 0xf, false);
    return __builtin_bit_cast(double, ((long long)hi << 32) | (unsigned)lo);
}
__device__ __forceinline__ double rc_from_left(const double v) { return rc_dpp<0x138, 0xf>(v); }    // wave_shr:1: lane t <- lane t-1 (lane 0: 0)
__device__ __forceinline__ double rc_from_right(const double v) { return rc_dpp<0x130, 0xf>(v); }   // wave_shl:1: lane t <- lane t+1 (lane 63: 0)

// per visit: the powers of r = a^C that the scan x_t = v_t + r x_{t-1} over the 64 lanes needs
struct RcScan { double r1, r2, r4, r8, wA, wB, wL; };
__device__ __forceinline__ RcScan rc_scan_setup(const double r, const int lane)
{
    RcScan S;
    S.r1 = r; S.r2 = r * r; S.r4 = S.r2 * S.r2; S.r8 = S.r4 * S.r4;
    const double r16 = S.r8 * S.r8, r32 = r16 * r16;
    auto pw = [&](int e) {      // r^e, 0 <= e <= 63
        double w = 1.0;
        if (e & 1) w *= S.r1;
        if (e & 2) w *= S.r2;
        if (e & 4) w *= S.r4;
        if (e & 8) w *= S.r8;
        if (e & 16) w *= r16;
        if (e & 32) w *= r32;
        return w;
    };
    S.wA = pw((lane & 15) + 1);                   // from lane 15 of the row in front
    S.wB = lane >= 32 ? pw(lane - 31) : 0.0;      // from lane 31
    S.wL = pw(lane);                              // what the value in front of the wave contributes to the value in front of this lane
    return S;
}
__device__ __forceinline__ double rc_scan(const RcScan& S, double v)
{
    v = __builtin_fma(S.r1, rc_dpp<0x111, 0xf>(v), v);      // row_shr:1
    v = __builtin_fma(S.r2, rc_dpp<0x112, 0xf>(v), v);      // row_shr:2
    v = __builtin_fma(S.r4, rc_dpp<0x114, 0xf>(v), v);      // row_shr:4
    v = __builtin_fma(S.r8, rc_dpp<0x118, 0xf>(v), v);      // row_shr:8
    v = __builtin_fma(S.wA, rc_dpp<0x142, 0xa>(v), v);      // row_bcast15 into rows 1 and 3
    v = __builtin_fma(S.wB, rc_dpp<0x143, 0xc>(v), v);      // row_bcast31 into rows 2 and 3
    return v;
}

// sum over the wave, valid in lane 63
__device__ __forceinline__ double rc_sum63(double v)
{
    v += rc_dpp<0x111, 0xf>(v);
    v += rc_dpp<0x112, 0xf>(v);
    v += rc_dpp<0x114, 0xf>(v);
    v += rc_dpp<0x118, 0xf>(v);
    v += rc_dpp<0x142, 0xa>(v);
    v += rc_dpp<0x143, 0xc>(v);
    return v;
}

// IterateGaussSeidel (PoissonSolver.cpp:66-77) of a level held in registers: up to iterno sweeps, stop after a sweep with ||dPhi|| < errorMin.
// ONE workgroup barrier per sweep: before it every wave publishes the end value of its chunk scan (the carry for the wave behind it), the
// old value of its first node (the right neighbour of the last node of the wave in front) and the norm of the PREVIOUS sweep -- whose
// stop test is therefore taken after the barrier, before this sweep is applied; after it lane 63 adds its last node's share of that
// neighbour, c = (1 - dh)/2 x_right, which is linear, and every lane t of the wave behind adds r^t (carry + that share) to its input.  A last barrier makes the waves' boundary values visible to
// the transfer that follows.  Node 0 (thread 0, k = 0) and node n-1 (right of thread 255) are boundary values (0 on these levels).
template <int C>
__device__ __forceinline__ void rc_iterate(RcCtx& X, double (&p)[C], const double* __restrict__ s, const double dh)
{
    typedef __attribute__((address_space(3))) const double lds_cf64;
    lds_cf64* sl = (lds_cf64*)(s) + X.tid;
    const double a = 0.5 * (1.0 + dh), omd2 = 0.5 * (1.0 - dh);
    double ratio = a;
#pragma unroll
    for (int q = 1; q < C; q <<= 1) ratio *= ratio;       // a^C
    const RcScan S = rc_scan_setup(ratio, X.lane);
    const double emin2 = X.emin * X.emin;
    double e2_prev = 0;
    for (int i = 0; i < X.iterno; ++i) {
        double xr = rc_from_right(p[0]);                    // lane 63: 0 for now
        double z[C];
        double run = 0.0;
#pragma unroll
        for (int k = 0; k < C; ++k) {
            const double right = (k + 1 < C) ? p[k + 1] : xr;
            const double c = __builtin_fma(omd2, right, 0.5 * sl[k << 8]);
            run = (X.tid == 0 && k == 0) ? p[0] : __builtin_fma(a, run, c);
            z[k] = run;
        }
        double v = rc_scan(S, run);
        if (X.lane == 63) { rc_carry(X, X.par)[X.wv] = v; rc_norm(X, X.par)[X.wv] = e2_prev; }
        if (X.lane == 0) rc_first(X, X.par)[X.wv] = p[0];
        __syncthreads();
        if (i > 0) {
            const rc_lds* nn = rc_norm(X, X.par);
            if ((nn[0] + nn[1]) + (nn[2] + nn[3]) < emin2) { X.par ^= 1u; break; }       // ||dPhi|| < errorMin: the previous sweep was the last
        }
        // the old first node of the wave behind: its share of this wave's last node, and of the carry into the next wave.  The value in
        // front of the wave -- the end of the scan of the wave in front plus that share of ITS last node -- reaches lane t's input with r^t
        // (what it adds to the end of this wave, r^64 <= 3e-19 of it, is dropped)
        const double dl = (X.wv < 3) ? omd2 * rc_first(X, X.par)[X.wv + 1] : 0.0;
        const double win = X.wv > 0 ? rc_carry(X, X.par)[X.wv - 1] + omd2 * rc_first(X, X.par)[X.wv] : 0.0;
        const double xin = __builtin_fma(S.wL, win, rc_from_left(v));
        if (X.lane == 63) z[C - 1] += dl;
        double e2 = 0, cin = xin;
#pragma unroll
        for (int k = 0; k < C; ++k) {
            cin *= a;
            const double x = (X.tid == 0 && k == 0) ? p[0] : z[k] + cin;
            const double dif = p[k] - x;
            e2 = __builtin_fma(dif, dif, e2);
            p[k] = x;
        }
        e2_prev = rc_sum63(e2);
        ++X.nsw;
        X.par ^= 1u;
    }
    // boundary values for the transfer that follows (restriction: the last node of the wave in front; prolongation: the first node of the wave
    // behind).  The parity flips once more behind the barrier: the transfer reads the buffers of X.par ^ 1 while a wave that is already in the
    // next level's first sweep writes those of X.par.
    if (X.lane == 0) rc_first(X, X.par)[X.wv] = p[0];
    if (X.lane == 63) rc_last(X, X.par)[X.wv] = p[C - 1];
    __syncthreads();
    X.par ^= 1u;
}

// Restrict (PoissonSolver.cpp:126-157): fine (p, s) -> coarse source (LDS, this thread's own entries); the coarse Phi starts from zero.
// dc: delta of the coarse level.
template <int CF>
__device__ __forceinline__ void rc_restrict(const RcCtx& X, const double (&p)[CF], const double* __restrict__ s_, double* __restrict__ sc_, const double dc)
{
    const rc_lds* s = (const rc_lds*)(s_);
    rc_lds* sc = (rc_lds*)(sc_);
    double pm = rc_from_left(p[CF - 1]);                      // fine node t CF - 1
    if (X.lane == 0) pm = X.wv > 0 ? rc_last(X, X.par ^ 1u)[X.wv - 1] : 0.0;
#pragma unroll
    for (int k = 0; k < CF / 2; ++k) {
        const double p0 = p[2 * k], pp = p[2 * k + 1];
        double v = 4. * (s[((2 * k) << 8) + X.tid] + pm - 2. * p0 + pp) - dc * (pp - pm);
        if (X.tid == 0 && k == 0) v = 0.0;                    // coarse node 0
        sc[(k << 8) + X.tid] = v;
        pm = pp;
    }
}

// Prolong (PoissonSolver.cpp:110-123): fine += coarse (the coarse level's boundary values were published by its last rc_iterate)
template <int CF>
__device__ __forceinline__ void rc_prolong(RcCtx& X, double (&p)[CF], const double (&pc)[CF / 2])
{
    double cr = rc_from_right(pc[0]);                         // coarse node (t + 1) CC
    if (X.lane == 63) cr = X.wv < 3 ? rc_first(X, X.par ^ 1u)[X.wv + 1] : 0.0;
#pragma unroll
    for (int k = 0; k < CF / 2; ++k) {
        const double c = pc[k], cn = (k + 1 < CF / 2) ? pc[k + 1] : cr;
        if (!(X.tid == 0 && k == 0)) p[2 * k] += c;
        p[2 * k + 1] += 0.5 * (c + cn);
    }
}

// ---- the levels with <= 129 nodes: ONE wave, every level in registers (no barriers, no LDS between entry and exit) -----------------
// 129 nodes: lane t holds nodes 2t, 2t + 1; 65 .. 3 nodes: node i in lane i (NL = n - 1 lanes hold nodes; the rest keep Phi = S = 0, and
// node n - 1, the zero boundary value, is what a shift from the right delivers).  Sweeps as in rc_iterate with the scan cut to the lanes
// in use; restriction computes the residual combination in place (DPP neighbours) and compacts the even lanes (one ds_bpermute pair),
// prolongation expands the same way.
template <int NL>
__device__ __forceinline__ RcScan rw_scan_setup(const double r, const int lane)
{
    RcScan S;
    S.r1 = r; S.r2 = r * r; S.r4 = S.r2 * S.r2; S.r8 = S.r4 * S.r4;
    S.wA = 0.0; S.wB = 0.0; S.wL = 0.0;
    if constexpr (NL > 16) {
        const double r16 = S.r8 * S.r8, r32 = r16 * r16;
        auto pw = [&](int e) {
            double w = 1.0;
            if (e & 1) w *= S.r1;
            if (e & 2) w *= S.r2;
            if (e & 4) w *= S.r4;
            if (e & 8) w *= S.r8;
            if (e & 16) w *= r16;
            if (e & 32) w *= r32;
            return w;
        };
        S.wA = pw((lane & 15) + 1);
        if constexpr (NL > 32) S.wB = lane >= 32 ? pw(lane - 31) : 0.0;
    }
    return S;
}
template <int NL>
__device__ __forceinline__ double rw_scan(const RcScan& S, double v)
{
    if constexpr (NL > 1) v = __builtin_fma(S.r1, rc_dpp<0x111, 0xf>(v), v);
    if constexpr (NL > 2) v = __builtin_fma(S.r2, rc_dpp<0x112, 0xf>(v), v);
    if constexpr (NL > 4) v = __builtin_fma(S.r4, rc_dpp<0x114, 0xf>(v), v);
    if constexpr (NL > 8) v = __builtin_fma(S.r8, rc_dpp<0x118, 0xf>(v), v);
    if constexpr (NL > 16) v = __builtin_fma(S.wA, rc_dpp<0x142, 0xa>(v), v);
    if constexpr (NL > 32) v = __builtin_fma(S.wB, rc_dpp<0x143, 0xc>(v), v);
    return v;
}
// sum over lanes 0 .. NL-1 (the others hold 0), returned wave-uniform
template <int NL>
__device__ __forceinline__ double rw_sum(double v)
{
    if constexpr (NL > 1) v += rc_dpp<0x111, 0xf>(v);
    if constexpr (NL > 2) v += rc_dpp<0x112, 0xf>(v);
    if constexpr (NL > 4) v += rc_dpp<0x114, 0xf>(v);
    if constexpr (NL > 8) v += rc_dpp<0x118, 0xf>(v);
    if constexpr (NL > 16) v += rc_dpp<0x142, 0xa>(v);
    if constexpr (NL > 32) v += rc_dpp<0x143, 0xc>(v);
    constexpr int src = NL >= 64 ? 63 : (NL > 16 ? 31 : NL - 1);  // the last lane in use: the prefix sum there has reached all of them
    const long long x = __builtin_bit_cast(long long, v);
    const int lo = __builtin_amdgcn_readlane((int)x, src), hi = __builtin_amdgcn_readlane((int)(x >> 32), src);
    return __builtin_bit_cast(double, ((long long)hi << 32) | (unsigned)lo);
}

template <int C, int NL>
__device__ __forceinline__ void rw_iterate(RcCtx& X, double (&p)[C], const double (&s)[C], const double dh)
{
    const double a = 0.5 * (1.0 + dh), omd2 = 0.5 * (1.0 - dh);
    double ratio = a;
#pragma unroll
    for (int q = 1; q < C; q <<= 1) ratio *= ratio;
    const RcScan S = rw_scan_setup<NL>(ratio, X.lane);
    const double emin2 = X.emin * X.emin;
    const bool act = X.lane < NL;
    for (int i = 0; i < X.iterno; ++i) {
        const double xr = rc_from_right(p[0]);
        double z[C];
        double run = 0.0;
#pragma unroll
        for (int k = 0; k < C; ++k) {
            const double right = (k + 1 < C) ? p[k + 1] : xr;
            const double c = __builtin_fma(omd2, right, 0.5 * s[k]);
            run = (X.lane == 0 && k == 0) ? p[0] : __builtin_fma(a, run, c);
            z[k] = run;
        }
        const double v = rw_scan<NL>(S, run);
        double cin = rc_from_left(v), e2 = 0;
#pragma unroll
        for (int k = 0; k < C; ++k) {
            cin *= a;
            double x = (X.lane == 0 && k == 0) ? p[0] : z[k] + cin;
            if (!act) x = 0.0;
            const double dif = p[k] - x;
            e2 = __builtin_fma(dif, dif, e2);
            p[k] = x;
        }
        ++X.nsw;
        if (rw_sum<NL>(e2) < emin2) break;
    }
}

template <int NL>
__device__ __forceinline__ void rw_level(const MgDesc& D, RcCtx& X, const int lvl, double& p, const double s)
{
    const double dh = D.lv[lvl].d * 0.5;
    double pa[1] = {p};
    const double sa[1] = {s};
    rw_iterate<1, NL>(X, pa, sa, dh);
    if constexpr (NL > 2) {
        // Restrict (PoissonSolver.cpp:126-157): the combination at every fine node, the even ones move to lane i / 2
        const double pm = rc_from_left(pa[0]), pr = rc_from_right(pa[0]);
        const double r = 4. * (s + pm - 2. * pa[0] + pr) - D.lv[lvl + 1].d * (pr - pm);
        double sc = __shfl(r, (2 * X.lane) & 63, 64);
        if (X.lane == 0 || X.lane >= NL / 2) sc = 0.0;
        double pc = 0.0;
        rw_level<NL / 2>(D, X, lvl + 1, pc, sc);
        // Prolong (PoissonSolver.cpp:110-123)
        const double e = __shfl(pc, X.lane >> 1, 64);
        const double er = rc_from_right(e);
        const double add = (X.lane & 1) ? 0.5 * (e + er) : e;
        if (X.lane > 0 && X.lane < NL) pa[0] += add;
        rw_iterate<1, NL>(X, pa, sa, dh);
    }
    p = pa[0];
}

// wave 0: the 129-node level `lvl` (source in Sl, natural order) and everything below it; its Phi goes to Pl
__device__ __forceinline__ void rw_cycle(const MgDesc& D, RcCtx& X, const int lvl, const rc_lds* Sl, rc_lds* Pl)
{
    const double dh = D.lv[lvl].d * 0.5;
    double p[2] = {0.0, 0.0};
    const double s[2] = {Sl[2 * X.lane], Sl[2 * X.lane + 1]};
    rw_iterate<2, 64>(X, p, s, dh);
    const double pm = rc_from_left(p[1]);
    double sc = 4. * (s[0] + pm - 2. * p[0] + p[1]) - D.lv[lvl + 1].d * (p[1] - pm);
    if (X.lane == 0) sc = 0.0;
    double pc = 0.0;
    rw_level<64>(D, X, lvl + 1, pc, sc);
    const double cr = rc_from_right(pc);
    if (X.lane > 0) p[0] += pc;
    p[1] += 0.5 * (pc + cr);
    rw_iterate<2, 64>(X, p, s, dh);
    Pl[2 * X.lane] = p[0];
    Pl[2 * X.lane + 1] = p[1];
    if (X.lane == 0) Pl[128] = 0.0;
}

// the levels with one node per thread (257 nodes) and below: restriction into LDS, the one-wave cycle, prolongation out of LDS
__device__ __forceinline__ void rc_wave_section(const MgDesc& D, Atom& A, RcCtx& X, const int lvl /* the 257-node level */, double (&p)[1], const double* __restrict__ s_)
{
    const int lc_lvl = lvl + 1;                               // 129 nodes
    const Lvl Lc = D.lv[lc_lvl];
    rc_lds* Pc = (rc_lds*)(A.stage + D.cs_phi[lc_lvl]);      // natural order here
    rc_lds* Sc = (rc_lds*)(A.stage + D.cs_src[lc_lvl]);
    const rc_lds* s = (const rc_lds*)(s_);
    // restriction: coarse node i = t / 2 under the fine nodes t - 1, t, t + 1 (even t)
    double pm = rc_from_left(p[0]), pp = rc_from_right(p[0]);
    if (X.lane == 0) pm = X.wv > 0 ? rc_last(X, X.par ^ 1u)[X.wv - 1] : 0.0;
    if (X.lane == 63) pp = X.wv < 3 ? rc_first(X, X.par ^ 1u)[X.wv + 1] : 0.0;
    if ((X.tid & 1) == 0) {
        const int i = X.tid >> 1;
        double sv = 4. * (s[X.tid] + pm - 2. * p[0] + pp) - Lc.d * (pp - pm);
        if (i == 0) sv = 0.0;
        Sc[i] = sv;
    }
    if (X.tid == 0) Sc[128] = 0.0;
    __syncthreads();
    if (X.tid < 64) { const long n0 = X.nsw; rw_cycle(D, X, lc_lvl, Sc, Pc); if (X.tid == 0) X.sc[32] = static_cast<double>(X.nsw - n0); X.nsw = n0; }
    __syncthreads();
    X.nsw += static_cast<long>(X.sc[32]);
    // prolongation: fine node t += coarse t/2 (even t), += (coarse (t-1)/2 + coarse (t+1)/2) / 2 (odd t)
    if (X.tid & 1) p[0] += 0.5 * (Pc[X.tid >> 1] + Pc[(X.tid >> 1) + 1]);
    else if (X.tid > 0) p[0] += Pc[X.tid >> 1];
}

template <int C>
__device__ __forceinline__ void rc_level(const MgDesc& D, Atom& A, RcCtx& X, const int lvl, double (&p)[C])
{
    const double dh = D.lv[lvl].d * 0.5;
    const double* s = A.stage + D.rc_src[lvl - D.rc_top];
    { RC_T0(); rc_iterate<C>(X, p, s, dh); RC_ADD(1, lvl - D.rc_top); }      // on the way down Phi starts from zero
    if constexpr (C > 1) {
        double pc[C / 2];
#pragma unroll
        for (int k = 0; k < C / 2; ++k) pc[k] = 0.0;
        { RC_T0(); rc_restrict<C>(X, p, s, A.stage + D.rc_src[lvl + 1 - D.rc_top], D.lv[lvl + 1].d); RC_ADD(7, 1); }
        rc_level<C / 2>(D, A, X, lvl + 1, pc);
        { RC_T0(); rc_prolong<C>(X, p, pc); RC_ADD(7, 2); }
    } else {
        RC_T0(); rc_wave_section(D, A, X, lvl, p, s); RC_ADD(7, 0);
    }
    { RC_T0(); rc_iterate<C>(X, p, s, dh); RC_ADD(1, lvl - D.rc_top); }
}

// all threads of the coarse workgroup; level rc_top: source complete in global memory, Phi = 0; on return its Phi is in copy 0
template <int C>
__device__ __forceinline__ void coarse_resident_cycle_c(const MgDesc& D, Atom& A, const double errorMin, const int iterno, long* nsweeps, unsigned long long* prof)
{
    const int top = D.rc_top;
    const Lvl L = D.lv[top];
    RcCtx X;
    X.sc = (rc_lds*)(A.stage + 2 * kStageArr - 64);
    X.par = 0;
    X.tid = static_cast<int>(threadIdx.x); X.lane = X.tid & 63; X.wv = X.tid >> 6;
    X.emin = errorMin; X.iterno = iterno; X.nsw = 0;
#ifdef DFTA_POISSON_RPROF
    X.prof = prof;
#endif
    double p[C];
    const double* __restrict__ Sg = A.src + L.off;
    rc_lds* s0 = (rc_lds*)(A.stage + D.rc_src[0]);
#pragma unroll
    for (int k = 0; k < C; ++k) { s0[(k << 8) + X.tid] = Sg[(k << 8) + X.tid]; p[k] = 0.0; }      // own entries only: no barrier needed
    rc_level<C>(D, A, X, top, p);
    double* __restrict__ Pg = A.phi0 + L.off;
#pragma unroll
    for (int k = 0; k < C; ++k) Pg[(k << 8) + X.tid] = p[k];
    if (X.tid == 0) Pg[C << 8] = 0.0;
    A.cur &= ~(1u << top);
    A.pend = 0; A.pend_r = 0; A.pend_z = 0;
    *nsweeps += X.nsw;
    __syncthreads();
}
// the cycle starts on level rc_top: 8193 nodes (32 per thread), or 4097 / 2049 where a staged group of 4 / 2 shares the levels above
__device__ __forceinline__ void coarse_resident_cycle(const MgDesc& D, Atom& A, const double errorMin, const int iterno, long* nsweeps, unsigned long long* prof = nullptr)
{
    switch (D.lv[D.rc_top].logC) {
        case 5:  coarse_resident_cycle_c<32>(D, A, errorMin, iterno, nsweeps, prof); break;
        case 4:  coarse_resident_cycle_c<16>(D, A, errorMin, iterno, nsweeps, prof); break;
        default: coarse_resident_cycle_c<8>(D, A, errorMin, iterno, nsweeps, prof); break;
    }
}
#endif

template <bool CS>
__device__ __forceinline__ double run_cycles(const MgDesc& D, Atom& A, int first_step, int max_vcycles, double errorMin,
                                             double errorMinLast, double* red, Counters& c)
{
    const int last = D.levels - 1;
    const int nramp = D.levels - 2 > 0 ? D.levels - 2 : 0;
    double err = 0;
    bool cs_skip = false, rc_skip = false;
    double err_prev = 0, err_first = 0;
    int stalled = 0;
    for (int step = first_step;; ++step) {
        int from, to, iterno = 3;
        double emin = errorMin;
        bool vleg_down = false;
        if (step == 0) { from = to = last; iterno = 15; }
        else if (step <= 2 * nramp) {
            const int q = (step - 1) >> 1;
            const int i = D.levels - 2 - q;
            if ((step - 1) & 1) { from = i; to = last; } else { from = last; to = i; }
        } else if (step == 2 * nramp + 1) { from = last; to = 0; emin = errorMinLast; }
        else {
            emin = errorMinLast;
            if ((step - (2 * nramp + 2)) & 1) { from = last; to = 0; vleg_down = true; } else { from = 0; to = last; }
        }
        const int dir = (from > to) ? -1 : 1;
        err = 1E10;
        if (!(dir < 0 && from == to)) {
            int first_lvl = (dir > 0) ? from : from - 1;
            if (CS && cs_skip) { first_lvl = D.cs_top - 1; cs_skip = false; }       // the section has done last .. cs_top
            if (rc_skip) { first_lvl = D.rc_top - 1; rc_skip = false; }             // the register cycle has done last .. rc_top
            for (int lvl = first_lvl;; lvl += dir) {
#ifdef DFTA_MG_SCAN_COARSE
                if (CS && D.rc_top > 0 && dir > 0 && lvl == D.rc_top && lvl > from && to == last && step > 2 * nramp + 1) {
                    // tolerance mode: the 8193-node level and everything below it in workgroup 0's registers (coarse_resident_cycle).  The
                    // restriction into it runs unfolded -- its source must be complete in global memory, by the group if the level above is shared
                    do_restrict(D, A, lvl, false);
                    if (A.g == 0) {
                        PROF_T0();
                        long nsw = 0;
                        coarse_resident_cycle(D, A, emin, iterno, &nsw);
                        c.sweeps += nsw;
                        PROF_ADD(5, 20);
                    }
                    rc_skip = true;
                    break;
                }
#endif
                if (CS && D.cs_top > 0 && dir > 0 && lvl == D.cs_top && lvl > from && to == last && step > 2 * nramp + 1) {
                    // the rest of this leg and the beginning of the next one (coarse_section)
                    if (A.g == 0) {
                        PROF_T0();
                        long nsw = 0;
                        coarse_section_enter(D, A);
                        __syncthreads();
                        if (threadIdx.x < 64) coarse_section(D, A, emin, iterno, &nsw);
                        if (threadIdx.x == 0) red[17] = static_cast<double>(nsw);
                        __syncthreads();
                        c.sweeps += static_cast<long>(red[17]);
                        coarse_section_leave(D, A);
                        __syncthreads();
                        PROF_ADD(5, 20);
                    }
                    cs_skip = true;
                    break;
                }
                {
                    PROF_T0();
                    if (dir > 0) { if (lvl > from) do_restrict(D, A, lvl, true); }
                    else do_prolong(D, A, lvl + 1, true);
                    PROF_ADD(dir > 0 ? 0 : 1, lvl);
                }
                {
                    PROF_T0();
                    err = do_iterate(D, A, lvl, emin, iterno, red, &c.sweeps);
                    PROF_ADD(2, lvl);
                }
                if (lvl == to) break;
            }
        }
        if (vleg_down) {
            ++c.vcycles;
            if (err < errorMinLast || c.vcycles >= max_vcycles) break;
            // DFTA_POISSON_ADAPTIVE: the cycle stands on its round-off floor (every participant sees the same err)
            if (D.adaptive) {
                if (c.vcycles == 1) err_first = err;
                stalled = (c.vcycles > 1 && err > 0.7 * err_prev && err < 1e-3 * err_first) ? stalled + 1 : 0;
                err_prev = err;
                if (stalled >= 2) break;
            }
        }
    }
    return err;
}

// ==== resident shared levels =======================================================================================
// The grouped solve above stages a shared level from global memory for every visit and writes it back: per V-cycle and
// shared level two copies through the coherent level behind the XCDs' L2s, three exchanges and a full barrier (70 % of a
// single-atom solve was hand-over, DESIGN.md 4.3).  Here a group of kResG member workgroups keeps its stretch of EVERY shared
// level in LDS for the whole solve (node range [m, m+1) * 128 * C_l of level l: 128 lanes x C_l nodes, C_l = 32, 16, 8, 4 at 131073
// nodes), with halo columns: the 115 nodes in front of the stretch (what the fused visit's warm-up reads) and up to ten nodes
// behind it.  A visit is ONE fused pass (gs_lds3) followed by ONE exchange in sentinel-validated slots that carries the three
// partial sums of dPhi^2, the new values of the nodes the neighbours keep in their halos and -- on the way down -- the tail
// of the next level's source, so that restriction and prolongation are local (PoissonSolver.cpp:110-157 on own nodes and
// halos).  One more workgroup per atom, the coarse workgroup, runs the levels below (<= 8193 nodes) with the code above and
// meets the members at the two hand-overs of a cycle, through the global arrays of the first coarse level.
#ifdef DFTA_POISSON_RPROF
__device__ unsigned long long g_rprof[2 * 8 * 8];    // [role][category][level & 7], ticks of member 0 / of the coarse workgroup of atom 0
#define RPROF_T0() const long long rprof_t0 = clock64()
#define RPROF_ADD(cat, lvl) do { if (threadIdx.x == 0) R.prof[(cat) * 8 + ((lvl) & 7)] += clock64() - rprof_t0; } while (0)   /* LDS: a global read-modify-write costs microseconds */
#else
#define RPROF_T0()
#define RPROF_ADD(cat, lvl)
#endif
#ifdef DFTA_MG_RES16
// Second configuration of the resident group (namespace mg_exact16; these shadow poisson_plan.h's constants for everything below): 16
// members of 256 sweeping lanes per atom -- the same 4096 lanes, the same nodes per lane, the same levels and passes -- on 17 compute
// units per atom instead of 33, i.e. up to 15 atoms per launch (the shards of an 8-rank periodic table).  A member's stretch is twice
// as long, and all its shared levels no longer fit its LDS at once (254 KB): level 0 and levels 1 .. kres-1 take TURNS in the same
// memory (kResOverlay).  Level 0 is in LDS from the prolongation into it until the restriction from it; in between its Phi image waits
// in the member's own global scratch (Res::spill, written and read back by the same threads; its source image stays there for the
// whole solve): 67 KB out and 134 KB in per member and V-cycle, ~2 us of a ~240 us cycle.
constexpr int kResNT = 256;
constexpr int kResG = 16;
constexpr int kResWG = kResG + 1;
constexpr bool kResOverlay = true;
#else
constexpr bool kResOverlay = false;
#endif
constexpr int kResHalves = kThreads / kResNT;      // threads per sweeping lane in the transfers (all four waves move data)
// overlay: n2 pairs of doubles between a member's LDS image and its global one, eight loads in flight per thread; pair i is moved by
// thread i mod 256 in both directions (a thread reads back what it wrote itself)
__device__ __forceinline__ void res_copy_pairs(double* __restrict__ dst, const double* __restrict__ src, const int n2, const int tid)
{
    typedef double d2 __attribute__((ext_vector_type(2)));
    d2* __restrict__ d = reinterpret_cast<d2*>(dst);
    const d2* __restrict__ s = reinterpret_cast<const d2*>(src);
    int i = tid;
    for (; i + 7 * kThreads < n2; i += 8 * kThreads) {
        d2 v[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) v[q] = s[i + q * kThreads];
#pragma unroll
        for (int q = 0; q < 8; ++q) d[i + q * kThreads] = v[q];
    }
    for (; i < n2; i += kThreads) d[i] = s[i];
}
template <int LOGC> struct ResLay {
    static constexpr int C = 1 << LOGC;
    static constexpr int H = (kWarm3 + 3 + C - 1) / C;       // halo columns in front of the stretch
    static constexpr int HN = H * C;                         // = nodes in the left halo
    static constexpr int RS = H + kResNT + 1;                // + one column behind it
    static constexpr int N = kResNT * C;                     // own nodes
    // nodes behind the stretch that are kept up to date: what the fused pass reads (3 of Phi, 2 of the source) on the last
    // shared level, and what the restriction of those needs on the levels above it
    static constexpr int NRP = LOGC >= 5 ? 10 : (LOGC == 4 ? 6 : (LOGC == 3 ? 4 : 3));
    static constexpr int NRS = LOGC >= 5 ? 9 : (LOGC == 4 ? 5 : (LOGC == 3 ? 3 : 2));
    static constexpr int doubles = C * RS;
    // node j relative to the member's first node (-HN <= j < N + C) -> index relative to column 0, row 0
    __device__ static __forceinline__ int off(int j) { return (j & (C - 1)) * RS + (j >> LOGC); }
};
static_assert(ResLay<5>::HN <= 128 && ResLay<4>::HN <= 128 && ResLay<3>::HN <= 128 && ResLay<2>::HN <= 128, "payload layout");

struct Res {
    int role;                 // 0: member, 1: the coarse workgroup
    int m;                    // member index
    int kres;                 // shared levels 0 .. kres-1
    int logC0;                // log2(nodes per lane) on level 0
    double* shm;              // the member's LDS
    int pat[kResMaxShared];   // column 0 of level l's Phi array inside it (the source follows C * RS doubles later); read through
    int sat[kResMaxShared];   // res_pp / res_ss with compile-time indices only -- a dynamic index would move the struct to scratch
    double* xs;               // [kResBuf][kResWG][4] sums
    double* xp;               // [kResBuf][kResWG][kResX] payload
    unsigned seq;             // exchanges so far
    bool overlay;             // kResOverlay and kres >= 2: level 0 shares its LDS with levels 1 .. kres-1
    double* spill;            // overlay: [2][C0 * RS0] the member's global images of level 0 (Phi, source), laid out as in LDS
    double* stash;            // overlay: LDS, 128 doubles -- the left halo of level 1's source between the visit of level 0 and the restriction
#ifdef DFTA_POISSON_RPROF
    unsigned long long* prof; // [8][8] ticks per category and level, in LDS
#endif
};

// a value that is the same in every lane (read from LDS after a barrier), moved to scalar registers: what is derived from it --
// the decisions of the cycle -- then stays scalar, and the loops that depend on it keep their state out of the vector registers
__device__ __forceinline__ double res_uniform(const double x)
{
    const long long b = __builtin_bit_cast(long long, x);
    const int lo = __builtin_amdgcn_readfirstlane(static_cast<int>(b));
    const int hi = __builtin_amdgcn_readfirstlane(static_cast<int>(b >> 32));
    return __builtin_bit_cast(double, (static_cast<long long>(hi) << 32) | static_cast<unsigned>(lo));
}
// the lane id behind an optimisation barrier: the per-lane addresses of an operation are computed where it runs.  (Hoisted out of
// the cycle loop -- dozens of inlined operations -- they would be live across everything and spill to scratch memory.)
__device__ __forceinline__ int res_tid()
{
    int t = threadIdx.x;
    asm volatile("" : "+v"(t));
    return t;
}
__device__ __forceinline__ double* res_pp(const Res& R, const int l)
{
    return R.shm + (l == 0 ? R.pat[0] : (l == 1 ? R.pat[1] : (l == 2 ? R.pat[2] : R.pat[3])));
}
__device__ __forceinline__ double* res_ss(const Res& R, const int l)
{
    return R.shm + (l == 0 ? R.sat[0] : (l == 1 ? R.sat[1] : (l == 2 ? R.sat[2] : R.sat[3])));
}
__device__ __forceinline__ void res_store(double* p, double v)
{
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ double* res_mine(const Res& R, int idx)     // slot idx of this participant's payload in the NEXT exchange
{
    return R.xp + ((size_t)(R.seq % kResBuf) * kResWG + (R.role ? kResG : R.m)) * kResX + idx;
}

// One exchange between the kResWG participants of an atom.  Everybody publishes four doubles (members: the partial sums of a
// visit; the coarse workgroup: zeros and, in [3], the number it hands over) and receives their totals (added in a fixed tree
// order, the same for everybody, so that all participants take the same decisions).  Members also receive up to two payload
// values per thread from their neighbours' slots (published before the call with res_store(res_mine())): value v = tid and
// v = tid + 256 with  v < 128: tail of the left neighbour (nt), 128 <= v < 256: source tail of the left neighbour (ns),
// 256 <= v: head of the right neighbour (nh).  want_cb (coarse workgroup): thread 64 + m, m >= 1, receives in cb[] the four
// values around the boundary between members m-1 and m (last node of m-1, first two nodes and first source value of m).
// FENCED: release before publishing, acquire after the last arrival (plain stores / loads of global level storage around it).
template <bool FENCED>
__device__ __forceinline__ void res_exchange(Atom& A, Res& R, const double m0, const double m1, const double m2, const double m3,
                                             const int nt, const int ns, const int nh, const int cb_hn, double* red,
                                             double (&tot)[4], double& r0, double& r1, double (&cb)[4])
{
    const unsigned s = R.seq++;
    const int b = s % kResBuf, tid = res_tid();
    const int me = R.role ? kResG : R.m;
    double* slots = R.xs + (size_t)b * kResWG * 4;
    const double* pay = R.xp + (size_t)b * kResWG * kResX;
    if (tid == 0) {
        if (FENCED) __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        res_store(slots + me * 4 + 0, m0); res_store(slots + me * 4 + 1, m1);
        res_store(slots + me * 4 + 2, m2); res_store(slots + me * 4 + 3, m3);
    }
    const double* p0 = nullptr;
    const double* p1 = nullptr;
    if (R.role == 0) {
        if (tid < 128) { if (R.m > 0 && tid < nt) p0 = pay + (size_t)(R.m - 1) * kResX + tid; }
        else { if (R.m > 0 && tid - 128 < ns) p0 = pay + (size_t)(R.m - 1) * kResX + tid; }
        if (tid < nh && R.m < kResG - 1) p1 = pay + (size_t)(R.m + 1) * kResX + kResXHead + tid;
    }
    const double* pc[4] = {nullptr, nullptr, nullptr, nullptr};
    if (R.role == 1 && cb_hn > 0 && tid > 64 && tid < 64 + kResG) {
        const int m = tid - 64;
        pc[0] = pay + (size_t)(m - 1) * kResX + kResXTail + cb_hn - 1;
        pc[1] = pay + (size_t)m * kResX + kResXHead;
        pc[2] = pay + (size_t)m * kResX + kResXHead + 1;
        pc[3] = pay + (size_t)m * kResX + kResXS0;
    }
    auto ld = [](const double* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); };
    auto is_sent = [](double x) { return static_cast<unsigned long long>(__double_as_longlong(x)) == kFastSentinel; };
    // Up to ten values per thread.  Every round re-issues the loads of ALL values that have not arrived yet together (one round
    // trip per round, not per value); a lost participant must not hang the GPU: after spin_max rounds the group's abort flag is
    // raised (and honoured at once by everybody who sees it), the host repeats the solve with one workgroup per atom.
    const double sentv = __longlong_as_double(static_cast<long long>(kFastSentinel));
    double q[4] = {0, 0, 0, 0}, v0 = 0, v1 = 0, c4[4] = {0, 0, 0, 0};
    const bool sums = tid < kResWG;             // first wave
    const double* pq = slots + (sums ? tid : 0) * 4;
    if (sums) { q[0] = sentv; q[1] = sentv; q[2] = sentv; q[3] = sentv; }
    if (p0) v0 = sentv;
    if (p1) v1 = sentv;
#pragma unroll
    for (int k = 0; k < 4; ++k) if (pc[k]) c4[k] = sentv;
    for (int spins = A.gave_up ? A.spin_max : 0;; ++spins) {
#pragma unroll
        for (int k = 0; k < 4; ++k) if (is_sent(q[k])) q[k] = ld(pq + k);
        if (is_sent(v0)) v0 = ld(p0);
        if (is_sent(v1)) v1 = ld(p1);
#pragma unroll
        for (int k = 0; k < 4; ++k) if (is_sent(c4[k])) c4[k] = ld(pc[k]);
        const bool missing = is_sent(q[0]) || is_sent(q[1]) || is_sent(q[2]) || is_sent(q[3]) || is_sent(v0) || is_sent(v1) ||
                             is_sent(c4[0]) || is_sent(c4[1]) || is_sent(c4[2]) || is_sent(c4[3]);
        if (!missing) break;
        bool give_up = spins > A.spin_max;
        if (!give_up && (spins & 255) == 255) give_up = (__hip_atomic_load(A.ctr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & 0x80000000u) != 0;
        if (give_up) {
            __hip_atomic_fetch_or(A.ctr, 0x80000000u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            A.gave_up = true;
#pragma unroll
            for (int k = 0; k < 4; ++k) { if (is_sent(q[k])) q[k] = 0; if (is_sent(c4[k])) c4[k] = 0; }
            if (is_sent(v0)) v0 = 0;
            if (is_sent(v1)) v1 = 0;
            break;
        }
        __builtin_amdgcn_s_sleep(1);
    }
    if (tid < 64) {
        const double extra = __shfl(q[3], kResG);             // the coarse workgroup's fourth value
        if (tid >= kResG) q[3] = 0;
        q[0] = wave_total(q[0]); q[1] = wave_total(q[1]); q[2] = wave_total(q[2]);
        if (tid == 0) {
            if (FENCED) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            double* bc = red + 20 + (s & 1u) * 4;              // two broadcast areas in turn: no barrier needed before the next exchange writes
            bc[0] = q[0]; bc[1] = q[1]; bc[2] = q[2]; bc[3] = extra;
        }
    }
    __syncthreads();
    {
        const double* bc = red + 20 + (s & 1u) * 4;
        tot[0] = res_uniform(bc[0]); tot[1] = res_uniform(bc[1]); tot[2] = res_uniform(bc[2]); tot[3] = res_uniform(bc[3]);
    }
    // everybody has published exchange s, i.e. is done with every earlier exchange: this participant's part of the buffer that is
    // half a rotation away is reset (by the threads that will store into it again): see kResBuf
    {
        const double sent = __longlong_as_double(static_cast<long long>(kFastSentinel));
        const int bo = (s + kResBuf / 2) % kResBuf;
        if (tid < 4) res_store(R.xs + ((size_t)bo * kResWG + me) * 4 + tid, sent);
        double* mine = R.xp + ((size_t)bo * kResWG + me) * kResX;
        res_store(mine + tid, sent);
        if (tid + 256 < kResX) res_store(mine + tid + 256, sent);
    }
    r0 = v0; r1 = v1;
    cb[0] = c4[0]; cb[1] = c4[1]; cb[2] = c4[2]; cb[3] = c4[3];
}

__device__ __forceinline__ double res_restrict_value(double s0, double pm, double p0, double pq, double dc)
{
    return 4. * (s0 + pm - 2. * p0 + pq) - dc * (pq - pm);     // PoissonSolver.cpp:126-157, the expression of restrict_to
}

// IterateGaussSeidel(l, errorMin, 3) on a shared level by a member.  down: the caller restricts to level l+1 next.
template <int LOGC>
__device__ __forceinline__ double res_visit(const MgDesc& D, Atom& A, Res& R, const int l, const double errorMin, const bool down,
                                            double* red, long* nsweeps)
{
    using Y = ResLay<LOGC>;
    using Yc = ResLay<(LOGC > 2 ? LOGC - 1 : 2)>;
    constexpr int C = Y::C, RS = Y::RS;
    const Lvl L = D.lv[l];
    const double dh = L.d * 0.5;
    const int tid = res_tid();
    double* PP = res_pp(R, l);
    double* SS = res_ss(R, l);
    const bool active = tid < kResNT;
    const int lo_g = (R.m * kResNT + tid) << LOGC;
    const bool lastl = (R.m == kResG - 1) && tid == kResNT - 1;
    const double xN = PP[Y::off(Y::N)];
    const bool careful = R.m == 0 && (__builtin_amdgcn_readfirstlane(lo_g) <= kWarm3);
    const bool to_shared = down && (l + 1 < R.kres);
    const bool to_coarse = down && (l + 1 == R.kres);
    // the old values of the stretch, in case the reference stops after the first or second sweep: parked in the level's (otherwise
    // unused) second global copy -- stores that nobody waits for; a thread reads back only what it wrote itself
    double* __restrict__ park = A.phi1 + L.off + (size_t)R.m * Y::N;
    RPROF_T0();
    if (active) {
#pragma unroll
        for (int k = 0; k < C; ++k) park[k * kResNT + tid] = PP[k * RS + tid];
    }
    double f1 = 0, f2 = 0, f3 = 0;
    if (D.dbg & 2) { f1 = 1; f2 = 1; f3 = 1; }
    else if (careful) gs_lds3<LOGC, RS, kResNT, 3, true>(SS, PP, tid, lo_g, lastl, xN, dh, f1, f2, f3);
    else gs_lds3<LOGC, RS, kResNT, 3, false>(SS, PP, tid, lo_g, lastl, xN, dh, f1, f2, f3);
    if (!active) { f1 = 0; f2 = 0; f3 = 0; }
    f1 = wave_total(f1); f2 = wave_total(f2); f3 = wave_total(f3);
    if ((tid & 63) == 0 && active) { red[tid >> 6] = f1; red[4 + (tid >> 6)] = f2; red[8 + (tid >> 6)] = f3; }
    __syncthreads();                                           // the pass's stores and the waves' partial sums are visible
    // what the neighbours (and, at the hand-over, the coarse workgroup) need of this stretch
    auto publish = [&]() {
        if (tid < Y::HN) res_store(res_mine(R, kResXTail + tid), PP[Y::off(Y::N - Y::HN + tid)]);
        if (tid < Y::NRP) res_store(res_mine(R, kResXHead + tid), PP[Y::off(tid)]);
        if (tid == kResXS0 - 256) res_store(res_mine(R, kResXS0), SS[Y::off(0)]);
        if constexpr (LOGC > 2) {
            if (to_shared && tid >= 128 && tid - 128 < Yc::HN) {
                // the tail of the next level's source: PoissonSolver::Restrict on nodes that lie inside this stretch
                const int jc = Yc::N - Yc::HN + (tid - 128), j = 2 * jc;
                res_store(res_mine(R, kResXSrc + tid - 128),
                          res_restrict_value(SS[Y::off(j)], PP[Y::off(j - 1)], PP[Y::off(j)], PP[Y::off(j + 1)], D.lv[l + 1].d));
            }
        }
        if (to_coarse && active) {
            // the first level of the coarse workgroup: this stretch's part of its source goes to global memory (the exchange
            // that follows is fenced); the node under the boundary to the left neighbour is the coarse workgroup's
            const Lvl Lk = D.lv[l + 1];
#pragma unroll
            for (int k = 0; k < C / 2; ++k) {
                if (tid == 0 && k == 0) continue;
                const int j = 2 * (tid * (C / 2) + k);
                const int ic = (R.m * Y::N) / 2 + tid * (C / 2) + k;
                A.src[Lk.off + addr(Lk, ic)] = res_restrict_value(SS[Y::off(j)], PP[Y::off(j - 1)], PP[Y::off(j)], PP[Y::off(j + 1)], Lk.d);
            }
        }
    };
    RPROF_ADD(0, l);
    { RPROF_T0();
    publish();
    // the hand-over: every thread's plain stores of the coarse level's source must be issued before thread 0's release fence
    // (inside the fenced exchange) -- a workgroup barrier; the other exchanges carry self-validating slots only and need none
    if (to_coarse) __syncthreads();
    RPROF_ADD(1, l); }
    double s1 = (red[0] + red[1]), s2 = (red[4] + red[5]), s3 = (red[8] + red[9]);
    if constexpr (kResNT > 128) { s1 += red[2] + red[3]; s2 += red[6] + red[7]; s3 += red[10] + red[11]; }     // four sweeping waves
    double tot[4], r0, r1, cb[4];
    const int ns = to_shared ? Yc::HN : 0;
    { RPROF_T0();
    if (to_coarse) res_exchange<true>(A, R, s1, s2, s3, 0.0, Y::HN, ns, Y::NRP, 0, red, tot, r0, r1, cb);
    else res_exchange<false>(A, R, s1, s2, s3, 0.0, Y::HN, ns, Y::NRP, 0, red, tot, r0, r1, cb);
    RPROF_ADD(2, l); }
    const double e1 = sqrt(tot[0]), e2 = sqrt(tot[1]), e3 = sqrt(tot[2]);
    const int K = (e1 < errorMin) ? 1 : ((e2 < errorMin) ? 2 : 3);
    if (K < 3) {
        // the reference stops after sweep K: back to the old values (the halos have not been touched yet), the same pass
        // storing sweep K's values, and the exchange once more
        RPROF_T0();
        if (active) {
#pragma unroll
            for (int k = 0; k < C; ++k) PP[k * RS + tid] = park[k * kResNT + tid];
        }
        __syncthreads();
        if (K == 1) gs_lds3<LOGC, RS, kResNT, 1, true>(SS, PP, tid, lo_g, lastl, xN, dh, f1, f2, f3);
        else gs_lds3<LOGC, RS, kResNT, 2, true>(SS, PP, tid, lo_g, lastl, xN, dh, f1, f2, f3);
        __syncthreads();
        publish();
        if (to_coarse) __syncthreads();
        if (to_coarse) res_exchange<true>(A, R, 0.0, 0.0, 0.0, 0.0, Y::HN, ns, Y::NRP, 0, red, tot, r0, r1, cb);
        else res_exchange<false>(A, R, 0.0, 0.0, 0.0, 0.0, Y::HN, ns, Y::NRP, 0, red, tot, r0, r1, cb);
        RPROF_ADD(7, l);
    }
    // the neighbours' new values go into the halos
    { RPROF_T0();
    if (R.m > 0) {
        if (tid < Y::HN) PP[Y::off(-Y::HN + tid)] = r0;
        if constexpr (LOGC > 2) {
            if (to_shared && tid >= 128 && tid - 128 < Yc::HN) {
                if (kResOverlay && R.overlay && l == 0) R.stash[tid - 128] = r0;      // level 1's arrays do not exist yet (res_restrict_local)
                else res_ss(R, l + 1)[Yc::off(-Yc::HN + tid - 128)] = r0;
            }
        }
    }
    if (R.m < kResG - 1 && tid < Y::NRP) PP[Y::off(Y::N + tid)] = r1;
    __syncthreads();
    RPROF_ADD(3, l); }
    *nsweeps += K;
    return K == 1 ? e1 : (K == 2 ? e2 : e3);
}

// The coarse workgroup's part in a member visit: it follows the exchange(s) to take the same decisions; at the hand-over it
// completes the source of its first level (the nodes under the members' boundaries) and marks it for a zero-Phi stage-in.
__device__ __forceinline__ double res_visit_passive(const MgDesc& D, Atom& A, Res& R, const int l, const double errorMin, const bool down,
                                                    double* red, long* nsweeps)
{
    const bool to_coarse = down && (l + 1 == R.kres);
    const int logC = R.logC0 - l;
    const int C = 1 << logC;
    const int hn = ((kWarm3 + 3 + C - 1) / C) * C;
    double tot[4], r0, r1, cb[4];
    RPROF_T0();
    if (to_coarse) res_exchange<true>(A, R, 0.0, 0.0, 0.0, 0.0, 0, 0, 0, hn, red, tot, r0, r1, cb);
    else res_exchange<false>(A, R, 0.0, 0.0, 0.0, 0.0, 0, 0, 0, 0, red, tot, r0, r1, cb);
    RPROF_ADD(0, l);
    const double e1 = sqrt(tot[0]), e2 = sqrt(tot[1]), e3 = sqrt(tot[2]);
    const int K = (e1 < errorMin) ? 1 : ((e2 < errorMin) ? 2 : 3);
    if (K < 3) {
        if (to_coarse) res_exchange<true>(A, R, 0.0, 0.0, 0.0, 0.0, 0, 0, 0, hn, red, tot, r0, r1, cb);
        else res_exchange<false>(A, R, 0.0, 0.0, 0.0, 0.0, 0, 0, 0, 0, red, tot, r0, r1, cb);
    }
    if (to_coarse) {
        const Lvl Lk = D.lv[l + 1];
        const int tid = res_tid();
        const int per = (kResNT << logC) / 2;                  // coarse nodes per member
        if (tid > 64 && tid < 64 + kResG) {
            const int m = tid - 64;
            A.src[Lk.off + addr(Lk, m * per)] = res_restrict_value(cb[3], cb[0], cb[1], cb[2], Lk.d);
        }
        if (tid == 0) { A.src[Lk.off + addr(Lk, 0)] = 0; A.src[Lk.off + addr(Lk, Lk.n - 1)] = 0; }
        A.pend_z = l + 1;
        __syncthreads();
    }
    *nsweeps += 0;      // the members count the sweeps of the shared levels
    return K == 1 ? e1 : (K == 2 ? e2 : e3);
}

// PoissonSolver::Restrict from shared level lc-1 (LOGC nodes per lane) to shared level lc on the member's stretch: own nodes and the
// nodes behind it; the nodes in front of it arrived with the last exchange.  Phi of the coarse level starts from zero everywhere.
template <int LOGC>
__device__ __forceinline__ void res_restrict_local(const MgDesc& D, Res& R, const int lc)
{
    using Yf = ResLay<LOGC>;
    using Yc = ResLay<LOGC - 1>;
    const double* __restrict__ Pf = res_pp(R, lc - 1);
    const double* __restrict__ Sf = res_ss(R, lc - 1);
    double* __restrict__ Pc = res_pp(R, lc);
    double* __restrict__ Sc = res_ss(R, lc);
    const double dc = D.lv[lc].d;
    constexpr int PER = Yc::C / kResHalves;
    const int tid = res_tid(), t = tid & (kResNT - 1), half = tid / kResNT;
    const bool ov = kResOverlay && R.overlay && lc == 1;
    auto value = [&](const int jc) -> double {
        const int j = 2 * jc;
        return res_restrict_value(Sf[Yf::off(j)], Pf[Yf::off(j - 1)], Pf[Yf::off(j)], Pf[Yf::off(j + 1)], dc);
    };
    if (ov) {
        // level 1 is about to take level 0's place: Phi of level 0 goes to the member's global image (its source is there already),
        // the restricted values wait in registers until every thread has read what it needs
        static_assert(Yf::doubles % 2 == 0, "pairs");
        res_copy_pairs(R.spill, Pf - Yf::H, Yf::doubles / 2, tid);
        double sv[PER];
#pragma unroll
        for (int kk = 0; kk < PER; ++kk) {
            const int jc = t * Yc::C + half * PER + kk;
            sv[kk] = (R.m == 0 && jc == 0) ? 0.0 : value(jc);
        }
        double sb = 0;
        if (tid < Yc::NRS && R.m < kResG - 1) sb = value(Yc::N + tid);
        double sh = 0;
        if (tid >= 128 && tid - 128 < Yc::HN && R.m > 0) sh = R.stash[tid - 128];
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < PER; ++kk) {
            const int k = half * PER + kk;
            Sc[k * Yc::RS + t] = sv[kk];
            Pc[k * Yc::RS + t] = 0;
        }
        if (tid < Yc::NRS) Sc[Yc::off(Yc::N + tid)] = sb;
        if (tid >= 128 && tid - 128 < Yc::HN) Sc[Yc::off(-Yc::HN + tid - 128)] = sh;
    } else {
#pragma unroll
        for (int kk = 0; kk < PER; ++kk) {
            const int k = half * PER + kk;
            const int jc = t * Yc::C + k;
            double sv = value(jc);
            if (R.m == 0 && jc == 0) sv = 0;                       // coarse node 0
            Sc[k * Yc::RS + t] = sv;
            Pc[k * Yc::RS + t] = 0;
        }
        // behind the stretch (for the last member only the level's last node: source 0)
        if (tid < Yc::NRS) {
            double sv = 0;
            if (R.m < kResG - 1) sv = value(Yc::N + tid);
            Sc[Yc::off(Yc::N + tid)] = sv;
        }
        // overlay: this level's arrays have held level 0 since the last cycle; the first member's left halo of the source is not
        // written by anybody else (the others' arrived with the exchange of the visit above)
        if (kResOverlay && R.overlay && R.m == 0) for (int i = tid; i < Yc::HN; i += kThreads) Sc[Yc::off(-Yc::HN + i)] = 0;
    }
    if (tid < Yc::C) Pc[Yc::off(Yc::N + tid)] = 0;
    for (int i = tid; i < Yc::HN; i += kThreads) Pc[Yc::off(-Yc::HN + i)] = 0;
    __syncthreads();
}

// PoissonSolver::Prolong (PoissonSolver.cpp:110-123) into shared level lf (LOGC nodes per lane) on the member's stretch and its halos.
// coarse(i): Phi of coarse node i RELATIVE to the member's first coarse node.
template <int LOGC, typename CF>
__device__ __forceinline__ void res_prolong(Res& R, const int lf, CF coarse)
{
    using Y = ResLay<LOGC>;
    double* __restrict__ Pf = res_pp(R, lf);
    constexpr int PER = Y::C / kResHalves;
    const int tid = res_tid(), t = tid & (kResNT - 1), half = tid / kResNT;
    auto corr = [&](int j) -> double {                         // fine node j relative to the stretch
        if ((j & 1) == 0) return coarse(j >> 1);
        return 0.5 * (coarse((j - 1) >> 1) + coarse((j + 1) >> 1));
    };
    if (kResOverlay && R.overlay && lf == 0) {
        // level 0 comes back into the memory level 1 .. kres-1 have used: the corrections wait in registers, the two images return
        // from the member's global scratch (every thread reads back what it wrote itself), then the corrections are added
        static_assert(Y::HN <= kThreads, "one halo node per thread");
        double cv[PER];
#pragma unroll
        for (int kk = 0; kk < PER; ++kk) cv[kk] = corr(t * Y::C + half * PER + kk);
        const double ch = (R.m > 0 && tid < Y::HN) ? corr(-Y::HN + tid) : 0.0;
        const double cb = (tid < Y::NRP && (R.m < kResG - 1 || tid == 0)) ? corr(Y::N + tid) : 0.0;
        __syncthreads();
        res_copy_pairs(Pf - Y::H, R.spill, Y::doubles, tid);
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < PER; ++kk) Pf[(half * PER + kk) * Y::RS + t] += cv[kk];
        if (R.m > 0 && tid < Y::HN) Pf[Y::off(-Y::HN + tid)] += ch;
        if (tid < Y::NRP && (R.m < kResG - 1 || tid == 0)) Pf[Y::off(Y::N + tid)] += cb;
        __syncthreads();
        return;
    }
#pragma unroll 4
    for (int kk = 0; kk < PER; ++kk) {
        const int k = half * PER + kk;
        Pf[k * Y::RS + t] += corr(t * Y::C + k);
    }
    if (R.m > 0) for (int i = tid; i < Y::HN; i += kThreads) Pf[Y::off(-Y::HN + i)] += corr(-Y::HN + i);
    if (tid < Y::NRP && (R.m < kResG - 1 || tid == 0)) Pf[Y::off(Y::N + tid)] += corr(Y::N + tid);
    __syncthreads();
}

// shared levels of a member at the start of a solve (PoissonSolver.h:55-74, PoissonSolver.cpp:80-103): Phi = 0, Source_l[p] =
// 4 Source_{l-1}[2p] = 4^l Source_0[2^l p] (exact scalings) on own nodes and halos, straight from the density
template <int LOGC>
__device__ __forceinline__ void res_init_level(const MgDesc& D, Atom& A, Res& R, const int l, const double* __restrict__ rho,
                                               const double* __restrict__ r, const double* __restrict__ psrc, const int src_all)
{
    using Y = ResLay<LOGC>;
    const bool img = kResOverlay && R.overlay && l == 0;       // level 0 starts in the member's global images (the ramp uses levels 1 .. only)
    double* PP = img ? R.spill + Y::H : res_pp(R, l);
    double* SS = img ? R.spill + Y::doubles + Y::H : res_ss(R, l);
    const int n = D.lv[l].n, N0 = D.lv[0].n;
    const int a = R.m * Y::N;
    const Lvl L0 = D.lv[0];
    for (int idx = threadIdx.x; idx < Y::C * Y::RS; idx += kThreads) {
        const int row = idx / Y::RS, col = idx % Y::RS - Y::H;
        const int i = a + col * Y::C + row;                    // node of level l
        double sv = 0;
        if (l == 0) {
            if (i >= 0 && i < N0) {
                sv = r[i];
                if (src_all || (i > 0 && i < N0 - 1)) sv *= psrc[i] * rho[i];
                // level 0 of the global storage: the source for the unit hooks (dfta_poisson_full_cycle repeats the cycle on it)
                if (col >= 0 && col < kResNT) A.src[L0.off + addr(L0, i)] = sv;
                else if (i == N0 - 1) A.src[L0.off + addr(L0, i)] = sv;
            }
        } else if (i > 0 && i < n - 1) {
            const int i0 = i << l;
            sv = r[i0];
            sv *= psrc[i0] * rho[i0];
            for (int q = 0; q < l; ++q) sv = 4 * sv;
        }
        PP[row * Y::RS + col] = 0;
        SS[row * Y::RS + col] = sv;
    }
}

// the coarse workgroup's levels at the start of a solve
__device__ __forceinline__ void res_init_coarse(const MgDesc& D, Atom& A, const Res& R, const double* __restrict__ rho,
                                                const double* __restrict__ r, const double* __restrict__ psrc, const double lowB, const double highB)
{
    A.cur = 0;
    for (int l = R.kres; l < D.levels; ++l) {
        const Lvl L = D.lv[l];
        for (int idx = threadIdx.x; idx < L.n; idx += kThreads) {
            const int p = node_of(L, idx);
            double sv = 0;
            if (p > 0 && p < L.n - 1) {
                const int i0 = p << l;
                sv = r[i0];
                sv *= psrc[i0] * rho[i0];
                for (int q = 0; q < l; ++q) sv = 4 * sv;
            }
            A.src_of(L)[idx] = sv;
            A.cur_phi(l, L)[idx] = 0;
        }
    }
    __syncthreads();
    const int cl = D.levels - 1;
    if (threadIdx.x == 0) {
        double* Pc = A.cur_phi(cl, D.lv[cl]);
        Pc[addr(D.lv[cl], 0)] = lowB;
        Pc[addr(D.lv[cl], D.lv[cl].n - 1)] = highB;
    }
    __syncthreads();
}

#define DFTA_RES_LEVEL(lc, CALL)                     \
    switch (lc) {                                    \
        case 5: { constexpr int LC = 5; CALL; } break; \
        case 4: { constexpr int LC = 4; CALL; } break; \
        case 3: { constexpr int LC = 3; CALL; } break; \
        default: { constexpr int LC = 2; CALL; } break; \
    }

// PoissonSolver::FullCycle (PoissonSolver.h:89-124) for both roles of a resident group: the leg structure of run_cycles, every
// operation carried out by whoever owns the level (members: levels < kres, coarse workgroup: the others), the two roles meeting
// in the exchanges of the members' visits and at the hand-over from the first coarse level back to the last shared one.
__device__ __forceinline__ double res_cycles(const MgDesc& D, Atom& A, Res& R, const int max_vcycles, const double errorMin,
                                             const double errorMinLast, double* red, Counters& c)
{
    const int last = D.levels - 1, kres = R.kres;
    const int nramp = D.levels - 2 > 0 ? D.levels - 2 : 0;
    const bool coarse = R.role == 1;
    double err = 0;
    bool cs_skip = false, rc_skip = false;
    double err_prev = 0, err_first = 0;
    int stalled = 0;
    for (int step = 0;; ++step) {
        int from, to, iterno = 3;
        double emin = errorMin;
        bool vleg_down = false;
        if (step == 0) { from = to = last; iterno = 15; }
        else if (step <= 2 * nramp) {
            const int q = (step - 1) >> 1;
            const int i = D.levels - 2 - q;
            if ((step - 1) & 1) { from = i; to = last; } else { from = last; to = i; }
        } else if (step == 2 * nramp + 1) { from = last; to = 0; emin = errorMinLast; }
        else {
            emin = errorMinLast;
            if ((step - (2 * nramp + 2)) & 1) { from = last; to = 0; vleg_down = true; } else { from = 0; to = last; }
        }
        const int dir = (from > to) ? -1 : 1;
        err = 1E10;
        if (!(dir < 0 && from == to)) {
            int first_lvl = (dir > 0) ? from : from - 1;
            if (cs_skip) { first_lvl = D.cs_top - 1; cs_skip = false; }
            if (rc_skip) { first_lvl = D.rc_top - 1; rc_skip = false; }
            for (int lvl = first_lvl;; lvl += dir) {
#ifdef DFTA_MG_SCAN_COARSE
                if (D.rc_top > 0 && dir > 0 && lvl == D.rc_top && lvl > from && to == last && step > 2 * nramp + 1) {
                    // tolerance mode: the coarse workgroup's levels in registers, from the first coarse level down and back up
                    if (coarse && !(D.dbg & 1)) {
                        RPROF_T0();
                        long nsw = 0;
#ifdef DFTA_POISSON_RPROF
                        coarse_resident_cycle(D, A, emin, iterno, &nsw, R.prof);
#else
                        coarse_resident_cycle(D, A, emin, iterno, &nsw);
#endif
                        c.sweeps += nsw;
                        RPROF_ADD(3, 0);
                    }
                    rc_skip = true;
                    break;
                }
#endif
                if (D.cs_top > 0 && dir > 0 && lvl == D.cs_top && lvl > from && to == last && step > 2 * nramp + 1) {
                    if (coarse && !(D.dbg & 1)) {
                        RPROF_T0();
                        long nsw = 0;
#ifdef DFTA_POISSON_RPROF
                        { const long long t_e = clock64();
                        coarse_section_enter(D, A);
                        __syncthreads();
                        if (threadIdx.x == 0) R.prof[7 * 8 + 3] += clock64() - t_e; }
                        if (threadIdx.x < 64) coarse_section(D, A, emin, iterno, &nsw, -1, R.prof);
#else
                        coarse_section_enter(D, A);
                        __syncthreads();
                        if (threadIdx.x < 64) coarse_section(D, A, emin, iterno, &nsw);
#endif
                        if (threadIdx.x == 0) red[17] = static_cast<double>(nsw);
                        __syncthreads();
                        c.sweeps += static_cast<long>(res_uniform(red[17]));
#ifdef DFTA_POISSON_RPROF
                        { const long long t_l = clock64();
                        coarse_section_leave(D, A);
                        __syncthreads();
                        if (threadIdx.x == 0) R.prof[7 * 8 + 4] += clock64() - t_l; }
#else
                        coarse_section_leave(D, A);
                        __syncthreads();
#endif
                        RPROF_ADD(3, 0);
                    }
                    cs_skip = true;
                    break;
                }
                // transfer into level lvl
                { RPROF_T0();
                if (dir > 0) {
                    if (lvl > from) {                                          // Restrict(lvl): fine lvl-1 -> coarse lvl
                        if (lvl < kres) { if (!coarse && !(D.dbg & 4)) { DFTA_RES_LEVEL(R.logC0 - (lvl - 1), (res_restrict_local<(LC > 2 ? LC : 3)>(D, R, lvl))) } }
                        else if (lvl > kres) { if (coarse) do_restrict(D, A, lvl, true); }
                        // lvl == kres: the members have written the source during their visit of level kres-1
                    }
                } else {                                                       // Prolong: coarse lvl+1 -> fine lvl
                    if (lvl + 1 < kres) {
                        if (!coarse && !(D.dbg & 4)) {
                            DFTA_RES_LEVEL(R.logC0 - lvl, ({
                                using Yc = ResLay<(LC > 2 ? LC - 1 : 2)>;
                                const double* Pc = res_pp(R, lvl + 1);
                                res_prolong<(LC > 2 ? LC : 3)>(R, lvl, [&](int i) { return Pc[Yc::off(i)]; });
                            }))
                        }
                    } else if (lvl + 1 == kres) {
                        // hand-over: the coarse workgroup has written the first coarse level back to its current global copy
                        double tot[4], r0, r1, cb[4];
                        res_exchange<true>(A, R, 0.0, 0.0, 0.0, coarse ? static_cast<double>((A.cur >> kres) & 1u) : 0.0, 0, 0, 0, 0, red, tot, r0, r1, cb);
                        if (!coarse) {
                            const Lvl Lk = D.lv[kres];
                            const double* __restrict__ Pg = ((tot[3] != 0.0) ? A.phi1 : A.phi0) + Lk.off;
                            DFTA_RES_LEVEL(R.logC0 - lvl, ({
                                using Y = ResLay<LC>;
                                const int a_c = (R.m * Y::N) / 2;
                                const int nck = Lk.n;
                                res_prolong<LC>(R, lvl, [&](int i) { const int ic = a_c + i; return (ic >= 0 && ic < nck) ? Pg[addr(Lk, ic)] : 0.0; });
                            }))
                        }
                    } else if (coarse) do_prolong(D, A, lvl + 1, true);
                }
                RPROF_ADD(dir > 0 ? 4 : ((lvl + 1 == kres) ? 6 : 5), lvl); }
                // IterateGaussSeidel(lvl)
                if (lvl < kres) {
                    const bool down = dir > 0 && lvl < to;
                    if (coarse) err = res_visit_passive(D, A, R, lvl, emin, down, red, &c.sweeps);
                    else { DFTA_RES_LEVEL(R.logC0 - lvl, (err = res_visit<LC>(D, A, R, lvl, emin, down, red, &c.sweeps))) }
                } else if (coarse && !(D.dbg & 1)) {
                    RPROF_T0();
                    err = res_uniform(iterate_gs<false>(D, A, lvl, emin, iterno, red, &c.sweeps));
                    RPROF_ADD(2, lvl - kres);
                }
                if (lvl == to) break;
            }
        }
        if (vleg_down) {
            ++c.vcycles;
            if (err < errorMinLast || c.vcycles >= max_vcycles) break;
            // DFTA_POISSON_ADAPTIVE: the cycle stands on its round-off floor (every participant sees the same err)
            if (D.adaptive) {
                if (c.vcycles == 1) err_first = err;
                stalled = (c.vcycles > 1 && err > 0.7 * err_prev && err < 1e-3 * err_first) ? stalled + 1 : 0;
                err_prev = err;
                if (stalled >= 2) break;
            }
        }
    }
    return err;
}

// SolvePoissonNonUniform (PoissonSolver.h:51-81) by a resident group: kResWG blocks per atom
__global__ __launch_bounds__(kThreads) void k_poisson_solve_res(const MgDesc* __restrict__ Dp, double* __restrict__ phi0, double* __restrict__ phi1,
                                                                double* __restrict__ src, const double* __restrict__ Ne,
                                                                const double* __restrict__ density, const double* __restrict__ r,
                                                                const double* __restrict__ psrc, double* __restrict__ U,
                                                                int* __restrict__ vcycles, double* __restrict__ errs,
                                                                unsigned long long* __restrict__ total_vcycles,
                                                                unsigned* __restrict__ group_ctr, double* __restrict__ res_slots,
                                                                const int* __restrict__ skip, int fault, int src_all,
                                                                double* __restrict__ res_spill)
{
    __shared__ double red[32];
    __shared__ __attribute__((aligned(16))) double shm[3 * kSeqCap + 2 * kStageArr];
    const MgDesc& D = *Dp;
    const int a = blockIdx.x / kResWG, g = blockIdx.x % kResWG;
    if (skip && skip[a]) return;
    if (fault && g == kResG - 1) return;                           // fault injection (tests): this member never arrives
    Atom A;
    A.phi0 = phi0 + (size_t)a * D.per_atom;
    A.phi1 = phi1 + (size_t)a * D.per_atom;
    A.src = src + (size_t)a * D.per_atom;
    A.lds = shm;
    A.stage = shm + 3 * kSeqCap;
    A.cur = 0;
    A.G = 1;                       // the code of the non-shared levels runs in the coarse workgroup alone
    A.g = (g == kResG) ? 0 : 1;
    A.ctr = group_ctr + a;
    A.bar = 0;
    A.part = nullptr; A.fslot = nullptr; A.xchg = nullptr;
    A.fseq = 0;
    A.pend = 0; A.pend_r = 0; A.pend_z = 0;
    A.lds_holds = -1;
    A.spin_max = D.spin_max;
    A.gave_up = false;
    Res R;
    R.role = (g == kResG) ? 1 : 0;
    R.m = g;
    R.kres = D.res_kres;
    R.logC0 = D.res_logC0;
    R.xs = res_slots + (size_t)a * res_slot_doubles();
    R.xp = R.xs + (size_t)kResBuf * kResWG * 4;
    R.seq = 0;
#ifdef DFTA_POISSON_RPROF
    __shared__ unsigned long long prof_acc[64];
    if (threadIdx.x < 64) prof_acc[threadIdx.x] = 0;
    R.prof = prof_acc;
    __syncthreads();
#endif
    R.shm = shm;
    {
        int at = 0, lvl0 = 0;
#pragma unroll
        for (int l = 0; l < kResMaxShared; ++l) {
            const int lc = R.logC0 - l;
            const int C = 1 << (lc > 0 ? lc : 0);
            const int H = (kWarm3 + 3 + C - 1) / C, RS = H + kResNT + 1;
            R.pat[l] = at + H;
            R.sat[l] = at + C * RS + H;
            if (l < R.kres) at += 2 * C * RS;
            if (kResOverlay && R.kres >= 2 && l == 0) { lvl0 = at; at = 0; }       // levels 1 .. share level 0's memory
        }
        // overlay: behind the larger of the two tenants (level 0: 2 C0 RS0 doubles), the stash of 128
        R.overlay = kResOverlay && R.kres >= 2;
        R.stash = shm + (lvl0 > at ? lvl0 : at);
        R.spill = R.overlay ? res_spill + ((size_t)a * kResG + (g < kResG ? g : 0)) * (size_t)lvl0 : nullptr;
    }
    const int N = D.lv[0].n;
    const double* rho = density + (size_t)a * N;
    Counters c{0, 0};
    // level 0 is a member level here (res_kres >= 1, and the planner makes a grid resident from 16385 nodes on): it is never sequential,
    // so its source needs no LDS block; the coarse workgroup's sequential levels get theirs through src_of (res_init_coarse)
    if (R.role == 0) {
        for (int l = 0; l < R.kres; ++l) { DFTA_RES_LEVEL(R.logC0 - l, (res_init_level<LC>(D, A, R, l, rho, r, psrc, src_all))) }
        __syncthreads();
    } else {
        res_init_coarse(D, A, R, rho, r, psrc, 0.0, Ne[a]);     // U(Rmax) = electron count (PoissonSolver.h:76 passes Z: neutral)
    }
    const double err = res_cycles(D, A, R, 100, 1E-3, 1E-14, red, c);      // FullCycle(1E-3, 1E-14), PoissonSolver.h:78
    if (R.role == 0) {
        // U = PhiLevels[0] (PoissonSolver.h:80); also into level 0 of the global storage (copy 0) for the unit hooks
        const Lvl L0 = D.lv[0];
        DFTA_RES_LEVEL(R.logC0, ({
            using Y = ResLay<LC>;
            const double* P = res_pp(R, 0);
            const int a0 = R.m * Y::N;
            for (int j = threadIdx.x; j < Y::N; j += kThreads) {
                const double v = P[Y::off(j)];
                U[(size_t)a * N + a0 + j] = v;
                A.phi0[L0.off + addr(L0, a0 + j)] = v;
            }
            if (R.m == kResG - 1 && threadIdx.x == 0) {
                const double v = P[Y::off(Y::N)];
                U[(size_t)a * N + N - 1] = v;
                A.phi0[L0.off + addr(L0, N - 1)] = v;
            }
        }))
    } else if (threadIdx.x == 0) {
        if (vcycles) vcycles[a] = (int)c.vcycles;
        if (errs) errs[a] = err;
        if (total_vcycles) atomicAdd(total_vcycles, (unsigned long long)c.vcycles);
    }
#ifdef DFTA_POISSON_RPROF
    __syncthreads();
    if (a == 0 && (R.role == 1 || R.m == 0) && threadIdx.x < 64) g_rprof[R.role * 64 + threadIdx.x] += prof_acc[threadIdx.x];
#endif
}

#ifndef DFTA_MG_RES16
// SolvePoissonNonUniform (PoissonSolver.h:51-81): one block per atom
__global__ __launch_bounds__(kThreads) void k_poisson_solve(const MgDesc* __restrict__ Dp, double* __restrict__ phi0, double* __restrict__ phi1,
                                                            double* __restrict__ src, const double* __restrict__ Ne,
                                                            const double* __restrict__ density, const double* __restrict__ r,
                                                            const double* __restrict__ psrc, double* __restrict__ U,
                                                            int* __restrict__ vcycles, double* __restrict__ errs,
                                                            unsigned long long* __restrict__ total_vcycles,
                                                            unsigned* __restrict__ group_ctr, double* __restrict__ group_part,
                                                            const int* __restrict__ skip, int fault, int src_all)
{
    __shared__ double red[20];
    __shared__ double seqmem[3 * kSeqCap];
    __shared__ double stagemem[2 * kStageArr];
    const MgDesc& D = *Dp;
    // consecutive blocks are the members of one group (they land on different XCDs, where the barrier is cheapest)
    const int a = blockIdx.x >> D.logG;
    if (skip && skip[a]) return;                                  // a frozen atom of the batch (finished SCF): U stays as it is
    if (fault && D.G > 1 && (blockIdx.x & (D.G - 1)) == D.G - 1) return;   // fault injection (tests): this member never arrives
    Atom A;
    A.phi0 = phi0 + (size_t)a * D.per_atom;
    A.phi1 = phi1 + (size_t)a * D.per_atom;
    A.src = src + (size_t)a * D.per_atom;
    A.lds = seqmem;
    A.stage = stagemem;
    A.cur = 0;
    A.G = D.G;
    A.g = blockIdx.x & (D.G - 1);
    A.ctr = group_ctr + a;
    A.bar = 0;
    A.part = group_part + (size_t)a * group_part_doubles(D.G);
    A.fslot = A.part + 6 * D.G + 2;
    A.xchg = A.part + (6 + kGrpBuf) * D.G + 2;
    A.fseq = 0;
    A.pend = 0;
    A.pend_r = 0;
    A.pend_z = 0;
    A.lds_holds = -1;
    A.spin_max = D.spin_max;
    A.gave_up = false;
    const Lvl L0 = D.lv[0];
    const int N = L0.n;
    const double* rho = density + (size_t)a * N;
    const bool coop0 = D.kcoop > 0;        // level 0 is shared by the group
    // source: Source[i] = r_i; Source[i] *= (4 pi Rp^2 delta^2) exp(2 i delta) * density[i], 1 <= i <= N-2
    if (coop0 || A.g == 0)
    for (int idx = coop0 ? A.lane() : static_cast<int>(threadIdx.x); idx < N; idx += coop0 ? kThreads * A.G : kThreads) {
        const int i = node_of(L0, idx);
        double s = r[i];
        if (src_all || (i > 0 && i < N - 1)) s *= psrc[i] * rho[i];      // PoissonSolver.h:72-74; uniform grid: every node (PoissonSolver.h:39-40)
        A.src[L0.off + idx] = s;   // global storage: what the chunked sweeps, the unit entries and dfta_poisson_get_level read
        // grids of <= 65 nodes (3 .. 6 levels): level 0 is sequential too, and initialize() and the sweeps read a sequential
        // level's source from its LDS block (src_of) -- nothing else fills that block in this kernel
        if (L0.seq) A.src_of(L0)[idx] = s;
    }
    __syncthreads();
    Counters c{0, 0};
    PROF_T0();
    initialize(D, A, 0.0, Ne[a]);                                  // U(Rmax) = electron count (PoissonSolver.h:76 passes Z: neutral)
    const double err = run_cycles<true>(D, A, 0, 100, 1E-3, 1E-14, red, c);      // FullCycle(1E-3, 1E-14), PoissonSolver.h:78
    PROF_ADD(5, 21);
    const double* __restrict__ P = A.cur_phi(0, L0);
    if (coop0 || A.g == 0)
        for (int i = coop0 ? A.lane() : static_cast<int>(threadIdx.x); i < N; i += coop0 ? kThreads * A.G : kThreads)
            U[(size_t)a * N + i] = P[addr(L0, i)];
    if (threadIdx.x == 0 && A.g == 0) {
        if (vcycles) vcycles[a] = (int)c.vcycles;
        if (errs) errs[a] = err;
        if (total_vcycles) atomicAdd(total_vcycles, (unsigned long long)c.vcycles);
    }
}

// unit-parity kernels on atom 0 ------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void k_unit(const MgDesc* __restrict__ Dp, double* phi0, double* phi1, double* src, int* cur, int op,
                                                   int lvl, int sweeps, double* out, unsigned* group_ctr, double* group_part)
{
    __shared__ double red[20];
    __shared__ double seqmem[3 * kSeqCap];
    __shared__ double stagemem[2 * kStageArr];
    const MgDesc& D = *Dp;
    Atom A;
    A.phi0 = phi0; A.phi1 = phi1; A.src = src; A.lds = seqmem;
    A.stage = stagemem;
    A.G = D.G;
    A.g = blockIdx.x;
    A.ctr = group_ctr;
    A.bar = 0;
    A.part = group_part;
    A.fslot = A.part + 6 * D.G + 2;
    A.xchg = A.part + (6 + kGrpBuf) * D.G + 2;
    A.fseq = 0;
    A.pend = 0;
    A.pend_r = 0;
    A.pend_z = 0;
    A.lds_holds = -1;
    A.spin_max = D.spin_max;
    A.gave_up = false;
    A.cur = 0;
    for (int l = 0; l < D.levels; ++l) A.cur |= (cur[l] ? 1u : 0u) << l;
    // sequential levels: global -> LDS (the solve kernel initialises them itself); they are workgroup 0's
    for (int l = 0; l < D.levels && A.g == 0; ++l) {
        const Lvl L = D.lv[l];
        if (!L.seq) continue;
        for (int idx = threadIdx.x; idx < L.n; idx += kThreads) {
            seqmem[L.soff + idx] = phi0[L.off + idx];
            seqmem[kSeqCap + L.soff + idx] = phi1[L.off + idx];
            seqmem[2 * kSeqCap + L.soff + idx] = src[L.off + idx];
        }
    }
    __syncthreads();
    Counters c{0, 0};
    const bool lead = A.g == 0;
    if (op == 0) {
        if (lvl < D.kcoop || lead)
            for (int s = 0; s < sweeps; ++s) {
                const double e = gauss_seidel(D, A, lvl, red);
                if (threadIdx.x == 0 && lead) out[s] = e;
            }
    } else if (op == 1) do_restrict(D, A, lvl);
    else if (op == 2) do_prolong(D, A, lvl);
    else if (op == 4) {                                   // IterateGaussSeidel(lvl, errorMin = out[0], iterno = sweeps)
        const double emin = out[0];
        group_sync(A);                                    // everybody has read out[0]
        const double e = do_iterate(D, A, lvl, emin, sweeps, red, &c.sweeps);
        if (threadIdx.x == 0 && lead) { out[0] = e; out[1] = (double)c.sweeps; }
    }
    else if (op == 5) {                                   // FullCycle(errorMin = out[0], errorMinLast = out[1]) with boundaries out[2], out[3]
        const double e1 = out[0], e2 = out[1], lowB = out[2], highB = out[3];
        group_sync(A);                                    // everybody has read out[]
        initialize(D, A, lowB, highB);
        const double e = run_cycles<true>(D, A, 0, 100, e1, e2, red, c);
        if (threadIdx.x == 0 && lead) { out[0] = e; out[1] = (double)c.vcycles; }
    }
    else if (op == 3) {
        const int nramp = D.levels - 2 > 0 ? D.levels - 2 : 0;
        const double e = run_cycles<false>(D, A, 2 * nramp + 2, 1, 1E-14, 1E-14, red, c);   // one VCycle(last, 1E-14, 3)
        if (threadIdx.x == 0 && lead) out[0] = e;
    }
    __syncthreads();
    for (int l = 0; l < D.levels && lead; ++l) {
        const Lvl L = D.lv[l];
        if (!L.seq) continue;
        for (int idx = threadIdx.x; idx < L.n; idx += kThreads) {
            phi0[L.off + idx] = seqmem[L.soff + idx];
            phi1[L.off + idx] = seqmem[kSeqCap + L.soff + idx];
            src[L.off + idx] = seqmem[2 * kSeqCap + L.soff + idx];
        }
    }
    if (threadIdx.x == 0 && lead) for (int l = 0; l < D.levels; ++l) cur[l] = (A.cur >> l) & 1u;
}


#endif   // DFTA_MG_RES16: the resident kernel alone
