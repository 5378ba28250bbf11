// numerov_api.cpp -- the C ABI of the Numerov layer (include/dftatom_hip.h): the per-call entries dfta_numerov_sweeps / _sweeps_dev /
// _match and the potential resident on the device, dfta_potential_*.  Host code only: what runs on the device is launched through the
// dfta_launch_* helpers of numerov.hip (internal.h); grouping, host boundary values and the staging layout are numerov_host.cpp's.
//
// Every entry is the same sequence -- validate, group the trials by (potential, l), sort them through Grouping::order and take their
// boundary values (host: libm, as the reference; device: a launch), build or reuse the slots' tables, launch, download, scatter the
// results back through the order -- written once below (fill_sorted, CallTables, call_boundary, scatter_sweeps).  What an entry accepts
// and rejects is its own and stays in the entry.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <memory>
#include <vector>

#include "internal.h"
#include "numerov_host.h"

namespace {

using dfta_nh::Grouping;
using dfta_nh::StageLayout;
using dfta_nh::stage_ptr;

dfta_nh::GridView grid_view(const dfta_grid* g)
{
    dfta_nh::GridView v;
    v.N = g->N; v.uniform = g->uniform; v.delta = g->delta; v.Rmax = g->Rmax; v.h = g->h; v.r = g->h_r.data();
    return v;
}

template <typename T>
hipError_t upload(DevBuf<T>& d, const std::vector<T>& h, hipStream_t s)
{
    hipError_t e = d.alloc(h.size());
    if (e != hipSuccess || h.empty()) return e;
    return hipMemcpyAsync(d.p, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice, s);
}

// host arrays of n trials in launch order (vectors of a per-call entry, or the staging block of a resident potential)
struct HostTrials {
    double *E, *us, *us1;
    double* uz;                    // match only (null: none); 0 where the grid has no start value at the origin
    int* start;
    int *limit, *l;                // null: not wanted
};
// sorted trial s = the caller's trial order[s] (null: s); host_bv: the boundary values as the reference's libm gives them
void fill_sorted(const int* order, int n, const dfta_grid* g, const double* E, const int* l, const int* nodesLimit, bool host_bv, bool for_match,
                 const HostTrials& h)
{
    const dfta_nh::GridView gv = grid_view(g);
    for (int s = 0; s < n; ++s) {
        const int t = order ? order[s] : s;
        h.E[s] = E[t];
        if (h.limit) h.limit[s] = nodesLimit ? nodesLimit[t] : 0;
        if (h.l) h.l[s] = l[t];
        if (h.uz) h.uz[s] = 0;
        if (host_bv) dfta_nh::host_boundary_of(gv, E[t], l[t], for_match, &h.start[s], &h.us[s], &h.us1[s], h.uz ? &h.uz[s] : nullptr);
    }
}

// results of n sorted sweeps back to the caller's order (count only for COUNT; any output may be null)
void scatter_sweeps(const int* order, int n, int kind, const int* count, const double* u0, const int* start, const int* trip,
                    int* count_out, double* u0_out, int* start_out, int* trip_out)
{
    for (int s = 0; s < n; ++s) {
        const int t = order ? order[s] : s;
        if (count_out && kind == DFTA_SWEEP_COUNT) count_out[t] = count[s];
        if (u0_out) u0_out[t] = u0[s];
        if (start_out) start_out[t] = start[s];
        if (trip_out) trip_out[t] = trip[s];
    }
}

// per-call entries: the slots' tables and the blocks of ONE call, uploaded from its grouping and built from the potentials dV
struct CallTables {
    DevBuf<int> slot_v, slot_l, blk_slot, blk_first, blk_cnt, trial_slot;
    DevBuf<double2> tab, bounds;
    int nslots = 0, nblocks = 0;
    int upload_grouping(dfta_ctx* ctx, const dfta_grid* g, const Grouping& G, bool for_match)
    {
        hipStream_t st = ctx->stream;
        nslots = (int)G.slot_v.size(); nblocks = (int)G.blk_slot.size();
        DFTA_HIP(ctx, upload(slot_v, G.slot_v, st));
        DFTA_HIP(ctx, upload(slot_l, G.slot_l, st));
        if (for_match) DFTA_HIP(ctx, upload(trial_slot, G.trial_slot, st));      // a match solve is one workgroup per trial: no blocks
        else {
            DFTA_HIP(ctx, upload(blk_slot, G.blk_slot, st));
            DFTA_HIP(ctx, upload(blk_first, G.blk_first, st));
            DFTA_HIP(ctx, upload(blk_cnt, G.blk_cnt, st));
        }
        DFTA_HIP(ctx, tab.alloc((size_t)nslots * g->N));
        DFTA_HIP(ctx, bounds.alloc((size_t)nslots * dfta_bounds_stride(g)));
        return DFTA_OK;
    }
    int build(dfta_ctx* ctx, const dfta_grid* g, const double* dV) { return dfta_launch_build_tab(ctx, g, tab, dV, slot_v, slot_l, nslots, bounds); }
    SlotTables tables() const
    {
        SlotTables t;
        t.tab = tab; t.bounds = bounds; t.slot_l = slot_l;
        return t;
    }
    WaveBlocks blocks() const
    {
        WaveBlocks b;
        b.slot = blk_slot; b.first = blk_first; b.cnt = blk_cnt; b.kind = nullptr; b.n = nblocks;
        return b;
    }
};

// per-call entries: the boundary values of n trials on the device -- uploaded from the host's (h non-null) or launched
struct CallBoundary {
    DevBuf<int> start;
    DevBuf<double> us, us1, uz;
};
int call_boundary(dfta_ctx* ctx, const dfta_grid* g, int n, const double* dE, const int* dL, bool for_match, const HostTrials* h, CallBoundary& b)
{
    hipStream_t st = ctx->stream;
    DFTA_HIP(ctx, b.start.alloc(n));
    DFTA_HIP(ctx, b.us.alloc(n));
    DFTA_HIP(ctx, b.us1.alloc(n));
    if (for_match) DFTA_HIP(ctx, b.uz.alloc(n));
    if (h) {
        DFTA_HIP(ctx, hipMemcpyAsync(b.start.p, h->start, sizeof(int) * n, hipMemcpyHostToDevice, st));
        DFTA_HIP(ctx, hipMemcpyAsync(b.us.p, h->us, sizeof(double) * n, hipMemcpyHostToDevice, st));
        DFTA_HIP(ctx, hipMemcpyAsync(b.us1.p, h->us1, sizeof(double) * n, hipMemcpyHostToDevice, st));
        if (for_match) DFTA_HIP(ctx, hipMemcpyAsync(b.uz.p, h->uz, sizeof(double) * n, hipMemcpyHostToDevice, st));
        return DFTA_OK;
    }
    BoundaryTrials t;
    t.E = dE; t.n = n; t.start = b.start; t.us = b.us; t.us1 = b.us1;
    t.for_match = for_match ? 1 : 0; t.l = for_match ? dL : nullptr; t.uz = for_match ? b.uz.p : nullptr;
    return dfta_launch_boundary(ctx, g, t, nullptr);
}

}  // namespace

extern "C" int dfta_numerov_sweeps(dfta_ctx* ctx, const dfta_grid* g, int kind, int boundary, int nV, const double* V,
                                   int ntrials, const int* vidx, const int* l, const double* E, const int* nodesLimit,
                                   int* count_out, double* u0_out, int* start_out, int* trip_out)
{
    if (!ctx || !g) return DFTA_ERR_INVALID;
    DFTA_ENTER(ctx);
    DFTA_REQUIRE(ctx, ntrials >= 0, "negative trial count");
    if (ntrials == 0) return DFTA_OK;                       // empty batch
    DFTA_REQUIRE(ctx, V && l && E && nV > 0, "null input");
    DFTA_REQUIRE(ctx, kind == DFTA_SWEEP_COUNT || kind == DFTA_SWEEP_ZERO, "kind");
    DFTA_REQUIRE(ctx, kind != DFTA_SWEEP_COUNT || (nodesLimit && count_out), "COUNT needs nodesLimit and count_out");
    DFTA_REQUIRE(ctx, kind != DFTA_SWEEP_ZERO || u0_out, "ZERO needs u0_out");
    if (kind == DFTA_SWEEP_COUNT)      // (this entry alone checks the range of the limits: dfta_potential_sweeps takes them as they come)
        for (int t = 0; t < ntrials; ++t) DFTA_REQUIRE(ctx, nodesLimit[t] >= 0 && nodesLimit[t] < (1 << 30), "nodesLimit out of range");
    const int N = g->N;
    Grouping G;
    if (dfta_nh::make_grouping(ntrials, vidx, l, nV, G) != DFTA_OK) { snprintf(ctx->err, sizeof(ctx->err), "invalid vidx/l"); return DFTA_ERR_INVALID; }
    const bool host_bv = boundary == DFTA_BOUNDARY_HOST;
    std::vector<double> sE(ntrials), sUs(ntrials), sUs1(ntrials);
    std::vector<int> sLim(ntrials), sStart(ntrials);
    HostTrials h;
    h.E = sE.data(); h.us = sUs.data(); h.us1 = sUs1.data(); h.uz = nullptr; h.start = sStart.data(); h.limit = sLim.data(); h.l = nullptr;
    fill_sorted(G.order.data(), ntrials, g, E, l, nodesLimit, host_bv, false, h);

    hipStream_t st = ctx->stream;
    DevBuf<double> dV, dE, dU0;
    DevBuf<int> dLim, dCount, dTrip;
    CallTables tb;
    CallBoundary bv;
    DFTA_HIP(ctx, dV.alloc((size_t)nV * N));
    DFTA_HIP(ctx, hipMemcpyAsync(dV.p, V, (size_t)nV * N * sizeof(double), hipMemcpyHostToDevice, st));
    DFTA_HIP(ctx, upload(dE, sE, st));
    DFTA_HIP(ctx, upload(dLim, sLim, st));
    int rc = tb.upload_grouping(ctx, g, G, false);
    if (rc) return rc;
    DFTA_HIP(ctx, dCount.alloc(ntrials));
    DFTA_HIP(ctx, dTrip.alloc(ntrials));
    DFTA_HIP(ctx, dU0.alloc(ntrials));
    rc = call_boundary(ctx, g, ntrials, dE, nullptr, false, host_bv ? &h : nullptr, bv);
    if (!rc) rc = tb.build(ctx, g, dV);
    if (rc) return rc;
    SweepTrials tr{};
    tr.E = dE; tr.limit = dLim; tr.start = bv.start; tr.us = bv.us; tr.us1 = bv.us1;
    tr.count = dCount; tr.u0 = dU0; tr.trip = dTrip;
    DFTA_HIP(ctx, dfta_timer_start(ctx));
    rc = dfta_launch_sweep(ctx, g, kind, tb.tables(), tb.blocks(), tr, nullptr, nullptr, 0);
    if (rc) return rc;
    DFTA_HIP(ctx, dfta_timer_stop(ctx));
    std::vector<int> hCount(ntrials), hTrip(ntrials), hStart(ntrials);
    std::vector<double> hU0(ntrials);
    DFTA_HIP(ctx, hipMemcpyAsync(hCount.data(), dCount.p, ntrials * sizeof(int), hipMemcpyDeviceToHost, st));
    DFTA_HIP(ctx, hipMemcpyAsync(hTrip.data(), dTrip.p, ntrials * sizeof(int), hipMemcpyDeviceToHost, st));
    DFTA_HIP(ctx, hipMemcpyAsync(hStart.data(), bv.start.p, ntrials * sizeof(int), hipMemcpyDeviceToHost, st));
    DFTA_HIP(ctx, hipMemcpyAsync(hU0.data(), dU0.p, ntrials * sizeof(double), hipMemcpyDeviceToHost, st));
    DFTA_HIP(ctx, hipStreamSynchronize(st));
    scatter_sweeps(G.order.data(), ntrials, kind, hCount.data(), hU0.data(), hStart.data(), hTrip.data(), count_out, u0_out, start_out, trip_out);
    return DFTA_OK;
}

// (device pointers in, device pointers out: the caller's trials are grouped and in launch order already -- nothing is sorted or
// scattered, and neither `kind` nor the trial count is checked here)
extern "C" int dfta_numerov_sweeps_dev(dfta_ctx* ctx, const dfta_grid* g, int kind, int nV, const double* dV, int ngroups,
                                       const int* group_off, const int* group_vidx, const int* group_l, const double* dE,
                                       const int* dLimit, const int* dStart, const double* dUs, const double* dUs1,
                                       int* dCount, double* dU0, int* dStartOut, int* dTrip)
{
    if (!ctx || !g) return DFTA_ERR_INVALID;
    DFTA_ENTER(ctx);
    DFTA_REQUIRE(ctx, dV && group_off && group_vidx && group_l && dE && ngroups > 0, "null input");
    const int ntrials = group_off[ngroups];
    Grouping G;
    DFTA_REQUIRE(ctx, dfta_nh::make_grouping_of_groups(ngroups, group_off, group_vidx, group_l, nV, G) == DFTA_OK, "group vidx/l");
    hipStream_t st = ctx->stream;
    CallTables tb;
    CallBoundary bv;
    int rc = tb.upload_grouping(ctx, g, G, false);
    if (rc) return rc;
    SweepTrials tr{};
    tr.E = dE; tr.limit = dLimit; tr.start = dStart; tr.us = dUs; tr.us1 = dUs1;
    tr.count = dCount; tr.u0 = dU0; tr.trip = dTrip;
    if (!dStart || !dUs || !dUs1) {
        rc = call_boundary(ctx, g, ntrials, dE, nullptr, false, nullptr, bv);
        if (rc) return rc;
        tr.start = bv.start; tr.us = bv.us; tr.us1 = bv.us1;
    }
    rc = tb.build(ctx, g, dV);
    if (!rc) rc = dfta_launch_sweep(ctx, g, kind, tb.tables(), tb.blocks(), tr, nullptr, nullptr, 0);
    if (rc) return rc;
    if (dStartOut) DFTA_HIP(ctx, hipMemcpyAsync(dStartOut, tr.start, ntrials * sizeof(int), hipMemcpyDeviceToDevice, st));
    DFTA_HIP(ctx, hipStreamSynchronize(st));   // scratch buffers die with this scope
    return DFTA_OK;
}

extern "C" int dfta_numerov_match(dfta_ctx* ctx, const dfta_grid* g, int boundary, int nV, const double* V, int ntrials,
                                  const int* vidx, const int* l, const double* E, double* Psi_out, long* matchPoint_out)
{
    if (!ctx || !g) return DFTA_ERR_INVALID;
    DFTA_ENTER(ctx);
    DFTA_REQUIRE(ctx, V && l && E && Psi_out && matchPoint_out && nV > 0 && ntrials >= 0, "null input");      // (null inputs are refused before the empty batch is accepted: unlike dfta_numerov_sweeps)
    if (ntrials == 0) return DFTA_OK;
    const int N = g->N;
    Grouping G;
    if (dfta_nh::make_grouping(ntrials, vidx, l, nV, G) != DFTA_OK) { snprintf(ctx->err, sizeof(ctx->err), "invalid vidx/l"); return DFTA_ERR_INVALID; }
    const bool host_bv = boundary == DFTA_BOUNDARY_HOST;
    std::vector<double> sE(ntrials), sUs(ntrials), sUs1(ntrials), sUz(ntrials);
    std::vector<int> sStart(ntrials), sL(ntrials);
    HostTrials h;
    h.E = sE.data(); h.us = sUs.data(); h.us1 = sUs1.data(); h.uz = sUz.data(); h.start = sStart.data(); h.limit = nullptr; h.l = sL.data();
    fill_sorted(G.order.data(), ntrials, g, E, l, nullptr, host_bv, true, h);

    hipStream_t st = ctx->stream;
    DevBuf<double> dV, dE, dPsi, dQ;
    DevBuf<int> dL, dMp;
    CallTables tb;
    CallBoundary bv;
    DFTA_HIP(ctx, dV.alloc((size_t)nV * N));
    DFTA_HIP(ctx, hipMemcpyAsync(dV.p, V, (size_t)nV * N * sizeof(double), hipMemcpyHostToDevice, st));
    DFTA_HIP(ctx, upload(dE, sE, st));
    DFTA_HIP(ctx, upload(dL, sL, st));
    int rc = tb.upload_grouping(ctx, g, G, true);
    if (rc) return rc;
    DFTA_HIP(ctx, dPsi.alloc((size_t)ntrials * N));
    DFTA_HIP(ctx, dQ.alloc((size_t)ntrials * N));
    DFTA_HIP(ctx, dMp.alloc(ntrials));
    rc = call_boundary(ctx, g, ntrials, dE, dL, true, host_bv ? &h : nullptr, bv);
    if (!rc) rc = tb.build(ctx, g, dV);
    if (rc) return rc;
    SlotTables tables = tb.tables();
    if (g->uniform) tables.bounds = nullptr;
    MatchTrials mt;
    mt.slot = tb.trial_slot; mt.E = dE; mt.start = bv.start; mt.us = bv.us; mt.us1 = bv.us1; mt.l = dL; mt.uz = bv.uz;
    mt.Psi = dPsi; mt.Q = dQ; mt.match_point = dMp; mt.n = ntrials;
    rc = dfta_launch_match(ctx, g, tables, mt, nullptr);
    if (rc) return rc;
    std::vector<double> hPsi((size_t)ntrials * N);
    std::vector<int> hMp(ntrials);
    DFTA_HIP(ctx, hipMemcpyAsync(hPsi.data(), dPsi.p, hPsi.size() * sizeof(double), hipMemcpyDeviceToHost, st));
    DFTA_HIP(ctx, hipMemcpyAsync(hMp.data(), dMp.p, ntrials * sizeof(int), hipMemcpyDeviceToHost, st));
    DFTA_HIP(ctx, hipStreamSynchronize(st));
    for (int s = 0; s < ntrials; ++s) {
        const int t = G.order[s];
        memcpy(Psi_out + (size_t)t * N, hPsi.data() + (size_t)s * N, sizeof(double) * N);
        matchPoint_out[t] = hMp[s];
    }
    return DFTA_OK;
}

// ---- a potential resident on the device (include/dftatom_hip.h: dfta_potential) -------------------------------------------------
// The reference's Numerov holds a REFERENCE to the caller's Potential and re-reads it on every call (Numerov.h:69,186); its L3 makes
// ~2100 calls on one Numerov object per SCF step.  dfta_numerov_sweeps re-uploads the 1 MB potential and rebuilds the slot table on each
// of them (0.8 ... 6 ms per call); here both are done once per potential, and a call costs its sweep.
// Differences to the per-call entries: ONE potential (no vidx), the boundary values always from the host, the table slot of a trial is
// its l (four slots, built once), and the trials travel in one staging block each way (numerov_host.h: StageLayout).
struct dfta_potential {
    dfta_ctx* ctx = nullptr;
    const dfta_grid* g = nullptr;
    std::vector<double> h_V;
    DevBuf<double> dV;
    DevBuf<double2> dTab;           // 4 slots: l = 0..3
    DevBuf<double2> dBounds;
    DevBuf<int> dSlots;             // slot_v (4 zeros), slot_l (0..3)
    dfta_scan_tables scan;          // tolerance mode: built on first use
    bool scan_built = false;
    // per-call scratch, grown on demand: one staging block in, one out
    size_t cap = 0;
    DevBuf<char> dIn, dOut;
    std::vector<char> hIn, hOut;
    DevBuf<double> dPsi, dQ;
    size_t psi_cap = 0;
    SlotTables tables() const
    {
        SlotTables t;
        t.tab = dTab; t.bounds = dBounds; t.slot_l = dSlots + 4;
        return t;
    }
};

namespace {
int potential_build(dfta_potential* p)
{
    dfta_ctx* ctx = p->ctx;
    const int N = p->g->N;
    DFTA_HIP(ctx, hipMemcpyAsync(p->dV, p->h_V.data(), sizeof(double) * N, hipMemcpyHostToDevice, ctx->stream));
    int rc = dfta_launch_build_tab(ctx, p->g, p->dTab, p->dV, p->dSlots, p->dSlots + 4, 4, p->dBounds);
    if (rc) return rc;
    if (p->scan_built) rc = dfta_launch_scan_build_tab(ctx, p->g, p->scan, p->dV, p->dSlots, p->dSlots + 4);
    return rc;
}
int potential_scratch(dfta_potential* p, int ntrials)
{
    dfta_ctx* ctx = p->ctx;
    const size_t need = dfta_nh::stage_scratch_bytes(ntrials);
    if (need <= p->cap) return DFTA_OK;
    p->dIn.reset(); p->dOut.reset(); p->cap = 0;
    DFTA_HIP(ctx, p->dIn.alloc(need));
    DFTA_HIP(ctx, p->dOut.alloc(need));
    p->hIn.resize(need); p->hOut.resize(need);
    p->cap = need;
    return DFTA_OK;
}
int potential_stage_in(dfta_potential* p, const StageLayout& L)
{
    DFTA_HIP(p->ctx, hipMemcpyAsync(p->dIn, p->hIn.data(), L.in_bytes, hipMemcpyHostToDevice, p->ctx->stream));
    return DFTA_OK;
}
// the out-block back to the host, and the results of n sweeps from it to the caller's order; *anybad: a trial the scan could not decide
int potential_stage_out(dfta_potential* p, const StageLayout& L, const int* order, int n, int kind, const int* start, int* count_out,
                        double* u0_out, int* start_out, int* trip_out, bool* anybad)
{
    dfta_ctx* ctx = p->ctx;
    DFTA_HIP(ctx, hipMemcpyAsync(p->hOut.data(), p->dOut, L.out_bytes, hipMemcpyDeviceToHost, ctx->stream));
    DFTA_HIP(ctx, hipStreamSynchronize(ctx->stream));
    void* o = p->hOut.data();
    scatter_sweeps(order, n, kind, stage_ptr<int>(o, L.count), stage_ptr<double>(o, L.u0), start ? start : stage_ptr<int>(o, L.start_out),
                   stage_ptr<int>(o, L.trip), count_out, u0_out, start_out, trip_out);
    if (anybad) *anybad = std::any_of(stage_ptr<int>(o, L.bad), stage_ptr<int>(o, L.bad) + n, [](int b) { return b != 0; });
    return DFTA_OK;
}
// tolerance mode: the scan sweeps (scan.hip), one workgroup per trial in the caller's order; *anybad: a trial it could not decide
int potential_scan_sweeps(dfta_potential* p, const StageLayout& L, int kind, int ntrials, const int* l, const double* E, const int* nodesLimit,
                          int* count_out, double* u0_out, int* start_out, int* trip_out, bool* anybad)
{
    dfta_ctx* ctx = p->ctx;
    const dfta_grid* g = p->g;
    if (!p->scan_built) {
        int rc = dfta_scan_tables_create(ctx, g, 4, &p->scan);
        if (rc) return rc;
        p->scan_built = true;
        rc = dfta_launch_scan_build_tab(ctx, g, p->scan, p->dV, p->dSlots, p->dSlots + 4);
        if (rc) return rc;
    }
    void* hi = p->hIn.data();
    for (int t = 0; t < ntrials; ++t) {
        DFTA_REQUIRE(ctx, l[t] >= 0 && l[t] <= 3, "l");
        stage_ptr<double>(hi, L.E)[t] = E[t]; stage_ptr<int>(hi, L.limit)[t] = nodesLimit ? nodesLimit[t] : 0; stage_ptr<int>(hi, L.blk_slot)[t] = l[t];
    }
    int rc = potential_stage_in(p, L);
    if (rc) return rc;
    void *di = p->dIn.p, *dn = p->dOut.p;
    DFTA_HIP(ctx, dfta_timer_start(ctx));
    rc = dfta_launch_scan_sweeps(ctx, g, kind, ntrials, p->scan, stage_ptr<int>(di, L.blk_slot), stage_ptr<double>(di, L.E), stage_ptr<int>(di, L.limit),
                                 stage_ptr<int>(dn, L.count), stage_ptr<double>(dn, L.u0), stage_ptr<int>(dn, L.start_out), stage_ptr<int>(dn, L.trip),
                                 stage_ptr<int>(dn, L.bad));
    if (rc) return rc;
    DFTA_HIP(ctx, dfta_timer_stop(ctx));
    return potential_stage_out(p, L, nullptr, ntrials, kind, nullptr, count_out, u0_out, start_out, trip_out, anybad);
}
}  // namespace

extern "C" void dfta_potential_destroy(dfta_potential* p)
{
    delete p;
}

extern "C" int dfta_potential_create(dfta_ctx* ctx, const dfta_grid* g, const double* V, dfta_potential** out)
{
    if (!ctx || !g || !V || !out) return DFTA_ERR_INVALID;
    DFTA_ENTER(ctx);
    const int N = g->N;
    std::unique_ptr<dfta_potential> p(new dfta_potential());
    p->ctx = ctx; p->g = g;
    p->h_V.assign(V, V + N);
    hipError_t e = p->dV.alloc(N);
    if (e == hipSuccess) e = p->dTab.alloc(4 * (size_t)N);
    if (e == hipSuccess) e = p->dBounds.alloc(4 * (size_t)dfta_bounds_stride(g));
    if (e == hipSuccess) e = p->dSlots.alloc(8);
    const int slots[8] = {0, 0, 0, 0, 0, 1, 2, 3};
    if (e == hipSuccess) e = hipMemcpy(p->dSlots, slots, sizeof(slots), hipMemcpyHostToDevice);
    if (e != hipSuccess) { snprintf(ctx->err, sizeof(ctx->err), "dfta_potential_create: %s", hipGetErrorString(e)); return DFTA_ERR_HIP; }
    const int rc = potential_build(p.get());
    if (rc) return rc;
    *out = p.release();
    return DFTA_OK;
}

extern "C" int dfta_potential_update(dfta_potential* p, const double* V)
{
    if (!p || !V) return DFTA_ERR_INVALID;
    DFTA_ENTER(p->ctx);
    if (memcmp(V, p->h_V.data(), sizeof(double) * p->g->N) == 0) return DFTA_OK;      // what the reference would re-read is what is resident
    DFTA_HIP(p->ctx, hipStreamSynchronize(p->ctx->stream));                            // h_V may still be the source of a copy
    p->h_V.assign(V, V + p->g->N);
    return potential_build(p);
}

extern "C" int dfta_potential_sweeps(dfta_potential* p, int kind, int sweep_mode, int ntrials, const int* l, const double* E, const int* nodesLimit,
                                     int* count_out, double* u0_out, int* start_out, int* trip_out)
{
    if (!p) return DFTA_ERR_INVALID;
    dfta_ctx* ctx = p->ctx;
    const dfta_grid* g = p->g;
    DFTA_ENTER(ctx);
    DFTA_REQUIRE(ctx, l && E && ntrials >= 0, "null input");
    DFTA_REQUIRE(ctx, kind == DFTA_SWEEP_COUNT || kind == DFTA_SWEEP_ZERO, "kind");
    DFTA_REQUIRE(ctx, kind != DFTA_SWEEP_COUNT || (nodesLimit && count_out), "COUNT needs nodesLimit and count_out");
    DFTA_REQUIRE(ctx, kind != DFTA_SWEEP_ZERO || u0_out, "ZERO needs u0_out");
    DFTA_REQUIRE(ctx, sweep_mode == DFTA_SWEEPS_EXACT || (sweep_mode == DFTA_SWEEPS_TOLERANCE && dfta_scan_supported(g)), "sweep mode / grid");
    if (ntrials == 0) return DFTA_OK;
    int rc = potential_scratch(p, ntrials);
    if (rc) return rc;
    StageLayout L;
    if (dfta_nh::stage_layout(ntrials, dfta_nh::kStageSweeps, &L) != DFTA_OK) return DFTA_ERR_INVALID;
    if (sweep_mode == DFTA_SWEEPS_TOLERANCE) {
        bool anybad = false;
        rc = potential_scan_sweeps(p, L, kind, ntrials, l, E, nodesLimit, count_out, u0_out, start_out, trip_out, &anybad);
        if (rc || !anybad) return rc;
        // a trial the scan could not decide: the whole call again on the exact kernels
    }
    Grouping G;
    if (dfta_nh::make_grouping(ntrials, nullptr, l, 1, G) != DFTA_OK) { snprintf(ctx->err, sizeof(ctx->err), "invalid l"); return DFTA_ERR_INVALID; }
    void *hi = p->hIn.data(), *di = p->dIn.p, *dn = p->dOut.p;
    HostTrials h;
    h.E = stage_ptr<double>(hi, L.E); h.us = stage_ptr<double>(hi, L.us); h.us1 = stage_ptr<double>(hi, L.us1); h.uz = nullptr;
    h.start = stage_ptr<int>(hi, L.start); h.limit = stage_ptr<int>(hi, L.limit); h.l = nullptr;
    fill_sorted(G.order.data(), ntrials, g, E, l, nodesLimit, true, false, h);
    const size_t nb = G.blk_slot.size();
    int *hBs = stage_ptr<int>(hi, L.blk_slot), *hBf = stage_ptr<int>(hi, L.blk_first), *hBc = stage_ptr<int>(hi, L.blk_cnt);
    for (size_t b = 0; b < nb; ++b) { hBs[b] = G.slot_l[G.blk_slot[b]]; hBf[b] = G.blk_first[b]; hBc[b] = G.blk_cnt[b]; }    // table slot = l
    rc = potential_stage_in(p, L);
    if (rc) return rc;
    WaveBlocks blocks;
    blocks.slot = stage_ptr<int>(di, L.blk_slot); blocks.first = stage_ptr<int>(di, L.blk_first); blocks.cnt = stage_ptr<int>(di, L.blk_cnt);
    blocks.kind = nullptr; blocks.n = (int)nb;
    SweepTrials tr{};
    tr.E = stage_ptr<double>(di, L.E); tr.us = stage_ptr<double>(di, L.us); tr.us1 = stage_ptr<double>(di, L.us1);
    tr.limit = stage_ptr<int>(di, L.limit); tr.start = stage_ptr<int>(di, L.start);
    tr.count = stage_ptr<int>(dn, L.count); tr.u0 = stage_ptr<double>(dn, L.u0); tr.trip = stage_ptr<int>(dn, L.trip);
    DFTA_HIP(ctx, dfta_timer_start(ctx));
    rc = dfta_launch_sweep(ctx, g, kind, p->tables(), blocks, tr, nullptr, nullptr, 0);
    if (rc) return rc;
    DFTA_HIP(ctx, dfta_timer_stop(ctx));
    return potential_stage_out(p, L, G.order.data(), ntrials, kind, h.start, count_out, u0_out, start_out, trip_out, nullptr);
}

extern "C" int dfta_potential_match(dfta_potential* p, int ntrials, const int* l, const double* E, double* Psi_out, long* matchPoint_out)
{
    if (!p) return DFTA_ERR_INVALID;
    dfta_ctx* ctx = p->ctx;
    const dfta_grid* g = p->g;
    DFTA_ENTER(ctx);
    DFTA_REQUIRE(ctx, l && E && Psi_out && matchPoint_out && ntrials >= 0, "null input");
    if (ntrials == 0) return DFTA_OK;
    const int N = g->N;
    hipStream_t st = ctx->stream;
    int rc = potential_scratch(p, ntrials);
    if (rc) return rc;
    if ((size_t)ntrials > p->psi_cap) {
        p->dPsi.reset(); p->dQ.reset(); p->psi_cap = 0;
        DFTA_HIP(ctx, p->dPsi.alloc((size_t)ntrials * N));
        DFTA_HIP(ctx, p->dQ.alloc((size_t)ntrials * N));
        p->psi_cap = ntrials;
    }
    StageLayout L;
    if (dfta_nh::stage_layout(ntrials, dfta_nh::kStageMatch, &L) != DFTA_OK) return DFTA_ERR_INVALID;
    for (int t = 0; t < ntrials; ++t) DFTA_REQUIRE(ctx, l[t] >= 0 && l[t] <= 3, "l");
    // (one workgroup per trial and the table slot of a trial is its l: nothing to group, the trials stay in the caller's order)
    void *hi = p->hIn.data(), *di = p->dIn.p, *dn = p->dOut.p;
    HostTrials h;
    h.E = stage_ptr<double>(hi, L.E); h.us = stage_ptr<double>(hi, L.us); h.us1 = stage_ptr<double>(hi, L.us1); h.uz = stage_ptr<double>(hi, L.uz);
    h.start = stage_ptr<int>(hi, L.start); h.limit = nullptr; h.l = stage_ptr<int>(hi, L.l);
    fill_sorted(nullptr, ntrials, g, E, l, nullptr, true, true, h);
    std::copy_n(l, ntrials, stage_ptr<int>(hi, L.trial_slot));
    rc = potential_stage_in(p, L);
    if (rc) return rc;
    SlotTables tables = p->tables();
    if (g->uniform) tables.bounds = nullptr;
    MatchTrials mt;
    mt.slot = stage_ptr<int>(di, L.trial_slot); mt.E = stage_ptr<double>(di, L.E); mt.start = stage_ptr<int>(di, L.start);
    mt.us = stage_ptr<double>(di, L.us); mt.us1 = stage_ptr<double>(di, L.us1); mt.l = stage_ptr<int>(di, L.l); mt.uz = stage_ptr<double>(di, L.uz);
    mt.Psi = p->dPsi; mt.Q = p->dQ; mt.match_point = stage_ptr<int>(dn, L.match_point); mt.n = ntrials;
    rc = dfta_launch_match(ctx, g, tables, mt, nullptr);
    if (rc) return rc;
    DFTA_HIP(ctx, hipMemcpyAsync(Psi_out, p->dPsi, sizeof(double) * ntrials * N, hipMemcpyDeviceToHost, st));
    DFTA_HIP(ctx, hipMemcpyAsync(p->hOut.data(), p->dOut, L.out_bytes, hipMemcpyDeviceToHost, st));
    DFTA_HIP(ctx, hipStreamSynchronize(st));
    for (int t = 0; t < ntrials; ++t) matchPoint_out[t] = stage_ptr<int>(p->hOut.data(), L.match_point)[t];
    return DFTA_OK;
}
