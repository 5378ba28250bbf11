// ctx_grid.cpp -- context and grid tables of libdftatom_hip (Aufbau and the electron configurations: scf_config.cpp).
//
// Grid tables replace the per-point exp() calls of NumerovFunctionNonUniformGrid (Numerov.h:76-101,
// 181-184) and of the SCF pointwise loops (DFTAtom.cpp:42,47,334,439-442; PoissonSolver.h:66-74).
// They are evaluated on the host with libm in exactly the reference's expression order, so device
// kernels work from bit-identical f(i) inputs and never call exp() on grid quantities.
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "common.h"

#ifndef M_PI
#define M_PI 3.14159265358979323846
#endif

extern "C" {

const char* dfta_version(void) { return "dftatom_amd 0.1 (gfx950)"; }

int dfta_ctx_create(int device, void* hip_stream, dfta_ctx** out)
{
    if (!out) return DFTA_ERR_INVALID;
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || device < 0 || device >= ndev) return DFTA_ERR_NO_DEVICE;
    if (hipSetDevice(device) != hipSuccess) return DFTA_ERR_NO_DEVICE;
    dfta_ctx* c = new dfta_ctx();
    c->device = device;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) != hipSuccess) { delete c; return DFTA_ERR_NO_DEVICE; }
    c->num_cu = prop.multiProcessorCount;
    snprintf(c->name, sizeof(c->name), "%s (%s)", prop.name, prop.gcnArchName);
    if (hip_stream) {
        c->stream = reinterpret_cast<hipStream_t>(hip_stream);
        c->own_stream = false;
    } else {
        if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) { delete c; return DFTA_ERR_NO_DEVICE; }
        c->own_stream = true;
    }
    if (hipEventCreate(&c->ev[0]) != hipSuccess || hipEventCreate(&c->ev[1]) != hipSuccess) { delete c; return DFTA_ERR_NO_DEVICE; }
    if (const char* e = dfta_knob("SWEEP_KERNEL"))
        c->sweep_kernel = !strcmp(e, "fused") ? DFTA_SWEEP_FUSED : (!strcmp(e, "pipe") ? DFTA_SWEEP_PIPELINED : DFTA_SWEEP_AUTO);
    *out = c;
    return DFTA_OK;
}

int dfta_ctx_set_sweep_kernel(dfta_ctx* ctx, int which)
{
    if (!ctx) return DFTA_ERR_INVALID;
    if (which < DFTA_SWEEP_AUTO || which > DFTA_SWEEP_PIPELINED) {
        snprintf(ctx->err, sizeof(ctx->err), "dfta_ctx_set_sweep_kernel: unknown kernel %d", which);
        return DFTA_ERR_INVALID;
    }
    ctx->sweep_kernel = which;
    return DFTA_OK;
}

int dfta_ctx_last_kernel_ms(dfta_ctx* ctx, float* ms)
{
    if (!ctx || !ms) return DFTA_ERR_INVALID;
    DFTA_REQUIRE(ctx, ctx->have_kernel_time, "no timed kernel yet");
    DFTA_HIP(ctx, hipEventSynchronize(ctx->ev[1]));
    DFTA_HIP(ctx, hipEventElapsedTime(ms, ctx->ev[0], ctx->ev[1]));
    return DFTA_OK;
}

void dfta_ctx_destroy(dfta_ctx* ctx)
{
    if (!ctx) return;
    for (hipEvent_t e : ctx->ev) if (e) (void)hipEventDestroy(e);
    if (ctx->own_stream && ctx->stream) (void)hipStreamDestroy(ctx->stream);
    delete ctx;
}

int dfta_ctx_synchronize(dfta_ctx* ctx)
{
    if (!ctx) return DFTA_ERR_INVALID;
    DFTA_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return DFTA_OK;
}

const char* dfta_last_error(const dfta_ctx* ctx) { return ctx ? ctx->err : "null context"; }

int dfta_ctx_device_info(const dfta_ctx* ctx, int* num_cu, char* name, int name_cap)
{
    if (!ctx) return DFTA_ERR_INVALID;
    if (num_cu) *num_cu = ctx->num_cu;
    if (name && name_cap > 0) { strncpy(name, ctx->name, static_cast<size_t>(name_cap) - 1); name[name_cap - 1] = 0; }
    return DFTA_OK;
}

int dfta_num_nodes(int mg_levels)   // PoissonSolver.h:127-135 with Ncoarse = 3
{
    int size = 3;
    for (int i = 0; i < mg_levels - 1; ++i) size = size * 2 - 1;
    return size;
}

// smallest double a with exp(a) >= 1e-200 (libm); the reference's cut-off test `exp(arg) < 1E-200`
// (Numerov.h:129) is then `arg < a` for a monotone exp.
static double far_threshold()
{
    auto key = [](double x) { int64_t b; memcpy(&b, &x, 8); return b < 0 ? INT64_MIN - b : b; };   // monotone map
    auto unkey = [](int64_t k) { int64_t b = k < 0 ? INT64_MIN - k : k; double x; memcpy(&x, &b, 8); return x; };
    int64_t lo = key(-461.0), hi = key(-460.0);   // exp(lo) < 1e-200 <= exp(hi)
    while (hi - lo > 1) {
        const int64_t mid = lo + (hi - lo) / 2;
        if (exp(unkey(mid)) < 1E-200) lo = mid; else hi = mid;
    }
    return unkey(hi);
}

// the grid's device tables: allocated and filled in the order given
struct Upload { DevBuf<double>* d; const double* h; size_t n; };
static int upload_tables(dfta_ctx* ctx, const Upload* ups, size_t count)
{
    for (size_t i = 0; i < count; ++i) {
        hipError_t e = ups[i].d->alloc(ups[i].n);
        if (e == hipSuccess) e = hipMemcpyAsync(ups[i].d->p, ups[i].h, ups[i].n * sizeof(double), hipMemcpyHostToDevice, ctx->stream);
        if (e != hipSuccess) {
            snprintf(ctx->err, sizeof(ctx->err), "grid upload: %s", hipGetErrorString(e));
            return DFTA_ERR_HIP;
        }
    }
    DFTA_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return DFTA_OK;
}

int dfta_grid_create(dfta_ctx* ctx, int mg_levels, double delta, double Rmax, dfta_grid** out)
{
    if (!ctx || !out) return DFTA_ERR_INVALID;
    DFTA_ENTER(ctx);
    DFTA_REQUIRE(ctx, mg_levels >= 3 && mg_levels <= 24 && delta > 0 && Rmax > 0, "grid parameters");
    std::unique_ptr<dfta_grid> owner(new dfta_grid());
    dfta_grid* g = owner.get();
    g->ctx = ctx;
    g->levels = mg_levels;
    const int N = dfta_num_nodes(mg_levels);
    g->N = N;
    g->delta = delta;
    g->Rmax = Rmax;
    // Numerov.h:79-86
    g->Rp = Rmax / (exp((static_cast<double>(N) - 1.) * delta) - 1.);
    const double Rp2 = g->Rp * g->Rp;
    g->twodelta = 2. * delta;
    const double delta2 = delta * delta;
    g->Rp2delta2 = Rp2 * delta2;
    g->delta2p4 = delta2 * 0.25;
    g->far_arg_threshold = far_threshold();

    std::vector<double>&r = g->h_r, &e1 = g->h_e1, &e2 = g->h_e2, &eh = g->h_eh;
    r.resize(N); e1.resize(N); e2.resize(N); eh.resize(N);
    std::vector<double> cl(static_cast<size_t>(4) * N, 0.0), cnst(N), psrc(N), fpr2(N);
    const double fourM_PI = 4. * M_PI;
    const double fourM_PIRp2delta2 = fourM_PI * g->Rp2delta2;   // PoissonSolver.h:64-70 (Rp*Rp*delta2grid == Rp2*delta2)
    for (int i = 0; i < N; ++i) {
        e1[i] = exp(static_cast<double>(i) * delta);              // Numerov.h:183, DFTAtom.cpp:334,439
        r[i] = g->Rp * (e1[i] - 1.);
        e2[i] = exp(static_cast<double>(i) * g->twodelta);         // Numerov.h:100, PoissonSolver.h:74
        eh[i] = exp(i * delta * 0.5);                               // DFTAtom.cpp:42
        cnst[i] = g->Rp * delta * e1[i];                            // DFTAtom.cpp:47,442
        psrc[i] = fourM_PIRp2delta2 * e2[i];                        // PoissonSolver.h:74
        fpr2[i] = fourM_PI * r[i] * r[i];                           // DFTAtom.cpp:340
        if (i > 0)
            for (unsigned l = 1; l < 4; ++l)
                cl[static_cast<size_t>(l) * N + i] = l * (l + 1.) / (r[i] * r[i]) * 0.5;   // Numerov.h:93
    }
    for (unsigned l = 0; l < 4; ++l)   // Numerov.h:110-116 at position = 1
        g->zero1[l] = pow(r[1], static_cast<double>(l) + 1) * exp(-1.0 * delta * 0.5);

    const Upload ups[] = {
        {&g->d_r, r.data(), (size_t)N}, {&g->d_e1, e1.data(), (size_t)N}, {&g->d_e2, e2.data(), (size_t)N},
        {&g->d_eh, eh.data(), (size_t)N}, {&g->d_cl, cl.data(), (size_t)4 * N}, {&g->d_cnst, cnst.data(), (size_t)N},
        {&g->d_psrc, psrc.data(), (size_t)N}, {&g->d_fpr2, fpr2.data(), (size_t)N}};
    if (int rc = upload_tables(ctx, ups, sizeof(ups) / sizeof(ups[0]))) return rc;
    g->d_rsrc = g->d_r;
    *out = owner.release();
    return DFTA_OK;
}

// Uniform grid r_i = i h, h = MaxR / NumSteps (DFTAtom.cpp:66-68, NumerovFunctionRegularGrid Numerov.h:16-70).
int dfta_grid_create_uniform(dfta_ctx* ctx, int mg_levels, double Rmax, dfta_grid** out)
{
    if (!ctx || !out) return DFTA_ERR_INVALID;
    DFTA_ENTER(ctx);
    DFTA_REQUIRE(ctx, mg_levels >= 3 && mg_levels <= 24 && Rmax > 0, "grid parameters");
    std::unique_ptr<dfta_grid> owner(new dfta_grid());
    dfta_grid* g = owner.get();
    g->ctx = ctx;
    g->levels = mg_levels;
    const int N = dfta_num_nodes(mg_levels);
    g->N = N;
    g->uniform = 1;
    g->delta = 0;
    g->Rmax = Rmax;
    g->Rp = 0;
    const long steps = N - 1;
    g->h = Rmax / steps;                         // Numerov.h:276 (h = startPoint / steps), DFTAtom.cpp:68
    g->h2 = g->h * g->h;
    g->h2p12 = g->h2 / 12.;
    g->Rp2delta2 = 1; g->delta2p4 = 0; g->twodelta = 0;
    g->far_arg_threshold = far_threshold();
    std::vector<double>&r = g->h_r, &e1 = g->h_e1, &e2 = g->h_e2, &eh = g->h_eh;
    r.resize(N); e1.assign(N, 1.0); e2.assign(N, 1.0); eh.assign(N, 1.0);
    std::vector<double> cl(static_cast<size_t>(4) * N, 0.0), cnst(N, 1.0), psrc(N), fpr2(N), rsrc(N);
    const double fourM_PI = 4. * M_PI;
    {
        // PoissonSolver::FillR(Source, 0, maxRadius) (PoissonSolver.cpp:200-210) and the factor of PoissonSolver.h:26-40
        const size_t Nn = static_cast<size_t>(N) - 1;
        for (size_t i = 0; i < static_cast<size_t>(N); ++i) rsrc[i] = (0.0 * (Nn - i) + Rmax * i) / Nn;
        const double dl = rsrc[1] - rsrc[0];
        const double delta2fourM_PI = (dl * dl) * fourM_PI;
        for (int i = 0; i < N; ++i) psrc[i] = delta2fourM_PI;
    }
    for (int i = 0; i < N; ++i) {
        r[i] = g->h * i;                                           // Numerov.h:313 (position = h * i), DFTAtom.cpp:102,126
        fpr2[i] = fourM_PI * r[i] * r[i];                          // DFTAtom.cpp:132
        if (i > 0)
            for (unsigned l = 1; l < 4; ++l)
                cl[static_cast<size_t>(l) * N + i] = l * (l + 1.) / (r[i] * r[i]) * 0.5;   // Numerov.h:23
    }
    for (unsigned l = 0; l < 4; ++l) g->zero1[l] = pow(g->h, static_cast<double>(l) + 1.);   // Numerov.h:38-41 at position = h (sweeps keep h; the match solve re-derives it)
    const Upload ups[] = {
        {&g->d_r, r.data(), (size_t)N}, {&g->d_e1, e1.data(), (size_t)N}, {&g->d_e2, e2.data(), (size_t)N},
        {&g->d_eh, eh.data(), (size_t)N}, {&g->d_cl, cl.data(), (size_t)4 * N}, {&g->d_cnst, cnst.data(), (size_t)N},
        {&g->d_psrc, psrc.data(), (size_t)N}, {&g->d_fpr2, fpr2.data(), (size_t)N}, {&g->d_rsrc_own, rsrc.data(), (size_t)N}};
    if (int rc = upload_tables(ctx, ups, sizeof(ups) / sizeof(ups[0]))) return rc;
    g->d_rsrc = g->d_rsrc_own;
    *out = owner.release();
    return DFTA_OK;
}

void dfta_grid_destroy(dfta_grid* g)
{
    if (!g) return;
    delete g;
}

int dfta_grid_is_uniform(const dfta_grid* g) { return g ? g->uniform : 0; }

int dfta_grid_num_nodes(const dfta_grid* g) { return g ? g->N : 0; }
double dfta_grid_rp(const dfta_grid* g) { return g ? g->Rp : 0.0; }
int dfta_grid_get_r(const dfta_grid* g, double* r_host)
{
    if (!g || !r_host) return DFTA_ERR_INVALID;
    memcpy(r_host, g->h_r.data(), sizeof(double) * g->h_r.size());
    return DFTA_OK;
}

}  // extern "C"
