// scf.hip -- one SCF iteration for a batch of atoms, state resident in HBM.
//
// Replaces the body of DFTAtom::CalculateNonUniformLDA (DFTAtom.cpp:346-491) and
// DFTAtom::CalculateNonUniformLSDA (DFTAtom.cpp:847-1022): flat-density start, level search for every
// (atom, spin), density mixing, multigrid Poisson, VWN, the pointwise potential/integrand pass, the five
// Simpson 3/8 integrals (reference summation order) and the energy assembly + convergence test.
// Potentials are stored as V[(atom * nspin + spin) * N + i].
// What a configuration and the options may be is scf_config.cpp's (pure host code); the accessors of the state are scf_api.cpp's.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <vector>

#include "ordered_sum.h"
#include "scf_state.h"
#include "xc.h"

namespace {

constexpr double kPi = 3.14159265358979323846;
constexpr double fourM_PI = 4. * kPi;
constexpr double kTotalEnergyErr = 1E-11;   // DFTAtom.cpp:349

// flat start density (DFTAtom.cpp:371-376 / 874-884)
__global__ void k_init_density(const AtomState* __restrict__ atoms, int lsda, int N, double MaxR, double* __restrict__ density,
                               double* __restrict__ dA, double* __restrict__ dB)
{
    const int a = blockIdx.y;
    const double volume = fourM_PI / 3. * MaxR * MaxR * MaxR;
    const AtomState s = atoms[a];
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < N; i += gridDim.x * blockDim.x) {
        const size_t o = (size_t)a * N + i;
        if (!lsda) density[o] = (i == 0) ? 0. : s.nE / volume;
        else {
            const double cA = s.nAlphaE / volume, cB = s.nBetaE / volume;
            dA[o] = (i == 0) ? 0. : cA;
            dB[o] = (i == 0) ? 0. : cB;
            density[o] = (i == 0) ? 0. : cA + cB;
        }
    }
}

// potential from U and v_xc (DFTAtom.cpp:387-392 / 895-904, also the first statement of the tail loop)
__global__ void k_potential(const AtomState* __restrict__ atoms, int lsda, int N, const double* __restrict__ r,
                            const double* __restrict__ U, const double* __restrict__ Vexc, const double* __restrict__ va,
                            const double* __restrict__ vb, double* __restrict__ V)
{
    const int a = blockIdx.y;
    const int Z = atoms[a].Z;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < N; i += gridDim.x * blockDim.x) {
        const size_t o = (size_t)a * N + i;
        if (!lsda) V[o] = (i == 0) ? 0. : (-Z + U[o]) / r[i] + Vexc[o];
        else {
            const double u = (i == 0) ? 0. : (-Z + U[o]) / r[i];
            V[((size_t)2 * a) * N + i] = (i == 0) ? 0. : u + va[o];
            V[((size_t)2 * a + 1) * N + i] = (i == 0) ? 0. : u + vb[o];
        }
    }
}

// newDensity /= 4 pi r^2; density = alpha density + (1-alpha) newDensity (DFTAtom.cpp:332-342); LSDA total (DFTAtom.cpp:933-934)
__global__ void k_mix(int lsda, int N, double alpha, double oneMinusAlpha, const double* __restrict__ fpr2,
                      double* __restrict__ newDensity, double* __restrict__ density, double* __restrict__ dA, double* __restrict__ dB,
                      const int* __restrict__ fin)
{
    const int a = blockIdx.y;
    if (fin[a]) return;        // a finished atom is frozen (the reference leaves its loop: DFTAtom.cpp:474-479)
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < N; i += gridDim.x * blockDim.x) {
        if (i == 0) continue;
        const size_t o = (size_t)a * N + i;
        if (!lsda) {
            double nd = newDensity[o];
            nd /= fpr2[i];
            newDensity[o] = nd;
            density[o] = alpha * density[o] + oneMinusAlpha * nd;
        } else {
            const size_t oa = ((size_t)2 * a) * N + i, ob = ((size_t)2 * a + 1) * N + i;
            double na = newDensity[oa], nb = newDensity[ob];
            na /= fpr2[i];
            nb /= fpr2[i];
            newDensity[oa] = na;
            newDensity[ob] = nb;
            const double x = alpha * dA[o] + oneMinusAlpha * na;
            const double y = alpha * dB[o] + oneMinusAlpha * nb;
            dA[o] = x;
            dB[o] = y;
            density[o] = x + y;
        }
    }
}

// new potential + the five integrands (DFTAtom.cpp:437-457 / 956-983); integrands: [atom][5][N]
__global__ void k_tail(const AtomState* __restrict__ atoms, int lsda, int N, const double* __restrict__ r,
                       const double* __restrict__ cnst, const double* __restrict__ density, const double* __restrict__ dA,
                       const double* __restrict__ dB, const double* __restrict__ U, const double* __restrict__ Vexc,
                       const double* __restrict__ va, const double* __restrict__ vb, const double* __restrict__ eexc,
                       double* __restrict__ V, double* __restrict__ integrands, int uniform)
{
    const int a = blockIdx.y;
    if (atoms[a].finished) return;
    const int Z = atoms[a].Z;
    double* nuclear = integrands + ((size_t)a * 5 + 0) * N;
    double* exccor = integrands + ((size_t)a * 5 + 1) * N;
    double* eexcD = integrands + ((size_t)a * 5 + 2) * N;
    double* hartree = integrands + ((size_t)a * 5 + 3) * N;
    double* potentiale = integrands + ((size_t)a * 5 + 4) * N;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < N; i += gridDim.x * blockDim.x) {
        const size_t o = (size_t)a * N + i;
        if (i == 0) {
            if (!lsda) V[o] = 0; else { V[((size_t)2 * a) * N] = 0; V[((size_t)2 * a + 1) * N] = 0; }
            nuclear[0] = 0; exccor[0] = 0; eexcD[0] = 0; hartree[0] = 0; potentiale[0] = 0;
            continue;
        }
        const double position = r[i];
        const double c = cnst[i];
        const double rho = density[o];
        if (!lsda) {
            const double pot = (-Z + U[o]) / position + Vexc[o];
            V[o] = pot;
            const double positiondensity = position * rho * c;
            nuclear[i] = Z * positiondensity;
            const double position2density = position * position * rho * c;
            exccor[i] = position2density * Vexc[o];
            eexcD[i] = position2density * eexc[o];
            hartree[i] = positiondensity * U[o];
            potentiale[i] = position2density * pot;
        } else {
            const double u = (-Z + U[o]) / position;
            const double pa = u + va[o], pb = u + vb[o];
            V[((size_t)2 * a) * N + i] = pa;
            V[((size_t)2 * a + 1) * N + i] = pb;
            const double positioncnst = position * c;
            const double positiondensity = positioncnst * rho;
            nuclear[i] = Z * positiondensity;
            const double position2cnst = position * positioncnst;
            const double position2density = position2cnst * rho;
            const double p2a = position2cnst * dA[o];
            const double p2b = position2cnst * dB[o];
            exccor[i] = position2density * Vexc[o];
            eexcD[i] = position2density * eexc[o];
            hartree[i] = positiondensity * U[o];
            // DFTAtom.cpp:981 on the logarithmic grid; the uniform-grid loop groups the product differently (DFTAtom.cpp:799)
            potentiale[i] = uniform ? (position * position) * (dA[o] * pa + dB[o] * pb) : p2a * pa + p2b * pb;
        }
    }
}

// energy assembly and the reference's stop test (DFTAtom.cpp:459-481 / 985-1006); one thread per atom
// Ex: null, or per atom the exchange energy of an orbital-dependent exchange (DFTA_EXCHANGE_KLI) or E_SIC (DFTA_EXCHANGE_SIC_KLI), added
// to eExcDif
__global__ void k_energies(AtomState* __restrict__ atoms, int natoms, const dfta::Job* __restrict__ jobs,
                           const double* __restrict__ occ, const double* __restrict__ integrals, double* __restrict__ records, int* __restrict__ fin,
                           const double* __restrict__ Ex)
{
    const int a = blockIdx.x * blockDim.x + threadIdx.x;
    if (a >= natoms) return;
    AtomState s = atoms[a];
    if (s.finished) return;     // energies, eigenvalues, step count and record stay those of the finishing step
    double Eelectronic = 0;
    bool conv = true;
    for (int k = s.job_off; k < s.job_end; ++k) {
        Eelectronic += occ[k] * jobs[k].E;                         // DFTAtom.cpp:561 (occ[k] == (double)jobs[k].occ for Aufbau)
        conv = conv && (jobs[k].converged != 0);
    }
    const double* I = integrals + (size_t)a * 5;
    const double Enuclear = -fourM_PI * I[0];
    double Exc = fourM_PI * I[1];
    const double eExcDif = Ex ? fourM_PI * I[2] + Ex[a] : fourM_PI * I[2];
    Exc += eExcDif;
    const double Ehartree = -2 * kPi * I[3];
    const double Epotential = fourM_PI * I[4];
    const double Ekinetic = Eelectronic - Epotential;
    const double Etotal = Eelectronic + Ehartree + eExcDif;
    s.e.Etotal = Etotal; s.e.Ekinetic = Ekinetic; s.e.Ecoul = -Ehartree; s.e.Enuclear = Enuclear; s.e.Exc = Exc;
    s.e.Eelectronic = Eelectronic; s.e.Ehartree = Ehartree; s.e.eExcDif = eExcDif; s.e.Epotential = Epotential;
    s.steps++;
    if (fabs((s.Eold - Etotal) / Etotal) < kTotalEnergyErr && conv && s.lastTimeConverged) s.finished = 1;
    else { s.Eold = Etotal; s.lastTimeConverged = conv ? 1 : 0; }
    atoms[a] = s;
    fin[a] = s.finished;
    if (records) {
        double* R = records + (size_t)a * DFTA_RECORD_DOUBLES;
        R[0] = s.Z; R[1] = Etotal; R[2] = Ekinetic; R[3] = -Ehartree; R[4] = Enuclear; R[5] = Exc; R[6] = s.finished;
        R[7] = s.steps; R[8] = s.job_end - s.job_off; R[9] = conv ? 1. : 0.;
        int m = 10;
        for (int k = s.job_off; k < s.job_end && m < DFTA_RECORD_DOUBLES; ++k) R[m++] = jobs[k].E;
        for (; m < DFTA_RECORD_DOUBLES; ++m) R[m] = 0;
    }
}

}  // namespace

// the linear mix of a step as its one launch: dfta_scf_step's, and dfta_mixer_step's (mixing.hip) with DFTA_MIX_LINEAR
int dfta_launch_linear_mix(dfta_ctx* ctx, const dfta_grid* g, int lsda, int natoms, double alpha, double oneMinusAlpha, double* newDensity,
                           double* density, double* dA, double* dB, const int* fin)
{
    const int N = g->N;
    hipLaunchKernelGGL(k_mix, dim3(std::min(64, (N + 255) / 256), natoms), dim3(256), 0, ctx->stream, lsda, N, alpha, oneMinusAlpha, g->d_fpr2,
                       newDensity, density, dA, dB, fin);
    DFTA_CHECK_LAUNCH(ctx);
    return DFTA_OK;
}

// rows idx[y] of src -> row y of dst, and back (the live atoms of a batch, see dfta_scf::live_solver)
__global__ void k_gather_rows(const double* __restrict__ src, const int* __restrict__ idx, int N, double* __restrict__ dst)
{
    const double* s = src + (size_t)idx[blockIdx.y] * N;
    double* d = dst + (size_t)blockIdx.y * N;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < N; i += gridDim.x * blockDim.x) d[i] = s[i];
}
__global__ void k_scatter_rows(const double* __restrict__ src, const int* __restrict__ idx, int N, double* __restrict__ dst)
{
    const double* s = src + (size_t)blockIdx.y * N;
    double* d = dst + (size_t)idx[blockIdx.y] * N;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < N; i += gridDim.x * blockDim.x) d[i] = s[i];
}

// The exchange stage on the step's orbitals for every live channel, then its potential into Vexc / va / vb / eexc: under
// DFTA_EXCHANGE_KLI in place of scf_xc, under DFTA_EXCHANGE_SIC_KLI after scf_xc and on top of the functional's (the stage knows which)
static int scf_exchange_stage(dfta_scf* s)
{
    const int nspin = s->nspin;
    s->h_live_ch.resize((size_t)s->nV);
    for (int a = 0; a < s->natoms; ++a)
        for (int sp = 0; sp < nspin; ++sp) s->h_live_ch[(size_t)a * nspin + sp] = s->h_atoms[a].finished ? 0 : 1;
    const dfta::Job* jobs = s->solver.d_jobs.p;
    int rc = s->kli.run(s->ctx, s->g, s->solver.d_Psi.p, &jobs->E, sizeof(dfta::Job), s->h_live_ch.data(), s->steps_done == 1, s->alpha,
                        1. - s->alpha);
    if (rc) return rc;
    return s->kli.assemble(s->ctx, s->g, s->lsda, s->d_density.p, s->d_dA.p, s->d_dB.p, s->d_fin.p, s->d_Vexc.p, s->d_va.p, s->d_vb.p, s->d_eexc.p);
}

static int scf_xc(dfta_scf* s)
{
    const size_t sz = (size_t)s->natoms * s->g->N;
    // PBE: one fused stencil + pointwise + divergence launch (gga.hip), frozen atoms skipped; PW92: pointwise, as VWN
    if (s->functional == DFTA_XC_PBE)
        return dfta_launch_pbe_radial(s->ctx, s->g, s->natoms, s->lsda ? s->d_dA : s->d_density, s->lsda ? s->d_dB.p : nullptr, s->d_Vexc,
                                      s->d_va, s->d_vb, s->d_eexc, s->d_fin);
    if (s->functional == DFTA_XC_PW92)
        return s->lsda ? dfta_launch_pw92_lsda(s->ctx, s->d_dA, s->d_dB, sz, s->d_Vexc, s->d_va, s->d_vb, s->d_eexc)
                       : dfta_launch_pw92_lda(s->ctx, s->d_density, sz, s->d_Vexc, s->d_eexc);
    if (!s->lsda && s->functional != DFTA_XC_VWN)
        return dfta_launch_chachiyo_lda(s->ctx, s->functional == DFTA_XC_CHACHIYO_IMPROVED, s->d_density, sz, s->d_Vexc, s->d_eexc);
    if (!s->lsda) return dfta_launch_vwn_lda(s->ctx, s->d_density, sz, s->d_Vexc, s->d_eexc);
    return dfta_launch_vwn_lsda(s->ctx, s->d_dA, s->d_dB, sz, s->d_Vexc, s->d_va, s->d_vb, s->d_eexc);
}

extern "C" {

void dfta_scf_destroy(dfta_scf* s)
{
    if (!s) return;
    if (s->poisson) dfta_poisson_destroy(s->poisson);
    for (auto& ls : s->live_solver) if (ls.p) dfta_poisson_destroy(ls.p);
    delete s;
}

int dfta_abi_version(void) { return DFTA_ABI_VERSION; }

int dfta_scf_create(dfta_ctx* ctx, const dfta_grid* g, int lsda, int natoms, const int* Z, double alpha, int levels_mode,
                    int tree_depth, dfta_scf** out)
{
    return dfta_scf_create_ex(ctx, g, lsda, natoms, Z, alpha, levels_mode, tree_depth, nullptr, out);
}

int dfta_scf_create_ex(dfta_ctx* ctx, const dfta_grid* g, int lsda, int natoms, const int* Z, double alpha, int levels_mode,
                       int tree_depth, const dfta_scf_options* options, dfta_scf** out)
{
    return dfta_scf_create_config(ctx, g, lsda, natoms, Z, nullptr, nullptr, nullptr, nullptr, alpha, levels_mode, tree_depth, options, out);
}

int dfta_scf_create_config(dfta_ctx* ctx, const dfta_grid* g, int lsda, int natoms, const int* Z, const int* nlev, const int* cn,
                           const int* cl, const double* cocc, double alpha, int levels_mode, int tree_depth,
                           const dfta_scf_options* options, dfta_scf** out)
{
    if (!ctx || !g || !out) return DFTA_ERR_INVALID;
    DFTA_ENTER(ctx);
    DFTA_REQUIRE(ctx, natoms >= 1 && Z && alpha >= 0 && alpha <= 1, "scf arguments");
    DFTA_REQUIRE(ctx, !nlev || (cn && cl && cocc), "configuration: n, l and occ are needed with nlev");
    dfta::ScfFacts facts = {lsda ? 1 : 0, g->uniform, dfta_scan_supported(g), 0u, kAndersonMaxHistory};
    for (int r = 0; r <= DFTA_INT_ROMBERG; ++r) if (dfta_integral_shape_ok(r, g->N)) facts.integrators_fit |= 1u << r;
    dfta_scf_options opt;
    if (const char* why = dfta::resolve_scf_options(options, facts, &opt)) DFTA_REQUIRE(ctx, false, why);
    dfta_scf* s = new dfta_scf();
    struct Guard { dfta_scf* s; ~Guard() { dfta_scf_destroy(s); } } guard{s};      // every error return below destroys what has been made
    s->solver.sweep_mode = opt.sweep_mode;
    s->solver.integ_rule = opt.integrator;
    s->functional = opt.functional;
    s->ctx = ctx; s->g = g; s->lsda = lsda ? 1 : 0; s->natoms = natoms; s->nspin = lsda ? 2 : 1; s->nV = natoms * s->nspin;
    s->alpha = alpha;
    const int N = g->N;
    if (dfta::plan_scf_config(natoms, Z, nlev, cn, cl, cocc, s->lsda, opt.aufbau, &s->cfg)) {
        snprintf(ctx->err, sizeof(ctx->err), "%s", dfta_config_last_error());
        return DFTA_ERR_INVALID;
    }
    s->h_atoms.resize(natoms);
    for (int a = 0; a < natoms; ++a) {
        const dfta::AtomConfig& c = s->cfg.atoms[a];
        AtomState& at = s->h_atoms[a];
        memset(&at, 0, sizeof(at));
        at.Z = c.Z; at.nE = c.nE; at.nAlphaE = c.nAlphaE; at.nBetaE = c.nBetaE; at.job_off = c.job_off; at.job_end = c.job_end;
    }
    int rc = s->solver.setup(ctx, g, levels_mode, tree_depth, s->nV, s->cfg.specs);
    if (rc) return rc;
    rc = opt.poisson_mode < 0 ? dfta_poisson_create(ctx, g, natoms, &s->poisson) : dfta_poisson_create_ex(ctx, g, natoms, opt.poisson_mode, &s->poisson);
    if (rc) return rc;

    hipStream_t st = ctx->stream;
    const size_t aN = (size_t)natoms * N;
    hipError_t e = hipSuccess;
    auto al = [&](auto& buf, size_t cnt) { if (e == hipSuccess) e = buf.alloc(cnt); };
    al(s->d_density, aN); al(s->d_dA, aN); al(s->d_dB, aN); al(s->d_V, aN * s->nspin); al(s->d_U, aN); al(s->d_Vexc, aN);
    al(s->d_va, aN); al(s->d_vb, aN); al(s->d_eexc, aN); al(s->d_newDensity, aN * s->nspin); al(s->d_integrands, aN * 5);
    al(s->d_integrals, (size_t)natoms * 5); al(s->d_records, (size_t)natoms * DFTA_RECORD_DOUBLES);
    al(s->d_atoms, natoms); al(s->d_Ne, natoms); al(s->d_fin, natoms);
    s->mixing = opt.mixing;
    if (e == hipSuccess && s->mixing == DFTA_MIX_ANDERSON) {       // the history ring: 2 mix_history doubles per node and spin channel
        rc = dfta_anderson_create(ctx, g, natoms, s->nspin, opt.mix_history, opt.mix_warmup, &s->anderson);
        if (rc) return rc;
    }
    if (e == hipSuccess) e = hipMemsetAsync(s->d_fin, 0, sizeof(int) * natoms, st);
    for (auto& ev : s->ev) if (e == hipSuccess) e = hipEventCreate(&ev.e);
    if (e == hipSuccess) e = hipMemcpyAsync(s->d_atoms, s->h_atoms.data(), sizeof(AtomState) * natoms, hipMemcpyHostToDevice, st);
    std::vector<double> h_ne(natoms);
    for (int a = 0; a < natoms; ++a) h_ne[a] = s->h_atoms[a].nE;
    if (e == hipSuccess) e = hipMemcpyAsync(s->d_Ne, h_ne.data(), sizeof(double) * natoms, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemsetAsync(s->d_records, 0, sizeof(double) * natoms * DFTA_RECORD_DOUBLES, st);
    if (e != hipSuccess) { snprintf(ctx->err, sizeof(ctx->err), "scf alloc: %s", hipGetErrorString(e)); return DFTA_ERR_HIP; }
    // DFTAtom.cpp:371-392 / 874-904: flat density, Poisson, v_xc, start potential
    const dim3 grid(std::min(64, (N + 255) / 256), natoms), block(256);
    hipLaunchKernelGGL(k_init_density, grid, block, 0, st, s->d_atoms.p, s->lsda, N, g->Rmax, s->d_density.p, s->d_dA.p, s->d_dB.p);
    rc = dfta_poisson_solve_launch(s->poisson, s->d_Ne, s->d_density, s->d_U, nullptr, nullptr, nullptr);
    if (!rc) rc = dfta_poisson_finish(s->poisson, s->d_Ne, s->d_density, s->d_U, nullptr, nullptr, nullptr);
    if (!rc) rc = scf_xc(s);
    if (rc) return rc;
    hipLaunchKernelGGL(k_potential, grid, block, 0, st, s->d_atoms.p, s->lsda, N, g->d_r, s->d_U.p, s->d_Vexc.p, s->d_va.p, s->d_vb.p, s->d_V.p);
    e = hipGetLastError();
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) { snprintf(ctx->err, sizeof(ctx->err), "scf init: %s", hipGetErrorString(e)); return DFTA_ERR_HIP; }
    unsigned long long dummy;
    rc = dfta_poisson_take_vcycles(s->poisson, &dummy);
    if (rc) return rc;
    s->debug_levels = dfta_knob("DEBUG_LEVELS") != nullptr;
    s->kli_y_mb = dfta_kli_budget_mb();
    s->h_frozen.assign(s->cfg.specs.size(), 0);
    guard.s = nullptr;
    *out = s;
    return DFTA_OK;
}

// The multigrid solver of the live atoms' size class (made when first wanted) and that class's size, or null: the batch's own solver
// does the work.  An optimisation only: the level solve and the mixing of this step have already run, so nothing may fail here
static dfta_poisson* scf_live_solver(dfta_scf* s, int nlive, int* cls_atoms)
{
    if (nlive <= 0 || dfta_knob("SCF_NOLIVE") != nullptr) return nullptr;
    for (int c = 0; c < kLiveClasses; ++c) {
        if (kLiveClassAtoms[c] < nlive) continue;
        if (kLiveClassAtoms[c] >= s->natoms) break;              // the batch's own solver is of that class already
        dfta_scf::LiveSolver& ls = s->live_solver[c];
        if (!ls.tried) {
            ls.tried = true;
            int Gbig = 0;
            dfta_poisson_group_state(s->poisson, &Gbig, nullptr, nullptr);
            // if the class solver cannot be made (memory), the batch's own solver does the work
            if (dfta_poisson_create_ex(s->ctx, s->g, kLiveClassAtoms[c], dfta_poisson_mode(s->poisson), &ls.p)) { ls.p = nullptr; s->ctx->err[0] = 0; (void)hipGetLastError(); }
            if (ls.p) {
                dfta_poisson_group_state(ls.p, &ls.G, nullptr, nullptr);
                if (ls.G <= Gbig) { dfta_poisson_destroy(ls.p); ls.p = nullptr; }     // nothing to gain on this grid
            }
        }
        *cls_atoms = kLiveClassAtoms[c];
        return ls.p;                                              // the smallest class that holds the live atoms, or the batch's solver
    }
    return nullptr;
}

// Gathered copies of the live atoms' densities for the solver of their size class: room for cls_atoms rows (grown when needed), skip flags,
// atom indices and electron counts staged and uploaded, the rows gathered.  *gathered = false: no room, the batch's own solver (same bits).
static int scf_gather_live(dfta_scf* s, const std::vector<int>& live_atoms, int cls_atoms, bool* gathered)
{
    dfta_ctx* ctx = s->ctx;
    hipStream_t st = ctx->stream;
    const int N = s->g->N, nlive = static_cast<int>(live_atoms.size());
    *gathered = false;
    if (s->live_cap < cls_atoms) {
        s->free_live();
        hipError_t e = s->d_liveIdx.alloc(2 * (size_t)cls_atoms);
        if (e == hipSuccess) e = s->d_liveNe.alloc(cls_atoms);
        if (e == hipSuccess) e = s->d_liveRho.alloc((size_t)cls_atoms * N);
        if (e == hipSuccess) e = s->d_liveU.alloc((size_t)cls_atoms * N);
        if (e != hipSuccess) {
            s->free_live();
            (void)hipGetLastError();
            return DFTA_OK;
        }
        s->live_cap = cls_atoms;
    }
    const int cap = s->live_cap;
    s->h_liveIdx.assign(2 * cap, 0);
    s->h_liveNe.assign(cap, 1.);
    for (int i = 0; i < cap; ++i) {
        const bool on = i < nlive;
        if (on) s->h_liveNe[i] = s->h_atoms[live_atoms[i]].nE;
        s->h_liveIdx[i] = on ? 0 : 1;
        s->h_liveIdx[cap + i] = on ? live_atoms[i] : 0;
    }
    DFTA_HIP(ctx, hipMemcpyAsync(s->d_liveIdx, s->h_liveIdx.data(), sizeof(int) * s->h_liveIdx.size(), hipMemcpyHostToDevice, st));
    DFTA_HIP(ctx, hipMemcpyAsync(s->d_liveNe, s->h_liveNe.data(), sizeof(double) * cap, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_gather_rows, dim3(std::min(256, (N + 255) / 256), nlive), dim3(256), 0, st, s->d_density.p, s->d_liveIdx + cap, N, s->d_liveRho.p);
    DFTA_CHECK_LAUNCH(ctx);
    *gathered = true;
    return DFTA_OK;
}

// The step's statistics into the caller's struct, which may be an older (shorter) or a newer (longer) one than this library's: fill this
// library's, hand over what both know.  solved_by: the multigrid solver that ran in this step.
static int scf_fill_stats(dfta_scf* s, const dfta::LevelStats& ls, dfta_poisson* solved_by, dfta_step_stats* user)
{
    dfta_ctx* ctx = s->ctx;
    const int user_size = user->struct_size;
    DFTA_REQUIRE(ctx, dfta::versioned_size_ok(user_size, dfta::kStatsMinSize), "dfta_step_stats::struct_size (set it to sizeof(dfta_step_stats) before the call)");
    dfta_step_stats mine;
    dfta_step_stats* const stats = &mine;
    DFTA_HIP(ctx, hipEventSynchronize(s->ev[3]));
    memset(stats, 0, sizeof(*stats));
    stats->struct_size = (int)sizeof(dfta_step_stats);
    stats->levels_fallbacks = (s->solver.scan_fallbacks + s->solver.persist_fallbacks) - s->fallbacks_seen;
    s->fallbacks_seen = s->solver.scan_fallbacks + s->solver.persist_fallbacks;
    DFTA_HIP(ctx, hipEventElapsedTime(&stats->ms_levels, s->ev[0], s->ev[1]));
    DFTA_HIP(ctx, hipEventElapsedTime(&stats->ms_poisson, s->ev[1], s->ev[2]));
    DFTA_HIP(ctx, hipEventElapsedTime(&stats->ms_tail, s->ev[2], s->ev[3]));
    stats->ms_poisson_kernel = stats->ms_poisson;
    stats->ms_sweep_kernels = ls.ms_sweep;
    stats->rounds = ls.rounds;
    stats->levels_layout = ls.layout;
    dfta_poisson_group_state(solved_by, &stats->poisson_groups, nullptr, nullptr);
    stats->sweeps_issued = ls.sweeps_issued;
    stats->points_traversed = ls.points_traversed;
    long ref = 0;
    long long pts = 0, skipped = 0;
    for (const auto& j : s->h_jobs) if (!j.frozen) {
        ref += j.n_count + j.n_zero + 1;   // + the matched solve of each level
        pts += j.n_points;
        if (j.nodes == 0) skipped += j.cur_len[1];     // the second bisection of a node-less level is pure arithmetic
        skipped += j.n_fixed;                            // a third bisection on its fixed point (walk_job)
    }
    stats->sweeps_reference = ref;
    stats->sweeps_reference_executed = ref - (long)skipped;
    stats->points_reference = (long)pts;
    unsigned long long vc = 0;
    int rc = dfta_poisson_take_vcycles(s->poisson, &vc);
    if (rc) return rc;
    for (auto& lv : s->live_solver) if (lv.p) {
        unsigned long long vl = 0;
        rc = dfta_poisson_take_vcycles(lv.p, &vl);
        if (rc) return rc;
        vc += vl;
    }
    stats->vcycles = (long)vc;
    dfta::copy_versioned(user, &mine, user_size, dfta::kStatsMinSize, sizeof(mine), user_size);
    return DFTA_OK;
}

int dfta_scf_step(dfta_scf* s, dfta_step_stats* stats)
{
    if (!s) return DFTA_ERR_INVALID;
    dfta_ctx* ctx = s->ctx;
    DFTA_ENTER(ctx);
    const dfta_grid* g = s->g;
    const int N = g->N, natoms = s->natoms;
    hipStream_t st = ctx->stream;
    const dim3 grid(std::min(64, (N + 255) / 256), natoms), block(256);

    DFTA_HIP(ctx, hipEventRecord(s->ev[0], st));
    DFTA_HIP(ctx, hipMemsetAsync(s->d_newDensity, 0, sizeof(double) * (size_t)s->nV * N, st));
    dfta::LevelStats ls;
    // bracket starts: every level solve starts from the bottoms planned at creation, -Z^2-1 (CHAINED hands E-3 from level to level inside
    // the solver, as DFTAtom.cpp:541; BATCHED clamps them to min Veff_l: LevelSolver::clamp_bottoms)
    // atoms that have met the reference's stop test (DFTAtom.cpp:474-479) are frozen: no level search, no mixing, no
    // Poisson solve, no new energies -- every atom of a batch ends in the state of its own last step
    bool any_frozen = false;
    for (int a = 0; a < natoms; ++a) {
        const AtomState& as = s->h_atoms[a];
        for (int k = as.job_off; k < as.job_end; ++k) s->h_frozen[k] = as.finished ? 1 : 0;
        any_frozen = any_frozen || as.finished;
    }
    int rc;
    {
        dfta_range r_levels("dfta: level search (LoopOverLevels: all subshells of the batch)");
        rc = s->solver.run(s->d_V, s->cfg.bottom.data(), s->solver.mode, s->d_newDensity, stats ? &ls : nullptr,
                           any_frozen ? s->h_frozen.data() : nullptr);
    }
    if (rc) return rc;
    {
        std::vector<dfta::Job>& jobs = s->h_jobs;
        rc = s->solver.fetch_jobs(jobs);
        if (rc) return rc;
        s->steps_done++;
        if (s->debug_levels) {
            for (size_t k = 0; k < jobs.size(); ++k)
                fprintf(stderr, "step %d job %zu n%d l%d: trust %d %d %d  len %d %d %d  pred_len %d %d %d  sweeps %d %d\n", s->steps_done, k, jobs[k].n,
                        jobs[k].l, jobs[k].trust[0], jobs[k].trust[1], jobs[k].trust[2], jobs[k].cur_len[0], jobs[k].cur_len[1],
                        jobs[k].cur_len[2], jobs[k].pred_len[0], jobs[k].pred_len[1], jobs[k].pred_len[2], jobs[k].n_count, jobs[k].n_zero);
        }
    }
    if (s->mixing == DFTA_MIX_ANDERSON) {
        rc = dfta_launch_anderson_mix(ctx, g, &s->anderson, s->lsda, natoms, s->alpha, 1. - s->alpha, s->d_newDensity.p, s->d_density.p, s->d_dA.p,
                                      s->d_dB.p, s->d_fin.p);
        if (rc) return rc;
    } else {
        rc = dfta_launch_linear_mix(ctx, g, s->lsda, natoms, s->alpha, 1. - s->alpha, s->d_newDensity.p, s->d_density.p, s->d_dA.p, s->d_dB.p,
                                    s->d_fin.p);
        if (rc) return rc;
    }
    DFTA_HIP(ctx, hipEventRecord(s->ev[1], st));
    // live atoms of this step (finished ones are frozen, see above) and the solver of their size class
    std::vector<int> live_atoms;
    for (int a = 0; a < natoms; ++a) if (!s->h_atoms[a].finished) live_atoms.push_back(a);
    const int nlive = static_cast<int>(live_atoms.size());
    int cls_atoms = 0;
    dfta_poisson* pl = scf_live_solver(s, nlive, &cls_atoms);
    bool use_live = false;
    if (pl) {
        rc = scf_gather_live(s, live_atoms, cls_atoms, &use_live);
        if (rc) return rc;
    }
    dfta_poisson* ps = use_live ? pl : s->poisson;
    {
        dfta_range r_poisson("dfta: multigrid Poisson solve (FullCycle)");
        const double* pNe = use_live ? s->d_liveNe : s->d_Ne;
        const double* pRho = use_live ? s->d_liveRho : s->d_density;
        double* pU = use_live ? s->d_liveU : s->d_U;
        const int* pSkip = use_live ? s->d_liveIdx : s->d_fin;
        rc = dfta_poisson_solve_launch(ps, pNe, pRho, pU, nullptr, nullptr, pSkip);
        if (rc) return rc;
        DFTA_HIP(ctx, hipEventRecord(s->ev[2], st));   // ev[1]..ev[2] brackets exactly the persistent multigrid kernel
        // synchronises and inspects the group barriers' abort flag on EVERY step; an aborted solve is repeated with one
        // workgroup per atom before anything reads U
        rc = dfta_poisson_finish(ps, pNe, pRho, pU, nullptr, nullptr, pSkip);
        if (rc) return rc;
        if (use_live) {
            hipLaunchKernelGGL(k_scatter_rows, dim3(std::min(256, (N + 255) / 256), nlive), dim3(256), 0, st, s->d_liveU.p, s->d_liveIdx + s->live_cap, N, s->d_U.p);
            DFTA_CHECK_LAUNCH(ctx);
        }
    }
    dfta_range r_tail("dfta: XC + integrands + ordered integrals + energies");
    const bool kli = s->exchange_mode == DFTA_EXCHANGE_KLI;
    const bool sic = s->exchange_mode == DFTA_EXCHANGE_SIC_KLI;
    rc = kli ? scf_exchange_stage(s) : scf_xc(s);
    if (rc) return rc;
    if (sic) {
        rc = scf_exchange_stage(s);
        if (rc) return rc;
    }
    hipLaunchKernelGGL(k_tail, grid, block, 0, st, s->d_atoms.p, s->lsda, N, g->d_r, g->d_cnst, s->d_density.p, s->d_dA.p, s->d_dB.p, s->d_U.p,
                       s->d_Vexc.p, s->d_va.p, s->d_vb.p, s->d_eexc.p, s->d_V.p, s->d_integrands.p, g->uniform);
    DFTA_CHECK_LAUNCH(ctx);
    // Simpson38(1, .) on the logarithmic grid (DFTAtom.cpp:459-467), Simpson38(h, .) on the uniform one (DFTAtom.cpp:167-177)
    // (tolerance mode of the sweeps: the two sums of Simpson 3/8 in parallel, as the normalisation integral of scan_match takes them --
    // 0.44 ms of ordered additions per step otherwise; the energies move by a few 1e-16 relative)
    if (s->solver.sweep_mode == DFTA_SWEEPS_TOLERANCE && s->solver.integ_rule == DFTA_INT_SIMPSON38 && !dfta_knob("SCF_ORDERED_SUMS"))
        rc = dfta_launch_integrate_simpson38_parallel(ctx, dfta_hstep(g), s->d_integrands, N, natoms * 5, (size_t)N, s->d_integrals);
    else
        rc = dfta_launch_integrate_ordered(ctx, s->solver.integ_rule, dfta_hstep(g), s->d_integrands, N, natoms * 5, (size_t)N, s->d_integrals);
    if (rc) return rc;
    hipLaunchKernelGGL(k_energies, dim3((natoms + 63) / 64), dim3(64), 0, st, s->d_atoms.p, natoms, s->solver.d_jobs.p, s->solver.d_occ.p, s->d_integrals.p,
                       s->d_records.p, s->d_fin.p, kli || sic ? s->kli.d_ExAtom.p : nullptr);
    DFTA_CHECK_LAUNCH(ctx);
    DFTA_HIP(ctx, hipEventRecord(s->ev[3], st));
    // the step ends synchronised with the atoms' state on the host: the next step freezes what has finished
    DFTA_HIP(ctx, hipMemcpyAsync(s->h_atoms.data(), s->d_atoms, sizeof(AtomState) * natoms, hipMemcpyDeviceToHost, st));
    DFTA_HIP(ctx, hipStreamSynchronize(st));
    if (kli || sic)
        for (int c = 0; c < s->nV; ++c)
            DFTA_REQUIRE(ctx, !(s->h_live_ch[c] && s->kli.h_status[c]), "exchange stage: the KLI system of a channel is singular or not finite");
    return stats ? scf_fill_stats(s, ls, ps, stats) : DFTA_OK;
}

}  // extern "C"
