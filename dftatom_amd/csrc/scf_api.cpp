// scf_api.cpp -- the read-only C ABI of the SCF layer (include/dftatom_hip.h): the accessors of a batch's state (scf_state.h) and the
// post-SCF analysis entries on its orbitals and densities (orbitals.hip, slater.hip, exchange.hip, bessel.hip, continuum.hip).  Host code only: what runs on the device is launched through the
// dfta_launch_* helpers (internal.h).  What an entry accepts and rejects is its own and stays in the entry.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <vector>

#include "bessel_plan.h"
#include "continuum_plan.h"
#include "exchange_plan.h"
#include "pseudo_plan.h"
#include "scf_state.h"
#include "slater_plan.h"
#include "xc.h"             // dfta_poisson_group_state

extern "C" {

int dfta_scf_get_energies(dfta_scf* s, dfta_energies* e, int* finished)
{
    if (!s) return DFTA_ERR_INVALID;
    dfta_ctx* ctx = s->ctx;
    DFTA_ENTER(ctx);
    for (int a = 0; a < s->natoms; ++a) {      // h_atoms is current: every step ends with its copy
        if (e) e[a] = s->h_atoms[a].e;
        if (finished) finished[a] = s->h_atoms[a].finished;
    }
    return DFTA_OK;
}

int dfta_scf_info(const dfta_scf* s, int* tree_depth, int* njobs, long* trials_per_round)
{
    if (!s) return DFTA_ERR_INVALID;
    if (tree_depth) *tree_depth = s->solver.depth;
    if (njobs) *njobs = s->solver.njobs;
    if (trials_per_round) *trials_per_round = s->solver.ntrials;
    return DFTA_OK;
}

int dfta_scf_set_integrator(dfta_scf* s, int rule)
{
    if (!s) return DFTA_ERR_INVALID;
    DFTA_REQUIRE(s->ctx, dfta_integral_shape_ok(rule, s->g->N), "integration rule / grid size");
    s->solver.integ_rule = rule;
    return DFTA_OK;
}

int dfta_scf_poisson_info(const dfta_scf* s, int* G, int* degraded, int* aborts)
{
    if (!s) return DFTA_ERR_INVALID;
    return dfta_poisson_group_state(s->poisson, G, degraded, aborts);
}

int dfta_scf_num_levels(const dfta_scf* s, int atom, int spin)
{
    if (!s || atom < 0 || atom >= s->natoms || spin < 0 || spin > 1) return -1;
    return s->cfg.nlev[spin][atom];
}

int dfta_scf_get_levels(dfta_scf* s, int atom, int spin, int* n, int* l, int* occ, double* E, int* converged)
{
    if (!s) return DFTA_ERR_INVALID;
    dfta_ctx* ctx = s->ctx;
    DFTA_ENTER(ctx);
    DFTA_REQUIRE(ctx, atom >= 0 && atom < s->natoms && spin >= 0 && spin < s->nspin, "atom/spin");
    const std::vector<dfta::Job>& jobs = s->h_jobs;
    DFTA_REQUIRE(ctx, !jobs.empty(), "no SCF step has run yet");
    const auto [k0, cnt] = s->channel(atom, spin);
    if (occ)                                     // the whole channel is checked before anything is written
        for (int k = 0; k < cnt; ++k) {
            const double o = s->solver.h_occ[k0 + k];
            DFTA_REQUIRE(ctx, o == std::floor(o), "a fractional occupation: read it with dfta_scf_get_occupations");
        }
    for (int k = 0; k < cnt; ++k) {
        const dfta::Job& j = jobs[k0 + k];
        if (n) n[k] = j.n;
        if (l) l[k] = j.l;
        if (occ) occ[k] = static_cast<int>(s->solver.h_occ[k0 + k]);
        if (E) E[k] = j.E;
        if (converged) converged[k] = j.converged;
    }
    return DFTA_OK;
}

int dfta_scf_get_occupations(dfta_scf* s, int atom, int spin, double* occ)
{
    if (!s) return DFTA_ERR_INVALID;
    dfta_ctx* ctx = s->ctx;
    DFTA_ENTER(ctx);
    DFTA_REQUIRE(ctx, atom >= 0 && atom < s->natoms && spin >= 0 && spin < s->nspin && occ, "atom/spin/occ");
    const auto [k0, cnt] = s->channel(atom, spin);
    for (int k = 0; k < cnt; ++k) occ[k] = s->solver.h_occ[k0 + k];
    return DFTA_OK;
}

int dfta_scf_get_level_status(dfta_scf* s, int atom, int spin, int* status, int* n_count, int* n_zero)
{
    if (!s) return DFTA_ERR_INVALID;
    dfta_ctx* ctx = s->ctx;
    DFTA_ENTER(ctx);
    DFTA_REQUIRE(ctx, atom >= 0 && atom < s->natoms && spin >= 0 && spin < s->nspin, "atom/spin");
    const std::vector<dfta::Job>& jobs = s->h_jobs;
    DFTA_REQUIRE(ctx, !jobs.empty(), "no SCF step has run yet");
    const auto [k0, cnt] = s->channel(atom, spin);
    for (int k = 0; k < cnt; ++k) {
        if (status) status[k] = jobs[k0 + k].status;
        if (n_count) n_count[k] = jobs[k0 + k].n_count;
        if (n_zero) n_zero[k] = jobs[k0 + k].n_zero;
    }
    return DFTA_OK;
}

int dfta_scf_get_array(dfta_scf* s, int atom, int which, double* out)
{
    if (!s) return DFTA_ERR_INVALID;
    dfta_ctx* ctx = s->ctx;
    DFTA_ENTER(ctx);
    DFTA_REQUIRE(ctx, atom >= 0 && atom < s->natoms && out, "atom/out");
    const int N = s->g->N;
    const double* src = nullptr;
    switch (which) {
    case 0: src = s->d_density + (size_t)atom * N; break;
    case 1: src = (s->lsda ? s->d_dA : s->d_density) + (size_t)atom * N; break;
    case 2: src = (s->lsda ? s->d_dB : s->d_density) + (size_t)atom * N; break;
    case 3: src = s->d_V + (size_t)atom * s->nspin * N; break;
    case 4: src = s->d_V + ((size_t)atom * s->nspin + (s->lsda ? 1 : 0)) * N; break;
    case 5: src = s->d_U + (size_t)atom * N; break;
    default: DFTA_REQUIRE(ctx, false, "which");
    }
    DFTA_HIP(ctx, hipMemcpyAsync(out, src, sizeof(double) * N, hipMemcpyDeviceToHost, ctx->stream));
    DFTA_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return DFTA_OK;
}

// ---- the orbitals of the last step (they exist once a step has run) -------------------------------------------------------------------
int dfta_scf_get_orbitals(dfta_scf* s, int atom, int spin, double* u)
{
    if (!s) return DFTA_ERR_INVALID;
    dfta_ctx* ctx = s->ctx;
    DFTA_ENTER(ctx);
    DFTA_REQUIRE(ctx, s->steps_done > 0, "no SCF step has run yet: there are no orbitals");
    DFTA_REQUIRE(ctx, atom >= 0 && atom < s->natoms && spin >= 0 && spin < s->nspin, "atom/spin");
    const auto [k0, cnt] = s->channel(atom, spin);
    DFTA_REQUIRE(ctx, u || cnt == 0, "u");
    if (cnt == 0) return DFTA_OK;
    const size_t N = s->g->N;
    DFTA_HIP(ctx, hipMemcpyAsync(u, s->solver.d_Psi + (size_t)k0 * N, sizeof(double) * cnt * N, hipMemcpyDeviceToHost, ctx->stream));
    DFTA_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return DFTA_OK;
}

int dfta_scf_orbital_properties(dfta_scf* s, double* props)
{
    if (!s) return DFTA_ERR_INVALID;
    dfta_ctx* ctx = s->ctx;
    DFTA_ENTER(ctx);
    DFTA_REQUIRE(ctx, s->steps_done > 0, "no SCF step has run yet: there are no orbitals");
    DFTA_REQUIRE(ctx, props, "props");
    const int njobs = s->solver.njobs;
    hipStream_t st = ctx->stream;
    if (!s->d_orb_props.p) {                  // first use: the levels' l and the result rows
        std::vector<int> hl(njobs);
        for (int k = 0; k < njobs; ++k) hl[k] = s->h_jobs[k].l;
        DFTA_HIP(ctx, s->d_orb_l.alloc(njobs));
        DFTA_HIP(ctx, hipMemcpyAsync(s->d_orb_l.p, hl.data(), sizeof(int) * njobs, hipMemcpyHostToDevice, st));
        DFTA_HIP(ctx, hipStreamSynchronize(st));          // hl is the source of the copy
        DFTA_HIP(ctx, s->d_orb_props.alloc((size_t)njobs * DFTA_ORB_PROPS));
    }
    const int rc = dfta_launch_orbital_properties(ctx, s->g, njobs, s->d_orb_l.p, s->solver.d_Psi.p, s->d_orb_props.p);
    if (rc) return rc;
    DFTA_HIP(ctx, hipMemcpyAsync(props, s->d_orb_props.p, sizeof(double) * njobs * DFTA_ORB_PROPS, hipMemcpyDeviceToHost, st));
    DFTA_HIP(ctx, hipStreamSynchronize(st));
    return DFTA_OK;
}

int dfta_scf_orbital_matrix(dfta_scf* s, int atom, int spin, int k, double* M)
{
    if (!s) return DFTA_ERR_INVALID;
    dfta_ctx* ctx = s->ctx;
    DFTA_ENTER(ctx);
    DFTA_REQUIRE(ctx, s->steps_done > 0, "no SCF step has run yet: there are no orbitals");
    DFTA_REQUIRE(ctx, atom >= 0 && atom < s->natoms && spin >= 0 && spin < s->nspin, "atom/spin");
    const auto [k0, cnt] = s->channel(atom, spin);
    DFTA_REQUIRE(ctx, k >= 0 && k <= 2, "k (0, 1 or 2)");
    DFTA_REQUIRE(ctx, M || cnt == 0, "M");
    if (cnt == 0) return DFTA_OK;
    if (!s->orb_scratch.norb_max) {           // first use: scratch for the longest channel of the batch
        int most = 1;
        for (int a = 0; a < s->natoms; ++a) most = std::max(most, std::max(s->cfg.nlev[0][a], s->cfg.nlev[1][a]));
        const int rc = dfta_orbital_scratch_create(ctx, s->g, most, &s->orb_scratch);
        if (rc) return rc;
    }
    hipStream_t st = ctx->stream;
    const int rc = dfta_launch_orbital_matrix(ctx, s->g, cnt, s->solver.d_Psi + (size_t)k0 * s->g->N, k, s->orb_scratch.slab.p,
                                              s->orb_scratch.ticket.p, s->orb_scratch.M.p);
    if (rc) return rc;
    DFTA_HIP(ctx, hipMemcpyAsync(M, s->orb_scratch.M.p, sizeof(double) * cnt * cnt, hipMemcpyDeviceToHost, st));
    DFTA_HIP(ctx, hipStreamSynchronize(st));
    return DFTA_OK;
}

// ---- Slater integrals of the SCF's orbitals (slater.hip; the orbitals are read in place) ---------------------------------------------
int dfta_scf_slater_rk(dfta_scf* s, int atom, int njobs, const int* jobs, double* R)
{
    if (!s) return DFTA_ERR_INVALID;
    dfta_ctx* ctx = s->ctx;
    DFTA_ENTER(ctx);
    DFTA_REQUIRE(ctx, s->steps_done > 0, "no SCF step has run yet: there are no orbitals");
    DFTA_REQUIRE(ctx, atom >= 0 && atom < s->natoms, "atom");
    DFTA_REQUIRE(ctx, s->g->N >= 5, "Slater integrals need a grid of 5 nodes");
    const auto [k0, norb] = s->atom_jobs(atom);
    DFTA_REQUIRE(ctx, njobs >= 0, "njobs");
    if (njobs == 0) return DFTA_OK;
    DFTA_REQUIRE(ctx, jobs && R, "jobs / R");
    if (const char* msg = dfta_slater::check_jobs(norb, njobs, jobs)) DFTA_REQUIRE(ctx, false, msg);
    return s->slater.run(ctx, s->g, s->solver.d_Psi + (size_t)k0 * s->g->N, njobs, jobs, R);
}

int dfta_scf_slater_fg(dfta_scf* s, int atom, int spin, double* F, double* G)
{
    if (!s) return DFTA_ERR_INVALID;
    dfta_ctx* ctx = s->ctx;
    DFTA_ENTER(ctx);
    DFTA_REQUIRE(ctx, s->steps_done > 0, "no SCF step has run yet: there are no orbitals");
    DFTA_REQUIRE(ctx, atom >= 0 && atom < s->natoms, "atom");
    DFTA_REQUIRE(ctx, s->g->N >= 5, "Slater integrals need a grid of 5 nodes");
    DFTA_REQUIRE(ctx, spin >= 0 && spin < s->nspin, "spin");
    const auto [c0, cnt] = s->channel(atom, spin);
    DFTA_REQUIRE(ctx, (F && G) || cnt == 0, "F / G");
    if (cnt == 0) return DFTA_OK;
    std::vector<int> l(cnt);
    for (int a = 0; a < cnt; ++a) l[a] = s->h_jobs[c0 + a].l;
    const int njobs = dfta_slater::fg_jobs(cnt, l.data(), nullptr, nullptr);
    DFTA_REQUIRE(ctx, njobs >= 0, "Slater table: an orbital with l > 4");
    std::vector<int> jobs((size_t)njobs * dfta_slater::kJobInts), kinds(njobs);
    std::vector<double> R(njobs);
    dfta_slater::fg_jobs(cnt, l.data(), jobs.data(), kinds.data());
    const int rc = s->slater.run(ctx, s->g, s->solver.d_Psi + (size_t)c0 * s->g->N, njobs, jobs.data(), R.data());
    if (rc) return rc;
    const size_t plane = (size_t)cnt * cnt;
    std::fill(F, F + (DFTA_SLATER_KMAX + 1) * plane, 0.);
    std::fill(G, G + (DFTA_SLATER_KMAX + 1) * plane, 0.);
    for (int j = 0; j < njobs; ++j) {             // each value once, mirrored; G^k(a,a) is F^k(a,a)
        const int a = jobs[(size_t)j * dfta_slater::kJobInts], b = jobs[(size_t)j * dfta_slater::kJobInts + 1];
        const int k = jobs[(size_t)j * dfta_slater::kJobInts + 4];
        double* T = kinds[j] == dfta_slater::kKindF ? F : G;
        T[k * plane + (size_t)a * cnt + b] = T[k * plane + (size_t)b * cnt + a] = R[j];
        if (a == b) G[k * plane + (size_t)a * cnt + a] = R[j];
    }
    return DFTA_OK;
}

int dfta_scf_coulomb_exchange(dfta_scf* s, int atom, double* EH, double* EXX)
{
    if (!s) return DFTA_ERR_INVALID;
    dfta_ctx* ctx = s->ctx;
    DFTA_ENTER(ctx);
    DFTA_REQUIRE(ctx, s->steps_done > 0, "no SCF step has run yet: there are no orbitals");
    DFTA_REQUIRE(ctx, atom >= 0 && atom < s->natoms, "atom");
    DFTA_REQUIRE(ctx, s->g->N >= 5, "Slater integrals need a grid of 5 nodes");
    const auto [k0, norb] = s->atom_jobs(atom);
    DFTA_REQUIRE(ctx, EH && EXX, "EH / EXX");
    std::vector<int> l(norb);
    for (int a = 0; a < norb; ++a) l[a] = s->h_jobs[k0 + a].l;
    dfta_slater::EnergyPlan plan;
    DFTA_REQUIRE(ctx, dfta_slater::plan_energy(s->cfg.nlev[0][atom], s->cfg.nlev[1][atom], l.data(), &plan) == 0,
                 "exchange energy: an orbital with l > 4");
    std::vector<double> R(plan.njobs());
    const int rc = s->slater.run(ctx, s->g, s->solver.d_Psi + (size_t)k0 * s->g->N, plan.njobs(), plan.jobs.data(), R.data());
    if (rc) return rc;
    dfta_slater::energy_sums(plan, s->solver.h_occ.data() + k0, s->lsda, R.data(), EH, EXX);
    return DFTA_OK;
}

// ---- screening functions and exchange potentials of the SCF's orbitals (exchange.hip; the orbitals are read in place) -----------------
int dfta_scf_screening_yk(dfta_scf* s, int atom, int njobs, const int* jobs, double* y)
{
    if (!s) return DFTA_ERR_INVALID;
    dfta_ctx* ctx = s->ctx;
    DFTA_ENTER(ctx);
    DFTA_REQUIRE(ctx, s->steps_done > 0, "no SCF step has run yet: there are no orbitals");
    DFTA_REQUIRE(ctx, atom >= 0 && atom < s->natoms, "atom");
    DFTA_REQUIRE(ctx, s->g->N >= 5, "screening functions need a grid of 5 nodes");
    const auto [k0, norb] = s->atom_jobs(atom);
    DFTA_REQUIRE(ctx, njobs >= 0, "njobs");
    if (njobs == 0) return DFTA_OK;
    DFTA_REQUIRE(ctx, jobs && y, "jobs / y");
    if (const char* msg = dfta_exchange::check_jobs(norb, njobs, jobs)) DFTA_REQUIRE(ctx, false, msg);
    return s->exchange.run_yk(ctx, s->g, s->solver.d_Psi + (size_t)k0 * s->g->N, njobs, jobs, y);
}

int dfta_scf_exchange_potentials(dfta_scf* s, int atom, int spin, double* X, double* D, double* vS, double* vKLI, double* vbar, double* M,
                                 int* homo)
{
    if (!s) return DFTA_ERR_INVALID;
    dfta_ctx* ctx = s->ctx;
    DFTA_ENTER(ctx);
    DFTA_REQUIRE(ctx, s->steps_done > 0, "no SCF step has run yet: there are no orbitals");
    DFTA_REQUIRE(ctx, atom >= 0 && atom < s->natoms && spin >= 0 && spin < s->nspin, "atom/spin");
    DFTA_REQUIRE(ctx, s->g->N >= 5, "exchange potentials need a grid of 5 nodes");
    const auto [c0, cnt] = s->channel(atom, spin);
    if (cnt == 0) {
        if (homo) *homo = -1;
        return DFTA_OK;
    }
    std::vector<int> l(cnt);
    std::vector<double> occ(cnt), E(cnt);
    for (int a = 0; a < cnt; ++a) {
        l[a] = s->h_jobs[c0 + a].l;
        E[a] = s->h_jobs[c0 + a].E;
        occ[a] = s->lsda ? s->solver.h_occ[c0 + a] : 0.5 * s->solver.h_occ[c0 + a];
    }
    const int h = dfta_exchange::pick_homo(cnt, E.data(), occ.data());
    if (const char* msg = dfta_exchange::check_channel(cnt, l.data(), occ.data(), h)) DFTA_REQUIRE(ctx, false, msg);
    dfta_exchange::ChannelPlan plan;
    DFTA_REQUIRE(ctx, dfta_exchange::plan_channel(cnt, l.data(), occ.data(), &plan) == 0, "exchange potentials: the channel");
    const int rc = s->exchange.run_potentials(ctx, s->g, s->solver.d_Psi + (size_t)c0 * s->g->N, plan, occ.data(), h, X, D, vS, vKLI, vbar, M);
    if (rc) return rc;
    if (homo) *homo = h;
    return DFTA_OK;
}

// ---- self-consistent exchange-only KLI: the switch and the accessors of the batched exchange stage (kli_stage.hip) -------------------
int dfta_scf_set_exchange(dfta_scf* s, int exchange)
{
    if (!s) return DFTA_ERR_INVALID;
    dfta_ctx* ctx = s->ctx;
    DFTA_ENTER(ctx);
    DFTA_REQUIRE(ctx, s->steps_done == 0, "dfta_scf_set_exchange: after the first step");
    DFTA_REQUIRE(ctx, exchange == DFTA_EXCHANGE_FUNCTIONAL || exchange == DFTA_EXCHANGE_KLI || exchange == DFTA_EXCHANGE_SIC_KLI,
                 "exchange (DFTA_EXCHANGE_FUNCTIONAL or DFTA_EXCHANGE_KLI or DFTA_EXCHANGE_SIC_KLI)");
    const bool sic = exchange == DFTA_EXCHANGE_SIC_KLI;
    if (exchange == DFTA_EXCHANGE_FUNCTIONAL) {
        s->kli.reset();
        s->exchange_mode = exchange;
        return DFTA_OK;
    }
    if (sic) {
        DFTA_REQUIRE(ctx, s->functional == DFTA_XC_VWN, "DFTA_EXCHANGE_SIC_KLI: functional must be DFTA_XC_VWN (the correction is VWN's)");
        DFTA_REQUIRE(ctx, s->mixing == DFTA_MIX_LINEAR, "DFTA_EXCHANGE_SIC_KLI: mixing must be DFTA_MIX_LINEAR");
    } else {
        DFTA_REQUIRE(ctx, s->functional == DFTA_XC_VWN, "DFTA_EXCHANGE_KLI: functional must be DFTA_XC_VWN (exchange-only: no correlation is added)");
        DFTA_REQUIRE(ctx, s->mixing == DFTA_MIX_LINEAR, "DFTA_EXCHANGE_KLI: mixing must be DFTA_MIX_LINEAR");
    }
    if (s->exchange_mode == exchange) return DFTA_OK;
    s->kli.reset();                          // from the other orbital-dependent value: its tables go
    s->exchange_mode = DFTA_EXCHANGE_FUNCTIONAL;
    // the channels of the batch, atom-major, nspin per atom; occupations N_a (LSDA) or N_a / 2 (LDA)
    std::vector<int> norb, atom, l;
    std::vector<double> occ;
    for (int a = 0; a < s->natoms; ++a)
        for (int sp = 0; sp < s->nspin; ++sp) {
            const auto [k0, cnt] = s->channel(a, sp);
            DFTA_REQUIRE(ctx, k0 == (int)l.size(), "DFTA_EXCHANGE_KLI: the batch's levels are not laid out channel by channel");
            norb.push_back(cnt);
            atom.push_back(a);
            for (int k = 0; k < cnt; ++k) {
                l.push_back(s->cfg.specs[k0 + k].l);
                occ.push_back(s->lsda ? s->solver.h_occ[k0 + k] : 0.5 * s->solver.h_occ[k0 + k]);
            }
        }
    const int rc = s->kli.create(ctx, s->g, s->nV, norb.data(), l.data(), occ.data(), atom.data(), s->natoms, s->kli_y_mb, sic);
    if (rc) return rc;
    s->exchange_mode = exchange;
    return DFTA_OK;
}

int dfta_scf_get_exchange(dfta_scf* s, int atom, int spin, double* vx, double* v_raw, double* Ex)
{
    if (!s) return DFTA_ERR_INVALID;
    dfta_ctx* ctx = s->ctx;
    DFTA_ENTER(ctx);
    DFTA_REQUIRE(ctx, s->exchange_mode == DFTA_EXCHANGE_KLI || s->exchange_mode == DFTA_EXCHANGE_SIC_KLI,
                 "dfta_scf_get_exchange: the exchange switch is not DFTA_EXCHANGE_KLI or DFTA_EXCHANGE_SIC_KLI");
    DFTA_REQUIRE(ctx, s->steps_done > 0, "no SCF step has run yet: there is no exchange potential");
    DFTA_REQUIRE(ctx, atom >= 0 && atom < s->natoms && spin >= 0 && spin < s->nspin, "atom/spin");
    const size_t N = s->g->N, c = (size_t)atom * s->nspin + spin;
    hipStream_t st = ctx->stream;
    if (vx) DFTA_HIP(ctx, hipMemcpyAsync(vx, s->kli.d_vx.p + c * N, sizeof(double) * N, hipMemcpyDeviceToHost, st));
    if (v_raw) DFTA_HIP(ctx, hipMemcpyAsync(v_raw, s->kli.d_vraw.p + c * N, sizeof(double) * N, hipMemcpyDeviceToHost, st));
    if (Ex) DFTA_HIP(ctx, hipMemcpyAsync(Ex, s->kli.d_ExAtom.p + atom, sizeof(double), hipMemcpyDeviceToHost, st));
    DFTA_HIP(ctx, hipStreamSynchronize(st));
    return DFTA_OK;
}

int dfta_scf_exchange_ms(dfta_scf* s, float* ms)
{
    if (!s) return DFTA_ERR_INVALID;
    dfta_ctx* ctx = s->ctx;
    DFTA_ENTER(ctx);
    DFTA_REQUIRE(ctx, ms, "ms");
    DFTA_REQUIRE(ctx, s->exchange_mode != DFTA_EXCHANGE_FUNCTIONAL && s->kli.timed, "dfta_scf_exchange_ms: no exchange stage has run");
    DFTA_HIP(ctx, hipEventElapsedTime(ms, s->kli.ev[0], s->kli.ev[1]));
    return DFTA_OK;
}

int dfta_scf_sic_table(dfta_scf* s, int atom, int spin, double* EH, double* EXC, double* vbar, double* c, int* homo)
{
    if (!s) return DFTA_ERR_INVALID;
    dfta_ctx* ctx = s->ctx;
    DFTA_ENTER(ctx);
    DFTA_REQUIRE(ctx, s->exchange_mode == DFTA_EXCHANGE_SIC_KLI, "dfta_scf_sic_table: the exchange switch is not DFTA_EXCHANGE_SIC_KLI");
    DFTA_REQUIRE(ctx, s->steps_done > 0, "no SCF step has run yet: there is no SIC table");
    DFTA_REQUIRE(ctx, atom >= 0 && atom < s->natoms && spin >= 0 && spin < s->nspin, "atom/spin");
    const auto rows = s->channel(atom, spin);
    const int k0 = rows.k0, cnt = rows.cnt;
    const size_t ch = (size_t)atom * s->nspin + spin;
    hipStream_t st = ctx->stream;
    auto get = [&](double* dst, const double* src) {
        return dst && cnt > 0 ? hipMemcpyAsync(dst, src + k0, sizeof(double) * cnt, hipMemcpyDeviceToHost, st) : hipSuccess;
    };
    DFTA_HIP(ctx, get(EH, s->kli.d_EH.p));
    DFTA_HIP(ctx, get(EXC, s->kli.d_EXC.p));
    DFTA_HIP(ctx, get(vbar, s->kli.d_vbarHF.p));
    DFTA_HIP(ctx, get(c, s->kli.d_c.p));
    if (homo) DFTA_HIP(ctx, hipMemcpyAsync(homo, s->kli.d_homo.p + ch, sizeof(int), hipMemcpyDeviceToHost, st));
    DFTA_HIP(ctx, hipStreamSynchronize(st));
    return DFTA_OK;
}

// ---- Bessel transforms of the SCF's arrays(bessel.hip; densities and orbitals are read in place) -------------------------------------
int dfta_scf_form_factors(dfta_scf* s, int nq, const double* q, double* out)
{
    if (!s) return DFTA_ERR_INVALID;
    dfta_ctx* ctx = s->ctx;
    DFTA_ENTER(ctx);
    DFTA_REQUIRE(ctx, nq >= 0, "dfta_scf_form_factors: nq");
    if (nq == 0) return DFTA_OK;
    DFTA_REQUIRE(ctx, q && out, "dfta_scf_form_factors: q / out");
    DFTA_REQUIRE(ctx, s->g->N >= 5, "form factors need a grid of 5 nodes");
    const size_t N = s->g->N;
    const int nchan = s->lsda ? 3 : 1, nrow = s->natoms * nchan;
    std::vector<int> l(nrow, 0);
    std::vector<const double*> rows(nrow);
    for (int a = 0; a < s->natoms; ++a) {            // the arrays dfta_scf_get_array(.., 0 / 1 / 2) returns
        rows[(size_t)a * nchan] = s->d_density + a * N;
        if (s->lsda) { rows[(size_t)a * nchan + 1] = s->d_dA + a * N; rows[(size_t)a * nchan + 2] = s->d_dB + a * N; }
    }
    if (const char* msg = dfta_bessel::check_transform(DFTA_BT_DENSITY, nrow, l.data(), nq, q)) DFTA_REQUIRE(ctx, false, msg);
    return s->bessel.run(ctx, s->g, DFTA_BT_DENSITY, nrow, l.data(), rows.data(), nq, q, out);
}

int dfta_scf_momentum_orbitals(dfta_scf* s, int nq, const double* q, double* out)
{
    if (!s) return DFTA_ERR_INVALID;
    dfta_ctx* ctx = s->ctx;
    DFTA_ENTER(ctx);
    DFTA_REQUIRE(ctx, s->steps_done > 0, "no SCF step has run yet: there are no orbitals");
    DFTA_REQUIRE(ctx, nq >= 0, "dfta_scf_momentum_orbitals: nq");
    if (nq == 0) return DFTA_OK;
    DFTA_REQUIRE(ctx, q && out, "dfta_scf_momentum_orbitals: q / out");
    DFTA_REQUIRE(ctx, s->g->N >= 5, "momentum orbitals need a grid of 5 nodes");
    const size_t N = s->g->N;
    const int njobs = s->solver.njobs;
    std::vector<int> l(njobs);
    std::vector<const double*> rows(njobs);
    for (int k = 0; k < njobs; ++k) {                // rows as dfta_scf_orbital_properties lists them
        l[k] = s->h_jobs[k].l;
        rows[k] = s->solver.d_Psi + k * N;
    }
    if (const char* msg = dfta_bessel::check_transform(DFTA_BT_ORBITAL, njobs, l.data(), nq, q)) DFTA_REQUIRE(ctx, false, msg);
    return s->bessel.run(ctx, s->g, DFTA_BT_ORBITAL, njobs, l.data(), rows.data(), nq, q, out);
}

// ---- continuum orbitals in the batch's resident potentials (continuum.hip; potentials and orbitals are read in place) ----------------------
namespace {

// the partner lists of dfta_scf_continuum: one per (channel, l) in use, the channel's levels with l_b = l +- 1 (power 1) or l_b = l
struct ContLists {
    std::vector<int> off{0}, rows, trial_list;
    std::vector<int> key;                // per list: channel * 5 + l
};
const char* scf_cont_lists(const dfta_scf* s, int ntrials, const int* atom, const int* spin, const int* l, int power, ContLists* out)
{
    out->trial_list.assign(ntrials, -1);
    for (int t = 0; t < ntrials; ++t) {
        const int key = (atom[t] * s->nspin + spin[t]) * (dfta_continuum_plan::kLmax + 1) + l[t];
        int list = (int)(std::find(out->key.begin(), out->key.end(), key) - out->key.begin());
        if (list == (int)out->key.size()) {
            const auto [k0, cnt] = s->channel(atom[t], spin[t]);
            for (int k = 0; k < cnt; ++k) {
                const int lb = s->h_jobs[k0 + k].l;
                if (power == 1 ? (lb == l[t] - 1 || lb == l[t] + 1) : lb == l[t]) out->rows.push_back(k0 + k);
            }
            if ((int)out->rows.size() - out->off.back() > dfta_continuum_plan::kMaxPartners) return "continuum: more than 16 partners in a list";
            out->off.push_back((int)out->rows.size());
            out->key.push_back(key);
        }
        out->trial_list[t] = list;
    }
    return nullptr;
}

}  // namespace

int dfta_scf_continuum(dfta_scf* s, int norm_mode, int ntrials, const int* atom, const int* spin, const int* l, const double* E,
                       const int* m, int power, double* logderiv, int* nodes, double* delta_or_phase, double* scale, int* status,
                       double* sums, int* partner_index, double* rows)
{
    if (!s) return DFTA_ERR_INVALID;
    dfta_ctx* ctx = s->ctx;
    DFTA_ENTER(ctx);
    DFTA_REQUIRE(ctx, ntrials >= 0, "dfta_scf_continuum: ntrials");
    if (ntrials == 0) return DFTA_OK;
    DFTA_REQUIRE(ctx, atom && spin && l && E && m, "dfta_scf_continuum arguments");
    DFTA_REQUIRE(ctx, power < 0 || s->steps_done > 0, "no SCF step has run yet: there are no orbitals");
    std::vector<int> vidx(ntrials);
    for (int t = 0; t < ntrials; ++t) {
        DFTA_REQUIRE(ctx, atom[t] >= 0 && atom[t] < s->natoms && spin[t] >= 0 && spin[t] < s->nspin, "dfta_scf_continuum: atom/spin");
        DFTA_REQUIRE(ctx, l[t] >= 0 && l[t] <= dfta_continuum_plan::kLmax, "continuum: l outside 0 .. 4");
        vidx[t] = atom[t] * s->nspin + spin[t];
    }
    ContLists lists;
    if (power >= 0)
        if (const char* msg = scf_cont_lists(s, ntrials, atom, spin, l, power, &lists)) DFTA_REQUIRE(ctx, false, msg);
    dfta_continuum_plan::Call c;
    c.norm_mode = norm_mode; c.N = s->g->N; c.nV = s->natoms * s->nspin; c.ntrials = ntrials;
    c.vidx = vidx.data(); c.l = l; c.E = E; c.m = m;
    c.npartner_rows = power >= 0 ? s->solver.njobs : 0; c.power = power >= 0 ? power : 0;
    c.nlists = power >= 0 ? (int)lists.key.size() : 0;
    c.list_off = lists.off.data(); c.list_rows = lists.rows.data(); c.trial_list = power >= 0 ? lists.trial_list.data() : nullptr;
    if (const char* msg = dfta_continuum_plan::check(c)) DFTA_REQUIRE(ctx, false, msg);
    dfta_continuum_out out;
    out.logderiv = logderiv; out.nodes = nodes; out.delta_or_phase = delta_or_phase; out.scale = scale; out.status = status;
    out.sums = power >= 0 ? sums : nullptr; out.rows = rows;
    if (const int rc = dfta_continuum_run(ctx, s->g, c, s->d_V, power >= 0 ? s->solver.d_Psi.p : nullptr, out)) return rc;
    if (partner_index && power >= 0)
        for (int t = 0; t < ntrials; ++t) {
            const int list = lists.trial_list[t], k0 = s->channel(atom[t], spin[t]).k0;
            for (int q = 0; q < dfta_continuum_plan::kMaxPartners; ++q) {
                const int j = lists.off[list] + q;
                partner_index[(size_t)t * dfta_continuum_plan::kMaxPartners + q] = j < lists.off[list + 1] ? lists.rows[j] - k0 : -1;
            }
        }
    return DFTA_OK;
}

// ---- pseudopotentials of the batch's valence levels (pseudo.hip; the resident orbitals and potentials are read in place) -----------------
int dfta_scf_pseudopotentials(dfta_scf* s, int nch, const int* atom, const int* level, const int* ic, double factor, const int* l_loc,
                              int* ic_used, double* u_ps, double* V_ps, double* coef, double* rc, double* match, int* iters, int* status,
                              double* rho_v, double* vH, double* vxc, double* V_ion, double* beta, double* kb)
{
    if (!s) return DFTA_ERR_INVALID;
    dfta_ctx* ctx = s->ctx;
    DFTA_ENTER(ctx);
    DFTA_REQUIRE(ctx, nch >= 0, "dfta_scf_pseudopotentials: nch");
    DFTA_REQUIRE(ctx, !s->lsda, "dfta_scf_pseudopotentials: spin-polarised batches are out of scope");
    DFTA_REQUIRE(ctx, s->exchange_mode == DFTA_EXCHANGE_FUNCTIONAL, "dfta_scf_pseudopotentials: exchange mode must be DFTA_EXCHANGE_FUNCTIONAL");
    DFTA_REQUIRE(ctx, s->steps_done > 0, "no SCF step has run yet: there are no orbitals");
    DFTA_REQUIRE(ctx, s->functional == DFTA_XC_VWN || s->functional == DFTA_XC_PW92 || s->functional == DFTA_XC_PBE,
                 "dfta_scf_pseudopotentials: functional (VWN, PW92 or PBE)");
    if (nch == 0) return DFTA_OK;
    DFTA_REQUIRE(ctx, atom && level, "dfta_scf_pseudopotentials arguments");
    const size_t N = s->g->N;
    hipStream_t st = ctx->stream;
    // the channels' rows, and the atoms in use numbered in the order of their first channel
    std::vector<int> vrow(nch), urow(nch), l(nch), local(nch), order;
    std::vector<double> eps(nch), occ(nch);
    for (int k = 0; k < nch; ++k) {
        DFTA_REQUIRE(ctx, atom[k] >= 0 && atom[k] < s->natoms, "dfta_scf_pseudopotentials: atom");
        const auto [k0, cnt] = s->channel(atom[k], 0);
        DFTA_REQUIRE(ctx, level[k] >= 0 && level[k] < cnt, "dfta_scf_pseudopotentials: level");
        const dfta::Job& j = s->h_jobs[k0 + level[k]];
        DFTA_REQUIRE(ctx, j.l <= dfta_pseudo_plan::kLmax, "pseudize: l outside 0 .. 4");
        DFTA_REQUIRE(ctx, s->solver.h_occ[k0 + level[k]] > 0., "dfta_scf_pseudopotentials: an unoccupied level");
        vrow[k] = atom[k]; urow[k] = k0 + level[k]; l[k] = j.l; eps[k] = j.E; occ[k] = s->solver.h_occ[k0 + level[k]];
        const int at = (int)(std::find(order.begin(), order.end(), atom[k]) - order.begin());
        if (at == (int)order.size()) order.push_back(atom[k]);
        local[k] = at;
    }
    std::vector<int> icv(nch);
    if (ic) icv.assign(ic, ic + nch);
    else {                                           // the default core nodes: the rule reads the orbitals on the host
        std::vector<double> u(N);
        for (int k = 0; k < nch; ++k) {
            DFTA_HIP(ctx, hipMemcpyAsync(u.data(), s->solver.d_Psi + (size_t)urow[k] * N, sizeof(double) * N, hipMemcpyDeviceToHost, st));
            DFTA_HIP(ctx, hipStreamSynchronize(st));
            icv[k] = dfta_pseudo_plan::default_ic(s->g->N, s->g->h_r.data(), u.data(), factor);
            DFTA_REQUIRE(ctx, icv[k] >= 0, "dfta_scf_pseudopotentials: factor");
        }
    }
    dfta_pseudo_plan::Call c;
    c.N = s->g->N; c.nch = nch; c.l = l.data(); c.ic = icv.data();
    if (const char* msg = dfta_pseudo_plan::check(c)) DFTA_REQUIRE(ctx, false, msg);
    if (ic_used) std::copy(icv.begin(), icv.end(), ic_used);
    DevBuf<int> dVrow, dUrow, dL, dIc;
    DevBuf<double> dEps;
    int e = dfta_upload_rows(ctx, vrow.data(), (size_t)nch, &dVrow);
    if (!e) e = dfta_upload_rows(ctx, urow.data(), (size_t)nch, &dUrow);
    if (!e) e = dfta_upload_rows(ctx, l.data(), (size_t)nch, &dL);
    if (!e) e = dfta_upload_rows(ctx, icv.data(), (size_t)nch, &dIc);
    if (!e) e = dfta_upload_rows(ctx, eps.data(), (size_t)nch, &dEps);
    if (e) return e;
    const bool ionic = rho_v || vH || vxc || V_ion || beta || kb;
    std::vector<double> hu, hv, hc;                  // the unscreening reads these three: the caller's arrays, or these
    if (ionic && !u_ps) { hu.resize(nch * N); u_ps = hu.data(); }
    if (ionic && !V_ps) { hv.resize(nch * N); V_ps = hv.data(); }
    if (ionic && !coef) { hc.resize((size_t)nch * DFTA_PS_COEF); coef = hc.data(); }
    dfta_pseudize_out out;
    out.u_ps = u_ps; out.V_ps = V_ps; out.coef = coef; out.rc = rc; out.match = match; out.iters = iters; out.status = status;
    if ((e = dfta_pseudize_run(ctx, s->g, nch, s->d_V, dVrow.p, s->solver.d_Psi, dUrow.p, dL.p, dEps.p, dIc.p, out))) return e;
    if (!ionic) return DFTA_OK;
    std::vector<double> a0(nch);
    for (int k = 0; k < nch; ++k) a0[k] = coef[(size_t)k * DFTA_PS_COEF];
    return dfta_pseudo_ionic(ctx, s->g, s->functional, (int)order.size(), nch, local.data(), l.data(), occ.data(), a0.data(), u_ps, V_ps, l_loc,
                             rho_v, vH, vxc, V_ion, beta, kb);
}

int dfta_scf_photoionization(dfta_scf* s, int atom, int neps, const double* eps, int norm_mode, double* omega_out, double* sigma_out)
{
    if (!s) return DFTA_ERR_INVALID;
    dfta_ctx* ctx = s->ctx;
    DFTA_ENTER(ctx);
    DFTA_REQUIRE(ctx, s->steps_done > 0, "no SCF step has run yet: there are no orbitals");
    DFTA_REQUIRE(ctx, atom >= 0 && atom < s->natoms && neps >= 0, "dfta_scf_photoionization: atom / neps");
    if (neps == 0) return DFTA_OK;
    DFTA_REQUIRE(ctx, eps && omega_out && sigma_out, "dfta_scf_photoionization arguments");
    for (int e = 0; e < neps; ++e) DFTA_REQUIRE(ctx, eps[e] > 0. && std::isfinite(eps[e]), "dfta_scf_photoionization: eps must be finite and > 0");
    constexpr int nl = dfta_continuum_plan::kLmax + 1, np = dfta_continuum_plan::kMaxPartners;
    // trials (spin, l', eps), eps fastest
    const int ntrials = s->nspin * nl * neps;
    std::vector<int> at(ntrials, atom), sp(ntrials), lt(ntrials), mt(ntrials, s->g->N - 2), status(ntrials), pidx((size_t)ntrials * np);
    std::vector<double> Et(ntrials), sums((size_t)ntrials * np);
    for (int t = 0; t < ntrials; ++t) { sp[t] = t / (nl * neps); lt[t] = (t / neps) % nl; Et[t] = eps[t % neps]; }
    if (const int rc = dfta_scf_continuum(s, norm_mode, ntrials, at.data(), sp.data(), lt.data(), Et.data(), mt.data(), 1, nullptr, nullptr,
                                          nullptr, nullptr, status.data(), sums.data(), pidx.data(), nullptr))
        return rc;
    const double K = (4. * (M_PI * M_PI)) * (1. / 137.035999084);
    for (int spin = 0; spin < s->nspin; ++spin) {
        const auto [k0, cnt] = s->channel(atom, spin);
        for (int k = 0; k < cnt; ++k) {
            const dfta::Job& j = s->h_jobs[k0 + k];
            const size_t row = (size_t)(k0 + k - s->h_atoms[atom].job_off) * neps;
            const double occ = s->solver.h_occ[k0 + k];
            for (int e = 0; e < neps; ++e) {
                double S[2] = {0., 0.};                                      // S_{l-1}, S_{l+1}
                for (int side = 0; side < 2; ++side) {
                    const int lp = j.l + (side ? 1 : -1);
                    if (lp < 0 || lp > dfta_continuum_plan::kLmax) continue;
                    const size_t t = ((size_t)spin * nl + lp) * neps + e;
                    S[side] = std::nan("");
                    if (!status[t])
                        for (int q = 0; q < np; ++q)
                            if (pidx[t * np + q] == k) S[side] = sums[t * np + q];
                }
                const double omega = eps[e] - j.E;
                omega_out[row + e] = omega;
                sigma_out[row + e] = (((K * omega) / 3.) * (occ / (2. * j.l + 1.))) * ((j.l * (S[0] * S[0])) + ((j.l + 1.) * (S[1] * S[1])));
            }
        }
    }
    return DFTA_OK;
}

int dfta_scf_get_records_dev(dfta_scf* s, double* dRecords)
{
    if (!s || !dRecords) return DFTA_ERR_INVALID;
    dfta_ctx* ctx = s->ctx;
    DFTA_ENTER(ctx);
    DFTA_HIP(ctx, hipMemcpyAsync(dRecords, s->d_records, sizeof(double) * (size_t)s->natoms * DFTA_RECORD_DOUBLES,
                                 hipMemcpyDeviceToDevice, ctx->stream));
    return DFTA_OK;
}

}  // extern "C"
