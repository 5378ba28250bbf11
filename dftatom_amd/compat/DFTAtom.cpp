// DFTAtom.cpp -- host orchestration of an SCF run on the device path, with the reference's console protocol.
//
// One dfta_scf object holds the whole state in HBM; each dfta_scf_step is one iteration of the reference's `for sp`
// loop (DFTAtom.cpp:396-484, LSDA 908-1009).  The text below reproduces what the reference prints, line for line.
#include "DFTAtom.h"

#include <algorithm>
#include <iomanip>
#include <iostream>

namespace DFT {

const char DFTAtom::orb[] = {'s', 'p', 'd', 'f'};
int DFTAtom::levelsMode = DFTA_LEVELS_BATCHED;
int DFTAtom::integrator = DFTA_INT_SIMPSON38;
int DFTAtom::sweepMode = DFTA_SWEEPS_EXACT;
int DFTAtom::functional = DFTA_XC_VWN;
int DFTAtom::charge = 0;
std::string DFTAtom::config;
int DFTAtom::poissonMode = -1;      // as dfta_poisson_create: exact unless $DFTA_DEBUG POISSON_MODE (--poisson= overrides)
int DFTAtom::mixing = DFTA_MIX_LINEAR;     // --mixing=anderson: Anderson density mixing, default history and warm-up
int DFTAtom::exchange = DFTA_EXCHANGE_FUNCTIONAL;   // --exchange=kli / sic: dfta_scf_set_exchange right after creation
std::ostream* DFTAtom::jsonOut = nullptr;
bool DFTAtom::orbitalTable = false;        // --orbital-table
bool DFTAtom::slaterTable = false;         // --slater-table
bool DFTAtom::exchangeTable = false;       // --exchange-table
bool DFTAtom::sicTable = false;            // --sic-table
bool DFTAtom::formFactorTable = false;     // --form-factor-table[=smax:ns]
double DFTAtom::formFactorSmax = 2.0;
int DFTAtom::formFactorPoints = 41;
bool DFTAtom::phaseShiftTable = false;     // --phase-shift-table[=emax:ne]
double DFTAtom::phaseShiftEmax = 2.0;
int DFTAtom::phaseShiftPoints = 8;
bool DFTAtom::pseudoTable = false;         // --pseudo-table[=factor]
double DFTAtom::pseudoFactor = 1.5;
bool DFTAtom::kbTable = false;             // --kb-table[=elo:ehi:ne]
double DFTAtom::kbElo = -2.0;
double DFTAtom::kbEhi = 1.0;
int DFTAtom::kbPoints = 7;
bool DFTAtom::photoTable = false;          // --photo-table[=emax:ne]
double DFTAtom::photoEmax = 4.0;
int DFTAtom::photoPoints = 8;

namespace {
struct LevelLine { int n, l; double occ, E; int status, n_count, n_zero; };

// DFTAtom::charge / config as the flat arrays of dfta_scf_create_config (one atom)
int build_configuration(int Z, bool lsda, std::vector<int>& nlev, std::vector<int>& n, std::vector<int>& l, std::vector<double>& occ)
{
    const int cap = 32;
    int nA = 0, nB = 0, an[cap], al[cap], bn[cap], bl[cap];
    double ao[cap], bo[cap];
    const int rc = DFTAtom::config.empty()
                       ? dfta_ion_config(Z, DFTAtom::charge, lsda ? 1 : 0, DFTA_AUFBAU_REFERENCE, cap, &nA, &nB, an, al, ao, bn, bl, bo)
                       : dfta_config_parse(Z, lsda ? 1 : 0, DFTA_AUFBAU_REFERENCE, DFTAtom::config.c_str(), cap, &nA, &nB, an, al, ao, bn, bl, bo);
    if (rc != DFTA_OK) return rc;
    nlev = {nA, nB};
    n.assign(an, an + nA); l.assign(al, al + nA); occ.assign(ao, ao + nA);
    n.insert(n.end(), bn, bn + nB); l.insert(l.end(), bl, bl + nB); occ.insert(occ.end(), bo, bo + nB);
    return DFTA_OK;
}

// an occupation as the reference prints its integers; a fractional one with its decimals
void print_occupation(std::ostream& os, double occ)
{
    if (occ == static_cast<double>(static_cast<long>(occ))) os << static_cast<long>(occ);
    else os << std::defaultfloat << std::setprecision(6) << occ << std::fixed;
}

std::vector<LevelLine> fetch_levels(dfta_scf* scf, int spin)
{
    const int cnt = dfta_scf_num_levels(scf, 0, spin);
    std::vector<int> n(cnt), l(cnt), conv(cnt);
    std::vector<double> E(cnt), occ(cnt);
    std::vector<LevelLine> out;
    if (cnt <= 0) return out;
    std::vector<int> st(cnt), nc(cnt), nz(cnt);
    if (dfta_scf_get_levels(scf, 0, spin, n.data(), l.data(), nullptr, E.data(), conv.data()) != DFTA_OK) throw std::runtime_error("dfta_scf_get_levels");
    if (dfta_scf_get_occupations(scf, 0, spin, occ.data()) != DFTA_OK) throw std::runtime_error("dfta_scf_get_occupations");
    if (dfta_scf_get_level_status(scf, 0, spin, st.data(), nc.data(), nz.data()) != DFTA_OK) throw std::runtime_error("dfta_scf_get_level_status");
    for (int i = 0; i < cnt; ++i) out.push_back({n[i], l[i], occ[i], E[i], st[i], nc[i], nz[i]});
    return out;
}

// one line per SCF step: full-precision values the 6-decimal console protocol cannot carry
void json_step(std::ostream& js, int sp, int Z, bool lsda, dfta_scf* scf, const dfta_energies& e, int finished, const dfta_step_stats& st)
{
    js << std::setprecision(17) << std::defaultfloat << "{\"step\": " << sp << ", \"Z\": " << Z << ", \"finished\": " << (finished ? "true" : "false")
       << ", \"Etotal\": " << e.Etotal << ", \"Ekin\": " << e.Ekinetic << ", \"Ecoul\": " << e.Ecoul << ", \"Eenuc\": " << e.Enuclear << ", \"Exc\": " << e.Exc
       << ", \"levels\": [";
    bool first = true;
    for (int spin = 0; spin < (lsda ? 2 : 1); ++spin)
        for (const auto& lv : fetch_levels(scf, spin)) {
            js << (first ? "" : ", ") << "{\"spin\": " << spin << ", \"n\": " << lv.n + 1 << ", \"l\": " << lv.l << ", \"occ\": " << lv.occ << ", \"E\": " << lv.E
               << ", \"status\": " << lv.status << ", \"count_sweeps\": " << lv.n_count << ", \"zero_sweeps\": " << lv.n_zero << "}";
            first = false;
        }
    js << "], \"rounds\": " << st.rounds << ", \"levels_layout\": " << st.levels_layout << ", \"vcycles\": " << st.vcycles
       << ", \"sweeps_reference\": " << st.sweeps_reference << ", \"sweeps_executed\": " << st.sweeps_reference_executed << ", \"sweeps_issued\": " << st.sweeps_issued
       << ", \"ms_levels\": " << st.ms_levels << ", \"ms_sweep_kernels\": " << st.ms_sweep_kernels << ", \"ms_poisson\": " << st.ms_poisson << ", \"ms_tail\": " << st.ms_tail
       << "}" << std::endl;
}

// --orbital-table: one line per level from the device's orbital properties (dfta_scf_orbital_properties: one launch for all levels)
void print_orbital_table(dfta_scf* scf, bool lsda)
{
    int njobs = 0;
    if (dfta_scf_info(scf, nullptr, &njobs, nullptr) != DFTA_OK) throw std::runtime_error("dfta_scf_info");
    std::vector<double> props(static_cast<size_t>(njobs) * DFTA_ORB_PROPS);
    if (dfta_scf_orbital_properties(scf, props.data()) != DFTA_OK) throw std::runtime_error("dfta_scf_orbital_properties");
    size_t row = 0;                                         // rows: the alpha levels, then the beta levels
    for (int spin = 0; spin < (lsda ? 2 : 1); ++spin)
        for (const auto& lv : fetch_levels(scf, spin)) {
            const double* p = props.data() + DFTA_ORB_PROPS * row++;
            std::cout << "Orbital " << (lsda ? (spin == 0 ? "alpha " : "beta ") : "") << lv.n + 1 << DFTAtom::orb[lv.l] << ": n = " << lv.n + 1 << " l = " << lv.l
                      << " occ = ";
            print_occupation(std::cout, lv.occ);
            std::cout << " E = " << std::fixed << std::setprecision(6) << lv.E << " <r> = " << p[DFTA_ORB_R1] << " <r^2> = " << p[DFTA_ORB_R2]
                      << " T = " << p[DFTA_ORB_T] << " r_peak = " << p[DFTA_ORB_RPEAK] << std::endl;
        }
    std::cout << std::endl;
}

// --slater-table: one line per F^k / G^k of each channel's table (dfta_scf_slater_fg: one launch per channel), then the Hartree and
// exact-exchange energies of the orbitals (dfta_scf_coulomb_exchange)
void print_slater_table(dfta_scf* scf, bool lsda)
{
    for (int spin = 0; spin < (lsda ? 2 : 1); ++spin) {
        const std::vector<LevelLine> lv = fetch_levels(scf, spin);
        const size_t n = lv.size();
        if (n == 0) continue;
        std::vector<int> l(n);
        for (size_t a = 0; a < n; ++a) l[a] = lv[a].l;
        const int njobs = dfta_slater_fg_jobs(static_cast<int>(n), l.data(), nullptr, nullptr);
        if (njobs < 0) throw std::runtime_error("dfta_slater_fg_jobs");
        std::vector<int> jobs(static_cast<size_t>(njobs) * 5), kinds(njobs);
        dfta_slater_fg_jobs(static_cast<int>(n), l.data(), jobs.data(), kinds.data());
        std::vector<double> F((DFTA_SLATER_KMAX + 1) * n * n), G((DFTA_SLATER_KMAX + 1) * n * n);
        if (dfta_scf_slater_fg(scf, 0, spin, F.data(), G.data()) != DFTA_OK) throw std::runtime_error("dfta_scf_slater_fg");
        for (int j = 0; j < njobs; ++j) {
            const int a = jobs[5 * j], b = jobs[5 * j + 1], k = jobs[5 * j + 4];
            const double v = (kinds[j] ? G : F)[(k * n + a) * n + b];
            std::cout << "Slater " << (lsda ? (spin == 0 ? "alpha " : "beta ") : "") << (kinds[j] ? "G" : "F") << k << "(" << lv[a].n + 1
                      << DFTAtom::orb[lv[a].l] << "," << lv[b].n + 1 << DFTAtom::orb[lv[b].l] << ") = " << std::fixed << std::setprecision(6) << v
                      << std::endl;
        }
    }
    double EH = 0, EXX = 0;
    if (dfta_scf_coulomb_exchange(scf, 0, &EH, &EXX) != DFTA_OK) throw std::runtime_error("dfta_scf_coulomb_exchange");
    std::cout << "EHartree = " << std::fixed << std::setprecision(6) << EH << " EXX = " << EXX << std::endl << std::endl;
}

// --exchange-table: per channel one line per shell with its eigenvalue, <a|v_x^HF,a|a>, <a|vS|a>, <a|vKLI|a> and the KLI constant c_a
// (dfta_scf_exchange_potentials: one call per channel), then E_x = 1/2 Sum n vbarHF over the channels (LDA: twice the one channel's) and
// r vKLI at the outermost node where the channel's density is positive
void print_exchange_table(dfta_scf* scf, const dfta_grid* grid, bool lsda)
{
    const int N = dfta_grid_num_nodes(grid);
    std::vector<double> r(N), D(N), vKLI(N);
    if (dfta_grid_get_r(grid, r.data()) != DFTA_OK) throw std::runtime_error("dfta_grid_get_r");
    double ex = 0;
    std::vector<std::pair<int, double>> tails;      // per channel: spin, r vKLI
    for (int spin = 0; spin < (lsda ? 2 : 1); ++spin) {
        const std::vector<LevelLine> lv = fetch_levels(scf, spin);
        const size_t n = lv.size();
        if (n == 0) continue;
        std::vector<double> vbar(DFTA_XP_COLS * n);
        if (dfta_scf_exchange_potentials(scf, 0, spin, nullptr, D.data(), nullptr, vKLI.data(), vbar.data(), nullptr, nullptr) != DFTA_OK)
            throw std::runtime_error("dfta_scf_exchange_potentials");
        double sum = 0;
        for (size_t a = 0; a < n; ++a) {
            const double* v = vbar.data() + DFTA_XP_COLS * a;
            sum += (lsda ? lv[a].occ : 0.5 * lv[a].occ) * v[DFTA_XP_HF];
            std::cout << "Exchange " << (lsda ? (spin == 0 ? "alpha " : "beta ") : "") << lv[a].n + 1 << DFTAtom::orb[lv[a].l] << ": E = " << std::fixed
                      << std::setprecision(6) << lv[a].E << " vbarHF = " << v[DFTA_XP_HF] << " vbarS = " << v[DFTA_XP_S] << " vbarKLI = " << v[DFTA_XP_KLI]
                      << " c = " << v[DFTA_XP_C] << std::endl;
        }
        ex += lsda ? 0.5 * sum : sum;
        int last = -1;
        for (int i = 0; i < N; ++i)
            if (D[i] > 0) last = i;
        if (last >= 0) tails.push_back({spin, r[last] * vKLI[last]});
    }
    std::cout << "EXX = " << std::fixed << std::setprecision(6) << ex;
    for (const auto& t : tails) std::cout << " r*vKLI" << (lsda ? (t.first == 0 ? "(alpha)" : "(beta)") : "") << " = " << t.second;
    std::cout << std::endl << std::endl;
}

// --sic-table (with --exchange=sic): per channel one line per shell with its eigenvalue, the self-Hartree and self-xc energies EH_a and EXC_a
// of one electron in the shell, <a|v_a^SIC|a> and the KLI constant c_a (dfta_scf_sic_table), then E_SIC (dfta_scf_get_exchange)
void print_sic_table(dfta_scf* scf, bool lsda)
{
    for (int spin = 0; spin < (lsda ? 2 : 1); ++spin) {
        const std::vector<LevelLine> lv = fetch_levels(scf, spin);
        const size_t n = lv.size();
        if (n == 0) continue;
        std::vector<double> EH(n), EXC(n), vbar(n), c(n);
        if (dfta_scf_sic_table(scf, 0, spin, EH.data(), EXC.data(), vbar.data(), c.data(), nullptr) != DFTA_OK)
            throw std::runtime_error("dfta_scf_sic_table");
        for (size_t a = 0; a < n; ++a)
            std::cout << "SIC " << (lsda ? (spin == 0 ? "alpha " : "beta ") : "") << lv[a].n + 1 << DFTAtom::orb[lv[a].l] << ": E = " << std::fixed
                      << std::setprecision(6) << lv[a].E << " EH = " << EH[a] << " EXC = " << EXC[a] << " vbar = " << vbar[a] << " c = " << c[a]
                      << std::endl;
    }
    double esic = 0;
    if (dfta_scf_get_exchange(scf, 0, 0, nullptr, nullptr, &esic) != DFTA_OK) throw std::runtime_error("dfta_scf_get_exchange");
    std::cout << "ESIC = " << std::fixed << std::setprecision(6) << esic << std::endl << std::endl;
}

// --form-factor-table: f(q) of the converged density at s_k = smax k / (ns - 1), q = ((4 pi) s) 0.529177210903 (s in 1 / Angstrom, q in
// atomic units), every q in one launch (dfta_scf_form_factors); LSDA: the magnetic form factor f_a - f_b beside it
void print_form_factor_table(dfta_scf* scf, bool lsda)
{
    const int ns = DFTAtom::formFactorPoints, nchan = lsda ? 3 : 1;
    std::vector<double> s(ns), q(ns), f(static_cast<size_t>(nchan) * ns);
    for (int k = 0; k < ns; ++k) {
        s[k] = ns > 1 ? DFTAtom::formFactorSmax * k / (ns - 1) : 0.;
        q[k] = ((4. * M_PI) * s[k]) * 0.529177210903;
    }
    if (dfta_scf_form_factors(scf, ns, q.data(), f.data()) != DFTA_OK) throw std::runtime_error("dfta_scf_form_factors");
    for (int k = 0; k < ns; ++k) {
        std::cout << "FormFactor s = " << std::fixed << std::setprecision(6) << s[k] << " q = " << q[k] << " f = " << f[k];
        if (lsda) std::cout << " fa-fb = " << f[ns + k] - f[2 * ns + k];
        std::cout << std::endl;
    }
    std::cout << std::endl;
}

// the normalisation of the continuum tables: the Riccati matching needs a short-range potential
int continuum_norm() { return DFTAtom::charge != 0 || !DFTAtom::config.empty() || DFTAtom::exchange != DFTA_EXCHANGE_FUNCTIONAL ? DFTA_CONT_WKB : DFTA_CONT_FREE; }

// --phase-shift-table: every (spin, l = 0 .. 4, E_k = Emax (k + 1) / ne) in one launch, end node N - 2; "status =" prints the trial's
// DFTA_CONT_* bits as they come (NONFINITE 1, STEP 2, WKB_TAIL 4, NORM 8)
void print_phase_shift_table(dfta_scf* scf, const dfta_grid* grid, bool lsda)
{
    const int ne = DFTAtom::phaseShiftPoints, nspin = lsda ? 2 : 1, nt = nspin * 5 * ne, norm = continuum_norm();
    std::vector<int> atom(nt, 0), spin(nt), l(nt), m(nt, dfta_grid_num_nodes(grid) - 2), nodes(nt), status(nt);
    std::vector<double> E(nt), ld(nt), delta(nt), scale(nt);
    for (int t = 0; t < nt; ++t) {
        spin[t] = t / (5 * ne); l[t] = (t / ne) % 5;
        E[t] = DFTAtom::phaseShiftEmax * (t % ne + 1) / ne;
    }
    if (dfta_scf_continuum(scf, norm, nt, atom.data(), spin.data(), l.data(), E.data(), m.data(), -1, ld.data(), nodes.data(), delta.data(),
                           scale.data(), status.data(), nullptr, nullptr, nullptr) != DFTA_OK)
        throw std::runtime_error("dfta_scf_continuum");
    for (int t = 0; t < nt; ++t) {
        std::cout << "PhaseShift ";
        if (lsda) std::cout << (spin[t] == 0 ? "alpha " : "beta ");
        std::cout << "l = " << l[t] << " E = " << std::fixed << std::setprecision(6) << E[t] << (norm == DFTA_CONT_FREE ? " delta = " : " phase = ") << delta[t]
                  << " dlog = " << ld[t] << " nodes = " << nodes[t] << " status = " << status[t] << std::endl;
    }
    std::cout << std::endl;
}

// --photo-table: sigma_nl(omega) of every subshell at eps_k = Emax (k + 1) / ne, one launch; 1 a_0^2 = 28.002852 Mb
void print_photo_table(dfta_scf* scf, bool lsda)
{
    const int ne = DFTAtom::photoPoints;
    std::vector<double> eps(ne);
    for (int k = 0; k < ne; ++k) eps[k] = DFTAtom::photoEmax * (k + 1) / ne;
    std::vector<LevelLine> levels = fetch_levels(scf, 0);
    const size_t nalpha = levels.size();
    if (lsda)
        for (const auto& lv : fetch_levels(scf, 1)) levels.push_back(lv);
    std::vector<double> omega(levels.size() * ne), sigma(levels.size() * ne);
    if (dfta_scf_photoionization(scf, 0, ne, eps.data(), continuum_norm(), omega.data(), sigma.data()) != DFTA_OK)
        throw std::runtime_error("dfta_scf_photoionization");
    for (size_t a = 0; a < levels.size(); ++a)
        for (int k = 0; k < ne; ++k) {
            std::cout << "Photo ";
            if (lsda) std::cout << (a < nalpha ? "alpha " : "beta ");
            std::cout << levels[a].n + 1 << DFTAtom::orb[levels[a].l] << " eps = " << std::fixed << std::setprecision(6) << eps[k] << " omega = " << omega[a * ne + k]
                      << " sigma = " << sigma[a * ne + k] << " Mb = " << sigma[a * ne + k] * 28.002852 << std::endl;
        }
    std::cout << std::endl;
}

// --pseudo-table: the Troullier-Martins pseudopotentials of the default valence levels (dfta_scf_pseudopotentials on the resident
// potential), with two checks: the eigenvalue of the nodeless level of V_ps by dfta_solve_levels, and the norm residual g
void print_pseudo_table(dfta_scf* scf, dfta_ctx* ctx, const dfta_grid* grid, bool lsda, int N)
{
    if (lsda) {
        std::cout << "Pseudo: spin-polarised atoms are out of scope" << std::endl << std::endl;
        return;
    }
    const std::vector<LevelLine> levels = fetch_levels(scf, 0);
    const int nlev = (int)levels.size();
    std::vector<int> n(nlev), l(nlev), occ(nlev), pick(nlev), atom;
    for (int k = 0; k < nlev; ++k) { n[k] = levels[k].n; l[k] = levels[k].l; occ[k] = levels[k].occ > 0. ? 1 : 0; }
    int nch = 0;
    if (dfta_pseudo_default_valence(nlev, n.data(), l.data(), occ.data(), nlev, pick.data(), &nch) != DFTA_OK)
        throw std::runtime_error("dfta_pseudo_default_valence");
    atom.assign(nch, 0);
    std::vector<int> ic(nch), iters(nch), status(nch);
    std::vector<double> Vps((size_t)nch * N), coef((size_t)nch * DFTA_PS_COEF), rc(nch), match((size_t)nch * DFTA_PS_MATCH), kb((size_t)nch * 3);
    if (dfta_scf_pseudopotentials(scf, nch, atom.data(), pick.data(), nullptr, DFTAtom::pseudoFactor, nullptr, ic.data(), nullptr, Vps.data(),
                                  coef.data(), rc.data(), match.data(), iters.data(), status.data(), nullptr, nullptr, nullptr, nullptr, nullptr,
                                  kb.data()) != DFTA_OK)
        throw std::runtime_error(std::string("dfta_scf_pseudopotentials: ") + dfta_last_error(ctx));
    for (int k = 0; k < nch; ++k) {
        const LevelLine& lv = levels[pick[k]];
        std::cout << "Pseudo " << lv.n + 1 << DFTAtom::orb[lv.l] << " status = " << status[k] << " ic = " << ic[k] << " rc = " << std::fixed
                  << std::setprecision(6) << rc[k] << " evaluations = " << iters[k] << " coef =";
        for (int q = 0; q < DFTA_PS_COEF; ++q) std::cout << " " << std::setprecision(9) << coef[(size_t)k * DFTA_PS_COEF + q];
        std::cout << " EKB = " << std::setprecision(6) << kb[(size_t)k * 3 + 2];
        double dE = std::nan("");
        if (!status[k]) {
            const double* V = Vps.data() + (size_t)k * N;
            const double bottom = *std::min_element(V + 1, V + N) - 1.0;
            const int vidx = 0, nn = lv.l, one = 1;
            dfta_level_result res = {};
            if (dfta_solve_levels(ctx, grid, DFTA_LEVELS_BATCHED, 0, 1, V, &bottom, nullptr, 1, &vidx, &nn, &lv.l, &one, &res, nullptr, nullptr, nullptr,
                                  nullptr) != DFTA_OK)
                throw std::runtime_error("dfta_solve_levels");
            dE = res.E - lv.E;
        }
        std::cout << " eigenvalue check = " << std::scientific << std::setprecision(2) << dE << " norm check = " << match[(size_t)k * DFTA_PS_MATCH + 7]
                  << std::fixed << std::endl;
    }
    std::cout << std::endl;
}

// --kb-table: the Kleinman-Bylander form of the default valence levels' pseudopotentials (the highest l local): per channel E_KB, the
// bound states of H_KB below 0 in the box that ends at the last node but one, the two ghost verdicts (dfta_kb_ghost_report), then u'/u
// at the atom's largest core radius in the all-electron potential, in V_ps,l and in H_KB at kbPoints energies in kbElo .. kbEhi
void print_kb_table(dfta_scf* scf, dfta_ctx* ctx, const dfta_grid* grid, bool lsda, int N)
{
    if (lsda) {
        std::cout << "KB: spin-polarised atoms are out of scope" << std::endl << std::endl;
        return;
    }
    const std::vector<LevelLine> levels = fetch_levels(scf, 0);
    const int nlev = (int)levels.size();
    std::vector<int> n(nlev), l(nlev), occ(nlev), pick(nlev);
    for (int k = 0; k < nlev; ++k) { n[k] = levels[k].n; l[k] = levels[k].l; occ[k] = levels[k].occ > 0. ? 1 : 0; }
    int nch = 0;
    if (dfta_pseudo_default_valence(nlev, n.data(), l.data(), occ.data(), nlev, pick.data(), &nch) != DFTA_OK)
        throw std::runtime_error("dfta_pseudo_default_valence");
    std::vector<int> atom(nch, 0), ic(nch), status(nch), lch(nch);
    std::vector<double> Vps((size_t)nch * N), beta((size_t)nch * N), kb((size_t)nch * 3), eps(nch);
    if (dfta_scf_pseudopotentials(scf, nch, atom.data(), pick.data(), nullptr, DFTAtom::pseudoFactor, nullptr, ic.data(), nullptr, Vps.data(), nullptr,
                                  nullptr, nullptr, nullptr, status.data(), nullptr, nullptr, nullptr, nullptr, beta.data(), kb.data()) != DFTA_OK)
        throw std::runtime_error(std::string("dfta_scf_pseudopotentials: ") + dfta_last_error(ctx));
    int loc = 0, icmax = 0;
    for (int k = 0; k < nch; ++k) {
        lch[k] = levels[pick[k]].l; eps[k] = levels[pick[k]].E;
        if (status[k]) { std::cout << "KB: the pseudization of a channel failed (status " << status[k] << ")" << std::endl << std::endl; return; }
        if (lch[k] > lch[loc]) loc = k;
        icmax = std::max(icmax, ic[k]);
    }
    std::vector<double> report((size_t)nch * DFTA_KB_REPORT), states((size_t)nch * DFTA_KB_MAX_STATES);
    if (dfta_kb_ghost_report(ctx, grid, 1, nch, atom.data(), lch.data(), eps.data(), Vps.data(), beta.data(), kb.data(), nullptr, N - 2, std::nan(""), 0., 512,
                             1e-5, report.data(), states.data()) != DFTA_OK)
        throw std::runtime_error(std::string("dfta_kb_ghost_report: ") + dfta_last_error(ctx));
    std::vector<double> r(N);
    dfta_grid_get_r(grid, r.data());
    const int ne = DFTAtom::kbPoints;
    std::vector<double> E(ne), ae(ne), sl(ne), nl(ne);
    for (int j = 0; j < ne; ++j) E[j] = DFTAtom::kbElo + (DFTAtom::kbEhi - DFTAtom::kbElo) * j / (ne > 1 ? ne - 1 : 1);
    for (int k = 0; k < nch; ++k) {
        const LevelLine& lv = levels[pick[k]];
        const double* rp = &report[(size_t)k * DFTA_KB_REPORT];
        std::cout << "KB " << lv.n + 1 << DFTAtom::orb[lv.l] << std::fixed << std::setprecision(6);
        if (k == loc) {
            std::cout << " local" << std::endl;
        } else {
            std::cout << " EKB = " << rp[1] << " states =";
            for (int q = 0; q < (int)rp[2]; ++q) std::cout << " " << states[(size_t)k * DFTA_KB_MAX_STATES + q];
            std::cout << " eps = " << rp[0] << " local levels = " << rp[4] << " " << rp[5] << " GKS = " << (rp[6] != rp[6] ? -1 : (int)rp[6])
                      << " direct = " << (int)rp[7] << " ghosts = " << (int)rp[3] << std::endl;
        }
        std::vector<int> zero(ne, 0), ll(ne, lv.l), mm(ne, icmax);
        const double one = 1.;
        std::vector<double> nobeta(N, 0.);
        if (dfta_scf_continuum(scf, continuum_norm(), ne, zero.data(), zero.data(), ll.data(), E.data(), mm.data(), -1, ae.data(), nullptr, nullptr, nullptr,
                               nullptr, nullptr, nullptr, nullptr) != DFTA_OK
            || dfta_kb_sweep(ctx, grid, 1, Vps.data() + (size_t)k * N, 1, nullptr, &lv.l, nobeta.data(), &one, ne, nullptr, E.data(), mm.data(), nullptr,
                             nullptr, sl.data(), nullptr, nullptr, nullptr, nullptr, nullptr) != DFTA_OK
            || dfta_kb_sweep(ctx, grid, 1, Vps.data() + (size_t)loc * N, 1, nullptr, &lv.l, k == loc ? nobeta.data() : beta.data() + (size_t)k * N,
                             k == loc ? &one : &kb[(size_t)k * 3], ne, nullptr, E.data(), mm.data(), nullptr, nullptr, nl.data(), nullptr, nullptr, nullptr,
                             nullptr, nullptr) != DFTA_OK)
            throw std::runtime_error(std::string("KB table: ") + dfta_last_error(ctx));
        for (int j = 0; j < ne; ++j)
            std::cout << "KB " << lv.n + 1 << DFTAtom::orb[lv.l] << " r = " << r[icmax] << " E = " << E[j] << " AE = " << ae[j] << " semilocal = " << sl[j]
                      << " KB = " << nl[j] << std::endl;
    }
    std::cout << std::endl;
}

void print_configuration(std::vector<LevelLine> levels)
{
    // levels sorted by energy for the final configuration line (DFTAtom.cpp:487-490)
    std::sort(levels.begin(), levels.end(), [](const LevelLine& a, const LevelLine& b) { return a.E < b.E; });
    for (const auto& lv : levels) {
        std::cout << lv.n + 1 << DFTAtom::orb[lv.l];
        print_occupation(std::cout, lv.occ);
        std::cout << " ";
    }
}
}  // namespace

void DFTAtom::Run(bool lsda, bool uniform, int Z, int MultigridLevels, double alpha, double MaxR, double deltaGrid)
{
    auto& rt = dfta_compat::Runtime::instance();
    dfta_grid* grid = uniform ? rt.uniform_grid(MultigridLevels, MaxR) : rt.grid(MultigridLevels, deltaGrid, MaxR);
    // banners of DFTAtom.cpp:70,358,658,857 (the non-uniform LDA one does say "LSD")
    std::cout << "Computing atom with Z=" << Z
              << (uniform ? (lsda ? " using LSDA with uniform grid" : " using LDA with uniform grid")
                          : (lsda ? " using LSDA with non-uniform grid" : " using LSD with non-uniform grid")) << std::endl;

    dfta_scf* scf = nullptr;
    dfta_scf_options opt = {};                    // zero = what the reference runs
    opt.struct_size = (int)sizeof(opt);
    opt.integrator = integrator; opt.functional = functional; opt.aufbau = DFTA_AUFBAU_REFERENCE;
    opt.poisson_mode = poissonMode; opt.sweep_mode = sweepMode; opt.mixing = mixing;
    if (charge == 0 && config.empty()) {
        dfta_compat::check(dfta_scf_create_ex(rt.ctx(), grid, lsda ? 1 : 0, 1, &Z, alpha, levelsMode, 0, &opt, &scf), rt.ctx(), "dfta_scf_create");
    } else {
        std::vector<int> nlev, n, l;
        std::vector<double> occ;
        if (build_configuration(Z, lsda, nlev, n, l, occ) != DFTA_OK)
            throw std::invalid_argument(std::string("electron configuration: ") + dfta_config_last_error());
        dfta_compat::check(dfta_scf_create_config(rt.ctx(), grid, lsda ? 1 : 0, 1, &Z, nlev.data(), n.data(), l.data(), occ.data(), alpha, levelsMode, 0,
                                                  &opt, &scf), rt.ctx(), "dfta_scf_create_config");
    }
    if (exchange != DFTA_EXCHANGE_FUNCTIONAL) dfta_compat::check(dfta_scf_set_exchange(scf, exchange), rt.ctx(), "dfta_scf_set_exchange");
    const int maxSteps = lsda ? 150 : 100;                                  // DFTAtom.cpp:396 / 908
    for (int sp = 0; sp < maxSteps; ++sp) {
        std::cout << "Step: " << sp << std::endl;
        dfta_step_stats stats = {};
        stats.struct_size = (int)sizeof(stats);
        dfta_compat::check(dfta_scf_step(scf, jsonOut ? &stats : nullptr), rt.ctx(), "dfta_scf_step");
        for (int spin = 0; spin < (lsda ? 2 : 1); ++spin)
            for (const auto& lv : fetch_levels(scf, spin)) {
                // DFTAtom.cpp:548-556: the non-uniform path loses the alpha/beta tag, the uniform one prints it (DFTAtom.cpp:266-273,698,717)
                std::cout << "Energy ";
                if (lsda && uniform) std::cout << (spin == 0 ? "alpha " : "beta ");
                std::cout << lv.n + 1 << orb[lv.l] << ": " << std::fixed << std::setprecision(6) << lv.E << " Num nodes: " << lv.n - lv.l << std::endl;
            }
        dfta_energies e;
        int finished = 0;
        dfta_compat::check(dfta_scf_get_energies(scf, &e, &finished), rt.ctx(), "dfta_scf_get_energies");
        std::cout << "Etotal = " << std::fixed << std::setprecision(6) << e.Etotal << " Ekin = " << e.Ekinetic << " Ecoul = " << e.Ecoul
                  << " Eenuc = " << e.Enuclear << " Exc = " << e.Exc << std::endl;
        if (jsonOut) json_step(*jsonOut, sp, Z, lsda, scf, e, finished, stats);
        if (finished) {
            std::cout << std::endl << "Finished!" << std::endl << std::endl;
            if (orbitalTable) print_orbital_table(scf, lsda);
            if (slaterTable) print_slater_table(scf, lsda);
            if (exchangeTable) print_exchange_table(scf, grid, lsda);
            if (sicTable && exchange == DFTA_EXCHANGE_SIC_KLI) print_sic_table(scf, lsda);
            if (formFactorTable) print_form_factor_table(scf, lsda);
            if (phaseShiftTable) print_phase_shift_table(scf, grid, lsda);
            if (photoTable) print_photo_table(scf, lsda);
            if (pseudoTable) print_pseudo_table(scf, rt.ctx(), grid, lsda, dfta_num_nodes(MultigridLevels));
            if (kbTable) print_kb_table(scf, rt.ctx(), grid, lsda, dfta_num_nodes(MultigridLevels));
            break;
        }
        std::cout << "********************************************************************************" << std::endl;
    }
    if (!lsda) print_configuration(fetch_levels(scf, 0));
    else {
        std::cout << "Alpha: ";
        print_configuration(fetch_levels(scf, 0));
        std::cout << "\nBeta: ";
        print_configuration(fetch_levels(scf, 1));
    }
    dfta_scf_destroy(scf);
}

const char* DFTAtom::CheckConfiguration(int Z, bool lsda)
{
    if (charge == 0 && config.empty()) return nullptr;
    std::vector<int> nlev, n, l;
    std::vector<double> occ;
    return build_configuration(Z, lsda, nlev, n, l, occ) == DFTA_OK ? nullptr : dfta_config_last_error();
}

void DFTAtom::CalculateNonUniformLDA(int Z, int MultigridLevels, double alpha, double MaxR, double deltaGrid) { Run(false, false, Z, MultigridLevels, alpha, MaxR, deltaGrid); }
void DFTAtom::CalculateNonUniformLSDA(int Z, int MultigridLevels, double alpha, double MaxR, double deltaGrid) { Run(true, false, Z, MultigridLevels, alpha, MaxR, deltaGrid); }
// DFTAtom.cpp:60-210, 646-844: the same SCF on r_i = i h (unreachable from the reference's GUI, DFTAtomFrame.cpp:191,194, but part of its surface)
void DFTAtom::CalculateUniformLDA(int Z, int MultigridLevels, double alpha, double MaxR) { Run(false, true, Z, MultigridLevels, alpha, MaxR, 0); }
void DFTAtom::CalculateUniformLSDA(int Z, int MultigridLevels, double alpha, double MaxR) { Run(true, true, Z, MultigridLevels, alpha, MaxR, 0); }

}  // namespace DFT
