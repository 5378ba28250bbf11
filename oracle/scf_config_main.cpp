// scf_config_main.cpp -- the pure host logic of the SCF layer (dftatom_amd/csrc/scf_config.cpp) as a stand-alone program, built with the
// sanitizers (make -C oracle scf_config); tests/test_scf_config.py runs it.
//
//   scf_config_main plan       plan_scf_config against the loop it replaced (kept below, verbatim): Aufbau and explicit configurations
//   scf_config_main refusals   what both refuse, what both accept, the sorted output, the atom a refusal names
//   scf_config_main options    resolve_scf_options: the struct_size protocol, defaults, one refusal per range check; the statistics copy
//
// Every check that fails prints a line "VIOLATION ..."; every mode ends with one summary line that says how many cases it ran.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "../dftatom_amd/csrc/scf_config.h"

static int g_violations = 0;
#define CHECK(cond, ...)                                                      \
    do {                                                                      \
        if (!(cond)) {                                                        \
            ++g_violations;                                                   \
            printf("VIOLATION %s:%d %s: ", __func__, __LINE__, #cond);        \
            printf(__VA_ARGS__);                                              \
            printf("\n");                                                     \
        }                                                                     \
    } while (0)

static bool same_bits(double a, double b) { return memcmp(&a, &b, sizeof(double)) == 0; }

// ---- the replaced code: config_channel + scf_configure of scf.hip, verbatim, over just enough of the state they wrote ---------------
struct dfta_ctx { char err[512] = {0}; };
struct AtomState {
    int Z;
    double nE;
    double nAlphaE, nBetaE;
    int job_off, job_end;
    int lastTimeConverged;
    int finished;
    int steps;
    double Eold;
    dfta_energies e;
};
struct dfta_scf {
    dfta_ctx* ctx = nullptr;
    int lsda = 0, natoms = 0, nspin = 1, nV = 0;
    std::vector<AtomState> h_atoms;
    std::vector<double> h_bottom0;
    std::vector<int> spin_nlev[2];
};
static std::string g_ref_config_err;
namespace dfta { static void config_set_error(const char* msg) { g_ref_config_err = msg; } }

// the levels of one spin channel of an explicit configuration: sorted by (n, l) (DFTAtom.cpp:367) and checked; ne += their electrons
static bool config_channel(dfta_ctx* ctx, int a, int lsda, int cnt, const int* n, const int* l, const double* occ,
                           std::vector<std::pair<std::pair<int, int>, double>>& lev, double& ne)
{
    lev.clear();
    for (int k = 0; k < cnt; ++k) lev.push_back({{n[k], l[k]}, occ[k]});
    std::stable_sort(lev.begin(), lev.end(), [](const auto& x, const auto& y) { return x.first < y.first; });
    const double perl = lsda ? 1. : 2.;
    for (size_t k = 0; k < lev.size(); ++k) {
        const int N = lev[k].first.first, L = lev[k].first.second;
        const double o = lev[k].second;
        // N: principal quantum number - 1, as dfta_get_subshells_ex and dfta_scf_get_levels report it
        if (L < 0 || L > 3 || N < L) { snprintf(ctx->err, sizeof(ctx->err), "atom %d: level n = %d, l = %d (needs 0 <= l < n, l <= 3)", a, N + 1, L); return false; }
        if (k > 0 && lev[k - 1].first == lev[k].first) { snprintf(ctx->err, sizeof(ctx->err), "atom %d: level n = %d, l = %d given twice", a, N + 1, L); return false; }
        if (!(o > 0) || o > perl * (2 * L + 1)) {
            snprintf(ctx->err, sizeof(ctx->err), "atom %d: level n = %d, l = %d: occupation %g outside (0, %g]", a, N + 1, L, o, perl * (2 * L + 1));
            return false;
        }
        ne += o;
    }
    return true;
}

// (Z, explicit configuration or Aufbau) of every atom -> its AtomState, the bracket bottoms, the levels per spin and the job list.
// Host only; on an error the text is in ctx->err (and, for an explicit configuration, in dfta_config_last_error()).
static int scf_configure(dfta_scf* s, const int* Z, const int* nlev, const int* cn, const int* cl, const double* cocc, int aufbau,
                         std::vector<dfta::JobSpec>& specs)
{
    dfta_ctx* ctx = s->ctx;
    const int lsda = s->lsda, natoms = s->natoms;
    s->h_atoms.resize(natoms);
    s->h_bottom0.resize(s->nV);
    s->spin_nlev[0].resize(natoms); s->spin_nlev[1].assign(natoms, 0);
    std::vector<std::pair<std::pair<int, int>, double>> lev;
    size_t coff = 0;                                           // running offset into the caller's n / l / occ
    for (int a = 0; a < natoms; ++a) {
        if (Z[a] < 1 || Z[a] > 118) {
            snprintf(ctx->err, sizeof(ctx->err), "Z out of range");
            if (nlev) dfta::config_set_error(ctx->err);
            return DFTA_ERR_INVALID;
        }
        AtomState& st = s->h_atoms[a];
        memset(&st, 0, sizeof(st));
        st.Z = Z[a];
        st.job_off = (int)specs.size();
        for (int spin = 0; spin < s->nspin; ++spin) s->h_bottom0[s->nspin * a + spin] = -double(Z[a]) * Z[a] - 1.;     // DFTAtom.cpp:407 / 919,929
        int an[32], al[32], ao[32], bn[32], bl[32], bo[32], nA = 0, nB = 0;
        if (nlev) {                                            // explicit configuration (fractional occupations, cations)
            nA = nlev[2 * a];
            nB = nlev[2 * a + 1];
            double ne = 0, neA = 0;
            bool ok = nA >= 0 && nB >= 0 && nA + nB >= 1 && nA <= 32 && nB <= 32 && (lsda || nB == 0);
            if (!ok) snprintf(ctx->err, sizeof(ctx->err), "atom %d: level counts %d / %d (1 .. 32 levels; LDA: no beta levels)", a, nA, nB);
            for (int spin = 0; ok && spin < (lsda ? 2 : 1); ++spin) {
                const int cnt = spin ? nB : nA;
                ok = config_channel(ctx, a, lsda, cnt, cn + coff, cl + coff, cocc + coff, lev, ne);
                coff += (size_t)cnt;
                for (size_t k = 0; ok && k < lev.size(); ++k) {
                    const double o = lev[k].second;
                    const int io = (o == std::floor(o)) ? static_cast<int>(o) : 0;     // Job::occ: the integer, 0 for a fractional one
                    specs.push_back({lsda ? 2 * a + spin : a, lev[k].first.first, lev[k].first.second, io, o});
                }
                if (spin == 0) neA = ne;
            }
            if (ok && ne > Z[a] + 1e-9) {
                snprintf(ctx->err, sizeof(ctx->err), "atom %d: %g electrons for Z = %d (anions are not supported)", a, ne, Z[a]);
                ok = false;
            }
            if (!ok) { dfta::config_set_error(ctx->err); return DFTA_ERR_INVALID; }
            st.nE = ne;
            st.nAlphaE = neA;
            st.nBetaE = ne - neA;
        } else if (!lsda) {
            nA = dfta_get_subshells_ex(Z[a], aufbau, an, al, ao, 32);
            if (nA < 0) return DFTA_ERR_INVALID;
            for (int k = 0; k < nA; ++k) specs.push_back({a, an[k], al[k], ao[k], static_cast<double>(ao[k])});
            st.nE = Z[a];
        } else {
            if (dfta_split_spin_ex(Z[a], aufbau, &nA, &nB, an, al, ao, bn, bl, bo, 32) != DFTA_OK) return DFTA_ERR_INVALID;
            int ne = 0;
            for (int k = 0; k < nA; ++k) { specs.push_back({2 * a, an[k], al[k], ao[k], static_cast<double>(ao[k])}); ne += ao[k]; }
            for (int k = 0; k < nB; ++k) specs.push_back({2 * a + 1, bn[k], bl[k], bo[k], static_cast<double>(bo[k])});
            st.nE = Z[a];
            st.nAlphaE = ne;
            st.nBetaE = Z[a] - ne;
        }
        s->spin_nlev[0][a] = nA;
        s->spin_nlev[1][a] = nB;
        st.job_end = (int)specs.size();
    }
    return DFTA_OK;
}
// ---- end of the replaced code --------------------------------------------------------------------------------------------------

// a batch as dfta_scf_create_config takes it (nlev empty: Aufbau)
struct Batch {
    std::vector<int> Z, nlev, n, l;
    std::vector<double> occ;
    void add(int z, int nA, int nB, const int* an, const int* al, const double* ao, const int* bn, const int* bl, const double* bo)
    {
        Z.push_back(z); nlev.push_back(nA); nlev.push_back(nB);
        n.insert(n.end(), an, an + nA); l.insert(l.end(), al, al + nA); occ.insert(occ.end(), ao, ao + nA);
        n.insert(n.end(), bn, bn + nB); l.insert(l.end(), bl, bl + nB); occ.insert(occ.end(), bo, bo + nB);
    }
};

// plans the batch with the planner and with the replaced loop; both must agree on refusal, and on everything when they accept.
// Returns the planner's status; *out (may be null): its plan
static int both(const char* what, const Batch& b, int lsda, int aufbau, dfta::ScfConfig* out = nullptr)
{
    const int natoms = static_cast<int>(b.Z.size());
    const bool expl = !b.nlev.empty();
    dfta::ScfConfig cfg;
    const int rc = dfta::plan_scf_config(natoms, b.Z.data(), expl ? b.nlev.data() : nullptr, b.n.data(), b.l.data(), b.occ.data(), lsda, aufbau, &cfg);
    dfta_ctx ctx;
    dfta_scf s;
    s.ctx = &ctx; s.lsda = lsda; s.natoms = natoms; s.nspin = lsda ? 2 : 1; s.nV = natoms * s.nspin;
    std::vector<dfta::JobSpec> specs;
    const int rrc = scf_configure(&s, b.Z.data(), expl ? b.nlev.data() : nullptr, b.n.data(), b.l.data(), b.occ.data(), aufbau, specs);
    CHECK((rc == DFTA_OK) == (rrc == DFTA_OK), "%s: planner %d (%s), replaced loop %d (%s)", what, rc, dfta_config_last_error(), rrc, ctx.err);
    CHECK(rc == DFTA_OK || rc == DFTA_ERR_INVALID, "%s: status %d", what, rc);
    if (rc != DFTA_OK) CHECK(dfta_config_last_error()[0] != 0, "%s: refused without a text", what);
    if (rc == DFTA_OK && rrc == DFTA_OK) {
        CHECK(cfg.specs.size() == specs.size() && cfg.bottom.size() == specs.size(), "%s: %zu jobs, %zu bottoms, replaced loop %zu", what, cfg.specs.size(), cfg.bottom.size(), specs.size());
        for (size_t k = 0; k < std::min(cfg.specs.size(), specs.size()); ++k) {
            const dfta::JobSpec &p = cfg.specs[k], &q = specs[k];
            CHECK(p.v == q.v && p.n == q.n && p.l == q.l && p.occ == q.occ && same_bits(p.docc, q.docc), "%s: job %zu is {%d %d %d %d %a}, replaced loop {%d %d %d %d %a}",
                  what, k, p.v, p.n, p.l, p.occ, p.docc, q.v, q.n, q.l, q.occ, q.docc);
            if (k < cfg.bottom.size()) CHECK(same_bits(cfg.bottom[k], s.h_bottom0[q.v]), "%s: bottom of job %zu %a, replaced loop %a", what, k, cfg.bottom[k], s.h_bottom0[q.v]);
        }
        CHECK(static_cast<int>(cfg.atoms.size()) == natoms && static_cast<int>(cfg.nlev[0].size()) == natoms && static_cast<int>(cfg.nlev[1].size()) == natoms, "%s: sizes", what);
        for (int a = 0; a < natoms && a < static_cast<int>(cfg.atoms.size()); ++a) {
            const dfta::AtomConfig& p = cfg.atoms[a];
            const AtomState& q = s.h_atoms[a];
            CHECK(p.Z == q.Z && p.job_off == q.job_off && p.job_end == q.job_end, "%s: atom %d Z %d jobs [%d, %d), replaced loop Z %d [%d, %d)", what, a, p.Z, p.job_off, p.job_end, q.Z, q.job_off, q.job_end);
            CHECK(cfg.nlev[0][a] == s.spin_nlev[0][a] && cfg.nlev[1][a] == s.spin_nlev[1][a], "%s: atom %d levels %d / %d, replaced loop %d / %d", what, a, cfg.nlev[0][a], cfg.nlev[1][a], s.spin_nlev[0][a], s.spin_nlev[1][a]);
            CHECK(same_bits(p.nE, q.nE), "%s: atom %d nE %a, replaced loop %a", what, a, p.nE, q.nE);
            if (lsda) CHECK(same_bits(p.nAlphaE, q.nAlphaE) && same_bits(p.nBetaE, q.nBetaE), "%s: atom %d electrons per spin %a / %a, replaced loop %a / %a", what, a, p.nAlphaE, p.nBetaE, q.nAlphaE, q.nBetaE);
        }
    }
    if (out) *out = cfg;
    return rc;
}

static bool same_plan(const dfta::ScfConfig& x, const dfta::ScfConfig& y)
{
    bool same = x.specs.size() == y.specs.size() && x.bottom == y.bottom && x.nlev[0] == y.nlev[0] && x.nlev[1] == y.nlev[1] && x.atoms.size() == y.atoms.size();
    for (size_t k = 0; same && k < x.specs.size(); ++k) same = memcmp(&x.specs[k], &y.specs[k], sizeof(dfta::JobSpec)) == 0;
    for (size_t a = 0; same && a < x.atoms.size(); ++a) {
        const dfta::AtomConfig &p = x.atoms[a], &q = y.atoms[a];
        same = p.Z == q.Z && same_bits(p.nE, q.nE) && same_bits(p.nAlphaE, q.nAlphaE) && same_bits(p.nBetaE, q.nBetaE) && p.job_off == q.job_off && p.job_end == q.job_end;
    }
    return same;
}

static bool add_ion(Batch& b, int Z, int q, int lsda, int aufbau)
{
    int nA = 0, nB = 0, an[32], al[32], bn[32], bl[32];
    double ao[32], bo[32];
    if (dfta_ion_config(Z, q, lsda, aufbau, 32, &nA, &nB, an, al, ao, bn, bl, bo) != DFTA_OK) return false;
    b.add(Z, nA, nB, an, al, ao, bn, bl, bo);
    return true;
}
static bool add_text(Batch& b, int Z, int lsda, const char* text)
{
    int nA = 0, nB = 0, an[32], al[32], bn[32], bl[32];
    double ao[32], bo[32];
    if (dfta_config_parse(Z, lsda, DFTA_AUFBAU_REFERENCE, text, 32, &nA, &nB, an, al, ao, bn, bl, bo) != DFTA_OK) return false;
    b.add(Z, nA, nB, an, al, ao, bn, bl, bo);
    return true;
}

static void plan()
{
    int cases = 0;
    char what[96];
    for (int lsda = 0; lsda < 2; ++lsda)
        for (int aufbau : {DFTA_AUFBAU_REFERENCE, DFTA_AUFBAU_TRANSITION_METALS}) {
            Batch all;
            for (int Z = 1; Z <= 118; ++Z) {
                all.Z.push_back(Z);
                Batch one;
                one.Z.push_back(Z);
                snprintf(what, sizeof(what), "Aufbau Z=%d lsda=%d aufbau=%d", Z, lsda, aufbau);
                dfta::ScfConfig auf, expl;
                CHECK(both(what, one, lsda, aufbau, &auf) == DFTA_OK, "%s refused: %s", what, dfta_config_last_error());
                ++cases;
                for (int q = 0; q <= 3 && q < Z; ++q) {
                    Batch ion;
                    snprintf(what, sizeof(what), "ion Z=%d q=%d lsda=%d aufbau=%d", Z, q, lsda, aufbau);
                    CHECK(add_ion(ion, Z, q, lsda, aufbau), "%s: dfta_ion_config: %s", what, dfta_config_last_error());
                    CHECK(both(what, ion, lsda, aufbau, &expl) == DFTA_OK, "%s refused: %s", what, dfta_config_last_error());
                    ++cases;
                    // the Aufbau plan is the plan of the explicit charge-0 configuration (LDA: nAlphaE = nE on both)
                    if (q == 0) CHECK(same_plan(auf, expl), "%s: differs from the Aufbau plan", what);
                }
            }
            snprintf(what, sizeof(what), "Aufbau Z=1..118 as one batch lsda=%d aufbau=%d", lsda, aufbau);
            dfta::ScfConfig cfg;
            CHECK(both(what, all, lsda, aufbau, &cfg) == DFTA_OK, "%s refused: %s", what, dfta_config_last_error());
            for (size_t a = 1; a < cfg.atoms.size(); ++a) CHECK(cfg.atoms[a].job_off == cfg.atoms[a - 1].job_end, "%s: atom %zu starts at %d", what, a, cfg.atoms[a].job_off);
            ++cases;
        }
    Batch frac, split;
    CHECK(add_text(frac, 18, 0, "[Ne] 3s2 3p5.5") && both("[Ne] 3s2 3p5.5", frac, 0, DFTA_AUFBAU_REFERENCE) == DFTA_OK, "refused: %s", dfta_config_last_error());
    CHECK(add_text(split, 7, 1, "[He] 2s2 2p2/1") && both("[He] 2s2 2p2/1", split, 1, DFTA_AUFBAU_REFERENCE) == DFTA_OK, "refused: %s", dfta_config_last_error());
    cases += 2;
    printf("plan: %d cases\n", cases);
}

// one atom, the levels of its two channels as {n, l, occ} rows (n: principal quantum number - 1)
struct L3 { int n, l; double occ; };
static Batch atom(int Z, const std::vector<L3>& alpha, const std::vector<L3>& beta = {})
{
    Batch b;
    b.Z.push_back(Z);
    b.nlev = {static_cast<int>(alpha.size()), static_cast<int>(beta.size())};
    for (const auto* ch : {&alpha, &beta})
        for (const L3& v : *ch) { b.n.push_back(v.n); b.l.push_back(v.l); b.occ.push_back(v.occ); }
    return b;
}

static void refusals()
{
    int cases = 0;
    auto refused = [&](const char* what, const Batch& b, int lsda) {
        CHECK(both(what, b, lsda, DFTA_AUFBAU_REFERENCE) == DFTA_ERR_INVALID, "%s accepted", what);
        ++cases;
    };
    Batch z0, z119;
    z0.Z = {0}; z119.Z = {119};
    refused("Aufbau Z = 0", z0, 0);
    refused("Aufbau Z = 119", z119, 1);
    refused("Z = 0", atom(0, {{0, 0, 1.}}), 0);
    refused("Z = 119", atom(119, {{0, 0, 1.}}), 0);
    refused("0 + 0 levels", atom(3, {}), 1);
    refused("33 levels", atom(3, std::vector<L3>(33, L3{0, 0, 1.})), 0);
    refused("beta levels in LDA", atom(3, {{0, 0, 1.}}, {{0, 0, 1.}}), 0);
    refused("l = -1", atom(3, {{0, -1, 1.}}), 0);
    refused("l = 4", atom(30, {{4, 4, 1.}}), 0);
    refused("n < l", atom(3, {{0, 1, 1.}}), 0);
    refused("a level twice", atom(5, {{0, 0, 1.}, {1, 0, 1.}, {0, 0, 1.}}), 0);
    refused("occupation 0", atom(3, {{0, 0, 0.}}), 0);
    refused("occupation -1", atom(3, {{0, 0, -1.}}), 0);
    refused("occupation NaN", atom(3, {{0, 0, std::numeric_limits<double>::quiet_NaN()}}), 0);
    refused("occupation above 2 (2l + 1) in LDA", atom(9, {{0, 0, 2.5}}), 0);
    refused("occupation above 2l + 1 in a spin channel", atom(9, {{0, 0, 1.5}}, {{0, 0, 1.}}), 1);
    refused("Z + 1 electrons", atom(2, {{0, 0, 2.}, {1, 0, 1.}}), 0);

    CHECK(both("Z + 1e-10 electrons", atom(3, {{0, 0, 2.}, {1, 0, 1. + 1e-10}}), 0, DFTA_AUFBAU_REFERENCE) == DFTA_OK, "refused: %s", dfta_config_last_error());
    ++cases;

    dfta::ScfConfig cfg;
    CHECK(both("unsorted levels", atom(7, {{1, 1, 3.}, {0, 0, 2.}, {1, 0, 2.}}), 0, DFTA_AUFBAU_REFERENCE, &cfg) == DFTA_OK, "refused: %s", dfta_config_last_error());
    for (size_t k = 1; k < cfg.specs.size(); ++k)
        CHECK(cfg.specs[k - 1].n < cfg.specs[k].n || (cfg.specs[k - 1].n == cfg.specs[k].n && cfg.specs[k - 1].l < cfg.specs[k].l), "jobs %zu, %zu not sorted by (n, l)", k - 1, k);
    CHECK(cfg.specs.size() == 3, "%zu jobs", cfg.specs.size());
    ++cases;

    Batch three;                                     // the third atom's 1s holds three electrons
    const int n0[] = {0}, l0[] = {0};
    const double two[] = {2.}, three_e[] = {3.};
    three.add(2, 1, 0, n0, l0, two, n0, l0, two);
    three.add(4, 1, 0, n0, l0, two, n0, l0, two);
    three.add(6, 1, 0, n0, l0, three_e, n0, l0, two);
    refused("a batch whose third atom is invalid", three, 0);
    CHECK(strstr(dfta_config_last_error(), "atom 2: ") != nullptr, "the text names no atom 2: %s", dfta_config_last_error());
    printf("refusals: %d cases\n", cases);
}

static void options()
{
    int cases = 0;
    const dfta::ScfFacts lda_log = {0, 0, 1, 0x1fu, 8};      // LDA, logarithmic grid, the scan and every rule fit
    const int lib = static_cast<int>(sizeof(dfta_scf_options));
    const dfta_scf_options defaults = {lib, DFTA_INT_SIMPSON38, DFTA_XC_VWN, DFTA_AUFBAU_REFERENCE, -1, DFTA_SWEEPS_EXACT, DFTA_MIX_LINEAR, 4, 3};
    dfta_scf_options got;
    CHECK(dfta::resolve_scf_options(nullptr, lda_log, &got) == nullptr && memcmp(&got, &defaults, sizeof(got)) == 0, "no options: not the defaults");
    ++cases;

    // a caller's struct of every size: valid members, none of them the default
    const dfta_scf_options given = {0, DFTA_INT_BOOLE, DFTA_XC_PW92, DFTA_AUFBAU_TRANSITION_METALS, DFTA_POISSON_TOLERANCE, DFTA_SWEEPS_TOLERANCE, DFTA_MIX_ANDERSON, 5, 7};
    std::vector<int> sizes;
    for (int sz = 8; sz <= lib; sz += 4) sizes.push_back(sz);
    sizes.push_back(lib + 4);
    sizes.push_back(4096);
    for (int sz : sizes) {
        std::vector<int> user(std::max(sz, lib) / sizeof(int), 0x5a5a5a5a);      // exactly the caller's bytes (a longer struct: unknown members behind)
        memcpy(user.data(), &given, std::min(sz, lib));
        user[0] = sz;
        const char* why = dfta::resolve_scf_options(reinterpret_cast<const dfta_scf_options*>(user.data()), lda_log, &got);
        CHECK(why == nullptr, "struct_size %d refused: %s", sz, why);
        ++cases;
        if (why) continue;
        CHECK(got.struct_size == lib, "struct_size %d: the result's is %d", sz, got.struct_size);
        const int *g = reinterpret_cast<const int*>(&got), *in = reinterpret_cast<const int*>(&given), *def = reinterpret_cast<const int*>(&defaults);
        for (int m = 1; m < lib / static_cast<int>(sizeof(int)); ++m) {
            const bool inside = (m + 1) * static_cast<int>(sizeof(int)) <= sz;
            CHECK(g[m] == (inside ? in[m] : def[m]), "struct_size %d: member %d is %d (%s: %d)", sz, m, g[m], inside ? "given" : "default", inside ? in[m] : def[m]);
        }
    }
    for (int sz : {0, 4, 6, 4100}) {
        std::vector<int> user(4100 / sizeof(int) + 1, 0);
        user[0] = sz;
        const char* why = dfta::resolve_scf_options(reinterpret_cast<const dfta_scf_options*>(user.data()), lda_log, &got);
        CHECK(why && strstr(why, "struct_size"), "struct_size %d: %s", sz, why ? why : "accepted");
        ++cases;
    }

    // one refusal per range check, with the text dfta_scf_create_config has always given
    auto refuse = [&](const char* text, const dfta::ScfFacts& f, int dfta_scf_options::*member, int value) {
        dfta_scf_options o = {lib, DFTA_INT_SIMPSON38, 0, 0, 0, 0, 0, 0, 0};
        o.*member = value;
        const char* why = dfta::resolve_scf_options(&o, f, &got);
        CHECK(why && !strcmp(why, text), "member = %d: '%s', expected '%s'", value, why ? why : "accepted", text);
        ++cases;
    };
    dfta::ScfFacts lsda_log = lda_log, lda_uniform = lda_log, no_scan = lda_log, odd_N = lda_log;
    lsda_log.lsda = 1; lda_uniform.uniform = 1; no_scan.scan_ok = 0; odd_N.integrators_fit = 0x17u;      // Boole does not fit
    refuse("poisson mode", lda_log, &dfta_scf_options::poisson_mode, -2);
    refuse("poisson mode", lda_log, &dfta_scf_options::poisson_mode, DFTA_POISSON_ADAPTIVE + 1);
    refuse("integration rule / grid size", lda_log, &dfta_scf_options::integrator, -1);
    refuse("integration rule / grid size", lda_log, &dfta_scf_options::integrator, DFTA_INT_ROMBERG + 1);
    refuse("integration rule / grid size", odd_N, &dfta_scf_options::integrator, DFTA_INT_BOOLE);
    refuse("functional (DFTA_XC_VWN .. DFTA_XC_PBE)", lda_log, &dfta_scf_options::functional, -1);
    refuse("functional (DFTA_XC_VWN .. DFTA_XC_PBE)", lda_log, &dfta_scf_options::functional, DFTA_XC_PBE + 1);
    refuse("the Chachiyo functional is LDA only (ExcCor.h)", lsda_log, &dfta_scf_options::functional, DFTA_XC_CHACHIYO);
    refuse("the Chachiyo functional is LDA only (ExcCor.h)", lsda_log, &dfta_scf_options::functional, DFTA_XC_CHACHIYO_IMPROVED);
    refuse("the PBE functional needs a logarithmic grid (no GGA on the uniform grid)", lda_uniform, &dfta_scf_options::functional, DFTA_XC_PBE);
    refuse("aufbau", lda_log, &dfta_scf_options::aufbau, 2);
    refuse("sweep mode", lda_log, &dfta_scf_options::sweep_mode, 2);
    refuse("the tolerance mode of the sweeps needs a logarithmic grid of 12 .. 20 multigrid levels", no_scan, &dfta_scf_options::sweep_mode, DFTA_SWEEPS_TOLERANCE);
    refuse("mixing (DFTA_MIX_LINEAR / DFTA_MIX_ANDERSON)", lda_log, &dfta_scf_options::mixing, 2);
    refuse("mix_history (1 .. 8; 0: the default, 4)", lda_log, &dfta_scf_options::mix_history, -1);
    refuse("mix_history (1 .. 8; 0: the default, 4)", lda_log, &dfta_scf_options::mix_history, 9);
    refuse("mix_warmup (1 .. 100; 0: the default, 3)", lda_log, &dfta_scf_options::mix_warmup, -1);
    refuse("mix_warmup (1 .. 100; 0: the default, 3)", lda_log, &dfta_scf_options::mix_warmup, 101);
    // ... and what those checks let through: Chachiyo in LDA, PBE on the logarithmic grid, the scan where it is supported
    for (int fn : {DFTA_XC_CHACHIYO, DFTA_XC_PBE}) {
        dfta_scf_options o = {lib, DFTA_INT_SIMPSON38, fn, 0, 0, DFTA_SWEEPS_TOLERANCE, 0, 0, 0};
        const char* why = dfta::resolve_scf_options(&o, lda_log, &got);
        CHECK(why == nullptr && got.functional == fn && got.poisson_mode == 0, "functional %d: %s", fn, why ? why : "accepted, wrong members");
        ++cases;
    }

    // the statistics: the library's struct into a caller's shorter or longer one
    const size_t slib = sizeof(dfta_step_stats);
    dfta_step_stats mine;
    memset(&mine, 0x11, sizeof(mine));
    mine.struct_size = static_cast<int>(slib);
    for (int sz : {16, static_cast<int>(slib), static_cast<int>(slib) + 32}) {
        std::vector<unsigned char> user(std::max<size_t>(static_cast<size_t>(sz), slib) + 16, 0xEE);      // the caller's struct, then a guard
        CHECK(dfta::copy_versioned(user.data(), &mine, sz, dfta::kStatsMinSize, slib, sz), "statistics of %d bytes refused", sz);
        const size_t filled = std::min<size_t>(static_cast<size_t>(sz), slib);
        int kept = 0;
        memcpy(&kept, user.data(), sizeof(int));
        CHECK(kept == sz, "statistics of %d bytes: struct_size came back as %d", sz, kept);
        CHECK(memcmp(user.data() + sizeof(int), reinterpret_cast<const unsigned char*>(&mine) + sizeof(int), filled - sizeof(int)) == 0, "statistics of %d bytes: the common part differs", sz);
        for (size_t i = filled; i < user.size(); ++i)
            if (user[i] != 0xEE) { CHECK(false, "statistics of %d bytes: byte %zu written", sz, i); break; }
        ++cases;
    }
    for (int sz : {0, 12, 18, 4100}) {
        std::vector<unsigned char> user(4200, 0xEE);
        CHECK(!dfta::copy_versioned(user.data(), &mine, sz, dfta::kStatsMinSize, slib, sz) && !dfta::versioned_size_ok(sz, dfta::kStatsMinSize), "statistics of %d bytes accepted", sz);
        CHECK(std::all_of(user.begin(), user.end(), [](unsigned char c) { return c == 0xEE; }), "statistics of %d bytes: refused, yet written", sz);
        ++cases;
    }
    printf("options: %d cases\n", cases);
}

int main(int argc, char** argv)
{
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "plan") plan();
    else if (mode == "refusals") refusals();
    else if (mode == "options") options();
    else { printf("usage: scf_config_main plan | refusals | options\n"); return 2; }
    printf("%d violations\n", g_violations);
    return g_violations ? 1 : 0;
}
