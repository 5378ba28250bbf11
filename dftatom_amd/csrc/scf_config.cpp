// scf_config.cpp -- the pure host logic of the SCF layer (scf_config.h): integer and text only, no device, no environment.
#include "scf_config.h"

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

extern "C" {

// ---- Aufbau (integer only; AufbauPrinciple.h:36-75,101-117 and DFTAtom.cpp:367, 611-638) -----------------
static void adjust_f_block(int& nrElectrons, int Z, int N, int L)
{
    if (L == 3) {
        if ((Z == 57 || Z == 58 || Z == 64) && N == 3) --nrElectrons;      // La, Ce, Gd: one 4f electron goes to 5d
        else if (N == 4) {
            if (Z == 89 || Z == 90) nrElectrons = 0;                        // Ac, Th
            else if (Z == 91 || Z == 92 || Z == 93 || Z == 96) --nrElectrons; // Pa, U, Np, Cm
        }
    } else if (Z == 103 && N == 5 && L == 2) nrElectrons = 0;              // Lr
}

// AufbauPrinciple.h:78-99,119-127: the s shell under a d shell that the Madelung rule leaves one (Pd: two) short hands
// the electron(s) over.  The reference defines this adjustment but never calls it (Cr comes out as 3d4 4s2); here it is an
// option, applied once, after the clamp to the electrons that are left (an s shell is never clamped, so once is enough).
static void adjust_transition_metal(int& nrElectrons, int Z, int N, int L)
{
    if (L != 0) return;
    const bool one = (Z == 24 || Z == 29 || Z == 41 || Z == 42 || Z == 44 || Z == 45 || Z == 47 || Z == 78 || Z == 79);
    if (one) {
        const int outer_s = Z <= 29 ? 3 : (Z <= 47 ? 4 : 5);              // 4s, 5s, 6s
        if (N == outer_s) --nrElectrons;
    } else if (Z == 46 && N == 4) nrElectrons -= 2;                        // Pd: 4d10 5s0
}

int dfta_get_subshells(int Z, int* n, int* l, int* occ, int cap) { return dfta_get_subshells_ex(Z, DFTA_AUFBAU_REFERENCE, n, l, occ, cap); }

int dfta_get_subshells_ex(int Z, int aufbau, int* n, int* l, int* occ, int cap)
{
    if (Z < 1 || !n || !l || !occ) return -1;
    struct S { int n, l, occ; };
    std::vector<S> lv;
    int electronCount = 0;
    bool stop = false;
    for (int NplusL = 0; !stop && NplusL < 10; ++NplusL)
        for (int N = 0; N <= NplusL; ++N) {
            const int L = NplusL - N;
            if (L > N) continue;
            int e = 2 * (2 * L + 1);
            adjust_f_block(e, Z, N, L);
            if (Z - electronCount < e) e = Z - electronCount;
            adjust_f_block(e, Z, N, L);
            if (aufbau == DFTA_AUFBAU_TRANSITION_METALS) adjust_transition_metal(e, Z, N, L);
            if (e > 0) { electronCount += e; lv.push_back({N, L, e}); }
            if (electronCount == Z) { stop = true; break; }
        }
    std::sort(lv.begin(), lv.end(), [](const S& a, const S& b) { return a.n < b.n || (a.n == b.n && a.l < b.l); });
    if (static_cast<int>(lv.size()) > cap) return -1;
    for (size_t i = 0; i < lv.size(); ++i) { n[i] = lv[i].n; l[i] = lv[i].l; occ[i] = lv[i].occ; }
    return static_cast<int>(lv.size());
}

int dfta_split_spin(int Z, int* nA, int* nB, int* an, int* al, int* aocc, int* bn, int* bl, int* bocc, int cap)
{
    return dfta_split_spin_ex(Z, DFTA_AUFBAU_REFERENCE, nA, nB, an, al, aocc, bn, bl, bocc, cap);
}

int dfta_split_spin_ex(int Z, int aufbau, int* nA, int* nB, int* an, int* al, int* aocc, int* bn, int* bl, int* bocc, int cap)
{
    if (!nA || !nB) return DFTA_ERR_INVALID;
    const int cnt = dfta_get_subshells_ex(Z, aufbau, an, al, aocc, cap);
    if (cnt < 0) return DFTA_ERR_INVALID;
    int m = 0;
    for (int i = 0; i < cnt; ++i) {
        const int maxe = 2 * al[i] + 1;
        int b;
        if (aocc[i] >= maxe) { b = aocc[i] - maxe; aocc[i] = maxe; }
        else b = 0;
        if (b != 0) { bn[m] = an[i]; bl[m] = al[i]; bocc[m] = b; ++m; }
    }
    *nA = cnt;
    *nB = m;
    return DFTA_OK;
}

}  // extern "C"

// ---- electron configurations (host only): text, charge rule, validation ----------------------------------------------------
namespace {

thread_local char g_config_err[160] = "";

int config_fail(const char* fmt, ...) __attribute__((format(printf, 1, 2)));
int config_fail(const char* fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_config_err, sizeof(g_config_err), fmt, ap);
    va_end(ap);
    return DFTA_ERR_INVALID;
}

struct Sub {
    int n, l;            // n: principal quantum number - 1, as dfta_get_subshells_ex reports it (the reference's m_N)
    double occ;          // total
    bool split;          // LSDA: alpha / beta given explicitly
    double a, b;
    bool core;           // taken from a noble-gas core (a token may replace it)
};

const char kSpd[] = "spdf";

// the Aufbau configuration of Z as subshells, sorted by (n, l)
int aufbau_subs(int Z, int aufbau, std::vector<Sub>& out)
{
    int n[32], l[32], o[32];
    const int cnt = dfta_get_subshells_ex(Z, aufbau, n, l, o, 32);
    if (cnt < 0) return config_fail("no Aufbau configuration for Z = %d", Z);
    out.clear();
    for (int k = 0; k < cnt; ++k) out.push_back({n[k], l[k], static_cast<double>(o[k]), false, 0., 0., true});
    return DFTA_OK;
}

// THE rules of a configuration, for emit (subshells, who = "") and for plan_scf_config (the levels of a spin channel, who = "atom <a>: ")
int check_Z(const char* who, int Z)
{
    return Z < 1 || Z > 118 ? config_fail("%sZ = %d out of range 1 .. 118", who, Z) : DFTA_OK;
}
// a level of a list sorted by (n, l); twice: it equals the one before it; full: what it holds at most
int check_level(const char* who, int n, int l, double occ, bool twice, double full)
{
    if (l < 0 || l > 3 || n < l) return config_fail("%slevel n = %d, l = %d: needs 0 <= l < n and l <= 3", who, n + 1, l);
    if (twice) return config_fail("%s%d%c given twice", who, n + 1, kSpd[l]);
    if (!(occ > 0) || occ > full) return config_fail("%s%d%c: occupation %g outside (0, %g]", who, n + 1, kSpd[l], occ, full);
    return DFTA_OK;
}
int check_electrons(const char* who, double ne, int Z)
{
    if (!(ne > 0)) return config_fail("%sno electrons", who);
    if (ne > Z + 1e-9) return config_fail("%s%g electrons for Z = %d: anions are not supported", who, ne, Z);
    return DFTA_OK;
}

// validation, the spin split and the output arrays (alpha levels, then beta levels; LDA: alpha only)
int emit(int Z, int lsda, std::vector<Sub> subs, int cap, int* nA, int* nB, int* an, int* al, double* aocc, int* bn, int* bl,
         double* bocc)
{
    if (int rc = check_Z("", Z)) return rc;
    std::stable_sort(subs.begin(), subs.end(), [](const Sub& x, const Sub& y) { return x.n < y.n || (x.n == y.n && x.l < y.l); });
    double ne = 0;
    for (size_t k = 0; k < subs.size(); ++k) {
        const Sub& s = subs[k];
        const double full = 2. * (2 * s.l + 1);
        if (int rc = check_level("", s.n, s.l, s.occ, k > 0 && subs[k - 1].n == s.n && subs[k - 1].l == s.l, full)) return rc;
        if (s.split && (!(s.a >= 0) || !(s.b >= 0) || s.a > full / 2 || s.b > full / 2))
            return config_fail("%d%c: spin occupations %g / %g outside [0, %g]", s.n + 1, kSpd[s.l], s.a, s.b, full / 2);
        ne += s.occ;
    }
    if (int rc = check_electrons("", ne, Z)) return rc;
    int ka = 0, kb = 0;
    for (const Sub& s : subs) {
        double a = s.occ, b = 0;
        if (lsda) {
            const double maxe = 2 * s.l + 1;                 // DFTAtom.cpp:611-638 / dfta_split_spin_ex
            if (s.split) { a = s.a; b = s.b; }
            else if (s.occ >= maxe) { a = maxe; b = s.occ - maxe; }
        }
        if (a != 0) {
            if (ka >= cap) return config_fail("more than %d levels", cap);
            an[ka] = s.n; al[ka] = s.l; aocc[ka] = a; ++ka;
        }
        if (b != 0) {
            if (kb >= cap) return config_fail("more than %d levels", cap);
            bn[kb] = s.n; bl[kb] = s.l; bocc[kb] = b; ++kb;
        }
    }
    *nA = ka;
    *nB = kb;
    g_config_err[0] = 0;
    return DFTA_OK;
}

bool parse_number(const char*& p, double& v)
{
    if (!((*p >= '0' && *p <= '9') || *p == '.')) return false;
    char* end = nullptr;
    v = strtod(p, &end);
    if (end == p) return false;
    p = end;
    return true;
}

// dfta_ion_config behind its argument checks; charge 0 is the Aufbau configuration as plan_scf_config takes it
int ion_config(int Z, int charge, int lsda, int aufbau, int cap, int* nA, int* nB, int* an, int* al, double* aocc, int* bn, int* bl,
               double* bocc)
{
    std::vector<Sub> subs;
    if (int rc = aufbau_subs(Z, aufbau, subs)) return rc;
    // the electrons leave the subshell of highest n, ties to the highest l (Fe+ = 3d6 4s1), one subshell after the other
    for (int q = charge; q > 0;) {
        size_t top = 0;
        for (size_t k = 1; k < subs.size(); ++k)
            if (subs[k].n > subs[top].n || (subs[k].n == subs[top].n && subs[k].l > subs[top].l)) top = k;
        const int take = std::min<int>(q, static_cast<int>(subs[top].occ));
        subs[top].occ -= take;
        q -= take;
        if (subs[top].occ == 0) subs.erase(subs.begin() + static_cast<long>(top));
    }
    return emit(Z, lsda, subs, cap, nA, nB, an, al, aocc, bn, bl, bocc);
}

}  // namespace

extern "C" {

const char* dfta_config_last_error(void) { return g_config_err; }

int dfta_config_parse(int Z, int lsda, int aufbau, const char* text, int cap, int* nA, int* nB, int* an, int* al, double* aocc,
                      int* bn, int* bl, double* bocc)
{
    if (!text || !nA || !nB || !an || !al || !aocc || (lsda && (!bn || !bl || !bocc))) return config_fail("null argument");
    if (aufbau != DFTA_AUFBAU_REFERENCE && aufbau != DFTA_AUFBAU_TRANSITION_METALS) return config_fail("aufbau option %d", aufbau);
    std::vector<Sub> subs;
    const char* p = text;
    bool any = false;
    for (;;) {
        while (*p == ' ' || *p == '\t' || *p == '\n' || *p == '\r') ++p;
        if (!*p) break;
        const char* tok = p;
        while (*p && *p != ' ' && *p != '\t' && *p != '\n' && *p != '\r') ++p;
        const std::string t(tok, p);
        if (t[0] == '[') {
            static const char* const gas[] = {"[He]", "[Ne]", "[Ar]", "[Kr]", "[Xe]", "[Rn]"};
            static const int gasZ[] = {2, 10, 18, 36, 54, 86};
            int zc = 0;
            for (int k = 0; k < 6; ++k) if (t == gas[k]) zc = gasZ[k];
            if (!zc) return config_fail("unknown core '%s' (one of [He] [Ne] [Ar] [Kr] [Xe] [Rn])", t.c_str());
            if (any) return config_fail("the core '%s' must come first", t.c_str());
            if (int rc = aufbau_subs(zc, aufbau, subs)) return rc;
            any = true;
            continue;
        }
        any = true;
        const char* q = t.c_str();
        char* end = nullptr;
        const long n = strtol(q, &end, 10);
        if (end == q || n < 1 || n > 99) return config_fail("'%s': expected <n><spdf><occupation>", t.c_str());
        q = end;
        const char* lc = *q ? strchr(kSpd, *q) : nullptr;
        if (!lc) return config_fail("'%s': expected <n><spdf><occupation>", t.c_str());
        ++q;
        Sub s{static_cast<int>(n) - 1, static_cast<int>(lc - kSpd), 0., false, 0., 0., false};
        if (!parse_number(q, s.occ)) return config_fail("'%s': missing occupation", t.c_str());
        if (*q == '/') {
            if (!lsda) return config_fail("'%s': an alpha / beta split needs LSDA", t.c_str());
            ++q;
            s.a = s.occ;
            if (!parse_number(q, s.b)) return config_fail("'%s': missing beta occupation", t.c_str());
            s.split = true;
            s.occ = s.a + s.b;
        }
        if (*q) return config_fail("'%s': trailing characters", t.c_str());
        bool dup = false;
        for (Sub& x : subs)
            if (x.n == s.n && x.l == s.l) {
                if (!x.core) return config_fail("%d%c given twice", s.n + 1, kSpd[s.l]);
                x = s;                                         // replaces what the core holds there
                dup = true;
            }
        if (!dup) subs.push_back(s);
    }
    if (!any) return config_fail("empty configuration");
    std::vector<Sub> kept;
    for (const Sub& s : subs) if (s.occ != 0) kept.push_back(s);       // occupation 0 removes the subshell
    return emit(Z, lsda, kept, cap, nA, nB, an, al, aocc, bn, bl, bocc);
}

int dfta_ion_config(int Z, int charge, int lsda, int aufbau, int cap, int* nA, int* nB, int* an, int* al, double* aocc,
                    int* bn, int* bl, double* bocc)
{
    if (!nA || !nB || !an || !al || !aocc || (lsda && (!bn || !bl || !bocc))) return config_fail("null argument");
    if (int rc = check_Z("", Z)) return rc;
    if (aufbau != DFTA_AUFBAU_REFERENCE && aufbau != DFTA_AUFBAU_TRANSITION_METALS) return config_fail("aufbau option %d", aufbau);
    if (charge < 0) return config_fail("charge %d: anions are not supported", charge);
    if (charge >= Z) return config_fail("charge %d leaves no electrons for Z = %d", charge, Z);
    return ion_config(Z, charge, lsda, aufbau, cap, nA, nB, an, al, aocc, bn, bl, bocc);
}

}  // extern "C"

namespace dfta {

int plan_scf_config(int natoms, const int* Z, const int* nlev, const int* cn, const int* cl, const double* cocc, int lsda, int aufbau,
                    ScfConfig* out)
{
    *out = ScfConfig();
    out->atoms.resize(natoms);
    out->nlev[0].resize(natoms); out->nlev[1].resize(natoms);
    struct Lev { int n, l; double occ; };
    std::vector<Lev> lev;
    size_t coff = 0;                                           // running offset into the caller's n / l / occ
    for (int a = 0; a < natoms; ++a) {
        char who[24];
        snprintf(who, sizeof(who), "atom %d: ", a);
        if (int rc = check_Z(who, Z[a])) return rc;
        int an[32], al[32], bn[32], bl[32], cnt[2];
        double ao[32], bo[32];
        const int *n[2] = {an, bn}, *l[2] = {al, bl};          // the levels of the two channels
        const double* occ[2] = {ao, bo};
        if (nlev) {                                            // explicit configuration (fractional occupations, cations)
            cnt[0] = nlev[2 * a]; cnt[1] = nlev[2 * a + 1];
            if (cnt[0] < 0 || cnt[1] < 0 || cnt[0] + cnt[1] < 1 || cnt[0] > 32 || cnt[1] > 32 || (!lsda && cnt[1] != 0))
                return config_fail("%slevel counts %d / %d (1 .. 32 levels; LDA: no beta levels)", who, cnt[0], cnt[1]);
            for (int spin = 0; spin < 2; ++spin) {
                n[spin] = cn + coff; l[spin] = cl + coff; occ[spin] = cocc + coff;
                coff += static_cast<size_t>(cnt[spin]);
            }
        } else if (int rc = ion_config(Z[a], 0, lsda, aufbau, 32, &cnt[0], &cnt[1], an, al, ao, bn, bl, bo)) return rc;     // Aufbau
        AtomConfig& at = out->atoms[a];
        at.Z = Z[a];
        at.job_off = static_cast<int>(out->specs.size());
        double ne = 0, neA = 0;
        for (int spin = 0; spin < (lsda ? 2 : 1); ++spin) {    // a channel: sorted by (n, l) (DFTAtom.cpp:367), checked, its jobs
            lev.clear();
            for (int k = 0; k < cnt[spin]; ++k) lev.push_back({n[spin][k], l[spin][k], occ[spin][k]});
            std::stable_sort(lev.begin(), lev.end(), [](const Lev& x, const Lev& y) { return x.n < y.n || (x.n == y.n && x.l < y.l); });
            for (size_t k = 0; k < lev.size(); ++k) {
                const Lev& v = lev[k];
                if (int rc = check_level(who, v.n, v.l, v.occ, k > 0 && lev[k - 1].n == v.n && lev[k - 1].l == v.l, (lsda ? 1. : 2.) * (2 * v.l + 1)))
                    return rc;
                ne += v.occ;
                const int io = (v.occ == std::floor(v.occ)) ? static_cast<int>(v.occ) : 0;     // Job::occ: the integer, 0 for a fractional one
                out->specs.push_back({lsda ? 2 * a + spin : a, v.n, v.l, io, v.occ});
                out->bottom.push_back(-double(Z[a]) * Z[a] - 1.);
            }
            if (spin == 0) neA = ne;
        }
        if (int rc = check_electrons(who, ne, Z[a])) return rc;
        at.nE = ne; at.nAlphaE = neA; at.nBetaE = ne - neA;
        at.job_end = static_cast<int>(out->specs.size());
        out->nlev[0][a] = cnt[0]; out->nlev[1][a] = cnt[1];
    }
    return DFTA_OK;
}

bool versioned_size_ok(int user_size, size_t min_size)
{
    return user_size >= static_cast<int>(min_size) && user_size % static_cast<int>(sizeof(int)) == 0 && user_size <= 4096;
}

bool copy_versioned(void* dst, const void* src, int user_size, size_t min_size, size_t lib_size, int dst_struct_size)
{
    if (!versioned_size_ok(user_size, min_size)) return false;
    memcpy(dst, src, std::min(static_cast<size_t>(user_size), lib_size));
    memcpy(dst, &dst_struct_size, sizeof(int));
    return true;
}

const char* resolve_scf_options(const dfta_scf_options* user, const ScfFacts& f, dfta_scf_options* out)
{
    dfta_scf_options opt = {(int)sizeof(dfta_scf_options), DFTA_INT_SIMPSON38, DFTA_XC_VWN, DFTA_AUFBAU_REFERENCE, -1, DFTA_SWEEPS_EXACT, DFTA_MIX_LINEAR, 0, 0};
    // the caller's struct may be shorter (an older header) or longer (a newer one) than this library's: members it does not have keep the
    // defaults above; those it has are taken as they are (0 = the reference's behaviour)
    if (user && !copy_versioned(&opt, user, user->struct_size, kOptionsMinSize, sizeof(opt), (int)sizeof(opt)))
        return "dfta_scf_options::struct_size (set it to sizeof(dfta_scf_options))";
    if (opt.poisson_mode < -1 || opt.poisson_mode > DFTA_POISSON_ADAPTIVE) return "poisson mode";
    if (opt.integrator < 0 || opt.integrator > DFTA_INT_ROMBERG || !((f.integrators_fit >> opt.integrator) & 1u)) return "integration rule / grid size";
    if (opt.functional < DFTA_XC_VWN || opt.functional > DFTA_XC_PBE) return "functional (DFTA_XC_VWN .. DFTA_XC_PBE)";
    if ((opt.functional == DFTA_XC_CHACHIYO || opt.functional == DFTA_XC_CHACHIYO_IMPROVED) && f.lsda) return "the Chachiyo functional is LDA only (ExcCor.h)";
    if (opt.functional == DFTA_XC_PBE && f.uniform) return "the PBE functional needs a logarithmic grid (no GGA on the uniform grid)";
    if (opt.aufbau != DFTA_AUFBAU_REFERENCE && opt.aufbau != DFTA_AUFBAU_TRANSITION_METALS) return "aufbau";
    if (opt.sweep_mode != DFTA_SWEEPS_EXACT && opt.sweep_mode != DFTA_SWEEPS_TOLERANCE) return "sweep mode";
    if (opt.sweep_mode != DFTA_SWEEPS_EXACT && !f.scan_ok) return "the tolerance mode of the sweeps needs a logarithmic grid of 12 .. 20 multigrid levels";
    if (opt.mixing != DFTA_MIX_LINEAR && opt.mixing != DFTA_MIX_ANDERSON) return "mixing (DFTA_MIX_LINEAR / DFTA_MIX_ANDERSON)";
    if (opt.mix_history < 0 || opt.mix_history > f.mix_history_max) return "mix_history (1 .. 8; 0: the default, 4)";
    if (opt.mix_warmup < 0 || opt.mix_warmup > 100) return "mix_warmup (1 .. 100; 0: the default, 3)";
    if (!opt.mix_history) opt.mix_history = 4;
    if (!opt.mix_warmup) opt.mix_warmup = 3;
    *out = opt;
    return nullptr;
}

}  // namespace dfta
