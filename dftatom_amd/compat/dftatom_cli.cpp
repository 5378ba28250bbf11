// dftatom_cli.cpp -- headless stand-in for the wxWidgets front end (DFTAtomFrame.cpp:174-199 + Options.h:48-54).
//
//   dftatom_cli Z MultigridLevels alpha MaxR deltaGrid method [chained] [--integrator=NAME] [--xc=NAME]
//   dftatom_cli --ini DFTAtom.ini [chained] [--integrator=NAME] [--uniform]
//
// method: 0 = LDA, 1 = LSDA (the two the GUI reaches, DFTAtomFrame.cpp:190-195); 2 / 3 = the uniform-grid entry points
// CalculateUniformLDA / LSDA, which the GUI has commented out.  --ini reads the keys the reference persists with
// wxFileConfig (Options.cpp:42-49: Z, MultigridLevels, MaxR, deltaGrid, alpha, Method; same defaults: 36, 12, 10, 0.001,
// 0.5, 0), one `key=value` per line, an optional leading '/' and [section] lines ignored.  Values are validated like the
// options dialog does (OptionsFrame.cpp:46,152-175: Z 1..118, levels 10..20, MaxR 1..90, deltaGrid in (0, 1], alpha in [0, 1]);
// any other method value is refused (exit code 2).
// --integrator: trapezoid | simpson13 | simpson38 (default, what the reference calls) | boole | romberg (README.md:81).
// --json[=FILE]: one JSON line per SCF step (17-digit energies and eigenvalues, per-level status bits and sweep counts, rounds, V-cycles,
//                phase times) to FILE, or to stderr -- the console protocol on stdout stays the reference's.
// --orbital-table: after "Finished!", one line per level with n, l, occupation, E and <r>, <r^2>, the kinetic energy T and r_peak of its
//                orbital (atomic units; include/dftatom_hip.h: dfta_scf_orbital_properties).  Without it the output is unchanged.
// --slater-table: after "Finished!" (and the orbital table), one line per Slater integral F^k(a,b), G^k(a,b) of the levels (per spin
//                channel with LSDA), then one line with the Hartree energy and the exact-exchange energy of the orbitals (atomic units;
//                include/dftatom_hip.h: dfta_scf_slater_fg, dfta_scf_coulomb_exchange).  Without it the output is unchanged.
// --exchange-table: after "Finished!" (and the Slater table), one line per shell (per spin channel with LSDA) with its eigenvalue, the
//                orbital averages vbarHF, vbarS, vbarKLI of the Fock, Slater and KLI exchange potentials and the KLI constant c, then one
//                line with E_x = 1/2 Sum n vbarHF and r vKLI at the outermost node where the channel's density is positive (atomic
//                units; include/dftatom_hip.h: dfta_scf_exchange_potentials).  Without it the output is unchanged.
// --form-factor-table[=smax:ns]: after "Finished!" (and the other tables), one line per s = sin(theta) / lambda = smax k / (ns - 1), k = 0 ..
//                ns - 1 (1 / Angstrom; default 0 .. 2 in 41 points): s, q = 4 pi s 0.529177210903 (atomic units) and the X-ray form factor
//                f(q) of the converged density; LSDA adds the magnetic form factor f_a - f_b (include/dftatom_hip.h:
//                dfta_scf_form_factors, one launch for the table).  Without it the output is unchanged.
// --phase-shift-table[=emax:ne]: after "Finished!" (and the other tables), one line per spin channel, l = 0 .. 4 and E = emax k / ne, k = 1 .. ne
//                (Ha; default 2:8): the scattering phase shift delta_l(E) of the converged potential, u'/u at the last node but one and the
//                node count of the outward solution (include/dftatom_hip.h: dfta_scf_continuum, one launch for the table).  With
//                --charge, --config or --exchange=kli|sic the potential has a Coulomb tail: the column is the WKB phase instead.
// --kb-table[=elo:ehi:ne]: after "Finished!" (and the other tables), the Kleinman-Bylander form of the default valence levels' pseudopotentials
//                (the highest l local): per channel E_KB, the bound states of H_KB, both ghost verdicts (dfta_kb_ghost_report), then u'/u at
//                the largest core radius in the all-electron potential, in V_ps,l and in H_KB at ne energies in elo .. ehi Ha (default -2:1:7).
// --photo-table[=emax:ne]: then one line per subshell and photoelectron energy eps = emax k / ne (default 4:8): the photon energy
//                omega = eps - E_nl and the photoionization cross section sigma_nl(omega) in a_0^2 and megabarn (dfta_scf_photoionization).
//                Without them the output is unchanged.
// --sweeps=exact|tolerance, --poisson=exact|tolerance|adaptive: the opt-in tolerance modes of the device path (include/dftatom_hip.h).
// --mixing=linear (default, the reference's density mixing) | anderson (Anderson acceleration: about half the SCF steps, same protocol).
// --exchange=functional (default) | kli: self-consistent exchange-only KLI -- every step's exchange potential from its own orbitals, no
//                correlation (with --xc=vwn and --mixing=linear only); same protocol, --exchange-table works on top of it.
// --exchange=sic: self-interaction-corrected LSDA -- VWN plus the Perdew-Zunger correction as one KLI potential per spin channel (-1/r tail,
//                HOMO near -IP; --xc=vwn and --mixing=linear only); same protocol.
// --sic-table:   with --exchange=sic, after "Finished!" one line per shell (per spin channel with LSDA) with its eigenvalue, the self-Hartree
//                and self-xc energies EH, EXC of one electron in it, <a|v_a^SIC|a> and the KLI constant c, then E_SIC.  Changes nothing else.
// --xc=vwn (default, what the reference runs) | chachiyo | chachiyo-improved (LDA only) | pw92 | pbe (logarithmic grid only).
// --charge=q: the cation X^q+ (electrons leave the subshell of highest n, then highest l: Fe+ = [Ar] 3d6 4s1);
// --config="[Ne] 3s2 3p5.5": an explicit, possibly fractional configuration ("2p3/1": LSDA alpha / beta split).  An invalid
// configuration exits with code 2 before anything runs.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <string>

#include "DFTAtom.h"

namespace {
struct Options {                         // Options.h:48-54 with the defaults of Options.cpp:6
    int Z = 36, MultigridLevels = 12;
    double MaxR = 10., deltaGrid = 0.001, alpha = 0.5;
    int method = 0;
};

bool load_ini(const char* path, Options& o)
{
    std::ifstream f(path);
    if (!f) return false;
    std::string line;
    while (std::getline(f, line)) {
        const size_t eq = line.find('=');
        if (line.empty() || line[0] == '[' || line[0] == ';' || line[0] == '#' || eq == std::string::npos) continue;
        std::string key = line.substr(0, eq), val = line.substr(eq + 1);
        while (!key.empty() && (key.back() == ' ' || key.back() == '\t')) key.pop_back();
        if (!key.empty() && key[0] == '/') key.erase(0, 1);
        if (key == "Z") o.Z = std::atoi(val.c_str());
        else if (key == "MultigridLevels") o.MultigridLevels = std::atoi(val.c_str());
        else if (key == "MaxR") o.MaxR = std::atof(val.c_str());
        else if (key == "deltaGrid") o.deltaGrid = std::atof(val.c_str());
        else if (key == "alpha") o.alpha = std::atof(val.c_str());
        else if (key == "Method") o.method = std::atoi(val.c_str());
    }
    return true;
}

const char* validate(const Options& o, bool uniform)
{
    // the options dialog's ranges (OptionsFrame.cpp:46-50,152-171); method 2 / 3 (uniform grid) is this front end's extension
    if (o.Z < 1 || o.Z > 118) return "Z must be between 1 and 118";
    if (o.MultigridLevels < 10 || o.MultigridLevels > 20) return "Please enter between 10 and 20 levels";
    if (!(o.MaxR >= 1 && o.MaxR <= 90)) return "MaxR must be between 1 and 90";
    if (!uniform && !(o.deltaGrid > 0 && o.deltaGrid <= 1)) return "deltaGrid must be in (0, 1]";
    if (!(o.alpha >= 0 && o.alpha <= 1)) return "alpha must be in [0, 1]";
    if (o.method < 0 || o.method > 1) return "method must be 0 (LDA), 1 (LSDA), 2 (uniform LDA) or 3 (uniform LSDA)";
    return nullptr;
}
}  // namespace

int main(int argc, char** argv)
{
    Options o;
    bool uniform = false, have = false, bad = false;
    int pos = 0;
    for (int i = 1; i < argc; ++i) {
        const std::string a = argv[i];
        if (a == "chained") DFT::DFTAtom::levelsMode = DFTA_LEVELS_CHAINED;
        else if (a == "--uniform") uniform = true;
        else if (a == "--ini" && i + 1 < argc) {
            if (!load_ini(argv[++i], o)) { std::cerr << "cannot read " << argv[i] << std::endl; return 2; }
            have = true;
        } else if (a == "--json") {
            DFT::DFTAtom::jsonOut = &std::cerr;
        } else if (a.rfind("--json=", 0) == 0) {
            static std::ofstream jf;
            jf.open(a.substr(7));
            if (!jf) { std::cerr << "cannot write " << a.substr(7) << std::endl; return 2; }
            DFT::DFTAtom::jsonOut = &jf;
        } else if (a == "--orbital-table") {
            DFT::DFTAtom::orbitalTable = true;
        } else if (a == "--slater-table") {
            DFT::DFTAtom::slaterTable = true;
        } else if (a == "--exchange-table") {
            DFT::DFTAtom::exchangeTable = true;
        } else if (a == "--form-factor-table") {
            DFT::DFTAtom::formFactorTable = true;
        } else if (a.rfind("--form-factor-table=", 0) == 0) {
            double smax = 0;
            int ns = 0;
            char tail = 0;
            if (std::sscanf(a.c_str() + 20, "%lf:%d%c", &smax, &ns, &tail) != 2 || !(smax >= 0 && smax <= 1e6) || ns < 1 || ns > 100000) {
                std::cerr << "bad form-factor table " << a.substr(20) << " (smax:ns, smax in 1/Angstrom, ns points)" << std::endl;
                return 2;
            }
            DFT::DFTAtom::formFactorTable = true;
            DFT::DFTAtom::formFactorSmax = smax;
            DFT::DFTAtom::formFactorPoints = ns;
        } else if (a == "--phase-shift-table") {
            DFT::DFTAtom::phaseShiftTable = true;
        } else if (a == "--photo-table") {
            DFT::DFTAtom::photoTable = true;
        } else if (a == "--pseudo-table") {
            DFT::DFTAtom::pseudoTable = true;
        } else if (a.rfind("--pseudo-table=", 0) == 0) {
            double f = 0;
            char tail = 0;
            if (std::sscanf(a.c_str() + 15, "%lf%c", &f, &tail) != 1 || !(f > 0 && f <= 100)) {
                std::cerr << "bad pseudo table " << a.substr(15) << " (factor: r_c over the radius of the orbital's largest |u|)" << std::endl;
                return 2;
            }
            DFT::DFTAtom::pseudoTable = true;
            DFT::DFTAtom::pseudoFactor = f;
        } else if (a == "--kb-table") {
            DFT::DFTAtom::kbTable = true;
        } else if (a.rfind("--kb-table=", 0) == 0) {
            double elo = 0, ehi = 0;
            int ne = 0;
            char tail = 0;
            if (std::sscanf(a.c_str() + 11, "%lf:%lf:%d%c", &elo, &ehi, &ne, &tail) != 3 || !(elo < ehi && elo >= -1e4 && ehi <= 1e4) || ne < 2 || ne > 100000) {
                std::cerr << "bad KB table " << a.substr(11) << " (elo:ehi:ne, energies in Ha, ne >= 2 of them)" << std::endl;
                return 2;
            }
            DFT::DFTAtom::kbTable = true;
            DFT::DFTAtom::kbElo = elo;
            DFT::DFTAtom::kbEhi = ehi;
            DFT::DFTAtom::kbPoints = ne;
        } else if (a.rfind("--phase-shift-table=", 0) == 0 || a.rfind("--photo-table=", 0) == 0) {
            const bool photo = a.rfind("--photo-table=", 0) == 0;
            const std::string v = a.substr(a.find('=') + 1);
            double emax = 0;
            int ne = 0;
            char tail = 0;
            if (std::sscanf(v.c_str(), "%lf:%d%c", &emax, &ne, &tail) != 2 || !(emax > 0 && emax <= 1e4) || ne < 1 || ne > 100000) {
                std::cerr << "bad continuum table " << v << " (emax:ne, emax in Ha, ne energies)" << std::endl;
                return 2;
            }
            (photo ? DFT::DFTAtom::photoTable : DFT::DFTAtom::phaseShiftTable) = true;
            (photo ? DFT::DFTAtom::photoEmax : DFT::DFTAtom::phaseShiftEmax) = emax;
            (photo ? DFT::DFTAtom::photoPoints : DFT::DFTAtom::phaseShiftPoints) = ne;
        } else if (a == "--sweeps=tolerance" || a == "--sweeps=exact") {
            DFT::DFTAtom::sweepMode = a == "--sweeps=tolerance" ? DFTA_SWEEPS_TOLERANCE : DFTA_SWEEPS_EXACT;
        } else if (a == "--poisson=tolerance" || a == "--poisson=adaptive" || a == "--poisson=exact") {
            DFT::DFTAtom::poissonMode = a == "--poisson=tolerance" ? DFTA_POISSON_TOLERANCE : (a == "--poisson=adaptive" ? DFTA_POISSON_ADAPTIVE : DFTA_POISSON_EXACT);
        } else if (a == "--mixing=linear" || a == "--mixing=anderson") {
            DFT::DFTAtom::mixing = a == "--mixing=anderson" ? DFTA_MIX_ANDERSON : DFTA_MIX_LINEAR;
        } else if (a == "--sic-table") {
            DFT::DFTAtom::sicTable = true;
        } else if (a == "--exchange=kli" || a == "--exchange=functional") {
            DFT::DFTAtom::exchange = a == "--exchange=kli" ? DFTA_EXCHANGE_KLI : DFTA_EXCHANGE_FUNCTIONAL;
        } else if (a == "--exchange=sic") {
            DFT::DFTAtom::exchange = DFTA_EXCHANGE_SIC_KLI;
        } else if (a.rfind("--exchange=", 0) == 0) {
            std::cerr << "unknown exchange " << a.substr(11) << std::endl;
            bad = true;
        } else if (a.rfind("--mixing=", 0) == 0) {
            std::cerr << "unknown mixing " << a.substr(9) << std::endl;
            bad = true;
        } else if (a.rfind("--xc=", 0) == 0) {
            const std::string n = a.substr(5);
            const char* names[] = {"vwn", "chachiyo", "chachiyo-improved", "pw92", "pbe"};      // DFTA_XC_VWN .. DFTA_XC_PBE
            int f = -1;
            for (int k = 0; k < 5; ++k) if (n == names[k]) f = k;
            if (f < 0) { std::cerr << "unknown functional " << n << std::endl; bad = true; }
            else DFT::DFTAtom::functional = f;
        } else if (a.rfind("--charge=", 0) == 0) {
            char* end = nullptr;
            const long q = std::strtol(a.c_str() + 9, &end, 10);
            if (end == a.c_str() + 9 || *end) { std::cerr << "bad charge " << a.substr(9) << std::endl; return 2; }
            DFT::DFTAtom::charge = static_cast<int>(q);
        } else if (a.rfind("--config=", 0) == 0) {
            DFT::DFTAtom::config = a.substr(9);
            if (DFT::DFTAtom::config.empty()) { std::cerr << "empty --config" << std::endl; return 2; }
        } else if (a.rfind("--integrator=", 0) == 0) {
            const std::string n = a.substr(13);
            const char* names[] = {"trapezoid", "simpson13", "simpson38", "boole", "romberg"};
            int r = -1;
            for (int k = 0; k < 5; ++k) if (n == names[k]) r = k;
            if (r < 0) { std::cerr << "unknown integrator " << n << std::endl; return 2; }
            DFT::DFTAtom::integrator = r;
        } else {
            switch (pos++) {
            case 0: o.Z = std::atoi(argv[i]); break;
            case 1: o.MultigridLevels = std::atoi(argv[i]); break;
            case 2: o.alpha = std::atof(argv[i]); break;
            case 3: o.MaxR = std::atof(argv[i]); break;
            case 4: o.deltaGrid = std::atof(argv[i]); break;
            case 5: o.method = std::atoi(argv[i]); have = true; break;
            default: break;
            }
        }
    }
    if (!have || bad) {
        std::cerr << "usage: " << argv[0] << " Z MultigridLevels alpha MaxR deltaGrid method(0 LDA, 1 LSDA, 2 uniform LDA, 3 uniform LSDA) [chained] [--integrator=NAME] [--xc=NAME]\n"
                  << "           [--charge=q | --config=\"[Ne] 3s2 3p5.5\"]\n"
                  << "       " << argv[0] << " --ini DFTAtom.ini [--uniform] [chained] [--integrator=NAME] [--xc=NAME] [--charge=q | --config=TEXT]\n"
                  << "       --xc=vwn (default) | chachiyo | chachiyo-improved | pw92 | pbe\n"
                  << "       --mixing=linear (default) | anderson: Anderson density mixing, fewer SCF steps\n"
                  << "       --exchange=functional (default) | kli: self-consistent exchange-only KLI (no correlation; --xc=vwn, --mixing=linear)\n"
                  << "                  | sic: VWN plus the Perdew-Zunger self-interaction correction through KLI (--xc=vwn, --mixing=linear)\n"
                  << "       --sic-table: with --exchange=sic, after Finished!, per shell its eigenvalue, EH, EXC, <v_SIC> and the KLI constant, then E_SIC\n"
                  << "       --orbital-table: after Finished!, one line per level with <r>, <r^2>, T and r_peak of its orbital\n"
                  << "       --slater-table: after Finished!, the Slater integrals F^k, G^k of the levels, then E_H and the exact-exchange energy\n"
                  << "       --exchange-table: after Finished!, per shell its eigenvalue, the orbital averages of the Fock, Slater and KLI exchange potentials and the KLI constant, then E_x and r vKLI at the density's outermost node\n"
                  << "       --form-factor-table[=smax:ns]: after Finished!, the X-ray form factor f(q) at ns values of s = sin(theta)/lambda in 0 .. smax 1/Angstrom (default 2:41)\n"
                  << "       --phase-shift-table[=emax:ne]: after Finished!, the scattering phase shifts delta_l(E), l = 0 .. 4, at ne energies in (0, emax] Ha (default 2:8), with u'/u and the node count\n"
                  << "       --pseudo-table[=factor]: after Finished!, the Troullier-Martins pseudopotentials of the default valence levels (LDA / GGA), r_c at factor x the radius of the orbital's largest |u| (default 1.5): r_c, coefficients, E_KB, eigenvalue and norm checks\n"
                  << "       --kb-table[=elo:ehi:ne]: after Finished!, the Kleinman-Bylander form of those pseudopotentials: E_KB, the bound states of H_KB, the two ghost verdicts, and u'/u at r_c in the all-electron potential, in V_ps and in H_KB at ne energies in elo .. ehi Ha (default -2:1:7)\n"
                  << "       --photo-table[=emax:ne]: after Finished!, the photoionization cross section of every subshell at ne photoelectron energies in (0, emax] Ha (default 4:8)\n"
                  << "       --charge=q: the cation (q > 0); --config: an electron configuration, fractional occupations allowed\n";
        return 2;
    }
    if (o.method == 2 || o.method == 3) { uniform = true; o.method -= 2; }
    if (const char* msg = validate(o, uniform)) { std::cerr << "error: " << msg << std::endl; return 2; }
    if (DFT::DFTAtom::charge != 0 && !DFT::DFTAtom::config.empty()) { std::cerr << "error: give --charge or --config, not both" << std::endl; return 2; }
    if (const char* msg = DFT::DFTAtom::CheckConfiguration(o.Z, o.method != 0)) { std::cerr << "error: electron configuration: " << msg << std::endl; return 2; }
    try {
        if (uniform) {
            if (o.method) DFT::DFTAtom::CalculateUniformLSDA(o.Z, o.MultigridLevels, o.alpha, o.MaxR);
            else          DFT::DFTAtom::CalculateUniformLDA(o.Z, o.MultigridLevels, o.alpha, o.MaxR);
        } else {
            if (o.method) DFT::DFTAtom::CalculateNonUniformLSDA(o.Z, o.MultigridLevels, o.alpha, o.MaxR, o.deltaGrid);
            else          DFT::DFTAtom::CalculateNonUniformLDA(o.Z, o.MultigridLevels, o.alpha, o.MaxR, o.deltaGrid);
        }
    } catch (const std::exception& e) {
        std::cerr << "error: " << e.what() << std::endl;
        return 1;
    }
    std::cout << std::endl;
    return 0;
}
