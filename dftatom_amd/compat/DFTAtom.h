// DFTAtom.h -- DFT::DFTAtom as the reference declares it (reference DFTAtom.h:9-35): the four static entry points and the
// private helpers of its orchestration, so that EITHER implementation of the class links against this directory's
// L2 classes (Numerov, PoissonSolver, VWNExchCor, Integral, AufbauPrinciple):
//   * dftatom_amd/compat/DFTAtom.cpp -- the device-resident SCF (dfta_scf_*): one launch sequence per step, state in HBM;
//     it defines the four entry points (and Run / levelsMode / integrator below) and never needs the private helpers;
//   * the reference's own DFTAtom.cpp, compiled unmodified against these headers (tests/test_ref_l3.py,
//     INTEGRATION.md): its LoopOverLevels / LocateInterval / Normalize* then drive the HIP kernels call by call.
// Both write the reference's console text to std::cout, so the wxWidgets front end (DFTAtomFrame.cpp:185-198) links
// against either unchanged.
#pragma once

#include <iosfwd>
#include <string>
#include <vector>

#include "AufbauPrinciple.h"
#include "Numerov.h"

namespace DFT {

class DFTAtom {
public:
    static const char orb[];

    static void CalculateNonUniformLDA(int Z, int MultigridLevels, double alpha, double MaxR, double deltaGrid);
    static void CalculateUniformLDA(int Z, int MultigridLevels, double alpha, double MaxR);
    static void CalculateNonUniformLSDA(int Z, int MultigridLevels, double alpha, double MaxR, double deltaGrid);
    static void CalculateUniformLSDA(int Z, int MultigridLevels, double alpha, double MaxR);

    // knobs of the device path (not in the reference)
    static int levelsMode;      // DFTA_LEVELS_BATCHED (default) or DFTA_LEVELS_CHAINED (the reference's exact bisection path)
    static int integrator;      // DFTA_INT_SIMPSON38 (default: what the reference calls) ... DFTA_INT_ROMBERG (what its README names)
    static int sweepMode;       // DFTA_SWEEPS_EXACT (default) / DFTA_SWEEPS_TOLERANCE (transfer-matrix scans; logarithmic grids of 12 .. 20 levels)
    static int poissonMode;     // -1 (default): as dfta_poisson_create, i.e. exact unless $DFTA_DEBUG POISSON_MODE says otherwise; DFTA_POISSON_EXACT / _TOLERANCE / _ADAPTIVE
    static int mixing;          // DFTA_MIX_LINEAR (default: the reference's mixing, DFTAtom.cpp:332-342) / DFTA_MIX_ANDERSON (about half the SCF steps)
    static int exchange;        // DFTA_EXCHANGE_FUNCTIONAL (default) / DFTA_EXCHANGE_KLI: self-consistent exchange-only KLI (functional VWN, linear mixing)
                                // / DFTA_EXCHANGE_SIC_KLI: VWN plus the Perdew-Zunger self-interaction correction through KLI (the same two)
    static int functional;      // DFTA_XC_VWN (default: what the reference runs), _CHACHIYO, _CHACHIYO_IMPROVED (LDA only), _PW92, _PBE (logarithmic grid)
    // electron configuration (not in the reference, which runs the neutral Aufbau atom): charge q > 0 runs the cation of dfta_ion_config,
    // a non-empty config the text of dfta_config_parse ("[Ne] 3s2 3p5.5", "2p3/1" LSDA splits); both unset (default): the Aufbau atom
    static int charge;
    static std::string config;
    // nullptr if charge / config describe a valid configuration of Z (LDA or LSDA), else the reason (dfta_config_last_error)
    static const char* CheckConfiguration(int Z, bool lsda);
    // per-step machine-readable output (metrics): when set, every SCF step appends ONE JSON line with 17-digit
    // energies and eigenvalues, per-level status bits (DFTA_LEVEL_*) and sweep counts, rounds, V-cycles and the phases' HIP-event times
    static std::ostream* jsonOut;
    // after "Finished!", one line per level: n, l, occupation, E and <r>, <r^2>, T, r_peak of its orbital (dfta_scf_orbital_properties)
    static bool orbitalTable;
    // after "Finished!" (and the orbital table), one line per F^k / G^k of the levels' Slater integrals, then E_H and the exact-exchange
    // energy of the orbitals (dfta_scf_slater_fg, dfta_scf_coulomb_exchange)
    static bool slaterTable;
    // after "Finished!" (and the Slater table), one line per shell and channel with its eigenvalue and the orbital averages of the Fock,
    // Slater and KLI exchange potentials, then E_x and r vKLI at the outermost node of the density (dfta_scf_exchange_potentials)
    static bool exchangeTable;
    // under DFTA_EXCHANGE_SIC_KLI, after "Finished!": one line per shell with its eigenvalue, EH_a, EXC_a, <a|v_a^SIC|a> and c_a, then E_SIC
    // (dfta_scf_sic_table)
    static bool sicTable;
    // after "Finished!" (and the other tables), the X-ray form factor of the converged density on formFactorPoints values of
    // s = sin(theta) / lambda from 0 to formFactorSmax (1 / Angstrom), one line each; LSDA adds f_a - f_b (dfta_scf_form_factors)
    static bool formFactorTable;
    static double formFactorSmax;
    static int formFactorPoints;
    // after "Finished!" (and the other tables): the phase-shift table -- for every spin channel, l = 0 .. 4 and E_k = Emax (k + 1) / ne the
    // scattering phase shift, u'/u at the last node but one and the node count of the outward solution (dfta_scf_continuum, one launch) --
    // and the photoionization table: omega and sigma_nl of every subshell at the photoelectron energies eps_k = Emax (k + 1) / ne
    // (dfta_scf_photoionization).  A charged atom or a KLI / SIC-KLI run is normalised by DFTA_CONT_WKB: the column then holds the WKB phase
    static bool phaseShiftTable, photoTable;
    // --pseudo-table[=factor]: after Finished!, the Troullier-Martins pseudopotentials of the default valence levels, core radii at
    // factor x the radius of the orbital's largest |u| (dfta_scf_pseudopotentials): r_c, the coefficients, E_KB and two checks
    static bool pseudoTable;
    static double pseudoFactor;
    static bool kbTable;
    static double kbElo, kbEhi;
    static int kbPoints;
    static double phaseShiftEmax, photoEmax;
    static int phaseShiftPoints, photoPoints;

private:
    static constexpr double fourM_PI = 4. * M_PI;

    // the reference's orchestration helpers (reference DFTAtom.h:20-33); defined by the reference's DFTAtom.cpp only
    static void LoopOverLevels(Numerov<NumerovFunctionRegularGrid>& numerov, std::vector<Subshell>& levels, std::vector<double>& newDensity, double& Eelectronic, double& BottomEnergy, int NumSteps, double MaxR, double h, bool& reallyConverged, double energyErr, bool lda = true, bool isAlpha = true);
    static void LocateInterval(Numerov<NumerovFunctionRegularGrid>& numerov, double& TopEnergy, double& BottomEnergy, double MaxR, int L, int NumSteps, int NumNodes, double energyErr);
    static void CalculateNonUniformDensity(std::vector<double>& density, double alpha, double oneMinusAlpha, double deltaGrid, double Rp, int NumGridNodes, Numerov<NumerovFunctionNonUniformGrid>& numerov, std::vector<Subshell>& levels, std::vector<double>& newDensity, double& Eelectronic, double& BottomEnergy, int NumSteps, double MaxR, double h, bool& reallyConverged, double energyErr, bool lda = true, bool isAlpha = true);
    static void LoopOverLevels(Numerov<NumerovFunctionNonUniformGrid>& numerov, std::vector<Subshell>& levels, std::vector<double>& newDensity, double& Eelectronic, double& BottomEnergy, int NumSteps, double Rp, double deltaGrid, bool& reallyConverged, double energyErr, bool lda = true, bool isAlpha = true);
    static void LocateInterval(Numerov<NumerovFunctionNonUniformGrid>& numerov, double& TopEnergy, double& BottomEnergy, int L, int NumSteps, int NumNodes, double energyErr);
    static void NormalizeNonUniform(std::vector<double>& Psi, double Rp, double deltaGrid);
    static void NormalizeUniform(std::vector<double>& Psi, double h);
    static void InitializeLevels(int Z, int& numAlphaElectrons, int& numBetaElectrons, std::vector<Subshell>& levelsAlpha, std::vector<Subshell>& levelsBeta);

    // the device-resident orchestration (compat/DFTAtom.cpp)
    static void Run(bool lsda, bool uniform, int Z, int MultigridLevels, double alpha, double MaxR, double deltaGrid);
};

}  // namespace DFT
