// scf_state.h -- the state of an SCF batch (dfta_scf): made and stepped by scf.hip, read by the accessors of scf_api.cpp.
#pragma once
#include <vector>

#include "internal.h"
#include "kli_stage.h"
#include "levels.h"

struct AtomState {          // per atom, device
    int Z;                  // nuclear charge: potential, energies, bracket bottoms, R[0] of the record
    double nE;              // electrons: the flat start density and the multigrid's outer boundary (== Z for a neutral atom)
    double nAlphaE, nBetaE; // electrons per spin (LSDA), DFTAtom.cpp:611-638
    int job_off, job_end;   // jobs of this atom in the level solver (alpha levels first, then beta)
    int lastTimeConverged;
    int finished;
    int steps;
    double Eold;
    dfta_energies e;
};

constexpr int kLiveClasses = 6;
constexpr int kLiveClassAtoms[kLiveClasses] = {7, 15, 16, 32, 64, 128};     // (7 / 15: the resident multigrid's two configurations)

struct dfta_scf {
    dfta_ctx* ctx = nullptr;
    const dfta_grid* g = nullptr;
    int lsda = 0, natoms = 0, nspin = 1, nV = 0;
    double alpha = 0.5;
    dfta::LevelSolver solver;             // holds the run's levels mode (mode) and quadrature (integ_rule: dfta_scf_set_integrator)
    dfta_poisson* poisson = nullptr;
    // Finished atoms are frozen, and the multigrid's workgroups per atom are a function of the batch size (1 for > 128 atoms ... 16 for
    // <= 16, the resident groups' 33 for <= 7): once the LIVE atoms of a batch fit a smaller size class, their solve goes to a second
    // solver made for that class, on gathered copies of their densities (results scattered back; the same bits -- every grouping of
    // the multigrid is bit-identical to one workgroup per atom).
    struct LiveSolver { dfta_poisson* p = nullptr; int G = 0; bool tried = false; };
    LiveSolver live_solver[kLiveClasses];
    int live_cap = 0;                     // atoms the gather buffers hold
    DevBuf<int> d_liveIdx;                // live_cap skip flags, then live_cap atom indices
    DevBuf<double> d_liveNe, d_liveRho, d_liveU;   // d_liveNe: the live atoms' electron counts
    void free_live() { d_liveIdx.reset(); d_liveNe.reset(); d_liveRho.reset(); d_liveU.reset(); live_cap = 0; }
    dfta::ScfConfig cfg;                  // as planned at creation: levels per spin, job list, per job the bracket start of every level solve
    std::vector<AtomState> h_atoms;
    std::vector<int> h_liveIdx;           // host staging of d_liveIdx and d_liveNe (the copies are asynchronous: they live to the step's last
    std::vector<double> h_liveNe;         // synchronisation at least)
    std::vector<dfta::Job> h_jobs;        // job results of the last step
    std::vector<unsigned char> h_frozen;  // per job: its atom has finished
    DevBuf<int> d_fin;                    // per atom: finished (device copy for the kernels that skip frozen atoms)
    bool debug_levels = false;            // $DFTA_DEBUG_LEVELS
    int functional = DFTA_XC_VWN;         // dfta_scf_options::functional
    int fallbacks_seen = 0;               // level-search fallbacks already reported in a step's statistics
    int steps_done = 0;
    int mixing = DFTA_MIX_LINEAR;         // dfta_scf_options::mixing
    dfta_anderson anderson;               // DFTA_MIX_ANDERSON: the atoms' history and the solve's scratch (mixing.hip); empty otherwise
    DevBuf<AtomState> d_atoms;
    DevBuf<double> d_Ne;                  // per atom: electrons, the multigrid's outer boundary U(Rmax)
    DevBuf<double> d_density, d_dA, d_dB, d_V, d_U, d_Vexc, d_va, d_vb, d_eexc, d_newDensity, d_integrands, d_integrals, d_records;
    DevEvent ev[5];
    // orbital expectation values and matrix elements (orbitals.hip): nothing is allocated before the first such call
    DevBuf<int> d_orb_l;                  // per job: l
    DevBuf<double> d_orb_props;           // njobs x DFTA_ORB_PROPS
    dfta_orbital_scratch orb_scratch;     // of dfta_scf_orbital_matrix, sized for the longest channel of the batch
    dfta_slater_scratch slater;           // of the Slater-integral calls (slater.hip): job table and results, made by the first such call
    dfta_exchange_scratch exchange;       // of the screening-function and exchange-potential calls (exchange.hip), made by the first such call
    dfta_bessel_scratch bessel;          // of the form-factor and momentum-orbital calls (bessel.hip), made by the first such call
    // dfta_scf_set_exchange: DFTA_EXCHANGE_KLI replaces the functional's launch of a step by the batched exchange stage (kli_stage.hip);
    // nothing of it is allocated otherwise
    int exchange_mode = DFTA_EXCHANGE_FUNCTIONAL;
    // (DFTA_EXCHANGE_SIC_KLI: the functional's launch stays and the stage, built with its SIC tables, adds its potential after it)
    double kli_y_mb = kKliDefaultYMB;     // DFTA_DEBUG KLI_Y_MB, read at creation
    dfta_kli_stage kli;
    std::vector<unsigned char> h_live_ch; // per channel (atom x nspin): its atom is live in this step

    // first job and number of levels of (atom, spin), and of the atom (alpha levels, then beta levels)
    struct Jobs { int k0, cnt; };
    Jobs channel(int atom, int spin) const { return {h_atoms[atom].job_off + (spin ? cfg.nlev[0][atom] : 0), cfg.nlev[spin][atom]}; }
    Jobs atom_jobs(int atom) const { return {h_atoms[atom].job_off, h_atoms[atom].job_end - h_atoms[atom].job_off}; }
};
