// kli_stage.h -- the batched exchange stage (kli_stage.hip): y rows, exchange operator, quadratures, the KLI solve on the device and the
// update of v_x for every live spin channel of a batch in one sequence of launches per chunk, with no host synchronisation in between.
// Owned by a dfta_scf whose exchange switch is DFTA_EXCHANGE_KLI or DFTA_EXCHANGE_SIC_KLI, or by one call of dfta_kli_channels /
// dfta_sic_channels.  Under `sic` the orbital-specific potentials are those of the Perdew-Zunger self-interaction correction: the y rows
// are the diagonals y^0_aa alone, X_a = (y^0_aa + v_a) u_a with v_a the fully polarised VWN potential of the orbital density, and two
// more quadratures per shell give E_SIC; the reduction to one local potential (solve, tail, mix) is the same kernels.
#pragma once
#include <vector>

#include "common.h"
#include "kli_plan.h"

constexpr double kKliDefaultYMB = 1024.;     // budget of the y rows of a chunk (DFTA_DEBUG KLI_Y_MB), MiB

struct dfta_kli_stage {
    dfta_kli::Plan plan;
    long max_rows = 0;                       // y rows of a chunk under the budget
    dfta_kli::Caps caps = {0, 0, 0};
    int N = 0, natoms = 0;
    bool sic = false;                        // the SIC-KLI builder of X_a instead of the exchange operator
    // tables of the batch
    DevBuf<dfta_kli::Channel> d_ch;
    DevBuf<int> d_jobs, d_first, d_tab, d_red;
    DevBuf<double> d_coef, d_occ;            // d_occ: the channel occupation n_a of every orbital row
    // a chunk's rows
    DevBuf<double> d_y, d_X, d_DvS;          // caps.yrows x N; caps.xrows x N; D (caps.chans x N), then vS
    DevBuf<double> d_vorb, d_eps;            // sic: v_a and eps_a of a chunk's shells, caps.xrows x N each
    DevBuf<double> d_redout;                 // every reduction of the batch
    // results, kept from step to step: per channel vx, v_raw (nch x N), per orbital row vbarHF and c, per channel the HOMO, the last
    // node with D > 0, v_raw r there, E_x of the channel and the solve's status (1: a pivot that is zero or not finite); per atom E_x
    DevBuf<double> d_vx, d_vraw, d_vbarHF, d_c, d_tail, d_ExCh, d_ExAtom;
    DevBuf<double> d_EH, d_EXC;              // sic: per orbital row EH_a and EXC_a; d_ExCh / d_ExAtom then hold E_SIC
    DevBuf<int> d_homo, d_ilast, d_status;
    std::vector<int> h_status, bounds;
    DevEvent ev[2];
    bool timed = false;

    bool active() const { return N > 0; }
    // atom: per channel, or null; natoms: rows of d_ExAtom (0: none).  Allocates everything; vx, v_raw, E_x start as zeros, the HOMOs as -1
    int create(dfta_ctx* ctx, const dfta_grid* g, int nch, const int* norb, const int* l, const double* occ, const int* atom, int natoms,
               double y_mb, bool sic = false);
    // One stage: for every chunk of live channels the y launch, the pointwise pass, the quadratures, the solve and the update of vx / v_raw.
    // dU: the orbital rows of the batch; the eigenvalue of row k is the double at Ebase + k * Estride (device).  live: per channel, null:
    // all.  Asynchronous on the context's stream; the events bracket it.
    // dump: null, or whole-batch device arrays (any of them null) that receive every chunk's rows: y and X / vorb / eps by y job and by
    // orbital row, D and vS by channel.
    struct Dump { double *y, *vorb, *eps, *X, *D, *vS; };
    int run(dfta_ctx* ctx, const dfta_grid* g, const double* dU, const void* Ebase, size_t Estride, const unsigned char* live, bool first,
            double alpha, double oneMinusAlpha, const Dump* dump = nullptr);
    // in place of the functional's launch: Vexc / va / vb / eexc of every atom that has not finished from vx and the mixed densities, E_x
    // per atom.  Channels atom-major, nspin per atom.  Under `sic`, AFTER the functional's launch on the mixed densities: adds the SIC
    // potential to Vexc / va / vb and takes it from eexc; E_SIC per atom
    int assemble(dfta_ctx* ctx, const dfta_grid* g, int lsda, const double* density, const double* dA, const double* dB, const int* fin,
                 double* Vexc, double* va, double* vb, double* eexc);
    void reset();
};
