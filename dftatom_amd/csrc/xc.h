// xc.h -- device-pointer launchers of the exchange-correlation kernels (xc.hip, gga.hip) and of the Poisson solve (poisson.hip)
#pragma once
#include "common.h"

int dfta_launch_vwn_lda(dfta_ctx* ctx, const double* dN, size_t sz, double* dVexc, double* dEexc);
int dfta_launch_vwn_lsda(dfta_ctx* ctx, const double* dNa, const double* dNb, size_t sz, double* dRes, double* dVa, double* dVb,
                         double* dEexc);
// the two irrational constants of the VWN kernels as their launchers pass them: (3 / (2 pi))^(2/3) and 2^(1/3), from the host's libm
double dfta_vwn_cx();
double dfta_vwn_cbrt2();
int dfta_launch_chachiyo_lda(dfta_ctx* ctx, int improved, const double* dN, size_t sz, double* dVexc, double* dEexc);
// Slater exchange + PW92 correlation (xc.hip), same outputs as the VWN launchers
int dfta_launch_pw92_lda(dfta_ctx* ctx, const double* dN, size_t sz, double* dVexc, double* dEexc);
int dfta_launch_pw92_lsda(dfta_ctx* ctx, const double* dNa, const double* dNb, size_t sz, double* dRes, double* dVa, double* dVb,
                          double* dEexc);
// gga.hip: PBE on the logarithmic grid for natoms x N densities in one fused launch; dNb == nullptr: LDA (dRes = Vexc, dVa / dVb unused);
// dFin: per atom, non-zero = frozen, leave its outputs alone (may be null)
int dfta_launch_pbe_radial(dfta_ctx* ctx, const dfta_grid* g, int natoms, const double* dNa, const double* dNb, double* dRes,
                           double* dVa, double* dVb, double* dEexc, const int* dFin);
// poisson.hip: launch (asynchronous) / finish (synchronises, inspects the group barriers' abort flag and repeats the solve with
// one workgroup per atom if it was raised).  dSkip: per atom, non-zero = leave this atom alone (may be null).  dNe: per atom, the
// electron count, the outer boundary value U(Rmax) (the reference's Z: (double)Z for a neutral atom).
int dfta_poisson_solve_launch(dfta_poisson* p, const double* dNe, const double* dDensity, double* dU, int* dVcycles, double* dErr,
                              const int* dSkip);
int dfta_poisson_finish(dfta_poisson* p, const double* dNe, const double* dDensity, double* dU, int* dVcycles, double* dErr,
                        const int* dSkip);
int dfta_poisson_take_vcycles(dfta_poisson* p, unsigned long long* out);
int dfta_poisson_group_state(const dfta_poisson* p, int* G, int* degraded, int* aborts);
