// scf_config.h -- the pure host logic of the SCF layer: Aufbau and spin split, the configuration parser and the charge rule (the C ABI
// entries dfta_get_subshells* / dfta_split_spin* / dfta_config_parse / dfta_ion_config / dfta_config_last_error), the plan of a batch's
// configuration (atoms, levels per spin, job list, bracket bottoms), the SCF options and the struct_size protocol of the versioned
// structs.  Plain C++17: no HIP header, no HIP call, no environment -- scf.hip passes in numbers, tests/test_scf_config.py
// (oracle/scf_config_main.cpp) does the same without a GPU.
#pragma once

#include <cstddef>
#include <vector>

#include "../../include/dftatom_hip.h"

namespace dfta {

// occ: the level's integer occupation as the reference's records hold it (Job::occ, 0 for a fractional one); docc: the occupation the
// density and the electronic energy are summed with
struct JobSpec { int v, n, l, occ; double docc; };

struct AtomConfig {
    int Z;
    double nE, nAlphaE, nBetaE;   // electrons, and per spin (LDA: nAlphaE = nE; only the LSDA start density reads the two)
    int job_off, job_end;         // the atom's jobs (alpha levels first, then beta)
};
struct ScfConfig {
    std::vector<AtomConfig> atoms;
    std::vector<int> nlev[2];     // per atom: levels per spin
    std::vector<JobSpec> specs;   // v = atom (LDA) or 2 atom + spin; sorted by (n, l) inside a channel (DFTAtom.cpp:367)
    std::vector<double> bottom;   // per job: the bracket bottom -Z^2 - 1 (DFTAtom.cpp:407 / 919,929)
};
// nlev (2 per atom: alpha, beta) with n / l / occ as dfta_scf_create_config takes them, or nlev null: the Aufbau configuration, which is
// the charge-0 configuration of dfta_ion_config on the same path.  DFTA_ERR_INVALID: the reason, prefixed "atom <a>: ", is the text
// dfta_config_last_error() returns
int plan_scf_config(int natoms, const int* Z, const int* nlev, const int* n, const int* l, const double* occ, int lsda, int aufbau, ScfConfig* out);

// ---- versioned structs: int struct_size first, grown at the end between versions of the header ------------------------------------
constexpr size_t kOptionsMinSize = 2 * sizeof(int), kStatsMinSize = 4 * sizeof(int);     // the version-6 prefixes
bool versioned_size_ok(int user_size, size_t min_size);
// the bytes both the caller's struct (user_size of them) and the library's (lib_size) hold go from src to dst, whose struct_size stays
// or becomes dst_struct_size; false: user_size is no valid size (nothing is copied)
bool copy_versioned(void* dst, const void* src, int user_size, size_t min_size, size_t lib_size, int dst_struct_size);

// ---- dfta_scf_options ---------------------------------------------------------------------------------------------------------------
struct ScfFacts {                 // what the checks need from the device or from another file
    int lsda, uniform;
    int scan_ok;                  // dfta_scan_supported(grid)
    unsigned integrators_fit;     // bit r: dfta_integral_shape_ok(r, N)
    int mix_history_max;          // kAndersonMaxHistory
};
// defaults, the caller's members (user may be null), every range check; mix_history / mix_warmup 0 resolved to their defaults.
// Returns null, or why the options are refused
const char* resolve_scf_options(const dfta_scf_options* user, const ScfFacts& facts, dfta_scf_options* out);

}  // namespace dfta
