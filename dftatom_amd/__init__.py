"""dftatom_amd -- MI355X (gfx950) radial-DFT inner loop behind a C ABI.

This package is a thin ctypes binding over ``dftatom_amd/libdftatom_hip.so`` (built from
``dftatom_amd/csrc`` by ``__graft_entry__.build()`` / ``make -C dftatom_amd/csrc``).  There is no CPU
fallback: if the shared library is missing, or no HIP device is usable, every entry point raises.

When PyTorch is used in the same process (bench.py: device memory, streams, torch.distributed), import
torch BEFORE this module so that both share one HIP runtime (same libamdhip64 soname).
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("DFTA_LIB_PATH") or os.path.join(_HERE, "libdftatom_hip.so")      # DFTA_LIB_PATH: measurement builds

OK = 0
SWEEP_COUNT, SWEEP_ZERO = 0, 1
SWEEP_KERNEL_AUTO, SWEEP_KERNEL_FUSED, SWEEP_KERNEL_PIPELINED = 0, 1, 2
BOUNDARY_DEVICE, BOUNDARY_HOST = 0, 1
LEVELS_CHAINED, LEVELS_BATCHED = 0, 1
LEVELS_SCAN_SWEEPS = 0x10          # OR-ed into the mode of solve_levels: tolerance mode of the sweeps (transfer-matrix scan)
SWEEPS_EXACT, SWEEPS_TOLERANCE = 0, 1
ABI_VERSION = 7
LEVEL_CONVERGED, LEVEL_ITERATION_CAP, LEVEL_FIXED_POINT, LEVEL_U0_NONFINITE = 1, 2, 4, 8
POISSON_DEFAULT, POISSON_EXACT, POISSON_TOLERANCE, POISSON_ADAPTIVE = -1, 0, 1, 2    # dfta_poisson_create_ex / dfta_scf_options::poisson_mode
INT_TRAPEZOID, INT_SIMPSON13, INT_SIMPSON38, INT_BOOLE, INT_ROMBERG = range(5)
XC_VWN, XC_CHACHIYO, XC_CHACHIYO_IMPROVED, XC_PW92, XC_PBE = range(5)
AUFBAU_REFERENCE, AUFBAU_TRANSITION_METALS = range(2)
MIX_LINEAR, MIX_ANDERSON = range(2)    # dfta_scf_options::mixing
RECORD_DOUBLES = 64
# columns of an orbital-property row (DFTA_ORB_*): NORM, <1/r>, <r>, <r^2>, <r^4>, T, r at the largest |u|, <1/r^3> (l >= 1, else 0)
ORB_PROPS = 8
ORB_NORM, ORB_RM1, ORB_R1, ORB_R2, ORB_R4, ORB_T, ORB_RPEAK, ORB_RM3 = range(8)
SLATER_KMAX = 8                        # DFTA_SLATER_KMAX: largest k of a Slater integral R^k
SLATER_F, SLATER_G = 0, 1              # kinds of slater_fg_jobs
XP_COLS = 4                            # DFTA_XP_*: columns of a vbar row of exchange_potentials
XP_HF, XP_S, XP_C, XP_KLI = range(4)   # <a|v_x^HF,a|a>, <a|vS|a>, the KLI constant c_a, <a|vKLI|a>
EXCHANGE_FUNCTIONAL, EXCHANGE_KLI = 0, 1   # dfta_scf_set_exchange: v_xc of the functional / exchange-only KLI from the step's orbitals
EXCHANGE_SIC_KLI = 2                       # ... / VWN plus the Perdew-Zunger self-interaction correction as one KLI potential per channel
BT_DENSITY, BT_ORBITAL = 0, 1         # DFTA_BT_*: kinds of bessel_transform
BESSEL_LMAX = 4                        # DFTA_BESSEL_LMAX: largest order of sph_bessel / bessel_transform
CONT_FREE, CONT_WKB = 0, 1             # DFTA_CONT_*: normalisation of continuum(): Riccati matching (short range) / WKB amplitude (any tail)
CONT_MAX_PARTNERS = 16                 # DFTA_CONT_MAX_PARTNERS: partners of one list
CONT_NONFINITE, CONT_STEP, CONT_WKB_TAIL, CONT_NORM = 1, 2, 4, 8      # status bits of a continuum trial
PS_COEF, PS_MATCH = 7, 8               # DFTA_PS_*: a0, a2 .. a12 of a pseudized channel; P0 .. P4, I_AE, I_ps, g
PS_NOBRACKET, PS_CAP, PS_NODES, PS_NONFINITE, PS_NOTPOSITIVE = 1, 2, 4, 8, 16      # status bits of a pseudized channel
KB_MAX_STATES, KB_REPORT = 8, 10       # DFTA_KB_*: bound states of a channel; doubles of a channel's ghost report
KB_SEARCH_NONFINITE, KB_SEARCH_FULL, KB_SEARCH_CAP = 1, 2, 4      # status bits of kb_bound_states

c_dp = C.POINTER(C.c_double)
c_ip = C.POINTER(C.c_int)
c_lp = C.POINTER(C.c_long)
vp = C.c_void_p


class DftaError(RuntimeError):
    pass


class LevelResult(C.Structure):
    _fields_ = [("E", C.c_double), ("top", C.c_double), ("bottom", C.c_double), ("n_count", C.c_int),
                ("n_zero", C.c_int), ("converged", C.c_int), ("matchPoint", C.c_int), ("status", C.c_int)]


class Energies(C.Structure):
    _fields_ = [(k, C.c_double) for k in ("Etotal", "Ekinetic", "Ecoul", "Enuclear", "Exc",
                                          "Eelectronic", "Ehartree", "eExcDif", "Epotential")]

    def as_list(self):
        return [self.Etotal, self.Ekinetic, self.Ecoul, self.Enuclear, self.Exc]


class ScfOptions(C.Structure):
    _fields_ = [("struct_size", C.c_int), ("integrator", C.c_int), ("functional", C.c_int), ("aufbau", C.c_int), ("poisson_mode", C.c_int), ("sweep_mode", C.c_int),
                ("mixing", C.c_int), ("mix_history", C.c_int), ("mix_warmup", C.c_int)]


class StepStats(C.Structure):
    _fields_ = [("struct_size", C.c_int), ("levels_fallbacks", C.c_int), ("sweeps_issued", C.c_long), ("sweeps_reference", C.c_long), ("points_traversed", C.c_long),
                ("vcycles", C.c_long), ("rounds", C.c_int), ("ms_levels", C.c_float), ("ms_poisson", C.c_float),
                ("ms_tail", C.c_float), ("ms_sweep_kernels", C.c_float), ("ms_poisson_kernel", C.c_float),
                ("sweeps_reference_executed", C.c_long), ("points_reference", C.c_long),
                ("levels_layout", C.c_int), ("poisson_groups", C.c_int)]


# every symbol include/dftatom_hip.h declares: name -> (restype, argtypes)
SIGNATURES = {
    "dfta_ctx_create": (C.c_int, [C.c_int, vp, C.POINTER(vp)]),
    "dfta_ctx_destroy": (None, [vp]),
    "dfta_ctx_synchronize": (C.c_int, [vp]),
    "dfta_last_error": (C.c_char_p, [vp]),
    "dfta_version": (C.c_char_p, []),
    "dfta_abi_version": (C.c_int, []),
    "dfta_ctx_device_info": (C.c_int, [vp, c_ip, C.c_char_p, C.c_int]),
    "dfta_ctx_last_kernel_ms": (C.c_int, [vp, C.POINTER(C.c_float)]),
    "dfta_ctx_set_sweep_kernel": (C.c_int, [vp, C.c_int]),
    "dfta_grid_create": (C.c_int, [vp, C.c_int, C.c_double, C.c_double, C.POINTER(vp)]),
    "dfta_grid_create_uniform": (C.c_int, [vp, C.c_int, C.c_double, C.POINTER(vp)]),
    "dfta_grid_is_uniform": (C.c_int, [vp]),
    "dfta_grid_destroy": (None, [vp]),
    "dfta_grid_num_nodes": (C.c_int, [vp]),
    "dfta_grid_rp": (C.c_double, [vp]),
    "dfta_grid_get_r": (C.c_int, [vp, c_dp]),
    "dfta_num_nodes": (C.c_int, [C.c_int]),
    "dfta_numerov_sweeps": (C.c_int, [vp, vp, C.c_int, C.c_int, C.c_int, c_dp, C.c_int, c_ip, c_ip, c_dp, c_ip,
                                      c_ip, c_dp, c_ip, c_ip]),
    "dfta_numerov_sweeps_scan": (C.c_int, [vp, vp, C.c_int, C.c_int, c_dp, C.c_int, c_ip, c_ip, c_dp, c_ip, c_ip, c_dp, c_ip, c_ip, c_ip]),
    "dfta_numerov_sweeps_dev": (C.c_int, [vp, vp, C.c_int, C.c_int, vp, C.c_int, c_ip, c_ip, c_ip, vp, vp, vp, vp, vp,
                                          vp, vp, vp, vp]),
    "dfta_numerov_match": (C.c_int, [vp, vp, C.c_int, C.c_int, c_dp, C.c_int, c_ip, c_ip, c_dp, c_dp, c_lp]),
    "dfta_potential_create": (C.c_int, [vp, vp, c_dp, C.POINTER(vp)]),
    "dfta_potential_update": (C.c_int, [vp, c_dp]),
    "dfta_potential_destroy": (None, [vp]),
    "dfta_potential_sweeps": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, c_ip, c_dp, c_ip, c_ip, c_dp, c_ip, c_ip]),
    "dfta_potential_match": (C.c_int, [vp, C.c_int, c_ip, c_dp, c_dp, c_lp]),
    "dfta_solve_levels": (C.c_int, [vp, vp, C.c_int, C.c_int, C.c_int, c_dp, c_dp, c_dp, C.c_int, c_ip, c_ip, c_ip, c_ip,
                                    C.POINTER(LevelResult), c_dp, c_dp, c_dp, c_lp]),
    "dfta_poisson_create": (C.c_int, [vp, vp, C.c_int, C.POINTER(vp)]),
    "dfta_poisson_destroy": (None, [vp]),
    "dfta_poisson_solve": (C.c_int, [vp, c_ip, c_dp, c_dp, c_ip, c_dp]),
    "dfta_poisson_solve_dev": (C.c_int, [vp, vp, vp, vp]),
    "dfta_poisson_group_info": (C.c_int, [vp, c_ip, c_ip, c_ip]),
    "dfta_poisson_predict_counts": (C.c_int, [vp, C.POINTER(C.c_ulonglong), C.POINTER(C.c_ulonglong)]),
    "dfta_scf_poisson_info": (C.c_int, [vp, c_ip, c_ip, c_ip]),
    "dfta_poisson_level_size": (C.c_int, [vp, C.c_int]),
    "dfta_poisson_set_level": (C.c_int, [vp, C.c_int, c_dp, c_dp]),
    "dfta_poisson_get_level": (C.c_int, [vp, C.c_int, c_dp, c_dp]),
    "dfta_poisson_gauss_seidel": (C.c_int, [vp, C.c_int, C.c_int, c_dp]),
    "dfta_poisson_iterate_gs": (C.c_int, [vp, C.c_int, C.c_double, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_int)]),
    "dfta_poisson_restrict": (C.c_int, [vp, C.c_int]),
    "dfta_poisson_prolong": (C.c_int, [vp, C.c_int]),
    "dfta_poisson_vcycle": (C.c_int, [vp, c_dp]),
    "dfta_poisson_full_cycle": (C.c_int, [vp, C.c_double, C.c_double, C.c_double, C.c_double, c_dp, c_ip]),
    "dfta_scf_set_integrator": (C.c_int, [vp, C.c_int]),
    "dfta_vwn_lda": (C.c_int, [vp, c_dp, C.c_size_t, c_dp, c_dp]),
    "dfta_vwn_lsda": (C.c_int, [vp, c_dp, c_dp, C.c_size_t, c_dp, c_dp, c_dp, c_dp]),
    "dfta_integrate": (C.c_int, [vp, C.c_int, C.c_double, c_dp, C.c_int, C.POINTER(C.c_double)]),
    "dfta_scf_create": (C.c_int, [vp, vp, C.c_int, C.c_int, c_ip, C.c_double, C.c_int, C.c_int, C.POINTER(vp)]),
    "dfta_scf_create_ex": (C.c_int, [vp, vp, C.c_int, C.c_int, c_ip, C.c_double, C.c_int, C.c_int, vp, C.POINTER(vp)]),
    "dfta_scf_destroy": (None, [vp]),
    "dfta_scf_step": (C.c_int, [vp, C.POINTER(StepStats)]),
    "dfta_scf_get_energies": (C.c_int, [vp, C.POINTER(Energies), c_ip]),
    "dfta_scf_info": (C.c_int, [vp, c_ip, c_ip, c_lp]),
    "dfta_scf_num_levels": (C.c_int, [vp, C.c_int, C.c_int]),
    "dfta_scf_get_levels": (C.c_int, [vp, C.c_int, C.c_int, c_ip, c_ip, c_ip, c_dp, c_ip]),
    "dfta_scf_get_level_status": (C.c_int, [vp, C.c_int, C.c_int, c_ip, c_ip, c_ip]),
    "dfta_scf_get_array": (C.c_int, [vp, C.c_int, C.c_int, c_dp]),
    "dfta_scf_get_records_dev": (C.c_int, [vp, vp]),
    "dfta_get_subshells": (C.c_int, [C.c_int, c_ip, c_ip, c_ip, C.c_int]),
    "dfta_get_subshells_ex": (C.c_int, [C.c_int, C.c_int, c_ip, c_ip, c_ip, C.c_int]),
    "dfta_split_spin_ex": (C.c_int, [C.c_int, C.c_int, c_ip, c_ip, c_ip, c_ip, c_ip, c_ip, c_ip, c_ip, C.c_int]),
    "dfta_chachiyo_lda": (C.c_int, [vp, C.c_int, c_dp, C.c_size_t, c_dp, c_dp]),
    "dfta_xc_pointwise": (C.c_int, [vp, C.c_int, C.c_size_t, c_dp, c_dp, c_dp, c_dp, c_dp, c_dp, c_dp, c_dp, c_dp, c_dp, c_dp]),
    "dfta_xc_radial": (C.c_int, [vp, vp, C.c_int, C.c_int, c_dp, c_dp, c_dp, c_dp, c_dp, c_dp]),
    "dfta_split_spin": (C.c_int, [C.c_int, c_ip, c_ip, c_ip, c_ip, c_ip, c_ip, c_ip, c_ip, C.c_int]),
    "dfta_ctx_measure_hbm": (C.c_int, [vp, C.c_size_t, C.c_int, c_dp, c_dp]),
    "dfta_poisson_create_ex": (C.c_int, [vp, vp, C.c_int, C.c_int, C.POINTER(vp)]),
    "dfta_poisson_mode": (C.c_int, [vp]),
    "dfta_config_parse": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_char_p, C.c_int, c_ip, c_ip, c_ip, c_ip, c_dp, c_ip, c_ip, c_dp]),
    "dfta_ion_config": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, c_ip, c_ip, c_ip, c_ip, c_dp, c_ip, c_ip, c_dp]),
    "dfta_config_last_error": (C.c_char_p, []),
    "dfta_scf_create_config": (C.c_int, [vp, vp, C.c_int, C.c_int, c_ip, c_ip, c_ip, c_ip, c_dp, C.c_double, C.c_int, C.c_int, vp,
                                         C.POINTER(vp)]),
    "dfta_scf_get_occupations": (C.c_int, [vp, C.c_int, C.c_int, c_dp]),
    "dfta_mixer_create": (C.c_int, [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(vp)]),
    "dfta_mixer_step": (C.c_int, [vp, C.c_double, c_dp, c_dp, c_dp, c_dp, c_ip]),
    "dfta_mixer_get": (C.c_int, [vp, C.c_int, c_ip, c_dp, c_dp, c_dp]),
    "dfta_mixer_destroy": (None, [vp]),
    "dfta_scf_get_orbitals": (C.c_int, [vp, C.c_int, C.c_int, c_dp]),
    "dfta_scf_orbital_properties": (C.c_int, [vp, c_dp]),
    "dfta_scf_orbital_matrix": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, c_dp]),
    "dfta_orbital_properties": (C.c_int, [vp, vp, C.c_int, c_ip, c_dp, c_dp]),
    "dfta_orbital_matrix": (C.c_int, [vp, vp, C.c_int, c_dp, C.c_int, c_dp]),
    "dfta_gaunt_3j2": (C.c_int, [C.c_int, C.c_int, C.c_int, c_dp]),
    "dfta_slater_fg_jobs": (C.c_int, [C.c_int, c_ip, c_ip, c_ip]),
    "dfta_slater_rk": (C.c_int, [vp, vp, C.c_int, c_dp, C.c_int, c_ip, c_dp]),
    "dfta_scf_slater_rk": (C.c_int, [vp, C.c_int, C.c_int, c_ip, c_dp]),
    "dfta_scf_slater_fg": (C.c_int, [vp, C.c_int, C.c_int, c_dp, c_dp]),
    "dfta_scf_coulomb_exchange": (C.c_int, [vp, C.c_int, c_dp, c_dp]),
    "dfta_exchange_jobs": (C.c_int, [C.c_int, c_ip, c_ip]),
    "dfta_screening_yk": (C.c_int, [vp, vp, C.c_int, c_dp, C.c_int, c_ip, c_dp]),
    "dfta_scf_screening_yk": (C.c_int, [vp, C.c_int, C.c_int, c_ip, c_dp]),
    "dfta_exchange_potentials": (C.c_int, [vp, vp, C.c_int, c_ip, c_dp, C.c_int, c_dp, c_dp, c_dp, c_dp, c_dp, c_dp, c_dp]),
    "dfta_scf_exchange_potentials": (C.c_int, [vp, C.c_int, C.c_int, c_dp, c_dp, c_dp, c_dp, c_dp, c_dp, c_ip]),
    "dfta_scf_set_exchange": (C.c_int, [vp, C.c_int]),
    "dfta_scf_get_exchange": (C.c_int, [vp, C.c_int, C.c_int, c_dp, c_dp, c_dp]),
    "dfta_scf_exchange_ms": (C.c_int, [vp, C.POINTER(C.c_float)]),
    "dfta_kli_channels": (C.c_int, [vp, vp, C.c_int, c_ip, c_ip, c_dp, c_dp, c_dp, C.c_int, C.c_double, c_dp, c_dp, c_dp, c_dp, c_ip, c_dp]),
    "dfta_sic_channels": (C.c_int, [vp, vp, C.c_int, c_ip, c_ip, c_dp, c_dp, c_dp, C.c_int, C.c_double] + [c_dp] * 12 + [c_ip, c_dp, c_dp, c_dp]),
    "dfta_scf_sic_table": (C.c_int, [vp, C.c_int, C.c_int, c_dp, c_dp, c_dp, c_dp, c_ip]),
    "dfta_sph_bessel": (C.c_int, [vp, C.c_int, C.c_size_t, c_dp, c_dp]),
    "dfta_bessel_transform": (C.c_int, [vp, vp, C.c_int, C.c_int, c_ip, c_dp, C.c_int, c_dp, c_dp]),
    "dfta_scf_form_factors": (C.c_int, [vp, C.c_int, c_dp, c_dp]),
    "dfta_scf_momentum_orbitals": (C.c_int, [vp, C.c_int, c_dp, c_dp]),
    "dfta_continuum": (C.c_int, [vp, vp, C.c_int, C.c_int, c_dp, C.c_int, c_ip, c_ip, c_dp, c_ip, C.c_int, c_dp, C.c_int, C.c_int, c_ip, c_ip,
                                 c_ip, c_dp, c_ip, c_dp, c_dp, c_ip, c_dp, c_dp]),
    "dfta_scf_continuum": (C.c_int, [vp, C.c_int, C.c_int, c_ip, c_ip, c_ip, c_dp, c_ip, C.c_int, c_dp, c_ip, c_dp, c_dp, c_ip, c_dp, c_ip,
                                     c_dp]),
    "dfta_scf_photoionization": (C.c_int, [vp, C.c_int, C.c_int, c_dp, C.c_int, c_dp, c_dp]),
    "dfta_pseudize": (C.c_int, [vp, vp, C.c_int, c_dp, c_dp, c_ip, c_dp, c_ip, c_dp, c_dp, c_dp, c_dp, c_dp, c_ip, c_ip]),
    "dfta_pseudo_ionic": (C.c_int, [vp, vp, C.c_int, C.c_int, C.c_int, c_ip, c_ip, c_dp, c_dp, c_dp, c_dp, c_ip] + [c_dp] * 6),
    "dfta_scf_pseudopotentials": (C.c_int, [vp, C.c_int, c_ip, c_ip, c_ip, C.c_double, c_ip, c_ip, c_dp, c_dp, c_dp, c_dp, c_dp, c_ip, c_ip]
                                  + [c_dp] * 6),
    "dfta_pseudo_default_valence": (C.c_int, [C.c_int, c_ip, c_ip, c_ip, C.c_int, c_ip, c_ip]),
    "dfta_pseudo_default_ic": (C.c_int, [vp, C.c_int, c_dp, C.c_double, c_ip]),
    "dfta_kb_sweep": (C.c_int, [vp, vp, C.c_int, c_dp, C.c_int, c_ip, c_ip, c_dp, c_dp, C.c_int, c_ip, c_dp, c_ip] + [c_dp] * 6 + [c_ip, c_dp]),
    "dfta_kb_bound_states": (C.c_int, [vp, vp, C.c_int, c_dp, C.c_int, c_ip, c_ip, c_dp, c_dp, c_ip, c_dp, c_dp, C.c_int, c_ip, c_dp, c_ip,
                                       c_ip]),
    "dfta_kb_ghost_report": (C.c_int, [vp, vp, C.c_int, C.c_int, c_ip, c_ip, c_dp, c_dp, c_dp, c_dp, c_ip, C.c_int, C.c_double, C.c_double,
                                       C.c_int, C.c_double, c_dp, c_dp]),
}

_lib = None


def load():
    """Load libdftatom_hip.so and bind every declared symbol.  Raises if the library is absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise DftaError("%s is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                        "(there is no CPU fallback)" % LIB_PATH)
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        f = getattr(lib, name)       # AttributeError if a declared symbol is not exported
        f.restype = res
        f.argtypes = args
    if lib.dfta_abi_version() != ABI_VERSION:      # the struct mirrors above follow the header (struct_size first, growth at the end)
        raise DftaError("%s was built from another version of include/dftatom_hip.h (ABI %d, binding %d): rebuild it"
                        % (LIB_PATH, lib.dfta_abi_version(), ABI_VERSION))
    _lib = lib
    return lib


def _dp(a):
    return a.ctypes.data_as(c_dp)


def _ip(a):
    return a.ctypes.data_as(c_ip)


def _i32(a):
    return np.ascontiguousarray(a, dtype=np.int32)


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


_CONFIG_CAP = 32


def _config_call(fn, *head):
    nA, nB = C.c_int(), C.c_int()
    an, al, bn, bl = (np.zeros(_CONFIG_CAP, np.int32) for _ in range(4))
    ao, bo = np.zeros(_CONFIG_CAP), np.zeros(_CONFIG_CAP)
    rc = fn(*head, _CONFIG_CAP, C.byref(nA), C.byref(nB), _ip(an), _ip(al), _dp(ao), _ip(bn), _ip(bl), _dp(bo))
    if rc != OK:
        raise DftaError("invalid electron configuration: %s" % load().dfta_config_last_error().decode())
    return {"alpha": [(int(an[k]), int(al[k]), float(ao[k])) for k in range(nA.value)],
            "beta": [(int(bn[k]), int(bl[k]), float(bo[k])) for k in range(nB.value)]}


def parse_config(Z, text, lsda=False, aufbau=AUFBAU_REFERENCE):
    """dfta_config_parse: '[Ne] 3s2 3p5.5', '1s2 2s1 2p3/1' (LSDA split) ... -> {"alpha": [(n, l, occ), ...], "beta": [...]}
    (LDA: every level under "alpha"), sorted by (n, l); n as get_subshells counts it (principal quantum number - 1).  Raises DftaError with the reason on an invalid configuration."""
    lib = load()
    return _config_call(lib.dfta_config_parse, int(Z), int(bool(lsda)), int(aufbau), text.encode())


def ion_config(Z, charge, lsda=False, aufbau=AUFBAU_REFERENCE):
    """dfta_ion_config: the Aufbau configuration of Z with `charge` electrons removed from the outermost subshell(s)
    (highest n, then highest l: Fe+ = 3d6 4s1), split by spin as the default path splits it."""
    lib = load()
    return _config_call(lib.dfta_ion_config, int(Z), int(charge), int(bool(lsda)), int(aufbau))


def config_electrons(cfg):
    """electron count of a configuration returned by parse_config / ion_config"""
    return sum(o for _, _, o in cfg["alpha"]) + sum(o for _, _, o in cfg["beta"])


class Context:
    """Device context (dfta_ctx).  `stream` may be a raw hipStream_t (int), e.g.
    torch.cuda.current_stream().cuda_stream; None -> stream owned by the context."""

    def __init__(self, device=0, stream=None):
        self.lib = load()
        h = vp()
        rc = self.lib.dfta_ctx_create(device, vp(stream) if stream else None, C.byref(h))
        if rc != OK:
            raise DftaError("dfta_ctx_create failed with status %d (no usable HIP device?)" % rc)
        self.h = h

    def check(self, rc):
        if rc != OK:
            raise DftaError("status %d: %s" % (rc, self.lib.dfta_last_error(self.h).decode()))

    def synchronize(self):
        self.check(self.lib.dfta_ctx_synchronize(self.h))

    def device_info(self):
        ncu = C.c_int()
        name = C.create_string_buffer(128)
        self.check(self.lib.dfta_ctx_device_info(self.h, C.byref(ncu), name, 128))
        return ncu.value, name.value.decode()

    def set_sweep_kernel(self, which):
        """SWEEP_KERNEL_AUTO / _FUSED / _PIPELINED: which (bit-identical) Numerov sweep kernel later calls launch."""
        self.check(self.lib.dfta_ctx_set_sweep_kernel(self.h, int(which)))

    def measure_hbm(self, doubles_per_array=1 << 27, reps=5):
        """attainable HBM bandwidth (GB/s) of the device: (copy, triad) -- measurement aid for the roofline denominators"""
        c, t = C.c_double(), C.c_double()
        self.check(self.lib.dfta_ctx_measure_hbm(self.h, int(doubles_per_array), int(reps), C.byref(c), C.byref(t)))
        return c.value, t.value

    def last_kernel_ms(self):
        ms = C.c_float()
        self.check(self.lib.dfta_ctx_last_kernel_ms(self.h, C.byref(ms)))
        return ms.value

    def close(self):
        if self.h:
            self.lib.dfta_ctx_destroy(self.h)
            self.h = None


class Grid:
    """Logarithmic grid r_i = Rp (exp(i delta) - 1), or -- delta = None / 0 -- the uniform grid r_i = i Rmax / (N - 1)."""

    def __init__(self, ctx, mg_levels, delta, Rmax):
        self.ctx = ctx
        h = vp()
        self.uniform = not delta
        if self.uniform:
            ctx.check(ctx.lib.dfta_grid_create_uniform(ctx.h, mg_levels, Rmax, C.byref(h)))
        else:
            ctx.check(ctx.lib.dfta_grid_create(ctx.h, mg_levels, delta, Rmax, C.byref(h)))
        self.h = h
        self.levels, self.delta, self.Rmax = mg_levels, (delta or 0.0), Rmax
        self.N = ctx.lib.dfta_grid_num_nodes(h)
        self.Rp = ctx.lib.dfta_grid_rp(h)

    def r(self):
        out = np.zeros(self.N)
        self.ctx.check(self.ctx.lib.dfta_grid_get_r(self.h, _dp(out)))
        return out

    def close(self):
        if self.h:
            self.ctx.lib.dfta_grid_destroy(self.h)
            self.h = None


def numerov_sweeps(ctx, grid, kind, V, l, E, limit=None, vidx=None, boundary=BOUNDARY_HOST):
    """Batched SolveSchrodingerCountNodes / SolutionInZero.  Returns dict(count, u0, start, trip)."""
    V = _f64(V).reshape(-1, grid.N)
    l = _i32(l)
    E = _f64(E)
    nt = len(E)
    lim = _i32(limit) if limit is not None else np.zeros(nt, np.int32)
    vi = _i32(vidx) if vidx is not None else np.zeros(nt, np.int32)
    count = np.zeros(nt, np.int32)
    u0 = np.zeros(nt)
    start = np.zeros(nt, np.int32)
    trip = np.zeros(nt, np.int32)
    ctx.check(ctx.lib.dfta_numerov_sweeps(ctx.h, grid.h, kind, boundary, V.shape[0], _dp(V), nt, _ip(vi), _ip(l), _dp(E),
                                          _ip(lim), _ip(count), _dp(u0), _ip(start), _ip(trip)))
    return {"count": count, "u0": u0, "start": start, "trip": trip}


def numerov_sweeps_scan(ctx, grid, kind, V, l, E, limit=None, vidx=None):
    """Tolerance mode of the same sweeps (transfer-matrix scan, one workgroup per trial).  Returns dict(count, u0, start, trip, fallback)."""
    V = _f64(V).reshape(-1, grid.N)
    l = _i32(l)
    E = _f64(E)
    nt = len(E)
    lim = _i32(limit) if limit is not None else np.zeros(nt, np.int32)
    vi = _i32(vidx) if vidx is not None else np.zeros(nt, np.int32)
    count, start, trip, fb = (np.zeros(nt, np.int32) for _ in range(4))
    u0 = np.zeros(nt)
    ctx.check(ctx.lib.dfta_numerov_sweeps_scan(ctx.h, grid.h, kind, V.shape[0], _dp(V), nt, _ip(vi), _ip(l), _dp(E), _ip(lim), _ip(count),
                                               _dp(u0), _ip(start), _ip(trip), _ip(fb)))
    return {"count": count, "u0": u0, "start": start, "trip": trip, "fallback": fb}


class Potential:
    """A potential resident on the device with its slot tables (dfta_potential): per-call sweeps without the upload and table build."""

    def __init__(self, ctx, grid, V):
        self.ctx, self.grid = ctx, grid
        h = vp()
        V = _f64(V)
        ctx.check(ctx.lib.dfta_potential_create(ctx.h, grid.h, _dp(V), C.byref(h)))
        self.h = h

    def update(self, V):
        V = _f64(V)
        self.ctx.check(self.ctx.lib.dfta_potential_update(self.h, _dp(V)))

    def sweeps(self, kind, l, E, limit=None, sweep_mode=SWEEPS_EXACT):
        l, E = _i32(l), _f64(E)
        nt = len(E)
        lim = _i32(limit) if limit is not None else np.zeros(nt, np.int32)
        count, start, trip = (np.zeros(nt, np.int32) for _ in range(3))
        u0 = np.zeros(nt)
        self.ctx.check(self.ctx.lib.dfta_potential_sweeps(self.h, kind, sweep_mode, nt, _ip(l), _dp(E), _ip(lim), _ip(count), _dp(u0), _ip(start), _ip(trip)))
        return {"count": count, "u0": u0, "start": start, "trip": trip}

    def match(self, l, E):
        l, E = _i32(l), _f64(E)
        nt = len(E)
        psi = np.zeros((nt, self.grid.N))
        mp = np.zeros(nt, np.int64)
        self.ctx.check(self.ctx.lib.dfta_potential_match(self.h, nt, _ip(l), _dp(E), _dp(psi), mp.ctypes.data_as(c_lp)))
        return psi, mp

    def close(self):
        if self.h:
            self.ctx.lib.dfta_potential_destroy(self.h)
            self.h = None


def numerov_match(ctx, grid, V, l, E, vidx=None, boundary=BOUNDARY_HOST):
    V = _f64(V).reshape(-1, grid.N)
    l = _i32(l)
    E = _f64(E)
    nt = len(E)
    vi = _i32(vidx) if vidx is not None else np.zeros(nt, np.int32)
    psi = np.zeros((nt, grid.N))
    mp = np.zeros(nt, np.int64)
    ctx.check(ctx.lib.dfta_numerov_match(ctx.h, grid.h, boundary, V.shape[0], _dp(V), nt, _ip(vi), _ip(l), _dp(E),
                                         _dp(psi), mp.ctypes.data_as(c_lp)))
    return psi, mp


def get_subshells(Z, aufbau=AUFBAU_REFERENCE):
    lib = load()
    n, l, occ = (np.zeros(32, np.int32) for _ in range(3))
    c = lib.dfta_get_subshells_ex(Z, aufbau, _ip(n), _ip(l), _ip(occ), 32)
    if c < 0:
        raise DftaError("dfta_get_subshells(%d) failed" % Z)
    return [(int(n[i]), int(l[i]), int(occ[i])) for i in range(c)]


def solve_levels(ctx, grid, V, levels, bottom0, vidx=None, mode=LEVELS_BATCHED, tree_depth=0, want_psi=False, hints=None):
    """Device-side LoopOverLevels for `levels` = [(n, l, occ), ...] on potentials V (nV x N).
    Returns dict(E, top, bottom, n_count, n_zero, converged, matchPoint, newDensity, Eelectronic, psi, issued)."""
    V = _f64(V).reshape(-1, grid.N)
    nV = V.shape[0]
    nl = len(levels)
    n = _i32([a for a, _, _ in levels])
    l = _i32([b for _, b, _ in levels])
    occ = _i32([c for _, _, c in levels])
    vi = _i32(vidx) if vidx is not None else np.zeros(nl, np.int32)
    b0 = _f64(np.broadcast_to(np.asarray(bottom0, dtype=np.float64), (nV,)))
    res = (LevelResult * nl)()
    nd = np.zeros((nV, grid.N))
    eel = np.zeros(nV)
    psi = np.zeros((nl, grid.N)) if want_psi else None
    issued = C.c_long(0)
    hh = _f64(hints) if hints is not None else None
    ctx.check(ctx.lib.dfta_solve_levels(ctx.h, grid.h, mode, tree_depth, nV, _dp(V), _dp(b0), _dp(hh) if hh is not None else None,
                                        nl, _ip(vi), _ip(n), _ip(l),
                                        _ip(occ), res, _dp(nd), _dp(eel), _dp(psi) if want_psi else None, C.byref(issued)))
    out = {k: np.array([getattr(res[i], k) for i in range(nl)]) for k in
           ("E", "top", "bottom", "n_count", "n_zero", "converged", "matchPoint", "status")}
    out.update(newDensity=nd, Eelectronic=eel, psi=psi, issued=issued.value)
    return out


def integrate(ctx, rule, delta, values):
    v = _f64(values)
    out = C.c_double()
    ctx.check(ctx.lib.dfta_integrate(ctx.h, rule, delta, _dp(v), len(v), C.byref(out)))
    return out.value


class Poisson:
    """DFT::PoissonSolver for a batch of atoms on one grid (dfta_poisson)."""

    def __init__(self, ctx, grid, batch=1, mode=POISSON_DEFAULT):
        self.ctx, self.grid, self.batch = ctx, grid, batch
        h = vp()
        if mode == POISSON_DEFAULT:
            ctx.check(ctx.lib.dfta_poisson_create(ctx.h, grid.h, batch, C.byref(h)))
        else:
            ctx.check(ctx.lib.dfta_poisson_create_ex(ctx.h, grid.h, batch, int(mode), C.byref(h)))
        self.h = h
        self.mode = ctx.lib.dfta_poisson_mode(h)

    def solve(self, Z, density):
        """SolvePoissonNonUniform: density (batch x N) -> U (batch x N), vcycles, err."""
        Z = _i32(np.atleast_1d(Z))
        rho = _f64(density).reshape(self.batch, self.grid.N)
        U = np.zeros_like(rho)
        vc = np.zeros(self.batch, np.int32)
        err = np.zeros(self.batch)
        self.ctx.check(self.ctx.lib.dfta_poisson_solve(self.h, _ip(Z), _dp(rho), _dp(U), _ip(vc), _dp(err)))
        return U, vc, err

    def group_info(self):
        """(workgroups per atom, degraded to one workgroup per atom?, solves that had to be repeated)"""
        g, d, a = C.c_int(), C.c_int(), C.c_int()
        self.ctx.check(self.ctx.lib.dfta_poisson_group_info(self.h, C.byref(g), C.byref(d), C.byref(a)))
        return g.value, bool(d.value), a.value

    def predict_counts(self):
        """(fused visits that ran with predicted start values and a hand-over check, visits whose check failed and that were repeated)
        since the solver was created"""
        c, r = C.c_ulonglong(), C.c_ulonglong()
        self.ctx.check(self.ctx.lib.dfta_poisson_predict_counts(self.h, C.byref(c), C.byref(r)))
        return c.value, r.value

    def level_size(self, lvl):
        return self.ctx.lib.dfta_poisson_level_size(self.h, lvl)

    def set_level(self, lvl, phi=None, src=None):
        self.ctx.check(self.ctx.lib.dfta_poisson_set_level(self.h, lvl, _dp(_f64(phi)) if phi is not None else None,
                                                           _dp(_f64(src)) if src is not None else None))

    def get_level(self, lvl):
        n = self.level_size(lvl)
        phi, src = np.zeros(n), np.zeros(n)
        self.ctx.check(self.ctx.lib.dfta_poisson_get_level(self.h, lvl, _dp(phi), _dp(src)))
        return phi, src

    def gauss_seidel(self, lvl, sweeps=1):
        err = np.zeros(sweeps)
        self.ctx.check(self.ctx.lib.dfta_poisson_gauss_seidel(self.h, lvl, sweeps, _dp(err)))
        return err

    def iterate_gs(self, lvl, error_min, iterno):
        """IterateGaussSeidel: returns (err of the last sweep, sweeps executed)."""
        err = C.c_double()
        n = C.c_int()
        self.ctx.check(self.ctx.lib.dfta_poisson_iterate_gs(self.h, lvl, error_min, iterno, C.byref(err), C.byref(n)))
        return err.value, n.value

    def restrict(self, lvl):
        self.ctx.check(self.ctx.lib.dfta_poisson_restrict(self.h, lvl))

    def prolong(self, lvl_src):
        self.ctx.check(self.ctx.lib.dfta_poisson_prolong(self.h, lvl_src))

    def vcycle(self):
        err = np.zeros(1)
        self.ctx.check(self.ctx.lib.dfta_poisson_vcycle(self.h, _dp(err)))
        return err[0]

    def full_cycle(self, low, high, error_min=1e-3, error_min_last=1e-14):
        """SetBoundaries + FullCycle on the source left by the last solve: returns (err, V-cycles)."""
        err, vc = C.c_double(), C.c_int()
        self.ctx.check(self.ctx.lib.dfta_poisson_full_cycle(self.h, low, high, error_min, error_min_last, C.byref(err), C.byref(vc)))
        return err.value, vc.value

    def close(self):
        if self.h:
            self.ctx.lib.dfta_poisson_destroy(self.h)
            self.h = None


def vwn_lda(ctx, n):
    n = _f64(n)
    v, e = np.zeros_like(n), np.zeros_like(n)
    ctx.check(ctx.lib.dfta_vwn_lda(ctx.h, _dp(n), n.size, _dp(v), _dp(e)))
    return v, e


def chachiyo_lda(ctx, n, improved=True):
    n = _f64(n)
    v, e = np.zeros_like(n), np.zeros_like(n)
    ctx.check(ctx.lib.dfta_chachiyo_lda(ctx.h, int(improved), _dp(n), n.size, _dp(v), _dp(e)))
    return v, e


def vwn_lsda(ctx, na, nb):
    na, nb = _f64(na), _f64(nb)
    r, va, vb, e = (np.zeros_like(na) for _ in range(4))
    ctx.check(ctx.lib.dfta_vwn_lsda(ctx.h, _dp(na), _dp(nb), na.size, _dp(r), _dp(va), _dp(vb), _dp(e)))
    return r, va, vb, e


def xc_pointwise(ctx, functional, na, nb=None, saa=None, sab=None, sbb=None):
    """e (per volume) and its partial derivatives for XC_PW92 / XC_PBE at independent points.  nb None: unpolarised
    (n = na, sigma = saa): returns dict(e, dn, dsigma); else dict(e, dna, dnb, dsaa, dsab, dsbb)."""
    na = _f64(na).ravel()
    sz = na.size
    arr = lambda a: None if a is None else _f64(np.broadcast_to(np.asarray(a, dtype=np.float64), na.shape)).ravel()
    nb, saa, sab, sbb = arr(nb), arr(saa), arr(sab), arr(sbb)
    p = lambda a: None if a is None else _dp(a)
    out = [np.zeros(sz) for _ in range(6)]
    pol = nb is not None
    ctx.check(ctx.lib.dfta_xc_pointwise(ctx.h, int(functional), sz, _dp(na), p(nb), p(saa), p(sab), p(sbb), _dp(out[0]), _dp(out[1]),
                                        _dp(out[2]) if pol else None, _dp(out[3]), _dp(out[4]) if pol else None,
                                        _dp(out[5]) if pol else None))
    if not pol:
        return {"e": out[0], "dn": out[1], "dsigma": out[3]}
    return dict(zip(("e", "dna", "dnb", "dsaa", "dsab", "dsbb"), out))


def xc_radial(ctx, grid, functional, na, nb=None):
    """The SCF's XC_PW92 / XC_PBE evaluation on `grid` for densities na (and nb: LSDA) of shape (natoms, N) or (N,).
    LDA: returns (Vexc, eexc); LSDA: (res, va, vb, eexc) -- the outputs k_tail consumes (include/dftatom_hip.h)."""
    na = _f64(na)
    shape = na.shape
    na = na.reshape(-1, grid.N)
    natoms = na.shape[0]
    res, eexc = np.zeros_like(na), np.zeros_like(na)
    if nb is None:
        ctx.check(ctx.lib.dfta_xc_radial(ctx.h, grid.h, int(functional), natoms, _dp(na), None, _dp(res), None, None, _dp(eexc)))
        return res.reshape(shape), eexc.reshape(shape)
    nb = _f64(nb).reshape(natoms, grid.N)
    va, vb = np.zeros_like(na), np.zeros_like(na)
    ctx.check(ctx.lib.dfta_xc_radial(ctx.h, grid.h, int(functional), natoms, _dp(na), _dp(nb), _dp(res), _dp(va), _dp(vb), _dp(eexc)))
    return res.reshape(shape), va.reshape(shape), vb.reshape(shape), eexc.reshape(shape)


def orbital_properties(ctx, grid, l, u):
    """dfta_orbital_properties on caller-supplied orbitals u = r R of shape (norb, N) with angular momenta l: (norb, ORB_PROPS), columns
    ORB_NORM .. ORB_RM3 (include/dftatom_hip.h has the definitions)."""
    u = _f64(u).reshape(-1, grid.N)
    l = _i32(np.atleast_1d(l))
    if len(l) != u.shape[0]:
        raise ValueError("%d angular momenta for %d orbitals" % (len(l), u.shape[0]))
    props = np.zeros((u.shape[0], ORB_PROPS))
    ctx.check(ctx.lib.dfta_orbital_properties(ctx.h, grid.h, u.shape[0], _ip(l), _dp(u), _dp(props)))
    return props


def orbital_matrix(ctx, grid, u, k):
    """dfta_orbital_matrix: M_ab = Q[u_a u_b r^k dr/di] (k = 0, 1, 2) for u of shape (norb <= 32, N): (norb, norb), symmetric bit for bit."""
    u = _f64(u).reshape(-1, grid.N)
    M = np.zeros((u.shape[0], u.shape[0]))
    ctx.check(ctx.lib.dfta_orbital_matrix(ctx.h, grid.h, u.shape[0], _dp(u), int(k), _dp(M)))
    return M


def gaunt_3j2(la, k, lb):
    """(la k lb; 0 0 0)^2, the angular factor of the exchange sum (host-only; 0.0 where parity or the triangle rule fails)"""
    out = C.c_double()
    if load().dfta_gaunt_3j2(int(la), int(k), int(lb), C.byref(out)) != OK:
        raise DftaError("dfta_gaunt_3j2(%d, %d, %d): arguments must be >= 0 and la, lb <= 4" % (la, k, lb))
    return out.value


def slater_fg_jobs(l):
    """dfta_slater_fg_jobs (host-only): (jobs, kinds) for orbitals of angular momenta l -- jobs (njobs, 5) int32 rows a, b, c, d, k,
    first the F^k(a,b) (a <= b, kinds SLATER_F), then the G^k(a,b) (a < b, SLATER_G)"""
    lib = load()
    l = _i32(np.atleast_1d(l))
    n = lib.dfta_slater_fg_jobs(len(l), _ip(l), None, None)
    if n < 0:
        raise DftaError("dfta_slater_fg_jobs: angular momenta must lie in 0 .. 4")
    jobs, kinds = np.zeros((n, 5), np.int32), np.zeros(n, np.int32)
    lib.dfta_slater_fg_jobs(len(l), _ip(l), _ip(jobs), _ip(kinds))
    return jobs, kinds


def slater_rk(ctx, grid, u, jobs):
    """dfta_slater_rk: the Slater integrals R^k(ab,cd) of the rows (a, b, c, d, k) of jobs over orbitals u = r R of shape (norb, N),
    every job in one launch: (njobs,).  F^k(a,b) = R^k(ab,ab), G^k(a,b) = R^k(ab,ba); 0 <= k <= SLATER_KMAX."""
    u = _f64(u).reshape(-1, grid.N)
    jobs = _i32(jobs).reshape(-1, 5)
    R = np.zeros(len(jobs))
    ctx.check(ctx.lib.dfta_slater_rk(ctx.h, grid.h, u.shape[0], _dp(u), len(jobs), _ip(jobs), _dp(R)))
    return R


def exchange_jobs(l):
    """dfta_exchange_jobs (host-only): the y jobs of a spin channel with angular momenta l, (njobs, 3) int32 rows x, y, k -- a, then
    b >= a, then k of the exchange sum ascending"""
    lib = load()
    l = _i32(np.atleast_1d(l))
    n = lib.dfta_exchange_jobs(len(l), _ip(l), None)
    if n < 0:
        raise DftaError("dfta_exchange_jobs: angular momenta must lie in 0 .. 4")
    jobs = np.zeros((n, 3), np.int32)
    lib.dfta_exchange_jobs(len(l), _ip(l), _ip(jobs))
    return jobs


def screening_yk(ctx, grid, u, jobs):
    """dfta_screening_yk: the screening functions y^k_xy(r) = Y^k_xy(r) / r of the rows (x, y, k) of jobs over orbitals u = r R of shape
    (norb, N), every job in one launch: (njobs, N).  y^0_aa is the Hartree potential of one electron in orbital a."""
    u = _f64(u).reshape(-1, grid.N)
    jobs = _i32(jobs).reshape(-1, 3)
    y = np.zeros((len(jobs), grid.N))
    ctx.check(ctx.lib.dfta_screening_yk(ctx.h, grid.h, u.shape[0], _dp(u), len(jobs), _ip(jobs), _dp(y)))
    return y


def _xp_outputs(norb, N):
    return {"X": np.zeros((norb, N)), "D": np.zeros(N), "vS": np.zeros(N), "vKLI": np.zeros(N), "vbar": np.zeros((norb, XP_COLS)),
            "M": np.zeros((norb, norb))}


def exchange_potentials(ctx, grid, l, occ, homo, u):
    """dfta_exchange_potentials for one spin channel: shells with angular momenta l, channel occupations occ, HOMO index homo and
    orbitals u (norb, N).  A dict: X (norb, N) the exchange operator applied to each orbital, D = Sum n u^2, vS Slater's potential,
    vKLI the KLI potential (N each), vbar (norb, XP_COLS) with columns XP_HF, XP_S, XP_C, XP_KLI, M (norb, norb), homo."""
    u = _f64(u).reshape(-1, grid.N)
    l, occ = _i32(np.atleast_1d(l)), _f64(np.atleast_1d(occ))
    if len(l) != u.shape[0] or len(occ) != u.shape[0]:
        raise ValueError("%d angular momenta and %d occupations for %d orbitals" % (len(l), len(occ), u.shape[0]))
    out = _xp_outputs(u.shape[0], grid.N)
    ctx.check(ctx.lib.dfta_exchange_potentials(ctx.h, grid.h, u.shape[0], _ip(l), _dp(occ), int(homo), _dp(u), _dp(out["X"]), _dp(out["D"]),
                                               _dp(out["vS"]), _dp(out["vKLI"]), _dp(out["vbar"]), _dp(out["M"])))
    out["homo"] = int(homo)
    return out


def kli_channels(ctx, grid, norb, l, occ, E, u, first_step=True, alpha=0.5, vx=None):
    """dfta_kli_channels: the batched exchange stage of a KLI step on caller-supplied spin channels.  norb: shells per channel; l, occ
    (channel occupations), E (eigenvalues, for the HOMO rule): the channels' shells end to end; u (sum norb, N) their orbitals.
    first_step: vx = v_raw; otherwise vx (nch, N) is mixed as alpha vx + (1 - alpha) v_raw.  A dict: vx, v_raw (nch, N), vbarHF, c (per
    shell), homo, Ex (per channel: 0.5 Sum n vbarHF)."""
    norb = _i32(np.atleast_1d(norb))
    nch, tot = len(norb), int(np.sum(norb))
    l, occ, E = _i32(np.atleast_1d(l)), _f64(np.atleast_1d(occ)), _f64(np.atleast_1d(E))
    u = _f64(u).reshape(-1, grid.N)
    if not (len(l) == len(occ) == len(E) == u.shape[0] == tot):
        raise ValueError("%d shells: %d l, %d occ, %d E, %d orbitals" % (tot, len(l), len(occ), len(E), u.shape[0]))
    if first_step:
        vx = np.zeros((nch, grid.N))
    else:
        vx = _f64(vx).reshape(nch, grid.N).copy()
    out = {"vx": vx, "v_raw": np.zeros((nch, grid.N)), "vbarHF": np.zeros(max(tot, 1)), "c": np.zeros(max(tot, 1)),
           "homo": np.zeros(nch, np.int32), "Ex": np.zeros(nch)}
    ctx.check(ctx.lib.dfta_kli_channels(ctx.h, grid.h, nch, _ip(norb), _ip(l), _dp(occ), _dp(E), _dp(u), int(bool(first_step)), float(alpha),
                                        _dp(out["vx"]), _dp(out["v_raw"]), _dp(out["vbarHF"]), _dp(out["c"]), _ip(out["homo"]), _dp(out["Ex"])))
    out["vbarHF"], out["c"] = out["vbarHF"][:tot], out["c"][:tot]
    return out


def sic_channels(ctx, grid, norb, l, occ, E, u, first_step=True, alpha=0.5, vx=None):
    """dfta_sic_channels: the SIC-KLI stage of a step on caller-supplied spin channels, arguments as kli_channels.  A dict: y0, vorb, eps,
    X (sum norb, N): the Hartree potential, the fully polarised VWN potential and energy density of each shell's one-electron density and
    X_a = (y0_a + v_a) u_a; D, vS, v_raw, vx (nch, N); vbar, vbarS, c, EH, EXC (per shell); M (a list of (norb, norb) matrices, one per
    channel); homo, Esic (per channel)."""
    norb = _i32(np.atleast_1d(norb))
    nch, tot = len(norb), int(np.sum(norb))
    l, occ, E = _i32(np.atleast_1d(l)), _f64(np.atleast_1d(occ)), _f64(np.atleast_1d(E))
    u = _f64(u).reshape(-1, grid.N)
    if not (len(l) == len(occ) == len(E) == u.shape[0] == tot):
        raise ValueError("%d shells: %d l, %d occ, %d E, %d orbitals" % (tot, len(l), len(occ), len(E), u.shape[0]))
    if first_step:
        vx = np.zeros((nch, grid.N))
    else:
        vx = _f64(vx).reshape(nch, grid.N).copy()
    rows, per = max(tot, 1), ("vbar", "vbarS", "c", "EH", "EXC")
    flatM = np.zeros(max(int(np.sum(norb.astype(np.int64) ** 2)), 1))
    out = {"vx": vx, "homo": np.zeros(nch, np.int32), "Esic": np.zeros(nch)}
    out.update({k: np.zeros((rows, grid.N)) for k in ("y0", "vorb", "eps", "X")})
    out.update({k: np.zeros((nch, grid.N)) for k in ("D", "vS", "v_raw")})
    out.update({k: np.zeros(rows) for k in per})
    ctx.check(ctx.lib.dfta_sic_channels(ctx.h, grid.h, nch, _ip(norb), _ip(l), _dp(occ), _dp(E), _dp(u), int(bool(first_step)), float(alpha),
                                        _dp(out["vx"]), _dp(out["y0"]), _dp(out["vorb"]), _dp(out["eps"]), _dp(out["X"]), _dp(out["D"]),
                                        _dp(out["vS"]), _dp(out["v_raw"]), _dp(out["vbar"]), _dp(out["c"]), _dp(out["EH"]), _dp(out["EXC"]),
                                        _ip(out["homo"]), _dp(out["Esic"]), _dp(out["vbarS"]), _dp(flatM)))
    for k in ("y0", "vorb", "eps", "X") + per:
        out[k] = out[k][:tot]
    ends = np.cumsum(norb.astype(np.int64) ** 2)
    out["M"] = [flatM[e - n * n:e].reshape(n, n) for n, e in zip(norb, ends)]
    return out


def sph_bessel(ctx, l, x):
    """dfta_sph_bessel: the device's spherical Bessel function j_l (0 <= l <= BESSEL_LMAX) at the arguments x >= 0, in x's shape"""
    x = _f64(x)
    out = np.zeros(x.shape)
    ctx.check(ctx.lib.dfta_sph_bessel(ctx.h, int(l), x.size, _dp(x), _dp(out)))
    return out


def bessel_transform(ctx, grid, kind, l, f, q):
    """dfta_bessel_transform: rows f of shape (nrow, N) with orders l at the momenta q (nq,), every (row, q) in one launch: (nrow, nq).
    BT_DENSITY: 4 pi Q[f r^2 j_l(q r) dr/di] (f = rho, l = 0: the X-ray form factor); BT_ORBITAL: sqrt(2/pi) Q[f r j_l(q r) dr/di]
    (f = u_nl = r R_nl: the momentum-space radial function)."""
    f = _f64(f).reshape(-1, grid.N)
    l = _i32(np.atleast_1d(l))
    q = _f64(np.atleast_1d(q))
    if len(l) != f.shape[0]:
        raise ValueError("%d orders for %d rows" % (len(l), f.shape[0]))
    out = np.zeros((f.shape[0], len(q)))
    ctx.check(ctx.lib.dfta_bessel_transform(ctx.h, grid.h, int(kind), f.shape[0], _ip(l), _dp(f), len(q), _dp(q), _dp(out)))
    return out


def _cont_outputs(nt, N, want_sums, want_rows):
    out = {"logderiv": np.zeros(nt), "nodes": np.zeros(nt, np.int32), "delta": np.zeros(nt), "scale": np.zeros(nt),
           "status": np.zeros(nt, np.int32)}
    if want_sums:
        out["sums"] = np.zeros((nt, CONT_MAX_PARTNERS))
    if want_rows:
        out["rows"] = np.zeros((nt, N))
    return out


def continuum(ctx, grid, V, l, E, m=None, vidx=None, norm=CONT_FREE, partners=None, power=0, lists=None, trial_list=None, want_rows=False):
    """dfta_continuum: outward sweeps at any finite energy.  V: (nV, N) potentials; per trial l (0 .. 4), E, end node m (None: N-2) and
    vidx (None: 0).  partners: (nrows, N) bound orbitals u; lists: a list of lists of partner rows (at most 16 each), trial_list: the
    list of every trial (-1: none; None with lists given: list 0 for every trial); power: r^power in the sums.  Returns "logderiv"
    (u'/u at r_m), "nodes", "delta" (CONT_FREE: the phase shift; CONT_WKB: the WKB phase at r_m), "scale" (the normalisation factor; 0
    for E <= 0), "status" (CONT_* bits), "sums" (ntrials, 16) with partners, "rows" (ntrials, N) on request -- energy-normalised for E > 0."""
    V = _f64(V).reshape(-1, grid.N)
    l = _i32(np.atleast_1d(l))
    E = _f64(np.atleast_1d(E))
    nt = len(E)
    if len(l) != nt:
        raise ValueError("%d orders for %d energies" % (len(l), nt))
    m = np.full(nt, grid.N - 2, np.int32) if m is None else _i32(np.broadcast_to(m, (nt,)))
    vidx = None if vidx is None else _i32(np.broadcast_to(vidx, (nt,)))
    P = None if partners is None else _f64(partners).reshape(-1, grid.N)
    nrows = 0 if P is None else P.shape[0]
    if lists is None and P is not None:
        lists = [list(range(nrows))]
    lists = lists or []
    off = _i32(np.concatenate([[0], np.cumsum([len(x) for x in lists])])) if lists else None
    flat = _i32([r for x in lists for r in x]) if lists else None
    if lists and trial_list is None:
        trial_list = np.zeros(nt, np.int32)
    tl = None if trial_list is None else _i32(np.broadcast_to(trial_list, (nt,)))
    out = _cont_outputs(nt, grid.N, bool(lists), want_rows)
    ptr = lambda a, f: None if a is None else f(a)       # noqa: E731
    ctx.check(ctx.lib.dfta_continuum(ctx.h, grid.h, int(norm), V.shape[0], _dp(V), nt, ptr(vidx, _ip), _ip(l), _dp(E), _ip(m), nrows,
                                     ptr(P, _dp), int(power), len(lists), ptr(off, _ip), ptr(flat, _ip), ptr(tl, _ip), _dp(out["logderiv"]),
                                     _ip(out["nodes"]), _dp(out["delta"]), _dp(out["scale"]), _ip(out["status"]), ptr(out.get("sums"), _dp),
                                     ptr(out.get("rows"), _dp)))
    return out


def pseudize(ctx, grid, V, u, l, eps, ic):
    """dfta_pseudize: Troullier-Martins pseudization of the channels (V[k], u[k], l[k], eps[k], ic[k]); V, u: (nch, N).  Returns
    "u_ps", "V_ps" (nch, N), "coef" (nch, 7: a0, a2 .. a12 in x = r / r_c), "rc", "match" (nch, 8: P0 .. P4, I_AE, I_ps, g), "iters",
    "status" (PS_* bits; with any bit the channel's floating-point outputs are NaN)."""
    V = _f64(V).reshape(-1, grid.N)
    u = _f64(u).reshape(-1, grid.N)
    l, eps, ic = _i32(np.atleast_1d(l)), _f64(np.atleast_1d(eps)), _i32(np.atleast_1d(ic))
    nch = len(l)
    if not (V.shape[0] == u.shape[0] == len(eps) == len(ic) == nch):
        raise ValueError("pseudize: %d potentials, %d orbitals, %d l, %d eps, %d ic" % (V.shape[0], u.shape[0], nch, len(eps), len(ic)))
    out = {"u_ps": np.zeros((nch, grid.N)), "V_ps": np.zeros((nch, grid.N)), "coef": np.zeros((nch, PS_COEF)), "rc": np.zeros(nch),
           "match": np.zeros((nch, PS_MATCH)), "iters": np.zeros(nch, np.int32), "status": np.zeros(nch, np.int32)}
    ctx.check(ctx.lib.dfta_pseudize(ctx.h, grid.h, nch, _dp(V), _dp(u), _ip(l), _dp(eps), _ip(ic), _dp(out["u_ps"]), _dp(out["V_ps"]),
                                    _dp(out["coef"]), _dp(out["rc"]), _dp(out["match"]), _ip(out["iters"]), _ip(out["status"])))
    return out


def pseudo_ionic(ctx, grid, ps, l, occ, atom=None, functional=XC_VWN, l_loc=None):
    """dfta_pseudo_ionic: unscreening and Kleinman-Bylander quantities of the channels of a pseudize() result `ps`; l, occ per channel,
    atom: the atom of each channel (None: one atom), l_loc: the local l per atom (None: the highest l of the atom).  Returns "rho_v",
    "vH", "vxc" (natoms, N), "V_ion", "beta" (nch, N), "kb" (nch, 3: <u|dV|u>, <u|dV^2|u>, E_KB; the local channel 0, 0, NaN)."""
    u, V = _f64(ps["u_ps"]).reshape(-1, grid.N), _f64(ps["V_ps"]).reshape(-1, grid.N)
    nch = u.shape[0]
    l, occ = _i32(np.atleast_1d(l)), _f64(np.atleast_1d(occ))
    atom = np.zeros(nch, np.int32) if atom is None else _i32(np.atleast_1d(atom))
    if not (len(l) == len(occ) == len(atom) == nch == V.shape[0]):
        raise ValueError("pseudo_ionic: the channel arrays disagree in length")
    natoms = int(atom.max()) + 1 if nch else 0
    a0 = _f64(np.asarray(ps["coef"]).reshape(-1, PS_COEF)[:, 0])
    ll = None if l_loc is None else _i32(np.broadcast_to(l_loc, (natoms,)))
    out = {"rho_v": np.zeros((natoms, grid.N)), "vH": np.zeros((natoms, grid.N)), "vxc": np.zeros((natoms, grid.N)),
           "V_ion": np.zeros((nch, grid.N)), "beta": np.zeros((nch, grid.N)), "kb": np.zeros((nch, 3))}
    ctx.check(ctx.lib.dfta_pseudo_ionic(ctx.h, grid.h, int(functional), natoms, nch, _ip(atom), _ip(l), _dp(occ), _dp(a0), _dp(u), _dp(V),
                                        None if ll is None else _ip(ll), _dp(out["rho_v"]), _dp(out["vH"]), _dp(out["vxc"]),
                                        _dp(out["V_ion"]), _dp(out["beta"]), _dp(out["kb"])))
    return out


def default_valence(n, l, occ):
    """dfta_pseudo_default_valence: the indices of the levels (n, l, occ > 0) that a pseudopotential keeps as valence -- per l the
    occupied level of largest n, if n >= n_max - max(0, l - 1).  Host integers only."""
    n, l, occ = _i32(n), _i32(l), _i32(np.ceil(np.asarray(occ, dtype=np.float64)))
    pick, cnt = np.zeros(max(len(n), 1), np.int32), C.c_int()
    if load().dfta_pseudo_default_valence(len(n), _ip(n), _ip(l), _ip(occ), len(pick), _ip(pick), C.byref(cnt)):
        raise DftaError("default_valence: invalid configuration")
    return pick[:cnt.value].copy()


def default_ic(grid, u, factor=1.5):
    """dfta_pseudo_default_ic: the core node of each orbital of u (nch, N): nearest to factor x the radius of the orbital's largest |u|,
    ORB_RPEAK, moved beyond the last node of u.  Host only."""
    u = _f64(u).reshape(-1, grid.N)
    ic = np.zeros(u.shape[0], np.int32)
    if load().dfta_pseudo_default_ic(grid.h, u.shape[0], _dp(u), float(factor), _ip(ic)):
        raise DftaError("default_ic: invalid arguments")
    return ic


def _kb_channels(grid, V, l, beta, q1, vidx):
    V = _f64(V).reshape(-1, grid.N)
    beta = _f64(beta).reshape(-1, grid.N)
    l, q1 = _i32(np.atleast_1d(l)), _f64(np.atleast_1d(q1))
    nch = beta.shape[0]
    if not (len(l) == len(q1) == nch):
        raise ValueError("kb: %d projectors, %d l, %d q1" % (nch, len(l), len(q1)))
    vidx = None if vidx is None else _i32(np.broadcast_to(vidx, (nch,)))
    return V, l, beta, q1, vidx, nch


def kb_sweep(ctx, grid, V, l, beta, q1, E, m=None, chan=None, vidx=None, want_rows=False):
    """dfta_kb_sweep: outward solves of (H_loc + |beta><beta| / q1 - E) u = 0.  V: (nV, N) local potentials; per channel l, a row of beta
    (nch, N), q1 and vidx (None: 0); per trial E, the end node m (None: N-2; at or beyond the last non-zero node of beta) and chan
    (None: 0).  Returns "u" and "du" (u~ and u~' at r_m), "logderiv", "Bh", "Bp", "D", "status" (CONT_NONFINITE, CONT_STEP) and, on
    request, "rows" (ntrials, N)."""
    V, l, beta, q1, vidx, nch = _kb_channels(grid, V, l, beta, q1, vidx)
    E = _f64(np.atleast_1d(E))
    nt = len(E)
    m = np.full(nt, grid.N - 2, np.int32) if m is None else _i32(np.broadcast_to(m, (nt,)))
    chan = None if chan is None else _i32(np.broadcast_to(chan, (nt,)))
    out = {k: np.zeros(nt) for k in ("u", "du", "logderiv", "Bh", "Bp", "D")}
    out["status"] = np.zeros(nt, np.int32)
    if want_rows:
        out["rows"] = np.zeros((nt, grid.N))
    ptr = lambda a, f: None if a is None else f(a)       # noqa: E731
    ctx.check(ctx.lib.dfta_kb_sweep(ctx.h, grid.h, V.shape[0], _dp(V), nch, ptr(vidx, _ip), _ip(l), _dp(beta), _dp(q1), nt, ptr(chan, _ip),
                                    _dp(E), _ip(m), _dp(out["u"]), _dp(out["du"]), _dp(out["logderiv"]), _dp(out["Bh"]), _dp(out["Bp"]),
                                    _dp(out["D"]), _ip(out["status"]), ptr(out.get("rows"), _dp)))
    return out


def kb_bound_states(ctx, grid, V, l, beta, q1, E_lo, E_hi, m=None, vidx=None, nscan=256):
    """dfta_kb_bound_states: the bound states of H_KB of every channel between E_lo and E_hi (per channel or one for all) in the box that
    ends at node m (None: N-2), by the sign of u~_m(E).  Returns "count", "energies" (nch, 8; NaN beyond count), "rounds", "status"
    (KB_SEARCH_* bits)."""
    V, l, beta, q1, vidx, nch = _kb_channels(grid, V, l, beta, q1, vidx)
    m = np.full(nch, grid.N - 2, np.int32) if m is None else _i32(np.broadcast_to(m, (nch,)))
    lo, hi = _f64(np.broadcast_to(E_lo, (nch,))), _f64(np.broadcast_to(E_hi, (nch,)))
    out = {"count": np.zeros(nch, np.int32), "energies": np.zeros((nch, KB_MAX_STATES)), "rounds": np.zeros(nch, np.int32),
           "status": np.zeros(nch, np.int32)}
    ctx.check(ctx.lib.dfta_kb_bound_states(ctx.h, grid.h, V.shape[0], _dp(V), nch, None if vidx is None else _ip(vidx), _ip(l), _dp(beta),
                                           _dp(q1), _ip(m), _dp(lo), _dp(hi), int(nscan), _ip(out["count"]), _dp(out["energies"]),
                                           _ip(out["rounds"]), _ip(out["status"])))
    return out


def kb_ghost_report(ctx, grid, ps, l=None, eps=None, atom=None, l_loc=None, m=None, E_lo=None, E_hi=0.0, nscan=512, tol=1e-5):
    """dfta_kb_ghost_report on the output `ps` of Scf.pseudopotentials(), or of pseudize() merged with pseudo_ionic() (then l, eps and
    atom per channel are given here; atom None: one atom).  l_loc as it was given to them.  Per channel (NaN for the local one):
    "eps_ref", "E_KB", "bound" (the states of H_KB in [E_lo, min(0, E_hi)] with the box at node m, None: N-2; E_lo None: per channel
    the bound below which H_KB has no state), "ghosts" (how many lie
    below eps_ref - tol), "e_loc" (nch, 2: the two lowest levels of the local potential at l), "gks" and "direct" (the two verdicts:
    1 ghost, 0 clean, -1 none), "status", "rounds"."""
    V, beta, kb = (_f64(ps[k]) for k in ("V_ps", "beta", "kb"))
    V, beta, kb = V.reshape(-1, grid.N), beta.reshape(-1, grid.N), kb.reshape(-1, 3)
    nch = V.shape[0]
    l = _i32(np.atleast_1d(ps["l"] if l is None else l))
    eps = _f64(np.atleast_1d(ps["eps"] if eps is None else eps))
    if atom is None:
        atom = ps["atom"] if "atom" in ps else np.zeros(nch, np.int32)
    seen = {}
    atom = _i32([seen.setdefault(int(a), len(seen)) for a in np.atleast_1d(atom)])      # numbered by first channel, as l_loc's rows
    natoms = int(atom.max()) + 1 if nch else 0
    ll = None if l_loc is None else _i32(np.broadcast_to(l_loc, (natoms,)))
    rep, st = np.zeros((nch, KB_REPORT)), np.zeros((nch, KB_MAX_STATES))
    ctx.check(ctx.lib.dfta_kb_ghost_report(ctx.h, grid.h, natoms, nch, _ip(atom), _ip(l), _dp(eps), _dp(V), _dp(beta), _dp(kb),
                                           None if ll is None else _ip(ll), int(grid.N - 2 if m is None else m), float("nan" if E_lo is None else E_lo),
                                           float(E_hi), int(nscan), float(tol), _dp(rep), _dp(st)))
    flag = lambda x: np.where(np.isnan(x), -1, np.nan_to_num(x)).astype(np.int32)      # noqa: E731
    return {"eps_ref": rep[:, 0], "E_KB": rep[:, 1], "bound": [row[~np.isnan(row)] for row in st], "ghosts": flag(rep[:, 3]),
            "e_loc": rep[:, 4:6], "gks": flag(rep[:, 6]), "direct": flag(rep[:, 7]), "status": flag(rep[:, 8]), "rounds": flag(rep[:, 9])}


class Mixer:
    """The SCF's density-mixing stage on its own (dfta_mixer): the launches dfta_scf_step issues for `mixing`, on the caller's arrays."""

    def __init__(self, ctx, grid, lsda=False, natoms=1, mixing=MIX_ANDERSON, history=4, warmup=3):
        self.ctx, self.grid, self.lsda, self.natoms, self.mixing, self.history = ctx, grid, bool(lsda), int(natoms), int(mixing), int(history)
        self.nspin = 2 if lsda else 1
        h = vp()
        ctx.check(ctx.lib.dfta_mixer_create(ctx.h, grid.h, int(self.lsda), self.natoms, self.mixing, self.history, int(warmup), C.byref(h)))
        self.h = h

    def step(self, alpha, acc, density, dA=None, dB=None, fin=None):
        """acc: Sum f Psi^2, (natoms, nspin, N); density, dA, dB: (natoms, N), the step's input; fin: (natoms,) frozen flags.
        Returns copies: (g as stored over acc, density, dA, dB) -- LDA: dA, dB are None."""
        n, N = self.natoms, self.grid.N
        acc = _f64(acc).reshape(n, self.nspin, N).copy()
        density = _f64(density).reshape(n, N).copy()
        fin = _i32(np.zeros(n) if fin is None else fin).reshape(n)
        if self.lsda:
            dA, dB = _f64(dA).reshape(n, N).copy(), _f64(dB).reshape(n, N).copy()
        self.ctx.check(self.ctx.lib.dfta_mixer_step(self.h, float(alpha), _dp(acc), _dp(density), _dp(dA) if self.lsda else None,
                                                    _dp(dB) if self.lsda else None, _ip(fin)))
        return acc, density, (dA if self.lsda else None), (dB if self.lsda else None)

    def get(self, atom):
        """MIX_ANDERSON: dict(state (8 ints), gamma (8), slab (chunks, 44), ring (nspin, history, 2, N)) of one atom after the last step"""
        N = self.grid.N
        state, gamma = np.zeros(8, np.int32), np.zeros(8)
        slab, ring = np.zeros(((N + 1023) // 1024, 44)), np.zeros((self.nspin, self.history, 2, N))
        self.ctx.check(self.ctx.lib.dfta_mixer_get(self.h, int(atom), _ip(state), _dp(gamma), _dp(slab), _dp(ring)))
        return {"state": state, "gamma": gamma, "slab": slab, "ring": ring}

    def close(self):
        if self.h:
            self.ctx.lib.dfta_mixer_destroy(self.h)
            self.h = None


class Scf:
    """Device-resident SCF state of a batch of atoms (dfta_scf): the body of CalculateNonUniformLDA/LSDA."""

    def __init__(self, ctx, grid, Z, lsda=False, alpha=0.5, levels_mode=LEVELS_BATCHED, tree_depth=0, integrator=INT_SIMPSON38,
                 functional=XC_VWN, aufbau=AUFBAU_REFERENCE, poisson_mode=POISSON_DEFAULT, sweep_mode=SWEEPS_EXACT, config=None,
                 charge=None, exchange=EXCHANGE_FUNCTIONAL, mixing=MIX_LINEAR, mix_history=0, mix_warmup=0):
        """mixing: MIX_LINEAR (the reference's) or MIX_ANDERSON (include/dftatom_hip.h: about half the steps); mix_history: pairs kept per
        atom (1 .. 8, 0: 4); mix_warmup: linear steps before the first accelerated one (0: 3).
        config: an electron configuration (parse_config's text, or its result) for every atom, or a list of them, one per atom;
        charge: an int for every atom, or a list of ints (ion_config: cations).  Neither: the Aufbau configuration of each Z.
        The nuclear charge stays Z; the electron count sets the start density and the Poisson boundary U(Rmax).
        exchange: EXCHANGE_KLI makes every step take its exchange potential from its own orbitals (exchange-only KLI, no correlation;
        functional XC_VWN and MIX_LINEAR only), EXCHANGE_SIC_KLI keeps VWN and adds the Perdew-Zunger self-interaction correction as
        one KLI potential per spin channel (-1/r tail, HOMO near -IP; the same two conditions): set_exchange() right after creation."""
        self.ctx, self.grid = ctx, grid
        self.Z = _i32(np.atleast_1d(Z))
        self.natoms = len(self.Z)
        self.lsda = bool(lsda)
        h = vp()
        opt = ScfOptions(C.sizeof(ScfOptions), integrator, functional, aufbau, poisson_mode, sweep_mode, int(mixing), int(mix_history),
                         int(mix_warmup))
        if config is not None and charge is not None:
            raise ValueError("give config or charge, not both")
        self.configs = None
        if config is not None or charge is not None:
            per = config if config is not None else charge
            if isinstance(per, (str, dict)) or np.ndim(per) == 0:
                per = [per] * self.natoms
            if len(per) != self.natoms:
                raise ValueError("%d configurations for %d atoms" % (len(per), self.natoms))
            cfgs = []
            for z, c in zip(self.Z, per):
                if isinstance(c, dict):
                    cfgs.append(c)
                elif config is not None:
                    cfgs.append(parse_config(int(z), c, self.lsda, aufbau))
                else:
                    cfgs.append(ion_config(int(z), int(c), self.lsda, aufbau))
            self.configs = cfgs
            nlev = _i32([[len(c["alpha"]), len(c["beta"])] for c in cfgs]).reshape(-1)
            flat = [lv for c in cfgs for lv in c["alpha"] + c["beta"]]
            n = _i32([lv[0] for lv in flat])
            l = _i32([lv[1] for lv in flat])
            occ = _f64([lv[2] for lv in flat])
            ctx.check(ctx.lib.dfta_scf_create_config(ctx.h, grid.h, int(self.lsda), self.natoms, _ip(self.Z), _ip(nlev), _ip(n), _ip(l),
                                                     _dp(occ), alpha, levels_mode, tree_depth, C.cast(C.byref(opt), vp), C.byref(h)))
        else:
            ctx.check(ctx.lib.dfta_scf_create_ex(ctx.h, grid.h, int(self.lsda), self.natoms, _ip(self.Z), alpha, levels_mode,
                                                 tree_depth, C.cast(C.byref(opt), vp), C.byref(h)))
        self.h = h
        self._exchange = EXCHANGE_FUNCTIONAL
        d, nj, tr = C.c_int(), C.c_int(), C.c_long()
        ctx.check(ctx.lib.dfta_scf_info(h, C.byref(d), C.byref(nj), C.byref(tr)))
        self.tree_depth, self.njobs, self.trials_per_round = d.value, nj.value, tr.value
        if exchange != EXCHANGE_FUNCTIONAL:
            try:
                self.set_exchange(exchange)
            except Exception:
                self.close()
                raise

    def step(self, want_stats=True):
        st = StepStats()
        st.struct_size = C.sizeof(StepStats)
        self.ctx.check(self.ctx.lib.dfta_scf_step(self.h, C.byref(st) if want_stats else None))
        return st

    def energies(self):
        e = (Energies * self.natoms)()
        fin = np.zeros(self.natoms, np.int32)
        self.ctx.check(self.ctx.lib.dfta_scf_get_energies(self.h, e, _ip(fin)))
        return [e[i] for i in range(self.natoms)], fin

    def levels(self, atom=0, spin=0):
        cnt = self.ctx.lib.dfta_scf_num_levels(self.h, atom, spin)
        n, l, occ, conv = (np.zeros(max(cnt, 1), np.int32) for _ in range(4))
        E, occupation = np.zeros(max(cnt, 1)), np.zeros(max(cnt, 1))
        if cnt > 0:
            self.ctx.check(self.ctx.lib.dfta_scf_get_occupations(self.h, atom, spin, _dp(occupation)))
            integral = bool(np.all(occupation[:cnt] == np.floor(occupation[:cnt])))
            self.ctx.check(self.ctx.lib.dfta_scf_get_levels(self.h, atom, spin, _ip(n), _ip(l), _ip(occ) if integral else None, _dp(E),
                                                            _ip(conv)))
            if not integral:
                occ = None              # a fractional occupation: the int getter has no value for it, see "occupation"
        status, nc, nz = (np.zeros(max(cnt, 1), np.int32) for _ in range(3))
        if cnt > 0:
            self.ctx.check(self.ctx.lib.dfta_scf_get_level_status(self.h, atom, spin, _ip(status), _ip(nc), _ip(nz)))
        return {"n": n[:cnt], "l": l[:cnt], "occ": None if occ is None else occ[:cnt], "occupation": occupation[:cnt], "E": E[:cnt],
                "converged": conv[:cnt], "status": status[:cnt], "n_count": nc[:cnt], "n_zero": nz[:cnt]}

    def array(self, which, atom=0):
        out = np.zeros(self.grid.N)
        self.ctx.check(self.ctx.lib.dfta_scf_get_array(self.h, atom, which, _dp(out)))
        return out

    def orbitals(self, atom=0, spin=0):
        """u = r R_nl of every level of (atom, spin), (nlev, N), in the order of levels(): the orbitals of the last step in which the atom
        was live -- eigenfunctions of that step's input potential (array(3 / 4) after the step is already the next one)."""
        cnt = self.ctx.lib.dfta_scf_num_levels(self.h, atom, spin)
        u = np.zeros((max(cnt, 0), self.grid.N))
        self.ctx.check(self.ctx.lib.dfta_scf_get_orbitals(self.h, int(atom), int(spin), _dp(u)))
        return u

    def orbital_jobs(self):
        """the rows of orbital_properties(): [(atom, spin, n, l), ...], atom-major, alpha then beta; n as levels() counts it"""
        rows = []
        for a in range(self.natoms):
            for spin in range(2 if self.lsda else 1):
                lv = self.levels(a, spin)
                rows += [(a, spin, int(n), int(l)) for n, l in zip(lv["n"], lv["l"])]
        return rows

    def orbital_properties(self):
        """(props, jobs): props (njobs, ORB_PROPS) of every orbital of the batch from one launch, jobs = orbital_jobs()"""
        props = np.zeros((self.njobs, ORB_PROPS))
        self.ctx.check(self.ctx.lib.dfta_scf_orbital_properties(self.h, _dp(props)))
        return props, self.orbital_jobs()

    def orbital_matrix(self, atom=0, spin=0, k=0):
        """M_ab = Q[u_a u_b r^k dr/di] over the levels of (atom, spin), k = 0 (overlap), 1 (dipole) or 2"""
        cnt = max(self.ctx.lib.dfta_scf_num_levels(self.h, atom, spin), 0)
        M = np.zeros((cnt, cnt))
        self.ctx.check(self.ctx.lib.dfta_scf_orbital_matrix(self.h, int(atom), int(spin), int(k), _dp(M)))
        return M

    def slater_rk(self, atom, jobs):
        """R^k(ab,cd) of the rows (a, b, c, d, k) of jobs over the orbitals of `atom`, read in place; indices count the atom's rows
        of orbital_jobs(): alpha levels, then beta levels (a cross-spin F^0 is a job like any other)"""
        jobs = _i32(jobs).reshape(-1, 5)
        R = np.zeros(len(jobs))
        self.ctx.check(self.ctx.lib.dfta_scf_slater_rk(self.h, int(atom), len(jobs), _ip(jobs), _dp(R)))
        return R

    def slater_fg(self, atom=0, spin=0):
        """(F, G), each (SLATER_KMAX + 1, nlev, nlev): F^k(a,b) and G^k(a,b) of the levels of (atom, spin) from one launch, symmetric
        bit for bit, G^k(a,a) = F^k(a,a), 0.0 where slater_fg_jobs has no job"""
        cnt = max(self.ctx.lib.dfta_scf_num_levels(self.h, atom, spin), 0)
        F, G = np.zeros((SLATER_KMAX + 1, cnt, cnt)), np.zeros((SLATER_KMAX + 1, cnt, cnt))
        self.ctx.check(self.ctx.lib.dfta_scf_slater_fg(self.h, int(atom), int(spin), _dp(F), _dp(G)))
        return F, G

    def coulomb_exchange(self, atom=0):
        """(E_H, E_x): the Hartree energy and the exact-exchange energy of the atom's orbitals and occupations (spherically averaged;
        include/dftatom_hip.h has the sums), from one launch"""
        eh, ex = C.c_double(), C.c_double()
        self.ctx.check(self.ctx.lib.dfta_scf_coulomb_exchange(self.h, int(atom), C.byref(eh), C.byref(ex)))
        return eh.value, ex.value

    def screening_yk(self, atom, jobs):
        """y^k_xy(r) of the rows (x, y, k) of jobs over the orbitals of `atom`, read in place: (njobs, N); indices count the atom's rows
        of orbital_jobs(): alpha levels, then beta levels"""
        jobs = _i32(jobs).reshape(-1, 3)
        y = np.zeros((len(jobs), self.grid.N))
        self.ctx.check(self.ctx.lib.dfta_scf_screening_yk(self.h, int(atom), len(jobs), _ip(jobs), _dp(y)))
        return y

    def exchange_potentials(self, atom=0, spin=0):
        """exchange_potentials() of the levels of (atom, spin), read in place: channel occupations N (LSDA) or N / 2 (LDA), the HOMO the
        occupied level of highest eigenvalue (the higher index on ties).  The dict also holds "occ", the channel occupations.
        None for a channel without levels."""
        cnt = max(self.ctx.lib.dfta_scf_num_levels(self.h, atom, spin), 0)
        out = _xp_outputs(cnt, self.grid.N)
        homo = C.c_int(-1)
        self.ctx.check(self.ctx.lib.dfta_scf_exchange_potentials(self.h, int(atom), int(spin), _dp(out["X"]), _dp(out["D"]), _dp(out["vS"]),
                                                                 _dp(out["vKLI"]), _dp(out["vbar"]), _dp(out["M"]), C.byref(homo)))
        if cnt == 0:
            return None
        out["homo"] = homo.value
        occ = self.levels(atom, spin)["occupation"]
        out["occ"] = occ if self.lsda else 0.5 * occ
        return out

    def form_factors(self, q):
        """(natoms, nchan, nq): f(q) = 4 pi Q[rho j_0(q r) r^2 dr/di] of every atom's densities as array(0 / 1 / 2) holds them now, read
        in place, one launch; nchan = 1 (LDA: rho) or 3 (LSDA: rho, rho_a, rho_b -- f_a - f_b is the magnetic form factor)"""
        q = _f64(np.atleast_1d(q))
        out = np.zeros((self.natoms, 3 if self.lsda else 1, len(q)))
        self.ctx.check(self.ctx.lib.dfta_scf_form_factors(self.h, len(q), _dp(q), _dp(out)))
        return out

    def momentum_orbitals(self, q):
        """(values, jobs): values (njobs, nq), the momentum-space radial functions sqrt(2/pi) Q[u_nl j_l(q r) r dr/di] of every orbital
        of the batch from one launch, jobs = orbital_jobs()"""
        q = _f64(np.atleast_1d(q))
        out = np.zeros((self.njobs, len(q)))
        self.ctx.check(self.ctx.lib.dfta_scf_momentum_orbitals(self.h, len(q), _dp(q), _dp(out)))
        return out, self.orbital_jobs()

    def _cont_norm(self, norm):
        """"auto": CONT_WKB when an atom of the batch is charged or the exchange switch is KLI / SIC-KLI (a -1/r tail), else CONT_FREE"""
        if norm != "auto":
            return int(norm)
        charged = self.configs is not None and any(config_electrons(c) != int(z) for c, z in zip(self.configs, self.Z))
        return CONT_WKB if charged or self._exchange != EXCHANGE_FUNCTIONAL else CONT_FREE

    def continuum(self, l, E, m=None, atom=0, spin=0, norm="auto", power=-1, want_rows=False):
        """dfta_scf_continuum: continuum() on the batch's resident potentials (array(3 / 4) as it is now), read in place; atom, spin per
        trial or one for all.  power >= 0: sums with the orbitals of the trial's channel -- l_b = l +- 1 for power 1 (dipole), l_b = l
        otherwise (power 0: overlaps) --, "partner_index" (ntrials, 16) naming the level of each column (-1: none).  The orbitals belong
        to the last step's input potential, the resident potential is the next step's."""
        l = _i32(np.atleast_1d(l))
        E = _f64(np.atleast_1d(E))
        nt = len(E)
        if len(l) != nt:
            raise ValueError("%d orders for %d energies" % (len(l), nt))
        m = np.full(nt, self.grid.N - 2, np.int32) if m is None else _i32(np.broadcast_to(m, (nt,)))
        atom, spin = _i32(np.broadcast_to(atom, (nt,))), _i32(np.broadcast_to(spin, (nt,)))
        out = _cont_outputs(nt, self.grid.N, power >= 0, want_rows)
        if power >= 0:
            out["partner_index"] = np.full((nt, CONT_MAX_PARTNERS), -1, np.int32)
        ptr = lambda a, f: None if a is None else f(a)       # noqa: E731
        self.ctx.check(self.ctx.lib.dfta_scf_continuum(self.h, self._cont_norm(norm), nt, _ip(atom), _ip(spin), _ip(l), _dp(E), _ip(m),
                                                       int(power), _dp(out["logderiv"]), _ip(out["nodes"]), _dp(out["delta"]),
                                                       _dp(out["scale"]), _ip(out["status"]), ptr(out.get("sums"), _dp),
                                                       ptr(out.get("partner_index"), _ip), ptr(out.get("rows"), _dp)))
        return out

    def pseudopotentials(self, atoms=None, levels=None, ic=None, factor=1.5, l_loc=None):
        """dfta_scf_pseudopotentials: Troullier-Martins pseudopotentials of valence levels, the resident orbitals and potentials read in
        place.  atoms: the atoms wanted (None: all); levels: per atom in `atoms` the level indices (None: default_valence of its levels);
        ic: a core node per channel (None: default_ic(factor)); l_loc: the local l per atom in `atoms` (None: the highest).  The
        potential is array(3) AS IT IS NOW (after a step: the next step's input; the orbitals belong to the last step's input).
        Returns "atom", "level", "l", "occ", "eps", "ic" per channel and the outputs of pseudize() and pseudo_ionic()."""
        atoms = list(range(self.natoms)) if atoms is None else [int(a) for a in np.atleast_1d(atoms)]
        at, lev, l, occ, eps = [], [], [], [], []
        for k, a in enumerate(atoms):
            if not 0 <= a < self.natoms:
                raise DftaError("pseudopotentials: atom %d outside 0 .. %d" % (a, self.natoms - 1))
            lv = self.levels(a, 0)
            keep = default_valence(lv["n"], lv["l"], lv["occupation"]) if levels is None else np.atleast_1d(levels[k])
            for j in keep:
                if not 0 <= j < len(lv["l"]):
                    raise DftaError("pseudopotentials: level %d of atom %d outside 0 .. %d" % (j, a, len(lv["l"]) - 1))
                at.append(a); lev.append(int(j)); l.append(int(lv["l"][j])); occ.append(float(lv["occupation"][j])); eps.append(float(lv["E"][j]))
        nch, N, na = len(at), self.grid.N, len(atoms)
        at, lev = _i32(at), _i32(lev)
        icv = None if ic is None else _i32(np.broadcast_to(ic, (nch,)))
        ll = None if l_loc is None else _i32(np.broadcast_to(l_loc, (na,)))
        out = {"atom": at, "level": lev, "l": _i32(l), "occ": _f64(occ), "eps": _f64(eps), "ic": np.zeros(nch, np.int32),
               "u_ps": np.zeros((nch, N)), "V_ps": np.zeros((nch, N)), "coef": np.zeros((nch, PS_COEF)), "rc": np.zeros(nch),
               "match": np.zeros((nch, PS_MATCH)), "iters": np.zeros(nch, np.int32), "status": np.zeros(nch, np.int32),
               "rho_v": np.zeros((na, N)), "vH": np.zeros((na, N)), "vxc": np.zeros((na, N)), "V_ion": np.zeros((nch, N)),
               "beta": np.zeros((nch, N)), "kb": np.zeros((nch, 3))}
        self.ctx.check(self.ctx.lib.dfta_scf_pseudopotentials(
            self.h, nch, _ip(at), _ip(lev), None if icv is None else _ip(icv), float(factor), None if ll is None else _ip(ll), _ip(out["ic"]),
            _dp(out["u_ps"]), _dp(out["V_ps"]), _dp(out["coef"]), _dp(out["rc"]), _dp(out["match"]), _ip(out["iters"]), _ip(out["status"]),
            _dp(out["rho_v"]), _dp(out["vH"]), _dp(out["vxc"]), _dp(out["V_ion"]), _dp(out["beta"]), _dp(out["kb"])))
        return out

    def kb_ghost_report(self, atoms=None, levels=None, ic=None, factor=1.5, l_loc=None, **search):
        """pseudopotentials(...) and then kb_ghost_report() on them (search: m, E_lo, E_hi, nscan, tol).  Returns (report, ps)."""
        ps = self.pseudopotentials(atoms, levels, ic, factor, l_loc)
        return kb_ghost_report(self.ctx, self.grid, ps, l_loc=l_loc, **search), ps

    def photoionization(self, eps, atom=0, norm="auto"):
        """dfta_scf_photoionization: {"omega", "sigma"} (subshells of the atom, neps) -- photon energies eps - E_nl (Ha) and cross
        sections (a_0^2) of every subshell at the photoelectron energies eps > 0 -- and "jobs", the subshells [(spin, n, l), ...]"""
        eps = _f64(np.atleast_1d(eps))
        jobs = [(sp, int(n), int(l)) for sp in range(2 if self.lsda else 1) for n, l in zip(*[self.levels(atom, sp)[k] for k in ("n", "l")])]
        om, sg = np.zeros((len(jobs), len(eps))), np.zeros((len(jobs), len(eps)))
        self.ctx.check(self.ctx.lib.dfta_scf_photoionization(self.h, int(atom), len(eps), _dp(eps), self._cont_norm(norm), _dp(om), _dp(sg)))
        return {"omega": om, "sigma": sg, "jobs": jobs}

    def set_integrator(self, rule):
        """INT_TRAPEZOID .. INT_ROMBERG: quadrature of the energy integrals and of the orbitals' normalisation."""
        self.ctx.check(self.ctx.lib.dfta_scf_set_integrator(self.h, int(rule)))

    def set_exchange(self, exchange):
        """EXCHANGE_FUNCTIONAL, EXCHANGE_KLI or EXCHANGE_SIC_KLI, before the first step (dfta_scf_set_exchange)."""
        self.ctx.check(self.ctx.lib.dfta_scf_set_exchange(self.h, int(exchange)))
        self._exchange = int(exchange)

    def exchange(self, atom=0, spin=0):
        """under EXCHANGE_KLI or EXCHANGE_SIC_KLI, after a step: {"vx", "v_raw"} (N each) of channel (atom, spin) and "Ex", the atom's
        exchange energy (EXCHANGE_SIC_KLI: E_SIC)"""
        vx, vr, ex = np.zeros(self.grid.N), np.zeros(self.grid.N), C.c_double()
        self.ctx.check(self.ctx.lib.dfta_scf_get_exchange(self.h, int(atom), int(spin), _dp(vx), _dp(vr), C.byref(ex)))
        return {"vx": vx, "v_raw": vr, "Ex": ex.value}

    def sic_table(self, atom=0, spin=0):
        """under EXCHANGE_SIC_KLI, after a step: per shell of channel (atom, spin) "EH", "EXC" (the self-Hartree and self-xc energy of one
        electron in the shell), "vbar" (<a| v_a^SIC |a>), "c" (the KLI constant), and "homo"; None for a channel without levels"""
        cnt = max(self.ctx.lib.dfta_scf_num_levels(self.h, atom, spin), 0)
        out = {k: np.zeros(max(cnt, 1)) for k in ("EH", "EXC", "vbar", "c")}
        homo = C.c_int(-1)
        self.ctx.check(self.ctx.lib.dfta_scf_sic_table(self.h, int(atom), int(spin), _dp(out["EH"]), _dp(out["EXC"]), _dp(out["vbar"]),
                                                       _dp(out["c"]), C.byref(homo)))
        if cnt == 0:
            return None
        out = {k: v[:cnt] for k, v in out.items()}
        out["homo"] = homo.value
        return out

    def exchange_ms(self):
        """HIP-event time of the last step's exchange stage, ms"""
        ms = C.c_float()
        self.ctx.check(self.ctx.lib.dfta_scf_exchange_ms(self.h, C.byref(ms)))
        return ms.value

    def poisson_info(self):
        g, d, a = C.c_int(), C.c_int(), C.c_int()
        self.ctx.check(self.ctx.lib.dfta_scf_poisson_info(self.h, C.byref(g), C.byref(d), C.byref(a)))
        return g.value, bool(d.value), a.value

    def records_into(self, device_ptr):
        self.ctx.check(self.ctx.lib.dfta_scf_get_records_dev(self.h, vp(device_ptr)))

    def close(self):
        if self.h:
            self.ctx.lib.dfta_scf_destroy(self.h)
            self.h = None
