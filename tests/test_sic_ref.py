"""The CPU reference of the self-interaction-corrected LSDA step (tests/_sic_ref.py: Perdew-Zunger SIC through KLI) against exact limits,
its own recorded figures and its float64 / longdouble evaluations, plan_channels_sic of dftatom_amd/csrc/kli_plan.cpp against its Python
statement, and the header and bindings of the feature.  No GPU."""
import os
import re

import numpy as np
import pytest

import _exchange_ref as X
import _kli_scf_ref as K
import _orb_ref as OR
import _sic_ref as R
import _slater_ref as S
import dftatom_amd as D

LD = np.longdouble
HERE = os.path.dirname(os.path.abspath(__file__))
CAP = 60
_runs = {}


def converged(name):
    """the reference run to its stop test (at most CAP steps), once per session"""
    if name not in _runs:
        r = R.make(name)
        r.run(CAP)
        _runs[name] = r
    return _runs[name]


def within(measured, want):
    """a MEASURED figure stands: the value lies in [want / 1.2, 1.2 want]"""
    return want / 1.2 <= measured <= 1.2 * want


# ---- convergence and the recorded figures ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(R.ATOMS))
def test_finishes_on_the_recorded_energy(name):
    """every atom meets the unchanged stop test within 60 steps -- Fe (LSDA, Aufbau), which exchange-only KLI cannot converge, included --
    in the recorded number of steps and on the recorded energies (1e-9 relative: what the GPU suite is compared with); Exc holds E_SIC"""
    r = converged(name)
    steps, E, Esic = R.MEASURED["E"][name]
    print("%s: %d steps, E = %.10f, E_SIC = %.10f" % (name, r.steps, r.en["Etotal"], r.Ex))
    assert r.finished, "%s: not finished after %d steps, E = %.9f" % (name, r.steps, r.en["Etotal"])
    assert r.steps == steps
    assert abs(r.en["Etotal"] - E) <= 1e-9 * abs(E) and abs(r.Ex - Esic) <= 1e-9 * abs(Esic) + 5e-11
    assert r.Ex < 0 and r.en["Etotal"] < 0


def test_hydrogen_is_free_of_self_interaction():
    """H (LSDA): E = -0.5 Ha and eps = -0.5 Ha to the grid's accuracy (plain VWN: -0.479 and -0.269); the distances are the MEASURED figures
    the GPU test leans on.  Half an electron: no longer -0.5 n, SIC is not linear in the occupation"""
    r = converged("H")
    dE, de = abs(r.en["Etotal"] + 0.5), abs(r.E[0][0] + 0.5)
    print("H: |E + 0.5| = %.3e, |eps + 0.5| = %.3e" % (dE, de))
    assert within(dE, R.MEASURED["H_E"]) and within(de, R.MEASURED["H_eps"])
    assert dE < 1e-6 and de < 1e-6
    half = converged("H05")
    assert half.finished and -0.31 < half.en["Etotal"] < -0.30


def test_hydrogen_orbital_terms_cancel_hartree_and_xc():
    """converged H: y0 of the orbital against U / r of the Poisson solve, v_a of the orbital density against v_up[rho_alpha, 0] of the mixed
    density -- equal to what the grid (second-order multigrid) and the mixing history allow; MEASURED"""
    r = converged("H")
    st = r.stage[0]
    y0 = np.asarray(st["y0"][0], dtype=np.float64)
    dh = float(np.max(np.abs(y0[1:] - r.U[1:] / r.pos[1:])) / np.max(np.abs(y0)))
    _, va, _, _ = r.xc(r.density, r.dA, r.dB)
    dx = float(np.max(np.abs(st["vorb"][0] - va)) / np.max(np.abs(va)))
    print("H: Hartree cancellation %.3e, xc cancellation %.3e" % (dh, dx))
    assert within(dh, R.MEASURED["H_cancel"]["hartree"]) and within(dx, R.MEASURED["H_cancel"]["xc"])


@pytest.mark.parametrize("name", list(R.MEASURED["eps"]))
def test_homo_eigenvalues(name):
    r = converged(name)
    homo = max(e for sp in range(2 if r.lsda else 1) for e, (_, _, f) in zip(r.E[sp], r.cfg[sp]) if f > 0)
    print("%s: HOMO %.6f" % (name, homo))
    assert abs(homo - R.MEASURED["eps"][name]) < 2e-6


@pytest.mark.parametrize("name", list(R.MEASURED["tail"]))
def test_potential_has_the_coulomb_tail(name):
    """r vx at the last node: -1 up to the mixing history, per channel; MEASURED (round-off where the channel has one shell)"""
    r = converged(name)
    for sp, want in enumerate(R.MEASURED["tail"][name]):
        t = abs(1 + float(r.pos[-1] * r.vx[sp][-1]))
        print("%s channel %d: |1 + r vx| = %.3e" % (name, sp, t))
        assert t < 1e-2
        assert t <= 1e-13 if want is None else within(t, want), (name, sp, t)


# ---- the stage ---------------------------------------------------------------------------------------------------------------------------
def test_sensitivity_longdouble_against_float64():
    """the stage in np.longdouble against float64 on the same orbitals (Ne after three steps); round-off, held to 2 x MEASURED"""
    r = R.make("Ne")
    for _ in range(3):
        r.step()
    a, b = r.exchange(0, dtype=np.float64), r.exchange(0, dtype=LD)
    dv = float(np.max(np.abs(b["v_raw"] - a["v_raw"])) / np.max(np.abs(a["v_raw"])))
    dx = float(abs(b["Esic"] - a["Esic"]) / abs(a["Esic"]))
    r.close()
    print("sensitivity: v_raw %.3e, E_SIC %.3e" % (dv, dx))
    assert R.MEASURED["sens"]["v_raw"] / 10 <= dv <= 2 * R.MEASURED["sens"]["v_raw"]
    assert dx <= 2 * R.MEASURED["sens"]["Esic"]


def hydrogenic():
    r, s = OR.grid(*R.GRID)
    return r.astype(np.float64), s.astype(np.float64), S.orbitals(r).astype(np.float64)


def test_one_shell_and_zero_orbital():
    """a channel of one shell: c = 0 and vKLI = vS = -(y0 + v_a) bit for bit where D > 0; an all-zero orbital: X, v_a, eps and the energies
    are exactly 0"""
    r, s, U = hydrogenic()
    o = K.O.oracle()
    for n in (1.0, 0.5):
        st = R.sic_stage(o, U[:1], [0], [n], [-50.0], r, s)
        ok = st["D"] > 0
        assert st["homo"] == 0 and len(st["c"]) == 1 and st["c"][0] == 0
        assert np.array_equal(st["vKLI"], st["vS"])
        want = -(st["y0"][0] + st["vorb"][0])[ok]            # one shell: the average of one potential is that potential
        assert np.max(np.abs(st["vS"][ok] - want)) <= 4 * OR.EPS * np.max(np.abs(want))
        assert st["Esic"] == -(n * (st["EH"][0] + st["EXC"][0])) and st["EH"][0] > 0 > st["EXC"][0]
    z = R.sic_stage(o, np.zeros((1, len(r))), [0], [1.], [-1.], r, s)
    assert not np.any(z["X"]) and not np.any(z["vorb"]) and not np.any(z["eps"]) and not np.any(z["v_raw"])
    assert z["EH"][0] == 0 and z["EXC"][0] == 0 and z["Esic"] == 0


def test_stage_functions():
    rng = np.random.default_rng(7)
    r = np.linspace(0., 3., 10)
    u = rng.standard_normal(10)
    rho = R.orbital_density(u, r)
    assert rho[0] == 0 and np.array_equal(rho[1:], (u[1:] * u[1:]) / ((R.FOURPI * r[1:]) * r[1:]))
    a, b = rng.standard_normal(10), rng.standard_normal(10)
    dA, dB = np.abs(rng.standard_normal(10)), np.abs(rng.standard_normal(10))
    dA[0] = dB[0] = 0
    V, va, vb, e = (rng.standard_normal(10) for _ in range(4))
    V2, va2, vb2, e2 = R.assemble_sic(True, V, va, vb, e, a, b, dA, dB, dA + dB)
    t = np.zeros(10)
    t[1:] = (dA[1:] * a[1:] + dB[1:] * b[1:]) / (dA + dB)[1:]
    assert np.array_equal(V2, V + t) and np.array_equal(e2, e - t) and np.array_equal(va2, va + a) and np.array_equal(vb2, vb + b)
    V2, _, _, e2 = R.assemble_sic(False, V, va, vb, e, a)
    assert np.array_equal(V2, V + a) and np.array_equal(e2, e - a)
    assert R.esic_channel([1., 3.], [2., 1.], [-0.5, -0.25]) == -((0. + 1. * (2. + -0.5)) + 3. * (1. + -0.25))
    assert R.esic_atom(False, [-2.5]) == -5.0 and R.esic_atom(True, [-2.5, -1.0]) == -3.5


# ---- kli_plan.cpp: plan_channels_sic -----------------------------------------------------------------------------------------------------
def test_sic_plan_standalone(tmp_path):
    """plan_channels_sic is pure host code: a stand-alone program (tests/sic_plan_main.cpp) built with ASan + UBSan makes the tables of four
    channels, checks the part the solve reads against plan_channels entry for entry, tries the refusals and plans chunks; what it prints
    equals the Python statement"""
    import shutil
    import subprocess
    csrc = os.path.join(HERE, "..", "dftatom_amd", "csrc")
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler is needed"
    exe = str(tmp_path / "sic_plan_main")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", csrc, "-o", exe,
                    os.path.join(HERE, "sic_plan_main.cpp"), os.path.join(csrc, "kli_plan.cpp"), os.path.join(csrc, "exchange_plan.cpp"),
                    os.path.join(csrc, "slater_plan.cpp")], check=True, timeout=300)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, (run.stdout, run.stderr)
    lines = {ln.split()[0]: ln.split()[1:] for ln in run.stdout.strip().split("\n")}
    norb = [3, 0, 5, 1]
    chans, jobs, red = R.plan_channels_sic(norb, atom=[0, 0, 1, 2])
    assert lines["channels"] == [":".join(str(x) for x in c) for c in chans]
    assert lines["jobs"] == ["%d:%d:%d" % j for j in jobs]
    assert lines["red"] == ["%d:%d:%d:%d" % q for q in red]
    assert len(jobs) == 9 and [c[8] for c in chans] == [18, 0, 35, 5]
    nj = [c[3] for c in chans]
    fmt = lambda ch: ["%d:%d" % c for c in ch]                                   # noqa: E731
    assert lines["all"] == fmt(K.plan_chunks(nj, None, 1000)) == ["0:4"]
    assert lines["each"] == fmt(K.plan_chunks(nj, None, 0)) == ["0:1", "1:3", "3:4"]
    assert lines["two"] == fmt(K.plan_chunks(nj, None, nj[0] + nj[2])) == ["0:3", "3:4"]
    assert lines["frozen"] == fmt(K.plan_chunks(nj, [1, 1, 0, 1], 1000)) == ["0:2", "3:4"]
    assert lines["none"] == []
    assert lines["caps"] == ["%d:%d:%d" % K.capacities(nj, norb, 0), "%d:%d:%d" % K.capacities(nj, norb, 1000)]


def test_row_counts_of_the_periodic_table():
    """Z = 1 .. 86, LDA: 814 y rows for the SIC stage against 6837 for exchange-only KLI"""
    sic = kli = 0
    for Z in range(1, 87):
        a, _ = K.aufbau_config(Z, False)
        l = [x for _, x, _ in a]
        sic += len(l)
        kli += len(X.y_jobs(l))
    assert (sic, kli) == (814, 6837)


# ---- header and binding ------------------------------------------------------------------------------------------------------------------
NEW = ("dfta_sic_channels", "dfta_scf_sic_table")


def test_header_and_binding():
    text = open(os.path.join(HERE, "..", "include", "dftatom_hip.h")).read()
    for name in NEW:
        assert re.search(r"\b%s\(" % name, text) and name in D.SIGNATURES
    assert re.search(r"#define DFTA_EXCHANGE_SIC_KLI\s+2\b", text) and D.EXCHANGE_SIC_KLI == 2
    assert (D.EXCHANGE_FUNCTIONAL, D.EXCHANGE_KLI) == (0, 1)
    assert callable(D.Scf.sic_table) and callable(D.sic_channels)
    lib = D.load()
    assert lib.dfta_abi_version() == D.ABI_VERSION          # entries were added, no struct grew
    cli = open(os.path.join(HERE, "..", "dftatom_amd", "compat", "dftatom_cli.cpp")).read()
    assert "--exchange=sic" in cli and "--sic-table" in cli
