"""GPU suite: the reference-shaped C++ layer (dftatom_amd/compat: DFT::Numerov, DFT::PoissonSolver, DFT::VWNExchCor,
DFT::Integral, DFT::AufbauPrinciple, DFT::DFTAtom) driven the way the reference's own orchestrator drives its classes,
checked against the oracle and against the README's published Argon run."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import _oracle as O      # noqa: E402  (checker only)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COMPAT = os.path.join(ROOT, "dftatom_amd", "compat")


def _run(exe, *args, timeout=600):
    path = os.path.join(COMPAT, exe)
    if not os.path.exists(path):
        subprocess.check_call(["make", "-C", COMPAT])
    return subprocess.run([path] + [str(a) for a in args], check=True, capture_output=True, text=True, timeout=timeout).stdout


def test_reference_shaped_classes_vs_oracle():
    out = _run("compat_check")
    o = O.oracle()
    L, d, R = 12, 2e-3, 25.0
    g = O.make_grid(L, d, R)
    rr = O.grid_r(g)
    m = re.search(r"grid N (\d+) Rp (\S+)", out)
    assert int(m.group(1)) == g.N and float(m.group(2)) == g.Rp
    V = O.coulomb_potential(g, 18)
    P = np.zeros(g.N)
    n = 0
    for m in re.finditer(r"numerov l (\d) E (\S+) count (-?\d+) u0 (\S+) mp (-?\d+) psisum (\S+)", out):
        l, E = int(m.group(1)), float(m.group(2))
        assert int(m.group(3)) == o.dfo_count_nodes(C.byref(g), O.dp(V), l, E, 3, None, None)      # node counts: exact
        assert float(m.group(4)) == o.dfo_solution_in_zero(C.byref(g), O.dp(V), l, E, None)         # u(0): bit-exact
        assert int(m.group(5)) == o.dfo_match(C.byref(g), O.dp(V), l, E, O.dp(P), None)
        assert float(m.group(6)) == float(np.sum(P)) or abs(float(m.group(6)) - np.sum(P)) <= 1e-12 * abs(np.sum(P))
        n += 1
    assert n == 24
    V10 = O.coulomb_potential(g, 10)
    assert int(re.search(r"reread count (\d+)", out).group(1)) == o.dfo_count_nodes(C.byref(g), O.dp(V10), 0, -20.0, 3, None, None)
    rho = 2.0 * np.exp(-2.0 * rr) / np.pi
    m = re.search(r"poisson vcycles (\d+) maxerr (\S+) usum (\S+)", out)
    p = o.dfo_poisson_create(L, d)
    U = np.zeros(g.N)
    o.dfo_solve_poisson_nonuniform(p, 2, R, O.dp(rho), O.dp(U))
    assert int(m.group(1)) == p.contents.n_vcycles
    assert abs(float(m.group(3)) - U.sum()) <= 1e-9 * abs(U.sum()) and float(m.group(2)) < 1e-6
    o.dfo_poisson_destroy(p)
    v, e = np.zeros(g.N), np.zeros(g.N)
    o.dfo_vwn_vexc(O.dp(rho), O.dp(v), g.N)
    o.dfo_vwn_eexcdif(O.dp(rho), O.dp(e), g.N)
    m = re.search(r"vwn vexc100 (\S+) eexc100 (\S+) lsda100 (\S+) va100 (\S+) mismatch_empty (\d)", out)
    assert abs(float(m.group(1)) - v[100]) <= 1e-12 * abs(v[100]) and abs(float(m.group(2)) - e[100]) <= 1e-12 * abs(e[100])
    assert m.group(5) == "1"                                   # size mismatch -> {} as in the reference (VWNExcCor.h:137)
    integrand = 4 * np.pi * rr ** 2 * rho * (g.Rp * d * np.exp(d * np.arange(g.N)))
    m = re.search(r"integral simpson38 (\S+) romberg (\S+)", out)
    assert abs(float(m.group(1)) - 2.0) < 1e-6 and abs(float(m.group(1)) - o.dfo_simpson38(1.0, O.dp(integrand), g.N)) < 1e-13
    assert "aufbau Rn 15 first 1s2 last 6p6" in out


def _run_env(exe, args, env):
    path = os.path.join(COMPAT, exe)
    if not os.path.exists(path):
        subprocess.check_call(["make", "-C", COMPAT])
    return subprocess.run([path] + [str(a) for a in args], check=True, capture_output=True, text=True, timeout=900, env=dict(os.environ, **env)).stdout


def test_per_call_level_search_is_served_from_what_was_integrated_ahead():
    """The reference's own orchestration asks for ONE trial energy per call (LocateInterval + the u(0) bisection: ~150 calls per level).  The
    compat layer mirrors that loop from the calls it sees (compat/call_stream.h) and integrates the tree of the caller's possible next
    energies in the launch it has to make anyway: the calls that follow are answered from the cache.  Same kernels, same potential,
    bit-identical energies -- so every eigenvalue equals the one-trial-per-call run's and the oracle's; only the number of launches changes
    (Rn @ 131 073 nodes on the reference's unmodified DFTAtom.cpp: 6.6 -> 0.76 s per SCF step; the CPU reference: 3.9 s)."""
    args = (18, 12, 0.002, 25, 5)
    spec = _run_env("percall_levels", args, {})
    plain = _run_env("percall_levels", args, {"DFTA_COMPAT_NOSPECULATE": "1"})
    lev = lambda out: [ln for ln in out.splitlines() if ln.startswith("level")]
    assert lev(spec) == lev(plain) and len(lev(spec)) == 5
    calls, launches, hits = (int(x) for x in re.search(r"calls (\d+) launches (\d+) hits (\d+)", spec).groups())
    pc, pl, ph = (int(x) for x in re.search(r"calls (\d+) launches (\d+) hits (\d+)", plain).groups())
    assert pc == calls and pl == 0 and ph == 0                    # the counters belong to the speculation path
    assert launches + hits == calls and calls > 600
    assert launches <= 0.12 * calls, (calls, launches)            # ~12 decisions per launch (4 095 trials), a few single trials while BottomEnergy is inferred
    # ... and the oracle's LoopOverLevels on the same potential gives the same eigenvalues (chained brackets: level k starts from E_{k-1} - 3)
    o = O.oracle()
    g = O.make_grid(12, 2e-3, 25.0)
    V = O.coulomb_potential(g, 18)
    lv = O.levels_array(O.subshells(18)[:5])
    dens = np.zeros(g.N)
    eel, bottom = C.c_double(0), C.c_double(-18.0 * 18.0 - 1.0)
    o.dfo_loop_over_levels(C.byref(g), O.dp(V), lv, 5, O.dp(dens), C.byref(eel), C.byref(bottom), 1, None)
    for k, ln in enumerate(lev(spec)):
        m = re.match(r"level n (\d+) l (\d+) nodes (\d+) E (\S+) top (\S+) converged (\d)", ln)
        assert (int(m.group(1)), int(m.group(2))) == (lv[k].n + 1, lv[k].l)
        assert float(m.group(4)) == lv[k].E, (k, m.group(4), lv[k].E)           # bit-exact


def test_headless_front_end_reproduces_readme_argon():
    """BASELINE.json config 1 on the device path: Ar, 14 levels, delta 5e-4, mixing 0.5, Rmax 25 (README.md:76), to
    convergence, console text in the reference's format; final values equal the README's to its six decimals."""
    out = _run("dftatom_cli", 18, 14, 0.5, 25, 0.0005, 0)
    assert out.startswith("Computing atom with Z=18 using LSD with non-uniform grid")
    assert "Finished!" in out
    lines = out.strip().splitlines()
    assert lines[-1].strip() == "1s2 2s2 2p6 3s2 3p6"
    last_levels = [ln for ln in lines if ln.startswith("Energy")][-5:]
    got = [float(re.search(r": (\S+) Num", ln).group(1)) for ln in last_levels]
    assert got == [-113.800134, -10.794172, -8.443439, -0.883384, -0.382330]                       # README.md:63-67
    assert [ln.split("Num nodes: ")[1] for ln in last_levels] == ["0", "1", "0", "2", "1"]
    et = [ln for ln in lines if ln.startswith("Etotal")][-1]
    vals = [float(x) for x in re.findall(r"= (-?\d+\.\d+)", et)]
    want = [-525.946200, 524.969813, 231.458124, -1253.131983, -29.242154]                          # README.md:68
    assert all(abs(a - b) <= 1.5e-6 for a, b in zip(vals, want)), (vals, want)
    nsteps = sum(1 for ln in lines if ln.startswith("Step:"))
    assert 25 <= nsteps <= 60          # the stop step itself is round-off noise (README: 32, compiled reference here: 35)


@pytest.mark.gpu
def test_bench_two_ranks_control_flow():
    """bench.py under torch.distributed.run with two ranks, as the driver launches it for N > 1 -- on this one-GPU box both
    ranks share device 0 and the collectives run over gloo (DFTA_BENCH_SHARED_GPU=1): the barriers, the max-over-ranks time,
    the summed work and rank 0's single JSON line are exercised, the number itself means nothing."""
    import json
    import socket
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = dict(os.environ, DFTA_BENCH_SHARED_GPU="1")
    out = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
                          "--master-port", str(port), os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1", "--full", "--pt-zmax", "7"],
                         env=env, capture_output=True, text=True, timeout=600, cwd=root)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["ranks_seen"] == 2 and d["steps"] == 2 and d["scaling"] == "weak" and d["value"] > 0
    assert d["config"]["parallelism"] == "replicas x2" and "cpu_baseline" not in d and "roofline" in d
    # BASELINE config 4 under --gpus N: after the replica timing every rank advances its shard of the periodic table
    # (here Z = 1..7: partition_atoms over two ranks), the records are gathered once, rank 0 reports the sweep on the line
    pt = d["extra"]["periodic_table"]
    assert pt["atoms"] == 7 and sum(pt["atoms_per_rank"]) == 7 and len(pt["shard_seconds"]) == 2 and pt["seconds"] >= max(pt["shard_seconds"]) > 0
    assert pt["finished"] == 7 and pt["slowest_rank"] in (0, 1)


@pytest.mark.gpu
def test_bench_gpus_flag_starts_the_ranks_itself():
    """`python bench.py --gpus 2` with no launcher around it (the form the driver uses for N = 1) must start two ranks itself
    and print one line with n_gpus = 2 (here both on device 0 over gloo: DFTA_BENCH_SHARED_GPU=1); without the shared-GPU test
    mode it must refuse with a non-zero exit code when the box has fewer devices than ranks asked for."""
    import json
    import subprocess
    import sys
    import torch
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    out = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1", "--no-periodic-table"],
                         env=dict(env, DFTA_BENCH_SHARED_GPU="1"), capture_output=True, text=True, timeout=600, cwd=root)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["config"]["parallelism"] == "replicas x2" and d["value"] > 0
    if torch.cuda.device_count() < 2:
        bad = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "0"],
                             env=env, capture_output=True, text=True, timeout=600, cwd=root)
        assert bad.returncode != 0 and "only" in bad.stderr and not [ln for ln in bad.stdout.splitlines() if ln.startswith("{")]


@pytest.mark.gpu
def test_bench_plain_run_times_the_steps_and_dumps_the_last_one(tmp_path):
    """`bench.py --steps K --warmup W` without --full: the headline line alone (no extras, no CPU baseline), K timed steps, and with
    --dump-outputs the arrays of the last timed step as float64 .npy files within 64 MB -- here a 24-atom batch whose radial arrays
    (3 MB per atom) pass the limit, so a seeded sample of atoms is written"""
    import json
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    dump = tmp_path / "out"
    out = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--atoms", "24",
                          "--dump-outputs", str(dump)], capture_output=True, text=True, timeout=600, cwd=root)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["steps"] == 2 and d["warmup"] == 1 and d["ms_per_step"] > 0 and d["value"] > 0 and d["dtype"] == "f64"
    assert d["unit"] == "sweeps/s" and d["higher_is_better"] is True and "extra" not in d and "cpu_baseline" not in d
    files = {p.stem: np.load(p) for p in dump.glob("*.npy")}
    assert sum(p.stat().st_size for p in dump.glob("*.npy")) <= 64 << 20
    assert all(a.dtype == np.float64 for a in files.values())
    assert files["energies"].shape == (24, 9) and files["energies"][0, 0] == d["etotal_last_step"]
    assert files["records"].shape == (24, 64) and files["eigenvalues"].shape == (24, 1, 15) and files["finished"].shape == (24,)
    picked = files["radial_atoms"]
    assert 1 <= len(picked) < 24 and np.all(np.diff(picked) > 0) and "radial_points" not in files
    for name in ("density", "potential", "hartree_U"):
        assert files[name].shape == (len(picked), 131073) and np.all(np.isfinite(files[name]))


@pytest.mark.gpu
def test_periodic_table_two_ranks_equal_one_rank(tmp_path):
    """examples/periodic_table.py (BASELINE config 4) for Z = 1..8 at 16385 nodes: two ranks (sharing device 0 on this box,
    records gathered over gloo) must return, atom for atom, the bits of the single-process run -- shards do not interact."""
    import json
    import socket
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    script = os.path.join(root, "examples", "periodic_table.py")
    one, two = str(tmp_path / "one.json"), str(tmp_path / "two.json")
    common = ["--zmin", "1", "--zmax", "8", "--levels", "14"]
    r1 = subprocess.run([sys.executable, script, *common, "--out", one], capture_output=True, text=True, timeout=600, cwd=root)
    assert r1.returncode == 0, r1.stderr[-2000:]
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = dict(os.environ, DFTA_BENCH_SHARED_GPU="1")
    r2 = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
                         "--master-port", str(port), script, *common, "--out", two], env=env, capture_output=True, text=True, timeout=600, cwd=root)
    assert r2.returncode == 0, r2.stderr[-2000:]
    a, b = json.load(open(one)), json.load(open(two))
    assert b["n_gpus"] == 2 and len(a["atoms"]) == len(b["atoms"]) == 8
    for x, y in zip(a["atoms"], b["atoms"]):
        assert x == y, (x, y)
    assert all(x["finished"] for x in a["atoms"])


def test_graft_entry_smoke_runs():
    """the driver's smoke(): one small invocation of the hot path on cuda:0 through the C ABI, checked against the oracle"""
    import importlib.util
    spec = importlib.util.spec_from_file_location("graft_entry", os.path.join(ROOT, "__graft_entry__.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mod.smoke()


@pytest.mark.gpu
def test_resident_potential_equals_per_call_upload():
    """dfta_potential (what DFT::Numerov now holds): the potential and its slot tables stay on the device between calls.  Exact mode: counts,
    trips, u(0), Psi and match points bit for bit what dfta_numerov_sweeps / _match return with an upload per call -- also after the caller
    has changed the values (dfta_potential_update: host memcmp, re-upload only then).  Tolerance mode: the scan sweeps' counts."""
    import dftatom_amd as D
    from golden.make_golden import GRIDS, screened_potential
    ctx = D.Context(0)
    L, d, R = GRIDS["L14"]
    grid = D.Grid(ctx, L, d, R)
    V = screened_potential(grid.r(), 86.0)
    P = D.Potential(ctx, grid, V)
    rng = np.random.default_rng(11)
    for nt in (1, 5, 130):
        l = rng.integers(0, 4, nt).astype(np.int32)
        E = -10.0 ** rng.uniform(-2, 3.7, nt)
        lim = rng.integers(0, 5, nt).astype(np.int32)
        a = D.numerov_sweeps(ctx, grid, D.SWEEP_COUNT, V, l, E, lim)
        b = P.sweeps(D.SWEEP_COUNT, l, E, lim)
        c = P.sweeps(D.SWEEP_COUNT, l, E, lim, D.SWEEPS_TOLERANCE)
        assert np.array_equal(a["count"], b["count"]) and np.array_equal(a["trip"], b["trip"]) and np.array_equal(a["start"], b["start"])
        assert np.array_equal(a["count"], c["count"]) and np.array_equal(a["start"], c["start"])
        za, zb = D.numerov_sweeps(ctx, grid, D.SWEEP_ZERO, V, l, E), P.sweeps(D.SWEEP_ZERO, l, E)
        assert np.array_equal(za["u0"], zb["u0"], equal_nan=True)
    pa, ma = D.numerov_match(ctx, grid, V, [0, 2, 3], [-100.0, -3.0, -0.5])
    pb, mb = P.match([0, 2, 3], [-100.0, -3.0, -0.5])
    assert np.array_equal(pa, pb) and np.array_equal(ma, mb)
    V2 = V * (1.0 + 1e-7)
    P.update(V)                                               # unchanged values: nothing is copied
    P.update(V2)
    assert np.array_equal(D.numerov_sweeps(ctx, grid, D.SWEEP_ZERO, V2, [0, 1], [-100.0, -7.0])["u0"], P.sweeps(D.SWEEP_ZERO, [0, 1], [-100.0, -7.0])["u0"])
    assert np.array_equal(D.numerov_sweeps(ctx, grid, D.SWEEP_COUNT, V2, [0], [-100.0], [3])["count"], P.sweeps(D.SWEEP_COUNT, [0], [-100.0], [3], D.SWEEPS_TOLERANCE)["count"])
    P.close()
    grid.close()
    ctx.close()
