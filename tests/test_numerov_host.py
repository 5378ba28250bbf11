"""CPU suite: the pure host logic of the Numerov layer (dftatom_amd/csrc/numerov_host.cpp), run as a stand-alone program under
AddressSanitizer + UndefinedBehaviorSanitizer (`make -C oracle numerov_host`: oracle/numerov_host_main.cpp, linked with the oracle;
nothing is loaded into Python).  The driver holds the checks -- its header lists them -- and prints one line per violation:

boundary   host_boundary on the logarithmic grids (4097, 2e-3, 25) and (16385, 5e-4, 25), 200 energies from -4000 to -1e-4 in geometric
           steps: the cut-off index of dfo_max_radius_index, start values bit for bit dfo_far's; host_boundary_uniform: the start
           index dfo_ucount_nodes reports on a 4097-node grid.  Energies for which the oracle alone has no value are dropped first;
           at least 150 must remain.
grouping   make_grouping for 1, 63, 64, 65, 129, 257 trials, one and three potentials, with and without vidx: a stable permutation,
           blocks of 1..64 trials of one slot that tile the trials, trial_slot in agreement, no more blocks than trials, bad l / vidx
           refused; the ready-made-groups entry against the loop it replaced (offsets 0, 1, 65, 65, 200: one group is empty).
staging    stage_layout for 1..300 trials and both calls: no overlap, aligned, inside the block, blocks within 64 bytes per trial.
persist    plan_persist for 2, 37, 64, 256 workgroups, every level count, equal and generated shares: disjoint contiguous workgroup
           lists, shares within bounds, the pool their complement, one plan mailbox per level -- and equal to what the loop it
           replaced writes, invalid cases included.
Every run must leave the sanitizers' report stream empty.
"""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def driver():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "oracle"), "numerov_host"], stdout=subprocess.DEVNULL)
    exe = os.path.join(ROOT, "oracle", "_build", "numerov_host_main")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")

    def run(mode):
        r = subprocess.run([exe, mode], capture_output=True, text=True, timeout=300, env=env)
        assert r.stderr == "", r.stderr[-4000:]
        assert "VIOLATION" not in r.stdout, "\n".join(ln for ln in r.stdout.splitlines() if ln.startswith("VIOLATION"))[:4000]
        assert r.returncode == 0 and r.stdout.splitlines()[-1] == "0 violations", r.stdout[-2000:]
        return r.stdout.splitlines()
    return run


def test_boundary_values_are_the_oracles(driver):
    out = driver("boundary")
    kept = {ln.rsplit(":", 1)[0]: int(ln.rsplit(":", 1)[1].split()[0]) for ln in out if ln.startswith("boundary ")}
    assert set(kept) == {"boundary log N=4097", "boundary log N=16385", "boundary uniform N=4097"}
    assert all(150 <= n <= 200 for n in kept.values()), kept


def test_grouping_properties(driver):
    assert "grouping: 24 cases" in driver("grouping")


def test_staging_layout_properties(driver):
    assert "staging: 600 layouts" in driver("staging")


def test_persist_plan_equals_the_replaced_loop(driver):
    assert "persist: %d plans" % (2 * (2 + 37 + 64 + 256)) in driver("persist")
