"""CPU suite: the pure host logic of the SCF layer (dftatom_amd/csrc/scf_config.cpp), run as a stand-alone program under
AddressSanitizer + UndefinedBehaviorSanitizer (`make -C oracle scf_config`: oracle/scf_config_main.cpp; nothing is loaded into
Python).  The driver holds the checks -- it carries the loop the planner replaced (config_channel + scf_configure of scf.hip), verbatim, as
its reference -- and prints one line per violation:

plan       plan_scf_config against the replaced loop -- job specs, job offsets, levels per spin, bracket bottoms, nE, in LSDA the electrons
           per spin, all bit for bit: the Aufbau configuration of Z = 1..118, LDA and LSDA, both Aufbau options, each atom alone (472) and
           all 118 as one batch (4); the explicit configurations of dfta_ion_config(Z, q) for q = 0..3 < Z (4 x 466), the q = 0 plan equal
           to the Aufbau plan; '[Ne] 3s2 3p5.5' for Z = 18 and '[He] 2s2 2p2/1' for Z = 7 in LSDA.  2342 cases.
refusals   refused by both, with a text: Z = 0 and 119 (Aufbau and explicit), 0 + 0 levels, 33 levels, beta levels in LDA, l = -1, l = 4,
           n < l, a level twice, occupations 0, -1, NaN, above 2 (2l + 1) in LDA and above 2l + 1 in a spin channel, Z + 1 electrons;
           Z + 1e-10 electrons accepted by both; unsorted levels come out sorted by (n, l); a batch whose third atom is invalid is refused
           with "atom 2: " in the text.
options    resolve_scf_options: struct_size 8, 12, ... sizeof, sizeof + 4 and 4096 accepted -- members beyond a shorter struct keep their
           defaults, members inside are taken as given --, 0, 4, 6 and 4100 refused; one refusal per range check with its text; the
           statistics copy: a 16-byte caller struct gets 16 bytes and keeps its size, a longer one is filled up to the library's size and
           no further (guard bytes behind), an invalid size writes nothing.
Every run must leave the sanitizers' report stream empty.
"""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def driver():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "oracle"), "scf_config"], stdout=subprocess.DEVNULL)
    exe = os.path.join(ROOT, "oracle", "_build", "scf_config_main")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")

    def run(mode):
        r = subprocess.run([exe, mode], capture_output=True, text=True, timeout=300, env=env)
        assert r.stderr == "", r.stderr[-4000:]
        assert "VIOLATION" not in r.stdout, "\n".join(ln for ln in r.stdout.splitlines() if ln.startswith("VIOLATION"))[:4000]
        assert r.returncode == 0 and r.stdout.splitlines()[-1] == "0 violations", r.stdout[-2000:]
        return r.stdout.splitlines()
    return run


def test_plan_equals_the_replaced_loop(driver):
    ions = sum(min(4, Z) for Z in range(1, 119))                 # q = 0..3 where q < Z
    assert "plan: %d cases" % (4 * (118 + 1 + ions) + 2) in driver("plan")


def test_refusals_are_the_replaced_loops(driver):
    assert "refusals: 20 cases" in driver("refusals")


def test_options_and_the_struct_size_protocol(driver):
    assert "options: 42 cases" in driver("options")
