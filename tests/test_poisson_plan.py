"""CPU suite: the multigrid's layout planner (dftatom_amd/csrc/poisson_plan.cpp), run as a stand-alone program under AddressSanitizer +
UndefinedBehaviorSanitizer (`make -C oracle plan`: oracle/plan_main.cpp, nothing is loaded into Python).

1. tests/golden/poisson_plans.json holds what the last commit before the planner existed decided on an MI355X -- every MgDesc member,
   the flags, the allocation counts -- for its inputs (grid, batch, mode, force_logG, knobs, the occupancies the runtime reported).
   The planner must reproduce every record, field for field.
2. A sweep over inputs one machine cannot record (batch 1..256, four grids, three modes, 64 .. 304 compute units, occupancy 0 .. 2)
   must satisfy the properties listed in oracle/plan_main.cpp: co-resident groups, contiguous levels, a staging memory without
   overlaps, resident => one workgroup's layout.  The driver checks the same properties on the plans of (1); as those equal the
   recorded ones, the properties hold for the recorded plans too.
Both runs must leave the sanitizers' report stream empty.
"""
import json
import os
import subprocess

import pytest

import _poisson_plans

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LV_FIELDS = ("n", "logC", "logT", "seq", "stage", "off", "soff", "d")
FLAG_KNOBS = {"POISSON_" + k: k.lower() for k in ("NOSTAGE", "NOSTAGE_WAVE", "NOSTAGE_SHARED", "NOCOARSE", "NOXW", "NORC", "NOFUSE3", "NOFUSE3_WAVE",
                                                 "NOHALF129", "NOFOLD", "NOFOLD_LDS", "NOFUSE_COOP", "PLAIN_LAUNCH")}


def atoi(text):
    digits = ""
    for ch in text.strip():
        if ch.isdigit() or (ch in "+-" and not digits):
            digits += ch
        else:
            break
    return int(digits) if digits not in ("", "+", "-") else 0


def case_line(inp):
    """a record's inputs as the driver reads them; the knob list is parsed as poisson.hip's read_knobs parses it"""
    t = {k: inp[k] for k in ("N", "levels", "delta", "uniform", "batch", "force_logG", "mode", "num_cu", "occ_solve")}
    t["occ_res"] = t["occ_res16"] = inp["occ_res"]          # (-1: the runtime was not asked, and the planner does not ask either)
    t["plain_launch"] = inp["rocp_tool"]
    for entry in filter(None, inp["knobs"].split(",")):
        name, _, val = entry.partition("=")
        if name in FLAG_KNOBS:
            t[FLAG_KNOBS[name]] = 1
        elif name == "POISSON_GROUP":
            t["group_set"] = 1
            if 0 <= atoi(val) <= 6 and (inp["batch"] << atoi(val)) <= 256:
                t["group"] = atoi(val)
        elif name in ("POISSON_RES", "POISSON_RES16"):
            t[name[8:].lower()] = int(atoi(val) != 0)
        elif name == "POISSON_FUSE_MIN_LOGC":
            t["fuse_min_logc"] = max(6, atoi(val))
        elif name == "POISSON_DBG":
            t["dbg"] = atoi(val)
        elif name == "FAULT_POISSON_MEMBER":
            t["fault"] = int(atoi(val) != 0)
        else:
            raise AssertionError("knob %s is not one the planner reads" % name)
    return " ".join("%s=%s" % kv for kv in t.items())


@pytest.fixture(scope="module")
def plan_main():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "oracle"), "plan"], stdout=subprocess.DEVNULL)
    exe = os.path.join(ROOT, "oracle", "_build", "plan_main")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")

    def run(args, stdin=""):
        r = subprocess.run([exe] + args, input=stdin, capture_output=True, text=True, timeout=300, env=env)
        assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr and "LeakSanitizer" not in r.stderr, r.stderr[-4000:]
        assert r.stderr == "", r.stderr[-4000:]
        return r
    return run


def test_planner_reproduces_the_recorded_plans(plan_main):
    header, records = _poisson_plans.load()
    assert len(records) >= 700 and header["parent_commit"].startswith("c50ad77")
    r = plan_main([], "\n".join(case_line(rec["in"]) for rec in records) + "\n")
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert [ln for ln in r.stdout.splitlines() if ln.startswith("VIOLATION")] == []
    assert r.returncode == 0 and len(lines) == len(records)
    for rec, line in zip(records, lines):
        got = json.loads(line)
        want = {k: rec[k] for k in ("flags", "alloc", "soff", "desc")}
        want["occ_res"], want["occ_solve"] = rec["in"]["occ_res"], rec["in"]["occ_solve"]
        got["desc"]["lv"] = [[lv[k] for k in LV_FIELDS] for lv in got["desc"]["lv"]]
        assert got == want, (rec["in"], {k: (got["desc"].get(k), want["desc"].get(k)) for k in want["desc"] if got["desc"].get(k) != want["desc"].get(k)},
                             {k: (got.get(k), want.get(k)) for k in want if k != "desc" and got.get(k) != want.get(k)})


def test_fixture_covers_the_thresholds():
    recs = _poisson_plans.load()[1]
    plain = [r["in"] for r in recs if not r["in"]["knobs"] and r["in"]["force_logG"] < 0]
    assert {(i["N"], i["uniform"]) for i in plain} == {(4097, 0), (16385, 0), (131073, 0), (1048577, 0), (16385, 1)}
    assert {i["batch"] for i in plain} == {1, 4, 5, 7, 8, 12, 15, 16, 17, 32, 33, 64, 65, 128, 129, 256}
    assert {i["mode"] for i in plain} == {0, 1, 2}
    assert any(r["in"]["force_logG"] == 0 for r in recs)
    assert any(r["flags"]["resident"] and not r["flags"]["res16"] for r in recs) and any(r["flags"]["res16"] for r in recs)
    assert {r["desc"]["logG"] for r in recs} >= {0, 1, 2, 3, 4, 5}


def test_sweep_properties(plan_main):
    r = plan_main(["--sweep"])
    assert r.returncode == 0, r.stdout[-4000:]
    assert "VIOLATION" not in r.stdout
    assert "sweep: %d plans, 0 violations" % (256 * 4 * 3 * 4 * 9) in r.stdout


def test_sequential_levels_over_budget_is_a_status(plan_main):
    # (no grid the library makes: 127 + 64 + 32 + ... nodes, all below 129, exceed the LDS budget of the sequential levels)
    r = plan_main([], "N=127 levels=7 delta=0x1p-10 batch=1 num_cu=256 occ_solve=2\n")
    assert json.loads(r.stdout.splitlines()[0]) == {"error": "sequential levels exceed LDS budget"}
