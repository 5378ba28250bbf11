#!/usr/bin/env python3
"""Recorded effort of the level search's host rounds (and of the scan search): tests/golden/levels_effort.json.

    python tests/golden/make_levels_effort.py [OUT]      (on a GPU, with the library of the commit whose effort is to be pinned;
                                                          DFTA_LIB_PATH=<libdftatom_hip.so of that commit> selects a build kept elsewhere)

The host rounds run in lock step, so the rounds, sweeps and points of a step are a function of the inputs alone.  Predictions never
change a result, so a change that loses one (a history bracket not carried, the scan predictor not run, ...) passes every other test;
tests/test_gpu_levels_effort.py compares the cases below with this file, field by field.  Every case runs twice here; a field is
written only if both runs agree in it in every step (the grouped members of the scan search race: its issued sweeps may not repeat).
Regenerate the file only from the commit BEFORE a change to the level search's host code, never with the change itself.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from _knobs import knobs  # noqa: E402
from golden.make_golden import GRIDS  # noqa: E402

OUT = os.path.join(HERE, "levels_effort.json")
FIELDS = ("levels_layout", "rounds", "sweeps_issued", "points_traversed", "sweeps_reference", "sweeps_reference_executed", "points_reference")
# fields the scan search may keep when its grouped members race
SCAN_FIELDS = ("levels_layout", "rounds", "sweeps_reference", "sweeps_reference_executed", "points_reference")

# name: atoms, knobs (set while the SCF is created), steps (None: to the end, at most 100), tolerance sweeps, layouts the steps must show
CASES = {
    "ar_latency": dict(Zs=[18], knobs=["LEVELS_NOPERSIST"], steps=7, tolerance=False, layouts=[1]),
    "z20_30_static_scan_predictor": dict(Zs=list(range(20, 31)), knobs=["LEVELS_NOPERSIST"], steps=5, tolerance=False, layouts=[0]),
    "z20_30_static": dict(Zs=list(range(20, 31)), knobs=["LEVELS_NOPERSIST", "LEVELS_NOSCANPREDICT_BATCH"], steps=5, tolerance=False, layouts=[0]),
    "z1_45_packed": dict(Zs=list(range(1, 46)), knobs=["LEVELS_NOPERSIST"], steps=4, tolerance=False, layouts=[2]),
    "last_live_atoms_switch": dict(Zs=[36] * 5 + [18] * 4 + [10] * 3 + [2], knobs=["LEVELS_NOPERSIST"], steps=None, tolerance=False, layouts=[0, 3]),
    "kr_tolerance_sweeps": dict(Zs=[36], knobs=[], steps=4, tolerance=True, layouts=[4]),
}


def run_case(D, ctx, grid, case):
    """the recorded fields of every step of one case: {field: [value of step 1, ...]}"""
    with knobs({k: "1" for k in case["knobs"]}):
        scf = D.Scf(ctx, grid, case["Zs"], lsda=False, **({"sweep_mode": D.SWEEPS_TOLERANCE} if case["tolerance"] else {}))
    out = {f: [] for f in FIELDS}
    steps = 0
    while steps < (case["steps"] or 100):
        st = scf.step()
        steps += 1
        for f in FIELDS:
            out[f].append(int(getattr(st, f)))
        if case["steps"] is None and scf.energies()[1].all():
            break
    scf.close()
    return out


def main():
    import dftatom_amd as D
    ctx = D.Context(0)
    L, d, R = GRIDS["L14"]
    grid = D.Grid(ctx, L, d, R)
    result, findings = {}, []
    for name, case in CASES.items():
        a, b = run_case(D, ctx, grid, case), run_case(D, ctx, grid, case)
        keep = {f: a[f] for f in FIELDS if a[f] == b[f]}
        lost = [f for f in FIELDS if f not in keep]
        must = SCAN_FIELDS if case["tolerance"] else FIELDS
        if any(f in must for f in lost):
            findings.append("%s: %s did not repeat" % (name, ", ".join(lost)))
        result[name] = keep
        print("%-30s %3d steps, layouts %s, rounds %s%s" % (name, len(a["rounds"]), sorted(set(a["levels_layout"])), a["rounds"][:8],
                                                             ("; NOT repeating: " + ", ".join(lost)) if lost else ""), flush=True)
    grid.close()
    ctx.close()
    with open(sys.argv[1] if len(sys.argv) > 1 else OUT, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
        f.write("\n")
    for line in findings:
        print("FINDING:", line)
    return 1 if findings else 0


if __name__ == "__main__":
    sys.exit(main())
