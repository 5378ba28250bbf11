"""GPU suite: the solver that dfta_poisson_create_ex builds has the layout the parent commit's creation chose on the same device
(tests/golden/poisson_plans.json, see tests/test_poisson_plan.py).  Creation only -- nothing is solved: the workgroups per atom and
the size of every level, for the recorded default-knob cases at 16 385 nodes (logarithmic and uniform grid, every recorded batch)
and at 131 073 nodes for batches 1, 7, 8, 15, 16 (the resident configurations' thresholds), in the three modes.
"""
import os

import pytest

import _poisson_plans
import dftatom_amd as D

pytestmark = pytest.mark.gpu


def test_created_solvers_match_the_recorded_plans():
    assert not os.environ.get("DFTA_DEBUG"), "the recorded cases are those without knobs"
    cases = [r for r in _poisson_plans.load()[1] if not r["in"]["knobs"] and r["in"]["force_logG"] < 0 and not r["in"]["rocp_tool"] and
             (r["in"]["N"] == 16385 or (r["in"]["N"] == 131073 and r["in"]["batch"] in (1, 7, 8, 15, 16)))]
    assert len(cases) == 2 * 16 * 3 + 5 * 3
    ctx = D.Context(0)
    grids = {}
    try:
        assert ctx.device_info()[0] == cases[0]["in"]["num_cu"], "the fixture was recorded on a device with another number of compute units"
        for r in cases:
            i = r["in"]
            key = (i["levels"], i["delta"], i["uniform"])
            if key not in grids:
                grids[key] = D.Grid(ctx, i["levels"], None if i["uniform"] else float.fromhex(i["delta"]), 25.0)
            assert grids[key].N == i["N"]
            p = D.Poisson(ctx, grids[key], i["batch"], i["mode"])
            try:
                want_G = (17 if r["flags"]["res16"] else 33) if r["flags"]["resident"] else r["desc"]["G"]
                assert p.group_info() == (want_G, False, 0), (i, p.group_info())
                assert [p.level_size(l) for l in range(i["levels"])] == [row[0] for row in r["desc"]["lv"]], i
                assert p.level_size(i["levels"]) == -1
            finally:
                p.close()
    finally:
        for g in grids.values():
            g.close()
        ctx.close()
