"""GPU suite (-m gpu): the EFFORT of the level search, step by step, against tests/golden/levels_effort.json.

Predictions (path bits, history brackets and their ratio extrapolation, the scan predictor, the candidate budget) never change a
result, so every other test passes when one of them is lost -- the step is slower with the same bits.  The host rounds run in lock
step: their rounds, issued sweeps and traversed points are a function of the inputs alone, and this test pins them (the device-side
search runs at its own pace and is covered by timing instead).  The expected values were recorded by tests/golden/make_levels_effort.py,
which also defines the cases; a case holds the fields that repeated between two runs when it was recorded.
"""
import json
import os

import pytest

pytestmark = pytest.mark.gpu

import dftatom_amd as D
from golden.make_golden import GRIDS                                          # noqa: E402
from golden.make_levels_effort import CASES, FIELDS, SCAN_FIELDS, OUT, run_case    # noqa: E402


@pytest.fixture(scope="module")
def ctx(torch_first):
    c = D.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def expected():
    with open(OUT) as f:
        return json.load(f)


@pytest.mark.parametrize("name", sorted(CASES))
def test_effort_of_every_step_is_the_recorded_one(ctx, expected, name):
    case, want = CASES[name], expected[name]
    # the host-round cases are lock-step: all seven fields are recorded; the scan search keeps at least the ones that cannot race
    assert set(want) >= set(SCAN_FIELDS if case["tolerance"] else FIELDS), sorted(want)
    L, d, R = GRIDS["L14"]
    grid = D.Grid(ctx, L, d, R)
    got = run_case(D, ctx, grid, case)
    grid.close()
    for f in FIELDS:
        print(name, f, got[f])
    seen = got["levels_layout"]
    assert sorted(set(seen)) == case["layouts"], seen
    assert seen == sorted(seen), seen                    # (the switch to the live jobs happens once, late)
    for f in sorted(want):
        assert got[f] == want[f], (name, f)
