"""GPU suite (-m gpu): the BITS of the radial-integral kernels -- orbitals.hip, slater.hip, bessel.hip, exchange.hip, kli_stage.hip and
their shared device header radial_device.h -- against tests/golden/radial_bits.json.

The kernels follow stated orders of operations (include/dftatom_hip.h), and the other tests hold them to references within rounding
bounds: a reordering passes those.  This one rebuilds every case of tests/golden/make_radial_bits.py (the recipe that recorded the file:
every direct entry on five grids from one short tile to four carries, and two steps of a KLI and of a SIC-KLI SCF) and compares SHA-256
digests and shapes, one case per call.  The inputs' digests come first, so that input drift on another machine fails with a message
that says so and cannot be mistaken for a kernel change.  A deliberate change of an order is recorded by regenerating the file from
that commit.
"""
import json

import pytest

pytestmark = pytest.mark.gpu

import dftatom_amd as D                                                       # noqa: E402
from golden.make_radial_bits import GRIDS, OUT, SCF_GRID, bessel_cases, digest, grid_cases, orbitals, scf_cases    # noqa: E402


def test_every_case_has_the_recorded_bits(torch_first):
    with open(OUT) as f:
        want = json.load(f)
    ctx = D.Context(0)
    ran, wrong = 0, []

    def compare(arrays):
        nonlocal ran
        for name, a in arrays.items():
            ran += 1
            if want["cases"].get(name) != digest(a):
                wrong.append(name)

    for name, (lv, d, Rm) in GRIDS.items():
        grid = D.Grid(ctx, lv, d, Rm)
        r = grid.r()
        u = orbitals(r)
        assert digest(r) == want["inputs"][name + "/r"], "the INPUT r of %s differs from the recording: not a kernel change" % name
        assert digest(u) == want["inputs"][name + "/u"], "the INPUT orbitals of %s differ from the recording: not a kernel change" % name
        compare(grid_cases(D, ctx, grid, name, u))
        if name == SCF_GRID:
            compare(scf_cases(D, ctx, grid))
        grid.close()
    compare(bessel_cases(D, ctx))
    ctx.close()
    assert len(want["inputs"]) == 2 * len(GRIDS)
    assert ran == len(want["cases"]), "%d cases ran, the file has %d" % (ran, len(want["cases"]))
    assert not wrong, "%d of %d cases changed bits: %s" % (len(wrong), ran, ", ".join(wrong))
    print("%d cases, every digest as recorded" % ran)
