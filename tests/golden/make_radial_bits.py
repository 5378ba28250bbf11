#!/usr/bin/env python3
"""The bits of the radial-integral kernels (orbitals.hip, slater.hip, bessel.hip, exchange.hip, kli_stage.hip): tests/golden/radial_bits.json.

    python tests/golden/make_radial_bits.py [OUT]       (on a GPU, with the library of the commit whose bits are to be pinned;
                                                          DFTA_LIB_PATH=<libdftatom_hip.so of that commit> selects a build kept elsewhere)

The other GPU tests hold these kernels to references within rounding bounds, which a change of the order of operations passes.  The
kernels promise stated orders, so a change that means to keep them (a refactor) must keep every bit: tests/test_gpu_radial_bits.py
rebuilds the cases below and compares SHA-256 digests of array.tobytes() (float64 or int32, C order) and shapes with this file.  A case
is one call: where a call returns several arrays, its digest runs over all of them in the order of their sorted names, and the shapes
are listed in that order.
The inputs are made from grid.r() with + - * / alone, which NumPy rounds the same everywhere; their digests are recorded too and
checked first.  Every case runs twice here; nothing is written unless both runs agree in every digest.
Regenerate the file only from the commit BEFORE a change to these kernels, never with the change itself.
"""
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from _knobs import knobs  # noqa: E402

OUT = os.path.join(HERE, "radial_bits.json")

# name: (multigrid levels, delta (None: uniform), Rmax); 2^levels + 1 nodes.  1025 and 2049: the last node is the first of a tile (its
# stencil reaches back across the boundary), 2049 with a full middle tile; 4097 logarithmic: cnst != 1, four carries
GRIDS = {"uni9": (3, None, 10.0), "uni33": (5, None, 10.0), "uni1025": (10, None, 10.0), "uni2049": (11, None, 10.0),
         "log4097": (12, 2e-3, 25.0)}
SCF_GRID = "log4097"
L = [0, 1, 0, 2, 0]
SLATER_JOBS = [(0, 0, 0, 0, 0), (0, 1, 0, 1, 0), (0, 1, 1, 0, 8), (2, 3, 2, 3, 8), (0, 1, 2, 3, 1), (2, 2, 2, 2, 8), (3, 2, 1, 0, 4),
               (4, 0, 4, 0, 0), (0, 4, 1, 2, 3), (4, 4, 4, 4, 8)]
# x = y, x < y, x > y, k = 0, 1, 8, the zero row
YK_JOBS = [(0, 0, 0), (0, 1, 1), (1, 0, 1), (2, 3, 8), (3, 2, 0), (1, 1, 8), (2, 2, 1), (4, 0, 0), (0, 4, 1), (4, 4, 8)]
XP_OCC = [1.0, 3.0, 1.0, 0.5]                    # rows 0 .. 3, the HOMO the last row
CH_NORB, CH_OCC, CH_E = [2, 2], [1.0, 3.0, 1.0, 2.0], [-2.0, -0.5, -1.0, -0.25]
BT_ROWS, BT_L = [0, 1, 2, 3, 1, 4], [0, 1, 2, 3, 4, 0]
BT_Q = [0.0, 0.05, 0.3, 0.5, 1.0, 2.0, 3.0, 7.5, 20.0]       # q r crosses the series switch (3) inside the grid from 0.3 on
BESSEL_X = [0.0, 1e-3, 0.5, 1.0, 2.0, 2.9999999999999996, 3.0, 3.0000000000000004, 4.0, 10.0, 100.0, 1e4]


def digest(arrays):
    """of one array, or of the arrays of one call in order: the SHA-256 of their bytes end to end, and their shapes"""
    if isinstance(arrays, np.ndarray):
        arrays = [arrays]
    h, shapes = hashlib.sha256(), []
    for a in arrays:
        a = np.ascontiguousarray(a)
        assert a.dtype in (np.float64, np.int32), a.dtype
        h.update(a.tobytes())
        shapes.append(list(a.shape))
    return {"sha256": h.hexdigest(), "shape": shapes}


def orbitals(r):
    """the five rows of the cases, float64 (5, N), from r with + - * / alone"""
    t = 1. / (1. + r * r)
    return np.array([r * t, r * r * t * t, r * (1. - 0.375 * r) * t * t, r * r * r * t * t * t, 0. * r])


def _all(d):
    """every output of a call that returns a dict, in the order of the sorted names (a Python int as int32)"""
    out = []
    for k in sorted(d):
        v = d[k]
        if isinstance(v, list):                  # sic_channels' M: one matrix per channel
            out += v
        else:
            out.append(np.atleast_1d(np.asarray(v, dtype=np.int32 if isinstance(v, (int, np.integer)) else None)))
    return out


def grid_cases(D, ctx, grid, name, u):
    """{case name: array, or the arrays of the call} of every direct entry on one grid"""
    out = {}
    out[name + "/orbital_properties"] = D.orbital_properties(ctx, grid, L, u)
    for k in (0, 1, 2):
        out["%s/orbital_matrix/k%d" % (name, k)] = D.orbital_matrix(ctx, grid, u, k)
    out[name + "/slater_rk"] = D.slater_rk(ctx, grid, u, SLATER_JOBS)
    out[name + "/screening_yk"] = D.screening_yk(ctx, grid, u, YK_JOBS)
    out[name + "/exchange_potentials"] = _all(D.exchange_potentials(ctx, grid, L[:4], XP_OCC, 3, u[:4]))
    for what, fn in (("kli_channels", D.kli_channels), ("sic_channels", D.sic_channels)):
        one = fn(ctx, grid, CH_NORB, L[:4], CH_OCC, CH_E, u[:4])
        two = fn(ctx, grid, CH_NORB, L[:4], CH_OCC, CH_E, u[:4], first_step=False, alpha=0.5, vx=one["vx"])
        # step 2 mixes v into itself (vx == v_raw again): step 3 mixes with another weight into another vx, so that alpha and the
        # first-step flag show in the bits
        three = fn(ctx, grid, CH_NORB, L[:4], CH_OCC, CH_E, u[:4], first_step=False, alpha=0.25, vx=0.5 * one["vx"])
        for n, step in enumerate((one, two, three)):
            out["%s/%s/step%d" % (name, what, n + 1)] = _all(step)
    rows = u[BT_ROWS]
    for kind, kname in ((D.BT_DENSITY, "density"), (D.BT_ORBITAL, "orbital")):
        with knobs(BESSEL_QBLOCK=8):             # one full block of 8 q's and a short one
            out["%s/bessel_transform/%s/qblock8" % (name, kname)] = D.bessel_transform(ctx, grid, kind, BT_L, rows, BT_Q)
        out["%s/bessel_transform/%s" % (name, kname)] = D.bessel_transform(ctx, grid, kind, BT_L, rows, BT_Q)
    return out


def bessel_cases(D, ctx):
    return {"sph_bessel/l%d" % l: D.sph_bessel(ctx, l, BESSEL_X) for l in range(5)}


def scf_cases(D, ctx, grid):
    """the exchange stage inside the SCF: two steps of Ne LDA under EXCHANGE_KLI and of N LSDA under EXCHANGE_SIC_KLI"""
    out = {}
    for name, Z, lsda, exchange in (("scf/ne_kli", 10, False, D.EXCHANGE_KLI), ("scf/n_sic", 7, True, D.EXCHANGE_SIC_KLI)):
        scf = D.Scf(ctx, grid, [Z], lsda=lsda, exchange=exchange)
        scf.step()
        scf.step()
        out[name + "/energies"] = np.array(scf.energies()[0][0].as_list())
        for spin in range(2 if lsda else 1):
            out["%s/exchange/spin%d" % (name, spin)] = _all(scf.exchange(0, spin))
            if exchange == D.EXCHANGE_SIC_KLI:
                out["%s/sic_table/spin%d" % (name, spin)] = _all(scf.sic_table(0, spin))
        scf.close()
    return out


def run_all(D, ctx):
    """(inputs, cases): {name: digest} of r and the orbitals of every grid, and of every case"""
    inputs, cases = {}, {}
    for name, (lv, d, Rm) in GRIDS.items():
        grid = D.Grid(ctx, lv, d, Rm)
        r = grid.r()
        u = orbitals(r)
        inputs[name + "/r"], inputs[name + "/u"] = digest(r), digest(u)
        arrays = grid_cases(D, ctx, grid, name, u)
        if name == SCF_GRID:
            arrays.update(scf_cases(D, ctx, grid))
        grid.close()
        cases.update({k: digest(v) for k, v in arrays.items()})
    cases.update({k: digest(v) for k, v in bessel_cases(D, ctx).items()})
    return inputs, cases


def main():
    import dftatom_amd as D
    ctx = D.Context(0)
    a, b = run_all(D, ctx), run_all(D, ctx)
    ctx.close()
    differ = sorted(k for k in a[1] if a[1][k] != b[1][k])
    if a[0] != b[0] or differ:
        print("FINDING: not reproducible:", differ or "the inputs")
        return 1
    def block(d):                                # one line per case
        return "{\n" + ",\n".join("  %s: %s" % (json.dumps(k), json.dumps(d[k], sort_keys=True)) for k in sorted(d)) + "\n }"
    with open(sys.argv[1] if len(sys.argv) > 1 else OUT, "w") as f:
        f.write('{\n "inputs": %s,\n "cases": %s\n}\n' % (block(a[0]), block(a[1])))
    print("%d inputs, %d cases" % (len(a[0]), len(a[1])))
    return 0


if __name__ == "__main__":
    sys.exit(main())
