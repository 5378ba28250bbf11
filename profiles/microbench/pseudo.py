"""Timing of the Troullier-Martins pseudization (dftatom_amd/csrc/pseudo.hip: k_pseudize), DESIGN.md 4.15.

    python profiles/microbench/pseudo.py --atoms 86 --levels 17          # Rn LDA at 131 073 nodes: its default valence channels
    python profiles/microbench/pseudo.py --atoms 1-86 --levels 14        # Z = 1 .. 86 at 16 385 nodes, every atom's channels in one launch

Three SCF steps; the valence orbitals of the third step (default_valence) in that step's input potential, core nodes default_ic(1.5);
pseudize() 3 + 15 times; the HIP-event time of the one launch (dfta_ctx_last_kernel_ms) -- median, min, max --, the evaluations of g per
channel, and the floor of the launch: the bytes it must move (per channel V and u read once for the check and the copies, u_ps and V_ps
written: 4 N doubles) over the measured HBM copy rate (Context.measure_hbm); then pseudo_ionic() on the result the same way (the y
launch, the density, the functional, the pointwise pass and the quadratures in one bracket), and before both the whole
Scf.pseudopotentials() call on the resident batch as host wall time (its two brackets are the launches timed above; the rest is the
default core nodes' read of the orbitals, the copies of the rows to the host and the Python wrapper), after --scf-steps steps in
all.  Prints one JSON line.
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))

GRIDS = {12: (2e-3, 25.0), 14: (5e-4, 25.0), 17: (1e-4, 50.0)}


def atoms(text):
    out = []
    for part in text.split(","):
        if "-" in part:
            a, b = part.split("-")
            out += list(range(int(a), int(b) + 1))
        else:
            out.append(int(part))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--atoms", default="86")
    ap.add_argument("--levels", type=int, default=17, choices=sorted(GRIDS))
    ap.add_argument("--factor", type=float, default=1.5)
    ap.add_argument("--scf-steps", type=int, default=30, help="SCF steps before the resident call is timed (the direct entries are timed after three)")
    args = ap.parse_args()
    import numpy as np
    import dftatom_amd as D
    Z = atoms(args.atoms)
    ctx = D.Context(0)
    grid = D.Grid(ctx, args.levels, *GRIDS[args.levels])
    scf = D.Scf(ctx, grid, Z)
    scf.step(want_stats=False)
    scf.step(want_stats=False)
    Vin = [scf.array(3, a) for a in range(len(Z))]
    scf.step(want_stats=False)
    V, u, l, eps, atom, occ = [], [], [], [], [], []
    for a in range(len(Z)):
        lv, U = scf.levels(a, 0), scf.orbitals(a, 0)
        for k in D.default_valence(lv["n"], lv["l"], lv["occupation"]):
            V.append(Vin[a]); u.append(U[k]); l.append(int(lv["l"][k])); eps.append(float(lv["E"][k]))
            atom.append(a); occ.append(float(lv["occupation"][k]))
    import time
    for _ in range(args.scf_steps - 3):              # the resident call wants a potential near the orbitals' own: more steps first
        scf.step(want_stats=False)
    wall = []
    for k in range(18):                              # the whole resident call: host wall time (its launches, copies and host work)
        t0 = time.perf_counter()
        res = scf.pseudopotentials(factor=args.factor)
        if k >= 3:
            wall.append((time.perf_counter() - t0) * 1e3)
    scf_bad = int(np.count_nonzero(res["status"]))   # (after three steps only, the resident potential is far from the orbitals' own and most channels find no bracket)
    scf.close()
    V, u = np.array(V), np.array(u)
    ic = D.default_ic(grid, u, args.factor)
    ms = []
    for k in range(18):
        out = D.pseudize(ctx, grid, V, u, l, eps, ic)
        if k >= 3:
            ms.append(ctx.last_kernel_ms())
    ms_ion = []
    for k in range(18):                              # the unscreening and the Kleinman-Bylander quantities: five launches
        D.pseudo_ionic(ctx, grid, out, l, occ, atom)
        if k >= 3:
            ms_ion.append(ctx.last_kernel_ms())
    copy_gbs, _ = ctx.measure_hbm()
    nbytes = 4 * 8 * grid.N * len(l)
    med = statistics.median(ms)
    print(json.dumps({"case": "pseudize", "Z": Z if len(Z) <= 12 else "%d..%d" % (Z[0], Z[-1]), "nodes": grid.N, "channels": len(l),
                      "status_nonzero": int(np.count_nonzero(out["status"])), "ic_min": int(ic.min()), "ic_max": int(ic.max()),
                      "iters_min": int(out["iters"].min()), "iters_max": int(out["iters"].max()), "ms_median": med, "ms_min": min(ms),
                      "ms_max": max(ms), "ionic_ms_median": statistics.median(ms_ion), "scf_steps": args.scf_steps, "scf_call_wall_ms_median": statistics.median(wall), "scf_call_status_nonzero": scf_bad, "bytes": nbytes, "hbm_copy_GBs": copy_gbs, "floor_ms": nbytes / copy_gbs * 1e-6}), flush=True)
    grid.close()
    ctx.close()


if __name__ == "__main__":
    main()
