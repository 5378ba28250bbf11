"""Timing of the outward sweeps (dftatom_amd/csrc/continuum.hip: k_partner_weight, k_continuum, k_continuum_scale), DESIGN.md 4.14, beside the
yardstick of the exact inward sweep (30-33 ns per dependent point, ~4 ms per full-length sweep at 131 073 nodes).

    python profiles/microbench/continuum.py --atoms 86 --levels 17 --per-l 256          # Rn LDA at 131 073 nodes, 5 x 256 trials, dipole partners
    python profiles/microbench/continuum.py --atoms 86 --levels 17 --per-l 256 --rows   # ... with the rows (1280 x 131 073 doubles to the host)
    python profiles/microbench/continuum.py --atoms 1-86 --levels 14 --per-l 64         # Z = 1 .. 86 at 16 385 nodes, 5 x 64 trials per atom

Three SCF steps, then Scf.continuum (l = 0 .. 4, `per-l` energies in (0, 8] Ha each, end node N - 2, dipole sums with the channel's
orbitals) 3 + 15 times; the HIP-event time of the call's launches (dfta_ctx_last_kernel_ms: the partner weighting and the sweeps; with
--rows also the scaling launches and the chunks' copies between them) -- median, min, max -- and the median over N - 2 nodes as ns per
dependent point of a lane.  Prints one JSON line.
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
    ap.add_argument("--per-l", type=int, default=256)
    ap.add_argument("--rows", action="store_true")
    ap.add_argument("--no-partners", action="store_true")
    args = ap.parse_args()
    import numpy as np
    import dftatom_amd as D
    Z = atoms(args.atoms)
    ctx = D.Context(0)
    grid = D.Grid(ctx, args.levels, *GRIDS[args.levels])
    scf = D.Scf(ctx, grid, Z)
    for _ in range(3):
        scf.step(want_stats=False)
    E1 = 8.0 * (np.arange(args.per_l) + 1) / args.per_l
    atom = np.repeat(np.arange(len(Z)), 5 * args.per_l)
    l = np.tile(np.repeat(np.arange(5), args.per_l), len(Z))
    E = np.tile(E1, 5 * len(Z))
    ms = []
    for k in range(18):
        out = scf.continuum(l, E, atom=atom, power=-1 if args.no_partners else 1, want_rows=args.rows)
        if k >= 3:
            ms.append(ctx.last_kernel_ms())
    assert not out["status"].any()
    med = statistics.median(ms)
    print(json.dumps({"case": "continuum", "Z": Z if len(Z) <= 12 else "%d..%d" % (Z[0], Z[-1]), "nodes": grid.N, "trials": len(E),
                      "waves": len(Z) * 5 * -(-args.per_l // 64), "partners": not args.no_partners, "rows": args.rows, "ms_median": med, "ms_min": min(ms),
                      "ms_max": max(ms), "ns_per_point": med * 1e6 / (grid.N - 2)}), flush=True)
    scf.close()
    grid.close()
    ctx.close()


if __name__ == "__main__":
    main()
