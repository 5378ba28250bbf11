"""Timing of the Kleinman-Bylander sweeps and of the bound-state search (dftatom_amd/csrc/kb.hip: k_kb), DESIGN.md 4.16.

    python profiles/microbench/kb.py --atoms 86 --levels 17 --energies 256      # Rn LDA at 131 073 nodes: its valence channels
    python profiles/microbench/kb.py --atoms 1-86 --levels 14 --energies 64     # Z = 1 .. 86 at 16 385 nodes, every atom's channels

--scf-steps SCF steps, then Scf.pseudopotentials() (the highest l local).  Every channel -- the local ones with beta = 0, q1 = 1 -- gets
--energies energies in -2 .. 1 Ha at the end node N - 2.  Timed, median of 15 calls after 3, the HIP-event time of
dfta_ctx_last_kernel_ms: ONE launch of kb_sweep() on all those trials; continuum() without partners on the same (potential, l, E, m)
trials -- the channel's own local potential -- in the same process; the whole kb_bound_states() search of every channel in -20 .. 0 Ha,
256 scan energies.  The floor is the bytes the sweep launch must move -- per channel Vloc, beta, r and s read once, 4 N doubles, and 7
doubles written per trial -- over the measured HBM copy rate (Context.measure_hbm).  No counters are collected.  Prints one JSON line.
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


def timed(ctx, call):
    ms = []
    for k in range(18):
        out = call()
        if k >= 3:
            ms.append(ctx.last_kernel_ms())
    return statistics.median(ms), min(ms), max(ms), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--atoms", default="86")
    ap.add_argument("--levels", type=int, default=17, choices=sorted(GRIDS))
    ap.add_argument("--energies", type=int, default=256)
    ap.add_argument("--scf-steps", type=int, default=30)
    args = ap.parse_args()
    import numpy as np
    import dftatom_amd as D
    Z = atoms(args.atoms)
    ctx = D.Context(0)
    grid = D.Grid(ctx, args.levels, *GRIDS[args.levels])
    scf = D.Scf(ctx, grid, Z)
    for _ in range(args.scf_steps):
        scf.step(want_stats=False)
    ps = scf.pseudopotentials()
    scf.close()
    good = np.nonzero(ps["status"] == 0)[0]
    nch, N = len(good), grid.N
    local = np.isnan(ps["kb"][good, 2])
    vidx = np.array([int(np.nonzero((ps["atom"][good] == ps["atom"][k]) & local)[0][0]) for k in good], np.int32)
    V, l = ps["V_ps"][good], ps["l"][good]
    beta = np.where(local[:, None], 0.0, ps["beta"][good])
    q1 = np.where(local, 1.0, ps["kb"][good, 0])
    E = np.tile(np.linspace(-2.0, 1.0, args.energies), nch)
    chan = np.repeat(np.arange(nch, dtype=np.int32), args.energies)
    m = np.full(len(E), N - 2, np.int32)
    kb = timed(ctx, lambda: D.kb_sweep(ctx, grid, V, l, beta, q1, E, m, chan=chan, vidx=vidx))
    cont = timed(ctx, lambda: D.continuum(ctx, grid, V, l[chan], E, m, vidx=vidx[chan]))
    nl = np.nonzero(~local)[0]
    srch = timed(ctx, lambda: D.kb_bound_states(ctx, grid, V, l[nl], beta[nl], q1[nl], -20.0, 0.0, vidx=vidx[nl], nscan=256))
    copy_gbs, _ = ctx.measure_hbm()
    nbytes = 4 * 8 * N * nch + 7 * 8 * len(E)
    points = float(len(E)) * (N - 1)
    print(json.dumps({"case": "kb", "Z": Z if len(Z) <= 12 else "%d..%d" % (Z[0], Z[-1]), "nodes": N, "channels": nch, "trials": len(E),
                      "status_nonzero": int(np.count_nonzero(kb[3]["status"])), "kb_ms_median": kb[0], "kb_ms_min": kb[1], "kb_ms_max": kb[2],
                      "continuum_ms_median": cont[0], "continuum_ms_min": cont[1], "continuum_ms_max": cont[2], "ratio": kb[0] / cont[0],
                      "kb_ns_per_point": kb[0] * 1e6 / points, "continuum_ns_per_point": cont[0] * 1e6 / points,
                      "search_channels": len(nl), "search_ms_median": srch[0], "search_ms_min": srch[1], "search_ms_max": srch[2],
                      "search_rounds_max": int(srch[3]["rounds"].max()) if len(nl) else 0, "search_states": int(srch[3]["count"].sum()) if len(nl) else 0,
                      "scf_steps": args.scf_steps, "bytes": nbytes, "hbm_copy_GBs": copy_gbs, "floor_ms": nbytes / copy_gbs * 1e-6,
                      "counters": "none collected"}), flush=True)
    grid.close()
    ctx.close()


if __name__ == "__main__":
    main()
