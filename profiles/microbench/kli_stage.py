"""Timing of the batched exchange stage of a self-consistent KLI step (dftatom_amd/csrc/kli_stage.hip), DESIGN.md 4.12.

    python profiles/microbench/kli_stage.py stage --atoms 86 --levels 17            # Rn LDA at 131 073 nodes
    python profiles/microbench/kli_stage.py stage --atoms 2,4,10,12,18,20,30,36,38,48,54,56 --levels 14
    python profiles/microbench/kli_stage.py steps --levels 14                        # steps to finish and wall time, KLI against VWN

stage: three steps, then 15 more; per step the stage's HIP-event time (Scf.exchange_ms) and the step's three phase times; then, on the same
state, the only way to the same potentials without the stage: a host loop of dfta_scf_exchange_potentials over the channels (vKLI and vbar
down, nothing else), wall clock around the loop, median of 15 after 3.  Prints one JSON line.  profiles/microbench/kli_stage.sh runs the
three commands above, each under its own time limit.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))

GRIDS = {12: (2e-3, 25.0), 14: (5e-4, 25.0), 17: (1e-4, 50.0)}
CLOSED = [2, 4, 10, 12, 18, 20, 30, 36]          # He Be Ne Mg Ar Ca Zn Kr


def host_loop(D, np, scf, Z):
    """vKLI and vbar of every channel through the one-channel entry; seconds"""
    lib, N = scf.ctx.lib, scf.grid.N
    v = np.zeros(N)
    t0 = time.perf_counter()
    for a in range(len(Z)):
        n = lib.dfta_scf_num_levels(scf.h, a, 0)
        vbar = np.zeros((n, D.XP_COLS))
        scf.ctx.check(lib.dfta_scf_exchange_potentials(scf.h, a, 0, None, None, None, v.ctypes.data_as(D.c_dp), vbar.ctypes.data_as(D.c_dp),
                                                       None, None))
    return time.perf_counter() - t0


def stage(args, D, np):
    Z = [int(z) for z in args.atoms.split(",")]
    ctx = D.Context(0)
    grid = D.Grid(ctx, args.levels, *GRIDS[args.levels])
    scf = D.Scf(ctx, grid, Z, exchange=D.EXCHANGE_KLI)
    ms, step_ms = [], []
    for k in range(18):
        st = scf.step()
        if k >= 3:
            ms.append(scf.exchange_ms())
            step_ms.append(st.ms_levels + st.ms_poisson + st.ms_tail)
    loops = [host_loop(D, np, scf, Z) for _ in range(18)][3:]
    njobs = sum(len(D.exchange_jobs(scf.levels(a, 0)["l"])) for a in range(len(Z)))
    out = {"case": "stage", "Z": Z, "nodes": grid.N, "channels": len(Z), "y_jobs": njobs, "y_rows_MB": njobs * grid.N * 8 / 2 ** 20,
           "stage_ms_median": statistics.median(ms), "stage_ms_min": min(ms), "stage_ms_max": max(ms),
           "step_ms_median": statistics.median(step_ms), "stage_share_of_step": statistics.median(ms) / statistics.median(step_ms),
           "host_loop_ms_median": 1e3 * statistics.median(loops), "host_loop_over_stage": 1e3 * statistics.median(loops) / statistics.median(ms)}
    print(json.dumps(out), flush=True)
    scf.close()
    grid.close()
    ctx.close()


def steps(args, D, np):
    ctx = D.Context(0)
    grid = D.Grid(ctx, args.levels, *GRIDS[args.levels])
    rows = []
    for z in CLOSED:
        row = {"Z": z}
        for name, ex in (("kli", D.EXCHANGE_KLI), ("vwn", D.EXCHANGE_FUNCTIONAL)):
            scf = D.Scf(ctx, grid, [z], exchange=ex)
            t0, n = time.perf_counter(), 0
            while n < args.cap and not scf.energies()[1][0]:
                scf.step(want_stats=False)
                n += 1
            ctx.synchronize()
            row[name] = {"steps": n, "finished": int(scf.energies()[1][0]), "seconds": time.perf_counter() - t0,
                         "Etotal": scf.energies()[0][0].Etotal}
            scf.close()
        rows.append(row)
    print(json.dumps({"case": "steps", "nodes": grid.N, "cap": args.cap, "atoms": rows}), flush=True)
    grid.close()
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("case", choices=("stage", "steps"))
    ap.add_argument("--atoms", default="86")
    ap.add_argument("--levels", type=int, default=17, choices=sorted(GRIDS))
    ap.add_argument("--cap", type=int, default=100)
    args = ap.parse_args()
    import numpy as np
    import dftatom_amd as D
    assert C.sizeof(C.c_double) == 8
    (stage if args.case == "stage" else steps)(args, D, np)


if __name__ == "__main__":
    main()
