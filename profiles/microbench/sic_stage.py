"""Timing of the SIC-KLI stage of a self-interaction-corrected step (dftatom_amd/csrc/kli_stage.hip: k_sic_*), DESIGN.md 4.13, on the
workloads of 4.12 and beside the exchange-only KLI stage of the same build (whose kernels this stage leaves untouched).

    python profiles/microbench/sic_stage.py stage --atoms 86 --levels 17            # Rn LDA at 131 073 nodes
    python profiles/microbench/sic_stage.py stage --atoms 2,4,10,12,18,20,30,36,38,48,54,56 --levels 14
    python profiles/microbench/sic_stage.py stage --atoms 1-86 --levels 14
    python profiles/microbench/sic_stage.py steps --atoms 1-86 --levels 14 --cap 100  # steps to finish of the batch under EXCHANGE_SIC_KLI

stage: three steps, then 15 more, for EXCHANGE_SIC_KLI and for EXCHANGE_KLI; per step the stage's HIP-event time (Scf.exchange_ms) and the
step's three phase times; medians.  Prints one JSON line.
"""
import argparse
import json
import os
import statistics
import sys
import time

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


def stage(args, D):
    Z = atoms(args.atoms)
    ctx = D.Context(0)
    grid = D.Grid(ctx, args.levels, *GRIDS[args.levels])
    out = {"case": "stage", "Z": Z if len(Z) <= 12 else "%d..%d" % (Z[0], Z[-1]), "nodes": grid.N, "channels": len(Z)}
    for name, ex in (("sic", D.EXCHANGE_SIC_KLI), ("kli", D.EXCHANGE_KLI)):
        scf = D.Scf(ctx, grid, Z, exchange=ex)
        ms, step_ms = [], []
        for k in range(18):
            st = scf.step()
            if k >= 3:
                ms.append(scf.exchange_ms())
                step_ms.append(st.ms_levels + st.ms_poisson + st.ms_tail)
        shells = [len(scf.levels(a, 0)["l"]) for a in range(len(Z))]
        rows = sum(shells) if name == "sic" else sum(len(D.exchange_jobs(scf.levels(a, 0)["l"])) for a in range(len(Z)))
        out[name] = {"y_rows": rows, "stage_ms_median": statistics.median(ms), "stage_ms_min": min(ms), "stage_ms_max": max(ms),
                     "step_ms_median": statistics.median(step_ms), "stage_share_of_step": statistics.median(ms) / statistics.median(step_ms)}
        scf.close()
    out["sic_over_kli"] = out["sic"]["stage_ms_median"] / out["kli"]["stage_ms_median"]
    print(json.dumps(out), flush=True)
    grid.close()
    ctx.close()


def steps(args, D):
    Z = atoms(args.atoms)
    ctx = D.Context(0)
    grid = D.Grid(ctx, args.levels, *GRIDS[args.levels])
    scf = D.Scf(ctx, grid, Z, exchange=D.EXCHANGE_SIC_KLI)
    t0, n = time.perf_counter(), 0
    while n < args.cap and not scf.energies()[1].all():
        scf.step(want_stats=False)
        n += 1
    ctx.synchronize()
    en, fin = scf.energies()
    per_atom = [int(e.steps) if hasattr(e, "steps") else None for e in en]
    print(json.dumps({"case": "steps", "nodes": grid.N, "cap": args.cap, "batch_steps": n, "seconds": time.perf_counter() - t0,
                      "finished": int(fin.sum()), "atoms": len(Z), "not_finished": [int(z) for z, f in zip(Z, fin) if not f],
                      "steps_per_atom": per_atom if all(p is not None for p in per_atom) else None,
                      "Etotal_first_last": [en[0].Etotal, en[-1].Etotal]}), flush=True)
    scf.close()
    grid.close()
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("case", choices=("stage", "steps"))
    ap.add_argument("--atoms", default="86")
    ap.add_argument("--levels", type=int, default=17, choices=sorted(GRIDS))
    ap.add_argument("--cap", type=int, default=100)
    args = ap.parse_args()
    import dftatom_amd as D
    (stage if args.case == "stage" else steps)(args, D)


if __name__ == "__main__":
    main()
