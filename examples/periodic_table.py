"""Periodic-table sweep (BASELINE.json config 4): LDA ground states of Z = 1 .. 86 on the 131073-node grid.

Atoms are independent: every rank takes its shard of `dftatom_amd.sweep.partition_atoms` (longest-processing-time on
subshells x expected SCF steps), advances all its atoms together (one `Scf` batch: every kernel works on the whole shard)
until each has met the reference's stop test or `--max-steps`; an atom that has finished is frozen in its own stop state and
costs nothing more (dfta_scf_step).  The fixed-size result records are gathered once (RCCL all_gather under torch.distributed).

    python examples/periodic_table.py                       # one GPU
    python -m torch.distributed.run --nnodes=1 --nproc-per-node 8 --master-addr 127.0.0.1 examples/periodic_table.py
    python examples/periodic_table.py --mixing anderson     # Anderson density mixing: about half the SCF steps
    python examples/periodic_table.py --charge 1            # the cations X+ (Z > charge)
    python examples/periodic_table.py --exx                 # E_H, the exact-exchange energy of the orbitals and the functional's E_xc per atom
    python examples/periodic_table.py --exchange kli --zmax 18 --levels 14   # self-consistent exchange-only KLI; lists the atoms that did not finish
    python examples/periodic_table.py --exchange sic --zmax 18 --levels 14   # self-interaction-corrected LSDA (Perdew-Zunger SIC through KLI)
    python examples/periodic_table.py --kli                 # E_x from the Fock averages and the tail r vKLI of the KLI exchange potential per atom
    python examples/periodic_table.py --form-factors        # X-ray form factors f(q) of every atom, one launch per shard
    python examples/periodic_table.py --ionization          # IE = E(X+) - E(X): neutral atom and cation of every Z in ONE batch per rank
"""
import argparse
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# total energies of the NIST LDA reference tables cited by the reference's README (Hartree)
NIST_LDA = {2: -2.834836, 10: -128.233481, 18: -525.946195, 36: -2750.147940, 54: -7228.856107, 86: -21861.346869}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--zmin", type=int, default=1)
    ap.add_argument("--zmax", type=int, default=86)
    ap.add_argument("--levels", type=int, default=17)
    ap.add_argument("--max-steps", type=int, default=100, help="the reference's cap (DFTAtom.cpp:396)")
    ap.add_argument("--out", default="")
    ap.add_argument("--partition", choices=("model", "work"), default="model",
                    help="model: balance the predicted shard times (critical path + work, dftatom_amd.sweep); work: LPT on subshells x steps")
    ap.add_argument("--xc", choices=("vwn", "pw92", "pbe"), default="vwn",
                    help="exchange-correlation functional: VWN (the reference's), Slater + PW92, or the PBE GGA (logarithmic grid)")
    ap.add_argument("--sweeps", choices=("exact", "tolerance"), default="exact", help="tolerance: the scan sweeps (DFTA_SWEEPS_TOLERANCE)")
    ap.add_argument("--poisson", choices=("exact", "tolerance", "adaptive"), default="exact",
                    help="tolerance: the multigrid's tolerance mode; adaptive: that, and the V-cycles stop at the round-off floor")
    ap.add_argument("--mixing", choices=("linear", "anderson"), default="linear",
                    help="anderson: Anderson density mixing (DFTA_MIX_ANDERSON), about half the SCF steps per atom")
    ap.add_argument("--exchange", choices=("functional", "kli", "sic"), default="functional",
                    help="kli: self-consistent exchange-only KLI (DFTA_EXCHANGE_KLI: every step's exchange potential from its own orbitals, no "
                         "correlation; --xc vwn and --mixing linear only).  The step cap is --max-steps; atoms that have not met the stop test "
                         "by then are listed (open-shell atoms such as Fe oscillate under this rule), not iterated further.  "
                         "sic: self-interaction-corrected LSDA (DFTA_EXCHANGE_SIC_KLI: VWN plus the Perdew-Zunger correction as one KLI "
                         "potential per spin channel; the same two conditions and the same listing)")
    ap.add_argument("--emulate-ranks", type=int, default=0,
                    help="one GPU, no launcher: run each of the N shards of an N-rank sweep alone, one after the other, and report the "
                         "per-shard wall times; their maximum PREDICTS the N-GPU wall time (shards never interact; the only collective "
                         "is a gather of 64 doubles per atom)")
    ap.add_argument("--charge", type=int, default=0, help="ionic charge of every atom (cations: dftatom_amd.ion_config); atoms with Z <= charge are skipped")
    ap.add_argument("--orbitals", action="store_true",
                    help="add <r> and r_peak of every atom's outermost level (the last of its alpha levels) to its row: Scf.orbital_properties()")
    ap.add_argument("--exx", action="store_true",
                    help="add the Hartree energy E_H, the exact-exchange (Hartree-Fock) energy of the Kohn-Sham orbitals and the functional's "
                         "own exchange-correlation energy to every atom's row: Scf.coulomb_exchange()")
    ap.add_argument("--kli", action="store_true",
                    help="add E_x = 1/2 Sum n <a|v_x^HF|a> and r vKLI at the outermost node of the density (alpha channel) to every atom's row: "
                         "Scf.exchange_potentials()")
    ap.add_argument("--form-factors", action="store_true",
                    help="after the table, every atom's X-ray form factor f(q) at s = sin(theta)/lambda = 0 .. 2 1/Angstrom in 41 points "
                         "(q = 4 pi s 0.529177210903 a.u.; LSDA adds f_a - f_b), one launch per shard: Scf.form_factors()")
    ap.add_argument("--photo", action="store_true",
                    help="after the table, the photoionization cross section (megabarn) of every atom's outermost subshell at the photoelectron "
                         "energies 0.25, 0.5 .. 2 Ha, one launch per atom: Scf.photoionization()")
    ap.add_argument("--pseudo", action="store_true",
                    help="after the table, the Troullier-Martins pseudopotentials of every atom's default valence levels, all atoms of a rank in one "
                         "call: r_c, a2, E_KB and the norm residual per channel (LDA / GGA only): Scf.pseudopotentials()")
    ap.add_argument("--ghosts", action="store_true",
                    help="after the table, the Kleinman-Bylander ghost report of those pseudopotentials (the highest l local): E_KB, the bound "
                         "states of H_KB and both verdicts per non-local channel: Scf.kb_ghost_report()")
    ap.add_argument("--lsda", action="store_true", help="spin-polarised (LSDA) instead of LDA")
    ap.add_argument("--ionization", action="store_true",
                    help="first ionization energies: the neutral atom and the +1 cation of every Z of a rank's shard advance in one batch; "
                         "IE = E(+1) - E(0) per Z (H+ has no electron: E = 0)")
    args = ap.parse_args()

    import numpy as np
    import torch
    import torch.distributed as dist
    import dftatom_amd as D
    from dftatom_amd import sweep

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    # DFTA_BENCH_SHARED_GPU=1 (tests on a one-GPU box): every rank on device 0, records gathered over gloo from host memory
    shared = world > 1 and os.environ.get("DFTA_BENCH_SHARED_GPU") == "1"
    if shared:
        local = 0
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group("gloo")
    elif world > 1:
        dist.init_process_group("nccl", device_id=torch.device("cuda", local))
    torch.cuda.set_device(local)
    ctx = D.Context(local, torch.cuda.current_stream().cuda_stream)
    delta, rmax = {14: (5e-4, 25.0), 17: (1e-4, 50.0)}.get(args.levels, (1e-4, 50.0))
    grid = D.Grid(ctx, args.levels, delta, rmax)

    Zs = [z for z in range(args.zmin, args.zmax + 1) if z > args.charge]
    cost = sweep.atom_cost if args.partition == "work" else None
    modes = dict(sweep_mode=D.SWEEPS_TOLERANCE if args.sweeps == "tolerance" else D.SWEEPS_EXACT,
                 poisson_mode={"tolerance": D.POISSON_TOLERANCE, "adaptive": D.POISSON_ADAPTIVE}.get(args.poisson, D.POISSON_EXACT),
                 functional={"vwn": D.XC_VWN, "pw92": D.XC_PW92, "pbe": D.XC_PBE}[args.xc],
                 mixing=D.MIX_ANDERSON if args.mixing == "anderson" else D.MIX_LINEAR)
    model = "tolerance" if args.sweeps == "tolerance" else "exact"
    if cost is None and model != "exact":
        cost_model = model
    else:
        cost_model = "exact"
    if args.emulate_ranks > 0:
        # the N shards of an N-rank sweep, one at a time on this GPU
        assert world == 1, "--emulate-ranks runs without a launcher"
        N = args.emulate_ranks
        shards = sweep.partition_atoms(Zs, N, cost=cost, model=cost_model)
        rows = []
        for r, zs in enumerate(shards):
            t0 = time.time()
            scf = D.Scf(ctx, grid, zs, lsda=False, **modes)
            steps = 0
            while steps < args.max_steps:
                scf.step(want_stats=False)
                steps += 1
                _, fin = scf.energies()
                if fin.all():
                    break
            ctx.synchronize()
            dt = time.time() - t0
            en, fin = scf.energies()
            scf.close()
            rows.append({"rank": r, "atoms": zs, "steps": steps, "seconds": dt, "finished": int(fin.sum()),
                         "predicted_seconds_model": sweep.shard_time_ms(zs, cost_model) / 1e3,
                         "etotal": {int(z): en[k].Etotal for k, z in enumerate(zs)}})
            print("shard %d/%d: %2d atoms, %3d steps, %.2f s (model %.2f s)" % (r, N, len(zs), steps, dt, rows[-1]["predicted_seconds_model"]), flush=True)
        pred = max(x["seconds"] for x in rows)
        res = {"emulated_ranks": N, "partition": args.partition, "sweeps": args.sweeps, "poisson": args.poisson, "levels": args.levels, "zmin": args.zmin, "zmax": args.zmax,
               "predicted_n_gpu_seconds": pred, "sum_of_shard_seconds": sum(x["seconds"] for x in rows), "shards": rows,
               "note": "PREDICTION from one GPU: every shard run alone; max over shards = wall time of an N-rank sweep up to the final "
                       "all_gather of 64 doubles per atom (microseconds)"}
        print("emulated %d ranks: predicted wall time %.2f s (slowest shard), sum of shards %.2f s" % (N, pred, res["sum_of_shard_seconds"]))
        if args.out:
            with open(args.out, "w") as f:
                json.dump(res, f, indent=1)
        grid.close()
        ctx.close()
        return
    if args.ionization:
        return ionization(args, D, dist, ctx, grid, sweep.partition_atoms(Zs, world, cost=cost, model=cost_model)[rank], modes, world, rank)
    mine = sweep.partition_atoms(Zs, world, cost=cost, model=cost_model)[rank]
    cap = max(len(s) for s in sweep.partition_atoms(Zs, world, cost=cost, model=cost_model))
    t0 = time.time()
    scf = D.Scf(ctx, grid, mine, lsda=args.lsda, charge=args.charge if args.charge else None,
                exchange={"kli": D.EXCHANGE_KLI, "sic": D.EXCHANGE_SIC_KLI}.get(args.exchange, D.EXCHANGE_FUNCTIONAL), **modes)
    steps = 0
    while steps < args.max_steps:
        scf.step(want_stats=False)
        steps += 1
        _, fin = scf.energies()
        if fin.all():
            break
    if args.exchange != "functional" and not fin.all():
        print("rank %d: not finished after %d steps under --exchange %s: Z = %s"
              % (rank, steps, args.exchange, [int(z) for z, f in zip(mine, fin) if not f]),
              flush=True)
    outer = {}
    if args.orbitals:                           # one launch for every orbital of this rank's batch; the row of each atom's outermost level
        props, jobs = scf.orbital_properties()
        for row, (a, spin, n, l) in enumerate(jobs):
            if spin == 0:                       # jobs are sorted by (n, l) within a channel: the last alpha row of an atom stays
                outer[int(mine[a])] = {"n": n + 1, "l": l, "r_mean": float(props[row, D.ORB_R1]), "r_peak": float(props[row, D.ORB_RPEAK])}
        if world > 1:
            parts = [None] * world
            dist.all_gather_object(parts, outer)
            outer = {z: v for p in parts for z, v in p.items()}
    exx = {}
    if args.exx:                                # one launch per atom: F^0 of all its shell pairs and the G^k of each channel
        en, _ = scf.energies()
        for a, z in enumerate(mine):
            eh, ex = scf.coulomb_exchange(a)
            exx[int(z)] = {"E_H": eh, "E_x_EXX": ex, "E_xc": en[a].Exc}
        if world > 1:
            parts = [None] * world
            dist.all_gather_object(parts, exx)
            exx = {z: v for p in parts for z, v in p.items()}
    kli = {}
    if args.kli:                                # per channel the y rows, the pointwise pass and the reductions; r of the grid for the tail
        r = grid.r()
        for a, z in enumerate(mine):
            ex, tail = 0.0, None
            for spin in ((0, 1) if args.lsda else (0,)):
                p = scf.exchange_potentials(a, spin)
                if p is None:
                    continue
                half = float(np.sum(p["occ"] * p["vbar"][:, D.XP_HF]))
                ex += 0.5 * half if args.lsda else half
                if spin == 0:
                    i = int(np.nonzero(p["D"] > 0)[0][-1])
                    tail = float(r[i] * p["vKLI"][i])
            kli[int(z)] = {"E_x_from_vbarHF": ex, "r_vKLI_tail": tail}
        if world > 1:
            parts = [None] * world
            dist.all_gather_object(parts, kli)
            kli = {z: v for p in parts for z, v in p.items()}
    ff = {}
    ff_s = [2.0 * k / 40 for k in range(41)]    # sin(theta) / lambda in 1 / Angstrom, as dftatom_cli --form-factor-table
    if args.form_factors:                       # one launch for every density of this rank's batch
        f = scf.form_factors([((4.0 * math.pi) * s) * 0.529177210903 for s in ff_s])
        for a, z in enumerate(mine):
            ff[int(z)] = {"f": f[a, 0].tolist(), **({"fa_minus_fb": (f[a, 1] - f[a, 2]).tolist()} if args.lsda else {})}
        if world > 1:
            parts = [None] * world
            dist.all_gather_object(parts, ff)
            ff = {z: v for p in parts for z, v in p.items()}
    photo = {}
    photo_eps = [0.25 * k for k in range(1, 9)]
    if args.photo:                              # per atom one launch: the trials (spin, l' = 0 .. 4, eps) with the dipole sums of its subshells
        for a, z in enumerate(mine):
            ph = scf.photoionization(photo_eps, atom=a)
            nalpha = sum(1 for j in ph["jobs"] if j[0] == 0)
            sp, n, l = ph["jobs"][nalpha - 1]   # the last alpha level: the outermost subshell
            photo[int(z)] = {"n": n + 1, "l": l, "omega": ph["omega"][nalpha - 1].tolist(), "sigma_Mb": (ph["sigma"][nalpha - 1] * 28.002852).tolist()}
        if world > 1:
            parts = [None] * world
            dist.all_gather_object(parts, photo)
            photo = {z: v for p in parts for z, v in p.items()}
    pseudo = {}
    if args.pseudo and not args.lsda and args.exchange == "functional":      # every channel of this rank's batch in one call
        ps = scf.pseudopotentials()
        for k in range(len(ps["atom"])):
            lv = scf.levels(int(ps["atom"][k]), 0)
            pseudo.setdefault(int(mine[ps["atom"][k]]), []).append(
                {"n": int(lv["n"][ps["level"][k]]) + 1, "l": int(ps["l"][k]), "status": int(ps["status"][k]), "rc": float(ps["rc"][k]),
                 "a2": float(ps["coef"][k][1]), "E_KB": float(ps["kb"][k][2]), "norm_residual": float(ps["match"][k][7])})
        if world > 1:
            parts = [None] * world
            dist.all_gather_object(parts, pseudo)
            pseudo = {z: v for p in parts for z, v in p.items()}
    ghosts = {}
    if args.ghosts and not args.lsda and args.exchange == "functional":      # every non-local channel of this rank's batch: one search
        rep, ps = scf.kb_ghost_report()
        for k in range(len(ps["atom"])):
            if rep["direct"][k] < 0 or ps["status"][k]:
                continue                            # the local channel; a channel that was not pseudized
            lv = scf.levels(int(ps["atom"][k]), 0)
            ghosts.setdefault(int(mine[ps["atom"][k]]), []).append(
                {"n": int(lv["n"][ps["level"][k]]) + 1, "l": int(ps["l"][k]), "eps": float(rep["eps_ref"][k]), "E_KB": float(rep["E_KB"][k]),
                 "bound": [float(e) for e in rep["bound"][k]], "gks": int(rep["gks"][k]), "direct": int(rep["direct"][k])})
        if world > 1:
            parts = [None] * world
            dist.all_gather_object(parts, ghosts)
            ghosts = {z: v for p in parts for z, v in p.items()}
    block = torch.zeros((cap, D.RECORD_DOUBLES), dtype=torch.float64, device="cuda")
    scf.records_into(block.data_ptr())          # rows beyond len(mine) stay zero (Z = 0: no atom)
    ctx.synchronize()
    table = sweep.gather_records(block.cpu() if shared else block, dist if world > 1 else None)
    elapsed = time.time() - t0
    if rank == 0:
        rows = [sweep.record_fields(table[z]) for z in sorted(table)]
        for r in rows:
            ref = NIST_LDA.get(r["Z"])
            o = outer.get(r["Z"])
            x = exx.get(r["Z"])
            kl = kli.get(r["Z"])
            print("Z %3d  Etotal %16.6f  steps %3d  finished %d%s%s%s%s" % (r["Z"], r["Etotal"], r["steps"], r["finished"],
                  "   %d%s <r> %.4f r_peak %.4f" % (o["n"], "spdf"[o["l"]], o["r_mean"], o["r_peak"]) if o else "",
                  "   E_H %.6f E_x(EXX) %.6f E_xc %.6f" % (x["E_H"], x["E_x_EXX"], x["E_xc"]) if x else "",
                  "   E_x(vbarHF) %.6f r*vKLI %.6f" % (kl["E_x_from_vbarHF"], kl["r_vKLI_tail"]) if kl else "",
                  "   NIST LDA %.6f (diff %.1e)" % (ref, r["Etotal"] - ref) if ref else ""))
        for r in rows:                          # the table of dftatom_cli --form-factor-table, per atom
            t = ff.get(r["Z"])
            if t:
                for k, s in enumerate(ff_s):
                    print("Z %3d  FormFactor s = %.6f q = %.6f f = %.6f%s" % (r["Z"], s, ((4.0 * math.pi) * s) * 0.529177210903, t["f"][k],
                          " fa-fb = %.6f" % t["fa_minus_fb"][k] if "fa_minus_fb" in t else ""))
        for r in rows:                          # sigma_nl(omega) of the outermost subshell, per atom
            t = photo.get(r["Z"])
            if t:
                for om, sg in zip(t["omega"], t["sigma_Mb"]):
                    print("Z %3d  Photo %d%s omega = %.6f sigma = %.6f Mb" % (r["Z"], t["n"], "spdf"[t["l"]], om, sg))
        for r in rows:                          # the pseudopotential of every default valence level, per atom
            for t in pseudo.get(r["Z"], []):
                print("Z %3d  Pseudo %d%s status = %d rc = %.6f a2 = %.6f EKB = %.6f norm = %.2e"
                      % (r["Z"], t["n"], "spdfg"[t["l"]], t["status"], t["rc"], t["a2"], t["E_KB"], t["norm_residual"]))
        for r in rows:                          # the ghost report of every non-local channel, per atom
            for t in ghosts.get(r["Z"], []):
                print("Z %3d  Ghost %d%s eps = %.6f EKB = %.6f states = %s GKS = %d direct = %d%s"
                      % (r["Z"], t["n"], "spdfg"[t["l"]], t["eps"], t["E_KB"], " ".join("%.6f" % e for e in t["bound"]), t["gks"], t["direct"],
                         "  DISAGREE" if t["gks"] != t["direct"] else ""))
        print("%d atoms, %d GPU(s), %d SCF steps of the longest-running atom of rank 0, %d atom-steps in all, %d finished, %.1f s"
              % (len(rows), world, steps, sum(r["steps"] for r in rows), sum(r["finished"] for r in rows), elapsed))
        if args.out:
            with open(args.out, "w") as f:
                json.dump({"n_gpus": world, "levels": args.levels, "steps": steps, "seconds": elapsed,
                           "atoms": [dict({"Z": r["Z"], "Etotal": r["Etotal"], "steps": r["steps"], "finished": r["finished"]},
                                          **({"outermost": outer[r["Z"]]} if r["Z"] in outer else {}),
                                          **({"exx": exx[r["Z"]]} if r["Z"] in exx else {}),
                                          **({"kli": kli[r["Z"]]} if r["Z"] in kli else {}),
                                          **({"form_factor": ff[r["Z"]]} if r["Z"] in ff else {}),
                                          **({"photoionization": photo[r["Z"]]} if r["Z"] in photo else {}),
                                          **({"pseudopotential": pseudo[r["Z"]]} if r["Z"] in pseudo else {}),
                                          **({"ghosts": ghosts[r["Z"]]} if r["Z"] in ghosts else {})) for r in rows]},
                          f, indent=1)
    scf.close()
    grid.close()
    ctx.close()
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


def ionization(args, D, dist, ctx, grid, mine, modes, world, rank):
    """neutral atoms and +1 cations of this rank's Z in ONE batch; results are matched to (Z, charge) by the batch's own order"""
    HARTREE_EV = 27.211386245988
    t0 = time.time()
    Z = list(mine) + [z for z in mine if z > 1]
    charge = [0] * len(mine) + [1] * (len(Z) - len(mine))
    scf = D.Scf(ctx, grid, Z, lsda=args.lsda, charge=charge, **modes)
    steps = 0
    while steps < args.max_steps:
        scf.step(want_stats=False)
        steps += 1
        if scf.energies()[1].all():
            break
    en, fin = scf.energies()
    scf.close()
    E = {(z, q): (en[k].Etotal, int(fin[k])) for k, (z, q) in enumerate(zip(Z, charge))}
    rows = {z: {"Z": z, "E0": E[(z, 0)][0], "E1": E[(z, 1)][0] if z > 1 else 0.0,
                "finished": E[(z, 0)][1] and (E[(z, 1)][1] if z > 1 else 1)} for z in mine}
    for r in rows.values():
        r["IE_Ha"] = r["E1"] - r["E0"]
        r["IE_eV"] = r["IE_Ha"] * HARTREE_EV
    if world > 1:
        parts = [None] * world
        dist.all_gather_object(parts, rows)
        rows = {z: r for p in parts for z, r in p.items()}
    elapsed = time.time() - t0
    if rank == 0:
        for z in sorted(rows):
            r = rows[z]
            print("Z %3d  E(0) %16.6f  E(+1) %16.6f  IE %10.6f Ha = %8.3f eV  finished %d" % (z, r["E0"], r["E1"], r["IE_Ha"], r["IE_eV"], r["finished"]))
        print("%d atoms + %d cations in one batch per rank, %d GPU(s), %d SCF steps (rank 0), %.1f s"
              % (len(rows), sum(1 for z in rows if z > 1), world, steps, elapsed))
        if args.out:
            with open(args.out, "w") as f:
                json.dump({"n_gpus": world, "levels": args.levels, "lsda": args.lsda, "steps": steps, "seconds": elapsed,
                           "ionization": [rows[z] for z in sorted(rows)]}, f, indent=1)
    grid.close()
    ctx.close()
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
