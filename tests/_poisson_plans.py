"""tests/golden/poisson_plans.json (what the last commit before the layout planner decided on an MI355X) expanded from its column layout:
load() -> (header, records), a record being {"in": {...}, "flags": {...}, "alloc": {...}, "soff": n, "desc": {... "cs": [...], "lv": [...]}}."""
import json
import os

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "poisson_plans.json")
FLAGS = ("resident", "res16", "plain_launch", "fault", "tol", "adaptive")
ALLOC = ("level_store", "cur", "group_ctr", "group_part", "res_slots", "res_spill")


def load():
    with open(FIXTURE) as f:
        fx = json.load(f)
    h = fx["header"]
    records = []
    for row in fx["records"]:
        r = dict(zip(h["record_fields"], row))
        p = dict(zip(h["plan_fields"], fx["plans"][r["plan"]]))
        inp = dict(zip(h["grid_fields"], fx["grids"][r["grid"]]))
        inp.update((k, r[k]) for k in h["record_fields"] if k not in ALLOC + ("grid", "plan"))
        desc = {k[2:]: v for k, v in p.items() if k.startswith("D.")}
        desc["cs"], desc["lv"] = fx["cs_tables"][p["cs"]], fx["lv_tables"][p["lv"]]
        records.append({"in": inp, "flags": {k: p[k] for k in FLAGS}, "alloc": {k: r[k] for k in ALLOC}, "soff": p["soff"], "desc": desc})
    return h, records
