#!/usr/bin/env python3
"""Writes tests/golden/optimizer_replay_cases.json: the cases of the teacher-forced optimizer replay (tests/bfgs_replay.py).

Everything in the fixture comes from the reference alone (oracle/bfgs_port.py on the fp64 oracles), nothing from a device:

  * the case list per group: gate, span, objective, flags, maxiter, target and start-point seeds (o.haar_unitary(5000 + t),
    o.x0_philox(3, t, r, k));
  * per group the yardstick ``e_ref``: the worst step deviation over the group's clear steps when the replay with a FLOAT64 metric
    is teacher-forced along the float32 port's own trajectory -- the effect of float32 rounding of the metric;
  * per group the port's branch census and the replay's count of unclear steps and items (and, for the noise-floor group, the
    shortest clear prefix);
  * per item the port's iters, evals, status and the criterion that ended it.

    python tools/make_replay_cases.py            # rewrites the fixture
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import bfgs_replay as br  # noqa: E402

SQ, WEAK, QUARTER = ["riswap", 0.5], ["riswap", 0.125], ["riswap", 0.25]
CG = ["cg", 0.3, -0.7, 0.9, 0.4, 1.0]


def _case(name, gate, k, items, cost="basic", flags=0, maxiter=2500, target="haar", hp_gate=None, trace_cap=128, nan_target=False):
    c = {"name": name, "gate": gate, "k": k, "cost": cost, "flags": flags, "maxiter": maxiter, "target": target, "hp_gate": hp_gate,
         "trace_cap": trace_cap, "items": [list(i) for i in items]}
    if nan_target:
        c["nan_target"] = True
    return c


# (t, r) per case: picked with the port alone so that the group takes the branches named in DESIGN.md ("Optimizer replay")
GROUPS = {
    "ordinary": [
        _case("cx-k1", ["cx"], 1, [(0, 0)], hp_gate="cx"),
        _case("cx-k2", ["cx"], 2, [(0, 0)], hp_gate="cx"),          # ten back-tracks, growth to 64, the far criterion
        _case("cx-k3", ["cx"], 3, [(0, 0), (1, 0)], hp_gate="cx"),
        _case("sqiswap-k1", SQ, 1, [(33, 2)], hp_gate="sqiswap"),   # growth to 512
        _case("sqiswap-k2", SQ, 2, [(2, 1)], hp_gate="sqiswap"),    # 92 iterations below the span
        _case("sqiswap-k3", SQ, 3, [(0, 0), (1, 0)], hp_gate="sqiswap"),
        _case("dense-k2", ["dense", 31337], 2, [(0, 0)], hp_gate="dense"),
        _case("cg-phases-k2", CG, 2, [(1, 0)]),
        _case("sqiswap-k4", SQ, 4, [(0, 0)], hp_gate="sqiswap"),
        _case("sqiswap-k5", SQ, 5, [(1, 0)], hp_gate="sqiswap"),
    ],
    "restarted": [
        _case("weak-k3", WEAK, 3, [(24, 3), (30, 1), (30, 3), (38, 0), (39, 2)], trace_cap=512),
        _case("weak-k5", WEAK, 5, [(0, 0), (9, 0), (28, 0)], trace_cap=512),  # (28, 0): 333 iterations, two restarts
    ],
    "noise_floor": [
        _case("sqiswap-k3-swap", SQ, 3, [(0, 1), (1, 0), (1, 1), (2, 2), (3, 0), (3, 2)], target="swap", hp_gate="sqiswap"),
        # a target just outside what two CX reach (c3 = 1e-4 off the chamber's floor): the minimum's loss lies between stop_loss and
        # far_loss, so |g| < gtol is the criterion that fires -- after steps whose decrease is below the loss band
        _case("cx-k2-floor", ["cx"], 2, [(0, 0)], target=["canonical", 0.3, 0.2, 1e-4], hp_gate="cx"),
    ],
    "long": [
        _case("quarter-k6", QUARTER, 6, [(0, 0), (1, 0)]),
        _case("weak-k7", WEAK, 7, [(1, 0), (2, 0)], trace_cap=512),  # (2, 0): 241 iterations, one restart
    ],
    "other": [
        _case("sqiswap-k3-no-exterior", SQ, 3, [(0, 0), (1, 0)], flags=br.FLAG_NO_EXTERIOR, hp_gate="sqiswap"),
        _case("sqiswap-k2-square", SQ, 2, [(0, 0), (2, 0)], cost="square", hp_gate="sqiswap"),
        _case("dense-k2-makhlin", ["dense", 31337], 2, [(1, 0), (2, 0)], cost="makhlin", hp_gate="dense"),
        _case("sqiswap-k2-maxiter5", SQ, 2, [(0, 0), (1, 0)], maxiter=5, hp_gate="sqiswap"),
        _case("sqiswap-k2-nan", SQ, 2, [(0, 0)], hp_gate="sqiswap", nan_target=True),
    ],
}


def port_census(records):
    """Branch counts of a list of port records (one list of per-step dicts + the end dict per item)."""
    c = {"steps": 0, "backtracks": 0, "short": 0, "skipped": 0, "first_scaling": 0, "nondescent": 0, "max_grow": 1.0,
         "restarts_per_item": [], "ends": {}}
    for rec in records:
        steps, end = rec[:-1], rec[-1]
        c["steps"] += len(steps)
        c["backtracks"] += sum(len(s["trials"]) - 1 for s in steps) + len(end["trials"])
        c["short"] += sum(s["short"] for s in steps)
        c["skipped"] += sum(not s["updated"] for s in steps)
        c["first_scaling"] += sum(s["first_scaling"] for s in steps)
        c["nondescent"] += sum(s["nondescent"] for s in steps)
        c["max_grow"] = max([c["max_grow"]] + [float(s["grow"]) for s in steps])
        c["restarts_per_item"].append(sum(s["periodic"] for s in steps))
        c["ends"][end["end"]] = c["ends"].get(end["end"], 0) + 1
    return c


def generate(name):
    """One group of the fixture, from the reference alone."""
    cases, records, replays = [], [], []
    for case in GROUPS[name]:
        case = json.loads(json.dumps(case))
        port = []
        for t, r in case["items"]:
            f, x, it, st, nev, xs, rec = br.run_port(case, t, r)
            port.append([int(it), int(nev), int(st), rec[-1]["end"]])
            records.append(rec)
            replays.append(br.replay_item(case, t, r, xs, h_dtype=np.float64))
        case["port"] = port
        cases.append(case)
    cen = br.census(replays)
    group = {"cases": cases, "e_ref": br.worst_clear(replays), "census": port_census(records), "unclear_steps": cen["unclear"],
             "unclear_items": cen["items_unclear"], "replayed_steps": cen["steps"]}
    if name == "noise_floor":
        group["min_clear_prefix"] = min(len(r["dev"]) for r in replays)
    return group


def main():
    fixture = {"groups": {name: generate(name) for name in GROUPS}}
    for name, g in fixture["groups"].items():
        print(f"{name:12s} items {sum(len(c['items']) for c in g['cases']):3d}  steps {g['replayed_steps']:5d}  unclear {g['unclear_steps']:3d}"
              f" (items {g['unclear_items']})  e_ref {g['e_ref']:.2e}  tol {br.tolerance(g['e_ref']):.2e}  census {g['census']}")
    with open(br.FIXTURE, "w") as fh:
        json.dump(fixture, fh, indent=1, sort_keys=True)
        fh.write("\n")


if __name__ == "__main__":
    main()
