#!/usr/bin/env python3
"""Writes tests/golden/q3_replay_cases.json: the cases of the three-qubit optimizer replay (tests/q3_replay_cases.py).

Everything in the fixture comes from the models alone (oracle/bfgs_port.py on tests/q3_ref.py and tests/q3m_ref.py), nothing from a
device, and it holds no matrices: templates, targets and start points by name and seed, per item the port's iters, evals, status and
the criterion that ended it, per group the yardstick ``e_ref`` (the worst deviation over the clear steps of the FLOAT64-metric
replay along the float32 port's own trajectory), the port's branch census and the replay's count of unclear steps and items.

Every start point has BasicCost <= 0.95 (overlap >= 0.05, the floor under which the evaluation kernels' parity bounds were not
measured); accepted steps only lower the loss, so the whole trajectory keeps that floor.  ``generate`` asserts it.

    python tools/make_q3_replay_cases.py            # rewrites the fixture
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import bfgs_replay as br  # noqa: E402
import q3_ref  # noqa: E402
import q3_replay_cases as qc  # noqa: E402
from make_replay_cases import port_census  # noqa: E402


def _case(name, template, items, cost="basic", maxiter=2500, nan_target=False):
    c = {"name": name, "template": template, "cost": cost, "maxiter": maxiter, "items": items}
    if nan_target:
        c["nan_target"] = True
    return c


def _parity(ms):
    return [[["parity", m], ["parity", m]] for m in ms]


def _seeded(target, seeds):
    return [[list(target), ["uniform", s]] for s in seeds]


# items picked with the port alone (a few dozen candidates per template) so that each group takes the branches DESIGN.md names
GROUPS = {
    "small": [
        # n = 15: one partial row batch; 34..40 iterations, back-tracks, short steps, growth to 64
        _case("table-k1", ["parity", 1], _parity([1, 7, 12, 13])),
        # n = 27, 78 and 80 iterations: ends by stop_loss and by the far criterion
        _case("line-k3", ["line3"], [[["reachable", 7], ["uniform", 4107]], [["reachable", 11], ["uniform", 4111]]]),
    ],
    "toffoli": [
        _case("toffoli-basic", ["toffoli"], _seeded(["ccx"], [4200, 4203, 4211])),              # 4211: the floor 1 - cos(pi/8) of a local minimum
        _case("toffoli-square", ["toffoli"], _seeded(["ccx"], [4200, 4207, 4211]), cost="square"),  # 21 and 24 back-tracks, growth to 64
    ],
    "cap": [
        # n = 99 = 6 row batches of 16 and one of 3; 183 and 256 iterations: one periodic restart each
        _case("table-k15", ["parity", 15], _parity([3, 4])),
    ],
    "mixed": [
        _case("vswap-far", ["vswap"], [[["local", t], ["uniform", 4300 + t]] for t in (2, 5, 6)]),           # n = 33
        _case("ccz-cx-square", ["ccz_cx"], [[["ccz_cx", t], ["uniform", 4400 + t]] for t in (3, 7)], cost="square"),  # n = 24, growth to 512
        _case("ten3", ["ten3"], [[["items", m], ["items", m]] for m in (1, 3)]),                              # n = 99, ten three-qubit positions
    ],
    "other": [
        _case("table-k1-maxiter5", ["parity", 1], _parity([7, 12]), maxiter=5),
        _case("ccz-cx-maxiter5", ["ccz_cx"], [[["ccz_cx", t], ["uniform", 4400 + t]] for t in (1, 4)], maxiter=5),
        _case("line-k3-nan", ["line3"], [[["reachable", 0], ["uniform", 4100]]], nan_target=True),
        _case("line-k3-own", ["line3"], [[["own"], ["uniform", 4500]]]),      # the start point is the solution: converged at iters 0
        _case("ccz-cx-own", ["ccz_cx"], [[["own"], ["uniform", 4501]]]),
        _case("line-k3-local", ["line3"], [[["local", i], ["local", i]] for i in (0, 2, 3)]),  # stop_loss near a solution
        _case("vswap-local", ["vswap"], [[["local", i], ["local", i]] for i in (2, 3)]),
    ],
}


def generate(name):
    """One group of the fixture, from the models alone."""
    cases, records, replays = [], [], []
    for case in GROUPS[name]:
        case = json.loads(json.dumps(case))
        port = []
        for item in case["items"]:
            if not case.get("nan_target"):
                w = qc.template(case).unitary(qc.start_point(case, item))
                assert q3_ref.basic_cost(w, qc.target_matrix(case, item)) <= 1.0 - qc.OVERLAP_FLOOR, (case["name"], item)
            f, x, it, st, nev, xs, rec = qc.port_run(case, item)
            port.append([int(it), int(nev), int(st), rec[-1]["end"]])
            records.append(rec)
            replays.append(qc.replay_item(case, item, xs, h_dtype=np.float64))
        case["port"] = port
        cases.append(case)
    cen = br.census(replays)
    return {"cases": cases, "e_ref": br.worst_clear(replays), "census": port_census(records), "unclear_steps": cen["unclear"],
            "unclear_items": cen["items_unclear"], "replayed_steps": cen["steps"]}


def main():
    fixture = {"groups": {name: generate(name) for name in GROUPS}}
    for name, g in fixture["groups"].items():
        print(f"{name:8s} items {sum(len(c['items']) for c in g['cases']):3d}  steps {g['replayed_steps']:5d}  unclear {g['unclear_steps']:3d}"
              f" (items {g['unclear_items']})  e_ref {g['e_ref']:.2e}  tol {br.tolerance(g['e_ref']):.2e}  census {g['census']}")
    with open(qc.FIXTURE, "w") as fh:
        json.dump(fixture, fh, indent=1, sort_keys=True)
        fh.write("\n")


if __name__ == "__main__":
    main()
