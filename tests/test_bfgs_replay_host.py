"""Host: the teacher-forced optimizer replay (tests/bfgs_replay.py) and its cases, from the reference alone -- no GPU.

  * oracle/bfgs_port.py with its recording outputs returns what the port returned before it had them, bit for bit;
  * tests/golden/optimizer_replay_cases.json is what tools/make_replay_cases.py produces;
  * the case list takes every branch of the iteration it claims to take (census), few of its decisions are unclear (caps), and every
    tolerance min(8 e_ref, 1e-2) is a measured 8 e_ref;
  * replayed along the float32 port's own trajectories, the replay predicts the port's iters, evals and status and stays inside the
    tolerance;
  * a port with one constant or rule changed is rejected: some clear step of some group leaves the tolerance.
"""
import functools
import hashlib
import json
import os
import sys

import numpy as np
import pytest

import bfgs_replay as br
from oracle import bfgs_port as bp
from oracle import slam_oracle as o

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import make_replay_cases as mk  # noqa: E402

FIX = br.load_fixture()["groups"]
GROUPS = ("ordinary", "restarted", "noise_floor", "long", "other")
PINNED = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bfgs_port_pinned.json")


def _items(group):
    for case in FIX[group]["cases"]:
        for (t, r), port in zip(case["items"], case["port"]):
            yield case, t, r, port


@functools.lru_cache(maxsize=None)
def _self_replay(group):
    """[(case, t, r, port row, replay result)]: the float32 replay along the float32 port's own trajectory."""
    out = []
    for case, t, r, port in _items(group):
        f, x, it, st, nev, xs, rec = br.run_port(case, t, r)
        assert [it, nev, st, rec[-1]["end"]] == port, (case["name"], t, r)
        out.append((case, t, r, port, br.replay_item(case, t, r, xs)))
    return out


def test_the_recording_port_is_the_port_bit_for_bit():
    """On the cases of test_gpu_minimize_parity.py::test_full_runs_follow_cpu_port (Haar targets of seed 777, start points of seed
    11, 6 x 4 items each): loss, final point, iters, status and evals as golden/bfgs_port_pinned.json holds them, written by the port
    before it had its recording outputs -- with the outputs on, and (first case) with them off."""
    with open(PINNED) as fh:
        pinned = json.load(fh)
    gates = {"cx": o.cx_matrix(), "sqiswap": o.riswap_matrix(0.5), "b": o.berkeley_matrix(), "dense": o.haar_unitary(31337),
             "cg-phases": o.conversion_gain_matrix(0.3, -0.7, 0.9, 0.4, 1.0)}
    targets = o.haar_batch(6, seed0=777)
    assert len(pinned) == 7
    for ci, (key, rows) in enumerate(sorted(pinned.items())):
        name, k = key.rsplit("-k", 1)
        k = int(k)
        for i, row in enumerate(rows):
            t, r = divmod(i, 4)
            x0 = o.x0_philox(11, t, r, k)
            xs, rec, trace = [], [], []
            f, x, it, st, nev = bp.minimize_port(x0, [gates[name]] * k, targets[t], xs=xs, record=rec, trace=trace)
            got = [float(f).hex(), hashlib.sha256(np.ascontiguousarray(x).tobytes()).hexdigest()[:16], int(it), int(st), int(nev)]
            assert got == row, (key, t, r)
            assert len(xs) == it and len(rec) == it + 1 and (it == 0 or np.array_equal(xs[-1], x))
            assert sum(len(s["trials"]) for s in rec) + 1 == nev and all(s["trials"][-1][1] <= 0 for s in rec[:-1])
            if ci == 0:
                f2, x2, it2, st2, nev2 = bp.minimize_port(x0, [gates[name]] * k, targets[t])
                assert (float(f2).hex(), it2, st2, nev2) == (got[0], it, st, nev) and np.array_equal(x2, x)


@pytest.mark.parametrize("group", ["long", "other"])
def test_the_fixture_is_what_the_generator_produces(group):
    assert json.loads(json.dumps(mk.generate(group))) == FIX[group]
    assert set(mk.GROUPS) == set(FIX) == set(GROUPS)


def test_census_the_case_list_takes_the_branches_it_claims():
    cen = {g: FIX[g]["census"] for g in GROUPS}
    for g in GROUPS:
        assert 1 <= sum(len(c["items"]) for c in FIX[g]["cases"]) <= 12, g
        assert cen[g]["backtracks"] > 0 and cen[g]["short"] > 0 and cen[g]["skipped"] > 0 and cen[g]["first_scaling"] > 0, g
    restarts = [n for g in GROUPS for n in cen[g]["restarts_per_item"]]
    assert sum(n == 1 for n in restarts) >= 5 and sum(n >= 2 for n in restarts) >= 1
    assert max(cen["restarted"]["restarts_per_item"]) == 2 and min(cen["restarted"]["restarts_per_item"]) >= 1
    assert max(cen["long"]["restarts_per_item"]) >= 1  # the periodic restart of slam_long_minimize.inc
    # growth: up to 64 in general, 512 at sqrt(iSWAP) k = 1
    assert cen["ordinary"]["max_grow"] == 512.0
    sq1 = next(c for c in FIX["ordinary"]["cases"] if c["name"] == "sqiswap-k1")
    rec = br.run_port(sq1, *sq1["items"][0])[6]
    assert max(s["grow"] for s in rec[:-1]) == 512.0
    # every way a run ends that an input is known for
    ends = {}
    for g in GROUPS:
        for e, n in cen[g]["ends"].items():
            ends[e] = ends.get(e, 0) + n
    assert set(ends) == {bp.END_STOP_LOSS, bp.END_GTOL, bp.END_FAR, bp.END_MAXITER, bp.END_STALL, bp.END_NONFINITE}, ends
    status = {row[2] for g in GROUPS for c in FIX[g]["cases"] for row in c["port"]}
    assert status == {br.ST_CONVERGED, br.ST_MAXITER, br.ST_STALLED, br.ST_NONFINITE}
    assert cen["ordinary"]["ends"].get(bp.END_FAR, 0) >= 1 and cen["ordinary"]["ends"].get(bp.END_STOP_LOSS, 0) >= 1
    stalled = [row[2] == br.ST_STALLED for c in FIX["noise_floor"]["cases"] for row in c["port"]]
    assert 3 * sum(stalled) >= len(stalled) - 1  # about a third of the noise-floor items stall
    # all three gate-class code paths of the short kernels, both long spans, the other instantiations
    names = {c["name"] for g in GROUPS for c in FIX[g]["cases"]}
    assert {"cx-k1", "cx-k2", "cx-k3", "sqiswap-k1", "sqiswap-k2", "sqiswap-k3", "sqiswap-k4", "sqiswap-k5", "dense-k2", "cg-phases-k2",
            "quarter-k6", "weak-k7", "sqiswap-k3-no-exterior", "sqiswap-k2-square", "dense-k2-makhlin", "sqiswap-k2-maxiter5",
            "sqiswap-k2-nan"} <= names
    # branches no input is known for (DESIGN.md names them): if one turns up, the documents are to say so
    assert all(cen[g]["nondescent"] == 0 for g in GROUPS) and bp.END_BACKTRACK not in ends


def test_caps_few_decisions_are_unclear_and_every_tolerance_is_measured():
    for g in GROUPS:
        grp = FIX[g]
        n_items = sum(len(c["items"]) for c in grp["cases"])
        assert 0.0 < grp["e_ref"] and br.TOL_FACTOR * grp["e_ref"] < br.TOL_CAP, g
        assert br.tolerance(grp["e_ref"]) == br.TOL_FACTOR * grp["e_ref"]
        assert grp["unclear_steps"] <= 0.02 * grp["replayed_steps"], g
        if g == "noise_floor":
            # every item has a clear prefix; the shortest the generator measured is 39 steps (cx-k2-floor), 55 on SWAP
            assert grp["min_clear_prefix"] >= 39
        else:
            assert n_items - grp["unclear_items"] >= 0.9 * n_items, g
    for g in GROUPS:  # the bands come from hp_ref alone and stay below twice its cap
        for c in FIX[g]["cases"]:
            bf, bg = br.bands(c)
            assert 0.0 < bf <= 2e-13 and bf == bg


@pytest.mark.parametrize("group", GROUPS)
def test_self_replay_predicts_the_port(group):
    tol = br.tolerance(FIX[group]["e_ref"])
    res = _self_replay(group)
    worst = br.worst_clear([r[4] for r in res])
    cen = br.census([r[4] for r in res])
    print(f"REPLAY host {group:12s} steps {cen['steps']:5d} unclear {cen['unclear']:3d} worst {worst:9.2e} tol {tol:9.2e}")
    assert worst <= tol
    for case, t, r, port, rp in res:
        assert max(rp["dev"], default=0.0) <= tol, (case["name"], t, r)  # unclear steps too: the branch followed has to match
        if not rp["item_unclear"]:
            assert [rp["iters"], rp["evals"], rp["status"], rp["end"]] == port, (case["name"], t, r)
        else:
            assert rp["noise_from"] is not None or rp["iters"] == port[0], (case["name"], t, r)
    if group != "noise_floor":
        assert cen["unclear"] <= 0.02 * cen["steps"] and cen["items_unclear"] <= 0.1 * len(res)
    else:
        assert all(r[4]["noise_from"] is not None and r[4]["noise_from"] >= FIX[group]["min_clear_prefix"] for r in res)


def _first_failure(group, names=None, cut=None):
    """The first clear step outside the group's tolerance when the (patched) port's trajectories are replayed by the healthy replay."""
    tol = br.tolerance(FIX[group]["e_ref"])
    for case, t, r, port in _items(group):
        if names is not None and case["name"] not in names:
            continue
        xs = br.run_port(case, t, r)[5][:cut]
        rp = br.replay_item(case, t, r, xs)
        for j, (d, u) in enumerate(zip(rp["dev"], rp["unclear"])):
            if d > tol and not u:
                return case["name"], (t, r), j, d
    return None


@functools.lru_cache(maxsize=None)
def _healthy(group, names, cut):
    return _first_failure(group, names, cut)


DEFECTS = {
    "GROW_FACTOR 4": ("GROW_FACTOR", 4.0, "ordinary", None, None),
    "RESTART_PERIOD 256": ("RESTART_PERIOD", 256, "restarted", ("weak-k3",), 136),
    "WOLFE_C2 0.9": ("WOLFE_C2", 0.9, "ordinary", None, None),
    "back-track clamp 0.2": ("BACKTRACK_MIN", 0.2, "ordinary", None, None),
    "no first-update scaling": ("FIRST_SCALING", False, "ordinary", None, None),
    "update from too-short steps": ("SKIP_SHORT_UPDATES", False, "ordinary", None, None),
    "STEP_MAX 1": ("STEP_MAX", 1.0, "ordinary", None, None),
}


@pytest.mark.parametrize("defect", sorted(DEFECTS))
def test_a_planted_defect_fails_a_clear_step(monkeypatch, defect):
    attr, value, group, names, cut = DEFECTS[defect]
    assert _healthy(group, names, cut) is None  # the healthy port passes where the defect is looked for
    monkeypatch.setattr(bp, attr, value)
    hit = _first_failure(group, names, cut)
    print(f"REPLAY planted {defect}: {hit}")
    assert hit is not None and hit[3] >= 0.05, defect  # (a wrong branch moves a step by tenths, not by a tolerance's worth)


def test_an_unclear_armijo_margin_is_followed_on_both_branches():
    """A loss band just wide enough to swallow the margin of a refused trial: the replay lists that trial as a candidate, goes on
    back-tracking as the port did, matches the observed step with the later candidate and marks the step and the item unclear."""
    tol = br.tolerance(FIX["ordinary"]["e_ref"])
    seen = 0
    for case, t, r, port in _items("ordinary"):
        xs, rec = br.run_port(case, t, r)[5:7]
        floor = np.inf  # the smallest accepted decrease so far bounds the band from above (a wider one starts the noise floor)
        for j, s in enumerate(rec[:-1]):
            floor = min(floor, -s["trials"][-1][1])
            refused = [m for _, m in s["trials"][:-1] if 1.01 * m < floor]
            if refused:
                k = case["k"]
                rp = br.replay(br.objective(case), [br.gate_matrix(case["gate"])] * k, br.target_matrix(case, t),
                               br.start_point(case, t, r), xs[:j + 1], (1.01 * min(refused), br.bands(case)[1]))
                assert len(rp["dev"]) == j + 1 and rp["unclear"][j] and rp["item_unclear"] and max(rp["dev"]) <= tol
                assert rp["steps"][j]["n_back"] == len(s["trials"]) - 1
                seen += 1
                break
    assert seen >= 3
