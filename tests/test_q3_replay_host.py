"""Host: the cases of the three-qubit optimizer replay (tests/q3_replay_cases.py, tests/golden/q3_replay_cases.json) and what makes
tests/test_gpu_q3_replay.py sound, from the models alone -- no GPU.

  * the fixture is what tools/make_q3_replay_cases.py produces (which asserts the 0.05 overlap floor at every start point);
  * replayed along the float32 port's own trajectories, the replay (tests/bfgs_replay.py, unchanged: it takes the objective and the
    bands as arguments) predicts the port's iters, evals and status and stays inside min(8 e_ref, 1e-2);
  * the case list takes every branch a group claims, few decisions are unclear, every tolerance is a measured 8 e_ref;
  * truncation: ``minimize_port(maxiter = j)`` returns the point after step j of the full run, bit for bit -- the CPU twin of what
    the GPU module's trajectory helper asserts of ``slam_q3_minimize``;
  * a port with one constant or rule changed is rejected: some clear step of some group leaves the tolerance.  The partial-batch
    defect (metric rows >= 96 never updated; n = 99 ends in a batch of three rows) is planted in the port's rank-2 update by zeroing
    those rows of its two outer products.

No ending by ST_STALLED or ST_LINESEARCH was found for these templates: over the 117 candidate items the port was run on while the
cases were chosen (16 + 12 of ``small``, 24 of ``toffoli``, 10 of ``cap``, 32 of ``mixed``, 23 of ``other``) every run ended by
stop_loss, the far criterion, maxiter or a non-finite first evaluation.  The case list holds none.
"""
import functools
import json
import os
import sys

import numpy as np
import pytest

import bfgs_replay as br
import q3_replay_cases as qc
from oracle import bfgs_port as bp

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import make_q3_replay_cases as mk  # noqa: E402

FIX = qc.load_fixture()["groups"]


def _items(group):
    for case in FIX[group]["cases"]:
        for item, port in zip(case["items"], case["port"]):
            yield case, item, port


@functools.lru_cache(maxsize=None)
def _self_replay(group):
    """[(case, item, port row, replay result)]: the float32 replay along the float32 port's own trajectory."""
    out = []
    for case, item, port in _items(group):
        f, x, it, st, nev, xs, rec = qc.port_run(case, item)
        assert [it, nev, st, rec[-1]["end"]] == port, (case["name"], item)
        out.append((case, item, port, qc.replay_item(case, item, xs)))
    return out


@pytest.mark.parametrize("group", qc.GROUPS)
def test_the_fixture_is_what_the_generator_produces(group):
    assert json.loads(json.dumps(mk.generate(group))) == FIX[group]
    assert set(mk.GROUPS) == set(FIX) == set(qc.GROUPS)
    assert os.path.getsize(qc.FIXTURE) < 64 * 1024  # names and seeds, no matrices


@pytest.mark.parametrize("group", qc.GROUPS)
def test_self_replay_predicts_the_port(group):
    tol = br.tolerance(FIX[group]["e_ref"])
    res = _self_replay(group)
    worst = br.worst_clear([r[3] for r in res])
    cen = br.census([r[3] for r in res])
    print(f"REPLAY host {group:8s} steps {cen['steps']:5d} unclear {cen['unclear']:3d} worst {worst:9.2e} tol {tol:9.2e}")
    for case, item, port, rp in res:
        assert max(rp["dev"], default=0.0) <= tol, (case["name"], item)  # unclear steps too: the branch followed has to match
        if not rp["item_unclear"]:
            assert [rp["iters"], rp["evals"], rp["status"], rp["end"]] == port, (case["name"], item)
        else:
            assert rp["noise_from"] is not None or rp["iters"] == port[0], (case["name"], item)
    assert cen["unclear"] <= 0.02 * cen["steps"] and cen["items_unclear"] <= 0.1 * len(res)


def test_census_the_case_list_takes_the_branches_it_claims():
    cen = {g: FIX[g]["census"] for g in qc.GROUPS}
    for g in qc.GROUPS:
        n_run = sum(row[0] > 0 for c in FIX[g]["cases"] for row in c["port"])
        assert cen[g]["backtracks"] > 0 and cen[g]["short"] > 0 and cen[g]["skipped"] > 0, g
        assert cen[g]["first_scaling"] >= n_run, g  # first scaling in every item that takes a step
    assert sum(cen["cap"]["restarts_per_item"]) >= 2 and min(cen["cap"]["restarts_per_item"]) >= 1
    assert all(cen[g]["first_scaling"] == sum(row[0] > 0 for c in FIX[g]["cases"] for row in c["port"]) + sum(cen[g]["restarts_per_item"])
               for g in qc.GROUPS)  # ... and once more after every periodic restart
    assert cen["small"]["max_grow"] >= 64.0 and cen["toffoli"]["max_grow"] >= 64.0 and cen["mixed"]["max_grow"] == 512.0
    assert cen["toffoli"]["backtracks"] >= 40  # SquareCost on the Toffoli landscape: 21 and 24 in one item
    assert cen["small"]["ends"] == {bp.END_FAR: 5, bp.END_STOP_LOSS: 1}
    assert set(cen["other"]["ends"]) == {bp.END_MAXITER, bp.END_NONFINITE, bp.END_STOP_LOSS}
    status = {row[2] for c in FIX["other"]["cases"] for row in c["port"]}
    assert status == {br.ST_CONVERGED, br.ST_MAXITER, br.ST_NONFINITE}
    rows = {c["name"]: c["port"] for g in qc.GROUPS for c in FIX[g]["cases"]}
    assert rows["line-k3-nan"] == [[0, 1, br.ST_NONFINITE, bp.END_NONFINITE]]
    assert rows["line-k3-own"] == [[0, 1, br.ST_CONVERGED, bp.END_STOP_LOSS]] == rows["ccz-cx-own"]
    assert all(row[0] == 5 and row[2] == br.ST_MAXITER for name in ("table-k1-maxiter5", "ccz-cx-maxiter5") for row in rows[name])
    # both instantiations, both costs in each, n even and odd, the parameter cap in both
    tp = {c["name"]: qc.template(c) for g in qc.GROUPS for c in FIX[g]["cases"]}
    assert {(tp[c["name"]].mixed, c["cost"]) for g in qc.GROUPS for c in FIX[g]["cases"]} == {(False, "basic"), (False, "square"),
                                                                                            (True, "basic"), (True, "square")}
    assert {t.n for t in tp.values()} == {15, 24, 27, 33, 45, 99}
    assert tp["table-k15"].n == 99 and not tp["table-k15"].mixed and tp["ten3"].n == 99 and tp["ten3"].mixed
    # branches no input is known for (the module docstring): if one turns up, the documents are to say so
    assert all(cen[g]["nondescent"] == 0 for g in qc.GROUPS)


def test_caps_few_decisions_are_unclear_and_every_tolerance_is_measured():
    for g in qc.GROUPS:
        grp = FIX[g]
        n_items = sum(len(c["items"]) for c in grp["cases"])
        assert 0.0 < grp["e_ref"] and br.TOL_FACTOR * grp["e_ref"] < br.TOL_CAP, g
        assert br.tolerance(grp["e_ref"]) == br.TOL_FACTOR * grp["e_ref"] < 1e-4
        assert grp["unclear_steps"] <= 0.02 * grp["replayed_steps"], g
        assert grp["unclear_items"] <= 0.1 * n_items, g
        for c in grp["cases"]:
            mixed = qc.template(c).mixed
            assert qc.bands(c) == ((1.36e-14, 1.92e-14) if mixed else (6.8e-15, 9.6e-15))
            assert qc.loss_bound(c) == (6.8e-15 if mixed else 3.4e-15)


@pytest.mark.parametrize("name", ["table-k1", "ccz-cx-square"])
def test_truncation_the_port_at_maxiter_j_is_the_full_run_after_step_j(name):
    """``maxiter`` enters the iteration only through ``it < maxiter``: the run with maxiter = j is the full run cut after step j."""
    case = next(c for g in qc.GROUPS for c in FIX[g]["cases"] if c["name"] == name)
    item = case["items"][0]
    f, x, it, st, nev, xs, rec = qc.port_run(case, item)
    evals = np.cumsum([1] + [len(s["trials"]) for s in rec[:-1]])  # evaluations after step j
    assert it >= 30
    for j in range(1, it + 3):
        fj, xj, itj, stj, nevj, xsj, _ = qc.run_port(case, item, maxiter=j)
        if j < it:
            assert (itj, stj, nevj) == (j, br.ST_MAXITER, evals[j]) and np.array_equal(xj, xs[j - 1]), j
            assert all(np.array_equal(a, b) for a, b in zip(xsj, xs))
        else:
            assert (itj, stj, nevj, fj) == (it, st, nev, f) and np.array_equal(xj, x), j


def _first_failure(group, names, cut):
    """The first clear step outside the group's tolerance when the (patched) port's trajectories are replayed by the healthy replay."""
    tol = br.tolerance(FIX[group]["e_ref"])
    for case, item, port in _items(group):
        if case["name"] not in names:
            continue
        xs = qc.run_port(case, item)[5][:cut]
        rp = qc.replay_item(case, item, xs)
        for j, (d, u) in enumerate(zip(rp["dev"], rp["unclear"])):
            if d > tol and not u:
                return case["name"], item, j, d
    return None


@functools.lru_cache(maxsize=None)
def _healthy(group, names, cut):
    return _first_failure(group, names, cut)


class _RowsNeverUpdated:
    """NumPy as the port sees it, with the rows >= 96 of every outer product zeroed: H += s w^T + v s^T never reaches them."""

    def __getattr__(self, name):
        return getattr(np, name)

    @staticmethod
    def outer(a, b):
        out = np.outer(a, b)
        out[96:] = 0
        return out


# defect: (attribute of oracle.bfgs_port, value, group, cases, steps replayed per item)
DEFECTS = {
    "GROW_FACTOR 4": ("GROW_FACTOR", 4.0, "small", ("table-k1",), None),
    "back-track clamp 0.2": ("BACKTRACK_MIN", 0.2, "toffoli", ("toffoli-square",), None),
    "no first-update scaling": ("FIRST_SCALING", False, "small", ("table-k1",), 12),
    "update from too-short steps": ("SKIP_SHORT_UPDATES", False, "small", ("table-k1",), None),
    "RESTART_PERIOD 64": ("RESTART_PERIOD", 64, "small", ("line-k3",), 72),
    "WOLFE_C2 0.9": ("WOLFE_C2", 0.9, "small", ("table-k1",), None),
    "metric rows >= 96 never updated": ("np", _RowsNeverUpdated(), "cap", ("table-k15",), 12),
    "metric rows >= 96 never updated (mixed)": ("np", _RowsNeverUpdated(), "mixed", ("ten3",), 12),
}


@pytest.mark.parametrize("defect", sorted(DEFECTS))
def test_a_planted_defect_fails_a_clear_step(monkeypatch, defect):
    attr, value, group, names, cut = DEFECTS[defect]
    assert _healthy(group, names, cut) is None  # the healthy port passes where the defect is looked for
    monkeypatch.setattr(bp, attr, value)
    hit = _first_failure(group, names, cut)
    print(f"REPLAY planted {defect}: {hit}")
    # a wrong branch moves a step by tenths, three stale rows of 99 by their components' share of it: neither by a tolerance's worth
    floor = 0.05 if attr != "np" else 100.0 * br.tolerance(FIX[group]["e_ref"])
    assert hit is not None and hit[3] >= floor, defect
