"""GPU: the order of independent instructions inside the optimizer round (minimize_body, eval_quad) is free; its floating-point
operations are not.  The library has to compute, byte for byte, what the commit before the round-order work computed, on the paths
that tests/golden/span1_parent_outputs.npz and host_paths_parent.npz do not reach.

tests/golden/round_order_parent.npz was recorded from that commit's build by tools/make_round_order_parent_fixture.py, which also runs
the cases here (its docstring lists them): the span-2 stage alone with and without ordered early exit (sqrt(iSWAP) and B), spans 1 and
2 through the multi-queue instantiation, span-1 stages from start points with an entry of 1e8 - 1 (also with maxiter = 1), and span 1
in trace mode with trace_cap = 8.  64 targets x 4 restarts each.

What is compared is what tests/test_gpu_span1_roomy.py compares: every winner whole; per-item records up to the winner under ordered
early exit (a restart behind it is dropped, pre-empted or finishes by itself depending on when the winner's flag becomes visible) and
whole otherwise, together with the stage's evaluation totals (all and accepted).  A trace row is compared for the items whose
records are.
"""
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "round_order_parent.npz")

ORDERED_STAGES = ["k2_ordered_sqiswap", "k2_ordered_b", "trace"]
PLAIN_STAGES = ["k2_plain_sqiswap", "k2_plain_b", "bigx0", "maxiter1"]
MULTI = ["multi_k1.sqiswap", "multi_k1.qiswap", "multi_k2.sqiswap", "multi_k2.qiswap"]


def _tool():
    spec = importlib.util.spec_from_file_location("make_round_order_parent_fixture", os.path.join(ROOT, "tools", "make_round_order_parent_fixture.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _same(a, b):
    return np.array_equal(a, b, equal_nan=a.dtype.kind == "f")


@pytest.fixture(scope="module")
def parent():
    with np.load(GOLDEN) as z:
        return {key: z[key] for key in z.files}


@pytest.fixture(scope="module")
def current(hip_ctx):
    return _tool().run_cases(hip_ctx)


def test_fixture_and_run_hold_the_same_arrays(parent, current):
    assert sorted(parent) == sorted(current)
    for key in parent:
        assert parent[key].shape == current[key].shape and parent[key].dtype == current[key].dtype, key


def test_the_cases_are_worth_their_names(parent):
    tool = _tool()
    # span 2 reaches part of the Haar targets with sqrt(iSWAP) (ordered early exit has winners to stop at) and all of them with B
    solved = parent["k2_ordered_sqiswap.best_loss"] < tool.STAGE_EXIT_LOSS
    assert 0 < solved.sum() < tool.N_TARGETS
    assert np.all(parent["k2_plain_b.best_loss"] < 1e-8)
    # the start points hold the entries at the edge of the validated range, and the kernel was given them
    assert np.sum(np.abs(tool.big_x0()) == tool.BIG_X) == tool.N_TARGETS * tool.RESTARTS // 8
    # maxiter = 1: no item makes a second step
    assert parent["maxiter1.item_iters"].max() == 1 and parent["bigx0.item_iters"].max() > 1
    # the trace is filled: some item ran past the cap, and the rows up to an item's iterations are numbers
    iters = parent["trace.item_iters"]
    assert iters.max() > tool.TRACE_CAP and np.isfinite(parent["trace.trace_loss"][iters >= 1][:, 0]).all()


@pytest.mark.parametrize("case", MULTI)
def test_multi_queue_results_are_the_parents(parent, current, case):
    for name in ("best_loss", "best_x", "best_cycles"):
        assert _same(parent[f"{case}.{name}"], current[f"{case}.{name}"]), (case, name)


@pytest.mark.parametrize("case", ORDERED_STAGES + PLAIN_STAGES)
def test_stage_winners_are_the_parents(parent, current, case):
    for name in ("best_loss", "best_x", "best_restart"):
        assert _same(parent[f"{case}.{name}"], current[f"{case}.{name}"]), (case, name)


@pytest.mark.parametrize("case", ORDERED_STAGES + PLAIN_STAGES)
def test_item_records_are_the_parents(parent, current, case):
    tool = _tool()
    restarts = np.arange(tool.RESTARTS)[None, :]
    if case in ORDERED_STAGES:
        # up to the winner where a restart went below the stage's exit level (module docstring); every restart elsewhere
        solved = parent[f"{case}.best_loss"] < tool.STAGE_EXIT_LOSS
        keep = ~solved[:, None] | (restarts <= parent[f"{case}.best_restart"][:, None])
    else:
        keep = np.ones((tool.N_TARGETS, tool.RESTARTS), dtype=bool)
        assert np.array_equal(parent[f"{case}.evals"], current[f"{case}.evals"]), case
    assert keep.sum() >= tool.N_TARGETS
    names = tool.TRACE_ITEM_KEYS + ("trace_loss", "trace_x") if case == "trace" else tool.ITEM_KEYS
    for name in names:
        a, b = parent[f"{case}.{name}"], current[f"{case}.{name}"]
        assert _same(a[keep], b[keep]), (case, name)
