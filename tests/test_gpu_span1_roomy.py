"""GPU: the span-1 optimizer kernel's register-budget hoists (roomy_regs, slam_device.hpp) change no floating-point operation, so
the library has to compute, byte for byte, what the commit before them computed.

tests/golden/span1_parent_outputs.npz was recorded from that commit's build by tools/make_span1_parent_fixture.py, which also runs
the cases here (its docstring lists them): span loops 1..3 with ordered early exit for sqrt(iSWAP), CNOT and B, and span-1 stages
with explicit start points, with pinned exterior layers and with SquareCost, 64 targets x 4 restarts each.

What is compared: every winner (loss, parameters, template size or restart index) and every per-item record (loss, iterations,
status, evaluations) that the scheduling cannot change.  Under ordered early exit the restarts up to a target's winner always run
to their own end; a restart behind it is dropped, pre-empted or finishes by itself depending on when the winner's flag becomes
visible, so its record differs between two runs of ONE build and is left out.  The stages without early exit are compared whole,
together with the stage's evaluation totals (all and accepted).
"""
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "span1_parent_outputs.npz")

LOOPS = ["loop_sqiswap", "loop_cx", "loop_b"]
ORDERED_STAGES = ["stage_sqiswap", "stage_cx", "stage_b", "stage_square"]
PLAIN_STAGES = ["stage_x0", "stage_noext"]


def _tool():
    spec = importlib.util.spec_from_file_location("make_span1_parent_fixture", os.path.join(ROOT, "tools", "make_span1_parent_fixture.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


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


@pytest.mark.parametrize("case", LOOPS)
def test_span_loop_results_are_the_parents(parent, current, case):
    for name in ("best_loss", "best_x", "best_cycles"):
        assert np.array_equal(parent[f"{case}.{name}"], current[f"{case}.{name}"]), (case, name)
    # the cases are worth their name: no Haar target is reached at span 1 (every span-1 restart runs to its end and the target goes
    # on to span 2), the loop converges, and sqrt(iSWAP) needs both of the longer templates
    cycles = parent[f"{case}.best_cycles"]
    assert np.all(parent[f"{case}.best_loss"] < 1e-8) and np.all(cycles >= 2)
    if case == "loop_sqiswap":
        assert set(np.unique(cycles)) == {2, 3}


@pytest.mark.parametrize("case", ORDERED_STAGES + PLAIN_STAGES)
def test_span1_stage_winners_are_the_parents(parent, current, case):
    for name in ("best_loss", "best_x", "best_restart"):
        assert np.array_equal(parent[f"{case}.{name}"], current[f"{case}.{name}"]), (case, name)


@pytest.mark.parametrize("case", ORDERED_STAGES + PLAIN_STAGES)
def test_span1_item_records_are_the_parents(parent, current, case):
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
    for name in tool.ITEM_KEYS:
        a, b = parent[f"{case}.{name}"], current[f"{case}.{name}"]
        assert np.array_equal(a[keep], b[keep]), (case, name, int(np.sum(a[keep] != b[keep])))
