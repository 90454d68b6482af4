"""GPU: the host paths whose text the "Host loop end" refactor (HISTORY.md) moved into shared functions -- the end of every span-loop
driver, the fold of the stages' counters, the V2 loop's epilogue block, the evaluation staging and the single-stage preamble of the V2
and smush families -- compute, byte for byte, and launch what the commit before it did.

tests/golden/host_paths_parent.npz was recorded from that commit's build by tools/make_host_paths_parent_fixture.py, which also runs
the cases here (its docstring lists them): the staged, one-launch and overlapped span loops, decompose_list with a wider layout,
decompose_predicted with and without carry, decompose_multi over two contexts, a plain stage with an active list and start points, the
three plain evaluation calls, and loop / stage / evaluation of a RiSwapGate template and stage / evaluation of a one-slice smush gate.

Per case every result array is compared, and `<case>.counts`: kernel_launches and items[k] of Context.stats() after a reset_stats()
(for both contexts of the multi case).  Times are not pinned.  The tool runs every case twice on the parent build and leaves out what
differs between the two runs: nothing did.  (The list case keeps the parameter rows of the listed targets only: the rows of targets
that no call has decomposed are not initialised.)
"""
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "host_paths_parent.npz")

CASES = ["staged", "wave", "overlap", "list", "predicted0", "predicted1", "multi", "multi1", "stage", "eval", "v2_loop", "v2_stage", "v2_eval",
         "smush_stage", "smush_eval"]


def _tool():
    spec = importlib.util.spec_from_file_location("make_host_paths_parent_fixture", os.path.join(ROOT, "tools", "make_host_paths_parent_fixture.py"))
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
    assert sorted({key.split(".")[0] for key in parent}) == sorted(CASES)
    for key in parent:
        assert parent[key].shape == current[key].shape and parent[key].dtype == current[key].dtype, key


@pytest.mark.parametrize("case", CASES)
def test_host_path_results_and_counts_are_the_parents(parent, current, case):
    keys = [key for key in parent if key.split(".")[0] == case]
    assert keys
    for key in keys:
        assert parent[key].tobytes() == current[key].tobytes(), key


def test_the_cases_reach_their_paths(parent):
    """the fixture itself: every loop runs both of its spans for all its targets (no Haar target is reached at span 1), and the launch
    counts are those of the paths the cases are named after"""
    tool = _tool()
    for case, restarts in (("staged", tool.RESTARTS), ("wave", tool.RESTARTS), ("overlap", 17), ("multi", tool.RESTARTS), ("multi1", tool.RESTARTS),
                           ("v2_loop", tool.RESTARTS)):
        assert parent[f"{case}.counts"][1:].tolist()[:4] == [0, tool.N_TARGETS * restarts, tool.N_TARGETS * restarts, 0], case
        assert np.all(parent[f"{case}.best_cycles"] == 2), case
    launches = {case: int(parent[f"{case}.counts"][0]) for case in CASES if f"{case}.counts" in parent}
    assert launches["staged"] == 2 and launches["wave"] == 3 and launches["overlap"] == 5  # per span; per span + merge; 2 per span + merge
    assert launches["multi"] == 4 and launches["multi1"] == 0  # per span one launch per gate class, booked by the leading context
    assert launches["stage"] == launches["v2_stage"] == launches["smush_stage"] == 1
    assert launches["list"] == launches["v2_loop"] == 2
    # the list call leaves the other targets alone; with carry the targets that miss at their predicted size go on to the next
    assert np.array_equal(parent["list.best_cycles"] == -1, ~np.isin(np.arange(tool.N_TARGETS), [6, 1, 4, 3, 0]))
    assert parent["predicted0.counts"][3] == parent["predicted1.counts"][3] and parent["predicted0.counts"][4] < parent["predicted1.counts"][4]
