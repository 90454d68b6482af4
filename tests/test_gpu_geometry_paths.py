"""GPU: the geometry unit after the "Geometry lookups" refactor (HISTORY.md) -- one target frame, one pair of row tests and one
histogram fold in its lookup kernels; one buffer carver, one window check and shared table checks in its entry points -- computes, byte
for byte, and refuses, code for code and word for word, what the commit before it did.

tests/golden/geometry_parent.npz was recorded from that commit's build by tools/make_geometry_parent_fixture.py, which also runs the
cases here (its docstring lists them): the coverage lookup over three tables (one beyond the LDS histogram), the family lookup under
both policies, candidate scores (k_cap 64 and 2, groups, and a launch whose blocks walk three LDS tiles), a region lookup with all
three polytope kinds, span prediction, Haar selection by span, the parallel-drive sampler with its extremes and filter, and the
windowed Weyl / KAK / target reads.  `refuse.*` holds SlamHipError.code and the message of the refusals of every touched entry point.
The tool runs every case twice on the parent build and leaves out what differs between the two runs: nothing did.
"""
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "geometry_parent.npz")

CASES = ["coverage", "family", "candidates", "region", "predict_spans", "haar_select_spans", "pd", "c1c2c3", "refuse"]
ENTRY_POINTS = ["targets_kak", "targets_c1c2c3", "get_targets", "predict_spans", "coverage_lookup", "family_lookup", "candidate_scores",
                "haar_select_spans", "pd_sample", "pd_extremes", "pd_filter", "region_lookup"]


def _tool():
    spec = importlib.util.spec_from_file_location("make_geometry_parent_fixture", os.path.join(ROOT, "tools", "make_geometry_parent_fixture.py"))
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
def test_geometry_results_and_refusals_are_the_parents(parent, current, case):
    keys = [key for key in parent if key.split(".")[0] == case]
    assert keys
    for key in keys:
        if case == "refuse":  # a readable failure: the code and the message
            assert (int(parent[key][0]), bytes(parent[key][1:].astype(np.uint8))) == (int(current[key][0]), bytes(current[key][1:].astype(np.uint8))), key
        assert parent[key].tobytes() == current[key].tobytes(), key


def test_the_cases_reach_their_paths(parent):
    """the fixture itself: the bins, rows, kinds and refusals the cases are there for are the ones that were hit"""
    tool = _tool()
    n = tool.N_TARGETS
    # coverage: tables of 4, 0 and 8193 rows -> 6 + 2 + 8195 bins; every target is counted once per table
    counts = parent["coverage.counts"]
    mixed, empty, far = counts[:6], counts[6:8], counts[8:]
    assert len(far) == 8195 and mixed.sum() == empty.sum() == far.sum() == n
    n_local = int(mixed[4])
    assert n_local >= 2 and empty.tolist() == [n_local, n - n_local]  # the identities; an empty table reaches nothing else
    assert mixed[0] >= 2 and mixed[1] >= 1 and mixed[2] > 0 and mixed[3] > 0  # CX and -i CX, sqrt(iSWAP), both half-space rows
    assert far[:8192].sum() == 0 and far[8192] == n - n_local and far[8193] == n_local and far[8194] == 0  # all beyond the LDS bins
    entries = parent["coverage.entries"]
    assert entries.shape == (3, n) and np.array_equal(np.bincount(entries[2], minlength=8195), far)
    # family: several members win under both policies, some targets are local or out of reach, and the two policies differ
    for policy in ("reference", "best"):
        assert parent[f"family.{policy}.counts"].sum() == n and len(np.unique(parent[f"family.{policy}.member"])) >= 4
        assert np.all(parent[f"family.{policy}.counts"][-2:] > 0)
    assert not np.array_equal(parent["family.reference.member"], parent["family.best.member"])
    # candidates: point hits at k = 1, hits at large k, the cap, groups that add up, and the tiled launch
    c64, c2 = parent["candidates.k64.counts"][0], parent["candidates.k2.counts"][0]
    G = len(parent["candidates.coords"])
    assert c64.shape == (G, 66) and np.all(c64.sum(axis=1) == n) and c64[:, 0].sum() > 0 and c64[:, 8:64].sum() > 0
    assert c2.shape == (G, 4) and np.array_equal(c2[:, :2], c64[:, :2]) and np.array_equal(c2[:, 2], c64[:, 64])
    assert np.array_equal(parent["candidates.k2.first_k"], np.minimum(parent["candidates.k64.first_k"], 3))
    groups = parent["candidates.groups.counts"]
    assert groups.shape == (3, G, 10) and np.array_equal(groups.sum(axis=(1, 2)) // G, np.bincount(np.arange(n) % 3))
    tiles = parent["candidates.tiles.counts"][0]
    assert len(tiles) > 32 * 32 and np.all(tiles.sum(axis=1) == tool.N_BIG) and -(-len(tiles) // 32) == tool.BIG_CHUNK  # 32 chunks
    # region: every region holds targets, the point polytope among them, and the first-region histogram counts every target
    region = parent["region.counts"]
    assert np.all(region[:3] > 0) and region[3:].sum() == n and region[3] == region[0] and region[6] > 0
    # spans: a wider tolerance and a longer template only ever reach more
    s1, s4 = parent["predict_spans.k1.tol0"], parent["predict_spans.k4.tol0"]
    assert set(np.unique(s1)) == {0, 1, 2} and set(np.unique(s4)) == {0, 1, 2, 3}
    assert np.all(parent["predict_spans.k4.tol1e-06"] <= s4)
    sel = {name: int(parent[f"haar_select_spans.{name}.n_selected"][0]) for name in ("margin0", "margin", "wide", "capped")}
    assert sel["margin0"] == sel["capped"] > 10 == len(parent["haar_select_spans.capped.indices"]) and sel["wide"] < sel["margin"] <= sel["margin0"]
    assert parent["haar_select_spans.margin0.span_counts"].sum() == 1000 and parent["haar_select_spans.margin0.span_counts"][2] == sel["margin0"]
    assert np.array_equal(parent["haar_select_spans.capped.indices"], parent["haar_select_spans.margin0.indices"][:10])
    # pd: the replay returns the batch's rows; the filter keeps some and drops some
    assert np.array_equal(parent["pd.replay.coords"], parent["pd.coords"][[0, 17, 299, 150, 17]])
    assert 0 < len(parent["pd.filter.indices"]) < 300 and np.all(np.diff(parent["pd.filter.indices"]) > 0)
    assert parent["pd.extremes.indices"][-1] >= 0 and np.array_equal(parent["pd.extremes.coords"], parent["pd.coords"][parent["pd.extremes.indices"]])
    # refusals: every touched entry point, a negative code each; a double fault reports the window
    refused = {key.split(".")[1] for key in parent if key.startswith("refuse.")}
    assert refused == set(ENTRY_POINTS)
    assert all(parent[key][0] < 0 for key in parent if key.startswith("refuse."))
    assert parent["refuse.coverage_lookup.window_and_table"].tobytes() == parent["refuse.coverage_lookup.window"].tobytes()
