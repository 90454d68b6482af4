"""CPU: the host side of candidate scoring and winner selection (slam_decomposition_amd/candidates.py) -- the grid, the folded
recurrence the device runs (tests/candidates_ref.py) against ``coverage.region``, durations under the speed-limit curves, cost scaling,
``pick_winner`` and ``select_basis`` on hand-made tables."""
import logging
import os
import sys

import numpy as np
import pytest

import candidates_ref as ref
from slam_decomposition_amd import candidates as cd
from slam_decomposition_amd import coverage, pulse_cost
from slam_decomposition_amd.gates import ConversionGainGate

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PI = np.pi


@pytest.fixture(scope="module")
def grid():
    return cd.build_gates()


def _tool():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import candidates as tool
    finally:
        sys.path.pop(0)
    return tool


def test_build_gates_is_the_tools_grid(grid):
    gates, per_strength = grid
    tool_gates, tool_per_strength = _tool().build_gates()
    assert len(gates) == len(tool_gates) == 177
    assert per_strength == tool_per_strength and sum(len(x) for x in per_strength) == 177
    assert [g.params for g in gates] == [g.params for g in tool_gates]
    # the tool takes the product's function: hold both to the reference's construction written out (bare_candidates.py:47-69)
    want, seen = [], []
    for k in np.linspace(0, 0.5, 17):
        for p in np.linspace(0, 1, 21):
            params = [0, 0, p * k * PI, (1 - p) * k * PI, 1]
            c = list(cd.c1c2c3(ConversionGainGate(*params).to_matrix()))
            if c[0] > 0.5:
                c[0] = -1 * c[0] + 1
            if c in seen:
                continue
            seen.append(c)
            want.append(params)
    assert [g.params for g in gates] == want and [c for inner in per_strength for c in inner] == seen
    raw = cd.gate_coords(gates)  # c1c2c3 as it comes; the grid's bookkeeping folds c1 to <= 1/2 (the same class at c3 = 0)
    assert (raw[:, 2] == 0).all()
    raw[:, 0] = np.where(raw[:, 0] > 0.5, -1 * raw[:, 0] + 1, raw[:, 0])
    assert np.array_equal(raw, np.array([c for inner in per_strength for c in inner]))
    # the same construction at another resolution, with the map back to the (strength, split) grid
    same, index = cd.candidate_grid()
    assert [g.params for g in same] == [g.params for g in gates] and index.shape == (17, 21)
    assert sorted(set(index.ravel().tolist())) == list(range(177)) and (index[0] == 0).all()
    small, idx = cd.candidate_grid(5, 4, 0.25)
    assert idx.shape == (5, 4) and idx.max() == len(small) - 1
    coords = cd.gate_coords(small)
    for a in range(5):
        for b in range(4):
            c = list(cd.c1c2c3(ConversionGainGate(0, 0, np.linspace(0, 1, 4)[b] * np.linspace(0, 0.25, 5)[a] * PI,
                                                  (1 - np.linspace(0, 1, 4)[b]) * np.linspace(0, 0.25, 5)[a] * PI).to_matrix()))
            got = list(coords[idx[a, b]])
            assert abs(min(c[0], 1 - c[0]) - min(got[0], 1 - got[0])) < 1e-12 and c[1:] == got[1:]


def test_the_binding_mirrors_the_headers_limits():
    import re

    from slam_decomposition_amd import _ffi

    hdr = open(os.path.join(ROOT, "include", "slam_hip.h")).read()
    assert int(re.search(r"#define SLAM_CANDIDATE_MAX_K (\d+)", hdr).group(1)) == _ffi.CANDIDATE_MAX_K >= 64
    assert int(re.search(r"#define SLAM_CANDIDATE_MAX_GATES (\d+)", hdr).group(1)) == _ffi.CANDIDATE_MAX_GATES
    assert "slam_candidate_scores" in _ffi.EXPORTED_SYMBOLS and hasattr(_ffi.Context, "candidate_scores")


def test_the_folded_recurrence_is_coverage_region():
    terms, pattern = ref.derived_terms()
    assert terms == ref.TERMS and pattern == ref.PATTERN and len(terms) == 72
    rng = np.random.default_rng(7)
    for _ in range(20):
        c1 = rng.uniform(0.02, 0.5)
        c2 = rng.uniform(0, c1)
        c3 = rng.uniform(0, c2)
        g = np.array([c1, c2, c3])
        rows = ref.folded_rows(g, 12)
        for k in range(2, 13):
            want = coverage.region(np.repeat(g[None], k, axis=0))
            got = rows[k - 2]
            assert np.array_equal(np.isfinite(got), np.isfinite(want)), (g, k)
            fin = np.isfinite(want)
            assert np.max(np.abs(got[fin] - want[fin])) <= 1e-10, (g, k)


def test_gate_duration(grid):
    # the identity has no duration under a curve; the grid keeps the gain-only gate of a class (gc = 0), so add conversion-only ones
    gates = grid[0][1:] + [ConversionGainGate(0, 0, s * PI, 0.0) for s in (1 / 32, 0.25, 0.4, 0.5)]
    curves = {"mid": cd.mid_speed_limit, "squared": cd.squared_speed_limit}
    seen_gc0 = seen_gg0 = False
    for g in gates:
        gc, gg = g.params[2], g.params[3]
        seen_gc0 |= gc == 0
        seen_gg0 |= gg == 0
        assert abs(cd.gate_duration(g, "linear") - g.cost()) <= 1e-14
        assert abs(cd.gate_duration(g, "bare") - g.cost()) <= 1e-14
        # the definition itself (ray meets gg' = pi/2 - gc') reproduces cost(): closed form, and the bracketed root of a callable
        x, y = cd.speed_limit_intersection(gc, gg, "linear")
        assert abs(g.params[-1] / ((y / gg) if gc == 0 else (x / gc)) - g.cost()) <= 1e-14
        assert abs(cd.gate_duration(g, cd.linear_speed_limit) - g.cost()) <= 1e-14
        for name, fn in curves.items():
            x, y = cd.speed_limit_intersection(gc, gg, name)
            assert abs(y - fn(x)) <= 1e-12 and 0 <= x <= PI / 2 + 1e-15
            assert abs(x * gg - y * gc) <= 1e-14  # on the gate's ray
            d = cd.gate_duration(g, name)
            assert abs(d - g.params[-1] * ((gg / y) if gc == 0 else (gc / x))) <= 1e-15
            assert abs(cd.gate_duration(g, "hardware", fn) - d) <= 1e-13  # the same curve as a user callable
            assert d <= g.cost() + 1e-15  # both curves lie outside the linear one
    assert seen_gc0 and seen_gg0
    iswap = ConversionGainGate(0, 0, PI / 2, 0)
    cx = ConversionGainGate(0, 0, PI / 4, PI / 4)
    assert abs(cd.gate_duration(iswap, "squared") - 1) < 1e-15 and abs(cd.gate_duration(iswap, "mid") - 1) < 1e-15
    assert abs(cd.gate_duration(cx, "squared") - 1 / np.sqrt(2)) < 1e-15
    with pytest.raises(ValueError, match="not shipped"):
        cd.gate_duration(cx, "hardware")
    with pytest.raises(ValueError, match="invalid speed_method"):
        cd.gate_duration(cx, "fast")
    sg = cd.scaled_gate(cx, "squared")
    assert isinstance(sg, cd.SpeedLimitedGate) and sg.cost() == sg.duration == cd.gate_duration(cx, "squared")
    assert type(cd.scaled_gate(cx, "linear")) is ConversionGainGate


def _scores(gates, haar_counts, cnot, swap):
    return cd.CandidateScores.from_counts(gates, np.asarray(haar_counts), {"cnot": np.asarray(cnot), "swap": np.asarray(swap)})


def test_atomic_cost_scaling_and_pick_winner(caplog):
    sq = ConversionGainGate(0, 0, PI / 4, 0)  # sqrt(iSWAP): cost 1/2
    cx = ConversionGainGate(0, 0, PI / 4, PI / 4)  # cost 1
    b = ConversionGainGate(0, 0, 3 * PI / 8, PI / 8)  # cost 1
    ident = ConversionGainGate(0, 0, 0.0, 0.0)
    g, s = cd.atomic_cost_scaling(sq, np.array([2.2, 2, 3]), "linear", 0.1)
    assert np.allclose(s, np.array([2.2, 2, 3]) * 0.5 + (np.array([2.2, 2, 3]) + 1) * 0.1, rtol=0, atol=1e-15) and g.cost() == 0.5
    g, s = cd.atomic_cost_scaling(cx, 3, "squared", 0.25)
    assert abs(s - (3 / np.sqrt(2) + 4 * 0.25)) < 1e-14 and isinstance(g, cd.SpeedLimitedGate)
    _, s = cd.atomic_cost_scaling(cx, 3, "bare", 0.25)
    assert s == 3 + 4 * 0.25
    with pytest.raises(NotImplementedError):
        cd.atomic_cost_scaling(sq, 2.2, "linear", 0.1, family_extension=True, metric=0)
    with pytest.raises(ValueError, match="invalid speed_method"):
        cd.atomic_cost_scaling(sq, 2.2, "warp")
    # k_cap = 4, n = 10 targets per candidate: bins k = 1..4, local, unreached
    gates = [ident, sq, cx, b, ConversionGainGate(0, 0, PI / 4, 0)]
    counts = [[0, 0, 0, 0, 1, 9],   # the identity reaches nothing
              [0, 7, 2, 0, 1, 0],   # haar 2.0
              [0, 0, 9, 0, 1, 0],   # haar 2.7
              [0, 9, 0, 0, 1, 0],   # haar 1.8
              [0, 7, 2, 0, 1, 0]]   # a copy of sqrt(iSWAP): ties with index 1
    sc = _scores(gates, counts, cnot=[5, 2, 1, 2, 2], swap=[5, 3, 3, 2, 3])
    assert sc.k_cap == 4 and sc.n_targets.tolist() == [10]
    assert sc.haar_score.tolist() == [np.inf, 2.0, 2.7, 1.8, 2.0]
    assert sc.volumes[0, 1].tolist() == [0.0, 0.7, 0.9, 0.9]
    with caplog.at_level(logging.INFO):
        # Haar, linear, free 1Q gates: sqrt(iSWAP) 2.0 * 0.5 = 1.0 beats B 1.8 * 1 -- and the tie with its copy goes to index 1
        gate, scaled, score = cd.pick_winner(sc, 0)
    assert gate is gates[1] and score == 1.0 and scaled.cost() == 0.5
    assert sum("winner: 2QGate" in r.getMessage() for r in caplog.records) == 1
    assert sum("scaled scores: 1.0" in r.getMessage() for r in caplog.records) == 1
    # expensive 1Q gates favour the fewest gates: B
    gate, _, score = cd.pick_winner(sc, 0, duration_1q=5.0)  # sqrt(iSWAP) 1.0 + 15.0, B 1.8 + 14.0
    assert gate is gates[3] and abs(score - (1.8 + 2.8 * 5.0)) < 1e-14
    # "bare": gate counts only
    gate, _, score = cd.pick_winner(sc, 0, "bare")
    assert gate is gates[3] and score == 1.8
    # CNOT: cx 1 * 1 = 1.0 ties sqrt(iSWAP) 2 * 0.5 = 1.0 -> the lower index (sqrt(iSWAP), 1)
    gate, _, score = cd.pick_winner(sc, 1)
    assert gate is gates[1] and score == 1.0
    gate, _, score = cd.pick_winner(sc, 1, "squared")  # cx lasts 1 / sqrt 2 under the quarter circle, sqrt(iSWAP) still 1/2 each
    assert gate is gates[2] and abs(score - 1 / np.sqrt(2)) < 1e-15
    # SWAP: sqrt(iSWAP) 3 * 0.5 = 1.5 < B 2; the identity's 5 > k_cap is "not reached" and never wins
    gate, _, score = cd.pick_winner(sc, 2)
    assert gate is gates[1] and score == 1.5
    # lambda: 0.25 * cnot + 0.75 * swap, scaled: sqrt(iSWAP) (0.5 + 2.25) / 2 = 1.375, cx 0.25 + 2.25 = 2.5, B 2.0
    gate, _, score = cd.pick_winner(sc, (-1, 0.25))
    assert gate is gates[1] and abs(score - 1.375) < 1e-15
    assert np.isinf(cd.metric_scores(sc, (-1, 0.25))[0]) and np.isinf(cd.metric_scores(sc, 2)[0])
    with pytest.raises(ValueError):
        cd.pick_winner(sc, 3)
    with pytest.raises(ValueError, match="finite"):
        cd.pick_winner(_scores(gates[:1], counts[:1], [5], [5]), 0)


def test_select_basis_on_a_hand_made_table(monkeypatch):
    sq = ConversionGainGate(0, 0, PI / 4, 0)  # 0.5
    cx = ConversionGainGate(0, 0, PI / 4, PI / 4)  # 1.0
    b = ConversionGainGate(0, 0, 3 * PI / 8, PI / 8)  # 1.0
    gates = [sq, cx, b]
    coords = cd.gate_coords(gates)
    k_cap = 4
    #          target: 0  1  2  3  4  5  6
    first_k = np.array([[2, 3, 3, 0, 2, 3, 5],   # sqrt(iSWAP): misses target 6
                        [1, 3, 3, 0, 2, 1, 3],   # cx
                        [2, 2, 2, 0, 2, 2, 2]])  # B
    named = np.array([[2, 3], [1, 3], [2, 2]])  # cnot, swap
    edges = np.array([[0, 1], [2, 1], [1, 2], [0, 1], [1, 0], [3, 2], [1, 2]])  # pairs (0,1): 0 3 4; (1,2): 1 2 6; (2,3): 5
    targets = np.broadcast_to(np.eye(4, dtype=np.complex128), (7, 4, 4))
    ctx = ref.TableCtx([first_k, named], coords)
    monkeypatch.setattr(cd.runtime, "get_context", lambda device=0, slot=0: ctx)

    def scaled(k, d, q):
        return np.where(k == 0, 0.0, k * d + (k + 1) * q)

    # weighted_overall, free 1Q gates: sqrt(iSWAP) inf, cx 13, B 12
    sel = cd.select_basis(targets, "weighted_overall", gates=gates, k_cap=k_cap)
    assert len(sel.winners) == 1 and sel.winners[0].index == 2 and sel.winners[0].total == 12.0 and sel.winners[0].n == 7
    assert sel.sizes.tolist() == first_k[2].tolist() and sel.sizes.dtype == np.int32 and sel.edges is None
    assert len(ctx.calls) == 1 and ctx.calls[0][0] == 3 and ctx.calls[0][3] == 1
    # weighted_pairwise: ONE grouped call; (0,1) both orientations in one group: sqrt(iSWAP) 2, cx 3, B 4; (1,2): B 6 beats cx 9;
    # (2,3): cx 1
    ctx.calls.clear()
    sel = cd.select_basis(targets, "weighted_pairwise", edges=edges, gates=gates, k_cap=k_cap, duration_1q=0.1)
    assert len(ctx.calls) == 1 and ctx.calls[0][3] == 3 and ctx.calls[0][2].tolist() == [0, 1, 1, 0, 0, 2, 1]
    assert sel.edges.tolist() == [[0, 1], [1, 2], [2, 3]] and sel.group_of.tolist() == [0, 1, 1, 0, 0, 2, 1]
    assert [w.index for w in sel.winners] == [0, 2, 1] and [w.n for w in sel.winners] == [3, 3, 1]
    dur = [0.5, 1.0, 1.0]
    for e, w in enumerate(sel.winners):
        members = np.nonzero(sel.group_of == e)[0]
        total = 0.0
        for t in members:
            total += float(scaled(first_k[w.index, t], dur[w.index], 0.1))
        assert w.total == total and w.gate is gates[w.index] and w.scaled_gate.cost() == dur[w.index]
        assert sel.sizes[members].tolist() == first_k[w.index, members].tolist()
    # the squared curve shortens cx: on (0,1) cx 3 / sqrt 2 = 2.12 still loses to sqrt(iSWAP) 2
    sel = cd.select_basis(targets, "weighted_pairwise", edges=edges, gates=gates, k_cap=k_cap, speed_method="squared")
    assert [w.index for w in sel.winners] == [0, 2, 1] and abs(sel.winners[2].total - 1 / np.sqrt(2)) < 1e-15
    # basic_overall on the CNOT metric: cx 1 * 1 ties sqrt(iSWAP) 2 * 0.5 -> index 0, which misses target 6
    with pytest.raises(ValueError, match=pulse_cost._UNREACHABLE):
        cd.select_basis(targets, "basic_overall", gates=gates, basic_metric=1, k_cap=k_cap)
    sel = cd.select_basis(targets, "basic_overall", gates=gates, basic_metric=1, k_cap=k_cap, duration_1q=0.5)  # cx 2.0 < sqrt(iSWAP) 2.5
    assert sel.winners[0].index == 1 and sel.sizes.tolist() == first_k[1].tolist()
    assert sel.winners[0].total == float(sum(scaled(k, 1.0, 0.5) for k in first_k[1]))
    # lambda_weight 0.47: sqrt(iSWAP) (0.94 + 1.59) / 2 = 1.265 wins the metric and misses target 6; with 1Q cost 2 B's two gates win
    # (B 2 + 6, cx 2.06 + 6.12, sqrt(iSWAP) 1.265 + 7.06)
    with pytest.raises(ValueError, match=pulse_cost._UNREACHABLE):
        cd.select_basis(targets, "lambda_weight", gates=gates, k_cap=k_cap)
    sel = cd.select_basis(targets, "lambda_weight", gates=gates, k_cap=k_cap, duration_1q=2.0)
    assert sel.winners[0].index == 2 and sel.sizes.tolist() == first_k[2].tolist()
    # uneven groups with a group out of every candidate's reach
    bad = first_k.copy()
    bad[:, 5] = 5
    ctx2 = ref.TableCtx([bad, named], coords)
    monkeypatch.setattr(cd.runtime, "get_context", lambda device=0, slot=0: ctx2)
    with pytest.raises(ValueError, match=pulse_cost._UNREACHABLE):
        cd.select_basis(targets, "weighted_pairwise", edges=edges, gates=gates, k_cap=k_cap)
    with pytest.raises(ValueError, match="Strategy not recognized"):
        cd.select_basis(targets, "fastest", gates=gates)
    with pytest.raises(ValueError, match="edges"):
        cd.select_basis(targets, "weighted_pairwise", gates=gates)
