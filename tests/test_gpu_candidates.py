"""GPU: slam_candidate_scores (csrc/slam_candidates.hpp) against the host's coverage model target by target, against the existing
device lookup over host-built tables, across groups and windows, at known values -- and the selection pipeline built on it
(slam_decomposition_amd/candidates.py) end to end."""
import os
import sys
import types

import numpy as np
import pytest

import candidates_ref as ref
from slam_decomposition_amd import _ffi, coverage, pulse_cost
from slam_decomposition_amd import candidates as cd
from slam_decomposition_amd.gates import canonical_matrix
from slam_decomposition_amd.sampler import DeviceHaarBatch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = pulse_cost.TOL
# sqrt(iSWAP) class, CNOT class with gc = gg, B, iSWAP, the grid's weakest gate, the identity, three generic gates
NINE = np.array([[0.25, 0.25, 0.0], [0.5, 0.0, 0.0], [0.5, 0.25, 0.0], [0.5, 0.5, 0.0], [1 / 32, 0.0, 0.0], [0.0, 0.0, 0.0],
                 [0.31, 0.17, 0.05], [0.44, 0.21, 0.13], [0.12, 0.07, 0.02]])
SQ, CNOT, B, ISWAP, WEAK, IDENT = range(6)


GOLDEN = np.load(os.path.join(ROOT, "tests", "golden", "candidate_first_k.npz"))  # tools/make_candidate_fixture.py


def _local(rng):
    """A Haar-ish random local gate A (x) B."""
    def su2():
        q = rng.normal(size=4)
        a, b, c, d = q / np.linalg.norm(q)
        return np.array([[a + 1j * b, c + 1j * d], [-c + 1j * d, a - 1j * b]])

    return np.kron(su2(), su2())


@pytest.fixture(scope="module")
def batch(hip_ctx):
    """515 targets of the recorded classes: 500 Haar classes, then identity, CNOT, SWAP, iSWAP, B, sqrt(iSWAP), sqrt(SWAP) and eight
    points 1e-5 off a k = 2 face of sqrt(iSWAP) and of a generic gate -- a canonical gate between random local gates each, the named
    ones as their usual matrices.  Returns (unitaries, the Weyl coordinates the device computes for them)."""
    assert np.array_equal(GOLDEN["gates"], NINE)
    rng = np.random.default_rng(11)
    u = np.stack([_local(rng) @ canonical_matrix(*c) @ _local(rng) for c in GOLDEN["coords"]])
    u[500:507] = [np.eye(4, dtype=np.complex128), cd.CX, cd.SWAP, canonical_matrix(0.5, 0.5, 0.0), canonical_matrix(0.5, 0.25, 0.0),
                  canonical_matrix(0.25, 0.25, 0.0), canonical_matrix(0.25, 0.25, 0.25)]
    assert u.shape == (515, 4, 4)
    hip_ctx.set_targets(u)
    return u, hip_ctx.targets_c1c2c3(0, 515)


@pytest.fixture(scope="module")
def host_first_k(batch):
    """``coverage.minimal_prefix`` per (gate, target) at k_cap = 64 (k_cap = 5 is its truncation), and per gate the smallest distance
    of an explicit target from a widened face of 1 .. 64 copies: the recorded values where the device's coordinates are the recorded
    ones -- 63 regions of up to 64 gates per candidate take the host 22 s --, else computed."""
    if np.array_equal(batch[1], GOLDEN["coords"]):
        return GOLDEN["first_k"].astype(np.int64), GOLDEN["face_margin"]
    return ref.first_k_table(NINE, batch[1], 64, TOL), np.array([ref.face_margins(batch[1][500:], g, 64, TOL).min() for g in NINE])


@pytest.mark.parametrize("k_cap", [5, 64])
def test_first_sizes_equal_the_host_model_target_by_target(hip_ctx, batch, host_first_k, k_cap):
    u, coords = batch
    hip_ctx.set_targets(u)
    counts, first_k = hip_ctx.candidate_scores(NINE, k_cap, want_first=True, tol=TOL)
    assert counts.shape == (1, 9, k_cap + 2) and first_k.shape == (9, 515) and first_k.dtype == np.int32
    # precondition on the explicit targets: none within 1e-9 of a widened face (device and host bounds differ by about 1e-11)
    table, face_margin = host_first_k
    assert face_margin.shape == (9,) and face_margin.min() > 1e-9
    want = np.where(table > k_cap, k_cap + 1, table)
    if k_cap == 5:  # cheap enough to compute here: the recorded table is the host model
        assert np.array_equal(want, ref.first_k_table(NINE, coords, 5, TOL))
        assert min(ref.face_margins(coords[500:], g, 5, TOL).min() for g in NINE) >= face_margin.min()
    bad = np.argwhere(first_k != want)
    assert len(bad) == 0, [(int(g), int(t), int(first_k[g, t]), int(want[g, t])) for g, t in bad[:10]]
    assert np.array_equal(counts, ref.counts_of(first_k, k_cap))
    assert (counts.sum(axis=2) == 515).all()
    # the face points fall on their sides of k = 2, the named targets where they are known to
    assert first_k[SQ, 507:511].tolist() == [2, 3, 2, 3] and first_k[6, 511:515].tolist() == [2, 3, 2, 3]
    assert (first_k[:, 500] == 0).all()
    assert first_k[CNOT, 501] == 1 and first_k[SQ, 501] == 2 and first_k[SQ, 502] == 3 and first_k[ISWAP, 503] == 1
    assert first_k[B, 504] == 1 and first_k[SQ, 505] == 1 and first_k[IDENT, 501] == k_cap + 1
    assert first_k[WEAK, 501] == (16 if k_cap == 64 else 6) and first_k[WEAK, 502] == (48 if k_cap == 64 else 6)


def test_counts_equal_the_table_lookup(hip_ctx):
    """The existing device path: one host-built single-gate table per candidate (rows k = 1 .. 12) through slam_coverage_lookup."""
    n = 4099
    DeviceHaarBatch(seed=5, n_samples=n).fill(hip_ctx)
    tables = []
    for g in NINE:
        bounds = np.zeros((12, 14))
        for k in range(2, 13):
            bounds[k - 1] = coverage.region(np.repeat(g[None], k, axis=0))
        points = np.zeros((12, 4))
        points[0] = coverage.alcove_coordinates(g[None])[0]
        tables.append(types.SimpleNamespace(kinds=np.array([0] + [1] * 11, dtype=np.int32), points=points, bounds=bounds))
    want, _ = hip_ctx.coverage_lookup(tables, 0, n, tol=TOL)
    counts, none = hip_ctx.candidate_scores(NINE, 12, tol=TOL)
    assert none is None
    for j in range(9):
        assert np.array_equal(counts[0, j], want[j]), j
    assert hip_ctx.last_candidate_kernel_ms > 0


def test_groups_windows_and_repeats(hip_ctx, batch):
    u, _ = batch
    hip_ctx.set_targets(u)
    whole, fk = hip_ctx.candidate_scores(NINE, 64, want_first=True, tol=TOL)
    again, fk2 = hip_ctx.candidate_scores(NINE, 64, want_first=True, tol=TOL)
    assert np.array_equal(whole, again) and np.array_equal(fk, fk2)
    rng = np.random.default_rng(3)
    groups = np.zeros(515, dtype=np.int32)
    groups[rng.permutation(515)[:115]] = 1  # sizes 400, 115 and 0
    per, fkg = hip_ctx.candidate_scores(NINE, 64, groups=groups, n_groups=3, want_first=True, tol=TOL)
    assert per.shape == (3, 9, 66) and np.array_equal(fkg, fk)
    assert np.array_equal(per.sum(axis=0), whole[0]) and (per[2] == 0).all()
    assert (per[0].sum(axis=1) == 400).all() and (per[1].sum(axis=1) == 115).all()
    assert np.array_equal(per, ref.counts_of(fk, 64, groups, 3))
    a, fa = hip_ctx.candidate_scores(NINE, 64, first=0, count=200, want_first=True, tol=TOL)
    b, fb = hip_ctx.candidate_scores(NINE, 64, first=200, count=315, want_first=True, tol=TOL)
    assert np.array_equal(a + b, whole) and np.array_equal(np.concatenate([fa, fb], axis=1), fk)
    gw, _ = hip_ctx.candidate_scores(NINE, 64, groups=groups[200:], n_groups=3, first=200, count=315, tol=TOL)
    assert np.array_equal(gw, ref.counts_of(fk[:, 200:], 64, groups[200:], 3))
    # one candidate, one target; an empty window
    one, f1 = hip_ctx.candidate_scores(NINE[B : B + 1], 64, first=501, count=1, want_first=True, tol=TOL)
    assert f1.tolist() == [[2]] and one[0, 0, 1] == 1 and one.sum() == 1
    zero, f0 = hip_ctx.candidate_scores(NINE, 3, first=7, count=0, want_first=True, tol=TOL)
    assert zero.shape == (1, 9, 5) and not zero.any() and f0.shape == (9, 0)
    # k_cap = 1: only the gate's own class
    c1, f1 = hip_ctx.candidate_scores(NINE, 1, want_first=True, tol=TOL)
    assert np.array_equal(f1, np.where(fk > 1, 2, fk))
    with pytest.raises(_ffi.SlamHipError, match="k_cap"):
        hip_ctx.candidate_scores(NINE, _ffi.CANDIDATE_MAX_K + 1)
    with pytest.raises(_ffi.SlamHipError, match="group_of"):
        hip_ctx.candidate_scores(NINE, 4, groups=np.full(515, 3, dtype=np.int32), n_groups=3)
    with pytest.raises(_ffi.SlamHipError, match="target window"):
        hip_ctx.candidate_scores(NINE, 4, first=500, count=16)


def test_known_values(hip_ctx):
    n = 4096
    DeviceHaarBatch(seed=21, n_samples=n).fill(hip_ctx)
    counts, _ = hip_ctx.candidate_scores(NINE, 8, tol=TOL)
    sc = cd.CandidateScores.from_counts(list(NINE), counts[0], coords=NINE)
    assert sc.n_targets.tolist() == [n]
    for g in (CNOT, ISWAP):
        assert counts[0, g, 2] == n and sc.haar_score[g] == 3.0
    assert counts[0, B, 1] == n and sc.haar_score[B] == 2.0
    assert counts[0, IDENT, 9] == n and np.isinf(sc.haar_score[IDENT])
    assert counts[0, WEAK, 9] > 0 and np.isinf(sc.haar_score[WEAK])
    assert np.isfinite(sc.haar_score[[SQ, 6, 7]]).all() and 2.0 < sc.haar_score[SQ] < 2.3  # 2 x 0.79 + 3 x 0.21
    assert sc.volumes[0, SQ, 2] == 1.0 and abs(sc.volumes[0, SQ, 1] - 0.79) < 0.03


def _tool():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import candidates as tool
    finally:
        sys.path.pop(0)
    return tool


def _scaled(raw, gate, method, q):
    d = 1.0 if method == "bare" else cd.gate_duration(gate, method)
    return raw * d + (raw + 1) * q


def test_scores_winners_and_per_edge_selection_end_to_end(hip_ctx):
    gates = cd.build_gates()[0]
    n = 4096
    sc = cd.score_candidates(gates, DeviceHaarBatch(seed=3, n_samples=n))
    assert sc.counts.shape == (1, 177, 66) and sc.n_targets.tolist() == [n] and sc.haar_score.shape == (177,)
    assert np.isinf(sc.haar_score[0]) and sc.named_scores["cnot"][0] == 65  # the identity
    # the named scores are the dev tool's first sizes (the strong half of the grid: the tool takes seconds per weak gate)
    tool = _tool()
    for j in list(range(97, 177, 9)) + [1]:
        c = sc.coords[j]
        want = [tool.first_size(t, c, 16) for t in (tool.CNOT_COORDS, tool.SWAP_COORDS)]
        got = [int(sc.named_scores[name][j]) for name in ("cnot", "swap")]
        assert [g if g <= 16 else None for g in got] == want, (j, got, want)
    # every winner is the argmin recomputed here from the integer counts and gate_duration
    ks = np.arange(1, 65)
    haar = np.array([np.inf if (row[65] > 0 or j == 0) else float((row[:64] * ks).sum()) / n for j, row in enumerate(sc.counts[0])])
    cnot = np.where(sc.named_scores["cnot"] > 64, np.inf, sc.named_scores["cnot"].astype(float))
    swap = np.where(sc.named_scores["swap"] > 64, np.inf, sc.named_scores["swap"].astype(float))
    assert np.array_equal(haar, sc.haar_score)
    for method in ("linear", "squared"):
        for metric, raw in ((0, haar), (1, cnot), (2, swap), ((-1, 0.47), 0.47 * cnot + (1 - 0.47) * swap)):
            want = [np.inf if not np.isfinite(r) else _scaled(r, g, method, 0.1) for r, g in zip(raw, gates)]
            j = int(np.argmin(want))
            gate, scaled, score = cd.pick_winner(sc, metric, method, 0.1)
            assert gate is gates[j] and score == want[j], (method, metric, j)
            assert scaled.cost() == cd.gate_duration(gates[j], method)
    # per-edge selection: 60 explicit targets over 4 edges, from ONE grouped call
    u = DeviceHaarBatch(seed=8, n_samples=56).as_array()
    u = np.concatenate([u, np.stack([cd.CX, cd.SWAP, canonical_matrix(0.5, 0.5, 0.0), np.eye(4, dtype=np.complex128)])])
    pairs = np.array([[0, 1], [1, 2], [2, 3], [3, 0]])
    edges = pairs[np.arange(60) % 4]
    edges[::3] = edges[::3, ::-1]  # orientation does not matter
    sel = cd.select_basis(u, "weighted_pairwise", edges=edges, speed_method="squared", duration_1q=0.1)
    fk = cd.score_candidates(gates, list(u), named=(), want_first=True).first_k
    assert fk.shape == (177, 60)
    assert sel.edges.tolist() == [[0, 1], [0, 3], [1, 2], [2, 3]] and len(sel.winners) == 4
    for e, w in enumerate(sel.winners):
        members = np.nonzero((np.sort(edges, axis=1) == sel.edges[e]).all(axis=1))[0]
        assert w.n == len(members) == 15
        totals = []
        for j, g in enumerate(gates):
            k = fk[j, members]
            if j == 0 or (k > 64).any():
                totals.append(np.inf)
                continue
            tot = 0.0
            for kk in k.tolist():
                tot += 0.0 if kk == 0 else float(_scaled(float(kk), g, "squared", 0.1))
            totals.append(tot)
        j = int(np.argmin(totals))
        assert w.index == j and w.total == totals[j], (e, w.index, j)
        assert sel.sizes[members].tolist() == fk[j, members].tolist()
