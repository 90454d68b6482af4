"""Host models for the candidate-scoring tests (CPU, NumPy only).

``folded_rows``  the recurrence ``candidate_rows_kernel`` (csrc/slam_candidates.hpp) runs, restated in NumPy with the SAME term table:
                 the region of k copies of one gate is the max-plus dynamic programme of ``coverage._region`` with the degree d folded
                 into the weight, so that the state is the Schubert class alone -- 4 + 6 + 4 = 14 weights, numbered like the subsets of
                 ``coverage._PATTERNS``;
``derived_terms`` the same table derived from the ring tables of ``coverage.py`` (what the hard-coded copy is pinned against);
``first_k_table`` ``coverage.minimal_prefix`` per (gate, target): what ``slam_candidate_scores`` must return;
``face_margins``  how far targets are from the faces that decide it;
``TableCtx``      a stand-in for ``_ffi.Context`` that serves a hand-made first-size table through ``candidate_scores``.
"""
import itertools

import numpy as np

from slam_decomposition_amd import coverage

# (from, x, to, d): q^d sigma_to is a term of sigma_from * sigma_x; states 0..3 Gr(1, 4), 4..9 Gr(2, 4), 10..13 Gr(3, 4)
TERMS = [
    (0, 0, 1, 1), (0, 1, 2, 1), (0, 2, 3, 1), (0, 3, 0, 0), (1, 0, 2, 1), (1, 1, 3, 1), (1, 2, 0, 0), (1, 3, 1, 0),
    (2, 0, 3, 1), (2, 1, 0, 0), (2, 2, 1, 0), (2, 3, 2, 0), (3, 0, 0, 0), (3, 1, 1, 0), (3, 2, 2, 0), (3, 3, 3, 0),
    (4, 4, 9, 2), (4, 5, 5, 1), (4, 6, 7, 1), (4, 7, 6, 1), (4, 8, 8, 1), (4, 9, 4, 0), (5, 4, 5, 1), (5, 5, 6, 1),
    (5, 5, 7, 1), (5, 6, 8, 1), (5, 7, 8, 1), (5, 8, 4, 0), (5, 8, 9, 1), (5, 9, 5, 0), (6, 4, 7, 1), (6, 5, 8, 1),
    (6, 6, 4, 0), (6, 7, 9, 1), (6, 8, 5, 0), (6, 9, 6, 0), (7, 4, 6, 1), (7, 5, 8, 1), (7, 6, 9, 1), (7, 7, 4, 0),
    (7, 8, 5, 0), (7, 9, 7, 0), (8, 4, 8, 1), (8, 5, 4, 0), (8, 5, 9, 1), (8, 6, 5, 0), (8, 7, 5, 0), (8, 8, 6, 0),
    (8, 8, 7, 0), (8, 9, 8, 0), (9, 4, 4, 0), (9, 5, 5, 0), (9, 6, 6, 0), (9, 7, 7, 0), (9, 8, 8, 0), (9, 9, 9, 0),
    (10, 10, 11, 1), (10, 11, 12, 1), (10, 12, 13, 1), (10, 13, 10, 0), (11, 10, 12, 1), (11, 11, 13, 1), (11, 12, 10, 0),
    (11, 13, 11, 0), (12, 10, 13, 1), (12, 11, 10, 0), (12, 12, 11, 0), (12, 13, 12, 0), (13, 10, 10, 0), (13, 11, 11, 0),
    (13, 12, 12, 0), (13, 13, 13, 0),
]
# state s bounds the half-space of pattern PATTERN[s] (the dual class's subset)
PATTERN = [3, 2, 1, 0, 9, 8, 6, 7, 5, 4, 13, 12, 11, 10]


def derived_terms():
    """``(terms, pattern)`` from the quantum cohomology tables in coverage.py."""
    terms, pattern, base = [], [None] * 14, 0
    for r in (1, 2, 3):
        subs = list(itertools.combinations(range(1, 5), r))
        assert subs == coverage._PATTERNS[base : base + len(subs)]
        parts = [coverage._partition_of(I, r) for I in subs]
        for pi, p in enumerate(parts):
            for xi, x in enumerate(parts):
                for d2, p2 in coverage._ring_mul(r, p, x):
                    terms.append((base + pi, base + xi, base + parts.index(p2), d2))
            pattern[base + pi] = coverage._PATTERNS.index(coverage._subset_of(coverage._dual(p, r), r))
        base += len(subs)
    return terms, pattern


def folded_rows(gate_coords, k_cap):
    """float [k_cap - 1, 14]: the bounds of k = 2 .. k_cap copies of the gate, in ``coverage.region``'s pattern order."""
    a = coverage.alcove_coordinates(np.asarray(gate_coords, dtype=np.float64).reshape(1, 3))[0]
    v = np.array([float(sum(a[i - 1] for i in I)) for I in coverage._PATTERNS])
    w = v.copy()
    rows = np.zeros((max(k_cap - 1, 0), 14))
    for k in range(2, k_cap + 1):
        n = np.full(14, -np.inf)
        for f, x, t, d in TERMS:
            n[t] = max(n[t], w[f] + v[x] - d)
        w = n
        rows[k - 2, PATTERN] = n
    return rows


def first_k_table(gate_coords, target_coords, k_cap, tol):
    """int [G, N]: ``coverage.minimal_prefix`` of k_cap copies of every gate (0 local target, k_cap + 1 not reached)."""
    g = np.asarray(gate_coords, dtype=np.float64).reshape(-1, 3)
    return np.stack([coverage.minimal_prefix(target_coords, np.repeat(c[None], k_cap, axis=0), k_cap, tol) for c in g])


def face_margins(target_coords, gate_coords, k_cap, tol):
    """float [N, faces]: distance of every target from every widened face of 1 .. k_cap copies of the gate under the host model
    (``coverage.contains``: the alcove-point match for k = 1, the finite half-spaces for k >= 2; both alcove points of the target)."""
    g = np.asarray(gate_coords, dtype=np.float64).reshape(1, 3)
    a = coverage.alcove_coordinates(g)[0]
    out = []
    for c, s in coverage.target_sums(target_coords):
        out += [np.abs(np.abs(c[j] - a[j]) - (max(tol, 0.0) + 1e-12)) for j in range(4)]
        for k in range(2, k_cap + 1):
            b = coverage.region(np.repeat(g, k, axis=0))
            out += [np.abs(s[p] - (b[p] - tol)) for p in range(14) if np.isfinite(b[p])]
    return np.stack(out, axis=1)


def counts_of(first_k, k_cap, group_of=None, n_groups=1):
    """int64 [E, G, k_cap + 2] from a first-size table: bin k - 1, bin k_cap local, bin k_cap + 1 not reached."""
    fk = np.asarray(first_k)
    bins = np.where(fk == 0, k_cap, np.where(fk > k_cap, k_cap + 1, fk - 1))
    grp = np.zeros(fk.shape[1], dtype=np.int64) if group_of is None else np.asarray(group_of)
    out = np.zeros((n_groups, fk.shape[0], k_cap + 2), dtype=np.int64)
    for g in range(fk.shape[0]):
        np.add.at(out[:, g, :], (grp, bins[g]), 1)
    return out


class TableCtx:
    """Serves hand-made first-size tables (int [G, N], told apart by N) for the candidates ``coords`` [G, 3] in place of the device."""

    def __init__(self, tables, coords):
        self.coords = np.asarray(coords, dtype=np.float64).reshape(-1, 3)
        self.tables = {np.asarray(t).shape[1]: np.asarray(t, dtype=np.int32) for t in tables}
        self.n_targets = 0
        self.calls = []

    def set_targets(self, targets):
        self.n_targets = len(targets)

    def candidate_scores(self, coords, k_cap, groups=None, n_groups=1, first=0, count=None, want_first=False, tol=1e-7):
        count = self.n_targets - first if count is None else count
        fk = self.tables[self.n_targets][:, first : first + count]
        coords = np.asarray(coords).reshape(-1, 3)
        fk = fk[[int(np.nonzero((self.coords == c).all(axis=1))[0][0]) for c in coords]]  # the rows of the candidates asked for
        self.calls.append((len(coords), count, None if groups is None else np.asarray(groups).copy(), n_groups))
        return counts_of(fk, k_cap, groups, n_groups), (fk.copy() if want_first else None)
