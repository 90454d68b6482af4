"""Makes tests/golden/reference_smush_coverage.json from the parallel-drive ("smush") coverage sets the reference ships as DATA
(src/slam/data/polytopes/polytope_coverage_[...]smush.pkl and src/slam/data/extended_results.json, written by
utils/gates/parallel_drive_volume.py:340-451 for six ConversionGainGates).

The pickles are read as numbers with the restricted unpickler of tools/make_reference_coverage_fixture.py (no monodromy, nothing of the
reference is imported or run).  Per gate: (gc, gg, t), the pickle's gate key, the recorded extended_results.json rows, the stored
scores [haar_score, cnot_score, swap_score]; per k < k_full: the base region's convex pieces as inequality / equality rows (small
integers) and the two hulls by their VERTICES -- the reference's own samples rounded to fractions of denominator <= 10 000
(parallel_drive_volume.py:351-353), so a vertex is stored exactly as [numerator, denominator] triples.  The tool asserts, in exact
rational arithmetic, that the vertices reproduce every inequality row of the pickle: every vertex satisfies every row, every row is
tight on at least three vertices that span its plane, and every vertex is the intersection of the rows tight on it.

usage (in the build container only; the GPU box has no reference tree): python3 tools/make_reference_smush_fixture.py
"""
import glob
import itertools
import json
import math
import os
import sys
from fractions import Fraction

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_reference_coverage_fixture import _num, _Restricted  # noqa: E402

SRC = "/root/reference/src/slam/data"
OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "reference_smush_coverage.json")
GATES = {  # name: (gc, gg, t, k_full)   parallel_drive_volume.py:91-96
    "iSwap": (math.pi / 2, 0.0, 1.0, 3), "sqiSwap": (math.pi / 2, 0.0, 0.5, 3), "CNOT": (math.pi / 4, math.pi / 4, 1.0, 3),
    "sqCNOT": (math.pi / 4, math.pi / 4, 0.5, 6), "B": (3 * math.pi / 8, math.pi / 8, 1.0, 2), "sqB": (3 * math.pi / 8, math.pi / 8, 0.5, 4),
}


def _frac(v) -> Fraction:
    return v if isinstance(v, Fraction) else Fraction(v)


def _rows(cp, key):
    return [[_frac(x) for x in row] for row in cp.__dict__.get(key, [])]


def _det3(M):
    return (M[0][0] * (M[1][1] * M[2][2] - M[1][2] * M[2][1]) - M[0][1] * (M[1][0] * M[2][2] - M[1][2] * M[2][0])
            + M[0][2] * (M[1][0] * M[2][1] - M[1][1] * M[2][0]))


def _vertices(ineq):
    """Vertices of {m : b + a . m >= 0 for every row} in exact arithmetic: the float halfspace intersection locates them, each is
    then solved exactly (Cramer) from three independent rows tight on it."""
    from scipy.optimize import linprog
    from scipy.spatial import HalfspaceIntersection

    A = np.array([[float(x) for x in r[1:]] for r in ineq])
    b = np.array([float(r[0]) for r in ineq])
    s = np.linalg.norm(A, axis=1)
    A, b = A / s[:, None], b / s  # unit normals (the rows hold integers up to ~1e32)
    # Chebyshev centre: max r subject to -a . m + r <= b
    res = linprog([0, 0, 0, -1], A_ub=np.concatenate([-A, np.ones((len(b), 1))], axis=1), b_ub=b, bounds=[(None, None)] * 3 + [(0, 1)])
    assert res.status == 0 and res.x[3] > 1e-9, "empty or flat hull"
    hs = HalfspaceIntersection(np.concatenate([-A, -b[:, None]], axis=1), res.x[:3])
    out, tried = set(), set()
    for p in hs.intersections:
        tight = [i for i in range(len(ineq)) if abs(b[i] + A[i] @ p) <= 1e-6]
        for i, j, k in itertools.combinations(tight, 3):  # every exact vertex near p: near-coincident vertices are kept apart
            if (i, j, k) in tried:
                continue
            tried.add((i, j, k))
            M = [ineq[i][1:], ineq[j][1:], ineq[k][1:]]
            det = _det3(M)
            if det == 0:
                continue
            rhs = [-ineq[i][0], -ineq[j][0], -ineq[k][0]]
            v = tuple(_det3([[rhs[r] if cc == c else M[r][cc] for cc in range(3)] for r in range(3)]) / det for c in range(3))
            if v not in out and all(r[0] + r[1] * v[0] + r[2] * v[1] + r[3] * v[2] >= 0 for r in ineq):
                out.add(v)
    return sorted(out)


def _check(ineq, verts):
    """The vertices reproduce the rows exactly (see the module docstring)."""
    for r in ineq:
        vals = [r[0] + sum(r[j + 1] * v[j] for j in range(3)) for v in verts]
        assert min(vals) >= 0, "a vertex violates a row"
        on = [v for v, x in zip(verts, vals) if x == 0]
        assert len(on) >= 3, "a row is not a facet of the vertices' hull"
        d = [[float(on[i][j] - on[0][j]) for j in range(3)] for i in range(1, len(on))]
        assert np.linalg.matrix_rank(np.array(d), tol=1e-12) == 2, "a row's tight vertices do not span its plane"
    for v in verts:
        tight = [r[1:] for r in ineq if r[0] + sum(r[j + 1] * v[j] for j in range(3)) == 0]
        assert np.linalg.matrix_rank(np.array([[float(x) for x in t] for t in tight]), tol=1e-12) == 3, "not a vertex"
        assert all(x.denominator <= 10000 for x in v), "a vertex is no fraction of denominator <= 10 000"


def _enc(x: Fraction):
    return x.numerator if x.denominator == 1 else [x.numerator, x.denominator]


def main():
    rec = json.load(open(os.path.join(SRC, "extended_results.json")))
    out = {}
    for name, (gc, gg, t, k_full) in GATES.items():
        lo, hi = sorted((gc, gg))
        key = f"2QGate({lo * t:.8f}, {hi * t:.8f}, 1.00000000)"  # ConversionGainGate(0, 0, min, max, t).normalize_duration(1)
        paths = [p for p in glob.glob(os.path.join(SRC, "polytopes", "polytope_coverage_*smush.pkl")) if key in os.path.basename(p)]
        assert len(paths) == 1, (name, key, paths)
        coverage, gate_hash, scores = _Restricted(open(paths[0], "rb")).load()
        assert list(gate_hash.keys()) == [key]
        rows = rec[name]
        assert sorted(int(k) for k in rows) == list(range(1, k_full + 1))
        per_k = {}
        for k in range(1, k_full):
            e = coverage[k].__dict__
            assert len(e["operations"]) == k and e["cost"] == k
            cps = e["convex_subpolytopes"]
            base, hulls = cps[:-2], cps[-2:]
            stored_base = [{"inequalities": [[_enc(x) for x in r] for r in _rows(cp, "inequalities")],
                            "equalities": [[_enc(x) for x in r] for r in _rows(cp, "equalities")]} for cp in base]
            stored_hulls = []
            for cp in hulls:
                ineq = _rows(cp, "inequalities")
                assert not _rows(cp, "equalities")
                verts = _vertices(ineq)
                _check(ineq, verts)
                stored_hulls.append({"vertices": [[_enc(x) for x in v] for v in verts], "n_rows": len(ineq)})
            per_k[str(k)] = {"base": stored_base, "hulls": stored_hulls}
        out[name] = {"gc": gc, "gg": gg, "t": t, "k_full": k_full, "gate_key": key, "rows": rows,
                     "scores": [float(_num(scores[0])), int(scores[1]), int(scores[2])], "regions": per_k}
    with open(OUT, "w") as f:
        json.dump(out, f, separators=(",", ":"))
    print(f"{len(out)} gates -> {OUT} ({os.path.getsize(OUT)} bytes)")
    for name, v in out.items():
        print(name, v["scores"], {k: [len(h["vertices"]) for h in r["hulls"]] for k, r in v["regions"].items()})


if __name__ == "__main__":
    main()
