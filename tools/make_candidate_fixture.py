"""Dev tool (CPU): records tests/golden/candidate_first_k.npz, the host model that tests/test_gpu_candidates.py holds
slam_candidate_scores to -- ``coverage.minimal_prefix`` of 64 copies of each of 9 candidate gates for 515 targets (22 s of
``coverage.region`` calls, which is why it is recorded and not recomputed per test run; the test recomputes it when the device's
Weyl coordinates differ from the recorded ones).

  gates   float [9, 3]    sqrt(iSWAP), CNOT, B, iSWAP, the grid's weakest gate (1/32, 0, 0), the identity, three generic gates
  coords  float [515, 3]  500 Haar classes (8 digits), then identity, CNOT, SWAP, iSWAP, B, sqrt(iSWAP), sqrt(SWAP), then pairs of points
                          1e-5 on either side of a k = 2 face: two faces of sqrt(iSWAP), two of the first generic gate
  first_k int8 [9, 515]   0 local target, k, 65 = not reached with 64 copies; tol = pulse_cost.TOL
  face_margin float [9]   per gate, the smallest distance of an explicit target (500 ..) from a widened face of 1 .. 64 copies

usage: tools/make_candidate_fixture.py"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import candidates as tool  # noqa: E402
import candidates_ref as ref  # noqa: E402
from slam_decomposition_amd import coverage, pulse_cost  # noqa: E402
from slam_decomposition_amd.gates import canonical_matrix  # noqa: E402
from slam_decomposition_amd.weyl import c1c2c3  # noqa: E402

GATES = np.array([[0.25, 0.25, 0.0], [0.5, 0.0, 0.0], [0.5, 0.25, 0.0], [0.5, 0.5, 0.0], [1 / 32, 0.0, 0.0], [0.0, 0.0, 0.0],
                  [0.31, 0.17, 0.05], [0.44, 0.21, 0.13], [0.12, 0.07, 0.02]])
NAMED = [(0.0, 0.0, 0.0), (0.5, 0.0, 0.0), (0.5, 0.5, 0.5), (0.5, 0.5, 0.0), (0.5, 0.25, 0.0), (0.25, 0.25, 0.0), (0.25, 0.25, 0.25)]


def face_points(gate, inside, outside):
    """Two Weyl points 1e-5 on either side of the k = 2 face of ``gate`` that the segment inside -> outside crosses."""
    g2 = np.repeat(np.asarray(gate)[None], 2, axis=0)
    lo, hi = np.asarray(inside, dtype=np.float64), np.asarray(outside, dtype=np.float64)
    assert coverage.contains(lo[None], g2, 0.0)[0] and not coverage.contains(hi[None], g2, 0.0)[0]
    d = (hi - lo) / np.linalg.norm(hi - lo)
    for _ in range(60):
        mid = 0.5 * (lo + hi)
        if coverage.contains(mid[None], g2, 0.0)[0]:
            lo = mid
        else:
            hi = mid
    return [lo - 1e-5 * d, lo + 1e-5 * d]


def main():
    haar = tool.haar_targets(500, seed=11)
    off = face_points(GATES[0], [0.3, 0.1, 0.02], [0.3, 0.25, 0.2]) + face_points(GATES[0], [0.7, 0.1, 0.02], [0.7, 0.25, 0.2])
    off += face_points(GATES[6], [0.4, 0.2, 0.05], [0.5, 0.5, 0.5]) + face_points(GATES[6], [0.4, 0.2, 0.05], [0.05, 0.02, 0.0])
    raw = np.concatenate([haar, np.array(NAMED), np.array(off)])
    # the canonical representative, 8 digits: what weyl_c1c2c3 returns for a unitary of the class on the device as on the host
    coords = np.array([c1c2c3(canonical_matrix(*c)) for c in raw])
    assert coords.shape == (515, 3)
    first_k = ref.first_k_table(GATES, coords, 64, pulse_cost.TOL)
    assert first_k.max() == 65 and first_k.min() == 0
    out = os.path.join(ROOT, "tests", "golden", "candidate_first_k.npz")
    face_margin = np.array([ref.face_margins(coords[500:], g, 64, pulse_cost.TOL).min() for g in GATES])
    assert face_margin.min() > 1e-9, face_margin
    np.savez_compressed(out, gates=GATES, coords=coords, first_k=first_k.astype(np.int8), face_margin=face_margin)
    print(out, os.path.getsize(out), "bytes;", [np.bincount(r, minlength=66)[[0, 1, 2, 3, 65]].tolist() for r in first_k])


if __name__ == "__main__":
    main()
