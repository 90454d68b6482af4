"""The fixed cases of the three-qubit tests (tests/test_q3_host.py, tests/test_gpu_q3.py), drawn from seeded NumPy generators so that
the CPU checks and the GPU tests see the same targets and start points."""
import functools
import math

import numpy as np

import q3_ref

CX = np.array([[1, 0, 0, 0], [0, 0, 0, 1], [0, 0, 1, 0], [0, 1, 0, 0]], dtype=np.complex128)  # qiskit CXGate: control = bit 0
_r = 1.0 / math.sqrt(2.0)
SQISWAP = np.array([[1, 0, 0, 0], [0, _r, 1j * _r, 0], [0, 1j * _r, _r, 0], [0, 0, 0, 1]], dtype=np.complex128)  # RiSwapGate(1/2)

TOFFOLI_EDGES = [(1, 2), (0, 2), (1, 2), (0, 2), (0, 1), (0, 1)]
LINE_EDGES = [(0, 1), (1, 2), (0, 1)]  # edge_params [[(0, 1)], [(1, 2)]] at k = 3
ALL_EDGES = [(0, 1), (1, 0), (0, 2), (2, 0), (1, 2), (2, 1)]


def haar(rng, dim):
    """Haar-random unitary: QR of a Ginibre matrix with the phases of R's diagonal moved into Q."""
    z = (rng.standard_normal((dim, dim)) + 1j * rng.standard_normal((dim, dim))) / math.sqrt(2.0)
    q, r = np.linalg.qr(z)
    d = np.diagonal(r)
    return q * (d / np.abs(d))


@functools.lru_cache(maxsize=None)
def local_cases():
    """Test 3: 32 targets of the sqrt(iSWAP) line template at k = 3, with start points 0.05 N(0, 1) away from their angles.
    Returns (targets [32, 8, 8], x0 [32, 27])."""
    rng = np.random.default_rng(3301)
    true = rng.uniform(0.0, 2.0 * math.pi, (32, 27))
    targets = np.stack([q3_ref.unitary(x, [SQISWAP] * 3, LINE_EDGES) for x in true])
    return targets, true + 0.05 * rng.standard_normal((32, 27))


@functools.lru_cache(maxsize=None)
def reachable_targets():
    """Test 5: 16 targets of the same template at random angles: [16, 8, 8]."""
    rng = np.random.default_rng(3302)
    return np.stack([q3_ref.unitary(x, [SQISWAP] * 3, LINE_EDGES) for x in rng.uniform(0.0, 2.0 * math.pi, (16, 27))])


@functools.lru_cache(maxsize=None)
def parity_case(k):
    """Test 1 at k gates: gate table (CX, sqrt(iSWAP), one Haar 4x4), gate indices and edges cycling through all six ordered pairs,
    64 Haar 8x8 targets and 64 parameter rows uniform in [-pi, 3 pi)."""
    rng = np.random.default_rng(3310 + k)
    gates = np.stack([CX, SQISWAP, haar(rng, 4)])
    gate_index = [(j + k) % 3 for j in range(k)]
    edges = [ALL_EDGES[(j + 2 * k) % 6] for j in range(k)]
    targets = np.stack([haar(rng, 8) for _ in range(64)])
    x = rng.uniform(-math.pi, 3.0 * math.pi, (64, 9 + 6 * k))
    return gates, gate_index, edges, targets, x
