"""The fixed cases of the mixed three-qubit tests (tests/test_q3m_host.py, tests/test_gpu_q3m.py), drawn from seeded NumPy generators so
that the CPU checks and the GPU tests see the same templates, targets and start points."""
import functools
import itertools
import math

import numpy as np

import q3m_ref
from q3_cases import CX, SQISWAP, haar
from slam_decomposition_amd.gates import CCZGate, VSwap

TRIPLES = list(itertools.permutations((0, 1, 2)))  # all six ordered triples
ALL_PAIRS = [(0, 1), (1, 0), (0, 2), (2, 0), (1, 2), (2, 1)]


class Case:
    """A template as the C entry points take it -- gates2 [G2, 4, 4], gates3 [G3, 8, 8], per position arity, table index and qubits --
    and as the model takes it -- per position the matrix and the edge."""

    def __init__(self, gates2, gates3, positions):
        """positions: [(arity, table index, edge)]"""
        self.gates2 = np.asarray(gates2, dtype=np.complex128).reshape(-1, 4, 4)
        self.gates3 = np.asarray(gates3, dtype=np.complex128).reshape(-1, 8, 8)
        self.arity = [p[0] for p in positions]
        self.index = [p[1] for p in positions]
        self.edges = [tuple(p[2]) for p in positions]
        self.qubits = [e + (0,) * (3 - len(e)) for e in self.edges]
        self.model_gates = [(self.gates3 if a == 3 else self.gates2)[i] for a, i in zip(self.arity, self.index)]
        self.n = q3m_ref.n_params(self.edges)

    def description(self):
        return self.gates2, self.gates3, self.arity, self.index, self.qubits


@functools.lru_cache(maxsize=None)
def parity_template(name):
    """The templates of the parity test.
    one-<i>: k = 1, a Haar 8x8 on the i-th of the six triples (every table entry and every row index matters);
    mixed5:  k = 5, arities [3, 2, 3, 2, 2], two Haar 8x8 and two 4x4 (sqrt(iSWAP), a Haar 4x4); over the positions every qubit occurs
             as a and as b, and as c as far as two triples allow (qubits 2 and 1; all six triples are in one-<i>);
    ten3:    10 three-qubit positions, the three gates of a full table, all six triples: n = 99, the parameter cap;
    wide14:  k = 14 with three-qubit positions at 3 and 10 and CX, sqrt(iSWAP), a Haar 4x4 elsewhere: n = 99."""
    rng = np.random.default_rng(3400 + sum(map(ord, name)))
    if name.startswith("one-"):
        return Case([], [haar(rng, 8)], [(3, 0, TRIPLES[int(name[4:])])])
    if name == "mixed5":
        return Case([SQISWAP, haar(rng, 4)], [haar(rng, 8), haar(rng, 8)],
                    [(3, 0, (0, 1, 2)), (2, 0, (1, 2)), (3, 1, (2, 0, 1)), (2, 1, (2, 1)), (2, 0, (1, 0))])
    if name == "ten3":
        return Case([], [haar(rng, 8) for _ in range(3)], [(3, j % 3, TRIPLES[(j + 1) % 6]) for j in range(10)])
    if name == "wide14":
        g3 = [haar(rng, 8), haar(rng, 8)]
        pos = [(3, 0, (1, 2, 0)) if j == 3 else (3, 1, (2, 1, 0)) if j == 10 else (2, j % 3, ALL_PAIRS[j % 6]) for j in range(14)]
        return Case([CX, SQISWAP, haar(rng, 4)], g3, pos)
    raise KeyError(name)


PARITY_NAMES = [f"one-{i}" for i in range(6)] + ["mixed5", "ten3", "wide14"]


@functools.lru_cache(maxsize=None)
def parity_items(name):
    """8 Haar 8x8 targets and 8 parameter rows uniform in [-pi, 3 pi) for the template: the first 8 draws with |Tr(T^+ W)| / 8 >= 0.05
    (BasicCost's gradient is singular at 0; tests/test_gpu_q3.py drops such items after the fact, and a Haar pair is one with
    probability 0.15).  Returns (targets [8, 8, 8], x [8, n])."""
    case = parity_template(name)
    rng = np.random.default_rng(3500 + sum(map(ord, name)))
    targets, xs = [], []
    while len(xs) < 8:
        t, x = haar(rng, 8), rng.uniform(-math.pi, 3.0 * math.pi, case.n)
        if q3m_ref.overlap(q3m_ref.unitary(x, case.model_gates, case.edges), t) >= 0.05:
            targets.append(t)
            xs.append(x)
    return np.stack(targets), np.stack(xs)


@functools.lru_cache(maxsize=None)
def vswap_case():
    """[VSwap, sqrt(iSWAP), VSwap] on (0, 1, 2), (0, 1), (2, 1, 0): n = 33."""
    return Case([SQISWAP], [VSwap().to_matrix()], [(3, 0, (0, 1, 2)), (2, 0, (0, 1)), (3, 0, (2, 1, 0))])


@functools.lru_cache(maxsize=None)
def local_cases():
    """8 targets of ``vswap_case`` at known angles, start points 0.05 N(0, 1) away from them (the size tests/q3_cases.local_cases
    uses).  Returns (targets [8, 8, 8], x0 [8, 33])."""
    case = vswap_case()
    rng = np.random.default_rng(3601)
    true = rng.uniform(0.0, 2.0 * math.pi, (8, case.n))
    targets = np.stack([q3m_ref.unitary(x, case.model_gates, case.edges) for x in true])
    return targets, true + 0.05 * rng.standard_normal((8, case.n))


@functools.lru_cache(maxsize=None)
def ccz_cx_case():
    """base_gates [CCZ, CX] on edge_params [[(0, 1, 2)], [(0, 1)]] at k = 2: n = 24."""
    return Case([CX], [CCZGate().to_matrix()], [(3, 0, (0, 1, 2)), (2, 0, (0, 1))])


@functools.lru_cache(maxsize=None)
def ccz_cx_targets():
    """8 targets of ``ccz_cx_case`` at random angles: [8, 8, 8]."""
    case = ccz_cx_case()
    rng = np.random.default_rng(3602)
    return np.stack([q3m_ref.unitary(x, case.model_gates, case.edges) for x in rng.uniform(0.0, 2.0 * math.pi, (8, case.n))])
