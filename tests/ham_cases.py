"""Fixed cases of the Hamiltonian-template tests (tests/test_ham_host.py on the CPU, tests/test_gpu_ham.py on the GPU), built once and
shared.  Everything here is NumPy on the host model tests/ham_ref.py."""
import functools
import json
import math
import os

import numpy as np

import ham_ref
from slam_decomposition_amd import hamiltonian as hm
from slam_decomposition_amd.gates import CParitySwap, DeltaSwap, VSwap

DEVICE_HAMILTONIANS = ("snail", "conversion_gain", "conversion_gain_phase", "circulator", "delta")
_CLASSES = {"snail": hm.SnailEffectiveHamiltonian, "conversion_gain": hm.ConversionGainHamiltonian,
            "conversion_gain_phase": hm.ConversionGainPhaseHamiltonian, "circulator": hm.CirculatorHamiltonian,
            "delta": hm.DeltaConversionGainHamiltonian}
Z_FLOOR = 0.05  # rows with |z| below it are left out: BasicCost is not differentiable at z = 0 (tests/q3m_cases.py applies the same)


def hamiltonian(name):
    return _CLASSES[name]()


def _random_unitary(rng, d):
    q, r = np.linalg.qr(rng.normal(size=(d, d)) + 1j * rng.normal(size=(d, d)))
    return q * (np.diag(r) / np.abs(np.diag(r)))


def _strength_and_phase_indices(terms):
    return sorted(set(int(s) for s in terms["s_index"])), sorted(set(int(p) for p in terms["phi_index"] if p >= 0))


def special_rows(name):
    """x = 0; one non-zero strength; the DeltaSwap point (its three conversion drives, where the Hamiltonian has them); every strength
    2 pi; a negative time (where the time is a parameter, else a negative strength)."""
    terms = hamiltonian(name).device_terms()
    n, ti = terms["n_params"], terms["t_index"]
    s_idx, p_idx = _strength_and_phase_indices(terms)
    base = np.zeros(n)
    if ti >= 0:
        base[ti] = 1.0
    rows = [np.zeros(n)]
    one = base.copy()
    one[s_idx[-1]] = 1.3
    rows.append(one)
    ds = base.copy()
    g = math.pi / (3.0 * math.sqrt(3.0) / 2.0)
    if name == "circulator":
        ds[:] = [float(p) for p in DeltaSwap().params]
    elif name == "delta":
        ds[[9, 10, 11]] = g
        ds[[7, 8]] = [math.pi / 2, math.pi / 2]
    else:
        ds[s_idx] = g
        ds[p_idx] = math.pi / 2
    rows.append(ds)
    big = base.copy()
    big[s_idx] = 2.0 * math.pi
    big[p_idx] = 0.7
    rows.append(big)
    neg = base.copy()
    neg[s_idx] = 0.4 + 0.1 * np.arange(len(s_idx))
    neg[p_idx] = -1.1
    if ti >= 0:
        neg[ti] = -0.8
    else:
        neg[s_idx[0]] = -0.9
    rows.append(neg)
    return np.stack(rows)


@functools.lru_cache(maxsize=None)
def parity_items(name):
    """(terms, targets [2], x [M, n], target_of [M]) of the evaluation-parity test: per target the special rows and 8 random rows
    (uniform in [-pi, pi), the time included) that pass the |z| floor, the items then shuffled so that target_of is out of order.
    Target 0 is a random unitary near the identity, target 1 a random point of the Hamiltonian."""
    rng = np.random.default_rng(20260 + DEVICE_HAMILTONIANS.index(name))
    h = hamiltonian(name)
    terms = h.device_terms()
    d, n = terms["dim"], terms["n_params"]
    g = rng.normal(size=(d, d)) + 1j * rng.normal(size=(d, d))
    g = g + g.conj().T
    targets = np.stack([hm.expm_hermitian(0.5 * g / np.linalg.norm(g, 2), 1.0), ham_ref.unitary(terms, rng.uniform(0.0, 1.0, n))])
    special = special_rows(name)
    xs, tof = [], []
    for t in range(2):
        kept_special = 0
        for row in special:
            if 1.0 - ham_ref.loss_grad(terms, row, targets[t])[0] >= Z_FLOOR:
                xs.append(row)
                tof.append(t)
                kept_special += 1
        assert kept_special >= 3
        kept = 0
        while kept < 8:
            row = rng.uniform(-math.pi, math.pi, n)
            if 1.0 - ham_ref.loss_grad(terms, row, targets[t])[0] >= Z_FLOOR:
                xs.append(row)
                tof.append(t)
                kept += 1
    order = rng.permutation(len(xs))
    return terms, targets, np.stack(xs)[order], np.array(tof, dtype=np.int32)[order]


@functools.lru_cache(maxsize=None)
def parity_reference(name, square):
    terms, targets, x, tof = parity_items(name)
    return ham_ref.batch(terms, x, targets, tof, square)


@functools.lru_cache(maxsize=None)
def big_items():
    """4096 rows of the circulator against two targets: more items than wavefronts, so every wavefront takes several."""
    rng = np.random.default_rng(4096)
    terms, targets, _, _ = parity_items("circulator")
    x = rng.uniform(-2.0, 2.0, (4096, terms["n_params"]))
    tof = rng.integers(0, 2, 4096).astype(np.int32)
    return terms, targets, x, tof


@functools.lru_cache(maxsize=None)
def big_reference(square):
    terms, targets, x, tof = big_items()
    return ham_ref.batch(terms, x, targets, tof, square)


@functools.lru_cache(maxsize=None)
def local_case():
    """The delta Hamiltonian: p* uniform in [0, 1)^12, its unitary as the target, 8 start points within +-0.05 of p*."""
    rng = np.random.default_rng(12)
    terms = hamiltonian("delta").device_terms()
    p = rng.uniform(0.0, 1.0, 12)
    x0 = p + rng.uniform(-0.05, 0.05, (8, 12))
    return terms, ham_ref.unitary(terms, p)[None], p, x0[None]


SEARCH_SEED = 5
SEARCH_RESTARTS = 64
SEARCH_NAMES = ("vswap", "deltaswap", "cparityswap")


def search_targets():
    return np.stack([VSwap().to_matrix(), DeltaSwap().to_matrix(), CParitySwap().to_matrix()])


def search_range():
    """phases in [-pi, pi), strengths in [0, 2), t in [1, 1]"""
    return np.array([-math.pi] * 3 + [0.0] * 3 + [1.0]), np.array([math.pi] * 3 + [2.0] * 3 + [1.0])


def error_gate_target():
    spec = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "error_gate_target.json")))
    t = np.zeros((spec["dim"], spec["dim"]), dtype=np.complex128)
    for r, c in spec["ones"]:
        t[r, c] = 1.0
    return t


def equal_up_to_phase(u, t):
    z = np.trace(np.asarray(t).conj().T @ np.asarray(u))
    return float(np.max(np.abs(np.asarray(u) * (abs(z) / z) - np.asarray(t))))


def scipy_minimize(terms, target, x0, square=False, gtol=1e-9):
    """SciPy BFGS on the host model with its analytic gradient; returns (loss, x, iterations)."""
    from scipy.optimize import minimize

    res = minimize(lambda x: ham_ref.loss_grad(terms, x, target, square)[:2], x0, jac=True, method="BFGS", options={"gtol": gtol, "maxiter": 2500})
    return float(res.fun), res.x, int(res.nit)
