"""Fixed cases of the time-sliced Hamiltonian tests (tests/test_hams_host.py on the CPU, tests/test_gpu_hams.py on the GPU), built once
and shared.  Everything here is NumPy on the host model tests/hams_ref.py."""
import functools
import math

import numpy as np

import ham_cases
import hams_ref
from slam_decomposition_amd import hamiltonian as hm

NAMES = ("smush", "smush1q", "circulator")
SLICES = (1, 2, 3, 8)  # 2: the first product; 3: the first slice with a prefix and a suffix; 8: the cap
Z_FLOOR = ham_cases.Z_FLOOR
SPECIAL = ("zero", "zero_slice", "equal", "one_slice_only", "two_pi", "negative_time", "degenerate")
_DEGENERATE_TERM = {"smush": 2, "smush1q": 2, "circulator": 0}  # a conversion term alone: eigenvalues +g, -g and zeros


def hamiltonian(name, n_slices):
    if name == "smush":
        return hm.ConversionGainSmush(n_slices=n_slices)
    if name == "smush1q":
        return hm.ConversionGainSmush1QPhase(n_slices=n_slices)
    return hm.TimeSliced(hm.CirculatorHamiltonian(), n_slices, sliced=("g_ab", "g_ac", "g_bc"))


def eval_flat(h, x):
    return np.asarray(h.construct_U_flat(*x))


def _roles(terms):
    """(shared strengths, per slice the strengths only it reads, phases)"""
    S = terms["n_slices"]
    per = [set(int(i) for i in terms["s_index"][s]) for s in range(S)]
    shared = set.intersection(*per) if S > 1 else set()
    own = [sorted(p - shared) for p in per]
    phases = sorted(set(int(p) for p in terms["phi_index"].ravel() if p >= 0))
    return sorted(shared), own, phases


def special_rows(name, n_slices):
    """The fixed rows, in the order of SPECIAL: x = 0; one slice with H = 0 among non-zero ones (at S = 1: H = 0 with t = 1); all slices
    equal; a parameter read by one slice only (all other per-slice strengths zero); every strength 2 pi; a negative time; a slice with
    degenerate eigenvalues (slice 0: one conversion term alone)."""
    terms = hamiltonian(name, n_slices).device_terms()
    n, ti, S = terms["n_params"], terms["t_index"], terms["n_slices"]
    shared, own, phases = _roles(terms)
    if S == 1:
        own = [sorted(set(int(i) for i in terms["s_index"][0]))]
        shared = []
    base = np.zeros(n)
    base[ti] = 1.0
    rows = [np.zeros(n)]
    zs = base.copy()
    zs[phases] = 0.3
    for s in range(S):
        if s != S // 2 or S == 1:
            zs[own[s]] = (0.5 + 0.1 * s) if S > 1 else 0.0
    rows.append(zs)
    eq = base.copy()
    for s in range(S):
        for k, i in enumerate(terms["s_index"][s]):
            eq[i] = 0.3 + 0.15 * k
    eq[phases] = 0.4 - 0.2 * np.arange(len(phases))
    eq[ti] = 0.9
    rows.append(eq)
    one = base.copy()
    one[shared] = 0.6
    one[phases] = 0.2
    one[own[S - 1][0]] = 1.1
    rows.append(one)
    big = base.copy()
    big[shared] = 2.0 * math.pi
    for s in range(S):
        big[own[s]] = 2.0 * math.pi
    big[phases] = 0.7
    rows.append(big)
    neg = base.copy()
    every = sorted(set(shared) | set(i for o in own for i in o))
    neg[every] = 0.4 + 0.1 * (np.arange(len(every)) % 7)
    neg[phases] = -1.1
    neg[ti] = -0.8
    rows.append(neg)
    deg = base.copy()
    deg[phases] = 0.3
    for s in range(1, S):
        deg[own[s]] = 0.5 + 0.1 * s
    deg[int(terms["s_index"][0][_DEGENERATE_TERM[name]])] = 0.8
    rows.append(deg)
    return np.stack(rows)


@functools.lru_cache(maxsize=None)
def parity_items(name, n_slices):
    """(terms, targets [2], x [M, n], target_of [M], kept [len(SPECIAL)]): per target the special rows that pass the |z| floor and 8 random
    rows (uniform in [-pi, pi), the time included) that pass it, shuffled so that target_of is out of order.  Target 0 is a random
    unitary near the identity, target 1 a random point of the pulse.  kept[i]: the number of targets special row i is kept for."""
    rng = np.random.default_rng(31000 + 100 * NAMES.index(name) + n_slices)
    h = hamiltonian(name, n_slices)
    terms = h.device_terms()
    d, n = terms["dim"], terms["n_params"]
    g = rng.normal(size=(d, d)) + 1j * rng.normal(size=(d, d))
    g = g + g.conj().T
    targets = np.stack([hm.expm_hermitian(0.5 * g / np.linalg.norm(g, 2), 1.0), hams_ref.unitary(terms, rng.uniform(0.0, 1.0, n))])
    special = special_rows(name, n_slices)
    kept = np.zeros(len(special), dtype=np.int64)
    xs, tof = [], []
    for t in range(2):
        for i, row in enumerate(special):
            if 1.0 - hams_ref.loss_grad(terms, row, targets[t])[0] >= Z_FLOOR:
                xs.append(row)
                tof.append(t)
                kept[i] += 1
        count = 0
        while count < 8:
            row = rng.uniform(-math.pi, math.pi, n)
            if 1.0 - hams_ref.loss_grad(terms, row, targets[t])[0] >= Z_FLOOR:
                xs.append(row)
                tof.append(t)
                count += 1
    order = rng.permutation(len(xs))
    return terms, targets, np.stack(xs)[order], np.array(tof, dtype=np.int32)[order], kept


@functools.lru_cache(maxsize=None)
def parity_reference(name, n_slices, square):
    terms, targets, x, tof, _ = parity_items(name, n_slices)
    return hams_ref.batch(terms, x, targets, tof, square)


@functools.lru_cache(maxsize=None)
def big_items():
    """4096 rows of the sliced circulator at S = 3 against two targets: more items than wavefronts, so every wavefront takes several."""
    rng = np.random.default_rng(4096)
    terms, targets, _, _, _ = parity_items("circulator", 3)
    x = rng.uniform(-1.5, 1.5, (4096, terms["n_params"]))
    tof = rng.integers(0, 2, 4096).astype(np.int32)
    return terms, targets, x, tof


@functools.lru_cache(maxsize=None)
def big_reference(square):
    terms, targets, x, tof = big_items()
    return hams_ref.batch(terms, x, targets, tof, square)


@functools.lru_cache(maxsize=None)
def local_case():
    """ConversionGainSmush1QPhase at S = 4: p* uniform in [0.5, 1.5)^17, its unitary as the target, 8 start points within +-0.05 of p*.
    The range keeps the pulse long enough for its slices not to commute: the slices' drives are told apart by commutators of order
    (t / S)^2, so around a short pulse the loss is nearly flat along their differences.  Measured on the model (central differences of
    its gradient at p*, SquareCost): with p* in [0, 1)^17 (t* = 0.47) the Hessian's eigenvalues go down to 7e-10, 5e-7, 7e-7 under a
    largest of 1.1, and SciPy BFGS on the model stops above 1e-10 from 5 of 8 such starts; with this range the smallest is 2e-5
    under 5.0 (beside the two zeros of the description's gauge freedom) and SciPy reaches 1e-10 from 8 of 8."""
    rng = np.random.default_rng(12)
    h = hamiltonian("smush1q", 4)
    terms = h.device_terms()
    p = rng.uniform(0.5, 1.5, terms["n_params"])
    x0 = p + rng.uniform(-0.05, 0.05, (8, terms["n_params"]))
    return terms, eval_flat(h, p)[None], p, x0[None]


SEARCH_SLICES = 4
SEARCH_SEED = 7
SEARCH_RESTARTS = 16
SEARCH_PLANTED_SEED = 2024


def search_hamiltonian():
    return hamiltonian("smush1q", SEARCH_SLICES)


def search_range():
    """the four phases in [-pi, pi), the strengths gc, gg, gz1, gz2, gx_s, gy_s in [0, 1.5), t in [1, 1]"""
    n_drive = 2 * SEARCH_SLICES
    return np.array([-math.pi] * 4 + [0.0] * (4 + n_drive) + [1.0]), np.array([math.pi] * 4 + [1.5] * (4 + n_drive) + [1.0])


@functools.lru_cache(maxsize=None)
def search_targets():
    """Two planted targets: the pulse at points drawn from the search range."""
    low, high = search_range()
    rng = np.random.default_rng(SEARCH_PLANTED_SEED)
    h = search_hamiltonian()
    return np.stack([eval_flat(h, rng.uniform(low, high)) for _ in range(2)])


def scipy_minimize(terms, target, x0, square=False, gtol=1e-9):
    """SciPy BFGS on the host model with its analytic gradient; returns (loss, x, iterations)."""
    from scipy.optimize import minimize

    res = minimize(lambda x: hams_ref.loss_grad(terms, x, target, square)[:2], x0, jac=True, method="BFGS", options={"gtol": gtol, "maxiter": 2500})
    return float(res.fun), res.x, int(res.nit)
