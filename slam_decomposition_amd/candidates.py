"""Which two-qubit basis gate should this hardware, or this circuit, use?  Candidate scoring and winner selection.

The reference answers in four steps: a grid of conversion-gain candidates (``build_gates``, src/slam/utils/gates/bare_candidates.py:47-69);
three coverage scores per candidate -- the Haar-expected gate count and the first sizes that reach CNOT and SWAP (``collect_data``,
bare_candidates.py:75-126); gate counts turned into durations under a speed-limit curve plus a 1Q gate time (``atomic_cost_scaling``,
src/slam/utils/gates/duraton_scaling.py:16-104; ``SpeedLimitedGate``, snail_death_gate.py:108-158); and the winner
(``pick_winner``, winner_selection.py:17-144), overall or against the 2Q blocks of a circuit, for the whole circuit or per coupling-map
edge (``SpeedGateSubstitute``, src/slam/utils/transpiler_pass/speed_limit_pass.py:104-314).

Here the scores of ALL candidates come from one device call, ``slam_candidate_scores``: per (candidate, target) the smallest number of
applications that reaches the target, the coverage rows derived on the device from the candidates' Weyl coordinates -- no host-built
table per candidate.  Everything above the integer counts is summed here, in a fixed order, so results are bit-reproducible.

Decisions where the reference leaves a choice or its behaviour is an accident:
  * durations solve the intersection of the gate's ray with the speed-limit curve exactly (closed form / bracketed root), not on the
    reference's 800-point grid with a growing tolerance;
  * ``pick_winner`` resolves ties to the LOWEST candidate index (the reference's order is that of an HDF5 group);
  * a local candidate has Haar score ``inf`` (the reference skips the identity); an unreached target makes a score ``inf``;
  * a local target costs 0, as in ``pulse_cost``;
  * the measured hardware speed-limit spline is not shipped: ``"hardware"`` needs the caller's curve.
"""
from __future__ import annotations

import logging
import math
from dataclasses import dataclass
from typing import Callable, Dict, List, NamedTuple, Optional, Sequence, Tuple, Union

import numpy as np

from . import coverage, pulse_cost, runtime
from .gates import ConversionGainGate, CXGate, SwapGate, gate_matrix
from .weyl import c1c2c3

CX = CXGate().to_matrix()
SWAP = SwapGate().to_matrix()
STRATEGIES = ("basic_overall", "lambda_weight", "weighted_overall", "weighted_pairwise")
_HALF_PI = np.pi / 2


# ---- gates and grids ---------------------------------------------------------------------------------------------------------------
def _grid(strengths, splits, elim_extra_weyl: bool):
    gates: List[ConversionGainGate] = []
    coordinate_list: List[list] = []
    seen: Dict[tuple, int] = {}
    index = np.zeros((len(strengths), len(splits)), dtype=np.int64)
    for a, k in enumerate(strengths):
        inner: list = []
        for b, p in enumerate(splits):
            gate = ConversionGainGate(0, 0, p * k * np.pi, (1 - p) * k * np.pi)
            c = list(c1c2c3(gate.to_matrix()))
            if elim_extra_weyl and c[0] > 0.5:
                c[0] = -1 * c[0] + 1
            key = tuple(c)
            if key in seen:
                index[a, b] = seen[key]
                continue
            seen[key] = index[a, b] = len(gates)
            inner.append(c)
            gates.append(gate)
        coordinate_list.append(inner)
    return gates, coordinate_list, index


def build_gates(elim_extra_weyl: bool = True) -> Tuple[List[ConversionGainGate], List[list]]:
    """bare_candidates.py:47-69: ``ConversionGainGate(0, 0, p k pi, (1 - p) k pi)`` for 17 strengths k in [0, 1/2] x 21 splits p in
    [0, 1], skipping a gate whose Weyl coordinates (c1 folded to <= 1/2) were seen before.  Returns (gates, coordinates per strength):
    177 gates, the identity first."""
    gates, coordinate_list, _ = _grid(np.linspace(0, 0.5, 17), np.linspace(0, 1, 21), elim_extra_weyl)
    return gates, coordinate_list


def candidate_grid(n_strength: int = 17, n_split: int = 21, max_strength: float = 0.5) -> Tuple[List[ConversionGainGate], np.ndarray]:
    """``build_gates`` at any resolution: ``(gates, index)`` with ``index[a, b]`` the position in ``gates`` of the gate that stands for
    grid point (strength a, split b) -- its own, or the earlier gate of the same Weyl class -- so that ``scores[index]`` is a score
    map over the (strength, split) grid."""
    if int(n_strength) < 1 or int(n_split) < 1:
        raise ValueError("the grid needs at least one strength and one split")
    gates, _, index = _grid(np.linspace(0, float(max_strength), int(n_strength)), np.linspace(0, 1, int(n_split)), True)
    return gates, index


def gate_coords(gates: Sequence) -> np.ndarray:
    """Weyl coordinates [G, 3] (units of pi, 8 digits) of gate objects / 4x4 arrays; a [G, 3] float array is taken as coordinates."""
    if isinstance(gates, np.ndarray) and gates.ndim == 2 and gates.shape[1] == 3 and not np.iscomplexobj(gates):
        return np.ascontiguousarray(gates, dtype=np.float64)
    return np.array([c1c2c3(gate_matrix(g)) for g in gates], dtype=np.float64).reshape(-1, 3)


def is_local(coords) -> np.ndarray:
    """bool[G]: the class of the identity (either alcove point vanishes)."""
    c = np.asarray(coords, dtype=np.float64).reshape(-1, 3)
    return (np.max(np.abs(coverage.alcove_coordinates(c)), axis=1) < 1e-8) | (np.max(np.abs(coverage.alcove_coordinates(c, 0.5)), axis=1) < 1e-8)


# ---- scores ------------------------------------------------------------------------------------------------------------------------
@dataclass
class CandidateScores:
    """What ``score_candidates`` returns.  ``counts`` int64 [E, G, k_cap + 2]: per target group and candidate, bin k - 1 = targets first
    reached with k applications, bin ``k_cap`` = local targets (no gate), bin ``k_cap + 1`` = targets not reached within ``k_cap``;
    ``n_targets`` int64 [E]; ``haar_score`` float [G] (one group) or [E, G]: sum_k k count_k / n, ``inf`` where a target is unreached
    and for a local candidate; ``volumes`` float [E, G, k_cap]: fraction of the targets reached with at most k applications;
    ``named_scores``: name -> int64 [G], the first size that reaches the named target (0 local, ``k_cap + 1`` not reached);
    ``first_k`` int32 [G, N] or None."""

    gates: list
    coords: np.ndarray
    counts: np.ndarray
    n_targets: np.ndarray
    k_cap: int
    haar_score: np.ndarray
    volumes: np.ndarray
    named_scores: Dict[str, np.ndarray]
    first_k: Optional[np.ndarray] = None

    @classmethod
    def from_counts(cls, gates, counts, named_scores=None, first_k=None, coords=None) -> "CandidateScores":
        """The derived fields from the integer counts ([G, k_cap + 2] or [E, G, k_cap + 2]), on the host."""
        counts = np.asarray(counts, dtype=np.int64)
        one_group = counts.ndim == 2
        if one_group:
            counts = counts[None]
        E, G, nb = counts.shape
        k_cap = nb - 2
        gates = list(gates)
        coords = gate_coords(gates) if coords is None else np.asarray(coords, dtype=np.float64).reshape(-1, 3)
        if len(coords) != G:
            raise ValueError(f"{len(coords)} gates for counts of {G} candidates")
        n = counts.sum(axis=2)
        if G and np.any(n != n[:, :1]):
            raise ValueError("every candidate of a group must account for the same number of targets")
        n_targets = n[:, 0] if G else np.zeros(E, dtype=np.int64)
        # sum_k k count_k: integer arithmetic, then one division -- independent of any summation order
        weighted = (counts[:, :, :k_cap] * np.arange(1, k_cap + 1, dtype=np.int64)).sum(axis=2)
        denom = np.maximum(n_targets, 1)[:, None].astype(np.float64)
        haar = weighted.astype(np.float64) / denom
        haar[counts[:, :, k_cap + 1] > 0] = np.inf
        haar[:, is_local(coords)] = np.inf
        volumes = np.cumsum(counts[:, :, :k_cap], axis=2).astype(np.float64) / denom[:, :, None]
        named = {k: np.asarray(v, dtype=np.int64) for k, v in (named_scores or {}).items()}
        return cls(gates, coords, counts, n_targets, k_cap, haar[0] if one_group else haar, volumes, named, first_k)


def _named_matrices(named) -> Tuple[List[str], np.ndarray]:
    names = [str(k) for k, _ in named]
    mats = [gate_matrix(m) for _, m in named]
    return names, (np.stack(mats) if mats else np.zeros((0, 4, 4), dtype=np.complex128))


def score_candidates(gates: Sequence, sampler, *, named=(("cnot", CX), ("swap", SWAP)), k_cap: int = 64, groups=None,
                     n_groups: Optional[int] = None, tol: float = pulse_cost.TOL, device=None, want_first: bool = False) -> CandidateScores:
    """``collect_data`` for every candidate at once: the sampler's targets become the resident batch (generated in place for a device
    sampler such as ``DeviceHaarBatch``, uploaded once for a list of 4x4 unitaries) and ONE ``slam_candidate_scores`` call counts, per
    candidate, how many targets are first reached with k = 1 .. ``k_cap`` applications.  ``groups`` (int [N], with ``n_groups``
    defaulting to ``max + 1``) splits the counts by target group.  The ``named`` targets go through the same device call as a small
    explicit batch.  ``want_first`` also returns the [G, N] table of first sizes."""
    gates = list(gates) if not isinstance(gates, np.ndarray) else gates
    coords = gate_coords(gates)
    if len(coords) < 1:
        raise ValueError("no candidate gates")
    k_cap = int(k_cap)
    ctx = runtime.get_context(0 if device is None else device)
    n = pulse_cost._load_targets(ctx, sampler)
    g = None
    E = 1
    if groups is not None:
        g = np.ascontiguousarray(groups, dtype=np.int32).reshape(-1)
        if g.size != n:
            raise ValueError(f"groups has {g.size} entries for {n} targets")
        E = int(n_groups) if n_groups is not None else (int(g.max()) + 1 if n else 1)
    first_k = None
    if n:
        counts, first_k = ctx.candidate_scores(coords, k_cap, groups=g, n_groups=E, first=0, count=n, want_first=want_first, tol=tol)
    else:
        counts = np.zeros((E, len(coords), k_cap + 2), dtype=np.int64)
        first_k = np.zeros((len(coords), 0), dtype=np.int32) if want_first else None
    names, mats = _named_matrices(named)
    named_scores = {}
    if names:
        ctx.set_targets(mats)
        _, fk = ctx.candidate_scores(coords, k_cap, first=0, count=len(names), want_first=True, tol=tol)
        named_scores = {name: fk[:, j].astype(np.int64) for j, name in enumerate(names)}
    return CandidateScores.from_counts(list(gates), counts if groups is not None else counts[0], named_scores, first_k, coords)


# ---- durations ---------------------------------------------------------------------------------------------------------------------
def linear_speed_limit(x):
    """gg = pi/2 - gc: the curve under which ``ConversionGainGate.cost()`` is the duration."""
    return _HALF_PI - x


def mid_speed_limit(x):
    """duraton_scaling.py:32-38: the circle centred at (-pi/4, -pi/4) through (pi/2, 0) and (0, pi/2)."""
    c = np.pi / 4
    return 0.5 * (-2 * c + np.sqrt(4 * c**2 - 8 * c * x + 4 * c * np.pi - 4 * x**2 + np.pi**2))


def squared_speed_limit(x):
    """duraton_scaling.py:40-41: the quarter circle of radius pi/2."""
    return np.sqrt(_HALF_PI**2 - x**2)


_CURVES = {"linear": linear_speed_limit, "mid": mid_speed_limit, "squared": squared_speed_limit}


def _method(speed_method: str) -> str:
    """The reference tests ``"<word>" in speed_method`` in this order (duraton_scaling.py:44-56)."""
    for word in ("hardware", "mid", "squared", "linear", "bare"):
        if word in str(speed_method):
            return word
    raise ValueError("invalid speed_method")


def _curve(speed_method, speed_limit_function: Optional[Callable] = None):
    """``(kind, callable)``: "linear" (also for "bare"), "mid", "squared", or "callable" with the caller's curve -- ``speed_method``
    itself, or ``speed_limit_function`` under "hardware"."""
    if callable(speed_method):
        return "callable", speed_method
    m = _method(speed_method)
    if m == "hardware":
        if speed_limit_function is None:
            raise ValueError('speed_method "hardware" needs speed_limit_function: the measured speed-limit spline is not shipped')
        return "callable", speed_limit_function
    return ("linear" if m == "bare" else m), None


def speed_limit_intersection(gc: float, gg: float, speed_method="linear", speed_limit_function: Optional[Callable] = None) -> Tuple[float, float]:
    """Where the ray through (|gc|, |gg|) meets the speed-limit curve gg' = s(gc'): ``(gc', gg')``.  Closed forms for "linear", "mid"
    and "squared"; a callable on [0, pi/2] (``speed_method`` itself, or ``speed_limit_function`` under "hardware") is solved by a
    bracketed root."""
    gc, gg = abs(float(gc)), abs(float(gg))
    if gc == 0.0 and gg == 0.0:
        raise ValueError("a gate without drive has no duration")  # snail_death_gate.py:128
    kind, fn = _curve(speed_method, speed_limit_function)
    if kind != "callable":
        if kind == "linear":
            mu = _HALF_PI / (gc + gg)
        elif kind == "squared":
            mu = _HALF_PI / math.hypot(gc, gg)
        else:  # (mu gc + c)^2 + (mu gg + c)^2 = 5 pi^2 / 8, c = pi/4:  A mu^2 + 2 B mu - pi^2 / 2 = 0, the positive root
            A, B = gc * gc + gg * gg, (np.pi / 4) * (gc + gg)
            mu = (np.pi**2 / 2) / (B + math.sqrt(B * B + A * np.pi**2 / 2))
        return mu * gc, mu * gg
    if gc == 0.0:
        return 0.0, float(fn(0.0))
    # f(mu) = mu gg - s(mu gc) on (0, pi / (2 gc)]: negative near 0 (s(0) > 0), and the curve ends on the gc axis
    from scipy.optimize import brentq

    hi = _HALF_PI / gc

    def f(mu):
        return mu * gg - float(fn(min(mu * gc, _HALF_PI)))

    if f(hi) < 0.0:
        raise ValueError("the speed-limit curve does not meet the gate's ray on [0, pi/2]")
    mu = hi if f(hi) == 0.0 else brentq(f, 0.0, hi, xtol=1e-300, rtol=8.9e-16, maxiter=500)
    return mu * gc, mu * gg


def gate_duration(gate, speed_method="linear", speed_limit_function: Optional[Callable] = None) -> float:
    """Duration of a ``ConversionGainGate`` driven as hard as the speed limit allows (``SpeedLimitedGate.cost``): the pulse time divided
    by gc'/gc (gg'/gg when gc = 0), (gc', gg') = ``speed_limit_intersection``.  "linear" and "bare" give ``gate.cost()``."""
    p = gate.params
    gc, gg, t = abs(float(p[2])), abs(float(p[3])), float(p[-1])
    if _curve(speed_method, speed_limit_function)[0] == "linear":
        return float(ConversionGainGate.cost(gate))
    sc, sg = speed_limit_intersection(gc, gg, speed_method, speed_limit_function)
    scale = sg / gg if gc == 0.0 else sc / gc
    return t / scale


class SpeedLimitedGate(ConversionGainGate):
    """A ``ConversionGainGate`` whose ``cost()`` / ``duration`` is ``gate_duration`` under a speed-limit curve (snail_death_gate.py:108-158)."""

    def __init__(self, p1, p2, g1, g2, t_el=1, speed_method="linear", speed_limit_function: Optional[Callable] = None):
        self.speed_method = speed_method
        self.slf = speed_limit_function
        super().__init__(p1, p2, g1, g2, t_el)

    def cost(self):
        return gate_duration(self, self.speed_method, self.slf)


def scaled_gate(gate, speed_method="linear", speed_limit_function: Optional[Callable] = None):
    """The gate object ``atomic_cost_scaling`` returns: a ``SpeedLimitedGate`` under a curve, a plain copy for "linear" / "bare"."""
    if _curve(speed_method, speed_limit_function)[0] == "linear":
        return ConversionGainGate(*gate.params)
    return SpeedLimitedGate(*gate.params, speed_method=speed_method, speed_limit_function=speed_limit_function)


def _is_bare(speed_method) -> bool:
    return not callable(speed_method) and "bare" in str(speed_method)


def scale_counts(k, duration: float, duration_1q: float = 0, bare: bool = False):
    """duraton_scaling.py:62-65, 103: ``k duration + (k + 1) duration_1q``; "bare" leaves the first factor out."""
    k = np.asarray(k, dtype=np.float64)
    return (k if bare else k * duration) + (k + 1) * duration_1q


def atomic_cost_scaling(gate, scores, speed_method="linear", duration_1q=0, scaled_gate_in=None, family_extension: bool = False,
                        metric=None, speed_limit_function: Optional[Callable] = None):
    """duraton_scaling.py:16-104: ``(scaled gate, scores * duration + (scores + 1) * duration_1q)`` for a scalar or an array of gate
    counts ([haar, cnot, swap] in the reference).  With ``family_extension`` the CNOT / SWAP entries are what the cheapest older
    sibling costs (``family_extend.GateFamily.lookup(policy="reference")``, the walk of ``recursive_sibling_check``): ``metric`` 1 or 2
    returns that cost alone, ``metric`` None replaces entries 1 and 2 of a three-vector, the Haar metric 0 raises."""
    sg = scaled_gate(gate, speed_method, speed_limit_function) if scaled_gate_in is None else scaled_gate_in
    duration = float(sg.cost())
    s = np.asarray(scores, dtype=np.float64)
    out = scale_counts(s, duration, duration_1q, _is_bare(speed_method))
    if family_extension:
        from .family_extend import GateFamily

        if metric == 0:
            raise NotImplementedError("Famextend scaling not implemented for haar, calculate it by hand lol")
        fam = GateFamily(ConversionGainGate(*gate.params), cost_1q=duration_1q, basis_factor=duration)
        cost = fam.lookup_unitaries(np.stack([CX, SWAP]), "reference").cost
        if metric == 1:
            return sg, float(cost[0])
        if metric == 2:
            return sg, float(cost[1])
        if isinstance(metric, tuple):
            lam = float(metric[1])
            return sg, lam * float(cost[0]) + (1 - lam) * float(cost[1])
        out = np.array(out, dtype=np.float64)
        if out.shape != (3,):
            raise ValueError("family_extension without a metric scales a [haar, cnot, swap] vector")
        out[1], out[2] = float(cost[0]), float(cost[1])
        return sg, out
    return sg, (float(out) if out.ndim == 0 else out)


# ---- the winner --------------------------------------------------------------------------------------------------------------------
Metric = Union[int, Tuple[int, float]]


def metric_scores(scores: CandidateScores, metric: Metric) -> np.ndarray:
    """float [G]: the unscaled gate count a metric looks at -- 0 Haar, 1 CNOT, 2 SWAP, (-1, lam) = lam CNOT + (1 - lam) SWAP; ``inf``
    where the candidate does not reach the target(s)."""
    def named(name):
        v = scores.named_scores[name].astype(np.float64)
        v[scores.named_scores[name] > scores.k_cap] = np.inf
        return v

    if isinstance(metric, tuple):
        if metric[0] != -1:
            raise ValueError("a custom metric is (-1, lambda)")
        lam = float(metric[1])
        return lam * named("cnot") + (1 - lam) * named("swap")
    if metric == 0:
        h = np.asarray(scores.haar_score, dtype=np.float64)
        if h.ndim != 1:
            raise ValueError("the Haar metric needs scores of one target group")
        return h
    if metric in (1, 2):
        return named("cnot" if metric == 1 else "swap")
    raise ValueError("metric must be 0 (Haar), 1 (CNOT), 2 (SWAP) or (-1, lambda)")


def _argmin_lowest_index(values: np.ndarray) -> int:
    """First index of the minimum; ``inf`` and NaN never win."""
    v = np.where(np.isfinite(values), values, np.inf)
    j = int(np.argmin(v))  # argmin returns the first occurrence: ties go to the lowest candidate index
    if not np.isfinite(v[j]):
        raise ValueError("no candidate has a finite score")
    return j


def _log_winner(gate, raw_scores, scaled_score, scaled):
    logging.info(f"winner: {gate}, scores: {raw_scores}, cost: {gate.cost()}")
    logging.info(f"scaled scores: {scaled_score}, scaled cost: {scaled.cost()}")


def pick_winner(scores: CandidateScores, metric: Metric = 0, speed_method="linear", duration_1q=0, family_extension: bool = False,
                speed_limit_function: Optional[Callable] = None):
    """winner_selection.py:17-144 for the metrics that need no circuit: the candidate with the lowest scaled score
    (``atomic_cost_scaling`` of the metric's gate count).  Ties go to the lowest candidate index; a candidate with an infinite score
    (local, or a target out of reach) never wins.  Returns ``(gate, scaled_gate, scaled_score)``."""
    raw = metric_scores(scores, metric)
    scaled = np.full(len(raw), np.inf)
    for j, gate in enumerate(scores.gates):
        if not np.isfinite(raw[j]):
            continue
        _, scaled[j] = atomic_cost_scaling(gate, raw[j], speed_method, duration_1q, family_extension=family_extension, metric=metric,
                                           speed_limit_function=speed_limit_function)
    j = _argmin_lowest_index(scaled)
    gate = scores.gates[j]
    sg = scaled_gate(gate, speed_method, speed_limit_function)
    h = np.asarray(scores.haar_score)
    raw_scores = [float(h[j]) if h.ndim == 1 else None] + [int(v[j]) for v in scores.named_scores.values()]
    _log_winner(gate, raw_scores, float(scaled[j]), sg)
    return gate, sg, float(scaled[j])


class GroupWinner(NamedTuple):
    """One group's answer from ``select_basis``: the candidate's ``index``, the ``gate``, its ``scaled_gate``, the group's ``total``
    scaled cost under it and ``n`` = the number of targets in the group (0: no winner, ``index`` -1)."""

    index: int
    gate: object
    scaled_gate: object
    total: float
    n: int


class BasisSelection(NamedTuple):
    """``select_basis``: ``winners`` per group (one group unless the strategy is per edge), ``edges`` int [E, 2] (the groups' sorted
    qubit pairs, else None), ``group_of`` int32 [N] and ``sizes`` int32 [N]: the number of gates of every target under its group's
    winner (0 for a local target)."""

    winners: List[GroupWinner]
    edges: Optional[np.ndarray]
    group_of: np.ndarray
    sizes: np.ndarray


def group_edges(edges) -> Tuple[np.ndarray, np.ndarray]:
    """Unordered qubit pairs as groups: ``(pairs int [E, 2] sorted, group_of int32 [N])``; (a, b) and (b, a) are one group."""
    e = np.asarray(edges, dtype=np.int64).reshape(-1, 2)
    pairs, group_of = np.unique(np.sort(e, axis=1), axis=0, return_inverse=True)
    return pairs, np.asarray(group_of, dtype=np.int32).reshape(-1)


def weighted_winners(first_k: np.ndarray, group_of: np.ndarray, n_groups: int, durations: np.ndarray, duration_1q: float = 0,
                     k_cap: int = 64, bare: bool = False) -> Tuple[np.ndarray, np.ndarray]:
    """Per group the candidate that minimises ``sum_t scaled(first_k[g, t])`` over the group's targets (``pick_winner`` with
    ``target_ops``): ``(index int [E], total float [E])``.  scaled(k) = k duration_g + (k + 1) duration_1q, 0 for a local target
    (k = 0), ``inf`` for an unreached one; targets are added in index order; ties go to the lowest candidate index; an empty group has
    index -1 and total 0."""
    fk = np.asarray(first_k)
    G, N = fk.shape
    k = fk.astype(np.float64)
    d = np.asarray(durations, dtype=np.float64).reshape(G, 1)
    cost = (k if bare else k * d) + (k + 1) * float(duration_1q)
    cost = np.where(fk == 0, 0.0, np.where(fk > k_cap, np.inf, cost))
    idx = np.full(n_groups, -1, dtype=np.int64)
    total = np.zeros(n_groups)
    for e in range(n_groups):
        members = np.nonzero(np.asarray(group_of) == e)[0]
        if len(members) == 0:
            continue
        sums = np.zeros(G)
        for t in members.tolist():  # in target order: the same doubles whatever the grouping
            sums = sums + cost[:, t]
        if not np.any(np.isfinite(sums)):
            raise ValueError(f"{pulse_cost._UNREACHABLE} (no candidate reaches every target of group {e} within k_cap = {k_cap} gates: "
                             "raise k_cap to reach it)")
        idx[e] = _argmin_lowest_index(sums)
        total[e] = sums[idx[e]]
    return idx, total


def select_basis(targets, strategy: str, *, edges=None, gates=None, basic_metric: Metric = 0, lambda_weight: float = 0.47,
                 speed_method="linear", duration_1q=0, k_cap: int = 64, device=None, haar_sampler=None,
                 speed_limit_function: Optional[Callable] = None) -> BasisSelection:
    """The four strategies of ``SpeedGateSubstitute`` (speed_limit_pass.py:139-309) on plain arrays: ``targets`` [N, 4, 4] are a
    circuit's consolidated 2Q blocks, ``edges`` int [N, 2] the qubit pair of each (``weighted_pairwise`` only), ``gates`` the
    candidates (default ``build_gates()``).

    ``basic_overall``     the winner of ``basic_metric`` (0 Haar over ``haar_sampler``, default 65 536 device Haar targets; 1 CNOT; 2 SWAP);
    ``lambda_weight``     the winner of (-1, ``lambda_weight``);
    ``weighted_overall``  the candidate with the lowest total scaled cost over the circuit's own targets;
    ``weighted_pairwise`` the same per unordered qubit pair -- all pairs from ONE grouped device call.
    A group with a target that its best candidate does not reach within ``k_cap`` raises the ``ValueError`` of ``pulse_cost``."""
    if strategy not in STRATEGIES:
        raise ValueError("Strategy not recognized")  # speed_limit_pass.py:309
    t = np.asarray(targets, dtype=np.complex128).reshape(-1, 4, 4)
    n = len(t)
    gates = build_gates()[0] if gates is None else list(gates)
    coords = gate_coords(gates)
    pairs = None
    group_of = np.zeros(n, dtype=np.int32)
    if strategy == "weighted_pairwise":
        if edges is None:
            raise ValueError("weighted_pairwise needs the qubit pair of every target (edges)")
        pairs, group_of = group_edges(edges)
        if len(group_of) != n:
            raise ValueError(f"{len(group_of)} edges for {n} targets")
    n_groups = max(len(pairs), 1) if pairs is not None else 1
    bare = _is_bare(speed_method)

    def winner(j, total, count):
        return GroupWinner(int(j), gates[j], scaled_gate(gates[j], speed_method, speed_limit_function), float(total), int(count))

    if strategy in ("basic_overall", "lambda_weight"):
        metric = basic_metric if strategy == "basic_overall" else (-1, float(lambda_weight))
        if metric == 0 and haar_sampler is None:
            from .sampler import DeviceHaarBatch

            haar_sampler = DeviceHaarBatch(seed=0, n_samples=1 << 16, device=0 if device is None else device)
        sc = score_candidates(gates, haar_sampler if metric == 0 else [], k_cap=k_cap, device=device)
        gate, _, _ = pick_winner(sc, metric, speed_method, duration_1q, speed_limit_function=speed_limit_function)
        j = next(i for i, g in enumerate(gates) if g is gate)
        own = score_candidates(coords[j : j + 1], list(t), named=(), k_cap=k_cap, device=device, want_first=True)
        duration = float(scaled_gate(gates[j], speed_method, speed_limit_function).cost())
        _, total = weighted_winners(own.first_k, group_of, 1, np.array([duration]), duration_1q, k_cap, bare)
        return BasisSelection([winner(j, total[0], n)], None, group_of, own.first_k[0].astype(np.int32))
    sc = score_candidates(coords, list(t), named=(), k_cap=k_cap, groups=group_of, n_groups=n_groups, device=device, want_first=True)
    # a candidate that misses a target of a group cannot win it: the durations of the others are all that is needed
    reaches_some = (sc.counts[:, :, k_cap + 1] == 0).any(axis=0) & ~is_local(coords)
    durations = np.array([float(scaled_gate(g, speed_method, speed_limit_function).cost()) if ok else np.inf
                          for g, ok in zip(gates, reaches_some)])
    durations = np.where(np.isfinite(durations), durations, 0.0)
    idx, total = weighted_winners(sc.first_k, group_of, n_groups, durations, duration_1q, k_cap, bare)
    sizes = np.zeros(n, dtype=np.int32)
    winners = []
    for e in range(n_groups):
        members = group_of == e
        if idx[e] < 0:
            winners.append(GroupWinner(-1, None, None, 0.0, 0))
            continue
        sizes[members] = sc.first_k[idx[e], members]
        winners.append(winner(idx[e], total[e], int(members.sum())))
        logging.info(f"winner score: {total[e]}, normalized score: {total[e] / max(int(members.sum()), 1)}")
    return BasisSelection(winners, pairs, group_of, sizes)
