"""Family-extended decomposition: the cheapest sibling gate per target (reference: ``recursive_sibling_check``,
src/slam/utils/gates/family_extend.py:17-117; figures of src/slam/scripts/haar_improvements.ipynb).

A target that needs k applications of a short conversion-gain pulse is often cheaper with the same pulse run 2 or 3 times as long
(an "older sibling"): fewer single-qubit layers in between.  The reference asks monodromy for k, builds the sibling (x2 when k is
even, x3 when odd), recurses, and keeps the sibling's circuit where it is strictly cheaper.  Here the family is explicit:

* ``GateFamily``: the members r = 2^a 3^b of a base ``ConversionGainGate`` up to a full iSWAP's strength, one coverage table per
  member (rows k = 1, 2, ... applications: ``coverage.region``), the links ``child_even`` / ``child_odd`` (member 2r / 3r) and the
  durations r * basis_factor;
* ``GateFamily.lookup``: the walk for Weyl coordinates [N, 3] in NumPy -- the host restatement the device is held to;
* ``slam_family_lookup`` (``_ffi.Context.family_lookup``): the same walk for every resident target in one launch, counted per
  (member, k); ``family_cost_from_distribution`` / ``family_sweep`` sum ``count * cost`` in row order (bit-for-bit reproducible);
* ``FamilyExtendedTemplate``: a basis for ``TemplateOptimizer`` that fits every target with its looked-up member at its looked-up k.

Decisions where the reference's behaviour is an accident:
  * a local target, identity included, takes 0 gates and costs 0 (the reference handles the exact identity only; other local
    targets trip its assert) -- as ``pulse_cost``;
  * at k = 1 the cost is (k + 1) cost_1q + k duration like everywhere else (the reference returns the literal 1.2, which is that for
    a unit-duration gate with cost_1q = 0.1 and wrong for every other member);
  * ``rec_iter_factor`` and ``use_smush`` are accepted and ignored (``use_smush=True`` raises the "Smush Polytope not in memory"
    error of ``MixedOrderBasisCircuitTemplate``); the disabled ``if False and ...`` phase-matching branch is not built;
  * a target beyond ``max_gates`` applications of the base gate raises ``ValueError("Monodromy did not find a polytope containing
    U ...")`` for the whole call, as ``pulse_cost`` does.

``policy="best"`` takes the cheapest of ALL members that contain the target (ties: the smaller r) instead of the one path the
reference walks: never dearer, and cheaper in real cases (CX under iSWAP^(1/6), cost_1q 0.1: the walk goes r = 1 (k 6) -> 2 (k 3) ->
6 (k 2) and returns 1.4; r = 3 (k 2) costs 1.3).
"""
from __future__ import annotations

import logging
from typing import List, NamedTuple, Optional, Sequence, Tuple

import numpy as np

from . import _ffi, coverage, pulse_cost, runtime, span_rules
from .basis import CircuitCoverage, CircuitTemplate, CoverageTable, MixedOrderBasisCircuitTemplate
from .gates import ConversionGainGate, gate_matrix

POLICIES = ("reference", "best")
_SMUSH_MSG = "Smush Polytope not in memory, need to compute using parallel_drive_volume.py"  # basis.py:291-294
_STOP = np.pi / 2 * (1 + 1e-12)  # family_extend.py:96: a sibling stronger than a full iSWAP is outside the family


class FamilyLookup(NamedTuple):
    """Per target: index of the winning member (-1: local or unreachable), its number of gates (0 local, -1 unreachable) and the cost
    (0.0 local, +inf unreachable)."""

    member: np.ndarray
    gates: np.ndarray
    cost: np.ndarray


def multipliers(strength: float, limit: float = _STOP) -> List[int]:
    """The r = 2^a 3^b >= 1, increasing, with ``strength * r <= limit``."""
    out = []
    a = 1
    while strength * a <= limit:
        r = a
        while strength * r <= limit:
            out.append(r)
            r *= 3
        a *= 2
    return sorted(out)


def walk(ks, child_even, child_odd, durations, cost_1q, policy="reference") -> FamilyLookup:
    """The choice between siblings, given per member the smallest number of applications that reaches each target: ``ks`` int
    [n_members, N], 0 where the member's table does not contain the target.  "reference": from member 0, own cost (k + 1) cost_1q +
    k duration; stop at k = 1; else on to ``child_even`` / ``child_odd`` by the parity of k, stop if that is -1 or does not contain
    the target; unwinding from the deepest level, a level keeps its child's result only where that is STRICTLY cheaper
    (family_extend.py:112-117).  "best": the cheapest member that contains the target, ties to the smaller index.  A target member 0
    does not contain is unreachable under both."""
    if policy not in POLICIES:
        raise ValueError(f"policy must be one of {POLICIES} (got {policy!r})")
    ks = np.asarray(ks, dtype=np.int64)
    n_members, n = ks.shape
    ce = np.asarray(child_even, dtype=np.int64)
    co = np.asarray(child_odd, dtype=np.int64)
    d = np.asarray(durations, dtype=np.float64)
    own = np.where(ks > 0, (ks + 1) * float(cost_1q) + ks * d[:, None], np.inf)
    cols = np.arange(n)
    if policy == "best":
        m = np.argmin(own, axis=0)  # the first minimum: the smaller member
    else:
        levels = []  # (member per target, still walking)
        cur = np.zeros(n, dtype=np.int64)
        alive = ks[0] > 0
        while np.any(alive):
            if len(levels) > n_members:
                raise ValueError("the family's links do not lead away from the base member")
            levels.append((cur, alive))
            k = ks[cur, cols]
            nxt = np.where(k % 2 == 0, ce[cur], co[cur])
            go = alive & (k > 1) & (nxt >= 0)
            go &= ks[np.where(go, nxt, 0), cols] > 0  # the child must contain the target
            cur, alive = np.where(go, nxt, cur), go
        m = np.zeros(n, dtype=np.int64)
        cost = np.full(n, np.inf)
        for lvl_m, lvl_alive in reversed(levels):
            mine = own[lvl_m, cols]
            keep_child = cost < mine  # strictly cheaper, or the level's own circuit stays
            take = lvl_alive & ~keep_child
            m = np.where(take, lvl_m, m)
            cost = np.where(take, mine, cost)
    reach = ks[0] > 0
    cost = np.where(reach, own[m, cols], np.inf)
    return FamilyLookup(np.where(reach, m, -1).astype(np.int32), np.where(reach, ks[m, cols], -1).astype(np.int32), cost)


class GateFamily:
    """A base ``ConversionGainGate`` and its older siblings (see the module docstring).

    ``multipliers`` [n]: r per member, increasing; ``gates``: member r = ``ConversionGainGate(pc, pg, gc, gg, t_el * r)`` normalised to
    unit duration; ``durations`` = r * ``basis_factor`` (default ``base_gate.cost()``: the reference's linear speed scaling);
    ``child_even`` / ``child_odd``: index of member 2r / 3r, -1 outside the family; ``tables``: per member a ``CoverageTable`` of the
    rows k = 1 .. ceil(max_gates / r) -- cut after the first row that reaches every target (``span_rules._reaches_everything``, exact
    for the CX / iSWAP / sqrt(iSWAP) / B classes; for other gates fullness is not decided and no row is cut)."""

    def __init__(self, base_gate: ConversionGainGate, cost_1q=0.1, basis_factor=None, max_gates=48):
        from .weyl import c1c2c3

        if not isinstance(base_gate, ConversionGainGate):
            raise ValueError("all base gates must be ConversionGainGate")  # basis.py:242-243
        if int(max_gates) < 1:
            raise ValueError("max_gates must be positive")
        pc, pg, gc, gg, t = (float(v) for v in base_gate.params)
        self.base_gate = base_gate
        self.cost_1q = float(cost_1q)
        self.basis_factor = float(base_gate.cost() if basis_factor is None else basis_factor)
        self.max_gates = int(max_gates)
        rs = multipliers((abs(gc) + abs(gg)) * t)
        if not rs:
            raise ValueError("the base gate is stronger than a full iSWAP: it has no family")
        if len(rs) > _ffi.FAMILY_MAX_MEMBERS:
            raise ValueError(f"the family has {len(rs)} members; at most {_ffi.FAMILY_MAX_MEMBERS} are implemented (use a stronger base gate)")
        self.multipliers = np.array(rs, dtype=np.int64)
        self.gates = []
        for r in rs:
            g = ConversionGainGate(pc, pg, gc, gg, t * r)
            g.normalize_duration(1)
            self.gates.append(g)
        self.gate_matrices = np.stack([gate_matrix(g) for g in self.gates])
        self.gate_coords = [c1c2c3(m) for m in self.gate_matrices]
        self.durations = self.multipliers * self.basis_factor
        index = {r: m for m, r in enumerate(rs)}
        self.child_even = np.array([index.get(2 * r, -1) for r in rs], dtype=np.int32)
        self.child_odd = np.array([index.get(3 * r, -1) for r in rs], dtype=np.int32)
        self._tables: List[Optional[CoverageTable]] = [None] * len(rs)

    def __len__(self):
        return len(self.gates)

    def member_index(self, r: int) -> int:
        hit = np.nonzero(self.multipliers == int(r))[0]
        if len(hit) == 0:
            raise ValueError(f"the family has no member x{r} (members: {self.multipliers.tolist()})")
        return int(hit[0])

    def own_cost(self, m: int, k: int) -> float:
        return (k + 1) * self.cost_1q + k * float(self.durations[m])

    def table(self, m: int) -> CoverageTable:
        """Member m's rows (built on first use and kept: a 48-gate region is a 60 ms dynamic programme)."""
        if self._tables[m] is None:
            r = int(self.multipliers[m])
            key = str(self.gates[m])
            entries = []
            for k in range(1, -(-self.max_gates // r) + 1):
                seq = [self.gate_coords[m]] * k
                entries.append(CircuitCoverage([key] * k, self.own_cost(m, k), [m] * k, seq))
                if span_rules._reaches_everything(np.array(seq)):
                    break  # every later row contains what this one does: the first hit is never behind it
            self._tables[m] = CoverageTable(entries)
        return self._tables[m]

    @property
    def tables(self) -> List[CoverageTable]:
        return [self.table(m) for m in range(len(self))]

    def row_costs(self) -> np.ndarray:
        """Cost of every (member, k) row, concatenated in member order: what the device compares and the totals are summed from."""
        return np.concatenate([np.arange(1, len(t) + 1) * self.durations[m] + (np.arange(1, len(t) + 1) + 1) * self.cost_1q
                               for m, t in enumerate(self.tables)])

    def rows(self) -> List[Tuple[int, int]]:
        """(multiplier r, k) of every row, in the order of ``row_costs`` and of the device's counts."""
        return [(int(self.multipliers[m]), k) for m, t in enumerate(self.tables) for k in range(1, len(t) + 1)]

    def unreachable_error(self) -> ValueError:
        return ValueError(f"{pulse_cost._UNREACHABLE} (the base gate's coverage set ends at max_gates = {self.max_gates} gates: raise "
                          "max_gates to reach it)")

    # ---- host lookup ----------------------------------------------------------------------------------------------------------------
    def first_k(self, m: int, coords, tol: float = pulse_cost.TOL, sums=None) -> np.ndarray:
        """Smallest number of applications of member m that reaches each target (0: none of the member's rows does)."""
        c = np.asarray(coords, dtype=np.float64).reshape(-1, 3)
        if sums is None:
            sums = coverage.target_sums(c)
        table = self.table(m)
        k_of = np.zeros(len(c), dtype=np.int64)
        for k in range(1, len(table) + 1):
            if np.all(k_of > 0):
                break
            if k > 1 and np.all(np.isneginf(table.bounds[k - 1])):
                inside = np.ones(len(c), dtype=bool)
            else:
                inside = coverage.contains(None, [self.gate_coords[m]] * k, tol, sums=sums)
            k_of = np.where((k_of == 0) & inside, k, k_of)
        return k_of

    def lookup(self, coords, policy="reference", tol: float = pulse_cost.TOL) -> FamilyLookup:
        """Member index, number of gates and cost per target for Weyl coordinates [N, 3] (units of pi): the walk of
        ``recursive_sibling_check`` ("reference") or the cheapest member ("best"), with the region test and the tolerance of the
        device's lookup (``coverage.contains``; ``pulse_cost.TOL``)."""
        if policy not in POLICIES:
            raise ValueError(f"policy must be one of {POLICIES} (got {policy!r})")
        c = np.asarray(coords, dtype=np.float64).reshape(-1, 3)
        sums = coverage.target_sums(c)
        local = np.zeros(len(c), dtype=bool)
        for cols, _ in sums:
            local |= (np.abs(cols[0]) <= 1e-8) & (np.abs(cols[3]) <= 1e-8)  # decreasing, sum 0: all four vanish
        ks = np.zeros((len(self), len(c)), dtype=np.int64)
        needed = np.zeros(len(self), dtype=bool)
        needed[0] = True
        for m in range(len(self)):  # children come after their parents: one ascending pass finds every member a walk can reach
            if policy == "reference" and not needed[m]:
                continue
            ks[m] = self.first_k(m, c, tol, sums)
            for child, parity in ((self.child_even[m], 0), (self.child_odd[m], 1)):
                if child >= 0 and np.any((ks[m] > 1) & (ks[m] % 2 == parity) & ~local):
                    needed[child] = True
        res = walk(ks, self.child_even, self.child_odd, self.durations, self.cost_1q, policy)
        return FamilyLookup(np.where(local, -1, res.member).astype(np.int32), np.where(local, 0, res.gates).astype(np.int32),
                            np.where(local, 0.0, res.cost))

    def lookup_unitaries(self, targets, policy="reference") -> FamilyLookup:
        from .weyl import c1c2c3

        t = np.asarray(targets, dtype=np.complex128).reshape(-1, 4, 4)
        return self.lookup(np.array([c1c2c3(u) for u in t]).reshape(-1, 3), policy)

    # ---- device lookup --------------------------------------------------------------------------------------------------------------
    def device_lookup(self, ctx, policy="reference", first: int = 0, count: Optional[int] = None, want_targets: bool = False):
        """``ctx.family_lookup`` of this family over the resident targets: ``(counts, base_counts, members, gates)``."""
        return ctx.family_lookup(self.tables, self.child_even, self.child_odd, self.durations, self.cost_1q, policy, first, count,
                                 want_targets, pulse_cost.TOL)


# ---- the reference's entry point ----------------------------------------------------------------------------------------------------
def recursive_sibling_check(basis: CircuitTemplate, target_u, basis_factor=1, rec_iter_factor=1, cost_1q=0.1, use_smush=False,
                            max_gates=48):
    """family_extend.py:17-117: ``(template, cost)`` -- a ``MixedOrderBasisCircuitTemplate`` of the winning member, bound and built
    at the winning number of gates, and (k + 1) cost_1q + k duration.  ``basis`` is a single-gate
    ``MixedOrderBasisCircuitTemplate``, ``basis_factor`` the duration of its gate.  A local target: ``(None, 0)``.
    ``rec_iter_factor`` is accepted and ignored (the reference overwrites it before use)."""
    from .weyl import c1c2c3

    if use_smush:
        raise ValueError(_SMUSH_MSG)
    if not getattr(basis, "mixed_order", False) or len(basis.base_gates) != 1:
        raise ValueError("recursive_sibling_check needs a MixedOrderBasisCircuitTemplate of one base gate")
    family = GateFamily(basis.base_gates[0], cost_1q=cost_1q, basis_factor=basis_factor, max_gates=max_gates)
    t = np.asarray(target_u, dtype=np.complex128)
    if t.shape != (4, 4):
        raise ValueError("targets must be 4x4 unitaries")
    res = family.lookup(np.array([c1c2c3(t)]), "reference")
    m, k = int(res.member[0]), int(res.gates[0])
    if k == 0:
        return None, 0
    if k < 0:
        raise family.unreachable_error()
    if m == 0 and int(basis.maximum_span_guess) >= k:
        template = basis  # the reference hands back the template it was given
    else:
        template = MixedOrderBasisCircuitTemplate(base_gates=[family.gates[m]], chatty_build=False, maximum_span_guess=k,
                                                  device=basis.device)
    entry = next(e for e in template.coverage if len(e) == k)
    template.set_polytope(entry)
    template._sequence = None
    template.build(k)
    return template, float(res.cost[0])


# ---- costs over a distribution ------------------------------------------------------------------------------------------------------
class FamilyCost(NamedTuple):
    """``family_cost_from_distribution``: ``total`` / ``average`` with the family, ``base_total`` / ``base_average`` with the base
    gate alone, ``counts`` = [(multiplier r, k, targets)] in row order, ``base_counts`` = [(k, targets)], ``local_count``, ``n``."""

    total: float
    average: float
    base_total: float
    base_average: float
    counts: List[Tuple[int, int, int]]
    base_counts: List[Tuple[int, int]]
    local_count: int
    n: int


def _ordered_sum(counts, costs) -> float:
    total = 0.0
    for k, c in zip(np.asarray(counts).tolist(), np.asarray(costs).tolist()):
        total += k * c
    return total


def _family_cost(family: GateFamily, ctx, n: int, policy: str) -> FamilyCost:
    rows = family.rows()
    e0 = len(family.table(0))
    if n == 0:
        return FamilyCost(0.0, 0.0, 0.0, 0.0, [(r, k, 0) for r, k in rows], [(k, 0) for k in range(1, e0 + 1)], 0, 0)
    counts, base_counts, _, _ = family.device_lookup(ctx, policy, 0, n)
    if int(counts[-1]) > 0 or int(base_counts[-1]) > 0:
        raise family.unreachable_error()
    costs = family.row_costs()
    total = _ordered_sum(counts[: len(rows)], costs)
    base_total = _ordered_sum(base_counts[:e0], costs[:e0])
    return FamilyCost(total, total / n, base_total, base_total / n, [(r, k, int(c)) for (r, k), c in zip(rows, counts[: len(rows)])],
                      [(k + 1, int(c)) for k, c in enumerate(base_counts[:e0])], int(counts[len(rows)]), n)


def family_cost_from_distribution(family: GateFamily, sampler, policy="reference", device=0) -> FamilyCost:
    """``TemplateOptimizer.cost_from_distribution`` (optimizer.py:168-178, its two log lines included) with every target at its
    cheapest sibling: one ``slam_family_lookup`` over the sampler's targets -- generated in place for a device sampler
    (``DeviceHaarBatch``), uploaded once otherwise; nothing but the counts comes back -- and ``count * cost`` summed in row order.
    An empty sampler costs 0.0; an unreachable target raises for the whole call."""
    if policy not in POLICIES:
        raise ValueError(f"policy must be one of {POLICIES} (got {policy!r})")
    ctx = runtime.get_context(device)
    n = pulse_cost._load_targets(ctx, sampler)
    res = _family_cost(family, ctx, n, policy)
    logging.info(f"Total circuit pulse cost: {res.total}")
    if n:
        logging.info(f"Average gate pulse cost: {res.average}")
    return res


class FamilySweep(NamedTuple):
    """``family_sweep``: per base gate (the x axis of haar_improvements.ipynb cell 4/5: ``fractions`` = base cost = share of a full
    iSWAP) the expected Haar cost and the cost of CX and SWAP, with (``fam_*``) and without (``no_fam_*``) the family; ``results``
    holds the ``FamilyCost`` per base gate and ``n`` the number of targets."""

    fractions: List[float]
    fam_haar: List[float]
    no_fam_haar: List[float]
    fam_cx: List[float]
    no_fam_cx: List[float]
    fam_swap: List[float]
    no_fam_swap: List[float]
    results: List[FamilyCost]
    n: int


_CX = np.array([[1, 0, 0, 0], [0, 0, 0, 1], [0, 0, 1, 0], [0, 1, 0, 0]], dtype=np.complex128)
_SWAP = np.array([[1, 0, 0, 0], [0, 0, 1, 0], [0, 1, 0, 0], [0, 0, 0, 1]], dtype=np.complex128)


def family_sweep(base_gates: Sequence[ConversionGainGate], sampler, cost_1q=0.1, max_gates=48, policy="reference", device=0,
                 basis_factors=None) -> FamilySweep:
    """haar_improvements.ipynb cell 4 for a list of base gates: E[Haar] over the sampler's targets -- made resident ONCE, one
    ``slam_family_lookup`` per base gate over the same batch -- and D[CX], D[SWAP] from the host lookup, each with and without the
    family.  (The reference draws ``random_unitary(seed=42)`` 2000 times, i.e. one unitary; here the sampler decides.)"""
    gates = list(base_gates)
    factors = [None] * len(gates) if basis_factors is None else list(basis_factors)
    if len(factors) != len(gates):
        raise ValueError("one basis factor per base gate")
    families = [GateFamily(g, cost_1q=cost_1q, basis_factor=f, max_gates=max_gates) for g, f in zip(gates, factors)]
    ctx = runtime.get_context(device)
    n = pulse_cost._load_targets(ctx, sampler)
    out = FamilySweep([], [], [], [], [], [], [], [], n)
    for fam in families:
        res = _family_cost(fam, ctx, n, policy)
        out.fractions.append(float(fam.base_gate.cost()))
        out.results.append(res)
        out.fam_haar.append(res.average)
        out.no_fam_haar.append(res.base_average)
        named = fam.lookup_unitaries(np.stack([_CX, _SWAP]), policy)
        if np.any(named.gates < 0):
            raise fam.unreachable_error()
        k0 = fam.first_k(0, fam_coords(np.stack([_CX, _SWAP])))
        out.fam_cx.append(float(named.cost[0]))
        out.fam_swap.append(float(named.cost[1]))
        out.no_fam_cx.append(fam.own_cost(0, int(k0[0])))
        out.no_fam_swap.append(fam.own_cost(0, int(k0[1])))
    return out


def fam_coords(targets) -> np.ndarray:
    """Weyl coordinates [N, 3] (8 digits, units of pi) of 4x4 unitaries, on the host."""
    from .weyl import c1c2c3

    return np.array([c1c2c3(u) for u in np.asarray(targets, dtype=np.complex128).reshape(-1, 4, 4)]).reshape(-1, 3)


# ---- fitting ------------------------------------------------------------------------------------------------------------------------
class FamilyExtendedTemplate(CircuitTemplate):
    """A basis for ``TemplateOptimizer(basis=..., objective=BasicCost())`` in which every target is fitted with its cheapest sibling:
    (member, k) per target from ``slam_family_lookup``, the members' matrices as ONE gate table, and one ``slam_decompose_list``
    per distinct (member, k) with the gate sequence ``[m] * k``.  After a run ``optimizer.family_members`` holds r and
    ``optimizer.family_costs`` the cost per target; ``DataDictEntry.cycles`` = k and ``Xk`` = the 6 (k + 1) angles of the MEMBER's
    template, ``member_template(r)``."""

    family_extended = True

    def __init__(self, base_gate: ConversionGainGate, cost_1q=0.1, max_gates=48, policy="reference", device=0, basis_factor=None):
        if policy not in POLICIES:
            raise ValueError(f"policy must be one of {POLICIES} (got {policy!r})")
        self.family = GateFamily(base_gate, cost_1q=cost_1q, basis_factor=basis_factor, max_gates=max_gates)
        self.policy = policy
        super().__init__(n_qubits=2, base_gates=list(self.family.gates), edge_params=[[(0, 1)]], no_exterior_1q=False, use_polytopes=False,
                         maximum_span_guess=max(len(t) for t in self.family.tables), preseed=False, device=device)
        self._member = 0

    def bind_member(self, m: int) -> None:
        """The member whose gate ``build`` / ``gate_sequence`` / ``eval`` lay out (the optimizer leaves the last target's bound)."""
        if not 0 <= int(m) < len(self.family):
            raise ValueError(f"member index {m} outside the family")
        self._member = int(m)

    def gate_sequence(self, k=None) -> List[int]:
        k = self.cycles if k is None else k
        return [self._member] * int(k)

    def member_template(self, r: int) -> CircuitTemplate:
        """The ``CircuitTemplate`` of member x``r`` alone: ``build(k); eval(Xk)`` reproduces a target fitted with it."""
        m = self.family.member_index(r)
        return CircuitTemplate(base_gates=[self.family.gates[m]], maximum_span_guess=max(len(self.family.table(m)), 1), device=self.device)

    def get_spanning_range(self, target_u):
        """The one-element range of the looked-up k (host lookup), with that member left bound."""
        res = self.family.lookup(fam_coords(np.asarray(target_u)[None]), self.policy)
        k = int(res.gates[0])
        if k < 0:
            raise self.family.unreachable_error()
        if k > 0:
            self.bind_member(int(res.member[0]))
        return range(k, k + 1)
