"""An independent, literal restatement of the family walk (reference: ``recursive_sibling_check``,
src/slam/utils/gates/family_extend.py:17-117): a recursive function, one target at a time, that takes each level's k from a plain
``for k in range(1, ...)`` loop over ``coverage.contains``.  It shares no code with ``family_extend.GateFamily.lookup`` /
``family_extend.walk``: the members, their links and their durations are rebuilt here from the base gate's parameters.

A member is the dict ``{"r", "coords", "duration", "k_max"}``; ``members`` is the list in increasing r.
"""
import math

import numpy as np

from slam_decomposition_amd import coverage
from slam_decomposition_amd.gates import ConversionGainGate
from slam_decomposition_amd.weyl import c1c2c3

TOL = 1e-7  # pulse_cost.TOL


def build_members(base_gate, basis_factor=None, max_gates=48):
    pc, pg, gc, gg, t = (float(v) for v in base_gate.params)
    factor = base_gate.cost() if basis_factor is None else basis_factor
    rs = []
    for a in range(12):
        for b in range(8):
            r = 2**a * 3**b
            if (abs(gc) + abs(gg)) * t * r <= math.pi / 2 * (1 + 1e-12):  # family_extend.py:96 after normalize_duration(1)
                rs.append(r)
    members = []
    for r in sorted(rs):
        g = ConversionGainGate(pc, pg, gc, gg, t * r)
        g.normalize_duration(1)
        members.append({"r": r, "coords": c1c2c3(g.to_matrix()), "duration": r * factor, "k_max": -(-max_gates // r), "gate": g})
    return members


def child_of(members, m, factor):
    want = members[m]["r"] * factor
    for j, mem in enumerate(members):
        if mem["r"] == want:
            return j
    return -1


def is_local(coords) -> bool:
    for shift in (0.0, 0.5):
        a = coverage.alcove_coordinates(np.asarray(coords).reshape(1, 3), shift)[0]
        if abs(a[0]) <= 1e-8 and abs(a[3]) <= 1e-8:
            return True
    return False


def smallest_k(member, coords, tol=TOL, memo=None):
    """The smallest number of applications of the member that reaches the target, or None within its k_max.  ``memo`` (a dict) keeps
    the answers of one test for both policies."""
    key = (member["r"], tuple(float(v) for v in np.ravel(coords)), tol)
    if memo is not None and key in memo:
        return memo[key]
    t = np.asarray(coords, dtype=np.float64).reshape(1, 3)
    found = None
    for k in range(1, member["k_max"] + 1):
        if coverage.contains(t, [member["coords"]] * k, tol)[0]:
            found = k
            break
    if memo is not None:
        memo[key] = found
    return found


def walk_tables(k_of, child_even, child_odd, durations, cost_1q, m=0):
    """The recursion itself on a hand-made table: ``k_of[m]`` = the k of member m (None / 0: the member does not contain the target).
    Returns ``(member, k, cost)``, or None where member m does not contain the target."""
    ki = k_of[m]
    if not ki:
        return None
    own_cost = (ki + 1) * cost_1q + ki * durations[m]  # "cost to beat"
    if ki == 1:
        return m, 1, own_cost
    sibling = child_even[m] if ki % 2 == 0 else child_odd[m]
    sib = walk_tables(k_of, child_even, child_odd, durations, cost_1q, sibling) if sibling >= 0 else None
    if sib is not None and sib[2] < own_cost:
        return sib
    return m, ki, own_cost


def best_tables(k_of, durations, cost_1q):
    """policy "best": the cheapest member that contains the target, the smaller member on a tie; None if member 0 does not."""
    if not k_of[0]:
        return None
    out = None
    for m, ki in enumerate(k_of):
        if ki:
            cost = (ki + 1) * cost_1q + ki * durations[m]
            if out is None or cost < out[2]:
                out = (m, ki, cost)
    return out


def family_ref(members, coords, cost_1q=0.1, policy="reference", tol=TOL, memo=None):
    """``(r, k, cost)`` for one target: (None, 0, 0.0) for a local one, (None, -1, inf) for one the base member does not reach."""
    if is_local(coords):
        return None, 0, 0.0
    if policy == "best":
        k_of = [smallest_k(mem, coords, tol, memo) for mem in members]
        res = best_tables(k_of, [mem["duration"] for mem in members], cost_1q)
    else:
        res = _recurse(members, coords, cost_1q, 0, tol, memo)
    if res is None:
        return None, -1, math.inf
    return members[res[0]]["r"], res[1], res[2]


def _recurse(members, coords, cost_1q, m, tol, memo=None):
    ki = smallest_k(members[m], coords, tol, memo)
    if ki is None:
        return None
    child_cost = (ki + 1) * cost_1q + ki * members[m]["duration"]
    if ki == 1:
        return m, 1, child_cost
    sibling = child_of(members, m, 2 if ki % 2 == 0 else 3)
    sib = _recurse(members, coords, cost_1q, sibling, tol, memo) if sibling >= 0 else None
    if sib is not None and sib[2] < child_cost:
        return sib
    return m, ki, child_cost
