"""Cost functions (reference: src/slam/cost_function.py:117-145).

``BasicCost``, ``SquareCost`` (the monotone map 0.8 (2 L - L^2) of BasicCost L, cost_function.py:169-173) and
``MakhlinFunctionalCost`` (cost_function.py:219-221) are the objectives the HIP optimizer implements (``slam_set_cost``); anything
else makes ``TemplateOptimizer`` raise the reference's "Unrecognized Cost Function".  The classes keep the reference's interface; ``unitary_fidelity`` on two single matrices is the reference's own
one-line NumPy expression (used for spot checks and logging, never inside the optimizer loop --
there the loss is fused into the HIP kernel).
"""
from __future__ import annotations

from abc import ABC

import numpy as np


class UnitaryCostFunction(ABC):
    def __init__(self):
        self.normalization = 1  # src/slam/cost_function.py:123

    def unitary_fidelity(self, current_u, target_u):
        raise NotImplementedError


class BasicCost(UnitaryCostFunction):
    """1 - |Tr(T^dagger U)| / d  (src/slam/cost_function.py:140-145)."""

    def unitary_fidelity(self, current_u, target_u):
        h = np.asarray(target_u).conj().T
        cur = np.asarray(current_u)
        return 1 - np.abs(np.trace(h @ cur)) / cur.shape[0]


class SquareCost(UnitaryCostFunction):
    """1 - (|Tr(T^dagger U)|^2 + d) / (d (d + 1))  (src/slam/cost_function.py:169-173): the objective most
    of the reference's notebooks use.  On the HIP path it is the same fused kernel with a different
    scalar map of |Tr| (and of the gradient scale)."""

    def unitary_fidelity(self, current_u, target_u):
        h = np.asarray(target_u).conj().T
        d = np.asarray(target_u).shape[0]
        return 1 - (np.abs(np.trace(h @ np.asarray(current_u))) ** 2 + d) / (d * (d + 1))


class MakhlinFunctionalCost(UnitaryCostFunction):
    """J = sum_i (g_i(U) - g_i(T))^2 over the Makhlin local invariants g = (Re G1, Im G1, Re G2) (src/slam/cost_function.py:219-221,
    weylchamber's ``J_T_LI``): the distance between the local-equivalence classes of U and T, zero whenever U = K1 T K2 with
    single-qubit K1, K2.  The reference's invariants come rounded to 8 digits, which leaves the functional piecewise constant
    below 1e-8; here -- on the host and in the HIP kernels -- it is the UNROUNDED functional."""

    def unitary_fidelity(self, current_u, target_u):
        from .weyl import g1g2g3

        d = np.asarray(g1g2g3(current_u)) - np.asarray(g1g2g3(target_u))
        return float(d @ d)
