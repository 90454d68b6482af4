"""Closed-form decompositions: circuits that equal their two-qubit targets from a formula -- no optimiser, no restarts, no failures.
``decompose`` dispatches on the basis gate as the reference's ``RootiSwapWeylDecomposition.run`` does
(src/slam/utils/transpiler_pass/weyl_decompose.py:475-480): ``RiSwapGate(1/2)`` to ``sqiswap_decompose``, a gate of the CNOT class or of
the iSWAP class (the reference's ``TwoQubitBasisDecomposer`` branch, what ``pass_manager_basic(gate="cx")`` runs) to ``cx_decompose``.

sqrt(iSWAP) gates (reference: ``RootiSwapWeylDecomposition.riswapWeylDecomp``,
src/slam/utils/transpiler_pass/weyl_decompose.py:343-449, after Huang et al., arXiv:2105.06074).

For ``RiSwapGate(1/2)`` a circuit that equals a two-qubit target is a formula: two gates where |z| <= x - y in the folded Weyl chamber,
three otherwise -- no optimiser, no restarts, no failures.  The whole pass runs on the GPU, one thread per target
(``slam_sqiswap_decompose``, csrc/slam_analytic.hpp); there is no CPU path.  Like the reference's pass it returns two or three gates
only: a local target and a target in sqrt(iSWAP)'s own class get a valid two-gate circuit.

    res = sqiswap_decompose(DeviceHaarBatch(seed=7, n_samples=1 << 20))
    res.cycles, res.Xk, res.loss, res.gap
    e = res.entries()[0]
    basis = CircuitTemplate(base_gates=[RiSwapGate(1 / 2)]); basis.build(e.cycles); basis.eval(e.Xk)   # the target, up to a phase

Gates of the CNOT class (CX, CZ, ...) and of the iSWAP class: one gate for a target of the gate's own class, two where c3 = 0, three
otherwise (``span_rules.minimal_span``; a local target gets two), with interior angles that are linear in the target's KAK coordinates
(Vatan and Williams, quant-ph/0308006; ``slam_cx_decompose``, csrc/slam_cx.hpp):

    res = cx_decompose(DeviceHaarBatch(seed=7, n_samples=1 << 20), CXGate())
    basis = CircuitTemplate(base_gates=[CXGate()]); basis.build(e.cycles); basis.eval(e.Xk)            # likewise

Gates of the B class, CAN(1/2, 1/4, 0): one gate for a target of that class, two for EVERY other target (Zhang, Vala, Sastry, Whaley,
PRL 93, 020502; ``slam_b_decompose``, csrc/slam_b.hpp).  ``decompose`` does not dispatch to it yet:

    res = b_decompose(DeviceHaarBatch(seed=7, n_samples=1 << 20), BerkeleyGate())
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import List

import numpy as np

from . import runtime
from .basis_abc import DataDictEntry
from .gates import CXGate, gate_matrix


@dataclass
class SqiswapDecomposition:
    """``cycles`` int32[N] (2 or 3), ``Xk`` float64[N, 24] (the 6 (cycles + 1) template angles in the front of each row, zeros
    behind), ``loss`` float64[N] (BasicCost of the circuit against its target), ``gap`` float64[N] (coordinate gap left by the interior
    formula, units of pi; loss <= 1 - cos(1.5 pi gap))."""

    cycles: np.ndarray
    Xk: np.ndarray
    loss: np.ndarray
    gap: np.ndarray
    success_threshold: float = 1e-10

    def __len__(self) -> int:
        return len(self.cycles)

    def entries(self) -> List[DataDictEntry]:
        """One ``DataDictEntry`` per target, as ``TemplateOptimizer.approximate_from_distribution`` returns them: ``Xk`` is the list
        of the 6 (cycles + 1) angles of ``CircuitTemplate(base_gates=[RiSwapGate(1/2)]).build(cycles)``."""
        return [DataDictEntry(int(self.loss[i] <= self.success_threshold), float(self.loss[i]), self.Xk[i, : 6 * (int(k) + 1)].tolist(), int(k))
                for i, k in enumerate(self.cycles)]


@dataclass
class CxDecomposition(SqiswapDecomposition):
    """The same fields for circuits of ``basis_gate`` (``cycles`` 1, 2 or 3; ``gap`` is the coordinate gap left by the alignment of the
    interior circuit): ``entries()`` rows are those of ``CircuitTemplate(base_gates=[basis_gate]).build(cycles)``."""

    basis_gate: object = None


def _resident(ctx, targets) -> int:
    """Makes ``targets`` the resident batch of ``ctx``; their number."""
    if hasattr(targets, "fill") and hasattr(targets, "n_samples"):  # a device sampler (an ndarray has a fill of its own)
        n = int(targets.n_samples)
        if n > 0:
            targets.fill(ctx)
    else:
        T = np.asarray(targets if isinstance(targets, np.ndarray) else [np.asarray(t) for t in targets], dtype=np.complex128)
        if T.size == 0:
            T = T.reshape(0, 4, 4)
        if T.ndim != 3 or T.shape[1:] != (4, 4):
            raise ValueError("targets must have shape [N, 4, 4]")
        n = len(T)
        if n > 0:
            ctx.set_targets(T)
    return n


def _empty(cls, *tail):
    """The result of class ``cls`` for no targets; ``tail`` are the fields behind the four arrays."""
    return cls(np.zeros(0, dtype=np.int32), np.zeros((0, 24)), np.zeros(0), np.zeros(0), *tail)


def sqiswap_decompose(targets, device: int = 0, success_threshold: float = 1e-10) -> SqiswapDecomposition:
    """Circuits of two or three sqrt(iSWAP) gates that equal ``targets``: an ``[N, 4, 4]`` array, a list of 4x4 matrices, any
    ``SampleFunction``, or a device sampler (``DeviceHaarBatch``, ``DeviceHaarSpanBatch``: anything with ``fill(ctx)``), whose targets
    are generated on the device and stay there."""
    ctx = runtime.get_context(device)
    n = _resident(ctx, targets)
    if n == 0:
        return _empty(SqiswapDecomposition, success_threshold)
    x, cycles, loss, gap = ctx.sqiswap_decompose(0, n)
    return SqiswapDecomposition(cycles, x, loss, gap, success_threshold)


def _gate_decompose(targets, basis_gate, check, call, device: int, success_threshold: float) -> CxDecomposition:
    """``cx_decompose`` and ``b_decompose``: ``check`` (of ``_ffi``) raises for a gate outside the class before any context is made,
    ``call`` names the ``Context`` method."""
    g = gate_matrix(basis_gate)
    check(g)
    ctx = runtime.get_context(device)
    n = _resident(ctx, targets)
    if n == 0:
        return _empty(CxDecomposition, success_threshold, basis_gate)
    x, cycles, loss, gap = getattr(ctx, call)(g, 0, n)
    return CxDecomposition(cycles, x, loss, gap, success_threshold, basis_gate)


def cx_decompose(targets, basis_gate=None, device: int = 0, success_threshold: float = 1e-10) -> CxDecomposition:
    """Circuits of one, two or three gates ``basis_gate`` (default ``CXGate()``; any gate object or 4x4 matrix of the CNOT class or of
    the iSWAP class: ``CZGate``, ``iSwapGate``, a ``CanonicalGate``, ``UnitaryGate`` or ``ConversionGainGate`` at those points) that
    equal ``targets``, which are given as for ``sqiswap_decompose``.  ``ValueError`` for a gate outside both classes."""
    from . import _ffi

    return _gate_decompose(targets, CXGate() if basis_gate is None else basis_gate, _ffi.cx_family, "cx_decompose", device, success_threshold)


def b_decompose(targets, basis_gate=None, device: int = 0, success_threshold: float = 1e-10) -> CxDecomposition:
    """Circuits of one or two gates ``basis_gate`` (default ``BerkeleyGate()``; any gate object or 4x4 matrix of the B class: a
    ``CanonicalGate`` or ``UnitaryGate`` at that point, dressed with local gates or not) that equal ``targets``, which are given as for
    ``sqiswap_decompose``: one gate for a target of the gate's own class, two for every other one (a local target included).
    ``ValueError`` for a gate outside the class."""
    from . import _ffi
    from .gates import BerkeleyGate

    return _gate_decompose(targets, BerkeleyGate() if basis_gate is None else basis_gate, _ffi.b_class, "b_decompose", device, success_threshold)


def decompose(targets, basis_gate, device: int = 0, success_threshold: float = 1e-10) -> SqiswapDecomposition:
    """The closed-form decomposition that exists for ``basis_gate``, chosen as the reference's pass chooses it: ``RiSwapGate(1/2)`` (any
    gate whose matrix is that gate's) goes to ``sqiswap_decompose``, a gate of the CNOT class or of the iSWAP class to
    ``cx_decompose``; ``NotImplementedError`` naming the gate's Weyl coordinates for anything else -- a gate of the B class included,
    which ``b_decompose`` takes when it is called by name."""
    from . import _ffi, weyl
    from .gates import RiSwapGate

    g = gate_matrix(basis_gate)
    if np.max(np.abs(g - gate_matrix(RiSwapGate(1 / 2)))) <= 1e-12:
        return sqiswap_decompose(targets, device, success_threshold)
    try:
        _ffi.cx_family(g)
    except ValueError:
        raise NotImplementedError(
            "closed-form decompositions exist for RiSwapGate(1/2) and for basis gates of the CNOT class (0.5, 0, 0) and of the iSWAP "
            f"class (0.5, 0.5, 0) only (got {basis_gate} with Weyl coordinates {tuple(float(v) for v in weyl.c1c2c3(g))}); a gate of "
            "the B class (0.5, 0.25, 0) is not dispatched here: call b_decompose") from None
    return cx_decompose(targets, basis_gate, device, success_threshold)
