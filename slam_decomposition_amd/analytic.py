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

All of the above assume a perfect basis gate.  ``approx_decompose`` is the other half of qiskit's ``TwoQubitBasisDecomposer``: given the
fidelity f of one basis gate (CNOT, iSWAP or B class) it builds the best circuit of 0, 1, 2 and 3 gates in closed form and returns the
one with the highest expected fidelity F_k f^k (``slam_approx_decompose``, csrc/slam_approx.hpp); a local target costs no gate.
``fidelity_sweep`` asks the same question of a whole distribution for many f in one launch:

    res = approx_decompose(DeviceHaarBatch(seed=7, n_samples=1 << 20), CXGate(), basis_fidelity=0.99)
    res.cycles, res.loss, res.predicted_loss, res.expected_fidelity
    sw = fidelity_sweep(DeviceHaarBatch(seed=7, n_samples=1 << 22), CXGate(), np.linspace(0.9, 1.0, 16))
    sw.counts, sw.average_gates, sw.average_fidelity

The three classes are three points of one line of the Weyl chamber, the supercontrolled gates CAN(1/2, beta, 0), on which every
full-strength conversion-gain gate lies.  ``sc_decompose`` is ``approx_decompose`` for any gate of that line (``slam_sc_decompose``,
csrc/slam_sc.hpp); ``decompose``, ``approx_decompose`` and ``fidelity_sweep`` go there for the gates between the three points:

    res = sc_decompose(DeviceHaarBatch(seed=7, n_samples=1 << 20), ConversionGainGate(0, 0, 0.4 * np.pi, 0.1 * np.pi, 1), basis_fidelity=0.99)

sqrt(iSWAP) is not on that line: two of it reach a solid region of the chamber, |z| <= x - y, and the nearest point of that region
has a closed form of its own (csrc/slam_sqapprox.hpp).  ``sqiswap_approx_decompose`` and ``sqiswap_fidelity_sweep`` are the entry
points for an imperfect ``RiSwapGate(1/2)`` -- 0, 1, 2 or 3 gates by expected fidelity, the sizes of ``sqiswap_decompose`` at f = 1
except that a local target costs no gate and a target of the gate's class one; ``approx_decompose``, ``fidelity_sweep`` and
``decompose`` do not dispatch to them yet:

    res = sqiswap_approx_decompose(DeviceHaarBatch(seed=7, n_samples=1 << 20), basis_fidelity=0.99)
    sw = sqiswap_fidelity_sweep(DeviceHaarBatch(seed=7, n_samples=1 << 22), np.linspace(0.9, 1.0, 16))
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


@dataclass
class ApproxDecomposition(CxDecomposition):
    """The fields of ``CxDecomposition`` for the circuit of highest expected fidelity (``cycles`` 0..3; a row of no gate holds one
    layer, 6 angles; ``gap`` is the chamber distance to the nearest point that ``cycles`` gates reach), and ``predicted_loss``
    float64[N] (1 - t_k of the closed form), ``expected_fidelity`` float64[N] ((4 + 16 (1 - loss)^2) / 20 * basis_fidelity^cycles)
    and ``basis_fidelity``."""

    predicted_loss: np.ndarray = None
    expected_fidelity: np.ndarray = None
    basis_fidelity: float = 1.0


@dataclass
class FidelitySweep:
    """``counts`` int64[n, 4] (targets per chosen size 0..3), ``average_gates`` and ``average_fidelity`` float64[n] per entry of
    ``basis_fidelities``, over ``n_targets`` targets."""

    basis_fidelities: np.ndarray
    counts: np.ndarray
    average_gates: np.ndarray
    average_fidelity: np.ndarray
    n_targets: int
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


_SC_FAMILY = -1  # what ``_approx_gate`` returns for a supercontrolled gate outside the three named classes


def _approx_gate(basis_gate):
    """``(matrix, family)`` of a gate that ``_ffi.approx_family`` accepts, ``(matrix, _SC_FAMILY)`` of any other supercontrolled gate
    (``_ffi.sc_class``); ``NotImplementedError`` naming its coordinates otherwise."""
    from . import _ffi, weyl

    g = gate_matrix(basis_gate)
    try:
        return g, _ffi.approx_family(g)
    except ValueError:
        pass
    try:
        _ffi.sc_class(g)
    except ValueError:
        raise NotImplementedError(
            "approximate closed-form decompositions exist for basis gates of the CNOT class (0.5, 0, 0), the iSWAP class (0.5, 0.5, 0) "
            "and the B class (0.5, 0.25, 0), and of every other supercontrolled class (0.5, beta, 0), "
            f"only (got {basis_gate} with Weyl coordinates {tuple(float(v) for v in weyl.c1c2c3(g))}); "
            "no closed form for the nearest two-gate point of sqrt(iSWAP) is established here") from None
    return g, _SC_FAMILY


def sc_decompose(targets, basis_gate, basis_fidelity: float = 1.0, cycles=None, device: int = 0,
                 success_threshold: float = 1e-10) -> ApproxDecomposition:
    """``approx_decompose`` for ANY supercontrolled ``basis_gate``, one of a class CAN(1/2, beta, 0) with 0 <= beta <= 1/2 -- the line
    of the Weyl chamber through the CNOT, the B and the iSWAP class, on which every full-strength conversion-gain gate
    (``ConversionGainGate(0, 0, gc, gg, 1)`` with gc + gg = pi/2) lies, dressed with local gates or not: per target the circuit of 0,
    1, 2 or 3 gates with the highest expected fidelity F_k * basis_fidelity^k (``slam_sc_decompose``, csrc/slam_sc.hpp; the
    construction of qiskit's ``TwoQubitBasisDecomposer``, exact with three gates for every target).  One known limit, shared with
    that decomposer: for 0 < beta < 1/2 two gates reach more than the plane c3 = 0, but the two-gate formula is exact on that plane
    only, so at ``basis_fidelity=1`` a target off it gets three gates even where an optimiser finds two; at beta = 1/4 this returns
    three where ``b_decompose`` returns two.  ``targets`` and ``cycles`` as for ``approx_decompose``.  ``ValueError`` for a gate off the
    line (before any context is made), a fidelity outside (0, 1] and a size outside 0..3."""
    from . import _ffi

    g = gate_matrix(basis_gate)
    _ffi.sc_class(g)
    f = _ffi.check_basis_fidelity(basis_fidelity)
    if cycles is not None and not (isinstance(cycles, (int, np.integer)) and 0 <= cycles <= 3):
        raise ValueError(f"cycles must be None or an integer in 0..3 for {basis_gate}, got {cycles!r}")
    ctx = runtime.get_context(device)
    n = _resident(ctx, targets)
    if n == 0:
        return _empty(ApproxDecomposition, success_threshold, basis_gate, np.zeros(0), np.zeros(0), f)
    x, size, loss, predicted, gap = ctx.sc_decompose(g, f, cycles, 0, n)
    expected = (4.0 + 16.0 * (1.0 - loss) ** 2) / 20.0 * f ** size
    return ApproxDecomposition(size, x, loss, gap, success_threshold, basis_gate, predicted, expected, f)


def approx_decompose(targets, basis_gate=None, basis_fidelity: float = 1.0, cycles=None, device: int = 0,
                     success_threshold: float = 1e-10) -> ApproxDecomposition:
    """Per target the circuit of 0, 1, 2 or 3 gates ``basis_gate`` (default ``CXGate()``; any gate of the CNOT, the iSWAP or the B
    class, which has no 3) with the highest expected fidelity F_k * basis_fidelity^k, F_k the average gate fidelity of the best circuit
    of k gates -- what qiskit's ``TwoQubitBasisDecomposer(gate, basis_fidelity)`` chooses; ties go to fewer gates, so
    ``basis_fidelity=1`` gives the fewest gates that equal the target and no gate for a local one.  ``cycles=k`` takes that size for
    every target.  ``targets`` are given as for ``sqiswap_decompose``.  A supercontrolled gate outside the three classes goes to
    ``sc_decompose``.  ``NotImplementedError`` for ``RiSwapGate(1/2)`` and every other gate that is not supercontrolled, ``ValueError``
    for a fidelity outside (0, 1] and a size the gate's class does not have."""
    from . import _ffi

    basis_gate = CXGate() if basis_gate is None else basis_gate
    g, family = _approx_gate(basis_gate)
    if family == _SC_FAMILY:
        return sc_decompose(targets, basis_gate, basis_fidelity, cycles, device, success_threshold)
    f = _ffi.check_basis_fidelity(basis_fidelity)
    k_max = 2 if family == _ffi.FAMILY_B else 3
    if cycles is not None and not (isinstance(cycles, (int, np.integer)) and 0 <= cycles <= k_max):
        raise ValueError(f"cycles must be None or an integer in 0..{k_max} for {basis_gate}, got {cycles!r}")
    ctx = runtime.get_context(device)
    n = _resident(ctx, targets)
    if n == 0:
        return _empty(ApproxDecomposition, success_threshold, basis_gate, np.zeros(0), np.zeros(0), f)
    x, size, loss, predicted, gap = ctx.approx_decompose(g, f, cycles, 0, n)
    expected = (4.0 + 16.0 * (1.0 - loss) ** 2) / 20.0 * f ** size
    return ApproxDecomposition(size, x, loss, gap, success_threshold, basis_gate, predicted, expected, f)


def _check_fidelities(basis_fidelities) -> np.ndarray:
    """``basis_fidelities`` as a float64 vector of 1.. ``_ffi.APPROX_MAX_FID`` entries of (0, 1]; ``ValueError`` otherwise."""
    from . import _ffi

    f = np.ascontiguousarray(basis_fidelities, dtype=np.float64).reshape(-1)
    if not 1 <= len(f) <= _ffi.APPROX_MAX_FID:
        raise ValueError(f"between 1 and {_ffi.APPROX_MAX_FID} basis fidelities per call, got {len(f)}")
    for v in f:
        _ffi.check_basis_fidelity(v)
    return f


def fidelity_sweep(targets, basis_gate, basis_fidelities, device: int = 0) -> FidelitySweep:
    """The Haar-expected (or any distribution's) gate count and fidelity of ``basis_gate`` at each of ``basis_fidelities`` (at most
    ``_ffi.APPROX_MAX_FID``), from one launch over ``targets`` (``slam_approx_counts``): the choice of ``approx_decompose`` per target
    and fidelity, counted per size, and the mean of the chosen expected fidelities (summed in fixed point, 2^-32: the result does not
    depend on the order of addition).  Refusals as ``approx_decompose``."""
    g, family = _approx_gate(basis_gate)
    f = _check_fidelities(basis_fidelities)
    ctx = runtime.get_context(device)
    n = _resident(ctx, targets)
    if n == 0:
        return FidelitySweep(f, np.zeros((len(f), 4), dtype=np.int64), np.full(len(f), np.nan), np.full(len(f), np.nan), 0, basis_gate)
    counts, fidsum = (ctx.sc_counts if family == _SC_FAMILY else ctx.approx_counts)(g, f, 0, n)
    return FidelitySweep(f, counts, counts @ np.arange(4.0) / n, fidsum / 4294967296.0 / n, n, basis_gate)


def sqiswap_approx_decompose(targets, basis_fidelity: float = 1.0, cycles=None, device: int = 0,
                             success_threshold: float = 1e-10) -> ApproxDecomposition:
    """The entry point for an imperfect sqrt(iSWAP): ``approx_decompose`` for ``RiSwapGate(1/2)``, which that function refuses.  Per
    target the circuit of 0, 1, 2 or 3 sqrt(iSWAP) gates with the highest expected fidelity F_k * basis_fidelity^k
    (``slam_sqiswap_approx_decompose``, csrc/slam_sqapprox.hpp): no gate, one gate, the nearest point of the region |z| <= x - y that
    two gates reach (the target itself inside it), and the three gates of ``sqiswap_decompose``; ties go to fewer gates, so
    ``basis_fidelity=1`` gives the sizes of ``sqiswap_decompose`` except that a local target costs no gate and a target of the gate's
    own class one.  ``cycles=k`` takes that size for every target.  ``targets`` are given as for ``sqiswap_decompose``; the result's
    ``basis_gate`` is ``RiSwapGate(1/2)``.  ``ValueError`` (before any context is made) for a fidelity outside (0, 1] and a size
    outside 0..3."""
    from . import _ffi
    from .gates import RiSwapGate

    f = _ffi.check_basis_fidelity(basis_fidelity)
    if cycles is not None and not (isinstance(cycles, (int, np.integer)) and 0 <= cycles <= 3):
        raise ValueError(f"cycles must be None or an integer in 0..3, got {cycles!r}")
    basis_gate = RiSwapGate(1 / 2)
    ctx = runtime.get_context(device)
    n = _resident(ctx, targets)
    if n == 0:
        return _empty(ApproxDecomposition, success_threshold, basis_gate, np.zeros(0), np.zeros(0), f)
    x, size, loss, predicted, gap = ctx.sqiswap_approx_decompose(f, cycles, 0, n)
    expected = (4.0 + 16.0 * (1.0 - loss) ** 2) / 20.0 * f ** size
    return ApproxDecomposition(size, x, loss, gap, success_threshold, basis_gate, predicted, expected, f)


def sqiswap_fidelity_sweep(targets, basis_fidelities, device: int = 0) -> FidelitySweep:
    """The entry point for the sweep of an imperfect sqrt(iSWAP): ``fidelity_sweep`` for ``RiSwapGate(1/2)``, which that function
    refuses -- the choice of ``sqiswap_approx_decompose`` per target at each of ``basis_fidelities`` (at most
    ``_ffi.APPROX_MAX_FID``), counted per size, and the mean of the chosen expected fidelities, from one launch
    (``slam_sqiswap_approx_counts``).  ``ValueError`` (before any context is made) for a fidelity outside (0, 1] and for no or too
    many fidelities."""
    from .gates import RiSwapGate

    f = _check_fidelities(basis_fidelities)
    basis_gate = RiSwapGate(1 / 2)
    ctx = runtime.get_context(device)
    n = _resident(ctx, targets)
    if n == 0:
        return FidelitySweep(f, np.zeros((len(f), 4), dtype=np.int64), np.full(len(f), np.nan), np.full(len(f), np.nan), 0, basis_gate)
    counts, fidsum = ctx.sqiswap_approx_counts(f, 0, n)
    return FidelitySweep(f, counts, counts @ np.arange(4.0) / n, fidsum / 4294967296.0 / n, n, basis_gate)


def decompose(targets, basis_gate, device: int = 0, success_threshold: float = 1e-10) -> SqiswapDecomposition:
    """The closed-form decomposition that exists for ``basis_gate``, chosen as the reference's pass chooses it: ``RiSwapGate(1/2)`` (any
    gate whose matrix is that gate's) goes to ``sqiswap_decompose``, a gate of the CNOT class or of the iSWAP class to
    ``cx_decompose``, any other supercontrolled gate CAN(1/2, beta, 0) -- the reference's ``TwoQubitBasisDecomposer`` branch again --
    to ``sc_decompose`` with a perfect gate; ``NotImplementedError`` naming the gate's Weyl coordinates for anything else -- a gate of
    the B class included, which ``b_decompose`` takes when it is called by name."""
    from . import _ffi, weyl
    from .gates import RiSwapGate

    g = gate_matrix(basis_gate)
    if np.max(np.abs(g - gate_matrix(RiSwapGate(1 / 2)))) <= 1e-12:
        return sqiswap_decompose(targets, device, success_threshold)
    try:
        _ffi.cx_family(g)
    except ValueError:
        try:
            family = _approx_gate(basis_gate)[1]  # the B class has a family of its own and keeps its refusal
        except NotImplementedError:
            family = None
        if family == _SC_FAMILY:
            return sc_decompose(targets, basis_gate, 1.0, None, device, success_threshold)
        raise NotImplementedError(
            "closed-form decompositions exist for RiSwapGate(1/2) and for basis gates of the CNOT class (0.5, 0, 0) and of the iSWAP "
            "class (0.5, 0.5, 0), and of every other supercontrolled class (0.5, beta, 0), "
            f"only (got {basis_gate} with Weyl coordinates {tuple(float(v) for v in weyl.c1c2c3(g))}); a gate of "
            "the B class (0.5, 0.25, 0) is not dispatched here: call b_decompose") from None
    return cx_decompose(targets, basis_gate, device, success_threshold)
