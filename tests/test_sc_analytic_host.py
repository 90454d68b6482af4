"""CPU: the yardstick of the closed-form decomposition into gates of any supercontrolled class CAN(1/2, beta, 0) -- tests/sc_ref.py, the
NumPy restatement the GPU tests compare ``slam_sc_decompose`` with -- does what it says, and the host side of the feature:
``_ffi.sc_class``, the dress builder against the library's own check of it, the exported symbols, and the dispatch of
``analytic.decompose`` / ``approx_decompose`` / ``fidelity_sweep`` in front of a recording context.

Bounds.  The construction is an identity, so what remains is the rounding of some twenty 2x2 and five 4x4 products: observed worst
BasicCost over beta in {0, 1e-3, 1/8, 0.3, 1/4, 0.45, 1/2} x 40 random chamber points with random local factors, 1.6e-15 (three gates,
and two gates on the plane c3 = 0); the assertion is 8x that, 1.3e-14.  The realised |Tr| / 4 of the 0-, 1- and 2-gate circuits against
t_k: observed 1.4e-15, asserted 1.2e-14.  The kernel's route (interior layers, then two KAK forms aligned) adds two eigen-decompositions:
its loss is held to the 1e-13 of the sibling families (tests/test_b_analytic_host.py), observed 1.1e-15.
"""
import ctypes

import numpy as np
import pytest

import approx_ref as ar
import kak_ref as kr
import sc_ref as sr

BETAS = (0.0, 1e-3, 1 / 8, 0.3, 1 / 4, 0.45, 1 / 2)
CG = dict(gc=3 * np.pi / 8 + 0.05, gg=np.pi / 8 - 0.05)  # gc + gg = pi / 2, off the B point: beta = (gc - gg) / pi


def _cg_gate():
    from slam_decomposition_amd.gates import ConversionGainGate

    return ConversionGainGate(0.0, 0.0, CG["gc"], CG["gg"], 1.0)


def _chamber_point(rng):
    c = -np.sort(-rng.uniform(0.0, 0.5, 3))
    c[2] *= rng.choice([-1.0, 1.0])
    return c


def _locals(rng):
    return tuple(kr.random_su2(rng, 2))


def test_the_construction_reproduces_its_targets():
    rng = np.random.default_rng(11)
    worst3 = worst2 = worst_t = 0.0
    for beta in BETAS:
        for _ in range(40):
            c = _chamber_point(rng)
            abc = 0.5 * np.pi * c
            K1, K2 = _locals(rng), _locals(rng)
            T = np.kron(*K1) @ sr.can(c) @ np.kron(*K2)
            worst3 = max(worst3, sr.loss_of(T, sr.circuit(3, abc, beta, K1, K2)))
            T0 = np.kron(*K1) @ sr.can((c[0], c[1], 0.0)) @ np.kron(*K2)
            worst2 = max(worst2, sr.loss_of(T0, sr.circuit(2, (abc[0], abc[1], 0.0), beta, K1, K2)))
            t = sr.traces(c[None] if c[2] >= 0 else np.array([[1 - c[0], c[1], -c[2]]]), beta)[0]
            for k in range(3):
                worst_t = max(worst_t, abs(1.0 - sr.loss_of(T, sr.circuit(k, abc, beta, K1, K2)) - t[k]))
    print(f"sc host construction: worst loss three gates {worst3:.3g}, two gates on c3 = 0 {worst2:.3g}, worst | |Tr|/4 - t_k | {worst_t:.3g}")
    assert worst3 <= 1.3e-14 and worst2 <= 1.3e-14
    assert worst_t <= 1.2e-14


def test_traces_are_those_of_the_named_families_at_their_points():
    rng = np.random.default_rng(2)
    c = rng.uniform(0.0, 1.0, (200, 3)) * [1.0, 0.5, 0.5]
    for family, beta in enumerate(ar.BETA):
        ours, theirs = sr.traces(c, beta), ar.traces(c, family)
        assert np.array_equal(ours[:, :2], theirs[:, :2])
        if family < 2:
            assert np.array_equal(ours, theirs)
            for f in (1.0, 0.99, 0.9):
                assert np.array_equal(sr.select(c, beta, f), ar.select(c, family, f))


@pytest.mark.parametrize("beta", BETAS)
def test_the_kernels_route_reaches_the_same_circuits(beta):
    """``sc_ref.decompose``: interior layers around a DRESSED gate, exterior layers by alignment -- exact sizes at f = 1, the predicted
    loss at every forced size."""
    rng = np.random.default_rng(int(beta * 1000) + 5)
    G = sr.dress(rng, sr.can((0.5, beta, 0.0)))
    worst = worst_forced = 0.0
    for j in range(6):
        c = _chamber_point(rng)
        if j == 0:
            c[2] = 0.0
        T = sr.dress(rng, sr.can(c))
        x, k, loss, predicted, gap = sr.decompose(T, G)
        assert k == (2 if j == 0 else 3) and len(x) == 6 * (k + 1)
        assert predicted == 0.0 and gap <= 1e-12
        worst = max(worst, loss)
        for force in range(4):
            x, k, loss, predicted, gap = sr.decompose(T, G, 0.9, force)
            assert k == force and len(x) == 6 * (k + 1)
            worst_forced = max(worst_forced, abs(loss - predicted))
    x, k, loss, _, _ = sr.decompose(G, G)
    assert k == 1 and loss <= 1e-13
    x, k, loss, _, _ = sr.decompose(np.kron(*_locals(rng)), G)
    assert k == 0 and len(x) == 6 and loss <= 1e-13
    print(f"sc host route beta {beta:g}: worst exact loss {worst:.3g}, worst |loss - predicted| over forced sizes {worst_forced:.3g}")
    assert worst <= 1e-13 and worst_forced <= 1e-13


def test_sc_class_accepts_the_line_and_refuses_the_rest():
    from slam_decomposition_amd import _ffi
    from slam_decomposition_amd.gates import (BerkeleyGate, CanonicalGate, CXGate, RiSwapGate, SwapGate, UnitaryGate, gate_matrix,
                                              iSwapGate)

    rng = np.random.default_rng(4)
    for beta in BETAS:
        for g in (sr.can((0.5, beta, 0.0)), sr.dress(rng, sr.can((0.5, beta, 0.0)))):
            assert abs(_ffi.sc_class(g) - beta) <= 1e-8
    for gate, beta in ((CXGate(), 0.0), (BerkeleyGate(), 0.25), (iSwapGate(), 0.5), (CanonicalGate(np.pi / 4, 0.15 * np.pi, 0.0), 0.3),
                       (_cg_gate(), (CG["gc"] - CG["gg"]) / np.pi)):
        assert abs(_ffi.sc_class(gate_matrix(gate)) - beta) <= 1e-8
    for gate in (SwapGate(), RiSwapGate(1 / 3), RiSwapGate(1 / 2), UnitaryGate(np.eye(4)), UnitaryGate(sr.can((0.5 - 1e-6, 0.3, 0.0)))):
        with pytest.raises(ValueError, match="Weyl coordinates"):
            _ffi.sc_class(gate_matrix(gate))
        with pytest.raises(ValueError, match="Weyl coordinates"):
            _ffi.sc_dress(gate_matrix(gate))


def test_symbols_are_declared_and_exported():
    from slam_decomposition_amd import _ffi

    lib = _ffi.load_library()
    for name, n_args in (("slam_sc_decompose", 12), ("slam_sc_counts", 9)):
        assert name in _ffi.EXPORTED_SYMBOLS
        fn = getattr(lib, name)
        assert fn.restype is ctypes.c_int and len(fn.argtypes) == n_args
    assert lib.slam_abi_version() == 7
    assert hasattr(_ffi.Context, "sc_decompose") and hasattr(_ffi.Context, "sc_counts")


@pytest.mark.parametrize("beta", BETAS)
def test_the_library_accepts_the_host_reduction(beta):
    """``_ffi.sc_dress`` rebuilds a dressed gate to 1e-12, and the library's own check of it, which runs before a context is needed,
    agrees: with a NULL context a good reduction gets as far as "ctx is NULL"; coordinates off the line, a gate that is not the reduced
    one, a perturbed factor, a bad fidelity and a bad size do not."""
    from slam_decomposition_amd import _ffi

    lib = _ffi.load_library()
    rng = np.random.default_rng(31)
    G = sr.dress(rng, sr.can((0.5, beta, 0.0)))
    g, dress = _ffi.sc_dress(G)
    assert dress.shape == (_ffi.SC_DRESS,)
    l1, l0, r1, r0 = dress[:32].view(np.complex128).reshape(4, 2, 2)
    assert sr.up_to_phase(G, np.kron(l1, l0) @ sr.can(dress[32:]) @ np.kron(r1, r0)) <= 1e-12
    fid = np.array([0.99, 0.9])

    def call(gate, d, f=0.99, force=-1):
        rc = lib.slam_sc_decompose(None, 0, 1, _ffi._ptr(np.ascontiguousarray(gate)), _ffi._ptr(np.ascontiguousarray(d)), f, force,
                                   None, None, None, None, None)
        return rc, lib.slam_last_error().decode()

    def call_counts(gate, d, n=2):
        rc = lib.slam_sc_counts(None, 0, 1, _ffi._ptr(np.ascontiguousarray(gate)), _ffi._ptr(np.ascontiguousarray(d)), n, _ffi._ptr(fid),
                                None, None)
        return rc, lib.slam_last_error().decode()

    for fn in (call, call_counts):
        rc, msg = fn(g, dress)
        assert rc != 0 and "ctx is NULL" in msg, msg
        for at, value in ((32, 0.5 - 1e-6), (33, 0.6), (34, 1e-6), (33, np.nan)):
            other = dress.copy()
            other[at] = value
            rc, msg = fn(g, other)
            assert rc != 0 and "coordinates" in msg, (at, msg)
        rc, msg = fn(sr.dress(np.random.default_rng(1), g), dress)
        assert rc != 0 and "rebuild the gate" in msg
        for at in (5, 8 * 1 + 2, 8 * 2 + 1, 8 * 3 + 6):
            bad = dress.copy()
            bad[at] += 1e-9
            rc, msg = fn(g, bad)
            assert rc != 0 and "rebuild the gate" in msg, (at, msg)
    for f in (0.0, 1.0 + 1e-12, -0.5, np.nan):
        rc, msg = call(g, dress, f=f)
        assert rc != 0 and "basis_fidelity" in msg
    for force in (-2, 4):
        rc, msg = call(g, dress, force=force)
        assert rc != 0 and "force_cycles" in msg
    for n in (0, 65):
        rc, msg = call_counts(g, dress, n)
        assert rc != 0 and "n_fid" in msg


class _RecordingCtx:
    n_targets = 0

    def __init__(self, calls):
        self.calls = calls

    def set_targets(self, T):
        self.n_targets = len(T)

    def _five(self, name, gate, count, size):
        self.calls.append((name, np.array(gate)))
        return np.zeros((count, 24)), np.full(count, size, dtype=np.int32), np.zeros(count), np.zeros(count), np.zeros(count)

    def sc_decompose(self, gate, f, cycles, first, count):
        return self._five("sc", gate, count, 3 if cycles is None else cycles)

    def approx_decompose(self, gate, f, cycles, first, count):
        return self._five("approx", gate, count, 3)

    def cx_decompose(self, gate, first, count):
        return self._five("cx", gate, count, 3)[:4]

    def sc_counts(self, gate, f, first, count):
        self.calls.append(("sc_counts", np.array(gate)))
        return np.tile(np.array([0, 0, 0, count], dtype=np.int64), (len(f), 1)), np.zeros(len(f), dtype=np.int64)

    def approx_counts(self, gate, f, first, count):
        self.calls.append(("approx_counts", np.array(gate)))
        return np.tile(np.array([0, 0, 0, count], dtype=np.int64), (len(f), 1)), np.zeros(len(f), dtype=np.int64)


def test_dispatch_reaches_sc_decompose_for_the_gates_between_the_named_classes(monkeypatch):
    from slam_decomposition_amd import analytic, runtime
    from slam_decomposition_amd.gates import BerkeleyGate, CanonicalGate, CXGate, ConversionGainGate, UnitaryGate, iSwapGate

    calls, made = [], []
    monkeypatch.setattr(runtime, "get_context", lambda device=0: made.append(device) or _RecordingCtx(calls))
    T = np.stack([np.eye(4, dtype=np.complex128)] * 3)
    rng = np.random.default_rng(8)
    between = [_cg_gate(), CanonicalGate(np.pi / 4, 0.15 * np.pi, 0.0), UnitaryGate(sr.dress(rng, sr.can((0.5, 1e-3, 0.0))))]
    for gate in between:
        for res in (analytic.decompose(T, gate), analytic.approx_decompose(T, gate, 0.99), analytic.sc_decompose(T, gate, 0.99)):
            assert calls[-1][0] == "sc" and np.array_equal(calls[-1][1], gate.to_matrix()), gate
            assert type(res) is analytic.ApproxDecomposition and res.basis_gate is gate and len(res) == 3
            assert [e.cycles for e in res.entries()] == [3, 3, 3] and len(res.entries()[0].Xk) == 24
        assert analytic.decompose(T, gate).basis_fidelity == 1.0
        assert list(analytic.approx_decompose(T, gate, 0.9, cycles=1).cycles) == [1, 1, 1]
        sw = analytic.fidelity_sweep(T, gate, [0.99, 0.9])
        assert calls[-1][0] == "sc_counts" and sw.n_targets == 3 and list(sw.average_gates) == [3.0, 3.0]
    # the B point of the conversion-gain family is of a named class: not here
    b_point = ConversionGainGate(0.0, 0.0, 3 * np.pi / 8, np.pi / 8, 1.0)
    for gate in (CXGate(), iSwapGate(), BerkeleyGate(), b_point):
        analytic.approx_decompose(T, gate, 0.99)
        assert calls[-1][0] == "approx", gate
        analytic.fidelity_sweep(T, gate, [0.99])
        assert calls[-1][0] == "approx_counts", gate
    for gate in (CXGate(), iSwapGate()):
        analytic.decompose(T, gate)
        assert calls[-1][0] == "cx", gate
    n_calls = len(calls)
    for gate in (BerkeleyGate(), b_point):
        with pytest.raises(NotImplementedError, match="b_decompose"):
            analytic.decompose(T, gate)
    assert len(calls) == n_calls
    # by name every gate of the line is taken, the named classes included
    for gate in (CXGate(), iSwapGate(), BerkeleyGate()):
        analytic.sc_decompose(T, gate)
        assert calls[-1][0] == "sc", gate
    empty = analytic.sc_decompose(np.zeros((0, 4, 4)), between[0])
    assert len(empty) == 0 and empty.Xk.shape == (0, 24) and empty.entries() == []


def test_gates_off_the_line_are_refused_before_any_context_is_made(monkeypatch):
    from slam_decomposition_amd import analytic, runtime
    from slam_decomposition_amd.gates import RiSwapGate, SwapGate, UnitaryGate

    made = []
    monkeypatch.setattr(runtime, "get_context", lambda device=0: made.append(device))
    T = np.stack([np.eye(4, dtype=np.complex128)] * 3)
    sqiswap = RiSwapGate(1 / 2)  # has a decomposer of its own: ``decompose`` takes it
    for gate in (SwapGate(), RiSwapGate(1 / 3), sqiswap, UnitaryGate(np.eye(4)), UnitaryGate(sr.can((0.5 - 1e-6, 0.3, 0.0)))):
        with pytest.raises(ValueError, match="Weyl coordinates"):
            analytic.sc_decompose(T, gate)
        with pytest.raises(NotImplementedError, match="Weyl coordinates") as e:
            analytic.approx_decompose(T, gate)
        assert "supercontrolled" in str(e.value) and "no closed form" in str(e.value)
        with pytest.raises(NotImplementedError, match="Weyl coordinates"):
            analytic.fidelity_sweep(T, gate, [0.99])
        if gate is not sqiswap:
            with pytest.raises(NotImplementedError, match="supercontrolled"):
                analytic.decompose(T, gate)
    for bad in (0.0, 1.5, float("nan")):
        with pytest.raises(ValueError, match="basis_fidelity"):
            analytic.sc_decompose(T, _cg_gate(), bad)
    for bad in (-1, 4, 1.5):
        with pytest.raises(ValueError, match="cycles"):
            analytic.sc_decompose(T, _cg_gate(), 0.99, cycles=bad)
    assert not made
