"""CPU: the yardstick of the closed-form B-class decomposition -- tests/b_ref.py, the NumPy restatement the GPU tests compare
``slam_b_decompose`` with -- does what it says, and the host side of the feature: ``_ffi.b_class``, the binding, the exported symbol, the
host's reduction of the basis gate against the library's own check of it, and ``analytic.b_decompose`` in front of a fake context.

Bounds: the class identity  B (RY(pi c3) (x) RZ(bz) RY(by) RZ(bz)) B ~ CAN(c)  to 1e-13 on Makhlin's invariants (measured 2.7e-15 over
2000 random chamber points, 8.9e-16 over the named points); circuits equal their targets up to a phase within 4 x kak_ref.tolerance(e_ref)
at matrix level (one alignment, as tests/test_gpu_complete_locals.py allows it; e_ref the LAPACK residual over the same targets) and with
BasicCost <= 1e-13; for the named cases, whose gap may be the size rule's tolerance, the matrix bound is 4 x kak_ref.tolerance(0) +
1.5 pi gap (a coordinate off by g moves the matrix by at most 1.5 pi g).  Measured: 4096 Haar targets over the four basis gates, worst
matrix error 1.1e-15 (tolerance 4e-13), worst loss 8.9e-16, worst gap 6.4e-16; named cases: gap = 1e-9 + rounding at CAN(0.5, 0.25, 1e-9)
(one gate inside the size tolerance), rounding elsewhere.
"""
import ctypes

import numpy as np
import pytest

import b_ref as br
import kak_ref as kr
from slam_decomposition_amd import weyl

GATES = br.basis_gates(np.random.default_rng(20))


def _invariants(U):
    return np.array(weyl.g1g2g3(U))


def _circuit(c):
    q1, q0 = br.interior(c)
    return br.B @ np.kron(q1, q0) @ br.B


def test_class_identity_on_random_chamber_points():
    """In the project's conventions (``gates.canonical_matrix``, units of pi), both signs of c3."""
    from slam_decomposition_amd.gates import canonical_matrix

    rng = np.random.default_rng(1)
    worst = 0.0
    for _ in range(2000):
        c = -np.sort(-rng.uniform(0.0, 0.5, 3))
        c[2] *= rng.choice([-1.0, 1.0])
        worst = max(worst, np.abs(_invariants(_circuit(c)) - _invariants(canonical_matrix(*c))).max())
    assert np.max(np.abs(canonical_matrix(0.3, 0.2, -0.1) - br.can((0.3, 0.2, -0.1)))) <= 1e-15
    print(f"B host identity: worst invariant difference over random points {worst:.3g}")
    assert worst <= 1e-13


def test_class_identity_on_the_named_points():
    """... and that the sign of c3 matters: the mirror class is another one."""
    worst = 0.0
    for name, gate in br.NAMED:
        c = br.fold(np.array(weyl.kak(gate)[3]))
        assert 0.5 >= c[0] >= c[1] >= abs(c[2]) - 1e-15, (name, c)
        worst = max(worst, np.abs(_invariants(_circuit(c)) - _invariants(gate)).max())
    print(f"B host identity: worst invariant difference over the named points {worst:.3g}")
    assert worst <= 1e-13
    c = np.array([0.3, 0.2, 0.1])
    assert np.abs(_invariants(_circuit(c * [1, 1, -1])) - _invariants(br.can(c))).max() > 1e-2
    # the singular face: bz moves by the square root of the distance, the class by the distance
    by0, bz0 = br.angles(np.array([0.5, 0.3, 0.1]))
    by1, bz1 = br.angles(np.array([0.5 - 1e-12, 0.3, 0.1]))
    assert bz0 == 0.0 and 1e-7 < bz1 < 1e-5
    assert br.angles(np.array([0.5, 0.0, 0.0])) == (np.pi, 0.0)  # the CNOT point: atan2(0, 0)


def test_haar_circuits_equal_their_targets():
    from slam_decomposition_amd.sampler import HaarBatch

    n = 4096
    T = HaarBatch(seed0=9100, n_samples=n).as_array()
    rng = np.random.default_rng(7)
    tol = 4 * kr.tolerance(max(kr.lapack_residual(t, rng) for t in T))
    err, loss, gap = np.zeros(n), np.zeros(n), np.zeros(n)
    for j, (name, G) in enumerate(GATES):  # a quarter of the targets per basis gate
        for i in range(j, n, len(GATES)):
            x, k, loss[i], gap[i] = br.decompose(T[i], G)
            assert k == 2 and len(x) == 18
            err[i] = br.up_to_phase(T[i], br.template(x, G, k))
    print(f"B host haar: worst |T - e^(ig) W| {err.max():.3g} (tol {tol:.3g}) worst loss {loss.max():.3g} worst gap {gap.max():.3g}")
    assert err.max() <= tol
    assert loss.max() <= 1e-13
    assert gap.max() <= 1e-12


@pytest.mark.parametrize("gname,G", GATES, ids=[n for n, _ in GATES])
def test_named_circuits_equal_their_targets(gname, G):
    rng = np.random.default_rng(5)
    for name, gate in br.NAMED:
        for _ in range(2):
            t = br.dress(rng, gate)
            x, k, loss, gap = br.decompose(t, G)
            assert len(x) == 6 * (k + 1) and np.all(np.isfinite(x))
            assert loss <= 1e-13, (name, loss)
            assert gap <= 1e-7
            assert loss <= 11.2 * gap ** 2 + 1e-14
            # up to a phase at matrix level: what the gap leaves (|dU| <= 1.5 pi gap) on top of the rounding
            err = br.up_to_phase(t, br.template(x, G, k))
            assert err <= 4 * kr.tolerance(0.0) + 1.5 * np.pi * gap, (name, err, gap)
            if name not in br.ON_BOUNDARY:
                assert k == br.expected_size(t[None])[0], (name, k)
            assert k == (1 if name in br.ONE_GATE else 2) or name in br.ON_BOUNDARY


def test_b_class_accepts_the_class_and_refuses_the_rest():
    from slam_decomposition_amd import _ffi
    from slam_decomposition_amd.gates import (BerkeleyGate, CanonicalGate, CXGate, RiSwapGate, SwapGate, UnitaryGate, gate_matrix,
                                              iSwapGate)

    rng = np.random.default_rng(4)
    for gate in (BerkeleyGate(), UnitaryGate(br.dress(rng, br.B)), CanonicalGate(np.pi / 4, np.pi / 8, 0.0)):
        assert _ffi.b_class(gate_matrix(gate)) is None
    assert _ffi.b_class(br.can((0.5, 0.25, 1e-9))) is None
    for gate in (CXGate(), iSwapGate(), SwapGate(), RiSwapGate(1 / 2), UnitaryGate(np.eye(4))):
        with pytest.raises(ValueError, match="Weyl coordinates"):
            _ffi.b_class(gate_matrix(gate))
        with pytest.raises(ValueError, match="Weyl coordinates"):
            _ffi.b_dress(gate_matrix(gate))


def test_conversion_gain_point_is_of_the_class():
    """``ConversionGainGate(0, 0, gc, gg, 1)`` has the coordinates (gc + gg, gc - gg, 0) / pi (conversion alone at pi/2 is iSWAP,
    pi/4 each is CNOT: tests/test_cx_analytic_host.py), so the B point is gc = 3 pi / 8, gg = pi / 8."""
    from slam_decomposition_amd import _ffi
    from slam_decomposition_amd.gates import ConversionGainGate

    assert _ffi.b_class(ConversionGainGate(0.0, 0.0, 3 * np.pi / 8, np.pi / 8, 1.0).to_matrix()) is None
    with pytest.raises(ValueError, match="Weyl coordinates"):
        _ffi.b_class(ConversionGainGate(0.0, 0.0, 3 * np.pi / 16, np.pi / 16, 1.0).to_matrix())


def test_symbol_is_declared_and_exported():
    from slam_decomposition_amd import _ffi

    assert "slam_b_decompose" in _ffi.EXPORTED_SYMBOLS
    lib = _ffi.load_library()
    assert hasattr(lib, "slam_b_decompose") and lib.slam_b_decompose.restype is ctypes.c_int
    assert len(lib.slam_b_decompose.argtypes) == 9
    assert lib.slam_abi_version() == 7
    assert hasattr(_ffi.Context, "b_decompose")  # (that include/slam_hip.h declares the symbol: tests/test_abi.py)


@pytest.mark.parametrize("gname,G", GATES, ids=[n for n, _ in GATES])
def test_the_library_accepts_the_host_reduction(gname, G):
    """``_ffi.b_dress`` against the library's own check of it, which runs before a context is needed: with a NULL context a good
    reduction gets as far as "ctx is NULL"; coordinates of another class, a gate that is not the reduced one and a perturbed factor do
    not."""
    from slam_decomposition_amd import _ffi

    lib = _ffi.load_library()
    g, dress = _ffi.b_dress(G)
    assert dress.shape == (_ffi.B_DRESS,)

    def call(gate, d):
        rc = lib.slam_b_decompose(None, 0, 1, _ffi._ptr(np.ascontiguousarray(gate)), _ffi._ptr(np.ascontiguousarray(d)), None, None, None, None)
        return rc, lib.slam_last_error().decode()

    rc, msg = call(g, dress)
    assert rc != 0 and "ctx is NULL" in msg, msg
    other = dress.copy()
    other[33] = 0.0
    rc, msg = call(g, other)
    assert rc != 0 and "coordinates" in msg
    rc, msg = call(br.dress(np.random.default_rng(1), g), dress)
    assert rc != 0 and "rebuild the gate" in msg
    for at in (5, 8 * 1 + 2, 8 * 2 + 1, 8 * 3 + 6):
        bad = dress.copy()
        bad[at] += 1e-9
        rc, msg = call(g, bad)
        assert rc != 0 and "rebuild the gate" in msg, (at, msg)


def test_b_decompose_goes_through_a_context_and_makes_none_when_it_refuses(monkeypatch):
    from slam_decomposition_amd import analytic, runtime
    from slam_decomposition_amd.gates import BerkeleyGate, CanonicalGate, CXGate, RiSwapGate, SwapGate, UnitaryGate, iSwapGate

    calls = []

    class FakeCtx:
        n_targets = 0

        def set_targets(self, T):
            self.n_targets = len(T)

        def b_decompose(self, gate, first, count):
            calls.append(np.array(gate))
            return np.zeros((count, 24)), np.full(count, 2, dtype=np.int32), np.zeros(count), np.zeros(count)

    made = []
    monkeypatch.setattr(runtime, "get_context", lambda device=0: made.append(device) or FakeCtx())
    T = np.stack([np.eye(4, dtype=np.complex128)] * 3)
    rng = np.random.default_rng(3)
    for gate in (BerkeleyGate(), CanonicalGate(np.pi / 4, np.pi / 8, 0.0), UnitaryGate(br.dress(rng, br.B))):
        res = analytic.b_decompose(T, gate)
        assert np.array_equal(calls[-1], gate.to_matrix()), gate
        assert isinstance(res, analytic.CxDecomposition) and res.basis_gate is gate and len(res) == 3
        assert [e.cycles for e in res.entries()] == [2, 2, 2] and len(res.entries()[0].Xk) == 18
    res = analytic.b_decompose(list(T), br.B)  # a list of targets, a plain matrix for the gate
    assert np.array_equal(calls[-1], br.B) and len(res) == 3
    assert analytic.b_decompose(T).basis_gate.name == BerkeleyGate().name  # the default basis gate
    n_made, n_calls = len(made), len(calls)
    for gate in (CXGate(), iSwapGate(), SwapGate(), RiSwapGate(1 / 2), UnitaryGate(np.eye(4))):
        with pytest.raises(ValueError, match="Weyl coordinates"):
            analytic.b_decompose(T, gate)
    assert len(made) == n_made and len(calls) == n_calls  # refused before any context was made
    empty = analytic.b_decompose(np.zeros((0, 4, 4)), BerkeleyGate())
    assert len(empty) == 0 and empty.Xk.shape == (0, 24) and empty.entries() == [] and len(calls) == n_calls


def test_decompose_still_refuses_the_class_and_names_b_decompose(monkeypatch):
    from slam_decomposition_amd import analytic, runtime
    from slam_decomposition_amd.gates import BerkeleyGate, UnitaryGate

    made = []
    monkeypatch.setattr(runtime, "get_context", lambda device=0: made.append(device))
    T = np.stack([np.eye(4, dtype=np.complex128)] * 3)
    for gate in (BerkeleyGate(), UnitaryGate(br.dress(np.random.default_rng(6), br.B))):
        with pytest.raises(NotImplementedError, match="Weyl coordinates") as e:
            analytic.decompose(T, gate)
        assert "b_decompose" in str(e.value)
    assert not made
