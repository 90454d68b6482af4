"""CPU: the yardstick of the closed-form CNOT- / iSWAP-class decomposition -- tests/cx_ref.py, the NumPy restatement the GPU tests
compare ``slam_cx_decompose`` with -- does what it says, and the host side of the feature: the dispatch of ``analytic.decompose``, the
binding, the exported symbol and the host's reduction of the basis gate against the library's own check of it.

Bounds: the class identities to 1e-13 on Makhlin's invariants (measured 3e-15); circuits equal their targets up to a phase within
4 x kak_ref.tolerance(e_ref) at matrix level (one alignment, as tests/test_gpu_complete_locals.py allows it; e_ref the LAPACK residual
over the same targets) and with BasicCost <= 1e-13; for the named cases, whose gap may be the size rule's tolerance, the matrix bound is
4 x kak_ref.tolerance(0) + 1.5 pi gap (a coordinate off by g moves the matrix by at most 1.5 pi g).  Measured: 4096 Haar targets over the
five basis gates, worst matrix error 1.7e-15 (tolerance 4e-13), worst loss 8.9e-16, worst gap 3.3e-16; named cases: loss <= 1.1e-15,
gap = 1e-9 + rounding where c3 = 1e-9, rounding elsewhere.
"""
import ctypes

import numpy as np
import pytest

import cx_ref as cr
import kak_ref as kr
from slam_decomposition_amd import weyl

GATES = cr.basis_gates(np.random.default_rng(20))


def _invariants(U):
    return np.array(weyl.g1g2g3(U))


def test_class_identities_on_random_angles():
    rng = np.random.default_rng(1)
    worst = 0.0
    for _ in range(200):
        t = rng.uniform(-2 * np.pi, 2 * np.pi, 3)
        worst = max(worst, np.abs(_invariants(cr.V3(t)) - _invariants(cr.can(0.5 + t / np.pi))).max())
        worst = max(worst, np.abs(_invariants(cr.V2(t[0], t[1])) - _invariants(cr.can((t[0] / np.pi, t[1] / np.pi, 0.0)))).max())
    print(f"CX host identities: worst invariant difference {worst:.3g}")
    assert worst <= 1e-13


def test_swap_rewriting_on_random_locals():
    """sw(a (x) b) = b (x) a; SWAP commutes with CAN gates; and the three rewritings of the module docstring, with random local layers
    and a dressed gate of the iSWAP class (which does NOT commute with SWAP)."""
    rng = np.random.default_rng(2)
    G = cr.dress(rng, cr.ISWAP)
    D = cr.SWAP @ G
    M, N, gap = cr.align(G, cr.sw(G))
    assert gap <= 1e-14 and cr.up_to_phase(cr.sw(G), M @ G @ N) <= 1e-14
    assert np.max(np.abs(cr.SWAP @ cr.ISWAP - cr.ISWAP @ cr.SWAP)) == 0.0 and np.max(np.abs(cr.SWAP @ G - G @ cr.SWAP)) > 1e-2
    for _ in range(20):
        a, b = kr.random_su2(rng), kr.random_su2(rng)
        assert np.max(np.abs(cr.sw(np.kron(a, b)) - np.kron(b, a))) <= 1e-15
        K = [np.kron(kr.random_su2(rng), kr.random_su2(rng)) for _ in range(4)]
        T3 = cr.SWAP @ (K[3] @ D @ K[2] @ D @ K[1] @ D @ K[0])
        assert cr.up_to_phase(T3, cr.sw(K[3]) @ G @ K[2] @ M @ G @ N @ cr.sw(K[1]) @ G @ K[0]) <= 1e-14
        T2 = K[2] @ D @ K[1] @ D @ K[0]
        assert cr.up_to_phase(T2, K[2] @ M @ G @ N @ cr.sw(K[1]) @ G @ K[0]) <= 1e-14
        T1 = cr.SWAP @ (K[1] @ D @ K[0])
        assert cr.up_to_phase(T1, cr.sw(K[1]) @ G @ K[0]) <= 1e-14


def test_haar_circuits_equal_their_targets():
    from slam_decomposition_amd.sampler import HaarBatch

    n = 4096
    T = HaarBatch(seed0=9100, n_samples=n).as_array()
    rng = np.random.default_rng(7)
    tol = 4 * kr.tolerance(max(kr.lapack_residual(t, rng) for t in T))
    err, loss, gap = np.zeros(n), np.zeros(n), np.zeros(n)
    for j, (name, G) in enumerate(GATES):  # a fifth of the targets per basis gate
        for i in range(j, n, len(GATES)):
            k, x, W, gap[i] = cr.decompose(T[i], G)
            assert k == 3 and len(x) == 24
            err[i], loss[i] = cr.up_to_phase(T[i], W), cr.loss(T[i], W)
    print(f"CX host haar: worst |T - e^(ig) W| {err.max():.3g} (tol {tol:.3g}) worst loss {loss.max():.3g} worst gap {gap.max():.3g}")
    assert err.max() <= tol
    assert loss.max() <= 1e-13
    assert gap.max() <= 1e-12


@pytest.mark.parametrize("gname,G", GATES, ids=[n for n, _ in GATES])
def test_named_circuits_equal_their_targets(gname, G):
    rng = np.random.default_rng(5)
    fam = cr.family_of(G)
    for name, gate in cr.NAMED:
        for _ in range(2):
            t = cr.dress(rng, gate)
            k, x, W, gap = cr.decompose(t, G)
            assert len(x) == 6 * (k + 1) and np.all(np.isfinite(x))
            assert cr.loss(t, W) <= 1e-13, (name, cr.loss(t, W))
            assert gap <= 1e-7
            # up to a phase at matrix level: what the gap leaves (|dU| <= 1.5 pi gap) on top of the rounding
            assert cr.up_to_phase(t, W) <= 4 * kr.tolerance(0.0) + 1.5 * np.pi * gap, (name, cr.up_to_phase(t, W), gap)
            if name not in cr.ON_BOUNDARY:
                assert k == cr.expected_size(t[None], fam)[0], (name, k)
            if name in cr.TWO_GATES:
                assert k == 2
            if name in cr.THREE_GATES:
                assert k == 3


def test_decompose_dispatches_before_any_context(monkeypatch):
    from slam_decomposition_amd import analytic, runtime
    from slam_decomposition_amd.gates import (BerkeleyGate, CanonicalGate, ConversionGainGate, CXGate, CZGate, RiSwapGate, SwapGate, UnitaryGate,
                                              iSwapGate)

    calls = []

    class FakeCtx:
        n_targets = 0

        def set_targets(self, T):
            self.n_targets = len(T)

        def sqiswap_decompose(self, first, count):
            calls.append(("sqiswap", None))
            return np.zeros((count, 24)), np.full(count, 2, dtype=np.int32), np.zeros(count), np.zeros(count)

        def cx_decompose(self, gate, first, count):
            calls.append(("cx", np.array(gate)))
            return np.zeros((count, 24)), np.full(count, 3, dtype=np.int32), np.zeros(count), np.zeros(count)

    made = []
    monkeypatch.setattr(runtime, "get_context", lambda device=0: made.append(device) or FakeCtx())
    T = np.stack([np.eye(4, dtype=np.complex128)] * 3)
    rng = np.random.default_rng(3)
    res = analytic.decompose(T, RiSwapGate(1 / 2))
    assert calls[-1][0] == "sqiswap" and type(res) is analytic.SqiswapDecomposition and len(res) == 3
    cx_like = [CXGate(), CZGate(), iSwapGate(), CanonicalGate(np.pi / 4, 0, 0), CanonicalGate(np.pi / 4, np.pi / 4, 0),
               UnitaryGate(cr.dress(rng, cr.CX12)), UnitaryGate(cr.dress(rng, cr.ISWAP)),
               ConversionGainGate(0.0, 0.0, np.pi / 2, 0.0, 1.0), ConversionGainGate(0.0, 0.0, np.pi / 4, np.pi / 4, 1.0)]
    for gate in cx_like:
        res = analytic.decompose(T, gate)
        assert calls[-1][0] == "cx" and np.array_equal(calls[-1][1], gate.to_matrix()), gate
        assert isinstance(res, analytic.CxDecomposition) and isinstance(res, analytic.SqiswapDecomposition) and res.basis_gate is gate
        assert [e.cycles for e in res.entries()] == [3, 3, 3] and len(res.entries()[0].Xk) == 24
    assert analytic.cx_decompose(T).basis_gate.name == "cx"  # the default basis gate
    n_made = len(made)
    for gate in (BerkeleyGate(), SwapGate(), RiSwapGate(1 / 3), UnitaryGate(np.eye(4))):
        with pytest.raises(NotImplementedError, match="Weyl coordinates"):
            analytic.decompose(T, gate)
        with pytest.raises(ValueError, match="Weyl coordinates"):
            analytic.cx_decompose(T, gate)
    assert len(made) == n_made  # refused before any context was made
    empty = analytic.cx_decompose(np.zeros((0, 4, 4)), CZGate())
    assert len(empty) == 0 and empty.Xk.shape == (0, 24) and empty.entries() == []


def test_conversion_gain_points_are_of_the_classes():
    """The two ConversionGainGate points the dispatch test uses: conversion alone at pi/2 is of the iSWAP class, conversion and gain at
    pi/4 each of the CNOT class."""
    from slam_decomposition_amd import _ffi
    from slam_decomposition_amd.gates import ConversionGainGate

    assert _ffi.cx_family(ConversionGainGate(0.0, 0.0, np.pi / 2, 0.0, 1.0).to_matrix()) == 1
    assert _ffi.cx_family(ConversionGainGate(0.0, 0.0, np.pi / 4, np.pi / 4, 1.0).to_matrix()) == 0


def test_symbol_is_declared_and_exported():
    from slam_decomposition_amd import _ffi

    assert "slam_cx_decompose" in _ffi.EXPORTED_SYMBOLS
    lib = _ffi.load_library()
    assert hasattr(lib, "slam_cx_decompose") and lib.slam_cx_decompose.restype is ctypes.c_int
    assert lib.slam_abi_version() == 7
    assert hasattr(_ffi.Context, "cx_decompose")


@pytest.mark.parametrize("gname,G", GATES, ids=[n for n, _ in GATES])
def test_the_library_accepts_the_host_reduction(gname, G):
    """``_ffi.cx_dress`` against the library's own check of it, which runs before a context is needed: with a NULL context a good
    reduction gets as far as "ctx is NULL", a wrong family, a gate that is not the reduced one and a perturbed factor do not."""
    from slam_decomposition_amd import _ffi

    lib = _ffi.load_library()
    family, g, dress = _ffi.cx_dress(G)
    assert family == cr.family_of(G) and dress.shape == (_ffi.CX_DRESS,)

    def call(fam, gate, d):
        rc = lib.slam_cx_decompose(None, 0, 1, fam, _ffi._ptr(np.ascontiguousarray(gate)), _ffi._ptr(np.ascontiguousarray(d)), None, None, None, None)
        return rc, lib.slam_last_error().decode()

    rc, msg = call(family, g, dress)
    assert rc != 0 and "ctx is NULL" in msg, msg
    rc, msg = call(2, g, dress)
    assert rc != 0 and "family" in msg
    rc, msg = call(1 - family, g, dress)
    assert rc != 0 and "coordinates" in msg
    rc, msg = call(family, cr.dress(np.random.default_rng(1), g), dress)
    assert rc != 0 and "rebuild the gate" in msg
    for at, what in ((5, "rebuild the gate"), (8 * 5 + 1, "CX12"), (8 * 10 + 6, "CX21")):
        bad = dress.copy()
        bad[at] += 1e-9
        rc, msg = call(family, g, bad)
        assert rc != 0 and what in msg, (at, msg)
