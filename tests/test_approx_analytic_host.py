"""CPU: the yardstick of the fidelity-aware approximate decomposition -- tests/approx_ref.py, the NumPy model the GPU tests compare
``slam_approx_decompose`` and ``slam_approx_counts`` with -- against an optimiser that knows nothing of it, the selection facts the
model gives, and the host side of the feature: the refusals of ``analytic.approx_decompose`` / ``analytic.fidelity_sweep`` before any
context exists and those of the two C entry points with a NULL context.

Bounds: |best BFGS loss - L_k| <= 3e-8 = 3 (pi/2) 5e-9, the effect of rounding three coordinates to 8 digits on a loss whose
derivative in a coordinate is at most pi/2 (measured: 4.4e-9 over the 72 cases).  The selection counts are exact.
"""
import ctypes

import numpy as np
import pytest

import approx_ref as ar
from oracle import slam_oracle as o

GATES = [("CX", 0, ar.CX), ("iSWAP", 1, ar.ISWAP), ("B", 2, o.canonical_matrix(0.5, 0.25, 0.0))]


@pytest.fixture(scope="module")
def batch_coordinates():
    return ar.coordinates(o.haar_batch(4096, seed0=91000))


@pytest.mark.parametrize("gname,family,G", GATES, ids=[g[0] for g in GATES])
def test_model_against_an_independent_optimum(gname, family, G):
    """10-restart SciPy BFGS on the oracle's BasicCost for the best circuit of k = 0, 1, 2 gates, seeds fixed."""
    from scipy.optimize import minimize

    worst = 0.0
    for s in range(7000, 7008):
        T = o.haar_unitary(s)
        c = ar.coordinates(T[None])
        for k in (0, 1, 2):
            rng = np.random.default_rng(1000 * s + 10 * k + family)
            best = np.inf
            for _ in range(10):
                x0 = rng.uniform(-np.pi, np.pi, 6 * (k + 1))
                r = minimize(o.loss_and_grad, x0, args=([G] * k, T), jac=True, method="BFGS", options={"gtol": 1e-10, "maxiter": 2000})
                best = min(best, float(r.fun))
            d = abs(best - float(ar.predicted_loss(c, family, k)[0]))
            worst = max(worst, d)
            assert d <= 3e-8, (gname, s, k, best, float(ar.predicted_loss(c, family, k)[0]))
    print(f"APPROX host {gname}: worst |BFGS - L_k| over 8 targets and k = 0, 1, 2: {worst:.3g}")


def test_selection_on_the_haar_batch(batch_coordinates):
    c = batch_coordinates
    assert np.bincount(ar.select(c, 0, 1.0), minlength=4).tolist() == [0, 0, 0, 4096]
    assert np.bincount(ar.select(c, 0, 0.9), minlength=4).tolist() == [92, 1137, 2780, 87]
    assert np.bincount(ar.select(c, 0, 0.6), minlength=4).tolist() == [4096, 0, 0, 0]
    assert np.bincount(ar.select(c, 2, 0.97), minlength=3).tolist() == [0, 1409, 2687]
    # no target of the batch is a tie within rounding at the fidelities the GPU tests use
    for f in (1.0, 0.999, 0.99, 0.97, 0.9, 0.8, 0.6):
        for family in range(3):
            assert int(np.sum(ar.tie_margin(c, family, f) < 1e-9)) == 0, (f, family)


def test_selection_of_named_targets():
    named = dict(ar.named_targets(np.random.default_rng(2)))
    for f in (1.0, 0.99, 0.5, 1e-3):
        for family in range(3):
            assert ar.select(ar.coordinates(named["identity"][None]), family, f)[0] == 0
            assert ar.select(ar.coordinates(named["local"][None]), family, f)[0] == 0
    assert ar.select(ar.coordinates(named["CX"][None]), 0, 1.0)[0] == 1
    assert ar.select(ar.coordinates(named["CZ"][None]), 0, 1.0)[0] == 1
    assert ar.select(ar.coordinates(named["iSWAP"][None]), 1, 1.0)[0] == 1
    assert ar.select(ar.coordinates(named["B"][None]), 2, 1.0)[0] == 1
    assert ar.select(ar.coordinates(named["CAN(0.3, 0.1, 0)"][None]), 0, 1.0)[0] == 2
    assert ar.select(ar.coordinates(named["SWAP"][None]), 0, 1.0)[0] == 3
    assert ar.select(ar.coordinates(named["SWAP"][None]), 1, 1.0)[0] == 3
    assert ar.select(ar.coordinates(named["SWAP"][None]), 2, 1.0)[0] == 2


def test_row_helper_multiplies_rows_out():
    rng = np.random.default_rng(5)
    x = rng.uniform(-np.pi, np.pi, 24)
    assert np.array_equal(ar.row_matrix(x, ar.CX, 0), o.layer_matrix(x[:6]))
    assert np.array_equal(ar.row_matrix(x, ar.CX, 2), o.template_eval(x[:18], [ar.CX, ar.CX]))
    # the batched form against the oracle's, row by row
    X = rng.uniform(-np.pi, np.pi, (5, 24))
    T = o.haar_batch(5, seed0=300)
    for k in range(4):
        one = np.array([ar.row_loss(X[i], ar.ISWAP, k, T[i]) for i in range(5)])
        assert np.max(np.abs(ar.rows_losses(X, ar.ISWAP, k, T) - one)) <= 1e-15


def test_public_functions_refuse_before_any_context(monkeypatch):
    from slam_decomposition_amd import analytic, runtime
    from slam_decomposition_amd.gates import BerkeleyGate, CXGate, RiSwapGate, SwapGate, UnitaryGate, iSwapGate

    made = []
    monkeypatch.setattr(runtime, "get_context", lambda device=0: made.append(device))
    T = np.stack([np.eye(4, dtype=np.complex128)] * 3)
    for f in (0.0, -0.1, 1.0 + 1e-12, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="basis_fidelity"):
            analytic.approx_decompose(T, CXGate(), basis_fidelity=f)
        with pytest.raises(ValueError, match="basis_fidelity"):
            analytic.fidelity_sweep(T, CXGate(), [0.9, f])
    for gate, bad in ((BerkeleyGate(), 3), (CXGate(), 4), (iSwapGate(), -1), (CXGate(), 1.5)):
        with pytest.raises(ValueError, match="cycles"):
            analytic.approx_decompose(T, gate, cycles=bad)
    with pytest.raises(ValueError):
        analytic.fidelity_sweep(T, CXGate(), [])
    with pytest.raises(ValueError):
        analytic.fidelity_sweep(T, CXGate(), np.linspace(0.5, 1.0, 65))
    with pytest.raises(NotImplementedError, match="Weyl coordinates") as e:
        analytic.approx_decompose(T, RiSwapGate(1 / 2))
    assert "0.25" in str(e.value) and "sqrt(iSWAP)" in str(e.value) and "no closed form" in str(e.value)
    for gate in (SwapGate(), RiSwapGate(1 / 3), UnitaryGate(np.eye(4))):
        with pytest.raises(NotImplementedError, match="Weyl coordinates"):
            analytic.approx_decompose(T, gate)
        with pytest.raises(NotImplementedError, match="Weyl coordinates"):
            analytic.fidelity_sweep(T, gate, [0.99])
    assert not made


def test_public_functions_go_through_a_context(monkeypatch):
    from slam_decomposition_amd import analytic, runtime
    from slam_decomposition_amd.gates import BerkeleyGate, CXGate

    calls = []

    class FakeCtx:
        n_targets = 0

        def set_targets(self, T):
            self.n_targets = len(T)

        def approx_decompose(self, gate, f, cycles, first, count):
            calls.append(("decompose", f, cycles))
            k = np.array([0, 1, 2][:count], dtype=np.int32)
            return np.zeros((count, 24)), k, np.array([0.0, 0.1, 0.0])[:count], np.array([0.0, 0.1, 0.0])[:count], np.zeros(count)

        def approx_counts(self, gate, f, first, count):
            calls.append(("counts", np.array(f)))
            return np.tile(np.array([[1, 1, 1, 0]], dtype=np.int64), (len(f), 1)), np.full(len(f), 3 << 31, dtype=np.int64)

    monkeypatch.setattr(runtime, "get_context", lambda device=0: FakeCtx())
    T = np.stack([np.eye(4, dtype=np.complex128)] * 3)
    res = analytic.approx_decompose(T, BerkeleyGate(), basis_fidelity=0.5, cycles=2)
    assert calls[-1] == ("decompose", 0.5, 2)
    assert isinstance(res, analytic.ApproxDecomposition) and isinstance(res, analytic.CxDecomposition) and res.basis_fidelity == 0.5
    assert np.allclose(res.expected_fidelity, [1.0, (4 + 16 * 0.81) / 20 * 0.5, 0.25], rtol=0, atol=1e-15)
    assert np.array_equal(res.predicted_loss, [0.0, 0.1, 0.0])
    e = res.entries()
    assert [len(v.Xk) for v in e] == [6, 12, 18] and [v.cycles for v in e] == [0, 1, 2]
    assert analytic.approx_decompose(T).basis_gate.name == CXGate().name and calls[-1] == ("decompose", 1.0, None)
    empty = analytic.approx_decompose(np.zeros((0, 4, 4)), CXGate(), 0.9)
    assert len(empty) == 0 and empty.Xk.shape == (0, 24) and empty.entries() == [] and len(empty.predicted_loss) == 0
    sw = analytic.fidelity_sweep(T, CXGate(), [0.9, 1.0])
    assert calls[-1][0] == "counts" and calls[-1][1].tolist() == [0.9, 1.0]
    assert sw.counts.shape == (2, 4) and sw.average_gates.tolist() == [1.0, 1.0] and sw.average_fidelity.tolist() == [0.5, 0.5]
    assert sw.n_targets == 3


def test_symbols_are_declared_and_exported():
    from slam_decomposition_amd import _ffi

    lib = _ffi.load_library()
    for name, n_args in (("slam_approx_decompose", 13), ("slam_approx_counts", 8)):
        assert name in _ffi.EXPORTED_SYMBOLS
        fn = getattr(lib, name)
        assert fn.restype is ctypes.c_int and len(fn.argtypes) == n_args
    assert lib.slam_abi_version() == 7
    assert hasattr(_ffi.Context, "approx_decompose") and hasattr(_ffi.Context, "approx_counts")


@pytest.mark.parametrize("gname,family,G", GATES, ids=[g[0] for g in GATES])
def test_c_abi_refusals_with_a_null_context(gname, family, G):
    """What needs no context is checked first: with a NULL context good arguments get as far as "ctx is NULL", bad ones do not."""
    from closed_form_ref import dress as dressed
    from slam_decomposition_amd import _ffi

    lib = _ffi.load_library()
    G = dressed(np.random.default_rng(11), G)
    fam, g, dress = _ffi.approx_dress(G)
    assert fam == family and dress.shape == ((_ffi.B_DRESS,) if family == 2 else (_ffi.CX_DRESS,))

    def call(fam=family, gate=g, d=dress, f=0.99, force=-1):
        rc = lib.slam_approx_decompose(None, 0, 1, fam, _ffi._ptr(np.ascontiguousarray(gate)), _ffi._ptr(np.ascontiguousarray(d)), f, force,
                                       None, None, None, None, None)
        return rc, lib.slam_last_error().decode()

    rc, msg = call()
    assert rc == -1 and "ctx is NULL" in msg, msg
    for force in range(0, 3 if family == 2 else 4):
        rc, msg = call(force=force)
        assert rc == -1 and "ctx is NULL" in msg, msg
    for bad in (3, -1):
        rc, msg = call(fam=bad)
        assert rc == -1 and "family" in msg
    bad = dress.copy()
    bad[5] += 1e-9
    rc, msg = call(d=bad)
    assert rc == -1 and "rebuild the gate" in msg  # the dress check runs before the fidelity's
    rc, msg = call(d=bad, f=2.0)
    assert rc == -1 and "rebuild the gate" in msg
    rc, msg = call(gate=dressed(np.random.default_rng(1), g))
    assert rc == -1 and "rebuild the gate" in msg
    for f in (0.0, -0.5, 1.0000001, float("nan"), float("inf")):
        rc, msg = call(f=f)
        assert rc == -1 and "basis_fidelity" in msg, (f, msg)
    for force in (-2, 3 if family == 2 else 4):
        rc, msg = call(force=force)
        assert rc == -1 and "force_cycles" in msg, (force, msg)

    def counts(fam=family, n=2, f=(0.9, 1.0)):
        fa = np.ascontiguousarray(f, dtype=np.float64)
        rc = lib.slam_approx_counts(None, 0, 1, fam, n, _ffi._ptr(fa), None, None)
        return rc, lib.slam_last_error().decode()

    rc, msg = counts()
    assert rc == -1 and "ctx is NULL" in msg, msg
    rc, msg = counts(fam=3)
    assert rc == -1 and "family" in msg
    for n in (0, -1, 65):
        rc, msg = counts(n=n, f=np.full(65, 0.9))
        assert rc == -1 and "n_fid" in msg
    for f in (0.0, 1.5, float("nan")):
        rc, msg = counts(f=(0.9, f))
        assert rc == -1 and "fidelities[1]" in msg
