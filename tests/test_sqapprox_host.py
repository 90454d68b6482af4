"""CPU: the yardstick of the fidelity-aware approximate sqrt(iSWAP) decomposition -- tests/sqapprox_ref.py, the NumPy model the GPU
tests compare ``slam_sqiswap_approx_decompose`` and ``slam_sqiswap_approx_counts`` with -- against optimisers that know nothing of it,
the model's rows multiplied out, and the host side of the feature: the refusals of ``analytic.sqiswap_approx_decompose`` /
``analytic.sqiswap_fidelity_sweep`` before any context exists, their way through a context, and the two C entry points with a NULL
context.

Bounds (set before anything ran):
  * t_2 against SLSQP over the region (linear constraints, ftol 1e-15, 6 starts): the optimiser may not end more than 1e-12 above the
    formula (a better point would refute it; 1e-12 is far above the rounding of ov, 4 ulp) and must come within 1e-9 of it (its own
    termination; the objective is flat to second order at the optimum);
  * the best BFGS loss on the oracle's one- and two-gate templates against L_1, L_2 of 8-digit coordinates: 3e-8 = 3 (pi/2) 5e-9, the
    effect of rounding three coordinates on a loss whose derivative in a coordinate is at most pi/2 -- the siblings' figure;
  * rows multiplied out against 1 - t_k on the row's own unrounded coordinates: 1e-11, a tenth of the project's success threshold.
Measured: SLSQP between -1.1e-16 and +6.7e-16 of the formula; BFGS (12 restarts) within 3.5e-9 (one gate) and 7.4e-10 (two gates) of
the 8-digit model; rows within 7.8e-16 over the whole batch of the GPU tests (4096 Haar targets and the named ones, sizes 0..3; this
file runs 64 of the Haar targets, 24 of them outside the region, and the named ones, within 4.4e-16).
"""
import ctypes

import numpy as np
import pytest

import analytic_ref as an
import sqapprox_ref as sr
from oracle import slam_oracle as o

N_HAAR = 4096
HARD = [("SWAP", (0.5, 0.5, 0.5)), ("CAN(0.5, 0.4, 0.4)", (0.5, 0.4, 0.4)), ("CAN(0.45, 0.45, 0.3)", (0.45, 0.45, 0.3)),
        ("CAN(0.3, 0.3, 0.3)", (0.3, 0.3, 0.3)), ("CAN(0.75, 0.2, 0.15)", (0.75, 0.2, 0.15))]


@pytest.fixture(scope="module")
def batch_coordinates():
    return sr.coordinates(o.haar_batch(N_HAAR, seed0=91000))


def _twelve(c):
    """Twelve targets: the five hard classes, then Haar targets of the batch that need three gates -- three on the ridge, four off it."""
    p, outside, ridge = sr.nearest_two_gate_point(c, c)
    pick = list(np.flatnonzero(ridge)[:3]) + list(np.flatnonzero(outside & ~ridge)[:4])
    T = [an.can(v) for _, v in HARD] + [o.haar_unitary(91000 + int(i)) for i in pick]
    return np.stack(T)


def test_the_batch_is_the_oracles(batch_coordinates):
    assert np.allclose(sr.coordinates(np.stack([o.haar_unitary(91000 + i) for i in (0, 77)])), batch_coordinates[[0, 77]], rtol=0, atol=0)


def test_two_gate_trace_against_a_constrained_maximum(batch_coordinates):
    """max ov(q - c) over the region |q3| <= min(q1, 1 - q1) - q2, q2 >= 0 (the chamber's two-gate region and its mirror images; all
    of it is reached by two gates), by SLSQP from the formula's neighbourhood and from five points of the region."""
    from scipy.optimize import minimize

    T = _twelve(batch_coordinates)
    c = sr.coordinates(T)
    p, outside, ridge = sr.nearest_two_gate_point(c, c)
    assert outside.all() and ridge.sum() >= 4  # SWAP is a ridge case too
    t2 = sr.traces(c, c)[:, 2]
    cons = [{"type": "ineq", "fun": lambda q, s=s, m=m: (q[0] if m == 0 else 1.0 - q[0]) - q[1] - s * q[2]} for s in (1.0, -1.0) for m in (0, 1)]
    cons.append({"type": "ineq", "fun": lambda q: q[1]})
    rng = np.random.default_rng(3)
    lo, hi = 0.0, 0.0
    for i in range(len(T)):
        starts = [np.array([0.25, 0.25, 0.0]), np.array([0.5, 0.0, 0.0]), np.array([0.5, 0.25, 0.25]), np.array([0.25, 0.0, 0.0]),
                  np.array([0.75, 0.1, 0.1]), c[i] * np.array([1.0, 0.5, 0.2]) + rng.uniform(-0.01, 0.01, 3)]
        best = -np.inf
        for q0 in starts:
            r = minimize(lambda q: -float(sr.ov(q - c[i])) ** 2, q0, method="SLSQP", constraints=cons, options={"ftol": 1e-15, "maxiter": 500})
            if r.success and all(con["fun"](r.x) >= -1e-12 for con in cons):
                best = max(best, float(np.sqrt(-r.fun)))
        d = best - t2[i]
        lo, hi = min(lo, d), max(hi, d)
        assert d <= 1e-12, (i, c[i], best, t2[i])      # nothing in the region is closer than the formula's point
        assert d >= -1e-9, (i, c[i], best, t2[i])      # and the optimiser finds it
    assert abs((1.0 - t2[0]) - 0.146446609406726) <= 1e-14  # SWAP: 1 - cos^2(pi/8)
    print(f"SQAPPROX host: SLSQP - t_2 over 12 targets in [{lo:.3g}, {hi:.3g}]")


@pytest.mark.parametrize("k,restarts", [(1, 12), (2, 12)])
def test_model_against_the_oracles_bfgs(batch_coordinates, k, restarts):
    """SciPy BFGS on the oracle's BasicCost of the k-gate template, seeds fixed, the lowest of the restarts."""
    from scipy.optimize import minimize

    T = _twelve(batch_coordinates)
    c = sr.coordinates(T)
    model = sr.predicted_loss(c, k, c)
    worst = 0.0
    for i in range(len(T)):
        rng = np.random.default_rng(500 + 10 * i + k)
        best = np.inf
        for _ in range(restarts):
            x0 = rng.uniform(-np.pi, np.pi, 6 * (k + 1))
            r = minimize(o.loss_and_grad, x0, args=([sr.S] * k, T[i]), jac=True, method="BFGS", options={"gtol": 1e-10, "maxiter": 2000})
            best = min(best, float(r.fun))
        worst = max(worst, abs(best - model[i]))
        assert abs(best - model[i]) <= 3e-8, (k, i, c[i], best, model[i])
    print(f"SQAPPROX host: worst |BFGS - L_{k}| over 12 targets: {worst:.3g}")


def test_selection_on_the_haar_batch(batch_coordinates):
    c = batch_coordinates
    assert int(np.sum(c[:, 0] > 0.5)) > 1000
    p, outside, ridge = sr.nearest_two_gate_point(c, c)
    assert (int(outside.sum()), int(ridge.sum())) == (886, 107)
    assert np.bincount(sr.select(c, 1.0, c), minlength=4).tolist() == [0, 0, 3210, 886]
    assert np.bincount(sr.select(c, 0.99, c), minlength=4).tolist() == [0, 50, 3916, 130]
    assert np.bincount(sr.select(c, 0.9, c), minlength=4).tolist() == [16, 2394, 1686, 0]
    assert np.bincount(sr.select(c, 0.6, c), minlength=4).tolist() == [3565, 531, 0, 0]
    # the sizes of f = 1 are those of sqiswap_decompose
    assert np.array_equal(sr.select(c, 1.0, c), an.size(c))
    # no target of the batch is a tie within rounding at an imperfect fidelity the GPU tests use; at f = 1 the ties are exact
    for f in (0.999, 0.99, 0.97, 0.9, 0.8, 0.6):
        assert int(np.sum(sr.tie_margin(c, f, c) < 1e-9)) == 0, f
    m = sr.tie_margin(c, 1.0, c)
    assert np.all((m == 0.0) | (m >= 1e-9))
    # the nearest point lies on the face of the region, in the chamber, and no farther than the target's own excess
    q = p[outside]
    assert np.abs(np.abs(q[:, 2]) - (q[:, 0] - q[:, 1])).max() <= 1e-15
    assert np.all(q[:, 0] <= 0.5) and np.all(q[:, 1] >= np.abs(q[:, 2]) - 1e-15)


def test_selection_of_named_targets():
    named = dict(sr.named_targets(np.random.default_rng(2)))

    def sel(name, f):
        c = sr.coordinates(named[name][None])
        return int(sr.select(c, f, c)[0])

    for f in (1.0, 0.99, 0.5, 1e-3):
        assert sel("identity", f) == 0 and sel("local", f) == 0
    assert sel("sqrt(iSWAP)", 1.0) == 1 and sel("dressed sqrt(iSWAP)", 1.0) == 1
    assert sel("CX", 1.0) == 2 and sel("iSWAP", 1.0) == 2 and sel("dressed CAN(0.5, 0, 0)", 1.0) == 2
    assert sel("on the face CAN(0.3, 0.2, 0.1)", 1.0) == 2
    assert sel("SWAP", 1.0) == 3 and sel("CAN(0.5, 0.4, 0.4)", 1.0) == 3 and sel("CAN(0.75, 0.2, 0.15)", 1.0) == 3
    assert sel("SWAP", 0.9) == 3 and sel("CAN(0.5, 0.4, 0.4)", 0.9) == 2 and sel("CAN(0.75, 0.2, 0.15)", 0.9) == 1


def test_rows_multiplied_out_give_the_predicted_loss(batch_coordinates):
    named = sr.named_targets(np.random.default_rng(21))
    c = batch_coordinates
    p, outside, ridge = sr.nearest_two_gate_point(c, c)
    pick = list(range(40)) + list(np.flatnonzero(ridge)[:12]) + list(np.flatnonzero(outside & ~ridge)[:12])
    T = [o.haar_unitary(91000 + int(i)) for i in pick] + [m for _, m in named]
    worst = 0.0
    for t in T:
        for k in range(4):
            kk, x, W, predicted, gap = sr.decompose(t, 1.0, k)
            assert kk == k and len(x) == 6 * (k + 1)
            G = o.layer_matrix(x) if k == 0 else o.template_eval(x, [sr.S] * k)  # through the oracle, not the model's own template
            d = abs(o.basic_cost(G, t) - predicted)
            worst = max(worst, d)
            assert d <= 1e-11, (k, sr.coordinates(t[None])[0], d)
        c8 = sr.coordinates(t[None])
        for f in (1.0, 0.99, 0.9):
            kk, x, W, predicted, gap = sr.decompose(t, f)
            if sr.tie_margin(c8, f, c8)[0] >= 1e-9 or f == 1.0:
                assert kk == sr.select(c8, f, c8)[0]
            assert abs(an.loss(t, W) - predicted) <= 1e-11
            if f == 1.0:
                assert predicted == 0.0 and gap <= 1e-7
    print(f"SQAPPROX host: worst |row multiplied out - (1 - t_k)| {worst:.3g}")


def test_public_functions_refuse_before_any_context(monkeypatch):
    from slam_decomposition_amd import analytic, runtime

    made = []
    monkeypatch.setattr(runtime, "get_context", lambda device=0: made.append(device))
    T = np.stack([np.eye(4, dtype=np.complex128)] * 3)
    for f in (0.0, -0.1, 1.0 + 1e-12, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="basis_fidelity"):
            analytic.sqiswap_approx_decompose(T, basis_fidelity=f)
        with pytest.raises(ValueError, match="basis_fidelity"):
            analytic.sqiswap_fidelity_sweep(T, [0.9, f])
    for bad in (4, -1, 1.5, "2"):
        with pytest.raises(ValueError, match="cycles"):
            analytic.sqiswap_approx_decompose(T, cycles=bad)
    with pytest.raises(ValueError, match="basis fidelities"):
        analytic.sqiswap_fidelity_sweep(T, [])
    with pytest.raises(ValueError, match="basis fidelities"):
        analytic.sqiswap_fidelity_sweep(T, np.linspace(0.5, 1.0, 65))
    assert not made
    # the general entry points keep their refusal of the gate, and its wording
    from slam_decomposition_amd.gates import RiSwapGate

    with pytest.raises(NotImplementedError, match="no closed form for the nearest two-gate point of sqrt\\(iSWAP\\)"):
        analytic.approx_decompose(T, RiSwapGate(1 / 2))
    with pytest.raises(NotImplementedError, match="no closed form for the nearest two-gate point of sqrt\\(iSWAP\\)"):
        analytic.fidelity_sweep(T, RiSwapGate(1 / 2), [0.99])
    assert not made


def test_public_functions_go_through_a_context(monkeypatch):
    from slam_decomposition_amd import analytic, runtime
    from slam_decomposition_amd.gates import RiSwapGate, gate_matrix

    calls = []

    class FakeCtx:
        n_targets = 0

        def set_targets(self, T):
            self.n_targets = len(T)
            calls.append(("set_targets", len(T)))

        def sample_haar(self, seed, n_targets, first_index=0):
            self.n_targets = int(n_targets)
            calls.append(("sample_haar", int(seed), int(n_targets)))

        def sqiswap_approx_decompose(self, f, cycles, first, count):
            calls.append(("decompose", f, cycles, first, count))
            k = np.array([0, 1, 2] * count, dtype=np.int32)[:count]
            loss = np.array([0.0, 0.1, 0.0] * count)[:count]
            return np.zeros((count, 24)), k, loss, loss.copy(), np.zeros(count)

        def sqiswap_approx_counts(self, f, first, count):
            calls.append(("counts", np.array(f), first, count))
            return np.tile(np.array([[1, 1, 1, 0]], dtype=np.int64), (len(f), 1)), np.full(len(f), 3 << 31, dtype=np.int64)

    ctx = FakeCtx()
    monkeypatch.setattr(runtime, "get_context", lambda device=0: ctx)
    T = np.stack([np.eye(4, dtype=np.complex128)] * 3)
    res = analytic.sqiswap_approx_decompose(T, basis_fidelity=0.5, cycles=2)
    assert calls[-2:] == [("set_targets", 3), ("decompose", 0.5, 2, 0, 3)]
    assert isinstance(res, analytic.ApproxDecomposition) and res.basis_fidelity == 0.5
    assert np.array_equal(gate_matrix(res.basis_gate), gate_matrix(RiSwapGate(1 / 2)))
    assert np.allclose(res.expected_fidelity, [1.0, (4 + 16 * 0.81) / 20 * 0.5, 0.25], rtol=0, atol=1e-15)
    assert np.array_equal(res.predicted_loss, [0.0, 0.1, 0.0])
    e = res.entries()
    assert [len(v.Xk) for v in e] == [6, 12, 18] and [v.cycles for v in e] == [0, 1, 2] and [v.success_label for v in e] == [1, 0, 1]
    analytic.sqiswap_approx_decompose(list(T))  # a list of matrices; the defaults
    assert calls[-1] == ("decompose", 1.0, None, 0, 3)
    n_calls = len(calls)
    empty = analytic.sqiswap_approx_decompose(np.zeros((0, 4, 4)), 0.9)
    assert len(empty) == 0 and empty.Xk.shape == (0, 24) and empty.entries() == [] and len(empty.predicted_loss) == 0
    assert len(empty.expected_fidelity) == 0 and empty.basis_fidelity == 0.9
    es = analytic.sqiswap_fidelity_sweep([], [0.9, 1.0])
    assert es.n_targets == 0 and es.counts.shape == (2, 4) and not es.counts.any() and np.all(np.isnan(es.average_fidelity))
    assert len(calls) == n_calls  # nothing reached the context
    sw = analytic.sqiswap_fidelity_sweep(T, [0.9, 1.0])
    assert calls[-1][0] == "counts" and calls[-1][1].tolist() == [0.9, 1.0] and calls[-1][2:] == (0, 3)
    assert sw.counts.shape == (2, 4) and sw.average_gates.tolist() == [1.0, 1.0] and sw.average_fidelity.tolist() == [0.5, 0.5]
    assert sw.n_targets == 3 and np.array_equal(gate_matrix(sw.basis_gate), gate_matrix(RiSwapGate(1 / 2)))
    with pytest.raises(ValueError, match="shape"):
        analytic.sqiswap_approx_decompose(np.zeros((2, 3, 3)))
    # a device sampler fills the context itself: nothing is uploaded
    from slam_decomposition_amd.sampler import DeviceHaarBatch

    calls.clear()
    analytic.sqiswap_approx_decompose(DeviceHaarBatch(seed=5, n_samples=7), 0.97)
    assert not any(name == "set_targets" for name, *_ in calls) and calls[-1] == ("decompose", 0.97, None, 0, 7)


def test_symbols_are_declared_and_exported():
    from slam_decomposition_amd import _ffi

    lib = _ffi.load_library()
    for name, n_args in (("slam_sqiswap_approx_decompose", 10), ("slam_sqiswap_approx_counts", 7)):
        assert name in _ffi.EXPORTED_SYMBOLS
        fn = getattr(lib, name)
        assert fn.restype is ctypes.c_int and len(fn.argtypes) == n_args
    assert lib.slam_abi_version() == 7
    assert hasattr(_ffi.Context, "sqiswap_approx_decompose") and hasattr(_ffi.Context, "sqiswap_approx_counts")
    header = open(_header_path()).read()
    assert "int slam_sqiswap_approx_decompose(slam_ctx* ctx" in header and "int slam_sqiswap_approx_counts(slam_ctx* ctx" in header
    assert "slam_sqiswap_approx_decompose and slam_sqiswap_approx_counts (new symbols only)" in header


def _header_path():
    import os

    return os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "slam_hip.h")


def test_c_abi_refusals_with_a_null_context():
    """What needs no context is checked first: with a NULL context good arguments get as far as "ctx is NULL", bad ones do not; nothing
    is written by a refused call."""
    from slam_decomposition_amd import _ffi

    lib = _ffi.load_library()
    out = [np.zeros((1, 24)), np.zeros(1, dtype=np.int32), np.zeros(1), np.zeros(1), np.zeros(1)]
    ptrs = [_ffi._ptr(a) for a in out]

    def call(f=0.99, force=-1):
        rc = lib.slam_sqiswap_approx_decompose(None, 0, 1, f, force, *ptrs)
        return rc, lib.slam_last_error().decode()

    for force in range(-1, 4):
        rc, msg = call(force=force)
        assert rc == -1 and "ctx is NULL" in msg, msg
    for f in (0.0, -0.5, 1.0000001, float("nan"), float("inf")):
        rc, msg = call(f=f)
        assert rc == -1 and "basis_fidelity" in msg, (f, msg)
    for force in (-2, 4):
        rc, msg = call(force=force)
        assert rc == -1 and "force_cycles" in msg, (force, msg)
    assert not any(np.any(a) for a in out)

    cbuf, sbuf = np.zeros((65, 4), dtype=np.int64), np.zeros(65, dtype=np.int64)

    def counts(n=2, f=(0.9, 1.0)):
        fa = np.ascontiguousarray(f, dtype=np.float64)
        rc = lib.slam_sqiswap_approx_counts(None, 0, 1, n, _ffi._ptr(fa), _ffi._ptr(cbuf), _ffi._ptr(sbuf))
        return rc, lib.slam_last_error().decode()

    rc, msg = counts()
    assert rc == -1 and "ctx is NULL" in msg, msg
    for n in (0, -1, 65):
        rc, msg = counts(n=n, f=np.full(65, 0.9))
        assert rc == -1 and "n_fid" in msg
    for f in (0.0, 1.5, float("nan")):
        rc, msg = counts(f=(0.9, f))
        assert rc == -1 and "fidelities[1]" in msg
    assert not cbuf.any() and not sbuf.any()
