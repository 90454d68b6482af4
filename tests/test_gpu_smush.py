"""Parallel-drive ("smush") templates on the GPU: eval parity with the SciPy oracle (tests/smush_ref.py), the reduction to the plain
conversion-gain template, item-by-item parity of the minimizer with oracle/pqn_port.py, the reference's vertex targets
(parallel_drive_volume.py), determinism, callback, shards and the conversion-gain param_vec_expand path."""
from __future__ import annotations

import itertools

import numpy as np
import pytest

import smush_ref as R
from oracle import slam_oracle as o
from oracle.pqn_port import minimize_port
from slam_decomposition_amd import _ffi
from slam_decomposition_amd.basisv2 import CircuitTemplateV2
from slam_decomposition_amd.cost_function import BasicCost, SquareCost
from slam_decomposition_amd.gates import CanonicalGate, ConversionGainGate, ConversionGainSmushGate, CXGate, SwapGate, iSwapGate
from slam_decomposition_amd.optimizer import TemplateOptimizer

pytestmark = pytest.mark.gpu

TWO_PI = 2 * np.pi


def smush_fn(N, offset, pc=0.0, pg=0.0, gc=np.pi / 2, gg=0.0, t=1.0):
    if offset == 0:
        return lambda *v: ConversionGainSmushGate(pc, pg, gc, gg, v[:N], v[N:], t_el=t)
    return lambda *v: ConversionGainSmushGate(pc, pg, v[0], v[1], v[2 : 2 + N], v[2 + N :], t_el=t)


def template(N, offset, k, **kw):
    fn_kw = {key: kw.pop(key) for key in ("pc", "pg", "gc", "gg", "t") if key in kw}
    b = CircuitTemplateV2(base_gates=[smush_fn(N, offset, **fn_kw)], param_vec_expand=[offset, N, N], **kw)
    b.build(k)
    return b


def haar(n, seed):
    return o.haar_batch(n, seed0=seed)


def local(rng):
    """a random local gate K1 (x) K2"""
    return np.kron(o.u3(*rng.uniform(-np.pi, np.pi, 3)), o.u3(*rng.uniform(-np.pi, np.pi, 3)))


def bound_all(b, lo=-TWO_PI, hi=TWO_PI):
    for name in b.parameter_names():
        if name.startswith("Q"):
            b.add_bound(name, max=hi, min=lo)


def device_eval(b, X, targets, square):
    ctx = _ffi.Context(0)
    try:
        ctx.set_targets(targets)
        ctx.set_cost(_ffi.COST_SQUARE if square else _ffi.COST_BASIC)
        b.set_device_gates(ctx)
        return b.device_eval(ctx, b.gate_sequence(), X, target_of=np.arange(len(X), dtype=np.int32), want_grad=True, want_unitary=True)
    finally:
        ctx.close()


def test_eval_parity_grid():
    rng = np.random.default_rng(7)
    cases = list(itertools.product([1, 2, 3, 6], [1, 2, 4, 8], [0, 2], [False, True]))
    worst = [0.0, 0.0, 0.0]
    for ci, (k, N, offset, square) in enumerate(cases):
        qn = offset + 2 * N
        if 6 * (k + 1) + qn * k > 128:
            continue
        pc, pg = [(0.0, 0.0), (np.pi, 0.0), (0.0, np.pi), (np.pi, np.pi)][ci % 4]
        gc, gg = (np.pi / 4, np.pi / 4) if ci % 3 == 0 else (np.pi / 2, 0.3)
        vz, noext = ci % 5 == 1, ci % 7 == 2
        b = template(N, offset, k, pc=pc, pg=pg, gc=gc, gg=gg, t=0.5 + 0.25 * (ci % 3), vz_only=vz, no_exterior_1q=noext)
        fn = b.base_gates[0]
        n_user = b.n_params
        X = rng.uniform(-3, 3, (3, n_user))
        X[1, b._n_p(k) :] = 0.0  # zero drives (w = 0 when gc = gg and the gate parameters are the drives)
        X[2, b._n_p(k) :] = rng.uniform(-1e-9, 1e-9, n_user - b._n_p(k))  # w ~ 1e-9
        if offset == 2:
            for j in range(k):
                X[1:, b._n_p(k) + qn * j : b._n_p(k) + qn * j + 2] = 0.6  # gc = gg
        Xd = b.to_device_vector(X)
        T = haar(3, 4000 + ci)
        loss, grad, W = device_eval(b, Xd, T, square)
        for m in range(3):
            lr, gr, Wr = R.loss_grad_unitary(Xd[m], fn, qn, k, T[m], square)
            assert np.all(np.isfinite(grad[m])) and np.isfinite(loss[m])
            worst[0] = max(worst[0], abs(loss[m] - lr))
            worst[1] = max(worst[1], np.abs(W[m] - Wr).max())
            worst[2] = max(worst[2], np.abs(grad[m] - gr).max())
            assert abs(loss[m] - lr) <= 1e-12, (k, N, offset, m)
            assert np.abs(W[m] - Wr).max() <= 1e-12, (k, N, offset, m)
            assert np.abs(grad[m] - gr).max() <= 1e-11, (k, N, offset, m, np.abs(grad[m] - gr).max())
    print("worst |dloss|, |dW|, |dgrad|:", worst)


def test_zero_drives_equal_plain_conversion_gain():
    rng = np.random.default_rng(3)
    k, N = 3, 4
    b = template(N, 2, k, t=0.8)
    plain = CircuitTemplateV2(base_gates=[lambda gc, gg: ConversionGainGate(0, 0, gc, gg, 0.8)])
    plain.build(k)
    for _ in range(4):
        P = rng.uniform(-3, 3, b._n_p(k))
        G = rng.uniform(-2, 2, (k, 2))
        Xs = np.concatenate([P] + [np.concatenate([g, np.zeros(2 * N)]) for g in G])
        Xp = np.concatenate([P, G.ravel()])
        assert np.abs(b.eval(Xs) - plain.eval(Xp)).max() <= 1e-13


def test_minimize_item_parity_with_pqn_port():
    rng = np.random.default_rng(11)
    for (k, N, offset, square) in [(1, 4, 0, True), (2, 2, 2, False)]:
        b = template(N, offset, k, gc=np.pi / 2, gg=0.0, t=1.0)
        bound_all(b)
        fn = b.base_gates[0]
        qn = offset + 2 * N
        n_dev, idx, ilo, ihi, blo, bhi = b.device_layout(k)
        T = haar(2, 9100 + k) if k > 1 else np.stack([local(rng) @ iSwapGate().to_matrix() @ local(rng) for _ in range(2)])
        R_ = 3
        x0 = rng.uniform(-2, 2, (2, R_, n_dev))
        x0 = np.clip(x0, blo, bhi)
        ctx = _ffi.Context(0)
        try:
            ctx.set_targets(T)
            ctx.set_cost(_ffi.COST_SQUARE if square else _ffi.COST_BASIC)
            b.set_device_gates(ctx)
            # (the far-point stop is off on both sides: where it fires depends on the metric's fp32 rounding)
            prm = _ffi.OptParams(restarts=R_, maxiter=2500, gtol=1e-9, stop_loss=1e-13, seed=0, flags=0, gtol_far=0.0)
            out = ctx.smush_minimize_stage(b.gate_sequence(), prm, 1e-10, ilo, ihi, blo, bhi, x0=x0)
        finally:
            ctx.close()
        for t in range(2):
            for r in range(R_):
                fun = lambda xx, t=t: R.loss_grad_unitary(xx, fn, qn, k, T[t], square)[:2]
                lp = minimize_port(fun, x0[t, r], blo, bhi, gtol_far=0.0)[0]
                lg = out["item_loss"][t, r]
                assert abs(lg - lp) <= 1e-8 or (lg < 1e-10 and lp < 1e-10), (k, t, r, lg, lp)


def weyl_distance(U, T):
    """max-norm distance of the Weyl coordinates, (c1, c2, c3) ~ (1 - c1, c2, c3) on the chamber's base face identified"""
    c, ct = o.c1c2c3_raw(U), o.c1c2c3_raw(T)
    mirror = np.array([1.0 - c[0], c[1], c[2]])
    return min(np.abs(c - ct).max(), np.abs(mirror - ct).max() if c[2] < 1e-6 else np.inf)


VERTICES = [np.eye(4, dtype=np.complex128), CXGate().to_matrix(), SwapGate().to_matrix(), iSwapGate().to_matrix(),
            CanonicalGate(np.pi / 4, np.pi / 8, np.pi / 8).to_matrix()]
GATE_LIST = [(np.pi / 2, 0, 1, "iSwap", 3), (np.pi / 2, 0, 1 / 2, "sqiSwap", 3), (np.pi / 4, np.pi / 4, 1, "CNOT", 3),
             (np.pi / 4, np.pi / 4, 1 / 2, "sqCNOT", 6), (3 * np.pi / 8, np.pi / 8, 1, "B", 2), (3 * np.pi / 8, np.pi / 8, 1 / 2, "sqB", 4)]


@pytest.mark.parametrize("row", GATE_LIST, ids=[g[3] for g in GATE_LIST])
def test_reference_vertex_targets(row):
    gc, gg, t, _, iters = row
    N = max(1, round(t / 0.25))  # duration_1q = 0.25
    b = template(N, 0, iters, gc=gc, gg=gg, t=t)
    bound_all(b)
    b.spanning_range = range(iters, iters + 1)
    # (stop_loss 1e-14: a SquareCost of 1e-10 still leaves the Weyl coordinates ~ 1e-5 off)
    opt = TemplateOptimizer(basis=b, objective=SquareCost(), override_fail=True, success_threshold=1e-10, training_restarts=16, seed=5,
                            stop_loss=1e-14)
    for T in VERTICES:
        ret = opt.approximate_target_U(T)
        assert ret.loss_result < 1e-10, (row[3], ret.loss_result)
        b.build(ret.cycles)
        # (a SquareCost below 1e-10 bounds the coordinates to ~ 1e-5; the optimizer's stalls end near 1e-11 .. 1e-10)
        assert weyl_distance(b.eval(ret.Xk), T) < 2e-5, row[3]


def test_local_smush_iswap_k1():
    rng = np.random.default_rng(21)
    b = template(4, 0, 1, gc=np.pi / 2, gg=0.0, t=1.0)
    bound_all(b)
    b.spanning_range = range(1, 2)
    opt = TemplateOptimizer(basis=b, objective=SquareCost(), override_fail=True, success_threshold=1e-10, training_restarts=16, seed=1,
                            stop_loss=1e-14)
    for _ in range(3):
        T = local(rng) @ iSwapGate().to_matrix() @ local(rng)
        ret = opt.approximate_target_U(T)
        assert ret.loss_result < 1e-9, ret.loss_result


def test_determinism_callback_and_shards():
    targets = haar(3, 5150)
    b = template(2, 0, 2, gc=np.pi / 4, gg=np.pi / 4, t=0.5)
    bound_all(b)
    b.spanning_range = range(2, 3)
    runs = []
    for kw in ({}, {}, {"use_callback": True}):
        opt = TemplateOptimizer(basis=b, objective=SquareCost(), override_fail=True, success_threshold=1e-10, training_restarts=4, seed=9, **kw)
        runs.append([opt.approximate_target_U(T) for T in targets])
    for a, c in zip(runs[0], runs[1]):
        assert a.loss_result == c.loss_result and np.array_equal(a.Xk, c.Xk)
    for a, c in zip(runs[0], runs[2]):
        assert np.array_equal(a.Xk, c.Xk)
    # shards: devices=[0, 0] gives the single-device result bit for bit
    single = TemplateOptimizer(basis=b, objective=SquareCost(), override_fail=True, success_threshold=1e-10, training_restarts=4, seed=9)
    sharded = TemplateOptimizer(basis=b, objective=SquareCost(), override_fail=True, success_threshold=1e-10, training_restarts=4, seed=9,
                                devices=[0, 0])
    l1, x1, c1 = single._run_batch_v2(targets, [2])
    l2, x2, c2 = sharded._run_batch_v2(targets, [2])
    assert np.array_equal(l1, l2) and np.array_equal(c1, c2) and all(np.array_equal(a, c) for a, c in zip(x1, x2))


def test_winner_is_lowest_index_restart_below_threshold():
    b = template(4, 0, 3, gc=np.pi / 2, gg=0.0, t=1.0)
    bound_all(b)
    _, _, ilo, ihi, blo, bhi = b.device_layout(3)
    T = haar(4, 6200)
    ctx = _ffi.Context(0)
    try:
        ctx.set_targets(T)
        ctx.set_cost(_ffi.COST_SQUARE)
        b.set_device_gates(ctx)
        prm = _ffi.OptParams(restarts=8, maxiter=2500, gtol=1e-9, stop_loss=1e-13, seed=3, flags=0)
        out = ctx.smush_minimize_stage(b.gate_sequence(), prm, 1e-10, ilo, ihi, blo, bhi)
        again = ctx.smush_minimize_stage(b.gate_sequence(), prm, 1e-10, ilo, ihi, blo, bhi)
    finally:
        ctx.close()
    assert np.array_equal(out["best_x"], again["best_x"]) and np.array_equal(out["item_loss"], again["item_loss"])
    for t in range(4):
        below = np.nonzero(out["item_loss"][t] < 1e-10)[0]
        if len(below):
            assert out["best_restart"][t] == below[0]
        else:
            assert out["best_loss"][t] == out["item_loss"][t].min()


def test_conversion_gain_expand_unused_parameters():
    b = CircuitTemplateV2(base_gates=[lambda *v: ConversionGainGate(0, 0, v[0], v[1], 1.0)], param_vec_expand=[2, 1, 1])
    assert not b.smush and b.n_gate_params == 4
    b.build(2)
    rng = np.random.default_rng(2)
    X = b.to_device_vector(rng.uniform(-2, 2, (3, b.n_params)))
    ctx = _ffi.Context(0)
    try:
        ctx.set_targets(haar(3, 7000))
        b.set_device_gates(ctx)
        loss, grad, _ = ctx.v2_eval(b.gate_sequence(), X, target_of=np.arange(3, dtype=np.int32))
    finally:
        ctx.close()
    n_p = 6 * 3
    for j in range(2):
        assert np.all(grad[:, n_p + 4 * j + 2 : n_p + 4 * j + 4] == 0.0)
        assert np.all(grad[:, n_p + 4 * j : n_p + 4 * j + 2] != 0.0)
    opt = TemplateOptimizer(basis=b, objective=BasicCost(), override_fail=True, training_restarts=2, seed=1)
    b.spanning_range = range(2, 3)
    opt.approximate_target_U(haar(1, 7100)[0])


def test_refusals_on_device():
    b = template(4, 0, 2)
    with pytest.raises(NotImplementedError):
        b.set_constraint(1.0)
    from slam_decomposition_amd.cost_function import MakhlinFunctionalCost

    with pytest.raises(NotImplementedError):
        TemplateOptimizer(basis=b, objective=MakhlinFunctionalCost())
    ctx = _ffi.Context(0)
    try:
        ctx.set_targets(haar(1, 1))
        ctx.set_cost(_ffi.COST_MAKHLIN)
        b.set_device_gates(ctx)
        with pytest.raises(_ffi.SlamHipError) as ei:
            ctx.smush_eval(b.gate_sequence(), np.zeros((1, 6 * 3 + 16)))
        assert ei.value.code == -3
    finally:
        ctx.close()
