"""GPU: the quasi-Newton metric's rank-2 update ``H += s w^T + v s^T`` on the matrix pipe (csrc/slam_device.hpp: h_update_mfma).

* Device check (slam_metric_update_check): the form the optimizer kernels run and the v_pk_fma_f32 form, which the check kernel keeps
  as the reference, give the same bits -- no mask, no tolerance -- on 64 items for NA = 3, 5, 6 (spans 1, 2, 3).  An fp32 MFMA
  accumulation is the same fmaf chain as the vector form's two dependent FMAs per element, in the same order.
* Optimizer runs at the smallest shapes that reach every caller of the update follow the NumPy port of the same iteration
  (oracle/bfgs_port.py, oracle/pqn_port.py) item by item, with the bounds of tests/test_gpu_minimize_parity.py and
  tests/test_gpu_v2.py; the one-wavefront loop, the speculative spans and a two-context multi-queue call equal the per-span launches
  bit for bit.
"""
import functools

import numpy as np
import pytest

from oracle import slam_oracle as o
from oracle.bfgs_port import minimize_port
from slam_decomposition_amd import _ffi

pytestmark = pytest.mark.gpu

N_ITEMS = 64
GATES = {"sqiswap": o.riswap_matrix(0.5), "cx": o.cx_matrix()}
N_T, R, SEED = 3, 2, 11
SEQS = [[0], [0, 0], [0, 0, 0]]
ORDERED = _ffi.FLAG_EARLY_EXIT | _ffi.FLAG_ORDERED


# ---------------------------------------------------------------------------------------------------------------------------------
# device check
# ---------------------------------------------------------------------------------------------------------------------------------
def _signed_pow10(rng, lo, hi, shape):
    return (rng.choice([-1.0, 1.0], shape) * 10.0 ** rng.uniform(lo, hi, shape)).astype(np.float32)


def _inputs(kind, na):
    """(h [64, nb, 4, 4], s, w, v [64, 4 na]) float32; every value finite, and so is every result."""
    nb, n = na * (na + 1) // 2, 4 * na
    rng = np.random.default_rng([na, sorted(KINDS).index(kind)])
    if kind == "random":
        h, s, w, v = (rng.standard_normal(sh).astype(np.float32) for sh in ((N_ITEMS, nb, 4, 4), (N_ITEMS, n), (N_ITEMS, n), (N_ITEMS, n)))
    elif kind == "no_step":
        # quads that do not step: w = v = 0 (s is whatever the round left there); every second item, so that both kinds share a wavefront
        h, s, w, v = (rng.standard_normal(sh).astype(np.float32) for sh in ((N_ITEMS, nb, 4, 4), (N_ITEMS, n), (N_ITEMS, n), (N_ITEMS, n)))
        w[::2] = 0.0
        v[::2] = 0.0
    elif kind == "wide_range":
        # H and s over 1e-30 .. 1e30, w and v over 1e-30 .. 1e8: the largest result is below 1e30 + 2e38 < FLT_MAX
        h = _signed_pow10(rng, -30, 30, (N_ITEMS, nb, 4, 4))
        s = _signed_pow10(rng, -30, 30, (N_ITEMS, n))
        w = _signed_pow10(rng, -30, 8, (N_ITEMS, n))
        v = _signed_pow10(rng, -30, 8, (N_ITEMS, n))
    elif kind == "denormal_products":
        # products of 1e-38 .. 1e-45 (fp32 denormals: 1.2e-38 .. 1.4e-45) added to zeros, denormals and small normal numbers; a quarter
        # of the s values are denormal themselves and meet w, v of order one
        s = _signed_pow10(rng, -22, -18, (N_ITEMS, n))
        w = _signed_pow10(rng, -23, -20, (N_ITEMS, n))
        v = _signed_pow10(rng, -23, -20, (N_ITEMS, n))
        sub = rng.random((N_ITEMS, n)) < 0.25
        s[sub] = _signed_pow10(rng, -44, -39, (N_ITEMS, n))[sub]
        w[sub] = _signed_pow10(rng, -1, 1, (N_ITEMS, n))[sub]
        h = _signed_pow10(rng, -44, -36, (N_ITEMS, nb, 4, 4))
        h[rng.random(h.shape) < 0.25] = 0.0
    elif kind == "distinct":
        # a value of its own in every (item, row, column) position: a swapped operand role or a transposed block cannot pass
        h = (1.0 + np.arange(N_ITEMS * nb * 16) / 4096.0).reshape(N_ITEMS, nb, 4, 4).astype(np.float32)
        s = (2.0 + np.arange(N_ITEMS * n) / 512.0).reshape(N_ITEMS, n).astype(np.float32)
        w = (-7.0 - np.arange(N_ITEMS * n) / 384.0).reshape(N_ITEMS, n).astype(np.float32)
        v = (5.0 + np.arange(N_ITEMS * n) / 640.0).reshape(N_ITEMS, n).astype(np.float32)
        assert len(np.unique(h)) == h.size and all(len(np.unique(a)) == a.size for a in (s, w, v))
    else:
        raise KeyError(kind)
    return h, s, w, v


KINDS = {"random", "no_step", "wide_range", "denormal_products", "distinct"}


@pytest.mark.parametrize("kind", sorted(KINDS))
@pytest.mark.parametrize("na", [3, 5, 6])
def test_matrix_pipe_update_equals_the_vector_form_bit_for_bit(hip_ctx, na, kind):
    h, s, w, v = _inputs(kind, na)
    shipped, vector = hip_ctx.metric_update_check(h, s, w, v)
    assert np.all(np.isfinite(vector))
    diff = shipped.view(np.uint32) != vector.view(np.uint32)
    print(f"na={na} {kind}: {int(diff.sum())} of {diff.size} elements differ")
    assert not diff.any(), (na, kind, np.argwhere(diff)[:4].tolist())
    if kind == "no_step":
        assert np.array_equal(shipped[::2].view(np.uint32), h[::2].view(np.uint32))  # H comes back untouched
        assert np.mean(shipped[1::2] != h[1::2]) > 0.9  # ... and the stepping quads beside them are updated
    if kind == "denormal_products":
        tiny = np.finfo(np.float32).tiny
        moved = shipped != h
        assert np.any(moved & (np.abs(shipped) < tiny) & (shipped != 0.0))  # denormal results are kept, not flushed
    if kind == "distinct":
        # the documented layout, against the update written out in float64 (each element: two roundings against the device's two)
        for a in range(na):
            for b in range(a, na):
                sa, sb = s[:, 4 * a : 4 * a + 4].astype(np.float64), s[:, 4 * b : 4 * b + 4].astype(np.float64)
                va, wb = v[:, 4 * a : 4 * a + 4].astype(np.float64), w[:, 4 * b : 4 * b + 4].astype(np.float64)
                want = h[:, b * (b + 1) // 2 + a] + va[:, :, None] * sb[:, None, :] + sa[:, :, None] * wb[:, None, :]
                got = shipped[:, b * (b + 1) // 2 + a].astype(np.float64)
                assert np.max(np.abs(got - want) / np.abs(want).max()) < 4 * np.finfo(np.float32).eps, (a, b)


def test_update_check_refuses_other_sizes(hip_ctx):
    z = np.zeros((2, 16), np.float32)
    with pytest.raises(_ffi.SlamHipError):
        hip_ctx.metric_update_check(np.zeros((2, 10, 4, 4), np.float32), z, z, z)  # NA = 4: no optimizer kernel has it


# ---------------------------------------------------------------------------------------------------------------------------------
# optimizer runs
# ---------------------------------------------------------------------------------------------------------------------------------
def _targets():
    return o.haar_batch(N_T, seed0=777)


@functools.lru_cache(maxsize=None)
def _port_runs(name, k):
    """The NumPy port's runs of the N_T x R items, computed once: (loss, status, evaluations) per item."""
    targets = _targets()
    rows = [[minimize_port(o.x0_philox(SEED, t, r, k), [GATES[name]] * k, targets[t]) for r in range(R)] for t in range(N_T)]
    return [[(f, st, nev) for f, _x, _it, st, nev in row] for row in rows]


@pytest.mark.parametrize("name", ["sqiswap", "cx"])
@pytest.mark.parametrize("k", [1, 2, 3])
def test_per_span_launches_follow_the_cpu_port(hip_ctx, k, name):
    """minimize_kernel<k>: same converged loss as the port item by item and -- rounding of the float32 metric aside -- the same
    number of evaluations (the bounds of tests/test_gpu_minimize_parity.py::test_full_runs_follow_cpu_port)."""
    hip_ctx.set_targets(_targets())
    hip_ctx.set_gates(GATES[name][None])
    out = hip_ctx.minimize_stage([0] * k, _ffi.OptParams(restarts=R, maxiter=2500, gtol=1e-9, stop_loss=1e-13, seed=SEED, flags=0))
    port = _port_runs(name, k)
    same_evals = 0
    for t in range(N_T):
        for r in range(R):
            f, st, nev = port[t][r]
            print(f"{name} k={k} item ({t}, {r}): loss {out['item_loss'][t, r]:.3e} / port {f:.3e}, evaluations {out['item_evals'][t, r]} / {nev}")
            assert out["item_status"][t, r] in (0, 4) and st in (0, 4)
            assert abs(out["item_loss"][t, r] - f) < 1e-6, (name, k, t, r, out["item_loss"][t, r], f)
            same_evals += int(out["item_evals"][t, r] == nev)
            assert abs(int(out["item_evals"][t, r]) - nev) <= max(8, nev // 4), (name, k, t, r, out["item_evals"][t, r], nev)
    assert same_evals >= (N_T * R) // 2, (name, k, same_evals)


def _equal(a, b):
    return all(np.array_equal(u, v) for u, v in zip(a, b))


def test_wave_loop_and_speculative_spans_equal_the_per_span_launches():
    """The same three targets through span_wave_kernel (a loop of one span: the one-wavefront loop) and span_spec_kernel (spans 1..3
    of a small batch: the speculative spans) against SLAM_FLAG_STAGED, the per-span launches: losses, parameters and cycles bit for
    bit."""
    with _ffi.Context(0) as ctx:
        ctx.set_targets(_targets())
        ctx.set_gates(GATES["sqiswap"][None])

        def run(k0, k1, extra):
            prm = _ffi.OptParams(restarts=R, maxiter=2500, gtol=1e-9, stop_loss=1e-13, seed=SEED, flags=ORDERED | extra)
            ctx.reset_stats()
            res = ctx.decompose_range(0, N_T, k0, k1, SEQS[k0 - 1 : k1], prm, 1e-10)
            return res, ctx.stats()["kernel_launches"]

        for k in (1, 2, 3):
            (wave, n_wave), (staged, n_staged) = run(k, k, 0), run(k, k, _ffi.FLAG_STAGED)
            assert n_wave == 1 and n_staged == 1
            assert _equal(wave, staged), k
        (spec, n_spec), (staged, n_staged) = run(1, 3, 0), run(1, 3, _ffi.FLAG_STAGED)
        assert n_spec == 4 and n_staged == 3  # three spans side by side + the merge / one launch per span
        assert _equal(spec, staged)
        assert np.all(spec[0] < 1e-8)


def test_two_context_multi_queue_call_equals_the_per_span_launches():
    """minimize_kernel<k, GC, MQ = true>: two contexts (two gates of one structure class, the same three targets) behind one launch
    per span leave in each context what its own per-span launches leave, bit for bit."""
    gates = [o.riswap_matrix(0.5), o.riswap_matrix(0.25)]
    prm = _ffi.OptParams(restarts=R, maxiter=2500, gtol=1e-9, stop_loss=1e-13, seed=SEED, flags=ORDERED)
    staged = _ffi.OptParams(restarts=R, maxiter=2500, gtol=1e-9, stop_loss=1e-13, seed=SEED, flags=ORDERED | _ffi.FLAG_STAGED)
    ctxs = [_ffi.Context(0) for _ in gates]
    try:
        for c, g in zip(ctxs, gates):
            c.set_targets(_targets())
            c.set_gates(g[None])
        solo = [c.decompose_range(0, N_T, 1, 3, SEQS, staged, 1e-10) for c in ctxs]
        for c in ctxs:
            c.reset_stats()
        _ffi.decompose_multi(ctxs, 0, N_T, 1, 3, SEQS, prm, 1e-10)
        assert ctxs[0].stats()["kernel_launches"] == 3 and ctxs[1].stats()["kernel_launches"] == 0  # one class: one launch per span
        for c, want in zip(ctxs, solo):
            assert _equal(c.fetch_results_range(3, 0, N_T), want)
    finally:
        for c in ctxs:
            c.close()


def test_v2_riswap_stage_follows_the_cpu_port(hip_ctx):
    """minimize_v2_kernel (CircuitTemplateV2, RiSwapGate class, k = 1, the gate parameter bounded to [0, 1]) from explicit start
    points against oracle/pqn_port.py, as tests/test_gpu_v2.py does for the constrained stage: the best of each target's restarts
    agrees to 1e-6 and at least 70 % of the items end in the port's minimum."""
    from oracle import pqn_port
    from oracle import v2_oracle as v
    from slam_decomposition_amd.basisv2 import CircuitTemplateV2, gate_map
    from slam_decomposition_amd.gates import RiSwapGate

    basis = CircuitTemplateV2(base_gates=[RiSwapGate])
    basis.build(1)
    for name in basis.parameter_names():
        if name.startswith("Q"):
            basis.add_bound(name, 1.0, 0.0)
    n_dev, _idx, ilo, ihi, blo, bhi = basis.device_layout(1)
    assert n_dev == 13
    targets = _targets()
    hip_ctx.set_targets(targets)
    hip_ctx.v2_set_gates(basis._gate_maps)
    rng = np.random.default_rng(8)
    x0 = np.concatenate([rng.uniform(-4 * np.pi, 4 * np.pi, (N_T, R, 12)), rng.uniform(0.0, 1.0, (N_T, R, 1))], axis=2)
    out = hip_ctx.v2_minimize_stage([0], _ffi.OptParams(restarts=R, seed=1), 1e-10, ilo, ihi, blo, bhi, x0=x0)
    gm = gate_map(RiSwapGate)[1:]
    agree = 0
    for t in range(N_T):
        fun = lambda xx: v.loss_and_grad(xx, [gm], 1, 1, targets[t], False, False)
        port = np.array([pqn_port.minimize_port(fun, x0[t, r], blo, bhi)[0] for r in range(R)])
        print(f"v2 target {t}: device {out['item_loss'][t]}, port {port}")
        agree += int(np.sum(np.abs(port - out["item_loss"][t]) < 1e-6))
        assert abs(port.min() - out["best_loss"][t]) < 1e-6, (t, port.min(), out["best_loss"][t])
        assert abs(fun(out["best_x"][t])[0] - out["best_loss"][t]) < 1e-12
    assert agree >= 0.7 * N_T * R, agree
