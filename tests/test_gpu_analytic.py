"""GPU: ``sqiswap_decompose_kernel`` (slam_sqiswap_decompose) and ``analytic.sqiswap_decompose`` on top of it: closed-form circuits of
two or three sqrt(iSWAP) gates that equal their targets (csrc/slam_analytic.hpp; the yardstick is tests/analytic_ref.py).

Bounds (all set before the kernel was written):

  * sizes: span_rules.minimal_span on the 8-digit coordinates, never below 2 (= ``ctx.predict_spans`` on Haar targets); on the
    exact size boundary CAN(0.3, 0.2, 0.1) either size is right;
  * the reported loss is that of the written row: |loss - loss2| <= 1e-14 against ``ctx.eval_unitary`` and the NumPy oracle;
  * gap <= 1e-7: at a chamber face an 8-ulp error in an arccos argument moves the angle by sqrt(2 * 8 * 2.2e-16) ~ 6e-8 rad = 4e-8 in
    units of pi (and the size rule's own tolerance lets a target 2e-8 beyond |z| = x - y through as two gates);
  * loss <= 11.2 gap^2 + 1e-14 (the BOUND of tests/test_gpu_complete_locals.py: derived there);
  * matrix level, on Haar targets whose conditioning u (analytic_ref) is >= 1e-4 -- at least 90 % of each size class; the restatement
    keeps 97.0 % / 96.1 % --: max |T - e^{ig} template(x)| <= 8 x kak_ref.tolerance(e_ref), e_ref the LAPACK residual over the same
    targets.  The completion tests allow 4 x for one alignment; the three-gate path chains two;
  * 65 536 Haar targets: every loss <= 1e-13, and the share of two-gate targets within 4 standard errors (0.0064) of 0.7927 (KAT-4).

Measured on an MI355X (``ANALYTIC`` lines with ``-s``): over the 18 named cases loss <= 6.7e-16, |loss - loss2| <= 1.1e-15,
gap <= 2.8e-16 except 3.4e-9 at CX, 7.2e-10 at CAN(0.3, 0.2, 0.1 + 1e-9) and 1.0e-9 at CAN(1e-9, 0, 0); 4096 Haar targets: loss <= 4.4e-16,
gap <= 1.1e-13, u >= 1e-4 for 97.6 % / 97.8 % of the two- / three-gate targets with a worst matrix error of 2.7e-15 / 3.4e-14 there
(5.9e-14 / 1.5e-13 over all; tolerance 8e-13); 65 536 Haar targets: loss <= 6.7e-16, gap <= 3.3e-12, share of two gates 0.7919; the 64
circuits rebuilt through the API: BasicCost <= 5.6e-16.
"""
import numpy as np
import pytest

import analytic_ref as ar
import kak_ref as kr
from oracle import slam_oracle as o

pytestmark = pytest.mark.gpu

BOUND = 11.2  # tests/test_gpu_complete_locals.py
SQISW_COORDS = (0.25, 0.25, 0.0)


def _dress(rng, W, n):
    """e^{i phi} (L1 (x) L2) W (R1 (x) R2) with random SU(2) factors and phases: n matrices."""
    ph = np.exp(1j * rng.uniform(0, 2 * np.pi, n))[:, None, None]
    return ph * (kr.kron2(kr.random_su2(rng, n), kr.random_su2(rng, n)) @ W @ kr.kron2(kr.random_su2(rng, n), kr.random_su2(rng, n)))


def _up_to_phase(T, W):
    tr = np.einsum("nij,nij->n", np.conj(W), T)
    return np.max(np.abs(T - (tr / np.abs(tr))[:, None, None] * W), axis=(1, 2))


def _reevaluate(ctx, T, x, cycles):
    """(W, loss2) of the rows through ``ctx.eval_unitary`` (the resident targets are T), per size class."""
    ctx.set_gates(ar.S[None])
    ctx.set_cost(0)
    W = np.zeros((len(x), 4, 4), dtype=np.complex128)
    loss2 = np.zeros(len(x))
    for k in (2, 3):
        idx = np.flatnonzero(cycles == k)
        if len(idx):
            W[idx], loss2[idx] = ctx.eval_unitary([0] * k, x[idx, : 6 * (k + 1)], idx)
    return W, loss2


def _common_checks(label, x, cycles, loss, gap, loss2):
    assert np.all(np.isfinite(x)) and np.all(np.isfinite(loss)) and np.all(np.isfinite(gap))
    assert np.all((cycles == 2) | (cycles == 3))
    print(f"ANALYTIC {label:<28s} rows {len(x)} sizes {sorted(set(cycles.tolist()))} worst loss {loss.max():.3g} gap {gap.max():.3g} "
          f"|loss - loss2| {np.abs(loss - loss2).max():.3g}")
    assert np.abs(loss - loss2).max() <= 1e-14
    assert gap.max() <= 1e-7, (label, gap.max())
    assert np.all(loss <= BOUND * gap ** 2 + 1e-14), (label, loss.max(), gap.max())
    for k in (2, 3):
        assert not np.any(x[cycles == k, 6 * (k + 1):])  # zeros behind the row


@pytest.mark.parametrize("name,gate", ar.NAMED, ids=[n for n, _ in ar.NAMED])
def test_named_and_hard_inputs(hip_ctx, name, gate):
    rng = np.random.default_rng(31)
    T = _dress(rng, gate, 65)
    hip_ctx.set_targets(T)
    x, cycles, loss, gap = hip_ctx.sqiswap_decompose()
    if name not in ar.ON_BOUNDARY:
        assert np.array_equal(cycles, ar.expected_size(T)), (name, cycles)
    W, loss2 = _reevaluate(hip_ctx, T, x, cycles)
    _common_checks(name, x, cycles, loss, gap, loss2)
    for i in (0, 64):  # ... and by the NumPy oracle
        k = int(cycles[i])
        assert abs(o.basic_cost(o.template_eval(x[i, : 6 * (k + 1)], [o.riswap_matrix(0.5)] * k), T[i]) - loss[i]) <= 1e-14


def test_haar_matrix_level(hip_ctx):
    from slam_decomposition_amd import weyl
    from slam_decomposition_amd.sampler import DeviceHaarBatch

    n = 4096
    DeviceHaarBatch(seed=7, n_samples=n).fill(hip_ctx)
    T = hip_ctx.get_targets(0, n)
    x, cycles, loss, gap = hip_ctx.sqiswap_decompose()
    assert np.array_equal(cycles, hip_ctx.predict_spans([SQISW_COORDS] * 3, 3))
    W, loss2 = _reevaluate(hip_ctx, T, x, cycles)
    _common_checks("haar 4096", x, cycles, loss, gap, loss2)
    k_ref, _, u, _, _ = ar.plan(weyl.c1c2c3_batch(T, ndigits=15), weyl.c1c2c3_batch(T, ndigits=8))
    assert np.array_equal(cycles, k_ref)
    keep = u >= 1e-4
    rng = np.random.default_rng(7)
    tol = 8 * kr.tolerance(max(kr.lapack_residual(t, rng) for t in T))
    err = _up_to_phase(T, W)
    for k in (2, 3):
        share = np.mean(keep[cycles == k])
        print(f"ANALYTIC haar k = {k}: {np.sum(cycles == k)} targets, u >= 1e-4 for {share:.4f}, worst |T - e^(ig) W| there "
              f"{err[keep & (cycles == k)].max():.3g} (all: {err[cycles == k].max():.3g}) tol {tol:.3g}")
        assert share >= 0.9
    assert err[keep].max() <= tol, (int(np.argmax(np.where(keep, err, 0))), err[keep].max(), tol)


def test_statistics_and_reproducibility(hip_ctx):
    n = 65536
    hip_ctx.sample_haar(11, n)
    x, cycles, loss, gap = hip_ctx.sqiswap_decompose()
    share = float(np.mean(cycles == 2))
    print(f"ANALYTIC haar 65536: worst loss {loss.max():.3g} worst gap {gap.max():.3g} share of two gates {share:.4f}")
    assert loss.max() <= 1e-13
    assert abs(share - 0.7927) <= 0.0064
    again = hip_ctx.sqiswap_decompose()
    for a, b in zip((x, cycles, loss, gap), again):
        assert np.array_equal(a, b)
    for first, count in ((0, 1), (63, 130), (n - 77, 77)):
        part = hip_ctx.sqiswap_decompose(first, count)
        for a, b in zip((x, cycles, loss, gap), part):
            assert np.array_equal(a[first:first + count], b)
    only = hip_ctx._lib.slam_sqiswap_decompose(hip_ctx._h, 0, 8, None, None, None, None)  # every output is optional
    assert only == 0


def test_api(hip_ctx):
    from slam_decomposition_amd import _ffi, analytic
    from slam_decomposition_amd.basis import CircuitTemplate
    from slam_decomposition_amd.cost_function import BasicCost
    from slam_decomposition_amd.gates import RiSwapGate
    from slam_decomposition_amd.optimizer import TemplateOptimizer
    from slam_decomposition_amd.sampler import DeviceHaarBatch, HaarBatch

    def same(a, b):
        return all(np.array_equal(getattr(a, f), getattr(b, f)) for f in ("cycles", "Xk", "loss", "gap"))

    hb = HaarBatch(seed0=4100, n_samples=64)
    targets = hb.as_array()
    res = analytic.sqiswap_decompose(targets)
    assert same(res, analytic.sqiswap_decompose(hb)) and same(res, analytic.sqiswap_decompose(list(targets)))
    db = DeviceHaarBatch(seed=5, n_samples=64)
    assert same(analytic.sqiswap_decompose(db), analytic.sqiswap_decompose(db.as_array()))
    assert res.Xk.shape == (64, 24) and len(res) == 64

    entries = res.entries()
    basis = CircuitTemplate(base_gates=[RiSwapGate(1 / 2)])
    cost = BasicCost()
    worst = 0.0
    for e, t in zip(entries, targets):
        assert len(e.Xk) == 6 * (e.cycles + 1) and e.success_label == 1
        basis.build(e.cycles)
        worst = max(worst, cost.unitary_fidelity(basis.eval(e.Xk), t))
    print(f"ANALYTIC api: worst BasicCost of the rebuilt circuits {worst:.3g}")
    assert worst <= 1e-13

    poly = TemplateOptimizer(CircuitTemplate(base_gates=[RiSwapGate(1 / 2)], maximum_span_guess=3, use_polytopes=True), BasicCost(),
                             training_restarts=16, seed=2)
    data = poly._approximate_batch(list(targets), log_index=False)
    assert [d.cycles for d in data] == [int(k) for k in res.cycles]

    hip_ctx.set_targets(targets)
    for first, count in ((60, 5), (-1, 2), (0, 65)):
        with pytest.raises(_ffi.SlamHipError):
            hip_ctx.sqiswap_decompose(first, count)
