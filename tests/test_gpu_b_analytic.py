"""GPU: ``b_decompose_kernel`` (slam_b_decompose) and ``analytic.b_decompose`` on top of it: closed-form circuits of one or two gates of
the B class that equal their targets (csrc/slam_b.hpp; the yardstick is tests/b_ref.py, which tests/test_b_analytic_host.py holds to the
same bounds on the CPU).

Bounds (all set before the kernel ran):

  * sizes: span_rules.minimal_span for family b on the 8-digit coordinates, local targets at two gates (= ``ctx.predict_spans`` on Haar
    targets); CAN(0.5, 0.25, 2e-8) lies on the rule's tolerance, where either size is right;
  * the reported loss is that of the written row: |loss - loss2| <= 1e-14 against ``ctx.eval_unitary`` and the NumPy oracle;
  * gap <= 1e-7 (the size rule's own tolerance: a target 2e-8 + rounding off the gate's class still gets one gate);
  * loss <= 11.2 gap^2 + 1e-14 (the BOUND of tests/test_gpu_complete_locals.py: derived there);
  * matrix level, on ALL Haar targets: max |T - e^{ig} template(x)| <= 4 x kak_ref.tolerance(e_ref), e_ref the LAPACK residual over
    the same targets (one alignment, as the completion tests allow it); loss <= 1e-13;
  * for two gates the gap is rounding only: on the Haar targets at most 4 x the worst gap of ``b_ref.decompose`` on the same targets on
    the CPU (4: one more alignment's rounding), floored at 1e-12, the bound of tests/test_gpu_cx_analytic.py.  The reference's worst
    gap over the 4096 targets, measured on the CPU before the first GPU run: 6.4e-16, so the bound is the floor, 1e-12; the device's
    worst gap on them, measured afterwards: 3.3e-16 for each of the four basis gates.

Measured on an MI355X (``B-ANALYTIC`` lines with ``-s``), the same for the four basis gates (B, CAN at the point, two
dressed members): over the 15 named cases loss <= 1.0e-15, |loss - loss2| <= 7.8e-16, gap <= 1e-15 except 1.0e-9 at CAN(0.5, 0.25, 1e-9) (one
gate inside the size tolerance); CAN(0.5, 0.25, 2e-8) came out as two gates; 4096 Haar targets: loss <= 1.0e-15, gap <= 3.3e-16, worst matrix
error 1.4e-15 over ALL targets (tolerance 4e-13); the 64 circuits rebuilt through the API (sizes 4 / 60): BasicCost <= 1.0e-15.
"""
import numpy as np
import pytest

import b_ref as br
import kak_ref as kr
from oracle import slam_oracle as o

pytestmark = pytest.mark.gpu

BOUND = 11.2  # tests/test_gpu_complete_locals.py
GATES = br.basis_gates(np.random.default_rng(20))
GATE_IDS = [n for n, _ in GATES]
N_HAAR = 4096


def _up_to_phase(T, W):
    tr = np.einsum("nij,nij->n", np.conj(W), T)
    return np.max(np.abs(T - (tr / np.abs(tr))[:, None, None] * W), axis=(1, 2))


def _reevaluate(ctx, G, x, cycles):
    """(W, loss2) of the rows through ``ctx.eval_unitary`` with the gate table [G] (the resident targets are the rows' own)."""
    ctx.set_gates(G[None])
    ctx.set_cost(0)
    W = np.zeros((len(x), 4, 4), dtype=np.complex128)
    loss2 = np.zeros(len(x))
    for k in (1, 2):
        idx = np.flatnonzero(cycles == k)
        if len(idx):
            W[idx], loss2[idx] = ctx.eval_unitary([0] * k, x[idx, : 6 * (k + 1)], idx)
    return W, loss2


def _common_checks(label, x, cycles, loss, gap, loss2):
    assert np.all(np.isfinite(x)) and np.all(np.isfinite(loss)) and np.all(np.isfinite(gap))
    assert np.all((cycles >= 1) & (cycles <= 2))
    print(f"B-ANALYTIC {label:<44s} rows {len(x)} sizes {sorted(set(cycles.tolist()))} worst loss {loss.max():.3g} gap {gap.max():.3g} "
          f"|loss - loss2| {np.abs(loss - loss2).max():.3g}")
    assert np.abs(loss - loss2).max() <= 1e-14
    assert gap.max() <= 1e-7, (label, gap.max())
    assert np.all(loss <= BOUND * gap ** 2 + 1e-14), (label, loss.max(), gap.max())
    for k in (1, 2):
        assert not np.any(x[cycles == k, 6 * (k + 1):])  # zeros behind the row


@pytest.mark.parametrize("name,gate", br.NAMED, ids=[n for n, _ in br.NAMED])
@pytest.mark.parametrize("gname,G", GATES, ids=GATE_IDS)
def test_named_and_hard_inputs(hip_ctx, gname, G, name, gate):
    rng = np.random.default_rng(31)
    T = br.dress(rng, gate, 65)
    hip_ctx.set_targets(T)
    x, cycles, loss, gap = hip_ctx.b_decompose(G)
    if name not in br.ON_BOUNDARY:
        assert np.array_equal(cycles, br.expected_size(T)), (name, cycles)
        assert np.all(cycles == (1 if name in br.ONE_GATE else 2))
    W, loss2 = _reevaluate(hip_ctx, G, x, cycles)
    _common_checks(f"{gname} / {name}", x, cycles, loss, gap, loss2)
    for i in (0, 64):  # ... and by the NumPy oracle
        k = int(cycles[i])
        assert abs(o.basic_cost(o.template_eval(x[i, : 6 * (k + 1)], [G] * k), T[i]) - loss[i]) <= 1e-14


@pytest.fixture(scope="module")
def haar():
    """The 4096 host-generated Haar targets of the matrix-level test, the tolerance their LAPACK residual gives and the worst gap the
    NumPy reference leaves on them (a quarter of the targets per basis gate), once for all gates."""
    from slam_decomposition_amd.sampler import HaarBatch

    T = HaarBatch(seed0=9200, n_samples=N_HAAR).as_array()
    rng = np.random.default_rng(7)
    tol = 4 * kr.tolerance(max(kr.lapack_residual(t, rng) for t in T))
    ref_gap = max(br.decompose(T[i], GATES[i % len(GATES)][1])[3] for i in range(N_HAAR))
    print(f"B-ANALYTIC reference: worst gap of b_ref.decompose over {N_HAAR} Haar targets {ref_gap:.3g}")
    return T, tol, ref_gap


@pytest.mark.parametrize("gname,G", GATES, ids=GATE_IDS)
def test_haar_matrix_level(hip_ctx, haar, gname, G):
    T, tol, ref_gap = haar
    hip_ctx.set_targets(T)
    x, cycles, loss, gap = hip_ctx.b_decompose(G)
    assert np.all(cycles == 2)
    assert np.array_equal(cycles, hip_ctx.predict_spans([br.POINT] * 2, 2))
    W, loss2 = _reevaluate(hip_ctx, G, x, cycles)
    _common_checks(f"{gname} / haar {N_HAAR}", x, cycles, loss, gap, loss2)
    err = _up_to_phase(T, W)
    gap_bound = max(4 * ref_gap, 1e-12)
    print(f"B-ANALYTIC {gname} / haar: worst |T - e^(ig) W| {err.max():.3g} tol {tol:.3g}; worst gap {gap.max():.3g} bound {gap_bound:.3g}")
    assert err.max() <= tol, (int(np.argmax(err)), err.max(), tol)
    assert loss.max() <= 1e-13
    assert gap.max() <= gap_bound, (int(np.argmax(gap)), gap.max(), gap_bound)


@pytest.mark.parametrize("gname,G", [GATES[0], GATES[3]], ids=[GATE_IDS[0], GATE_IDS[3]])
def test_windows_and_reproducibility(hip_ctx, gname, G):
    from slam_decomposition_amd import _ffi

    n = 4096
    hip_ctx.sample_haar(11, n)
    full = hip_ctx.b_decompose(G)
    again = hip_ctx.b_decompose(G)
    for a, b in zip(full, again):
        assert np.array_equal(a, b)
    for first, count in ((0, 1), (63, 130), (n - 77, 77)):
        part = hip_ctx.b_decompose(G, first, count)
        for a, b in zip(full, part):
            assert np.array_equal(a[first:first + count], b)
    g, dress = _ffi.b_dress(G)
    lib, h = hip_ctx._lib, hip_ctx._h
    assert lib.slam_b_decompose(h, 0, 8, _ffi._ptr(g), _ffi._ptr(dress), None, None, None, None) == 0  # every output is optional
    hip_ctx.set_targets(hip_ctx.get_targets(0, 64))
    for first, count in ((60, 5), (-1, 2), (0, 65)):
        with pytest.raises(_ffi.SlamHipError):
            hip_ctx.b_decompose(G, first, count)
    out = [np.zeros((8, 24)), np.zeros(8, dtype=np.int32), np.zeros(8), np.zeros(8)]
    ptrs = [_ffi._ptr(a) for a in out]
    with pytest.raises(_ffi.SlamHipError):  # an out-of-range window, outputs given
        _ffi._check(lib.slam_b_decompose(h, 60, 8, _ffi._ptr(g), _ffi._ptr(dress), *ptrs))
    cx = np.ascontiguousarray(br.CX)
    with pytest.raises(_ffi.SlamHipError):  # a foreign gate, with its own (true) factors: the coordinates are not the class's
        from slam_decomposition_amd import weyl

        _, l1, l0, c, r1, r0 = weyl.kak(cx)
        foreign = np.concatenate([np.stack([l1, l0, r1, r0]).astype(np.complex128).view(np.float64).ravel(), np.asarray(c, dtype=np.float64)])
        _ffi._check(lib.slam_b_decompose(h, 0, 8, _ffi._ptr(cx), _ffi._ptr(foreign), *ptrs))
    other = np.ascontiguousarray(br.dress(np.random.default_rng(3), g))
    with pytest.raises(_ffi.SlamHipError):  # a gate that is not the one the factors were made for
        _ffi._check(lib.slam_b_decompose(h, 0, 8, _ffi._ptr(other), _ffi._ptr(dress), *ptrs))
    bad = dress.copy()
    bad[8 * 2] += 1e-9
    with pytest.raises(_ffi.SlamHipError):  # a factor that is not the host's
        _ffi._check(lib.slam_b_decompose(h, 0, 8, _ffi._ptr(g), _ffi._ptr(bad), *ptrs))
    assert not any(np.any(a) for a in out)  # nothing was written by the refused calls
    with pytest.raises(ValueError):  # a gate outside the class never reaches the library
        hip_ctx.b_decompose(br.CX)


def test_api(hip_ctx):
    from slam_decomposition_amd import analytic
    from slam_decomposition_amd.basis import CircuitTemplate
    from slam_decomposition_amd.cost_function import BasicCost
    from slam_decomposition_amd.gates import BerkeleyGate, CanonicalGate, UnitaryGate
    from slam_decomposition_amd.optimizer import TemplateOptimizer
    from slam_decomposition_amd.sampler import DeviceHaarBatch, HaarBatch

    def same(a, b):
        return all(np.array_equal(getattr(a, f), getattr(b, f)) for f in ("cycles", "Xk", "loss", "gap"))

    hb = HaarBatch(seed0=4100, n_samples=64)
    targets = hb.as_array()
    rng = np.random.default_rng(8)
    # a few targets of the gate's own class and a few local ones among the Haar ones
    mixed = targets.copy()
    mixed[:4] = br.dress(rng, br.B, 4)
    mixed[4:8] = br.dress(rng, np.eye(4, dtype=np.complex128), 4)
    cost = BasicCost()
    for gate in (BerkeleyGate(), CanonicalGate(np.pi / 4, np.pi / 8, 0.0), UnitaryGate(GATES[3][1])):
        res = analytic.b_decompose(targets, gate)
        assert same(res, analytic.b_decompose(hb, gate)) and same(res, analytic.b_decompose(list(targets), gate))
        db = DeviceHaarBatch(seed=5, n_samples=64)
        assert same(analytic.b_decompose(db, gate), analytic.b_decompose(db.as_array(), gate))
        assert res.Xk.shape == (64, 24) and len(res) == 64 and res.basis_gate is gate
        assert isinstance(res, analytic.CxDecomposition) and np.all(res.cycles == 2)
        with pytest.raises(NotImplementedError, match="b_decompose"):
            analytic.decompose(targets, gate)

        res = analytic.b_decompose(mixed, gate)
        basis = CircuitTemplate(base_gates=[gate])
        worst = 0.0
        for e, t in zip(res.entries(), mixed):
            assert len(e.Xk) == 6 * (e.cycles + 1) and e.success_label == 1
            basis.build(e.cycles)
            worst = max(worst, cost.unitary_fidelity(basis.eval(e.Xk), t))
        print(f"B-ANALYTIC api {gate}: sizes {np.bincount(res.cycles, minlength=3)[1:].tolist()} worst BasicCost of the rebuilt circuits {worst:.3g}")
        assert worst <= 1e-13
        assert res.cycles.tolist() == [1] * 4 + [2] * 60

        # the optimizer's sizes on the same batch.  It refuses a batch with a local target as the reference does (build(0), ValueError),
        # where the closed form gives a valid two-gate circuit: the comparison is over the batch without the four local ones
        def poly():
            return TemplateOptimizer(CircuitTemplate(base_gates=[gate], maximum_span_guess=2, use_polytopes=True), BasicCost(),
                                     training_restarts=16, seed=2)

        with pytest.raises(ValueError):
            poly()._approximate_batch(list(mixed), log_index=False)
        keep = np.r_[0:4, 8:64]
        data = poly()._approximate_batch(list(mixed[keep]), log_index=False)
        assert [d.cycles for d in data] == [int(k) for k in res.cycles[keep]]
    assert analytic.b_decompose(targets).basis_gate.name == BerkeleyGate().name
