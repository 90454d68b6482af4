"""GPU: ``cx_decompose_kernel`` (slam_cx_decompose) and ``analytic.cx_decompose`` / ``analytic.decompose`` on top of it: closed-form
circuits of one, two or three gates of the CNOT class or of the iSWAP class that equal their targets (csrc/slam_cx.hpp; the yardstick is
tests/cx_ref.py, which tests/test_cx_analytic_host.py holds to the same bounds on the CPU).

Bounds (all set before the kernel ran):

  * sizes: span_rules.minimal_span for the family on the 8-digit coordinates, local targets at two gates (= ``ctx.predict_spans`` on Haar
    targets); CAN(0.3, 0.2, 2e-8) lies on the rule's tolerance, where either size is right;
  * the reported loss is that of the written row: |loss - loss2| <= 1e-14 against ``ctx.eval_unitary`` and the NumPy oracle;
  * gap <= 1e-7 (the size rule's own tolerance: a target 2e-8 + rounding off the c3 = 0 face or off the gate's class still gets the
    smaller circuit); for three gates the gap is rounding only: <= 1e-12 on Haar targets;
  * loss <= 11.2 gap^2 + 1e-14 (the BOUND of tests/test_gpu_complete_locals.py: derived there);
  * matrix level, on ALL Haar targets: max |T - e^{ig} template(x)| <= 4 x kak_ref.tolerance(e_ref), e_ref the LAPACK residual over
    the same targets (one alignment, as the completion tests allow it); loss <= 1e-13.

Measured on an MI355X (``CX-ANALYTIC`` lines with ``-s``), the same for the five basis gates (CX, CZ, iSWAP, a dressed member
of each class): over the 14 named cases loss <= 1.0e-15, |loss - loss2| <= 1.3e-15, gap <= 4.5e-16 except 1.0e-9 at CAN(0.3, 0.2, 1e-9) (two
gates inside the size tolerance); CAN(0.3, 0.2, 2e-8) came out as three gates; 4096 Haar targets: loss <= 1.0e-15, gap <= 4.5e-16, worst
matrix error 1.5e-15 over ALL targets (tolerance 4e-13); the 64 circuits rebuilt through the API (sizes 4 / 8 / 52): BasicCost <= 7.8e-16.
"""
import numpy as np
import pytest

import cx_ref as cr
import kak_ref as kr
from oracle import slam_oracle as o

pytestmark = pytest.mark.gpu

BOUND = 11.2  # tests/test_gpu_complete_locals.py
GATES = cr.basis_gates(np.random.default_rng(20))
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
    for k in (1, 2, 3):
        idx = np.flatnonzero(cycles == k)
        if len(idx):
            W[idx], loss2[idx] = ctx.eval_unitary([0] * k, x[idx, : 6 * (k + 1)], idx)
    return W, loss2


def _common_checks(label, x, cycles, loss, gap, loss2):
    assert np.all(np.isfinite(x)) and np.all(np.isfinite(loss)) and np.all(np.isfinite(gap))
    assert np.all((cycles >= 1) & (cycles <= 3))
    print(f"CX-ANALYTIC {label:<44s} rows {len(x)} sizes {sorted(set(cycles.tolist()))} worst loss {loss.max():.3g} gap {gap.max():.3g} "
          f"|loss - loss2| {np.abs(loss - loss2).max():.3g}")
    assert np.abs(loss - loss2).max() <= 1e-14
    assert gap.max() <= 1e-7, (label, gap.max())
    assert np.all(loss <= BOUND * gap ** 2 + 1e-14), (label, loss.max(), gap.max())
    for k in (1, 2, 3):
        assert not np.any(x[cycles == k, 6 * (k + 1):])  # zeros behind the row


@pytest.mark.parametrize("name,gate", cr.NAMED, ids=[n for n, _ in cr.NAMED])
@pytest.mark.parametrize("gname,G", GATES, ids=GATE_IDS)
def test_named_and_hard_inputs(hip_ctx, gname, G, name, gate):
    rng = np.random.default_rng(31)
    fam = cr.family_of(G)
    T = cr.dress(rng, gate, 65)
    hip_ctx.set_targets(T)
    x, cycles, loss, gap = hip_ctx.cx_decompose(G)
    if name not in cr.ON_BOUNDARY:
        assert np.array_equal(cycles, cr.expected_size(T, fam)), (name, cycles)
    if name in cr.TWO_GATES:
        assert np.all(cycles == 2)
    if name in cr.THREE_GATES:
        assert np.all(cycles == 3)
    W, loss2 = _reevaluate(hip_ctx, G, x, cycles)
    _common_checks(f"{gname} / {name}", x, cycles, loss, gap, loss2)
    for i in (0, 64):  # ... and by the NumPy oracle
        k = int(cycles[i])
        assert abs(o.basic_cost(o.template_eval(x[i, : 6 * (k + 1)], [G] * k), T[i]) - loss[i]) <= 1e-14


@pytest.fixture(scope="module")
def haar(hip_ctx):
    """The 4096 device Haar targets of the matrix-level test and the tolerance their LAPACK residual gives, once for all gates."""
    from slam_decomposition_amd.sampler import DeviceHaarBatch

    DeviceHaarBatch(seed=7, n_samples=N_HAAR).fill(hip_ctx)
    T = hip_ctx.get_targets(0, N_HAAR)
    rng = np.random.default_rng(7)
    return T, 4 * kr.tolerance(max(kr.lapack_residual(t, rng) for t in T))


@pytest.mark.parametrize("gname,G", GATES, ids=GATE_IDS)
def test_haar_matrix_level(hip_ctx, haar, gname, G):
    T, tol = haar
    hip_ctx.set_targets(T)
    x, cycles, loss, gap = hip_ctx.cx_decompose(G)
    assert np.all(cycles == 3)
    assert np.array_equal(cycles, hip_ctx.predict_spans([cr.CLASSES[cr.family_of(G)]] * 3, 3))
    W, loss2 = _reevaluate(hip_ctx, G, x, cycles)
    _common_checks(f"{gname} / haar {N_HAAR}", x, cycles, loss, gap, loss2)
    err = _up_to_phase(T, W)
    print(f"CX-ANALYTIC {gname} / haar: worst |T - e^(ig) W| {err.max():.3g} tol {tol:.3g}")
    assert err.max() <= tol, (int(np.argmax(err)), err.max(), tol)
    assert loss.max() <= 1e-13
    assert gap.max() <= 1e-12


@pytest.mark.parametrize("gname,G", [GATES[0], GATES[4]], ids=[GATE_IDS[0], GATE_IDS[4]])
def test_windows_and_reproducibility(hip_ctx, gname, G):
    from slam_decomposition_amd import _ffi

    n = 4096
    hip_ctx.sample_haar(11, n)
    full = hip_ctx.cx_decompose(G)
    again = hip_ctx.cx_decompose(G)
    for a, b in zip(full, again):
        assert np.array_equal(a, b)
    for first, count in ((0, 1), (63, 130), (n - 77, 77)):
        part = hip_ctx.cx_decompose(G, first, count)
        for a, b in zip(full, part):
            assert np.array_equal(a[first:first + count], b)
    family, g, dress = _ffi.cx_dress(G)
    lib, h = hip_ctx._lib, hip_ctx._h
    assert lib.slam_cx_decompose(h, 0, 8, family, _ffi._ptr(g), _ffi._ptr(dress), None, None, None, None) == 0  # every output is optional
    hip_ctx.set_targets(hip_ctx.get_targets(0, 64))
    for first, count in ((60, 5), (-1, 2), (0, 65)):
        with pytest.raises(_ffi.SlamHipError):
            hip_ctx.cx_decompose(G, first, count)
    out = [np.zeros((8, 24)), np.zeros(8, dtype=np.int32), np.zeros(8), np.zeros(8)]
    ptrs = [_ffi._ptr(a) for a in out]
    with pytest.raises(_ffi.SlamHipError):  # an unknown family
        _ffi._check(lib.slam_cx_decompose(h, 0, 8, 2, _ffi._ptr(g), _ffi._ptr(dress), *ptrs))
    other = np.ascontiguousarray(cr.dress(np.random.default_rng(3), g))
    with pytest.raises(_ffi.SlamHipError):  # a gate that is not the one the factors were made for
        _ffi._check(lib.slam_cx_decompose(h, 0, 8, family, _ffi._ptr(other), _ffi._ptr(dress), *ptrs))
    bad = dress.copy()
    bad[8 * 6] += 1e-9
    with pytest.raises(_ffi.SlamHipError):  # a factor that is not the host's
        _ffi._check(lib.slam_cx_decompose(h, 0, 8, family, _ffi._ptr(g), _ffi._ptr(bad), *ptrs))
    assert not any(np.any(a) for a in out)  # nothing was written by the refused calls
    with pytest.raises(ValueError):  # a gate of neither class never reaches the library
        hip_ctx.cx_decompose(cr.can((0.5, 0.25, 0.0)))


def test_api(hip_ctx):
    from slam_decomposition_amd import analytic
    from slam_decomposition_amd.basis import CircuitTemplate
    from slam_decomposition_amd.cost_function import BasicCost
    from slam_decomposition_amd.gates import CXGate, CZGate, RiSwapGate, UnitaryGate, iSwapGate
    from slam_decomposition_amd.optimizer import TemplateOptimizer
    from slam_decomposition_amd.sampler import DeviceHaarBatch, HaarBatch

    def same(a, b):
        return all(np.array_equal(getattr(a, f), getattr(b, f)) for f in ("cycles", "Xk", "loss", "gap"))

    hb = HaarBatch(seed0=4100, n_samples=64)
    targets = hb.as_array()
    rng = np.random.default_rng(8)
    # a few targets of smaller circuits among the Haar ones (none of them local)
    mixed = targets.copy()
    mixed[:4] = cr.dress(rng, cr.CX12, 4)
    mixed[4:8] = cr.dress(rng, cr.ISWAP, 4)
    mixed[8:12] = cr.dress(rng, cr.can((0.3, 0.2, 0.0)), 4)
    cost = BasicCost()
    for gate in (CXGate(), iSwapGate(), CZGate(), UnitaryGate(GATES[4][1])):
        res = analytic.cx_decompose(targets, gate)
        assert same(res, analytic.cx_decompose(hb, gate)) and same(res, analytic.cx_decompose(list(targets), gate))
        db = DeviceHaarBatch(seed=5, n_samples=64)
        assert same(analytic.cx_decompose(db, gate), analytic.cx_decompose(db.as_array(), gate))
        assert res.Xk.shape == (64, 24) and len(res) == 64 and res.basis_gate is gate
        assert same(res, analytic.decompose(targets, gate))

        res = analytic.cx_decompose(mixed, gate)
        basis = CircuitTemplate(base_gates=[gate])
        worst = 0.0
        for e, t in zip(res.entries(), mixed):
            assert len(e.Xk) == 6 * (e.cycles + 1) and e.success_label == 1
            basis.build(e.cycles)
            worst = max(worst, cost.unitary_fidelity(basis.eval(e.Xk), t))
        print(f"CX-ANALYTIC api {gate}: sizes {np.bincount(res.cycles, minlength=4)[1:].tolist()} worst BasicCost of the rebuilt circuits {worst:.3g}")
        assert worst <= 1e-13
        assert sorted(set(res.cycles.tolist())) == [1, 2, 3]

        poly = TemplateOptimizer(CircuitTemplate(base_gates=[gate], maximum_span_guess=3, use_polytopes=True), BasicCost(),
                                 training_restarts=16, seed=2)
        data = poly._approximate_batch(list(mixed), log_index=False)
        assert [d.cycles for d in data] == [int(k) for k in res.cycles]
    sq = analytic.decompose(targets, RiSwapGate(1 / 2))
    assert same(sq, analytic.sqiswap_decompose(targets)) and type(sq) is analytic.SqiswapDecomposition
