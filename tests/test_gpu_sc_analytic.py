"""GPU: ``sc_decompose_kernel`` (slam_sc_decompose), ``sc_counts_kernel`` (slam_sc_counts) and ``analytic.sc_decompose`` with the
dispatch on top of them (csrc/slam_sc.hpp; the yardstick is tests/sc_ref.py, which tests/test_sc_analytic_host.py holds to its targets
on the CPU).

The basis gates: CAN(1/2, beta, 0) for beta in {1e-3, 1/8, 0.3, 0.45, 1/2 - 1e-3}, bare and dressed with fixed random local gates.  The
batch: the 256 targets of ``DeviceHaarBatch(seed=7)``, then identity, a random local gate, CX, iSWAP, SWAP, B, CAN(0.3, 0.2, 0),
CAN(0.3, 0.2, 1e-9), CAN(0.3, 0.2, 2e-8), CAN(1/2, 0.3, -0.1) and its c1 > 1/2 neighbour CAN(0.7, 0.2, 0.1) (dressed with local gates),
then the gate itself and a dressed copy of it.  No target is left out of a size comparison: the seed is one at which the model's two
largest E_k differ by at least 1e-9 on all 256 Haar targets for every gate and fidelity here (2.2e-6 on the CPU port of the sampler;
asserted on the device's targets below).

Bounds, those ``tests/test_gpu_cx_analytic.py`` holds its family to: loss <= 1e-13 and gap <= 1e-12 where the chosen size is exact (the
target 1e-9 off the plane c3 = 0 gets two gates, within the exact tie of cos: its gap is that 1e-9), |loss - loss of the row through
``slam_eval_unitary``| <= 1e-14.  With a forced size: predicted = the model on the device's own unrounded coordinates to 1e-14,
realised loss = predicted to 1e-13.

Measured on an MI355X (``SC`` lines with ``-s``), worst over the ten basis gates: f = 1 sizes [2, 2, 5, 260], loss
1.1e-15, gap 5.6e-16, |loss - loss2| 1.0e-15, smallest Haar margin 2.3e-6; forced sizes |predicted - model| 3.3e-16, |loss - predicted|
1.1e-15; beta = 1/4: sizes [2, 3, 4, 260] against ``b_decompose``'s [0, 3, 266, 0].
"""
import numpy as np
import pytest

import kak_ref as kr
import sc_ref as sr

pytestmark = pytest.mark.gpu

BETAS = (1e-3, 1 / 8, 0.3, 0.45, 0.5 - 1e-3)
N_HAAR = 256
FIDELITIES = (0.999, 0.99, 0.9)
BLOCK = 64  # kKakBlock


def _gates():
    rng = np.random.default_rng(20)
    out = []
    for beta in BETAS:
        g = sr.can((0.5, beta, 0.0))
        out += [(f"beta {beta:g}", beta, g), (f"dressed beta {beta:g}", beta, sr.dress(rng, g))]
    return out


GATES = _gates()
GATE_IDS = [g[0] for g in GATES]
NAMED = (("identity", None), ("local", None), ("CX", (0.5, 0.0, 0.0)), ("iSWAP", (0.5, 0.5, 0.0)), ("SWAP", (0.5, 0.5, 0.5)),
         ("B", (0.5, 0.25, 0.0)), ("CAN(0.3, 0.2, 0)", (0.3, 0.2, 0.0)), ("CAN(0.3, 0.2, 1e-9)", (0.3, 0.2, 1e-9)),
         ("CAN(0.3, 0.2, 2e-8)", (0.3, 0.2, 2e-8)), ("CAN(0.5, 0.3, -0.1)", (0.5, 0.3, -0.1)), ("CAN(0.7, 0.2, 0.1)", (0.7, 0.2, 0.1)))
NAMES = [n for n, _ in NAMED] + ["G", "dressed G"]
SIZE_AT_1 = {"identity": 0, "local": 0, "CX": 2, "iSWAP": 2, "SWAP": 3, "B": 2, "CAN(0.3, 0.2, 0)": 2, "CAN(0.3, 0.2, 1e-9)": 2,
             "CAN(0.3, 0.2, 2e-8)": 3, "CAN(0.5, 0.3, -0.1)": 3, "CAN(0.7, 0.2, 0.1)": 3, "G": 1, "dressed G": 1}
NEAR_THE_PLANE = NAMES.index("CAN(0.3, 0.2, 1e-9)")


@pytest.fixture(scope="module")
def common(hip_ctx):
    """The gate-independent part of the batch, once for all tests: [256 + 11, 4, 4]."""
    from slam_decomposition_amd.sampler import DeviceHaarBatch

    DeviceHaarBatch(seed=7, n_samples=N_HAAR).fill(hip_ctx)
    haar = hip_ctx.get_targets(0, N_HAAR)
    rng = np.random.default_rng(21)
    named = []
    for name, c in NAMED:
        if name == "identity":
            named.append(np.eye(4, dtype=np.complex128))
        elif name == "local":
            named.append(kr.kron2(kr.random_su2(rng, 1), kr.random_su2(rng, 1))[0])
        else:
            named.append(sr.dress(rng, sr.can(c)))
    return np.concatenate([haar, np.stack(named)])


def _batch(common, G):
    """(targets [256 + 13, 4, 4], 8-digit coordinates)."""
    T = np.concatenate([common, np.stack([G, sr.dress(np.random.default_rng(22), G)])])
    return T, sr.coordinates(T)


def _reevaluate(ctx, G, x, cycles, T):
    """The loss of every row again: sizes 1..3 through ``ctx.eval_unitary`` with the gate table [G] (the resident targets are the
    rows' own), a row of no gate multiplied out by the oracle."""
    ctx.set_gates(np.asarray(G)[None])
    ctx.set_cost(0)
    loss2 = np.zeros(len(x))
    for k in (1, 2, 3):
        idx = np.flatnonzero(cycles == k)
        if len(idx):
            loss2[idx] = ctx.eval_unitary([0] * k, x[idx, : 6 * (k + 1)], idx)[1]
    for i in np.flatnonzero(cycles == 0):
        loss2[i] = sr.row_loss(x[i], G, 0, T[i])
    return loss2


@pytest.mark.parametrize("gname,beta,G", GATES, ids=GATE_IDS)
def test_exact_mode(hip_ctx, common, gname, beta, G):
    T, c = _batch(common, G)
    hip_ctx.set_targets(T)
    x, cycles, loss, predicted, gap = hip_ctx.sc_decompose(G)
    assert np.all(np.isfinite(x)) and np.all(np.isfinite(loss)) and np.all(np.isfinite(gap))
    margin = sr.tie_margin(c[:N_HAAR], beta, 1.0)
    assert margin.min() >= 1e-9  # no Haar target is left out
    want = sr.select(c, beta, 1.0)
    assert np.array_equal(cycles[:N_HAAR], want[:N_HAAR]) and np.all(cycles[:N_HAAR] == 3)
    for i, name in enumerate(NAMES):
        assert cycles[N_HAAR + i] == want[N_HAAR + i] == SIZE_AT_1[name], (name, cycles[N_HAAR + i], want[N_HAAR + i])
    for k in range(4):
        assert not np.any(x[cycles == k, 6 * (k + 1):])  # zeros behind the row
    loss2 = _reevaluate(hip_ctx, G, x, cycles, T)
    exact = np.ones(len(T), dtype=bool)
    exact[N_HAAR + NEAR_THE_PLANE] = False
    print(f"SC {gname:<22s} f = 1: sizes {np.bincount(cycles, minlength=4).tolist()} worst loss {loss.max():.3g} gap {gap[exact].max():.3g} "
          f"|loss - loss2| {np.abs(loss - loss2).max():.3g} smallest margin {margin.min():.3g}")
    assert loss.max() <= 1e-13
    assert gap[exact].max() <= 1e-12
    assert abs(gap[N_HAAR + NEAR_THE_PLANE] - 1e-9) <= 1e-12
    assert np.abs(loss - loss2).max() <= 1e-14
    assert not np.any(predicted)
    for i in (0, N_HAAR - 1, len(T) - 1):  # ... and by the NumPy oracle
        assert abs(sr.row_loss(x[i], G, int(cycles[i]), T[i]) - loss[i]) <= 1e-14


@pytest.mark.parametrize("gname,beta,G", GATES, ids=GATE_IDS)
def test_fidelity_mode(hip_ctx, common, gname, beta, G):
    from slam_decomposition_amd import analytic

    T, c = _batch(common, G)
    hip_ctx.set_targets(T)
    cu = hip_ctx.targets_kak().c  # the kernel's own unrounded coordinates
    assert np.abs(cu[:N_HAAR] - c[:N_HAAR]).max() <= 1e-8
    rows = []
    for k in range(4):
        model = sr.predicted_loss(cu, beta, k)
        x, cycles, loss, predicted, gap = hip_ctx.sc_decompose(G, 0.99, k)
        assert np.all(cycles == k) and not np.any(x[:, 6 * (k + 1):])
        d_model, d_real = np.abs(predicted - model).max(), np.abs(loss - predicted).max()
        print(f"SC {gname:<22s} k = {k}: worst |predicted - model| {d_model:.3g} |loss - predicted| {d_real:.3g} worst loss {loss.max():.3g}")
        assert d_model <= 1e-14, (k, int(np.argmax(np.abs(predicted - model))))
        assert d_real <= 1e-13, (k, int(np.argmax(np.abs(loss - predicted))))
        for f in FIDELITIES:  # a forced size does not depend on the fidelity
            again = hip_ctx.sc_decompose(G, f, k)
            assert np.array_equal(again[0], x) and np.array_equal(again[2], loss) and np.array_equal(again[3], predicted)
        rows.append(loss)
    fid = np.array(FIDELITIES)
    counts, fidsum = hip_ctx.sc_counts(G, fid)
    again = hip_ctx.sc_counts(G, fid)
    assert np.array_equal(counts, again[0]) and np.array_equal(fidsum, again[1])
    for j, f in enumerate(FIDELITIES):
        res = analytic.sc_decompose(T, G, f)
        assert sr.tie_margin(c[:N_HAAR], beta, f).min() >= 1e-9
        assert np.array_equal(res.cycles[:N_HAAR], sr.select(c, beta, f)[:N_HAAR])
        assert np.array_equal(res.cycles, sr.select(cu, beta, f))
        best = np.max([(4.0 + 16.0 * (1.0 - rows[k]) ** 2) / 20.0 * f ** k for k in range(4)], axis=0)
        # the realised loss is the predicted one to 1e-13, so F = 0.2 + 0.8 t^2 is the best one to 1.6e-13
        assert np.abs(res.expected_fidelity - best).max() <= 2e-13
        assert np.array_equal(counts[j], np.bincount(res.cycles, minlength=4)), (f, counts[j])
        assert abs(fidsum[j] / 2.0 ** 32 / len(T) - res.expected_fidelity.mean()) <= 1e-9
        sw = analytic.fidelity_sweep(T, G, [f])
        assert np.array_equal(sw.counts[0], counts[j])
        assert np.array_equal(analytic.approx_decompose(T, G, f).cycles, res.cycles)
    print(f"SC {gname:<22s} sweep: average gates {(counts @ np.arange(4) / len(T)).round(4).tolist()}")


def test_consistency_with_the_named_families(hip_ctx, common):
    from slam_decomposition_amd import analytic
    from slam_decomposition_amd.gates import BerkeleyGate, CXGate, gate_matrix, iSwapGate

    for gate in (CXGate(), iSwapGate()):
        T, _ = _batch(common, gate_matrix(gate))
        for f in (1.0, 0.99, 0.9):
            ours, theirs = analytic.sc_decompose(T, gate, f), analytic.approx_decompose(T, gate, f)
            assert np.array_equal(ours.cycles, theirs.cycles), (gate, f)
            assert np.abs(ours.loss - theirs.loss).max() <= 1e-13
    # beta = 1/4: two B gates reach everything, this formula's two gates the plane c3 = 0 only -- never fewer gates than b_decompose
    # on a non-local target (which b_decompose gives two gates, this one none), and exact all the same
    gate = BerkeleyGate()
    T, _ = _batch(common, gate_matrix(gate))
    ours, theirs = analytic.sc_decompose(T, gate), analytic.b_decompose(T, gate)
    local = np.zeros(len(T), dtype=bool)
    local[[N_HAAR + NAMES.index("identity"), N_HAAR + NAMES.index("local")]] = True
    assert np.all(ours.cycles[~local] >= theirs.cycles[~local]) and np.all(ours.cycles[local] == 0)
    assert np.all(ours.cycles[:N_HAAR] == 3) and np.all(theirs.cycles[:N_HAAR] == 2)
    assert ours.loss.max() <= 1e-13
    print(f"SC beta 1/4: sizes {np.bincount(ours.cycles, minlength=4).tolist()} against b_decompose's "
          f"{np.bincount(theirs.cycles, minlength=4).tolist()}, worst loss {ours.loss.max():.3g}")


@pytest.mark.parametrize("gname,beta,G", [GATES[5]], ids=[GATE_IDS[5]])
def test_windows_and_refusals(hip_ctx, gname, beta, G):
    from slam_decomposition_amd import _ffi

    n = 300
    hip_ctx.sample_haar(11, n)
    full = hip_ctx.sc_decompose(G, 0.99)
    for a, b in zip(full, hip_ctx.sc_decompose(G, 0.99)):
        assert np.array_equal(a, b)
    lib, h = hip_ctx._lib, hip_ctx._h
    g, dress = _ffi.sc_dress(G)
    gp, dp = _ffi._ptr(g), _ffi._ptr(dress)
    poison = -7.25
    first = 7
    for count in (1, BLOCK - 1, BLOCK, BLOCK + 1):
        out = [np.full((count + 2, 24), poison), np.full(count + 2, -7, dtype=np.int32)] + [np.full(count + 2, poison) for _ in range(3)]
        _ffi._check(lib.slam_sc_decompose(h, first, count, gp, dp, 0.99, -1, *[_ffi._ptr(a) for a in out]))
        for a, b in zip(full, out):
            assert np.array_equal(a[first:first + count], b[:count]), count
            assert np.all(b[count:] == (-7 if b.dtype == np.int32 else poison)), count  # nothing behind the window
    # every output is optional
    fid = np.array([0.9, 1.0])
    for keep in range(-1, 5):
        out = [np.zeros((8, 24)), np.zeros(8, dtype=np.int32), np.zeros(8), np.zeros(8), np.zeros(8)]
        ptrs = [_ffi._ptr(a) if j == keep else None for j, a in enumerate(out)]
        assert lib.slam_sc_decompose(h, first, 8, gp, dp, 0.99, -1, *ptrs) == 0
        if keep >= 0:
            assert np.array_equal(out[keep], full[keep][first:first + 8])
    assert lib.slam_sc_decompose(h, 0, 0, gp, dp, 0.99, -1, *(None,) * 5) == 0
    assert lib.slam_sc_counts(h, 0, 8, gp, dp, 2, _ffi._ptr(fid), None, None) == 0
    x, cycles, loss, predicted, gap = hip_ctx.sc_decompose(G, 0.9, None, 5, 0)
    assert x.shape == (0, 24) and len(cycles) == 0 and len(predicted) == 0
    counts, fidsum = hip_ctx.sc_counts(G, fid, 5, 0)
    assert not counts.any() and not fidsum.any()
    wc, ws = hip_ctx.sc_counts(G, np.array([0.99]), first, BLOCK + 1)
    assert np.array_equal(wc[0], np.bincount(full[1][first:first + BLOCK + 1], minlength=4))
    # refusals: nothing is written
    out = [np.zeros((8, 24)), np.zeros(8, dtype=np.int32), np.zeros(8), np.zeros(8), np.zeros(8)]
    ptrs = [_ffi._ptr(a) for a in out]
    off, corrupt = dress.copy(), dress.copy()
    off[32] = 0.5 - 1e-6
    corrupt[8 * 2 + 3] += 1e-9
    other = np.ascontiguousarray(sr.dress(np.random.default_rng(3), g))
    good = (0, 8, gp, dp, 0.99, -1)
    for bad in ((n - 4, 8) + good[2:], (-1, 2) + good[2:], (0, n + 1) + good[2:],                       # windows
                good[:4] + (0.0, -1), good[:4] + (1.5, -1), good[:4] + (float("nan"), -1),               # fidelities
                good[:5] + (4,), good[:5] + (-2,),                                                        # sizes
                good[:3] + (_ffi._ptr(off),) + good[4:], good[:3] + (_ffi._ptr(corrupt),) + good[4:],    # off the line, a corrupted dress
                good[:2] + (_ffi._ptr(other),) + good[3:], good[:2] + (None,) + good[3:]):               # another gate, no gate
        with pytest.raises(_ffi.SlamHipError) as e:
            _ffi._check(lib.slam_sc_decompose(h, *bad, *ptrs))
        assert e.value.code == -1
    assert not any(np.any(a) for a in out)
    cbuf, sbuf = np.zeros((2, 4), dtype=np.int64), np.zeros(2, dtype=np.int64)
    for bad in ((n - 4, 8, gp, dp, 2), (0, 8, gp, _ffi._ptr(off), 2), (0, 8, gp, dp, 0), (0, 8, gp, dp, 65)):
        with pytest.raises(_ffi.SlamHipError) as e:
            _ffi._check(lib.slam_sc_counts(h, *bad, _ffi._ptr(np.full(65, 0.9)), _ffi._ptr(cbuf), _ffi._ptr(sbuf)))
        assert e.value.code == -1
    assert not cbuf.any() and not sbuf.any()
    with pytest.raises(ValueError):  # a gate off the line never reaches the library
        hip_ctx.sc_decompose(sr.can((0.25, 0.25, 0.0)))
    with pytest.raises(ValueError):
        hip_ctx.sc_decompose(G, 0.9, 4)


def test_circuits_through_the_api(hip_ctx, common):
    from slam_decomposition_amd import analytic
    from slam_decomposition_amd.basis import CircuitTemplate
    from slam_decomposition_amd.cost_function import BasicCost
    from slam_decomposition_amd.gates import ConversionGainGate, UnitaryGate
    from slam_decomposition_amd.sampler import DeviceHaarBatch

    cost = BasicCost()
    sub = np.concatenate([common[:8], common[N_HAAR + 2:N_HAAR + 10]])  # 8 Haar targets, CX .. CAN(0.5, 0.3, -0.1)
    cg = ConversionGainGate(0.0, 0.0, 0.4 * np.pi, 0.1 * np.pi, 1.0)  # gc + gg = pi / 2: the class (1/2, 0.3, 0)
    for gate in (cg, UnitaryGate(GATES[3][2])):
        for res in (analytic.decompose(sub, gate), analytic.sc_decompose(sub, gate, 0.999)):
            assert isinstance(res, analytic.ApproxDecomposition) and res.basis_gate is gate and len(res) == 16
            basis = CircuitTemplate(base_gates=[gate])
            for e, t, k in zip(res.entries(), sub, res.cycles):
                assert e.cycles == k >= 1 and len(e.Xk) == 6 * (k + 1)
                basis.build(e.cycles)
                again = cost.unitary_fidelity(basis.eval(e.Xk), t)
                assert abs(again - e.loss_result) <= 1e-14
                if res.basis_fidelity == 1.0:
                    assert again <= 1e-13 and e.success_label == 1
    db = DeviceHaarBatch(seed=5, n_samples=300)
    a, b = analytic.sc_decompose(db, cg, 0.97), analytic.sc_decompose(db.as_array(), cg, 0.97)
    assert all(np.array_equal(getattr(a, n), getattr(b, n)) for n in ("cycles", "Xk", "loss", "gap", "predicted_loss"))
    sw = analytic.fidelity_sweep(db, cg, [0.97, 1.0])
    assert np.array_equal(sw.counts[0], np.bincount(a.cycles, minlength=4)) and sw.n_targets == 300
    assert abs(sw.average_fidelity[0] - a.expected_fidelity.mean()) <= 1e-9 and abs(sw.average_fidelity[1] - 1.0) <= 1e-9
    assert sw.average_gates[1] == 3.0
