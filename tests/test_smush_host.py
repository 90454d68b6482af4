"""Parallel-drive ("smush") gates on the host: the gate matrix against a SciPy restatement of hamiltonian.py:114-144, the reduction to
ConversionGainGate, the block form the kernels use, the CircuitTemplateV2(param_vec_expand=...) layout and refusals, and the oracle's
analytic gradient against central differences (no GPU needed)."""
from __future__ import annotations

import numpy as np
import pytest

import smush_ref as R
from slam_decomposition_amd.basisv2 import CircuitTemplateV2, smush_map
from slam_decomposition_amd.gates import ConversionGainGate, ConversionGainSmushGate, RiSwapGate, conversion_gain_matrix, gate_matrix

Q = np.array([[1, 0, 1, 0], [0, 1, 0, 1], [0, 1, 0, -1], [1, 0, -1, 0]]) / np.sqrt(2)  # columns b1 .. b4


def test_host_matrix_matches_expm_restatement():
    rng = np.random.default_rng(0)
    for _ in range(20):
        N = int(rng.integers(1, 7))
        pc, pg, gc, gg, t = rng.uniform(-3, 3, 5)
        gx, gy = rng.uniform(-3, 3, N), rng.uniform(-3, 3, N)
        g = ConversionGainSmushGate(pc, pg, gc, gg, gx, gy, t_el=t)
        assert np.abs(gate_matrix(g) - R.smush_matrix(pc, pg, gc, gg, gx, gy, t)).max() < 1e-13
        assert g.name == "2QSmushGate" and g.xy_len == N and len(g.params) == 5 + 2 * N
        assert np.isclose(g.cost(), (abs(gc) + abs(gg)) * t / (np.pi / 2))


def test_drives_off_is_conversion_gain():
    rng = np.random.default_rng(1)
    for _ in range(10):
        pc, pg, gc, gg, t = rng.uniform(-3, 3, 5)
        g = ConversionGainSmushGate(pc, pg, gc, gg, np.zeros(3), np.zeros(3), t_el=t)
        assert np.abs(gate_matrix(g) - conversion_gain_matrix(pc, pg, gc, gg, t)).max() < 1e-13
        assert np.abs(gate_matrix(g) - gate_matrix(ConversionGainGate(pc, pg, gc, gg, t))).max() < 1e-13


def test_block_form():
    rng = np.random.default_rng(2)
    for pc in (0.0, np.pi):
        for pg in (0.0, np.pi):
            g = ConversionGainSmushGate(pc, pg, *rng.uniform(-2, 2, 2), rng.uniform(-2, 2, 4), rng.uniform(-2, 2, 4), t_el=0.9)
            B = Q.T @ gate_matrix(g) @ Q
            assert np.abs(B[:2, 2:]).max() < 1e-13 and np.abs(B[2:, :2]).max() < 1e-13


@pytest.mark.parametrize("offset", [0, 2])
@pytest.mark.parametrize("vz_only", [False, True])
@pytest.mark.parametrize("no_ext", [False, True])
def test_template_layout(offset, vz_only, no_ext):
    N, k = 4, 3
    fn = ((lambda *v: ConversionGainSmushGate(0, 0, np.pi / 2, 0, v[:N], v[N:], t_el=1)) if offset == 0
          else (lambda *v: ConversionGainSmushGate(0, 0, v[0], v[1], v[2:2 + N], v[2 + N:], t_el=1)))
    b = CircuitTemplateV2(base_gates=[fn], param_vec_expand=[offset, N, N], vz_only=vz_only, no_exterior_1q=no_ext)
    assert b.smush and b.n_gate_params == offset + 2 * N
    b.build(k)
    layers = (k - 1) if no_ext else (k + 1)
    n_p = (2 if vz_only else 6) * layers
    qn = offset + 2 * N
    names = b.parameter_names()
    assert len(names) == n_p + qn * k and names[n_p] == "Q0" and names[-1] == f"Q{qn * k - 1}"
    x = np.arange(len(names), dtype=np.float64)
    assert np.array_equal(b.from_qiskit_order(b.to_qiskit_order(x)), x)
    assert names.index("Q10") < names.index("Q2") or sorted(names).index("Q10") < sorted(names).index("Q2")
    n_dev, idx, *_ = b.device_layout(k)
    assert n_dev == 6 * (k + 1) + qn * k and len(set(idx.tolist())) == len(idx)
    assert np.array_equal(idx[n_p:], 6 * (k + 1) + np.arange(qn * k))
    for name in names:
        if name.startswith("Q"):
            b.add_bound(name, max=2 * np.pi, min=-2 * np.pi)
    assert len(b.parameter_guess()) == len(names)
    gates = b.gates_of(x * 0.01)
    assert len(gates) == k and all(type(g).__name__ == "ConversionGainSmushGate" for g in gates)
    assert np.isclose(b.circuit_cost(x * 0.01), sum(g.cost() for g in gates))


def test_phase_folding_and_map():
    N = 2
    sel = smush_map(lambda *v: ConversionGainSmushGate(np.pi, -np.pi, v[0], v[1], v[2:4], v[4:], t_el=0.5), 6)
    assert sel[0] == N and sel[1] == 0.5 and sel[2][:2] == [0, 1] and sel[3][:2] == [-1.0, -1.0]
    assert sel[2][2:] == [2, 3, 4, 5] and sel[3][2:] == [1.0] * 4


def test_refusals():
    N = 2
    bad = [
        lambda *v: ConversionGainSmushGate(0.3, 0, 1.0, 0.0, v[:N], v[N:], t_el=1),        # non-pi phase
        lambda *v: ConversionGainSmushGate(v[0], 0, 1.0, 0.0, v[:N], v[N:], t_el=1),       # parametric phase
        lambda *v: ConversionGainSmushGate(0, 0, 1.0, 0.0, v[:N], v[N:], t_el=v[0]),       # parametric t
        lambda *v: ConversionGainSmushGate(0, 0, v[0] + v[1], 0.0, v[:N], v[N:], t_el=1),  # two parameters in one value
        lambda *v: ConversionGainSmushGate(0, 0, 1.0, 0.0, np.sin(v[:N]), v[N:], t_el=1),   # not affine
    ]
    for fn in bad:
        with pytest.raises(NotImplementedError):
            CircuitTemplateV2(base_gates=[fn], param_vec_expand=[0, N, N])
    with pytest.raises(NotImplementedError):
        CircuitTemplateV2(param_vec_expand=[1, 2])  # RiSwapGate takes one parameter
    with pytest.raises(AssertionError):
        CircuitTemplateV2(base_gates=[RiSwapGate, RiSwapGate], param_vec_expand=[0, 1, 1])
    fn = lambda *v: ConversionGainSmushGate(0, 0, 1.0, 0.0, v[:N], v[N:], t_el=1)
    with pytest.raises(NotImplementedError):
        CircuitTemplateV2(base_gates=[fn], param_vec_expand=[0, N, N], use_polytopes=True)
    b = CircuitTemplateV2(base_gates=[fn], param_vec_expand=[0, N, N])
    with pytest.raises(NotImplementedError):
        b.set_constraint(1.0)
    b.build(6)  # sqCNOT's row needs six gates
    with pytest.raises(NotImplementedError):
        b.build(7)
    big = CircuitTemplateV2(base_gates=[lambda *v: ConversionGainSmushGate(0, 0, 1.0, 0.0, v[:20], v[20:], t_el=1)], param_vec_expand=[0, 20, 20])
    big.build(2)
    with pytest.raises(NotImplementedError):
        big.build(3)  # 24 + 120 > 128 device parameters
    v2 = CircuitTemplateV2()
    with pytest.raises(NotImplementedError):
        v2.build(6)


def test_oracle_gradient_against_central_differences():
    rng = np.random.default_rng(5)
    T = np.linalg.qr(rng.normal(size=(4, 4)) + 1j * rng.normal(size=(4, 4)))[0]
    N, k = 3, 2
    cases = [(lambda *v: ConversionGainSmushGate(np.pi, 0, v[0], v[1], v[2:2 + N], v[2 + N:], t_el=0.7), 2 + 2 * N, False),
             (lambda *v: ConversionGainSmushGate(0, 0, np.pi / 4, np.pi / 4, v[:N], v[N:], t_el=0.5), 2 * N, True)]
    for fn, qn, zero in cases:
        x = rng.uniform(-2, 2, 6 * (k + 1) + qn * k)
        if zero:
            x[6 * (k + 1):] = 0.0  # w = 0 exactly: gc = gg and no drives
        for square in (False, True):
            _, g, _ = R.loss_grad_unitary(x, fn, qn, k, T, square)
            assert np.abs(g - R.fd_grad(x, fn, qn, k, T, square)).max() < 1e-8
