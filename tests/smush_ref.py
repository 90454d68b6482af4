"""NumPy / SciPy oracle for parallel-drive ("smush") templates: CircuitTemplateV2(param_vec_expand=...) with
ConversionGainSmushGate (reference: src/slam/utils/gates/custom_gates.py:215-257, hamiltonian.py:114-144).

Restated independently of the block form the kernels use: every time slice is ``scipy.linalg.expm`` of the full 4x4
Hamiltonian, and the gradient with respect to a pulse value is the Frechet derivative of that exponential
(``scipy.linalg.expm_frechet``) pushed through the template by left / right products.  The derivative of a raw pulse value
with respect to the gate's parameters is read off the gate callable (affine maps: a unit step is exact).
"""
from __future__ import annotations

import numpy as np
import scipy.linalg as sla

from oracle import slam_oracle as o
from oracle.v2_oracle import template_eval  # noqa: F401  (re-exported for the tests)

_a = np.array([[0, 0], [1, 0]], dtype=np.complex128)  # qutip.create(2)
A = np.kron(_a, np.eye(2))
B = np.kron(np.eye(2), _a)


def dH_terms(pc: float, pg: float):
    """dH/dgc, dH/dgg, dH/dgx, dH/dgy (hamiltonian.py:114-144)."""
    conv = np.exp(1j * pc) * A @ B.conj().T
    gain = np.exp(1j * pg) * A @ B
    return conv + conv.conj().T, gain + gain.conj().T, A + A.conj().T, B + B.conj().T


def hamiltonian(pc, pg, gc, gg, gx, gy) -> np.ndarray:
    Hc, Hg, Hx, Hy = dH_terms(pc, pg)
    return gc * Hc + gg * Hg + gx * Hx + gy * Hy


def smush_matrix(pc, pg, gc, gg, gx, gy, t) -> np.ndarray:
    """U_{N-1} ... U_0, U_s = expm(-i t / N H_s)."""
    N = len(gx)
    U = np.eye(4, dtype=np.complex128)
    for s in range(N):
        U = sla.expm(-1j * (t / N) * hamiltonian(pc, pg, gc, gg, gx[s], gy[s])) @ U
    return U


def gate_values(gate):
    """(pc, pg, gc, gg, gx, gy, t) of a ConversionGainSmushGate (params [pc, pg, gc, gg, *gx, *gy, t])."""
    p = [float(v) for v in gate.params]
    N = int(gate.xy_len)
    return p[0], p[1], p[2], p[3], np.array(p[4 : 4 + N]), np.array(p[4 + N : 4 + 2 * N]), p[-1]


def gate_matrix_and_raw_grads(gate):
    """G and dG / d(gc, gg, gx[0..N), gy[0..N)) of one smush gate, by Frechet derivatives of the slice exponentials."""
    pc, pg, gc, gg, gx, gy, t = gate_values(gate)
    N = len(gx)
    tau = t / N
    Hc, Hg, Hx, Hy = dH_terms(pc, pg)
    S = [sla.expm(-1j * tau * hamiltonian(pc, pg, gc, gg, gx[s], gy[s])) for s in range(N)]
    pre = [np.eye(4, dtype=np.complex128)]  # pre[s] = S_{s-1} .. S_0
    for s in range(N):
        pre.append(S[s] @ pre[s])
    suf = [None] * (N + 1)  # suf[s] = S_{N-1} .. S_{s}
    suf[N] = np.eye(4, dtype=np.complex128)
    for s in range(N - 1, -1, -1):
        suf[s] = suf[s + 1] @ S[s]
    dG = np.zeros((2 + 2 * N, 4, 4), dtype=np.complex128)
    for s in range(N):
        Hs = -1j * tau * hamiltonian(pc, pg, gc, gg, gx[s], gy[s])
        for r, E in ((0, Hc), (1, Hg), (2 + s, Hx), (2 + N + s, Hy)):
            _, dS = sla.expm_frechet(Hs, -1j * tau * E)
            dG[r] += suf[s + 1] @ dS @ pre[s]
    return pre[N], dG


def raw_values(gate) -> np.ndarray:
    pc, pg, gc, gg, gx, gy, t = gate_values(gate)
    return np.concatenate([[gc, gg], gx, gy])


def raw_jacobian(gate_fn, q) -> np.ndarray:
    """d raw / d q of an affine gate callable (a unit step per parameter)."""
    q = np.asarray(q, dtype=np.float64)
    r0 = raw_values(gate_fn(*q))
    J = np.zeros((r0.size, q.size))
    for m in range(q.size):
        e = np.zeros(q.size)
        e[m] = 1.0
        J[:, m] = raw_values(gate_fn(*(q + e))) - r0
    return J


def cost(W, target, square):
    return o.square_cost(W, target) if square else o.basic_cost(W, target)


def loss_grad_unitary(x_dev, gate_fn, qn: int, k: int, target, square=False):
    """Loss, analytic gradient (device order: 6 (k + 1) U-gate angles, then qn parameters per gate) and W of a smush template."""
    x = np.asarray(x_dev, dtype=np.float64)
    n_p = 6 * (k + 1)
    assert x.size == n_p + qn * k
    qs = [x[n_p + qn * j : n_p + qn * (j + 1)] for j in range(k)]
    gates = [gate_fn(*q) for q in qs]
    GdG = [gate_matrix_and_raw_grads(g) for g in gates]
    Ks = [o.layer_matrix(x[6 * j : 6 * j + 6]) for j in range(k + 1)]
    right = [np.eye(4, dtype=np.complex128)]  # right[j] = G_j K_{j-1} ... K_0 (right[0] = 1)
    for j in range(1, k + 1):
        right.append(GdG[j - 1][0] @ Ks[j - 1] @ right[j - 1])
    left = [None] * (k + 1)  # left[j] = K_k G_k ... G_{j+1} (left[k] = 1)
    left[k] = np.eye(4, dtype=np.complex128)
    for j in range(k - 1, -1, -1):
        left[j] = left[j + 1] @ Ks[j + 1] @ GdG[j][0]
    W = Ks[k] @ right[k]
    Th = np.asarray(target).conj().T
    t = np.trace(Th @ W)
    at = abs(t)
    basic = 1.0 - at / 4.0
    scale = 1.6 * (1.0 - basic) if square else 1.0

    def dl(dW):
        return scale * (-np.real(np.conj(t) * np.trace(Th @ dW)) / (4.0 * at))

    grad = np.zeros(x.size)
    for j in range(k + 1):
        xs = x[6 * j : 6 * j + 6]
        Am, Bm = o.u3(*xs[3:6]), o.u3(*xs[0:3])
        dB, dA = o._du3(*xs[0:3]), o._du3(*xs[3:6])
        for m in range(3):
            grad[6 * j + m] = dl(left[j] @ np.kron(Am, dB[m]) @ right[j])
            grad[6 * j + 3 + m] = dl(left[j] @ np.kron(dA[m], Bm) @ right[j])
    for j in range(1, k + 1):
        pre, post = left[j] @ Ks[j], Ks[j - 1] @ right[j - 1]
        draw = np.array([dl(pre @ dGr @ post) for dGr in GdG[j - 1][1]])
        grad[n_p + qn * (j - 1) : n_p + qn * j] = draw @ raw_jacobian(gate_fn, qs[j - 1])
    return float(cost(W, target, square)), grad, W


def loss_only(x_dev, gate_fn, qn, k, target, square=False) -> float:
    x = np.asarray(x_dev, dtype=np.float64)
    n_p = 6 * (k + 1)
    mats = [np.asarray(gate_fn(*x[n_p + qn * j : n_p + qn * (j + 1)])) for j in range(k)]
    W = o.layer_matrix(x[0:6])
    for j in range(k):
        W = o.layer_matrix(x[6 * (j + 1) : 6 * (j + 2)]) @ mats[j] @ W
    return float(cost(W, target, square))


def fd_grad(x_dev, gate_fn, qn, k, target, square=False, h=1e-6) -> np.ndarray:
    x = np.asarray(x_dev, dtype=np.float64)
    g = np.zeros_like(x)
    for i in range(x.size):
        e = np.zeros_like(x)
        e[i] = h
        g[i] = (loss_only(x + e, gate_fn, qn, k, target, square) - loss_only(x - e, gate_fn, qn, k, target, square)) / (2 * h)
    return g
