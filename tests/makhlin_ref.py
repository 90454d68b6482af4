"""NumPy restatement of MakhlinFunctionalCost for the tests, written in the MAGIC-BASIS form of weylchamber (W_B = Q^+ W Q,
m = W_B^T W_B) -- not the Y = sigma_y (x) sigma_y form the library and its kernels use (Q Q^T = -Y makes the two equal).

  G1 = tr(m)^2 / (16 det W),  G2 = (tr(m)^2 - tr(m^2)) / (4 det W),  g = (Re G1, Im G1, Re G2),  J(W; T) = |g(W) - g(T)|^2

The analytic gradient uses the adjoint seed S with dJ = Re Tr(S dW) (for unitary W), built here from the magic-basis derivatives
  d tr m = Tr(2 Q W_B^T Q^+ dW),  d tr m^2 = Tr(4 Q m W_B^T Q^+ dW),  d det W = det W Tr(W^+ dW).
"""
import numpy as np

from oracle import slam_oracle as o

Q = np.array([[1, 0, 0, 1j], [0, 1j, 1, 0], [0, 1j, -1, 0], [1, 0, 0, -1j]], dtype=np.complex128) / np.sqrt(2)

SWAP = np.array([[1, 0, 0, 0], [0, 0, 1, 0], [0, 1, 0, 0], [0, 0, 0, 1]], dtype=np.complex128)


def _G(W):
    W = np.asarray(W, dtype=np.complex128)
    WB = Q.conj().T @ W @ Q
    m = WB.T @ WB
    d = np.linalg.det(W)
    t = np.trace(m)
    return t * t / (16 * d), (t * t - np.trace(m @ m)) / (4 * d), m, WB, d


def g_magic(W) -> np.ndarray:
    G1, G2, _, _, _ = _G(W)
    return np.array([G1.real, G1.imag, G2.real])


def J(W, T) -> float:
    dg = g_magic(W) - g_magic(T)
    return float(dg @ dg)


def seed(W, T) -> np.ndarray:
    """S with dJ = Re Tr(S dW) along unitary directions."""
    G1, G2, m, WB, d = _G(W)
    dg = g_magic(W) - g_magic(T)
    t = np.trace(m)
    S_tr = 2 * Q @ WB.T @ Q.conj().T
    S_tr2 = 4 * Q @ m @ WB.T @ Q.conj().T
    Wh = np.asarray(W).conj().T
    S_G1 = 2 * t * S_tr / (16 * d) - G1 * Wh
    S_G2 = (2 * t * S_tr - S_tr2) / (4 * d) - G2 * Wh
    return (2 * dg[0] - 2j * dg[1]) * S_G1 + 2 * dg[2] * S_G2


def loss_and_grad(x, gate_seq, T):
    """J(CircuitTemplate.eval(x); T) and its analytic gradient (prefix / suffix products as oracle.loss_and_grad)."""
    k = len(gate_seq)
    x = np.asarray(x, dtype=np.float64)
    Ks = [o.layer_matrix(x[6 * j : 6 * j + 6]) for j in range(k + 1)]
    right = [np.eye(4, dtype=np.complex128)]
    for j in range(1, k + 1):
        right.append(gate_seq[j - 1] @ Ks[j - 1] @ right[j - 1])
    left = [None] * (k + 1)
    left[k] = np.eye(4, dtype=np.complex128)
    for j in range(k - 1, -1, -1):
        left[j] = left[j + 1] @ Ks[j + 1] @ gate_seq[j]
    W = Ks[k] @ right[k]
    S = seed(W, T)
    grad = np.zeros(6 * (k + 1))
    for j in range(k + 1):
        E = right[j] @ S @ left[j]  # Tr(S L dK R) = Tr(E dK)
        A = o.u3(*x[6 * j + 3 : 6 * j + 6])
        B = o.u3(*x[6 * j : 6 * j + 3])
        dB = o._du3(*x[6 * j : 6 * j + 3])
        dA = o._du3(*x[6 * j + 3 : 6 * j + 6])
        for mm in range(3):
            grad[6 * j + mm] = np.real(np.trace(E @ np.kron(A, dB[mm])))
            grad[6 * j + 3 + mm] = np.real(np.trace(E @ np.kron(dA[mm], B)))
    return J(W, T), grad


def fd_grad(x, gate_seq, T, h=1e-6) -> np.ndarray:
    x = np.asarray(x, dtype=np.float64)
    g = np.zeros_like(x)
    for i in range(x.size):
        e = np.zeros_like(x)
        e[i] = h
        g[i] = (J(o.template_eval(x + e, gate_seq), T) - J(o.template_eval(x - e, gate_seq), T)) / (2 * h)
    return g


def random_local(rng) -> np.ndarray:
    """A random single-qubit product U3 (x) U3."""
    return np.kron(o.u3(*rng.uniform(0, 2 * np.pi, 3)), o.u3(*rng.uniform(0, 2 * np.pi, 3)))
