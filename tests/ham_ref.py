"""Host model of the Hamiltonian templates (csrc/slam_ham.hpp), the literal definition: H from the term operators, numpy.linalg.eigh,
the loss, and the gradient by the divided-difference formula

    z = Tr(T^+ exp(-i t H)) / d,   B = V^+ T^+ V,   Phi_ab = exp(-i t (l_a + l_b) / 2) sinc(t (l_a - l_b) / 2),   K = V (B o Phi) V^+,
    dz/dx_j = (-i t / d) Tr(K dH/dx_j),   dz/dt = (1 / d) sum_a B_aa (-i l_a) exp(-i t l_a).

BasicCost = 1 - |z|; SquareCost = d (2 L - L^2) / (d + 1) of BasicCost L (= 1 - (|Tr|^2 + d) / (d (d + 1)))."""
import numpy as np


def hamiltonian(terms, x):
    x = np.asarray(x, dtype=np.float64)
    d = int(terms["dim"])
    h = np.zeros((d, d), dtype=np.complex128)
    for m, s, p in zip(terms["matrices"], terms["s_index"], terms["phi_index"]):
        c = x[s] * np.exp(1j * (x[p] if p >= 0 else 0.0))
        h += c * m + np.conj(c) * m.conj().T
    return h


def time_of(terms, x):
    return float(x[terms["t_index"]]) if terms["t_index"] >= 0 else 1.0


def unitary(terms, x):
    w, v = np.linalg.eigh(hamiltonian(terms, x))
    return (v * np.exp(-1j * time_of(terms, x) * w)) @ v.conj().T


def cost_of_z(az, d, square):
    basic = 1.0 - az
    return d * (2.0 * basic - basic * basic) / (d + 1.0) if square else basic


def loss_grad(terms, x, target, square=False):
    """(loss, gradient [n], U) at x for one dim x dim target (any finite matrix)."""
    x = np.asarray(x, dtype=np.float64)
    d = int(terms["dim"])
    n = int(terms["n_params"])
    t = time_of(terms, x)
    lam, v = np.linalg.eigh(hamiltonian(terms, x))
    e = np.exp(-1j * t * lam)
    u = (v * e) @ v.conj().T
    b = v.conj().T @ np.asarray(target, dtype=np.complex128).conj().T @ v
    z = np.sum(np.diag(b) * e) / d
    az = abs(z)
    loss = cost_of_z(az, d, square)
    # d loss = Re(sigma dz)
    dl = (2.0 * d * az / (d + 1.0)) if square else 1.0  # -d loss / d|z|
    sigma = -dl * np.conj(z) / az if az > 0.0 else 0.0
    half_sum = 0.5 * t * (lam[:, None] + lam[None, :])
    half_dif = 0.5 * t * (lam[:, None] - lam[None, :])
    phi = np.exp(-1j * half_sum) * np.sinc(half_dif / np.pi)
    k = v @ (b * phi) @ v.conj().T
    g = np.zeros(n)
    for m, s, p in zip(terms["matrices"], terms["s_index"], terms["phi_index"]):
        ph = np.exp(1j * (x[p] if p >= 0 else 0.0))
        dh_s = ph * m + np.conj(ph) * m.conj().T
        g[s] += np.real(sigma * (-1j * t / d) * np.trace(k @ dh_s))
        if p >= 0:
            dh_p = 1j * x[s] * ph * m
            dh_p = dh_p + dh_p.conj().T
            g[p] += np.real(sigma * (-1j * t / d) * np.trace(k @ dh_p))
    if terms["t_index"] >= 0:
        g[terms["t_index"]] += np.real(sigma * np.sum(np.diag(b) * (-1j * lam) * e) / d)
    return loss, g, u


def batch(terms, xs, targets, target_of, square=False):
    out = [loss_grad(terms, xs[m], targets[target_of[m]], square) for m in range(len(xs))]
    return np.array([o[0] for o in out]), np.stack([o[1] for o in out]), np.stack([o[2] for o in out])
