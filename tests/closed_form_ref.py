"""What the test-side restatements of the closed-form decompositions (tests/analytic_ref.py, tests/cx_ref.py, tests/b_ref.py) define
word for word alike, in NumPy; each of them re-exports these names.  Nothing is shared with csrc/.

Conventions: kron(a, b) puts a on the high bit; CAN(c) = exp(i pi/2 (c1 XX + c2 YY + c3 ZZ)).  A template row holds six angles per
layer: U3(theta, phi, lam) of qubit 0 (the low bit), then of qubit 1.
"""
from __future__ import annotations

import numpy as np

_I = np.eye(2, dtype=np.complex128)
_X = np.array([[0, 1], [1, 0]], dtype=np.complex128)
_Y = np.array([[0, -1j], [1j, 0]], dtype=np.complex128)
_Z = np.array([[1, 0], [0, -1]], dtype=np.complex128)
_PP = [np.kron(p, p) for p in (_X, _Y, _Z)]
SIZE_TOL = 2e-8  # span_rules._TOL: the size rule is evaluated on coordinates rounded to 8 digits


def can(c) -> np.ndarray:
    out = np.eye(4, dtype=np.complex128)
    for j in range(3):
        a = 0.5 * np.pi * c[j]
        out = out @ (np.cos(a) * np.eye(4) + 1j * np.sin(a) * _PP[j])
    return out


def u3(t, p, l) -> np.ndarray:
    c, s = np.cos(0.5 * t), np.sin(0.5 * t)
    return np.array([[c, -np.exp(1j * l) * s], [np.exp(1j * p) * s, np.exp(1j * (p + l)) * c]])


def u3_angles(m):
    """(theta, phi, lam) with m = e^{i g} U3(theta, phi, lam)."""
    c, s = abs(m[0, 0]), abs(m[1, 0])
    g = np.angle(m[0, 0]) if c > 0 else 0.0
    phi = (np.angle(m[1, 0]) if s > 0 else 0.0) - g
    lam = np.angle(m[1, 1]) - g - phi if c >= s else np.angle(-m[0, 1]) - g
    return 2.0 * np.arctan2(s, c), phi, lam


def template(x, G, k) -> np.ndarray:
    """K_k G K_{k-1} ... G K_0 of a row of 6 (k + 1) angles, K = U3(qubit 1) (x) U3(qubit 0)."""
    x = np.asarray(x, dtype=np.float64)
    W = np.eye(4, dtype=np.complex128)
    for j in range(k + 1):
        if j:
            W = G @ W
        p = x[6 * j:6 * j + 6]
        W = np.kron(u3(*p[3:6]), u3(*p[0:3])) @ W
    return W


def fold_chamber(c) -> np.ndarray:
    """(c1, c2, c3) with c3 >= 0 (as c1c2c3 returns them) -> c1 <= 1/2, c3 of either sign."""
    c = np.array(c, dtype=np.float64, copy=True)
    m = c[..., 0] > 0.5
    c[..., 0] = np.where(m, 1.0 - c[..., 0], c[..., 0])
    c[..., 2] = np.where(m, -c[..., 2], c[..., 2])
    return c


def loss(T, W) -> float:
    return float(1.0 - abs(np.trace(np.conj(T).T @ W)) / 4.0)


def up_to_phase(T, W) -> float:
    tr = np.trace(np.conj(W).T @ T)
    return float(np.max(np.abs(T - tr / abs(tr) * W)))


def dress(rng, W, n=None):
    """e^{i phi} (L1 (x) L2) W (R1 (x) R2) with random SU(2) factors and phases: n matrices (or one)."""
    import kak_ref as kr

    m = 1 if n is None else n
    ph = np.exp(1j * rng.uniform(0, 2 * np.pi, m))[:, None, None]
    out = ph * (kr.kron2(kr.random_su2(rng, m), kr.random_su2(rng, m)) @ W @ kr.kron2(kr.random_su2(rng, m), kr.random_su2(rng, m)))
    return out[0] if n is None else out
