"""Weyl-chamber coordinates on the host (two calls per target: SURVEY.md §8(a) A10).

Restates ``weylchamber.c1c2c3`` (called at src/slam/basis_abc.py:80-84 and
src/slam/optimizer.py:85,103); a batched device version is a "next" row (§8(f) rank 1).
"""
from __future__ import annotations

import numpy as np

_SY = np.array([[0, -1j], [1j, 0]], dtype=np.complex128)
_YY = np.kron(_SY, _SY)
_M = np.array([[1, 1, 0], [1, 0, 1], [0, 1, 1]])


def g1g2g3(U):
    """Makhlin's local invariants (g1, g2, g3) = (Re G1, Im G1, Re G2) of a two-qubit unitary, unrounded:
    M = U^T Y U Y (Y = sigma_y (x) sigma_y), G1 = tr(M)^2 / (16 det U), G2 = (tr(M)^2 - tr(M^2)) / (4 det U) -- the
    magic-basis form of weylchamber.g1g2g3 without the basis change (Q Q^T = -Y)."""
    U = np.asarray(U, dtype=np.complex128)
    M = U.T @ _YY @ U @ _YY
    d = complex(np.linalg.det(U))
    t = complex(np.trace(M))
    G1 = t * t / (16 * d)
    G2 = (t * t - complex(np.trace(M @ M))) / (4 * d)
    return (float(G1.real), float(G1.imag), float(G2.real))


def c1c2c3(U, ndigits: int = 8):
    """(c1, c2, c3) in units of pi, rounded to ``ndigits`` like weylchamber does."""
    U = np.asarray(U, dtype=np.complex128)
    Ut = _YY @ U.T @ _YY
    ev = np.linalg.eigvals(U @ Ut / np.sqrt(complex(np.linalg.det(U))))
    two_S = np.angle(ev) / np.pi
    two_S = np.where(two_S <= -0.5, two_S + 2.0, two_S)
    S = np.sort(two_S / 2.0)[::-1]
    n = int(round(float(S.sum())))
    S = S - np.r_[np.ones(n), np.zeros(4 - n)]
    S = np.roll(S, -n)
    c1, c2, c3 = _M @ S[:3]
    if c3 < 0:
        c1 = 1 - c1
        c3 = -c3
    return tuple(float(round(v + 0.0, ndigits) + 0.0) for v in (c1, c2, c3))


def c1c2c3_batch(U, ndigits: int = 8) -> np.ndarray:
    """:func:`c1c2c3` for a stack of unitaries ``U[N, 4, 4]`` -> float64[N, 3] (same values, one batched
    ``eigvals`` call instead of N)."""
    U = np.asarray(U, dtype=np.complex128)
    if U.ndim != 3 or U.shape[1:] != (4, 4):
        raise ValueError("expected an array of shape [N, 4, 4]")
    if U.shape[0] == 0:
        return np.zeros((0, 3))
    Ut = _YY @ np.swapaxes(U, 1, 2) @ _YY
    det = np.linalg.det(U).astype(np.complex128)
    ev = np.linalg.eigvals(U @ Ut / np.sqrt(det)[:, None, None])
    two_S = np.angle(ev) / np.pi
    two_S = np.where(two_S <= -0.5, two_S + 2.0, two_S)
    S = -np.sort(-two_S / 2.0, axis=1)  # descending
    n = np.rint(S.sum(axis=1)).astype(int)
    out = np.empty((U.shape[0], 3))
    for nn in np.unique(n):  # n is 0..2 in practice: a handful of groups
        m = n == nn
        Sg = S[m] - np.r_[np.ones(nn), np.zeros(4 - nn)]
        Sg = np.roll(Sg, -nn, axis=1)
        out[m] = Sg[:, :3] @ _M.T
    flip = out[:, 2] < 0
    out[flip, 0] = 1 - out[flip, 0]
    out[flip, 2] = -out[flip, 2]
    return np.round(out + 0.0, ndigits) + 0.0


# ---- KAK decomposition (csrc/slam_kak.hpp restated for one matrix) ---------------------------------------------------------------
_H = 0.70710678118654752440
_Q = _H * np.array([[1, 0, 0, 1j], [0, 1j, 1, 0], [0, 1j, -1, 0], [1, 0, 0, -1j]], dtype=np.complex128)
# Q^+ CAN(c) Q = diag(exp(i pi R_s)), s = _SIGMA[column], with R = ((c1+c2-c3)/2, (c1-c2+c3)/2, (-c1+c2+c3)/2, -(c1+c2+c3)/2)
_SIGMA = (1, 0, 3, 2)
_IX = np.array([[0, 1j], [1j, 0]])
_IY = np.array([[0, 1], [-1, 0]], dtype=np.complex128)
_IZ = np.array([[1j, 0], [0, -1j]])


def _su2(m):
    """The SU(2) matrix nearest to a multiple of one: [[a, b], [-b*, a*]] / sqrt(|a|^2 + |b|^2)."""
    a = 0.5 * (m[0, 0] + np.conj(m[1, 1]))
    b = 0.5 * (m[0, 1] - np.conj(m[1, 0]))
    n = np.sqrt(abs(a) ** 2 + abs(b) ** 2)
    a, b = a / n, b / n
    return np.array([[a, b], [-np.conj(b), np.conj(a)]])


def _split_local(K):
    """(a, b) in SU(2) with K = a (x) b for K in SU(2) (x) SU(2): b from the 2x2 block of largest norm (no small pivot)."""
    blocks = [(i, j) for i in range(2) for j in range(2)]
    i, j = max(blocks, key=lambda ij: float(np.sum(np.abs(K[2 * ij[0]:2 * ij[0] + 2, 2 * ij[1]:2 * ij[1] + 2]) ** 2)))
    blk = K[2 * i:2 * i + 2, 2 * j:2 * j + 2]
    b = blk / np.sqrt(blk[0, 0] * blk[1, 1] - blk[0, 1] * blk[1, 0])
    b = _su2(b)
    a = np.array([[0.5 * np.trace(b.conj().T @ K[2 * r:2 * r + 2, 2 * c:2 * c + 2]) for c in range(2)] for r in range(2)])
    return _su2(a), b


def _joint_jacobi(X, Y):
    """The kernel's joint Jacobi sweeps over the commuting symmetric pair, with the rotations accumulated: V^T (X + iY) V diagonal."""
    V = np.eye(4)
    for _ in range(12):
        off = sum(X[i, j] ** 2 + Y[i, j] ** 2 for i in range(3) for j in range(i + 1, 4))
        if off < 1e-31:
            break
        for p in range(3):
            for q in range(p + 1, 4):
                h1x, h1y = X[p, p] - X[q, q], Y[p, p] - Y[q, q]
                h2x, h2y = 2.0 * X[p, q], 2.0 * Y[p, q]
                ton = (h1x * h1x + h1y * h1y) - (h2x * h2x + h2y * h2y)
                toff = 2.0 * (h1x * h2x + h1y * h2y)
                if toff == 0.0 and ton >= 0.0:
                    continue
                th = 0.25 * np.arctan2(toff, ton)
                G = np.eye(4)
                G[p, p] = G[q, q] = np.cos(th)
                G[q, p] = np.sin(th)
                G[p, q] = -np.sin(th)
                X, Y, V = G.T @ X @ G, G.T @ Y @ G, V @ G
    return V, X, Y


def mirror_kak(phase, a1, a2, c, b1, b2):
    """The same product written with the mirror image (1 - c1, c2, -c3) of c:
    CAN(c) = -i (iZ (x) iX) CAN(1 - c1, c2, -c3) (iY (x) 1)."""
    return phase - 0.5 * np.pi, a1 @ _IZ, a2 @ _IX, (1.0 - c[0], c[1], -c[2]), _IY @ b1, b2


def kak(U):
    """U = exp(i phase) (a1 (x) a2) CAN(c) (b1 (x) b2), CAN(c) = exp(i pi/2 (c1 XX + c2 YY + c3 ZZ)): ``(phase, a1, a2, c, b1, b2)`` with the
    2x2 factors in SU(2) and c (units of pi) the chamber point of ``c1c2c3(U, ndigits=-1)`` -- the route of ``kak_kernel``: joint
    Jacobi diagonalisation of Re, Im of m = U_B U_B^T in the magic basis with the rotations kept (O1 = V, F = D^(1/2),
    O2 = F^-1 V^T U_B), the eigenphases ordered as the chamber fold orders them."""
    U = np.asarray(U, dtype=np.complex128)
    if U.shape != (4, 4):
        raise ValueError("expected a 4x4 matrix")
    det = complex(np.linalg.det(U))
    B = _Q.conj().T @ U @ _Q
    m = B @ B.T
    V, X, Y = _joint_jacobi(m.real.copy(), m.imag.copy())
    dphi = 0.5 * np.arctan2(det.imag, det.real)
    ev = (np.diag(X) + 1j * np.diag(Y)) * np.exp(-1j * dphi)
    two_s = np.angle(ev) / np.pi
    two_s = np.where(two_s <= -0.5 + 1e-12, two_s + 2.0, two_s)
    S = 0.5 * two_s
    order = sorted(range(4), key=lambda k: -S[k])  # stable: ties keep the column order
    S = S[order]
    n = min(max(int(np.rint(S.sum())), 0), 3)
    S = S - np.r_[np.ones(n), np.zeros(4 - n)]
    R = [S[(i + n) & 3] for i in range(4)]
    col = [order[(i + n) & 3] for i in range(4)]
    c = (R[0] + R[1], R[0] + R[2], R[1] + R[2])
    h = np.array([R[_SIGMA[j]] for j in range(4)])
    O1 = np.stack([V[:, col[_SIGMA[j]]] for j in range(4)], axis=1)
    if np.linalg.det(O1) < 0:
        O1[:, 0] = -O1[:, 0]
    phase = 0.5 * dphi
    O2 = (np.exp(-1j * (np.pi * h + phase))[:, None] * (O1.T @ B)).real
    a1, a2 = _split_local(_Q @ O1 @ _Q.conj().T)
    b1, b2 = _split_local(_Q @ O2 @ _Q.conj().T)
    out = (phase, a1, a2, c, b1, b2)
    if c[2] < 0.0:
        out = mirror_kak(*out)
    phase, a1, a2, c, b1, b2 = out
    return float(phase), a1, a2, np.array([c[0] + 0.0, c[1] + 0.0, c[2] + 0.0]), b1, b2
