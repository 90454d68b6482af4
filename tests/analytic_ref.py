"""Test-side restatement of the closed-form sqrt(iSWAP) decomposition (``slam_sqiswap_decompose``, csrc/slam_analytic.hpp), in NumPy.
Nothing is shared with csrc/; the alignments use ``slam_decomposition_amd.weyl.kak``.

Conventions: S = exp(i pi/8 (XX + YY)), class (1/4, 1/4, 0); coordinates c in units of pi, folded to c1 <= 1/2 by
(c1, c2, c3) -> (1 - c1, c2, -c3); radians (x, y, z) = pi/2 c; RX(a) = exp(-i a X / 2), RZ likewise; in kron(A, B) A acts on the high
bit.  A template row holds six angles per layer: U3(theta, phi, lam) of qubit 0 (the low bit), then of qubit 1.

Two gates, |z| <= x - y (Huang et al., arXiv:2105.06074):  V = S kron(C1, C2) S has class (x, y, z) for

    C   = sin(x + y - z) sin(x - y + z) sin(-x - y - z) sin(-x + y + z)                  (clamped at 0)
    alpha, beta = arccos(cos 2x - cos 2y + cos 2z +- 2 sqrt(C))                           (arguments clamped to [-1, 1])
    num = 4 cos^2 x cos^2 z sin^2 y,  den = num + cos 2x cos 2y cos 2z
    gamma = arccos(s sqrt(num / den)),  s = +1 for z >= 0, -1 for z < 0                    (den = 0: gamma = 0)
    C1 = RZ(gamma) RX(alpha) RZ(gamma),  C2 = RX(beta).

Three gates: CAN(c) = CAN(c - s) CAN(s) for each of the 12 signed placements s of (1/4, 1/4, 0), and CAN(s) = Ls S Rs with local
Clifford-like Ls, Rs; the placement whose reduced class f = fold(c - s) has the largest margin (f1 - f2) - |f3| is taken (the lowest
index among equals), V(f) is aligned to CAN(c - s):  CAN(c - s) ~ L1 V R1, and with T = A CAN(c) B the circuit is
    T ~ (A L1) S C S (R1 Ls) S (Rs B).

``u`` is the conditioning of the interior formula: min(1 - |arg alpha|, 1 - |arg beta|, 1 - sqrt(num / den)) at the class the
formula is fed.
"""
from __future__ import annotations

import numpy as np

from closed_form_ref import SIZE_TOL, _PP, _X, _Y, _Z, can, fold_chamber, loss, u3, u3_angles, up_to_phase  # noqa: F401 (re-exported)
from slam_decomposition_amd import weyl

S = np.array([[1, 0, 0, 0], [0, np.sqrt(0.5), 1j * np.sqrt(0.5), 0], [0, 1j * np.sqrt(0.5), np.sqrt(0.5), 0], [0, 0, 0, 1]], dtype=np.complex128)

# the 12 signed placements of (1/4, 1/4, 0): positions (0, 1), (0, 2), (1, 2) times signs ++, +-, -+, --
SHIFTS = np.zeros((12, 3))
for _p, (_i, _j) in enumerate(((0, 1), (0, 2), (1, 2))):
    for _s, (_a, _b) in enumerate(((1, 1), (1, -1), (-1, 1), (-1, -1))):
        SHIFTS[4 * _p + _s, _i] = 0.25 * _a
        SHIFTS[4 * _p + _s, _j] = 0.25 * _b


def template(x, k) -> np.ndarray:
    """K_k S K_{k-1} ... S K_0 of a row of 6 (k + 1) angles, K = U3(qubit 1) (x) U3(qubit 0)."""
    x = np.asarray(x, dtype=np.float64)
    W = np.eye(4, dtype=np.complex128)
    for j in range(k + 1):
        if j:
            W = S @ W
        p = x[6 * j:6 * j + 6]
        W = np.kron(u3(*p[3:6]), u3(*p[0:3])) @ W
    return W


def fold(c) -> np.ndarray:
    """The class of CAN(c), c[..., 3] anywhere, as (f1, f2, f3) with 1/2 >= f1 >= f2 >= |f3|: each coordinate modulo 1, any permutation,
    signs flipped in pairs."""
    c = np.asarray(c, dtype=np.float64)
    r = c - np.rint(c)
    neg = np.sum(r < 0, axis=-1) % 2 == 1
    a = -np.sort(-np.abs(r), axis=-1)
    a[..., 2] = np.where(neg, -a[..., 2], a[..., 2])
    return a


def size(c8) -> np.ndarray:
    """2 or 3 from coordinates rounded to 8 digits: the rule of span_rules.minimal_span for the sqrt(iSWAP) class, never below 2."""
    f = fold_chamber(c8)
    return np.where(np.abs(f[..., 2]) <= f[..., 0] - f[..., 1] + SIZE_TOL, 2, 3)


def interior(f, reference_gamma: bool = False):
    """(alpha, beta, gamma, u) of the folded class f[..., 3] (units of pi).  ``reference_gamma``: the expression of the reference's
    transcription (cos^2 y in the numerator, cos 2x + cos 2y cos 2z in the denominator), kept for the regression guard only."""
    f = np.asarray(f, dtype=np.float64)
    x, y, z = (0.5 * np.pi * f[..., j] for j in range(3))
    C = np.sin(x + y - z) * np.sin(x - y + z) * np.sin(-x - y - z) * np.sin(-x + y + z)
    rC = 2.0 * np.sqrt(np.maximum(C, 0.0))
    base = np.cos(2 * x) - np.cos(2 * y) + np.cos(2 * z)
    aa = np.clip(base + rC, -1.0, 1.0)
    ab = np.clip(base - rC, -1.0, 1.0)
    if reference_gamma:
        num = 4 * np.cos(x) ** 2 * np.cos(z) ** 2 * np.cos(y) ** 2
        den = num + np.cos(2 * x) + np.cos(2 * y) * np.cos(2 * z)
    else:
        num = 4 * np.cos(x) ** 2 * np.cos(z) ** 2 * np.sin(y) ** 2
        den = num + np.cos(2 * x) * np.cos(2 * y) * np.cos(2 * z)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(den > 0, num / np.where(den > 0, den, 1.0), 1.0)
    rq = np.sqrt(np.clip(q, 0.0, 1.0))
    gamma = np.where(den > 0, np.arccos(np.where(z < 0, -rq, rq)), 0.0)
    u = np.minimum(np.minimum(1 - np.abs(aa), 1 - np.abs(ab)), 1 - rq)
    return np.arccos(aa), np.arccos(ab), gamma, u


def best_shift(c):
    """(index, reduced class f, margin) of the best of the 12 placements for the chamber point c[..., 3]."""
    c = np.asarray(c, dtype=np.float64)
    f = fold(c[..., None, :] - SHIFTS)
    m = (f[..., 0] - f[..., 1]) - np.abs(f[..., 2])
    i = np.argmax(m, axis=-1)  # the first of equal margins
    return i, np.take_along_axis(f, i[..., None, None], axis=-2)[..., 0, :], np.take_along_axis(m, i[..., None], axis=-1)[..., 0]


def plan(c, c8=None):
    """Vectorised front half: sizes k, the class fed to the interior formula, its conditioning u, the shift index (-1 for k = 2) and the
    shift margin (nan for k = 2) of chamber points c[N, 3] (unrounded; c8 = the same rounded to 8 digits)."""
    c = np.asarray(c, dtype=np.float64)
    k = size(np.round(c, 8) if c8 is None else c8)
    i, f3, m = best_shift(c)
    f = np.where((k == 2)[..., None], fold_chamber(c), f3)
    u = interior(f)[3]
    return k, f, u, np.where(k == 2, -1, i), np.where(k == 2, np.nan, m)


def interior_row(f) -> np.ndarray:
    """The six angles of the layer C = kron(C1, C2): RX(beta) = U3(beta, -pi/2, pi/2) on qubit 0 and
    RZ(gamma) RX(alpha) RZ(gamma) = e^{-i gamma} U3(alpha, gamma - pi/2, gamma + pi/2) on qubit 1."""
    al, be, ga, _ = interior(np.asarray(f, dtype=np.float64))
    h = 0.5 * np.pi
    return np.array([be, -h, h, al, ga - h, ga + h])


def align(W, T):
    """(L1, L2, R1, R2, gap) with T ~ kron(L1, L2) W kron(R1, R2) up to a phase for W, T of (nearly) one class: KAK of both, W's
    mirrored where that brings its chamber point closer to T's."""
    kw, kt = weyl.kak(W), weyl.kak(T)
    cw, ct = np.asarray(kw[3]), np.asarray(kt[3])
    d0 = np.max(np.abs(cw - ct))
    d1 = np.max(np.abs(np.array([1 - cw[0], cw[1], -cw[2]]) - ct))
    if d1 < d0:
        kw = weyl.mirror_kak(*kw)
    return kt[1] @ kw[1].conj().T, kt[2] @ kw[2].conj().T, kw[4].conj().T @ kt[4], kw[5].conj().T @ kt[5], min(d0, d1)


_ROT = (np.eye(2, dtype=np.complex128), np.sqrt(0.5) * np.array([[1, -1j], [-1j, 1]]), np.sqrt(0.5) * np.array([[1, -1], [1, 1]], dtype=np.complex128))


def shift_locals(i):
    """(Ls, Rs) as pairs of 2x2 matrices with CAN(SHIFTS[i]) = kron(*Ls) S kron(*Rs), found by aligning S to CAN(s)."""
    L1, L2, R1, R2, gap = align(S, can(SHIFTS[i]))
    assert gap < 1e-14
    return (L1, L2), (R1, R2)


def _layer_angles(q1, q0):
    return list(u3_angles(q0)) + list(u3_angles(q1))


def decompose(T):
    """(k, x, W, gap, u): the 6 (k + 1) template angles of a circuit of k = 2 or 3 sqrt(iSWAP) gates for the 4x4 unitary T, its unitary
    W = template(x, k), the chamber distance of the alignment that carries the interior formula's error, and the conditioning u."""
    T = np.asarray(T, dtype=np.complex128)
    kt = weyl.kak(T)
    c = np.asarray(kt[3])
    k, f, u, i, _ = plan(c[None])
    k, f, u, i = int(k[0]), f[0], float(u[0]), int(i[0])
    mid = interior_row(f)
    V = template(np.r_[np.zeros(6), mid, np.zeros(6)], 2)
    if k == 2:
        L1, L2, R1, R2, gap = align(V, T)
        x = np.r_[_layer_angles(R1, R2), mid, _layer_angles(L1, L2)]
    else:
        raw = c - SHIFTS[i]
        L1, L2, R1, R2, gap = align(V, can(raw))
        (s1, s2), (t1, t2) = shift_locals(i)
        x = np.r_[_layer_angles(t1 @ kt[4], t2 @ kt[5]), _layer_angles(R1 @ s1, R2 @ s2), mid, _layer_angles(kt[1] @ L1, kt[2] @ L2)]
    return k, x, template(x, k), float(gap), u


def _named():
    cnot = np.array([[1, 0, 0, 0], [0, 0, 0, 1], [0, 0, 1, 0], [0, 1, 0, 0]], dtype=np.complex128)
    iswap = np.array([[1, 0, 0, 0], [0, 0, 1j, 0], [0, 1j, 0, 0], [0, 0, 0, 1]], dtype=np.complex128)
    swap = np.array([[1, 0, 0, 0], [0, 0, 1, 0], [0, 1, 0, 0], [0, 0, 0, 1]], dtype=np.complex128)
    out = [("identity", np.eye(4, dtype=np.complex128)), ("sqrt(iSWAP)", S), ("CX", cnot), ("iSWAP", iswap), ("B", can((0.5, 0.25, 0.0))), ("SWAP", swap)]
    for c in ((0.3, 0.2, 0.1), (0.3, 0.2, 0.1 + 1e-9), (0.3, 0.2, 0.1 - 1e-9), (0.5, 0.5, 0.5), (0.5, 0.25, 0.25), (0.2, 0.2, 0.2), (0.2, 0.2, -0.2),
              (0.4, 0.1, 0.05), (0.4, 0.1, -0.05), (0.3, 0.2, 0.0), (0.5, 0.3, 0.1), (1e-9, 0.0, 0.0)):
        out.append(("CAN(%g, %g, %.10g)" % c, can(c)))
    return out


# the named and hard inputs: (name, gate); "CAN(0.3, 0.2, 0.1)" lies on the size boundary |z| = x - y, where either size is right
NAMED = _named()
ON_BOUNDARY = ("CAN(0.3, 0.2, 0.1)",)


def expected_size(T) -> np.ndarray:
    """2 or 3 per matrix of T[N, 4, 4]: span_rules.minimal_span for the sqrt(iSWAP) class on the 8-digit coordinates, never below 2."""
    from slam_decomposition_amd import span_rules

    return np.maximum(span_rules.minimal_span(weyl.c1c2c3_batch(np.asarray(T)), (0.25, 0.25, 0.0)), 2)
