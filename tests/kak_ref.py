"""Test-side yardsticks for the KAK decomposition (``slam_kak`` / ``slam_targets_kak`` / ``weyl.kak``).  NumPy and LAPACK only; no code
is shared with csrc/slam_kak.hpp or ``slam_decomposition_amd.weyl``.

  * ``rebuild`` forms exp(i phase) (a1 (x) a2) CAN(c) (b1 (x) b2) with CAN(c) in closed form: XX, YY, ZZ commute, so
    CAN(c) = prod_P (cos(pi c_P / 2) 1 + i sin(pi c_P / 2) P (x) P) -- diagonal in the magic basis with phases pi a_j(c), the a_j of
    tests/weyl_ref.py.
  * ``factor_defect`` is max(|a a^+ - 1|, |det a - 1|) over the four 2x2 factors.
  * ``lapack_kak`` is a second, independent fp64 decomposition (``numpy.linalg.eigh`` of a random real combination of Re m and Im m,
    the local factors split by the SVD of the rearranged matrix).  It exists only to measure ``e_ref``: the residual a plain fp64
    implementation reaches on the same inputs.  It makes no attempt at the chamber and none at degenerate spectra beyond the
    random combination, so its residual on the named classes is what such a code gives there.
  * ``tolerance(e_ref)`` = min(max(8 e_ref, 1.2e-14), 1e-13): ``hp_ref.TOL_FACTOR`` and ``TOL_CAP``, with the floor 8 x 1.5e-15 (the worst
    residual of the NumPy port of the kernel's route over the named classes and 2000 Haar matrices, measured before the kernel was
    written).
"""
from __future__ import annotations

import numpy as np

import hp_ref as hp

FLOOR = 1.2e-14
_X = np.array([[0, 1], [1, 0]], dtype=np.complex128)
_Y = np.array([[0, -1j], [1j, 0]], dtype=np.complex128)
_Z = np.array([[1, 0], [0, -1]], dtype=np.complex128)
_PP = [np.kron(p, p) for p in (_X, _Y, _Z)]
_MAGIC = np.array([[1, 0, 0, 1j], [0, 1j, 1, 0], [0, 1j, -1, 0], [1, 0, 0, -1j]], dtype=np.complex128) / np.sqrt(2.0)


def tolerance(e_ref) -> float:
    return min(max(hp.TOL_FACTOR * float(np.max(e_ref)), FLOOR), hp.TOL_CAP)


def can(c) -> np.ndarray:
    """CAN(c) for c[..., 3] in units of pi -> [..., 4, 4]."""
    c = np.asarray(c, dtype=np.float64)
    out = np.broadcast_to(np.eye(4, dtype=np.complex128), c.shape[:-1] + (4, 4)).copy()
    for j in range(3):
        a = 0.5 * np.pi * c[..., j]
        out = out @ (np.cos(a)[..., None, None] * np.eye(4) + 1j * np.sin(a)[..., None, None] * _PP[j])
    return out


def kron2(a, b) -> np.ndarray:
    """Batched Kronecker product of [..., 2, 2] factors: ``a`` on the high bit of the basis index."""
    a, b = np.asarray(a), np.asarray(b)
    return np.einsum("...ij,...kl->...ikjl", a, b).reshape(a.shape[:-2] + (4, 4))


def rebuild(phase, a1, a2, c, b1, b2) -> np.ndarray:
    phase = np.asarray(phase, dtype=np.float64)
    return np.exp(1j * phase)[..., None, None] * (kron2(a1, a2) @ can(c) @ kron2(b1, b2))


def residual(U, r) -> np.ndarray:
    """max |U - rebuild(r)| per matrix."""
    return np.max(np.abs(np.asarray(U) - rebuild(*r)), axis=(-2, -1))


def factor_defect(r) -> np.ndarray:
    """max over the four factors of max(|a a^+ - 1|, |det a - 1|), per matrix."""
    worst = 0.0
    for a in (r[1], r[2], r[4], r[5]):
        a = np.asarray(a)
        uni = np.max(np.abs(a @ np.conj(np.swapaxes(a, -1, -2)) - np.eye(2)), axis=(-2, -1))
        det = np.abs(a[..., 0, 0] * a[..., 1, 1] - a[..., 0, 1] * a[..., 1, 0] - 1.0)
        worst = np.maximum(worst, np.maximum(uni, det))
    return worst


def _split_svd(K):
    """The nearest a (x) b to a 4x4 K, by the SVD of its rearrangement, each factor scaled to determinant 1."""
    R = K.reshape(2, 2, 2, 2).transpose(0, 2, 1, 3).reshape(4, 4)
    u, s, vh = np.linalg.svd(R)
    a = (np.sqrt(s[0]) * u[:, 0]).reshape(2, 2)
    b = (np.sqrt(s[0]) * vh[0]).reshape(2, 2)
    a = a / np.sqrt(np.linalg.det(a))
    b = b / np.sqrt(np.linalg.det(b))
    if np.real(np.vdot(np.kron(a, b), K)) < 0:
        a = -a
    return a, b


def lapack_kak(U, rng):
    """(phase, a1, a2, diag, b1, b2) with U ~ exp(i phase) (a1 (x) a2) Q diag Q^+ (b1 (x) b2): see the module docstring."""
    U = np.asarray(U, dtype=np.complex128)
    d = np.linalg.det(U)
    phase = np.angle(d) / 4.0
    B = _MAGIC.conj().T @ (U * np.exp(-1j * phase)) @ _MAGIC
    m = B @ B.T
    t = rng.uniform(0.2, 1.2)
    _, P = np.linalg.eigh(np.cos(t) * m.real + np.sin(t) * m.imag)
    if np.linalg.det(P) < 0:
        P[:, 0] = -P[:, 0]
    ev = np.diag(P.T @ m @ P)
    F = np.exp(0.5j * np.angle(ev))
    O2 = (np.conj(F)[:, None] * (P.T @ B)).real
    if np.linalg.det(O2) < 0:
        F[0], O2[0] = -F[0], -O2[0]
    a1, a2 = _split_svd(_MAGIC @ P @ _MAGIC.conj().T)
    b1, b2 = _split_svd(_MAGIC @ O2 @ _MAGIC.conj().T)
    return phase, a1, a2, F, b1, b2


def lapack_residual(U, rng) -> float:
    phase, a1, a2, F, b1, b2 = lapack_kak(U, rng)
    R = np.exp(1j * phase) * np.kron(a1, a2) @ (_MAGIC @ np.diag(F) @ _MAGIC.conj().T) @ np.kron(b1, b2)
    return float(np.max(np.abs(R - U)))


_E_REF = {}


def e_ref_of(name, U) -> float:
    """max over the matrices of a fixture group of the LAPACK decomposition's residual (computed once per group)."""
    if name not in _E_REF:
        rng = np.random.default_rng(20240611)
        _E_REF[name] = max(lapack_residual(u, rng) for u in U)
    return _E_REF[name]


def mirror(c) -> np.ndarray:
    c = np.array(c, dtype=np.float64)
    c[..., 0] = 1.0 - c[..., 0]
    return c


def random_su2(rng, n=None) -> np.ndarray:
    """Haar SU(2) matrices from normalised Gaussian quaternions: [n, 2, 2] (or [2, 2])."""
    q = rng.standard_normal((1 if n is None else n, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    a, b = q[:, 0] + 1j * q[:, 1], q[:, 2] + 1j * q[:, 3]
    m = np.stack([np.stack([a, b], -1), np.stack([-np.conj(b), np.conj(a)], -1)], -2)
    return m[0] if n is None else m


MATRIX_GROUP_NAMES = ("general", "named", "det-cut", "phase-edge", "drifted")
CHAMBER_TOL = 1e-13


def check_group(path, g, U, r, with_residual=True) -> None:
    """The residual, factor and coordinate assertions on one fixture group of matrices ``U`` and their decomposition ``r``; prints
    one ``KAK`` line.  ``with_residual=False`` (the ``drifted`` group: matrices unitary only to 2e-10): coordinates and factors."""
    import weyl_ref as w

    name = g["meta"]["name"]
    tol = tolerance(e_ref_of(name, U))
    res = residual(U, r)
    fac = factor_defect(r)
    c = np.asarray(r[3])
    d = w.distance(c, g["ref"])
    out = w.chamber_violation(c)
    ctol = w.tolerance(g["e_ref"])
    print(f"KAK {path:<12s} {name:<11s} residual {res.max():.3g} factors {fac.max():.3g} tol {tol:.3g} e_ref {e_ref_of(name, U):.3g} "
          f"coordinates {d.max():.3g} tol {ctol:.3g} outside {out.max():.1g} cases {len(U)}")
    if with_residual:
        assert res.max() <= tol, (path, name, int(np.argmax(res)), res.max(), tol)
    assert fac.max() <= tol, (path, name, int(np.argmax(fac)), fac.max(), tol)
    assert d.max() <= ctol, (path, name, int(np.argmax(d)), d.max(), ctol)
    assert out.max() <= CHAMBER_TOL, (path, name, out.max())
