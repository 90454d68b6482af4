"""A plain 40-digit reference for the classification kernels (tests/golden/weyl_lookup_reference.npz): the Weyl class of a 4x4 matrix
and what the coverage lookups decide about it.

Written from the definitions with mpmath (``mp.dps = 40``), every fp64 input taken exactly, sharing no code with ``oracle/``,
``slam_decomposition_amd/coverage.py`` or the kernels (the matrix helpers and the Makhlin invariants come from tests/hp_ref.py):

  * THE CLASS.  With the magic basis Q, the eigenvalues of (Q^+ U Q)(Q^+ U Q)^T / sqrt(det U) (principal root) are found by
    ``mp.eig``; their phases are pi t_k.  For CAN(c) = exp(i pi/2 (c1 XX + c2 YY + c3 ZZ)) these phases are 2 pi a_j(c) with
    a = ((c1+c2-c3)/2, (c1-c2+c3)/2, (-c1+c2+c3)/2, (-c1-c2-c3)/2), and the other branch of the root moves all four by pi.
  * THE CANONICAL POINT is stated outright, not folded to: among ALL triples c = (a_p + a_q, a_p + a_r, a_q + a_r) -- over the two
    branches (t_k / 2 or t_k / 2 + 1/2), every lift a_k = frac(.) - {0, 1} with sum a = 0 and every choice of three of the four
    indices in every order -- the one that satisfies

        0 <= c1 < 1,   c2 <= min(c1, 1 - c1),   0 <= c3 <= c2,   and c1 <= 1/2 where c3 = 0

    Every comparison is made with a slack of 1e-32 (the 40-digit phases of an exactly degenerate class carry 1e-40 of noise, sixteen
    orders below fp64).  All triples that satisfy it must coincide to 1e-30, else the input is refused.
  * THE CROSS-CHECK is independent of that search: the Makhlin invariants (``hp_ref.local_invariants``) of the matrix and of
    CAN(point), the latter by ``mp.expm``, agree to 1e-30.  An fp64 matrix is unitary to 1e-16 only and its invariants carry the
    moduli of the eigenvalues, which the class (phases only) ignores; so the check is made on the unitary polar factor of the matrix
    (Newton iteration at 40 digits), whose eigenphases equal the matrix's own to first order in that 1e-16 (inside a degenerate cluster the next order is
    divided by a splitting that is itself rounding noise: up to 1e-17 was seen, 1e-15 is asserted, far below every tolerance).
  * THE DECISIONS work from the exact arrays a kernel receives.  Both alcove points of the class (frac of a_j(c) + shift, sorted
    decreasingly, 1 taken off the s = sum largest, sorted again), the 14 sums over the subsets K of {1..4} of gamma_{5-k}, then per
    entry a SIGNED MARGIN: the largest, over the two alcove points, of the smallest slack of its conditions
        one gate        t1 - |a_j - q_j|,  t1 = max(tol, 0) + 1e-12          (j = 1..4)
        half-spaces     sum_p - (bound_p - tol)                              (finite bounds only)
        facets          tol - (n . c - b)                                    (c = the chamber point itself)
    and for the "local" rule min(1e-8 - |a_1|, 1e-8 - |a_4|).  An entry contains the target iff its margin is >= 0, a region iff one
    of its parts does (margin: the largest of its parts').  The margin of a case is the smallest |margin| over every entry or region
    of the table and the local rule: no perturbation of the sums below it changes any decision.  Where c3 rounds to 0 at 8 digits
    the kernel may hold (1 - c1, c2, 0) instead of (c1, c2, 0); facets are then evaluated at both and must agree (else margin 0).

The part below ``# ---- fixture`` needs NumPy only: the GPU tests read the committed fixture through it and never import mpmath.  A
target is stored as the fp64 numbers it is built from -- four tangents t_k, a pair of stored local factors K1, K2 and a stored phase
g: U = g K1 diag((1 - t^2 + 2 i t) / (1 + t^2)) K2 -- and ``build_unitaries`` forms the product with one IEEE operation per NumPy
call on real arrays (no BLAS, no complex multiply, no libm), so every machine gets the same bits; the reference was computed from
exactly these matrices, and ``checksum`` pins them.
"""
from __future__ import annotations

import itertools
import math
import os

import numpy as np

import hp_ref as hp

try:  # the GPU machine reads the fixture only
    from mpmath import mp, mpc, mpf
except ImportError:  # pragma: no cover
    mp = mpc = mpf = None

DPS = 40
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "weyl_lookup_reference.npz")
MARGIN = 3e-8  # see DESIGN.md: 8-digit rounding moves a sum of three alcove coordinates by at most 2.25e-8, a unit facet by 8.7e-9
HALF_INTEGER_GUARD = 1e-4  # reference * 1e8 this close to a half-integer: np.round(reference, 8) is not decided by the class

PATTERNS = [K for r in (1, 2, 3) for K in itertools.combinations((1, 2, 3, 4), r)]  # the 14 subsets K, the order of the tables' bounds


# ---- the class of a matrix (mpmath) ---------------------------------------------------------------------------------------------
def polar_unitary(A, iterations=6):
    """The unitary polar factor of a nearly unitary list matrix: X <- (X + X^{-+}) / 2."""
    X = mp.matrix(A)
    for _ in range(iterations):
        X = (X + (X ** -1).H) / 2
    return [[mpc(X[i, j]) for j in range(4)] for i in range(4)]


def eigenphases(A):
    """t_k (units of pi, in (-1, 1]) of the eigenvalues of (Q^+ A Q)(Q^+ A Q)^T / sqrt(det A)."""
    Q = hp._magic()
    B = hp.mm(hp.dag(Q), hp.mm(A, Q))
    m = hp.mm(B, hp.transpose(B))
    s = mp.sqrt(mp.det(mp.matrix(A)))
    E = mp.eig(mp.matrix([[z / s for z in row] for row in m]), left=False, right=False)
    return [mp.arg(e) / mp.pi for e in E]


def in_chamber(c) -> bool:
    c1, c2, c3 = c
    d = mpf(10) ** -32
    return -d <= c1 < 1 - d and c2 <= min(c1, 1 - c1) + d and -d <= c3 <= c2 + d and (abs(c3) > d or 2 * c1 <= 1 + d)


def chamber_point(phases):
    """The canonical point of the class with eigenphases pi t_k: exhaustive search, see the module docstring."""
    found = []
    tiny = mpf(10) ** -30
    for shift in (mpf(0), mpf(1) / 2):
        b = [t / 2 + shift for t in phases]
        b = [x - mp.floor(x) for x in b]
        for lift in itertools.product((0, 1), repeat=4):
            a = [x - n for x, n in zip(b, lift)]
            if abs(mp.fsum(a)) > tiny:
                continue
            for p, q, r in itertools.permutations(range(4), 3):
                c = (a[p] + a[q], a[p] + a[r], a[q] + a[r])
                if in_chamber(c):
                    found.append(c)
    if not found:
        raise ArithmeticError("no triple of the class lies in the chamber")
    spread = max(abs(c[j] - found[0][j]) for c in found for j in range(3))
    if spread > tiny:
        raise ArithmeticError(f"the chamber rule does not single out one point (spread {mp.nstr(spread, 5)})")
    return found[0]


_PAULI = None


def canonical_gate(c):
    """CAN(c) = exp(i pi/2 (c1 XX + c2 YY + c3 ZZ)) by ``mp.expm``."""
    global _PAULI
    if _PAULI is None:
        X = [[mpc(0), mpc(1)], [mpc(1), mpc(0)]]
        Y = [[mpc(0), mpc(0, -1)], [mpc(0, 1), mpc(0)]]
        Z = [[mpc(1), mpc(0)], [mpc(0), mpc(-1)]]
        _PAULI = [hp.kron(P, P) for P in (X, Y, Z)]
    H = mp.matrix(4, 4)
    for i in range(4):
        for j in range(4):
            H[i, j] = mpc(0, 1) * mp.pi / 2 * sum(c[k] * _PAULI[k][i][j] for k in range(3))
    E = mp.expm(H)
    return [[mpc(E[i, j]) for j in range(4)] for i in range(4)]


def weyl_class(U, check=True):
    """The canonical chamber point (three mpf, units of pi) of the fp64 matrix ``U``, cross-checked by the Makhlin invariants."""
    A = hp.mat(U)
    c = chamber_point(eigenphases(A))
    if check:
        P = polar_unitary(A)
        cp = chamber_point(eigenphases(P))
        drift = max(abs(x - y) for x, y in zip(c, cp))
        if c[2] < mpf(10) ** -15:  # on the c3 = 0 face the two may sit on either side of the mirror
            drift = min(drift, max(abs(1 - c[0] - cp[0]), abs(c[1] - cp[1]), abs(c[2] - cp[2])))
        if drift > mpf(10) ** -15:
            raise ArithmeticError(f"the class of the matrix and of its polar factor differ by {mp.nstr(drift, 5)}")
        gu, gc = hp.local_invariants(P), hp.local_invariants(canonical_gate(cp))
        err = max(abs(x - y) for x, y in zip(gu, gc))
        if err > mpf(10) ** -30:
            raise ArithmeticError(f"Makhlin invariants of the matrix and of CAN(point) differ by {mp.nstr(err, 5)}")
    return c


# ---- the decisions (any exact number type: mpf, or float for searching) -------------------------------------------------------------
def _floor(x):
    return math.floor(x) if isinstance(x, float) else mp.floor(x)


def alcove_point(c, shift):
    """The alcove point (decreasing, sum 0, a_1 - a_4 <= 1) of i^{2 shift} CAN(c)."""
    c1, c2, c3 = c
    v = [(c1 + c2 - c3) / 2 + shift, (c1 - c2 + c3) / 2 + shift, (-c1 + c2 + c3) / 2 + shift, (-c1 - c2 - c3) / 2 + shift]
    f = sorted((x - _floor(x) for x in v), reverse=True)
    s = int(round(float(sum(f))))
    return sorted((x - 1 if j < s else x for j, x in enumerate(f)), reverse=True)


def views(c):
    """[(alcove point, its 14 sums)] for shift 0 and 1/2."""
    half = 0.5 if isinstance(c[0], float) else mpf(1) / 2
    out = []
    for shift in (0 * half, half):
        a = alcove_point(c, shift)
        out.append((a, [sum(a[4 - k] for k in K) for K in PATTERNS]))
    return out


def _num(x, like):
    return float(x) if isinstance(like, float) else mpf(float(x))


def box_margin(vw, point, tol):
    t1 = max(float(tol), 0.0) + 1e-12  # the fp64 number the kernel forms
    return max(min(_num(t1, a[0]) - abs(a[j] - _num(point[j], a[0])) for j in range(4)) for a, _ in vw)


def halfspace_margin(vw, bounds, tol):
    lo = [float(b) - float(tol) for b in bounds]  # as the kernel: bound - tol in fp64
    best = None
    for a, s in vw:
        m = min([s[p] - _num(lo[p], a[0]) for p in range(14) if math.isfinite(lo[p])], default=math.inf)
        best = m if best is None or m > best else best
    return best


def local_margin(vw):
    return max(min(_num(1e-8, a[0]) - abs(a[0]), _num(1e-8, a[0]) - abs(a[3])) for a, _ in vw)


def exactly_local(c) -> bool:
    """Within 1e-9 of (0, 0, 0) or of (1, 0, 0): the 8-digit coordinates are exactly that vertex and the target is local, whatever the
    1e-8 box of the rule."""
    return max(min(abs(float(c[0])), abs(1.0 - float(c[0]))), abs(float(c[1])), abs(float(c[2]))) <= 1e-9


def lookup(c, kinds, points, bounds, tol, vw=None):
    """coverage_lookup's bin of the class c in one table (first containing entry; n: local; n + 1: none) and the case's margin.
    ``vw``: the alcove points to use instead of ``views(c)``."""
    vw = views(c) if vw is None else vw
    if exactly_local(c):
        return len(kinds), math.inf
    n = len(kinds)
    ms = [box_margin(vw, points[e], tol) if kinds[e] == 0 else halfspace_margin(vw, bounds[e], tol) for e in range(n)]
    loc = local_margin(vw)
    first = next((e for e in range(n) if ms[e] >= 0), n + 1)
    margin = min([abs(loc)] + [abs(m) for m in ms])
    return (n if loc >= 0 else first), margin


def span_table(point, bounds):
    """predict_spans' regions as a lookup table: entry 0 the first gate's class, entry k - 1 the half-spaces of the first k gates."""
    k_max = len(bounds)
    kinds = [0] + [1] * (k_max - 1)
    return kinds, [point] * k_max, bounds


def predict_span(c, point, bounds, tol, vw=None):
    """predict_spans' answer (0 local, 1 .. k_max, k_max + 1 out of reach) and the margin."""
    kinds, points, bounds = span_table(point, bounds)
    b, margin = lookup(c, kinds, points, bounds, tol, vw)
    k_max = len(kinds)
    return (0 if b == k_max else (k_max + 1 if b == k_max + 1 else b + 1)), margin


def _region_flags(c, vw, ro, kinds, fo, facets, aux, tol):
    flags, margin = [], math.inf
    for r in range(len(ro) - 1):
        best = None
        for p in range(int(ro[r]), int(ro[r + 1])):
            if kinds[p] == 0:
                m = min([_num(float(tol), c[0]) - (sum(_num(facets[f][j], c[0]) * c[j] for j in range(3)) - _num(facets[f][3], c[0]))
                         for f in range(int(fo[p]), int(fo[p + 1]))], default=math.inf)
            elif kinds[p] == 1:
                m = halfspace_margin(vw, aux[p], tol)
            else:
                m = box_margin(vw, aux[p][:4], tol)
            best = m if best is None or m > best else best
        if best is None:
            best = -math.inf  # a region without parts contains nothing
        flags.append(best >= 0)
        margin = min(margin, abs(best))
    return flags, margin


def region_flags(c, ro, kinds, fo, facets, aux, tol, c3_digits=8, vw=None):
    """region_lookup: (flags per region, first containing region or R, margin)."""
    vw = views(c) if vw is None else vw
    flags, margin = _region_flags(c, vw, ro, kinds, fo, facets, aux, tol)
    if abs(float(c[2])) * 10 ** c3_digits <= 0.5:  # c3 rounds to 0: the kernel may hold the mirrored representative
        f2, m2 = _region_flags((1 - c[0], c[1], c[2]), vw, ro, kinds, fo, facets, aux, tol)
        margin = min(margin, m2) if f2 == flags else 0.0
    first = next((r for r, f in enumerate(flags) if f), len(flags))
    return flags, first, margin


def rounds_safely(c) -> bool:
    """No coordinate * 1e8 within 1e-4 of a half-integer: np.round(reference, 8) is what any fp64 evaluation within 1e-13 rounds to."""
    for x in c:
        y = x * 10 ** 8
        if abs(y - _floor(y) - (0.5 if isinstance(y, float) else mpf(1) / 2)) <= HALF_INTEGER_GUARD:
            return False
    return True


# ---- fixture (NumPy only) -------------------------------------------------------------------------------------------------
BIT_KEYS = ("t", "ref", "e_ref", "x", "points", "bounds", "facets", "aux", "point", "tols", "gcoords")
COMPLEX_KEYS = ("k1", "k2", "g", "targets", "gates")


def save_fixture(path, groups) -> None:
    """The bit-exact format of ``hp_ref.save_fixture`` with this fixture's array names."""
    saved = hp.BIT_KEYS, hp.COMPLEX_KEYS
    hp.BIT_KEYS, hp.COMPLEX_KEYS = BIT_KEYS, COMPLEX_KEYS
    try:
        hp.save_fixture(path, groups)
    finally:
        hp.BIT_KEYS, hp.COMPLEX_KEYS = saved


def load_fixture(path=FIXTURE):
    return hp.load_fixture(path)


def build_unitaries(t, k1, k2, g) -> np.ndarray:
    """U[n] = g[n] K1[n] diag(d(t[n])) K2[n], d = ((1 - t^2) + 2 i t) / (1 + t^2): one IEEE operation per NumPy call, real arrays,
    a fixed order of additions -- the same bits on every machine."""
    t = np.ascontiguousarray(t, dtype=np.float64)
    tt = np.multiply(t, t)
    den = np.add(1.0, tt)
    dr = np.divide(np.subtract(1.0, tt), den)
    di = np.divide(np.add(t, t), den)
    ar, ai, br, bi = (np.ascontiguousarray(v) for v in (k1.real, k1.imag, k2.real, k2.imag))
    # A = K1 diag(d): column k scaled
    pr = np.subtract(np.multiply(ar, dr[:, None, :]), np.multiply(ai, di[:, None, :]))
    pi = np.add(np.multiply(ar, di[:, None, :]), np.multiply(ai, dr[:, None, :]))
    ur = np.zeros((len(t), 4, 4))
    ui = np.zeros((len(t), 4, 4))
    for k in range(4):
        a_r, a_i, b_r, b_i = pr[:, :, k, None], pi[:, :, k, None], br[:, None, k, :], bi[:, None, k, :]
        ur = np.add(ur, np.subtract(np.multiply(a_r, b_r), np.multiply(a_i, b_i)))
        ui = np.add(ui, np.add(np.multiply(a_r, b_i), np.multiply(a_i, b_r)))
    gr, gi = np.ascontiguousarray(g.real)[:, None, None], np.ascontiguousarray(g.imag)[:, None, None]
    out = np.empty((len(t), 4, 4), dtype=np.complex128)
    out.real = np.subtract(np.multiply(gr, ur), np.multiply(gi, ui))
    out.imag = np.add(np.multiply(gr, ui), np.multiply(gi, ur))
    return out


def checksum(U) -> int:
    """A 64-bit sum of the bit patterns (position-weighted) of a complex128 array."""
    u = hp.bits(U).ravel()
    w = (np.arange(u.size, dtype=np.uint64) * np.uint64(2654435761) + np.uint64(1)) | np.uint64(1)
    return int(np.sum(u * w, dtype=np.uint64))


def unitaries_of(group, bank) -> np.ndarray:
    """The matrices of a fixture group: stored whole (``targets``) or built from (t, pair, phase)."""
    if "targets" in group:
        U = group["targets"]
    else:
        U = build_unitaries(group["t"], bank["k1"][group["pair"]], bank["k2"][group["pair"]], bank["g"][group["phase"]])
    if checksum(U) != int(group["meta"]["checksum"]):
        raise AssertionError(f"group {group['meta']['name']}: the rebuilt matrices differ from the ones the reference was computed from")
    return U


def mirror_ok(ref) -> np.ndarray:
    """Where the comparison is modulo c1 -> 1 - c1: |c3_ref| <= 5e-9 (the rule of ``_canon`` in tests/test_gpu_weyl.py)."""
    return np.abs(np.asarray(ref)[:, 2]) <= 5e-9


def distance(got, ref) -> np.ndarray:
    """max_j |got_j - ref_j| per case, modulo the c3 = 0 mirror only where ``mirror_ok``."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    d = np.max(np.abs(got - ref), axis=1)
    m = got.copy()
    m[:, 0] = 1.0 - m[:, 0]
    return np.where(mirror_ok(ref), np.minimum(d, np.max(np.abs(m - ref), axis=1)), d)


def chamber_violation(c) -> np.ndarray:
    """How far each point is outside 0 <= c1 <= 1, c2 <= min(c1, 1 - c1), 0 <= c3 <= c2 (0: inside)."""
    c = np.asarray(c, dtype=np.float64)
    c1, c2, c3 = c[:, 0], c[:, 1], c[:, 2]
    v = np.stack([-c1, c1 - 1.0, c2 - c1, c2 - (1.0 - c1), -c3, c3 - c2], axis=1)
    return np.maximum(v.max(axis=1), 0.0)


def rounded_equal(got, ref) -> np.ndarray:
    """got == np.round(ref, 8), up to the mirror only where the reference's c3 rounds to 0."""
    got = np.asarray(got, dtype=np.float64)
    want = np.round(np.asarray(ref, dtype=np.float64), 8) + 0.0
    eq = np.all(got == want, axis=1)
    m = want.copy()
    m[:, 0] = np.round(1.0 - np.asarray(ref)[:, 0], 8)
    return eq | ((want[:, 2] == 0.0) & np.all(got == m, axis=1))


def tolerance(e_ref) -> float:
    """8 * max(e_ref), never above 1e-13: ``hp_ref.TOL_FACTOR`` and ``TOL_CAP``."""
    return min(hp.TOL_FACTOR * float(np.max(e_ref)), hp.TOL_CAP)


class Table:
    """kinds / points / bounds as ``_ffi.Context.coverage_lookup`` reads them."""

    def __init__(self, kinds, points, bounds):
        self.kinds = np.asarray(kinds, dtype=np.int32)
        self.points = np.asarray(points, dtype=np.float64).reshape(-1, 4)
        self.bounds = np.asarray(bounds, dtype=np.float64).reshape(-1, 14)

    def __len__(self):
        return len(self.kinds)
