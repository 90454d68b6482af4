"""NumPy model of the state objectives of the three-qubit templates (cost_function.MutualInformation / MutualInformationSquare,
csrc/slam_q3.hpp STATE = true): tests/q3m_ref.py's factors applied to a start state, the LITERAL definition of the objective -- 2x2 and
4x4 partial traces, ``eigvalsh``, base 2 -- and its analytic gradient from dS = -Tr(d rho log2 rho) over stored prefix and suffix
products.  Nothing of the kernel's scheme: no determinant, no S(rho_ab) = S(rho_c), no series.

Conventions: a state is 8 amplitudes, basis index q0 + 2 q1 + 4 q2; ``pair[q]`` is the pair of qubits left when q is traced out, and
the objective's term q is I(a:b) = S(rho_a) + S(rho_b) - S(rho_ab) for (a, b) = pair[q] (qiskit's ``partial_trace(sv, [q])`` and
``mutual_information``).  log2 of a singular rho is taken on its support: a zero eigenvalue of a positive matrix moves at second order,
so it adds nothing to dS (the convention of the kernel at a product state)."""
import numpy as np

import q3_ref
import q3m_ref

PAIR = {0: (1, 2), 1: (0, 2), 2: (0, 1)}
EIG_FLOOR = 1e-300


def w_state():
    v = np.zeros(8, dtype=np.complex128)
    v[[1, 2, 4]] = 1.0 / np.sqrt(3.0)
    return v


def ghz_state():
    v = np.zeros(8, dtype=np.complex128)
    v[[0, 7]] = 1.0 / np.sqrt(2.0)
    return v


def pre_ghz_state():
    """(|000> + |101>) / sqrt 2: a CX on (0, 1) maps it onto GHZ."""
    v = np.zeros(8, dtype=np.complex128)
    v[[0, 5]] = 1.0 / np.sqrt(2.0)
    return v


def random_state(rng):
    v = rng.normal(size=8) + 1j * rng.normal(size=8)
    return v / np.linalg.norm(v)


def partial_trace(rho8, keep):
    """The state of the qubits ``keep`` (index sum_i bit_{keep[i]} << i) of the 8x8 rho8."""
    rest = [q for q in range(3) if q not in keep]
    d = 1 << len(keep)
    out = np.zeros((d, d), dtype=np.complex128)
    for r in range(1 << len(rest)):
        idx = [sum(((i >> j) & 1) << q for j, q in enumerate(keep)) + sum(((r >> j) & 1) << q for j, q in enumerate(rest)) for i in range(d)]
        out += rho8[np.ix_(idx, idx)]
    return out


def entropy(rho):
    ev = np.linalg.eigvalsh(rho)
    ev = ev[ev > EIG_FLOOR]
    return float(-np.sum(ev * np.log2(ev)))


def log2_on_support(rho):
    ev, vec = np.linalg.eigh(rho)
    lg = np.where(ev > EIG_FLOOR, np.log2(np.where(ev > EIG_FLOOR, ev, 1.0)), 0.0)
    return (vec * lg) @ vec.conj().T


def lift(op, keep):
    """op on the qubits ``keep`` (1 or 2 of them, ascending) times the identity on the rest, as an 8x8."""
    return q3_ref.embed_1q(op, keep[0]) if len(keep) == 1 else q3_ref.embed_2q(op, keep[0], keep[1])


def mutual_informations(v):
    """(I(1:2), I(0:2), I(0:1)) of the state v."""
    rho8 = np.outer(v, v.conj())
    s1 = [entropy(partial_trace(rho8, (q,))) for q in range(3)]
    return tuple(s1[PAIR[q][0]] + s1[PAIR[q][1]] - entropy(partial_trace(rho8, PAIR[q])) for q in range(3))


def qubit_entropies(v):
    rho8 = np.outer(v, v.conj())
    return tuple(entropy(partial_trace(rho8, (q,))) for q in range(3))


def monotone(v, square=False):
    mi = mutual_informations(v)
    return float(sum(i * i for i in mi)) if square else float(sum(mi))


def monotone_and_operator(v, square=False):
    """(L, K): the objective and the Hermitian 8x8 K with dL = Tr(K d|v><v|) = 2 Re(v^+ K dv)."""
    rho8 = np.outer(v, v.conj())
    mi = mutual_informations(v)
    k = np.zeros((8, 8), dtype=np.complex128)
    for q in range(3):
        a, b = PAIR[q]
        # dI = -Tr(d rho_a log2 rho_a) - Tr(d rho_b log2 rho_b) + Tr(d rho_ab log2 rho_ab)
        kq = -lift(log2_on_support(partial_trace(rho8, (a,))), (a,)) - lift(log2_on_support(partial_trace(rho8, (b,))), (b,)) \
            + lift(log2_on_support(partial_trace(rho8, (a, b))), (a, b))
        k += (2.0 * mi[q] if square else 1.0) * kq
    f = float(sum(i * i for i in mi)) if square else float(sum(mi))
    return f, k


def final_state(x, gates, edges, psi):
    v = np.asarray(psi, dtype=np.complex128)
    for m, _ in q3m_ref.factors(x, gates, edges):
        v = m @ v
    return v


def loss(x, gates, edges, psi, square=False):
    return monotone(final_state(x, gates, edges, psi), square)


def loss_grad(x, gates, edges, psi, square=False):
    """(loss, gradient [n], final state [8])."""
    fs = q3m_ref.factors(x, gates, edges)
    pre = [np.asarray(psi, dtype=np.complex128)]  # pre[l] = F_{l-1} ... F_0 psi
    for m, _ in fs:
        pre.append(m @ pre[-1])
    v = pre[-1]
    f, k = monotone_and_operator(v, square)
    g = np.zeros(len(x))
    suf = v.conj() @ k  # v^+ K F_{L-1} ... F_{l+1}
    for l in range(len(fs) - 1, -1, -1):
        m, ds = fs[l]
        for idx, dm in ds:
            g[idx] = float(2.0 * np.real(suf @ (dm @ pre[l])))
        suf = suf @ m
    return f, g, v


def purities(v):
    """Tr rho_q^2 for q = 0, 1, 2."""
    rho8 = np.outer(v, v.conj())
    return tuple(float(np.real(np.trace(r @ r))) for r in (partial_trace(rho8, (q,)) for q in range(3)))
