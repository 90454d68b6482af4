"""NumPy model of the mixed three-qubit templates (basis3q.py with three-qubit base gates, csrc/slam_q3.hpp MIXED = true): tests/q3_ref.py
plus positions that hold an 8x8 gate on an ordered triple.  As there: explicit Kronecker products and basis permutations, the gradient
from the product rule over stored prefix and suffix products -- nothing of the kernel's scheme.

Conventions: a position is (gate, edge).  A 4x4 gate takes an edge (a, b) and is followed by a U3 on a, on b; an 8x8 gate takes an edge
(a, b, c) of all three qubits -- gate-local basis index bit_a + 2 bit_b + 4 bit_c, like ``circuit.append(gate, [a, b, c])`` -- and is
followed by a U3 on a, on b, on c.  Parameters in circuit order: n = 9 + 3 * sum(len(edge))."""
import numpy as np

import q3_ref
from q3_ref import basic_cost, embed_1q, embed_2q, equal_up_to_phase, overlap, square_cost, u3  # noqa: F401  (re-exported)


def embed_3q(g, a, b, c):
    """The 8x8 g on the ordered triple (a, b, c), in the standard order (q0, q1, q2)."""
    g = np.asarray(g, dtype=np.complex128)
    assert sorted((a, b, c)) == [0, 1, 2]
    perm = np.zeros((8, 8))
    for s in range(8):
        perm[((s >> a) & 1) + 2 * ((s >> b) & 1) + 4 * ((s >> c) & 1), s] = 1.0  # |s> in standard order -> its index in (a, b, c) order
    return perm.T @ g @ perm


def n_params(edges):
    return 9 + 3 * sum(len(e) for e in edges)


def factors(x, gates, edges):
    """The circuit's 8x8 factors in time order, each with its parameters' derivatives: [(matrix, [(parameter index, dmatrix)])]."""
    x = np.asarray(x, dtype=np.float64)
    assert len(edges) == len(gates) and len(x) == n_params(edges)
    out = []

    def add_u(base, q):
        out.append((embed_1q(u3(*x[base : base + 3]), q), [(base + i, embed_1q(d, q)) for i, d in enumerate(q3_ref.du3(*x[base : base + 3]))]))

    for q in range(3):
        add_u(3 * q, q)
    base = 9
    for g, e in zip(gates, edges):
        g = np.asarray(g)
        assert g.shape == (1 << len(e),) * 2
        out.append((embed_2q(g, *e) if len(e) == 2 else embed_3q(g, *e), []))
        for q in e:
            add_u(base, q)
            base += 3
    return out


def unitary(x, gates, edges):
    w = np.eye(8, dtype=np.complex128)
    for m, _ in factors(x, gates, edges):
        w = m @ w
    return w


def loss(x, gates, edges, t, square=False):
    w = unitary(x, gates, edges)
    return square_cost(w, t) if square else basic_cost(w, t)


def loss_grad(x, gates, edges, t, square=False):
    """(loss, gradient [n], unitary): q3_ref.loss_grad over this module's factors."""
    fs = factors(x, gates, edges)
    pre = [np.eye(8, dtype=np.complex128)]  # pre[l] = F_{l-1} ... F_0
    for m, _ in fs:
        pre.append(m @ pre[-1])
    w = pre[-1]
    th = t.conj().T
    tr = np.trace(th @ w)
    a = abs(tr)
    if square:  # 1 - (|tr|^2 + 8) / 72
        f = 1.0 - (a * a + 8.0) / 72.0
        z = -2.0 * np.conj(tr) / 72.0
    else:  # 1 - |tr| / 8;  d|tr| = Re(conj(tr) dtr) / |tr|
        f = 1.0 - a / 8.0
        z = -np.conj(tr) / (8.0 * a) if a > 0 else 0.0
    g = np.zeros(len(x))
    suf = th  # T^+ F_{L-1} ... F_{l+1}
    for l in range(len(fs) - 1, -1, -1):
        m, ds = fs[l]
        for idx, dm in ds:
            g[idx] = float(np.real(z * np.trace(suf @ dm @ pre[l])))
        suf = suf @ m
    return float(f), g, w
