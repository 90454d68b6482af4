"""Host model of the time-sliced Hamiltonian templates (csrc/slam_hams.hpp), the literal definition on the helpers of tests/ham_ref.py:

    U = U_S ... U_1,   U_s = exp(-i (t / S) H_s)  from numpy.linalg.eigh of every slice, the product taken in slice order,
    z = Tr(T^+ U) / d,   P_s = U_s ... U_1 (P_0 = 1),   Q_s = U_S ... U_s (Q_{S+1} = 1),   T_s^+ = P_{s-1} T^+ Q_{s+1},

and per slice the single-exponential divided-difference formula with T_s in the place of T and tau = t / S in the place of t:
B = V_s^+ T_s^+ V_s, Phi, K = V_s (B o Phi) V_s^+, dz/dx_j += (-i tau / d) Tr(K dH_s/dx_j); dz/dt = (1 / S) sum_s (1 / d) sum_a B_aa (-i l_a) e_a.
A description is ``hamiltonian.TimeSliced.device_terms()``: ``n_slices`` and index arrays [S, K]."""
import numpy as np

import ham_ref


def slice_terms(terms, s):
    out = {k: v for k, v in terms.items() if k != "n_slices"}
    out["s_index"], out["phi_index"] = terms["s_index"][s], terms["phi_index"][s]
    return out


def slice_unitaries(terms, x):
    S = int(terms["n_slices"])
    tau = ham_ref.time_of(terms, x) / S
    out = []
    for s in range(S):
        w, v = np.linalg.eigh(ham_ref.hamiltonian(slice_terms(terms, s), x))
        out.append((w, v, (v * np.exp(-1j * tau * w)) @ v.conj().T))
    return tau, out


def unitary(terms, x):
    x = np.asarray(x, dtype=np.float64)
    total = np.eye(int(terms["dim"]), dtype=np.complex128)
    for _, _, u in slice_unitaries(terms, x)[1]:
        total = u @ total
    return total


def loss_grad(terms, x, target, square=False):
    """(loss, gradient [n], U) at x for one dim x dim target (any finite matrix)."""
    x = np.asarray(x, dtype=np.float64)
    d, n, S = int(terms["dim"]), int(terms["n_params"]), int(terms["n_slices"])
    tau, sl = slice_unitaries(terms, x)
    prefix = [np.eye(d, dtype=np.complex128)]  # P_0 .. P_S
    for _, _, u in sl:
        prefix.append(u @ prefix[-1])
    suffix = [np.eye(d, dtype=np.complex128)]  # Q_{S+1}, Q_S, .. Q_1
    for _, _, u in reversed(sl):
        suffix.append(suffix[-1] @ u)
    suffix = suffix[::-1]                      # suffix[s] = Q_{s+1} for the 0-based slice s - 1, i.e. suffix[s + 1] follows slice s
    u_total = prefix[-1]
    td = np.asarray(target, dtype=np.complex128).conj().T
    z = np.trace(td @ u_total) / d
    az = abs(z)
    loss = ham_ref.cost_of_z(az, d, square)
    dl = (2.0 * d * az / (d + 1.0)) if square else 1.0
    sigma = -dl * np.conj(z) / az if az > 0.0 else 0.0
    g = np.zeros(n)
    dz_dt = 0.0
    for s, (lam, v, _) in enumerate(sl):
        ts_dag = prefix[s] @ td @ suffix[s + 1]
        e = np.exp(-1j * tau * lam)
        b = v.conj().T @ ts_dag @ v
        half_sum = 0.5 * tau * (lam[:, None] + lam[None, :])
        half_dif = 0.5 * tau * (lam[:, None] - lam[None, :])
        phi = np.exp(-1j * half_sum) * np.sinc(half_dif / np.pi)
        k = v @ (b * phi) @ v.conj().T
        for m, si, pi in zip(terms["matrices"], terms["s_index"][s], terms["phi_index"][s]):
            ph = np.exp(1j * (x[pi] if pi >= 0 else 0.0))
            dh_s = ph * m + np.conj(ph) * m.conj().T
            g[si] += np.real(sigma * (-1j * tau / d) * np.trace(k @ dh_s))
            if pi >= 0:
                dh_p = 1j * x[si] * ph * m
                dh_p = dh_p + dh_p.conj().T
                g[pi] += np.real(sigma * (-1j * tau / d) * np.trace(k @ dh_p))
        dz_dt = dz_dt + np.sum(np.diag(b) * (-1j * lam) * e) / d / S
    if terms["t_index"] >= 0:
        g[terms["t_index"]] += np.real(sigma * dz_dt)
    return loss, g, u_total


def batch(terms, xs, targets, target_of, square=False):
    out = [loss_grad(terms, xs[m], targets[target_of[m]], square) for m in range(len(xs))]
    return np.array([o[0] for o in out]), np.stack([o[1] for o in out]), np.stack([o[2] for o in out])
