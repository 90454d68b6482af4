"""What the state objective costs in the three-qubit optimizer kernel (csrc/slam_q3.hpp, STATE = true): ns per fused loss + gradient
evaluation inside slam_q3s_minimize next to slam_q3m_minimize on the same template, in the same process, alternating.  Writes
profiles/q3s_probe.json.

Two templates: three CX on the line (0, 1), (1, 2), (0, 1) (n = 27; both calls run the two-qubit-only instantiations) and CX / CCZ / CX
(n = 30; the mixed ones).  The unitary objective gets Haar 8x8 targets under BasicCost, the state objective Haar-random start states
under MutualInformation; no early exit, so every item runs to its own end.  The two objectives take different numbers of iterations,
which is why the figure is per evaluation.  Boxes of one pool differ by several per cent: only numbers of one run compare.

    python tools/q3s_probe.py [--items 4096] [--restarts 8] [--reps 5] [--out profiles/q3s_probe.json]
"""
import argparse
import json
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def haar(rng, dim):
    z = (rng.standard_normal((dim, dim)) + 1j * rng.standard_normal((dim, dim))) / math.sqrt(2.0)
    q, r = np.linalg.qr(z)
    d = np.diagonal(r)
    return q * (d / np.abs(d))


def summary(ms, out, n_params):
    ev = int(out["item_evals"].sum())
    med = float(np.median(ms))
    return {"n_params": n_params, "kernel_ms": [float(v) for v in ms], "kernel_ms_median": med, "spread": (max(ms) - min(ms)) / med, "evals": ev,
            "ns_per_eval": med * 1e6 / ev, "mean_evals_per_item": ev / out["item_evals"].size, "median_loss": float(np.median(out["best_loss"]))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--items", type=int, default=4096)
    ap.add_argument("--restarts", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "q3s_probe.json"))
    a = ap.parse_args()

    from slam_decomposition_amd import _ffi
    from slam_decomposition_amd.gates import CCZGate, CXGate, gate_matrix

    rng = np.random.default_rng(20261)
    targets = np.stack([haar(rng, 8) for _ in range(a.items)])
    states = targets[:, :, 0].copy()  # (a column of a Haar unitary is a Haar-random state)
    cx, ccz = gate_matrix(CXGate())[None], gate_matrix(CCZGate())[None]
    templates = {"cx_line_k3": (cx, np.zeros((0, 8, 8)), [2, 2, 2], [0, 0, 0], [(0, 1, 0), (1, 2, 0), (0, 1, 0)]),
                 "cx_ccz_cx": (cx, ccz, [2, 3, 2], [0, 0, 0], [(0, 1, 0), (0, 1, 2), (1, 2, 0)])}
    prm = _ffi.OptParams(restarts=a.restarts, maxiter=2500, gtol=1e-9, stop_loss=1e-13, seed=1, flags=0)
    rows = {}
    with _ffi.Context(0) as ctx:
        name, cus, _ = ctx.device_info()
        for key, desc in templates.items():
            n = 9 + 3 * sum(desc[2])
            ms_u, ms_s = [], []
            for rep in range(a.reps + 1):  # (the first pass of a kernel pays its load); the two calls alternate
                out_u = ctx.q3m_minimize(*desc, targets, prm, 1e-10, cost_kind=_ffi.COST_BASIC)
                out_s = ctx.q3s_minimize(*desc, states, prm, 1e-10, cost_kind=_ffi.COST_MUTUAL_INFO)
                if rep:
                    ms_u.append(out_u["kernel_ms"])
                    ms_s.append(out_s["kernel_ms"])
            row = {"q3m_minimize_basic": summary(ms_u, out_u, n), "q3s_minimize_mutual_information": summary(ms_s, out_s, n)}
            row["ns_per_eval_ratio_state_over_unitary"] = row["q3s_minimize_mutual_information"]["ns_per_eval"] / row["q3m_minimize_basic"]["ns_per_eval"]
            rows[key] = row
            print(key, json.dumps(row), flush=True)
    doc = {"what": "one optimizer stage, items x restarts work items, no early exit; ns_per_eval = median kernel time over the repetitions / fused "
                   "loss+gradient evaluations (throughput of the whole chip); spread = (max - min) / median over them; the two calls alternate "
                   "within one process",
           "device": name, "compute_units": cus, "items": a.items, "restarts": a.restarts, "reps": a.reps, "templates": rows}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
