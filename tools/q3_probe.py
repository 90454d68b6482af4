"""Throughput of the three-qubit optimizer kernel (csrc/slam_q3.hpp: minimize_q3_kernel) next to the two-qubit kernel that runs the
same quasi-Newton iteration on a 4x4 chain at the same number of gates -- minimize_long_kernel from six gates on, the quad kernel
below (slam_minimize_stage picks it) -- in one process: 4096 Haar targets x 8 restarts, one stage, no early exit, sqrt(iSWAP), at
k = 3, 6, 12; the three-qubit template on the edges cycling (0, 1), (1, 2).  Writes profiles/q3_probe.json.

    python tools/q3_probe.py [--targets 4096] [--restarts 8] [--out profiles/q3_probe.json]
"""
import argparse
import json
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from slam_decomposition_amd import _ffi  # noqa: E402
from slam_decomposition_amd.basis3q import ThreeQubitCircuitTemplate  # noqa: E402
from slam_decomposition_amd.gates import RiSwapGate, gate_matrix  # noqa: E402


def haar(rng, dim):
    z = (rng.standard_normal((dim, dim)) + 1j * rng.standard_normal((dim, dim))) / math.sqrt(2.0)
    q, r = np.linalg.qr(z)
    d = np.diagonal(r)
    return q * (d / np.abs(d))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--targets", type=int, default=4096)
    ap.add_argument("--restarts", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "q3_probe.json"))
    a = ap.parse_args()
    rng = np.random.default_rng(20260)
    targets8 = np.stack([haar(rng, 8) for _ in range(a.targets)])
    gate = gate_matrix(RiSwapGate(1 / 2))
    basis = ThreeQubitCircuitTemplate([RiSwapGate(1 / 2)], [[(0, 1)], [(1, 2)]], maximum_span_guess=15)
    prm = _ffi.OptParams(restarts=a.restarts, maxiter=2500, gtol=1e-9, stop_loss=1e-13, seed=1, flags=0)
    rows = []
    with _ffi.Context(0) as ctx:
        name, cus, _ = ctx.device_info()
        ctx.sample_haar(20260, a.targets)
        ctx.set_gates(gate[None])
        for k in (3, 6, 12):
            row = {"k": k}
            for rep in range(2):  # (the first pass of a kernel pays its load)
                out = ctx.q3_minimize(basis.gate_matrices, basis.gate_sequence(k), basis.edge_sequence(k), targets8, prm, 1e-10)
            ev = int(out["item_evals"].sum())
            row["q3"] = {"n_params": 9 + 6 * k, "kernel_ms": out["kernel_ms"], "evals": ev, "evals_per_s": ev / (out["kernel_ms"] * 1e-3),
                         "ns_per_eval": out["kernel_ms"] * 1e6 / ev, "mean_evals_per_item": ev / out["item_evals"].size,
                         "median_loss": float(np.median(out["best_loss"]))}
            for rep in range(2):
                ctx.reset_stats()
                ctx.minimize_stage([0] * k, prm, want_items=False)
                st = ctx.stats()
            ev = int(st["evals"][k])
            row["two_qubit"] = {"kernel": "minimize_long_kernel" if k > _ffi.MAX_SPAN_QUAD else "minimize_kernel (quad)", "n_params": 6 * (k + 1),
                                "kernel_ms": st["kernel_ms"], "evals": ev, "evals_per_s": ev / (st["kernel_ms"] * 1e-3),
                                "ns_per_eval": st["kernel_ms"] * 1e6 / ev, "mean_evals_per_item": ev / (a.targets * a.restarts)}
            row["ns_per_eval_ratio"] = row["q3"]["ns_per_eval"] / row["two_qubit"]["ns_per_eval"]
            rows.append(row)
            print(json.dumps(row))
    doc = {"what": "one optimizer stage, targets x restarts items, no early exit, sqrt(iSWAP); ns_per_eval = kernel time / fused loss+gradient "
                   "evaluations (throughput of the whole chip)", "device": name, "compute_units": cus, "targets": a.targets, "restarts": a.restarts,
           "rows": rows}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
