"""What an evaluation of a Hamiltonian template costs inside the optimizer kernel (csrc/slam_ham.hpp, minimize_ham_kernel), next to the
three-qubit circuit kernel and to SciPy on the host -- one job on one box, writes profiles/ham_probe.json:

  device   ns per fused loss + gradient evaluation inside slam_ham_minimize for the CirculatorHamiltonian (7 parameters) and the
           DeltaConversionGainHamiltonian (12), 4096 Haar 8x8 targets x 8 restarts, BasicCost, no early exit; next to slam_q3_minimize
           for the sqrt(iSWAP) line template at k = 3 (27 parameters) in the same process, the three alternating, several repetitions;
  host     targets per second of SciPy BFGS on the host model tests/ham_ref.py (analytic gradient, the same start points and
           tolerances) on up to 16 cores, on the first targets of the same batch, next to the device's.

Boxes of one pool differ by several per cent: only numbers of one job compare.

    python tools/ham_probe.py [--targets 4096] [--restarts 8] [--reps 3] [--host-targets 32]
"""
import argparse
import json
import math
import multiprocessing
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def haar(rng, dim):
    z = (rng.standard_normal((dim, dim)) + 1j * rng.standard_normal((dim, dim))) / math.sqrt(2.0)
    q, r = np.linalg.qr(z)
    d = np.diagonal(r)
    return q * (d / np.abs(d))


def hamiltonians():
    from slam_decomposition_amd import hamiltonian as hm

    return {"circulator": hm.CirculatorHamiltonian(), "delta": hm.DeltaConversionGainHamiltonian()}


def start_points(name, n_targets, restarts):
    """phases in [-pi, pi), strengths in [0, 2), t = 1"""
    terms = hamiltonians()[name].device_terms()
    n = terms["n_params"]
    low, high = np.zeros(n), np.full(n, 2.0)
    for p in terms["phi_index"]:
        if p >= 0:
            low[p], high[p] = -math.pi, math.pi
    if terms["t_index"] >= 0:
        low[terms["t_index"]] = high[terms["t_index"]] = 1.0
    return np.random.default_rng(7).uniform(low, high, (n_targets, restarts, n))


def host_job(job):
    """All restarts of one target by SciPy BFGS on the model; returns the number of evaluations."""
    import ham_ref
    from scipy.optimize import minimize

    name, target, x0 = job
    terms = hamiltonians()[name].device_terms()
    evals = 0
    for x in x0:
        res = minimize(lambda v: ham_ref.loss_grad(terms, v, target, False)[:2], x, jac=True, method="BFGS", options={"gtol": 1e-9, "maxiter": 2500})
        evals += int(res.nfev)
    return evals


def summary(ms, out, n_params, n_targets):
    ev = int(out["item_evals"].sum())
    med = float(np.median(ms))
    return {"n_params": n_params, "kernel_ms": [float(v) for v in ms], "kernel_ms_median": med, "spread": (max(ms) - min(ms)) / med, "evals": ev,
            "ns_per_eval": med * 1e6 / ev, "mean_evals_per_item": ev / out["item_evals"].size, "targets_per_s": n_targets / (med * 1e-3),
            "median_best_loss": float(np.median(out["best_loss"]))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--targets", type=int, default=4096)
    ap.add_argument("--restarts", type=int, default=8)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--host-targets", type=int, default=32)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ham_probe.json"))
    a = ap.parse_args()
    rng = np.random.default_rng(20260)  # (tools/q3_probe.py's targets)
    targets8 = np.stack([haar(rng, 8) for _ in range(a.targets)])
    x0 = {name: start_points(name, a.targets, a.restarts) for name in hamiltonians()}

    # ---- host first: its worker processes are started before this process opens the device
    cores = min(16, os.cpu_count() or 1)
    host = {}
    with multiprocessing.get_context("spawn").Pool(cores) as pool:
        for name in hamiltonians():
            jobs = [(name, targets8[t], x0[name][t]) for t in range(a.host_targets)]
            pool.map(host_job, jobs[:cores])  # (imports paid)
            t0 = time.perf_counter()
            evals = pool.map(host_job, jobs)
            dt = time.perf_counter() - t0
            host[name] = {"targets": a.host_targets, "restarts": a.restarts, "processes": cores, "seconds": dt, "targets_per_s": a.host_targets / dt,
                          "evals": int(sum(evals)), "us_per_eval_per_core": dt * cores * 1e6 / sum(evals)}
            print("host", name, json.dumps(host[name]), flush=True)

    from slam_decomposition_amd import _ffi
    from slam_decomposition_amd.basis3q import ThreeQubitCircuitTemplate
    from slam_decomposition_amd.gates import RiSwapGate

    prm = _ffi.OptParams(restarts=a.restarts, maxiter=2500, gtol=1e-9, stop_loss=1e-13, seed=1, flags=0)
    line = ThreeQubitCircuitTemplate([RiSwapGate(1 / 2)], [[(0, 1)], [(1, 2)]], maximum_span_guess=15)
    terms = {name: h.device_terms() for name, h in hamiltonians().items()}
    with _ffi.Context(0) as ctx:
        device, cus, _ = ctx.device_info()
        calls = {"circulator": lambda: ctx.ham_minimize(terms["circulator"], targets8, prm, 1e-10, x0["circulator"]),
                 "delta": lambda: ctx.ham_minimize(terms["delta"], targets8, prm, 1e-10, x0["delta"]),
                 "q3_k3": lambda: ctx.q3_minimize(line.gate_matrices, line.gate_sequence(3), line.edge_sequence(3), targets8, prm, 1e-10)}
        ms = {key: [] for key in calls}
        last = {}
        for rep in range(a.reps + 1):  # (the first pass of a kernel pays its load); the three alternate
            for key, call in calls.items():
                last[key] = call()
                if rep:
                    ms[key].append(last[key]["kernel_ms"])
    n_of = {"circulator": 7, "delta": 12, "q3_k3": 27}
    dev = {key: summary(ms[key], last[key], n_of[key], a.targets) for key in calls}
    for key in dev:
        print("device", key, json.dumps(dev[key]), flush=True)
    doc = {"what": "one optimizer stage, targets x restarts items, BasicCost, no early exit, Haar 8x8 targets; ns_per_eval = median kernel time "
                   "over the repetitions / fused loss+gradient evaluations (throughput of the whole chip); spread = (max - min) / median; host = "
                   "SciPy BFGS on tests/ham_ref.py from the same start points, one process per core",
           "device": device, "compute_units": cus, "targets": a.targets, "restarts": a.restarts, "reps": a.reps, "kernels": dev, "host": host,
           "ratios": {"ham_over_q3_k3_ns_per_eval": {k: dev[k]["ns_per_eval"] / dev["q3_k3"]["ns_per_eval"] for k in ("circulator", "delta")},
                      "device_over_host_targets_per_s": {k: dev[k]["targets_per_s"] / host[k]["targets_per_s"] for k in ("circulator", "delta")}}}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
    print("ratios", json.dumps(doc["ratios"]))
    print("wrote", a.out)


if __name__ == "__main__":
    main()
