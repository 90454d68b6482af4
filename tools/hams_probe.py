"""What an evaluation of a time-sliced Hamiltonian template costs inside the optimizer kernel (csrc/slam_hams.hpp, minimize_hams_kernel)
as the number of slices grows, next to the single-exponential kernel and to SciPy on the host -- one job on one box, writes
profiles/hams_probe.json:

  device   ns per fused loss + gradient evaluation inside slam_hams_minimize at S = 1, 2, 4, 8 for the sliced circulator (8x8, the
           three strengths per slice, 3 + 3 S + 1 parameters) and for ConversionGainSmush1QPhase (4x4, 8 + 2 S + 1 parameters), Haar
           targets x 8 restarts, BasicCost, no early exit; next to slam_ham_minimize on the unsliced circulator in the same process,
           the kernels alternating, medians of several repetitions;
  host     targets per second of SciPy BFGS on the host model tests/hams_ref.py (analytic gradient, the same start points and
           tolerances) on up to 16 cores, on the first targets of the same batches.

Reported: the S = 1 ratio to slam_ham_minimize and the slope per slice (least squares of ns per evaluation over S).  Boxes of one pool
differ by several per cent: only numbers of one job compare.

    python tools/hams_probe.py [--targets 4096] [--restarts 8] [--reps 3] [--host-targets 16]
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

SLICES = (1, 2, 4, 8)
PULSES = ("circulator", "smush1q")


def haar(rng, dim):
    z = (rng.standard_normal((dim, dim)) + 1j * rng.standard_normal((dim, dim))) / math.sqrt(2.0)
    q, r = np.linalg.qr(z)
    d = np.diagonal(r)
    return q * (d / np.abs(d))


def pulse(name, n_slices):
    from slam_decomposition_amd import hamiltonian as hm

    if name == "smush1q":
        return hm.ConversionGainSmush1QPhase(n_slices=n_slices)
    return hm.TimeSliced(hm.CirculatorHamiltonian(), n_slices, sliced=("g_ab", "g_ac", "g_bc"))


def start_points(terms, n_targets, restarts):
    """phases in [-pi, pi), strengths in [0, 2), t = 1"""
    n = terms["n_params"]
    low, high = np.zeros(n), np.full(n, 2.0)
    for p in np.asarray(terms["phi_index"]).ravel():
        if p >= 0:
            low[p], high[p] = -math.pi, math.pi
    if terms["t_index"] >= 0:
        low[terms["t_index"]] = high[terms["t_index"]] = 1.0
    return np.random.default_rng(7).uniform(low, high, (n_targets, restarts, n))


def host_job(job):
    """All restarts of one target by SciPy BFGS on the model; returns the number of evaluations."""
    import hams_ref
    from scipy.optimize import minimize

    name, n_slices, target, x0 = job
    terms = pulse(name, n_slices).device_terms()
    evals = 0
    for x in x0:
        res = minimize(lambda v: hams_ref.loss_grad(terms, v, target, False)[:2], x, jac=True, method="BFGS", options={"gtol": 1e-9, "maxiter": 2500})
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
    ap.add_argument("--host-targets", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hams_probe.json"))
    a = ap.parse_args()
    rng = np.random.default_rng(20260)
    targets = {"circulator": np.stack([haar(rng, 8) for _ in range(a.targets)]), "smush1q": np.stack([haar(rng, 4) for _ in range(a.targets)])}
    terms = {(name, s): pulse(name, s).device_terms() for name in PULSES for s in SLICES}
    x0 = {key: start_points(t, a.targets, a.restarts) for key, t in terms.items()}

    # ---- host first: its worker processes are started before this process opens the device
    cores = min(16, os.cpu_count() or 1)
    host = {}
    with multiprocessing.get_context("spawn").Pool(cores) as pool:
        for (name, s) in terms:
            jobs = [(name, s, targets[name][t], x0[(name, s)][t]) for t in range(a.host_targets)]
            if not host:
                pool.map(host_job, jobs[:cores])  # (imports paid)
            t0 = time.perf_counter()
            evals = pool.map(host_job, jobs)
            dt = time.perf_counter() - t0
            host[f"{name}_S{s}"] = {"targets": a.host_targets, "restarts": a.restarts, "processes": cores, "seconds": dt,
                                    "targets_per_s": a.host_targets / dt, "evals": int(sum(evals)), "us_per_eval_per_core": dt * cores * 1e6 / sum(evals)}
            print("host", name, s, json.dumps(host[f"{name}_S{s}"]), flush=True)

    from slam_decomposition_amd import _ffi
    from slam_decomposition_amd import hamiltonian as hm

    prm = _ffi.OptParams(restarts=a.restarts, maxiter=2500, gtol=1e-9, stop_loss=1e-13, seed=1, flags=0)
    base = hm.CirculatorHamiltonian().device_terms()
    base_x0 = start_points(base, a.targets, a.restarts)
    with _ffi.Context(0) as ctx:
        device, cus, _ = ctx.device_info()
        calls = {"ham_circulator": lambda: ctx.ham_minimize(base, targets["circulator"], prm, 1e-10, base_x0)}
        for (name, s), t in terms.items():
            calls[f"{name}_S{s}"] = (lambda name=name, s=s, t=t: ctx.hams_minimize(t, targets[name], prm, 1e-10, x0[(name, s)]))
        ms = {key: [] for key in calls}
        last = {}
        for rep in range(a.reps + 1):  # (the first pass of a kernel pays its load); the kernels alternate
            for key, call in calls.items():
                last[key] = call()
                if rep:
                    ms[key].append(last[key]["kernel_ms"])
    n_of = {"ham_circulator": 7, **{f"{name}_S{s}": t["n_params"] for (name, s), t in terms.items()}}
    dev = {key: summary(ms[key], last[key], n_of[key], a.targets) for key in calls}
    for key in dev:
        print("device", key, json.dumps(dev[key]), flush=True)
    slope = {}
    for name in PULSES:
        ns = [dev[f"{name}_S{s}"]["ns_per_eval"] for s in SLICES]
        k, c = np.polyfit(SLICES, ns, 1)
        slope[name] = {"ns_per_eval_per_slice": float(k), "intercept_ns": float(c)}
    doc = {"what": "one optimizer stage, targets x restarts items, BasicCost, no early exit, Haar targets; ns_per_eval = median kernel time over "
                   "the repetitions / fused loss+gradient evaluations (throughput of the whole chip); spread = (max - min) / median; slope = least "
                   "squares of ns_per_eval over S = 1, 2, 4, 8; host = SciPy BFGS on tests/hams_ref.py from the same start points, one process per "
                   "core",
           "device": device, "compute_units": cus, "targets": a.targets, "restarts": a.restarts, "reps": a.reps, "kernels": dev, "host": host,
           "ratios": {"hams_S1_over_ham_ns_per_eval": dev["circulator_S1"]["ns_per_eval"] / dev["ham_circulator"]["ns_per_eval"],
                      "slope": slope,
                      "device_over_host_targets_per_s": {k: dev[k]["targets_per_s"] / host[k]["targets_per_s"] for k in host}}}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
    print("ratios", json.dumps(doc["ratios"]))
    print("wrote", a.out)


if __name__ == "__main__":
    main()
