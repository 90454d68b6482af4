"""What a three-qubit position costs in the optimizer kernel (csrc/slam_q3.hpp, minimize_q3_kernel<true>), and that the two-qubit-only
kernel did not change -- one job on one box, every measurement in a fresh child process, writes profiles/q3m_probe.json:

  mixed    this build: ns per evaluation inside slam_q3m_minimize for 10 VSwap on the triples cycling (0, 1, 2), (1, 2, 0) (n = 99), and
           inside slam_q3_minimize for the sqrt(iSWAP) line template of tools/q3_probe.py at k = 12 (n = 81) and k = 15 (n = 99); from
           these the cost of a position of either arity (the model is in the JSON);
  q3       minimize_q3_kernel<false> at k = 3, 6, 12 as tools/q3_probe.py runs it, several repetitions, for this build and for a build of
           the parent commit (--parent-lib), alternating, twice each: the ratio new / parent next to the spread over the repetitions;
  own      tools/q3_probe.py itself for both builds.

Boxes of one pool differ by several per cent: only numbers of one job compare.

    python tools/q3m_probe.py [--parent-lib path/to/parent/libslamhip.so] [--targets 4096] [--restarts 8] [--reps 5]
"""
import argparse
import json
import math
import os
import subprocess
import sys
import tempfile

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


def worker(a):
    """One child: the measurements of `a.worker` with the library the environment selects; one JSON document on the last line."""
    from slam_decomposition_amd import _ffi
    from slam_decomposition_amd.basis3q import ThreeQubitCircuitTemplate
    from slam_decomposition_amd.gates import RiSwapGate, VSwap

    rng = np.random.default_rng(20260)  # (tools/q3_probe.py's targets)
    targets8 = np.stack([haar(rng, 8) for _ in range(a.targets)])
    prm = _ffi.OptParams(restarts=a.restarts, maxiter=2500, gtol=1e-9, stop_loss=1e-13, seed=1, flags=0)
    line = ThreeQubitCircuitTemplate([RiSwapGate(1 / 2)], [[(0, 1)], [(1, 2)]], maximum_span_guess=15)
    doc = {}

    def timed(call):
        ms = []
        for rep in range(a.reps + 1):  # (the first pass of a kernel pays its load)
            out = call()
            if rep:
                ms.append(out["kernel_ms"])
        return ms, out

    with _ffi.Context(0) as ctx:
        name, cus, _ = ctx.device_info()
        doc["device"], doc["compute_units"] = name, cus
        if a.worker == "mixed":
            vs = ThreeQubitCircuitTemplate([VSwap()], [[(0, 1, 2)], [(1, 2, 0)]], maximum_span_guess=10)
            vs.build(10)
            ms, out = timed(lambda: ctx.q3m_minimize(vs.gate_matrices, vs.gate_matrices3, *vs.mixed_description(10), targets8, prm, 1e-10))
            doc["three_qubit_k10"] = summary(ms, out, vs.n_params)
            ks = (12, 15)
        else:
            ks = (3, 6, 12)
        for k in ks:
            ms, out = timed(lambda: ctx.q3_minimize(line.gate_matrices, line.gate_sequence(k), line.edge_sequence(k), targets8, prm, 1e-10))
            doc[f"two_qubit_k{k}"] = summary(ms, out, 9 + 6 * k)
    print(json.dumps(doc))


def child(args, lib):
    env = dict(os.environ)
    env.pop("SLAM_HIP_LIB", None)
    if lib:
        env["SLAM_HIP_LIB"] = os.path.abspath(lib)
    r = subprocess.run([sys.executable] + args, env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
        raise SystemExit(f"child {args} failed with status {r.returncode}: nothing more is started")
    return r.stdout


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--targets", type=int, default=4096)
    ap.add_argument("--restarts", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--parent-lib", default=None, help="libslamhip.so built from the parent commit")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "q3m_probe.json"))
    ap.add_argument("--worker", choices=["mixed", "q3"], default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.worker:
        return worker(a)
    me = [os.path.abspath(__file__), "--targets", str(a.targets), "--restarts", str(a.restarts), "--reps", str(a.reps)]

    def run_worker(kind, lib):
        doc = json.loads(child(me + ["--worker", kind], lib).strip().splitlines()[-1])
        print(kind, "parent" if lib else "this", json.dumps(doc), flush=True)
        return doc

    mixed = run_worker("mixed", None)
    t3, t12, t15 = (mixed[key]["ns_per_eval"] for key in ("three_qubit_k10", "two_qubit_k12", "two_qubit_k15"))
    p2 = (t15 - t12) / 3.0
    p3 = (t3 - (t15 - 15.0 * p2)) / 10.0
    cost = {"model": "ns_per_eval = c0 + p2 * (two-qubit positions) + p3 * (three-qubit positions); a position is its gate forward and "
                     "twice backward, its U3s (2 or 3) with their derivatives, and its 6 or 9 parameters' share of the optimizer's vector "
                     "and metric work; p2 = (k15 - k12) / 3, c0 = k15 - 15 p2, p3 = (three_qubit_k10 - c0) / 10",
            "ns_per_two_qubit_position": p2, "ns_per_three_qubit_position": p3, "ratio": p3 / p2,
            "ns_per_eval_ratio_at_n99": t3 / t15}
    doc = {"what": "one optimizer stage, targets x restarts items, no early exit, Haar 8x8 targets; ns_per_eval = median kernel time over the "
                   "repetitions / fused loss+gradient evaluations (throughput of the whole chip); spread = (max - min) / median over them",
           "device": mixed["device"], "compute_units": mixed["compute_units"], "targets": a.targets, "restarts": a.restarts, "reps": a.reps,
           "mixed": mixed, "position_cost": cost}
    if a.parent_lib:
        rounds = []
        for _ in range(2):
            rounds.append({"this": run_worker("q3", None), "parent": run_worker("q3", a.parent_lib)})
        ratios = {}
        for key in ("two_qubit_k3", "two_qubit_k6", "two_qubit_k12"):
            new = np.median([r["this"][key]["kernel_ms_median"] for r in rounds])
            old = np.median([r["parent"][key]["kernel_ms_median"] for r in rounds])
            same = all(r["this"][key]["evals"] == r["parent"][key]["evals"] == rounds[0]["this"][key]["evals"] for r in rounds)
            spread = max(r[w][key]["spread"] for r in rounds for w in ("this", "parent"))
            between = [r["this"][key]["kernel_ms_median"] for r in rounds]
            ratios[key] = {"new_over_parent": float(new / old), "same_evals": bool(same), "largest_spread_within_a_process": float(spread),
                           "this_build_process_to_process": float(abs(between[0] - between[1]) / np.mean(between))}
        doc["existing_kernel"] = {"what": "minimize_q3_kernel<false> (this build) against minimize_q3_kernel (parent build), alternating processes",
                                  "rounds": rounds, "ratios": ratios}
        own = {}
        for who, lib in (("this", None), ("parent", a.parent_lib)):
            with tempfile.TemporaryDirectory() as tmp:
                path = os.path.join(tmp, "q3_probe.json")
                child([os.path.join(ROOT, "tools", "q3_probe.py"), "--targets", str(a.targets), "--restarts", str(a.restarts), "--out", path], lib)
                own[who] = json.load(open(path))["rows"]
            print("q3_probe.py", who, json.dumps([{"k": r["k"], "q3_ns": r["q3"]["ns_per_eval"], "two_qubit_ns": r["two_qubit"]["ns_per_eval"]}
                                                  for r in own[who]]), flush=True)
        doc["q3_probe_rows"] = own
    else:
        doc["existing_kernel"] = "not measured: no --parent-lib given"
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
    print("position cost", json.dumps(cost))
    print("wrote", a.out)


if __name__ == "__main__":
    main()
