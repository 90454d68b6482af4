"""Dev tool (GPU): throughput of the smush-gate optimizer (slam_smush_minimize_stage, csrc/slam_smush.hpp) on the two configurations
of the reference's parallel-drive studies (parallel_drive_volume.py): iSWAP-class smush (gc = pi/2, gg = 0, t = 1, N = 4) at k = 3 and
sqCNOT smush (gc = gg = pi/4, t = 1/2, N = 2) at k = 6; +-2 pi bounds on every drive, SquareCost, 4096 Haar targets x 16 restarts,
one span stage per call (ordered early exit at 1e-10).  Per case: ms per call (median of 3 after one warm-up), evaluations/s,
decompositions/s (targets per second), algorithmic flops per evaluation from the shapes and the share of the fp64 vector peak
(78.6 TFLOP/s nominal on an MI355X).  For comparison the reference's method -- SciPy L-BFGS-B with finite differences on the
NumPy oracle (tests/smush_ref.py), restarts in order until one is below 1e-10 -- on a few targets, one per process on 16 cores.
Writes OUT_JSON (default profiles/smush_probe.json).  Kernel times come from a separate run under
`rocprofv3 --kernel-trace --stats --output-format csv -- python tools/smush_probe.py N_TARGETS 0` (N_CPU_TARGETS = 0: nothing is
written); its kernel_trace.csv, given as KERNEL_TRACE_CSV, adds the median kernel time per case (the first call of a case is its warm-up).
usage: tools/smush_probe.py [N_TARGETS] [N_CPU_TARGETS] [OUT_JSON] [KERNEL_TRACE_CSV]"""
import json
import multiprocessing as mp
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from oracle import slam_oracle as o  # noqa: E402
from slam_decomposition_amd import _ffi  # noqa: E402
from slam_decomposition_amd.basisv2 import CircuitTemplateV2  # noqa: E402
from slam_decomposition_amd.gates import ConversionGainSmushGate  # noqa: E402

PI = np.pi
PEAK = 78.6e12
n_t = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
n_cpu = int(sys.argv[2]) if len(sys.argv) > 2 else 16
out_path = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "smush_probe.json")
trace_csv = sys.argv[4] if len(sys.argv) > 4 else None
RESOURCES = {"minimize_smush_kernel": "256 VGPRs, 0 AGPRs, no scratch, 1 wave/SIMD, 13.0 KiB dynamic LDS",
             "eval_smush_kernel": "215 VGPRs, 0 AGPRs, no scratch, 2 waves/SIMD, 13.0 KiB dynamic LDS"}  # (the build's resource-usage lines)
CPU_RESTARTS = 2  # (the CPU side stops after two restarts: its rate is an upper bound of the reference's, the ratio a lower bound)
CASES = {"iswap_smush_k3": (PI / 2, 0.0, 1.0, 4, 3), "sqcnot_smush_k6": (PI / 4, PI / 4, 0.5, 2, 6)}


def template(gc, gg, t, N, k):
    b = CircuitTemplateV2(base_gates=[lambda *v: ConversionGainSmushGate(0, 0, gc, gg, v[:N], v[N:], t_el=t)], param_vec_expand=[0, N, N])
    b.build(k)
    for name in b.parameter_names():
        if name.startswith("Q"):
            b.add_bound(name, max=2 * PI, min=-2 * PI)
    return b


def flops_per_eval(N, k):
    """fp64 flops of one loss + gradient: per slice and block 40 (build) forward and 40 + 3 x 56 (2x2 complex products) + 40
    (derivatives) backward, for both blocks of every gate; the U-gate layers as in the long kernels (a 4x4 complex column product
    per layer and scan level, the six derivatives); the adjoint of every gate (a 4x4 complex product) and its block projection."""
    per_slice = 2 * (40 + 56) + 2 * (40 + 3 * 56 + 40)
    layers = k + 1
    scan_levels = int(np.ceil(np.log2(layers))) if layers > 1 else 0
    mat = 4 * 4 * 4 * 8  # a 4x4 complex product
    return k * N * per_slice + layers * (2 * mat + 2 * scan_levels * mat + 400) + k * (2 * mat + 64)


def cpu_reference(args):
    """The reference's loop for one target: L-BFGS-B (SciPy finite differences) per restart until one is below 1e-10."""
    import scipy.optimize as opt
    import smush_ref as R

    (gc, gg, t, N, k), T, seed = args
    fn = lambda *v: ConversionGainSmushGate(0, 0, gc, gg, v[:N], v[N:], t_el=t)
    qn, n = 2 * N, 6 * (k + 1) + 2 * N * k
    bounds = [(-4 * PI, 4 * PI)] * (6 * (k + 1)) + [(-2 * PI, 2 * PI)] * (qn * k)
    rng = np.random.default_rng(seed)
    t0 = time.perf_counter()
    best, evals = np.inf, 0
    for _ in range(CPU_RESTARTS):
        x0 = np.array([rng.uniform(lo, hi) for lo, hi in bounds])
        res = opt.minimize(lambda x: R.loss_only(x, fn, qn, k, T, True), x0, method="L-BFGS-B", bounds=bounds, options={"maxiter": 2500})
        best, evals = min(best, float(res.fun)), evals + int(res.nfev)
        if best < 1e-10:
            break
    return time.perf_counter() - t0, best, evals


def main():
    out = {"n_targets": n_t, "restarts": 16, "cost": "SquareCost", "bounds": "+-2 pi on every drive", "cases": {}}
    targets = o.haar_batch(n_t, seed0=880000)
    for name, (gc, gg, t, N, k) in CASES.items():
        b = template(gc, gg, t, N, k)
        _, _, ilo, ihi, blo, bhi = b.device_layout(k)
        ctx = _ffi.Context(0)
        ctx.set_targets(targets)
        ctx.set_cost(_ffi.COST_SQUARE)
        b.set_device_gates(ctx)
        prm = _ffi.OptParams(restarts=16, maxiter=2500, gtol=1e-9, stop_loss=1e-11, seed=1, flags=_ffi.FLAG_EARLY_EXIT | _ffi.FLAG_ORDERED,
                             gtol_far=0.0)
        times, evals, solved = [], 0, 0.0
        for rep in range(4):
            ctx.reset_stats()
            t0 = time.perf_counter()
            res = ctx.smush_minimize_stage(b.gate_sequence(), prm, 1e-10, ilo, ihi, blo, bhi, want_items=False)
            dt = time.perf_counter() - t0
            if rep:
                times.append(dt)
                st = ctx.stats()
                evals = int(sum(st["evals"]))
                solved = float(np.mean(res["best_loss"] < 1e-10))
        ctx.close()
        ms = float(np.median(times)) * 1e3
        fpe = flops_per_eval(N, k)
        out["cases"][name] = {"gc": gc, "gg": gg, "t": t, "N": N, "k": k, "n_params": b.device_layout(k)[0], "ms_per_call": ms,
                              "evals_per_call": evals, "evals_per_s": evals / (ms * 1e-3), "decompositions_per_s": n_t / (ms * 1e-3),
                              "solved_fraction": solved, "flops_per_eval": fpe,
                              "fp64_peak_share": evals * fpe / (ms * 1e-3) / PEAK}
        if n_cpu <= 0:
            continue
        jobs = [((gc, gg, t, N, k), targets[i], 1000 + i) for i in range(n_cpu)]
        t0 = time.perf_counter()
        with mp.get_context("spawn").Pool(16) as pool:
            cpu = pool.map(cpu_reference, jobs)
        wall = time.perf_counter() - t0
        out["cases"][name]["cpu_reference"] = {"method": "SciPy L-BFGS-B, finite differences, NumPy/SciPy oracle, 16 processes",
                                               "restarts_cap": CPU_RESTARTS,
                                               "targets": n_cpu, "wall_s": wall, "decompositions_per_s": n_cpu / wall,
                                               "solved_fraction": float(np.mean([c[1] < 1e-10 for c in cpu])),
                                               "mean_target_s": float(np.mean([c[0] for c in cpu]))}
        out["cases"][name]["gpu_over_cpu"] = out["cases"][name]["decompositions_per_s"] / (n_cpu / wall)
        print(name, json.dumps(out["cases"][name]), flush=True)
    if n_cpu <= 0:
        return  # (the kernel-trace run: nothing written)
    if trace_csv:
        import csv

        with open(trace_csv) as fh:
            rows = [r for r in csv.DictReader(fh) if "minimize_smush_kernel" in r.get("Kernel_Name", "")]
        rows.sort(key=lambda r: int(r["Start_Timestamp"]))
        ms = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-6 for r in rows]
        per_case = len(ms) // len(CASES)
        for i, name in enumerate(CASES):
            timed = sorted(ms[i * per_case + 1 : (i + 1) * per_case])
            out["cases"][name]["kernel_ms_median"] = timed[len(timed) // 2] if timed else None
        out["kernel_times"] = "rocprofv3 --kernel-trace --stats, a separate run: minimize_smush_kernel, median of the timed calls per case"
    out["resources"] = RESOURCES
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as fh:
        json.dump(out, fh, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
