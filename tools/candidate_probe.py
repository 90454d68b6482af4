"""Dev tool (GPU): throughput of candidate scoring (candidates.score_candidates -> slam_candidate_scores) on 2^20 device Haar targets,
k_cap = 64 -- the reference grid (177 gates) and a 65 x 65 ``candidate_grid`` -- as (gate, target) pairs per second from the wall
time of the whole call (targets generated in place, coordinates up, two kernels, counts back, the named targets, the scores) and from
the device time of the kernels alone.  Next to it, in the same process, the route that existed before on the reference grid:
``Context.coverage_lookup`` over host-built single-gate tables (rows k = 1 .. 64 from ``coverage.region``), table building and launch
timed separately; both routes must give the same counts.  Median of 5 runs after 2 warm-ups.  Writes one JSON file (default
profiles/candidate_probe.json) and prints it.
usage: tools/candidate_probe.py [--log2n 20] [--grid 65] [--no-tables] [--out PATH]"""
import argparse
import json
import os
import sys
import time
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from slam_decomposition_amd import candidates as cd, coverage, pulse_cost, runtime  # noqa: E402
from slam_decomposition_amd.sampler import DeviceHaarBatch  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--log2n", type=int, default=20)
ap.add_argument("--grid", type=int, default=65)
ap.add_argument("--k-cap", type=int, default=64)
ap.add_argument("--no-tables", action="store_true", help="skip the host-built tables (minutes of host time)")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "candidate_probe.json"))
args = ap.parse_args()
n, k_cap = 1 << args.log2n, args.k_cap
WARM, REPS = 2, 5
sampler = DeviceHaarBatch(seed=0xCA4D, n_samples=n)
ctx = runtime.get_context(0)


def med(ts):
    return {"median_ms": round(float(np.median(ts)) * 1e3, 3), "min_ms": round(min(ts) * 1e3, 3), "max_ms": round(max(ts) * 1e3, 3)}


def score_case(gates):
    wall, kern = [], []
    for r in range(WARM + REPS):
        a = time.perf_counter()
        sc = cd.score_candidates(gates, sampler, k_cap=k_cap)
        b = time.perf_counter()
        # the named targets' small call ran last: time the big one's kernels on the resident batch separately
        sampler.fill(ctx)
        ctx.candidate_scores(sc.coords, k_cap, first=0, count=n, tol=pulse_cost.TOL)
        if r >= WARM:
            wall.append(b - a)
            kern.append(ctx.last_candidate_kernel_ms * 1e-3)
    pairs = len(gates) * n
    finite = np.isfinite(sc.haar_score)
    best = int(np.argmin(np.where(finite, sc.haar_score, np.inf)))
    return sc, {"gates": len(gates), "pairs": pairs, "score_candidates_wall": med(wall), "kernels": med(kern),
                "pairs_per_s_wall": pairs / float(np.median(wall)), "pairs_per_s_kernels": pairs / float(np.median(kern)),
                "candidates_with_finite_haar_score": int(finite.sum()), "lowest_haar_score": float(sc.haar_score[best]),
                "lowest_haar_score_coords": sc.coords[best].tolist()}


out = {"n_targets": n, "k_cap": k_cap, "warmups": WARM, "reps": REPS}
ref_gates = cd.build_gates()[0]
sc_ref, out["reference_grid"] = score_case(ref_gates)
print("reference grid done", flush=True)
grid_gates, index = cd.candidate_grid(args.grid, args.grid)
_, out[f"grid_{args.grid}x{args.grid}"] = score_case(grid_gates)
print("fine grid done", flush=True)

if not args.no_tables:
    t0 = time.perf_counter()
    tables = []
    for j, g in enumerate(sc_ref.coords):
        bounds = np.zeros((k_cap, 14))
        for k in range(2, k_cap + 1):
            bounds[k - 1] = coverage.region(np.repeat(g[None], k, axis=0))
        points = np.zeros((k_cap, 4))
        points[0] = coverage.alcove_coordinates(g[None])[0]
        tables.append(types.SimpleNamespace(kinds=np.array([0] + [1] * (k_cap - 1), dtype=np.int32), points=points, bounds=bounds))
        if j % 20 == 0:
            print(f"tables {j + 1}/{len(sc_ref.coords)} after {time.perf_counter() - t0:.0f} s", flush=True)
    build_s = time.perf_counter() - t0
    sampler.fill(ctx)
    ts = []
    for r in range(WARM + REPS):
        a = time.perf_counter()
        counts, _ = ctx.coverage_lookup(tables, 0, n, tol=pulse_cost.TOL)
        if r >= WARM:
            ts.append(time.perf_counter() - a)
    new_ts = []
    for r in range(WARM + REPS):
        a = time.perf_counter()
        new_counts, _ = ctx.candidate_scores(sc_ref.coords, k_cap, first=0, count=n, tol=pulse_cost.TOL)
        if r >= WARM:
            new_ts.append(time.perf_counter() - a)
    differing = int(sum(int(np.abs(np.asarray(c) - new_counts[0, j]).sum()) for j, c in enumerate(counts)) // 2)
    out["coverage_lookup_over_host_tables"] = {
        "gates": len(tables), "rows": len(tables) * k_cap, "host_table_build_s": round(build_s, 2), "lookup_call": med(ts),
        "pairs_per_s_lookup_call": len(tables) * n / float(np.median(ts)),
        "candidate_scores_call_same_batch": med(new_ts),
        "lookup_call_over_candidate_scores_call": round(float(np.median(ts) / np.median(new_ts)), 3),
        "end_to_end_s": {"tables_then_lookup": round(build_s + float(np.median(ts)), 2), "candidate_scores": round(float(np.median(new_ts)), 4)},
        "targets_counted_differently": differing,
    }
text = json.dumps(out, indent=1)
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write(text + "\n")
print(text)
