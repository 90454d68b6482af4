"""Dev tool (GPU): the family-extended cost of 2^22 device Haar targets (family_extend.family_cost_from_distribution ->
slam_family_lookup) for the iSWAP^(1/4), ^(1/8) and ^(1/16) families (48 gates), timed as a whole call -- targets generated in place,
tables uploaded, one launch, counts back, totals summed -- against the route that needs no family kernel: ``ctx.coverage_lookup`` of
all member tables with the entry of every target brought back, then the walk in NumPy (family_extend.walk) and the sum on the host.
The two routes alternate, one warm-up each, then 7 timed repetitions; both must give the same histogram.  Also: the lookup alone
on the resident batch.  Writes one JSON file (default profiles/family_probe.json) and prints it.
usage: tools/family_probe.py [--log2n 22] [--out PATH]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from slam_decomposition_amd import family_extend as fe, pulse_cost, runtime  # noqa: E402
from slam_decomposition_amd.gates import ConversionGainGate  # noqa: E402
from slam_decomposition_amd.sampler import DeviceHaarBatch  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--log2n", type=int, default=22)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "family_probe.json"))
ap.add_argument("--reps", type=int, default=7)
args = ap.parse_args()
n = 1 << args.log2n
sampler = DeviceHaarBatch(seed=0xFA111, n_samples=n)
ctx = runtime.get_context(0)


def coverage_route(fam, policy):
    """Without slam_family_lookup: every member's first containing row per target from slam_coverage_lookup, then the walk on the host."""
    sampler.fill(ctx)
    tables = fam.tables
    _, entries = ctx.coverage_lookup(tables, 0, n, want_entries=True, tol=pulse_cost.TOL)
    sizes = np.array([len(t) for t in tables])[:, None]
    local = entries[0] == sizes[0]
    ks = np.where(entries < sizes, entries + 1, 0)
    res = fe.walk(ks, fam.child_even, fam.child_odd, fam.durations, fam.cost_1q, policy)
    if np.any(~local & (res.gates < 0)):
        raise fam.unreachable_error()
    off = np.concatenate([[0], np.cumsum(sizes[:, 0])])
    rows = (off[np.maximum(res.member, 0)] + res.gates - 1)[~local]
    counts = np.bincount(rows, minlength=int(off[-1]))
    return fe._ordered_sum(counts, fam.row_costs()), counts


def timed(fn, reps):
    ts = []
    for _ in range(reps):
        a = time.perf_counter()
        out = fn()
        ts.append(time.perf_counter() - a)
    return out, ts


out = {"n_targets": n, "reps": args.reps, "policy": "reference", "families": {}}
for root in (4, 8, 16):
    t0 = time.perf_counter()
    fam = fe.GateFamily(ConversionGainGate(0, 0, np.pi / 2, 0, 1 / root), cost_1q=0.1, max_gates=48)
    rows = len(fam.rows())
    build_s = time.perf_counter() - t0
    # warm-up of both routes (buffers, code objects), then alternate
    res = fe.family_cost_from_distribution(fam, sampler)
    total2, counts2 = coverage_route(fam, "reference")
    same = [c for _, _, c in res.counts] == counts2.tolist() and total2 == res.total
    t_dev, t_cov = [], []
    for _ in range(args.reps):
        _, a = timed(lambda: fe.family_cost_from_distribution(fam, sampler), 1)
        _, b = timed(lambda: coverage_route(fam, "reference"), 1)
        t_dev += a
        t_cov += b
    sampler.fill(ctx)
    _, t_look = timed(lambda: fam.device_lookup(ctx, "reference", 0, n), args.reps)
    _, t_best = timed(lambda: fam.device_lookup(ctx, "best", 0, n), args.reps)
    _, t_fill = timed(lambda: (sampler.fill(ctx), ctx.synchronize() if hasattr(ctx, "synchronize") else None), args.reps)
    best = fe.family_cost_from_distribution(fam, sampler, policy="best")
    ms = lambda ts: {"median_ms": round(float(np.median(ts)) * 1e3, 3), "min_ms": round(min(ts) * 1e3, 3), "max_ms": round(max(ts) * 1e3, 3)}  # noqa: E731
    out["families"][f"iswap^(1/{root})"] = {
        "members": fam.multipliers.tolist(), "rows": rows, "host_table_build_s": round(build_s, 2),
        "family_cost_from_distribution": ms(t_dev), "coverage_lookup_then_numpy_walk": ms(t_cov),
        "speedup_median": round(float(np.median(t_cov) / np.median(t_dev)), 2), "same_histogram_and_total": bool(same),
        "lookup_alone_reference": ms(t_look), "lookup_alone_best": ms(t_best), "generate_targets_alone": ms(t_fill),
        "targets_per_s_lookup_alone": n / float(np.median(t_look)),
        "average_cost": res.average, "average_cost_base_alone": res.base_average, "average_cost_best": best.average,
        "winning_rows": [(r, k, c) for r, k, c in res.counts if c],
    }
text = json.dumps(out, indent=1)
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write(text + "\n")
print(text)
