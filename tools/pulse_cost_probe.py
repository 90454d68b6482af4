"""Dev tool (GPU): throughput of the coverage lookup (slam_coverage_lookup, pulse_cost.py) on 2^22 device Haar targets -- a one-gate
set at 26 gates (pi/32 conversion), a two-gate set at 16 gates, a three-gate set at 26 gates (3 653 entries) and the 17 gate sets of
tests/golden/reference_coverage_polytopes.json in one launch; an empty table gives the floor (Weyl coordinates and local test only).
Per case: wall time of the call (table upload, launch, counts back; median of 5 after one warm-up), targets/s, and the mean cost.
Prints one JSON line.  usage: tools/pulse_cost_probe.py [LOG2_N]"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from slam_decomposition_amd import pulse_cost, runtime  # noqa: E402
from slam_decomposition_amd.basis import CoverageTable, MixedOrderBasisCircuitTemplate  # noqa: E402
from slam_decomposition_amd.gates import ConversionGainGate  # noqa: E402
from slam_decomposition_amd.sampler import DeviceHaarBatch  # noqa: E402

PI = np.pi
n = 1 << (int(sys.argv[1]) if len(sys.argv) > 1 else 22)


def tpl(gates, span):
    return MixedOrderBasisCircuitTemplate([ConversionGainGate(0, 0, gc, gg, 1) for gc, gg in gates], maximum_span_guess=span)


t0 = time.perf_counter()
cases = {
    "one_gate_pi32_x26": [tpl([(PI / 32, 0.0)], 26)],
    "two_gate_x16": [tpl([(PI / 8, 0.0), (PI / 16, PI / 16)], 16)],
    "three_gate_x26": [tpl([(PI / 32, 0.0), (PI / 64, PI / 64), (PI / 96, PI / 48)], 26)],
}
ref = json.load(open(os.path.join(ROOT, "tests", "golden", "reference_coverage_polytopes.json")))
cases["sweep_17_reference_sets"] = [
    MixedOrderBasisCircuitTemplate([ConversionGainGate(0, 0, *v["gates"][0])], maximum_span_guess=max(len(e["operations"]) for e in v["coverage"]))
    for v in ref.values()
]
for ts in cases.values():
    for t in ts:
        t.coverage_table()
host_s = time.perf_counter() - t0

ctx = runtime.get_context(0)
DeviceHaarBatch(seed=0x5C0, n_samples=n).fill(ctx)
out = {"n_targets": n, "host_table_build_s": round(host_s, 2), "cases": {}}


def timed(tables):
    ctx.coverage_lookup(tables, 0, n, tol=pulse_cost.TOL)  # warm-up (buffers)
    ts = []
    for _ in range(5):
        a = time.perf_counter()
        counts, _ = ctx.coverage_lookup(tables, 0, n, tol=pulse_cost.TOL)
        ts.append(time.perf_counter() - a)
    return counts, float(np.median(ts))


_, s = timed([CoverageTable([])])
out["cases"]["empty_table"] = {"entries": 0, "ms": round(s * 1e3, 3), "targets_per_s": n / s}
for name, ts in cases.items():
    counts, s = timed([t.coverage_table() for t in ts])
    out["cases"][name] = {
        "tables": len(ts), "entries": int(sum(len(t.coverage) for t in ts)), "ms": round(s * 1e3, 3), "targets_per_s": n / s,
        "mean_cost": [pulse_cost.total_cost(t, c) / n for t, c in zip(ts, counts)] if len(ts) > 1 else pulse_cost.total_cost(ts[0], counts[0]) / n,
        "deepest_entry_hit": [int(np.nonzero(c[: len(t.coverage)])[0].max()) for t, c in zip(ts, counts)][:3],
    }
print(json.dumps(out))
