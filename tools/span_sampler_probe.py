"""Dev tool (GPU): 65 536 Haar targets that all need three sqrt(iSWAP) gates, resident on the device, two ways --
  selected   sampler.DeviceHaarSpanBatch: slam_haar_select_spans in chunks (drawn, classified and ranked in registers; only the
             selected stream indices come back), then slam_sample_haar_indexed regenerates the batch in place;
  host_route what had to be done before: slam_sample_haar about five times as many targets, slam_predict_spans, the spans back,
             a host filter, slam_get_targets of the lot and slam_set_targets of the survivors.
Both are whole calls from nothing to a drained stream (slam_synchronize), median of 7 after one warm-up; the two batches are checked
to be the same targets.  Prints one JSON line and writes it to profiles/span_sampler_probe.json (or to the path given).
usage: tools/span_sampler_probe.py [OUT.json] [N_TARGETS]"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from slam_decomposition_amd import runtime  # noqa: E402
from slam_decomposition_amd.sampler import DeviceHaarSpanBatch  # noqa: E402

out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "span_sampler_probe.json")
n = int(sys.argv[2]) if len(sys.argv) > 2 else 65536
SEED, SPAN, REPS = 20261018, 3, 7
seq = [(0.25, 0.25, 0.0)] * 3
ctx = runtime.get_context(0)


def selected():
    b = DeviceHaarSpanBatch(seq, SPAN, seed=SEED, n_samples=n)
    b.fill(ctx)
    ctx.synchronize()
    return b


def host_route():
    m = int(n / 0.2043 * 1.03)  # the three-gate share of Haar targets, and 3 % to spare (36 standard deviations at 65 536)
    ctx.sample_haar(SEED, m)
    keep = np.nonzero(ctx.predict_spans(seq, 3) == SPAN)[0][:n]
    if len(keep) < n:
        raise RuntimeError(f"{len(keep)} of {m} candidates need three gates: fewer than {n}")
    ctx.set_targets(ctx.get_targets(0, m)[keep])
    ctx.synchronize()
    return keep


def timed(fn):
    fn()
    ts = []
    for _ in range(REPS):
        a = time.perf_counter()
        r = fn()
        ts.append(time.perf_counter() - a)
    return r, float(np.median(ts)), ts


keep, t_host, ts_host = timed(host_route)
T_host = ctx.get_targets(0, n)
b, t_sel, ts_sel = timed(selected)
T_sel = ctx.get_targets(0, n)
out = {
    "n_targets": n, "span": SPAN, "gate": "sqrt(iSWAP)", "reps": REPS,
    "selected_ms": round(t_sel * 1e3, 3), "host_route_ms": round(t_host * 1e3, 3), "host_route_over_selected": round(t_host / t_sel, 2),
    "selected_all_ms": [round(t * 1e3, 3) for t in ts_sel], "host_route_all_ms": [round(t * 1e3, 3) for t in ts_host],
    "candidates_scanned": int(b.candidates_scanned), "acceptance": b.acceptance, "span_counts": b.span_counts.tolist(),
    "same_indices": bool(np.array_equal(b.indices, keep)), "same_targets": bool(np.array_equal(T_sel, T_host)),
}
line = json.dumps(out)
print(line)
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    f.write(line + "\n")
