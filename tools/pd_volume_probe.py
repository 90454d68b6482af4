"""Dev tool (GPU): the parallel-drive coverage pipeline (parallel_drive.py) on one MI355X.  Per stage, wall time around calls that end
in a device synchronise (median of 5 after one warm-up): the sampling kernel (slam_pd_sample, 2^20 samples, iSWAP k = 2 and sqCNOT
k = 5), extremes + prefilter (slam_pd_extremes + slam_pd_filter) and the survivors it leaves, the host hull (qhull), and the region
lookup (slam_region_lookup, 2^22 targets, the reference's sqCNOT regions).  Then the whole six-gate table at the defaults
(extended_coverage: 2^20 samples per k; volumes on 2^22 device Haar targets) next to the reference's recorded rows and scores.
usage: tools/pd_volume_probe.py [OUT.json]   (default profiles/pd_volume_probe.json)"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from slam_decomposition_amd import parallel_drive as pd, runtime  # noqa: E402

OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "pd_volume_probe.json")
REF = json.load(open(os.path.join(ROOT, "tests", "golden", "reference_smush_coverage.json")))
ctx = runtime.get_context(0)
out = {"device": ctx.device_info()[0], "stages": {}, "table": {}}


def timed(fn, reps=5):
    fn()
    ts = []
    for _ in range(reps):
        a = time.perf_counter()
        r = fn()
        ts.append(time.perf_counter() - a)
    return r, float(np.median(ts))


n = 1 << 20
for name, k in (("iSwap", 2), ("sqCNOT", 5)):
    v = REF[name]
    N = int(round(v["t"] / 0.25))
    _, s = timed(lambda: ctx.pd_sample(v["gc"], v["gg"], v["t"], N, k, n, seed=1))
    ctx.pd_sample(v["gc"], v["gg"], v["t"], N, k, n, seed=1)
    (ext_idx, ext), s_ext = timed(lambda: ctx.pd_extremes(pd._directions()))
    pre = pd.hull_facets(np.unique(ext, axis=0))
    (idx, pts), s_f = timed(lambda: ctx.pd_filter(pre, capacity=n))
    _, s_h = timed(lambda: pd.hull_facets(pts), reps=3)
    out["stages"][f"{name}_k{k}"] = {
        "n_samples": n, "slices": k * N, "sample_ms": round(s * 1e3, 3), "samples_per_s": n / s,
        "extremes_ms": round(s_ext * 1e3, 3), "prefilter_facets": int(len(pre)), "filter_ms": round(s_f * 1e3, 3),
        "survivors": int(len(idx)), "host_hull_ms": round(s_h * 1e3, 3)}

v = REF["sqCNOT"]
ec = pd.ExtendedCoverage.from_rows((v["gc"], v["gg"], v["t"]), v["k_full"], v["regions"])
nt = 1 << 22
ctx.sample_haar(21, nt)
ks, ro, kinds, fo, facets, aux = ec._table()
_, s = timed(lambda: ctx.region_lookup(ro, kinds, fo, facets, aux, 0, nt, tol=pd.TOL))
out["stages"]["region_lookup_sqCNOT_reference"] = {"n_targets": nt, "regions": len(ro) - 1, "facets": int(len(facets)),
                                                   "ms": round(s * 1e3, 3), "targets_per_s": nt / s}

for name, v in REF.items():
    a = time.perf_counter()
    ec = pd.extended_coverage(v["gc"], v["gg"], v["t"])
    s_cov = time.perf_counter() - a
    a = time.perf_counter()
    res = ec.results()
    s_vol = time.perf_counter() - a
    out["table"][name] = {
        "rows": res, "scores": ec.scores, "recorded_rows": v["rows"], "recorded_scores": v["scores"],
        "hull_vertices": {k: int(len(r.vertices)) for k, r in ec.regions.items()}, "stats": {k: ec.stats[k] for k in ec.stats},
        "first_counts": ec.first_counts, "extended_coverage_s": round(s_cov, 3), "volumes_s": round(s_vol, 3)}

os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
with open(OUT, "w") as f:
    json.dump(out, f, indent=1, default=float)
print(json.dumps(out["stages"]))
print(json.dumps({k: [v["scores"], v["recorded_scores"]] for k, v in out["table"].items()}))
