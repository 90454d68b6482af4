"""Dev tool (GPU): what the fidelity-aware approximate decomposition costs next to the exact siblings and next to the Weyl-coordinate
floor.  In one process, on one resident batch of 2^20 device Haar targets: ``slam_approx_decompose`` at f = 1 alternates with
``slam_cx_decompose`` (CX) and with ``slam_b_decompose`` (B), one warm-up each, then the median of 7 of each -- once as the kernel
and its synchronise alone (every output NULL) and once as the whole ``Context`` call with the rows read back.  Then, on 2^22 targets,
``slam_approx_counts`` with 16 fidelities alternates with ``ctx.coverage_lookup`` of an empty table (Weyl coordinates and the local
test only: the floor of DESIGN.md section 8).  Writes one JSON file (default profiles/approx_probe.json) and prints it.
usage: tools/approx_probe.py [--log2n 20] [--log2n-sweep 22] [--out PATH]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from slam_decomposition_amd import _ffi, pulse_cost, runtime  # noqa: E402
from slam_decomposition_amd.basis import CoverageTable  # noqa: E402
from slam_decomposition_amd.gates import BerkeleyGate, CXGate, gate_matrix  # noqa: E402
from slam_decomposition_amd.sampler import DeviceHaarBatch  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--log2n", type=int, default=20)
ap.add_argument("--log2n-sweep", type=int, default=22)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "approx_probe.json"))
ap.add_argument("--reps", type=int, default=7)
args = ap.parse_args()
ctx = runtime.get_context(0)
lib, h = ctx._lib, ctx._h


def alternate(a, b, reps):
    """Median seconds of ``a`` and of ``b``, alternating, after one warm-up each."""
    a(), b()
    ta, tb = [], []
    for _ in range(reps):
        for fn, ts in ((a, ta), (b, tb)):
            t0 = time.perf_counter()
            fn()
            ts.append(time.perf_counter() - t0)
    return ta, tb


def ms(ts):
    return {"median_ms": round(float(np.median(ts)) * 1e3, 3), "min_ms": round(min(ts) * 1e3, 3), "max_ms": round(max(ts) * 1e3, 3)}


n = 1 << args.log2n
DeviceHaarBatch(seed=0xA99, n_samples=n).fill(ctx)
out = {"n_targets": n, "reps": args.reps, "decompose": {}}
for name, gate in (("cx", CXGate()), ("b", BerkeleyGate())):
    G = gate_matrix(gate)
    family, g, dress = _ffi.approx_dress(G)
    pg, pd = _ffi._ptr(g), _ffi._ptr(dress)
    if family == _ffi.FAMILY_B:
        sibling_kernel = lambda: _ffi._check(lib.slam_b_decompose(h, 0, n, pg, pd, None, None, None, None))  # noqa: E731
        sibling_call = lambda: ctx.b_decompose(G)  # noqa: E731
    else:
        sibling_kernel = lambda: _ffi._check(lib.slam_cx_decompose(h, 0, n, family, pg, pd, None, None, None, None))  # noqa: E731
        sibling_call = lambda: ctx.cx_decompose(G)  # noqa: E731
    approx_kernel = lambda: _ffi._check(lib.slam_approx_decompose(h, 0, n, family, pg, pd, 1.0, -1, None, None, None, None, None))  # noqa: E731
    approx_call = lambda: ctx.approx_decompose(G, 1.0)  # noqa: E731
    ka, ks = alternate(approx_kernel, sibling_kernel, args.reps)
    ca, cs = alternate(approx_call, sibling_call, args.reps)
    a, s = approx_call(), sibling_call()
    out["decompose"][name] = {
        "approx_kernel_and_sync": ms(ka), "sibling_kernel_and_sync": ms(ks),
        "ratio_kernel_median": round(float(np.median(ka) / np.median(ks)), 4),
        "approx_whole_call": ms(ca), "sibling_whole_call": ms(cs), "ratio_whole_call_median": round(float(np.median(ca) / np.median(cs)), 4),
        "same_sizes": bool(np.array_equal(a[1], s[1])), "worst_loss_approx": float(a[2].max()), "worst_loss_sibling": float(s[2].max()),
        "targets_per_s_approx_kernel": n / float(np.median(ka)),
    }

m = 1 << args.log2n_sweep
DeviceHaarBatch(seed=0xA99, n_samples=m).fill(ctx)
fid = np.linspace(0.9, 1.0, 16)
empty = [CoverageTable([])]
G = gate_matrix(CXGate())
ts, tf = alternate(lambda: ctx.approx_counts(G, fid), lambda: ctx.coverage_lookup(empty, 0, m, tol=pulse_cost.TOL), args.reps)
counts, fidsum = ctx.approx_counts(G, fid)
out["sweep"] = {
    "n_targets": m, "n_fidelities": len(fid), "fidelity_sweep": ms(ts), "coverage_lookup_empty_table": ms(tf),
    "ratio_median": round(float(np.median(ts) / np.median(tf)), 4), "targets_per_s": m / float(np.median(ts)),
    "basis_fidelities": fid.round(6).tolist(), "counts": counts.tolist(), "average_gates": (counts @ np.arange(4) / m).tolist(),
    "average_fidelity": (fidsum / 2.0 ** 32 / m).tolist(),
}
text = json.dumps(out, indent=1)
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write(text + "\n")
print(text)
