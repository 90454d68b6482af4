"""Dev tool (GPU): rate of the closed-form CNOT- / iSWAP-class decomposition (slam_cx_decompose) on ONE resident batch of device Haar
targets, for both families (CXGate, iSwapGate), next to the closed-form sqrt(iSWAP) decomposition (slam_sqiswap_decompose, the figure of
tools/analytic_probe.py) on the same batch in the same run.  Every timing is a host clock around a call that ends in a device
synchronise; the calls alternate over the rounds and the median and the minimum are kept.  "whole" brings all four outputs to the host
(201 MB of rows at 2^20 targets, pageable memory), "device" passes NULL for every output: the kernel, the upload of its 1.1 kB table and
its launch alone (the host's reduction of the basis gate, three weyl.kak calls, is done once outside the clock for "device" and inside
it for "whole", as Context.cx_decompose does it).  Writes profiles/cx_probe.json and prints it.
usage: tools/cx_probe.py [N] [ROUNDS]"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from slam_decomposition_amd import _ffi  # noqa: E402
from slam_decomposition_amd.gates import CXGate, iSwapGate  # noqa: E402

args = [a for a in sys.argv[1:] if not a.startswith("--")]
N = int(args[0]) if args else 1 << 20
ROUNDS = int(args[1]) if len(args) > 1 else 7

ctx = _ffi.Context(0)
ctx.sample_haar(7, N)
GATES = {"cx": CXGate().to_matrix(), "iswap": iSwapGate().to_matrix()}
DRESS = {name: _ffi.cx_dress(g) for name, g in GATES.items()}


def cx_whole(name):
    return lambda: ctx.cx_decompose(GATES[name], 0, N)


def cx_device(name):
    family, g, dress = DRESS[name]
    return lambda: _ffi._check(ctx._lib.slam_cx_decompose(ctx._h, 0, N, family, _ffi._ptr(g), _ffi._ptr(dress), None, None, None, None))


def sq_whole():
    return ctx.sqiswap_decompose(0, N)


def sq_device():
    _ffi._check(ctx._lib.slam_sqiswap_decompose(ctx._h, 0, N, None, None, None, None))


calls = {"cx_whole": cx_whole("cx"), "cx_device": cx_device("cx"), "iswap_whole": cx_whole("iswap"), "iswap_device": cx_device("iswap"),
         "sqiswap_whole": sq_whole, "sqiswap_device": sq_device}
times = {name: [] for name in calls}
kept = {}
for r in range(ROUNDS + 1):  # round 0 warms every call up (code objects, buffers, result arrays)
    for name, fn in calls.items():
        t0 = time.perf_counter()
        res = fn()
        dt = time.perf_counter() - t0
        if r:
            times[name].append(dt)
        if name.endswith("_whole"):
            kept[name] = res
out = {"N": N, "rounds": ROUNDS, "device": ctx.device_info()[0], "calls": {}}
for name in calls:
    t = np.array(times[name])
    out["calls"][name] = {"targets": N, "ms_median": round(1e3 * float(np.median(t)), 3), "ms_min": round(1e3 * float(t.min()), 3),
                          "targets_per_s_median": float(N / np.median(t)), "targets_per_s_best": float(N / t.min())}
for fam in ("cx", "iswap"):
    x, cycles, loss, gap = kept[fam + "_whole"]
    out[fam] = {"sizes": np.bincount(cycles, minlength=4)[1:].tolist(), "worst_loss": float(loss.max()), "worst_gap": float(gap.max())}
    for kind in ("device", "whole"):
        out[fam][f"rate_over_sqiswap_{kind}"] = float(np.median(times[f"sqiswap_{kind}"]) / np.median(times[f"{fam}_{kind}"]))
ctx.close()
os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
with open(os.path.join(ROOT, "profiles", "cx_probe.json"), "w") as f:
    json.dump(out, f, indent=1)
    f.write("\n")
print(json.dumps(out))
