"""Dev tool (GPU): rate of the closed-form B-class decomposition (slam_b_decompose, BerkeleyGate) on ONE resident batch of device Haar
targets, next to the closed-form CNOT-class decomposition (slam_cx_decompose, CXGate) and the closed-form sqrt(iSWAP) decomposition
(slam_sqiswap_decompose) on the same batch in the same run.  Every timing is a host clock around a call that ends in a device
synchronise; the calls alternate over the rounds and the median and the minimum are kept.  "whole" brings all four outputs to the host
(201 MB of rows at 2^20 targets, pageable memory), "device" passes NULL for every output: the kernel, the upload of its table and its
launch alone (the host's reduction of the basis gate is done once outside the clock for "device" and inside it for "whole", as
Context.b_decompose and Context.cx_decompose do it).  Writes profiles/b_probe.json and prints it.
usage: tools/b_probe.py [N] [ROUNDS]"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from slam_decomposition_amd import _ffi  # noqa: E402
from slam_decomposition_amd.gates import BerkeleyGate, CXGate  # noqa: E402

args = [a for a in sys.argv[1:] if not a.startswith("--")]
N = int(args[0]) if args else 1 << 20
ROUNDS = int(args[1]) if len(args) > 1 else 7

ctx = _ffi.Context(0)
ctx.sample_haar(7, N)
B, CX = BerkeleyGate().to_matrix(), CXGate().to_matrix()
B_DRESS = _ffi.b_dress(B)
CX_DRESS = _ffi.cx_dress(CX)


def b_whole():
    return ctx.b_decompose(B, 0, N)


def b_device():
    g, dress = B_DRESS
    _ffi._check(ctx._lib.slam_b_decompose(ctx._h, 0, N, _ffi._ptr(g), _ffi._ptr(dress), None, None, None, None))


def cx_whole():
    return ctx.cx_decompose(CX, 0, N)


def cx_device():
    family, g, dress = CX_DRESS
    _ffi._check(ctx._lib.slam_cx_decompose(ctx._h, 0, N, family, _ffi._ptr(g), _ffi._ptr(dress), None, None, None, None))


def sq_whole():
    return ctx.sqiswap_decompose(0, N)


def sq_device():
    _ffi._check(ctx._lib.slam_sqiswap_decompose(ctx._h, 0, N, None, None, None, None))


calls = {"b_whole": b_whole, "b_device": b_device, "cx_whole": cx_whole, "cx_device": cx_device, "sqiswap_whole": sq_whole,
         "sqiswap_device": sq_device}
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
x, cycles, loss, gap = kept["b_whole"]
out["b"] = {"sizes": np.bincount(cycles, minlength=3)[1:].tolist(), "worst_loss": float(loss.max()), "worst_gap": float(gap.max())}
for other in ("cx", "sqiswap"):
    for kind in ("device", "whole"):
        out["b"][f"rate_over_{other}_{kind}"] = float(np.median(times[f"{other}_{kind}"]) / np.median(times[f"b_{kind}"]))
ctx.close()
os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
with open(os.path.join(ROOT, "profiles", "b_probe.json"), "w") as f:
    json.dump(out, f, indent=1)
    f.write("\n")
print(json.dumps(out))
