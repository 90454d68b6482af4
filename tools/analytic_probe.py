"""Dev tool (GPU): rate of the closed-form sqrt(iSWAP) decomposition (slam_sqiswap_decompose) on ONE resident batch of device Haar
targets, next to the KAK decomposition alone on the same batch (slam_targets_kak: one of the two or three decompositions each target
costs here) and to the optimizer's span loop (spans 1..3, 32 restarts, early exit, the bench's parameters) on the first 65 536 of them.
Every timing is a host clock around a call that ends in a device synchronise; the calls alternate over the rounds and the median and
the minimum are kept.  "whole" brings all four outputs to the host (201 MB of rows at 2^20 targets, pageable memory), "device" passes
NULL for every output: the kernel and its launch alone.  Writes profiles/analytic_probe.json and prints it.
usage: tools/analytic_probe.py [N] [ROUNDS]"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import slam_oracle as o  # noqa: E402
from slam_decomposition_amd import _ffi  # noqa: E402

args = [a for a in sys.argv[1:] if not a.startswith("--")]
N = int(args[0]) if args else 1 << 20
ROUNDS = int(args[1]) if len(args) > 1 else 7
N_OPT = min(N, 65536)

ctx = _ffi.Context(0)
ctx.sample_haar(7, N)
ctx.set_gates(o.riswap_matrix(0.5)[None])
prm = _ffi.OptParams(restarts=32, maxiter=2500, gtol=1e-9, stop_loss=1e-13, seed=1, flags=_ffi.FLAG_EARLY_EXIT | _ffi.FLAG_ORDERED)
seqs = [[0], [0, 0], [0, 0, 0]]


def whole():
    return ctx.sqiswap_decompose(0, N)


def device():
    _ffi._check(ctx._lib.slam_sqiswap_decompose(ctx._h, 0, N, None, None, None, None))


def kak():
    return ctx.targets_kak(0, N)


def optimizer():
    return ctx.decompose_range(0, N_OPT, 1, 3, seqs, prm, 1e-10)


calls = {"whole": (whole, N), "device": (device, N), "targets_kak": (kak, N), "optimizer_32_restarts": (optimizer, N_OPT)}
times = {name: [] for name in calls}
for r in range(ROUNDS + 1):  # round 0 warms every call up (code objects, buffers, result arrays)
    for name, (fn, _) in calls.items():
        t0 = time.perf_counter()
        res = fn()
        dt = time.perf_counter() - t0
        if r:
            times[name].append(dt)
        if name == "whole":
            x, cycles, loss, gap = res
        if name == "optimizer_32_restarts":
            opt_loss = res[0]
out = {"N": N, "rounds": ROUNDS, "device": ctx.device_info()[0], "calls": {}}
for name, (_, n) in calls.items():
    t = np.array(times[name])
    out["calls"][name] = {"targets": n, "ms_median": round(1e3 * float(np.median(t)), 3), "ms_min": round(1e3 * float(t.min()), 3),
                          "targets_per_s_median": float(n / np.median(t)), "targets_per_s_best": float(n / t.min())}
out["share_two_gates"] = float(np.mean(cycles == 2))
out["worst_loss"] = float(loss.max())
out["worst_gap"] = float(gap.max())
out["optimizer_solved_below_1e-10"] = float(np.mean(opt_loss < 1e-10))
ctx.close()
os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
with open(os.path.join(ROOT, "profiles", "analytic_probe.json"), "w") as f:
    json.dump(out, f, indent=1)
    f.write("\n")
print(json.dumps(out))
