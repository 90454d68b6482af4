"""Dev tool (GPU): rate of the fidelity-aware approximate sqrt(iSWAP) decomposition (slam_sqiswap_approx_decompose,
slam_sqiswap_approx_counts) on ONE resident batch of device Haar targets, next to its two parents on the same batch in the same run,
one process: the exact sqrt(iSWAP) decomposition (slam_sqiswap_decompose; the yardstick -- the same two or three KAK steps) and the
approximate CNOT-class decomposition (slam_approx_decompose, slam_approx_counts; CXGate).  Every timing is a host clock around a call
that ends in a device synchronise; the calls alternate over the rounds and the median and the minimum are kept.  "device" passes NULL
for every output (the kernel and its launch alone; for CX also the upload of its table, the host's reduction of the gate done once
outside the clock), "whole" is the ``Context`` call with all outputs on the host (pageable memory).  The decompositions run on the
first N targets, the sweeps of 16 fidelities on all 4 N.  Each launch runs under a time limit of its own: a watchdog thread ends the
process with status 124 when one call has not returned after LIMIT seconds.  Writes profiles/sqapprox_probe.json and prints it.
usage: tools/sqapprox_probe.py [N] [ROUNDS]"""
import json
import os
import sys
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from slam_decomposition_amd import _ffi  # noqa: E402
from slam_decomposition_amd.gates import CXGate  # noqa: E402

args = [a for a in sys.argv[1:] if not a.startswith("--")]
N = int(args[0]) if args else 1 << 20
ROUNDS = int(args[1]) if len(args) > 1 else 7
LIMIT = 60.0


def limited(fn):
    """fn() under its own time limit."""
    watchdog = threading.Timer(LIMIT, lambda: (sys.stderr.write(f"sqapprox_probe: a call ran past {LIMIT} s\n"), os._exit(124)))
    watchdog.daemon = True
    watchdog.start()
    try:
        return fn()
    finally:
        watchdog.cancel()


ctx = _ffi.Context(0)
limited(lambda: ctx.sample_haar(7, 4 * N))
CX = CXGate().to_matrix()
CX_DRESS = _ffi.approx_dress(CX)
FID = np.linspace(0.9, 1.0, 16)
lib, h, P = ctx._lib, ctx._h, _ffi._ptr
NONE4, NONE5 = (None,) * 4, (None,) * 5


def sq_device(f):
    return lambda: _ffi._check(lib.slam_sqiswap_approx_decompose(h, 0, N, f, -1, *NONE5))


def exact_device():
    _ffi._check(lib.slam_sqiswap_decompose(h, 0, N, *NONE4))


def cx_device():
    family, g, dress = CX_DRESS
    _ffi._check(lib.slam_approx_decompose(h, 0, N, family, P(g), P(dress), 1.0, -1, *NONE5))


def sq_sweep():
    _ffi._check(lib.slam_sqiswap_approx_counts(h, 0, 4 * N, len(FID), P(FID), None, None))


def cx_sweep():
    _ffi._check(lib.slam_approx_counts(h, 0, 4 * N, CX_DRESS[0], len(FID), P(FID), None, None))


calls = {"sq_device_f1": sq_device(1.0), "sq_device_f099": sq_device(0.99), "exact_device": exact_device, "cx_device": cx_device,
         "sq_whole_f1": lambda: ctx.sqiswap_approx_decompose(1.0, None, 0, N), "sq_whole_f099": lambda: ctx.sqiswap_approx_decompose(0.99, None, 0, N),
         "exact_whole": lambda: ctx.sqiswap_decompose(0, N), "cx_whole": lambda: ctx.approx_decompose(CX, 1.0, None, 0, N),
         "sq_sweep": sq_sweep, "cx_sweep": cx_sweep}
times = {name: [] for name in calls}
kept = {}
for r in range(ROUNDS + 1):  # round 0 warms every call up (code objects, buffers, result arrays)
    for name, fn in calls.items():
        t0 = time.perf_counter()
        res = limited(fn)
        dt = time.perf_counter() - t0
        if r:
            times[name].append(dt)
        if "_whole" in name:
            kept[name] = res
out = {"N": N, "rounds": ROUNDS, "device": ctx.device_info()[0], "calls": {}}
for name in calls:
    t = np.array(times[name])
    n = 4 * N if name.endswith("_sweep") else N
    out["calls"][name] = {"targets": n, "ms_median": round(1e3 * float(np.median(t)), 3), "ms_min": round(1e3 * float(t.min()), 3),
                          "targets_per_s_median": float(n / np.median(t)), "targets_per_s_best": float(n / t.min())}
for name, res in kept.items():
    cycles, loss, gap = res[1], res[2], res[-1]
    out[name] = {"sizes": np.bincount(cycles, minlength=4).tolist(), "worst_loss": float(loss.max()), "worst_gap": float(gap.max())}
    if len(res) == 5:
        out[name]["worst_loss_minus_predicted"] = float(np.abs(loss - res[3]).max())
med = {name: float(np.median(times[name])) for name in calls}
out["ratios"] = {"sq_f1_over_exact_device": med["sq_device_f1"] / med["exact_device"], "sq_f099_over_exact_device": med["sq_device_f099"] / med["exact_device"],
                 "sq_f1_over_cx_device": med["sq_device_f1"] / med["cx_device"], "sq_f099_over_sq_f1_device": med["sq_device_f099"] / med["sq_device_f1"],
                 "sq_f1_over_exact_whole": med["sq_whole_f1"] / med["exact_whole"], "sq_f1_over_cx_whole": med["sq_whole_f1"] / med["cx_whole"],
                 "sq_over_cx_sweep": med["sq_sweep"] / med["cx_sweep"]}
counts, fidsum = limited(lambda: ctx.sqiswap_approx_counts(FID, 0, 4 * N))
out["sweep"] = {"fidelities": FID.tolist(), "average_gates": (counts @ np.arange(4.0) / (4 * N)).tolist(),
                "average_fidelity": (fidsum / 4294967296.0 / (4 * N)).tolist()}
ctx.close()
os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
with open(os.path.join(ROOT, "profiles", "sqapprox_probe.json"), "w") as f:
    json.dump(out, f, indent=1)
    f.write("\n")
print(json.dumps(out))
