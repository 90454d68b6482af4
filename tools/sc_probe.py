"""Dev tool (GPU): rate of the closed-form supercontrolled decomposition (slam_sc_decompose, slam_sc_counts; CAN(1/2, 0.3, 0)) on ONE
resident batch of device Haar targets, next to the approximate CNOT-class decomposition (slam_approx_decompose, slam_approx_counts;
CXGate) on the same batch in the same run, one process.  Every timing is a host clock around a call that ends in a device synchronise;
the calls alternate over the rounds and the median and the minimum are kept.  "device" passes NULL for every output (the kernel, the
upload of its table and its launch alone; the host's reduction of the basis gate is done once outside the clock), "whole" is the
``Context`` call with all five outputs on the host (pageable memory), the reduction inside the clock.  The decompositions run on the
first N targets, the sweeps of 16 fidelities on all 4 N.  Each launch runs under a time limit of its own: a watchdog thread ends the
process with status 124 when one call has not returned after LIMIT seconds.  Writes profiles/sc_probe.json and prints it.
usage: tools/sc_probe.py [N] [ROUNDS]"""
import json
import os
import sys
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from slam_decomposition_amd import _ffi  # noqa: E402
from slam_decomposition_amd.gates import CanonicalGate, CXGate  # noqa: E402

args = [a for a in sys.argv[1:] if not a.startswith("--")]
N = int(args[0]) if args else 1 << 20
ROUNDS = int(args[1]) if len(args) > 1 else 7
LIMIT = 60.0
BETA = 0.3


def limited(fn):
    """fn() under its own time limit."""
    watchdog = threading.Timer(LIMIT, lambda: (sys.stderr.write(f"sc_probe: a call ran past {LIMIT} s\n"), os._exit(124)))
    watchdog.daemon = True
    watchdog.start()
    try:
        return fn()
    finally:
        watchdog.cancel()


ctx = _ffi.Context(0)
limited(lambda: ctx.sample_haar(7, 4 * N))
SC, CX = CanonicalGate(np.pi / 4, 0.5 * np.pi * BETA, 0.0).to_matrix(), CXGate().to_matrix()
assert abs(_ffi.sc_class(SC) - BETA) < 1e-8
SC_DRESS = _ffi.sc_dress(SC)
CX_DRESS = _ffi.approx_dress(CX)
FID = np.linspace(0.9, 1.0, 16)
lib, h, P = ctx._lib, ctx._h, _ffi._ptr
NONE5 = (None,) * 5


def sc_device():
    g, dress = SC_DRESS
    _ffi._check(lib.slam_sc_decompose(h, 0, N, P(g), P(dress), 1.0, -1, *NONE5))


def cx_device():
    family, g, dress = CX_DRESS
    _ffi._check(lib.slam_approx_decompose(h, 0, N, family, P(g), P(dress), 1.0, -1, *NONE5))


def sc_sweep():
    g, dress = SC_DRESS
    _ffi._check(lib.slam_sc_counts(h, 0, 4 * N, P(g), P(dress), len(FID), P(FID), None, None))


def cx_sweep():
    _ffi._check(lib.slam_approx_counts(h, 0, 4 * N, CX_DRESS[0], len(FID), P(FID), None, None))


calls = {"sc_device": sc_device, "cx_device": cx_device, "sc_whole": lambda: ctx.sc_decompose(SC, 1.0, None, 0, N),
         "cx_whole": lambda: ctx.approx_decompose(CX, 1.0, None, 0, N), "sc_sweep": sc_sweep, "cx_sweep": cx_sweep}
times = {name: [] for name in calls}
kept = {}
for r in range(ROUNDS + 1):  # round 0 warms every call up (code objects, buffers, result arrays)
    for name, fn in calls.items():
        t0 = time.perf_counter()
        res = limited(fn)
        dt = time.perf_counter() - t0
        if r:
            times[name].append(dt)
        if name.endswith("_whole"):
            kept[name] = res
out = {"N": N, "rounds": ROUNDS, "beta": BETA, "device": ctx.device_info()[0], "calls": {}}
for name in calls:
    t = np.array(times[name])
    n = 4 * N if name.endswith("_sweep") else N
    out["calls"][name] = {"targets": n, "ms_median": round(1e3 * float(np.median(t)), 3), "ms_min": round(1e3 * float(t.min()), 3),
                          "targets_per_s_median": float(n / np.median(t)), "targets_per_s_best": float(n / t.min())}
for who in ("sc", "cx"):
    x, cycles, loss, predicted, gap = kept[f"{who}_whole"]
    out[who] = {"sizes": np.bincount(cycles, minlength=4).tolist(), "worst_loss": float(loss.max()), "worst_gap": float(gap.max())}
for kind in ("device", "whole", "sweep"):
    out["sc"][f"time_over_cx_{kind}"] = float(np.median(times[f"sc_{kind}"]) / np.median(times[f"cx_{kind}"]))
counts, fidsum = limited(lambda: ctx.sc_counts(SC, FID, 0, 4 * N))
out["sc"]["sweep_fidelities"] = FID.tolist()
out["sc"]["sweep_average_gates"] = (counts @ np.arange(4.0) / (4 * N)).tolist()
out["sc"]["sweep_average_fidelity"] = (fidsum / 4294967296.0 / (4 * N)).tolist()
ctx.close()
os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
with open(os.path.join(ROOT, "profiles", "sc_probe.json"), "w") as f:
    json.dump(out, f, indent=1)
    f.write("\n")
print(json.dumps(out))
