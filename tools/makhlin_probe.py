"""Dev tool (GPU): MakhlinFunctionalCost (cost 2) against BasicCost (cost 0) on ONE resident batch of Haar targets, sqrt(iSWAP)
templates of k = 1, 3 and 8 gates: one optimizer stage per (cost, k) -- the same targets, restarts, Philox start points and iteration
cap, no early exit -- and the kernel time, evaluations and evaluations per second of each.  With --swap it also records what the
device BFGS does on SWAP with the 3-gate template under cost 2 (item losses and stop reasons of 64 restarts, and TemplateOptimizer's
result), the check of the far-point stop (gtol_far = 1e-5 / far_loss = 1e-6) near a chamber corner.  Prints one JSON line.
usage: tools/makhlin_probe.py [N] [R] [--swap]"""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from oracle import slam_oracle as o  # noqa: E402
from slam_decomposition_amd import _ffi  # noqa: E402

args = [a for a in sys.argv[1:] if not a.startswith("--")]
N = int(args[0]) if args else 16384
R = int(args[1]) if len(args) > 1 else 8
MAXITER = 300
# sqrt(iSWAP): what the API runs (cost 0 takes the structured GC_XRI1 kernels, cost 2 the dense ones); a Haar gate: both costs in the
# dense gate class, so the ratio isolates the loss / seed stage.  At k = 1 the cost-2 functional is constant (every 1Q layer is exterior):
# every restart stops after its first evaluation (zero gradient), and the k = 1 row measures launch overhead only.
out = {"N": N, "R": R, "maxiter": MAXITER, "stages": {}}
ctx = _ffi.Context(0)
ctx.sample_haar(0x5A11, N)
prm = _ffi.OptParams(restarts=R, maxiter=MAXITER, seed=11)
for gname, gm in (("sqrt_iswap", o.riswap_matrix(0.5)), ("dense", o.haar_unitary(9))):
    ctx.set_gates(gm[None])
    for k in (1, 3, 8):
        for cost in (_ffi.COST_BASIC, _ffi.COST_MAKHLIN):
            ctx.set_cost(cost)
            ctx.minimize_stage([0] * k, prm, want_items=False)  # warm-up (attributes, buffers)
            ctx.reset_stats()
            res = ctx.minimize_stage([0] * k, prm, want_items=False)
            st = ctx.stats()
            ms, ev = st["kernel_ms_span"][k], st["evals"][k]
            out["stages"][f"{gname}_k{k}_cost{cost}"] = {"kernel_ms": round(ms, 3), "evals": int(ev),
                                                        "evals_per_s": float(ev / (ms * 1e-3)) if ms > 0 else None,
                                                        "solved": float(np.mean(res["best_loss"] < 1e-10))}
        a, b = out["stages"][f"{gname}_k{k}_cost0"], out["stages"][f"{gname}_k{k}_cost2"]
        out["stages"][f"{gname}_k{k}_eval_rate_ratio_2_over_0"] = (b["evals_per_s"] / a["evals_per_s"]) if a["evals_per_s"] and b["evals_per_s"] else None
ctx.set_cost(_ffi.COST_BASIC)

if "--swap" in sys.argv:
    SWAP = np.array([[1, 0, 0, 0], [0, 0, 1, 0], [0, 1, 0, 0], [0, 0, 0, 1]], dtype=np.complex128)
    c2 = _ffi.Context(0)
    c2.set_targets(SWAP[None])
    c2.set_gates(o.riswap_matrix(0.5)[None])
    c2.set_cost(_ffi.COST_MAKHLIN)
    st = c2.minimize_stage([0] * 3, _ffi.OptParams(restarts=64, seed=3))
    loss = st["item_loss"][0]
    status = st["item_status"][0]
    out["swap_stage"] = {"restarts": 64, "below_1e-10": int(np.sum(loss < 1e-10)), "loss_min": float(loss.min()), "loss_median": float(np.median(loss)),
                         "loss_max": float(loss.max()), "status_counts": {int(s): int(np.sum(status == s)) for s in np.unique(status)},
                         "iters_median": float(np.median(st["item_iters"][0]))}
    c2.close()
    from slam_decomposition_amd import gates as G
    from slam_decomposition_amd.basis import CircuitTemplate
    from slam_decomposition_amd.cost_function import MakhlinFunctionalCost
    from slam_decomposition_amd.optimizer import TemplateOptimizer

    d = TemplateOptimizer(CircuitTemplate(base_gates=[G.RiSwapGate(0.5)], maximum_span_guess=3), MakhlinFunctionalCost(), seed=3,
                          override_fail=True).approximate_target_U(SWAP)
    out["swap_template_optimizer"] = {"success": int(d.success_label), "loss": float(d.loss_result), "cycles": int(d.cycles)}
ctx.close()
print(json.dumps(out))
