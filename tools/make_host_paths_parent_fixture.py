"""Dev tool (GPU): the outputs that tests/test_gpu_host_paths.py pins, and -- run as a script at the PARENT commit -- the fixture
tests/golden/host_paths_parent.npz they are compared with.  The host refactor behind it ("Host loop end", HISTORY.md) moves text
between functions of the host units and touches no kernel, so every array here has to come out byte-equal.

    python tools/make_host_paths_parent_fixture.py [out.npz]     (SLAM_HIP_LIB honoured)

One case per host path whose text moved.  Unless a case says otherwise: 8 Haar targets, the sqrt(iSWAP) gate, 3 restarts, spans 1..2,
SLAM_FLAG_EARLY_EXIT | SLAM_FLAG_ORDERED (results independent of scheduling).
  staged          the per-span launches (SLAM_FLAG_STAGED)
  wave            the one-launch forms of the loop (default flags)
  overlap         the spans side by side on helper contexts (SLAM_FLAG_OVERLAP, 17 restarts: with at most 16 the one-launch loop
                  still takes the call)
  list            slam_decompose_list for five of the targets with k_layout = 3
  predicted0/1    slam_decompose_predicted, spans 1..3, carry 0 and 1 (+ the two counts it returns)
  multi           slam_decompose_multi over two contexts (sqrt(iSWAP) and CNOT); `multi1.*` is the second context
  stage           slam_minimize_stage, span 2, an active list and explicit start points
  eval            slam_eval_loss_grad, slam_eval_unitary and slam_eval_c1c2c3 at span 2
  v2_loop / v2_stage / v2_eval        the RiSwapGate template (one parameter per gate): span loop 1..2, span-1 stage, span-2 evaluation
  smush_stage / smush_eval            one parallel-drive gate of one time slice: span-1 stage and evaluation
Per case: every result array, and from Context.stats() after a reset_stats() the launch count and items[k] (`<case>.counts`: kernel_launches,
then items[0 .. ]).  Times are not kept.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

N_TARGETS, RESTARTS, EXIT_LOSS = 8, 3, 1e-10
SEQS = [[0], [0, 0]]
SEQS3 = [[0], [0, 0], [0, 0, 0]]


def run_cases(ctx) -> dict:
    """Every pinned array, keyed '<case>.<name>'."""
    from oracle import slam_oracle as o
    from slam_decomposition_amd import _ffi
    from slam_decomposition_amd import gates as G
    from slam_decomposition_amd.basisv2 import CircuitTemplateV2
    from slam_decomposition_amd.weyl import c1c2c3

    loop = _ffi.FLAG_EARLY_EXIT | _ffi.FLAG_ORDERED
    sqiswap, cx = o.riswap_matrix(0.5), o.cx_matrix()
    targets = o.haar_batch(N_TARGETS, seed0=7300)
    rng = np.random.default_rng(41)
    out = {}

    def prm(flags=loop, restarts=RESTARTS, seed=5):
        return _ffi.OptParams(restarts=restarts, seed=seed, flags=flags)

    def counts(case, c):
        st = c.stats()
        out[f"{case}.counts"] = np.array([st["kernel_launches"]] + list(st["items"]), dtype=np.int64)

    def triple(case, r):
        out[f"{case}.best_loss"], out[f"{case}.best_x"], out[f"{case}.best_cycles"] = (np.array(a) for a in r)

    def winners(case, r):
        for key in ("best_loss", "best_x", "best_restart"):
            out[f"{case}.{key}"] = r[key]

    ctx.set_cost(_ffi.COST_BASIC)
    ctx.set_targets(targets)
    ctx.set_gates(sqiswap[None])

    for case, p in (("staged", prm(loop | _ffi.FLAG_STAGED)), ("wave", prm()), ("overlap", prm(loop | _ffi.FLAG_OVERLAP, restarts=17))):
        ctx.reset_stats()
        triple(case, ctx.decompose_range(0, N_TARGETS, 1, 2, SEQS, p, EXIT_LOSS))
        counts(case, ctx)

    ctx.set_targets(targets)  # (forgets the resident results: the list call lays its rows out for span 3)
    ctx.reset_stats()
    listed = np.array([6, 1, 4, 3, 0], dtype=np.int32)
    ctx.decompose_list(listed, 1, 2, SEQS, prm(), EXIT_LOSS, k_layout=3)
    counts("list", ctx)
    triple("list", ctx.fetch_results_range(3, 0, N_TARGETS))
    out["list.best_x"] = out["list.best_x"][listed]  # (the parameter rows of targets no call has decomposed are not initialised)

    coords = [c1c2c3(sqiswap)] * 3
    for carry in (0, 1):
        ctx.set_targets(targets)
        ctx.reset_stats()
        out[f"predicted{carry}.n_local_unreachable"] = np.array(
            ctx.decompose_predicted(coords, 3, SEQS3, prm(), EXIT_LOSS, 0, N_TARGETS, carry=bool(carry)), dtype=np.int64)
        counts(f"predicted{carry}", ctx)
        triple(f"predicted{carry}", ctx.fetch_results_range(3, 0, N_TARGETS))

    with _ffi.Context(0) as other:
        ctx.set_targets(targets)
        other.set_targets(targets)
        other.set_gates(cx[None])
        ctx.reset_stats()
        other.reset_stats()
        _ffi.decompose_multi([ctx, other], 0, N_TARGETS, 1, 2, SEQS, prm(), EXIT_LOSS)
        for case, c in (("multi", ctx), ("multi1", other)):
            counts(case, c)
            triple(case, c.fetch_results_range(2, 0, N_TARGETS))

    active = np.array([5, 2, 7, 0], dtype=np.int32)
    x0 = rng.uniform(0.0, 2.0 * np.pi, size=(len(active), RESTARTS, 18))
    ctx.reset_stats()
    winners("stage", ctx.minimize_stage([0, 0], prm(), active=active, x0=x0))
    counts("stage", ctx)

    tof = np.arange(N_TARGETS, dtype=np.int32)[::-1].copy()
    x = rng.uniform(-np.pi, np.pi, size=(N_TARGETS, 18))
    out["eval.loss"], out["eval.grad"] = ctx.eval_loss_grad([0, 0], x, tof)
    w, out["eval.unitary_loss"] = ctx.eval_unitary([0, 0], x, tof)
    out["eval.unitary"] = np.ascontiguousarray(w).view(np.float64)
    out["eval.c1c2c3"] = ctx.eval_c1c2c3([0, 0], x)

    v2 = CircuitTemplateV2(base_gates=[G.RiSwapGate])
    v2.set_device_gates(ctx)
    ctx.reset_stats()
    triple("v2_loop", ctx.v2_decompose_range(0, N_TARGETS, 1, 2, SEQS, [v2.device_layout(k)[2:6] for k in (1, 2)], prm(), EXIT_LOSS))
    counts("v2_loop", ctx)
    ctx.reset_stats()
    winners("v2_stage", ctx.v2_minimize_stage([0], prm(), EXIT_LOSS, *v2.device_layout(1)[2:6], active=active,
                                              x0=rng.uniform(0.0, 2.0 * np.pi, size=(len(active), RESTARTS, 13))))
    counts("v2_stage", ctx)
    loss, grad, w = ctx.v2_eval([0, 0], rng.uniform(-np.pi, np.pi, size=(N_TARGETS, 20)), tof, want_unitary=True)
    out["v2_eval.loss"], out["v2_eval.grad"], out["v2_eval.unitary"] = loss, grad, np.ascontiguousarray(w).view(np.float64)

    smush = CircuitTemplateV2(base_gates=[lambda *v: G.ConversionGainSmushGate(0.0, 0.0, np.pi / 2, 0.0, v[:1], v[1:], t_el=0.25)],
                              param_vec_expand=[0, 1, 1])
    smush.build(1)
    assert smush.n_slices == 1
    for name in smush.parameter_names():
        if name.startswith("Q"):
            smush.add_bound(name, max=2 * np.pi, min=-2 * np.pi)
    smush.set_device_gates(ctx)
    n_dev = smush.device_layout(1)[0]
    ctx.reset_stats()
    winners("smush_stage", ctx.smush_minimize_stage(smush.gate_sequence(), prm(), EXIT_LOSS, *smush.device_layout(1)[2:6], active=active,
                                                    x0=rng.uniform(-1.0, 1.0, size=(len(active), RESTARTS, n_dev))))
    counts("smush_stage", ctx)
    loss, grad, w = ctx.smush_eval(smush.gate_sequence(), rng.uniform(-1.0, 1.0, size=(N_TARGETS, n_dev)), tof, want_unitary=True)
    out["smush_eval.loss"], out["smush_eval.grad"], out["smush_eval.unitary"] = loss, grad, np.ascontiguousarray(w).view(np.float64)
    return out


if __name__ == "__main__":
    from slam_decomposition_amd import _ffi

    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "host_paths_parent.npz")
    with _ffi.Context(0) as ctx:
        arrays = run_cases(ctx)
        again = run_cases(ctx)
    # what the scheduling can change must not be pinned: print and leave out what differs between two runs of this one build
    for key in sorted(arrays):
        if arrays[key].tobytes() != again[key].tobytes():
            print("differs between two runs of one build, left out:", key)
            del arrays[key]
    np.savez_compressed(path, **arrays)
    print("wrote", path, os.path.getsize(path), "bytes,", len(arrays), "arrays")
