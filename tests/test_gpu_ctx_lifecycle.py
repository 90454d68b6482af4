"""GPU: a context gives back what it took.  Six cycles of create, use, close; "use" touches every lazily created resource of a context
once on tiny shapes -- the speculative streams and events, the helper contexts with their borrowed targets, the pinned argument staging,
the pinned bucket counts, the long kernels' metric buffer, the V2 and smush buffers, and the launch cache of every kernel family.

Two checks.  Every array returned in cycle 6 equals cycle 1's bit for bit: a fresh context and the sixth one of a process launch the same
work.  And device memory in use (hipMemGetInfo) after the close of cycle 6 exceeds that after the close of cycle 2 by less than half the
footprint of one cycle.  The footprint is what the contexts of a cycle themselves hold: in use just before cycle 1's close() minus in use
before cycle 1's create, taken after one throw-away cycle has paid what the process pays once (code objects, the runtime's own pools: several
hundred MB, more than the contexts), and never more than what cycle 1's close() gives back.  The contexts of a cycle that leaked whole in
cycles 3..6 would therefore keep at least four footprints, eight times the bound; the half is the margin for the allocator's granularity.  The guard is coarse (a leaked kilobyte does not
show): the owners in slam_host.hpp are the real protection."""
import ctypes

import numpy as np
import pytest

from slam_decomposition_amd import _ffi
from slam_decomposition_amd import gates as G
from slam_decomposition_amd.basisv2 import CircuitTemplateV2
from slam_decomposition_amd.weyl import c1c2c3

pytestmark = pytest.mark.gpu

N, R = 64, 4
SEQS = [[0], [0, 0], [0, 0, 0]]
LOOP = _ffi.FLAG_EARLY_EXIT | _ffi.FLAG_ORDERED  # the span loop's usual flags: what the one-launch forms of the loop require


def _in_use(hip):
    free, total = ctypes.c_size_t(), ctypes.c_size_t()
    assert hip.hipMemGetInfo(ctypes.byref(free), ctypes.byref(total)) == 0
    return total.value - free.value


def _prm(flags, restarts=R, seed=7):
    return _ffi.OptParams(restarts=restarts, maxiter=200, gtol=1e-9, stop_loss=1e-13, seed=seed, flags=flags)


def _use(ctx, other, v2, smush):
    """every call of one cycle; returns the arrays that must not depend on the cycle"""
    out = []
    cx = G.CXGate().to_matrix()
    for c, gate in ((ctx, cx), (other, G.RiSwapGate(0.5).to_matrix())):
        c.sample_haar(2025, N)
        c.set_gates(gate[None])
    # the span loop: speculative spans (side streams, fork / join events) ...
    ctx.reset_stats()
    out += ctx.decompose_range(0, N, 1, 3, SEQS, _prm(LOOP), 1e-10)
    assert ctx.stats()["kernel_launches"] == 4  # one launch per span + the merge
    # ... SLAM_FLAG_OVERLAP at the same shape (the one-launch loop still takes a call of at most 16 restarts) and at 17 restarts,
    # where the spans run side by side on helper contexts that borrow this context's targets ...
    out += ctx.decompose_range(0, N, 1, 3, SEQS, _prm(LOOP | _ffi.FLAG_OVERLAP), 1e-10)
    ctx.reset_stats()
    out += ctx.decompose_range(0, N, 1, 3, SEQS, _prm(LOOP | _ffi.FLAG_OVERLAP, restarts=17), 1e-10)
    assert ctx.stats()["kernel_launches"] == 7  # per span the inputs and the optimizer kernel, then the merge
    # ... and the per-span launches
    out += ctx.decompose_range(0, N, 1, 3, SEQS, _prm(LOOP | _ffi.FLAG_STAGED), 1e-10)
    # two contexts in one chain: argument blocks staged through pinned memory
    _ffi.decompose_multi([ctx, other], 0, N, 1, 3, SEQS, _prm(LOOP), 1e-10)
    for c in (ctx, other):
        out += c.fetch_results_range(3, 0, N)
    # the polytope mode: pinned bucket counts
    out.append(np.asarray(ctx.decompose_predicted([c1c2c3(cx)] * 3, 3, SEQS, _prm(LOOP), 1e-10, 0, N)))
    out += ctx.fetch_results_range(3, 0, N)
    # one stage of six gates: the wavefront-per-item kernel and its metric buffer
    st = ctx.minimize_stage([0] * 6, _prm(0), active=np.arange(8, dtype=np.int32))
    out += [st[key] for key in sorted(st)]
    rng = np.random.default_rng(3)
    tof = np.arange(8, dtype=np.int32)
    out += ctx.eval_loss_grad([0, 0], rng.uniform(-np.pi, np.pi, (8, 18)), tof)
    # parametrised gates: a RiSwapGate template of one gate, stage and evaluation
    ctx.v2_set_gates(v2._gate_maps)
    st = ctx.v2_minimize_stage([0], _prm(0), 1e-10, *v2.device_layout(1)[2:6])
    out += [st[key] for key in sorted(st)]
    out += ctx.v2_eval([0], rng.uniform(-np.pi, np.pi, (8, 13)), tof)[:2]
    # parallel-drive gates: one gate of four time slices
    smush.set_device_gates(ctx)
    st = ctx.smush_minimize_stage(smush.gate_sequence(), _prm(0), 1e-10, *smush.device_layout(1)[2:6], active=tof)
    out += [st[key] for key in sorted(st)]
    return [np.array(a) for a in out]


def test_six_context_lifecycles_launch_the_same_work_and_give_their_memory_back():
    v2 = CircuitTemplateV2(base_gates=[G.RiSwapGate])
    smush = CircuitTemplateV2(base_gates=[lambda *v: G.ConversionGainSmushGate(0.0, 0.0, np.pi / 2, 0.0, v[:4], v[4:], t_el=1.0)],
                              param_vec_expand=[0, 4, 4])
    smush.build(1)
    for name in smush.parameter_names():
        if name.startswith("Q"):
            smush.add_bound(name, max=2 * np.pi, min=-2 * np.pi)
    assert _ffi.device_count() >= 1
    hip = ctypes.CDLL("libamdhip64.so")
    results, after_close = [], []
    before_first = footprint = given_back = None
    for cycle in range(-1, 6):  # cycle -1: thrown away, it pays what the process pays once
        if cycle == 0:
            before_first = _in_use(hip)
        ctx, other = _ffi.Context(0), _ffi.Context(0)
        try:
            out = _use(ctx, other, v2, smush)
            before_close = _in_use(hip)
        finally:
            ctx.close()
            other.close()
        if cycle < 0:
            continue
        results.append(out)
        after_close.append(_in_use(hip))
        if cycle == 0:
            given_back = before_close - after_close[0]
            footprint = min(before_close - before_first, given_back)
    assert len(results[0]) == len(results[5]) and len(results[0]) > 30
    for i, (a, b) in enumerate(zip(results[0], results[5])):
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), f"array {i} of cycle 6 differs from cycle 1's"
    grown = after_close[5] - after_close[1]
    print(f"footprint of one cycle {footprint} bytes (cycle 1's close gave back {given_back}); in use after close, per cycle, minus before "
          f"the first: {[a - before_first for a in after_close]}; grown between cycles 2 and 6: {grown}")
    assert footprint > 0
    assert grown < footprint / 2
