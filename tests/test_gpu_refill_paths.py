"""GPU: the refill path of the optimizer's persistent wavefronts -- the scan that drops or hands out queue positions by their
target's early-exit flag (whatever the flag's age, a result may not depend on it: an item handed out late is pre-empted), the reset
of a quad that takes an item, start points, queue switches of the multi-queue launch, the wave-local queue.  Every test compares
the library against itself through a path that shares none of these decisions: the same stage without early exit reduced on the
host, explicit start points from the oracle's Philox, one call per context, the staged launches."""
import numpy as np
import pytest

from oracle import slam_oracle as o
from slam_decomposition_amd import _ffi

pytestmark = pytest.mark.gpu

SQ = o.riswap_matrix(0.5)
CX = o.cx_matrix()
SEQS = [[0], [0, 0], [0, 0, 0]]
ORDERED = _ffi.FLAG_EARLY_EXIT | _ffi.FLAG_ORDERED


def _philox_x0(seed, n_targets, restarts, k, pick=None):
    """Explicit start points [n_targets, R, n] = the in-kernel Philox ones (pick: one restart index per target, R = 1)."""
    if pick is not None:
        return np.stack([o.x0_philox(seed, t, int(pick[t]), k)[None] for t in range(n_targets)])
    return np.stack([np.stack([o.x0_philox(seed, t, r, k) for r in range(restarts)]) for t in range(n_targets)])


def _cx_targets(n):
    """Even indices: two CNOTs between random local layers (solved at span 2); odd indices: Haar (solved at span 3 only)."""
    rng = np.random.default_rng(31)
    T = o.haar_batch(n, seed0=9100)
    for t in range(0, n, 2):
        T[t] = o.template_eval(rng.uniform(0, 2 * np.pi, 18), [CX, CX])
    return T


@pytest.mark.parametrize("N,R", [(40, 40), (1, 33), (17, 1)])
def test_ordered_early_exit_is_the_host_reduction_of_the_run_without(hip_ctx, N, R):
    """CNOT, spans 1..3, ordered early exit: about half of the span-2 stage's targets and all of the span-3 stage's succeed early,
    so items are dropped at the pull and pre-empted in flight; 40 x 40 gives a wavefront several scan windows and chunk
    switches and an item count that is no multiple of 16 or 64.  The stage result must be, bit for bit, the lowest-index
    restart below the exit level (else the lowest loss) of the run WITHOUT early exit -- loss, restart, and the parameters of
    that restart run alone from its explicit start point -- and the span loop's losses / parameters / cycles the host's
    reduction of those stages."""
    seed, stop, thr = 21, 1e-13, 1e-10
    hip_ctx.set_targets(_cx_targets(N))
    hip_ctx.set_gates(CX[None])
    loop = hip_ctx.decompose(1, 3, SEQS, _ffi.OptParams(restarts=R, seed=seed, flags=ORDERED | _ffi.FLAG_STAGED, stop_loss=stop), thr)
    want_loss = np.full(N, np.inf)
    want_x = np.zeros((N, 24))
    want_cyc = np.full(N, -1, dtype=np.int32)
    n_pre = 0
    for k in (1, 2, 3):
        full = hip_ctx.minimize_stage([0] * k, _ffi.OptParams(restarts=R, seed=seed, flags=0, stop_loss=stop))
        got = hip_ctx.minimize_stage([0] * k, _ffi.OptParams(restarts=R, seed=seed, flags=ORDERED, stop_loss=stop))
        n_pre += int((got["item_status"] == _ffi.ST_PREEMPTED).sum())

        def winner(level):
            r = np.empty(N, dtype=np.int32)
            for t in range(N):
                below = np.nonzero(full["item_loss"][t] < level)[0]
                r[t] = below[0] if len(below) else int(np.argmin(full["item_loss"][t]))
            return r

        want_r = winner(stop)
        alone = hip_ctx.minimize_stage([0] * k, _ffi.OptParams(restarts=1, seed=999, flags=0, stop_loss=stop), x0=_philox_x0(seed, N, R, k, want_r))
        assert np.array_equal(got["best_restart"], want_r), k
        assert np.array_equal(got["best_loss"], full["item_loss"][np.arange(N), want_r]), k
        assert np.array_equal(got["best_loss"], alone["best_loss"]) and np.array_equal(got["best_x"], alone["best_x"]), k
        # the span loop exits at its own threshold: its stage winner is the lowest-index restart below THAT level
        loop_r = winner(thr)
        alone = hip_ctx.minimize_stage([0] * k, _ffi.OptParams(restarts=1, seed=999, flags=0, stop_loss=stop), x0=_philox_x0(seed, N, R, k, loop_r))
        for t in range(N):
            if want_loss[t] < thr:
                continue  # solved at a shorter span: the loop does not come here
            if alone["best_loss"][t] < want_loss[t]:
                want_loss[t] = alone["best_loss"][t]
                want_x[t] = 0.0
                want_x[t, : 6 * (k + 1)] = alone["best_x"][t]
                want_cyc[t] = k
    assert np.array_equal(loop[0], want_loss) and np.array_equal(loop[1], want_x) and np.array_equal(loop[2], want_cyc)
    if R > 1:
        assert n_pre > 0, "the case needs restarts that an earlier success cuts off"
    if N >= 2 and R > 1:
        assert set(want_cyc.tolist()) == {2, 3}


@pytest.mark.parametrize("k", [1, 2])
def test_start_points_of_the_refill_equal_explicit_ones_item_by_item(hip_ctx, k):
    """sqrt(iSWAP), 24 x 20: every item of the in-kernel Philox path (span 1: the parked ring, span 2: the blocks dealt over the
    wave at the refill) ends where the same item ends from the oracle's start point passed explicitly (neither ring nor blocks)."""
    N, R, seed = 24, 20, 17
    hip_ctx.set_targets(o.haar_batch(N, seed0=7300))
    hip_ctx.set_gates(SQ[None])
    plain = hip_ctx.minimize_stage([0] * k, _ffi.OptParams(restarts=R, seed=seed, flags=0))
    explicit = hip_ctx.minimize_stage([0] * k, _ffi.OptParams(restarts=R, seed=999, flags=0), x0=_philox_x0(seed, N, R, k))
    for key in ("item_loss", "item_iters", "best_loss", "best_x", "best_restart"):
        assert np.array_equal(plain[key], explicit[key]), key


def test_queue_switches_of_the_multi_queue_launch_equal_one_call_per_context():
    """slam_decompose_multi, three contexts (three sub-problems behind one launch per span), windows of 5 / 16 / 23 targets x 20
    restarts: a wavefront's parked start points and its reset quads belong to the queue it leaves -- every context must hold
    exactly what its own call leaves."""
    R = 20
    prm = _ffi.OptParams(restarts=R, maxiter=2500, gtol=1e-9, stop_loss=1e-13, seed=31, flags=ORDERED)
    ctxs = [_ffi.Context(0) for _ in range(3)]
    try:
        for c, alpha in zip(ctxs, (0.5, 0.4, 0.6)):
            c.sample_haar(808, 48)
            c.set_gates(o.riswap_matrix(alpha)[None])
        for first, count in ((0, 5), (5, 16), (21, 23)):
            solo = [c.decompose_range(first, count, 1, 3, SEQS, prm, 1e-10) for c in ctxs]
            _ffi.decompose_multi(ctxs, first, count, 1, 3, SEQS, prm, 1e-10)
            for c, want in zip(ctxs, solo):
                got = c.fetch_results_range(3, first, count)
                for a, b in zip(got, want):
                    assert np.array_equal(a, b), (first, count)
    finally:
        for c in ctxs:
            c.close()


@pytest.mark.parametrize("N", [900, 3])
def test_wave_local_queue_equals_the_staged_launches(N):
    """40 restarts per target, more than a wavefront has quads.  900 targets: the whole span loop of a target runs in one wavefront
    (span_wave_kernel: LDS flag, wave-local refill; taken for more than 16 restarts only when targets x restarts fill the chip, and
    above two targets per compute unit the speculative form is not chosen) -- ONE launch, against the three per-span launches of
    SLAM_FLAG_STAGED, bit for bit.  3 targets: too few items for that kernel, the library serves the call with the per-span
    launches itself; the results must not depend on which path it picks."""
    with _ffi.Context(0) as ctx:
        ctx.sample_haar(2024, N)
        ctx.set_gates(SQ[None])
        res, launches = [], []
        for extra in (_ffi.FLAG_NO_OVERLAP, _ffi.FLAG_STAGED):
            prm = _ffi.OptParams(restarts=40, maxiter=2500, gtol=1e-9, stop_loss=1e-13, seed=12, flags=ORDERED | extra)
            ctx.reset_stats()
            res.append(ctx.decompose_range(0, N, 1, 3, SEQS, prm, 1e-10) + (ctx.fetch_span_losses(0, N),))
            launches.append(ctx.stats()["kernel_launches"])
        for a, b in zip(*res):
            assert np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(np.nan_to_num(a), np.nan_to_num(b))
        assert np.all(res[0][0] < 1e-8)
        if N == 900:
            assert launches == [1, 3], "the first call was not served by span_wave_kernel"


@pytest.mark.parametrize("case", ["no_exterior", "makhlin"])
def test_reset_code_of_the_other_instantiations(hip_ctx, case):
    """8 x 8 at span 2 with SLAM_FLAG_NO_EXTERIOR, and under MakhlinFunctionalCost (its own kernel): Philox start points against the
    same ones passed explicitly, item by item."""
    N, R, k, seed = 8, 8, 2, 5
    hip_ctx.set_targets(o.haar_batch(N, seed0=7400))
    hip_ctx.set_gates(SQ[None])
    flags = _ffi.FLAG_NO_EXTERIOR if case == "no_exterior" else 0
    hip_ctx.set_cost(_ffi.COST_MAKHLIN if case == "makhlin" else _ffi.COST_BASIC)
    try:
        plain = hip_ctx.minimize_stage([0] * k, _ffi.OptParams(restarts=R, seed=seed, flags=flags))
        explicit = hip_ctx.minimize_stage([0] * k, _ffi.OptParams(restarts=R, seed=999, flags=flags), x0=_philox_x0(seed, N, R, k))
    finally:
        hip_ctx.set_cost(_ffi.COST_BASIC)
    for key in ("item_loss", "item_iters", "best_loss", "best_x", "best_restart"):
        assert np.array_equal(plain[key], explicit[key]), key
    assert np.all(np.isfinite(plain["item_loss"]))
