"""GPU: the span loop's bookkeeping -- winner over the restarts, merge into the running best, row copy and zero fill, span_loss,
compaction of the unsolved targets, predicted sizes, list mode, evaluation counters -- against the host model of
tests/span_loop_model.py, bit for bit, at the sizes where ``enqueue_stage_epilogue`` changes kernels (2048, 8192 targets) and on
every path a span loop can take (per-span launches, side-by-side spans, the one-wavefront loop, list, predicted, multi, V2).

The optimizer is kept cheap so that the sizes can be real: sqrt(iSWAP), device Haar targets, ``maxiter=3``, default ``gtol`` and
``stop_loss`` -- three iterations from a random start end anywhere between 1e-3 and 1, evaluation counts differ item by item.
The item tables come from paths that share none of the loop's bookkeeping: ``item_loss`` / ``item_evals`` of
``minimize_stage(flags=0)`` per span over all resident targets (an item -- target, restart, span -- is keyed by its resident index
and does not depend on the batch or the number of restarts around it), the winners' parameters from a ONE-restart
``minimize_stage`` started at the winning restart's Philox start point, computed here on top of the oracle's ``philox4x32``.

The threshold of a case is an order statistic of the stage losses of the FIRST span the case runs (span 1, except for the
``k_min = 2`` windows and the predicted call, which start at span 2), taken from the model's tables, never from the loop: one
designated target ends that span with ``best == threshold`` exactly and the model keeps it (strict ``<``).  Every case asserts ON
THE MODEL that its first two spans both keep and drop at least 10 % of their targets, that at least one target is unsolved after
``k_max`` and that at least one stage winner is not the lowest-loss restart (cases of one target can only assert the designated
target; cases of one restart have no second restart to win).  No tolerance appears in this module.

All cases but the multi-context one run on ONE context that a first call (``primed``) has taken through the grid epilogue with
a threshold nothing reaches: every row of ``best_x`` then holds 24 stale non-zero values and both active lists hold stale
indices, so that a missing zero fill or a hole in a compacted list shows as a wrong result instead of reading fresh memory."""
import numpy as np
import pytest

import span_loop_model as model
from oracle import slam_oracle as o
from slam_decomposition_amd import _ffi

pytestmark = pytest.mark.gpu

SQ = o.riswap_matrix(0.5)
SEQS = [[0], [0, 0], [0, 0, 0]]
ORDERED = _ffi.FLAG_EARLY_EXIT | _ffi.FLAG_ORDERED
STAGED, OVERLAP, NO_OVERLAP = _ffi.FLAG_STAGED, _ffi.FLAG_OVERLAP, _ffi.FLAG_NO_OVERLAP
HAAR_SEED, SEED = 4242, 19
NMAX, RMAX = 8192 + 256 + 37, 17
MAXITER = 3
NEVER = 1e-300  # a threshold no loss is below


def _prm(R, flags, seed=SEED):
    return _ffi.OptParams(restarts=R, maxiter=MAXITER, seed=seed, flags=flags)


def philox_x0_batch(seed, t, r, k):
    """``oracle.x0_philox(seed, t[i], r[i], k)`` for arrays t, r: float64 [M, 6 (k + 1)]."""
    t, r = np.asarray(t, dtype=np.int64), np.asarray(r, dtype=np.int64)
    n = o.n_params(k)
    pairs = n // 2
    ctr = np.zeros((len(t), pairs, 4), dtype=np.uint32)
    ctr[..., 0] = np.arange(pairs, dtype=np.uint32)[None, :]
    ctr[..., 1] = r.astype(np.uint32)[:, None]
    ctr[..., 2] = (t & 0xFFFFFFFF).astype(np.uint32)[:, None]
    ctr[..., 3] = np.uint32(k)
    w = o.philox4x32(ctr, (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)).astype(np.uint64)
    u0 = ((w[..., 0] >> np.uint64(5)) * np.uint64(1 << 26) + (w[..., 1] >> np.uint64(6))).astype(np.float64) * (1.0 / 9007199254740992.0)
    u1 = ((w[..., 2] >> np.uint64(5)) * np.uint64(1 << 26) + (w[..., 3] >> np.uint64(6))).astype(np.float64) * (1.0 / 9007199254740992.0)
    x = np.empty((len(t), n))
    x[:, 0::2] = u0 * o.TWO_PI
    x[:, 1::2] = u1 * o.TWO_PI
    return x


class Tables:
    """Item tables of one gate over the first ``n`` Haar targets, on a context of their own that runs single stages only."""

    def __init__(self, gate, n, restarts):
        self.ctx = _ffi.Context(0)
        self.ctx.sample_haar(HAAR_SEED, n)
        self.ctx.set_gates(gate[None])
        self.loss, self.evals, self.px, self.have = {}, {}, {}, {}
        for k in (1, 2, 3):
            out = self.ctx.minimize_stage([0] * k, _prm(restarts, 0))
            self.loss[k], self.evals[k] = out["item_loss"], out["item_evals"]
            self.px[k] = np.full((n, restarts, 6 * (k + 1)), np.nan)
            self.have[k] = np.zeros((n, restarts), dtype=bool)
        assert all(np.all(np.isfinite(v)) for v in self.loss.values())

    def params(self, k, t, r):
        """Parameters of the items (t[i], r[i]) of span k: each run alone, as a one-restart stage from its explicit start point."""
        t, r = np.asarray(t, dtype=np.int64), np.asarray(r, dtype=np.int64)
        need = ~self.have[k][t, r]
        if need.any():
            tt, rr = t[need], r[need]
            out = self.ctx.minimize_stage([0] * k, _prm(1, 0, seed=999), active=tt.astype(np.int32), x0=philox_x0_batch(SEED, tt, rr, k)[:, None, :])
            assert np.array_equal(out["best_loss"], self.loss[k][tt, rr]), "an item run alone does not end where it ends in its stage"
            self.px[k][tt, rr] = out["best_x"]
            self.have[k][tt, rr] = True
        return self.px[k][t, r]

    def sliced(self, n, R):
        return {k: v[:n, :R] for k, v in self.loss.items()}

    def close(self):
        self.ctx.close()


class Book:
    pass


@pytest.fixture(scope="module")
def book():
    b = Book()
    b.tab = Tables(SQ, NMAX, RMAX)
    b.ctx = _ffi.Context(0)
    b.cu = b.ctx.device_info()[1]
    b.ctx.sample_haar(HAAR_SEED, NMAX)
    b.ctx.set_gates(SQ[None])
    b.ctx.reset_stats()
    b.primed = b.ctx.decompose_range(0, NMAX, 1, 3, SEQS, _prm(3, ORDERED | STAGED), NEVER) + (b.ctx.fetch_span_losses(0, NMAX),)
    b.primed_items = b.ctx.stats()["items"][:4]
    yield b
    b.ctx.close()
    b.tab.close()


def _same(a, b):
    """Bit for bit, NaN positions compared separately."""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(np.nan_to_num(a, nan=0.0), np.nan_to_num(b, nan=0.0))


def order_statistic_threshold(stage_min, q):
    """The value with exactly floor(q n) of the n stage losses below it (one target: its own loss)."""
    v = np.sort(np.asarray(stage_min, dtype=np.float64))
    return float(v[min(int(q * len(v)), len(v) - 1)])


QUANTILES = (0.5, 0.4, 0.3, 0.25, 0.2, 0.15, 0.12, 0.1)


def case_shortcomings(mod, loss, thr, R, spans):
    """What keeps a case from being worth running (module docstring): conditions on the MODEL, empty when all hold."""
    k0 = spans[0]
    a0 = mod.active[k0]
    at_thr = a0[mod.span_loss[a0, k0 - 1] == thr]
    bad = []
    if len(at_thr) < 1:
        bad.append("no designated target with best == threshold")
    if len(spans) > 1 and mod.carry and not np.all(np.isin(at_thr, mod.active[k0 + 1])):
        bad.append("the model must KEEP a target whose best equals the threshold")
    if len(a0) < 20:
        return bad
    for k in spans[:2]:
        act = mod.active[k]
        kept = int((~(mod.span_loss[act, k - 1] < thr)).sum())
        if not (10 * kept >= len(act) and 10 * (len(act) - kept) >= len(act)):
            bad.append(f"span {k} keeps {kept} of {len(act)}")
    last = mod.active[spans[-1]]
    if int((~(mod.span_loss[last, spans[-1] - 1] < thr)).sum()) < 1:
        bad.append("every target is solved")
    if R > 1 and not any(np.any(mod.winner[k] != np.argmin(loss[k][mod.active[k]], axis=1)) for k in spans):
        bad.append("every winner is the lowest-loss restart")
    return bad


def run_model(tab, n_res, R, k_min, k_max, targets=None, first_size=None, carry=True, ordered=True, thr_from=None, thr_span=None,
              spans=None, winner_rule=True, extra=None, loss=None, params_of=None, n_of=model.default_n_of, nmax=24):
    """Threshold from the tables, then the model.  The threshold is the order statistic of the first-span stage losses at the first
    quantile of QUANTILES for which the MODEL meets the conditions of ``case_shortcomings`` (and ``extra(threshold)`` names no
    further one) -- asserted: a case that meets them at no quantile fails.  ``thr_from`` / ``thr_span``: the targets and the span
    whose stage losses give the order statistic (default: the case's targets at ``k_min``).  ``loss`` / ``params_of(threshold)``
    replace the tables and the parameter source of ``tab``."""
    loss = tab.sliced(n_res, R) if loss is None else loss
    sel = np.arange(n_res) if targets is None else np.asarray(targets)
    src = sel if thr_from is None else np.asarray(thr_from)
    spans = list(range(k_min, k_max + 1)) if spans is None else spans
    stage_min = loss[k_min if thr_span is None else thr_span][src].min(axis=1)
    kw = dict(targets=sel, n_resident=n_res, first_size=first_size, carry=carry, ordered=ordered, n_of=n_of, nmax=nmax)
    tried = {}
    for q in QUANTILES:
        thr = order_statistic_threshold(stage_min, q)
        dry = model.run_span_loop(loss, lambda k, t, r: np.zeros((len(t), n_of(k))), thr, k_min, k_max, **kw)
        tried[q] = case_shortcomings(dry, loss, thr, R if winner_rule else 1, spans) + (extra(thr) if extra else [])
        if not tried[q]:
            break
    assert not tried[q], tried
    mod = model.run_span_loop(loss, tab.params if params_of is None else params_of(thr), thr, k_min, k_max, **kw)
    print(f"[case] n_res={n_res} R={R} spans={spans} quantile={q} threshold={thr!r} active={[len(mod.active[k]) for k in spans]} "
          f"unsolved={len(mod.unsolved)}")
    return loss, thr, mod


def assert_results(ctx, mod, n_res, returned=None, window=None):
    loss, x, cyc = ctx.fetch_results_range(3, 0, n_res)
    span = ctx.fetch_span_losses(0, n_res)
    assert np.array_equal(cyc, mod.best_cycles)
    assert _same(loss, mod.best_loss)  # (+inf outside the window or list)
    assert _same(span, mod.span_loss)  # (NaN: span not run; all NaN outside)
    assert np.array_equal(x[mod.ran], mod.best_x[mod.ran])  # whole rows: the zeros behind 6 (cycles + 1) included
    if returned is not None:
        first, count = window
        for got, want in zip(returned, (loss, x, cyc)):
            assert np.array_equal(got, want[first : first + count])


def assert_items(st, mod, R, spans, launches=None):
    for k in range(1, 4):
        want = len(mod.active[k]) * R if k in spans else 0
        assert st["items"][k] == want, (k, st["items"][k], want)
        assert st["evals_accepted"][k] + st["evals_preempted"][k] <= st["evals"][k], k
    if launches is not None:
        assert st["kernel_launches"] == launches, (st["kernel_launches"], launches)


def test_batched_start_points_equal_the_oracle():
    t = np.array([0, 1, 7, 8484, 2**31 - 1, 3])
    r = np.array([0, 16, 3, 2, 1, 5])
    for k in (1, 2, 3):
        got = philox_x0_batch(SEED, t, r, k)
        for i in range(len(t)):
            assert np.array_equal(got[i], o.x0_philox(SEED, int(t[i]), int(r[i]), k))


def test_a_threshold_nothing_reaches_keeps_every_target_on_every_span(book):
    """The priming call: 8485 x 3 through the grid epilogue with nothing ever below the threshold -- every target runs all three
    spans, the best is the strict running minimum of the three stage minima."""
    loss = book.tab.sliced(NMAX, 3)
    mod = model.run_span_loop(loss, lambda k, t, r: np.zeros((len(t), 6 * (k + 1))), NEVER, 1, 3, nmax=24)
    got_loss, got_x, got_cyc, got_span = book.primed
    assert np.array_equal(got_cyc, mod.best_cycles) and _same(got_loss, mod.best_loss) and _same(got_span, mod.span_loss)
    assert len(set(got_cyc.tolist())) == 3 and book.primed_items == [0, NMAX * 3, NMAX * 3, NMAX * 3]
    width = 6 * (got_cyc + 1)
    col = np.arange(24)[None, :]
    assert np.all(got_x[col >= width[:, None]] == 0.0) and np.all(got_x[col < width[:, None]] != 0.0)


def _staged_cases():
    cases = []
    for N in (1, 255, 256, 257, 2048):              # stage_epilogue_kernel<256>
        for R in (1, 4, 5):
            cases.append((N, R, 0, 1))
    cases += [(2049, 3, 0, 1), (8192, 3, 0, 1)]     # stage_epilogue_kernel<1024>: chunks of 3 and 8 per thread
    for N in (8193, NMAX):                          # stage_epilogue_grid_kernel (8485 = 8192 + 256 + 37)
        for R in (3, 17):
            cases.append((N, R, 0, 1))
    # an unaligned window and a loop that starts at span 2, once per epilogue kernel
    cases += [(257, 4, 3, 1), (257, 4, 3, 2), (2049, 3, 3, 1), (2049, 3, 3, 2), (8193, 3, 3, 1), (8193, 3, 3, 2)]
    return cases


@pytest.mark.parametrize("N,R,first,k_min", _staged_cases())
def test_per_span_launches_equal_the_model(book, N, R, first, k_min):
    """ORDERED | STAGED: optimizer launch + one epilogue launch per span; the epilogue kernel follows the call's size."""
    n_res = N if first == 0 else N + first + 5
    spans = list(range(k_min, 4))
    loss, thr, mod = run_model(book.tab, n_res, R, k_min, 3, targets=np.arange(first, first + N))
    ctx = book.ctx
    ctx.sample_haar(HAAR_SEED, n_res)
    ctx.reset_stats()
    ret = ctx.decompose_range(first, N, k_min, 3, SEQS[k_min - 1 :], _prm(R, ORDERED | STAGED), thr)
    assert_results(ctx, mod, n_res, ret, (first, N))
    assert_items(ctx.stats(), mod, R, spans, launches=sum(len(mod.active[k]) > 0 for k in spans))


@pytest.mark.parametrize("N,R", [(1, 3), (63, 3), (64, 3), (65, 3), (8229, 3), (1, 17), (63, 17), (64, 17), (65, 17)])
def test_side_by_side_spans_equal_the_model(book, N, R):
    """ORDERED | OVERLAP: all spans of all targets at once, span_merge_kernel applies the loop afterwards.  Up to 16 restarts and
    two targets per compute unit the spans come from one wavefront per (target, span) -- one launch per span and the merge; beyond
    that, and with more than 16 restarts at any size, from helper contexts -- two launches per span and the merge."""
    loss, thr, mod = run_model(book.tab, N, R, 1, 3)
    ctx = book.ctx
    ctx.sample_haar(HAAR_SEED, N)
    ctx.reset_stats()
    ret = ctx.decompose_range(0, N, 1, 3, SEQS, _prm(R, ORDERED | OVERLAP), thr)
    assert_results(ctx, mod, N, ret, (0, N))
    helpers = R > 16 or N > 4 * book.cu
    assert N > 4 * book.cu or N <= 2 * book.cu
    assert_items(ctx.stats(), mod, R, [1, 2, 3], launches=7 if helpers else 4)


@pytest.mark.parametrize("R", [5, 16])
@pytest.mark.parametrize("size", ["1", "65", "2cu+1", "4cu", "4cu+1"])
def test_wave_loop_equals_the_model(book, size, R):
    """ORDERED | NO_OVERLAP: up to two targets per compute unit one wavefront per (target, span) and the merge; up to four the
    whole loop of a target in one wavefront (span_wave_kernel, ONE launch); one target more falls through to the per-span launches
    and must still match."""
    cu = book.cu
    N = {"1": 1, "65": 65, "2cu+1": 2 * cu + 1, "4cu": 4 * cu, "4cu+1": 4 * cu + 1}[size]
    assert N <= NMAX
    loss, thr, mod = run_model(book.tab, N, R, 1, 3)
    ctx = book.ctx
    ctx.sample_haar(HAAR_SEED, N)
    ctx.reset_stats()
    ret = ctx.decompose_range(0, N, 1, 3, SEQS, _prm(R, ORDERED | NO_OVERLAP), thr)
    assert_results(ctx, mod, N, ret, (0, N))
    assert_items(ctx.stats(), mod, R, [1, 2, 3], launches=4 if N <= 2 * cu else (1 if N <= 4 * cu else 3))


def test_wave_loop_window_from_span_2_equals_the_model(book):
    """span_wave_kernel on an unaligned window with k_min = 2."""
    N, R, first = 2 * book.cu + 1, 5, 3
    n_res = N + first + 5
    loss, thr, mod = run_model(book.tab, n_res, R, 2, 3, targets=np.arange(first, first + N))
    ctx = book.ctx
    ctx.sample_haar(HAAR_SEED, n_res)
    ctx.reset_stats()
    ret = ctx.decompose_range(first, N, 2, 3, SEQS[1:], _prm(R, ORDERED | NO_OVERLAP), thr)
    assert_results(ctx, mod, n_res, ret, (first, N))
    assert_items(ctx.stats(), mod, R, [2, 3], launches=1)


def test_list_mode_equals_the_model(book):
    """decompose_list: a shuffled, non-contiguous 2049-target subset of 5000 resident targets (init_results_kernel in list mode,
    stage_epilogue_kernel<1024>); nobody else is touched."""
    n_res, n_list, R = 5000, 2049, 3
    lst = np.random.default_rng(8).permutation(n_res)[:n_list]
    assert not np.array_equal(lst, np.sort(lst)) and lst.max() - lst.min() >= n_list
    loss, thr, mod = run_model(book.tab, n_res, R, 1, 3, targets=lst)
    ctx = book.ctx
    ctx.sample_haar(HAAR_SEED, n_res)
    ctx.reset_stats()
    ctx.decompose_list(lst, 1, 3, SEQS, _prm(R, ORDERED), thr, k_layout=3)
    assert_results(ctx, mod, n_res)
    assert int((~mod.ran).sum()) == n_res - n_list
    assert_items(ctx.stats(), mod, R, [1, 2, 3], launches=3)


@pytest.mark.parametrize("carry", [False, True])
def test_predicted_sizes_equal_the_model(book, carry):
    """decompose_predicted: 3000 Haar targets, sqrt(iSWAP) -- about four in five need two gates (a size list above 1024 entries:
    stage_append_kernel loops), the rest three, nobody one.  The sizes are the library's own lookup (``predict_spans``); the
    threshold is the order statistic of the span-2 stage losses of the size-2 targets."""
    from slam_decomposition_amd.weyl import c1c2c3

    n, R = 3000, 3
    coords = [c1c2c3(SQ)] * 3
    tol = 5e-4 if carry else 2e-8
    ctx = book.ctx
    ctx.sample_haar(HAAR_SEED, n)
    size = ctx.predict_spans(coords, 3, 0, n, tol=tol)
    assert int((size == 2).sum()) > 1024 and int((size == 3).sum()) >= 20 and int((size == 1).sum()) == 0
    loss, thr, mod = run_model(book.tab, n, R, 1, 3, first_size=size, carry=carry, thr_from=np.nonzero(size == 2)[0], thr_span=2, spans=[2, 3])
    assert len(mod.active[1]) == 0
    if carry:
        assert len(mod.active[3]) > int((size == 3).sum())
    ctx.reset_stats()
    n_loc, n_unr = ctx.decompose_predicted(coords, 3, SEQS, _prm(R, ORDERED), thr, 0, n, carry=carry, tol=tol)
    assert n_loc == int((size == 0).sum()) and n_unr == int((size > 3).sum())
    assert_results(ctx, mod, n)
    assert_items(ctx.stats(), mod, R, [2, 3], launches=2)


def test_multi_context_call_equals_the_model(book):
    """decompose_multi: two contexts with different gates behind one chain of kernels (stage_epilogue_multi_kernel), a window of 513
    targets; each context against the model of its own tables."""
    N, R, first = 513, 3, 3
    n_res = N + first + 5
    gate_b = o.riswap_matrix(0.4)
    tab_b = Tables(gate_b, n_res, R)
    other = _ffi.Context(0)
    try:
        sel = np.arange(first, first + N)
        loss_b = tab_b.sliced(n_res, R)

        def second_gate(thr):
            """The second gate's tables under the first one's threshold: every span must still keep and drop."""
            dry = model.run_span_loop(loss_b, lambda k, t, r: np.zeros((len(t), 6 * (k + 1))), thr, 1, 3, targets=sel, n_resident=n_res, nmax=24)
            return [w for w in case_shortcomings(dry, loss_b, thr, R, [1, 2, 3]) if "threshold" not in w]

        loss_a, thr, mod_a = run_model(book.tab, n_res, R, 1, 3, targets=sel, extra=second_gate)
        mod_b = model.run_span_loop(loss_b, tab_b.params, thr, 1, 3, targets=sel, n_resident=n_res, nmax=24)
        ctxs = [book.ctx, other]
        for c, g in zip(ctxs, (SQ, gate_b)):
            c.sample_haar(HAAR_SEED, n_res)
            c.set_gates(g[None])
            c.reset_stats()
        _ffi.decompose_multi(ctxs, first, N, 1, 3, SEQS, _prm(R, ORDERED), thr)
        for c, mod in zip(ctxs, (mod_a, mod_b)):
            assert_results(c, mod, n_res)
            assert_items(c.stats(), mod, R, [1, 2, 3])  # every context is booked the items of its own queues
    finally:
        book.ctx.set_gates(SQ[None])
        other.close()
        tab_b.close()


def test_v2_loop_equals_the_model(book):
    """slam_v2_decompose_range, RiSwapGate with its parameter free: rows of 6 (k + 1) + k parameters (13, 20, 27 -- the row copy's
    tail loop), 2049 targets (stage_epilogue_kernel<1024>).  The model's tables come from ``v2_minimize_stage`` without early
    exit; a stage's winner and its parameters from the same call with the threshold as its exit level."""
    from slam_decomposition_amd.basisv2 import CircuitTemplateV2
    from slam_decomposition_amd.gates import RiSwapGate

    N, R = 2049, 3
    basis = CircuitTemplateV2(base_gates=[RiSwapGate], maximum_span_guess=3)
    lay = {}
    for k in (1, 2, 3):
        basis.build(k)
        lay[k] = basis.device_layout(k)
    assert [lay[k][0] for k in (1, 2, 3)] == [13, 20, 27]
    ctx = book.ctx
    ctx.sample_haar(HAAR_SEED, N)
    ctx.v2_set_gates(basis._gate_maps)
    loss = {k: ctx.v2_minimize_stage([0] * k, _prm(R, 0), 1.0, *lay[k][2:6])["item_loss"] for k in (1, 2, 3)}

    def params_of(thr):
        stage = {k: ctx.v2_minimize_stage([0] * k, _prm(R, 0), thr, *lay[k][2:6]) for k in (1, 2, 3)}
        for k in (1, 2, 3):
            assert np.array_equal(stage[k]["item_loss"], loss[k])  # (the exit level decides the winner, not where an item ends)

        def params(k, t, r):
            assert np.array_equal(stage[k]["best_restart"][t], r) and np.array_equal(stage[k]["best_loss"][t], loss[k][t, r])
            return stage[k]["best_x"][t]

        return params

    _, thr, mod = run_model(None, N, R, 1, 3, loss=loss, params_of=params_of, n_of=lambda k: lay[k][0], nmax=27)
    ctx.reset_stats()
    got_loss, got_x, got_cyc = ctx.v2_decompose_range(0, N, 1, 3, SEQS, [lay[k][2:6] for k in (1, 2, 3)], _prm(R, ORDERED), thr)
    assert np.array_equal(got_cyc, mod.best_cycles) and _same(got_loss, mod.best_loss) and np.array_equal(got_x, mod.best_x)
    assert got_x.shape == (N, 27) and len(set(got_cyc.tolist())) == 3
    assert _same(ctx.fetch_span_losses(0, N), mod.span_loss)
    assert_items(ctx.stats(), mod, R, [1, 2, 3], launches=3)


@pytest.mark.parametrize("N", [257, 2049, NMAX])
def test_counters_without_early_exit_are_exact(book, N):
    """flags = STAGED only: nothing is pre-empted, so every per-span figure is a function of the item tables and the model's active
    sets (which do not depend on the winner rule).  The results are the model's with the lowest-loss winner."""
    R = 3
    loss, thr, mod = run_model(book.tab, N, R, 1, 3, ordered=False, winner_rule=False)
    accepted = {}
    for k in (1, 2, 3):
        book.tab.ctx.reset_stats()
        book.tab.ctx.minimize_stage([0] * k, _prm(R, 0), active=mod.active[k].astype(np.int32), want_items=False)
        accepted[k] = book.tab.ctx.stats()["evals_accepted"][k]
    ctx = book.ctx
    ctx.sample_haar(HAAR_SEED, N)
    ctx.reset_stats()
    ret = ctx.decompose_range(0, N, 1, 3, SEQS, _prm(R, STAGED), thr)
    assert_results(ctx, mod, N, ret, (0, N))
    st = ctx.stats()
    for k in (1, 2, 3):
        act = mod.active[k]
        assert st["items"][k] == len(act) * R, k
        assert st["evals"][k] == int(book.tab.evals[k][act, :R].sum(dtype=np.int64)), k
        assert st["evals_preempted"][k] == 0, k
        assert st["evals_accepted"][k] == accepted[k] and 0 < accepted[k] <= st["evals"][k], k
