"""A recording stand-in for ``_ffi.Context`` and the driver cases of ``TemplateOptimizer`` that run against it (CPU, no library).

``FakeCtx`` 'optimises' by formula: the loss, the parameters and the iteration count of an item are a pure function of
(global target index, template size k, restart) and nothing else, so a sharded run and an unsharded one must agree.  The losses
straddle the success threshold (``(t + k) % 3 == 0`` succeeds) and are not monotone in k (k = 2 is worse than k = 1), so both
branches of the span loop's merge rule are taken.  Every context keeps its OWN transcript -- (method, encoded arguments) in call
order -- because helper threads interleave; ``Book`` hands the contexts out in place of ``runtime.get_context`` / ``_ffi.Context``.

``CASES`` are the strategy runs that ``tests/test_optimizer_driver_host.py`` compares with ``tests/golden/
optimizer_driver_transcripts.json``; ``tools/make_driver_transcripts.py`` records that file from the same functions.
"""
import contextlib
import ctypes
import hashlib
import threading

import numpy as np

from slam_decomposition_amd import _ffi, runtime
from slam_decomposition_amd.basis_abc import RowBlocks

N_SPANS = _ffi.MAX_SPAN_EVAL
BIG = 128  # arrays with more elements are recorded as a digest


# ---- what the stand-in 'computes' ------------------------------------------------------------------------------------------------
def item_loss(t, k, r):
    if (t + k) % 3 == 0 and r >= t % 2:
        return 1e-12 * (r + 1)
    return 0.5 / k + (0.3 if k == 2 else 0.0) + 0.001 * ((t + r) % 4)


def item_x(t, k, r, n):
    return t + 0.1 * k + 0.01 * r + 0.001 * np.arange(n)


def stage_winner(t, k, R, threshold):
    """(loss, restart) a stage ends with: the first restart below the threshold, else the lowest loss (first occurrence)."""
    losses = [item_loss(t, k, r) for r in range(R)]
    for r, v in enumerate(losses):
        if v < threshold:
            return v, r
    r = int(np.argmin(losses))
    return losses[r], r


# ---- encoding of arguments and results (JSON, exact) -----------------------------------------------------------------------------
def _plain(v):
    if isinstance(v, list):
        return [_plain(x) for x in v]
    if isinstance(v, complex):
        return [_plain(v.real), _plain(v.imag)]
    if isinstance(v, float) and not np.isfinite(v):
        return repr(v)
    return v


def encode(v):
    if v is None or isinstance(v, (bool, int, str)):
        return v
    if isinstance(v, float):
        return _plain(v)
    if isinstance(v, np.generic):
        return _plain(v.item())
    if isinstance(v, np.ndarray):
        head = {"dtype": str(v.dtype), "shape": list(v.shape)}
        if v.size > BIG:
            return dict(head, sha1=hashlib.sha1(np.ascontiguousarray(v).tobytes()).hexdigest())
        return dict(head, v=_plain(v.tolist()))
    if isinstance(v, ctypes.Array):
        return [encode(x) for x in v]
    if isinstance(v, ctypes.Structure):
        return {name: encode(getattr(v, name)) for name, _ in v._fields_}
    if isinstance(v, dict):
        return {str(key): encode(x) for key, x in v.items()}
    if isinstance(v, (list, tuple, range)):
        return [encode(x) for x in v]
    if isinstance(v, RowBlocks):
        return encode(v.as_array())
    raise TypeError(f"cannot record a {type(v).__name__}")


class FakeCtx:
    def __init__(self, book, device, slot):
        self.book, self.device, self.slot = book, device, slot
        self.log = []
        self.n_targets = 0
        self.v2_qn = self.smush_qn = 0
        self.reset_stats(record=False)

    def _rec(self, name, **args):
        self.log.append([name, {key: encode(v) for key, v in args.items()}])
        fail = self.book.fail.get((self.device, self.slot, name))
        if fail is not None:
            raise fail

    # -- residency
    def _resident(self, n):
        self.n_targets = n
        self.res_loss = np.full(n, np.inf)
        self.res_x = {}
        self.res_cycles = np.full(n, -1, dtype=np.int32)
        self.res_span = np.full((n, N_SPANS), np.nan)

    def set_targets(self, targets):
        t = np.asarray(targets)
        self._rec("set_targets", index=np.real(t[:, 0, 0]), sha1=hashlib.sha1(np.ascontiguousarray(t).tobytes()).hexdigest())
        self._resident(len(t))

    def sample_haar(self, seed, n_targets, first_index=0):
        self._rec("sample_haar", seed=seed, n_targets=n_targets, first_index=first_index)
        self._resident(int(n_targets))

    def set_gates(self, gates):
        self._rec("set_gates", gates=np.asarray(gates))

    def v2_set_gates(self, gates):
        self._rec("v2_set_gates", gates=list(gates))
        self.v2_qn = int(gates[0].n_params)

    def v2_set_constraint(self, k, weights, cost_max=0.0):
        self._rec("v2_set_constraint", k=k, weights=weights, cost_max=cost_max)

    def set_cost(self, kind):
        self._rec("set_cost", kind=kind)

    def close(self):
        self._rec("close")

    # -- statistics
    def reset_stats(self, record=True):
        if record:
            self._rec("reset_stats")
        self.launches = 0
        self.items = [0] * (N_SPANS + 1)

    def stats(self):
        self._rec("stats")
        zeros = [0] * (N_SPANS + 1)
        return {"kernel_ms": 0.25 * self.launches, "kernel_launches": self.launches, "evals": [3 * v for v in self.items], "items": list(self.items),
                "total_ms": 0.5 * self.launches + 0.125 * sum(self.items), "kernel_ms_span": [0.0] * (N_SPANS + 1), "wave_rounds": list(zeros),
                "evals_accepted": list(zeros), "evals_preempted": list(zeros)}

    # -- the span loop
    def _span_loop(self, local, ks, params, threshold, n_of):
        """The loop of optimizer.py:233-303 for the resident targets ``local`` over the sizes ``ks``; results stay resident."""
        R = int(params.restarts)
        self.launches += 1
        for i in local:
            i, t = int(i), int(params.target_base) + int(i)
            self.res_loss[i], self.res_cycles[i], self.res_span[i] = np.inf, -1, np.nan
            for k in ks:
                loss, r = stage_winner(t, k, R, threshold)
                self.items[k] += R
                if self.res_cycles[i] < 0 or loss < self.res_loss[i]:
                    self.res_loss[i], self.res_cycles[i], self.res_x[i] = loss, k, item_x(t, k, r, n_of(k))
                self.res_span[i, k - 1] = self.res_loss[i]
                if self.res_loss[i] < threshold:
                    break

    def _rows(self, first, count, width):
        x = np.zeros((count, width))
        for j in range(count):
            row = self.res_x.get(first + j)
            if row is not None:
                x[j, : len(row)] = row
        return x

    def decompose_range(self, first, count, k_min, k_max, gate_seqs, params, success_threshold, fetch=True, pinned=False):
        self._rec("decompose_range", first=first, count=count, k_min=k_min, k_max=k_max, gate_seqs=gate_seqs, params=params,
                  success_threshold=success_threshold, fetch=fetch, pinned=pinned)
        assert 0 <= first and first + count <= self.n_targets
        self._span_loop(range(first, first + count), range(k_min, k_max + 1), params, success_threshold, lambda k: 6 * (k + 1))
        return self._fetch(k_max, first, count) if fetch else None

    def decompose_list(self, targets, k_min, k_max, gate_seqs, params, success_threshold, k_layout=0):
        self._rec("decompose_list", targets=np.asarray(targets), k_min=k_min, k_max=k_max, gate_seqs=gate_seqs, params=params,
                  success_threshold=success_threshold, k_layout=k_layout)
        self._span_loop(targets, range(k_min, k_max + 1), params, success_threshold, lambda k: 6 * (k + 1))

    def decompose_predicted(self, gate_coords_seq, k_max, gate_seqs, params, success_threshold, first=0, count=None, carry=False, tol=2e-8):
        self._rec("decompose_predicted", gate_coords_seq=gate_coords_seq, k_max=k_max, gate_seqs=gate_seqs, params=params,
                  success_threshold=success_threshold, first=first, count=count, carry=carry, tol=tol)
        for i in range(first, first + count):  # the size a target 'needs': 1 + t % k_max
            self._span_loop([i], [1 + (int(params.target_base) + i) % k_max], params, success_threshold, lambda k: 6 * (k + 1))
        return self.book.predicted

    def _fetch(self, k_max, first, count):
        return self.res_loss[first : first + count].copy(), self._rows(first, count, 6 * (k_max + 1)), self.res_cycles[first : first + count].copy()

    def fetch_results_range(self, k_max, first, count, pinned=False):
        self._rec("fetch_results_range", k_max=k_max, first=first, count=count, pinned=pinned)
        return self._fetch(k_max, first, count)

    def fetch_span_losses(self, first, count):
        self._rec("fetch_span_losses", first=first, count=count)
        return self.res_span[first : first + count].copy()

    # -- V2 / smush templates
    def v2_decompose_range(self, first, count, k_min, k_max, gate_seqs, layouts, params, threshold):
        self._rec("v2_decompose_range", first=first, count=count, k_min=k_min, k_max=k_max, gate_seqs=gate_seqs, layouts=layouts, params=params,
                  threshold=threshold)
        n_of = lambda k: 6 * (k + 1) + self.v2_qn * k
        self._span_loop(range(first, first + count), range(k_min, k_max + 1), params, threshold, n_of)
        return self.res_loss[first : first + count].copy(), self._rows(first, count, n_of(k_max)), self.res_cycles[first : first + count].copy()

    def _stage(self, n, params, threshold, active, want_items, trace_cap=None):
        act = np.arange(self.n_targets) if active is None else np.asarray(active)
        R, na = int(params.restarts), len(act)
        k = self._k
        self.launches += 1
        self.items[k] += na * R
        out = {"best_loss": np.empty(na), "best_x": np.empty((na, n)), "best_restart": np.empty(na, dtype=np.int32)}
        items = want_items or trace_cap is not None
        if items:
            out.update(item_loss=np.empty((na, R)), item_iters=np.empty((na, R), dtype=np.int32), item_status=np.zeros((na, R), dtype=np.int32))
        if trace_cap is not None:
            out.update(trace_loss=np.full((na, R, trace_cap), np.nan), trace_x=np.full((na, R, trace_cap, n), np.nan))
        elif want_items:
            out["item_evals"] = np.empty((na, R), dtype=np.int32)
        for j, i in enumerate(act):
            t = int(params.target_base) + int(i)
            out["best_loss"][j], r = stage_winner(t, k, R, threshold)
            out["best_x"][j], out["best_restart"][j] = item_x(t, k, r, n), r
            for r in range(R if items else 0):
                it = 300 if (t, k, r) == self.book.long_item else 2 + (t + r) % 3
                out["item_loss"][j, r], out["item_iters"][j, r] = item_loss(t, k, r), it
                if trace_cap is None:
                    out["item_evals"][j, r] = 2 * it
                    continue
                for s in range(min(it, trace_cap)):
                    out["trace_loss"][j, r, s] = item_loss(t, k, r) + 0.0625 * (it - 1 - s)
                    out["trace_x"][j, r, s] = item_x(t, k, r, n) + s
        return out

    def v2_minimize_stage(self, gate_seq, params, exit_loss, init_lo, init_hi, bound_lo=None, bound_hi=None, active=None, x0=None,
                          want_items=True, _name="v2_minimize_stage"):
        self._rec(_name, gate_seq=gate_seq, params=params, exit_loss=exit_loss, init_lo=init_lo, init_hi=init_hi, bound_lo=bound_lo,
                  bound_hi=bound_hi, active=active, x0=x0, want_items=want_items)
        self._k = len(gate_seq)
        out = self._stage(6 * (self._k + 1) + self.v2_qn * self._k, params, exit_loss, active, want_items)
        if not want_items:
            out.update(item_loss=None, item_iters=None, item_status=None, item_evals=None)
        return out

    def minimize_stage_trace(self, gate_seq, params, exit_loss, trace_cap, active=None, x0=None):
        self._rec("minimize_stage_trace", gate_seq=gate_seq, params=params, exit_loss=exit_loss, trace_cap=trace_cap, active=active, x0=x0)
        self._k = len(gate_seq)
        return self._stage(6 * (self._k + 1), params, exit_loss, active, True, trace_cap=int(trace_cap))

    # -- evaluations
    def eval_c1c2c3(self, gate_seq, x, ndigits=8):
        x = np.asarray(x)
        self._rec("eval_c1c2c3", gate_seq=gate_seq, x=x, ndigits=ndigits)
        return np.stack([x[:, 0], x[:, 1], x[:, 0] + x[:, 2]], axis=1)

    def eval_loss_grad(self, gate_seq, x, target_of, want_grad=True):
        """A convex quadratic, so that a simplex search ends soon; the calls are counted, not recorded (there are thousands)."""
        self.book.evals += 1
        x = np.asarray(x)
        return ((x - 1.0) ** 2).sum(axis=1) + 0.25 * np.asarray(target_of), None


class Book:
    """The contexts of one case: slot ``slot`` of ``device`` for ``runtime.get_context``, a fresh one per ``_ffi.Context(device)``
    (keyed ``(device, "fresh")``: the cases create at most one per device)."""

    def __init__(self):
        self.ctxs = {}
        self.fail = {}  # (device, slot, method) -> exception to raise there
        self.predicted = (0, 0)  # what decompose_predicted reports: (n_local, n_unreachable)
        self.long_item = None  # (t, k, r) of a restart that takes 300 iterations
        self.evals = 0
        self._lock = threading.Lock()

    def get_context(self, device=0, slot=0):
        with self._lock:
            if (device, slot) not in self.ctxs:
                self.ctxs[(device, slot)] = FakeCtx(self, device, slot)
            return self.ctxs[(device, slot)]

    def fresh_context(self, device=0):
        with self._lock:
            assert (device, "fresh") not in self.ctxs
            ctx = self.ctxs[(device, "fresh")] = FakeCtx(self, device, "fresh")
            return ctx

    @contextlib.contextmanager
    def installed(self):
        saved = runtime.get_context, _ffi.Context
        runtime.get_context, _ffi.Context = self.get_context, self.fresh_context
        try:
            yield self
        finally:
            runtime.get_context, _ffi.Context = saved

    def transcripts(self):
        return {f"{d}/{s}": ctx.log for (d, s), ctx in sorted(self.ctxs.items(), key=lambda kv: (kv[0][0], str(kv[0][1])))}


# ---- the cases -------------------------------------------------------------------------------------------------------------------
def index_targets(n):
    """Targets that 'are' their index (element [0, 0])."""
    t = np.zeros((n, 4, 4), dtype=np.complex128)
    t[:, 0, 0] = np.arange(n)
    return t


def fixed_optimizer(**kw):
    from slam_decomposition_amd.basis import CircuitTemplate
    from slam_decomposition_amd.cost_function import BasicCost
    from slam_decomposition_amd.gates import CXGate
    from slam_decomposition_amd.optimizer import TemplateOptimizer

    kw.setdefault("training_restarts", 4)
    return TemplateOptimizer(CircuitTemplate(base_gates=[CXGate()], maximum_span_guess=3), BasicCost(), seed=1, **kw)


def v2_optimizer(**kw):
    from slam_decomposition_amd.basisv2 import CircuitTemplateV2
    from slam_decomposition_amd.cost_function import BasicCost
    from slam_decomposition_amd.gates import RiSwapGate
    from slam_decomposition_amd.optimizer import TemplateOptimizer

    return TemplateOptimizer(CircuitTemplateV2(base_gates=[RiSwapGate], maximum_span_guess=3), BasicCost(), seed=1, training_restarts=4, **kw)


def device_sampler(n):
    from slam_decomposition_amd.sampler import DeviceHaarBatch

    return DeviceHaarBatch(seed=5, n_samples=n, start=100)


def run_case(call, opt, book=None, extra=lambda opt: {}, results=True):
    """Run ``call(opt)`` against the stand-in contexts and collect everything the test compares: the transcripts per context, the
    three returned arrays (or the exception), ``_span_losses``, ``last_stats`` / ``last_stats_per_device`` and the case's extras.
    ``results=False`` leaves the arrays out (the simplex search of the host method: only its preparation and statistics are pinned)."""
    book = book or Book()
    out = {}
    with book.installed():
        try:
            returned = call(opt)
            out["returned"] = encode(returned) if results else None
        except Exception as exc:
            out["error"] = [type(exc).__name__, str(exc)]
    out["transcripts"] = book.transcripts()
    out["span_losses"] = encode(getattr(opt, "_span_losses", None)) if results else None
    out["last_stats"] = encode(opt.last_stats)
    out["last_stats_per_device"] = encode(opt.last_stats_per_device)
    out["extra"] = encode(extra(opt))
    return out, book


class _Entry:
    """A coverage entry as ``_run_batch_mixed_order`` reads it: a length and the gate indices."""

    def __init__(self, gate_indices):
        self.gate_indices = list(gate_indices)

    def __len__(self):
        return len(self.gate_indices)


def _mixed(opt, coords):
    n = len(coords)
    masks = [np.arange(n) % 2 == 0, np.arange(n) < 4, np.ones(n, bool)]  # overlapping
    entries = [(_Entry(g), m, None) for g, m in zip(([0], [0, 0], [0, 0]), masks)]
    opt.basis.minimal_spans = lambda c: None
    opt.basis.candidate_entries = lambda c: entries
    opt._mixed_entries = entries
    return opt._run_batch_mixed_order(index_targets(n), coords)


def _mixed_extra(opt):
    ids = [id(e) for e, _, _ in getattr(opt, "_mixed_entries", [])]
    return {"circuit_polytopes": [ids.index(id(e)) for e in getattr(opt, "circuit_polytopes", None) or []],
            "entries_tried": getattr(opt, "_entries_tried", None)}


class _Family:
    multipliers = np.array([1, 2, 4], dtype=np.int64)
    durations = np.array([0.25, 0.5, 1.0])
    cost_1q = 0.125

    def __init__(self, members, gates):
        self.members, self.gates = np.asarray(members, dtype=np.int32), np.asarray(gates, dtype=np.int32)

    def device_lookup(self, ctx, policy="reference", first=0, count=None, want_targets=False):
        ctx._rec("family.device_lookup", policy=policy, first=first, count=count, want_targets=want_targets)
        return None, None, self.members, self.gates

    def unreachable_error(self):
        return ValueError("no member of the family reaches the target")


def _family(opt, members, gates, sampler=False):
    opt.basis.family, opt.basis.policy = _Family(members, gates), "reference"
    if sampler:
        opt._device_sampler = device_sampler(len(members))
    return opt._run_batch_family(index_targets(len(members)), len(members))


def _family_extra(opt):
    return {"family_members": opt.family_members, "family_costs": opt.family_costs}


def _predicted(opt, n):
    opt._device_sampler = device_sampler(n)
    opt.basis._gate_coords_all = [np.array([0.5, 0.0, 0.0])]
    return opt._run_batch_predicted(runtime.get_context(0), n)


def _windows(opt, n):
    return opt._run_batch_windows(n, index_targets(n), [1, 2, 3], [[0], [0, 0], [0, 0, 0]], opt._opt_params())


def _callback(opt, spans_per_target):
    return opt._run_batch_callback(index_targets(len(spans_per_target)), spans_per_target)


def _callback_extra(opt):
    records = getattr(opt, "_callback_records", None) or []
    return {"records": [[[tl, cl] for tl, cl in per] for per in records],
            "same_growing_list": [all(tl is per[0][0] for tl, _ in per) for per in records]}


def _with(opt, **attrs):
    for key, v in attrs.items():
        setattr(opt.basis if key == "_span_exact" else opt, key, v)
    return opt


def _book(**attrs):
    book = Book()
    for key, v in attrs.items():
        setattr(book, key, v)
    return book


_COORDS = np.full((6, 3), 0.25)
_SPANS = np.array([1, 2, 2, 3, 1])
_UNSUPPORTED = _ffi.SlamHipError(-3, "span x parameters per gate beyond the device kernels")

# name -> () -> (result, book)
CASES = {
    "run_batch_one_device": lambda: run_case(lambda o: o._run_batch(index_targets(7), [1, 2, 3]), fixed_optimizer()),
    "run_batch_one_device_no_span_losses": lambda: run_case(lambda o: o._run_batch(index_targets(7), [1, 2, 3]),
                                                            _with(fixed_optimizer(), _want_span_losses=False)),
    "run_batch_one_device_sampler": lambda: run_case(lambda o: o._run_batch(index_targets(7), [1, 2, 3]),
                                                     _with(fixed_optimizer(), _device_sampler=device_sampler(7))),
    "run_batch_not_deterministic": lambda: run_case(lambda o: o._run_batch(index_targets(7), [2, 3]), fixed_optimizer(deterministic=False)),
    "run_batch_two_devices": lambda: run_case(lambda o: o._run_batch(index_targets(7), [1, 2, 3]), fixed_optimizer(devices=[0, 1])),
    "run_batch_two_devices_no_span_losses": lambda: run_case(lambda o: o._run_batch(index_targets(7), [1, 2, 3]),
                                                             _with(fixed_optimizer(devices=[0, 1]), _want_span_losses=False)),
    "run_batch_two_devices_sampler": lambda: run_case(lambda o: o._run_batch(index_targets(7), [1, 2, 3]),
                                                      _with(fixed_optimizer(devices=[0, 1]), _device_sampler=device_sampler(7))),
    "run_batch_two_devices_one_target": lambda: run_case(lambda o: o._run_batch(index_targets(1), [1, 2, 3]), fixed_optimizer(devices=[0, 1])),
    "run_batch_auto_shards": lambda: run_case(lambda o: o._run_batch(index_targets(7), [1, 2, 3]),
                                              _with(fixed_optimizer(auto_shards=2), AUTO_SHARD_MIN_TARGETS=4)),
    "run_batch_auto_shards_below_minimum": lambda: run_case(lambda o: o._run_batch(index_targets(7), [1, 2, 3]),
                                                            _with(fixed_optimizer(auto_shards=2), AUTO_SHARD_MIN_TARGETS=8)),
    "run_batch_shard_raises": lambda: run_case(lambda o: o._run_batch(index_targets(7), [1, 2, 3]), fixed_optimizer(devices=[0, 1]),
                                               _book(fail={(1, 1, "decompose_range"): RuntimeError("shard 1 cannot run")})),
    "run_batch_span_too_large": lambda: run_case(lambda o: o._run_batch(index_targets(2), [16, 17]), fixed_optimizer()),
    "run_batch_span_too_large_any_order": lambda: run_case(lambda o: o._run_batch(index_targets(2), [1, 17]), fixed_optimizer()),
    "run_batch_empty_range": lambda: run_case(lambda o: o._run_batch(index_targets(2), []), fixed_optimizer()),
    "run_batch_span_zero": lambda: run_case(lambda o: o._run_batch(index_targets(2), [0, 1]), fixed_optimizer()),
    "windows": lambda: run_case(lambda o: _windows(o, 10), _with(fixed_optimizer(windows_in_flight=2), WINDOW_TARGETS=3)),
    "windows_sampler": lambda: run_case(lambda o: _windows(o, 10), _with(fixed_optimizer(windows_in_flight=2), WINDOW_TARGETS=3,
                                                                         _device_sampler=device_sampler(10), _want_span_losses=False)),
    "any_order": lambda: run_case(lambda o: o._run_batch(index_targets(10), [1, 3]), fixed_optimizer()),
    "any_order_sampler": lambda: run_case(lambda o: o._run_batch(index_targets(10), [1, 3]), _with(fixed_optimizer(), _device_sampler=device_sampler(10))),
    "any_order_descending": lambda: run_case(lambda o: o._run_batch(index_targets(10), [3, 2, 1]), fixed_optimizer()),
    "by_span_exact": lambda: run_case(lambda o: o._run_batch_by_span(index_targets(5), _SPANS), _with(fixed_optimizer(), _span_exact=True)),
    "by_span_exact_sampler": lambda: run_case(lambda o: o._run_batch_by_span(index_targets(5), _SPANS),
                                              _with(fixed_optimizer(), _span_exact=True, _device_sampler=device_sampler(5), _want_span_losses=False)),
    "by_span_lower_bound": lambda: run_case(lambda o: o._run_batch_by_span(index_targets(5), _SPANS), _with(fixed_optimizer(), _span_exact=False)),
    "by_span_zero": lambda: run_case(lambda o: o._run_batch_by_span(index_targets(2), np.array([0, 1])), fixed_optimizer()),
    "by_span_too_large": lambda: run_case(lambda o: o._run_batch_by_span(index_targets(2), np.array([1, 17])), fixed_optimizer()),
    "mixed_order": lambda: run_case(lambda o: _mixed(o, _COORDS), fixed_optimizer(), extra=_mixed_extra),
    "mixed_order_no_span_losses": lambda: run_case(lambda o: _mixed(o, _COORDS), _with(fixed_optimizer(), _want_span_losses=False), extra=_mixed_extra),
    "mixed_order_local_target": lambda: run_case(lambda o: _mixed(o, np.concatenate([_COORDS, np.zeros((1, 3))])), fixed_optimizer(), extra=_mixed_extra),
    "predicted": lambda: run_case(lambda o: _predicted(o, 7), fixed_optimizer()),
    "predicted_unreachable": lambda: run_case(lambda o: _predicted(o, 7), fixed_optimizer(), _book(predicted=(0, 2))),
    "predicted_local": lambda: run_case(lambda o: _predicted(o, 7), fixed_optimizer(), _book(predicted=(1, 0))),
    "family": lambda: run_case(lambda o: _family(o, [0, 2, 0, 1, 2, 0], [2, 1, 2, 3, 1, 1]), fixed_optimizer(), extra=_family_extra),
    "family_sampler": lambda: run_case(lambda o: _family(o, [0, 2, 0, 1, 2, 0], [2, 1, 2, 3, 1, 1], sampler=True),
                                       _with(fixed_optimizer(), _want_span_losses=False), extra=_family_extra),
    "family_unreachable": lambda: run_case(lambda o: _family(o, [0, -1, 0], [2, -1, 1]), fixed_optimizer(), extra=_family_extra),
    "family_local": lambda: run_case(lambda o: _family(o, [0, -1, 0], [2, 0, 1]), fixed_optimizer(), extra=_family_extra),
    "v2_range": lambda: run_case(lambda o: o._run_batch_v2(index_targets(7), [1, 2, 3]), v2_optimizer()),
    "v2_stage_loop": lambda: run_case(lambda o: o._run_batch_v2(index_targets(7), [1, 3]), v2_optimizer()),
    "v2_range_two_devices": lambda: run_case(lambda o: o._run_batch_v2(index_targets(7), [1, 2, 3]), v2_optimizer(devices=[0, 1])),
    "v2_stage_loop_two_devices": lambda: run_case(lambda o: o._run_batch_v2(index_targets(7), [1, 3]), v2_optimizer(devices=[0, 1])),
    "v2_two_devices_one_target": lambda: run_case(lambda o: o._run_batch_v2(index_targets(1), [1, 3]), v2_optimizer(devices=[0, 1])),
    "v2_range_unsupported": lambda: run_case(lambda o: o._run_batch_v2(index_targets(3), [1, 2]), v2_optimizer(),
                                             _book(fail={(0, 0, "v2_decompose_range"): _UNSUPPORTED})),
    "v2_stage_unsupported_two_devices": lambda: run_case(lambda o: o._run_batch_v2(index_targets(4), [1, 3]), v2_optimizer(devices=[0, 1]),
                                                         _book(fail={(1, "fresh", "v2_minimize_stage"): _UNSUPPORTED})),
    "v2_other_library_error": lambda: run_case(lambda o: o._run_batch_v2(index_targets(3), [1, 3]), v2_optimizer(),
                                               _book(fail={(0, 0, "v2_minimize_stage"): _ffi.SlamHipError(-2, "bad argument")})),
    "v2_span_zero": lambda: run_case(lambda o: o._run_batch_v2(index_targets(3), [0, 1]), v2_optimizer()),
    "v2_span_too_large": lambda: run_case(lambda o: o._run_batch_v2(index_targets(3), [1, 6]), v2_optimizer()),
    "callback": lambda: run_case(lambda o: _callback(o, [[1, 2, 3], [1, 2, 3], [2, 3]]), fixed_optimizer(use_callback=True, training_restarts=3),
                                 _book(long_item=(1, 1, 1)), extra=_callback_extra),
    "callback_override_fail": lambda: run_case(lambda o: _callback(o, [[1], [1, 2], [2]]),
                                               fixed_optimizer(use_callback=True, override_fail=True, training_restarts=3), extra=_callback_extra),
    "callback_nothing_ran": lambda: run_case(lambda o: _callback(o, [[1], []]), fixed_optimizer(use_callback=True), extra=_callback_extra),
    "callback_span_too_large": lambda: run_case(lambda o: _callback(o, [[17]]), fixed_optimizer(use_callback=True), extra=_callback_extra),
    "host_method": lambda: run_case(lambda o: o._run_batch_host_method(index_targets(3), [1]), fixed_optimizer(override_method="Nelder-Mead"),
                                    results=False),
    "host_method_span_too_large": lambda: run_case(lambda o: o._run_batch_host_method(index_targets(2), [17]),
                                                   fixed_optimizer(override_method="Nelder-Mead")),
}
