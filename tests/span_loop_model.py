"""Host model of the span loop's bookkeeping (pure NumPy): what ``slam_decompose*`` must return, given the per-stage item tables.

The loop it restates is the reference's (optimizer.py:287-303): spans in increasing order, restarts in index order, the running
best replaced by a strictly lower result, both loops left at the first ``best < threshold``.  Per stage that is

* stage winner: the lowest-index restart with ``loss < threshold``; if there is none, the lowest loss, ties to the lower index.
  NaN and +inf never win: a row without a loss below +inf gives (+inf, restart 0) -- the first result the sequential loop saw;
* a target takes a stage's result if it has none yet, or if the result is strictly lower;
* a target leaves the loop once ``best < threshold`` (strict).

``ordered=False`` is the loop without early exit: the winner is the lowest loss whatever the threshold.  Whether a target leaves
does not depend on that choice (some restart is below the threshold or none is), so the active sets are the same in both modes.

Inputs are indexed by RESIDENT target: ``item_loss[k]`` is float64 [N, R] for every span k the case runs, ``params(k, t, r)``
returns the parameters [len(t), n_of(k)] of the (target, restart) pairs ``t[i], r[i]`` (or ``params[k]`` is an array [N, R, n_of(k)]).
``targets`` selects the window or list the call works on; every other resident target keeps (+inf, -1, NaN).  ``first_size``
(int [N], resident index) is the predicted mode: 0 = local target (result (0, 0), no stage), 1..k_max = the span at which the target
joins the loop, larger = out of reach (no stage); with ``carry`` off a target runs at its own size only.
"""
from dataclasses import dataclass, field
from typing import Dict

import numpy as np

MAX_SPAN_EVAL = 16


def default_n_of(k: int) -> int:
    return 6 * (k + 1)


def stage_winner(loss: np.ndarray, threshold: float, ordered: bool = True) -> np.ndarray:
    """Winning restart of every row of ``loss[M, R]`` (int32 [M])."""
    loss = np.asarray(loss, dtype=np.float64)
    clean = np.where(np.isnan(loss), np.inf, loss)
    win = np.argmin(clean, axis=1)  # first occurrence of the minimum: ties to the lower index; an all-inf row gives 0
    if ordered:
        below = clean < threshold
        hit = below.any(axis=1)
        win = np.where(hit, np.argmax(below, axis=1), win)
    return win.astype(np.int32)


@dataclass
class SpanLoopResult:
    best_loss: np.ndarray
    best_cycles: np.ndarray
    best_x: np.ndarray
    span_loss: np.ndarray
    ran: np.ndarray                                   # bool [N]: the target went through at least one stage
    active: Dict[int, np.ndarray] = field(default_factory=dict)   # span -> sorted resident indices the stage works on
    winner: Dict[int, np.ndarray] = field(default_factory=dict)   # span -> winning restart of each of them
    stage_loss: Dict[int, np.ndarray] = field(default_factory=dict)
    unsolved: np.ndarray = None                       # resident indices still at or above the threshold after k_max (carry on)
    carry: bool = True                                # targets that miss the threshold went on to the next span


def _params_of(params, k, t, r, n):
    if callable(params):
        out = np.asarray(params(k, t, r), dtype=np.float64)
    else:
        out = np.asarray(params[k], dtype=np.float64)[t, r]
    if out.shape != (len(t), n):
        raise ValueError(f"parameters of span {k}: shape {out.shape}, expected {(len(t), n)}")
    return out


def run_span_loop(item_loss, params, threshold, k_min, k_max, *, targets=None, n_resident=None, first_size=None, carry=True,
                  ordered=True, n_of=default_n_of, nmax=None) -> SpanLoopResult:
    spans = range(k_min, k_max + 1)
    if n_resident is None:
        n_resident = int(np.asarray(item_loss[k_min]).shape[0])
    N = int(n_resident)
    nmax = n_of(k_max) if nmax is None else int(nmax)
    sel = np.arange(N) if targets is None else np.asarray(targets, dtype=np.int64).reshape(-1)
    if len(np.unique(sel)) != len(sel) or (len(sel) and (sel.min() < 0 or sel.max() >= N)):
        raise ValueError("targets must be distinct resident indices")
    res = SpanLoopResult(np.full(N, np.inf), np.full(N, -1, dtype=np.int32), np.zeros((N, nmax)),
                         np.full((N, MAX_SPAN_EVAL), np.nan), np.zeros(N, dtype=bool))
    if first_size is None:
        size = np.full(N, k_min, dtype=np.int64)
    else:
        size = np.asarray(first_size, dtype=np.int64)
        local = sel[size[sel] == 0]
        res.best_loss[local] = 0.0
        res.best_cycles[local] = 0
    carried = np.zeros(0, dtype=np.int64)
    for k in spans:
        act = np.sort(np.concatenate([carried, sel[size[sel] == k]]))
        res.active[k] = act
        L = np.asarray(item_loss[k], dtype=np.float64)[act]
        win = stage_winner(L, threshold, ordered)
        sl = np.where(np.isnan(L), np.inf, L)[np.arange(len(act)), win] if len(act) else np.zeros(0)
        res.winner[k] = win
        res.stage_loss[k] = sl
        take = (res.best_cycles[act] < 0) | (sl < res.best_loss[act])
        tk = act[take]
        if len(tk):
            n = n_of(k)
            res.best_loss[tk] = sl[take]
            res.best_cycles[tk] = k
            res.best_x[tk] = 0.0
            res.best_x[tk, :n] = _params_of(params, k, tk, win[take], n)
        res.span_loss[act, k - 1] = res.best_loss[act]
        res.ran[act] = True
        carried = act[~(res.best_loss[act] < threshold)] if carry else np.zeros(0, dtype=np.int64)
    res.unsolved = carried
    res.carry = bool(carry)
    return res


def sequential_reference_loop(item_loss, params, threshold, k_min, k_max, n_of=default_n_of):
    """The reference's loop, literally: target by target, span by span, restart by restart, ``break`` (optimizer.py:253-303).
    Returns (best_loss [N], best_cycles [N], best_x [N, n_of(k_max)], span_loss [N, 16])."""
    N, R = np.asarray(item_loss[k_min]).shape
    best_loss = np.full(N, np.inf)
    best_cycles = np.full(N, -1, dtype=np.int32)
    best_x = np.zeros((N, n_of(k_max)))
    span_loss = np.full((N, MAX_SPAN_EVAL), np.nan)
    for t in range(N):
        best_result, best_xk, cycles = None, None, -1
        for k in range(k_min, k_max + 1):
            for r in range(R):
                fun = float(item_loss[k][t][r])
                if best_result is None or fun < best_result:
                    best_result = fun
                    best_xk = _params_of(params, k, np.array([t]), np.array([r]), n_of(k))[0]
                    cycles = k
                if best_result < threshold:
                    break
            span_loss[t, k - 1] = best_result
            if best_result < threshold:
                break
        best_loss[t] = best_result
        best_cycles[t] = cycles
        best_x[t, : len(best_xk)] = best_xk
    return best_loss, best_cycles, best_x, span_loss
