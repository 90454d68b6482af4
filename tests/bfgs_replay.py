"""Teacher-forced replay of oracle/bfgs_port.py along an observed optimizer trajectory (NumPy only).

Free-running, the kernel's and the port's trajectories drift apart (the float32 metric is summed in another order), which is why the
end-to-end comparisons in test_gpu_minimize_parity.py are loose.  Here the port never runs free: at step j it starts from the OBSERVED
point x_j, predicts the accepted step with its own line search on oracle evaluations, is compared with the observed step

    dev_j = |s_obs - s_pred|_2 / |s_pred|_2,        s_obs = xs[j] - x_j,

and then adopts the observed point: the metric update, the next direction and every later branch decision (``short``, the curvature
test, the stall counter, growth, periodic restart, non-descent reset) use the port's formulas with s = s_obs and
y = g(xs[j]) - g(x_j) from the oracle.  A wrong back-track count moves dev_j by at least 0.5 and a wrong growth factor by at least
0.87, while float32 rounding of the metric moves it by 1e-7 .. 1e-3.

Unclear decisions.  The oracle's loss and gradient are known to the evaluation kernels' accuracy only, so a comparison whose margin
lies inside that accuracy cannot be settled from the reference alone: an Armijo margin inside the loss band (any trial), ``short`` or
the curvature test inside the gradient band, a termination threshold inside its band.  There the replay follows both branches and
keeps the one that matches the observation best; the step (and the item) is marked unclear and is held to the step tolerance all the
same.  The bands (``bands``) are twice the tolerance tests/hp_ref.py holds the evaluation kernels to -- two evaluations enter every
comparison -- and never come from anything a device returns.

Noise floor.  A step whose accepted decrease f_j - f_{j+1} is below the loss band is unclear by definition; the replay stops there
(``noise_from``) and the caller checks the rest of the item for a non-increasing trace, recorded losses, final status and final loss.
"""
from __future__ import annotations

import json
import os

import numpy as np

import hp_ref as hp
import makhlin_ref as mr
from oracle import bfgs_port as bp
from oracle import slam_oracle as o
# bound here once: a test that plants a defect in oracle.bfgs_port does not change the replay
from oracle.bfgs_port import (ARMIJO_C1, BACKTRACK_MAX, BACKTRACK_MIN, CURV_EPS, GROW_FACTOR, GROW_MAX, MAX_BACKTRACK, RESTART_PERIOD,
                              STALL_DF, STALL_GNORM, STEP_MAX, WOLFE_C2)

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "optimizer_replay_cases.json")
TOL_FACTOR = 8.0  # two for each of: the mat-vec's summation order, the rank-2 update's accumulate order, refined-seed reciprocals / y
TOL_CAP = 1e-2    # a condition, not a measurement: fifty times below the smallest effect of a wrong branch (0.5)
ST_CONVERGED, ST_MAXITER, ST_LINESEARCH, ST_NONFINITE, ST_STALLED = range(5)
FLAG_NO_EXTERIOR = 32
DEFAULTS = dict(maxiter=2500, gtol=1e-9, stop_loss=1e-13, gtol_far=1e-5, far_loss=1e-6)


# ---- cases ---------------------------------------------------------------------------------------------------------------------
def gate_matrix(spec):
    kind = spec[0]
    if kind == "cx":
        return o.cx_matrix()
    if kind == "riswap":
        return o.riswap_matrix(float(spec[1]))
    if kind == "dense":
        return o.haar_unitary(int(spec[1]))
    if kind == "cg":
        return o.conversion_gain_matrix(*[float(v) for v in spec[1:]])
    raise ValueError(spec)


def target_matrix(case, t):
    """"haar": o.haar_unitary(5000 + t); "swap"; ["canonical", c1, c2, c3]: a fixed point of the Weyl chamber.  ``nan_target``: one
    entry of the target is NaN, so the first evaluation is not finite (explicit start points are refused unless finite)."""
    tg = case["target"]
    if tg == "swap":
        T = mr.SWAP.copy()
    elif tg == "haar":
        T = o.haar_unitary(5000 + int(t))
    else:
        T = o.canonical_matrix(*[float(v) for v in tg[1:]])
    if case.get("nan_target"):
        T[0, 0] = np.nan
    return T


def objective(case):
    k = int(case["k"])
    lg = {"basic": o.loss_and_grad, "square": o.square_loss_and_grad, "makhlin": mr.loss_and_grad}[case["cost"]]
    return bp.pinned_exterior(lg, k) if int(case["flags"]) & FLAG_NO_EXTERIOR else lg


def start_point(case, t, r):
    k = int(case["k"])
    x0 = o.x0_philox(3, int(t), int(r), k)
    if int(case["flags"]) & FLAG_NO_EXTERIOR:  # the kernel pins the parameters of layers 0 and k at zero
        x0[:6] = 0.0
        x0[6 * k:] = 0.0
    return x0


_HP_TOL = None


def bands(case):
    """(loss band, gradient band per component): twice the tolerance the evaluation kernels are held to for this cost -- that of the
    hp_ref group of the same gate and span (its general-position and near-solution inputs) where the fixture has one, the worst over
    the fixed-gate groups of that cost and kernel family (spans 1..5, spans 6..16) otherwise; never above twice hp.TOL_CAP."""
    global _HP_TOL
    if _HP_TOL is None:
        groups = hp.load_fixture()
        tol = hp.tolerances(groups)
        _HP_TOL = {}
        for (gi, ci, kind), v in tol.items():
            m = groups[gi]["meta"]
            if m["family"] in ("short", "long") and kind in ("general", "near_solution"):
                for key in ((m["costs"][ci], m["gate"], int(m["k"])), (m["costs"][ci], None, m["family"])):
                    _HP_TOL[key] = max(_HP_TOL.get(key, 0.0), v)
    cost = case["cost"]
    tol = _HP_TOL.get((cost, case.get("hp_gate"), int(case["k"])), _HP_TOL[(cost, None, "short" if int(case["k"]) <= 5 else "long")])
    b = 2.0 * min(tol, hp.TOL_CAP)
    return b, b


def tolerance(e_ref):
    return min(TOL_FACTOR * e_ref, TOL_CAP)


def load_fixture(path=FIXTURE):
    with open(path) as fh:
        return json.load(fh)


# ---- the replay ----------------------------------------------------------------------------------------------------------------
class _State:
    """What the port carries from one accepted step to the next."""

    __slots__ = ("H", "hs1", "scaled", "grow", "alpha", "p", "nstall", "flags")


def _first_alpha(grow, p):
    return min(grow, STEP_MAX / max(np.sqrt(p @ p), 1e-300))


def _line_search(ev, x, f, g, st, band_f, n):
    """The port's line search from x along st.p.  Returns (candidates, failed, nondescent, (H, hs1, p, g.p) after a non-descent
    reset if there was one): ``candidates`` are the trials the search
    may accept -- (alpha, number of back-tracks before it, unclear, margin) -- in the order it meets them: a clear acceptance ends the
    list, an acceptance inside the band is listed and the search goes on as if it had been refused.  ``failed``: the search can run
    out of back-tracks (always True after an unclear last candidate; the only outcome when ``candidates`` is empty)."""
    p = st.p
    gp = g @ p
    nondescent = not (gp < 0)
    H, hs1 = st.H, st.hs1
    if nondescent:
        H, hs1, p = np.eye(n, dtype=st.H.dtype), 0.0, -g
        gp = g @ p
    alpha = st.alpha
    cands = []
    nback = 0
    unclear_before = False
    while True:
        ft, _ = ev(x + alpha * p)
        if not np.isfinite(ft):
            ft = np.inf
        margin = ft - f - ARMIJO_C1 * alpha * gp
        unclear = abs(margin) <= band_f
        if margin <= 0 or unclear:
            cands.append((alpha, nback, unclear or unclear_before, margin))
            if not unclear:
                return cands, False, nondescent, (H, hs1, p, gp)
        unclear_before = unclear_before or unclear
        denom = 2.0 * (ft - f - gp * alpha)
        a_new = -gp * alpha * alpha / denom if denom > 0 and np.isfinite(denom) else 0.5 * alpha
        alpha = min(max(a_new, BACKTRACK_MIN * alpha), BACKTRACK_MAX * alpha)
        nback += 1
        if nback > MAX_BACKTRACK:
            return cands, True, nondescent, (H, hs1, p, gp)


def _advance(st, dirn, s, g, gt, it, nback, n, short, updated):
    """The port's update with the observed pair (s, y = gt - g) for one setting of the two branch decisions; returns the next state."""
    H, hs1, p, gp = dirn
    y = gt - g
    sy = s @ y
    sg = s @ gt
    nx = _State()
    nx.scaled, nx.nstall = st.scaled, st.nstall
    q = (H @ gt.astype(H.dtype)).astype(np.float64)
    first = False
    if updated:
        rho = 1.0 / sy
        fac = 1.0
        if not st.scaled:
            fac = sy / (y @ y)
            hs1 = fac - 1.0
            first = True
        nx.scaled = True
        q = q + hs1 * gt
        u = q + fac * p
        c = rho * (1.0 + rho * (y @ u))
        w = c * s - rho * u
        v = -rho * u
        H = H + np.outer(s.astype(H.dtype), w.astype(H.dtype)) + np.outer(v.astype(H.dtype), s.astype(H.dtype))
        pn = -(q + s * (w @ gt) + v * sg)
    else:
        pn = -(q + hs1 * gt)
    nx.H, nx.hs1, nx.p = H, hs1, pn
    grow = 1.0 if nback else st.grow  # a back-track ends the compounding
    nx.grow = min(grow * GROW_FACTOR, GROW_MAX) if short else 1.0
    nx.alpha = _first_alpha(nx.grow, pn)
    periodic = it % RESTART_PERIOD == 0
    if periodic:
        nx.H, nx.hs1, nx.scaled, nx.p = np.eye(n, dtype=H.dtype), 0.0, False, -gt
        nx.alpha = _first_alpha(nx.grow, nx.p)
    nx.flags = {"short": short, "updated": updated, "first_scaling": first, "periodic": periodic, "grow": nx.grow}
    return nx


def replay(lg, gate_seq, target, x0, xs_obs, band, h_dtype=np.float32, maxiter=2500, gtol=1e-9, stop_loss=1e-13, gtol_far=1e-5,
           far_loss=1e-6):
    """Replays the port along ``xs_obs`` (the observed points after every accepted step).  Returns a dict:

    ``dev`` [steps replayed], ``unclear`` [same], ``steps`` (per step: n_back, short, updated, first_scaling, nondescent, periodic,
    grow), ``f`` (the oracle's loss at x0 and at every observed point replayed), ``noise_from`` (index of the first noise-floor step,
    or None), ``item_unclear``, and the port's prediction ``iters``, ``evals``, ``status`` (None from the noise floor on), ``end``.
    """
    band_f, band_g = band
    n = len(x0)
    ev = lambda xx: lg(xx, gate_seq, target)  # noqa: E731
    x = np.array(x0, dtype=np.float64)
    xs_obs = np.asarray(xs_obs, dtype=np.float64).reshape(-1, n)
    out = {"dev": [], "unclear": [], "steps": [], "f": [], "noise_from": None, "item_unclear": False, "iters": None, "evals": None,
           "status": None, "end": None}
    f, g = ev(x)
    out["f"].append(f)
    nev = 1

    def finish(it, status, end):
        out["iters"], out["evals"], out["status"], out["end"] = it, nev, status, end
        return out

    if not np.isfinite(f):
        return finish(0, ST_NONFINITE, bp.END_NONFINITE)

    def termination(f, gnorm):
        """(converged, unclear, criterion)"""
        conv = f < stop_loss or gnorm < gtol or (gnorm < gtol_far and f > far_loss)
        crit = bp.END_STOP_LOSS if f < stop_loss else bp.END_GTOL if gnorm < gtol else bp.END_FAR
        lo = (f - band_f < stop_loss) or (gnorm - band_g < gtol) or (gnorm - band_g < gtol_far and f + band_f > far_loss)
        hi = (f + band_f < stop_loss) or (gnorm + band_g < gtol) or (gnorm + band_g < gtol_far and f - band_f > far_loss)
        return conv, lo != hi, crit

    st = _State()
    st.H, st.hs1, st.scaled, st.grow, st.nstall, st.flags = np.eye(n, dtype=h_dtype), 0.0, False, 1.0, 0, {}
    st.p = -(st.H @ g.astype(h_dtype)).astype(np.float64)
    st.alpha = _first_alpha(1.0, st.p)
    states = [st]
    n_obs = len(xs_obs)
    conv, unc, crit = termination(f, np.abs(g).max())
    if unc:
        out["item_unclear"] = True
        conv = n_obs == 0
    if conv:
        return finish(0, ST_CONVERGED, crit)
    if maxiter <= 0:
        return finish(0, ST_MAXITER, bp.END_MAXITER)

    it = 0
    while True:
        # ---- the port's line search from x, for every branch an unclear decision of the previous step left open
        searches = [_line_search(ev, x, f, g, s_, band_f, n) for s_ in states]
        if it == n_obs:
            # the observed run ended here without a termination criterion of an accepted step: the trailing failed trials
            best = None
            for s_, (cands, failed, _, _) in zip(states, searches):
                if failed and (best is None or not cands):
                    best = (s_, cands)
            if best is None:
                # the port accepts another step (clearly, in every open branch): it predicts a longer run
                cands = searches[0][0]
                nev += cands[-1][1] + 1
                return finish(it + 1, None, None)
            if best[1] or len(states) > 1:
                out["item_unclear"] = True
            nev += MAX_BACKTRACK + 1
            gnorm = np.abs(g).max()
            if abs(gnorm - STALL_GNORM) <= band_g:
                out["item_unclear"] = True
            return finish(it, ST_STALLED if gnorm < STALL_GNORM else ST_LINESEARCH, bp.END_BACKTRACK)
        s_obs = xs_obs[it] - x
        pick = None
        for si, (cands, failed, nondescent, dirn) in enumerate(searches):
            for (alpha, nback, unclear, margin) in cands:
                s_pred = alpha * dirn[2]
                dev = np.linalg.norm(s_obs - s_pred) / np.linalg.norm(s_pred)
                if pick is None or dev < pick[0]:
                    pick = (dev, si, alpha, nback, unclear, nondescent, dirn)
        if pick is None:
            # no trial the port could accept, in any branch: it predicts the end of the run here
            nev += MAX_BACKTRACK + 1
            gnorm = np.abs(g).max()
            return finish(it, ST_STALLED if gnorm < STALL_GNORM else ST_LINESEARCH, bp.END_BACKTRACK)
        dev, si, alpha, nback, unclear, nondescent, dirn = pick
        st = states[si]
        step_unclear = unclear or len(states) > 1
        nev += nback + 1
        # ---- adopt the observed point
        xt = xs_obs[it].copy()
        ft, gt = ev(xt)
        if not np.isfinite(ft) or f - ft < band_f:
            # noise floor (or a non-finite accepted point, which no tolerance admits: the caller's loss check reports it)
            out["noise_from"] = it
            out["item_unclear"] = True
            out["f"].append(ft)
            return out
        it += 1
        out["dev"].append(dev)
        out["f"].append(ft)
        y = gt - g
        sy = s_obs @ y
        ss = s_obs @ s_obs
        s1 = np.abs(s_obs).sum()
        thr_short = (1.0 - WOLFE_C2) * -(s_obs @ g)
        short = sy < thr_short
        short_unclear = abs(sy - thr_short) <= 1.3 * s1 * band_g
        thr_curv = CURV_EPS * np.sqrt(ss * (y @ y))
        curv = sy > thr_curv
        curv_unclear = abs(sy - thr_curv) <= s1 * band_g
        st.nstall = st.nstall + 1 if (f - ft) <= STALL_DF else 0  # (never counts: such a step is a noise-floor step)
        branches = [(short, (not short) and curv)]
        if short_unclear:
            branches.append((not short, short and curv))
        if curv_unclear and (not short or short_unclear):
            branches.append((False, not curv))
        branches = list(dict.fromkeys(b for b in branches if not (b[1] and not sy > 0)))
        if len(branches) > 1:
            step_unclear = True
        states = [_advance(st, dirn, s_obs, g, gt, it, nback, n, sh, up) for sh, up in branches]
        fl = dict(states[0].flags)
        fl.update(n_back=nback, nondescent=nondescent)
        out["steps"].append(fl)
        out["unclear"].append(bool(step_unclear))
        if step_unclear:
            out["item_unclear"] = True
        x, f, g = xt, ft, gt
        conv, unc, crit = termination(f, np.abs(g).max())
        if unc:
            out["item_unclear"] = True
            conv = it == n_obs
        if conv or st.nstall >= 2 or it >= maxiter:
            out["steps"][-1]["periodic"] = False  # (the run ends before the restart)
        if conv:
            return finish(it, ST_CONVERGED, crit)
        if st.nstall >= 2:
            return finish(it, ST_STALLED, bp.END_STALL)
        if it >= maxiter:
            return finish(it, ST_MAXITER, bp.END_MAXITER)


def census(results):
    """Branch counts over a list of replay results."""
    c = {"steps": 0, "unclear": 0, "backtracks": 0, "short": 0, "skipped": 0, "first_scaling": 0, "nondescent": 0, "periodic": 0,
         "max_grow": 1.0, "items_unclear": 0, "max_iters": 0}
    for r in results:
        c["steps"] += len(r["dev"])
        c["unclear"] += int(sum(r["unclear"]))
        c["items_unclear"] += int(r["item_unclear"])
        c["max_iters"] = max(c["max_iters"], len(r["dev"]))
        for s in r["steps"]:
            c["backtracks"] += s["n_back"]
            c["short"] += int(s["short"])
            c["skipped"] += int(not s["updated"])
            c["first_scaling"] += int(s["first_scaling"])
            c["nondescent"] += int(s["nondescent"])
            c["periodic"] += int(s["periodic"])
            c["max_grow"] = max(c["max_grow"], float(s["grow"]))
    return c


def worst_clear(results):
    return max([d for r in results for d, u in zip(r["dev"], r["unclear"]) if not u], default=0.0)


def run_port(case, t, r, h_dtype=np.float32):
    """The port on one item of a case: (loss, x, iters, status, evals, xs, record)."""
    k = int(case["k"])
    gates = [gate_matrix(case["gate"])] * k
    xs, rec = [], []
    prm = dict(DEFAULTS, maxiter=int(case["maxiter"]))
    f, x, it, st, nev = bp.minimize_port(start_point(case, t, r), gates, target_matrix(case, t), h_dtype=h_dtype, loss_and_grad=objective(case),
                                         xs=xs, record=rec, **prm)
    return f, x, it, st, nev, xs, rec


def replay_item(case, t, r, xs_obs, h_dtype=np.float32):
    k = int(case["k"])
    gates = [gate_matrix(case["gate"])] * k
    prm = dict(DEFAULTS, maxiter=int(case["maxiter"]))
    return replay(objective(case), gates, target_matrix(case, t), start_point(case, t, r), xs_obs, bands(case), h_dtype=h_dtype, **prm)
