"""The cases of the three-qubit optimizer replay (tests/test_q3_replay_host.py, tests/test_gpu_q3_replay.py): templates, targets and
start points by name and seed, built from tests/q3_cases.py and tests/q3m_cases.py, and the objective of each as the
``(x, gates, target) -> (f, g)`` callable oracle/bfgs_port.minimize_port and tests/bfgs_replay.replay take.

A case of tests/golden/q3_replay_cases.json (tools/make_q3_replay_cases.py):

    {"name", "template": [kind, ...], "cost": "basic" | "square", "maxiter", "items": [[target spec, start spec], ...],
     "port": [[iters, evals, status, end], ...]}                       (+ "nan_target": true)

Templates (``template``): ["parity", k] -- q3_cases.parity_case(k), two-qubit positions only; ["line3"] -- sqrt(iSWAP) on
q3_cases.LINE_EDGES; ["toffoli"] -- six CX on q3_cases.TOFFOLI_EDGES; ["vswap"], ["ccz_cx"], ["ten3"] -- q3m_cases.vswap_case(),
ccz_cx_case(), parity_template("ten3") (``MIXED = true``).

Targets: ["parity", m] -- target m of parity_case(k); ["reachable", t] -- q3_cases.reachable_targets()[t]; ["ccx"]; ["local", i] --
target i of the module's local_cases(); ["ccz_cx", t] -- q3m_cases.ccz_cx_targets()[t]; ["items", m] -- q3m_cases.parity_items(name)
target m; ["own"] -- the template's unitary at the start point itself.
Start points: ["parity", m] -- row m of parity_case(k); ["local", i]; ["items", m]; ["uniform", seed] --
default_rng(seed).uniform(0, 2 pi, n).
"""
from __future__ import annotations

import functools
import json
import math
import os

import numpy as np

import q3_cases
import q3_ref
import q3m_cases
import q3m_ref
from oracle import bfgs_port as bp

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "q3_replay_cases.json")
GROUPS = ("small", "toffoli", "cap", "mixed", "other")
DEFAULTS = dict(gtol=1e-9, stop_loss=1e-13, gtol_far=1e-5, far_loss=1e-6)
OVERLAP_FLOOR = 0.05  # |Tr(T^+ W)| / 8 under which the evaluation kernels' parity bounds were not measured (BasicCost's gradient is singular at 0)
# the parity tests' bounds on the loss and on a gradient component (test_gpu_q3.py, test_gpu_q3m.py), by template family
LOSS_BOUND = {False: 3.4e-15, True: 6.8e-15}
GRAD_BOUND = {False: 4.8e-15, True: 9.6e-15}


class Template:
    """A template for the device call and for the model."""

    def __init__(self, spec):
        kind = spec[0]
        self.spec = list(spec)
        if kind in ("parity", "line3", "toffoli"):
            self.mixed = False
            if kind == "parity":
                gates, gate_index, edges, _, _ = q3_cases.parity_case(int(spec[1]))
            elif kind == "line3":
                gates, gate_index, edges = q3_cases.SQISWAP[None], [0] * 3, q3_cases.LINE_EDGES
            else:
                gates, gate_index, edges = q3_cases.CX[None], [0] * 6, q3_cases.TOFFOLI_EDGES
            self.table, self.gate_index, self.edges = gates, list(gate_index), [tuple(e) for e in edges]
            self.model_gates = [gates[i] for i in gate_index]
            self.n = 9 + 6 * len(edges)
            self.ref = q3_ref
        else:
            self.mixed = True
            self.case = {"vswap": q3m_cases.vswap_case, "ccz_cx": q3m_cases.ccz_cx_case,
                         "ten3": lambda: q3m_cases.parity_template("ten3")}[kind]()
            self.model_gates, self.edges, self.n = self.case.model_gates, self.case.edges, self.case.n
            self.ref = q3m_ref

    def unitary(self, x):
        return self.ref.unitary(x, self.model_gates, self.edges)

    def objective(self, square):
        """``lg(x, gates, target)`` of the port and the replay: the model's loss and gradient."""
        def lg(x, gates, target):
            f, g, _ = self.ref.loss_grad(x, gates, self.edges, target, square)
            return f, g
        return lg

    def minimize(self, ctx, targets, prm, x0, cost_kind):
        if self.mixed:
            return ctx.q3m_minimize(*self.case.description(), targets, prm, 1e-10, cost_kind=cost_kind, x0=x0)
        return ctx.q3_minimize(self.table, self.gate_index, self.edges, targets, prm, 1e-10, cost_kind=cost_kind, x0=x0)


@functools.lru_cache(maxsize=None)
def _template(spec):
    return Template(spec)


def template(case):
    return _template(tuple(case["template"]))


def start_point(case, item):
    tp = template(case)
    kind, arg = item[1]
    if kind == "parity":
        return q3_cases.parity_case(int(case["template"][1]))[4][int(arg)].copy()
    if kind == "local":
        return (q3m_cases if tp.mixed else q3_cases).local_cases()[1][int(arg)].copy()
    if kind == "items":
        return q3m_cases.parity_items(case["template"][0])[1][int(arg)].copy()
    if kind == "uniform":
        return np.random.default_rng(int(arg)).uniform(0.0, 2.0 * math.pi, tp.n)
    raise ValueError(item)


def target_matrix(case, item):
    tp = template(case)
    spec = item[0]
    kind = spec[0]
    if kind == "parity":
        t = q3_cases.parity_case(int(case["template"][1]))[3][int(spec[1])]
    elif kind == "reachable":
        t = q3_cases.reachable_targets()[int(spec[1])]
    elif kind == "ccx":
        t = q3_ref.CCX
    elif kind == "local":
        t = (q3m_cases if tp.mixed else q3_cases).local_cases()[0][int(spec[1])]
    elif kind == "ccz_cx":
        t = q3m_cases.ccz_cx_targets()[int(spec[1])]
    elif kind == "items":
        t = q3m_cases.parity_items(case["template"][0])[0][int(spec[1])]
    elif kind == "own":
        t = tp.unitary(start_point(case, item))
    else:
        raise ValueError(item)
    t = np.array(t, dtype=np.complex128)
    if case.get("nan_target"):
        t[0, 0] = np.nan  # the first evaluation is not finite (an explicit start point that is not finite is refused)
    return t


def objective(case):
    return template(case).objective(case["cost"] == "square")


def bands(case):
    """(loss band, gradient band): twice the parity tests' bounds -- two evaluations enter every comparison."""
    m = template(case).mixed
    return 2.0 * LOSS_BOUND[m], 2.0 * GRAD_BOUND[m]


def loss_bound(case):
    return LOSS_BOUND[template(case).mixed]


def params(case):
    return dict(DEFAULTS, maxiter=int(case["maxiter"]))


_PORT_RUNS = {}


def port_run(case, item):
    """``run_port`` with the defaults, once per (case, item): the generator and the host tests share the runs.  Read only."""
    key = json.dumps([case["template"], case["cost"], case["maxiter"], bool(case.get("nan_target")), item])
    if key not in _PORT_RUNS:
        _PORT_RUNS[key] = run_port(case, item)
    return _PORT_RUNS[key]


def run_port(case, item, h_dtype=np.float32, maxiter=None):
    """The port on one item: (loss, x, iters, status, evals, xs, record)."""
    tp = template(case)
    xs, rec = [], []
    prm = params(case)
    if maxiter is not None:
        prm["maxiter"] = maxiter
    f, x, it, st, nev = bp.minimize_port(start_point(case, item), tp.model_gates, target_matrix(case, item), h_dtype=h_dtype,
                                         loss_and_grad=objective(case), xs=xs, record=rec, **prm)
    return f, x, it, st, nev, xs, rec


def replay_item(case, item, xs_obs, h_dtype=np.float32):
    import bfgs_replay as br

    tp = template(case)
    return br.replay(objective(case), tp.model_gates, target_matrix(case, item), start_point(case, item), xs_obs, bands(case),
                     h_dtype=h_dtype, **params(case))


def load_fixture(path=FIXTURE):
    with open(path) as fh:
        return json.load(fh)
