"""CPU: how ``_ffi.Context`` marshals its six stage calls and three evaluations, pinned against a stub library (no ``libslamhip.so``).

Per call: the C symbol, the position and value of every scalar, which pointers are NULL, that contiguous inputs go through without a copy,
that every output pointer is the array returned under its documented key, and the keys / shapes / dtypes of what comes back --
asymmetries included: ``minimize_stage(want_items=False)`` leaves the ``item_*`` keys out while the V2 / smush form keeps them as
``None``, the trace forms have no ``item_evals``, and the V2 / smush trace call passes NULL where ``x0`` would go."""
import ctypes as C
import itertools

import numpy as np
import pytest

from slam_decomposition_amd import _ffi

N_TARGETS, V2_QN, SMUSH_QN, R, CAP = 5, 2, 3, 3, 7
SEQ = [0, 1, 0]
K = len(SEQ)


class StubLib:
    """Every attribute is a C function that records ``(name, args)`` -- with the gate sequence read while it is alive -- and returns 0."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def fn(*args):
            seq = np.ctypeslib.as_array((C.c_int32 * args[1]).from_address(args[2].value)).tolist()
            self.calls.append((name, args, seq))
            return 0

        return fn


def make_ctx():
    ctx = _ffi.Context.__new__(_ffi.Context)
    ctx._h = C.c_void_p()
    ctx._lib = StubLib()
    ctx.n_targets, ctx.v2_qn, ctx.smush_qn = N_TARGETS, V2_QN, SMUSH_QN
    return ctx


def same_array(arg, array):
    return (arg is None and array is None) or (arg is not None and array is not None and arg.value == array.ctypes.data)


STAGE_KEYS = ["best_loss", "best_x", "best_restart", "item_loss", "item_iters", "item_status"]


def expected_outputs(na, n, trace):
    shapes = {"best_loss": ((na,), np.float64), "best_x": ((na, n), np.float64), "best_restart": ((na,), np.int32),
              "item_loss": ((na, R), np.float64), "item_iters": ((na, R), np.int32), "item_status": ((na, R), np.int32)}
    if trace:
        shapes.update(trace_loss=((na, R, CAP), np.float64), trace_x=((na, R, CAP, n), np.float64))
    else:
        shapes["item_evals"] = ((na, R), np.int32)
    return shapes


# method -> (C symbol, parameters per gate, has the four per-parameter vectors, is a trace call)
STAGES = {
    "minimize_stage": ("slam_minimize_stage", 0, False, False),
    "minimize_stage_trace": ("slam_minimize_stage_trace", 0, False, True),
    "v2_minimize_stage": ("slam_v2_minimize_stage", V2_QN, True, False),
    "v2_minimize_stage_trace": ("slam_v2_minimize_stage_trace", V2_QN, True, True),
    "smush_minimize_stage": ("slam_smush_minimize_stage", SMUSH_QN, True, False),
    "smush_minimize_stage_trace": ("slam_smush_minimize_stage_trace", SMUSH_QN, True, True),
}


def _stage_cases():
    """Every method crossed with the arguments it has: active, x0 (not the V2 / smush trace forms), bounds (V2 / smush), want_items
    (not the trace forms)."""
    for method, (_, _, vectors, trace) in sorted(STAGES.items()):
        for with_active, with_x0, with_bounds, want_items in itertools.product([False, True], repeat=4):
            if not ((with_x0 and vectors and trace) or (with_bounds and not vectors) or (not want_items and trace)):
                yield method, with_active, with_x0, with_bounds, want_items


@pytest.mark.parametrize("method,with_active,with_x0,with_bounds,want_items", list(_stage_cases()))
def test_stage_call(method, with_active, with_x0, with_bounds, want_items):
    symbol, qn, vectors, trace = STAGES[method]
    takes_x0 = not (vectors and trace)
    ctx = make_ctx()
    n = 6 * (K + 1) + qn * K
    active = np.array([4, 1], dtype=np.int32) if with_active else None
    na = 2 if with_active else N_TARGETS
    x0 = np.arange(na * R * n, dtype=np.float64).reshape(na, R, n) if with_x0 else None
    lo, hi = np.full(n, -1.0), np.full(n, 2.0)
    blo, bhi = (np.full(n, -3.0), np.full(n, 4.0)) if with_bounds else (None, None)
    prm = _ffi.OptParams(restarts=R)
    positional = [SEQ, prm] + ([1e-9] if (vectors or trace) else []) + ([CAP] if trace else []) + ([lo, hi, blo, bhi] if vectors else [])
    kw = {"active": active}
    if takes_x0:
        kw["x0"] = x0
    if not trace:
        kw["want_items"] = want_items
    out = getattr(ctx, method)(*positional, **kw)

    (name, args, seq), = ctx._lib.calls
    assert name == symbol and seq == SEQ
    assert args[0] is ctx._h and args[1] == K and args[2] is not None and args[4] == na
    assert same_array(args[3], active) and same_array(args[5], x0)  # (contiguous inputs of the right type are not copied)
    i = 6
    if vectors:
        for arg, v in zip(args[6:10], (lo, hi, blo, bhi)):
            assert same_array(arg, v)
        i = 10
    assert args[i]._obj is prm
    i += 1
    if vectors or trace:
        assert args[i] == 1e-9 and isinstance(args[i], float)
        i += 1
    if trace:
        assert args[i] == CAP and isinstance(args[i], int)
        i += 1
    want = expected_outputs(na, n, trace)
    order = STAGE_KEYS + (["trace_loss", "trace_x"] if trace else ["item_evals"])
    assert len(args) == i + len(order)
    for arg, key in zip(args[i:], order):
        assert same_array(arg, out.get(key)), key
    if want_items:
        assert sorted(out) == sorted(want)
    elif vectors:
        assert sorted(out) == sorted(want) and all(out[key] is None for key in order[3:])
    else:
        assert sorted(out) == sorted(order[:3])
    for key, (shape, dtype) in want.items():
        if out.get(key) is not None:
            assert out[key].shape == shape and out[key].dtype == dtype and out[key].flags.c_contiguous, key


def test_stage_inputs_of_another_type_are_converted():
    ctx = make_ctx()
    ctx.minimize_stage(SEQ, _ffi.OptParams(restarts=R), active=[4, 1], x0=np.zeros((2, R, 24), dtype=np.float32))
    (_, args, _), = ctx._lib.calls
    assert args[3] is not None and args[4] == 2 and args[5] is not None


@pytest.mark.parametrize("method", sorted(STAGES))
def test_stage_shape_errors(method):
    symbol, qn, vectors, trace = STAGES[method]
    ctx = make_ctx()
    n = 6 * (K + 1) + qn * K
    prm = _ffi.OptParams(restarts=R)
    head = [SEQ, prm] + ([1e-9] if (vectors or trace) else []) + ([CAP] if trace else [])
    if vectors:
        with pytest.raises(ValueError) as err:
            getattr(ctx, method)(*head, np.zeros(n), np.zeros(n + 1))
        assert str(err.value) == f"per-parameter arrays must have shape [{n}]"
        head += [np.zeros(n), np.zeros(n)]
    if not (vectors and trace):
        with pytest.raises(ValueError) as err:
            getattr(ctx, method)(*head, x0=np.zeros((N_TARGETS, R, n + 1)))
        assert str(err.value) == f"x0 must have shape [{N_TARGETS}, {R}, {n}]"
        with pytest.raises(ValueError) as err:
            getattr(ctx, method)(*head, active=np.array([0, 2, 3]), x0=np.zeros((2, R, n)))
        assert str(err.value) == f"x0 must have shape [3, {R}, {n}]"
    assert ctx._lib.calls == []


EVALS = {"v2_eval": ("slam_v2_eval_loss_grad", V2_QN), "smush_eval": ("slam_smush_eval_loss_grad", SMUSH_QN)}


@pytest.mark.parametrize("method", sorted(EVALS))
@pytest.mark.parametrize("with_targets,want_grad,want_unitary", list(itertools.product([False, True], repeat=3)))
def test_v2_like_eval_call(method, with_targets, want_grad, want_unitary):
    symbol, qn = EVALS[method]
    ctx = make_ctx()
    n, M = 6 * (K + 1) + qn * K, 4
    x = np.arange(M * n, dtype=np.float64).reshape(M, n)
    tof = np.array([3, 0, 0, 2], dtype=np.int32) if with_targets else None
    loss, grad, w = getattr(ctx, method)(SEQ, x, tof, want_grad=want_grad, want_unitary=want_unitary)
    (name, args, seq), = ctx._lib.calls
    assert name == symbol and seq == SEQ and len(args) == 9
    assert args[0] is ctx._h and args[1] == K and same_array(args[3], x) and args[5] == M
    if with_targets:
        assert same_array(args[4], tof)
    else:
        assert args[4] is not None  # (zeros: every row against target 0)
    assert same_array(args[6], loss) and loss.shape == (M,) and loss.dtype == np.float64
    assert same_array(args[7], grad) and (grad is None) == (not want_grad)
    if want_grad:
        assert grad.shape == (M, n) and grad.dtype == np.float64
    assert (args[8] is None) == (w is None) == (not want_unitary)
    if want_unitary:
        assert w.shape == (M, 4, 4) and w.dtype == np.complex128 and args[8].value == w.ctypes.data
    with pytest.raises(ValueError) as err:
        getattr(ctx, method)(SEQ, np.zeros((M, n + 1)))
    assert str(err.value) == f"x must have shape [M, {n}]"


@pytest.mark.parametrize("want_grad", [False, True])
def test_eval_loss_grad_call(want_grad):
    ctx = make_ctx()
    n, M = 6 * (K + 1), 4
    x = np.zeros((M, n))
    tof = np.array([3, 0, 0, 2], dtype=np.int32)
    loss, grad = ctx.eval_loss_grad(SEQ, x, tof, want_grad=want_grad)
    (name, args, seq), = ctx._lib.calls
    assert name == "slam_eval_loss_grad" and seq == SEQ and len(args) == 8
    assert args[0] is ctx._h and args[1] == K and same_array(args[3], x) and same_array(args[4], tof) and args[5] == M
    assert same_array(args[6], loss) and same_array(args[7], grad) and (grad is None) == (not want_grad)
    assert loss.shape == (M,) and (grad is None or grad.shape == (M, n))
    with pytest.raises(ValueError) as err:
        ctx.eval_loss_grad(SEQ, np.zeros((M, n + 1)), tof)
    assert str(err.value) == f"x must have shape [M, {n}]"
    with pytest.raises(ValueError) as err:
        ctx.eval_loss_grad(SEQ, x, tof[:3])
    assert str(err.value) == "target_of must have shape [M]"


def test_opt_params_carry_every_field():
    prm = _ffi.OptParams(restarts=3, maxiter=70, gtol=1e-7, stop_loss=1e-11, seed=2**64 + 5, flags=9, gtol_far=1e-4, far_loss=1e-5,
                         items_per_quad=2, target_base=2**40)
    assert [getattr(prm, name) for name, _ in prm._fields_] == [3, 70, 1e-7, 1e-11, 5, 9, 2, 1e-4, 1e-5, 2**40]
