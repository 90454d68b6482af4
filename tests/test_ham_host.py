"""CPU: the Hamiltonian templates' host side -- slam_decomposition_amd/hamiltonian.py, the host model tests/ham_ref.py (against
scipy.linalg.expm, mpmath at 40 digits and central differences), the C ABI's refusals (no context needed) and the bookkeeping of
``TemplateOptimizer._run_batch_ham`` on the recording stand-in of tests/fake_ctx.py.  tests/test_gpu_ham.py holds the GPU side."""
import ctypes as C
import math

import numpy as np
import pytest

import fake_ctx
import ham_cases
import ham_ref
from slam_decomposition_amd import _ffi, gates
from slam_decomposition_amd import hamiltonian as hm
from slam_decomposition_amd.basis import HamiltonianTemplate
from slam_decomposition_amd.cost_function import BasicCost, MakhlinFunctionalCost, MutualInformation, SquareCost
from slam_decomposition_amd.optimizer import TemplateOptimizer

EPS = np.finfo(np.float64).eps
INVALID, UNSUPPORTED = -1, -3


def _scale(terms, x):
    """max(1, |t| ||H||_2): what the rounding error of exp(-i t H) from an eigen-decomposition is proportional to"""
    return max(1.0, abs(ham_ref.time_of(terms, x)) * np.linalg.norm(ham_ref.hamiltonian(terms, x), 2))


@pytest.mark.parametrize("name", ham_cases.DEVICE_HAMILTONIANS)
def test_model_against_scipy_expm(name):
    from scipy.linalg import expm

    terms, targets, x, tof = ham_cases.parity_items(name)
    loss, _, u = ham_cases.parity_reference(name, False)
    d = terms["dim"]
    for m in range(len(x)):
        ref = expm(-1j * ham_ref.time_of(terms, x[m]) * ham_ref.hamiltonian(terms, x[m]))
        # (SciPy's Pade approximant itself is good to a few ulp times the norm; the eigen-decomposition likewise)
        assert np.max(np.abs(u[m] - ref)) < 64 * EPS * _scale(terms, x[m])
        assert abs(loss[m] - (1.0 - abs(np.trace(targets[tof[m]].conj().T @ ref)) / d)) < 64 * EPS * _scale(terms, x[m])


@pytest.mark.parametrize("name", ham_cases.DEVICE_HAMILTONIANS)
def test_model_against_mpmath_at_40_digits(name):
    """The model's own error on the evaluation cases of the GPU test, so that the GPU bounds are not limited by it: at most
    32 eps max(1, |t| ||H||) in the unitary and in the loss (measured: 5.0e-15 in U, 2.4e-15 in the loss, both on the delta Hamiltonian)."""
    import mpmath

    terms, targets, x, tof = ham_cases.parity_items(name)
    loss, _, u = ham_cases.parity_reference(name, False)
    d = terms["dim"]
    worst_u = worst_l = 0.0
    with mpmath.workdps(40):
        for m in range(len(x)):
            h = ham_ref.hamiltonian(terms, x[m])
            ref = mpmath.expm(mpmath.matrix(h.tolist()) * mpmath.mpc(0, -ham_ref.time_of(terms, x[m])))
            ref = np.array([[complex(ref[i, j]) for j in range(d)] for i in range(d)])
            e_u = np.max(np.abs(u[m] - ref))
            e_l = abs(loss[m] - (1.0 - abs(np.trace(targets[tof[m]].conj().T @ ref)) / d))
            worst_u, worst_l = max(worst_u, e_u), max(worst_l, e_l)
            assert e_u < 32 * EPS * _scale(terms, x[m]) and e_l < 32 * EPS * _scale(terms, x[m]), (m, e_u, e_l)
    print(f"model vs mpmath {name}: U {worst_u:.3e} loss {worst_l:.3e}")


@pytest.mark.parametrize("square", [False, True], ids=["basic", "square"])
@pytest.mark.parametrize("name", ham_cases.DEVICE_HAMILTONIANS)
def test_model_gradient_against_central_differences(name, square):
    """Step 1e-6: truncation h^2 |f'''| / 6 with |f'''| <= (|t| ||dH||)^3 of order 1e3 at the 2 pi rows gives 2e-10, rounding eps / h
    1e-10: the bound is 1e-8."""
    terms, targets, x, tof = ham_cases.parity_items(name)
    _, grad, _ = ham_cases.parity_reference(name, square)
    n = terms["n_params"]
    for m in range(0, len(x), 3):
        fd = np.zeros(n)
        for j in range(n):
            e = np.zeros(n)
            e[j] = 1e-6
            fd[j] = (ham_ref.loss_grad(terms, x[m] + e, targets[tof[m]], square)[0] - ham_ref.loss_grad(terms, x[m] - e, targets[tof[m]], square)[0]) / 2e-6
        assert np.max(np.abs(fd - grad[m])) < 1e-8, (m, fd, grad[m])


def test_circulator_reproduces_the_gate_classes():
    h = hm.CirculatorHamiltonian()
    for gate in (gates.VSwap(), gates.DeltaSwap()):
        assert np.array_equal(h.construct_U(*[float(p) for p in gate.params]), gate.to_matrix())
    args = (0.3, -1.2, 2.0, 0.7, 1.1, 0.2)
    assert np.array_equal(h.H(*args), gates.circulator_hamiltonian(*args))  # bit for bit: it IS that function


def test_argument_counts_and_dimensions():
    want = {"snail": (1, 4), "conversion_gain": (2, 4), "conversion_gain_phase": (5, 4), "circulator": (7, 8), "delta": (12, 8)}
    for name, (n, d) in want.items():
        h = ham_cases.hamiltonian(name)
        assert (h.n_params, h.dim) == (n, d) and len(h.parameter_names) == n
        t = HamiltonianTemplate(h)
        assert t.n_qubits == {4: 2, 8: 3}[d] and list(t.get_spanning_range(None)) == [1] and len(t.parameter_guess()) == n
    assert ham_cases.hamiltonian("circulator").parameter_names[-1] == "t" and ham_cases.hamiltonian("conversion_gain_phase").parameter_names[-1] == "t"
    assert ham_cases.hamiltonian("delta").device_terms()["t_index"] == -1


@pytest.mark.parametrize("name", ham_cases.DEVICE_HAMILTONIANS)
def test_device_terms_reassemble_h_exactly(name):
    h = ham_cases.hamiltonian(name)
    terms = h.device_terms()
    assert len(terms["matrices"]) <= hm.MAX_TERMS and terms["n_params"] <= hm.MAX_PARAMS
    rng = np.random.default_rng(3)
    for _ in range(4):
        x = rng.uniform(-3.0, 3.0, terms["n_params"])
        # construct_U hands its arguments to H in order; the time, where it is one, is the last and not H's
        h_args = x[:-1] if terms["t_index"] >= 0 else x
        assert np.array_equal(hm.assemble(terms, x), h.H(*h_args))
        assert np.max(np.abs(ham_ref.hamiltonian(terms, x) - h.H(*h_args))) < 4 * EPS * 3.0
        assert np.array_equal(HamiltonianTemplate(h).eval(x), h.construct_U(*x))


def test_delta_literal_phase_wiring():
    """hamiltonian.py:287-300 as written: cphi_ab (argument 6) is unused, its gradient is exactly 0; cphi_ac (argument 7) feeds the a-b
    and the a-c conversion terms, and its gradient is the sum of the two terms' contributions."""
    terms, targets, x, tof = ham_cases.parity_items("delta")
    _, grad, _ = ham_cases.parity_reference("delta", True)
    assert np.all(grad[:, 6] == 0.0) and np.any(grad[:, 7] != 0.0)
    split = dict(terms, n_params=13, phi_index=terms["phi_index"].copy())
    assert list(terms["phi_index"][[0, 2]]) == [7, 7]
    split["phi_index"][0] = 12  # the a-b conversion term on a phase of its own
    for m in range(0, len(x), 5):
        g13 = ham_ref.loss_grad(split, np.append(x[m], x[m][7]), targets[tof[m]], True)[1]
        assert abs(g13[7] + g13[12] - grad[m, 7]) < 16 * EPS * max(1.0, np.max(np.abs(g13)))
        assert np.max(np.abs(np.delete(g13[:12], 7) - np.delete(grad[m], 7))) < 16 * EPS * max(1.0, np.max(np.abs(g13)))


def test_host_only_hamiltonians_have_no_device_description():
    for cls, word in ((hm.FSimHamiltonian, "eta"), (hm.ConversionGainSmush, "time slices"), (hm.ConversionGainSmush1QPhase, "time slices")):
        with pytest.raises(NotImplementedError, match=word):
            cls().device_terms()
        with pytest.raises(NotImplementedError):
            HamiltonianTemplate(cls())
    u = hm.FSimHamiltonian.construct_U(0.4, 2.0)
    assert np.max(np.abs(u @ u.conj().T - np.eye(4))) < 8 * EPS
    one = hm.ConversionGainSmush.construct_U(0.1, 0.2, 0.5, 0.3, [0.0], [0.0])
    assert np.max(np.abs(one - hm.ConversionGainPhaseHamiltonian.construct_U(0.1, 0.2, 0.5, 0.3, 1.0))) < 8 * EPS
    two = hm.ConversionGainSmush1QPhase.construct_U(0.0, 0.0, 0.1, 0.2, 0.5, 0.3, 0.0, 0.0, [0.2, 0.4], [0.1, 0.3])
    same = hm.ConversionGainSmush.construct_U(0.1, 0.2, 0.5, 0.3, [0.2, 0.4], [0.1, 0.3])
    assert np.max(np.abs(two - same)) < 8 * EPS


def test_optimizer_refusals():
    t = HamiltonianTemplate(hm.CirculatorHamiltonian())
    for objective in (MakhlinFunctionalCost(), MutualInformation()):
        with pytest.raises(NotImplementedError):
            TemplateOptimizer(t, objective)
    with pytest.raises(NotImplementedError):
        TemplateOptimizer(t, BasicCost(), use_callback=True)
    with pytest.raises(NotImplementedError):
        TemplateOptimizer(t, BasicCost(), override_method="Nelder-Mead")
    with pytest.raises(NotImplementedError):
        TemplateOptimizer(t, BasicCost(), devices=[0, 1])
    with pytest.raises(ValueError):
        HamiltonianTemplate(hm.CirculatorHamiltonian(), start_low=1.0, start_high=0.0)
    opt = TemplateOptimizer(t, SquareCost(), override_method="BFGS")
    with pytest.raises(ValueError, match="8x8"):
        opt.approximate_target_U(np.eye(4))


# ---- the C ABI: everything is checked before the context -----------------------------------------------------------------------------
def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _call(kind, **over):
    """slam_ham_eval / slam_ham_minimize with a NULL context on a good two-mode description, `over` replacing arguments."""
    lib = _ffi.load_library()
    a = dict(dim=4, n=2, k=2, mats=np.zeros((2, 4, 4, 2)), s=np.array([0, 1], np.int32), p=np.array([-1, -1], np.int32), t=-1,
             targets=np.zeros((1, 4, 4, 2)), nt=1, x=np.zeros((3, 2)), tof=np.zeros(3, np.int32), M=3, cost=0,
             prm=_ffi.OptParams(restarts=3, maxiter=10, gtol=1e-9, stop_loss=1e-13, seed=1, flags=0), x0=np.zeros((1, 3, 2)))
    a["mats"][0, 2, 1, 0] = a["mats"][1, 3, 0, 0] = 1.0
    a.update(over)
    head = (None, a["dim"], a["n"], a["k"], _ptr(a["mats"]), _ptr(a["s"]), _ptr(a["p"]), a["t"], _ptr(a["targets"]), a["nt"])
    if kind == "eval":
        loss = np.zeros(max(int(a["M"]), 1))
        rc = lib.slam_ham_eval(*head, _ptr(a["x"]), _ptr(a["tof"]), a["M"], a["cost"], _ptr(loss), None, None)
    else:
        rc = lib.slam_ham_minimize(*head, a["cost"], C.byref(a["prm"]), 1e-10, _ptr(a["x0"]), *([None] * 9))
    return rc, lib.slam_last_error().decode()


@pytest.mark.parametrize("kind", ["eval", "minimize"])
def test_abi_refusals_come_before_the_context(kind):
    rc, msg = _call(kind)
    assert rc == INVALID and "ctx is NULL" in msg, msg  # everything else is in order: the context is looked at last
    bad = np.zeros((2, 4, 4, 2))
    bad[0, 1, 1, 1] = np.nan
    many = np.zeros((3, 4, 4, 2))
    many[:, 2, 1, 0] = 1.0  # three terms on one entry
    nan_t = np.full((1, 4, 4, 2), np.inf)
    cases = [
        (dict(dim=5), INVALID, "dim"), (dict(dim=2), INVALID, "dim"),
        (dict(n=33), UNSUPPORTED, "32 parameters"), (dict(n=0), INVALID, "n_params"),
        (dict(k=17), UNSUPPORTED, "16 terms"), (dict(k=0), INVALID, "n_terms"),
        (dict(s=np.array([0, 2], np.int32)), INVALID, "s_index[1]"), (dict(s=np.array([-1, 0], np.int32)), INVALID, "s_index[0]"),
        (dict(p=np.array([-2, 0], np.int32)), INVALID, "phi_index[0]"), (dict(p=np.array([0, 2], np.int32)), INVALID, "phi_index[1]"),
        (dict(t=2), INVALID, "t_index"), (dict(t=-2), INVALID, "t_index"),
        (dict(mats=bad), INVALID, "matrices"),
        (dict(k=3, mats=many, s=np.zeros(3, np.int32), p=np.full(3, -1, np.int32)), UNSUPPORTED, "more than two contributions"),
        (dict(targets=nan_t), INVALID, "targets"), (dict(nt=0), INVALID, "targets"),
        (dict(cost=2), INVALID, "cost kind"), (dict(cost=3), INVALID, "cost kind"), (dict(cost=-1), INVALID, "cost kind"),
    ]
    if kind == "eval":
        cases += [(dict(tof=np.array([0, 1, 0], np.int32)), INVALID, "target_of[1]"), (dict(M=0), INVALID, "M must"),
                  (dict(x=np.full((3, 2), np.nan)), INVALID, "x: entry")]
    else:
        cases += [(dict(x0=None), INVALID, "x0 is required"), (dict(x0=np.full((1, 3, 2), np.inf)), INVALID, "x0[0]"),
                  (dict(x0=np.full((1, 3, 2), 2e8)), INVALID, "x0[0]"),
                  (dict(prm=_ffi.OptParams(restarts=0, maxiter=10, gtol=1e-9, stop_loss=1e-13, seed=1, flags=0)), INVALID, "restarts")]
    for over, code, word in cases:
        rc, msg = _call(kind, **over)
        assert rc == code and word in msg and "ctx is NULL" not in msg, (over.keys(), rc, msg)


# ---- TemplateOptimizer._run_batch_ham on the recording stand-in ----------------------------------------------------------------------
class _HamCtx(fake_ctx.FakeCtx):
    def ham_minimize(self, terms, targets, params, exit_loss, x0, cost_kind=0):
        self._rec("ham_minimize", dim=terms["dim"], n_params=terms["n_params"], targets=np.asarray(targets), params=params, exit_loss=exit_loss,
                  x0=np.asarray(x0), cost_kind=cost_kind)
        self._k = 1
        out = self._stage(terms["n_params"], params, exit_loss, np.arange(len(targets)), True)
        out["item_x"] = np.zeros(out["item_loss"].shape + (terms["n_params"],))
        out["kernel_ms"] = 0.25
        return out


def test_run_batch_ham_bookkeeping():
    low, high = ham_cases.search_range()
    opt = TemplateOptimizer(HamiltonianTemplate(hm.CirculatorHamiltonian(), low, high), SquareCost(), seed=11, training_restarts=4, override_fail=True)
    book = fake_ctx.Book()
    book.ctxs[(0, 0)] = ctx = _HamCtx(book, 0, 0)
    targets = np.stack([np.eye(8, dtype=np.complex128) * (1 + i) for i in range(5)])
    with book.installed():
        data = opt.approximate_target_U(targets)
        single = opt.approximate_target_U(targets[0])
    (name, rec), (_, rec1) = ctx.log
    assert name == "ham_minimize" and rec["dim"] == 8 and rec["n_params"] == 7 and rec["cost_kind"] == _ffi.COST_SQUARE
    assert rec["exit_loss"] == opt.success_threshold and rec["params"]["restarts"] == 4 and rec["params"]["seed"] == 11
    assert rec["params"]["flags"] & _ffi.FLAG_EARLY_EXIT and rec["params"]["flags"] & _ffi.FLAG_ORDERED
    # the start points: default_rng(seed).uniform(low, high, (N, R, n)) -- reproducible, and what a CPU comparison can draw itself
    x0 = np.random.default_rng(11).uniform(low, high, (5, 4, 7))
    assert rec["x0"]["shape"] == [5, 4, 7] and rec["x0"] == fake_ctx.encode(x0)
    assert np.all(x0[..., 6] == 1.0) and np.all(np.abs(x0[..., :3]) <= math.pi) and np.all((x0[..., 3:6] >= 0) & (x0[..., 3:6] < 2))
    assert rec1["x0"]["shape"] == [1, 4, 7] and rec1["x0"] == fake_ctx.encode(np.random.default_rng(11).uniform(low, high, (1, 4, 7)))
    assert isinstance(data, list) and len(data) == 5 and not isinstance(single, list)
    for t, entry in enumerate(data):
        loss, r = fake_ctx.stage_winner(t, 1, 4, opt.success_threshold)
        assert entry.cycles == 1 and entry.loss_result == loss and entry.success_label == int(loss <= opt.success_threshold)
        assert np.array_equal(entry.Xk, fake_ctx.item_x(t, 1, r, 7))  # Xk in argument order, all n of them
    assert single.loss_result == data[0].loss_result and np.array_equal(single.Xk, data[0].Xk)
    assert list(opt.training_loss) == [e.loss_result for e in data] + [single.loss_result] and list(opt.best_cycle_list) == [1] * 6
    assert opt.last_stats["kernel_launches"] == 1 and opt.last_stats["items"][1] == 4
    # approximate_from_distribution takes a list of targets
    with book.installed():
        tl, cl, data2 = opt.approximate_from_distribution(list(targets[:2]))
    assert [e.loss_result for e in data2] == [e.loss_result for e in data[:2]] and cl == []


def test_search_start_points_are_solvable_on_the_cpu():
    """The seed of the GPU search test, checked here: SciPy BFGS on the host model, from the very start points the GPU test hands to
    the device, must solve (loss < 1e-10) at least 16 of the 64 for every target.  Counts with SEARCH_SEED = 5: VSwap 55, DeltaSwap 47,
    CParitySwap 48 of 64."""
    low, high = ham_cases.search_range()
    terms = ham_cases.hamiltonian("circulator").device_terms()
    targets = ham_cases.search_targets()
    x0 = HamiltonianTemplate(hm.CirculatorHamiltonian(), low, high).start_points(ham_cases.SEARCH_SEED, len(targets), ham_cases.SEARCH_RESTARTS)
    counts = [sum(ham_cases.scipy_minimize(terms, targets[t], x0[t, r])[0] < 1e-10 for r in range(ham_cases.SEARCH_RESTARTS))
              for t in range(len(targets))]
    print("SciPy BFGS successes of the 64 start points per target:", dict(zip(ham_cases.SEARCH_NAMES, counts)))
    assert min(counts) >= 16, counts
