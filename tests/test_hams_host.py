"""CPU: the time-sliced Hamiltonian templates' host side -- hamiltonian.TimeSliced and the n_slices constructors, the host model
tests/hams_ref.py (against mpmath at 40 digits, central differences and tests/ham_ref.py at one slice), the new C ABI's refusals (no
context needed) and the routing of ``TemplateOptimizer``.  tests/test_gpu_hams.py holds the GPU side."""
import ctypes as C

import numpy as np
import pytest

import fake_ctx
import ham_ref
import hams_cases
import hams_ref
from slam_decomposition_amd import _ffi
from slam_decomposition_amd import hamiltonian as hm
from slam_decomposition_amd.basis import HamiltonianTemplate
from slam_decomposition_amd.cost_function import BasicCost
from slam_decomposition_amd.optimizer import TemplateOptimizer

EPS = np.finfo(np.float64).eps
INVALID, UNSUPPORTED = -1, -3
CASES = [(name, s) for name in hams_cases.NAMES for s in hams_cases.SLICES]


def _scale(terms, x):
    """max(1, |t| max_s ||H_s||_2): what the rounding error of the product of S slice exponentials, each over t / S, is proportional to"""
    norms = [np.linalg.norm(ham_ref.hamiltonian(hams_ref.slice_terms(terms, s), x), 2) for s in range(terms["n_slices"])]
    return max(1.0, abs(ham_ref.time_of(terms, x)) * max(norms))


@pytest.mark.parametrize("name,n_slices", CASES)
def test_fixed_rows_pass_the_floor(name, n_slices):
    """Every fixed row of the GPU parity test is compared: it has |z| >= Z_FLOOR for at least one of the two targets."""
    terms, targets, x, tof, kept = hams_cases.parity_items(name, n_slices)
    assert np.all(kept >= 1), dict(zip(hams_cases.SPECIAL, kept))
    assert np.all(1.0 - hams_cases.parity_reference(name, n_slices, False)[0] >= hams_cases.Z_FLOOR)
    assert np.any(np.diff(tof) < 0) and len(x) >= 7 + 16


@pytest.mark.parametrize("name,n_slices", CASES)
def test_model_against_mpmath_at_40_digits(name, n_slices):
    """The model's own error on the evaluation cases of the GPU test: at most 32 eps max(1, |t| max ||H_s||) per slice exponential and
    their errors add over the product, so S times that in the unitary and in the loss.  Measured (worst over the three pulses): U
    7.0e-15 / 7.1e-15 / 6.6e-15 / 7.6e-15 and loss 1.6e-15 / 1.6e-15 / 1.7e-15 / 1.8e-15 at S = 1 / 2 / 3 / 8."""
    import mpmath

    terms, targets, x, tof, _ = hams_cases.parity_items(name, n_slices)
    loss, _, u = hams_cases.parity_reference(name, n_slices, False)
    d, S = terms["dim"], n_slices
    worst_u = worst_l = 0.0
    with mpmath.workdps(40):
        for m in range(len(x)):
            tau = mpmath.mpf(ham_ref.time_of(terms, x[m])) / S
            ref = mpmath.eye(d)
            for s in range(S):
                h = ham_ref.hamiltonian(hams_ref.slice_terms(terms, s), x[m])
                ref = mpmath.expm(mpmath.matrix(h.tolist()) * mpmath.mpc(0, -tau)) * ref
            ref = np.array([[complex(ref[i, j]) for j in range(d)] for i in range(d)])
            e_u = np.max(np.abs(u[m] - ref))
            e_l = abs(loss[m] - (1.0 - abs(np.trace(targets[tof[m]].conj().T @ ref)) / d))
            worst_u, worst_l = max(worst_u, e_u), max(worst_l, e_l)
            bound = 32 * EPS * _scale(terms, x[m]) * S
            assert e_u < bound and e_l < bound, (m, e_u, e_l, bound)
    print(f"hams model vs mpmath {name} S={n_slices}: U {worst_u:.3e} loss {worst_l:.3e}")


@pytest.mark.parametrize("square", [False, True], ids=["basic", "square"])
@pytest.mark.parametrize("name,n_slices", CASES)
def test_model_gradient_against_central_differences(name, n_slices, square):
    """Step h = 1e-6.  Truncation h^2 |f'''| / 6: the third derivative of 1 - |z| carries |z'|^3 / |z|^2 with |z'| <= |t| ||H|| (the time,
    the steepest direction), about 25 at the 2 pi rows, and |z| >= 0.05: |f'''| up to 6e6, truncation up to 1e-6 -- the bound.  (A wrong
    term in the gradient shows at 1e-2 and above.)  Rounding eps / h is 1e-10."""
    terms, targets, x, tof, _ = hams_cases.parity_items(name, n_slices)
    _, grad, _ = hams_cases.parity_reference(name, n_slices, square)
    n = terms["n_params"]
    for m in range(0, len(x), 5):
        fd = np.zeros(n)
        for j in range(n):
            e = np.zeros(n)
            e[j] = 1e-6
            fd[j] = (hams_ref.loss_grad(terms, x[m] + e, targets[tof[m]], square)[0] - hams_ref.loss_grad(terms, x[m] - e, targets[tof[m]], square)[0]) / 2e-6
        assert np.max(np.abs(fd - grad[m])) < 1e-6, (m, fd, grad[m])


@pytest.mark.parametrize("name", hams_cases.NAMES)
def test_one_slice_is_the_single_exponential_model(name):
    """S = 1 against tests/ham_ref.py on the same rows: the same eigh, the same formula -- equal to a few rounding errors."""
    terms, targets, x, tof, _ = hams_cases.parity_items(name, 1)
    one = hams_ref.slice_terms(terms, 0)
    for square in (False, True):
        loss, grad, u = hams_cases.parity_reference(name, 1, square)
        ref = ham_ref.batch(one, x, targets, tof, square)
        assert np.max(np.abs(loss - ref[0])) < 8 * EPS and np.max(np.abs(u - ref[2])) < 8 * EPS
        assert np.max(np.abs(grad - ref[1])) < 64 * EPS * max(1.0, np.max(np.abs(ref[1])))


@pytest.mark.parametrize("n_slices", hams_cases.SLICES)
def test_flat_form_is_the_reference_signature(n_slices):
    """construct_U_flat(scalars.., gx0.., gy0.., t) is the static construct_U(scalars.., gxvector, gyvector, t), bit for bit."""
    rng = np.random.default_rng(n_slices)
    N = n_slices
    for cls, k in ((hm.ConversionGainSmush, 4), (hm.ConversionGainSmush1QPhase, 8)):
        h = cls(n_slices=N)
        assert h.n_params == k + 2 * N + 1 and h.dim == 4 and len(h.parameter_names) == h.n_params
        assert h.parameter_names[k:] == tuple([f"gx{s}" for s in range(N)] + [f"gy{s}" for s in range(N)] + ["t"])
        x = rng.uniform(-2.0, 2.0, h.n_params)
        want = cls.construct_U(*x[:k], list(x[k:k + N]), list(x[k + N:k + 2 * N]), x[-1])
        assert np.array_equal(h.construct_U_flat(*x), want)
        assert np.array_equal(HamiltonianTemplate(h).eval(x), want)
        assert np.max(np.abs(hams_ref.unitary(h.device_terms(), x) - want)) < 32 * EPS * N * max(1.0, 2.0 * 6 * 2.0)
    assert hm.ConversionGainSmush.parameter_names.fget(hm.ConversionGainSmush(n_slices=2))[:4] == ("phi_c", "phi_g", "gc", "gg")
    assert hm.ConversionGainSmush1QPhase(n_slices=2).parameter_names[:8] == ("phi_a", "phi_b", "phi_c", "phi_g", "gc", "gg", "gz1", "gz2")


def test_no_argument_classes_are_unchanged():
    for cls in (hm.ConversionGainSmush, hm.ConversionGainSmush1QPhase):
        h = cls()
        assert h.n_slices is None and h.parameter_names[-3:] == ("gxvector", "gyvector", "t")
        with pytest.raises(NotImplementedError, match="time slices"):
            h.device_terms()
        with pytest.raises(NotImplementedError, match="time slices"):
            h.construct_U_flat(0.0)


@pytest.mark.parametrize("n_slices", hams_cases.SLICES)
def test_equal_slices_are_the_unsliced_hamiltonian(n_slices):
    """TimeSliced with every slice equal: the S exponentials over t / S commute, their product is exp(-i t H)."""
    rng = np.random.default_rng(50 + n_slices)
    base = hm.CirculatorHamiltonian()
    h = hm.TimeSliced(base, n_slices, sliced=("g_ab", "g_ac", "g_bc"))
    S = n_slices
    assert h.parameter_names == ("phi_ab", "phi_ac", "phi_bc") + tuple(f"{g}{s}" for g in ("g_ab", "g_ac", "g_bc") for s in range(S)) + ("t",)
    assert h.n_params == 3 + 3 * S + 1 and h.dim == 8 and h.device_terms()["t_index"] == h.n_params - 1
    for _ in range(3):
        xb = rng.uniform(-2.0, 2.0, 7)
        x = np.concatenate([xb[:3], np.repeat(xb[3:6], S), xb[6:]])
        want = base.construct_U(*xb)
        assert np.max(np.abs(h.construct_U(*x) - want)) < 32 * EPS * S * max(1.0, 2.0 * 6.0)
        assert np.max(np.abs(HamiltonianTemplate(h).eval(x) - want)) < 32 * EPS * S * max(1.0, 2.0 * 6.0)
    # a Hamiltonian without a time, a phase among the sliced arguments
    h2 = hm.TimeSliced(hm.ConversionGainHamiltonian(), 2, sliced=("gg",))
    assert h2.parameter_names == ("gc", "gg0", "gg1") and h2.device_terms()["t_index"] == -1
    u = h2.construct_U(0.3, 0.5, 0.5)
    assert np.max(np.abs(u - hm.ConversionGainHamiltonian.construct_U(0.3, 0.5))) < 64 * EPS


@pytest.mark.parametrize("name,n_slices", CASES)
def test_device_terms_reassemble_every_slice(name, n_slices):
    h = hams_cases.hamiltonian(name, n_slices)
    terms = h.device_terms()
    S, n = n_slices, terms["n_params"]
    assert terms["n_slices"] == S and terms["s_index"].shape == terms["phi_index"].shape == (S, len(terms["matrices"]))
    assert terms["s_index"].dtype == np.int32 and n <= hm.MAX_PARAMS and len(terms["matrices"]) <= hm.MAX_TERMS
    rng = np.random.default_rng(3)
    for _ in range(3):
        x = rng.uniform(-3.0, 3.0, n)
        for s in range(S):
            got = hm.assemble(hm.slice_terms(terms, s), x)
            if name == "circulator":
                want = h.H(*x, s=s)
                assert np.array_equal(want, hm.CirculatorHamiltonian().H(*x[:3], x[3 + s], x[3 + S + s], x[3 + 2 * S + s]))
            else:
                k = n - 2 * S - 1
                want = h.H(*x[:k], x[k + s], x[k + S + s])  # the reference's formula
            assert np.max(np.abs(got - want)) < 4 * EPS * 3.0, (s, got - want)
            assert np.max(np.abs(ham_ref.hamiltonian(hams_ref.slice_terms(terms, s), x) - want)) < 4 * EPS * 3.0


def test_time_sliced_refusals():
    base = hm.CirculatorHamiltonian()
    with pytest.raises(ValueError, match="strength or phase"):
        hm.TimeSliced(base, 2, sliced=("t",))
    with pytest.raises(ValueError, match="strength or phase"):
        hm.TimeSliced(base, 2, sliced=("g_xy",))
    for bad in (0, 9, -1, 2.5):
        with pytest.raises(ValueError, match="n_slices"):
            hm.TimeSliced(base, bad, sliced=("g_ab",))
        with pytest.raises(ValueError, match="n_slices"):
            hm.ConversionGainSmush(n_slices=bad)
    with pytest.raises(ValueError, match="at most 32"):
        hm.TimeSliced(base, 8, sliced=("g_ab", "g_ac", "g_bc", "phi_ab", "phi_ac"))  # 1 + 40 + 1
    with pytest.raises(NotImplementedError):
        hm.TimeSliced(hm.FSimHamiltonian(), 2)
    assert hm.TimeSliced(base, 8, sliced=("g_ab", "g_ac", "g_bc")).n_params == 28
    t = HamiltonianTemplate(hm.ConversionGainSmush1QPhase(n_slices=4), np.zeros(17), np.arange(17.0))
    assert t.n_params == 17 and t.n_qubits == 2 and t.start_points(1, 2, 3).shape == (2, 3, 17) and np.all(t.start_points(1, 2, 3)[..., 0] == 0.0)


# ---- the C ABI: everything is checked before the context -----------------------------------------------------------------------------
def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _call(kind, **over):
    """slam_hams_eval / slam_hams_minimize with a NULL context on a good two-slice two-mode description, `over` replacing arguments."""
    lib = _ffi.load_library()
    a = dict(dim=4, n=3, k=2, S=2, mats=np.zeros((2, 4, 4, 2)), s=np.array([[0, 1], [0, 2]], np.int32), p=np.full((2, 2), -1, np.int32), t=-1,
             targets=np.zeros((1, 4, 4, 2)), nt=1, x=np.zeros((3, 3)), tof=np.zeros(3, np.int32), M=3, cost=0,
             prm=_ffi.OptParams(restarts=3, maxiter=10, gtol=1e-9, stop_loss=1e-13, seed=1, flags=0), x0=np.zeros((1, 3, 3)))
    a["mats"][0, 2, 1, 0] = a["mats"][1, 3, 0, 0] = 1.0
    a.update(over)
    head = (None, a["dim"], a["n"], a["k"], a["S"], _ptr(a["mats"]), _ptr(a["s"]), _ptr(a["p"]), a["t"], _ptr(a["targets"]), a["nt"])
    if kind == "eval":
        loss = np.full(max(int(a["M"]), 1), 7.0)
        rc = lib.slam_hams_eval(*head, _ptr(a["x"]), _ptr(a["tof"]), a["M"], a["cost"], _ptr(loss), None, None)
        assert np.all(loss == 7.0)  # nothing is written on a refusal
    else:
        rc = lib.slam_hams_minimize(*head, a["cost"], C.byref(a["prm"]), 1e-10, _ptr(a["x0"]), *([None] * 9))
    return rc, lib.slam_last_error().decode()


@pytest.mark.parametrize("kind", ["eval", "minimize"])
def test_abi_refusals_come_before_the_context(kind):
    rc, msg = _call(kind)
    assert rc == INVALID and "ctx is NULL" in msg, msg  # everything else is in order: the context is looked at last
    many = np.zeros((3, 4, 4, 2))
    many[:, 2, 1, 0] = 1.0  # three terms on one entry
    cases = [
        (dict(S=0), INVALID, "n_slices"), (dict(S=9), UNSUPPORTED, "n_slices"), (dict(S=-1), INVALID, "n_slices"),
        (dict(s=np.array([[0, 1], [0, 3]], np.int32)), INVALID, "slice 1: s_index[1]"),
        (dict(s=np.array([[0, 1], [-1, 2]], np.int32)), INVALID, "slice 1: s_index[0]"),
        (dict(p=np.array([[-1, -1], [-1, 3]], np.int32)), INVALID, "slice 1: phi_index[1]"),
        (dict(p=np.array([[-2, -1], [-1, -1]], np.int32)), INVALID, "slice 0: phi_index[0]"),
        (dict(k=3, mats=many, s=np.zeros((2, 3), np.int32), p=np.full((2, 3), -1, np.int32)), UNSUPPORTED, "slice 0: entry (2, 1)"),
        (dict(n=33), UNSUPPORTED, "32 parameters"), (dict(k=17), UNSUPPORTED, "16 terms"), (dict(dim=5), INVALID, "dim"), (dict(t=3), INVALID, "t_index"),
        (dict(cost=2), INVALID, "cost kind"), (dict(cost=-1), INVALID, "cost kind"),
        (dict(targets=np.full((1, 4, 4, 2), np.inf)), INVALID, "targets"),
    ]
    if kind == "eval":
        cases += [(dict(x=np.full((3, 3), np.nan)), INVALID, "x: entry"), (dict(tof=np.array([0, 1, 0], np.int32)), INVALID, "target_of[1]")]
    else:
        cases += [(dict(x0=None), INVALID, "x0 is required"), (dict(x0=np.full((1, 3, 3), np.inf)), INVALID, "x0[0]"),
                  (dict(x0=np.full((1, 3, 3), np.nan)), INVALID, "x0[0]")]
    for over, code, word in cases:
        rc, msg = _call(kind, **over)
        assert rc == code and word in msg and "ctx is NULL" not in msg, (over.keys(), rc, msg)


def test_diagonal_halves_of_a_phase_free_term_merge():
    """gz1 A^+ A + gz2 B^+ B of ConversionGainSmush1QPhase: entry (0, 0) takes one contribution from each in the new calls (both halves
    of a phase-free term on the diagonal merge) -- the description passes every check.  The slam_ham_* pair is unchanged and counts
    four; and a diagonal term that carries a phase is not merged by the new calls either."""
    lib = _ffi.load_library()
    terms = hm.ConversionGainSmush1QPhase(n_slices=2).device_terms()
    m = np.ascontiguousarray(terms["matrices"])
    assert m[4][0, 0] == 0.5 and m[5][0, 0] == 0.5 and np.count_nonzero(m[4]) == 2 and np.count_nonzero(m[5]) == 2
    n, K = terms["n_params"], len(m)
    targets, x, tof, loss = np.zeros((1, 4, 4, 2)), np.zeros((1, n)), np.zeros(1, np.int32), np.zeros(1)

    def hams(phi):
        rc = lib.slam_hams_eval(None, 4, n, K, 2, _ptr(m.view(np.float64)), _ptr(terms["s_index"]), _ptr(phi), terms["t_index"], _ptr(targets), 1,
                                _ptr(x), _ptr(tof), 1, 0, _ptr(loss), None, None)
        return rc, lib.slam_last_error().decode()

    rc, msg = hams(terms["phi_index"])
    assert rc == INVALID and "ctx is NULL" in msg, msg
    one = hm.slice_terms(terms, 0)
    rc = lib.slam_ham_eval(None, 4, n, K, _ptr(m.view(np.float64)), _ptr(one["s_index"]), _ptr(one["phi_index"]), terms["t_index"], _ptr(targets), 1,
                           _ptr(x), _ptr(tof), 1, 0, _ptr(loss), None, None)
    assert rc == UNSUPPORTED and "entry (0, 0)" in lib.slam_last_error().decode()
    phased = terms["phi_index"].copy()
    phased[1, 4] = phased[1, 5] = 0  # slice 1: the z terms on a phase
    rc, msg = hams(phased)
    assert rc == UNSUPPORTED and "slice 1: entry (0, 0)" in msg, msg


# ---- TemplateOptimizer: a sliced description goes to the new stage --------------------------------------------------------------------
class _HamsCtx(fake_ctx.FakeCtx):
    def _minimize(self, tag, terms, targets, params, exit_loss, x0, cost_kind):
        self._rec(tag, n_params=terms["n_params"], n_slices=terms.get("n_slices"), x0=np.asarray(x0), cost_kind=cost_kind)
        self._k = 1
        out = self._stage(terms["n_params"], params, exit_loss, np.arange(len(targets)), True)
        out["item_x"] = np.zeros(out["item_loss"].shape + (terms["n_params"],))
        out["kernel_ms"] = 0.25
        return out

    def ham_minimize(self, terms, targets, params, exit_loss, x0, cost_kind=0):
        return self._minimize("ham_minimize", terms, targets, params, exit_loss, x0, cost_kind)

    def hams_minimize(self, terms, targets, params, exit_loss, x0, cost_kind=0):
        return self._minimize("hams_minimize", terms, targets, params, exit_loss, x0, cost_kind)


def test_optimizer_routes_sliced_descriptions_to_the_new_stage():
    low, high = hams_cases.search_range()
    book = fake_ctx.Book()
    book.ctxs[(0, 0)] = ctx = _HamsCtx(book, 0, 0)
    sliced = TemplateOptimizer(HamiltonianTemplate(hams_cases.search_hamiltonian(), low, high), BasicCost(), seed=11, training_restarts=4, override_fail=True)
    plain = TemplateOptimizer(HamiltonianTemplate(hm.ConversionGainPhaseHamiltonian()), BasicCost(), seed=11, training_restarts=4, override_fail=True)
    targets = np.stack([np.eye(4, dtype=np.complex128)] * 3)
    with book.installed():
        data = sliced.approximate_target_U(targets)
        plain.approximate_target_U(targets)
    (name, rec), (name1, rec1) = ctx.log
    assert name == "hams_minimize" and rec["n_slices"] == 4 and rec["n_params"] == 17 and name1 == "ham_minimize" and rec1["n_slices"] is None
    assert rec["x0"] == fake_ctx.encode(np.random.default_rng(11).uniform(low, high, (3, 4, 17)))
    assert len(data) == 3 and all(e.cycles == 1 and len(e.Xk) == 17 for e in data) and sliced.last_ham_stage["item_loss"].shape == (3, 4)


def test_local_start_points_converge_on_the_cpu():
    """The local-convergence case of the GPU test on the model: SciPy BFGS under SquareCost from the 8 starts within +-0.05 of p* ends
    below 1e-10 from every one (hams_cases.local_case explains the range of p*)."""
    terms, target, p, x0 = hams_cases.local_case()
    losses = [hams_cases.scipy_minimize(terms, target[0], x0[0, r], True)[0] for r in range(8)]
    print("SciPy BFGS local convergence, SquareCost:", losses)
    assert max(losses) < 1e-10


def test_search_start_points_are_solvable_on_the_cpu():
    """The seed, ranges and restart count of the GPU search test, checked here: SciPy BFGS on the host model, from the very start points
    the GPU test hands to the device, must solve (loss < 1e-10) at least half of the 16 for both planted targets, so that "at least one
    restart succeeds" is a condition the model alone meets with room.  Counts with SEARCH_SEED = 7: 16 and 16 of 16."""
    low, high = hams_cases.search_range()
    h = hams_cases.search_hamiltonian()
    terms = h.device_terms()
    targets = hams_cases.search_targets()
    x0 = HamiltonianTemplate(h, low, high).start_points(hams_cases.SEARCH_SEED, len(targets), hams_cases.SEARCH_RESTARTS)
    counts = [sum(hams_cases.scipy_minimize(terms, targets[t], x0[t, r])[0] < 1e-10 for r in range(hams_cases.SEARCH_RESTARTS))
              for t in range(len(targets))]
    print("SciPy BFGS successes of the 16 start points per planted target:", counts)
    assert min(counts) >= 8, counts
