"""Host: the model of the span loop's bookkeeping (tests/span_loop_model.py) on hand-worked tables, against a literal sequential
restatement of the reference's loop on random tables, and against the oracle's ``run_reference`` on one tiny real case."""
import numpy as np
import pytest
import scipy.optimize as opt

from oracle import slam_oracle as o
import span_loop_model as m

INF, NAN = np.inf, np.nan
THR = 0.25  # (exactly representable: a table entry can equal it)


def _tagged_params(k, t, r):
    """Parameters that name their (span, target, restart): every entry of a row is 100 k + 10 t + r + 1 (never zero)."""
    return np.repeat((100.0 * k + 10.0 * np.asarray(t) + np.asarray(r) + 1.0)[:, None], m.default_n_of(k), axis=1)


def _row(k, t, r, nmax=24):
    x = np.zeros(nmax)
    x[: 6 * (k + 1)] = 100.0 * k + 10.0 * t + r + 1.0
    return x


def test_stage_winner_rules():
    L = np.array([[0.9, 0.2, 0.1],      # first below the threshold wins, not the lowest
                  [0.9, 0.5, 0.5],      # none below: the lowest, ties to the lower index
                  [0.9, THR, 0.7],      # a loss EQUAL to the threshold is not below it: the lowest loss (which it is) wins
                  [THR, 0.3, 0.2],      # equal to the threshold at index 0, below at index 2
                  [INF, INF, INF],      # nothing finite: restart 0
                  [NAN, 0.8, INF],      # NaN never wins
                  [NAN, INF, 0.1]])
    assert m.stage_winner(L, THR).tolist() == [1, 1, 1, 2, 0, 1, 2]
    assert m.stage_winner(L, THR, ordered=False).tolist() == [2, 1, 1, 2, 0, 1, 2]


def test_hand_worked_loop_ties_threshold_equality_and_inf_rows():
    #            target 0            1                  2                  3                  4
    L1 = np.array([[0.9, 0.2], [0.5, 0.5], [INF, INF], [THR, 0.6], [0.3, 0.4]])
    L2 = np.array([[9.0, 9.0], [0.5, 0.1], [INF, 0.7], [0.3, THR], [0.3, 0.35]])
    L3 = np.array([[9.0, 9.0], [9.0, 9.0], [INF, INF], [0.24, 0.0], [0.3, 0.3]])
    res = m.run_span_loop({1: L1, 2: L2, 3: L3}, _tagged_params, THR, 1, 3)
    # 0: solved at span 1 by restart 1.  1: tie at span 1 (restart 0), solved at span 2.  2: (+inf, span 1, restart 0) first, 0.7 at
    # span 2, span 3 brings nothing.  3: best == threshold at span 1 -- KEPT; span 2's 0.25 is not strictly lower; span 3's first
    # restart below the threshold wins although restart 1 is lower.  4: 0.3 three times -- only the first is taken; never solved.
    assert res.best_loss.tolist() == [0.2, 0.1, 0.7, 0.24, 0.3]
    assert res.best_cycles.tolist() == [1, 2, 2, 3, 1]
    want_x = np.stack([_row(1, 0, 1), _row(2, 1, 1), _row(2, 2, 1), _row(3, 3, 0), _row(1, 4, 0)])
    assert np.array_equal(res.best_x, want_x)
    assert [res.active[k].tolist() for k in (1, 2, 3)] == [[0, 1, 2, 3, 4], [1, 2, 3, 4], [2, 3, 4]]
    assert res.unsolved.tolist() == [2, 4]
    want_span = np.full((5, 16), NAN)
    want_span[:, 0] = [0.2, 0.5, INF, THR, 0.3]
    want_span[1:, 1] = [0.1, 0.7, THR, 0.3]
    want_span[2:, 2] = [0.7, 0.24, 0.3]
    assert np.array_equal(np.isnan(res.span_loss), np.isnan(want_span))
    assert np.array_equal(np.nan_to_num(res.span_loss), np.nan_to_num(want_span))
    assert res.winner[1].tolist() == [1, 0, 0, 0, 0] and res.winner[3].tolist() == [0, 0, 0]


def test_a_target_that_never_has_a_finite_loss_keeps_the_first_stage():
    L = {k: np.full((1, 3), INF) for k in (1, 2, 3)}
    res = m.run_span_loop(L, _tagged_params, THR, 1, 3)
    assert res.best_loss.tolist() == [INF] and res.best_cycles.tolist() == [1]
    assert np.array_equal(res.best_x[0], _row(1, 0, 0))
    assert np.array_equal(res.span_loss[0, :3], [INF, INF, INF]) and np.all(np.isnan(res.span_loss[0, 3:]))


def test_k_min_2_and_windows_leave_the_rest_untouched():
    L2 = np.array([[0.1, 0.1], [0.6, 0.5], [0.2, 0.3], [0.9, 0.9]])
    L3 = np.array([[0.0, 0.0], [0.7, 0.2], [0.0, 0.0], [0.1, 0.1]])
    res = m.run_span_loop({2: L2, 3: L3}, _tagged_params, THR, 2, 3, targets=[1, 2])
    assert res.best_loss.tolist() == [INF, 0.2, 0.2, INF] and res.best_cycles.tolist() == [-1, 3, 2, -1]
    assert res.ran.tolist() == [False, True, True, False]
    assert np.all(np.isnan(res.span_loss[[0, 3]])) and np.all(res.best_x[[0, 3]] == 0.0)
    assert np.all(np.isnan(res.span_loss[:, 0]))  # span 1 was not run for anybody
    assert np.array_equal(res.best_x[1], _row(3, 1, 1)) and np.array_equal(res.best_x[2], _row(2, 2, 0))
    assert [res.active[k].tolist() for k in (2, 3)] == [[1, 2], [1]]
    # a list in another order is the same set of targets
    res2 = m.run_span_loop({2: L2, 3: L3}, _tagged_params, THR, 2, 3, targets=[2, 1])
    assert np.array_equal(res2.best_loss, res.best_loss) and np.array_equal(res2.best_x, res.best_x)
    # a wider row (k_layout above k_max): zeros behind
    res3 = m.run_span_loop({2: L2, 3: L3}, _tagged_params, THR, 2, 2, targets=[1, 2], nmax=24)
    assert res3.best_x.shape == (4, 24) and np.array_equal(res3.best_x[1], _row(2, 1, 1))


@pytest.mark.parametrize("carry", [False, True])
def test_predicted_sizes_with_and_without_carry(carry):
    size = np.array([0, 1, 2, 2, 3, 4, 1])  # local, 1, 2, 2, 3, out of reach, 1
    L1 = np.full((7, 2), 0.5)
    L1[6] = [0.3, 0.1]
    L2 = np.full((7, 2), 0.4)
    L2[2] = [0.2, 0.1]
    L3 = np.full((7, 2), 0.35)
    L3[1] = [0.0, 0.0]
    res = m.run_span_loop({1: L1, 2: L2, 3: L3}, _tagged_params, THR, 1, 3, first_size=size, carry=carry)
    assert res.best_loss[0] == 0.0 and res.best_cycles[0] == 0 and not res.ran[0]
    assert res.best_loss[5] == INF and res.best_cycles[5] == -1 and not res.ran[5]
    if carry:
        assert [res.active[k].tolist() for k in (1, 2, 3)] == [[1, 6], [1, 2, 3], [1, 3, 4]]
        assert res.best_loss.tolist() == [0.0, 0.0, 0.2, 0.35, 0.35, INF, 0.1]
        assert res.best_cycles.tolist() == [0, 3, 2, 3, 3, -1, 1]
        assert np.array_equal(np.isnan(res.span_loss[3, :4]), [True, False, False, True])
    else:
        assert [res.active[k].tolist() for k in (1, 2, 3)] == [[1, 6], [2, 3], [4]]
        assert res.best_loss.tolist() == [0.0, 0.5, 0.2, 0.4, 0.35, INF, 0.1]
        assert res.best_cycles.tolist() == [0, 1, 2, 2, 3, -1, 1]
        assert np.array_equal(np.isnan(res.span_loss[3, :4]), [True, False, True, True])
    assert np.array_equal(res.best_x[2], _row(2, 2, 0)) and np.array_equal(res.best_x[6], _row(1, 6, 1))


def test_unordered_mode_takes_the_lowest_loss_and_has_the_same_active_sets():
    rng = np.random.default_rng(5)
    L = {k: rng.choice([0.1, 0.2, THR, 0.3, 0.6], size=(200, 4)) for k in (1, 2, 3)}
    a = m.run_span_loop(L, _tagged_params, THR, 1, 3)
    b = m.run_span_loop(L, _tagged_params, THR, 1, 3, ordered=False)
    for k in (1, 2, 3):
        assert np.array_equal(a.active[k], b.active[k])
        assert np.array_equal(b.winner[k], np.argmin(L[k][b.active[k]], axis=1))
    assert np.any(a.best_loss != b.best_loss)


@pytest.mark.parametrize("seed", range(6))
def test_model_equals_the_literal_sequential_loop_on_random_tables(seed):
    """Few distinct values: ties inside a row, ties across spans, entries equal to the threshold and +inf are all frequent."""
    rng = np.random.default_rng(seed)
    N, R = 300, 1 + seed
    k_min = 1 + seed % 2
    values = np.array([0.0, 0.1, 0.2, THR, 0.3, 0.5, INF])
    L = {k: rng.choice(values, size=(N, R), p=[0.02, 0.04, 0.05, 0.2, 0.25, 0.24, 0.2]) for k in range(k_min, 4)}
    res = m.run_span_loop(L, _tagged_params, THR, k_min, 3)
    loss, cyc, x, span = m.sequential_reference_loop(L, _tagged_params, THR, k_min, 3)
    assert np.array_equal(res.best_loss, loss) and np.array_equal(res.best_cycles, cyc) and np.array_equal(res.best_x, x)
    assert np.array_equal(np.isnan(res.span_loss), np.isnan(span)) and np.array_equal(np.nan_to_num(res.span_loss), np.nan_to_num(span))
    assert len(set(cyc.tolist())) == 4 - k_min and np.any(loss == THR) and (R > 3 or np.any(np.isinf(span[:, k_min - 1])))


def test_model_equals_run_reference_on_a_tiny_real_case():
    """sqrt(iSWAP), spans 1..2, two restarts, targets built from one and from two gates: the item table is filled by the same SciPy
    calls ``run_reference`` makes (same start points, analytic gradient), and the model must name what its loop returns."""
    gate = o.riswap_matrix(0.5)
    rng = np.random.default_rng(6)
    targets = [o.template_eval(rng.uniform(0, 2 * np.pi, 12), [gate]), o.template_eval(rng.uniform(0, 2 * np.pi, 18), [gate, gate])]
    R, thr = 2, 1e-8  # (SciPy's BFGS stops at its gradient tolerance with losses of a few 1e-10)

    def x0_fn_of(t):
        return lambda k, r: o.x0_philox(11, t, r, k)

    L = {k: np.empty((2, R)) for k in (1, 2)}
    X = {k: np.empty((2, R, 6 * (k + 1))) for k in (1, 2)}
    for t, T in enumerate(targets):
        for k in (1, 2):
            for r in range(R):
                res = opt.minimize(fun=lambda xx: o.loss_and_grad(xx, [gate] * k, T), jac=True, method="BFGS", x0=x0_fn_of(t)(k, r),
                                   options={"maxiter": 2500})
                L[k][t, r], X[k][t, r] = float(res.fun), res.x
    model = m.run_span_loop(L, X, thr, 1, 2)
    for t, T in enumerate(targets):
        loss, xk, cyc, _ = o.run_reference(T, [gate], range(1, 3), R, thr, x0_fn=x0_fn_of(t), analytic_jac=True)
        assert model.best_loss[t] == loss and model.best_cycles[t] == cyc
        assert np.array_equal(model.best_x[t, : len(xk)], xk) and np.all(model.best_x[t, len(xk):] == 0.0)
    # the one-gate target stops the loop at its first restart; the two-gate target goes through every restart of span 1 before the
    # second restart of span 2 solves it
    assert model.best_cycles.tolist() == [1, 2] and np.all(model.best_loss < thr)
    assert model.winner[1][0] == 0 and not np.any(L[1][1] < thr) and model.winner[2].tolist() == [1]
