"""CPU: the yardstick of the closed-form sqrt(iSWAP) decomposition -- tests/analytic_ref.py, the NumPy restatement the GPU tests
compare ``slam_sqiswap_decompose`` with -- does what it says: its circuits equal their targets, with the sizes span_rules gives.

Bounds: loss <= 1e-14 (measured: <= 4.5e-16 on 3000-4000 Haar targets and the named list; the loss is quadratic in the coordinate
gap, so the sqrt(ulp) error of an arccos at a chamber face does not show in it); best shift margin >= 0 for every three-gate target
(0.0725 at the least over Haar targets, 0 at SWAP).  The guard on the stated deviation from the reference: with the reference's
expression for gamma the two-gate circuit built for CAN(0.3, 0.2, 0.05) misses that class by more than 1e-2.
"""
import numpy as np
import pytest

import analytic_ref as ar
import kak_ref as kr
from slam_decomposition_amd import weyl
from slam_decomposition_amd.sampler import random_unitary


@pytest.fixture(scope="module")
def haar():
    T = np.stack([random_unitary(4, seed=770000 + i) for i in range(512)])
    return T, [ar.decompose(t) for t in T]


def test_haar_circuits_equal_their_targets(haar):
    T, res = haar
    loss = np.array([ar.loss(t, r[2]) for t, r in zip(T, res)])
    k = np.array([r[0] for r in res])
    print(f"ANALYTIC host haar: worst loss {loss.max():.3g} worst gap {max(r[3] for r in res):.3g} share of two gates {np.mean(k == 2):.4f}")
    assert loss.max() <= 1e-14
    assert np.array_equal(k, ar.expected_size(T))


@pytest.mark.parametrize("name,gate", ar.NAMED, ids=[n for n, _ in ar.NAMED])
def test_named_circuits_equal_their_targets(name, gate):
    rng = np.random.default_rng(5)
    for _ in range(4):
        t = np.exp(1j * rng.uniform(0, 2 * np.pi)) * np.kron(kr.random_su2(rng), kr.random_su2(rng)) @ gate @ np.kron(kr.random_su2(rng), kr.random_su2(rng))
        k, x, W, gap, u = ar.decompose(t)
        assert len(x) == 6 * (k + 1) and np.all(np.isfinite(x))
        assert ar.loss(t, W) <= 1e-14, (name, ar.loss(t, W))
        assert gap <= 1e-7
        if name not in ar.ON_BOUNDARY:
            assert k == ar.expected_size(t[None])[0], (name, k)


def test_shift_margin_is_never_negative(haar):
    T, res = haar
    c = np.array([weyl.kak(t)[3] for t, r in zip(T, res) if r[0] == 3])
    named3 = np.array([weyl.kak(g)[3] for _, g in ar.NAMED if ar.expected_size(g[None])[0] == 3])
    for pts in (c, named3):
        _, f, m = ar.best_shift(pts)
        assert len(pts) > 0 and m.min() >= 0.0, m.min()
        assert np.all(np.abs(f[:, 2]) <= f[:, 0] - f[:, 1])
    print(f"ANALYTIC host margins: least over {len(c)} Haar targets {ar.best_shift(c)[2].min():.4f}")


def test_shift_locals_are_exact():
    """CAN(s) = Ls S Rs up to a phase for each of the 12 placements."""
    for i in range(12):
        (l1, l2), (r1, r2) = ar.shift_locals(i)
        assert ar.up_to_phase(ar.can(ar.SHIFTS[i]), np.kron(l1, l2) @ ar.S @ np.kron(r1, r2)) <= 1e-14


def test_the_reference_gamma_misses_generic_classes():
    f = np.array([0.3, 0.2, 0.05])
    h = 0.5 * np.pi
    gaps = []
    for ref in (False, True):
        al, be, ga, _ = ar.interior(f, reference_gamma=ref)
        V = ar.template(np.r_[np.zeros(6), [be, -h, h, al, ga - h, ga + h], np.zeros(6)], 2)
        gaps.append(float(np.max(np.abs(ar.fold_chamber(np.array(weyl.c1c2c3(V, ndigits=12))) - f))))
    assert gaps[0] <= 1e-12 and gaps[1] > 1e-2, gaps
