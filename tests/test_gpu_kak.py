"""GPU: ``kak_kernel`` through slam_kak and slam_targets_kak on the matrix groups of tests/golden/weyl_lookup_reference.npz, with the
yardsticks of tests/kak_ref.py.  Every case is asserted, no masks:

  * residual  max |U - rebuild(...)| <= tol = min(max(8 e_ref, 1.2e-14), 1e-13), e_ref = the residual of the independent LAPACK
    decomposition on the same group (not on ``drifted``, whose matrices are unitary to 2e-10 only);
  * factors   each 2x2 factor unitary with |det - 1| within the same tol;
  * coordinates within ``weyl_ref.tolerance(e_ref)`` of the 40-digit chamber point and in the chamber to 1e-13 -- the yardstick of
    tests/test_gpu_weyl_hp.py -- and equal to ``c1c2c3(U, ndigits=-1)`` to 1e-13 (modulo the mirror where |c3_ref| <= 5e-9).

One ``KAK`` line per (path, kind) is printed (``-s``).
"""
import numpy as np
import pytest

import kak_ref as kr
import weyl_ref as w

pytestmark = pytest.mark.gpu

GROUPS = w.load_fixture()
BANK = GROUPS[0]
BY_NAME = {g["meta"]["name"]: g for g in GROUPS[1:]}


@pytest.mark.parametrize("name", kr.MATRIX_GROUP_NAMES)
def test_kak_of_matrices(hip_ctx, name):
    g = BY_NAME[name]
    U = w.unitaries_of(g, BANK)
    r = hip_ctx.kak(U)
    kr.check_group("kak", g, U, r, with_residual=name != "drifted")
    plain = hip_ctx.c1c2c3(U, ndigits=-1)
    d = np.max(np.abs(r.c - plain), axis=1)
    d = np.where(w.mirror_ok(g["ref"]), np.minimum(d, np.max(np.abs(kr.mirror(r.c) - plain), axis=1)), d)
    assert d.max() <= 1e-13, (name, int(np.argmax(d)), d.max())
    hip_ctx.set_targets(U)
    res = hip_ctx.targets_kak(0, len(U))
    kr.check_group("targets_kak", g, U, res, with_residual=name != "drifted")
    lo = len(U) // 3
    part = hip_ctx.targets_kak(lo, len(U) - lo)  # a window of the batch
    for got, whole in zip(part, res):
        assert np.array_equal(got, whole[lo:])


@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_batch_sizes_around_one_block(hip_ctx, n):
    g = BY_NAME["named"]
    U = w.unitaries_of(g, BANK)
    whole = hip_ctx.kak(U)
    part = hip_ctx.kak(U[:n])
    for got, ref in zip(part, whole):
        assert got.shape[0] == n and np.array_equal(got, ref[:n])
    tol = kr.tolerance(kr.e_ref_of("named", U))
    assert kr.residual(U[:n], part).max() <= tol and kr.factor_defect(part).max() <= tol
    hip_ctx.set_targets(U[:n])
    for got, ref in zip(hip_ctx.targets_kak(), part):
        assert np.array_equal(got, ref)


def test_empty_batch(hip_ctx):
    r = hip_ctx.kak(np.zeros((0, 4, 4), dtype=complex))
    assert r.phase.shape == (0,) and r.a1.shape == (0, 2, 2) and r.c.shape == (0, 3)
