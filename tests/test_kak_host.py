"""CPU: ``weyl.kak`` (the NumPy restatement of csrc/slam_kak.hpp) against the 40-digit chamber points of
tests/golden/weyl_lookup_reference.npz and the closed-form product of tests/kak_ref.py, with the assertions of tests/test_gpu_kak.py;
argument validation of the new Python entry points."""
import numpy as np
import pytest

import kak_ref as kr
import weyl_ref as w

GROUPS = w.load_fixture()
BANK = GROUPS[0]
BY_NAME = {g["meta"]["name"]: g for g in GROUPS[1:]}


def _host_kak(U):
    from slam_decomposition_amd import weyl

    rs = [weyl.kak(u) for u in U]
    return tuple(np.stack([np.asarray(r[j]) for r in rs]) for j in range(6))


@pytest.mark.parametrize("name", kr.MATRIX_GROUP_NAMES)
def test_host_kak_on_the_fixture(name):
    g = BY_NAME[name]
    U = w.unitaries_of(g, BANK)
    kr.check_group("weyl.kak", g, U, _host_kak(U), with_residual=name != "drifted")


def test_mirror_image_is_the_same_product():
    from slam_decomposition_amd import weyl

    rng = np.random.default_rng(5)
    for c in ((0.7, 0.2, 0.0), (0.31, 0.2, 0.11), (0.5, 0.5, 0.5)):
        U = np.exp(0.3j) * kr.kron2(kr.random_su2(rng), kr.random_su2(rng)) @ kr.can(c) @ kr.kron2(kr.random_su2(rng), kr.random_su2(rng))
        r = weyl.kak(U)
        m = weyl.mirror_kak(*r)
        assert np.allclose(m[3], (1 - r[3][0], r[3][1], -r[3][2]), atol=0, rtol=0)
        assert np.max(np.abs(kr.rebuild(*m) - U)) <= kr.FLOOR
        assert float(kr.factor_defect(m)) <= kr.FLOOR


def test_reference_decomposition_is_independent_and_sane():
    U = w.unitaries_of(BY_NAME["general"], BANK)
    assert kr.e_ref_of("general", U) < 1e-13  # generic spectra: a plain fp64 code is accurate there


def _bare_context(n_targets=4):
    from slam_decomposition_amd import _ffi

    ctx = _ffi.Context.__new__(_ffi.Context)  # no device: only the checks that run before the library is called
    ctx._lib, ctx._h, ctx.n_targets, ctx.n_gates = None, None, n_targets, 1
    return ctx


def test_binding_validates_shapes_before_the_call():
    ctx = _bare_context()
    with pytest.raises(ValueError):
        ctx.kak(np.zeros((4, 4), dtype=complex))
    with pytest.raises(ValueError):
        ctx.kak(np.zeros((2, 4, 3), dtype=complex))
    for first, count in ((-1, 1), (0, 5), (3, 2), (0, -1)):
        with pytest.raises(ValueError):
            ctx.targets_kak(first, count)
    with pytest.raises(ValueError):
        ctx.complete_locals([0, 0], np.zeros((3, 12)), np.zeros(3, dtype=np.int32))  # rows of a k = 1 template
    with pytest.raises(ValueError):
        ctx.complete_locals([0], np.zeros((3, 12)), np.zeros(2, dtype=np.int32))
    with pytest.raises(ValueError):
        ctx.complete_locals([], np.zeros((3, 6)), np.zeros(3, dtype=np.int32))
    with pytest.raises(ValueError):
        ctx.complete_locals([0], np.zeros(12), np.zeros(1, dtype=np.int32))


def test_host_kak_and_template_validate_their_arguments():
    from slam_decomposition_amd import weyl
    from slam_decomposition_amd.basis import CircuitTemplate
    from slam_decomposition_amd.gates import RiSwapGate

    with pytest.raises(ValueError):
        weyl.kak(np.eye(2))
    b = CircuitTemplate(base_gates=[RiSwapGate(1 / 2)], no_exterior_1q=True, maximum_span_guess=3)
    with pytest.raises(ValueError):
        b.undo_invariant_transform(np.eye(4), np.zeros(6))  # not built
    b.build(2)
    with pytest.raises(ValueError):
        b.undo_invariant_transform(np.eye(3), np.zeros(6))
    with pytest.raises(ValueError):
        b.undo_invariant_transform(np.eye(4), np.zeros(18))  # the exterior layers are not part of this template's Xk


def test_complete_local_gates_validates_and_refuses_v2():
    from slam_decomposition_amd.basis import CircuitTemplate
    from slam_decomposition_amd.basis_abc import DataDictEntry
    from slam_decomposition_amd.basisv2 import CircuitTemplateV2
    from slam_decomposition_amd.cost_function import BasicCost, MakhlinFunctionalCost
    from slam_decomposition_amd.gates import RiSwapGate
    from slam_decomposition_amd.optimizer import TemplateOptimizer

    v2 = TemplateOptimizer(CircuitTemplateV2(base_gates=[RiSwapGate]), BasicCost())
    with pytest.raises(NotImplementedError):
        v2.complete_local_gates(np.eye(4)[None], [DataDictEntry(1, 0.0, [0.0] * 13, 1)])
    opt = TemplateOptimizer(CircuitTemplate(base_gates=[RiSwapGate(1 / 2)], maximum_span_guess=3), MakhlinFunctionalCost())
    eye = np.eye(4, dtype=complex)[None]
    with pytest.raises(ValueError):
        opt.complete_local_gates(np.eye(4), [DataDictEntry(1, 0.0, [0.0] * 12, 1)])  # not a stack
    with pytest.raises(ValueError):
        opt.complete_local_gates(eye, [])  # one target, no entry
    with pytest.raises(ValueError):
        opt.complete_local_gates(eye, [DataDictEntry(1, 0.0, [], 0)])  # nothing was fitted
    with pytest.raises(ValueError):
        opt.complete_local_gates(eye, [DataDictEntry(1, 0.0, [0.0] * 12, 2)])  # 12 parameters are a k = 1 row
