"""CPU: family-extended decomposition on the host (slam_decomposition_amd/family_extend.py; reference
src/slam/utils/gates/family_extend.py:17-117) -- the family's members, links and tables, the walk and its unwind on hand-made tables,
hand-worked real cases, ``GateFamily.lookup`` against the one-target-at-a-time restatement of tests/family_ref.py on Haar targets,
``recursive_sibling_check``, and the argument checks of ``_ffi.Context.family_lookup`` that need no device.  No GPU."""
import math
import os

import numpy as np
import pytest

import family_ref
from slam_decomposition_amd import _ffi, coverage, family_extend as fe
from slam_decomposition_amd.basis import MixedOrderBasisCircuitTemplate
from slam_decomposition_amd.gates import ConversionGainGate
from slam_decomposition_amd.weyl import c1c2c3

PI = np.pi
CX = np.array([[1, 0, 0, 0], [0, 0, 0, 1], [0, 0, 1, 0], [0, 1, 0, 0]], dtype=np.complex128)
SWAP = np.array([[1, 0, 0, 0], [0, 0, 1, 0], [0, 1, 0, 0], [0, 0, 0, 1]], dtype=np.complex128)


def iswap_root(n):
    return ConversionGainGate(0, 0, PI / 2, 0, 1 / n)


def cx_root(n):
    return ConversionGainGate(0, 0, PI / 4, PI / 4, 1 / n)  # conversion and gain at equal strength: the CNOT class at t = 1


def u3(t, p, l):
    return np.array([[np.cos(t / 2), -np.exp(1j * l) * np.sin(t / 2)], [np.exp(1j * p) * np.sin(t / 2), np.exp(1j * (p + l)) * np.cos(t / 2)]])


_FAMILIES = {}


def family(kind, n, max_gates):
    key = (kind, n, max_gates)
    if key not in _FAMILIES:
        _FAMILIES[key] = fe.GateFamily(iswap_root(n) if kind == "iswap" else cx_root(n), cost_1q=0.1, max_gates=max_gates)
    return _FAMILIES[key]


# ---- the walk on hand-made tables -----------------------------------------------------------------------------------------------------
# members r = 1, 2, 3, 4, 6, 8, 12, 16 with unit base duration; links as GateFamily builds them
_R = [1, 2, 3, 4, 6, 8, 12, 16]
_EVEN = [_R.index(2 * r) if 2 * r in _R else -1 for r in _R]
_ODD = [_R.index(3 * r) if 3 * r in _R else -1 for r in _R]
_DUR = [0.05 * r for r in _R]

SYNTHETIC = {
    # name: (k per member (0: does not contain), durations, expected (r, k) of the walk)
    "even parity, the child wins": ([4, 2, 0, 1, 0, 0, 0, 0], _DUR, (4, 1)),
    "odd parity, the child wins": ([3, 0, 1, 0, 0, 0, 0, 0], _DUR, (3, 1)),
    "odd k at a member whose x3 child is missing": ([3, 0, 3, 0, 0, 0, 0, 0], [0.05, 0.1, 0.01, 0.2, 0.3, 0.4, 0.6, 0.8], (3, 3)),
    "the child does not contain the target": ([6, 0, 2, 0, 0, 0, 0, 0], _DUR, (1, 6)),
    "k = 1 at the base": ([1, 1, 1, 1, 1, 1, 1, 1], _DUR, (1, 1)),
    "k = 1 at a sibling ends the walk": ([2, 1, 0, 1, 0, 0, 0, 0], [0.05, 0.1, 0.15, 0.0001, 0.3, 0.4, 0.6, 0.8], (2, 1)),
    # own cost at r = 1: 3 * 0.1 + 2 * 0.05 = 0.4; at r = 2 (k 1): 2 * 0.1 + 0.2 = 0.4 exactly -- the child must lose
    "an exact cost tie": ([2, 1, 0, 0, 0, 0, 0, 0], [0.05, 0.2, 0.15, 0.2, 0.3, 0.4, 0.6, 0.8], (1, 2)),
    "depth 4": ([8, 4, 0, 2, 0, 1, 0, 0], _DUR, (8, 1)),
    "depth 4, a middle level wins": ([8, 4, 0, 2, 0, 2, 0, 0], [0.05, 0.1, 0.15, 0.2, 0.3, 5.0, 0.6, 0.8], (4, 2)),
    "the walk misses the best member": ([6, 3, 2, 0, 2, 0, 0, 0], _DUR, (2, 3)),
    "the base does not contain the target": ([0, 2, 1, 1, 0, 0, 0, 0], _DUR, None),
}


@pytest.mark.parametrize("name", list(SYNTHETIC))
def test_walk_on_hand_made_tables(name):
    ks, dur, want = SYNTHETIC[name]
    if name == "an exact cost tie":
        assert (2 + 1) * 0.1 + 2 * dur[0] == (1 + 1) * 0.1 + 1 * dur[1]
    ref = family_ref.walk_tables(ks, _EVEN, _ODD, dur, 0.1)
    got = fe.walk(np.array(ks)[:, None], _EVEN, _ODD, dur, 0.1, "reference")
    if want is None:
        assert ref is None and got.member[0] == -1 and got.gates[0] == -1 and math.isinf(got.cost[0])
    else:
        assert (_R[ref[0]], ref[1]) == want, ref
        assert (_R[got.member[0]], int(got.gates[0])) == want and got.cost[0] == ref[2]
    # "best": the minimum of own cost over all members that contain the target, never dearer than the walk
    bref = family_ref.best_tables(ks, dur, 0.1)
    best = fe.walk(np.array(ks)[:, None], _EVEN, _ODD, dur, 0.1, "best")
    if want is None:
        assert bref is None and best.gates[0] == -1
        return
    assert (int(best.member[0]), int(best.gates[0])) == bref[:2] and best.cost[0] == bref[2]
    assert best.cost[0] <= got.cost[0]
    costs = [(k + 1) * 0.1 + k * d for k, d in zip(ks, dur) if k]
    assert best.cost[0] == min(costs)


def test_best_beats_the_walk_and_ties_go_to_the_smaller_member():
    ks, dur, _ = SYNTHETIC["the walk misses the best member"]  # walk: r 1 (k 6) -> 2 (k 3) -> 6 (k 2); r = 3 (k 2) is cheaper
    got = fe.walk(np.array(ks)[:, None], _EVEN, _ODD, dur, 0.1, "reference")
    best = fe.walk(np.array(ks)[:, None], _EVEN, _ODD, dur, 0.1, "best")
    assert (_R[got.member[0]], got.gates[0]) == (2, 3) and (_R[best.member[0]], best.gates[0]) == (3, 2) and best.cost[0] < got.cost[0]
    tie = fe.walk(np.array([2, 1, 0, 0, 0, 0, 0, 0])[:, None], _EVEN, _ODD, [0.05, 0.2, 0.15, 0.2, 0.3, 0.4, 0.6, 0.8], 0.1, "best")
    assert tie.member[0] == 0 and tie.gates[0] == 2
    # all targets of a batch at once equal one at a time
    names = [n for n in SYNTHETIC if SYNTHETIC[n][1] is _DUR]
    batch = np.array([SYNTHETIC[n][0] for n in names]).T
    for policy in fe.POLICIES:
        whole = fe.walk(batch, _EVEN, _ODD, _DUR, 0.1, policy)
        for j, n in enumerate(names):
            one = fe.walk(np.array(SYNTHETIC[n][0])[:, None], _EVEN, _ODD, _DUR, 0.1, policy)
            assert (whole.member[j], whole.gates[j], whole.cost[j]) == (one.member[0], one.gates[0], one.cost[0]), (policy, n)
    with pytest.raises(ValueError, match="policy"):
        fe.walk(batch, _EVEN, _ODD, _DUR, 0.1, "cheapest")


# ---- members, links, tables -----------------------------------------------------------------------------------------------------------
def test_members_and_stop_condition():
    assert fe.GateFamily(iswap_root(16)).multipliers.tolist() == [1, 2, 3, 4, 6, 8, 9, 12, 16]
    assert fe.GateFamily(ConversionGainGate(0, 0, PI / 4, PI / 4, 1 / 5)).multipliers.tolist() == [1, 2, 3, 4]  # gc + gg = pi/2 at t = 1/5
    assert fe.GateFamily(iswap_root(1)).multipliers.tolist() == [1]
    assert fe.GateFamily(iswap_root(3)).multipliers.tolist() == [1, 2, 3]  # 3 * (1/3) = 1 up to rounding: the 1e-12 of the stop condition
    with pytest.raises(ValueError, match="stronger than a full iSWAP"):
        fe.GateFamily(ConversionGainGate(0, 0, PI / 2, 0, 1.5))
    with pytest.raises(ValueError, match="ConversionGainGate"):
        fe.GateFamily(CX)
    with pytest.raises(ValueError, match="at most 32"):
        fe.GateFamily(iswap_root(1000))
    fam = fe.GateFamily(iswap_root(16), cost_1q=0.25, max_gates=20)
    assert fam.basis_factor == iswap_root(16).cost() and abs(fam.basis_factor - 1 / 16) < 1e-15
    assert np.array_equal(fam.durations, fam.multipliers * fam.basis_factor)
    rs = fam.multipliers.tolist()
    for m, r in enumerate(rs):
        assert fam.child_even[m] == (rs.index(2 * r) if 2 * r in rs else -1)
        assert fam.child_odd[m] == (rs.index(3 * r) if 3 * r in rs else -1)
        g = fam.gates[m]
        assert g.params[-1] == 1 and abs(g.params[2] - PI / 2 * r / 16) < 1e-15 and abs(g.cost() - r / 16) < 1e-15  # unit duration
        assert np.allclose(fam.gate_coords[m], [r / 32, r / 32, 0])  # iSWAP is (1/2, 1/2, 0)
    assert fe.GateFamily(iswap_root(4), basis_factor=2.0).durations.tolist() == [2.0, 4.0, 6.0, 8.0]
    ref = family_ref.build_members(iswap_root(16), max_gates=20)
    assert [mem["r"] for mem in ref] == rs and [mem["duration"] for mem in ref] == fam.durations.tolist()


def test_tables_rows_and_early_stop():
    fam = fe.GateFamily(iswap_root(8), cost_1q=0.1, max_gates=20)
    assert fam.multipliers.tolist() == [1, 2, 3, 4, 6, 8]
    # k = 1 .. ceil(max_gates / r); sqrt(iSWAP) (r = 4) and iSWAP (r = 8) reach every target with three gates: cut there
    assert [len(t) for t in fam.tables] == [20, 10, 7, 3, 4, 3]
    assert fam.table(1) is fam.table(1)
    for m, t in enumerate(fam.tables):
        assert t.kinds.tolist() == [0] + [1] * (len(t) - 1)
        assert np.allclose(t.points[0], coverage.alcove_coordinates(fam.gate_coords[m])[0])
        for k in range(2, len(t) + 1):
            full = np.all(np.isneginf(t.bounds[k - 1]))
            assert full == (m in (3, 5) and k == 3)
            if not full:
                assert np.array_equal(t.bounds[k - 1], coverage.region([fam.gate_coords[m]] * k))
        assert np.array_equal(t.costs, [(k + 1) * 0.1 + k * fam.durations[m] for k in range(1, len(t) + 1)])
    assert np.array_equal(fam.row_costs(), np.concatenate([t.costs for t in fam.tables]))
    assert fam.rows()[:3] == [(1, 1), (1, 2), (1, 3)] and fam.rows()[20] == (2, 1) and len(fam.rows()) == 47


# ---- hand-worked real cases (cost_1q = 0.1, linear durations) ------------------------------------------------------------------------
def test_hand_worked_cases():
    coords = fe.fam_coords(np.stack([CX, SWAP]))
    # iSWAP^(1/n) reaches CX in n applications (n >= 2) and SWAP in ceil(3n / 2)
    for n in (2, 4, 6, 8):
        fam = family("iswap", n, 16)
        assert fam.first_k(0, coords).tolist() == [n, -(-3 * n // 2)], n
    f4, f6 = family("iswap", 4, 16), family("iswap", 6, 16)

    def result(fam, U, policy="reference"):
        r = fam.lookup_unitaries(U[None], policy)
        return int(fam.multipliers[r.member[0]]), int(r.gates[0]), float(r.cost[0])

    assert result(f4, CX)[:2] == (2, 2) and abs(result(f4, CX)[2] - 1.3) < 1e-12  # r 1 (k 4) -> 2 (k 2) -> 4 (k 2): sqrt(iSWAP) x 2
    assert result(f4, SWAP)[:2] == (2, 3) and abs(result(f4, SWAP)[2] - 1.9) < 1e-12  # r 1 (k 6) -> 2 (k 3), x6 outside
    assert result(f6, SWAP)[:2] == (3, 3) and abs(result(f6, SWAP)[2] - 1.9) < 1e-12  # r 1 (k 9) -> 3 (k 3)
    assert abs(f6.own_cost(0, 9) - 2.5) < 1e-12  # without the family
    assert result(f6, CX)[:2] == (2, 3) and abs(result(f6, CX)[2] - 1.4) < 1e-12  # r 1 (k 6) -> 2 (k 3) -> 6 (k 2: 2.3)
    assert result(f6, CX, "best")[:2] == (3, 2) and abs(result(f6, CX, "best")[2] - 1.3) < 1e-12
    # the restatement says the same
    for fam, n in ((f4, 4), (f6, 6)):
        mem = family_ref.build_members(iswap_root(n), max_gates=16)
        for U in (CX, SWAP):
            for policy in fe.POLICIES:
                assert result(fam, U, policy) == family_ref.family_ref(mem, c1c2c3(U), 0.1, policy)
    # local targets cost 0 (the identity and any other), a target of the base gate's own class costs 2 cost_1q + duration
    loc = np.kron(u3(0.3, 0.2, 0.1), u3(1.0, 0.5, 0.2))
    r = f4.lookup_unitaries(np.stack([np.eye(4), loc, iswap_root(4).to_matrix(), loc @ iswap_root(4).to_matrix()]))
    assert r.member.tolist() == [-1, -1, 0, 0] and r.gates.tolist() == [0, 0, 1, 1]
    assert r.cost[:2].tolist() == [0.0, 0.0] and np.allclose(r.cost[2:], 2 * 0.1 + 0.25, rtol=0, atol=1e-15)
    # out of reach of max_gates applications of the base gate
    weak = fe.GateFamily(iswap_root(8), max_gates=6)
    r = weak.lookup_unitaries(np.stack([CX, SWAP]))
    assert r.member.tolist() == [-1, -1] and r.gates.tolist() == [-1, -1] and np.all(np.isinf(r.cost))
    assert family_ref.family_ref(family_ref.build_members(iswap_root(8), max_gates=6), c1c2c3(CX))[1] == -1


# ---- GateFamily.lookup against the restatement, on Haar targets -----------------------------------------------------------------------
@pytest.fixture(scope="module")
def haar_coords():
    from scipy.stats import unitary_group

    U = unitary_group.rvs(4, size=2000, random_state=20261019)
    return fe.fam_coords(U)


@pytest.mark.parametrize("kind", ["iswap", "cx"])
def test_lookup_equals_the_restatement_on_haar_targets(haar_coords, kind):
    fam = family(kind, 4, 16)
    if kind == "cx":
        assert np.allclose(fam.gate_coords[-1], [0.5, 0, 0]) and fam.multipliers.tolist() == [1, 2, 3, 4]  # CX^(1/4) .. CX
    mem = family_ref.build_members(fam.base_gate, max_gates=16)
    ref_cost, got, memo = {}, {}, {}
    for policy in ("best", "reference"):
        got[policy] = fam.lookup(haar_coords, policy)
        assert np.all(got[policy].gates > 0)  # Haar targets: none local, none beyond 16 gates
        ref_cost[policy] = np.zeros(len(haar_coords))
        for i, c in enumerate(haar_coords):
            r, k, cost = family_ref.family_ref(mem, c, 0.1, policy, memo=memo)
            assert (r, k, cost) == (int(fam.multipliers[got[policy].member[i]]), int(got[policy].gates[i]), float(got[policy].cost[i])), (policy, i)
            ref_cost[policy][i] = cost
    base = np.array([fam.own_cost(0, int(k)) for k in fam.first_k(0, haar_coords)])
    assert np.all(got["best"].cost <= got["reference"].cost) and np.all(got["reference"].cost <= base)
    assert got["reference"].cost.mean() < base.mean()  # the family pays on Haar targets
    assert len(np.unique(got["reference"].member)) >= 2


# ---- recursive_sibling_check ----------------------------------------------------------------------------------------------------------
def test_recursive_sibling_check_returns_the_bound_template_and_the_cost():
    base = iswap_root(4)
    basis = MixedOrderBasisCircuitTemplate(base_gates=[base], chatty_build=False, maximum_span_guess=6)
    tpl, cost = fe.recursive_sibling_check(basis, CX, cost_1q=0.1, basis_factor=base.cost())
    assert abs(cost - 1.3) < 1e-12 and isinstance(tpl, MixedOrderBasisCircuitTemplate) and tpl is not basis
    assert tpl.cycles == 2 and tpl.gate_sequence() == [0, 0] and len(tpl.circuit_polytope) == 2
    assert np.allclose(c1c2c3(tpl.gate_matrices[0]), [0.25, 0.25, 0])  # sqrt(iSWAP), the winning member
    assert abs(tpl.base_gates[0].cost() - 0.5) < 1e-15 and tpl.n_params == 18
    tpl, cost = fe.recursive_sibling_check(basis, SWAP, cost_1q=0.1, basis_factor=base.cost())
    assert abs(cost - 1.9) < 1e-12 and tpl.cycles == 3 and np.allclose(c1c2c3(tpl.gate_matrices[0]), [0.25, 0.25, 0])
    # a target of the base gate's own class: the template that was handed in, at one gate; the cost is own cost, not the literal 1.2
    tpl, cost = fe.recursive_sibling_check(basis, base.to_matrix(), cost_1q=0.1, basis_factor=base.cost())
    assert tpl is basis and tpl.cycles == 1 and abs(cost - (2 * 0.1 + 0.25)) < 1e-15
    # basis_factor is the duration of the root gate (the reference's default of 1: unit-duration gates)
    _, cost = fe.recursive_sibling_check(basis, CX, cost_1q=0.25)
    assert cost == 3 * 0.25 + 2 * 2.0
    assert fe.recursive_sibling_check(basis, np.eye(4)) == (None, 0)
    assert fe.recursive_sibling_check(basis, np.kron(u3(0.3, 0.2, 0.1), u3(1.0, 0.5, 0.2))) == (None, 0)
    assert fe.recursive_sibling_check(basis, CX, rec_iter_factor=7)[1] == fe.recursive_sibling_check(basis, CX)[1]  # ignored
    with pytest.raises(ValueError, match="Smush Polytope not in memory"):
        fe.recursive_sibling_check(basis, CX, use_smush=True)
    with pytest.raises(ValueError, match="Monodromy did not find a polytope containing U.*max_gates = 3"):
        fe.recursive_sibling_check(basis, SWAP, max_gates=3)


# ---- what needs no device ---------------------------------------------------------------------------------------------------------------
def test_the_new_symbol_is_declared_and_bound():
    assert "slam_family_lookup" in _ffi.EXPORTED_SYMBOLS and hasattr(_ffi.Context, "family_lookup")
    if os.path.exists(_ffi.LIB_PATH):
        assert hasattr(_ffi.load_library(), "slam_family_lookup")


def test_family_lookup_refuses_malformed_families_before_any_context():
    fam = family("iswap", 4, 16)
    ctx = object.__new__(_ffi.Context)  # no library handle, no device: every call below must raise before it would be needed
    ok = (fam.tables, fam.child_even, fam.child_odd, fam.durations)

    def call(tables=ok[0], even=ok[1], odd=ok[2], dur=ok[3], cost_1q=0.1, policy="reference"):
        return _ffi.Context.family_lookup(ctx, tables, even, odd, dur, cost_1q, policy)

    with pytest.raises(ValueError, match="1..32 members"):
        call(tables=[])
    with pytest.raises(ValueError, match="1..32 members"):
        call(tables=[fam.table(0)] * 33, even=[-1] * 33, odd=[-1] * 33, dur=[1.0] * 33)
    with pytest.raises(ValueError, match="child_even must have one entry per member"):
        call(even=fam.child_even[:-1])
    with pytest.raises(ValueError, match="durations must have one entry per member"):
        call(dur=fam.durations[:2])
    with pytest.raises(ValueError, match=r"child_even\[1\] = 1"):  # a member as its own child
        call(even=[1, 1, -1, -1])
    with pytest.raises(ValueError, match=r"child_odd\[2\] = 0"):  # a link back to the base
        call(odd=[2, -1, 0, -1])
    with pytest.raises(ValueError, match=r"child_odd\[0\] = 4"):  # outside the family
        call(odd=[4, -1, -1, -1])
    with pytest.raises(ValueError, match="finite"):
        call(dur=[0.25, np.inf, 0.75, 1.0])
    with pytest.raises(ValueError, match="finite"):
        call(cost_1q=np.nan)
    with pytest.raises(ValueError, match="policy"):
        call(policy="cheapest")

    class Bad:
        kinds, points, bounds = np.zeros(2, np.int32), np.zeros((2, 3)), np.zeros((2, 14))

    with pytest.raises(ValueError, match="member 1: points must have shape"):
        call(tables=[fam.table(0), Bad, fam.table(2), fam.table(3)])
    # a well-formed family reaches the library call (there is no handle here)
    with pytest.raises(AttributeError):
        call()
    args = _ffi.family_arguments(*ok, 0.1, "best")
    assert args[0].tolist() == [0, 16, 19, 25, 28] and args[-1] == _ffi.POLICY_BEST and args[1].dtype == np.int32
    if os.path.exists(_ffi.LIB_PATH):  # the library's own checks need no device either
        lib = _ffi.load_library()
        cnt = np.zeros(64, dtype=np.int64)
        rc = lib.slam_family_lookup(None, 0, 0, 4, *[_ffi._ptr(a) for a in args[:7]], 0.1, 1e-7, 0, _ffi._ptr(cnt), _ffi._ptr(cnt), None, None)
        assert rc != 0 and "ctx is NULL" in lib.slam_last_error().decode()


def test_template_and_optimizer_refusals():
    from slam_decomposition_amd.cost_function import BasicCost, MakhlinFunctionalCost
    from slam_decomposition_amd.optimizer import TemplateOptimizer

    tpl = fe.FamilyExtendedTemplate(iswap_root(4), max_gates=16)
    assert tpl.gate_matrices.shape == (4, 4, 4) and tpl.policy == "reference" and tpl.family.max_gates == 16
    assert list(tpl.get_spanning_range(CX)) == [2] and tpl.gate_sequence(2) == [1, 1]  # sqrt(iSWAP) is member 1
    assert list(tpl.get_spanning_range(np.eye(4))) == [0]
    member = tpl.member_template(2)
    assert np.allclose(c1c2c3(member.gate_matrices[0]), [0.25, 0.25, 0]) and len(member.base_gates) == 1
    with pytest.raises(ValueError, match="no member x5"):
        tpl.member_template(5)
    with pytest.raises(ValueError, match="policy"):
        fe.FamilyExtendedTemplate(iswap_root(4), policy="cheapest")
    TemplateOptimizer(basis=tpl, objective=BasicCost())
    for kwargs in ({"use_callback": True}, {"override_method": "Nelder-Mead"}):
        with pytest.raises(NotImplementedError, match="FamilyExtendedTemplate"):
            TemplateOptimizer(basis=tpl, objective=BasicCost(), **kwargs)
    with pytest.raises(NotImplementedError, match="FamilyExtendedTemplate"):
        TemplateOptimizer(basis=tpl, objective=MakhlinFunctionalCost())
