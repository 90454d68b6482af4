"""GPU: slam_family_lookup against the host lookup (GateFamily.lookup), its histograms and reproducible totals, edge rows, the
fitting of the chosen sibling circuits (FamilyExtendedTemplate through TemplateOptimizer) and family_sweep.

Margins.  A target within rounding of a region face may fall either way on the two sides (they add the same numbers in a different
order): the per-target comparison leaves out targets whose host answer changes when every region is widened or shrunk by 2e-7 --
on the CPU, 1 or 2 of 20 000 SciPy Haar targets for each family and policy used here (cap: 0.5 %).  The fitting test leaves out
targets within 2e-4 of a face of any member (a circuit that has to reach the very boundary of its region converges slowly): 0 of
256 SciPy Haar targets on the CPU (cap: 2 %)."""
import logging

import numpy as np
import pytest

from slam_decomposition_amd import _ffi, family_extend as fe, pulse_cost
from slam_decomposition_amd.cost_function import BasicCost
from slam_decomposition_amd.gates import BerkeleyGate, ConversionGainGate
from slam_decomposition_amd.optimizer import TemplateOptimizer
from slam_decomposition_amd.sampler import DeviceHaarBatch

pytestmark = pytest.mark.gpu

PI = np.pi
CX = np.array([[1, 0, 0, 0], [0, 0, 0, 1], [0, 0, 1, 0], [0, 1, 0, 0]], dtype=np.complex128)
SWAP = np.array([[1, 0, 0, 0], [0, 0, 1, 0], [0, 1, 0, 0], [0, 0, 0, 1]], dtype=np.complex128)
MARGIN = 2e-7


def iswap_root(n):
    return ConversionGainGate(0, 0, PI / 2, 0, 1 / n)


def u3(t, p, l):
    return np.array([[np.cos(t / 2), -np.exp(1j * l) * np.sin(t / 2)], [np.exp(1j * p) * np.sin(t / 2), np.exp(1j * (p + l)) * np.cos(t / 2)]])


FAMILIES = {
    "iswap^(1/4)": lambda: fe.GateFamily(iswap_root(4), cost_1q=0.1, max_gates=16),
    "iswap^(1/6), 9 gates": lambda: fe.GateFamily(iswap_root(6), cost_1q=0.1, max_gates=9),
    "cx^(1/4)": lambda: fe.GateFamily(ConversionGainGate(0, 0, PI / 4, PI / 4, 1 / 4), cost_1q=0.1, max_gates=16),
}
_BUILT = {}


def family(name):
    if name not in _BUILT:
        _BUILT[name] = FAMILIES[name]()
    return _BUILT[name]


@pytest.fixture(scope="module")
def haar(hip_ctx):
    """20 000 device Haar targets and the coordinates the kernels compute for them (8 digits), read back once."""
    n = 20000
    sampler = DeviceHaarBatch(seed=20261019, n_samples=n)
    sampler.fill(hip_ctx)
    return sampler, hip_ctx.targets_c1c2c3(0, n)


def _bins(fam, member, gates):
    """Per-target outputs -> the bins of counts_out (rows in member order, then local, then unreachable)."""
    off = np.concatenate([[0], np.cumsum([len(t) for t in fam.tables])])
    E = int(off[-1])
    return np.where(gates > 0, off[np.maximum(member, 0)] + gates - 1, np.where(gates == 0, E, E + 1)), E


@pytest.mark.parametrize("policy", fe.POLICIES)
@pytest.mark.parametrize("name", list(FAMILIES))
def test_device_lookup_equals_the_host_lookup(hip_ctx, haar, name, policy):
    sampler, coords = haar
    n = len(coords)
    fam = family(name)
    sampler.fill(hip_ctx)
    counts, base_counts, member, gates = fam.device_lookup(hip_ctx, policy, want_targets=True)
    want = fam.lookup(coords, policy)
    wide, narrow = fam.lookup(coords, policy, tol=pulse_cost.TOL + MARGIN), fam.lookup(coords, policy, tol=pulse_cost.TOL - MARGIN)
    clear = (wide.member == narrow.member) & (wide.gates == narrow.gates)
    print(f"{name} / {policy}: {int((~clear).sum())} of {n} targets within {MARGIN} of a face; "
          f"{int(((member != want.member) | (gates != want.gates)).sum())} differ in all")
    assert (~clear).sum() <= 0.005 * n
    assert np.array_equal(member[clear], want.member[clear]) and np.array_equal(gates[clear], want.gates[clear])
    assert len(np.unique(member)) >= 2 and np.all(gates > 0)  # several members win; Haar targets are neither local nor out of reach
    # the histograms: exactly the per-target outputs, and member 0's alone exactly what the coverage lookup of its table says
    bins, E = _bins(fam, member, gates)
    assert counts.shape == (E + 2,) and np.array_equal(counts, np.bincount(bins, minlength=E + 2)) and counts.sum() == n
    alone, _ = hip_ctx.coverage_lookup([fam.table(0)], tol=pulse_cost.TOL)
    assert np.array_equal(base_counts, alone[0])
    # reproducible; a window; no per-target outputs asked for
    c2, b2, m2, g2 = fam.device_lookup(hip_ctx, policy, want_targets=True)
    assert np.array_equal(c2, counts) and np.array_equal(b2, base_counts) and np.array_equal(m2, member) and np.array_equal(g2, gates)
    c3, b3, m3, g3 = fam.device_lookup(hip_ctx, policy, first=1000, count=3000, want_targets=True)
    assert np.array_equal(m3, member[1000:4000]) and np.array_equal(g3, gates[1000:4000]) and c3.sum() == b3.sum() == 3000
    c4, b4, m4, g4 = fam.device_lookup(hip_ctx, policy)
    assert m4 is None and g4 is None and np.array_equal(c4, counts) and np.array_equal(b4, base_counts)
    # the total: integer counts times the rows' costs, in row order -- to the last bit the host's sum of per-target costs in that order
    costs = fam.row_costs()
    total = fe._ordered_sum(counts[:E], costs)
    by_row = 0.0
    for e in range(E):
        by_row += int((bins == e).sum()) * float(costs[e])
    assert total == by_row
    assert np.array_equal(costs[bins[gates > 0]], (gates + 1) * fam.cost_1q + gates * fam.durations[member])  # the cost each target was given
    if policy == "best":
        ref_counts, _, _, _ = fam.device_lookup(hip_ctx, "reference")
        assert total <= fe._ordered_sum(ref_counts[:E], costs)
    assert total < fe._ordered_sum(base_counts[: len(fam.table(0))], costs[: len(fam.table(0))])  # the family pays


def test_edge_rows(hip_ctx):
    fam = family("iswap^(1/4)")
    rng = np.random.default_rng(7)
    loc = [np.kron(u3(*rng.uniform(0, 2 * PI, 3)), u3(*rng.uniform(0, 2 * PI, 3))) for _ in range(3)]
    special = [np.eye(4), loc[0], loc[1], CX, SWAP, BerkeleyGate().to_matrix(), iswap_root(4).to_matrix(), loc[2] @ iswap_root(2).to_matrix(),
               iswap_root(1).to_matrix() @ loc[0], -1j * np.eye(4), np.exp(0.3j) * CX]
    DeviceHaarBatch(seed=3, n_samples=257).fill(hip_ctx)  # one block and one lane
    T = hip_ctx.get_targets(0, 257)
    T[: len(special)] = np.stack(special)
    T[256] = SWAP  # the lane of the second block
    hip_ctx.set_targets(T)
    coords = hip_ctx.targets_c1c2c3(0, 257)
    for policy in fe.POLICIES:
        counts, base_counts, member, gates = fam.device_lookup(hip_ctx, policy, want_targets=True)
        want = fam.lookup(coords, policy)
        assert np.array_equal(member, want.member) and np.array_equal(gates, want.gates), policy
        r = np.where(member >= 0, fam.multipliers[np.maximum(member, 0)], 0)
        # identity, two local gates | CX, SWAP: sqrt(iSWAP) x 2, x 3 | B: sqrt(iSWAP) x 2 | the base gate's own class, a sibling's, iSWAP's
        assert list(zip(r[:9].tolist(), gates[:9].tolist())) == [(0, 0), (0, 0), (0, 0), (2, 2), (2, 3), (2, 2), (1, 1), (2, 1), (4, 1)]
        assert (r[9], gates[9]) == (0, 0) and (r[10], gates[10]) == (2, 2) and (r[256], gates[256]) == (2, 3)  # global phases
        bins, E = _bins(fam, member, gates)
        assert np.array_equal(counts, np.bincount(bins, minlength=E + 2)) and counts[E] == 4 and counts[E + 1] == 0
        assert base_counts[len(fam.table(0))] == 4 and base_counts.sum() == 257
        # a window that starts inside the first block and ends with the last lane
        c2, b2, m2, g2 = fam.device_lookup(hip_ctx, policy, first=5, count=252, want_targets=True)
        assert np.array_equal(m2, member[5:]) and np.array_equal(g2, gates[5:]) and c2.sum() == 252 and c2[E] == 1
    # out of reach: six applications of iSWAP^(1/8) reach neither CX (8) nor SWAP (12), siblings or not
    weak = fe.GateFamily(iswap_root(8), max_gates=6)
    for policy in fe.POLICIES:
        counts, base_counts, member, gates = weak.device_lookup(hip_ctx, policy, want_targets=True)
        want = weak.lookup(coords, policy)
        assert np.array_equal(member, want.member) and np.array_equal(gates, want.gates)
        assert gates[3] == gates[4] == gates[256] == -1 and member[3] == member[4] == -1 and gates[0] == 0 and gates[6] > 0
        assert counts[-1] == (gates < 0).sum() >= 3 and base_counts[-1] == counts[-1] and counts.sum() == 257
        with pytest.raises(ValueError, match="Monodromy did not find a polytope containing U.*max_gates = 6"):
            fe.family_cost_from_distribution(weak, list(T[:8]), policy)
    # the library's own argument checks
    with pytest.raises(_ffi.SlamHipError, match="target window"):
        fam.device_lookup(hip_ctx, first=10, count=250)
    lib = _ffi.load_library()
    args = list(_ffi.family_arguments(fam.tables, fam.child_even, fam.child_odd, fam.durations, 0.1, "reference"))
    cnt, cnt0 = np.zeros(int(args[0][-1]) + 2, dtype=np.int64), np.zeros(int(args[0][1]) + 2, dtype=np.int64)

    def raw(n_members=len(fam), even=args[4], dur=args[6], policy=0):
        a = [args[0], args[1], args[2], args[3], even, args[5], dur]
        return lib.slam_family_lookup(hip_ctx._h, 0, 257, n_members, *[_ffi._ptr(np.ascontiguousarray(x)) for x in a], 0.1, 1e-7, policy,
                                      _ffi._ptr(cnt), _ffi._ptr(cnt0), None, None)

    assert raw() == 0
    for kwargs, msg in (({"n_members": 0}, "n_members"), ({"n_members": 33}, "n_members"), ({"policy": 2}, "policy"),
                        ({"even": np.array([0, 3, -1, -1], dtype=np.int32)}, "child_even"),
                        ({"dur": np.array([0.25, np.nan, 0.75, 1.0])}, "durations")):
        assert raw(**kwargs) == -1 and msg in lib.slam_last_error().decode(), kwargs


def test_cost_from_distribution(caplog):
    fam = family("iswap^(1/6), 9 gates")
    sampler = DeviceHaarBatch(seed=9, n_samples=4096)
    with caplog.at_level(logging.INFO):
        res = fe.family_cost_from_distribution(fam, sampler)
    msgs = [r.getMessage() for r in caplog.records]
    assert f"Total circuit pulse cost: {res.total}" in msgs and f"Average gate pulse cost: {res.total / 4096}" in msgs
    assert res.n == 4096 and res.average == res.total / 4096 and res.base_average == res.base_total / 4096
    assert sum(c for _, _, c in res.counts) + res.local_count == 4096 and sum(c for _, c in res.base_counts) + res.local_count == 4096
    assert [(r, k) for r, k, _ in res.counts] == fam.rows()
    s = 0.0
    for (r, k, c) in res.counts:
        s += c * fam.own_cost(fam.member_index(r), k)
    assert s == res.total and res.total < res.base_total
    best = fe.family_cost_from_distribution(fam, sampler, policy="best")
    assert best.total < res.total and best.base_total == res.base_total  # CX-like targets: x3 beats the walk's x2
    assert fe.family_cost_from_distribution(fam, sampler) == res  # reproducible
    # the base curve is what cost_from_distribution gives for the base gate's own template (sum of gate costs) plus the 1Q layers
    caplog.clear()
    with caplog.at_level(logging.INFO):
        empty = fe.family_cost_from_distribution(fam, DeviceHaarBatch(seed=9, n_samples=0))
    assert empty.total == 0.0 and empty.n == 0 and not any("Average gate pulse cost" in r.getMessage() for r in caplog.records)
    # a host sampler is uploaded once; its total is the host lookup's
    from slam_decomposition_amd.sampler import HaarBatch

    targets = list(HaarBatch(seed0=123, n_samples=40))
    host = fam.lookup_unitaries(np.stack(targets))
    assert abs(fe.family_cost_from_distribution(fam, targets).total - host.cost.sum()) < 1e-9


def _clear_of_all_faces(fam, coords, margin):
    wide = np.array([fam.first_k(m, coords, pulse_cost.TOL + margin) for m in range(len(fam))])
    narrow = np.array([fam.first_k(m, coords, pulse_cost.TOL - margin) for m in range(len(fam))])
    return np.all(wide == narrow, axis=0)


def test_the_chosen_siblings_reach_their_targets():
    """The claim the feature rests on: the looked-up (member, k) circuits really fit."""
    basis = fe.FamilyExtendedTemplate(iswap_root(4), cost_1q=0.1, max_gates=16)
    fam = basis.family
    n = 256
    sampler = DeviceHaarBatch(seed=424242, n_samples=n)
    opt = TemplateOptimizer(basis=basis, objective=BasicCost(), training_restarts=32, seed=11, override_fail=True)
    loss, _, data = opt.approximate_from_distribution(sampler)
    T = sampler.as_array()
    coords = fe.fam_coords(T)
    want = fam.lookup(coords)
    clear = _clear_of_all_faces(fam, coords, 2e-4)
    print(f"{int((~clear).sum())} of {n} targets within 2e-4 of a face; worst loss among the others {np.max(np.asarray(loss)[clear]):.3e}; "
          f"(r, k) used: {sorted(set(zip(opt.family_members.tolist(), [int(e.cycles) for e in data])))}")
    assert (~clear).sum() <= 0.02 * n
    cycles = np.array([e.cycles for e in data])
    assert np.array_equal(cycles[clear], want.gates[clear])
    assert np.array_equal(opt.family_members[clear], fam.multipliers[want.member[clear]])
    assert np.array_equal(opt.family_costs[clear], want.cost[clear])
    assert np.all(np.asarray(loss)[clear] < opt.success_threshold)
    assert all(len(e.Xk) == 6 * (e.cycles + 1) for e in data) and all(e.success_label == 1 for e, c in zip(data, clear) if c)
    assert len(set(opt.family_members.tolist())) >= 2
    cost = BasicCost()
    for i in np.nonzero(clear)[0][:10]:
        tpl = basis.member_template(int(opt.family_members[i]))
        tpl.build(int(data[i].cycles))
        assert cost.unitary_fidelity(tpl.eval(data[i].Xk), T[i]) < opt.success_threshold, i
    # the template is left at the last target's member and size
    assert basis.cycles == cycles[-1] and basis.gate_sequence() == [fam.member_index(int(opt.family_members[-1]))] * int(cycles[-1])


def test_weak_base_gate_named_targets_are_fitted_with_siblings():
    """iSWAP^(1/8) alone needs 8 gates for CX and 12 for SWAP; its family fits them as sqrt(iSWAP) x 2 and x 3."""
    basis = fe.FamilyExtendedTemplate(iswap_root(8), cost_1q=0.1, max_gates=12)
    assert basis.family.first_k(0, fe.fam_coords(np.stack([CX, SWAP]))).tolist() == [8, 12]
    opt = TemplateOptimizer(basis=basis, objective=BasicCost(), training_restarts=32, seed=5)
    for U, k in ((CX, 2), (SWAP, 3)):
        e = opt.approximate_target_U(U)
        assert e.cycles == k and e.success_label == 1 and e.loss_result < opt.success_threshold
        assert opt.family_members.tolist() == [4] and abs(opt.family_costs[0] - ((k + 1) * 0.1 + k * 0.5)) < 1e-12
        tpl = basis.member_template(4)
        tpl.build(k)
        assert BasicCost().unitary_fidelity(tpl.eval(e.Xk), U) < opt.success_threshold
    with pytest.raises(ValueError):
        opt.approximate_target_U(np.eye(4))  # a local target, as the mixed-order path
    far = fe.FamilyExtendedTemplate(iswap_root(8), max_gates=6)
    with pytest.raises(ValueError, match="Monodromy did not find a polytope containing U"):
        TemplateOptimizer(basis=far, objective=BasicCost()).approximate_target_U(SWAP)
    # without a 1Q cost every sibling ties with the base gate and loses: SWAP stays at 24 base gates, beyond the optimizer kernels
    deep = fe.FamilyExtendedTemplate(iswap_root(16), cost_1q=0.0, max_gates=24)
    with pytest.raises(NotImplementedError, match="template spans up to 16"):
        TemplateOptimizer(basis=deep, objective=BasicCost()).approximate_target_U(SWAP)


class _CountingBatch(DeviceHaarBatch):
    fills = 0

    def fill(self, ctx, first=0, count=None):
        self.fills += 1
        super().fill(ctx, first, count)


def test_family_sweep():
    sampler = _CountingBatch(seed=31, n_samples=4096)
    sweep = fe.family_sweep([iswap_root(2), iswap_root(4), iswap_root(6)], sampler, cost_1q=0.1, max_gates=16)
    assert sampler.fills == 1 and sweep.n == 4096  # the batch was generated once for the three base gates
    assert np.allclose(sweep.fractions, [1 / 2, 1 / 4, 1 / 6])
    for fam, base in zip(sweep.fam_haar, sweep.no_fam_haar):
        assert fam <= base
    assert sweep.fam_haar[1] < sweep.no_fam_haar[1] and sweep.fam_haar[2] < sweep.no_fam_haar[2]
    # the hand-worked table: D[CX], D[SWAP] with the family / with the base gate alone (n applications for CX, ceil(3n / 2) for SWAP)
    assert np.allclose(sweep.fam_cx, [1.3, 1.3, 1.4], rtol=0, atol=1e-12) and np.allclose(sweep.fam_swap, [1.9, 1.9, 1.9], rtol=0, atol=1e-12)
    assert np.allclose(sweep.no_fam_cx, [3 * 0.1 + 2 / 2, 5 * 0.1 + 4 / 4, 7 * 0.1 + 6 / 6], rtol=0, atol=1e-12)
    assert np.allclose(sweep.no_fam_swap, [4 * 0.1 + 3 / 2, 7 * 0.1 + 6 / 4, 10 * 0.1 + 9 / 6], rtol=0, atol=1e-12)
    # each entry is the single call's result on the same targets
    single = fe.family_cost_from_distribution(fe.GateFamily(iswap_root(4), cost_1q=0.1, max_gates=16), DeviceHaarBatch(seed=31, n_samples=4096))
    assert sweep.results[1] == single
    best = fe.family_sweep([iswap_root(6)], DeviceHaarBatch(seed=31, n_samples=4096), max_gates=16, policy="best")
    assert abs(best.fam_cx[0] - 1.3) < 1e-12 and best.fam_haar[0] <= sweep.fam_haar[2]
