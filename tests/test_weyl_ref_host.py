"""CPU: the 40-digit classification reference (tests/weyl_ref.py) and its fixture tests/golden/weyl_lookup_reference.npz.

  * the fixture is complete, within its size limit, and a sample of it is recomputed bit for bit;
  * the reference maps CAN(c), built from the closed form at 40 digits, back to c on a grid of the chamber and its boundary;
  * the NumPy ports pass the assertions the GPU test makes of the kernels: ``oracle.c1c2c3_jacobi_port`` (coordinates),
    ``test_pulse_cost_host.table_lookup``, ``coverage.minimal_prefix`` and the parallel-drive host lookup (decisions);
  * the checks bite: four wrong stand-ins fail them.  Failure counts on the committed fixture (3 493 matrices, 3 145 of them decision
    targets), printed with ``-s`` and asserted from below:
        rounding to 7 digits                       3 272 coordinates unequal at 8 digits, 63 wrong decisions   (asserted: > 3 000, > 0)
        dropping the shift-1/2 alcove point        534 wrong lookups of 1 635                                  (asserted: > 300)
        dropping the mirrored hull part            294 wrong region rows of 1 510                              (asserted: > 100)
        a fold that skips the c3 < 0 mirror        556 coordinates off by more than 1e-13                      (asserted: > 300)
"""
import os

import numpy as np
import pytest

import hp_ref as hp
import test_pulse_cost_host as host
import weyl_ref as w
from oracle import slam_oracle as o
from slam_decomposition_amd import coverage
from slam_decomposition_amd import parallel_drive as pd

pytest.importorskip("mpmath")
mp = w.mp

GROUPS = w.load_fixture()
BANK = GROUPS[0]
MATRIX_GROUPS = [g for g in GROUPS[1:] if "x" not in g]
DECISION = {t: [g for g in GROUPS[1:] if g["meta"].get("type") == t] for t in ("coverage", "span", "region")}
_cache = {}


def _mats(g):
    return w.unitaries_of(g, BANK)


def _port(g, ndigits):
    key = (g["meta"]["name"], ndigits)
    if key not in _cache:
        _cache[key] = np.array([o.c1c2c3_jacobi_port(u, ndigits) for u in _mats(g)])
    return _cache[key]


def _coordinate_kinds(g):
    """The input kind of every case for the coordinate checks: a decision group is one kind, whatever its targets were placed for."""
    return np.array(["decision"] * len(g["ref"]) if "type" in g["meta"] else g["meta"]["kinds"])


def _e_ref_max(g, kind):
    if "e_ref" in g:
        return float(np.max(g["e_ref"][_coordinate_kinds(g) == kind]))
    return max(float.fromhex(v) for v in g["meta"]["e_ref_max"].values())


# ---- the fixture -------------------------------------------------------------------------------------------------------------------
def test_fixture_is_complete_and_small():
    names = [g["meta"]["name"] for g in GROUPS]
    for want in ("bank", "general", "named", "det-cut", "phase-edge", "drifted", "template"):
        assert want in names
    assert len(DECISION["coverage"]) == 3 and len(DECISION["span"]) == 5 and len(DECISION["region"]) == 2
    assert os.path.getsize(w.FIXTURE) <= os.path.getsize(hp.FIXTURE)
    for g in GROUPS[1:]:
        m = g["meta"]
        assert sum(m["made"].values()) == len(m["kinds"]) == len(g["ref"])
        for kind, made in m["made"].items():
            assert made > 0 and m["rejected"][kind] <= 0.1 * (made + m["rejected"][kind]), (m["name"], kind)
        if "type" in m:
            assert m["min_margin"] >= w.MARGIN and m["unplaced_sides"] <= 0.1 * 2 * (m["faces"] - m["faces_not_cutting_the_chamber"]), m["name"]
            assert "face" in m["made"] and "local" in m["made"]
            for kind in ("integer", "mirror"):  # left out only where every such class lies on a face of the table
                assert kind in m["made"] or (kind in m["skipped"] and m["type"] == "span"), (m["name"], kind)
            assert len(g["expect"]) == len(g["ref"])
    for g in DECISION["coverage"] + DECISION["region"]:
        assert "c2=c3=0" in g["meta"]["made"]
        assert "gate" in g["meta"]["made"] or ("gate" in g["meta"]["skipped"] and g["meta"]["type"] == "region"), g["meta"]["name"]


def test_tables_are_the_ones_the_package_builds():
    for n, g in enumerate(DECISION["coverage"]):
        t = host._template(*host.GATE_SETS[n]).coverage_table()
        assert np.array_equal(t.kinds, g["kinds"]) and np.array_equal(t.points, g["points"]) and np.array_equal(t.bounds, g["bounds"])
    for g in DECISION["span"]:
        gc = g["gcoords"]
        assert np.array_equal(coverage.alcove_coordinates(gc[:1])[0], g["point"])
        for k in range(2, len(gc) + 1):
            assert np.array_equal(coverage.region(gc[:k]), g["bounds"][k - 1])


def test_a_sample_is_recomputed_bit_for_bit():
    n = 0
    with mp.workdps(w.DPS):
        for g in MATRIX_GROUPS:
            U = _mats(g)
            step = 37 if "type" in g["meta"] else 17
            for i in range(len(U) // 2 % step, len(U), step):
                c = w.weyl_class(U[i])
                assert np.array_equal(hp.bits(np.array([float(x) for x in c])), hp.bits(g["ref"][i])), (g["meta"]["name"], i)
                t = g["meta"].get("type")
                if t == "coverage":
                    row, m = w.lookup(c, g["kinds"], g["points"], g["bounds"], 1e-7)
                    row = [row]
                elif t == "span":
                    r = [w.predict_span(c, g["point"], g["bounds"], tol) for tol in (2e-8, 5e-4)]
                    row, m = [x[0] for x in r], min(x[1] for x in r)
                elif t == "region":
                    flags, first, m = w.region_flags(c, g["ro"], g["kinds"], g["fo"], g["facets"], g["aux"], 1e-7)
                    row = [int(f) for f in flags] + [first]
                if t:
                    assert row == g["expect"][i].tolist() and m >= w.MARGIN, (g["meta"]["name"], i, row, m)
                n += 1
    assert n >= 90


def test_reference_on_closed_forms():
    """CAN(c) = prod_k (cos(pi c_k / 2) + i sin(pi c_k / 2) s_k (x) s_k) at 40 digits, rounded once: the reference returns c, up to the
    mirror on the c3 = 0 face, to 1e-15."""
    grid = [(a / 8, b / 8, c / 8) for a in range(0, 8) for b in range(0, 5) for c in range(0, 5) if b <= min(a, 8 - a) and c <= b]
    grid += [(0.3, 0.2, 0.1), (0.7, 0.2, 0.1), (0.45, 0.4, 0.39), (0.9, 0.05, 0.0), (0.5, 0.5, 0.5)]
    pauli = [[[0, 1], [1, 0]], [[0, -1j], [1j, 0]], [[1, 0], [0, -1]]]
    with mp.workdps(w.DPS):
        for c in grid:
            U = hp.eye()
            for ck, s in zip(c, pauli):
                ss = hp.kron([[w.mpc(z) for z in r] for r in s], [[w.mpc(z) for z in r] for r in s])
                ang = mp.pi * w.mpf(ck) / 2
                U = hp.mm(U, [[mp.cos(ang) * (i == j) + w.mpc(0, 1) * mp.sin(ang) * ss[i][j] for j in range(4)] for i in range(4)])
            got = np.array([[float(x) for x in w.weyl_class(hp.to_np(U))]])
            assert w.distance(got, np.array([c]))[0] < 1e-15, (c, got)
            assert w.chamber_violation(got)[0] < 1e-15


# ---- the NumPy ports under the GPU test's assertions --------------------------------------------------------------------------------
def test_jacobi_port_coordinates():
    for g in MATRIX_GROUPS:
        kinds = _coordinate_kinds(g)
        raw = _port(g, -1)
        d = w.distance(raw, g["ref"])
        for kind in sorted(set(kinds)):
            sel = kinds == kind
            assert d[sel].max() <= w.tolerance(_e_ref_max(g, kind)), (g["meta"]["name"], kind, d[sel].max())
        assert w.chamber_violation(raw).max() <= 1e-13
        r8 = _port(g, 8)
        assert w.rounded_equal(r8, g["ref"]).all(), g["meta"]["name"]
        assert w.chamber_violation(r8).max() <= 1e-15


def _coverage_port(g, coords, tol=1e-7):
    return host.table_lookup(w.Table(g["kinds"], g["points"], g["bounds"]), coords, tol)[:, None]


def _span_port(g, coords):
    gc = g["gcoords"]
    return np.stack([coverage.minimal_prefix(coords, gc, len(gc), tol=tol) for tol in (2e-8, 5e-4)], axis=1)


def _region_port(g, coords, drop_last_part=False):
    R = len(g["ro"]) - 1
    sums = coverage.target_sums(coords)
    flags = np.zeros((len(coords), R), dtype=np.int64)
    for r in range(R):
        parts = list(range(g["ro"][r], g["ro"][r + 1]))
        if drop_last_part and r < R // 2:  # the extended regions come first; their last part is the mirrored hull
            parts = parts[:-1]
        for p in parts:
            part = pd.Part(int(g["kinds"][p]), g["facets"][g["fo"][p]:g["fo"][p + 1]], g["aux"][p])
            flags[:, r] |= pd._part_contains(part, coords, sums, 1e-7)
    first = np.where(flags.any(axis=1), np.argmax(flags, axis=1), R)
    return np.concatenate([flags, first[:, None]], axis=1)


PORTS = {"coverage": _coverage_port, "span": _span_port, "region": _region_port}


def test_host_lookups_decide_as_the_reference():
    for t, groups in DECISION.items():
        for g in groups:
            got = PORTS[t](g, _port(g, 8))
            bad = np.nonzero(np.any(got != g["expect"], axis=1))[0]
            assert len(bad) == 0, (g["meta"]["name"], bad[:5], got[bad[:5]], g["expect"][bad[:5]], g["ref"][bad[:5]])


# ---- the checks bite ---------------------------------------------------------------------------------------------------------------
def test_rounding_to_seven_digits_fails():
    unequal = wrong = 0
    for g in MATRIX_GROUPS:
        unequal += int((~w.rounded_equal(_port(g, 7), g["ref"])).sum())
        t = g["meta"].get("type")
        if t:
            wrong += int(np.any(PORTS[t](g, _port(g, 7)) != g["expect"], axis=1).sum())
    print("7 digits: coordinates unequal", unequal, "wrong decisions", wrong)
    assert unequal > 3000 and wrong > 0


def test_dropping_the_second_alcove_point_fails():
    wrong = 0
    for g in DECISION["coverage"]:
        for c, want in zip(_port(g, 8), g["expect"][:, 0]):
            c = tuple(float(v) for v in c)
            wrong += w.lookup(c, g["kinds"], g["points"], g["bounds"], 1e-7, vw=w.views(c)[:1])[0] != want
    for g in DECISION["span"]:
        for c, want in zip(_port(g, 8), g["expect"]):
            c = tuple(float(v) for v in c)
            wrong += [w.predict_span(c, g["point"], g["bounds"], tol, vw=w.views(c)[:1])[0] for tol in (2e-8, 5e-4)] != want.tolist()
    print("shift 0 only: wrong lookups", wrong)
    assert wrong > 300


def test_dropping_the_mirrored_hull_fails():
    wrong = 0
    for g in DECISION["region"]:
        wrong += int(np.any(_region_port(g, _port(g, 8), drop_last_part=True) != g["expect"], axis=1).sum())
    print("no mirrored hull: wrong region flags", wrong)
    assert wrong > 100


def _fold_without_mirror(U):
    """weylchamber's recipe (LAPACK eigenvalues) with the ``c3 < 0`` mirror left out."""
    yy = np.kron([[0, -1j], [1j, 0]], [[0, -1j], [1j, 0]])
    ev = np.linalg.eigvals(U @ (yy @ U.T @ yy) / np.sqrt(complex(np.linalg.det(U))))
    two_s = np.angle(ev) / np.pi
    two_s = np.where(two_s <= -0.5, two_s + 2.0, two_s)
    S = np.sort(two_s / 2.0)[::-1]
    n = int(round(float(S.sum())))
    S = np.roll(S - np.r_[np.ones(n), np.zeros(4 - n)], -n)
    return [S[0] + S[1], S[0] + S[2], S[1] + S[2]]


def test_a_fold_without_the_mirror_fails():
    off = 0
    for g in MATRIX_GROUPS:
        got = np.array([_fold_without_mirror(u) for u in _mats(g)])
        off += int((w.distance(got, g["ref"]) > 1e-13).sum())
    print("no c3 < 0 mirror: coordinates off", off)
    assert off > 300
