"""GPU: the classification kernels against the 40-digit reference of tests/weyl_ref.py (fixture
tests/golden/weyl_lookup_reference.npz, made by tools/make_weyl_reference.py).

  * ``weyl_c1c2c3`` through slam_c1c2c3, slam_targets_c1c2c3 and slam_eval_c1c2c3: unrounded within 8 * max(e_ref) of the kind (never
    above 1e-13; e_ref = the LAPACK oracle's own error against the 40-digit point), modulo the c3 = 0 mirror only where
    |c3_ref| <= 5e-9, and in the chamber; at 8 digits equal to ``np.round(reference, 8)``.
  * slam_coverage_lookup, slam_predict_spans and slam_region_lookup: the decision the reference derives from the 40-digit class and
    the very arrays the kernel receives, on targets placed on both sides of every finite face (margin >= 3e-8: the decision does not
    depend on the 8-digit rounding) and at the special classes.

Every fixture case is asserted: no masks, no allowed disagreements.  One ``WEYL`` line per (path, kind) is printed (``-s``).
"""
import numpy as np
import pytest

import weyl_ref as w

pytestmark = pytest.mark.gpu

GROUPS = w.load_fixture()
BANK = GROUPS[0]
MATRIX_GROUPS = [g for g in GROUPS[1:] if "x" not in g]
DECISION = {t: [g for g in GROUPS[1:] if g["meta"].get("type") == t] for t in ("coverage", "span", "region")}
CHAMBER_TOL = 1e-13


def _coordinate_kinds(g):
    """The input kind of every case for the coordinate checks: a decision group is one kind, whatever its targets were placed for."""
    return np.array(["decision"] * len(g["ref"]) if "type" in g["meta"] else g["meta"]["kinds"])


def _e_ref_max(g, kind):
    if "e_ref" in g:
        return float(np.max(g["e_ref"][_coordinate_kinds(g) == kind]))
    return max(float.fromhex(v) for v in g["meta"]["e_ref_max"].values())


def _check_unrounded(path, g, got):
    kinds = _coordinate_kinds(g)
    d = w.distance(got, g["ref"])
    out = w.chamber_violation(got)
    for kind in sorted(set(kinds)):
        sel = kinds == kind
        tol = w.tolerance(_e_ref_max(g, kind))
        print(f"WEYL {path:<16s} {g['meta']['name']:<26s} {kind:<10s} worst {d[sel].max():.3g} tol {tol:.3g} outside {out[sel].max():.1g} cases {int(sel.sum())}")
        assert d[sel].max() <= tol, (path, g["meta"]["name"], kind, int(np.argmax(np.where(sel, d, -1))), d[sel].max(), tol)
        assert out[sel].max() <= CHAMBER_TOL, (path, g["meta"]["name"], kind, out[sel].max())


def _check_rounded(path, g, got):
    ok = w.rounded_equal(got, g["ref"])
    bad = np.nonzero(~ok)[0]
    print(f"WEYL {path:<16s} {g['meta']['name']:<26s} 8 digits   unequal {len(bad)} cases {len(ok)}")
    assert len(bad) == 0, (path, g["meta"]["name"], bad[:5], got[bad[:5]], g["ref"][bad[:5]])
    assert w.chamber_violation(got).max() <= 1e-15, (path, g["meta"]["name"])


def test_fixture_is_complete():
    names = [g["meta"]["name"] for g in GROUPS]
    for want in ("bank", "general", "named", "det-cut", "phase-edge", "drifted", "template"):
        assert want in names
    assert len(DECISION["coverage"]) == 3 and len(DECISION["span"]) == 5 and len(DECISION["region"]) == 2


@pytest.mark.parametrize("ndigits", [-1, 8])
def test_coordinates_of_matrices(hip_ctx, ndigits):
    check = _check_unrounded if ndigits < 0 else _check_rounded
    for g in MATRIX_GROUPS:
        U = w.unitaries_of(g, BANK)
        check("c1c2c3", g, hip_ctx.c1c2c3(U, ndigits=ndigits))
        hip_ctx.set_targets(U)
        res = hip_ctx.targets_c1c2c3(0, len(U), ndigits=ndigits)
        check("targets_c1c2c3", g, res)
        lo = len(U) // 3
        assert np.array_equal(hip_ctx.targets_c1c2c3(lo, len(U) - lo, ndigits=ndigits), res[lo:])  # a window of the batch


@pytest.mark.parametrize("ndigits", [-1, 8])
def test_coordinates_of_a_template(hip_ctx, ndigits):
    (g,) = [g for g in GROUPS[1:] if "x" in g]
    assert w.checksum(g["x"].astype(np.complex128)) == int(g["meta"]["checksum"])
    k = int(g["meta"]["span"])
    hip_ctx.set_targets(np.eye(4, dtype=complex)[None])
    hip_ctx.set_gates(g["gates"])
    got = hip_ctx.eval_c1c2c3([0] * k, g["x"], ndigits=ndigits)
    (_check_unrounded if ndigits < 0 else _check_rounded)("eval_c1c2c3", g, got)


def _report(path, g, got, want):
    kinds = np.array(g["meta"]["kinds"])
    got, want = np.asarray(got).reshape(len(kinds), -1), np.asarray(want).reshape(len(kinds), -1)
    wrong = np.any(got != want, axis=1)
    for kind in sorted(set(kinds)):
        sel = kinds == kind
        print(f"WEYL {path:<16s} {g['meta']['name']:<26s} {kind:<10s} wrong {int(wrong[sel].sum())} margin >= {g['meta']['min_margin']:.3g} cases {int(sel.sum())}")
    bad = np.nonzero(wrong)[0]
    assert len(bad) == 0, (path, g["meta"]["name"], bad[:8], kinds[bad[:8]], got[bad[:8]], want[bad[:8]], g["ref"][bad[:8]])


def test_coverage_lookup_entries(hip_ctx):
    """One launch over the three tables with every coverage target resident; a table's row is asserted on the targets that were
    placed -- and whose margin was computed -- for it.  Then each table alone on the window of its own targets."""
    groups = DECISION["coverage"]
    tables = [w.Table(g["kinds"], g["points"], g["bounds"]) for g in groups]
    mats = [w.unitaries_of(g, BANK) for g in groups]
    first = np.cumsum([0] + [len(m) for m in mats])
    hip_ctx.set_targets(np.concatenate(mats))
    counts, entries = hip_ctx.coverage_lookup(tables, want_entries=True, tol=1e-7)
    assert entries.shape == (3, first[-1])
    for t, g in enumerate(groups):
        assert np.array_equal(counts[t], np.bincount(entries[t], minlength=len(tables[t]) + 2))
        _report("coverage_lookup", g, entries[t, first[t]:first[t + 1]], g["expect"][:, 0])
        c1, e1 = hip_ctx.coverage_lookup([tables[t]], first=int(first[t]), count=len(mats[t]), want_entries=True, tol=1e-7)
        assert np.array_equal(e1[0], g["expect"][:, 0])
        assert np.array_equal(c1[0], np.bincount(g["expect"][:, 0], minlength=len(tables[t]) + 2))


def test_predict_spans(hip_ctx):
    from slam_decomposition_amd import coverage

    for g in DECISION["span"]:
        gc = g["gcoords"]
        # the arrays predict_spans sends are the ones the reference decided from
        assert np.array_equal(coverage.alcove_coordinates(gc[:1])[0], g["point"])
        for k in range(2, len(gc) + 1):
            assert np.array_equal(coverage.region(gc[:k]), g["bounds"][k - 1])
        U = w.unitaries_of(g, BANK)
        hip_ctx.set_targets(U)
        got = np.stack([hip_ctx.predict_spans(gc, len(gc), 0, len(U), tol=tol) for tol in (2e-8, 5e-4)], axis=1)
        _report("predict_spans", g, got, g["expect"])
        lo = len(U) // 2
        assert np.array_equal(hip_ctx.predict_spans(gc, len(gc), lo, len(U) - lo, tol=2e-8), g["expect"][lo:, 0])


def test_region_lookup_flags(hip_ctx):
    """Flags and the first containing region from single-target windows; the whole batch's counts are their sums."""
    for g in DECISION["region"]:
        U = w.unitaries_of(g, BANK)
        hip_ctx.set_targets(U)
        R = len(g["ro"]) - 1
        args = (g["ro"], g["kinds"], g["fo"], g["facets"], g["aux"])
        got = np.zeros((len(U), R + 1), dtype=np.int64)
        for i in range(len(U)):
            c = hip_ctx.region_lookup(*args, i, 1, tol=1e-7)
            assert c[R:].sum() == 1 and np.all((c[:R] == 0) | (c[:R] == 1))
            got[i, :R] = c[:R]
            got[i, R] = int(np.argmax(c[R:]))
        _report("region_lookup", g, got, g["expect"])
        whole = hip_ctx.region_lookup(*args, 0, len(U), tol=1e-7)
        assert np.array_equal(whole[:R], g["expect"][:, :R].sum(axis=0))
        assert np.array_equal(whole[R:], np.bincount(g["expect"][:, R], minlength=R + 1))
