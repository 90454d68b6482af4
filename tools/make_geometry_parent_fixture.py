"""Dev tool (GPU): the outputs that tests/test_gpu_geometry_paths.py pins, and -- run as a script at the PARENT commit -- the fixture
tests/golden/geometry_parent.npz they are compared with.  The refactor behind it ("Geometry lookups", HISTORY.md) gives the lookup
kernels of the geometry unit one target frame, one pair of row tests and one histogram fold, and its entry points one buffer carver
and one window check: every array, and every refusal, has to come out as the commit before it gave it.

    python tools/make_geometry_parent_fixture.py [out.npz]     (SLAM_HIP_LIB honoured)

Unless a case says otherwise the resident batch is 515 device Haar targets (two full blocks of 256 and a 3-lane tail) in which the
identity, CX, SWAP, sqrt(iSWAP), iSWAP and -i CX replace lanes of all three blocks, so that the local bin and the one-gate rows have hits.
  coverage        one call, three tables, with per-target entries: kind-0 and kind-1 rows mixed; an empty table; a table of 8192 kind-0
                  rows that match nothing and a last kind-1 row of -inf bounds at index 8192 -- its hit, the local and the unreachable
                  bin lie beyond the 8192 bins of the LDS histogram and are counted in global memory directly
  family          iswap^(1/6) with at most 6 gates (members x1 x2 x3 x4 x6: member 0 has an even and an odd child; some targets are out
                  of reach, and the two policies choose differently), both policies, with member_out / gates_out
  candidates      the 41 gates of candidate_grid(9, 9): k_cap 64 and 2 with first_k; 3 groups (k_cap 8); and, counts only, the 2131 gates
                  of candidate_grid(65, 65) against 16 387 Haar targets with k_cap 4 -- 65 target blocks, so 32 chunks of
                  ceil(2131 / 32) = 67 candidates (the formula of slam_candidate_scores, asserted below): three LDS tiles per block
  region          three regions over five polytopes of all three kinds; regions 0 and 2 are unions of two
  predict_spans   sqrt(iSWAP) x 4: k_max 1 and 4, tol 0 and 1e-6
  haar_select_spans   1000 candidates (four blocks, the last partial), spans 2..2 of sqrt(iSWAP) x 3: margin 0, 1e-6 and 1e-3 (which
                  turns candidates away), a capacity below the number selected, span_counts
  pd              pd_sample of 300 samples (k = 2, 2 slices), a replay by `indices` with all three outputs, pd_extremes, pd_filter
                  (survivors sorted by index, as the binding returns them)
  c1c2c3          targets_c1c2c3, targets_kak and get_targets on the window [3, 403)
  refuse          per entry point of the unit that takes a window, a table or staging: a bad window, a NULL output and a malformed table
                  (where it has one) -- `refuse.<entry>.<what>` holds SlamHipError.code and the message's bytes
"""
import os
import sys
from types import SimpleNamespace

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

N_TARGETS, SEED, TOL = 515, 20261020, 1e-7
SPECIAL_LANES = [0, 1, 255, 256, 511, 512, 514]
N_BIG, BIG_GRID, BIG_CHUNK = 16387, (65, 65), 67
WINDOW = (3, 400)
PD = dict(gc=0.7, gg=0.3, t=1.0, n_slices=2, k=2)


def _special():
    from oracle import slam_oracle as o

    cx = o.cx_matrix()
    swap = np.array([[1, 0, 0, 0], [0, 0, 1, 0], [0, 1, 0, 0], [0, 0, 0, 1]], dtype=np.complex128)
    return [np.eye(4, dtype=np.complex128), cx, swap, o.riswap_matrix(0.5), o.riswap_matrix(1.0), -1j * cx, np.eye(4, dtype=np.complex128)]


def resident_batch(ctx):
    ctx.sample_haar(SEED, N_TARGETS)
    T = ctx.get_targets(0, N_TARGETS).copy()
    for lane, u in zip(SPECIAL_LANES, _special()):
        T[lane] = u
    ctx.set_targets(T)


def _table(kinds, points, bounds):
    return SimpleNamespace(kinds=np.asarray(kinds, dtype=np.int32), points=np.asarray(points, dtype=np.float64).reshape(-1, 4),
                           bounds=np.asarray(bounds, dtype=np.float64).reshape(-1, 14))


def _refusal(out, key, call):
    from slam_decomposition_amd import _ffi

    try:
        _ffi._check(call())
    except _ffi.SlamHipError as e:
        out[f"refuse.{key}"] = np.concatenate([np.array([e.code], dtype=np.int64),
                                               np.frombuffer(str(e).encode("utf-8"), dtype=np.uint8).astype(np.int64)])
        return
    raise AssertionError(f"{key}: the call was not refused")


def run_cases(ctx) -> dict:
    """Every pinned array, keyed '<case>.<name>'."""
    import ctypes as C

    from oracle import slam_oracle as o
    from slam_decomposition_amd import _ffi, candidates as cd, coverage, family_extend as fe
    from slam_decomposition_amd.gates import ConversionGainGate
    from slam_decomposition_amd.weyl import c1c2c3

    out = {}
    sq, cx = np.asarray(c1c2c3(o.riswap_matrix(0.5))), np.asarray(c1c2c3(o.cx_matrix()))
    point = lambda c: coverage.alcove_coordinates(np.asarray(c)[None])[0]
    ninf = np.full(14, -np.inf)
    resident_batch(ctx)

    # ---- coverage
    mixed = _table([0, 0, 1, 1], [point(cx), point(sq), np.zeros(4), np.zeros(4)], [ninf, ninf, coverage.region([sq] * 2), coverage.region([sq] * 3)])
    empty = _table([], np.zeros((0, 4)), np.zeros((0, 14)))
    n0 = 8192
    far = _table([0] * n0 + [1], np.concatenate([9.0 + np.arange(4 * n0, dtype=np.float64).reshape(n0, 4), np.zeros((1, 4))]),
                 np.full((n0 + 1, 14), -np.inf))
    counts, entries = ctx.coverage_lookup([mixed, empty, far], want_entries=True, tol=TOL)
    out["coverage.counts"], out["coverage.entries"] = np.concatenate(counts), entries

    # ---- family
    fam = fe.GateFamily(ConversionGainGate(0, 0, np.pi / 2, 0, 1 / 6), cost_1q=0.1, max_gates=6)
    assert fam.child_even[0] > 0 and fam.child_odd[0] > 0
    for policy in fe.POLICIES:
        r = fam.device_lookup(ctx, policy, want_targets=True)
        for name, a in zip(("counts", "base_counts", "member", "gates"), r):
            out[f"family.{policy}.{name}"] = a

    # ---- candidates
    coords = cd.gate_coords(cd.candidate_grid(9, 9)[0])
    out["candidates.coords"] = coords
    for k_cap in (64, 2):
        out[f"candidates.k{k_cap}.counts"], out[f"candidates.k{k_cap}.first_k"] = ctx.candidate_scores(coords, k_cap, want_first=True, tol=TOL)
    out["candidates.groups.counts"], _ = ctx.candidate_scores(coords, 8, groups=np.arange(N_TARGETS) % 3, n_groups=3, tol=TOL)

    # ---- region: polytopes 0 (facets) + 1 (CX's class) | 2 (two sqrt(iSWAP)) | 3 (facets) + 4 (two CX)
    facets = np.array([[1, 0, 0, 0.4], [0, -1, 0, -0.1], [0, 0, 1, 0.05], [1, 1, 1, 0.6]], dtype=np.float64)
    aux = np.zeros((5, 14))
    aux[1, :4], aux[2], aux[4] = point(cx), coverage.region([sq] * 2), coverage.region([cx] * 2)
    out["region.counts"] = ctx.region_lookup([0, 2, 3, 5], [0, 2, 1, 0, 1], [0, 2, 2, 2, 4, 4], facets, aux, tol=TOL)

    # ---- predict_spans
    for k_max in (1, 4):
        for tol in (0.0, 1e-6):
            out[f"predict_spans.k{k_max}.tol{tol:g}"] = ctx.predict_spans([sq] * 4, k_max, tol=tol)

    # ---- haar_select_spans
    for name, margin, cap in (("margin0", 0.0, 1000), ("margin", 1e-6, 1000), ("wide", 1e-3, 1000), ("capped", 0.0, 10)):
        idx, n_sel, span_counts = ctx.haar_select_spans(SEED, 5, 1000, [sq] * 3, 3, 2, 2, cap, margin=margin)
        assert n_sel > 10
        out[f"haar_select_spans.{name}.indices"], out[f"haar_select_spans.{name}.span_counts"] = idx, span_counts
        out[f"haar_select_spans.{name}.n_selected"] = np.array([n_sel], dtype=np.int64)

    # ---- pd
    replay = np.array([0, 17, 299, 150, 17], dtype=np.int64)
    c, p, u = ctx.pd_sample(n_samples=0, seed=3, indices=replay, want_coords=True, want_params=True, want_unitaries=True, **PD)
    out["pd.replay.coords"], out["pd.replay.params"], out["pd.replay.unitaries"] = c, p, np.ascontiguousarray(u).view(np.float64)
    out["pd.coords"], _, _ = ctx.pd_sample(n_samples=300, seed=3, want_coords=True, **PD)
    dirs = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, 0, 1], [1, 1, 1], [1, -1, 0.5], [0, 0, 0]], dtype=np.float64)
    out["pd.extremes.indices"], out["pd.extremes.coords"] = ctx.pd_extremes(dirs)
    out["pd.filter.indices"], out["pd.filter.coords"] = ctx.pd_filter(np.array([[1, 0, 0, 0.3], [0, 1, 0, 0.2]], dtype=np.float64), capacity=300)

    # ---- c1c2c3: a window that is not at 0
    first, count = WINDOW
    out["c1c2c3.coords"] = ctx.targets_c1c2c3(first, count)
    for name, a in zip(_ffi.KakResult._fields, ctx.targets_kak(first, count)):
        out[f"c1c2c3.kak.{name}"] = np.ascontiguousarray(a).view(np.float64)
    out["c1c2c3.targets"] = np.ascontiguousarray(ctx.get_targets(first, count)).view(np.float64)

    # ---- refusals, through the C entry points themselves
    lib, h, P = ctx._lib, ctx._h, _ffi._ptr
    i32, f64, i64 = (lambda *v: np.array(v, dtype=np.int32)), (lambda *v: np.array(v, dtype=np.float64)), (lambda n: np.zeros(n, dtype=np.int64))
    n = N_TARGETS
    buf = np.zeros(64 * n)
    off, kinds, pts, bds = i32(0, 1), i32(1), np.zeros((1, 4)), np.full((1, 14), -np.inf)
    m64 = C.c_int64(0)
    ms = C.c_double(0.0)
    _refusal(out, "targets_kak.window", lambda: lib.slam_targets_kak(h, 1, n, *[P(buf)] * 6))
    _refusal(out, "targets_kak.null", lambda: lib.slam_targets_kak(h, 0, n, P(buf), None, P(buf), P(buf), P(buf), P(buf)))
    _refusal(out, "targets_c1c2c3.window", lambda: lib.slam_targets_c1c2c3(h, -1, 2, 8, P(buf)))
    _refusal(out, "targets_c1c2c3.null", lambda: lib.slam_targets_c1c2c3(h, 0, n, 8, None))
    _refusal(out, "get_targets.window", lambda: lib.slam_get_targets(h, n, 1, P(buf)))
    _refusal(out, "get_targets.null", lambda: lib.slam_get_targets(h, n, 1, None))  # (its NULL check comes first)
    _refusal(out, "predict_spans.window", lambda: lib.slam_predict_spans(h, 0, n + 1, 1, P(f64(0, 0, 0, 0)), None, 0.0, P(buf)))
    _refusal(out, "predict_spans.null", lambda: lib.slam_predict_spans(h, 0, n, 1, P(f64(0, 0, 0, 0)), None, 0.0, None))
    _refusal(out, "predict_spans.table", lambda: lib.slam_predict_spans(h, 0, n, 2, P(f64(0, 0, 0, 0)), None, 0.0, P(buf)))
    cov = lambda first, count, off, kinds, counts: lib.slam_coverage_lookup(h, first, count, len(off) - 1, P(off), P(kinds), P(pts), P(bds), TOL,
                                                                            counts, None)
    _refusal(out, "coverage_lookup.window", lambda: cov(2, n - 1, off, kinds, P(i64(3))))
    _refusal(out, "coverage_lookup.null", lambda: cov(0, n, off, kinds, None))
    _refusal(out, "coverage_lookup.table_start", lambda: cov(0, n, i32(1, 2), kinds, P(i64(3))))
    _refusal(out, "coverage_lookup.table_order", lambda: cov(0, n, i32(0, 1, 0), kinds, P(i64(8))))
    _refusal(out, "coverage_lookup.table_kind", lambda: cov(0, n, off, i32(2), P(i64(3))))
    _refusal(out, "coverage_lookup.window_and_table", lambda: cov(0, n + 1, i32(1, 2), kinds, None))  # the first failing check wins
    none, dur = i32(-1), f64(1.0)
    famc = lambda first, count, off, kinds, child, counts: lib.slam_family_lookup(h, first, count, 1, P(off), P(kinds), P(pts), P(bds), P(child),
                                                                                 P(none), P(dur), 0.1, TOL, 0, counts, P(i64(3)), None, None)
    _refusal(out, "family_lookup.window", lambda: famc(0, -1, off, kinds, none, P(i64(3))))
    _refusal(out, "family_lookup.null", lambda: famc(0, n, off, kinds, none, None))
    _refusal(out, "family_lookup.table_start", lambda: famc(0, n, i32(1, 2), kinds, none, P(i64(3))))
    _refusal(out, "family_lookup.table_rows", lambda: famc(0, n, i32(0, 0), kinds, none, P(i64(3))))
    _refusal(out, "family_lookup.table_kind", lambda: famc(0, n, off, i32(-1), none, P(i64(3))))
    _refusal(out, "family_lookup.table_child", lambda: famc(0, n, off, kinds, i32(0), P(i64(3))))
    cand = lambda first, count, coords, counts: lib.slam_candidate_scores(h, first, count, len(coords) // 3, P(coords), 2, TOL, None, 1, counts, None,
                                                                          C.byref(ms))
    _refusal(out, "candidate_scores.window", lambda: cand(n - 1, 2, f64(0.25, 0.25, 0), P(i64(4))))
    _refusal(out, "candidate_scores.null", lambda: cand(0, n, f64(0.25, 0.25, 0), None))
    _refusal(out, "candidate_scores.table", lambda: cand(0, n, f64(0.25, np.nan, 0), P(i64(4))))
    sel = lambda n_cand, k_max, bounds, n_sel, idx: lib.slam_haar_select_spans(h, SEED, 0, n_cand, k_max, P(f64(0, 0, 0, 0)), bounds, 0.0, 0.0, 1, 1, 4,
                                                                               n_sel, idx, None)
    _refusal(out, "haar_select_spans.window", lambda: sel(-1, 1, None, C.byref(m64), P(i64(4))))
    _refusal(out, "haar_select_spans.null", lambda: sel(8, 1, None, C.byref(m64), None))
    _refusal(out, "haar_select_spans.table", lambda: sel(8, 2, None, C.byref(m64), P(i64(4))))
    pds = lambda n_s, idx, k: lib.slam_pd_sample(h, PD["gc"], PD["gg"], PD["t"], 2, k, 4 * np.pi, 3, 0, n_s, idx, 8, None, None, None)
    _refusal(out, "pd_sample.window", lambda: pds(0, None, 2))
    _refusal(out, "pd_sample.table", lambda: pds(2, P(np.array([0, -1], dtype=np.int64)), 2))
    _refusal(out, "pd_sample.span", lambda: pds(2, None, 0))
    _refusal(out, "pd_extremes.null", lambda: lib.slam_pd_extremes(h, P(f64(1, 0, 0)), 1, P(i64(1)), None))
    _refusal(out, "pd_extremes.table", lambda: lib.slam_pd_extremes(h, P(f64(1, np.inf, 0)), 1, P(i64(1)), P(buf)))
    _refusal(out, "pd_extremes.count", lambda: lib.slam_pd_extremes(h, P(f64(1, 0, 0)), 0, P(i64(1)), P(buf)))
    _refusal(out, "pd_filter.null", lambda: lib.slam_pd_filter(h, P(f64(1, 0, 0, 0.3)), 1, 1e-12, 4, C.byref(m64), None, P(buf)))
    _refusal(out, "pd_filter.table", lambda: lib.slam_pd_filter(h, P(f64(1, 0, np.nan, 0.3)), 1, 1e-12, 4, C.byref(m64), P(i64(4)), P(buf)))
    _refusal(out, "pd_filter.count", lambda: lib.slam_pd_filter(h, P(f64(1, 0, 0, 0.3)), -1, 1e-12, 4, C.byref(m64), P(i64(4)), P(buf)))
    reg = lambda first, count, ro, ki, fo, counts: lib.slam_region_lookup(h, first, count, len(ro) - 1, P(ro), P(ki), P(fo), P(f64(1, 0, 0, 0.4)), None,
                                                                         TOL, counts)
    _refusal(out, "region_lookup.window", lambda: reg(n, 1, i32(0, 1), i32(0), i32(0, 1), P(i64(3))))
    _refusal(out, "region_lookup.null", lambda: reg(0, n, i32(0, 1), i32(0), i32(0, 1), None))
    _refusal(out, "region_lookup.table_kind", lambda: reg(0, n, i32(0, 1), i32(3), i32(0, 1), P(i64(3))))
    _refusal(out, "region_lookup.table_order", lambda: reg(0, n, i32(0, 1), i32(0), i32(0, -1), P(i64(3))))
    _refusal(out, "region_lookup.table_aux", lambda: reg(0, n, i32(0, 1), i32(1), i32(0, 0), P(i64(3))))

    # ---- candidates, counts only, last (another resident batch): several LDS tiles per block
    big = cd.gate_coords(cd.candidate_grid(*BIG_GRID)[0])
    G, t_blocks = len(big), (N_BIG + 255) // 256
    n_chunks = min((2048 + t_blocks - 1) // t_blocks, (G + 7) // 8)  # slam_candidate_scores
    assert (G + n_chunks - 1) // n_chunks == BIG_CHUNK > 32, (G, t_blocks, n_chunks)
    ctx.sample_haar(SEED + 1, N_BIG)
    out["candidates.tiles.counts"], _ = ctx.candidate_scores(big, 4, tol=TOL)
    return out


if __name__ == "__main__":
    from slam_decomposition_amd import _ffi

    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "geometry_parent.npz")
    with _ffi.Context(0) as ctx:
        arrays = run_cases(ctx)
        again = run_cases(ctx)
    # what the scheduling can change must not be pinned: print and leave out what differs between two runs of this one build
    # (expected: nothing -- pd_filter's survivors arrive sorted by index from the binding)
    for key in sorted(arrays):
        if arrays[key].tobytes() != again[key].tobytes():
            print("differs between two runs of one build, left out:", key)
            del arrays[key]
    np.savez_compressed(path, **arrays)
    print("wrote", path, os.path.getsize(path), "bytes,", len(arrays), "arrays")
