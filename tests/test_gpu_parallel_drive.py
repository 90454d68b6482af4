"""parallel_drive.py on the GPU: the sampling kernel against a host replay, the region lookup against the reference's own regions
(tests/golden/reference_smush_coverage.json), the exactness of the prefilter, the whole pipeline at 2^20 samples for the reference's
six gates, and argument errors."""
import json
import os

import numpy as np
import pytest
from scipy.spatial import ConvexHull

from slam_decomposition_amd import _ffi, runtime
from slam_decomposition_amd import parallel_drive as pd
from slam_decomposition_amd.gates import BerkeleyGate, CXGate, SwapGate, smush_matrix
from slam_decomposition_amd.weyl import c1c2c3_batch

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_smush_coverage.json")
REF = json.load(open(FIXTURE))
K_FULL = {"iSwap": 3, "sqiSwap": 3, "CNOT": 3, "sqCNOT": 6, "B": 2, "sqB": 4}
BOUND = 4 * np.pi


def _n_slices(t):
    return int(round(t / 0.25))


def _host_coords(params, v, k, ndigits):
    W = np.array([pd.template_matrix(p, v["gc"], v["gg"], v["t"], _n_slices(v["t"]), k) for p in params])
    return pd.fold(c1c2c3_batch(W, ndigits))


@pytest.fixture(scope="module")
def ctx():
    return runtime.get_context(0)


def test_sampling_kernel_matches_a_host_replay(ctx):
    for name, v in REF.items():
        N = _n_slices(v["t"])
        for k in range(1, v["k_full"]):
            raw, prm, _ = ctx.pd_sample(v["gc"], v["gg"], v["t"], N, k, 48, seed=11, ndigits=-1, want_coords=True, want_params=True)
            assert prm.shape == (48, 6 * (k - 1) + k * (2 + 2 * N))
            assert np.all(np.abs(prm) < BOUND) and prm.std() > 5.0
            host = _host_coords(prm, v, k, 15)
            assert np.abs(raw - host).max() < 1e-9, (name, k, np.abs(raw - host).max())
            r8, _, _ = ctx.pd_sample(v["gc"], v["gg"], v["t"], N, k, 48, seed=11, want_coords=True)
            assert np.abs(r8 - _host_coords(prm, v, k, 8)).max() <= 2e-8, (name, k)
            assert np.all(r8[:, 0] <= 0.5) and np.all(r8[:, 2] >= 0.0)


def test_slice_exponential_matches_smush_matrix(ctx):
    for v in REF.values():
        for t in (0.25, 1.0):  # one slice: tau = 0.25 and tau = 1 (||tau H|| up to ~27: seven squarings)
            _, prm, U = ctx.pd_sample(v["gc"], v["gg"], t, 1, 1, 64, seed=5, want_params=True, want_unitaries=True)
            for p, u in zip(prm, U):
                ref = smush_matrix(p[0], p[1], v["gc"], v["gg"], [p[2]], [p[3]], t)
                assert np.abs(u - ref).max() < 1e-12, (t, np.abs(u - ref).max())


def test_sampling_is_reproducible_and_seeded(ctx):
    v = REF["sqiSwap"]
    a, pa, _ = ctx.pd_sample(v["gc"], v["gg"], v["t"], 2, 2, 4096, seed=3, want_coords=True, want_params=True)
    b, pb, _ = ctx.pd_sample(v["gc"], v["gg"], v["t"], 2, 2, 4096, seed=3, want_coords=True, want_params=True)
    c, pc, _ = ctx.pd_sample(v["gc"], v["gg"], v["t"], 2, 2, 4096, seed=4, want_coords=True, want_params=True)
    assert np.array_equal(a, b) and np.array_equal(pa, pb)
    assert not np.array_equal(pa, pc) and not np.array_equal(a, c)
    # replay by index: the same rows as in the batch
    idx = np.array([0, 17, 4095, 2000])
    d, pdd, _ = ctx.pd_sample(v["gc"], v["gg"], v["t"], 2, 2, 0, seed=3, indices=idx, want_coords=True, want_params=True)
    assert np.array_equal(d, a[idx]) and np.array_equal(pdd, pa[idx])


def _lookup_flags(ctx, ec):
    """Device D[CNOT], D[SWAP], D[B] per partial k: one named gate resident at a time."""
    ks, ro, kinds, fo, facets, aux = ec._table()
    out = {k: [] for k in ks}
    for g in (CXGate(), SwapGate(), BerkeleyGate()):
        ctx.set_targets(g.to_matrix()[None])
        counts = ctx.region_lookup(ro, kinds, fo, facets, aux, 0, 1, tol=pd.TOL)
        for j, k in enumerate(ks):
            out[k].append(bool(counts[j]))
    return out


def test_lookup_on_the_reference_regions(ctx):
    n = 1 << 22
    checked = 0
    for name, v in REF.items():
        ec = pd.ExtendedCoverage.from_rows((v["gc"], v["gg"], v["t"]), v["k_full"], v["regions"])
        vols = ec.volumes(n_targets=n, seed=21)
        sig = 0.0
        for k, row in v["rows"].items():
            k = int(k)
            rv = float(row[1])
            se = max(np.sqrt(rv * (1 - rv) / n), 1e-6)
            sig += se
            assert abs(vols[k][1] - rv) <= 5 * se, (name, k, vols[k], rv)
            checked += 1
        haar = pd.scores_from({k: x[1] for k, x in vols.items()}, {k: (False, False) for k in range(1, v["k_full"])}, v["k_full"])[0]
        assert abs(haar - v["scores"][0]) <= 5 * sig, (name, haar, v["scores"][0])
        flags = _lookup_flags(ctx, ec)
        for k in range(1, v["k_full"]):
            assert flags[k] == list(v["rows"][str(k)][2:]), (name, k, flags[k])
        print(name, "first-containing-region histogram", ec.first_counts)
    assert checked == 21


def test_prefilter_keeps_every_hull_vertex(ctx):
    v = REF["iSwap"]
    n = 1 << 16
    for k in (1, 2):
        allc, _, _ = ctx.pd_sample(v["gc"], v["gg"], v["t"], 4, k, n, seed=9, want_coords=True)
        ref = {tuple(p) for p in allc[ConvexHull(allc).vertices]}
        verts, wit, _, st = pd._device_hull(ctx, n)
        assert {tuple(p) for p in verts} == ref, (k, len(ref), len(verts))
        assert np.array_equal(allc[wit], verts)
        assert st["survivors"] < n // 4


@pytest.mark.parametrize("name", list(K_FULL))
def test_end_to_end_at_2_20_samples(ctx, name):
    v = REF[name]
    ec = pd.extended_coverage(v["gc"], v["gg"], v["t"], n_samples=1 << 20, seed=1)
    assert ec.k_full == K_FULL[name]
    N = _n_slices(v["t"])
    for k in range(1, ec.k_full):
        reg = ec.regions[k]
        _, prm, _ = ctx.pd_sample(v["gc"], v["gg"], v["t"], N, k, 0, seed=1, indices=reg.witnesses, want_params=True)
        assert np.array_equal(prm[0], ec.witness(k, 0))
        host = _host_coords(prm, v, k, 8)
        assert np.abs(host - reg.vertices).max() <= 2e-8, (name, k, np.abs(host - reg.vertices).max())
    n = 1 << 22
    vols = ec.volumes(n_targets=n, seed=22)
    assert vols[ec.k_full] == (1.0, 1.0)
    err = 0.0
    for k in range(1, ec.k_full):
        rv = float(v["rows"][str(k)][1])
        se = max(np.sqrt(rv * (1 - rv) / n), 1e-6)
        err += 5 * se
        assert vols[k][1] >= rv - 5 * se, (name, k, vols[k], rv)
        assert vols[k][1] >= vols[k][0]
    res = ec.results()
    for k in range(1, ec.k_full):
        for got, want in zip(res[str(k)][2:], v["rows"][str(k)][2:]):
            assert got or not want, (name, k, res[str(k)], v["rows"][str(k)])
    haar, cnot, swap = ec.scores
    assert cnot <= v["scores"][1] and swap <= v["scores"][2]
    assert haar <= v["scores"][0] + err, (name, haar, v["scores"][0])
    print(name, "scores", ec.scores, "recorded", v["scores"], {k: ec.stats[k] for k in ec.stats})


def test_bad_arguments(ctx):
    v = REF["iSwap"]
    with pytest.raises(ValueError):
        pd.extended_coverage(v["gc"], v["gg"], 1.0, n_samples=0)
    with pytest.raises(ValueError):
        pd.extended_coverage(v["gc"], v["gg"], -1.0)
    with pytest.raises(NotImplementedError):
        pd.extended_coverage(v["gc"], v["gg"], 1.0, k_full=_ffi.PD_MAX_SPAN + 2)
    for kw in ({"k": 0}, {"k": _ffi.PD_MAX_SPAN + 1}, {"n_slices": 0}, {"n_slices": _ffi.PD_MAX_SLICES + 1}, {"n_samples": 0}, {"t": 0.0}):
        args = {"gc": v["gc"], "gg": v["gg"], "t": 1.0, "n_slices": 4, "k": 1, "n_samples": 16}
        args.update(kw)
        with pytest.raises(_ffi.SlamHipError) as e:
            ctx.pd_sample(**args)
        assert e.value.code < 0
    with pytest.raises(_ffi.SlamHipError) as e:
        ctx.region_lookup([0], [], [0], np.zeros((0, 4)))  # no region
    assert e.value.code < 0
