"""How much of the Weyl chamber k parallel-drive ("smush") gates reach, and what that does to a gate's Haar score.

Reference: src/slam/utils/gates/parallel_drive_volume.py:88-451.  For a conversion-gain gate ``(gc, gg, t)`` and each k it draws random
templates of k ``ConversionGainSmushGate(pc, pg, gc, gg, gx[0:N], gy[0:N], t)`` (N = round(t / 0.25) slices, free phases, a U3 (x) U3
layer between consecutive gates and none outside, every parameter uniform in (-4 pi, 4 pi)), folds their Weyl coordinates into
``c1 <= 1/2`` ("left") and mirrors them ("right"), and takes

    region_k = base_k  u  hull(left)  u  hull(right)

where ``base_k`` is the coverage region of k plain gates.  It stops at the first k whose base region is the whole chamber.  Outputs:
``extended_results.json`` rows ``[base_vol, extended_vol, D[CNOT], D[SWAP], D[B]]`` and the scores ``[haar_score, cnot_score,
swap_score]``, ``haar_score = sum_k k (V_k - V_{k-1})``.

Here the sampling runs on the device (``slam_pd_sample``: Philox-drawn parameters, slice exponentials, Weyl coordinates; millions of
samples where the reference takes 3 000), an exact prefilter keeps the points off the host (``slam_pd_extremes`` + ``slam_pd_filter``:
samples strictly inside the hull of a few extreme samples cannot be vertices of the full hull), SciPy's qhull builds the hull, and the
Haar volumes come from resident device targets (``slam_region_lookup``).  The reference's hulls are over rationals of denominator <=
10 000 (parallel_drive_volume.py:351-353); these are over the 8-digit coordinates themselves.  Every hull vertex keeps the index of
the sample that produced it, so ``witness`` returns a parameter vector that reaches it.

Coordinates are ``weylchamber.c1c2c3`` triples (units of pi, ``c3 >= 0``).  The reference's monodromy coordinates of such a point are
``coverage.alcove_coordinates(c)[:, :3]``, a linear map inside the chamber (``m = MONO @ c``).
"""
from __future__ import annotations

from dataclasses import dataclass, field
from fractions import Fraction
from typing import Dict, List, Optional, Sequence

import numpy as np

from . import _ffi, coverage, runtime
from .gates import ConversionGainGate, smush_matrix
from .weyl import c1c2c3

TOL = 1e-7  # region membership on the device: CircuitCoverage.inside's tolerance (span_rules._TOL + 8e-8), as pulse_cost.TOL
FLAG_TOL = 1e-9  # D[CNOT] / D[SWAP] / D[B] on the host
NAMED_POINTS = {"CNOT": (0.5, 0.0, 0.0), "SWAP": (0.5, 0.5, 0.5), "B": (0.5, 0.25, 0.0)}
MONO = 0.5 * np.array([[1.0, 1.0, -1.0], [1.0, -1.0, 1.0], [-1.0, 1.0, 1.0]])  # monodromy coordinates m = MONO @ c
MONO_INV = np.array([[1.0, 1.0, 0.0], [1.0, 0.0, 1.0], [0.0, 1.0, 1.0]])  # c = MONO_INV @ m
KIND_FACETS, KIND_COVERAGE, KIND_CLASS = 0, 1, 2  # slam_region_lookup polytope kinds


@dataclass
class Part:
    """One convex piece of a region: ``facets`` rows (n, b), inside iff n . c <= b (|n| = 1); or a coverage region of k >= 2 plain
    gates (``aux`` = the 14 bounds of ``coverage.region``); or one gate's class (``aux[:4]`` = its alcove point)."""

    kind: int
    facets: np.ndarray = field(default_factory=lambda: np.zeros((0, 4)))
    aux: np.ndarray = field(default_factory=lambda: np.zeros(14))


@dataclass
class Region:
    """region_k: ``base`` parts, then the hull parts (left hull, its mirror).  ``vertices`` are the left hull's vertices (Weyl
    coordinates) and ``witnesses`` the indices of the samples that produced them (-1 when the region came from stored rows)."""

    k: int
    base: List[Part]
    hulls: List[Part]
    vertices: np.ndarray = field(default_factory=lambda: np.zeros((0, 3)))
    witnesses: np.ndarray = field(default_factory=lambda: np.zeros(0, dtype=np.int64))

    @property
    def parts(self) -> List[Part]:
        return self.base + self.hulls


# ---- geometry -------------------------------------------------------------------------------------------------------------------------
def mirror_facets(facets: np.ndarray) -> np.ndarray:
    """Facets of the mirror image c -> (1 - c1, c2, c3): n . c' <= b  ->  (-n1, n2, n3) . c <= b - n1."""
    f = np.array(facets, dtype=np.float64).reshape(-1, 4)
    out = f.copy()
    out[:, 0] = -f[:, 0]
    out[:, 3] = f[:, 3] - f[:, 0]
    return out


def fold(coords) -> np.ndarray:
    """parallel_drive_volume.py:297-305: the "left" point of each sample, ``(1 - c1, c2, c3)`` where ``c1 > 1/2``."""
    c = np.array(coords, dtype=np.float64).reshape(-1, 3)
    c[:, 0] = np.where(c[:, 0] > 0.5, 1.0 - c[:, 0], c[:, 0])
    return c


def hull_facets(points) -> np.ndarray:
    """qhull facets (n, b) of the convex hull of ``points`` (n . c <= b inside, |n| = 1), duplicates of coplanar pieces removed."""
    from scipy.spatial import ConvexHull

    h = ConvexHull(np.asarray(points, dtype=np.float64))
    f = np.concatenate([h.equations[:, :3], -h.equations[:, 3:]], axis=1)
    _, keep = np.unique(np.round(f, 10), axis=0, return_index=True)
    return f[np.sort(keep)]


def _rows_to_facets(rows, equal: bool) -> np.ndarray:
    """Monodromy-coordinate rows ``[b, a0, a1, a2]`` (b + a . m >= 0, or = 0 for equalities) -> facets (n, b) in Weyl coordinates."""
    out = []
    for row in rows:
        r = [float(Fraction(x[0], x[1])) if isinstance(x, (list, tuple)) else float(x) for x in row]
        n = -np.asarray(r[1:]) @ MONO
        b = r[0]
        s = float(np.linalg.norm(n))
        if s > 0.0:
            n, b = n / s, b / s
        out.append([*n, b])
        if equal:
            out.append([*(-n), -b])
    return np.array(out, dtype=np.float64).reshape(-1, 4)


def _to_float(x) -> float:
    return float(Fraction(int(x[0]), int(x[1]))) if isinstance(x, (list, tuple)) else float(x)


def _part_from_stored(cp) -> Part:
    """A convex polytope as the reference stores it: ``{"inequalities": rows, "equalities": rows}`` or ``{"vertices": [[m0, m1, m2],
    ...]}`` in monodromy coordinates (Fractions as [numerator, denominator])."""
    if "vertices" in cp:
        m = np.array([[_to_float(x) for x in v] for v in cp["vertices"]])
        return Part(KIND_FACETS, hull_facets(m @ MONO_INV.T))
    f = np.concatenate([_rows_to_facets(cp.get("inequalities", []), False), _rows_to_facets(cp.get("equalities", []), True)])
    return Part(KIND_FACETS, f)


def _directions() -> np.ndarray:
    """The fixed search directions of the prefilter: the 26 of the cube's faces, edges and corners, and 102 on a Fibonacci sphere."""
    cube = np.array([[x, y, z] for x in (-1, 0, 1) for y in (-1, 0, 1) for z in (-1, 0, 1) if (x, y, z) != (0, 0, 0)], dtype=np.float64)
    m = 102
    i = np.arange(m) + 0.5
    phi = np.arccos(1.0 - 2.0 * i / m)
    th = np.pi * (1.0 + 5.0 ** 0.5) * i
    fib = np.stack([np.cos(th) * np.sin(phi), np.sin(th) * np.sin(phi), np.cos(phi)], axis=1)
    d = np.concatenate([cube, fib])
    return d / np.linalg.norm(d, axis=1, keepdims=True)


def full_coverage_k(gate_coords, k_cap: int = 64) -> int:
    """The first k whose coverage region (k plain gates) is the whole chamber: contains SWAP and every point of a 1/64 grid of the
    chamber (the reference hard-codes these k: 3, 3, 3, 6, 2, 4 for its six gates, parallel_drive_volume.py:91-96)."""
    h = 1.0 / 64
    g = np.arange(0.0, 1.0 + h / 2, h)
    x, y, z = np.meshgrid(g, g[g <= 0.5], g[g <= 0.5], indexing="ij")
    pts = np.stack([x.ravel(), y.ravel(), z.ravel()], axis=1)
    pts = pts[(pts[:, 1] <= np.minimum(pts[:, 0], 1.0 - pts[:, 0])) & (pts[:, 2] <= pts[:, 1])]
    pts = np.concatenate([pts, np.array([NAMED_POINTS["SWAP"]])])
    sums = coverage.target_sums(pts)
    gc = np.asarray(gate_coords, dtype=np.float64).reshape(1, 3)
    for k in range(2, k_cap + 1):
        if coverage.contains(None, np.repeat(gc, k, axis=0), tol=1e-9, sums=sums).all():
            return k
    raise ValueError(f"the gate does not reach the whole chamber within {k_cap} applications")


def _u3(theta, phi, lam) -> np.ndarray:
    c, s = np.cos(theta / 2.0), np.sin(theta / 2.0)
    return np.array([[c, -np.exp(1j * lam) * s], [np.exp(1j * phi) * s, np.exp(1j * (phi + lam)) * c]], dtype=np.complex128)


def template_matrix(params, gc: float, gg: float, t: float, n_slices: int, k: int) -> np.ndarray:
    """The unitary of one sample on the host: W = G_k K_{k-1} ... K_1 G_1, K_j = U3(q1) (x) U3(q0) from ``params[6 (j - 1):6 j]``,
    G_j = ``gates.smush_matrix`` of its (pc, pg, gx[0..N), gy[0..N)) -- the parameter order of ``slam_pd_sample``."""
    x = np.asarray(params, dtype=np.float64).reshape(-1)
    N = int(n_slices)
    q = 2 + 2 * N
    if x.size != 6 * (k - 1) + k * q:
        raise ValueError(f"expected {6 * (k - 1) + k * q} parameters, got {x.size}")
    W = np.eye(4, dtype=np.complex128)
    for j in range(k):
        if j > 0:
            p = x[6 * (j - 1) : 6 * j]
            W = np.kron(_u3(*p[3:6]), _u3(*p[0:3])) @ W
        g = x[6 * (k - 1) + j * q : 6 * (k - 1) + (j + 1) * q]
        W = smush_matrix(g[0], g[1], gc, gg, g[2 : 2 + N], g[2 + N :], t) @ W
    return W


# ---- membership on the host ----------------------------------------------------------------------------------------------------------
def _part_contains(part: Part, c: np.ndarray, sums, tol: float) -> np.ndarray:
    if part.kind == KIND_FACETS:
        if len(part.facets) == 0:
            return np.ones(len(c), dtype=bool)
        return np.all(c @ part.facets[:, :3].T - part.facets[:, 3][None, :] <= tol, axis=1)
    out = np.zeros(len(c), dtype=bool)
    if part.kind == KIND_COVERAGE:
        for _, cols in sums:
            ok = np.ones(len(c), dtype=bool)
            for p, v in enumerate(cols):
                if np.isfinite(part.aux[p]):
                    ok &= v >= part.aux[p] - tol
            out |= ok
        return out
    t1 = max(tol, 0.0) + 1e-12
    for cols, _ in sums:
        ok = np.ones(len(c), dtype=bool)
        for j in range(4):
            ok &= np.abs(cols[j] - part.aux[j]) <= t1
        out |= ok
    return out


class ExtendedCoverage:
    """The extended regions of one gate, k = 1 .. k_full - 1 (``regions[k]``); region k_full is the whole chamber."""

    def __init__(self, gate, k_full: int, regions: Dict[int, Region], n_slices: int = 0, seed: int = 0, bound: float = 4 * np.pi,
                 device: int = 0, stats: Optional[dict] = None):
        self.gc, self.gg, self.t = (float(v) for v in gate)
        self.k_full = int(k_full)
        self.regions = dict(regions)
        self.n_slices = int(n_slices)
        self.seed = int(seed)
        self.bound = float(bound)
        self.device = device
        self.stats = dict(stats or {})
        self._volumes = None
        self.first_counts = None

    # -- construction from stored data ---------------------------------------------------------------------------------------------
    @classmethod
    def from_rows(cls, gate, k_full: int, regions: Dict, device: int = 0) -> "ExtendedCoverage":
        """``regions[k] = {"base": [convex polytopes], "hulls": [convex polytopes]}`` in monodromy coordinates, the way the reference
        stores its coverage sets (``CircuitPolytope.convex_subpolytopes``: the base region's pieces, then the two hulls); a convex
        polytope is ``{"inequalities": rows, "equalities": rows}`` (rows ``[b, a0, a1, a2]``: b + a . m >= 0) or ``{"vertices": ...}``."""
        out = {}
        for k, v in regions.items():
            k = int(k)
            out[k] = Region(k, [_part_from_stored(cp) for cp in v["base"]], [_part_from_stored(cp) for cp in v["hulls"]])
        return cls(gate, k_full, out, device=device)

    # -- membership --------------------------------------------------------------------------------------------------------------------
    def contains(self, coords, k: int, tol: float = TOL, base_only: bool = False) -> np.ndarray:
        """bool[N]: the Weyl coordinates ``coords[N, 3]`` (c3 >= 0) lie in region k (k >= k_full: everywhere)."""
        c = np.asarray(coords, dtype=np.float64).reshape(-1, 3)
        if int(k) >= self.k_full:
            return np.ones(len(c), dtype=bool)
        reg = self.regions[int(k)]
        sums = coverage.target_sums(c)
        out = np.zeros(len(c), dtype=bool)
        for part in reg.base if base_only else reg.parts:
            out |= _part_contains(part, c, sums, tol)
        return out

    def flags(self, k: int, tol: float = FLAG_TOL):
        """(D[CNOT], D[SWAP], D[B]) of region k (parallel_drive_volume.py:380-400)."""
        pts = np.array([NAMED_POINTS[n] for n in ("CNOT", "SWAP", "B")])
        return tuple(bool(v) for v in self.contains(pts, k, tol))

    # -- witnesses ---------------------------------------------------------------------------------------------------------------------
    def witness(self, k: int, i: int) -> np.ndarray:
        """The parameter vector (``template_matrix`` order) of the sample that produced vertex i of region k's hull."""
        reg = self.regions[int(k)]
        w = int(reg.witnesses[int(i)])
        if w < 0:
            raise ValueError("this region has no sampled witnesses (it was built from stored rows)")
        ctx = runtime.get_context(self.device)
        _, params, _ = ctx.pd_sample(self.gc, self.gg, self.t, self.n_slices, int(k), 1, seed=self.seed, bound=self.bound,
                                     indices=[w], want_params=True)
        return params[0]

    # -- volumes and scores ------------------------------------------------------------------------------------------------------------
    def _table(self):
        """[extended region k for k = 1 .. K] + [base region k for k = 1 .. K] as slam_region_lookup arrays (K = k_full - 1)."""
        ks = sorted(k for k in self.regions if k < self.k_full)
        regs = [self.regions[k].parts for k in ks] + [self.regions[k].base for k in ks]
        ro, kinds, fo, facets, aux = [0], [], [0], [], []
        for parts in regs:
            for p in parts:
                kinds.append(p.kind)
                facets.append(p.facets.reshape(-1, 4))
                fo.append(fo[-1] + len(p.facets))
                aux.append(np.resize(np.asarray(p.aux, dtype=np.float64), 14))
            ro.append(len(kinds))
        return ks, np.array(ro), np.array(kinds), np.array(fo), np.concatenate(facets) if facets else np.zeros((0, 4)), np.array(aux)

    def volumes(self, n_targets: int = 2 ** 22, seed: int = 7, device=None) -> Dict[int, tuple]:
        """``{k: (base_vol, extended_vol)}``: the fraction of ``n_targets`` device Haar targets (``slam_sample_haar``) in each region,
        one ``slam_region_lookup``; ``(1.0, 1.0)`` at k_full.  The first-containing-region histogram of the extended regions is kept
        as ``first_counts`` (it equals the score's weights only when the regions nest)."""
        n = int(n_targets)
        if n < 1:
            raise ValueError("n_targets must be >= 1")
        ctx = runtime.get_context(self.device if device is None else device)
        ks, ro, kinds, fo, facets, aux = self._table()
        out: Dict[int, tuple] = {}
        if ks:
            if 2 * len(ks) > _ffi.REGION_MAX:
                raise NotImplementedError(f"at most {_ffi.REGION_MAX // 2} partial k")
            ctx.sample_haar(int(seed), n)
            counts = ctx.region_lookup(ro, kinds, fo, facets, aux, 0, n, tol=TOL)
            K = len(ks)
            for j, k in enumerate(ks):
                out[k] = (counts[K + j] / n, counts[j] / n)
            self.first_counts = {k: int(counts[2 * K + j]) for j, k in enumerate(ks)}
        out[self.k_full] = (1.0, 1.0)
        self.n_targets = n
        self._volumes = out
        return out

    def _vols(self):
        return self._volumes if self._volumes is not None else self.volumes()

    def results(self) -> Dict[str, list]:
        """The reference's extended_results.json rows: ``{str(k): [base_vol, extended_vol, D[CNOT], D[SWAP], D[B]]}``, and
        ``[1, 1, 1, 1, 1]`` at k_full."""
        vols = self._vols()
        out = {}
        for k in range(1, self.k_full):
            out[str(k)] = [vols[k][0], vols[k][1], *self.flags(k)]
        out[str(self.k_full)] = [1, 1, 1, 1, 1]
        return out

    @property
    def scores(self) -> List:
        """``[haar_score, cnot_score, swap_score]`` (parallel_drive_volume.py:148-172,372-391)."""
        vols = self._vols()
        return scores_from(
            {k: v[1] for k, v in vols.items()}, {k: self.flags(k) for k in range(1, self.k_full)}, self.k_full)


def scores_from(volumes: Dict[int, float], flags: Dict[int, Sequence[bool]], k_full: int) -> List:
    """haar_score = sum_k k (V_k - V_{k-1}) (V_0 = 0, V_{k_full} = 1); cnot_score / swap_score = the first k whose D[.] is true, else
    k_full."""
    haar, prev = 0.0, 0.0
    for k in range(1, k_full + 1):
        v = 1.0 if k == k_full else float(volumes[k])
        haar += k * (v - prev)
        prev = v
    cnot = next((k for k in range(1, k_full) if flags[k][0]), k_full)
    swap = next((k for k in range(1, k_full) if flags[k][1]), k_full)
    return [haar, cnot, swap]


# ---- the device pipeline ----------------------------------------------------------------------------------------------------------------
def _device_hull(ctx, n_samples: int):
    """Hull of the resident samples: extremes -> their hull -> drop what is strictly inside it -> qhull of the rest."""
    import time

    from scipy.spatial import ConvexHull
    from scipy.spatial import QhullError

    _, ext = ctx.pd_extremes(_directions())
    sub = np.unique(ext, axis=0)
    try:
        pre = hull_facets(sub)
    except (QhullError, ValueError):
        pre = np.zeros((0, 4))  # degenerate extremes: no prefilter
    if len(pre) == 0:
        pre = np.array([[0.0, 0.0, 0.0, -1.0]])  # a facet no sample is strictly inside: everything survives
    idx, pts = ctx.pd_filter(pre, capacity=n_samples)
    t0 = time.perf_counter()
    h = ConvexHull(pts)
    facets = np.concatenate([h.equations[:, :3], -h.equations[:, 3:]], axis=1)
    _, keep = np.unique(np.round(facets, 10), axis=0, return_index=True)
    facets = facets[np.sort(keep)]
    hull_s = time.perf_counter() - t0
    return pts[h.vertices], idx[h.vertices], facets, {"survivors": int(len(idx)), "prefilter_facets": int(len(pre)), "hull_s": hull_s}


def extended_coverage(gc: float, gg: float, t: float, n_samples: int = 2 ** 20, seed: int = 0, k_full: Optional[int] = None,
                      slice_duration: float = 0.25, bound: float = 4 * np.pi, device: int = 0) -> ExtendedCoverage:
    """parallel_drive_volume.py:148-409 for the gate ``ConversionGainGate(0, 0, gc, gg, t)`` (un-normalised): ``n_samples`` random
    parallel-drive templates per k = 1 .. k_full - 1 (the reference takes 3 000), N = round(t / slice_duration) slices per gate,
    parameters uniform in (-bound, bound).  ``k_full`` (the first k whose plain coverage is the whole chamber) is derived when None."""
    if int(n_samples) != n_samples or n_samples < 1:
        raise ValueError("n_samples must be a positive integer")
    if not (t > 0) or not np.isfinite(t):
        raise ValueError("t must be a finite positive pulse time")
    if not (slice_duration > 0):
        raise ValueError("slice_duration must be positive")
    if not (bound > 0) or not np.isfinite(bound):
        raise ValueError("bound must be finite and positive")
    N = int(round(t / slice_duration))
    if N < 1:
        raise ValueError(f"t / slice_duration = {t / slice_duration:g} rounds to no slice")
    if N > _ffi.PD_MAX_SLICES:
        raise NotImplementedError(f"{N} slices per gate: the device sampler takes at most {_ffi.PD_MAX_SLICES}")
    g = np.asarray(c1c2c3(ConversionGainGate(0, 0, gc, gg, t).to_matrix()), dtype=np.float64)
    if k_full is None:
        k_full = full_coverage_k(g)
    k_full = int(k_full)
    if k_full < 1:
        raise ValueError("k_full must be >= 1")
    if k_full - 1 > _ffi.PD_MAX_SPAN:
        raise NotImplementedError(f"k_full = {k_full}: the device sampler takes k <= {_ffi.PD_MAX_SPAN}")
    ctx = runtime.get_context(device)
    regions: Dict[int, Region] = {}
    stats: Dict[int, dict] = {}
    for k in range(1, k_full):
        ctx.pd_sample(gc, gg, t, N, k, int(n_samples), seed=seed, bound=bound)
        verts, wit, facets, st = _device_hull(ctx, int(n_samples))
        if k == 1:
            base = [Part(KIND_CLASS, aux=np.concatenate([coverage.alcove_coordinates(g)[0], np.zeros(10)]))]
        else:
            base = [Part(KIND_COVERAGE, aux=coverage.region(np.repeat(g[None], k, axis=0)))]
        regions[k] = Region(k, base, [Part(KIND_FACETS, facets), Part(KIND_FACETS, mirror_facets(facets))], verts, wit)
        stats[k] = st
    return ExtendedCoverage((gc, gg, t), k_full, regions, n_slices=N, seed=seed, bound=bound, device=device, stats=stats)
