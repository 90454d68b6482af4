#!/usr/bin/env python3
"""Generate tests/golden/weyl_lookup_reference.npz: 40-digit Weyl classes (tests/weyl_ref.py, mpmath) of matrices at general and at
hard inputs, and what slam_coverage_lookup / slam_predict_spans / slam_region_lookup must decide about targets placed on both sides of
every finite face of their tables.

    python tools/make_weyl_reference.py            # writes the fixture (CPU only, a few minutes on 8 cores)

Groups: ``bank`` (the stored local factors K1 = L Q, K2 = Q^+ R and phases g the compact targets are built from), the coordinate
groups (``general``, ``named``, ``det-cut``, ``phase-edge``, ``drifted``, and ``template``: parameters of a 16-gate template for
slam_eval_c1c2c3) and one decision group per table: ``coverage:<n>`` (test_pulse_cost_host.GATE_SETS[n], tol 1e-7), ``span:<name>`` (the
five predictor sequences of tests/test_gpu_round4.py, tol 2e-8 and 5e-4) and ``region:<gate>`` (two gates of
tests/golden/reference_smush_coverage.json through ``ExtendedCoverage.from_rows``).  Every case carries its kind, the reference point
rounded to fp64 and the expected decisions; ``e_ref`` is the error of ``oracle.c1c2c3`` (LAPACK) on the same matrix.  A decision target
below the 3e-8 margin, or a reference coordinate within 1e-4 of a half-integer at 8 digits, is rejected and counted per kind in the
group's metadata; more than 10 % rejected in a kind is an error.
"""
import json
import multiprocessing
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import hp_ref as hp  # noqa: E402
import weyl_ref as w  # noqa: E402
from oracle import slam_oracle as o  # noqa: E402

mp, mpf = w.mp, w.mpf
SEED = 20261017
N_PAIRS, N_PHASES = 16, 8
OFFSET = 4.3e-8  # how far from its face a face target is placed (4.5e-8 puts c1 on a rounding tie where the bound is a multiple of 1e-8)
COVERAGE_TOL, REGION_TOL, SPAN_TOLS = 1e-7, 1e-7, (2e-8, 5e-4)
REGION_GATES = ("B", "CNOT")
NAMED = {
    "I": (0, 0, 0), "CX": (0.5, 0, 0), "iSWAP": (0.5, 0.5, 0), "SWAP": (0.5, 0.5, 0.5), "SWAP+": (0.5, 0.5, -0.5), "sqiSWAP": (0.25, 0.25, 0),
    "B": (0.5, 0.25, 0), "(1,0,0)": (1, 0, 0),
    "edge c2=c3=0": (0.3, 0, 0), "edge c1=c2,c3=0": (0.3, 0.3, 0), "edge c1=c2=c3": (0.3, 0.3, 0.3), "edge c2=c3=1-c1": (0.7, 0.3, 0.3),
    "edge c2=1-c1,c3=0": (0.7, 0.3, 0), "edge c1=c2=1/2": (0.5, 0.5, 0.2),
    "face c3=0": (0.4, 0.2, 0), "face c1=c2": (0.4, 0.4, 0.1), "face c2=1-c1": (0.6, 0.4, 0.1), "face c2=c3": (0.4, 0.2, 0.2),
    "right": (0.8, 0.15, 0.05), "right c3=0": (0.9, 0.05, 0),
}
PERTURBATIONS = (0.0, 1e-15, 1e-12, 1e-10, 1e-8, 1e-6)


# ---- the bank and compact targets -------------------------------------------------------------------------------------------------
def make_bank(rng):
    """K1 = (V (x) V') Q and K2 = Q^+ (V'' (x) V''') from 40-digit SU(2) factors at drawn angles, and phases e^{i phi}: all rounded once."""
    Q = hp._magic()
    k1, k2 = [], []
    for _ in range(N_PAIRS):
        ang = [hp.F(v) for v in rng.uniform(-np.pi, np.pi, 12)]
        su2 = [[[z * mp.expj(-(ang[i + 1] + ang[i + 2]) / 2) for z in row] for row in hp.u3(*ang[i:i + 3])] for i in (0, 3, 6, 9)]  # det 1
        k1.append(hp.to_np(hp.mm(hp.kron(su2[0], su2[1]), Q)))
        k2.append(hp.to_np(hp.mm(hp.dag(Q), hp.kron(su2[2], su2[3]))))
    g = [complex(1.0)] + [complex(mp.expj(hp.F(v))) for v in rng.uniform(-np.pi, np.pi, N_PHASES - 1)]
    return {"k1": np.stack(k1), "k2": np.stack(k2), "g": np.array(g, dtype=np.complex128)}


def tangents(c):
    """t_j = tan(pi a_j(c) / 2) of the diagonal e^{i pi a_j} of CAN(c) in the magic basis, a_j reduced to (-1, 1]."""
    c1, c2, c3 = (mpf(x) if not isinstance(x, mpf) else x for x in c)
    a = [(c1 + c2 - c3) / 2, (c1 - c2 + c3) / 2, (-c1 + c2 + c3) / 2, (-c1 - c2 - c3) / 2]
    a = [x - 2 * mp.floor((x + 1) / 2) for x in a]
    return [float(mp.tan(mp.pi * x / 2)) for x in a]


def ref_of(U):
    """(reference point mpf[3], the same as fp64[3], e_ref) of one matrix."""
    c = w.weyl_class(U)
    ref = np.array([float(x) for x in c])
    e = float(w.distance(np.array([o.c1c2c3(U, 15)], dtype=np.float64), ref[None])[0])
    return c, ref, e


class Compact:
    """Accumulates compact cases of one group."""

    def __init__(self, bank, rng):
        self.bank, self.rng = bank, rng
        self.t, self.pair, self.phase, self.kind, self.ref, self.e_ref = [], [], [], [], [], []
        self.rejected = {}

    def matrix(self, t, pair, phase):
        return w.build_unitaries(np.array([t]), self.bank["k1"][[pair]], self.bank["k2"][[pair]], self.bank["g"][[phase]])[0]

    def draw(self):
        return int(self.rng.integers(N_PAIRS)), int(self.rng.integers(N_PHASES))

    def add(self, kind, t, pair, phase, ref, e):
        self.t.append(t), self.pair.append(pair), self.phase.append(phase), self.kind.append(kind), self.ref.append(ref), self.e_ref.append(e)

    def reject(self, kind):
        self.rejected[kind] = self.rejected.get(kind, 0) + 1

    def arrays(self):
        return {"t": np.array(self.t).reshape(-1, 4), "pair": np.array(self.pair, dtype=np.int32), "phase": np.array(self.phase, dtype=np.int32),
                "ref": np.array(self.ref).reshape(-1, 3), "e_ref": np.array(self.e_ref)}

    def finish(self, name, extra_meta=None, **arrays):
        kinds = sorted(set(self.kind))
        made = {k: self.kind.count(k) for k in kinds}
        for k in set(kinds) | set(self.rejected):
            r = self.rejected.get(k, 0)
            if r > 0.1 * (r + made.get(k, 0)):
                raise SystemExit(f"{name}: {r} of {r + made.get(k, 0)} inputs of kind {k!r} rejected (more than 10 %)")
        g = self.arrays()
        g.update(arrays)
        U = w.build_unitaries(g["t"], self.bank["k1"][g["pair"]], self.bank["k2"][g["pair"]], self.bank["g"][g["phase"]])
        meta = {"name": name, "kinds": self.kind, "made": made, "rejected": {k: self.rejected.get(k, 0) for k in kinds}, "checksum": str(w.checksum(U))}
        meta.update(extra_meta or {})
        g["meta"] = meta
        return g


# ---- coordinate groups --------------------------------------------------------------------------------------------------------------
def coordinate_case(cp, kind, c, pair=None, phase=None):
    p0, g0 = cp.draw()
    pair, phase = p0 if pair is None else pair, g0 if phase is None else phase
    t = tangents(c)
    U = cp.matrix(t, pair, phase)
    cref, ref, e = ref_of(U)
    if not w.rounds_safely(cref):
        cp.reject(kind)
        return None
    cp.add(kind, t, pair, phase, ref, e)
    return U


def group_named(bank):
    rng = np.random.default_rng([SEED, 1])
    cp = Compact(bank, rng)
    for name, c in NAMED.items():
        for eps in PERTURBATIONS:
            for _ in range(2):
                d = rng.normal(size=3)
                d /= np.linalg.norm(d)
                coordinate_case(cp, "named", [mpf(float(x)) + mpf(eps) * mpf(float(y)) for x, y in zip(c, d)])
    return cp.finish("named")


def group_det_cut(bank):
    """det U = g^4 det(K1 D K2) within 1e-16 of the negative real axis, on both sides: g = fp64(e^{i (phi + j pi / 2 + eps)}), phi a
    fourth of what det(K1 D K2) lacks to pi, over the stored pairs, j and a ladder of eps; kept where the 40-digit determinant says so.  Each case brings its own phase into the bank."""
    rng = np.random.default_rng([SEED, 2])
    cp = Compact(bank, rng)
    extra_g = []
    classes = [(0.5, 0, 0), (0.5, 0.5, 0.5), (0.25, 0.25, 0), (0, 0, 0)] + [tuple(chamber_points(rng, 1)[0]) for _ in range(8)]
    for c in classes:
        t = tangents(c)
        want = {1: None, -1: None}
        for pair in rng.permutation(N_PAIRS):
            U1 = w.build_unitaries(np.array([t]), bank["k1"][[pair]], bank["k2"][[pair]], np.ones(1, dtype=np.complex128))[0]
            base = (mp.pi - mp.arg(mp.det(mp.matrix(hp.mat(U1))))) / 4
            for j in rng.permutation(4):
                for step in range(-3, 4):
                    g = complex(mp.expj(base + int(j) * mp.pi / 2 + mpf(step) * mpf("1.1e-16")))
                    U = w.build_unitaries(np.array([t]), bank["k1"][[pair]], bank["k2"][[pair]], np.array([g]))[0]
                    d = mp.det(mp.matrix(hp.mat(U)))
                    side = 1 if d.imag > 0 else -1
                    if d.real < 0 and abs(mp.arg(d)) > mp.pi - mpf("1e-16") and want[side] is None:
                        want[side] = (g, U, int(pair))
            if want[1] is not None and want[-1] is not None:
                break
        for side in (1, -1):
            if want[side] is None:
                raise SystemExit(f"det-cut: no phase found on side {side} for class {c}")
            g, U, pair = want[side]
            cref, ref, e = ref_of(U)
            if not w.rounds_safely(cref):
                cp.reject("det-cut")
                continue
            extra_g.append(g)
            cp.add("det-cut", t, pair, N_PHASES + len(extra_g) - 1, ref, e)
    return cp, extra_g


def group_phase_edge(bank):
    """An eigenphase at two_S = -1/2 + eta: a_3 = -1/4 + eta / 2 with det U = 1 (phase 1 of the bank)."""
    rng = np.random.default_rng([SEED, 3])
    cp = Compact(bank, rng)
    for eta in ("1e-13", "-1e-13", "1e-11", "-1e-11"):
        for _ in range(6):
            x, y = (mpf(float(v)) for v in rng.uniform(-0.45, 0.45, 2))
            a3 = mpf(-1) / 4 + mpf(eta) / 2
            a = [x, y, a3, -(x + y + a3)]
            c = [a[0] + a[1], a[0] + a[2], a[1] + a[2]]
            pair = int(rng.integers(N_PAIRS))
            U = coordinate_case(cp, "phase-edge", c, pair, 0)
            if U is not None:
                ph = w.eigenphases(hp.mat(U))
                if min(abs(p - (mpf(-1) / 2 + mpf(eta))) for p in ph) > mpf("1e-15"):
                    raise SystemExit("phase-edge: no eigenphase where it was placed")
    return cp.finish("phase-edge")


def group_dense(name, kind_mats, seed):
    """Whole matrices: [(kind, U)]."""
    kinds, refs, es, Us, rejected = [], [], [], [], {}
    for kind, U in kind_mats:
        cref, ref, e = ref_of(U)
        if not w.rounds_safely(cref):
            rejected[kind] = rejected.get(kind, 0) + 1
            continue
        kinds.append(kind), refs.append(ref), es.append(e), Us.append(U)
    U = np.stack(Us)
    ks = sorted(set(kinds))
    for k in ks:
        if rejected.get(k, 0) > 0.1 * (rejected.get(k, 0) + kinds.count(k)):
            raise SystemExit(f"{name}: too many rejected")
    meta = {"name": name, "kinds": kinds, "made": {k: kinds.count(k) for k in ks}, "rejected": {k: rejected.get(k, 0) for k in ks},
            "checksum": str(w.checksum(U))}
    return {"meta": meta, "targets": U, "ref": np.array(refs), "e_ref": np.array(es)}


def group_general(_bank):
    return group_dense("general", [("general", u) for u in o.haar_batch(48, seed0=4242)], 4)


def group_drifted(_bank):
    """The fp64 product of a 16-gate sqrt(iSWAP) template, and the same times (1 + 1e-10); ``template``: its parameters, for
    slam_eval_c1c2c3, whose reference is the class of the 40-digit product."""
    rng = np.random.default_rng([SEED, 5])
    gate = o.riswap_matrix(0.5)
    x = rng.uniform(0, 2 * np.pi, (6, 6 * 17))
    mats = []
    for xi in x:
        W = o.template_eval(xi, [gate] * 16)
        mats += [("drifted", W), ("drifted", W * (1.0 + 1e-10))]
    dense = group_dense("drifted", mats, 5)
    chain = hp.fixed_chain([gate] * 16)
    refs, es = [], []
    for xi in x:
        with mp.workdps(w.DPS):
            W = hp.to_np(hp.unitary(chain, xi))  # the 40-digit product, rounded once: its class is the template's to 1e-16
            c = w.weyl_class(W)
        ref = np.array([float(v) for v in c])
        if not w.rounds_safely(c):
            raise SystemExit("template: a reference coordinate sits on a rounding tie; change the seed")
        refs.append(ref)
        es.append(float(w.distance(np.array([o.c1c2c3(o.template_eval(xi, [gate] * 16), 15)], dtype=np.float64), ref[None])[0]))
    tpl = {"meta": {"name": "template", "kinds": ["drifted"] * len(x), "made": {"drifted": len(x)}, "rejected": {"drifted": 0}, "span": 16,
                    "checksum": str(w.checksum(x.astype(np.complex128)))},
           "x": x, "gates": gate[None], "ref": np.array(refs), "e_ref": np.array(es)}
    return dense, tpl


# ---- searching (vectorised fp64; decisions come from the 40-digit reference afterwards) ---------------------------------------------
def chamber_points(rng, n):
    out = []
    while len(out) < n:
        t = rng.uniform(0, 1, (4 * n + 16, 3)) * np.array([1.0, 0.5, 0.5])
        out += list(t[(t[:, 1] <= np.minimum(t[:, 0], 1 - t[:, 0])) & (t[:, 2] <= t[:, 1])])
    return np.array(out[:n])


def np_views(C):
    """Vectorised ``weyl_ref.views``: per shift (A [N, 4], S [N, 14])."""
    C = np.asarray(C, dtype=np.float64).reshape(-1, 3)
    c1, c2, c3 = C[:, 0], C[:, 1], C[:, 2]
    base = np.stack([(c1 + c2 - c3) / 2, (c1 - c2 + c3) / 2, (-c1 + c2 + c3) / 2, (-c1 - c2 - c3) / 2], axis=1)
    out = []
    for shift in (0.0, 0.5):
        f = -np.sort(-((base + shift) - np.floor(base + shift)), axis=1)
        s = np.rint(f.sum(axis=1)).astype(int)
        a = -np.sort(-(f - (np.arange(4)[None, :] < s[:, None])), axis=1)
        S = np.stack([sum(a[:, 4 - k] for k in K) for K in w.PATTERNS], axis=1)
        out.append((a, S))
    return out


class Face:
    """One face: ``slack(C)`` of the face itself and ``others(C)``, the smallest other slack of the same entry (fp64, vectorised), and
    ``exact(c)``: the face's slack at a 40-digit point."""

    def __init__(self, kind, slack, others, exact):
        self.kind, self.slack, self.others, self.exact = kind, slack, others, exact


def halfspace_faces(bounds, tol, kind):
    lo = np.asarray(bounds, dtype=np.float64) - tol
    fin = np.nonzero(np.isfinite(lo))[0]
    faces = []
    for p in fin:
        for sh in (0, 1):
            rest = [q for q in fin if q != p]

            def slack(C, p=p, sh=sh):
                return np_views(C)[sh][1][:, p] - lo[p]

            def others(C, rest=rest, sh=sh):
                S = np_views(C)[sh][1]
                return np.min(S[:, rest] - lo[rest], axis=1) if rest else np.full(len(S), np.inf)

            def exact(c, p=p, sh=sh):
                return w.views(c)[sh][1][p] - mpf(float(lo[p]))

            faces.append(((int(p), float(lo[p]), sh), Face(kind, slack, others, exact)))
    return faces


def facet_faces(facets, tol, kind):
    F = np.asarray(facets, dtype=np.float64).reshape(-1, 4)
    faces = []
    for f in range(len(F)):
        rest = [q for q in range(len(F)) if q != f]

        def slack(C, f=f):
            return tol - (np.asarray(C) @ F[f, :3] - F[f, 3])

        def others(C, rest=rest):
            C = np.asarray(C)
            return np.min(tol - (C @ F[rest, :3].T - F[rest, 3][None, :]), axis=1) if rest else np.full(len(C), np.inf)

        def exact(c, f=f):
            return mpf(float(tol)) - (sum(mpf(float(F[f, j])) * c[j] for j in range(3)) - mpf(float(F[f, 3])))

        faces.append((tuple(np.round(F[f], 12).tolist()), Face(kind, slack, others, exact)))
    return faces


def crossings(face, cloud, rng, tries=24):
    """Segments (x, y) across the face, best first: those where the rest of the entry holds at the crossing (the decision flips)."""
    sl, ot = face.slack(cloud), face.others(cloud)
    inside = np.nonzero((sl > 1e-4) & (ot > 1e-4))[0]
    if len(inside) == 0:
        inside = np.nonzero(sl > 1e-4)[0]
    outside = np.nonzero(sl < -1e-6)[0]
    if len(inside) == 0 or len(outside) == 0:
        return []  # the face's plane does not cut the chamber (a redundant half-space), or only touches its boundary
    xs = cloud[rng.choice(inside, tries)]
    ys = cloud[rng.choice(outside, tries)]
    lo, hi = np.zeros(tries), np.ones(tries)
    for _ in range(50):
        mid = 0.5 * (lo + hi)
        pos = face.slack(xs + mid[:, None] * (ys - xs)) > 0
        lo, hi = np.where(pos, mid, lo), np.where(pos, hi, mid)
    act = face.others(xs + lo[:, None] * (ys - xs))
    order = np.argsort(-np.minimum(act, 1e-2), kind="stable")
    return [(float(min(act[i], 1e-2)), face, xs[i], ys[i]) for i in order[:4]]


def place(face, x, y, value):
    """The point of the segment x -> y where the face's slack is ``value``, by bisection at 40 digits."""
    X, Y = [mpf(float(v)) for v in x], [mpf(float(v)) for v in y]
    at = lambda s: [a + s * (b - a) for a, b in zip(X, Y)]  # noqa: E731
    lo, hi = mpf(0), mpf(1)
    if not (face.exact(at(lo)) > value > face.exact(at(hi))):
        return None
    for _ in range(70):
        mid = (lo + hi) / 2
        if face.exact(at(mid)) > value:
            lo = mid
        else:
            hi = mid
    return at(lo)


def decision_group(args):
    """One table: targets on both sides of every distinct finite face, and the special targets."""
    name, spec, bank, index = args
    mp.dps = w.DPS
    rng = np.random.default_rng([SEED, 100 + index])
    cp = Compact(bank, rng)
    expect, min_margin = [], [np.inf]
    corners = np.array([[0, 0, 0], [1, 0, 0], [0.5, 0.5, 0], [0.5, 0.5, 0.5]])
    cloud = np.concatenate([chamber_points(rng, 16000), rng.dirichlet([0.3] * 4, 8000) @ corners])  # the second part hugs the boundary

    def decide(c):
        """(expected row, margin) of a 40-digit class."""
        if spec["type"] == "coverage":
            b, m = w.lookup(c, spec["kinds"], spec["points"], spec["bounds"], COVERAGE_TOL)
            return [b], m
        if spec["type"] == "span":
            rows = [w.predict_span(c, spec["point"], spec["bounds"], tol) for tol in SPAN_TOLS]
            return [r[0] for r in rows], min(r[1] for r in rows)
        flags, first, m = w.region_flags(c, spec["ro"], spec["kinds"], spec["fo"], spec["facets"], spec["aux"], REGION_TOL)
        return [int(f) for f in flags] + [first], m

    screened, skipped = [0], set()

    def target(kind, c, screen=False):
        """Try one intended class; True if it was kept.  ``screen``: part of a search -- an fp64 look at the intended class first, so
        that only candidates that should pass are built (those that then fail are the rejected ones)."""
        if screen and decide(tuple(float(v) for v in c))[1] < 1.2 * w.MARGIN:
            screened[0] += 1
            return False
        pair, phase = cp.draw()
        t = tangents(c)
        cref, ref, e = ref_of(cp.matrix(t, pair, phase))
        row, m = decide(cref)
        if m < w.MARGIN or not w.rounds_safely(cref):
            cp.reject(kind)
            return False
        cp.add(kind, t, pair, phase, ref, e)
        expect.append(row)
        min_margin[0] = min(min_margin[0], float(m))
        return True

    # faces
    faces, boxes = {}, []
    if spec["type"] in ("coverage", "span"):
        tols = [COVERAGE_TOL] if spec["type"] == "coverage" else list(SPAN_TOLS)
        kinds, points, bounds = (spec["kinds"], spec["points"], spec["bounds"]) if spec["type"] == "coverage" else w.span_table(spec["point"], spec["bounds"])
        for e in range(len(kinds)):
            for tol in tols:
                if kinds[e] == 0:
                    boxes.append((np.asarray(points[e]), tol))
                else:
                    for key, f in halfspace_faces(bounds[e], tol, "face"):
                        faces.setdefault(("h",) + key, f)
    else:
        for p in range(len(spec["kinds"])):
            if spec["kinds"][p] == 0:
                for key, f in facet_faces(spec["facets"][spec["fo"][p]:spec["fo"][p + 1]], REGION_TOL, "face"):
                    faces.setdefault(("f",) + key, f)
            elif spec["kinds"][p] == 1:
                for key, f in halfspace_faces(spec["aux"][p], REGION_TOL, "face"):
                    faces.setdefault(("h",) + key, f)
            else:
                boxes.append((np.asarray(spec["aux"][p][:4]), REGION_TOL))
    unplaced = uncut = 0
    grouped = {}
    for key in sorted(faces, key=repr):  # the two alcove points of a half-space are two ways to cross the same face
        grouped.setdefault(key[:-1], []).append(faces[key])
    for n_face, key in enumerate(sorted(grouped, key=repr)):
        segs = [s for face in grouped[key] for s in crossings(face, cloud, rng)]
        if not segs:
            uncut += 1
            continue
        # best first: crossings where the rest of the entry holds; among equals the alcove point alternates from face to face
        segs.sort(key=lambda s: (-s[0], (grouped[key].index(s[1]) + n_face) % 2))
        for value in (OFFSET, -OFFSET):
            done = False
            for _, face, x, y in segs[:6]:
                c = place(face, x, y, mpf(value))
                if c is not None and target("face", c, screen=True):
                    done = True
                    break
            unplaced += not done
    # one-gate boxes: the gate itself, and points displaced so that the largest |a_j - q_j| is t1 -+ OFFSET
    seen = set()
    for q, tol in boxes:
        if (tuple(q), tol) in seen:
            continue
        seen.add((tuple(q), tol))
        cq = [mpf(float(q[0])) + mpf(float(q[1])), mpf(float(q[0])) + mpf(float(q[2])), mpf(float(q[1])) + mpf(float(q[2]))]
        if spec["type"] != "span":  # (at tol 2e-8 a gate is 2e-8 inside its own box: below the margin)
            target("gate", cq)
        for off in (-OFFSET, OFFSET):
            r = max(tol, 0.0) + 1e-12 + off
            kept = 0
            for _ in range(40):
                if r <= 0 or kept == 2:
                    break
                d = rng.normal(size=3)
                da = 0.5 * np.array([d[0] + d[1] - d[2], d[0] - d[1] + d[2], -d[0] + d[1] + d[2], -d[0] - d[1] - d[2]])
                d = d / np.max(np.abs(da))
                kept += target("box", [a + mpf(r) * mpf(float(b)) for a, b in zip(cq, d)], screen=True)
    if spec["type"] == "region":  # the gate itself (it may sit on a facet of its own hull: looked at first)
        if not target("gate", [mpf(float(v)) for v in spec["gcoords"][0]], screen=True):
            skipped.add("gate")
    # special targets
    for _ in range(2):
        target("local", [mpf(0)] * 3)
    # (with tol = 2e-8 a class of the chamber's edge c2 = c3 = 0 can lie exactly on a face of a region, 2e-8 inside it: below the
    # margin whatever c1 is, so a span group looks first and may keep none)
    for c1 in (1e-7, 1e-6, 1e-3):
        target("c2=c3=0", [mpf(c1), mpf(0), mpf(0)], screen=spec["type"] == "span")
    for plane in (0, 1):  # an alcove coordinate within 1e-9 of an integer: c1 = c2 + c3 (shift 0), c1 + c2 + c3 = 1 (shift 1/2)
        for _ in range(3):
            for attempt in range(400):
                c2, c3 = sorted(rng.uniform(0.02, 0.45, 2), reverse=True)
                c1 = c2 + c3 if plane == 0 else 1.0 - c2 - c3
                if c2 + 0.01 < min(c1, 1 - c1) and decide((float(c1), float(c2), float(c3)))[1] > 2 * w.MARGIN:
                    break
            else:
                skipped.add("integer")  # every such class lies on a face of this table
                continue
            for off in (-1e-9, 1e-9, 0.0):
                target("integer", [mpf(float(c1)) + mpf(off), mpf(float(c2)), mpf(float(c3))])
    for _ in range(3):  # classes whose 8-digit coordinates are (1 - c1, c2, 0) of the canonical point, or sit next to it
        for attempt in range(400):
            c1, c2 = rng.uniform(0.55, 0.95), rng.uniform(0.02, 0.4)
            if c2 + 0.01 < 1 - c1 and decide((1 - c1, c2, 0.0))[1] > 2 * w.MARGIN:
                break
        else:
            skipped.add("mirror")  # the c3 = 0 face is itself a face of this table (CX circuits): every such class is below the margin
            continue
        for c3 in (0.0, 1e-12, -1e-12, 1e-10, -1e-10):
            target("mirror", [mpf(float(c1)), mpf(float(c2)), mpf(c3)])
    kept = 0
    for c in chamber_points(rng, 40):
        kept += kept < 12 and target("general", [mpf(float(v)) for v in c], screen=True)
    arrays = {k: v for k, v in spec.items() if k != "type"}
    e_max = {k: float(max(e for e, kd in zip(cp.e_ref, cp.kind) if kd == k)).hex() for k in sorted(set(cp.kind))}
    cp.arrays = lambda: {k: v for k, v in Compact.arrays(cp).items() if k != "e_ref"}  # a decision group keeps the maximum only
    g = cp.finish(name, {"type": spec["type"], "e_ref_max": e_max, "min_margin": float(min_margin[0]), "faces": len(grouped), "faces_not_cutting_the_chamber": int(uncut), "unplaced_sides": int(unplaced), "screened": int(screened[0]), "skipped": sorted(skipped)},
                  expect=np.array(expect, dtype=np.int32), **arrays)
    return g


# ---- the tables -------------------------------------------------------------------------------------------------------------------------
def table_specs():
    import test_pulse_cost_host as host
    from benchlib.workloads import sweep_gate
    from slam_decomposition_amd import coverage, gates as G, parallel_drive as pd
    from slam_decomposition_amd.weyl import c1c2c3

    specs = []
    for n in range(3):
        t = host._template(*host.GATE_SETS[n]).coverage_table()
        specs.append((f"coverage:{n}", {"type": "coverage", "kinds": np.asarray(t.kinds, dtype=np.int32), "points": np.array(t.points), "bounds": np.array(t.bounds)}))
    cases = {
        "cx": [G.CXGate().to_matrix()] * 3,
        "sqiswap": [G.RiSwapGate(0.5).to_matrix()] * 3,
        "iswap,b,iswap": [G.RiSwapGate(1.0).to_matrix(), G.BerkeleyGate().to_matrix(), G.RiSwapGate(1.0).to_matrix()],
        "cg52 x 5": [sweep_gate(52)] * 5,
        "cg100,cg27,sqiswap": [sweep_gate(100), sweep_gate(27), G.RiSwapGate(0.5).to_matrix()],
    }
    for name, mats in cases.items():
        g = np.array([c1c2c3(m) for m in mats], dtype=np.float64)
        bounds = np.full((len(g), 14), -np.inf)  # what _ffi.Context.predict_spans sends
        for k in range(2, len(g) + 1):
            bounds[k - 1] = coverage.region(g[:k])
        specs.append((f"span:{name}", {"type": "span", "gcoords": g, "point": np.ascontiguousarray(coverage.alcove_coordinates(g[:1])[0]), "bounds": bounds}))
    ref = json.load(open(os.path.join(ROOT, "tests", "golden", "reference_smush_coverage.json")))
    for name in REGION_GATES:
        v = ref[name]
        ec = pd.ExtendedCoverage.from_rows((v["gc"], v["gg"], v["t"]), v["k_full"], v["regions"])
        ks, ro, kinds, fo, facets, aux = ec._table()
        gate = np.array([c1c2c3(G.ConversionGainGate(0, 0, v["gc"], v["gg"], v["t"]).to_matrix())], dtype=np.float64)
        specs.append((f"region:{name}", {"type": "region", "gcoords": gate, "ro": ro.astype(np.int32), "kinds": kinds.astype(np.int32), "fo": fo.astype(np.int32),
                                         "facets": np.array(facets, dtype=np.float64), "aux": np.array(aux, dtype=np.float64)}))
    return specs


def main():
    t0 = time.time()
    mp.dps = w.DPS
    only = sys.argv[1] if len(sys.argv) > 1 and not sys.argv[1].endswith(".npz") else None
    out = next((a for a in sys.argv[1:] if a.endswith(".npz")), w.FIXTURE)
    bank = make_bank(np.random.default_rng([SEED, 0]))
    det, extra_g = group_det_cut(bank)
    full_bank = dict(bank, g=np.concatenate([bank["g"], np.array(extra_g, dtype=np.complex128)]))
    det.bank = full_bank
    specs = [s for s in table_specs() if only is None or s[0].startswith(only)]
    with multiprocessing.Pool(min(len(specs), 10, os.cpu_count() or 1)) as pool:
        pending = pool.map_async(decision_group, [(name, spec, bank, i) for i, (name, spec) in enumerate(specs)], chunksize=1)
        dense, tpl = group_drifted(bank)
        groups = [{"meta": {"name": "bank"}, **full_bank}, group_general(bank), group_named(bank), det.finish("det-cut"), group_phase_edge(bank), dense, tpl]
        groups += pending.get()
    w.save_fixture(out, groups)
    for g in groups[1:]:
        m = g["meta"]
        print(f"{m['name']:<28s} made {m['made']} rejected {m['rejected']}" + (f" faces {m['faces']} (not cutting the chamber {m['faces_not_cutting_the_chamber']}) unplaced sides {m['unplaced_sides']} min margin {m['min_margin']:.3g}" if "faces" in m else "")
              + f" max e_ref {float(np.max(g['e_ref'])) if 'e_ref' in g else max(float.fromhex(v) for v in m['e_ref_max'].values()):.3g}")
    print(f"{out}: {os.path.getsize(out)} bytes, {time.time() - t0:.0f} s")


if __name__ == "__main__":
    main()
