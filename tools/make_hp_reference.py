#!/usr/bin/env python3
"""Generate tests/golden/hp_eval_reference.npz: 40-digit losses and gradients (tests/hp_ref.py, mpmath) of the four families of fused
evaluation kernels at general-position and at hard inputs, rounded to fp64, with the fp64 oracles' own error at every input.

    python tools/make_hp_reference.py            # writes the fixture (CPU only, about three minutes)

Per group (family, span, gate set): the inputs as fp64 bit patterns (x, targets, gate matrices or gate descriptors), per cost the loss
and the gradient, ``e_ref`` = max(|loss error|, max |gradient error|) of the fp64 oracle (oracle.slam_oracle, oracle.v2_oracle,
tests/smush_ref.py, tests/makhlin_ref.py) against the 40-digit value, the input kind of every case, and whether
``oracle.bfgs_port.minimize_port(maxiter=1)`` accepts a first step from it (fixed-gate families, BasicCost).  tests/test_hp_ref_host.py
recomputes a sample and requires bit equality; tests/test_gpu_hp_eval.py compares the kernels with it.
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import hp_ref as hp  # noqa: E402
import makhlin_ref as mk  # noqa: E402
import smush_ref as sr  # noqa: E402
from oracle import slam_oracle as o  # noqa: E402
from oracle import v2_oracle as v  # noqa: E402
from oracle.bfgs_port import minimize_port  # noqa: E402
from slam_decomposition_amd.gates import ConversionGainSmushGate  # noqa: E402

PI = np.pi
CG = o.conversion_gain_matrix(0.3, -0.7, 0.9, 0.4, 1.0)
ISWAP, SQ, B, CX = o.riswap_matrix(1.0), o.riswap_matrix(0.5), o.berkeley_matrix(), o.cx_matrix()
DENSE = o.haar_unitary(9)
# (name, gate table, sequence of span k): the seven gate sets of the short family
SHORT_SETS = [
    ("cx", [CX], lambda k: [0] * k),
    ("sqiswap", [SQ], lambda k: [0] * k),
    ("iswap", [ISWAP], lambda k: [0] * k),
    ("b", [B], lambda k: [0] * k),
    ("cg", [CG], lambda k: [0] * k),
    ("dense", [DENSE], lambda k: [0] * k),
    ("mixed", [ISWAP, B, CG], lambda k: [j % 3 for j in range(k)]),  # iSWAP alone, then promoted to the classes of B and of CG
]
# the hard inputs: one span of every gate-structure class (cx, xri1, xri, xgen, dense)
SPECIAL_SPANS = {"cx": [1], "sqiswap": [2], "iswap": [], "b": [4], "cg": [5], "dense": [3], "mixed": []}
LONG_TABLE = [DENSE, CG, SQ, CX]
THETAS = [PI, -0.0, 5e-324, 2 * PI, 0.0]
LARGE = [3.0e7, -1.9e8, 2.1e8, -5.0e8, 1.9e9]
DELTAS = [1e-2, 1e-4, 1e-6, 1e-8]
EPS = [0.0, 1e-8, 1e-5, 1e-3]


def diag_target(W, delta):
    """fp64(W diag(e^{i delta}, -1, 1, -1)): |Tr(T^+ W)| = |e^{-i delta} - 1| ~ delta."""
    with hp.mp.workdps(hp.DPS):
        d = [hp.mp.expj(hp.F(delta)), hp.mpc(-1), hp.mpc(1), hp.mpc(-1)]
        return hp.to_np([[W[i][j] * d[j] for j in range(4)] for i in range(4)])


def angle_slots(n_u):
    """True for the theta slots (the kernels halve them) among the first n_u U-gate parameters."""
    return np.array([i % 3 == 0 for i in range(n_u)])


def special_inputs(rng, n, n_u, lo, hi, chain, want_large=True):
    """(kind, x, target or None = the group's Haar target) of the hard inputs; ``n_u`` U-gate angles in front of the n parameters."""
    th = np.nonzero(angle_slots(n_u))[0]
    out = []
    x = rng.uniform(lo, hi, n)
    x[th] = 0.0
    out.append(("theta", x, None))
    x = rng.uniform(lo, hi, n)
    x[th] = [THETAS[i % len(THETAS)] for i in range(len(th))]
    out.append(("theta", x, None))
    for kind, half in (("node", 0.0), ("tie", 0.5), ("node", 0.0), ("tie", 0.5)):
        arg = (rng.integers(-64, 129, n) + half) * PI / 32  # the argument the table reduction sees
        x = arg.copy()
        x[th] = 2.0 * arg[th]
        out.append((kind, x, None))
    if want_large:
        for vals in (LARGE[:2], LARGE[2:], LARGE):
            x = rng.uniform(lo, hi, n)
            others = np.nonzero(~angle_slots(n_u))[0]
            slots = [th[1]] + list(rng.choice(others, size=len(vals) - 1, replace=False))  # one of them a half angle
            x[slots] = vals
            out.append(("large", x, None))
    for delta in DELTAS:
        x = rng.uniform(lo, hi, n)
        out.append(("small_trace", x, diag_target(hp.unitary(chain, x), delta)))
    xs = rng.uniform(lo, hi, n)
    with hp.mp.workdps(hp.DPS):
        Ts = hp.to_np(hp.unitary(chain, xs))
    z = rng.uniform(-1, 1, n)
    for eps in EPS:
        out.append(("near_solution", xs + eps * z, Ts))
    return out


def pack_cases(cases, haar_target):
    """Deduplicated targets + target_of."""
    targets, tof = [haar_target], []
    for _, _, T in cases:
        if T is None:
            tof.append(0)
            continue
        for i, Q in enumerate(targets):
            if Q is T or np.array_equal(Q, T):
                tof.append(i)
                break
        else:
            targets.append(T)
            tof.append(len(targets) - 1)
    return np.stack(targets), np.array(tof, dtype=np.int32)


def finish_group(meta, chain, cases, haar_target, oracle_fn, extra, want_W=False):
    """Evaluate every case with hp_ref and with the fp64 oracle ``oracle_fn(x, T, cost) -> (loss, grad[, W])``."""
    costs = meta["costs"]
    targets, tof = pack_cases(cases, haar_target)
    M, n = len(cases), len(cases[0][1])
    loss = np.zeros((len(costs), M))
    grad = np.zeros((len(costs), M, n))
    e_ref = np.zeros((len(costs), M))
    Ws = np.zeros((M, 4, 4), dtype=np.complex128)
    e_w = np.zeros(M)
    for m, (kind, x, _) in enumerate(cases):
        T = targets[tof[m]]
        W, l, g = hp.evaluate(chain, x, T, costs)
        Ws[m] = W
        for ci, c in enumerate(costs):
            loss[ci, m], grad[ci, m] = l[c], g[c]
            ref = oracle_fn(x, T, c)
            e_ref[ci, m] = max(abs(ref[0] - l[c]), float(np.max(np.abs(ref[1] - g[c]))))
            if want_W and ci == 0:
                e_w[m] = float(np.max(np.abs(ref[2] - W)))
        hp._slice_cache.clear()
    meta = dict(meta, kinds=[c[0] for c in cases])
    g = dict(meta=meta, x=np.stack([c[1] for c in cases]), targets=targets, tof=tof, loss=loss, grad=grad, e_ref=e_ref, **extra)
    if want_W:
        g["W"] = Ws
        g["e_ref_w"] = e_w
    return g


def fixed_oracle(gs):
    def fn(x, T, cost):
        if cost == "basic":
            return o.loss_and_grad(x, gs, T)
        if cost == "square":
            return o.square_loss_and_grad(x, gs, T)
        return mk.loss_and_grad(x, gs, T)

    return fn


def step_flags(cases, targets, tof, gs):
    """1: minimize_port(maxiter = 1) accepts a step from x; 0: it converges at x (near-solution, eps = 0 / 1e-8 only); -1: large angles,
    stand-alone evaluation only."""
    flags = []
    for m, (kind, x, _) in enumerate(cases):
        if kind == "large":
            flags.append(-1)
            continue
        f, _, it, status, nev = minimize_port(x, gs, targets[tof[m]], maxiter=1)
        if it == 0:
            assert kind == "near_solution" and status == 0, (kind, m, f, status)
        flags.append(int(it))
    return flags


def fixed_group(family, name, table, seq, k, seed, with_special, costs):
    rng = np.random.default_rng(seed)
    gs = [table[i] for i in seq]
    chain = hp.fixed_chain(gs)
    n = 6 * (k + 1)
    haar = o.haar_unitary(1000 + seed)
    cases = [("general", rng.uniform(-2 * PI, 4 * PI, n), None) for _ in range(3 if with_special else 2)]
    if with_special:
        cases += special_inputs(rng, n, n, -2 * PI, 4 * PI, chain)
    meta = dict(family=family, gate=name, k=k, costs=costs, gclass=hp.classify_gates_host(gs))
    g = finish_group(meta, chain, cases, haar, fixed_oracle(gs), dict(gates=np.stack(table), seq=np.array(seq, dtype=np.int32)))
    g["meta"]["step"] = step_flags(cases, g["targets"], g["tof"], gs)
    return g


# ---- CircuitTemplateV2 ------------------------------------------------------------------------------------------------------
def v2_group(name, gmap, qn, k, seed, mode):
    """``gmap`` = (sel, scale, offset) over (a, phi_c, b, phi_g); device order.  mode: general | vz_only | no_exterior | bound | hard."""
    rng = np.random.default_rng(seed)
    maps = [gmap] * k
    chain = hp.v2_chain(maps, qn)
    n_u = 6 * (k + 1)
    n = n_u + qn * k
    haar = o.haar_unitary(2000 + seed)
    cases = [("general", rng.uniform(-4 * PI, 4 * PI, n), None) for _ in range(3)]
    if mode == "vz_only":  # rz(lam) = U(0, 0, lam) up to a phase: theta = phi = 0 in every layer
        for kind, x, _ in list(cases):
            x = x.copy()
            x[:n_u].reshape(-1, 3)[:, :2] = 0.0
            cases.append(("vz_only", x, None))
    if mode == "no_exterior":  # layers 0 and k pinned at U(0, 0, 0)
        for kind, x, _ in list(cases):
            x = x.copy()
            x[:6] = 0.0
            x[6 * k : n_u] = 0.0
            cases.append(("no_exterior", x, None))
    if mode == "bound":  # gate parameters ON the box bounds the optimizer projects to (alpha in {0, 1/2} for RiSwapGate)
        for kind, x, _ in list(cases):
            x = x.copy()
            x[n_u:] = rng.choice([0.0, 0.5], size=n - n_u)
            cases.append(("bound", x, None))
    if mode == "hard":
        cases += special_inputs(rng, n, n_u, -4 * PI, 4 * PI, chain)  # large angles: slam_v2_eval_loss_grad takes any x (sincos_any)
    meta = dict(family="v2", gate=name, k=k, costs=["basic", "square"], qn=qn, mode=mode)

    def oracle_fn(x, T, cost):
        f, g = v.loss_and_grad(x, maps, qn, k, T, False, cost == "square")
        fns = [lambda *q: v.cg_matrix(v.raw_of(q, gmap))] * k
        return f, g, v.template_eval(x, fns, qn, k)

    sel, scale, offset = gmap
    extra = dict(sel=np.array([sel], dtype=np.int32), scale=np.array([scale]), offset=np.array([offset]), seq=np.zeros(k, dtype=np.int32))
    return finish_group(meta, chain, cases, haar, oracle_fn, extra, want_W=True)


# ---- parallel drive -----------------------------------------------------------------------------------------------------------
def smush_group(N, offset, k, t, gc, gg, seed, hard=False):
    """ConversionGainSmushGate(0, 0, gc, gg, gx[0..N), gy[0..N), t) with the drives (offset 0) or (gc, gg, drives) (offset 2) as the gate's
    parameters.  The hard inputs put u = (tau w)^2 of BOTH 2x2 blocks of every slice where ``sm_slice`` changes its formula: with
    gc = gg the blocks have w = |gx + gy| and |gy - gx|, so one drive of a slice is 0 and the other +- sqrt(u) / tau."""
    rng = np.random.default_rng(seed)
    qn = offset + 2 * N
    if offset == 0:
        desc = (N, t, [-1, -1] + list(range(2 * N)), [0.0, 0.0] + [1.0] * (2 * N), [gc, gg] + [0.0] * (2 * N))
        fn = lambda *q: ConversionGainSmushGate(0.0, 0.0, gc, gg, q[:N], q[N:], t_el=t)
    else:
        desc = (N, t, list(range(2 + 2 * N)), [1.0] * (2 + 2 * N), [0.0] * (2 + 2 * N))
        fn = lambda *q: ConversionGainSmushGate(0.0, 0.0, q[0], q[1], q[2 : 2 + N], q[2 + N :], t_el=t)
    chain = hp.smush_chain([desc] * k, qn)
    n_u = 6 * (k + 1)
    n = n_u + qn * k
    tau = t / N
    haar = o.haar_unitary(3000 + seed)
    cases = [("general", rng.uniform(-3, 3, n), None) for _ in range(3)]
    u_kinds = [("w0", 0.0), ("w1e-9", None), ("handover", 0.04 * (1 - 2.0**-40)), ("handover", 0.04 * (1 + 2.0**-40)), ("handover", 0.04 - 1e-3),
               ("handover", 0.04 + 1e-3), ("series", 1e-3), ("series", 1e-2)]
    u_of_case = [None, None, None]
    for kind, u in u_kinds:
        x = rng.uniform(-3, 3, n)
        for j in range(k):
            q = x[n_u + qn * j : n_u + qn * (j + 1)]
            if offset == 2:
                q[0] = q[1] = 0.6  # gc = gg: d = 0 (offset 0: the constants are equal)
            drives = q[offset:]
            if u is None:
                drives[:] = rng.uniform(-1e-9, 1e-9, 2 * N) / tau
            else:
                r = np.sqrt(u) / tau
                for s in range(N):
                    on_x = bool(rng.integers(0, 2))
                    drives[s] = (r if rng.integers(0, 2) else -r) if on_x else 0.0
                    drives[N + s] = 0.0 if on_x else (r if rng.integers(0, 2) else -r)
        cases.append((kind, x, None))
        u_of_case.append(float(tau * tau * (np.sqrt(u) / tau) ** 2) if u is not None else 1e-18)
    if hard:
        # eval_smush has its own U3 trig entry (sm_sincos of the half angle), trace and cost tail: the hard inputs of the other families,
        # gate parameters (the drives) included.  No large angles: sm_sincos returns NaN from |x| = 2e8 on by design (the GPU module
        # pins that).
        extra_cases = special_inputs(rng, n, n_u, -3, 3, chain, want_large=False)
        cases += extra_cases
        u_of_case += [None] * len(extra_cases)
    meta = dict(family="smush", gate=f"N{N}_off{offset}", k=k, costs=["basic", "square"], qn=qn, n_slices=N, u=u_of_case)

    def oracle_fn(x, T, cost):
        return sr.loss_grad_unitary(x, fn, qn, k, T, cost == "square")

    extra = dict(t=np.array([desc[1]]), sel=np.array([desc[2]], dtype=np.int32), scale=np.array([desc[3]]), offset=np.array([desc[4]]),
                 seq=np.zeros(k, dtype=np.int32))
    return finish_group(meta, chain, cases, haar, oracle_fn, extra, want_W=True)


def main():
    t0 = time.time()
    groups = []
    seed = 0
    for name, table, seq_of in SHORT_SETS:
        for k in range(1, 6):
            seed += 1
            costs = ["basic", "square"] + (["makhlin"] if name == "dense" else [])
            groups.append(fixed_group("short", name, table, seq_of(k), k, seed, k in SPECIAL_SPANS[name], costs))
            print(f"short {name} k={k}: {time.time() - t0:.0f} s", flush=True)
    for k in (6, 7, 8, 12, 16):
        seed += 1
        costs = ["basic", "square"] + (["makhlin"] if k == 7 else [])
        groups.append(fixed_group("long", "mixed4", LONG_TABLE, [(3 * j + 1) % 4 for j in range(k)], k, seed, k == 6, costs))
        print(f"long k={k}: {time.time() - t0:.0f} s", flush=True)
    # conversion-gain lambdas (raw angles a = gc t, phi_c, b = gg t, phi_g)
    cg_gc_gg = ([0, -1, 1, -1], [1.5, 0.0, 1.5, 0.0], [0.0, 0.3, 0.0, -0.2])   # lambda gc, gg: ConversionGainGate(0.3, -0.2, gc, gg, 1.5)
    cg_4 = ([2, 0, 3, 1], [0.7, 1.0, 0.7, 1.0], [0.0, 0.0, 0.0, 0.0])          # lambda p1, p2, g1, g2: ConversionGainGate(p1, p2, g1, g2, 0.7)
    cg_unit = ([0, -1, 1, -1], [1.0, 0.0, 1.0, 0.0], [0.0, 0.3, 0.0, -0.2])    # t = 1: the gate parameters ARE the table arguments
    riswap = ([0, -1, -1, -1], [-0.5 * PI, 0.0, 0.0, 0.0], [0.0, 0.0, 0.0, 0.0])  # RiSwapGate(alpha) = CG(0, 0, -pi alpha / 2, 0, 1)
    for name, gmap, qn, k, mode in (("cg_gc_gg", cg_gc_gg, 2, 1, "general"), ("cg_gc_gg", cg_gc_gg, 2, 2, "vz_only"),
                                    ("cg_gc_gg", cg_gc_gg, 2, 3, "no_exterior"), ("cg_4", cg_4, 4, 2, "general"),
                                    ("riswap", riswap, 1, 3, "bound"), ("riswap", riswap, 1, 5, "general"),
                                    ("cg_unit", cg_unit, 2, 2, "hard")):
        seed += 1
        groups.append(v2_group(name, gmap, qn, k, seed, mode))
        print(f"v2 {name} k={k} {mode}: {time.time() - t0:.0f} s", flush=True)
    for N, offset, k, t, gc, gg in ((1, 0, 6, 0.5, PI / 4, PI / 4), (1, 2, 3, 1.0, 0.0, 0.0), (4, 0, 2, 1.0, PI / 4, PI / 4), (4, 2, 1, 0.5, 0.0, 0.0),
                                    (8, 0, 1, 1.0, PI / 4, PI / 4), (8, 2, 1, 0.5, 0.0, 0.0)):
        seed += 1
        groups.append(smush_group(N, offset, k, t, gc, gg, seed, hard=(N, offset) == (4, 0)))
        print(f"smush N={N} offset={offset} k={k}: {time.time() - t0:.0f} s", flush=True)
    hp.save_fixture(hp.FIXTURE, groups)
    print(f"{hp.FIXTURE}: {os.path.getsize(hp.FIXTURE)} bytes, {len(groups)} groups, {sum(len(g['meta']['kinds']) for g in groups)} cases, "
          f"{time.time() - t0:.0f} s")


if __name__ == "__main__":
    main()
