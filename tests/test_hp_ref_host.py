"""CPU: the 40-digit reference (tests/hp_ref.py) and its committed fixture (tests/golden/hp_eval_reference.npz).

  * a fixed sample of the fixture -- every family, every input kind -- recomputed with hp_ref: bit equality with the stored fp64
    values, so the fixture cannot drift from its generator (tools/make_hp_reference.py);
  * hp_ref against facts it did not produce: KAT-1's recorded SquareCost, K^+ K = 1 for a layer, SquareCost = 0.8 (2 L - L^2), the
    conversion-gain closed form, the smush gate without drives;
  * the stored oracle error ``e_ref`` of every fixed-gate group outside the large-angle kind is below 1e-14 -- what the tolerance rule of
    tests/test_gpu_hp_eval.py (8 * e_ref, at most 1e-13) rests on;
  * the side finding: at |x| >= 3e7 the fp64 oracle (it forms phi + lam in fp64 before exponentiating) is off by more than 1e-12, and is
    not once the big values are reduced mod 4 pi in 40 digits first.
"""
import json
import os

import numpy as np
import pytest

pytest.importorskip("mpmath")

import hp_ref as hp  # noqa: E402
from hp_ref import mp, mpf  # noqa: E402
from oracle import slam_oracle as o  # noqa: E402

GROUPS = hp.load_fixture()


def _find(family, gate=None, k=None, mode=None):
    for g in GROUPS:
        m = g["meta"]
        if m["family"] == family and gate in (None, m["gate"]) and k in (None, m["k"]) and mode in (None, m.get("mode")):
            return g
    raise KeyError((family, gate, k, mode))


def _first_of_each_kind(g):
    kinds = g["meta"]["kinds"]
    return [kinds.index(kd) for kd in sorted(set(kinds))]


def _last_of_each_kind(g):
    kinds = g["meta"]["kinds"]
    return [len(kinds) - 1 - kinds[::-1].index(kd) for kd in sorted(set(kinds))]


SAMPLE = [
    ("short", "sqiswap", 2, None, _last_of_each_kind),   # every input kind of the fixed-gate families
    ("short", "dense", 3, None, lambda g: [0, 3]),       # ... with the Makhlin functional
    ("short", "mixed", 5, None, lambda g: [1]),
    ("long", None, 6, None, lambda g: [0, 7]),
    ("long", None, 16, None, lambda g: [1]),
    ("v2", None, None, "hard", _first_of_each_kind),
    ("v2", None, None, "vz_only", lambda g: [3]),
    ("v2", None, None, "no_exterior", lambda g: [2]),
    ("v2", None, None, "bound", lambda g: [3]),
    ("smush", "N4_off0", None, None, _last_of_each_kind),  # w = 0, ~1e-9, series, both sides of the hand-over
    ("smush", "N1_off2", None, None, lambda g: [0, 4]),
    ("smush", "N8_off2", None, None, lambda g: [5]),
]


@pytest.mark.parametrize("family,gate,k,mode,pick", SAMPLE, ids=[f"{s[0]}-{s[1]}-{s[2]}-{s[3]}" for s in SAMPLE])
def test_fixture_is_what_the_generator_computes(family, gate, k, mode, pick):
    g = _find(family, gate, k, mode)
    chain = hp.chain_of(g)
    costs = g["meta"]["costs"]
    for m in pick(g):
        W, loss, grad = hp.evaluate(chain, g["x"][m], g["targets"][g["tof"][m]], costs)
        for ci, c in enumerate(costs):
            assert loss[c] == g["loss"][ci, m], (m, c)
            assert np.array_equal(grad[c], g["grad"][ci, m]), (m, c)
        if "W" in g:
            assert np.array_equal(W, g["W"][m])


def test_every_family_kind_and_gate_class_is_in_the_fixture():
    kinds = {}
    for g in GROUPS:
        kinds.setdefault(g["meta"]["family"], set()).update(g["meta"]["kinds"])
    fixed = {"general", "theta", "node", "tie", "large", "small_trace", "near_solution"}
    assert kinds["short"] == fixed and kinds["long"] == fixed
    assert kinds["v2"] == fixed | {"vz_only", "no_exterior", "bound"}
    # (no large angles for smush: its sincos returns NaN from |x| = 2e8 on by design, pinned in tests/test_gpu_hp_eval.py)
    assert kinds["smush"] == (fixed - {"large"}) | {"w0", "w1e-9", "handover", "series"}
    assert {g["meta"]["gclass"] for g in GROUPS if g["meta"]["family"] == "short"} == {0, 1, 2, 3, 4}
    assert {(g["meta"]["gate"], g["meta"]["k"]) for g in GROUPS if g["meta"]["family"] == "short"} == {
        (n, k) for n in ("cx", "sqiswap", "iswap", "b", "cg", "dense", "mixed") for k in range(1, 6)}
    assert sorted(g["meta"]["k"] for g in GROUPS if g["meta"]["family"] == "long") == [6, 7, 8, 12, 16]
    assert {g["meta"]["n_slices"] for g in GROUPS if g["meta"]["family"] == "smush"} == {1, 4, 8}
    # the optimizer check of the GPU module leaves nothing out: every input below 2e8 either accepts a first step or (near a solution,
    # eps = 0 / 1e-8) converges at x0
    for g in GROUPS:
        if g["meta"]["family"] in ("short", "long"):
            for kd, st, x in zip(g["meta"]["kinds"], g["meta"]["step"], g["x"]):
                assert (st == -1) == (kd == "large") and (st == 0) <= (kd == "near_solution")
        if g["meta"]["family"] != "smush":
            for kd, x in zip(g["meta"]["kinds"], g["x"]):
                assert (np.max(np.abs(x)) >= 2e7) == (kd == "large")
    # the hand-over cases sit where they claim: u = tau^2 r^2 as the kernel forms it, on both sides of 0.04
    for g in GROUPS:
        if g["meta"]["family"] == "smush":
            u = [v for kd, v in zip(g["meta"]["kinds"], g["meta"]["u"]) if kd == "handover"]
            assert sum(v < 0.04 for v in u) == 2 and sum(v >= 0.04 for v in u) == 2 and min(abs(v - 0.04) for v in u) < 1e-13


def test_hp_ref_against_facts_it_did_not_produce():
    with mp.workdps(hp.DPS):
        # KAT-1 (scripts/decomp_trajectory.ipynb): the recorded SquareCost of the recorded parameters against SWAP
        kat = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "kat1.json")))
        swap = np.array([[1, 0, 0, 0], [0, 0, 1, 0], [0, 1, 0, 0], [0, 0, 0, 1]], dtype=complex)
        chain = hp.fixed_chain([o.riswap_matrix(0.5)] * 3)
        _, loss, _ = hp.evaluate(chain, kat["params"], swap, ("basic", "square"), want_grad=False)
        # (the parameters are printed with 15-16 digits: 3e-15, as test_gpu_eval_parity.py)
        assert abs(loss["square"] - kat["square_cost_vs_swap"]) < 3e-15
        assert abs(loss["basic"] - 2.2193e-09) < 5e-14  # the notebook prints BasicCost with five digits
        # a layer is unitary to the working precision (the fp64 gate matrices only to 1e-16)
        K = hp.layer([hp.F(v) for v in (0.3, -1.7, 2.9, 4.1, 0.01, -6.0)])
        KK = hp.mm(hp.dag(K), K)
        assert max(abs(KK[i][j] - (1 if i == j else 0)) for i in range(4) for j in range(4)) < mpf("1e-38")
        # SquareCost from its own definition = 0.8 (2 L - L^2) of BasicCost
        W = hp.unitary(hp.fixed_chain([o.berkeley_matrix()]), np.linspace(-3, 4, 12))
        T = hp.mat(o.haar_unitary(4))
        L, S = hp.basic_cost(W, T), hp.square_cost(W, T)
        assert abs(S - mpf("0.8") * (2 * L - L * L)) < mpf("1e-38")
        # mp.expm of the Hamiltonians against the closed forms: two decoupled rotations (hamiltonian.py:84-111) ...
        a, pc, b, pg = (hp.F(v) for v in (0.7, 0.3, -1.1, 2.0))
        G = hp.cg_gate(a, pc, b, pg)
        want = {(1, 1): mp.cos(a), (2, 2): mp.cos(a), (2, 1): -1j * mp.expj(pc) * mp.sin(a), (1, 2): -1j * mp.expj(-pc) * mp.sin(a),
                (0, 0): mp.cos(b), (3, 3): mp.cos(b), (3, 0): -1j * mp.expj(pg) * mp.sin(b), (0, 3): -1j * mp.expj(-pg) * mp.sin(b)}
        assert max(abs(G[i][j] - want.get((i, j), 0)) for i in range(4) for j in range(4)) < mpf("1e-36")
        # ... and a smush gate without drives is the conversion-gain gate of the whole pulse
        S4 = hp.smush_gate([a, b] + [mpf(0)] * 8, 4, 1.0)
        assert max(abs(S4[i][j] - hp.cg_gate(a, 0, b, 0)[i][j]) for i in range(4) for j in range(4)) < mpf("1e-36")
    # the Makhlin functional vanishes on locally equivalent gates
    rng = np.random.default_rng(1)
    Wl = np.kron(o.u3(*rng.uniform(0, 6, 3)), o.u3(*rng.uniform(0, 6, 3))) @ o.cx_matrix() @ np.kron(o.u3(*rng.uniform(0, 6, 3)), o.u3(*rng.uniform(0, 6, 3)))
    with mp.workdps(hp.DPS):
        assert hp.makhlin_cost(hp.mat(Wl), hp.mat(o.cx_matrix())) < mpf("1e-28")  # fp64 inputs: unitary to 1e-16 only, squared
        g = hp.local_invariants(hp.mat(o.cx_matrix()))
        assert max(abs(g[0]), abs(g[1]), abs(g[2] - 1)) < mpf("1e-38")  # CNOT: (G1, G2) = (0, 1)


def test_difference_step_is_converged_where_the_gradient_carries_one_over_t():
    """The stored gradient (h = 1e-20 at 40 digits) against h = 1e-30 at 80 digits at the smallest-trace input, |t| = 1e-8."""
    g = _find("short", "sqiswap", 2)
    m = len(g["meta"]["kinds"]) - 1 - g["meta"]["kinds"][::-1].index("small_trace")
    _, _, grad = hp.evaluate(hp.chain_of(g), g["x"][m], g["targets"][g["tof"][m]], ("basic",), dps=80, h="1e-30")
    assert np.max(np.abs(grad["basic"] - g["grad"][0, m])) < 1e-19  # absolute: truncation and rounding of the differences, see hp_ref
    assert 0.1 < np.max(np.abs(grad["basic"])) <= 0.5 + 1e-9


def test_oracle_error_of_the_fixed_gate_groups_is_below_1e_14():
    """BasicCost and SquareCost: below 1e-14 for every fixed-gate group outside the large-angle kind (worst here: 2.6e-15, small trace).
    The Makhlin functional is a quartic in the entries of W over det W with |tr m|^2 up to 16 and J, |grad J| of a few units: its fp64
    restatement (tests/makhlin_ref.py) is within 1.1e-14 (dense, k = 5), so it is held to 1.25e-14 = 1e-13 / 8 -- the largest oracle
    error for which the rule 8 * e_ref stays under the cap of 1e-13 without the cap deciding."""
    worst = {}
    for g in GROUPS:
        if g["meta"]["family"] in ("short", "long"):
            keep = [m for m, kd in enumerate(g["meta"]["kinds"]) if kd != "large"]
            for ci, c in enumerate(g["meta"]["costs"]):
                worst[c] = max(worst.get(c, 0.0), float(np.max(g["e_ref"][ci, keep])))
    print("worst fixed-gate e_ref outside the large-angle kind:", worst)
    assert worst["basic"] < 1e-14 and worst["square"] < 1e-14
    assert worst["makhlin"] < 1.25e-14
    for tol in hp.tolerances(GROUPS).values():
        assert 0.0 < tol <= 1e-13


def test_the_fp64_oracle_is_the_inaccurate_side_at_large_angles():
    g = _find("short", "sqiswap", 2)
    gs = hp.gate_list(g)
    large = [m for m, kd in enumerate(g["meta"]["kinds"]) if kd == "large"]
    assert len(large) == 3
    for m in large:
        assert g["e_ref"][0, m] > 1e-12  # BasicCost: the stored error of oracle.loss_and_grad at this x
        x = g["x"][m]
        with mp.workdps(hp.DPS):
            four_pi = 4 * mp.pi
            xr = np.array([float(hp.F(v) - four_pi * mp.nint(hp.F(v) / four_pi)) if abs(v) > 1e3 else v for v in x])
        f, gr = o.loss_and_grad(xr, gs, g["targets"][g["tof"][m]])
        assert max(abs(f - g["loss"][0, m]), np.max(np.abs(gr - g["grad"][0, m]))) < 1e-14


SINCOS_SRC = r"""
#include "slam_sincos.hpp"
#include <cstdio>
struct D2 { double x, y; };
int main(int argc, char** argv) {
    static const double raw[slamdev::kSincosTableDoubles] = SLAM_SINCOS_TABLE;
    const D2* tbl = reinterpret_cast<const D2*>(raw);
    FILE* f = fopen(argv[1], "r");
    double x;
    while (fscanf(f, "%la", &x) == 1) {
        double s, c;
        slamdev::sincos_tbl(x, tbl, s, c);
        printf("%a %a\n", s, c);
    }
    return 0;
}
"""


def test_host_build_of_sincos_tbl_on_nodes_ties_and_degenerate_arguments(tmp_path):
    """The kernels' table-driven sincos (csrc/slam_sincos.hpp, compiled for the host as in test_sincos_host.py) where its range reduction
    selects: on the nodes n pi/32 and the ties (n + 1/2) pi/32 (|r| = pi/64, the largest polynomial argument) with their fp64 neighbours,
    up to the table path's limit 2e8, and at +-0.0, denormals, pi, 2 pi -- against 40 digits, to the 3e-16 the header states.
    test_sincos_host.py draws uniform arguments, which never land on any of these."""
    import shutil
    import subprocess

    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    rng = np.random.default_rng(3)
    n = np.concatenate([np.arange(-130, 131), rng.integers(-2_000_000_000, 2_000_000_000, 4000)]).astype(np.float64)
    xs = []
    for half in (0.0, 0.5):
        x = (n + half) * np.pi / 32
        xs += [x, np.nextafter(x, np.inf), np.nextafter(x, -np.inf)]
    xs = np.concatenate(xs + [np.array([0.0, -0.0, 5e-324, -5e-324, 2.2250738585072014e-308, np.pi, -np.pi, 2 * np.pi, 1.9e8, -1.9e8, 3.0e7])])
    xs = xs[np.abs(xs) < 2.0e8]
    (tmp_path / "x.txt").write_text("\n".join(float(v).hex() for v in xs))
    (tmp_path / "t.cpp").write_text(SINCOS_SRC)
    subprocess.run(["g++", "-O2", "-mfma", "-ffp-contract=off", "-I", os.path.join(root, "slam_decomposition_amd", "csrc"), "-o",
                    str(tmp_path / "t"), str(tmp_path / "t.cpp")], check=True)
    out = subprocess.run([str(tmp_path / "t"), str(tmp_path / "x.txt")], capture_output=True, text=True, check=True).stdout.split()
    got = np.array([float.fromhex(v) for v in out]).reshape(-1, 2)
    assert len(got) == len(xs)
    worst = 0.0
    with mp.workdps(hp.DPS):
        for x, (s, c) in zip(xs, got):
            worst = max(worst, float(abs(hp.F(s) - mp.sin(hp.F(x)))), float(abs(hp.F(c) - mp.cos(hp.F(x)))))
    print("sincos_tbl on nodes / ties / degenerate arguments: worst", worst)
    assert worst < 3e-16


def test_makhlin_oracle_error_is_at_the_resolution_of_its_fp64_inputs():
    """Why the Makhlin restatement (tests/makhlin_ref.py) is held to 1.25e-14 and not to the 1e-14 of the trace costs: at its worst input
    (dense gate, k = 5, J = 1.9, |grad| up to 2.2) its gradient error is 1.09e-14, and moving ONE of the 36 fp64 parameters by ONE ulp
    moves the 40-digit gradient by 4.2e-15.  An evaluation whose backward error is an ulp in a handful of its inputs -- as good as fp64
    arithmetic gets -- is therefore off by 1e-14: the functional's conditioning at that point, not a loose restatement."""
    g = _find("short", "dense", 5)
    ci = g["meta"]["costs"].index("makhlin")
    m = int(np.argmax(g["e_ref"][ci]))
    assert g["meta"]["kinds"][m] == "general" and 1.0e-14 < g["e_ref"][ci, m] < 1.25e-14
    chain, x, T = hp.chain_of(g), g["x"][m], g["targets"][g["tof"][m]]
    moved = 0.0
    for j in (0, 1, 7, len(x) - 2):
        xp = x.copy()
        xp[j] = np.nextafter(xp[j], np.inf)
        _, _, grad = hp.evaluate(chain, xp, T, ("makhlin",))
        moved = max(moved, float(np.max(np.abs(grad["makhlin"] - g["grad"][ci, m]))))
    print("one ulp in one input moves the 40-digit Makhlin gradient by", moved)
    assert moved > g["e_ref"][ci, m] / 4
