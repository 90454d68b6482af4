// slam_q3.hpp -- three-qubit templates (8x8 targets): ONE WAVEFRONT per (target, restart) item, sibling of slam_long.hpp (gfx950 only).
//
// The circuit, in time order: U3 on q0, q1, q2 (parameters 0..8), then per two-qubit gate j = 0..k-1 on the edge (a_j, b_j): the gate, a
// U3 on a_j, a U3 on b_j (parameters 9 + 6 j ..) -- n = 9 + 6 k parameters, k <= 15.  Matrices are qiskit little-endian: basis index
// q0 + 2 q1 + 4 q2; a gate's 4x4 on (a, b) has qubit a as its bit 0 and qubit b as its bit 1.
//   * lane l holds entry (r = l & 7, c = l >> 3) of the 8x8 running product P.  Left-multiplying by a U3 on qubit q mixes rows r and
//     r ^ (1 << q), by a gate on (a, b) the four rows r ^ {0, 1 << a, 1 << b, both}: every exchange is a lane XOR of 1, 2 (DPP quad_perm)
//     or 4 (ds_swizzle, bit mode) -- no LDS memory traffic, and the edge enters through two wave-uniform qubit numbers only;
//   * backward, P_{l-1} = M_l^+ P_l undoes the factors (they are unitary: no prefix is stored) while the adjoint is carried TRANSPOSED,
//     B^T_{l-1} = M_l^T B^T_l from B^T_L = z conj(T) (z = the loss seed), so right-multiplication is row mixing too;
//   * the three derivatives of a U3 on qubit q come from the 2x2 block trace R[s', s] = sum_{r: bit_q(r) = s} sum_c P[r, c] B^T[r with
//     bit q := s', c]: two complex products per lane (own entry, partner at XOR 1 << q) and masked wave sums:
//         d/dphi = -Im R'[1, 1],  d/dtheta = 1/2 Re(e^{i phi} R'[1, 0] - e^{-i phi} R'[0, 1])   (P', B^T after the gate),
//         d/dlam = -Im R[1, 1]                                                                  (P, B^T before it);
//   * the optimizer is the iteration of slam_long_minimize.inc, its body copied for n = 9 + 6 k (n may be odd: slot n is padding):
//     fp32 inverse metric in device memory (lane l owns columns 2 l, 2 l + 1), cautious update, Armijo backtracking, periodic restart,
//     the same stopping tests and status codes, the restart-major work queue with ordered early exit, Philox start points.
// Loss, gradient, parameters, steps: fp64.
//
// Mixed templates (eval_q3_kernel<true>, minimize_q3_kernel<true>): a position may hold a three-qubit gate on the ordered triple
// (a, b, c) -- gate-local bit 0 is qubit a, bit 1 is b, bit 2 is c -- followed by a U3 on a, on b, on c: n = 9 + 3 sum(arity_j) <= 99.
//   * such a gate mixes all eight rows: the new entry is sum_m G[idx][idx ^ m] P[row ^ x(m)], idx = bit_a | bit_b << 1 | bit_c << 2 of
//     the lane's row, x(m) = (m & 1) << a | (m >> 1 & 1) << b | (m >> 2) << c.  (a, b, c) is a permutation of (0, 1, 2), so x runs over
//     all seven lane XORs: the partners come from ONE fixed chain of exchanges in Gray-code order of the LANE mask (XOR 1, 2, 1, 4, 1,
//     2, 1: seven exchanges per real component, DPP and ds_swizzle, no LDS data traffic), and the edge enters through the table column
//     m = x^-1(mask) only -- wave-uniform integer work, no branch on the qubit numbers;
//   * the table E[i][m] = G[i][i ^ m] (64 double2 = 1 KB) is kept once per DISTINCT three-qubit gate (at most kQ3MaxGates3) behind the
//     wavefront's other LDS and reached through the position's gate index; backward uses the modes of q3_mix4 (G, G^+ on P, G^T on B^T);
//   * parameter offsets come from a running base (positions have 6 or 9 parameters).
// The two-qubit-only kernels are the MIXED = false instantiations of the same bodies: nothing of the above is compiled into them.
//
// State objectives (eval_q3_kernel<MIXED, true>, minimize_q3_kernel<MIXED, true>; slam_q3s_*): the mutual information left in
// v = W(x) psi for a start state psi.  P starts as the matrix with psi in column 0, step 3 of eval_q3 forms the three one-qubit reduced
// states from column 0 and seeds the backward pass with the loss's derivative there; everything else is the same code, and nothing of
// it is compiled into the STATE = false instantiations.  Seven of the eight columns idle (accepted: the optimizer body is wave-wide).
//
// Reference behaviour: CircuitTemplate(n_qubits, edge_params) src/slam/basis.py:52-169; BasicCost / SquareCost
// src/slam/cost_function.py:140-145,169-173; MutualInformation / MutualInformationSquare src/slam/cost_function.py:44-99; the restart
// loop src/slam/optimizer.py:253-295.
#pragma once
#include "slam_long.hpp"

namespace slamdev {

constexpr int kQ3MaxSpan = 15;
constexpr int kQ3N = 9 + 6 * kQ3MaxSpan;  // 99 parameters at most
constexpr int kQ3NP = 128;                // vector length in LDS: component i = 2 lane + a, a = 0, 1
constexpr int kQ3Slots = 2;
constexpr int kQ3HStride = kQ3NP;         // floats per row of the inverse Hessian in device memory
constexpr int kQ3RowBatch = 16;

// LDS of one wavefront, in doubles
constexpr int kQ3OffTbl = 0;                                // sincos table (64 double2)
constexpr int kQ3OffX = kQ3OffTbl + kSincosLdsDoubles;      // trial point x[NP]
constexpr int kQ3OffG = kQ3OffX + kQ3NP;                    // gradient g[NP]
constexpr int kQ3OffTrig = kQ3OffG + kQ3NP;                 // (cos, sin) of every (half-)angle: [100] double2
constexpr int kQ3OffGate = kQ3OffTrig + 2 * (kQ3N + 1);     // per position j the 16 entries E_j[i][m] = G_j[i][i ^ m]: [k][16] double2
constexpr int kQ3OffF32 = kQ3OffGate + 32 * kQ3MaxSpan;     // three fp32 vectors [NP] of the metric pass
constexpr int kQ3LdsDoubles = kQ3OffF32 + 3 * kQ3NP / 2;
constexpr size_t kQ3LdsBytes = (size_t)kQ3LdsDoubles * sizeof(double);
static_assert(16 * kQ3LdsBytes <= 160 * 1024, "four wavefronts per SIMD need sixteen wavefronts' LDS per CU");
// mixed templates: the tables of the distinct three-qubit gates behind everything else, E_g[i][m] = G_g[i][i ^ m]: [g][64] double2
constexpr int kQ3MaxGates3 = 3;
constexpr int kQ3OffGate3 = kQ3LdsDoubles;
constexpr int kQ3MLdsDoubles = kQ3OffGate3 + 128 * kQ3MaxGates3;
constexpr size_t kQ3MLdsBytes = (size_t)kQ3MLdsDoubles * sizeof(double);
static_assert(12 * kQ3MLdsBytes <= 160 * 1024, "minimize_q3_kernel<true>: three wavefronts per SIMD need twelve wavefronts' LDS per CU");

struct Q3Args {
    const double* targets;    // [n_active][8][8][2]
    const double* x0;         // [M][n] or nullptr (Philox)
    StageCtl* ctl;
    int32_t restarts;
    int32_t maxiter;
    double gtol, stop_loss, gtol_far, far_loss, exit_loss;
    uint64_t seed;
    int64_t target_base;
    uint32_t flags;           // SLAM_FLAG_EARLY_EXIT | SLAM_FLAG_ORDERED
    int32_t cost_kind;
    int32_t* solved;
    ItemRec* item_rec;        // [M]
    double* item_x;           // [M][n]
    const double* gates;      // [k][4][4][2]: the gate of every position
    uint64_t edges;           // position j: a = bits 4 j, 4 j + 1; b = bits 4 j + 2, 4 j + 3
    int32_t k;
    float* hmem;              // [gridDim.x][n][kQ3HStride]
};

struct Q3EvalArgs {
    const double* targets;
    const double* x;          // [M][n]
    const int32_t* target_of; // [M]
    int64_t n_items;
    double* loss;
    double* grad;             // [M][n] or nullptr
    double* unitary;          // [M][8][8][2] or nullptr
    int32_t cost_kind;
    const double* gates;
    uint64_t edges;
    int32_t k;
};

// mixed templates: what the two-qubit structures do not carry
struct Q3MArgs : Q3Args {
    const double* gates3;     // [n_gates3][8][8][2]: the distinct three-qubit gates
    uint64_t ext;             // position j: bits 4 j, 4 j + 1 = qubit c (3: a two-qubit position); bits 4 j + 2, 4 j + 3 = its entry of gates3
    int32_t n_gates3;
    int32_t n;                // 9 + 3 sum(arity)
};
struct Q3MEvalArgs : Q3EvalArgs {
    const double* gates3;
    uint64_t ext;
    int32_t n_gates3;
    int32_t n;
};

// the value of lane (l ^ (1 << q)), q wave-uniform
__device__ __forceinline__ double q3_xchg(double v, int q) {
    if (q == 0) return dpp_f64<0xB1>(v);
    if (q == 1) return dpp_f64<0x4E>(v);
    // ds_swizzle bit mode: and 0x1F, or 0, xor 4 (within each half of the wavefront)
    const int lo = __builtin_amdgcn_ds_swizzle(__double2loint(v), 0x101F), hi = __builtin_amdgcn_ds_swizzle(__double2hiint(v), 0x101F);
    return __hiloint2double(hi, lo);
}

// the 2x2 complex matrices of one U3: M[2 s' + s]
struct Q3Mat {
    double r[4], i[4];
};
// mode 0: U3; 1: its inverse U3^+; 2: its transpose
template <int MODE>
__device__ __forceinline__ Q3Mat q3_u3_mat(const U3t& t) {
    const double epr = t.cp * t.cl - t.sp * t.sl, epi = t.sp * t.cl + t.cp * t.sl;  // e^{i (phi + lam)}
    Q3Mat m;
    m.r[0] = t.c; m.i[0] = 0.0;
    const double u01r = -t.s * t.cl, u01i = -t.s * t.sl, u10r = t.s * t.cp, u10i = t.s * t.sp;
    if (MODE == 0) {
        m.r[1] = u01r; m.i[1] = u01i; m.r[2] = u10r; m.i[2] = u10i; m.r[3] = t.c * epr; m.i[3] = t.c * epi;
    } else if (MODE == 1) {
        m.r[1] = u10r; m.i[1] = -u10i; m.r[2] = u01r; m.i[2] = -u01i; m.r[3] = t.c * epr; m.i[3] = -(t.c * epi);
    } else {
        m.r[1] = u10r; m.i[1] = u10i; m.r[2] = u01r; m.i[2] = u01i; m.r[3] = t.c * epr; m.i[3] = t.c * epi;
    }
    return m;
}
// row mixing by a 2x2 on qubit q: (vr, vi) = this lane's entry, (wr, wi) = the partner's, bit = bit q of the lane's row
__device__ __forceinline__ void q3_mix2(const Q3Mat& m, bool bit, double& vr, double& vi, double wr, double wi) {
    const double ar = bit ? m.r[3] : m.r[0], ai = bit ? m.i[3] : m.i[0];
    const double br = bit ? m.r[2] : m.r[1], bi = bit ? m.i[2] : m.i[1];
    const double nr = fma(ar, vr, fma(-ai, vi, fma(br, wr, -(bi * wi))));
    const double ni = fma(ar, vi, fma(ai, vr, fma(br, wi, bi * wr)));
    vr = nr;
    vi = ni;
}
// row mixing by the 4x4 of position `tab` on the edge (a, b); idx = bit a | bit b << 1 of the lane's row.
// mode 0: G; 1: G^+; 2: G^T
template <int MODE>
__device__ __forceinline__ void q3_mix4(const double2* tab, int a, int b, int idx, double& vr, double& vi) {
    double sr[4], si[4];
    sr[0] = vr; si[0] = vi;
    sr[1] = q3_xchg(vr, a); si[1] = q3_xchg(vi, a);
    sr[2] = q3_xchg(vr, b); si[2] = q3_xchg(vi, b);
    sr[3] = q3_xchg(sr[1], b); si[3] = q3_xchg(si[1], b);
    double nr = 0.0, ni = 0.0;
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        const double2 e = tab[(MODE == 0 ? idx : (idx ^ m)) * 4 + m];
        const double ei = MODE == 1 ? -e.y : e.y;
        nr = fma(e.x, sr[m], fma(-ei, si[m], nr));
        ni = fma(e.x, si[m], fma(ei, sr[m], ni));
    }
    vr = nr;
    vi = ni;
}

// E_j[i][m] = G_j[i][i ^ m] of every position into LDS (once per launch); the caller fences
__device__ __forceinline__ void q3_load_gates(double* lds, const double* gates, int k) {
    double2* tab = reinterpret_cast<double2*>(lds + kQ3OffGate);
    for (int e = threadIdx.x; e < 16 * k; e += kWave) {
        const int pos = e >> 4, i = (e >> 2) & 3, m = e & 3;
        tab[e] = *reinterpret_cast<const double2*>(gates + 32 * pos + (i * 4 + (i ^ m)) * 2);
    }
}

// row mixing by the 8x8 whose table is `tab` on the triple (a, b, c); idx = bit a | bit b << 1 | bit c << 2 of the lane's row.
// The running value walks the lane masks 0, 1, 3, 2, 6, 7, 5, 4; mask x pairs with the gate-local m = x^-1(mask).  Modes as q3_mix4.
template <int MODE>
__device__ __forceinline__ void q3_mix8(const double2* tab, int a, int b, int c, int idx, double& vr, double& vi) {
    double cr = vr, ci = vi, nr = 0.0, ni = 0.0;
#pragma unroll
    for (int t = 0; t < 8; ++t) {
        const int x = t ^ (t >> 1);  // Gray code: the lane mask of step t
        const int m = ((x >> a) & 1) | (((x >> b) & 1) << 1) | (((x >> c) & 1) << 2);
        const double2 e = tab[(MODE == 0 ? idx : (idx ^ m)) * 8 + m];
        const double ei = MODE == 1 ? -e.y : e.y;
        nr = fma(e.x, cr, fma(-ei, ci, nr));
        ni = fma(e.x, ci, fma(ei, cr, ni));
        if (t < 7) {
            const int q = (t & 1) == 0 ? 0 : (t == 3 ? 2 : 1);  // the bit in which the masks of steps t and t + 1 differ
            cr = q3_xchg(cr, q);
            ci = q3_xchg(ci, q);
        }
    }
    vr = nr;
    vi = ni;
}
// E_g[i][m] = G_g[i][i ^ m] of every distinct three-qubit gate into LDS (once per launch); the caller fences
__device__ __forceinline__ void q3_load_gates3(double* lds, const double* gates3, int n_gates3) {
    double2* tab = reinterpret_cast<double2*>(lds + kQ3OffGate3);
    for (int e = threadIdx.x; e < 64 * n_gates3; e += kWave) {
        const int g = e >> 6, i = (e >> 3) & 7, m = e & 7;
        tab[e] = *reinterpret_cast<const double2*>(gates3 + 128 * g + (i * 8 + (i ^ m)) * 2);
    }
}

// the sum over the 8 lanes of this lane's column (lanes 8 c .. 8 c + 7), in each of them: the first three steps of wave_sum
__device__ __forceinline__ double q3_col_sum(double v) {
    v += dpp_f64<0xB1>(v);
    v += dpp_f64<0x4E>(v);
    v += dpp_f64<0x141>(v);
    return v;
}

// Entropy (base 2) of a one-qubit reduced state of unit trace from its determinant D, and dS/dD.  With s = sqrt(1 - 4 D) the
// eigenvalues are (1 -+ s) / 2; the small one is taken as lam = 2 D / (1 + s) (no cancellation near D = 0), and
// dS/dD = log2((1 - lam) / lam) / s = (2 / ln 2) atanh(s) / s.  The two singular points:
//   * D = 1/4 (s = 0, the maximally mixed state: every qubit of GHZ): the quotient is 0/0 with the limit 2 / ln 2 -- below s^2 = 1e-2
//     it is the series (2 / ln 2) sum_n s^(2 n) / (2 n + 1), nine terms (the first one left out is below 1e-20);
//   * D = 0 (lam = 0, a product state: every successful minimum): dS/dD diverges while dD vanishes -- where the clamped eigenvalue is
//     0 the qubit gives 0 to the loss and 0 to the gradient.
// D is clamped to [0, 1/4] (rounding puts it outside), so both outputs are finite for every finite D.
__device__ __forceinline__ double q3_qubit_entropy(double D, double& dSdD) {
    D = fmin(fmax(D, 0.0), 0.25);
    const double u = fma(-4.0, D, 1.0);
    const double s = sqrt(u);
    const double lam = 2.0 * D / (1.0 + s);
    if (!(lam > 0.0)) {
        dSdD = 0.0;
        return 0.0;
    }
    const double om = 1.0 - lam;
    const double l0 = log2(lam), l1 = log2(om);
    const double S = -(lam * l0 + om * l1);
    if (u < 1e-2) {
        double p = 1.0 / 19.0;
#pragma unroll
        for (int m = 17; m >= 1; m -= 2) p = fma(p, u, 1.0 / (double)m);
        dSdD = 2.8853900817779268 * p;  // 2 / ln 2
    } else {
        dSdD = (l1 - l0) / s;  // (s >= 0.1 here: the difference is at least 0.29, nothing cancels)
    }
    return S;
}

// ---------------------------------------------------------------------------------------------------------------------------
// Fused loss + gradient of one item by the whole wavefront.  In: the trial point in lds[kQ3OffX ..], this lane's target entry
// T[r][c], the gate tables in LDS.  Out: the loss (wave-uniform), the gradient in lds[kQ3OffG ..], this lane's entry of W.
// ---------------------------------------------------------------------------------------------------------------------------
// MIXED: `ext` and `n_mixed` are Q3MArgs' ext and n.
// STATE: the mutual-information objectives of a start state psi (SLAM_COST_MUTUAL_INFO, SLAM_COST_MUTUAL_INFO_SQUARE).  (tre, tim) is
// this lane's entry of the 8x8 whose column 0 is psi and whose other columns are zero; P starts there, so column 0 of P is the state
// v = W psi all the way (the other seven columns stay zero and idle), and (wre, wim) is this lane's entry of that matrix.  Only the
// seed of the backward pass differs: B^T has column 0 only, 2 conj(dL / d conj(v)) -- d loss = Re(sum B^T dP) as for the trace.
template <bool HUGE_ARGS, bool MIXED = false, bool STATE = false>
__device__ __forceinline__ double eval_q3(double* lds, double tre, double tim, int k, uint64_t edges, int cost_kind, double& wre, double& wim,
                                          uint64_t ext = 0, int n_mixed = 0) {
    const int lane = threadIdx.x;
    const int n = MIXED ? n_mixed : 9 + 6 * k;
    const double2* gtab3 = reinterpret_cast<const double2*>(lds + kQ3OffGate3);
    const double2* tbl = reinterpret_cast<const double2*>(lds + kQ3OffTbl);
    const double* xs = lds + kQ3OffX;
    double* gs = lds + kQ3OffG;
    double2* trig = reinterpret_cast<double2*>(lds + kQ3OffTrig);
    const double2* gtab = reinterpret_cast<const double2*>(lds + kQ3OffGate);
    // ---- 1. trig entries: lane l handles parameters 2 l and 2 l + 1
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int i = 2 * lane + h;
        if (i < n) {
            const double xv = xs[i];
            const double arg = (i % 3 == 0) ? 0.5 * xv : xv;
            double s, co;
            if constexpr (HUGE_ARGS) sincos_any(arg, tbl, s, co);
            else sincos_tbl(arg, tbl, s, co);
            trig[i] = make_double2(co, s);
        }
    }
    lds_fence();
    // ---- 2. forward: P = M_L ... M_1
    double pr = ((lane & 7) == (lane >> 3)) ? 1.0 : 0.0, pi = 0.0;
    if constexpr (STATE) {  // P_0 = psi in column 0
        pr = tre;
        pi = tim;
    }
    auto u3_fwd = [&](int base, int q) {
        const Q3Mat m = q3_u3_mat<0>(load_u3(reinterpret_cast<const double*>(trig), base));
        q3_mix2(m, (lane >> q) & 1, pr, pi, q3_xchg(pr, q), q3_xchg(pi, q));
    };
    u3_fwd(0, 0);
    u3_fwd(3, 1);
    u3_fwd(6, 2);
    int base = 9;  // (MIXED only: the first parameter of the position's U3s)
#pragma unroll 1
    for (int j = 0; j < k; ++j) {
        const int a = (int)(edges >> (4 * j)) & 3, b = (int)(edges >> (4 * j + 2)) & 3;
        if constexpr (MIXED) {
            const int c = (int)(ext >> (4 * j)) & 3;
            if (c != 3) {
                const int idx = ((lane >> a) & 1) | (((lane >> b) & 1) << 1) | (((lane >> c) & 1) << 2);
                q3_mix8<0>(gtab3 + 64 * ((int)(ext >> (4 * j + 2)) & 3), a, b, c, idx, pr, pi);
                u3_fwd(base, a);
                u3_fwd(base + 3, b);
                u3_fwd(base + 6, c);
                base += 9;
            } else {
                q3_mix4<0>(gtab + 16 * j, a, b, ((lane >> a) & 1) | (((lane >> b) & 1) << 1), pr, pi);
                u3_fwd(base, a);
                u3_fwd(base + 3, b);
                base += 6;
            }
        } else {
            q3_mix4<0>(gtab + 16 * j, a, b, ((lane >> a) & 1) | (((lane >> b) & 1) << 1), pr, pi);
            u3_fwd(9 + 6 * j, a);
            u3_fwd(12 + 6 * j, b);
        }
    }
    wre = pr;
    wim = pi;
    double fout, br, bi;
    if constexpr (STATE) {
        // ---- 3 (STATE). rho_q[s][s'] = sum over the rows with bit q = s of v conj(v at bit q := s'): the lane's entry, its partner
        // at XOR 1 << q, masked sums over the lane's own column -- three exchanges each, not a wave sum's four and eight lane reads:
        // the lanes of column 0 get rho_q, the others (all zeros) a zero matrix, S = 0 and a zero seed; S_q from D_q = det rho_q
        // per qubit its entropy, dS/dD and dD_q / d conj(v): at a row with bit q = t that is rho_q[1-t][1-t] v - rho_q[t][1-t] (v of
        // the partner row)
        const double m2 = fma(pr, pr, pi * pi);
        double S[3], dS[3], dr[3], di[3];
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            const bool bit = (lane >> q) & 1;
            const double wr = q3_xchg(pr, q), wi = q3_xchg(pi, q);
            const double r00 = q3_col_sum(bit ? 0.0 : m2), r11 = q3_col_sum(bit ? m2 : 0.0);
            const double cr = q3_col_sum(bit ? 0.0 : fma(pr, wr, pi * wi));  // rho_q[0][1] = sum v[bit 0] conj(v[bit 1])
            const double ci = q3_col_sum(bit ? 0.0 : fma(pi, wr, -(pr * wi)));
            S[q] = q3_qubit_entropy(fma(r00, r11, -fma(cr, cr, ci * ci)), dS[q]);
            const double dd = bit ? r00 : r11, oi = bit ? -ci : ci;
            dr[q] = fma(dd, pr, -fma(cr, wr, -(oi * wi)));
            di[q] = fma(dd, pi, -fma(cr, wi, oi * wr));
        }
        // a pure state: S(rho_ab) = S(rho_c), so I(a:b) = S_a + S_b - S_c = T - 2 S_c with T = S_0 + S_1 + S_2.
        // MutualInformation = sum_c I = T; MutualInformationSquare = sum_c (T - 2 S_c)^2, d/dS_q = 2 (4 S_q - T)
        const double T = S[0] + S[1] + S[2];
        const bool sq = (cost_kind == 4);
        if (sq) {
            double acc = 0.0;
#pragma unroll
            for (int q = 0; q < 3; ++q) acc = fma(fma(-2.0, S[q], T), fma(-2.0, S[q], T), acc);
            fout = acc;
        } else {
            fout = T;
        }
        fout = long_readlane(fout, 0);  // (lane 0 is in column 0)
        // B^T = 2 conj(dL / d conj(v))
        double gr = 0.0, gi = 0.0;
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            const double w = (sq ? 2.0 * fma(4.0, S[q], -T) : 1.0) * dS[q];
            gr = fma(w, dr[q], gr);
            gi = fma(w, di[q], gi);
        }
        br = 2.0 * gr;
        bi = -2.0 * gi;
    } else {
    // ---- 3. t = Tr(T^+ W), the loss and its seed z: d loss = Re(z dt)
    const double tr = wave_sum(fma(tre, pr, tim * pi));
    const double ti = wave_sum(fma(tre, pi, -(tim * pr)));
    const double at2 = tr * tr + ti * ti;
    const double rat = (at2 > 1e-300) ? fast_rsqrt(at2) : 0.0;
    const double at = at2 * rat;
    const double basic = 1.0 - 0.125 * at;  // BasicCost, cost_function.py:140-145
    const bool sq = (cost_kind == 1);       // SquareCost = 8/9 (2 L - L^2) of BasicCost L at d = 8 (cost_function.py:169-173)
    const double c0 = sq ? 16.0 / 9.0 : 1.0, c1 = sq ? -8.0 / 9.0 : 0.0, d1 = sq ? -16.0 / 9.0 : 0.0;
    fout = basic * fma(c1, basic, c0);
    const double inv = (0.125 * rat) * fma(d1, basic, c0);
    const double zr = -tr * inv, zi = ti * inv;
    // B^T = z conj(T)
    br = zr * tre + zi * tim;
    bi = zi * tre - zr * tim;
    }
    // ---- 4. backward: every factor undone on P and carried (transposed) through B^T, its derivatives on the way
    auto u3_bwd = [&](int base, int q) {
        const U3t t = load_u3(reinterpret_cast<const double*>(trig), base);
        const bool bit = (lane >> q) & 1;
        const double pbr = q3_xchg(br, q), pbi = q3_xchg(bi, q);
        const double oi = fma(pr, bi, pi * br);                                 // Im(P B^T), own entries
        const double xr = fma(pr, pbr, -(pi * pbi)), xi = fma(pr, pbi, pi * pbr);  // P (B^T of the partner row)
        double gph = bit ? -oi : 0.0;
        double gth = bit ? -0.5 * fma(t.cp, xr, t.sp * xi) : 0.5 * fma(t.cp, xr, -(t.sp * xi));
        const Q3Mat mi = q3_u3_mat<1>(t), mt = q3_u3_mat<2>(t);
        q3_mix2(mi, bit, pr, pi, q3_xchg(pr, q), q3_xchg(pi, q));
        q3_mix2(mt, bit, br, bi, pbr, pbi);
        double gla = bit ? -fma(pr, bi, pi * br) : 0.0;
        gth = wave_sum(gth);
        gph = wave_sum(gph);
        gla = wave_sum(gla);
        if (lane == 0) {
            gs[base] = gth;
            gs[base + 1] = gph;
            gs[base + 2] = gla;
        }
    };
#pragma unroll 1
    for (int j = k - 1; j >= 0; --j) {
        const int a = (int)(edges >> (4 * j)) & 3, b = (int)(edges >> (4 * j + 2)) & 3;
        if constexpr (MIXED) {
            const int c = (int)(ext >> (4 * j)) & 3;
            if (c != 3) {
                base -= 9;
                u3_bwd(base + 6, c);
                u3_bwd(base + 3, b);
                u3_bwd(base, a);
                const int idx = ((lane >> a) & 1) | (((lane >> b) & 1) << 1) | (((lane >> c) & 1) << 2);
                const double2* tab = gtab3 + 64 * ((int)(ext >> (4 * j + 2)) & 3);
                q3_mix8<1>(tab, a, b, c, idx, pr, pi);
                q3_mix8<2>(tab, a, b, c, idx, br, bi);
            } else {
                base -= 6;
                u3_bwd(base + 3, b);
                u3_bwd(base, a);
                const int idx = ((lane >> a) & 1) | (((lane >> b) & 1) << 1);
                q3_mix4<1>(gtab + 16 * j, a, b, idx, pr, pi);
                q3_mix4<2>(gtab + 16 * j, a, b, idx, br, bi);
            }
        } else {
            u3_bwd(12 + 6 * j, b);
            u3_bwd(9 + 6 * j, a);
            const int idx = ((lane >> a) & 1) | (((lane >> b) & 1) << 1);
            q3_mix4<1>(gtab + 16 * j, a, b, idx, pr, pi);
            q3_mix4<2>(gtab + 16 * j, a, b, idx, br, bi);
        }
    }
    u3_bwd(6, 2);
    u3_bwd(3, 1);
    u3_bwd(0, 0);
    lds_fence();
    return fout;
}

// this lane's entry of the item's 8x8: the target's T[r][c], or (STATE) of the matrix whose column 0 is the state [8][2] of that index
template <bool STATE>
__device__ __forceinline__ double2 q3_item_entry(const double* base, int64_t index, int lane, int ent) {
    if constexpr (STATE) return lane < 8 ? *reinterpret_cast<const double2*>(base + index * 16 + 2 * lane) : make_double2(0.0, 0.0);
    else return *reinterpret_cast<const double2*>(base + index * 128 + ent);
}

// the wavefront's LDS prologue
template <bool MIXED, class Args>
__device__ __forceinline__ void q3_prologue(double* lds, const Args& a) {
    load_sincos_table(reinterpret_cast<double2*>(lds + kQ3OffTbl), threadIdx.x);
    q3_load_gates(lds, a.gates, a.k);
    if constexpr (MIXED) q3_load_gates3(lds, a.gates3, a.n_gates3);
    lds_fence();
}

// ---------------------------------------------------------------------------------------------------------------------------
// slam_q3_eval / slam_q3m_eval: one item per wavefront, grid-stride
// ---------------------------------------------------------------------------------------------------------------------------
// (MIXED: LDS lets twelve of these wavefronts onto a CU, not sixteen -- see kQ3MLdsBytes)
// STATE (slam_q3s_eval): `targets` holds the start states [n][8][2], `unitary` the final states [M][8][2]
template <bool MIXED, bool STATE = false>
__global__ void __launch_bounds__(kWave, 4) eval_q3_kernel(std::conditional_t<MIXED, Q3MEvalArgs, Q3EvalArgs> a) {
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const int lane = threadIdx.x;
    int n = 9 + 6 * a.k;
    uint64_t ext = 0;
    if constexpr (MIXED) {
        n = a.n;
        ext = a.ext;
    }
    q3_prologue<MIXED>(lds, a);
    const int ent = ((lane & 7) * 8 + (lane >> 3)) * 2;  // entry (r, c) of a row-major 8x8
    for (int64_t m = blockIdx.x; m < a.n_items; m += gridDim.x) {
#pragma unroll
        for (int s = 0; s < kQ3Slots; ++s) {
            const int i = 2 * lane + s;
            lds[kQ3OffX + i] = i < n ? a.x[m * n + i] : 0.0;
        }
        lds_fence();
        const double2 t = q3_item_entry<STATE>(a.targets, (int64_t)a.target_of[m], lane, ent);
        double wr, wi;
        const double f = eval_q3<true, MIXED, STATE>(lds, t.x, t.y, a.k, a.edges, a.cost_kind, wr, wi, ext, n);
        if (lane == 0) a.loss[m] = f;
        if (a.grad) {
#pragma unroll
            for (int s = 0; s < kQ3Slots; ++s) {
                const int i = 2 * lane + s;
                if (i < n) a.grad[m * n + i] = lds[kQ3OffG + i];
            }
        }
        if constexpr (STATE) {
            if (a.unitary && lane < 8) *reinterpret_cast<double2*>(a.unitary + m * 16 + 2 * lane) = make_double2(wr, wi);
        } else {
            if (a.unitary) *reinterpret_cast<double2*>(a.unitary + m * 128 + ent) = make_double2(wr, wi);
        }
        lds_fence();
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// slam_q3_minimize: the quasi-Newton iteration of slam_long_minimize.inc (its body, copied: slam_q3_minimize.inc, shared with the
// Hamiltonian templates of slam_ham.hpp) around eval_q3; one body, instantiated for
// the two-qubit-only templates (MIXED = false) and the mixed ones; STATE (slam_q3s_minimize): `targets` holds the start states [n][8][2]
// ---------------------------------------------------------------------------------------------------------------------------
template <bool MIXED, bool STATE = false>
__global__ void __launch_bounds__(kWave, 3) minimize_q3_kernel(std::conditional_t<MIXED, Q3MArgs, Q3Args> args) {
#define Q3_MIN_SETUP     \
    int n = 9 + 6 * k;   \
    uint64_t ext = 0;    \
    if constexpr (MIXED) { \
        n = args.n;      \
        ext = args.ext;  \
    }
#define Q3_MIN_PROLOGUE q3_prologue<MIXED>(lds, args);
#define Q3_MIN_EVAL eval_q3<false, MIXED, STATE>(lds, tre, tim, k, args.edges, args.cost_kind, wre, wim, ext, n)
#include "slam_q3_minimize.inc"
#undef Q3_MIN_SETUP
#undef Q3_MIN_PROLOGUE
#undef Q3_MIN_EVAL
}

}  // namespace slamdev
