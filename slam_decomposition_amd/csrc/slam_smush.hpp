// slam_smush.hpp -- CircuitTemplateV2(param_vec_expand=...) with parallel-drive ("smush") gates (gfx950 only).
//
// Reference: ConversionGainSmushGate (src/slam/utils/gates/custom_gates.py:215-257, hamiltonian.py:114-144): a conversion-gain pulse
// with single-qubit drives during it, cut into N time slices with their own drive amplitudes,
//     G = U_{N-1} ... U_0,  U_s = exp(-i tau H_s),  tau = t / N,
//     H_s = gx[s] (A + A^+) + gy[s] (B + B^+) + gc (e^{i pc} A B^+ + h.c.) + gg (e^{i pg} A B + h.c.),  A = a (x) 1,  B = 1 (x) a.
// For pc, pg in {0, pi} every H_s is real symmetric and commutes with X (x) X.  In the basis Q = [b1 b2 b3 b4],
// b1 = (|00> + |11>) / sqrt2, b2 = (|01> + |10>) / sqrt2, b3 = (|00> - |11>) / sqrt2, b4 = (|01> - |10>) / sqrt2:
//     Q^T H_s Q = diag(h+, h-),  h+ = [[gg, gx + gy], [gx + gy, gc]],  h- = [[-gg, gy - gx], [gy - gx, -gc]]
// (pc = pi is gc -> -gc, pg = pi is gg -> -gg: the host folds the phases into the signs of the gc / gg maps).  A slice is two real
// symmetric 2x2 exponentials,
//     exp(-i tau h) = e^{-i tau m} [cos(tau w) 1 - i sin(tau w) / w (d Z + r X)],  m = (h11 + h22) / 2, d = (h11 - h22) / 2, r = h12,
// w = sqrt(d^2 + r^2), and G = Q diag(E+, E-) Q^T with E+- the products of the N slice blocks.  sin(tau w) / w and the derivative
// term (tau w cos(tau w) - sin(tau w)) / w^3 are functions of w^2 with a series branch near 0: w = 0 happens exactly at zero drives
// whenever gc = gg (the reference's CNOT row), and nothing divides by it.
//
// Every raw pulse value (gc, gg, gx[s], gy[s]) of gate j is affine in at most one of the gate's QN parameters:
// raw = scale * q[sel] + offset (sel = -1: constant), as for slam_v2_gate.  Parameter vector, index order: P0 .. P{6(k+1)-1} (the U
// gates, as slam_device.hpp), then the QN parameters of gate 1, gate 2, ...: n = 6 (k + 1) + QN k <= 128, k <= 6.
//
// Work decomposition (slam_long.hpp's): ONE WAVEFRONT per (target, restart) item; quad j owns layer j (K_j G_j, G_0 = 1), lane c column c
// forward and row c backward; prefix / suffix products by a Hillis-Steele scan through LDS.  The quad of a smush gate builds column c of
// G_j from the slice blocks (lane c runs the 2-vector chains of column (c == 1 || c == 2) of E+ and E-).  Backward, it forms the gate's
// 4x4 adjoint Gam = Pre_{j-1} Suf_j K_j (dL = Re Tr(Gam dG)) through LDS, turns it into the block adjoints Q^T Gam Q, and lane 0 (E+) and
// lane 1 (E-) run the 2x2 slice chains backwards (prefix P_s = S_s^+ P_{s+1}, suffix adjoint R_{s-1} = R_s S_s).
// The optimizer is the projected quasi-Newton loop of minimize_v2_kernel / oracle/pqn_port.py (box bounds, the metric restarted after a
// failed line search), one item per wavefront, the fp32 inverse Hessian in device memory as in minimize_long_kernel.
#pragma once
#include "slam_long.hpp"
#include "slam_v2.hpp"

namespace slamdev {

// (kSmushMaxSpan, kSmushMaxSlices, kSmushRaw, kSmushNP and SmushMap, the device copy of slam_smush_gate: slam_types.hpp)

// LDS of one wavefront, in doubles
constexpr int kSmOffTbl = 0;                                   // sincos table (64 double2)
constexpr int kSmOffX = kSmOffTbl + kSincosLdsDoubles;         // trial point x[NP]
constexpr int kSmOffG = kSmOffX + kSmushNP;                    // gradient g[NP]
constexpr int kSmOffTrig = kSmOffG + kSmushNP;                 // (cos, sin) of the 6 angles of every layer: [L][6] double2
constexpr int kSmOffPre = kSmOffTrig + 12 * kSmushMaxLayers;   // Pre_j, column-major 4x4 complex: [L][16] double2
constexpr int kSmOffQ = kSmOffPre + 32 * kSmushMaxLayers;      // Q_j
constexpr int kSmOffV = kSmOffQ + 32 * kSmushMaxLayers;        // per layer: V = Suf_j K_j, then Gam (row-major 4x4 complex)
constexpr int kSmOffGam = kSmOffV + 32 * kSmushMaxLayers;
constexpr int kSmOffE = kSmOffGam + 32 * kSmushMaxLayers;      // per layer: E+ and E- (column-major 2x2 complex): [L][2][4] double2
constexpr int kSmOffF32 = kSmOffE + 16 * kSmushMaxLayers;      // three fp32 vectors [NP] (mat-vec / update broadcasts)
constexpr int kSmLdsDoubles = kSmOffF32 + 3 * kSmushNP / 2;
constexpr size_t kSmLdsBytes = (size_t)kSmLdsDoubles * sizeof(double);

struct SmushEvalArgs {
    const double* targets;
    const double* x;          // [M][n]
    const int32_t* target_of; // [M]
    int64_t n_items;
    double* loss;
    double* grad;             // [M][n] or nullptr
    double* unitary;          // [M][32] or nullptr
    int32_t cost_kind;
    const SmushMap* maps;     // [k]
    int32_t k;
    int32_t qn;
};

struct SmushArgs {
    const double* targets;    // resident targets
    const int32_t* active;    // [n_active] target index per slot, or nullptr = identity
    int32_t n_active;
    int32_t restarts;
    const double* x0;         // [M][n] or nullptr
    const double* init_lo;    // [n] start points ~ U[init_lo, init_hi)
    const double* init_hi;
    const double* bound_lo;   // [n] box bounds (-inf / +inf: none)
    const double* bound_hi;
    int32_t maxiter;
    double gtol, stop_loss, gtol_far, far_loss, exit_loss;
    uint32_t flags;           // SLAM_FLAG_EARLY_EXIT | SLAM_FLAG_ORDERED
    uint64_t seed;
    int64_t target_base;
    int32_t cost_kind;
    const SmushMap* maps;     // [k]
    int32_t k;
    int32_t qn;
    int32_t bounded;          // 0: no finite bound (plain BFGS): no metric restart after a failed line search
    int32_t* solved;
    ItemRec* item_rec;        // [M]
    double* item_x;           // [M][n]
    StageCtl* ctl;
    float* hmem;              // [gridDim.x][n][kSmushNP]
    double* trace_loss;       // [M][trace_cap] or nullptr
    double* trace_x;          // [M][trace_cap][n]
    int32_t trace_cap;
};

// sincos of the table path; |x| >= 2e8 (far outside any pulse or angle the optimizer reaches) gives NaN -- no out-of-line call
__device__ __forceinline__ void sm_sincos(double x, const double2* tbl, double& s, double& c) {
    const bool ok = fabs(x) < kSincosTblLimit;
    sincos_tbl(ok ? x : 0.0, tbl, s, c);
    s = ok ? s : (double)NAN;
    c = ok ? c : (double)NAN;
}

// one slice block exp(-i tau h) = phi [C - i Sn (d Z + r X)], phi = e^{-i tau m}.  Also Sn = sin(tau w) / w and
// s2 = (tau w cos(tau w) - sin(tau w)) / w^3 (the derivative terms), both from u = (tau w)^2 with a series branch near 0.
struct SmSlice {
    double pr, pi;  // phi
    double C, Sn, s2;
};
__device__ __forceinline__ SmSlice sm_slice(double m, double d, double r, double tau, const double2* tbl) {
    SmSlice o;
    double sp, cp;
    sm_sincos(tau * m, tbl, sp, cp);
    o.pr = cp;
    o.pi = -sp;
    const double u = tau * tau * fma(d, d, r * r);
    const double x = sqrt(u);
    double sx, cx;
    sm_sincos(x, tbl, sx, cx);
    o.C = cx;
    double sinc, g;
    if (u < 0.04) {
        // sin(x) / x and (x cos x - sin x) / x^3 to < 1e-17 for x < 0.2
        sinc = 1.0 + u * (-1.0 / 6 + u * (1.0 / 120 + u * (-1.0 / 5040 + u * (1.0 / 362880 + u * (-1.0 / 39916800)))));
        g = -1.0 / 3 + u * (1.0 / 30 + u * (-1.0 / 840 + u * (1.0 / 45360 + u * (-1.0 / 3991680 + u * (1.0 / 518918400)))));
    } else {
        const double rx = 1.0 / x;
        sinc = sx * rx;
        g = fma(x, cx, -sx) * (rx * rx * rx);
    }
    o.Sn = tau * sinc;
    o.s2 = tau * tau * tau * g;
    return o;
}
// S as a 2x2 complex: S00 = phi (C - i Sn d), S11 = phi (C + i Sn d), S01 = S10 = phi (-i Sn r)
__device__ __forceinline__ void sm_slice_mat(const SmSlice& o, double d, double r, double (&Sr)[4], double (&Si)[4]) {
    const double a = o.Sn * d, b = o.Sn * r;
    // phi (C - i a)
    Sr[0] = o.pr * o.C + o.pi * a;  Si[0] = o.pi * o.C - o.pr * a;
    Sr[3] = o.pr * o.C - o.pi * a;  Si[3] = o.pi * o.C + o.pr * a;
    Sr[1] = o.pi * b;               Si[1] = -o.pr * b;  // phi (-i b)
    Sr[2] = Sr[1];                  Si[2] = Si[1];
}
// index 0 = (0,0), 1 = (0,1), 2 = (1,0), 3 = (1,1)

__device__ __forceinline__ double sm_raw(const SmushMap* mp, int r, const double* xg) {
    const int s = mp->sel[r];
    return s >= 0 ? fma(mp->scale[r], xg[s], mp->offset[r]) : mp->offset[r];
}

// 2x2 complex products, row-major index (0,0) (0,1) (1,0) (1,1)
__device__ __forceinline__ void c22_mul(const double (&ar)[4], const double (&ai)[4], const double (&br)[4], const double (&bi)[4], double (&cr)[4],
                                        double (&ci)[4]) {
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int l = 0; l < 2; ++l) {
            const double xr = ar[2 * i] * br[l] - ai[2 * i] * bi[l] + ar[2 * i + 1] * br[2 + l] - ai[2 * i + 1] * bi[2 + l];
            const double xi = ar[2 * i] * bi[l] + ai[2 * i] * br[l] + ar[2 * i + 1] * bi[2 + l] + ai[2 * i + 1] * br[2 + l];
            cr[2 * i + l] = xr;
            ci[2 * i + l] = xi;
        }
}
// C = A^+ B
__device__ __forceinline__ void c22_hmul(const double (&ar)[4], const double (&ai)[4], const double (&br)[4], const double (&bi)[4], double (&cr)[4],
                                         double (&ci)[4]) {
    double hr[4] = {ar[0], ar[2], ar[1], ar[3]}, hi[4] = {-ai[0], -ai[2], -ai[1], -ai[3]};
    c22_mul(hr, hi, br, bi, cr, ci);
}

// ---------------------------------------------------------------------------------------------------------------------------
// Fused loss + gradient of one item by the whole wavefront.  In: the trial point in lds[kSmOffX ..] (zeros beyond n), the target
// column of this lane.  Out: the loss (wave-uniform), the gradient in lds[kSmOffG ..], W = Pre_{L-1} in LDS.
// ---------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ double eval_smush(double* lds, const double (&tre)[4], const double (&tim)[4], const SmushMap* maps, int k, int qn,
                                             int cost_kind) {
    const int lane = threadIdx.x;
    const int c = lane & 3;
    const int j = lane >> 2;  // layer of this quad
    const int L = k + 1;
    const int np = 6 * L;
    const double2* tbl = reinterpret_cast<const double2*>(lds + kSmOffTbl);
    const double* xs = lds + kSmOffX;
    double* gs = lds + kSmOffG;
    double2* trig = reinterpret_cast<double2*>(lds + kSmOffTrig);
    double2* Pre = reinterpret_cast<double2*>(lds + kSmOffPre);
    double2* Q = reinterpret_cast<double2*>(lds + kSmOffQ);
    double2* Vx = reinterpret_cast<double2*>(lds + kSmOffV);
    double2* Gx = reinterpret_cast<double2*>(lds + kSmOffGam);
    double2* Ex = reinterpret_cast<double2*>(lds + kSmOffE);
    const bool mine = j < L;
    const int jg = (j >= 1 && j <= k) ? j - 1 : 0;  // gate j = 1..k of this quad
    const SmushMap* mp = maps + jg;
    const double* xg = xs + np + qn * jg;  // the gate's parameters

    // ---- 1. trig entries: lane c of quad j handles parameters c and c + 4 of layer j
    if (mine) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int m = c + 4 * h;
            if (m < 6) {
                const double xv = xs[6 * j + m];
                double s, co;
                sm_sincos((m == 0 || m == 3) ? 0.5 * xv : xv, tbl, s, co);
                trig[6 * j + m] = make_double2(co, s);
            }
        }
    }
    // ---- 2. column c of G_j: lane c runs column e = (c == 1 || c == 2) of E+ and E- through the slices
    double Fr[4], Fi[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) { Fr[r] = r == c ? 1.0 : 0.0; Fi[r] = 0.0; }
    if (mine && j >= 1) {
        const int N = mp->n_slices;
        const double tau = mp->t / (double)N;
        const double gc = sm_raw(mp, 0, xg), gg = sm_raw(mp, 1, xg);
        const double mP = 0.5 * (gg + gc), dP = 0.5 * (gg - gc);
        const int e = (c == 1 || c == 2) ? 1 : 0;
        double ur[2] = {e == 0 ? 1.0 : 0.0, e == 1 ? 1.0 : 0.0}, ui[2] = {0.0, 0.0};  // E+ column e
        double vr[2] = {ur[0], ur[1]}, vi[2] = {0.0, 0.0};                             // E- column e
        for (int s = 0; s < N; ++s) {
            const double gx = sm_raw(mp, 2 + s, xg), gy = sm_raw(mp, 2 + N + s, xg);
            double Sr[4], Si[4];
            {
                const double rP = gx + gy;
                sm_slice_mat(sm_slice(mP, dP, rP, tau, tbl), dP, rP, Sr, Si);
                const double a0r = Sr[0] * ur[0] - Si[0] * ui[0] + Sr[1] * ur[1] - Si[1] * ui[1];
                const double a0i = Sr[0] * ui[0] + Si[0] * ur[0] + Sr[1] * ui[1] + Si[1] * ur[1];
                const double a1r = Sr[2] * ur[0] - Si[2] * ui[0] + Sr[3] * ur[1] - Si[3] * ui[1];
                const double a1i = Sr[2] * ui[0] + Si[2] * ur[0] + Sr[3] * ui[1] + Si[3] * ur[1];
                ur[0] = a0r; ui[0] = a0i; ur[1] = a1r; ui[1] = a1i;
            }
            {
                const double rM = gy - gx;
                sm_slice_mat(sm_slice(-mP, -dP, rM, tau, tbl), -dP, rM, Sr, Si);
                const double a0r = Sr[0] * vr[0] - Si[0] * vi[0] + Sr[1] * vr[1] - Si[1] * vi[1];
                const double a0i = Sr[0] * vi[0] + Si[0] * vr[0] + Sr[1] * vi[1] + Si[1] * vr[1];
                const double a1r = Sr[2] * vr[0] - Si[2] * vi[0] + Sr[3] * vr[1] - Si[3] * vi[1];
                const double a1i = Sr[2] * vi[0] + Si[2] * vr[0] + Sr[3] * vi[1] + Si[3] * vr[1];
                vr[0] = a0r; vi[0] = a0i; vr[1] = a1r; vi[1] = a1i;
            }
        }
        if (c < 2) {  // E+ / E- column c for the backward pass (column-major: [blk][col][row])
            Ex[j * 8 + 0 + 2 * c] = make_double2(ur[0], ui[0]);
            Ex[j * 8 + 1 + 2 * c] = make_double2(ur[1], ui[1]);
            Ex[j * 8 + 4 + 2 * c] = make_double2(vr[0], vi[0]);
            Ex[j * 8 + 5 + 2 * c] = make_double2(vr[1], vi[1]);
        }
        const double sg = (c >= 2) ? -1.0 : 1.0;  // columns 2, 3 take -E-
        Fr[0] = 0.5 * fma(sg, vr[0], ur[0]); Fi[0] = 0.5 * fma(sg, vi[0], ui[0]);
        Fr[1] = 0.5 * fma(sg, vr[1], ur[1]); Fi[1] = 0.5 * fma(sg, vi[1], ui[1]);
        Fr[2] = 0.5 * fma(-sg, vr[1], ur[1]); Fi[2] = 0.5 * fma(-sg, vi[1], ui[1]);
        Fr[3] = 0.5 * fma(-sg, vr[0], ur[0]); Fi[3] = 0.5 * fma(-sg, vi[0], ui[0]);
    }
    lds_fence();
    // ---- 3. M_j = K_j G_j: column c into Pre_j and Q_j
    if (mine) {
        const U3t B = load_u3(reinterpret_cast<const double*>(trig), 6 * j), A = load_u3(reinterpret_cast<const double*>(trig), 6 * j + 3);
        u3_col(B, Fr[0], Fi[0], Fr[1], Fi[1]);
        u3_col(B, Fr[2], Fi[2], Fr[3], Fi[3]);
        u3_col(A, Fr[0], Fi[0], Fr[2], Fi[2]);
        u3_col(A, Fr[1], Fi[1], Fr[3], Fi[3]);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            Pre[j * 16 + c * 4 + r] = make_double2(Fr[r], Fi[r]);
            Q[j * 16 + c * 4 + r] = make_double2(Fr[r], Fi[r]);
        }
    }
    lds_fence();
    // ---- 4. scans: Pre_j <- Pre_j Pre_{j-s}, Q_j <- Q_{j+s} Q_j, s = 1, 2, 4
#pragma unroll 1
    for (int s = 1; s < L; s <<= 1) {
        const bool dp = mine && j >= s;
        const bool dq = j + s < L;
        double pr[4], pi[4], qr[4], qi[4];
        if (dp) {
            double br[4], bi[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const double2 e = Pre[(j - s) * 16 + c * 4 + r];
                br[r] = e.x; bi[r] = e.y;
            }
            mat_col(Pre + j * 16, br, bi, pr, pi);
        }
        if (dq) {
            double ar[4], ai[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const double2 e = Q[(j + s) * 16 + r * 4 + c];
                ar[r] = e.x; ai[r] = e.y;
            }
            row_mat(ar, ai, Q + j * 16, qr, qi);
        }
        lds_fence();
        if (dp) {
#pragma unroll
            for (int r = 0; r < 4; ++r) Pre[j * 16 + c * 4 + r] = make_double2(pr[r], pi[r]);
        }
        if (dq) {
#pragma unroll
            for (int r = 0; r < 4; ++r) Q[j * 16 + r * 4 + c] = make_double2(qr[r], qi[r]);
        }
        lds_fence();
    }
    // ---- 5. t = Tr(T^+ W), W = Pre_{L-1}; row c of Z = z T^+ (dL = Re Tr(Z dW))
    double pr = 0.0, pi = 0.0;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const double2 w = Pre[(L - 1) * 16 + c * 4 + r];
        pr = fma(tre[r], w.x, fma(tim[r], w.y, pr));
        pi = fma(tre[r], w.y, fma(-tim[r], w.x, pi));
    }
    quad_sum2(pr, pi);
    const double at2 = pr * pr + pi * pi;
    const double rat = (at2 > 1e-300) ? fast_rsqrt(at2) : 0.0;
    const double at = at2 * rat;
    const double basic = 1.0 - 0.25 * at;  // BasicCost, cost_function.py:140-145
    const bool sq = (cost_kind == 1);      // SquareCost = 0.8 (2 L - L^2) of BasicCost L (cost_function.py:169-173)
    const double c0 = sq ? 1.6 : 1.0, c1 = sq ? -0.8 : 0.0, d1 = sq ? -1.6 : 0.0;
    const double fout = basic * fma(c1, basic, c0);
    const double inv = (0.25 * rat) * fma(d1, basic, c0);
    const double zr = -pr * inv, zi = pi * inv;
    double Zr[4], Zi[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        Zr[r] = zr * tre[r] + zi * tim[r];
        Zi[r] = zi * tre[r] - zr * tim[r];
    }
    // ---- 6. the six derivatives of every layer (as eval_long), and V = Suf_j K_j of the gate layers
    if (mine) {
        const U3t B = load_u3(reinterpret_cast<const double*>(trig), 6 * j), A = load_u3(reinterpret_cast<const double*>(trig), 6 * j + 3);
        double Ur[4], Ui[4];
        if (j == L - 1) {
#pragma unroll
            for (int r = 0; r < 4; ++r) { Ur[r] = Zr[r]; Ui[r] = Zi[r]; }
        } else {
            row_mat(Zr, Zi, Q + (j + 1) * 16, Ur, Ui);  // row c of Suf_j = Z Q_{j+1}
        }
        if (j >= 1) {  // row c of V = Suf_j K_j (u3_row, slam_device.hpp; K = A (x) B: B on pairs (0,1), (2,3), A on (0,2), (1,3))
            double vr[4], vi[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) { vr[r] = Ur[r]; vi[r] = Ui[r]; }
            u3_row(B, vr[0], vi[0], vr[1], vi[1]);
            u3_row(B, vr[2], vi[2], vr[3], vi[3]);
            u3_row(A, vr[0], vi[0], vr[2], vi[2]);
            u3_row(A, vr[1], vi[1], vr[3], vi[3]);
#pragma unroll
            for (int r = 0; r < 4; ++r) Vx[j * 16 + c * 4 + r] = make_double2(vr[r], vi[r]);
        }
        double Hr[4], Hi[4], fr[4], fi[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const double2 e = Pre[j * 16 + c * 4 + r];
            Hr[r] = e.x; Hi[r] = e.y;
            fr[r] = e.x; fi[r] = e.y;
        }
        u3_col_inv(A, fr[0], fi[0], fr[2], fi[2]);
        u3_col_inv(A, fr[1], fi[1], fr[3], fi[3]);
        u3_col_inv(B, fr[0], fi[0], fr[1], fi[1]);
        u3_col_inv(B, fr[2], fi[2], fr[3], fi[3]);
        double part[6];
        const double m1 = im_mul(Ur[1], Ui[1], Hr[1], Hi[1]);
        const double m2 = im_mul(Ur[2], Ui[2], Hr[2], Hi[2]);
        const double m3 = im_mul(Ur[3], Ui[3], Hr[3], Hi[3]);
        part[1] = -(m1 + m3);
        part[4] = -(m2 + m3);
        double thA2 = 0.0;
        u3_row_dtheta_first(A, Ur[0], Ui[0], Ur[2], Ui[2], Hr[0], Hi[0], Hr[2], Hi[2], thA2);
        u3_row_dtheta_first(A, Ur[1], Ui[1], Ur[3], Ui[3], Hr[1], Hi[1], Hr[3], Hi[3], thA2);
        double tB01r, tB01i, tB23r, tB23i;
        u3_row_t(B, Ur[0], Ui[0], Ur[1], Ui[1], tB01r, tB01i);
        u3_row_t(B, Ur[2], Ui[2], Ur[3], Ui[3], tB23r, tB23i);
        double th01, la01, th23, la23;
        dtheta_dlam_last(B, Ur[0], Ui[0], tB01r, tB01i, fr[0], fi[0], fr[1], fi[1], th01, la01);
        dtheta_dlam_last(B, Ur[2], Ui[2], tB23r, tB23i, fr[2], fi[2], fr[3], fi[3], th23, la23);
        part[0] = th01 + th23;
        part[2] = la01 + la23;
        part[5] = -(im_mul(Ur[2], Ui[2], fr[2], fi[2]) + im_mul(Ur[3], Ui[3], fr[3], fi[3]));
        part[3] = 0.5 * thA2;
        quad_sum2(part[0], part[1]);
        quad_sum2(part[2], part[3]);
        quad_sum2(part[4], part[5]);
        const double v0 = c == 0 ? part[0] : (c == 1 ? part[1] : (c == 2 ? part[2] : part[3]));
        gs[6 * j + c] = v0;
        if (c < 2) gs[6 * j + 4 + c] = c == 0 ? part[4] : part[5];
    }
    lds_fence();
    // ---- 7. the gate adjoint Gam = Pre_{j-1} V, row c by lane c
    const bool gate = mine && j >= 1;
    if (gate) {
        double gr[4] = {0.0, 0.0, 0.0, 0.0}, gi[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            const double2 p = Pre[(j - 1) * 16 + a * 4 + c];  // P[c][a]
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const double2 v = Vx[j * 16 + a * 4 + b];   // V[a][b]
                gr[b] = fma(p.x, v.x, fma(-p.y, v.y, gr[b]));
                gi[b] = fma(p.x, v.y, fma(p.y, v.x, gi[b]));
            }
        }
#pragma unroll
        for (int b = 0; b < 4; ++b) Gx[j * 16 + c * 4 + b] = make_double2(gr[b], gi[b]);
        if (c == 0)
            for (int i = 0; i < qn; ++i) gs[np + qn * (j - 1) + i] = 0.0;
    }
    lds_fence();
    // ---- 8. block adjoints and the slice chains backwards: lane 0 E+, lane 1 E-
    if (gate && c < 2) {
        const int blk = c;
        const double sg = blk ? -1.0 : 1.0;
        const int I0[2] = {0, 1}, I1[2] = {3, 2};  // b1 / b3 on |00>, |11>; b2 / b4 on |01>, |10> (second entry signed by sg)
        double Rr[4], Ri[4];
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int l = 0; l < 2; ++l) {
                const double2 e00 = Gx[j * 16 + I0[i] * 4 + I0[l]], e01 = Gx[j * 16 + I0[i] * 4 + I1[l]];
                const double2 e10 = Gx[j * 16 + I1[i] * 4 + I0[l]], e11 = Gx[j * 16 + I1[i] * 4 + I1[l]];
                Rr[2 * i + l] = 0.5 * (e00.x + e11.x + sg * (e01.x + e10.x));
                Ri[2 * i + l] = 0.5 * (e00.y + e11.y + sg * (e01.y + e10.y));
            }
        double Pr[4], Pi[4];  // E of this block, row-major
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int l = 0; l < 2; ++l) {
                const double2 e = Ex[j * 8 + 4 * blk + 2 * l + i];
                Pr[2 * i + l] = e.x; Pi[2 * i + l] = e.y;
            }
        const int N = mp->n_slices;
        const double tau = mp->t / (double)N;
        const double gc = sm_raw(mp, 0, xg), gg = sm_raw(mp, 1, xg);
        const double m = sg * 0.5 * (gg + gc), d = sg * 0.5 * (gg - gc);
        double dgc = 0.0, dgg = 0.0;
        double* gq = gs + np + qn * (j - 1);
        for (int s = N - 1; s >= 0; --s) {
            const double gx = sm_raw(mp, 2 + s, xg), gy = sm_raw(mp, 2 + N + s, xg);
            const double r = blk ? gy - gx : gx + gy;
            const SmSlice o = sm_slice(m, d, r, tau, tbl);
            double Sr[4], Si[4];
            sm_slice_mat(o, d, r, Sr, Si);
            double tr[4], ti[4];
            c22_hmul(Sr, Si, Pr, Pi, tr, ti);  // P_s = S_s^+ P_{s+1}
#pragma unroll
            for (int q = 0; q < 4; ++q) { Pr[q] = tr[q]; Pi[q] = ti[q]; }
            double Br[4], Bi[4];
            c22_mul(Pr, Pi, Rr, Ri, Br, Bi);  // dL_s = Re Tr(B dS_s)
            // Im Tr(B S)
            const double tsi = Br[0] * Si[0] + Bi[0] * Sr[0] + Br[1] * Si[2] + Bi[1] * Sr[2] + Br[2] * Si[1] + Bi[2] * Sr[1] + Br[3] * Si[3] + Bi[3] * Sr[3];
            const double dm = tau * tsi;  // Re(-i tau Tr(B S))
            const double b0r = Br[0] + Br[3], b0i = Bi[0] + Bi[3];
            const double bzr = Br[0] - Br[3], bzi = Bi[0] - Bi[3];
            const double bxr = Br[1] + Br[2], bxi = Bi[1] + Bi[2];
            const double kr = d * bzr + r * bxr, ki = d * bzi + r * bxi;  // d bz + r bx
            // dS/dd = phi [-tau d Sn 1 - i d s2 (d Z + r X) - i Sn Z]: Re(phi (-tau d Sn b0 - i d s2 k - i Sn bz))
            const double xdr = -o.Sn * tau * d * b0r + d * o.s2 * ki + o.Sn * bzi;
            const double xdi = -o.Sn * tau * d * b0i - d * o.s2 * kr - o.Sn * bzr;
            const double dd = o.pr * xdr - o.pi * xdi;
            const double xrr = -o.Sn * tau * r * b0r + r * o.s2 * ki + o.Sn * bxi;
            const double xri = -o.Sn * tau * r * b0i - r * o.s2 * kr - o.Sn * bxr;
            const double dr = o.pr * xrr - o.pi * xri;
            double t2r[4], t2i[4];
            c22_mul(Rr, Ri, Sr, Si, t2r, t2i);  // R_{s-1} = R_s S_s
#pragma unroll
            for (int q = 0; q < 4; ++q) { Rr[q] = t2r[q]; Ri[q] = t2i[q]; }
            // block +: (m, d, r) = ((gg + gc) / 2, (gg - gc) / 2, gx + gy); block -: (-(gg + gc) / 2, (gc - gg) / 2, gy - gx)
            dgc += sg * 0.5 * (dm - dd);
            dgg += sg * 0.5 * (dm + dd);
            const double dr_other = __shfl_xor(dr, 1);
            if (blk == 0) {
                const int sx = mp->sel[2 + s], sy = mp->sel[2 + N + s];
                if (sx >= 0) gq[sx] += mp->scale[2 + s] * (dr - dr_other);
                if (sy >= 0) gq[sy] += mp->scale[2 + N + s] * (dr + dr_other);
            }
        }
        const double dgc_o = __shfl_xor(dgc, 1), dgg_o = __shfl_xor(dgg, 1);
        if (blk == 0) {
            const int s0 = mp->sel[0], s1 = mp->sel[1];
            if (s0 >= 0) gq[s0] += mp->scale[0] * (dgc + dgc_o);
            if (s1 >= 0) gq[s1] += mp->scale[1] * (dgg + dgg_o);
        }
    }
    lds_fence();
    return fout;
}

__device__ __forceinline__ void smush_prologue(double* lds) {
    load_sincos_table(reinterpret_cast<double2*>(lds + kSmOffTbl), threadIdx.x);
    lds_fence();
}

// ---------------------------------------------------------------------------------------------------------------------------
// slam_smush_eval_loss_grad: one item per wavefront
// ---------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kWave, 2) eval_smush_kernel(SmushEvalArgs a) {
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const int lane = threadIdx.x;
    const int n = 6 * (a.k + 1) + a.qn * a.k;
    smush_prologue(lds);
    for (int64_t item = blockIdx.x; item < a.n_items; item += gridDim.x) {
        const int64_t tgt = a.target_of[item];
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const int i = 2 * lane + s;
            lds[kSmOffX + i] = (i < n) ? a.x[item * n + i] : 0.0;
        }
        lds_fence();
        double tre[4], tim[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const double2 t = *reinterpret_cast<const double2*>(a.targets + tgt * 32 + (lane & 3) * 2 + 8 * r);
            tre[r] = t.x;
            tim[r] = t.y;
        }
        const double f = eval_smush(lds, tre, tim, a.maps, a.k, a.qn, a.cost_kind);
        if (lane == 0) a.loss[item] = f;
        if (a.grad) {
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                const int i = 2 * lane + s;
                if (i < n) a.grad[item * n + i] = lds[kSmOffG + i];
            }
        }
        if (a.unitary && lane < 16) {
            const double2 e = reinterpret_cast<const double2*>(lds + kSmOffPre)[a.k * 16 + lane];  // element (r = lane & 3, col = lane >> 2)
            const int r = lane & 3, cc = lane >> 2;
            a.unitary[item * 32 + (r * 4 + cc) * 2] = e.x;
            a.unitary[item * 32 + (r * 4 + cc) * 2 + 1] = e.y;
        }
        lds_fence();
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// Projected quasi-Newton minimisation (oracle/pqn_port.py without the cost constraint), one item per wavefront, persistent wavefronts
// pulling restart-major queue positions.  Lane l holds components 2 l and 2 l + 1 of x, g, p, hg; the fp32 inverse Hessian H (n rows of
// kSmushNP floats in device memory, this wavefront's slice; symmetric, so lane l's two COLUMNS of row j give its two components of H v)
// -- one mat-vec pass and one rank-2 update pass per accepted point.
// ---------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kWave, 1) minimize_smush_kernel(SmushArgs args) {
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const int lane = threadIdx.x;
    const int k = args.k;
    const int n = 6 * (k + 1) + args.qn * k;
    float* f32a = reinterpret_cast<float*>(lds + kSmOffF32);  // [NP] g' (mat-vec broadcast)
    float* f32b = f32a + kSmushNP;                             // [NP] s  (update broadcast)
    float* f32c = f32b + kSmushNP;                             // [NP] v
    float2* const Hm = reinterpret_cast<float2*>(args.hmem + (size_t)blockIdx.x * (size_t)n * kSmushNP) + lane;  // + j * 64: row j
    smush_prologue(lds);
    const unsigned n_act = (unsigned)args.n_active;
    const unsigned n_items = n_act * (unsigned)args.restarts;
    const bool early = args.flags & 1u, ordered = args.flags & 2u;
    unsigned rounds = 0;
    double lo[2], hi[2];
    bool in[2];
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        const int i = 2 * lane + s;
        in[s] = i < n;
        lo[s] = in[s] ? args.bound_lo[i] : 0.0;
        hi[s] = in[s] ? args.bound_hi[i] : 0.0;
    }
    const bool lane_in = 2 * lane < n;

    while (true) {
        unsigned pos = 0;
        if (lane == 0) pos = atomicAdd(&args.ctl->work_counter, 1u);
        pos = (unsigned)__builtin_amdgcn_readfirstlane((int)pos);
        if (pos >= n_items) break;
        const unsigned rs = pos / n_act;         // restart (restart-major queue: every target's restart r before any r + 1)
        const unsigned sl = pos - rs * n_act;    // stage slot
        const unsigned item = sl * (unsigned)args.restarts + rs;
        const int mine = args.restarts - (int)rs;
        if (early) {
            const int fl = __hip_atomic_load(&args.solved[sl], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (ordered ? (fl > mine) : (fl != 0)) {
                if (lane == 0) item_rec_store_dropped(args.item_rec + item, ST_PREEMPTED);
                continue;
            }
        }
        const int tgt = args.active ? args.active[sl] : (int)sl;
        double tre[4], tim[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const double2 t = *reinterpret_cast<const double2*>(args.targets + (int64_t)tgt * 32 + (lane & 3) * 2 + 8 * r);
            tre[r] = t.x;
            tim[r] = t.y;
        }
        double x[2], g[2], p[2], hg[2];
        {
            double x0v[2] = {0.0, 0.0};
            if (lane_in) {
                if (args.x0) {
                    x0v[0] = args.x0[(int64_t)item * n + 2 * lane];
                    x0v[1] = (2 * lane + 1 < n) ? args.x0[(int64_t)item * n + 2 * lane + 1] : 0.0;
                } else {
                    // Philox block `lane` = the parameter pair (2 lane, 2 lane + 1): x0_philox(seed, target, restart, k | 0x300, i)
                    uint32_t w[4];
                    philox4x32_10((uint32_t)lane, rs, (uint32_t)(tgt + (int)args.target_base), (uint32_t)(k | 0x300), (uint32_t)args.seed,
                                  (uint32_t)(args.seed >> 32), w);
                    x0v[0] = x0_from_words(w[0], w[1]);
                    x0v[1] = x0_from_words(w[2], w[3]);
#pragma unroll
                    for (int s = 0; s < 2; ++s) {
                        const int i = 2 * lane + s;
                        if (i < n) {
                            const double u = x0v[s] * (1.0 / 6.283185307179586476925286766559);
                            x0v[s] = fma(u, args.init_hi[i] - args.init_lo[i], args.init_lo[i]);
                        }
                    }
                }
            }
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                x[s] = in[s] ? fmin(fmax(x0v[s], lo[s]), hi[s]) : 0.0;
                g[s] = 0.0; p[s] = 0.0; hg[s] = 0.0;
            }
        }
        bool ident = true, scaled = false, fresh = true, done = false;
        double hs1 = 0.0, f = 0.0, alpha = 0.0, gp = 0.0, grow = 1.0, gnorm = 0.0;
        int iters = 0, nback = 0, nstall = 0, nev = 0, nacc = 0, nouter = 0, status = ST_MAXITER;
        while (!done) {
            // ---- trial point: projection of x + alpha p onto the box
            double xt[2], sv[2];
            double gs0 = 0.0;
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                xt[s] = in[s] ? fmin(fmax(fma(alpha, p[s], x[s]), lo[s]), hi[s]) : 0.0;
                sv[s] = xt[s] - x[s];
                gs0 = fma(g[s], sv[s], gs0);
                lds[kSmOffX + 2 * lane + s] = xt[s];
            }
            const double gs = wave_sum(gs0);
            lds_fence();
            const double ft = eval_smush(lds, tre, tim, args.maps, k, args.qn, args.cost_kind);
            ++rounds;
            ++nev;
            const bool finite = isfinite(ft);
            double gt[2];
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                const double v = in[s] ? lds[kSmOffG + 2 * lane + s] : 0.0;
                const bool blocked = (xt[s] <= lo[s] && v > 0.0) || (xt[s] >= hi[s] && v < 0.0);
                gt[s] = (finite && !blocked) ? v : 0.0;
            }
            const bool acc = fresh ? finite : (finite && ft <= f + kArmijoC1 * gs);
            const bool step = acc && !fresh;
            if (acc) {
                ++nacc;
                if (!step) { sv[0] = 0.0; sv[1] = 0.0; }
                // ---- q = H g' (fp32 metric; the identity while nothing of it is in memory)
                double qv[2];
                if (ident) {
                    qv[0] = (double)(float)gt[0];
                    qv[1] = (double)(float)gt[1];
                } else {
                    f32a[2 * lane] = (float)gt[0];
                    f32a[2 * lane + 1] = (float)gt[1];
                    lds_fence();
                    float a0 = 0.0f, a1 = 0.0f;
                    if (lane_in) {
                        for (int jr = 0; jr < n; ++jr) {
                            const float2 h = Hm[(size_t)jr * 64];
                            const float gj = f32a[jr];
                            a0 = fmaf(h.x, gj, a0);
                            a1 = fmaf(h.y, gj, a1);
                        }
                    }
                    qv[0] = (double)a0;
                    qv[1] = (double)a1;
                    lds_fence();
                }
                double sy = 0.0, yy = 0.0, ss = 0.0, sg = 0.0;
#pragma unroll
                for (int s = 0; s < 2; ++s) {
                    const double ya = gt[s] - g[s];
                    sy = fma(sv[s], ya, sy);
                    yy = fma(ya, ya, yy);
                    ss = fma(sv[s], sv[s], ss);
                    sg = fma(sv[s], gt[s], sg);
                }
                sy = wave_sum(sy);
                yy = wave_sum(yy);
                ss = wave_sum(ss);
                sg = wave_sum(sg);
                const bool too_short = sy < (1.0 - kWolfeC2) * (-gs);
                const bool curv = step && !too_short && sy > 0.0 && (sy * sy > (kCurvEps * kCurvEps) * (ss * yy));
                const bool first = curv && !scaled;
                scaled = scaled || curv;
                const double fac = first ? (sy * fast_rcp(yy)) : 1.0;
                hs1 = first ? fac - 1.0 : hs1;
                double yu = 0.0, ua[2];
#pragma unroll
                for (int s = 0; s < 2; ++s) {
                    qv[s] = fma(hs1, gt[s], qv[s]);
                    ua[s] = fma(-fac, hg[s], qv[s]);
                    yu = fma(gt[s] - g[s], ua[s], yu);
                }
                yu = wave_sum(yu);
                const double rho = curv ? fast_rcp(sy) : 0.0;
                const double cf = rho * (1.0 + rho * yu);
                double wa[2], va[2], wg = 0.0;
#pragma unroll
                for (int s = 0; s < 2; ++s) {
                    wa[s] = cf * sv[s] - rho * ua[s];
                    va[s] = -rho * ua[s];
                    wg = fma(wa[s], gt[s], wg);
                }
                wg = wave_sum(wg);
                // ---- H += s w^T + v s^T (fp32): row j gets s_j w + v_j s
                if (curv) {
                    f32b[2 * lane] = (float)sv[0];
                    f32b[2 * lane + 1] = (float)sv[1];
                    f32c[2 * lane] = (float)va[0];
                    f32c[2 * lane + 1] = (float)va[1];
                    lds_fence();
                    const float w0 = (float)wa[0], w1 = (float)wa[1], s0 = (float)sv[0], s1 = (float)sv[1];
                    if (lane_in) {
                        for (int jr = 0; jr < n; ++jr) {
                            float2 h = ident ? make_float2(jr == 2 * lane ? 1.0f : 0.0f, jr == 2 * lane + 1 ? 1.0f : 0.0f) : Hm[(size_t)jr * 64];
                            const float sj = f32b[jr], vj = f32c[jr];
                            h.x = fmaf(vj, s0, h.x); h.y = fmaf(vj, s1, h.y);
                            h.x = fmaf(sj, w0, h.x); h.y = fmaf(sj, w1, h.y);
                            Hm[(size_t)jr * 64] = h;
                        }
                    }
                    ident = false;
                    lds_fence();
                }
                nstall = (step && (f - ft) <= kStallDf) ? nstall + 1 : 0;
                f = ft;
                if (step) ++iters;
                nback = 0;
                grow = (step && too_short) ? fmin(grow * kGrowFactor, kGrowMax) : 1.0;
#pragma unroll
                for (int s = 0; s < 2; ++s) {
                    x[s] = xt[s];
                    g[s] = gt[s];
                    hg[s] = qv[s] + sv[s] * wg + va[s] * sg;
                    const bool out = (x[s] <= lo[s] && hg[s] > 0.0) || (x[s] >= hi[s] && hg[s] < 0.0);
                    p[s] = (out || !in[s]) ? 0.0 : -hg[s];
                }
                if (args.trace_loss && step && iters <= args.trace_cap) {  // (wave-uniform; nothing when off)
                    const int64_t row = (int64_t)item * args.trace_cap + (iters - 1);
                    if (lane == 0) args.trace_loss[row] = f;
#pragma unroll
                    for (int s = 0; s < 2; ++s)
                        if (in[s]) args.trace_x[row * n + 2 * lane + s] = x[s];
                }
            } else if (fresh) {
                f = ft;
                status = ST_NONFINITE;
                break;
            } else {
                const double denom = 2.0 * (ft - f - gs);
                const double anew = (finite && denom > 0.0 && isfinite(denom)) ? (-gs * alpha * fast_rcp(denom)) : 0.5 * alpha;
                alpha = fmin(fmax(anew, 0.1 * alpha), 0.5 * alpha);
                grow = 1.0;
                ++nback;
            }
            {
                double m = 0.0, d1 = 0.0, d2 = 0.0;
#pragma unroll
                for (int s = 0; s < 2; ++s) {
                    const bool blocked = (x[s] <= lo[s] && g[s] > 0.0) || (x[s] >= hi[s] && g[s] < 0.0);
                    m = max_abs(m, blocked ? 0.0 : g[s]);
                    d1 = fma(g[s], p[s], d1);
                    d2 = fma(p[s], p[s], d2);
                }
                gnorm = wave_max_abs(m);
                gp = wave_sum(d1);
                const double pp = wave_sum(d2);
                if (acc) {
                    alpha = (pp > 1e-300) ? fmin(grow, kStepMax * fast_rsqrt(pp)) : grow;
                    if (f < args.stop_loss || gnorm < args.gtol || (gnorm < args.gtol_far && f > args.far_loss)) { status = ST_CONVERGED; done = true; }
                    else if (nstall >= 2) { status = ST_STALLED; done = true; }
                    else if (iters >= args.maxiter) { status = ST_MAXITER; done = true; }
                } else if (nback > kMaxBacktrack) {
                    status = (gnorm < kStallGnorm) ? ST_STALLED : ST_LINESEARCH;
                    done = true;
                }
            }
            fresh = false;
            const bool periodic = step && !done && ((iters & (kRestartPeriod - 1)) == 0);
            if (!done && (!(gp < 0.0) || periodic)) {
                ident = true;
                hs1 = 0.0;
                scaled = periodic ? false : scaled;
                double gg2 = 0.0;
#pragma unroll
                for (int s = 0; s < 2; ++s) {
                    hg[s] = g[s];
                    const bool out = (x[s] <= lo[s] && g[s] > 0.0) || (x[s] >= hi[s] && g[s] < 0.0);
                    p[s] = (out || !in[s]) ? 0.0 : -g[s];
                    gg2 = fma(g[s], p[s], gg2);
                }
                gp = wave_sum(gg2);
                if (periodic) alpha = (gp < -1e-300) ? fmin(grow, kStepMax * fast_rsqrt(-gp)) : grow;
                if (!(gp < 0.0)) { status = ST_CONVERGED; done = true; }  // a KKT point of the box-constrained problem
            }
            // a failed line search with bounds: the metric starts over from the identity at the same point (pqn_port.py)
            if (args.bounded && done && status == ST_LINESEARCH && nouter < kMaxMultiplierUpdates) {
                ident = true;
                hs1 = 0.0;
                scaled = false;
                ++nouter;
                done = false; fresh = true; alpha = 0.0; nstall = 0; nback = 0; status = ST_MAXITER;
            }
            // ---- early exit across the restarts of one target (optimizer.py:287-295)
            if (early && !done) {
                const int fl = __hip_atomic_load(&args.solved[sl], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (ordered ? (fl > mine) : (fl != 0)) { status = ST_PREEMPTED; done = true; }
            }
        }
        if (early && status != ST_PREEMPTED && f < args.exit_loss && lane == 0)
            __hip_atomic_fetch_max(&args.solved[sl], mine, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (lane == 0) item_rec_store(args.item_rec + item, f, iters, status, nev, nacc);
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const int i = 2 * lane + s;
            if (i < n) args.item_x[(int64_t)item * n + i] = x[s];
        }
    }
    if (lane == 0 && rounds) atomicAdd(&args.ctl->rounds, (unsigned long long)rounds);
}

}  // namespace slamdev
