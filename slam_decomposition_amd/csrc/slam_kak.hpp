// slam_kak.hpp -- batched KAK decomposition and local-gate completion on the device (gfx950 only).
//
// U = e^{i phase} (A1 (x) A2) CAN(c) (B1 (x) B2),  CAN(c) = exp(i pi/2 (c1 XX + c2 YY + c3 ZZ)),  A1, A2, B1, B2 in SU(2), c in the Weyl
// chamber of weyl_c1c2c3 (slam_weyl.hpp).  The reference leaves this step to qiskit's KAK code in its transpiler pass and names the
// gap VariationalTemplate.undo_invariant_transform (src/slam/basis_abc.py:86-90, a stub).
//
// weyl_c1c2c3 diagonalises m = U_B U_B^T (U_B = Q^+ U Q, magic basis) with joint Jacobi sweeps and keeps the eigenvalues only.  The
// rotations it discards are the local gates: with V^T m V = D,
//     U_B = O1 F O2,   O1 = V,   F = D^{1/2},   O2 = F^-1 V^T U_B  (real orthogonal because O2 O2^T = F^-1 D F^-1 = 1),
// whatever the degeneracy of D, and Q O Q^+ is in SU(2) (x) SU(2) for O in SO(4).  The chamber fold is bookkeeping on the columns:
//   * the half-phases S_k of D / sqrt(det U) are sorted, 1 is taken off the n = sum S largest and the list is rolled by n, exactly as
//     weyl_c1c2c3 does it: R_0..R_3 with c = (R0 + R1, R0 + R2, R1 + R2), sum R = 0.  Taking 1 off S_k is the other square root of D_k;
//   * Q^+ CAN(c) Q = diag(e^{i pi R_s(j)}) with s = (1, 0, 3, 2) for this Q, so column j of O1 is the Jacobi column that carries
//     R_s(j); an odd permutation is repaired by the sign of one column (a sign of a column of O1 and of the same row of O2 cancels);
//   * F_j = e^{i phase} e^{i pi R_s(j)}, phase = arg(det U) / 4 on the principal branches of weyl_c1c2c3: det F = det U because
//     sum R = 0, hence det O2 = +1 once det O1 = +1 -- no sign is tracked through the fold;
//   * the mirror c3 < 0 -> (1 - c1, c2, -c3) is a fixed local Clifford on each side:
//     CAN(c) = -i (iZ (x) iX) CAN(1 - c1, c2, -c3) (iY (x) 1).
// One thread per matrix, fp64 throughout; bookkeeping like weyl_c1c2c3, not a hot loop.  __device__ functions only: kak_kernel and
// complete_locals_kernel are in slam_geometry_kernels.hpp.
#pragma once
#include "slam_weyl.hpp"
#include "slam_pd.hpp"

namespace slamdev {

constexpr int kKakRecord = 36;  // phase, a1[2][2], a2[2][2], c[3], b1[2][2], b2[2][2] (complex entries as re, im)
constexpr int kKakBlock = 64;

struct Kak {
    double phase;
    cplx a1[2][2], a2[2][2], b1[2][2], b2[2][2];
    double c[3];
};

__device__ __forceinline__ cplx cconj(cplx a) { return {a.re, -a.im}; }
__device__ __forceinline__ cplx cscale(cplx a, double s) { return {a.re * s, a.im * s}; }

// the SU(2) matrix nearest to a multiple of one: [[a, b], [-b*, a*]] / sqrt(|a|^2 + |b|^2)
__device__ __forceinline__ void su2_project(cplx (&m)[2][2]) {
    cplx a = {0.5 * (m[0][0].re + m[1][1].re), 0.5 * (m[0][0].im - m[1][1].im)};
    cplx b = {0.5 * (m[0][1].re - m[1][0].re), 0.5 * (m[0][1].im + m[1][0].im)};
    const double r = 1.0 / sqrt(a.re * a.re + a.im * a.im + b.re * b.re + b.im * b.im);
    a = cscale(a, r);
    b = cscale(b, r);
    m[0][0] = a;
    m[0][1] = b;
    m[1][0] = {-b.re, b.im};
    m[1][1] = cconj(a);
}

__device__ __forceinline__ void mul2(const cplx (&x)[2][2], const cplx (&y)[2][2], cplx (&z)[2][2]) {
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int c = 0; c < 2; ++c) z[r][c] = cadd(cmul(x[r][0], y[0][c]), cmul(x[r][1], y[1][c]));
}
__device__ __forceinline__ void dagger2(const cplx (&x)[2][2], cplx (&z)[2][2]) {
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int c = 0; c < 2; ++c) z[r][c] = cconj(x[c][r]);
}

// K = Q O Q^+ of a real 4x4 O (in SO(4) up to rounding) split into K = a (x) b, a on the high bit of the basis index.  b comes from the
// 2x2 block of K of largest norm -- |a_rc| >= 1/sqrt(2) there, no small pivot --, a_rc = tr(b^+ K_rc) / 2; both are projected onto SU(2).
__device__ inline void magic_to_local(const double (&O)[4][4], cplx (&a)[2][2], cplx (&b)[2][2]) {
    const double h = 0.70710678118654752440;
    cplx T[4][4];  // T = Q O: rows of Q = h (1,0,0,i), h (0,i,1,0), h (0,i,-1,0), h (1,0,0,-i)
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        T[0][c] = {h * O[0][c], h * O[3][c]};
        T[1][c] = {h * O[2][c], h * O[1][c]};
        T[2][c] = {-h * O[2][c], h * O[1][c]};
        T[3][c] = {h * O[0][c], -h * O[3][c]};
    }
    cplx K[4][4];  // K = T Q^+: column j of Q^+ = conj(row j of Q)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const cplx t0 = T[r][0], t1 = T[r][1], t2 = T[r][2], t3 = T[r][3];
        K[r][0] = {h * (t0.re + t3.im), h * (t0.im - t3.re)};   // t0 - i t3
        K[r][1] = {h * (t1.im + t2.re), h * (-t1.re + t2.im)};  // -i t1 + t2
        K[r][2] = {h * (t1.im - t2.re), h * (-t1.re - t2.im)};  // -i t1 - t2
        K[r][3] = {h * (t0.re - t3.im), h * (t0.im + t3.re)};   // t0 + i t3
    }
    double best = -1.0;
    cplx blk[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            double nrm = 0.0;
#pragma unroll
            for (int r = 0; r < 2; ++r)
#pragma unroll
                for (int c = 0; c < 2; ++c) nrm += K[2 * i + r][2 * j + c].re * K[2 * i + r][2 * j + c].re + K[2 * i + r][2 * j + c].im * K[2 * i + r][2 * j + c].im;
            const bool take = nrm > best;
            best = take ? nrm : best;
#pragma unroll
            for (int r = 0; r < 2; ++r)
#pragma unroll
                for (int c = 0; c < 2; ++c) blk[r][c] = take ? K[2 * i + r][2 * j + c] : blk[r][c];
        }
    // b = blk / sqrt(det blk): the modulus is left to the projection
    const cplx dt = csub(cmul(blk[0][0], blk[1][1]), cmul(blk[0][1], blk[1][0]));
    double sn, cs;
    sincos(-0.5 * atan2(dt.im, dt.re), &sn, &cs);
    const cplx w = {cs, sn};
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int c = 0; c < 2; ++c) b[r][c] = cmul(blk[r][c], w);
    su2_project(b);
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            cplx s = {0.0, 0.0};
#pragma unroll
            for (int r = 0; r < 2; ++r)
#pragma unroll
                for (int c = 0; c < 2; ++c) s = cadd(s, cmul(cconj(b[r][c]), K[2 * i + r][2 * j + c]));
            a[i][j] = cscale(s, 0.5);
        }
    su2_project(a);
}

// the same product with the mirror image (1 - c1, c2, -c3) of c
__device__ inline void kak_mirror(Kak& k) {
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const cplx p = k.a1[r][0], q = k.a1[r][1];
        k.a1[r][0] = {-p.im, p.re};   // a1 iZ: column 0 times i, column 1 times -i
        k.a1[r][1] = {q.im, -q.re};
        const cplx s = k.a2[r][0], t = k.a2[r][1];
        k.a2[r][0] = {-t.im, t.re};   // a2 iX: columns swapped, times i
        k.a2[r][1] = {-s.im, s.re};
    }
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        const cplx p = k.b1[0][c], q = k.b1[1][c];
        k.b1[0][c] = q;               // iY b1, iY = [[0, 1], [-1, 0]]
        k.b1[1][c] = {-p.re, -p.im};
    }
    k.phase -= 1.57079632679489661923;
    k.c[0] = 1.0 - k.c[0];
    k.c[2] = -k.c[2];
}

__device__ inline double det4_real(const double (&A)[4][4]) {
    const double s0 = A[0][0] * A[1][1] - A[1][0] * A[0][1], s1 = A[0][0] * A[1][2] - A[1][0] * A[0][2];
    const double s2 = A[0][0] * A[1][3] - A[1][0] * A[0][3], s3 = A[0][1] * A[1][2] - A[1][1] * A[0][2];
    const double s4 = A[0][1] * A[1][3] - A[1][1] * A[0][3], s5 = A[0][2] * A[1][3] - A[1][2] * A[0][3];
    const double c5 = A[2][2] * A[3][3] - A[3][2] * A[2][3], c4 = A[2][1] * A[3][3] - A[3][1] * A[2][3];
    const double c3 = A[2][1] * A[3][2] - A[3][1] * A[2][2], c2 = A[2][0] * A[3][3] - A[3][0] * A[2][3];
    const double c1 = A[2][0] * A[3][2] - A[3][0] * A[2][2], c0 = A[2][0] * A[3][1] - A[3][0] * A[2][1];
    return s0 * c5 - s1 * c4 + s2 * c3 + s3 * c2 - s4 * c1 + s5 * c0;
}

// The KAK decomposition of the 4x4 unitary at Uin (row-major re, im).  The steps up to the sorted half-phases repeat weyl_c1c2c3
// operation for operation (that function stays as it is: its results are pinned), with the Jacobi rotations accumulated in V.
__device__ inline void kak_decompose(const double* __restrict__ Uin, Kak& out) {
    cplx U[4][4];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) U[r][c] = {Uin[(r * 4 + c) * 2], Uin[(r * 4 + c) * 2 + 1]};
    cplx det = cmul(U[0][0], det3(U, 1, 2, 3, 1, 2, 3));
    det = csub(det, cmul(U[0][1], det3(U, 1, 2, 3, 0, 2, 3)));
    det = cadd(det, cmul(U[0][2], det3(U, 1, 2, 3, 0, 1, 3)));
    det = csub(det, cmul(U[0][3], det3(U, 1, 2, 3, 0, 1, 2)));
    const double h = 0.70710678118654752440;
    cplx T[4][4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const cplx u0 = U[r][0], u1 = U[r][1], u2 = U[r][2], u3 = U[r][3];
        T[r][0] = {h * (u0.re + u3.re), h * (u0.im + u3.im)};
        T[r][1] = {h * (-u1.im - u2.im), h * (u1.re + u2.re)};
        T[r][2] = {h * (u1.re - u2.re), h * (u1.im - u2.im)};
        T[r][3] = {h * (-u0.im + u3.im), h * (u0.re - u3.re)};
    }
    cplx B[4][4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const cplx t0 = T[0][c], t1 = T[1][c], t2 = T[2][c], t3 = T[3][c];
        B[0][c] = {h * (t0.re + t3.re), h * (t0.im + t3.im)};
        B[1][c] = {h * (t1.im + t2.im), h * (-t1.re - t2.re)};
        B[2][c] = {h * (t1.re - t2.re), h * (t1.im - t2.im)};
        B[3][c] = {h * (t0.im - t3.im), h * (-t0.re + t3.re)};
    }
    double X[4][4], Y[4][4], V[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) V[i][j] = i == j ? 1.0 : 0.0;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = i; j < 4; ++j) {
            cplx s = {0.0, 0.0};
#pragma unroll
            for (int k = 0; k < 4; ++k) s = cadd(s, cmul(B[i][k], B[j][k]));
            X[i][j] = X[j][i] = s.re;
            Y[i][j] = Y[j][i] = s.im;
        }
    for (int sweep = 0; sweep < 12; ++sweep) {
        double off = 0.0;
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = i + 1; j < 4; ++j) off += X[i][j] * X[i][j] + Y[i][j] * Y[i][j];
        if (off < 1e-31) break;
#pragma unroll
        for (int p = 0; p < 3; ++p)
#pragma unroll
            for (int q = p + 1; q < 4; ++q) {
                const double h1x = X[p][p] - X[q][q], h1y = Y[p][p] - Y[q][q];
                const double h2x = 2.0 * X[p][q], h2y = 2.0 * Y[p][q];
                const double ton = (h1x * h1x + h1y * h1y) - (h2x * h2x + h2y * h2y);
                const double toff = 2.0 * (h1x * h2x + h1y * h2y);
                if (toff == 0.0 && ton >= 0.0) continue;
                const double theta = 0.25 * atan2(toff, ton);
                double sn, cs;
                sincos(theta, &sn, &cs);
#pragma unroll
                for (int w = 0; w < 3; ++w) {
                    double (&A)[4][4] = w == 0 ? X : (w == 1 ? Y : V);
#pragma unroll
                    for (int r = 0; r < 4; ++r) {  // columns p, q
                        const double ap = A[r][p], aq = A[r][q];
                        A[r][p] = cs * ap + sn * aq;
                        A[r][q] = -sn * ap + cs * aq;
                    }
                    if (w == 2) continue;  // V <- V G only
#pragma unroll
                    for (int c = 0; c < 4; ++c) {  // rows p, q
                        const double ap = A[p][c], aq = A[q][c];
                        A[p][c] = cs * ap + sn * aq;
                        A[q][c] = -sn * ap + cs * aq;
                    }
                }
            }
    }
    const double dabs = sqrt(sqrt(det.re * det.re + det.im * det.im));
    const double dphi = 0.5 * atan2(det.im, det.re);
    double sdn, sdc;
    sincos(dphi, &sdn, &sdc);
    const cplx isq = {sdc / dabs, -sdn / dabs};
    double S[4];
    int id[4] = {0, 1, 2, 3};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const cplx ev = cmul({X[k][k], Y[k][k]}, isq);
        double two_s = atan2(ev.im, ev.re) * 0.31830988618379067154;
        if (two_s <= -0.5 + 1e-12) two_s += 2.0;
        S[k] = 0.5 * two_s;
    }
    // sort descending, the columns with their phases (equal phases keep their order)
#define SLAM_KSWAP(a, b) { const bool sw_ = S[a] < S[b]; const double sa_ = S[a], sb_ = S[b]; const int ia_ = id[a], ib_ = id[b]; \
                           S[a] = sw_ ? sb_ : sa_; S[b] = sw_ ? sa_ : sb_; id[a] = sw_ ? ib_ : ia_; id[b] = sw_ ? ia_ : ib_; }
    SLAM_KSWAP(0, 1) SLAM_KSWAP(2, 3) SLAM_KSWAP(0, 2) SLAM_KSWAP(1, 3) SLAM_KSWAP(1, 2)
#undef SLAM_KSWAP
    int n = (int)rint(S[0] + S[1] + S[2] + S[3]);
    n = n < 0 ? 0 : (n > 3 ? 3 : n);
#pragma unroll
    for (int i = 0; i < 4; ++i)
        if (i < n) S[i] -= 1.0;
    double R[4];
    int col[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        R[i] = 0.0;
        col[i] = 0;
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const bool hit = s == ((i + n) & 3);
            R[i] = hit ? S[s] : R[i];
            col[i] = hit ? id[s] : col[i];
        }
    }
    out.c[0] = R[0] + R[1];
    out.c[1] = R[0] + R[2];
    out.c[2] = R[1] + R[2];
    // column j of the magic basis carries R_s(j), s = (1, 0, 3, 2)
    double O1[4][4], hj[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int s = j ^ 1;
        hj[j] = R[s];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            double v = V[r][0];
#pragma unroll
            for (int k = 1; k < 4; ++k) v = col[s] == k ? V[r][k] : v;
            O1[r][j] = v;
        }
    }
    if (det4_real(O1) < 0.0) {
#pragma unroll
        for (int r = 0; r < 4; ++r) O1[r][0] = -O1[r][0];
    }
    out.phase = 0.5 * dphi;
    // O2 = Re(F^-1 O1^T U_B)
    double O2[4][4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        double fs, fc;
        sincos(-(3.14159265358979323846 * hj[j] + out.phase), &fs, &fc);
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            double sr = 0.0, si = 0.0;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                sr += O1[r][j] * B[r][c].re;
                si += O1[r][j] * B[r][c].im;
            }
            O2[j][c] = fc * sr - fs * si;
        }
    }
    magic_to_local(O1, out.a1, out.a2);
    magic_to_local(O2, out.b1, out.b2);
    if (out.c[2] < 0.0) kak_mirror(out);
    out.c[0] += 0.0;
    out.c[1] += 0.0;
    out.c[2] += 0.0;
}

__device__ __forceinline__ void kak_store(const Kak& k, double* __restrict__ o) {
    o[0] = k.phase;
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            const int e = 2 * (2 * r + c);
            o[1 + e] = k.a1[r][c].re;
            o[2 + e] = k.a1[r][c].im;
            o[9 + e] = k.a2[r][c].re;
            o[10 + e] = k.a2[r][c].im;
            o[20 + e] = k.b1[r][c].re;
            o[21 + e] = k.b1[r][c].im;
            o[28 + e] = k.b2[r][c].re;
            o[29 + e] = k.b2[r][c].im;
        }
    o[17] = k.c[0];
    o[18] = k.c[1];
    o[19] = k.c[2];
}

// ---------------------------------------------------------------------------------
// Local-gate completion.  A fit up to single-qubit gates (MakhlinFunctionalCost, or a template without exterior layers) ends at x with
// W = template(x) = K1 T K2 for unknown local K1, K2.  With the KAK forms of W and T on the same chamber point,
//     T = e^{i .} (A_T A_W^+) W (B_W^+ B_T),
// so L = A_T A_W^+ goes into layer k and R = B_W^+ B_T into layer 0 of the template (W = K_k G_k ... G_1 K_0, K = U3(q1) (x) U3(q0),
// include/slam_hip.h).  The two chamber points are aligned first: on the c3 = 0 face (c1, c2, 0) and (1 - c1, c2, 0) are one class, so
// the mirror image of W's point is tried and kept when it is closer to T's (max norm); `gap` is that distance.
// ---------------------------------------------------------------------------------
struct CompleteArgs {
    int32_t k;
    int32_t seq[16];  // SLAM_MAX_SPAN_EVAL
    const double* gates;
    const double* targets;
    const double* x;
    const int32_t* target_of;
    int64_t M;
    double* x_out;
    double* loss_out;
    double* gap_out;
};

// W = K_k G_k ... G_1 K_0 of one parameter row
__device__ inline void template_forward(const CompleteArgs& a, const double* __restrict__ x, double (&wr)[4][4], double (&wi)[4][4]) {
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            wr[r][c] = r == c ? 1.0 : 0.0;
            wi[r][c] = 0.0;
        }
    for (int j = 0; j <= a.k; ++j) {
        if (j > 0) {
            const double* __restrict__ g = a.gates + 32 * (int64_t)a.seq[j - 1];
            double er[4][4], ei[4][4];
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    er[r][c] = g[(r * 4 + c) * 2];
                    ei[r][c] = g[(r * 4 + c) * 2 + 1];
                }
            pd_left_mul(er, ei, wr, wi);
        }
        const double* __restrict__ p = x + 6 * j;
        pd_u3_rows(p[0], p[1], p[2], 0, 1, wr, wi);  // qubit 0: the low bit of the basis index
        pd_u3_rows(p[0], p[1], p[2], 2, 3, wr, wi);
        pd_u3_rows(p[3], p[4], p[5], 0, 2, wr, wi);  // qubit 1: the high bit
        pd_u3_rows(p[3], p[4], p[5], 1, 3, wr, wi);
    }
}

// U3(theta, phi, lam) = [[c, -e^{i lam} s], [e^{i phi} s, e^{i (phi + lam)} c]]
__device__ inline void u3_matrix(const double* __restrict__ p, cplx (&m)[2][2]) {
    double s, c, sp, cp, sl, cl;
    sincos(0.5 * p[0], &s, &c);
    sincos(p[1], &sp, &cp);
    sincos(p[2], &sl, &cl);
    m[0][0] = {c, 0.0};
    m[0][1] = {-cl * s, -sl * s};
    m[1][0] = {cp * s, sp * s};
    m[1][1] = {(cp * cl - sp * sl) * c, (sp * cl + cp * sl) * c};
}

// (theta, phi, lam) with m = e^{i g} U3(theta, phi, lam) for a 2x2 unitary m.  The phases are read from the larger of the two
// entries of each column pair, so the result is finite and accurate at theta = 0 and theta = pi (atan2(0, 0) = 0 stands for the
// phase of an entry that vanishes; its value does not matter there).
__device__ inline void u3_angles(const cplx (&m)[2][2], double* __restrict__ p) {
    const double c = sqrt(m[0][0].re * m[0][0].re + m[0][0].im * m[0][0].im);
    const double s = sqrt(m[1][0].re * m[1][0].re + m[1][0].im * m[1][0].im);
    const double g = atan2(m[0][0].im, m[0][0].re);
    p[0] = 2.0 * atan2(s, c);
    p[1] = atan2(m[1][0].im, m[1][0].re) - g;
    p[2] = c >= s ? atan2(m[1][1].im, m[1][1].re) - g - p[1] : atan2(-m[0][1].im, -m[0][1].re) - g;
}

// ---------------------------------------------------------------------------------
// The steps that complete_locals_kernel (slam_geometry_kernels.hpp) and the closed-form kernels (slam_analytic.hpp, slam_cx.hpp,
// slam_b.hpp) share: a closed-form family computes its interior layers and its size rule, everything after that is here.
// ---------------------------------------------------------------------------------
// the three U3 angles of m at p
__device__ __forceinline__ void put_u3(const cplx (&m)[2][2], double* __restrict__ p) {
    double ang[3];
    u3_angles(m, ang);
    p[0] = ang[0];
    p[1] = ang[1];
    p[2] = ang[2];
}

// a 2x2 complex matrix, row-major (re, im)
__device__ __forceinline__ void load2(const double* __restrict__ p, cplx (&m)[2][2]) {
    m[0][0] = {p[0], p[1]};
    m[0][1] = {p[2], p[3]};
    m[1][0] = {p[4], p[5]};
    m[1][1] = {p[6], p[7]};
}

// Aligns the chamber point of kw with that of kt: the mirror image of kw's is taken where it is closer (max norm).  Returns the
// distance that remains, the `gap`.
__device__ __forceinline__ double kak_align(Kak& kw, const Kak& kt) {
    const double d0 = fmax(fmax(fabs(kw.c[0] - kt.c[0]), fabs(kw.c[1] - kt.c[1])), fabs(kw.c[2] - kt.c[2]));
    const double d1 = fmax(fmax(fabs(1.0 - kw.c[0] - kt.c[0]), fabs(kw.c[1] - kt.c[1])), fabs(-kw.c[2] - kt.c[2]));
    if (d1 < d0) kak_mirror(kw);
    return fmin(d0, d1);
}

// The exterior layers of a row whose interior circuit W has the KAK form kv, aligned with the target's kt: R = B_W^+ B_T at `bottom`
// (layer 0), L = A_T A_W^+ at `top` (layer k).  Index 1 of a pair acts on qubit 1 (angles 3..5 of a layer), index 2 on qubit 0.
__device__ __forceinline__ void exterior_layers(const Kak& kv, const Kak& kt, double* __restrict__ bottom, double* __restrict__ top) {
    cplx dg[2][2], m[2][2];
    dagger2(kv.b2, dg);
    mul2(dg, kt.b2, m);
    put_u3(m, bottom);
    dagger2(kv.b1, dg);
    mul2(dg, kt.b1, m);
    put_u3(m, bottom + 3);
    dagger2(kv.a2, dg);
    mul2(kt.a2, dg, m);
    put_u3(m, top);
    dagger2(kv.a1, dg);
    mul2(kt.a1, dg, m);
    put_u3(m, top + 3);
}

// the loss of the row x against the target T, from a forward pass of its own: 1 - |Tr(T^+ W(x))| / 4
__device__ __forceinline__ double template_loss(const CompleteArgs& fw, const double* __restrict__ T, const double* __restrict__ x,
                                                double (&wr)[4][4], double (&wi)[4][4]) {
    template_forward(fw, x, wr, wi);
    double tr = 0.0, ti = 0.0;
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const double t_re = T[(r * 4 + c) * 2], t_im = T[(r * 4 + c) * 2 + 1];
            tr += t_re * wr[r][c] + t_im * wi[r][c];
            ti += t_re * wi[r][c] - t_im * wr[r][c];
        }
    // tr^2 + ti^2 as the kernels have always formed it: the contraction is spelled out, so that where this is inlined cannot change it
    return 1.0 - 0.25 * sqrt(fma(tr, tr, ti * ti));
}

}  // namespace slamdev
