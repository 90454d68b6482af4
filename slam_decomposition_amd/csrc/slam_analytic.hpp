// slam_analytic.hpp -- closed-form decomposition into two or three sqrt(iSWAP) gates on the device (gfx950 only).
//
// The reference's RootiSwapWeylDecomposition.riswapWeylDecomp (src/slam/utils/transpiler_pass/weyl_decompose.py:343-449) after Huang
// et al., arXiv:2105.06074, restated from the paper: the reference's transcription of the interior angle gamma (cos^2 y, and the
// denominator num + cos 2x + cos 2y cos 2z) and its `canonicalize` do not reproduce generic targets and are not followed.
//
// S = exp(i pi/8 (XX + YY)), class (1/4, 1/4, 0).  Coordinates c in units of pi, folded to c1 <= 1/2 by (c1, c2, c3) -> (1 - c1, c2, -c3);
// (x, y, z) = pi/2 c.  For |z| <= x - y the two-gate circuit V = S (C1 (x) C2) S has class (x, y, z) with
//     C     = sin(x + y - z) sin(x - y + z) sin(-x - y - z) sin(-x + y + z)              (clamped at 0)
//     alpha, beta = arccos(cos 2x - cos 2y + cos 2z +- 2 sqrt(C))                         (arguments clamped to [-1, 1])
//     num   = 4 cos^2 x cos^2 z sin^2 y,   den = num + cos 2x cos 2y cos 2z
//     gamma = arccos(s sqrt(num / den)),   s = +1 for z >= 0, -1 for z < 0                (den <= 0, the CNOT class: gamma = 0)
//     C1 = RZ(gamma) RX(alpha) RZ(gamma) = e^{-i gamma} U3(alpha, gamma - pi/2, gamma + pi/2),   C2 = RX(beta) = U3(beta, -pi/2, pi/2),
// C1 on the qubit of the high bit.  Otherwise three gates: CAN gates commute, CAN(c) = CAN(c - s) CAN(s) for each of the 12 signed
// placements s of (1/4, 1/4, 0), and CAN(s) = Ls S Rs with fixed local gates (shift_locals).  The placement whose reduced class
// f = fold(c - s) has the largest margin (f1 - f2) - |f3| is taken (the lowest index among equals; the margin is never negative), V(f)
// is built as above and aligned to CAN(c - s) by the KAK forms of both, CAN(c - s) ~ L1 V R1, so that with T = e^{i .} A CAN(c) B
//     T ~ (A L1) S C S (R1 Ls) S (Rs B).
// With two gates V(fold(c)) is aligned to T itself: T ~ L V R.  An alignment is kak_align (slam_kak.hpp): the mirror image of V's
// chamber point is taken where it is closer; `gap` is the distance that remains -- the error of the interior formula, which is the
// only inexact step (sqrt(ulp) where an arccos argument reaches +-1: on chamber faces).
//
// The size is that of span_rules.minimal_span, never below 2: |z| <= x - y + 2e-8 on coordinates rounded to 8 digits.  Local targets
// and targets of S's own class get a valid two-gate circuit.
//
// One thread per target, fp64.  kak_decompose is inlined once: the KAK forms of T, V and CAN(c - s) come from a loop of at most three
// steps (the step is wave-uniform); the template rows pass through x_out, read back by template_forward.  The alignment and the loss
// are the shared steps of slam_kak.hpp (kak_align, template_loss); the exterior layers are written out here, because those of three
// gates multiply the placement's local gates into the same four products that two gates use as they are.
#pragma once
#include "slam_kak.hpp"

namespace slamdev {

// RiSwapGate(1/2), row-major (re, im): template_forward's gate table
__device__ const double kSqiswapGate[32] = {1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0,
                                            0.0, 0.0, 0.70710678118654752440, 0.0, 0.0, 0.70710678118654752440, 0.0, 0.0,
                                            0.0, 0.0, 0.0, 0.70710678118654752440, 0.70710678118654752440, 0.0, 0.0, 0.0,
                                            0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0};

struct AnalyticArgs {
    const double* targets;  // [M][32]
    int64_t M;
    double* x_out;          // [M][24]
    int32_t* cycles;        // [M]
    double* loss;           // [M]
    double* gap;            // [M]
};

// the class of CAN(c), c anywhere, as (f1, f2, f3) with 1/2 >= f1 >= f2 >= |f3|: each coordinate modulo 1, any permutation, signs
// flipped in pairs
__device__ __forceinline__ void analytic_fold(const double (&c)[3], double (&f)[3]) {
    double a[3];
    int neg = 0;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const double r = c[j] - rint(c[j]);
        neg += r < 0.0 ? 1 : 0;
        a[j] = fabs(r);
    }
    double t;
#define SLAM_AF(i, j) { t = fmax(a[i], a[j]); a[j] = fmin(a[i], a[j]); a[i] = t; }
    SLAM_AF(0, 1) SLAM_AF(1, 2) SLAM_AF(0, 1)
#undef SLAM_AF
    f[0] = a[0];
    f[1] = a[1];
    f[2] = (neg & 1) ? -a[2] : a[2];
}

// placement i of (1/4, 1/4, 0): positions (0, 1), (0, 2), (1, 2) times signs ++, +-, -+, --
__device__ __forceinline__ void analytic_shift(int i, double (&s)[3]) {
    const int pos = i >> 2;
    const double sa = (i & 2) ? -0.25 : 0.25, sb = (i & 1) ? -0.25 : 0.25;
    s[0] = pos == 2 ? 0.0 : sa;
    s[1] = pos == 0 ? sb : (pos == 1 ? 0.0 : sa);
    s[2] = pos == 0 ? 0.0 : sb;
}

// CAN(s_i) = (g p (x) g) S (p^+ g^+ (x) g^+): g = 1, RX(pi/2), RY(pi/2) turns the XX + YY of S into the placement's pair of axes, the
// Pauli matrix p on one qubit flips the signs (Z both, X the second, Y the first of XX, YY).  Returns g and g p.
__device__ __forceinline__ void shift_locals(int i, cplx (&g)[2][2], cplx (&gp)[2][2]) {
    const double h = 0.70710678118654752440;
    const int pos = i >> 2, sg = i & 3;
    // p: 0 = 1, 1 = Z, 2 = X, 3 = Y
    const int p = sg == 0 ? 0 : (sg == 3 ? 1 : ((sg == 1) == (pos < 2) ? 2 : 3));
    if (pos == 0) {
        g[0][0] = {1.0, 0.0}; g[0][1] = {0.0, 0.0}; g[1][0] = {0.0, 0.0}; g[1][1] = {1.0, 0.0};
    } else if (pos == 1) {
        g[0][0] = {h, 0.0}; g[0][1] = {0.0, -h}; g[1][0] = {0.0, -h}; g[1][1] = {h, 0.0};
    } else {
        g[0][0] = {h, 0.0}; g[0][1] = {-h, 0.0}; g[1][0] = {h, 0.0}; g[1][1] = {h, 0.0};
    }
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const cplx a = g[r][0], b = g[r][1];
        if (p == 0) { gp[r][0] = a; gp[r][1] = b; }
        else if (p == 1) { gp[r][0] = a; gp[r][1] = {-b.re, -b.im}; }            // columns times (1, -1)
        else if (p == 2) { gp[r][0] = b; gp[r][1] = a; }                          // columns swapped
        else { gp[r][0] = {-b.im, b.re}; gp[r][1] = {a.im, -a.re}; }              // Y = [[0, -i], [i, 0]]: (i b, -i a)
    }
}

// the six angles of the layer C1 (x) C2 for the folded class f (units of pi): qubit 0 (C2), then qubit 1 (C1).  face: f is known to
// lie on the face |z| = x - y of the region, where C vanishes analytically; it is taken as 0 (alpha = beta) and not from its rounding
// residue (slam_sqapprox.hpp)
__device__ inline void analytic_interior(const double (&f)[3], double* __restrict__ p, bool face = false) {
    const double hp = 1.57079632679489661923;
    const double x = hp * f[0], y = hp * f[1], z = hp * f[2];
    const double C = face ? 0.0 : sin(x + y - z) * sin(x - y + z) * sin(-x - y - z) * sin(-x + y + z);
    const double rc = 2.0 * sqrt(fmax(C, 0.0));
    const double c2x = cos(2.0 * x), c2y = cos(2.0 * y), c2z = cos(2.0 * z);
    const double base = c2x - c2y + c2z;
    const double alpha = acos(fmin(fmax(base + rc, -1.0), 1.0));
    const double beta = acos(fmin(fmax(base - rc, -1.0), 1.0));
    const double cx = cos(x), cz = cos(z), sy = sin(y);
    const double num = 4.0 * cx * cx * cz * cz * sy * sy;
    const double den = num + c2x * c2y * c2z;
    double gamma = 0.0;
    if (den > 0.0) {
        const double rq = sqrt(fmin(fmax(num / den, 0.0), 1.0));
        gamma = acos(z < 0.0 ? -rq : rq);
    }
    p[0] = beta;
    p[1] = -hp;
    p[2] = hp;
    p[3] = alpha;
    p[4] = gamma - hp;
    p[5] = gamma + hp;
}

// CAN(c) in the computational basis (row-major re, im): (c1 - c2) sigma_x on span(00, 11) with phase pi/2 c3, (c1 + c2) sigma_x on
// span(01, 10) with phase -pi/2 c3
__device__ inline void analytic_can(const double (&c)[3], double (&u)[32]) {
    const double hp = 1.57079632679489661923;
    double sm, cm, sp, cp, s3, c3;
    sincos(hp * (c[0] - c[1]), &sm, &cm);
    sincos(hp * (c[0] + c[1]), &sp, &cp);
    sincos(hp * c[2], &s3, &c3);
#pragma unroll
    for (int j = 0; j < 32; ++j) u[j] = 0.0;
    const cplx e = {c3, s3}, ec = {c3, -s3};
    const cplx d0 = cmul(e, {cm, 0.0}), o0 = cmul(e, {0.0, sm}), d1 = cmul(ec, {cp, 0.0}), o1 = cmul(ec, {0.0, sp});
    u[0] = d0.re;  u[1] = d0.im;  u[6] = o0.re;  u[7] = o0.im;    // row 0: columns 0, 3
    u[10] = d1.re; u[11] = d1.im; u[12] = o1.re; u[13] = o1.im;   // row 1: columns 1, 2
    u[18] = o1.re; u[19] = o1.im; u[20] = d1.re; u[21] = d1.im;   // row 2: columns 1, 2
    u[24] = o0.re; u[25] = o0.im; u[30] = d0.re; u[31] = d0.im;   // row 3: columns 0, 3
}

// The three-gate construction of sqiswap_decompose_kernel in three pieces, for sqiswap_approx_decompose_kernel (slam_sqapprox.hpp).
// They are copies, statement for statement: the kernel below keeps its own statements, because moved onto these functions -- any one of
// them -- it compiles to another register allocation (gfx950, checked on the ISA), and its generated code stays as it is.
// The placement of the chamber point c whose reduced class has the largest margin (the lowest index among equals): its index into
// shift, the reduced class into f, c - s into raw.  All three keep what they held if no margin exceeds -1 (none does not).
__device__ __forceinline__ void analytic_best_shift(const double (&c)[3], int& shift, double (&f)[3], double (&raw)[3]) {
    double best = -1.0;
    for (int s = 0; s < 12; ++s) {
        double sh[3], fs[3];
        analytic_shift(s, sh);
        const double rs[3] = {c[0] - sh[0], c[1] - sh[1], c[2] - sh[2]};
        analytic_fold(rs, fs);
        const double m = (fs[0] - fs[1]) - fabs(fs[2]);
        if (m > best) {
            best = m;
            shift = s;
            f[0] = fs[0]; f[1] = fs[1]; f[2] = fs[2];
            raw[0] = rs[0]; raw[1] = rs[1]; raw[2] = rs[2];
        }
    }
}

// L = A A_V^+, R = B_V^+ B of the aligned pair (kv, kr); index 1 of a pair acts on qubit 1 (angles 3..5 of a layer), index 2 on qubit 0
__device__ __forceinline__ void analytic_align_products(const Kak& kv, const Kak& kr, cplx (&L1)[2][2], cplx (&L2)[2][2], cplx (&R1)[2][2],
                                                        cplx (&R2)[2][2]) {
    cplx dg[2][2];
    dagger2(kv.a1, dg);
    mul2(kr.a1, dg, L1);
    dagger2(kv.a2, dg);
    mul2(kr.a2, dg, L2);
    dagger2(kv.b1, dg);
    mul2(dg, kr.b1, R1);
    dagger2(kv.b2, dg);
    mul2(dg, kr.b2, R2);
}

// the row of three gates: T ~ (A L1) S C S (R1 Ls) S (Rs B) with the interior layer `mid` and the local gates of placement `shift`
__device__ __forceinline__ void analytic_row3(int shift, const Kak& kt, const cplx (&L1)[2][2], const cplx (&L2)[2][2], const cplx (&R1)[2][2],
                                              const cplx (&R2)[2][2], const double (&mid)[6], double* __restrict__ xo) {
    cplx g[2][2], gp[2][2], dg[2][2], m[2][2];
    shift_locals(shift, g, gp);
    // layer 0 = Rs B_T = (p^+ g^+ B1) (x) (g^+ B2)
    dagger2(g, dg);
    mul2(dg, kt.b2, m);
    put_u3(m, xo);
    dagger2(gp, dg);
    mul2(dg, kt.b1, m);
    put_u3(m, xo + 3);
    // layer 1 = R1 Ls = (R1 g p) (x) (R2 g)
    mul2(R2, g, m);
    put_u3(m, xo + 6);
    mul2(R1, gp, m);
    put_u3(m, xo + 9);
#pragma unroll
    for (int j = 0; j < 6; ++j) xo[12 + j] = mid[j];
    // layer 3 = A_T L1
    mul2(kt.a2, L2, m);
    put_u3(m, xo + 18);
    mul2(kt.a1, L1, m);
    put_u3(m, xo + 21);
}

__global__ __launch_bounds__(kKakBlock) void sqiswap_decompose_kernel(AnalyticArgs a) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.M) return;
    const double* __restrict__ T = a.targets + 32 * i;
    double* __restrict__ xo = a.x_out + 24 * i;
    CompleteArgs fw{};  // template_forward reads k, seq and gates
    fw.gates = kSqiswapGate;
    fw.k = 2;
    double u[32], wr[4][4], wi[4][4];
#pragma unroll
    for (int j = 0; j < 32; ++j) u[j] = T[j];
    Kak kt, kv, kr, cur;
    int k = 2, shift = 0;
    double raw[3] = {0.0, 0.0, 0.0};
#pragma unroll 1
    for (int step = 0; step < 3; ++step) {
        if (step == 2 && k == 2) break;
        kak_decompose(u, cur);
        if (step == 0) {
            kt = cur;
            // the size, on coordinates rounded to 8 digits as weyl_c1c2c3 rounds them
            double c8[3];
#pragma unroll
            for (int j = 0; j < 3; ++j) c8[j] = rint(kt.c[j] * 1e8) / 1e8;
            if (c8[0] > 0.5) {
                c8[0] = 1.0 - c8[0];
                c8[2] = -c8[2];
            }
            k = fabs(c8[2]) <= c8[0] - c8[1] + 2e-8 ? 2 : 3;
            double f[3] = {kt.c[0], kt.c[1], kt.c[2]};
            if (f[0] > 0.5) {
                f[0] = 1.0 - f[0];
                f[2] = -f[2];
            }
            if (k == 3) {
                double best = -1.0;
                for (int s = 0; s < 12; ++s) {
                    double sh[3], fs[3];
                    analytic_shift(s, sh);
                    const double rs[3] = {kt.c[0] - sh[0], kt.c[1] - sh[1], kt.c[2] - sh[2]};
                    analytic_fold(rs, fs);
                    const double m = (fs[0] - fs[1]) - fabs(fs[2]);
                    if (m > best) {
                        best = m;
                        shift = s;
                        f[0] = fs[0]; f[1] = fs[1]; f[2] = fs[2];
                        raw[0] = rs[0]; raw[1] = rs[1]; raw[2] = rs[2];
                    }
                }
            }
            // V = S C S through the row: zeros in layers 0 and 2
#pragma unroll
            for (int j = 0; j < 6; ++j) {
                xo[j] = 0.0;
                xo[12 + j] = 0.0;
            }
            analytic_interior(f, xo + 6);
            template_forward(fw, xo, wr, wi);
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    u[(r * 4 + c) * 2] = wr[r][c];
                    u[(r * 4 + c) * 2 + 1] = wi[r][c];
                }
        } else if (step == 1) {
            kv = cur;
            if (k == 3) analytic_can(raw, u);
        } else {
            kr = cur;
        }
    }
    // align V to T (two gates) or to CAN(c - s) (three): the side to align to is `kr`
    if (k == 2) kr = kt;
    a.gap[i] = kak_align(kv, kr);
    a.cycles[i] = k;
    // L = A A_V^+, R = B_V^+ B; index 1 of a pair acts on qubit 1 (angles 3..5 of a layer), index 2 on qubit 0.  Both sizes use the four
    // products, three gates with further factors, so they are formed once here and not through exterior_layers
    cplx dg[2][2], L1[2][2], L2[2][2], R1[2][2], R2[2][2], m[2][2];
    dagger2(kv.a1, dg);
    mul2(kr.a1, dg, L1);
    dagger2(kv.a2, dg);
    mul2(kr.a2, dg, L2);
    dagger2(kv.b1, dg);
    mul2(dg, kr.b1, R1);
    dagger2(kv.b2, dg);
    mul2(dg, kr.b2, R2);
    double mid[6];
#pragma unroll
    for (int j = 0; j < 6; ++j) mid[j] = xo[6 + j];
    if (k == 2) {
        put_u3(R2, xo);
        put_u3(R1, xo + 3);
        put_u3(L2, xo + 12);
        put_u3(L1, xo + 15);
#pragma unroll
        for (int j = 18; j < 24; ++j) xo[j] = 0.0;
    } else {
        cplx g[2][2], gp[2][2];
        shift_locals(shift, g, gp);
        // layer 0 = Rs B_T = (p^+ g^+ B1) (x) (g^+ B2)
        dagger2(g, dg);
        mul2(dg, kt.b2, m);
        put_u3(m, xo);
        dagger2(gp, dg);
        mul2(dg, kt.b1, m);
        put_u3(m, xo + 3);
        // layer 1 = R1 Ls = (R1 g p) (x) (R2 g)
        mul2(R2, g, m);
        put_u3(m, xo + 6);
        mul2(R1, gp, m);
        put_u3(m, xo + 9);
#pragma unroll
        for (int j = 0; j < 6; ++j) xo[12 + j] = mid[j];
        // layer 3 = A_T L1
        mul2(kt.a2, L2, m);
        put_u3(m, xo + 18);
        mul2(kt.a1, L1, m);
        put_u3(m, xo + 21);
    }
    fw.k = k;
    a.loss[i] = template_loss(fw, T, xo, wr, wi);
}

}  // namespace slamdev
