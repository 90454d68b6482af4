// slam_b.hpp -- closed-form decomposition into one or two gates of the B class on the device (gfx950 only).  Two B gates reach every
// two-qubit unitary (Zhang, Vala, Sastry, Whaley, PRL 93, 020502; span_rules.minimal_span, family b), so the formula covers all targets.
//
// RP(t) = exp(+i t P / 2) (the sign matters: the other one on the first qubit gives the mirror class); in a (x) b the factor a acts on
// the qubit of the high bit; B = CAN(1/2, 1/4, 0).  For a chamber point folded to 1/2 >= c1 >= c2 >= |c3| (units of pi;
// c1 > 1/2 -> (1 - c1, c2, -c3), span_rules._fold)
//     B (RY(pi c3) (x) RZ(bz) RY(by) RZ(bz)) B   is of the class of CAN(c1, c2, c3),
//     sin(by / 2) = sqrt(2) sin(pi c1 / 2) cos(pi c2 / 2),
//     bz = atan2(sqrt(max(cos(pi c1) cos(pi c2), 0)), sqrt(2) sin(pi c2 / 2) cos(pi c1 / 2)):
// the paper's arccos / arcsin forms rewritten so that nothing is divided and nothing is an acos of a value near 1
// (1 - 2 sin^2(pi c1 / 2) cos^2(pi c2 / 2) = cos^2(by / 2), cos(bz) cos(by / 2) = sqrt(2) sin(pi c2 / 2) cos(pi c1 / 2)).  On the face
// c1 = 1/2, bz has a square-root singularity in the distance from the face -- a property of the map, not an error: the circuit's
// coordinates depend on bz^2.  cos(pi c1) is formed there as sin(pi (1/2 - c1)), whose argument is exact, and the radicand is clamped at
// 0.  At the CNOT point both arguments of atan2 vanish: by = pi, and every bz gives the same layer.  The kernel needs the layer, not
// the angles: its entries are sin(by / 2) and the two arguments of the atan2, which are cos(by / 2) sin(bz) and cos(by / 2) cos(bz).
//
// The basis gate.  The host writes G = e^{i .} (l1 (x) l0) CAN(1/2, 1/4, 0) (r1 (x) r0) (to the size rule's tolerance), so a circuit of
// B-gates is one of G-gates with r^+ on the left and l^+ on the right of the interior layer: the table holds the gate, then r0^+, l0^+,
// r1^+, l1^+ (slam_analytic.hip).  The layer of qubit 0 is a general SU(2), not one rotation about an axis.  The exterior layers come
// from aligning the interior circuit W (evaluated through G itself by template_forward) with the target: KAK forms of both, then
// kak_align and exterior_layers (slam_kak.hpp); `gap` is the distance that remains -- rounding for two gates, the target's distance
// from the gate's class (at most the size rule's tolerance) for one.
//
// The size is that of span_rules.minimal_span for family b on coordinates rounded to 8 digits, tolerance 2e-8: 1 in the gate's own
// class, else 2; a local target gets a valid two-gate circuit.
//
// One thread per target, fp64.  kak_decompose is inlined once: the KAK forms of T and W come from a loop of two steps (the step is
// wave-uniform); the rows pass through x_out, read back by template_forward.  Everything after the interior layer and the size rule
// is the shared epilogue of slam_kak.hpp (kak_align, exterior_layers, template_loss).
#pragma once
#include "slam_kak.hpp"

namespace slamdev {

constexpr int kBTable = 32 + 4 * 8;  // doubles in device memory: the gate, then r0^+, l0^+, r1^+, l1^+ (2x2 complex, row-major re, im)

struct BArgs {
    const double* targets;  // [M][32]
    const double* table;    // [kBTable]
    int64_t M;
    double* x_out;          // [M][24]
    int32_t* cycles;        // [M]
    double* loss;           // [M]
    double* gap;            // [M]
};

// the three U3 angles of L q R, L and R at e and e + 8
__device__ inline void b_interior(const double* __restrict__ e, const cplx (&q)[2][2], double* __restrict__ p) {
    cplx L[2][2], R[2][2], lq[2][2], m[2][2];
    load2(e, L);
    load2(e + 8, R);
    mul2(L, q, lq);
    mul2(lq, R, m);
    put_u3(m, p);
}

__global__ __launch_bounds__(kKakBlock) void b_decompose_kernel(BArgs a) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.M) return;
    const double* __restrict__ T = a.targets + 32 * i;
    double* __restrict__ xo = a.x_out + 24 * i;
    CompleteArgs fw{};  // template_forward reads k, seq and gates
    fw.gates = a.table;
    double u[32], wr[4][4], wi[4][4];
#pragma unroll
    for (int j = 0; j < 32; ++j) u[j] = T[j];
    Kak kt, kv, cur;
    int k = 2;
#pragma unroll 1
    for (int step = 0; step < 2; ++step) {
        kak_decompose(u, cur);
        if (step == 1) {
            kv = cur;
        } else {
            kt = cur;
            // the size, on coordinates rounded to 8 digits as weyl_c1c2c3 rounds them
            double c8[3];
#pragma unroll
            for (int j = 0; j < 3; ++j) c8[j] = rint(kt.c[j] * 1e8) / 1e8;
            if (c8[0] > 0.5) {
                c8[0] = 1.0 - c8[0];
                c8[2] = -c8[2];
            }
            const bool same = fmax(fmax(fabs(c8[0] - 0.5), fabs(fabs(c8[1]) - 0.25)), fabs(c8[2])) < 2e-8;
            k = same ? 1 : 2;
#pragma unroll
            for (int j = 0; j < 24; ++j) xo[j] = 0.0;
            if (k == 2) {
                // the folded point: d = 1/2 - c1 >= 0 is exact near the face
                const bool up = kt.c[0] > 0.5;
                const double pi = 3.14159265358979323846, rt2 = 1.41421356237309504880;
                const double d = up ? kt.c[0] - 0.5 : 0.5 - kt.c[0];
                const double c1 = up ? 1.0 - kt.c[0] : kt.c[0], c2 = kt.c[1], c3 = up ? -kt.c[2] : kt.c[2];
                double s1, h1, s2, h2, s3, h3;
                sincos(0.5 * pi * c1, &s1, &h1);
                sincos(0.5 * pi * c2, &s2, &h2);
                sincos(0.5 * pi * c3, &s3, &h3);
                // RZ(bz) RY(by) RZ(bz) = [[e^{i bz} cos(by / 2), sin(by / 2)], [-sin(by / 2), e^{-i bz} cos(by / 2)]], and the two
                // arguments of the atan2 ARE cos(by / 2) sin(bz) and cos(by / 2) cos(bz): the layer is written from them, no angle is formed
                const double sy = fmin(rt2 * s1 * h2, 1.0);
                const double qr = rt2 * s2 * h1, qi = sqrt(fmax(sin(pi * d) * cos(pi * c2), 0.0));
                cplx q[2][2];
                q[0][0] = {qr, qi};
                q[0][1] = {sy, 0.0};
                q[1][0] = {-sy, 0.0};
                q[1][1] = {qr, -qi};
                // RY(pi c3) = [[h3, s3], [-s3, h3]]
                b_interior(a.table + 32, q, xo + 6);
                q[0][0] = {h3, 0.0};
                q[0][1] = {s3, 0.0};
                q[1][0] = {-s3, 0.0};
                q[1][1] = {h3, 0.0};
                b_interior(a.table + 48, q, xo + 9);
            }
            // W = the interior circuit, exterior layers still 1
            fw.k = k;
            template_forward(fw, xo, wr, wi);
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    u[(r * 4 + c) * 2] = wr[r][c];
                    u[(r * 4 + c) * 2 + 1] = wi[r][c];
                }
        }
    }
    a.gap[i] = kak_align(kv, kt);
    a.cycles[i] = k;
    exterior_layers(kv, kt, xo, xo + 6 * k);
    a.loss[i] = template_loss(fw, T, xo, wr, wi);
}

}  // namespace slamdev
