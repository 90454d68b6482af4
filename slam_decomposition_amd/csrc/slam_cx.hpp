// slam_cx.hpp -- closed-form decomposition into one, two or three gates of the CNOT class or of the iSWAP class on the device (gfx950
// only).  The counterpart of the reference's TwoQubitBasisDecomposer branch (src/slam/utils/transpiler_pass/weyl_decompose.py:475-480),
// which qiskit carries out there; the circuits are those of Vatan and Williams, quant-ph/0308006, checked here numerically.
//
// RP(t) = exp(-i t P / 2); in a (x) b the factor a acts on the qubit of the high bit.  CX12 = |0><0| (x) 1 + |1><1| (x) X,
// CX21 = 1 (x) |0><0| + X (x) |1><1|.  For every real t
//     V3(t)    = CX21 (1 (x) RY(t3)) CX12 (RZ(t1) (x) RY(t2)) CX21   is of the class of CAN(1/2 + t1/pi, 1/2 + t2/pi, 1/2 + t3/pi),
//     V2(a, b) = CX12 (RX(a) (x) RZ(b)) CX12                         is of the class of CAN(a/pi, b/pi, 0),
// so the interior angles are LINEAR in the KAK coordinates c of the target: t_j = pi (c_j - 1/2) for any representative c, a = pi c1,
// b = pi c2 where c3 = 0 -- no arccos, no inexact step.
//
// The basis gate.  The host writes G = e^{i .} (l1 (x) l0) C (r1 (x) r0) with C = CAN(1/2, 0, 0) (family 0, the CNOT class) or
// C = CAN(1/2, 1/2, 0) (family 1, the iSWAP class), and D = C (family 0) or D = SWAP C = C SWAP (family 1): D is of the CNOT class in both,
// CX12 = e^{i .} a12 D b12 and CX21 = e^{i .} a21 D b21 with fixed local a, b.  A circuit K_k D K_{k-1} ... D K_0 of D-gates is one of
// C-gates once the SWAPs are moved out: for family 1, SWAP K SWAP = sw(K) exchanges the two qubits of a local layer, so
//     k = 3:  SWAP T ~ K3 D K2 D K1 D K0   <=>   T ~ sw(K3) C K2 C sw(K1) C K0,     and SWAP CAN(c) ~ CAN(c + 1/2): t_j = pi c_j,
//     k = 2:       T ~ K2 D K1 D K0        <=>   T ~ K2 C sw(K1) C K0,
// and a circuit of C-gates is one of G-gates with r^+ on the left and l^+ on the right of every interior layer.  Only the INTERIOR
// layers are computed this way: each is L rot(axis, angle) R on either qubit, with L, R, the axis and the angle's index in a table of
// six entries that the host folds from the factors above (CxEntry; slam_analytic.hip).  The exterior layers come from aligning the
// interior circuit W (evaluated through G itself by template_forward) with the target: KAK forms of both, then kak_align and
// exterior_layers (slam_kak.hpp); `gap` is the distance that remains -- rounding for three gates, the target's distance from the
// c3 = 0 face (two gates) or from the gate's class (one gate) otherwise, at most the size rule's tolerance.
//
// The size is that of span_rules.minimal_span for the family on coordinates rounded to 8 digits, tolerance 2e-8: 1 in the gate's own
// class, 2 where |c3| < 2e-8, else 3; a local target gets a valid two-gate circuit.
//
// One thread per target, fp64.  kak_decompose is inlined once: the KAK forms of T and W come from a loop of two steps (the step is
// wave-uniform); the rows pass through x_out, read back by template_forward.  Everything after the interior layers and the size rule
// is the shared epilogue of slam_kak.hpp (kak_align, exterior_layers, template_loss).
#pragma once
#include "slam_kak.hpp"

namespace slamdev {

// one interior factor: m = L rot(axis, ang[src]) R.  axis: 0 none, 1 X, 2 Y, 3 Z
struct CxEntry {
    double L[8], R[8];  // 2x2 complex, row-major (re, im)
    double axis, src;
};
constexpr int kCxEntries = 6;                  // [slot][qubit]: slot 0 the layer of two gates, 1 and 2 the layers of three; qubit 0 first
constexpr int kCxTable = 32 + kCxEntries * 18;  // doubles in device memory: the gate, then the entries

struct CxArgs {
    const double* targets;  // [M][32]
    const double* table;    // [kCxTable]
    int64_t M;
    int32_t family;
    double* x_out;          // [M][24]
    int32_t* cycles;        // [M]
    double* loss;           // [M]
    double* gap;            // [M]
};

// the three U3 angles of L rot(axis, t) R
__device__ inline void cx_interior(const double* __restrict__ e, const double (&ang)[3], double* __restrict__ p) {
    cplx L[2][2], R[2][2], r[2][2], lr[2][2], m[2][2];
    load2(e, L);
    load2(e + 8, R);
    const int axis = (int)e[16], src = (int)e[17];
    const double t = src == 0 ? ang[0] : (src == 1 ? ang[1] : ang[2]);
    double s, c;
    sincos(0.5 * t, &s, &c);
    if (axis == 0) { c = 1.0; s = 0.0; }
    r[0][0] = {c, axis == 3 ? -s : 0.0};
    r[1][1] = {c, axis == 3 ? s : 0.0};
    r[0][1] = {axis == 2 ? -s : 0.0, axis == 1 ? -s : 0.0};
    r[1][0] = {axis == 2 ? s : 0.0, axis == 1 ? -s : 0.0};
    mul2(L, r, lr);
    mul2(lr, R, m);
    put_u3(m, p);
}

__global__ __launch_bounds__(kKakBlock) void cx_decompose_kernel(CxArgs a) {
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
    int k = 3;
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
            const double own2 = a.family ? 0.5 : 0.0;
            const bool same = fmax(fmax(fabs(c8[0] - 0.5), fabs(fabs(c8[1]) - own2)), fabs(c8[2])) < 2e-8;
            k = same ? 1 : (fabs(c8[2]) < 2e-8 ? 2 : 3);
            const double pi = 3.14159265358979323846;
            const double off = (k == 3 && a.family == 0) ? 0.5 : 0.0;
            const double ang[3] = {pi * (kt.c[0] - off), pi * (kt.c[1] - off), pi * (kt.c[2] - off)};
#pragma unroll
            for (int j = 0; j < 24; ++j) xo[j] = 0.0;
            const double* __restrict__ ent = a.table + 32;
            if (k == 2) {
                cx_interior(ent, ang, xo + 6);
                cx_interior(ent + 18, ang, xo + 9);
            } else if (k == 3) {
                cx_interior(ent + 36, ang, xo + 6);
                cx_interior(ent + 54, ang, xo + 9);
                cx_interior(ent + 72, ang, xo + 12);
                cx_interior(ent + 90, ang, xo + 15);
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
