// slam_sc.hpp -- closed-form decomposition into 0, 1, 2 or 3 gates of ANY supercontrolled class CAN(1/2, beta, 0), 0 <= beta <= 1/2, on
// the device (gfx950 only): the line of the Weyl chamber whose points beta = 0, 1/4, 1/2 are the CNOT, the B and the iSWAP class
// (slam_cx.hpp, slam_b.hpp), and every full-strength conversion-gain gate (gc + gg = pi / 2 at t = 1) between them.  The reference hands
// these gates to qiskit's TwoQubitBasisDecomposer (src/slam/utils/transpiler_pass/weyl_decompose.py:475-480), which is exact for every
// supercontrolled gate -- three gates reach any target -- and chooses the size by expected fidelity; this is that construction.
//
// Ud(a, b, c) = exp(i (a XX + b YY + c ZZ)) = CAN(2a/pi, 2b/pi, 2c/pi); rz(t) = diag(e^{-i t/2}, e^{i t/2}); S = Ud(pi/4, beta', 0),
// beta' = pi beta / 2; e+- = e^{+-i beta'}, E+- = e^{+-2i beta'}; in a (x) b the factor a acts on the qubit of the high bit.  With
//     K11l = 1/(1+i) [[-i e-, e-], [-i e+, -e+]]        K11r = 1/sqrt2 [[i e-, -e-], [e+, -i e+]]
//     K3221l = 1/sqrt2 [[1 + i cos 2beta', i sin 2beta'], [i sin 2beta', 1 - i cos 2beta']]
//     K21r = 1/(1-i) [[-i E-, E-], [i E+, E+]]          K32r = 1/(1-i) [[e+, -e-], [-i e+, -i e-]]
//     K22l = 1/sqrt2 [[1, -1], [1, 1]]                  K22r = [[0, 1], [-1, 0]]                  ipz = [[i, 0], [0, -i]]
// the interior circuits (leftmost factor applied last)
//     three gates:  S (K3221l (x) K32r rz(-2c) K21r) S (K22l rz(-2a) K11l (x) K22r rz(2b) K11r) S      is of the class of Ud(a, b, c),
//     two gates:    S (K11l^+ rz(-2a) K11l (x) ipz K11r^+ rz(2b) K11r) S                                is of the class of Ud(a, b, 0)
// for every real a, b, c: any representative of the target's class serves, the chamber point with c1 > 1/2 included.  The construction's
// exterior factors (K12, K31, the target's own KAK factors) are not formed: as in the siblings the exterior layers come from aligning
// the interior circuit W -- evaluated through the gate itself by template_forward -- with the target, KAK forms of both
// (slam_kak.hpp), which also absorbs a gate up to 4e-8 off the line.
//
// The basis gate.  The host writes G = e^{i .} (l1 (x) l0) CAN(1/2, beta, 0) (r1 (x) r0) (slam_analytic.hip, sc_fold_dress), so every S is
// (l1^+ (x) l0^+) G (r1^+ (x) r0^+) and an interior layer K of the S-circuit is r^+ K l^+ in the G-circuit.  Each interior factor is a
// sandwich L rz(t) R; the table holds the gate, then six entries (L, R) with r^+ folded into L and l^+ into R:
//     0, 1  two gates, qubit 0 (t = pi c2), qubit 1 (t = -pi c1)
//     2, 3  three gates, first layer, qubit 0 (t = pi c2), qubit 1 (t = -pi c1)
//     4, 5  three gates, second layer, qubit 0 (t = -pi c3), qubit 1 (constant: L = r1^+ K3221l l1^+, R = 1, t = 0)
//
// Size: that of slam_approx.hpp word for word.  t_0, t_1 (with the gate's beta'), t_2 = |cos c|, t_3 = 1 on the kernel's unrounded
// coordinates folded to c1 <= 1/2, F_k = (4 + 16 t_k^2) / 20, E_k = F_k f^k, the largest E_k in the order 0, 1, 2, 3 with strict >.
// cos of anything below 1e-8 is exactly 1, so the ties of f = 1 are exact ties: no gate for a local target, one in the gate's own
// class, two on the plane c3 = 0, three elsewhere.  For 0 < beta < 1/2 the set that two gates reach exactly is a polytope larger than
// that plane; this formula is exact on the plane only, so a target off it gets three gates even where an optimiser finds two (at
// beta = 1/4 b_decompose_kernel returns two for every target).  Off the plane the two-gate circuit is the best of its kind,
// |Tr(T^+ W)| = 4 |cos c|.  The alignment takes the representative of W's class that the trace formula prefers, as
// approx_decompose_kernel does.
//
// sc_decompose_kernel: one thread per target, fp64, the shape of approx_decompose_kernel (one inlined kak_decompose in a wave-uniform
// loop of two steps, rows through x_out, the table at wave-uniform addresses).  sc_counts_kernel: the sweep, approx_counts_kernel with
// the gate's beta' in place of the family.
#pragma once
#include "slam_approx.hpp"

namespace slamdev {

constexpr int kScEntries = 6;
constexpr int kScTable = 32 + kScEntries * 16;  // doubles in device memory: the gate, then the entries (L, R)

struct ScArgs {
    const double* targets;  // [M][32]
    const double* table;    // [kScTable]
    int64_t M;
    int32_t force;          // -1: select
    double beta_p;          // beta' = pi beta / 2
    double fidelity;
    double* x_out;          // [M][24]
    int32_t* cycles;        // [M]
    double* loss;           // [M]
    double* gap;            // [M]
    double* predicted;      // [M]
};

// t_k of the chamber point c (c3 >= 0, c1 in [0, 1]) for the gate class (1/2, beta, 0), bp = pi beta / 2
__device__ __forceinline__ void sc_traces(const double (&c)[3], double bp, double (&t)[4]) {
    const double hp = 1.57079632679489661923, qp = 0.78539816339744830962;
    const bool up = c[0] > 0.5;
    const double a = hp * (up ? 1.0 - c[0] : c[0]), b = hp * c[1], z = hp * (up ? -c[2] : c[2]);
    double sa, ca, sb, cb, sz, cz, sq, cq, sr, cr;
    sincos(a, &sa, &ca);
    sincos(b, &sb, &cb);
    sincos(z, &sz, &cz);
    sincos(qp - a, &sq, &cq);
    sincos(bp - b, &sr, &cr);
    const double r0 = ca * cb * cz, i0 = sa * sb * sz, r1 = cq * cr * cz, i1 = sq * sr * sz;
    t[0] = fmin(sqrt(r0 * r0 + i0 * i0), 1.0);
    t[1] = fmin(sqrt(r1 * r1 + i1 * i1), 1.0);
    t[2] = fabs(cz);
    t[3] = 1.0;
}

// the three U3 angles of L rz(t) R, L and R at e and e + 8
__device__ inline void sc_interior(const double* __restrict__ e, double t, double* __restrict__ p) {
    cplx L[2][2], R[2][2], m[2][2];
    load2(e, L);
    load2(e + 8, R);
    double s, c;
    sincos(0.5 * t, &s, &c);
    const cplx lo = {c, -s}, hi = {c, s};
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        L[r][0] = cmul(L[r][0], lo);
        L[r][1] = cmul(L[r][1], hi);
    }
    mul2(L, R, m);
    put_u3(m, p);
}

__global__ __launch_bounds__(kKakBlock) void sc_decompose_kernel(ScArgs a) {
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
    int k = 0;
    double tk = 1.0;
#pragma unroll 1
    for (int step = 0; step < 2; ++step) {
        kak_decompose(u, cur);
        if (step == 1) {
            kv = cur;
        } else {
            kt = cur;
            double t[4], e;
            sc_traces(kt.c, a.beta_p, t);
            k = a.force >= 0 ? a.force : approx_select(t, 0, a.fidelity, e);
            tk = k == 0 ? t[0] : (k == 1 ? t[1] : (k == 2 ? t[2] : t[3]));
#pragma unroll
            for (int j = 0; j < 24; ++j) xo[j] = 0.0;
            const double pi = 3.14159265358979323846;
            const double* __restrict__ ent = a.table + 32;
            if (k == 2) {
                sc_interior(ent, pi * kt.c[1], xo + 6);
                sc_interior(ent + 16, -pi * kt.c[0], xo + 9);
            } else if (k == 3) {
                sc_interior(ent + 32, pi * kt.c[1], xo + 6);
                sc_interior(ent + 48, -pi * kt.c[0], xo + 9);
                sc_interior(ent + 64, -pi * kt.c[2], xo + 12);
                sc_interior(ent + 80, 0.0, xo + 15);
            }
            // W = the interior circuit, exterior layers still 1 (k = 0: the identity)
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
    // the representative of W's class that the trace formula prefers
    const double g0 = approx_overlap(kv.c[0] - kt.c[0], kv.c[1] - kt.c[1], kv.c[2] - kt.c[2]);
    const double g1 = approx_overlap(1.0 - kv.c[0] - kt.c[0], kv.c[1] - kt.c[1], -kv.c[2] - kt.c[2]);
    if (g1 > g0) kak_mirror(kv);
    a.gap[i] = fmax(fmax(fabs(kv.c[0] - kt.c[0]), fabs(kv.c[1] - kt.c[1])), fabs(kv.c[2] - kt.c[2]));
    a.cycles[i] = k;
    a.predicted[i] = 1.0 - tk;
    if (k == 0) {
        // one layer: (A_T A_W^+) (B_W^+ B_T) per qubit, qubit 0 first
        cplx dg[2][2], l[2][2], r[2][2], m[2][2];
        dagger2(kv.a2, dg);
        mul2(kt.a2, dg, l);
        dagger2(kv.b2, dg);
        mul2(dg, kt.b2, r);
        mul2(l, r, m);
        put_u3(m, xo);
        dagger2(kv.a1, dg);
        mul2(kt.a1, dg, l);
        dagger2(kv.b1, dg);
        mul2(dg, kt.b1, r);
        mul2(l, r, m);
        put_u3(m, xo + 3);
    } else {
        exterior_layers(kv, kt, xo, xo + 6 * k);
    }
    a.loss[i] = template_loss(fw, T, xo, wr, wi);
}

struct ScCountsArgs {
    const double* targets;       // [M][32]
    const double* fidelities;    // [n_fid], device memory
    int64_t M;
    double beta_p;
    int32_t n_fid;
    unsigned long long* counts;  // [n_fid][4]
    unsigned long long* fidsum;  // [n_fid], units of 2^-32
};

__global__ __launch_bounds__(kApproxCountsBlock) void sc_counts_kernel(ScCountsArgs a) {
    __shared__ unsigned int hist[kApproxMaxFid * 4];
    __shared__ unsigned long long sums[kApproxMaxFid];
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = i < a.M;
    for (int b = threadIdx.x; b < a.n_fid * 4; b += blockDim.x) hist[b] = 0u;
    for (int b = threadIdx.x; b < a.n_fid; b += blockDim.x) sums[b] = 0ull;
    __syncthreads();
    double t[4] = {1.0, 1.0, 1.0, 1.0};
    if (live) {
        double c[3];
        weyl_c1c2c3(a.targets + i * 32, -1, c);
        sc_traces(c, a.beta_p, t);
    }
    const const_as_ptr<double> kfid = (const_as_ptr<double>)a.fidelities;
    const bool first_lane = (threadIdx.x & 63) == 0;
    for (int32_t j = 0; j < a.n_fid; ++j) {
        const double f = kfid[j];
        double e;
        const int k = approx_select(t, 0, f, e);
        unsigned long long s = live ? (unsigned long long)llrint(e * 4294967296.0) : 0ull;
#pragma unroll
        for (int w = 32; w >= 1; w >>= 1) s += __shfl_xor(s, w, 64);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const unsigned int n = (unsigned int)__popcll(__ballot(live && k == q));
            if (first_lane && n) atomicAdd(&hist[4 * j + q], n);
        }
        if (first_lane) atomicAdd(&sums[j], s);
    }
    __syncthreads();
    for (int b = threadIdx.x; b < a.n_fid * 4; b += blockDim.x) {
        const unsigned int v = hist[b];
        if (v) atomicAdd(&a.counts[b], (unsigned long long)v);
    }
    for (int b = threadIdx.x; b < a.n_fid; b += blockDim.x) {
        const unsigned long long v = sums[b];
        if (v) atomicAdd(&a.fidsum[b], v);
    }
}

}  // namespace slamdev
