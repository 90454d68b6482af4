// slam_approx.hpp -- fidelity-aware approximate closed-form decomposition on the device (gfx950 only): the best circuit of 0, 1, 2 or 3
// gates of the CNOT, the iSWAP or the B class for each target, and the size whose EXPECTED fidelity is highest when one basis gate has
// the fidelity f.  The second half of the reference's TwoQubitBasisDecomposer branch
// (src/slam/utils/transpiler_pass/weyl_decompose.py:475-480, qiskit's TwoQubitBasisDecomposer(basis_fidelity)); slam_cx.hpp and slam_b.hpp
// are the first half, the exact circuits of the fewest gates.
//
// Coordinates c in units of pi, folded as span_rules._fold does: (x, y, z) = (c1, c2, c3), or (1 - c1, c2, -c3) where c1 > 1/2;
// a = pi x / 2, b = pi y / 2, c = pi z / 2.  The basis gate G has the class (1/2, beta, 0): beta = 0 (family 0, the CNOT class), 1/2
// (family 1, the iSWAP class), 1/4 (family 2, the B class); beta' = pi beta / 2.  The best circuit of k gates reaches
// |Tr(T^+ W)| = 4 t_k:
//     t_0 = |cos a cos b cos c + i sin a sin b sin c|
//     t_1 = |cos(pi/4 - a) cos(beta' - b) cos c + i sin(pi/4 - a) sin(beta' - b) sin c|
//     t_2 = |cos c|  (families 0, 1: two gates reach exactly the plane c3 = 0, the nearest point is (c1, c2, 0));  1  (family 2)
//     t_3 = 1        (families 0, 1; family 2 has no k = 3)
// L_k = 1 - t_k is the BasicCost loss, F_k = (4 + 16 t_k^2) / 20 the average gate fidelity (1 - SquareCost), E_k = F_k f^k the expected
// fidelity.  The k with the largest E_k is taken, compared in the order k = 0, 1, 2, 3 with strict >: ties go to fewer gates.  The t_k
// come from the kernel's own unrounded coordinates; cos of anything below 1e-8 is exactly 1, so a target of a class that k gates reach
// has t_k = 1 exactly and the ties of f = 1 are exact ties.
//
// Circuits.  The interior layers are those of the siblings at the nearest reachable point: none for k = 0 and k = 1 (W = 1, W = G), V2 of
// slam_cx.hpp at (c1, c2, 0) for two gates of families 0 and 1, the exact B formula of slam_b.hpp, the exact V3.  The exterior layers
// come from aligning W with the target (KAK forms of both).  With T = A_T CAN(c_T) B_T and W = A_W CAN(c_W) B_W the row
// (A_T A_W^+) W (B_W^+ B_T) = A_T CAN(c_W) B_T has Tr(T^+ row) = Tr CAN(c_W - c_T), which depends on the REPRESENTATIVE c_W of W's class:
// the chamber point or its mirror image (1 - c1, c2, -c3), the same class everywhere (kak_mirror).  kak_align takes the one closer in
// max norm; here the trace formula is evaluated for both and the larger one is taken, which attains t_k in every case above (k = 0 with
// c1 > 1/2 aligns the identity's image (1, 0, 0)).  A row of no gate holds ONE layer, (A_T A_W^+)(B_W^+ B_T) per qubit.
//
// approx_decompose_kernel: one thread per target, fp64, the structure of cx_decompose_kernel: kak_decompose is inlined once, the KAK
// forms of T and W come from a loop of two steps (the step is wave-uniform), the rows pass through x_out, the table (the gate and the
// family's interior factors, as cx_fold_dress / b_fold_dress fold them) is read at wave-uniform addresses.
//
// approx_counts_kernel: the sweep.  One thread per target; the coordinates (weyl_c1c2c3, unrounded) and the t_k once, then the selection
// for each of n_fid <= 64 fidelities in a wave-uniform loop (the fidelities through the constant address space: scalar loads).  Per
// fidelity a wave counts its lanes per size by ballot and sums llrint(E 2^32) over its lanes; lane 0 adds both to the block's histogram
// in LDS ([n_fid][4] counts, [n_fid] sums), and every non-empty bin is folded into global memory with one 64-bit atomic.  Integer sums:
// counts and fidelity sums do not depend on the order of addition.
#pragma once
#include "slam_cx.hpp"
#include "slam_b.hpp"

namespace slamdev {

constexpr int kApproxMaxFid = 64;
constexpr int kApproxCountsBlock = 256;

struct ApproxArgs {
    const double* targets;  // [M][32]
    const double* table;    // [kCxTable] (families 0, 1) or [kBTable] (family 2)
    int64_t M;
    int32_t family;
    int32_t force;          // -1: select
    double fidelity;
    double* x_out;          // [M][24]
    int32_t* cycles;        // [M]
    double* loss;           // [M]
    double* gap;            // [M]
    double* predicted;      // [M]
};

// t_k of the chamber point c (c3 >= 0, c1 in [0, 1]); t[3] = 1 for family 2 too, where it is never selected
__device__ __forceinline__ void approx_traces(const double (&c)[3], int family, double (&t)[4]) {
    const double hp = 1.57079632679489661923, qp = 0.78539816339744830962;
    const bool up = c[0] > 0.5;
    const double a = hp * (up ? 1.0 - c[0] : c[0]), b = hp * c[1], z = hp * (up ? -c[2] : c[2]);
    const double bp = family == 0 ? 0.0 : (family == 1 ? qp : 0.5 * qp);
    double sa, ca, sb, cb, sz, cz, sq, cq, sr, cr;
    sincos(a, &sa, &ca);
    sincos(b, &sb, &cb);
    sincos(z, &sz, &cz);
    sincos(qp - a, &sq, &cq);
    sincos(bp - b, &sr, &cr);
    const double r0 = ca * cb * cz, i0 = sa * sb * sz, r1 = cq * cr * cz, i1 = sq * sr * sz;
    t[0] = fmin(sqrt(r0 * r0 + i0 * i0), 1.0);
    t[1] = fmin(sqrt(r1 * r1 + i1 * i1), 1.0);
    t[2] = family == 2 ? 1.0 : fabs(cz);
    t[3] = 1.0;
}

// the k with the largest E_k = (4 + 16 t_k^2) / 20 f^k, the first of equals; E of that k
__device__ __forceinline__ int approx_select(const double (&t)[4], int family, double f, double& e_best) {
    const int nk = family == 2 ? 3 : 4;
    int k = 0;
    double p = 1.0, best = -1.0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const double e = (0.2 + 0.8 * t[j] * t[j]) * p;
        if (j < nk && e > best) {
            best = e;
            k = j;
        }
        p *= f;
    }
    e_best = best;
    return k;
}

// |Tr CAN(d)|^2 / 16
__device__ __forceinline__ double approx_overlap(double d1, double d2, double d3) {
    const double hp = 1.57079632679489661923;
    double s1, c1, s2, c2, s3, c3;
    sincos(hp * d1, &s1, &c1);
    sincos(hp * d2, &s2, &c2);
    sincos(hp * d3, &s3, &c3);
    const double re = c1 * c2 * c3, im = s1 * s2 * s3;
    return re * re + im * im;
}

__global__ __launch_bounds__(kKakBlock) void approx_decompose_kernel(ApproxArgs a) {
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
            approx_traces(kt.c, a.family, t);
            k = a.force >= 0 ? a.force : approx_select(t, a.family, a.fidelity, e);
            tk = k == 0 ? t[0] : (k == 1 ? t[1] : (k == 2 ? t[2] : t[3]));
#pragma unroll
            for (int j = 0; j < 24; ++j) xo[j] = 0.0;
            const double pi = 3.14159265358979323846;
            const double* __restrict__ ent = a.table + 32;
            if (a.family == 2) {
                if (k == 2) {
                    // the exact B formula at the folded point, as b_decompose_kernel writes it (slam_b.hpp)
                    const bool up = kt.c[0] > 0.5;
                    const double rt2 = 1.41421356237309504880;
                    const double d = up ? kt.c[0] - 0.5 : 0.5 - kt.c[0];
                    const double c1 = up ? 1.0 - kt.c[0] : kt.c[0], c2 = kt.c[1], c3 = up ? -kt.c[2] : kt.c[2];
                    double s1, h1, s2, h2, s3, h3;
                    sincos(0.5 * pi * c1, &s1, &h1);
                    sincos(0.5 * pi * c2, &s2, &h2);
                    sincos(0.5 * pi * c3, &s3, &h3);
                    const double sy = fmin(rt2 * s1 * h2, 1.0);
                    const double qr = rt2 * s2 * h1, qi = sqrt(fmax(sin(pi * d) * cos(pi * c2), 0.0));
                    cplx q[2][2];
                    q[0][0] = {qr, qi};
                    q[0][1] = {sy, 0.0};
                    q[1][0] = {-sy, 0.0};
                    q[1][1] = {qr, -qi};
                    b_interior(ent, q, xo + 6);
                    q[0][0] = {h3, 0.0};
                    q[0][1] = {s3, 0.0};
                    q[1][0] = {-s3, 0.0};
                    q[1][1] = {h3, 0.0};
                    b_interior(ent + 16, q, xo + 9);
                }
            } else {
                // V2 at (c1, c2, 0), V3 at c: linear in any representative of the target's class (slam_cx.hpp)
                const double off = (k == 3 && a.family == 0) ? 0.5 : 0.0;
                const double ang[3] = {pi * (kt.c[0] - off), pi * (kt.c[1] - off), pi * (kt.c[2] - off)};
                if (k == 2) {
                    cx_interior(ent, ang, xo + 6);
                    cx_interior(ent + 18, ang, xo + 9);
                } else if (k == 3) {
                    cx_interior(ent + 36, ang, xo + 6);
                    cx_interior(ent + 54, ang, xo + 9);
                    cx_interior(ent + 72, ang, xo + 12);
                    cx_interior(ent + 90, ang, xo + 15);
                }
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

struct ApproxCountsArgs {
    const double* targets;       // [M][32]
    const double* fidelities;    // [n_fid], device memory
    int64_t M;
    int32_t family;
    int32_t n_fid;
    unsigned long long* counts;  // [n_fid][4]
    unsigned long long* fidsum;  // [n_fid], units of 2^-32
};

__global__ __launch_bounds__(kApproxCountsBlock) void approx_counts_kernel(ApproxCountsArgs a) {
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
        approx_traces(c, a.family, t);
    }
    const const_as_ptr<double> kfid = (const_as_ptr<double>)a.fidelities;
    const bool first_lane = (threadIdx.x & 63) == 0;
    for (int32_t j = 0; j < a.n_fid; ++j) {
        const double f = kfid[j];
        double e;
        const int k = approx_select(t, a.family, f, e);
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
