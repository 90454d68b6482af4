// slam_sqapprox.hpp -- fidelity-aware approximate closed-form decomposition into sqrt(iSWAP) gates on the device (gfx950 only): the best
// circuit of 0, 1, 2 or 3 gates S = sqrt(iSWAP) for each target, and the size whose EXPECTED fidelity is highest when one S has the
// fidelity f.  What slam_approx.hpp is for the supercontrolled classes, for the gate of slam_analytic.hpp, which is not supercontrolled:
// the set that two S reach is a solid region of the chamber, not a plane, and the nearest point of it has a closed form of its own.
//
// Coordinates c in units of pi; S has the class (1/4, 1/4, 0).  Folding: (x, y, z) = (c1, c2, c3), or (1 - c1, c2, -c3) where c1 > 1/2;
// w = |z|, s = sign(z).  Overlap: ov(d) = sqrt((cos d1' cos d2' cos d3')^2 + (sin d1' sin d2' sin d3')^2), d' = pi d / 2, which is
// |Tr CAN(d)| / 4 (the square root of approx_overlap).  The best circuit of k gates reaches |Tr(T^+ W)| = 4 t_k:
//     t_0 = ov(x, y, z)
//     t_1 = ov(1/4 - x, 1/4 - y, z)
//     t_3 = 1
//     t_2: two S reach exactly the region w <= x - y (span_rules.minimal_span, slam_analytic.hpp).  h = w - x + y.
//          h <= 0:  t_2 = 1, the nearest point is the target itself.
//          h > 0:   u = h / 3, p = (x + u, y - u, s (w - u)): the foot of the perpendicular on the face w = x - y, which is also the
//                   stationary point of ov on that face (ov is symmetric under permutations and sign flips of its argument).
//                   Where x + u > 1/2 the foot lies beyond the fold c1 = 1/2, where the region has a ridge: r = y + w - 1/2,
//                   p = (1/2, y - r / 2, s (w - r / 2)).
//                   t_2 = ov(p - (x, y, z)) in both cases.
// The "inside" test is the size rule of sqiswap_decompose_kernel: w <= x - y + 2e-8 on coordinates rounded to 8 digits; t_2 is exactly
// 1 there, so the sizes at f = 1 are those of that kernel wherever it returns its minimum.  Everything else is evaluated on the kernel's
// own unrounded coordinates; cos of anything below 1e-8 is exactly 1, so a target that k gates reach has t_k = 1 exactly and the ties
// of f = 1 are exact ties: no gate for a local target, one for a target of S's class, two inside the region, three elsewhere.
//
// Selection: L_k = 1 - t_k (BasicCost), F_k = (4 + 16 t_k^2) / 20, E_k = F_k f^k; the largest E_k in the order k = 0, 1, 2, 3 with
// strict >, so ties go to fewer gates (approx_select).
//
// Circuits.  k = 0, 1: W = 1, W = S, the exterior aligned as approx_decompose_kernel aligns it (both representatives of W's class,
// the one the trace formula prefers; a row of no gate holds ONE layer).  k = 2: the interior S (C1 (x) C2) S of analytic_interior at p,
// aligned the same way.  Where p is the projected point it lies on the face of the region, where analytic_interior's C vanishes
// analytically: the interior is given the face (C = 0, alpha = beta) and does not rediscover it through a clamped rounding residue, of
// which 2 sqrt(C) would make 1e-8 of angle.  Inside the region (t_2 = 1) the interior is the formula of slam_analytic.hpp unchanged.
// k = 3: the construction of sqiswap_decompose_kernel, through the device functions that hold a copy of its statements
// (analytic_best_shift, analytic_align_products, analytic_row3 in slam_analytic.hpp): the 12 placements, the largest margin, shift_locals.  `loss` is template_loss of the
// finished row, `predicted` is 1 - t_k, `gap` the max-norm chamber distance that remains after the alignment (k = 3: kak_align's, of
// V against CAN(c - s)).
//
// sqiswap_approx_decompose_kernel: one thread per target, fp64, the structure of its two parents: kak_decompose is inlined once, the
// KAK forms of T, W (and CAN(c - s)) come from a loop whose step is wave-uniform -- two steps for k <= 2, three for k = 3 -- and the
// rows pass through x_out.
//
// sqiswap_approx_counts_kernel: the sweep, approx_counts_kernel's scheme.  One thread per target; the coordinates (weyl_c1c2c3,
// unrounded) and the four t_k once, then the selection for each of n_fid <= 64 fidelities in a wave-uniform loop (the fidelities
// through the constant address space).  Per fidelity a wave counts its lanes per size by ballot and sums llrint(E 2^32) over its
// lanes; lane 0 adds both to the block's histogram in LDS, and every non-empty bin is folded into global memory with one 64-bit atomic.
// Integer sums: counts and fidelity sums do not depend on the order of addition.
#pragma once
#include "slam_analytic.hpp"
#include "slam_approx.hpp"

namespace slamdev {

struct SqApproxArgs {
    const double* targets;  // [M][32]
    int64_t M;
    int32_t force;          // -1: select
    double fidelity;
    double* x_out;          // [M][24]
    int32_t* cycles;        // [M]
    double* loss;           // [M]
    double* gap;            // [M]
    double* predicted;      // [M]
};

// t_k of the chamber point c (c3 >= 0, c1 in [0, 1]); p: the nearest point that two gates reach, folded (p1 <= 1/2, p3 of either
// sign); face: p is the projected point, on the face of the region (false: p is the folded target itself, t_2 = 1)
__device__ __forceinline__ void sqapprox_traces(const double (&c)[3], double (&t)[4], double (&p)[3], bool& face) {
    const bool up = c[0] > 0.5;
    const double x = up ? 1.0 - c[0] : c[0], y = c[1], z = up ? -c[2] : c[2];
    t[0] = fmin(sqrt(approx_overlap(x, y, z)), 1.0);
    t[1] = fmin(sqrt(approx_overlap(0.25 - x, 0.25 - y, z)), 1.0);
    t[2] = 1.0;
    t[3] = 1.0;
    p[0] = x;
    p[1] = y;
    p[2] = z;
    // inside: the size rule of sqiswap_decompose_kernel, on coordinates rounded to 8 digits as weyl_c1c2c3 rounds them
    double c8[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) c8[j] = rint(c[j] * 1e8) / 1e8;
    if (c8[0] > 0.5) {
        c8[0] = 1.0 - c8[0];
        c8[2] = -c8[2];
    }
    face = !(fabs(c8[2]) <= c8[0] - c8[1] + 2e-8);
    if (face) {
        const double w = fabs(z), h = fmax(w - x + y, 0.0), u = h / 3.0;
        double dx = u, dy = -u, dw = -u;
        if (x + u > 0.5) {  // the ridge at the fold
            const double r = y + w - 0.5;
            dx = 0.5 - x;
            dy = -0.5 * r;
            dw = -0.5 * r;
        }
        const double dz = z < 0.0 ? -dw : dw;
        p[0] = x + dx;
        p[1] = y + dy;
        p[2] = z + dz;
        t[2] = fmin(sqrt(approx_overlap(dx, dy, dz)), 1.0);
    }
}

__global__ __launch_bounds__(kKakBlock) void sqiswap_approx_decompose_kernel(SqApproxArgs a) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.M) return;
    const double* __restrict__ T = a.targets + 32 * i;
    double* __restrict__ xo = a.x_out + 24 * i;
    CompleteArgs fw{};  // template_forward reads k, seq and gates
    fw.gates = kSqiswapGate;
    double u[32], wr[4][4], wi[4][4];
#pragma unroll
    for (int j = 0; j < 32; ++j) u[j] = T[j];
    Kak kt, kv, kr, cur;
    int k = 0, shift = 0;
    double tk = 1.0;
    double raw[3] = {0.0, 0.0, 0.0};
#pragma unroll 1
    for (int step = 0; step < 3; ++step) {
        if (step == 2 && k != 3) break;
        kak_decompose(u, cur);
        if (step == 0) {
            kt = cur;
            double t[4], f[3], e;
            bool face;
            sqapprox_traces(kt.c, t, f, face);
            k = a.force >= 0 ? a.force : approx_select(t, 0, a.fidelity, e);
            tk = k == 0 ? t[0] : (k == 1 ? t[1] : (k == 2 ? t[2] : t[3]));
#pragma unroll
            for (int j = 0; j < 24; ++j) xo[j] = 0.0;
            if (k == 3) {
                // the reduced class of the best placement, inside the region: the interior formula as it is
                analytic_best_shift(kt.c, shift, f, raw);
                face = false;
            }
            if (k >= 2) analytic_interior(f, xo + 6, face);
            // W = the interior circuit, exterior layers still 1: the identity, S, S C S (three gates: V = S C S of the reduced class)
            fw.k = k == 3 ? 2 : k;
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
    a.cycles[i] = k;
    a.predicted[i] = 1.0 - tk;
    if (k == 3) {
        // V aligned to CAN(c - s), then the placement's local gates: the row of sqiswap_decompose_kernel
        a.gap[i] = kak_align(kv, kr);
        cplx L1[2][2], L2[2][2], R1[2][2], R2[2][2];
        analytic_align_products(kv, kr, L1, L2, R1, R2);
        double mid[6];
#pragma unroll
        for (int j = 0; j < 6; ++j) mid[j] = xo[6 + j];
        analytic_row3(shift, kt, L1, L2, R1, R2, mid, xo);
    } else {
        // the representative of W's class that the trace formula prefers
        const double g0 = approx_overlap(kv.c[0] - kt.c[0], kv.c[1] - kt.c[1], kv.c[2] - kt.c[2]);
        const double g1 = approx_overlap(1.0 - kv.c[0] - kt.c[0], kv.c[1] - kt.c[1], -kv.c[2] - kt.c[2]);
        if (g1 > g0) kak_mirror(kv);
        a.gap[i] = fmax(fmax(fabs(kv.c[0] - kt.c[0]), fabs(kv.c[1] - kt.c[1])), fabs(kv.c[2] - kt.c[2]));
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
    }
    fw.k = k;
    a.loss[i] = template_loss(fw, T, xo, wr, wi);
}

struct SqApproxCountsArgs {
    const double* targets;       // [M][32]
    const double* fidelities;    // [n_fid], device memory
    int64_t M;
    int32_t n_fid;
    unsigned long long* counts;  // [n_fid][4]
    unsigned long long* fidsum;  // [n_fid], units of 2^-32
};

__global__ __launch_bounds__(kApproxCountsBlock) void sqiswap_approx_counts_kernel(SqApproxCountsArgs a) {
    __shared__ unsigned int hist[kApproxMaxFid * 4];
    __shared__ unsigned long long sums[kApproxMaxFid];
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = i < a.M;
    for (int b = threadIdx.x; b < a.n_fid * 4; b += blockDim.x) hist[b] = 0u;
    for (int b = threadIdx.x; b < a.n_fid; b += blockDim.x) sums[b] = 0ull;
    __syncthreads();
    double t[4] = {1.0, 1.0, 1.0, 1.0};
    if (live) {
        double c[3], p[3];
        bool face;
        weyl_c1c2c3(a.targets + i * 32, -1, c);
        sqapprox_traces(c, t, p, face);
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
