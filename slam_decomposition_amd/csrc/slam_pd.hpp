// slam_pd.hpp -- parallel-drive ("smush") coverage on the device (gfx950 only).
//
// The reference answers "how much of the Weyl chamber do k parallel-drive gates reach" by forward-evaluating random templates one at a
// time (src/slam/utils/gates/parallel_drive_volume.py:176-256: CircuitTemplateV2(no_exterior_1q=1, vz_only=0,
// param_vec_expand=[2, N, N]) over ConversionGainSmushGate(pc, pg, gc, gg, gx[0:N], gy[0:N], t), every parameter uniform in
// (-4 pi, 4 pi)), folding their Weyl coordinates into x <= 1/2 and taking a convex hull.  Here (the kernels themselves are in
// slam_geometry_kernels.hpp, this header holds the __device__ functions under them):
//   pd_sample_kernel     one thread per sample: parameters from Philox keyed (seed, sample index, k), the k-gate product with a U3 x U3
//                        layer between consecutive gates, Weyl coordinates (weyl_c1c2c3), folded;
//   pd_extremes_kernel   the sample that is extreme in each of D fixed directions (integer keys, atomicMax: order-independent);
//   pd_filter_kernel     drops every sample strictly inside the hull of those extremes and compacts the rest -- a point inside a
//                        sub-hull is inside the full hull and is no vertex of it, so the final hull is unchanged;
//   region_lookup_kernel resident Haar targets against a list of regions (unions of convex polytopes): per-region counts and a
//                        first-containing-region histogram.
// Every slice of a smush gate is exp(-i tau H) of the general 4x4 Hermitian H of gates.smush_hamiltonian (free phases: the X (x) X
// block form of slam_smush.hpp does not apply): scaling and squaring with a degree-12 Taylor polynomial in fp64.  Only the forward
// product is needed, so no derivative is formed.
#pragma once
#include "slam_weyl.hpp"

namespace slamdev {

constexpr int kPdMaxSpan = 8;      // SLAM_PD_MAX_SPAN
constexpr int kPdMaxSlices = 16;   // SLAM_PD_MAX_SLICES

struct PdSpec {
    double gc, gg, tau, bound;
    int32_t n_slices, k, n_params;
    uint64_t seed;
};

// parameter i of sample idx, uniform in (-bound, bound): words (0,1) / (2,3) of the Philox block of pair i >> 1, as x0_philox
__device__ __forceinline__ double pd_param(uint64_t seed, uint64_t idx, uint32_t k, uint32_t i, double bound) {
    uint32_t w[4];
    philox4x32_10(i >> 1, (uint32_t)idx, (uint32_t)(idx >> 32), k | 0x50440000u /* "PD" */, (uint32_t)seed, (uint32_t)(seed >> 32), w);
    const uint32_t a = (i & 1) ? w[2] : w[0], b = (i & 1) ? w[3] : w[1];
    const uint64_t m = ((uint64_t)(a >> 5) << 26) + (uint64_t)(b >> 6);
    return bound * (((double)m + 0.5) * (2.0 / 9007199254740992.0) - 1.0);  // (m + 1/2) / 2^53 in (0, 1)
}

// y = H v for H = gx (A + A^+) + gy (B + B^+) + gc (e^{i pc} A B^+ + h.c.) + gg (e^{i pg} A B + h.c.) (gates.smush_hamiltonian):
// A + A^+ flips the high bit of the basis index, B + B^+ the low bit, A B^+ maps |01> to |10>, A B maps |00> to |11>
struct PdHam {
    double gx, gy, gcr, gci, ggr, ggi;  // gc e^{i pc}, gg e^{i pg}
};
__device__ __forceinline__ void pd_hv(const PdHam& h, const double (&vr)[4], const double (&vi)[4], double (&yr)[4], double (&yi)[4]) {
    yr[0] = h.gy * vr[1] + h.gx * vr[2] + (h.ggr * vr[3] + h.ggi * vi[3]);
    yi[0] = h.gy * vi[1] + h.gx * vi[2] + (h.ggr * vi[3] - h.ggi * vr[3]);
    yr[1] = h.gy * vr[0] + h.gx * vr[3] + (h.gcr * vr[2] + h.gci * vi[2]);
    yi[1] = h.gy * vi[0] + h.gx * vi[3] + (h.gcr * vi[2] - h.gci * vr[2]);
    yr[2] = h.gx * vr[0] + h.gy * vr[3] + (h.gcr * vr[1] - h.gci * vi[1]);
    yi[2] = h.gx * vi[0] + h.gy * vi[3] + (h.gcr * vi[1] + h.gci * vr[1]);
    yr[3] = h.gx * vr[1] + h.gy * vr[2] + (h.ggr * vr[0] - h.ggi * vi[0]);
    yi[3] = h.gx * vi[1] + h.gy * vi[2] + (h.ggr * vi[0] + h.ggi * vr[0]);
}

// E = exp(-i tau H): X = -i tau H / 2^q with ||tau H||_1 / 2^q <= 1/4, E = T_12(X)^(2^q) (Horner, column by column: column c of
// I + X P / n depends on column c of P only).  The truncation error is below 1e-17 per factor.
__device__ __forceinline__ void pd_slice_expm(const PdHam& hm, double tau, double (&er)[4][4], double (&ei)[4][4]) {
    const double nrm = tau * (fabs(hm.gx) + fabs(hm.gy) + fmax(sqrt(hm.gcr * hm.gcr + hm.gci * hm.gci), sqrt(hm.ggr * hm.ggr + hm.ggi * hm.ggi)));
    int q = 0;
    if (nrm > 0.25) {
        (void)frexp(nrm * 4.0, &q);  // nrm * 4 = m 2^q, m in [1/2, 1): 2^q >= 4 nrm
        q = q < 60 ? q : 60;
    }
    const double h = ldexp(tau, -q);
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        double vr[4] = {0.0, 0.0, 0.0, 0.0}, vi[4] = {0.0, 0.0, 0.0, 0.0};
        vr[c] = 1.0;
        for (int n = 12; n >= 1; --n) {
            double yr[4], yi[4];
            pd_hv(hm, vr, vi, yr, yi);
            const double f = h / (double)n;  // v <- e_c + (-i h / n) H v
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                vr[r] = (r == c ? 1.0 : 0.0) + f * yi[r];
                vi[r] = -f * yr[r];
            }
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            er[r][c] = vr[r];
            ei[r][c] = vi[r];
        }
    }
    for (int s = 0; s < q; ++s) {
        double tr[4][4], ti[4][4];
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                double ar = 0.0, ai = 0.0;
#pragma unroll
                for (int m = 0; m < 4; ++m) {
                    ar += er[r][m] * er[m][c] - ei[r][m] * ei[m][c];
                    ai += er[r][m] * ei[m][c] + ei[r][m] * er[m][c];
                }
                tr[r][c] = ar;
                ti[r][c] = ai;
            }
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                er[r][c] = tr[r][c];
                ei[r][c] = ti[r][c];
            }
    }
}

// W <- E W (column by column)
__device__ __forceinline__ void pd_left_mul(const double (&er)[4][4], const double (&ei)[4][4], double (&wr)[4][4], double (&wi)[4][4]) {
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        double yr[4], yi[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            double ar = 0.0, ai = 0.0;
#pragma unroll
            for (int m = 0; m < 4; ++m) {
                ar += er[r][m] * wr[m][c] - ei[r][m] * wi[m][c];
                ai += er[r][m] * wi[m][c] + ei[r][m] * wr[m][c];
            }
            yr[r] = ar;
            yi[r] = ai;
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            wr[r][c] = yr[r];
            wi[r][c] = yi[r];
        }
    }
}

// rows (r0, r1) of W <- U3(theta, phi, lam) applied to them; U3 = [[c, -e^{i lam} s], [e^{i phi} s, e^{i (phi + lam)} c]]
__device__ __forceinline__ void pd_u3_rows(double theta, double phi, double lam, int r0, int r1, double (&wr)[4][4], double (&wi)[4][4]) {
    double s, c, sp, cp, sl, cl;
    sincos(0.5 * theta, &s, &c);
    sincos(phi, &sp, &cp);
    sincos(lam, &sl, &cl);
    const double u01r = -cl * s, u01i = -sl * s;
    const double u10r = cp * s, u10i = sp * s;
    const double u11r = (cp * cl - sp * sl) * c, u11i = (sp * cl + cp * sl) * c;
#pragma unroll
    for (int col = 0; col < 4; ++col) {
        const double ar = wr[r0][col], ai = wi[r0][col], br = wr[r1][col], bi = wi[r1][col];
        wr[r0][col] = c * ar + (u01r * br - u01i * bi);
        wi[r0][col] = c * ai + (u01r * bi + u01i * br);
        wr[r1][col] = (u10r * ar - u10i * ai) + (u11r * br - u11i * bi);
        wi[r1][col] = (u10r * ai + u10i * ar) + (u11r * bi + u11i * br);
    }
}

// (value, index) -> an unsigned key whose order is the value's (rounded to float) and, among equal values, the lower index first
__device__ __forceinline__ unsigned long long pd_key(double v, int64_t i) {
    uint32_t u = __float_as_uint((float)v);
    u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    return ((unsigned long long)u << 32) | (unsigned long long)(0xFFFFFFFFu - (uint32_t)i);
}

__device__ __forceinline__ unsigned long long wave_max_u64(unsigned long long v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, off), hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), off);
        const unsigned long long o = ((unsigned long long)hi << 32) | lo;
        v = o > v ? o : v;
    }
    return v;
}

}  // namespace slamdev
