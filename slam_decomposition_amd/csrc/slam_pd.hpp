// slam_pd.hpp -- parallel-drive ("smush") coverage on the device (gfx950 only).
//
// The reference answers "how much of the Weyl chamber do k parallel-drive gates reach" by forward-evaluating random templates one at a
// time (src/slam/utils/gates/parallel_drive_volume.py:176-256: CircuitTemplateV2(no_exterior_1q=1, vz_only=0,
// param_vec_expand=[2, N, N]) over ConversionGainSmushGate(pc, pg, gc, gg, gx[0:N], gy[0:N], t), every parameter uniform in
// (-4 pi, 4 pi)), folding their Weyl coordinates into x <= 1/2 and taking a convex hull.  Here:
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
constexpr int kPdBlock = 128;
constexpr int kPdScanBlock = 256;
constexpr int kRegionBlock = 256;
constexpr int kRegionMax = 256;    // SLAM_REGION_MAX

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

// One thread per sample.  Sample vector (CircuitTemplateV2 index order, no_exterior_1q): P = 6 (k - 1) U3 angles (layer j = 1 .. k - 1:
// qubit 0's theta, phi, lambda, then qubit 1's; layer j is K = U3(q1) (x) U3(q0), between gates j and j + 1), then per gate
// (pc, pg, gx[0..N), gy[0..N)).  W = G_k K_{k-1} ... K_1 G_1, G = S_{N-1} ... S_0.
__global__ __launch_bounds__(kPdBlock) void pd_sample_kernel(PdSpec sp, int64_t first_index, int64_t n, const int64_t* __restrict__ indices,
                                                             int ndigits, double* __restrict__ coords, double* __restrict__ params,
                                                             double* __restrict__ unitaries) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    const uint64_t idx = indices ? (uint64_t)indices[t] : (uint64_t)(first_index + t);
    const uint32_t k = (uint32_t)sp.k;
    const int N = sp.n_slices;
    double wr[4][4], wi[4][4];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            wr[r][c] = r == c ? 1.0 : 0.0;
            wi[r][c] = 0.0;
        }
    double* __restrict__ prow = params ? params + t * (int64_t)sp.n_params : nullptr;
    const uint32_t gate0 = 6u * (k - 1u);
    for (uint32_t j = 0; j < k; ++j) {
        if (j > 0) {
            double x[6];
#pragma unroll
            for (int m = 0; m < 6; ++m) {
                x[m] = pd_param(sp.seed, idx, k, 6u * (j - 1u) + m, sp.bound);
                if (prow) prow[6u * (j - 1u) + m] = x[m];
            }
            pd_u3_rows(x[0], x[1], x[2], 0, 1, wr, wi);  // qubit 0: the low bit of the basis index
            pd_u3_rows(x[0], x[1], x[2], 2, 3, wr, wi);
            pd_u3_rows(x[3], x[4], x[5], 0, 2, wr, wi);  // qubit 1: the high bit
            pd_u3_rows(x[3], x[4], x[5], 1, 3, wr, wi);
        }
        const uint32_t base = gate0 + j * (2u + 2u * (uint32_t)N);
        const double pc = pd_param(sp.seed, idx, k, base, sp.bound), pg = pd_param(sp.seed, idx, k, base + 1u, sp.bound);
        if (prow) {
            prow[base] = pc;
            prow[base + 1u] = pg;
        }
        double spc, cpc, spg, cpg;
        sincos(pc, &spc, &cpc);
        sincos(pg, &spg, &cpg);
        PdHam hm;
        hm.gcr = sp.gc * cpc;
        hm.gci = sp.gc * spc;
        hm.ggr = sp.gg * cpg;
        hm.ggi = sp.gg * spg;
        for (int s = 0; s < N; ++s) {
            hm.gx = pd_param(sp.seed, idx, k, base + 2u + (uint32_t)s, sp.bound);
            hm.gy = pd_param(sp.seed, idx, k, base + 2u + (uint32_t)(N + s), sp.bound);
            if (prow) {
                prow[base + 2u + (uint32_t)s] = hm.gx;
                prow[base + 2u + (uint32_t)(N + s)] = hm.gy;
            }
            double er[4][4], ei[4][4];
            pd_slice_expm(hm, sp.tau, er, ei);
            pd_left_mul(er, ei, wr, wi);
        }
    }
    double u[32];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            u[(r * 4 + c) * 2] = wr[r][c];
            u[(r * 4 + c) * 2 + 1] = wi[r][c];
        }
    if (unitaries) {
#pragma unroll
        for (int e = 0; e < 32; ++e) unitaries[t * 32 + e] = u[e];
    }
    double cw[3];
    weyl_c1c2c3(u, ndigits, cw);
    if (cw[0] > 0.5) cw[0] = 1.0 - cw[0];  // parallel_drive_volume.py:297-305: the "left" point of every sample
    coords[t * 3 + 0] = cw[0];
    coords[t * 3 + 1] = cw[1];
    coords[t * 3 + 2] = cw[2];
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

// best[d] = max over samples of pd_key(dir_d . p, index); 0 = no sample
__global__ __launch_bounds__(kPdScanBlock) void pd_extremes_kernel(const double* __restrict__ coords, int64_t n, const double* __restrict__ dirs,
                                                                   int32_t n_dirs, unsigned long long* __restrict__ best) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = i < n;
    const double p0 = live ? coords[i * 3] : 0.0, p1 = live ? coords[i * 3 + 1] : 0.0, p2 = live ? coords[i * 3 + 2] : 0.0;
    const const_as_ptr<double> kd = (const_as_ptr<double>)dirs;
    for (int32_t d = 0; d < n_dirs; ++d) {
        const double v = kd[3 * d] * p0 + kd[3 * d + 1] * p1 + kd[3 * d + 2] * p2;
        const unsigned long long key = wave_max_u64(live ? pd_key(v, i) : 0ull);
        if (__lane_id() == 0 && key) atomicMax(&best[d], key);
    }
}

__global__ void pd_gather_kernel(const double* __restrict__ coords, const unsigned long long* __restrict__ best, int32_t n_dirs,
                                 int64_t* __restrict__ idx_out, double* __restrict__ c_out) {
    const int d = blockIdx.x * blockDim.x + threadIdx.x;
    if (d >= n_dirs) return;
    const unsigned long long key = best[d];
    const int64_t i = key ? (int64_t)(0xFFFFFFFFu - (uint32_t)key) : -1;
    idx_out[d] = i;
#pragma unroll
    for (int j = 0; j < 3; ++j) c_out[d * 3 + j] = i >= 0 ? coords[i * 3 + j] : 0.0;
}

// keep every sample that is not strictly inside (by more than eps) all facets n . p <= b; survivors are appended in wave-sized
// groups (one counter update per wavefront), so their order depends on scheduling -- the host sorts them by index
__global__ __launch_bounds__(kPdScanBlock) void pd_filter_kernel(const double* __restrict__ coords, int64_t n, const double* __restrict__ facets,
                                                                 int32_t n_facets, double eps, unsigned int* __restrict__ n_out,
                                                                 int64_t* __restrict__ idx_out, double* __restrict__ c_out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = i < n;
    const double p0 = live ? coords[i * 3] : 0.0, p1 = live ? coords[i * 3 + 1] : 0.0, p2 = live ? coords[i * 3 + 2] : 0.0;
    const const_as_ptr<double> kf = (const_as_ptr<double>)facets;
    bool inside = live;
    for (int32_t f = 0; f < n_facets; ++f) {
        if (!__any(inside)) break;  // wave-uniform exit: every lane already has a facet it is not strictly inside
        const double v = kf[4 * f] * p0 + kf[4 * f + 1] * p1 + kf[4 * f + 2] * p2 - kf[4 * f + 3];
        inside = inside && (v < -eps);
    }
    const bool keep = live && !inside;
    const unsigned long long m = __ballot(keep);
    const int lane = (int)__lane_id();
    unsigned int base = 0u;
    if (lane == 0 && m) base = atomicAdd(n_out, (unsigned int)__popcll(m));
    base = (unsigned int)__shfl((int)base, 0);
    if (keep) {
        const unsigned int pos = base + (unsigned int)__popcll(m & ((1ull << lane) - 1ull));
        idx_out[pos] = i;
        c_out[(int64_t)pos * 3] = p0;
        c_out[(int64_t)pos * 3 + 1] = p1;
        c_out[(int64_t)pos * 3 + 2] = p2;
    }
}

// ---------------------------------------------------------------------------------
// Region lookup: regions r = 0 .. R - 1, each a union of polytopes [region_offsets[r], region_offsets[r + 1]); polytope p is
//   kind 0  facets [facet_offsets[p], facet_offsets[p + 1]) of double4 (n, b): inside iff n . c <= b + tol for every facet, c = the
//           target's Weyl coordinates (8 digits, c3 >= 0)
//   kind 1  a coverage region of two or more gates: aux[p][0..14) = the bounds of coverage.region (as slam_coverage_lookup kind 1)
//   kind 2  one gate's class: aux[p][0..4) = its alcove point (as slam_coverage_lookup kind 0)
// counts[r] += targets inside region r; counts[R + r] += targets whose first containing region is r, counts[2R] those in none.  One
// thread per target; region, polytope and facet indices are wave-uniform (scalar loads), and a facet walk ends as soon as no lane of
// the wavefront can still be inside.  Integer counts through an LDS histogram, then one 64-bit atomic per non-empty bin and block.
// ---------------------------------------------------------------------------------
__global__ __launch_bounds__(kRegionBlock) void region_lookup_kernel(const double* __restrict__ U, int64_t M, int32_t n_regions,
                                                                     const int32_t* __restrict__ region_offsets, const int32_t* __restrict__ kinds,
                                                                     const int32_t* __restrict__ facet_offsets, const double* __restrict__ facets,
                                                                     const double* __restrict__ aux, double tol, unsigned long long* __restrict__ counts) {
    __shared__ unsigned int hist[2 * kRegionMax + 1];
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = i < M;
    double c[3] = {0.0, 0.0, 0.0}, pt[2][4], sm[2][kSpanPatterns];
    if (live) weyl_c1c2c3(U + i * 32, 8, c);
#pragma unroll
    for (int sh = 0; sh < 2; ++sh) {
        double a[4];
        alcove_point(c[0], c[1], c[2], sh ? 0.5 : 0.0, a);
        const double g1 = a[3], g2 = a[2], g3 = a[1], g4 = a[0];  // the order of span_predict_kernel
        const double s[kSpanPatterns] = {g1, g2, g3, g4, g1 + g2, g1 + g3, g1 + g4, g2 + g3, g2 + g4, g3 + g4,
                                         g1 + g2 + g3, g1 + g2 + g4, g1 + g3 + g4, g2 + g3 + g4};
#pragma unroll
        for (int j = 0; j < 4; ++j) pt[sh][j] = a[j];
#pragma unroll
        for (int p = 0; p < kSpanPatterns; ++p) sm[sh][p] = s[p];
    }
    const int nb = 2 * n_regions + 1;
    for (int b = threadIdx.x; b < nb; b += blockDim.x) hist[b] = 0u;
    __syncthreads();
    const double t1 = (tol > 0.0 ? tol : 0.0) + 1e-12;
    const const_as_ptr<int32_t> kro = (const_as_ptr<int32_t>)region_offsets;
    const const_as_ptr<int32_t> kki = (const_as_ptr<int32_t>)kinds;
    const const_as_ptr<int32_t> kfo = (const_as_ptr<int32_t>)facet_offsets;
    const const_as_ptr<double> kf = (const_as_ptr<double>)facets;
    const const_as_ptr<double> ka = (const_as_ptr<double>)aux;
    int first = n_regions;
    for (int32_t r = 0; r < n_regions; ++r) {
        bool in_r = false;
        for (int32_t p = kro[r]; p < kro[r + 1]; ++p) {
            if (!__any(live && !in_r)) break;
            const int32_t kind = kki[p];
            bool ok = live && !in_r;
            if (kind == 0) {
                for (int32_t f = kfo[p]; f < kfo[p + 1]; ++f) {
                    if (!__any(ok)) break;
                    const double v = kf[4 * f] * c[0] + kf[4 * f + 1] * c[1] + kf[4 * f + 2] * c[2] - kf[4 * f + 3];
                    ok = ok && (v <= tol);
                }
            } else if (kind == 1) {
                const const_as_ptr<double> bd = ka + (int64_t)p * kSpanPatterns;
                bool ok0 = true, ok1 = true;
#pragma unroll
                for (int q = 0; q < kSpanPatterns; ++q) {
                    const double lo = bd[q] - tol;
                    ok0 = ok0 && (sm[0][q] >= lo);
                    ok1 = ok1 && (sm[1][q] >= lo);
                }
                ok = ok && (ok0 || ok1);
            } else {
                const const_as_ptr<double> q = ka + (int64_t)p * kSpanPatterns;
                const double q0 = q[0], q1 = q[1], q2 = q[2], q3 = q[3];
                bool hit = false;
#pragma unroll
                for (int sh = 0; sh < 2; ++sh)
                    hit = hit || (fabs(pt[sh][0] - q0) <= t1 && fabs(pt[sh][1] - q1) <= t1 && fabs(pt[sh][2] - q2) <= t1 && fabs(pt[sh][3] - q3) <= t1);
                ok = ok && hit;
            }
            in_r = in_r || ok;
        }
        if (in_r) {
            atomicAdd(&hist[r], 1u);
            if (first == n_regions) first = r;
        }
    }
    if (live) atomicAdd(&hist[n_regions + first], 1u);
    __syncthreads();
    for (int b = threadIdx.x; b < nb; b += blockDim.x) {
        const unsigned int v = hist[b];
        if (v) atomicAdd(&counts[b], (unsigned long long)v);
    }
}

}  // namespace slamdev
