// slam_geometry_kernels.hpp -- the __global__ kernels of the geometry unit (gfx950 only).  Included by slam_geometry.hip alone, which
// is therefore the one unit that emits them; the __device__ functions they call stay in slam_weyl.hpp, slam_pd.hpp and slam_kak.hpp,
// where other units (slam_analytic.hip) and headers (slam_span_sampler.hpp) include them freely.
#pragma once
#include "slam_kak.hpp"

namespace slamdev {

// ---- slam_weyl.hpp ------------------------------------------------------------------------------------------------------------------
__global__ void c1c2c3_kernel(const double* __restrict__ U, int64_t M, int ndigits, double* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < M) weyl_c1c2c3(U + i * 32, ndigits, out + i * 3);
}

// the span predictor of slam_weyl.hpp: one thread per target
__global__ void span_predict_kernel(const double* __restrict__ U, int64_t M, SpanRegions r, int32_t* __restrict__ spans) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= M) return;
    double c[3], pt[2][4], sm[2][kSpanPatterns];
    weyl_c1c2c3(U + i * 32, 8, c);
    const bool local = target_frame(c, pt, sm);
    spans[i] = span_classify(local, pt, sm, r, r.tol);
}

constexpr int kCoverageBlock = 256;
constexpr int kCoverageLdsBins = 8192;  // 32 KiB of LDS at most: a 26-gate set of three gates (3 653 entries) fits

// the coverage lookup of slam_weyl.hpp
__global__ __launch_bounds__(kCoverageBlock) void coverage_lookup_kernel(
    const double* __restrict__ U, int64_t M, int32_t n_tables, const int32_t* __restrict__ offsets, const int32_t* __restrict__ kinds,
    const double* __restrict__ points, const double* __restrict__ bounds, double tol, int32_t lds_bins,
    unsigned long long* __restrict__ counts, int32_t* __restrict__ entry_out) {
    extern __shared__ unsigned int hist[];
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = i < M;
    double pt[2][4], sm[2][kSpanPatterns];
    const bool local = coverage_target(U, i, live, pt, sm);
    const double t1 = point_tol(tol);
    const const_as_ptr<int32_t> koffsets = (const_as_ptr<int32_t>)offsets;
    const const_as_ptr<int32_t> kkinds = (const_as_ptr<int32_t>)kinds;
    const const_as_ptr<double> kpoints = (const_as_ptr<double>)points;
    const const_as_ptr<double> kbounds = (const_as_ptr<double>)bounds;
    const int32_t base0 = koffsets[0];
    for (int32_t t = 0; t < n_tables; ++t) {
        const int32_t e0 = koffsets[t], e1 = koffsets[t + 1];
        const int32_t n = e1 - e0;
        const int32_t nb = n + 2;
        const int32_t nl = nb < lds_bins ? nb : lds_bins;
        unsigned long long* __restrict__ cnt = counts + (int64_t)(e0 - base0) + 2 * (int64_t)t;
        hist_clear(hist, nl, blockDim.x);
        __syncthreads();
        bool searching = live && !local;
        int32_t found = local ? n : n + 1;
        for (int32_t e = e0; e < e1; ++e) {
            if (!__any(searching)) break;  // wave-uniform exit: e is the same in every lane
            const bool hit = coverage_row_hit(kkinds, kpoints, kbounds, e, pt, sm, tol, t1);
            if (searching && hit) {
                found = e - e0;
                searching = false;
            }
        }
        if (live) {
            if (entry_out) entry_out[(int64_t)t * M + i] = found;
            hist_count(hist, nl, cnt, found);
        }
        __syncthreads();
        hist_fold(hist, nl, blockDim.x, [&](int b) { return &cnt[b]; });
        __syncthreads();  // the next table clears the histogram
    }
}

// ---------------------------------------------------------------------------------
// Family lookup (recursive_sibling_check, src/slam/utils/gates/family_extend.py:17-117, for every resident target): a gate family is
// a base pulse and the same pulse run r = 2^a 3^b times as long ("older siblings"); member m has one table of rows k = 1, 2, ...
// (k applications of it, rows as above) and the cost of row k is (k + 1) cost_1q + k duration_m, computed by the host and read here.
// The walk starts at member 0, finds the first row k of the member that contains the target, and moves on to child_even[m] (k even)
// or child_odd[m] (k odd) until k = 1, the child is missing or the child does not contain the target; unwinding, a level keeps its
// child's result only where that is STRICTLY cheaper.  That unwind is a minimum over the visited levels with ties to the shallower
// one, so one running record (cost, member, k) replaces the per-level records: a level replaces it iff it is strictly cheaper.
// policy 1 ("best") visits every member instead of one path; ties go to the smaller member index by the same rule.
// Children have larger indices than their parents (checked by the host), so ONE ascending pass over the members serves every lane's
// path: lanes whose walk is not at member m idle during m, the row index stays wave-uniform, and the rows arrive by scalar loads as
// in coverage_lookup_kernel.  Two histograms per block in LDS -- all rows + local + unreachable, and member 0's alone (the cost
// without the family, from the same pass) -- folded into global memory with one 64-bit atomic per non-empty bin.
// ---------------------------------------------------------------------------------
constexpr int kFamilyMaxMembers = 32;
constexpr int kFamilyMaxBins = 8192;  // E + 2 + E_0 + 2 bins of LDS at most (32 KiB)

__global__ __launch_bounds__(kCoverageBlock) void family_lookup_kernel(
    const double* __restrict__ U, int64_t M, int32_t n_members, const int32_t* __restrict__ offsets, const int32_t* __restrict__ kinds,
    const double* __restrict__ points, const double* __restrict__ bounds, const double* __restrict__ costs,
    const int32_t* __restrict__ child_even, const int32_t* __restrict__ child_odd, double tol, int32_t policy,
    unsigned long long* __restrict__ counts, unsigned long long* __restrict__ base_counts, int32_t* __restrict__ member_out,
    int32_t* __restrict__ gates_out) {
    extern __shared__ unsigned int hist[];
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = i < M;
    double pt[2][4], sm[2][kSpanPatterns];
    const bool local = coverage_target(U, i, live, pt, sm);
    const double t1 = point_tol(tol);
    const const_as_ptr<int32_t> koffsets = (const_as_ptr<int32_t>)offsets;
    const const_as_ptr<int32_t> kkinds = (const_as_ptr<int32_t>)kinds;
    const const_as_ptr<double> kpoints = (const_as_ptr<double>)points;
    const const_as_ptr<double> kbounds = (const_as_ptr<double>)bounds;
    const const_as_ptr<double> kcosts = (const_as_ptr<double>)costs;
    const const_as_ptr<int32_t> keven = (const_as_ptr<int32_t>)child_even;
    const const_as_ptr<int32_t> kodd = (const_as_ptr<int32_t>)child_odd;
    const int32_t E = koffsets[n_members], E0 = koffsets[1];
    const int32_t n_bins = E + 2 + E0 + 2;  // <= kFamilyMaxBins (host)
    hist_clear(hist, n_bins, blockDim.x);
    __syncthreads();
    int32_t cur = (live && !local) ? 0 : -1;  // reference policy: the member the walk is at (-1: over)
    bool reachable = live && !local;            // member 0 contains the target (decided at m = 0)
    double best_cost = __builtin_inf();
    int32_t best_row = -1, best_m = -1, best_k = -1, base_k = 0;
    for (int32_t m = 0; m < n_members; ++m) {
        const int32_t e0 = koffsets[m], e1 = koffsets[m + 1];
        const bool active = policy ? reachable : (cur == m);
        bool searching = active;
        int32_t k = 0;
        for (int32_t e = e0; e < e1; ++e) {
            if (!__any(searching)) break;  // wave-uniform exit: e is the same in every lane
            const bool hit = coverage_row_hit(kkinds, kpoints, kbounds, e, pt, sm, tol, t1);
            if (searching && hit) {
                k = e - e0 + 1;
                searching = false;
            }
        }
        if (!__any(active)) continue;
        const int32_t ce = keven[m], co = kodd[m];
        if (active) {
            if (k > 0) {
                const double c = kcosts[e0 + k - 1];  // (per-lane row: a vector load of eight bytes)
                if (c < best_cost) {
                    best_cost = c;
                    best_row = e0 + k - 1;
                    best_m = m;
                    best_k = k;
                }
                cur = k == 1 ? -1 : ((k & 1) ? co : ce);
            } else {
                cur = -1;
            }
            if (m == 0) {
                base_k = k;
                reachable = k > 0;
            }
        }
    }
    if (live) {
        const int32_t bin = local ? E : (best_row >= 0 ? best_row : E + 1);
        const int32_t bin0 = local ? E0 : (base_k > 0 ? base_k - 1 : E0 + 1);
        atomicAdd(&hist[bin], 1u);
        atomicAdd(&hist[E + 2 + bin0], 1u);
        if (member_out) member_out[i] = local ? -1 : best_m;
        if (gates_out) gates_out[i] = local ? 0 : best_k;
    }
    __syncthreads();
    hist_fold(hist, n_bins, blockDim.x, [&](int b) { return b < E + 2 ? &counts[b] : &base_counts[b - (E + 2)]; });
}

// ---- slam_pd.hpp --------------------------------------------------------------------------------------------------------------------
constexpr int kPdBlock = 128;
constexpr int kPdScanBlock = 256;
constexpr int kRegionBlock = 256;
constexpr int kRegionMax = 256;    // SLAM_REGION_MAX

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
    target_frame(c, pt, sm);  // (kind 0 reads c itself; a dead lane's frame is that of c = 0 and never counts)
    const int nb = 2 * n_regions + 1;
    hist_clear(hist, nb, blockDim.x);
    __syncthreads();
    const double t1 = point_tol(tol);
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
                // row_bounds_hit / row_point_hit written out: called here they make the compiler reload the region's polytope range
                // in every pass of the loop, and the lookup ran 1-2 % slower (profiles/geometry_frame_ab.txt)
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
    hist_fold(hist, nb, blockDim.x, [&](int b) { return &counts[b]; });
}

// ---- slam_kak.hpp -------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kKakBlock) void kak_kernel(const double* __restrict__ U, int64_t M, double* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= M) return;
    Kak k;
    kak_decompose(U + i * 32, k);
    kak_store(k, out + i * kKakRecord);
}

// local-gate completion (slam_kak.hpp): one thread per row
__global__ __launch_bounds__(kKakBlock) void complete_locals_kernel(CompleteArgs a) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.M) return;
    const int n = 6 * (a.k + 1);
    const double* __restrict__ x = a.x + i * n;
    double* __restrict__ xo = a.x_out + i * n;
    const double* __restrict__ T = a.targets + 32 * (int64_t)a.target_of[i];
    double wr[4][4], wi[4][4], u[32];
    template_forward(a, x, wr, wi);
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            u[(r * 4 + c) * 2] = wr[r][c];
            u[(r * 4 + c) * 2 + 1] = wi[r][c];
        }
    Kak kw, kt;
    kak_decompose(u, kw);
    kak_decompose(T, kt);
    a.gap_out[i] = kak_align(kw, kt);
    // L = A_T A_W^+ (layer k), R = B_W^+ B_T (layer 0); index 1 of a pair acts on qubit 1, index 2 on qubit 0
    cplx dg[2][2], L1[2][2], L2[2][2], R1[2][2], R2[2][2], u3[2][2], m[2][2];
    dagger2(kw.a1, dg);
    mul2(kt.a1, dg, L1);
    dagger2(kw.a2, dg);
    mul2(kt.a2, dg, L2);
    dagger2(kw.b1, dg);
    mul2(dg, kt.b1, R1);
    dagger2(kw.b2, dg);
    mul2(dg, kt.b2, R2);
    for (int j = 6; j < n - 6; ++j) xo[j] = x[j];
    u3_matrix(x, u3);
    mul2(u3, R2, m);
    put_u3(m, xo);
    u3_matrix(x + 3, u3);
    mul2(u3, R1, m);
    put_u3(m, xo + 3);
    u3_matrix(x + n - 6, u3);
    mul2(L2, u3, m);
    put_u3(m, xo + n - 6);
    u3_matrix(x + n - 3, u3);
    mul2(L1, u3, m);
    put_u3(m, xo + n - 3);
    a.loss_out[i] = template_loss(a, T, xo, wr, wi);
}

}  // namespace slamdev
