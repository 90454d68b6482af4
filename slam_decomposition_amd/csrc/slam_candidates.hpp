// slam_candidates.hpp -- candidate basis-gate scoring (slam_candidate_scores; gfx950 only).  Included by slam_geometry.hip alone, which
// is the one unit that emits these kernels.
//
// The reference scores a grid of ConversionGainGate candidates by what k applications of each can reach (collect_data,
// src/slam/utils/gates/bare_candidates.py:75-126: the Haar-expected gate count and the first sizes that reach CNOT and SWAP).  Here the
// question is asked per (candidate, target): the smallest k in 1 .. k_cap such that k copies of the candidate, with free local gates in
// between, reach the target -- coverage.contains(t, [g] * k, tol) on the host.
//
// Rows.  The region of k copies of one gate is a max-plus dynamic programme over the small quantum cohomology rings of Gr(1, 4),
// Gr(2, 4) and Gr(3, 4) (coverage._region).  There the state is keyed by (degree d, partition) and the bound is the value minus d; d is
// additive along a product, so it folds into the weight and the state is the partition alone: 4 + 6 + 4 = 14 weights, numbered like the
// 14 subsets I of coverage._PATTERNS (the Schubert class of subset I).  One more copy of the gate is
//     w'[to] = max over the ring's terms  q^d sigma_to  in  sigma_from * sigma_x  of  w[from] + v[x] - d,      v[x] = sum_{i in I_x} a_i,
// 72 terms in all (SLAM_CAND_TERMS, generated from the tables in coverage.py and pinned against coverage.region by
// tests/test_candidates_host.py), and the half-space of pattern kCandPattern[s] (the dual class) is bounded by w[s].
// candidate_rows_kernel runs that recurrence, one thread per candidate, and leaves rows k = 2 .. k_cap in device memory;
// nothing but the three coordinates per candidate comes from the host.
//
// Lookup.  candidate_scores_kernel: one thread per target (both alcove points and the 2 x 14 sums in registers, coverage_target), the
// candidate index and k wave-uniform, so the rows arrive by scalar loads as in coverage_lookup_kernel; a wavefront leaves a candidate's
// k-loop when none of its lanes is still searching.  grid.y splits the candidates into chunks so that a small batch still fills the
// device.  With one group the block counts a tile of kCandTile candidates at a time in an LDS histogram (one clear and two barriers
// per TILE) and folds its non-empty bins into `counts` with one 64-bit atomic each; with groups every target adds to its group's bin
// directly.  Integer counts: the result does not depend on the grid, the window or the order of the additions.
#pragma once
#include "slam_weyl.hpp"

namespace slamdev {

constexpr int kCandMaxK = 64;   // SLAM_CANDIDATE_MAX_K
constexpr int kCandBlock = 256;
constexpr int kCandTile = 32;   // candidates per LDS histogram: 32 x 66 bins x 4 B = 8.25 KiB
constexpr int kCandRowsBlock = 64;

// X(from, x, to, d): q^d sigma_to is a term of sigma_from * sigma_x; states 0..3 Gr(1, 4), 4..9 Gr(2, 4), 10..13 Gr(3, 4)
#define SLAM_CAND_TERMS(X)                                                                                                              \
    X(0, 0, 1, 1) X(0, 1, 2, 1) X(0, 2, 3, 1) X(0, 3, 0, 0) X(1, 0, 2, 1) X(1, 1, 3, 1) X(1, 2, 0, 0) X(1, 3, 1, 0)                      \
    X(2, 0, 3, 1) X(2, 1, 0, 0) X(2, 2, 1, 0) X(2, 3, 2, 0) X(3, 0, 0, 0) X(3, 1, 1, 0) X(3, 2, 2, 0) X(3, 3, 3, 0)                      \
    X(4, 4, 9, 2) X(4, 5, 5, 1) X(4, 6, 7, 1) X(4, 7, 6, 1) X(4, 8, 8, 1) X(4, 9, 4, 0) X(5, 4, 5, 1) X(5, 5, 6, 1)                      \
    X(5, 5, 7, 1) X(5, 6, 8, 1) X(5, 7, 8, 1) X(5, 8, 4, 0) X(5, 8, 9, 1) X(5, 9, 5, 0) X(6, 4, 7, 1) X(6, 5, 8, 1)                      \
    X(6, 6, 4, 0) X(6, 7, 9, 1) X(6, 8, 5, 0) X(6, 9, 6, 0) X(7, 4, 6, 1) X(7, 5, 8, 1) X(7, 6, 9, 1) X(7, 7, 4, 0)                      \
    X(7, 8, 5, 0) X(7, 9, 7, 0) X(8, 4, 8, 1) X(8, 5, 4, 0) X(8, 5, 9, 1) X(8, 6, 5, 0) X(8, 7, 5, 0) X(8, 8, 6, 0)                      \
    X(8, 8, 7, 0) X(8, 9, 8, 0) X(9, 4, 4, 0) X(9, 5, 5, 0) X(9, 6, 6, 0) X(9, 7, 7, 0) X(9, 8, 8, 0) X(9, 9, 9, 0)                      \
    X(10, 10, 11, 1) X(10, 11, 12, 1) X(10, 12, 13, 1) X(10, 13, 10, 0) X(11, 10, 12, 1) X(11, 11, 13, 1) X(11, 12, 10, 0)              \
    X(11, 13, 11, 0) X(12, 10, 13, 1) X(12, 11, 10, 0) X(12, 12, 11, 0) X(12, 13, 12, 0) X(13, 10, 10, 0) X(13, 11, 11, 0)              \
    X(13, 12, 12, 0) X(13, 13, 13, 0)

// state s bounds the half-space of this pattern (the dual class's subset, coverage._PATTERNS order)
#define SLAM_CAND_PATTERNS {3, 2, 1, 0, 9, 8, 6, 7, 5, 4, 13, 12, 11, 10}

// rows of every candidate: points[g][4] (k = 1: the alcove point of the gate) and rows[g][k - 2][14] (k = 2 .. k_cap)
__global__ __launch_bounds__(kCandRowsBlock) void candidate_rows_kernel(const double* __restrict__ coords, int32_t G, int32_t k_cap,
                                                                        double* __restrict__ points, double* __restrict__ rows) {
    const int32_t g = (int32_t)(blockIdx.x * blockDim.x + threadIdx.x);
    if (g >= G) return;
    double a[4];
    alcove_point(coords[3 * (int64_t)g], coords[3 * (int64_t)g + 1], coords[3 * (int64_t)g + 2], 0.0, a);
#pragma unroll
    for (int j = 0; j < 4; ++j) points[4 * (int64_t)g + j] = a[j];
    // sums over the subsets I (coverage._PATTERNS order, 1-based indices into the decreasing point), added left to right as on the host
    const double v[kSpanPatterns] = {a[0], a[1], a[2], a[3], a[0] + a[1], a[0] + a[2], a[0] + a[3], a[1] + a[2], a[1] + a[3], a[2] + a[3],
                                     a[0] + a[1] + a[2], a[0] + a[1] + a[3], a[0] + a[2] + a[3], a[1] + a[2] + a[3]};
    constexpr int pattern[kSpanPatterns] = SLAM_CAND_PATTERNS;
    double w[kSpanPatterns];
#pragma unroll
    for (int s = 0; s < kSpanPatterns; ++s) w[s] = v[s];
    double* __restrict__ out = rows + (int64_t)g * (k_cap - 1) * kSpanPatterns;
    for (int k = 2; k <= k_cap; ++k) {
        double n[kSpanPatterns];
#pragma unroll
        for (int s = 0; s < kSpanPatterns; ++s) n[s] = -INFINITY;
#define SLAM_CAND_STEP(from, x, to, d) n[to] = fmax(n[to], w[from] + v[x] - (double)(d));
        SLAM_CAND_TERMS(SLAM_CAND_STEP)
#undef SLAM_CAND_STEP
#pragma unroll
        for (int s = 0; s < kSpanPatterns; ++s) {
            w[s] = n[s];
            out[pattern[s]] = n[s];
        }
        out += kSpanPatterns;
    }
}

// counts[group][g][k_cap + 2]: bins 0 .. k_cap - 1 = first reached at k = bin + 1, bin k_cap = local target, bin k_cap + 1 = not reached;
// first_k[g][M] (or NULL): k, 0 local, k_cap + 1 not reached.  Block (x, y): targets [256 x, 256 x + 256), candidates [chunk y, chunk y + chunk).
__global__ __launch_bounds__(kCandBlock) void candidate_scores_kernel(const double* __restrict__ U, int64_t M, int32_t G, int32_t chunk,
                                                                      int32_t k_cap, const double* __restrict__ points,
                                                                      const double* __restrict__ rows, double tol,
                                                                      const int32_t* __restrict__ group_of,
                                                                      unsigned long long* __restrict__ counts, int32_t* __restrict__ first_k) {
    __shared__ unsigned int hist[kCandTile * (kCandMaxK + 2)];
    const int64_t i = (int64_t)blockIdx.x * kCandBlock + threadIdx.x;
    const bool live = i < M;
    double pt[2][4], sm[2][kSpanPatterns];
    const bool local = coverage_target(U, i, live, pt, sm);
    const double t1 = point_tol(tol);
    const const_as_ptr<double> kpoints = (const_as_ptr<double>)points;
    const const_as_ptr<double> krows = (const_as_ptr<double>)rows;
    const int32_t nb = k_cap + 2;
    const int32_t g_lo = (int32_t)blockIdx.y * chunk;
    const int32_t g_hi = g_lo + chunk < G ? g_lo + chunk : G;
    const int64_t grp = (group_of && live) ? group_of[i] : 0;
    for (int32_t t0 = g_lo; t0 < g_hi; t0 += kCandTile) {
        const int32_t tn = g_hi - t0 < kCandTile ? g_hi - t0 : kCandTile;
        if (!group_of) {
            hist_clear(hist, tn * nb, kCandBlock);
            __syncthreads();
        }
        for (int32_t j = 0; j < tn; ++j) {
            const int32_t g = t0 + j;
            bool searching = live && !local;
            int32_t found = local ? 0 : k_cap + 1;
            {  // k = 1
                const bool hit = row_point_hit(pt, kpoints + (int64_t)g * 4, t1);
                if (searching && hit) {
                    found = 1;
                    searching = false;
                }
            }
            const const_as_ptr<double> rg = krows + (int64_t)g * (k_cap - 1) * kSpanPatterns;
            for (int32_t k = 2; k <= k_cap; ++k) {
                if (!__any(searching)) break;  // wave-uniform exit: (g, k) is the same in every lane
                const bool hit = row_bounds_hit(sm, rg + (int64_t)(k - 2) * kSpanPatterns, tol);
                if (searching && hit) {
                    found = k;
                    searching = false;
                }
            }
            if (live) {
                if (first_k) first_k[(int64_t)g * M + i] = found;
                const int32_t b = found == 0 ? k_cap : (found > k_cap ? k_cap + 1 : found - 1);
                if (!group_of)
                    atomicAdd(&hist[j * nb + b], 1u);
                else
                    atomicAdd(&counts[(grp * G + g) * nb + b], 1ull);
            }
        }
        if (!group_of) {
            __syncthreads();
            hist_fold(hist, tn * nb, kCandBlock, [&](int b) { return &counts[(int64_t)t0 * nb + b]; });
            __syncthreads();  // the next tile clears the histogram
        }
    }
}

}  // namespace slamdev
