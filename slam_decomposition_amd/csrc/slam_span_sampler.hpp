// slam_span_sampler.hpp -- Haar candidates selected by template size on the device (slam_haar_select_spans).
//
// Reference: Haar2Sample / Haar3Sample (src/slam/sampler.py:73-107) draw a unitary on the host, run the analytic sqrt(iSWAP) pass, count
// its gates and throw the draw away on a mismatch.  Here one thread draws candidate i of the Philox stream (haar_unitary, the generator
// of slam_sample_haar), classifies it in registers (weyl_c1c2c3 + span_classify, the classifier of slam_predict_spans) and votes; a
// rejected candidate never reaches memory.  What leaves the device is the ordered list of the selected candidates' stream indices.
//
// Order without atomics -- the position of a selected candidate is its rank among the selected ones:
//   haar_span_select_kernel   per wavefront the 64-bit ballot of the votes (masks[wave]), per block the number of votes (totals[block]:
//                             the wavefronts' popcounts meet in LDS)
//   span_scan_kernel          one block: exclusive scan of totals -> offsets[block], the grand total -> *n_selected
//   span_scatter_kernel       same geometry as the first kernel: rank = offsets[block] + popcounts of the block's earlier wavefronts
//                             + popcount of the own mask below the lane; ranks below `capacity` write first_index + t
// so the list is a function of the arguments alone.  The span histogram (integers) goes through LDS and one 64-bit atomic per
// non-empty bin and block, as in coverage_lookup_kernel.
#pragma once
#include "slam_sampler.hpp"
#include "slam_weyl.hpp"

namespace slamdev {

constexpr int kSelBlock = 256;                  // 4 wavefronts: one per SIMD, the whole register file for the fused generator + classifier
constexpr int kSelWaves = kSelBlock / 64;
constexpr int kSelBins = 16 + 2;                // SLAM_MAX_SPAN_EVAL + 2: 0 local, 1 .. k_max, k_max + 1 out of reach
constexpr int kScanBlock = 1024;

struct SelArgs {
    uint64_t seed;
    int64_t first_index, n;
    double margin;             // > 0: the span must not change at tol + margin and tol - margin
    int32_t span_lo, span_hi;  // selected: span_lo <= span <= span_hi
};

__global__ __launch_bounds__(kSelBlock) void haar_span_select_kernel(SpanRegions r, SelArgs a, unsigned long long* __restrict__ masks,
                                                                     uint32_t* __restrict__ totals, unsigned long long* __restrict__ counts) {
    __shared__ unsigned int hist[kSelBins];
    __shared__ unsigned int wave_votes[kSelWaves];
    hist_clear(hist, kSelBins, kSelBlock);
    __syncthreads();
    const int64_t t = (int64_t)blockIdx.x * kSelBlock + threadIdx.x;
    bool vote = false;
    if (t < a.n) {
        double zr[4][4], zi[4][4];
        haar_unitary(a.seed, (uint64_t)(a.first_index + t), zr, zi);
        double U[32];
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            U[2 * e] = zr[e >> 2][e & 3];
            U[2 * e + 1] = zi[e >> 2][e & 3];
        }
        // slam_sample_haar rounds every entry to a double on its way to memory before slam_predict_spans reads it; the empty
        // statement keeps the compiler from contracting the generator's last multiply into the classifier's first additions
#pragma unroll
        for (int e = 0; e < 32; ++e) asm volatile("" : "+v"(U[e]));
        double c[3];
        weyl_c1c2c3(U, 8, c);
        double pt[2][4], sm[2][kSpanPatterns];
        const bool local = target_frame(c, pt, sm);  // one frame for the three classifications: it does not depend on the tolerance
        const int span = span_classify(local, pt, sm, r, r.tol);
        atomicAdd(&hist[span], 1u);
        vote = span >= a.span_lo && span <= a.span_hi;
        if (vote && a.margin > 0.0)
            vote = span_classify(local, pt, sm, r, r.tol + a.margin) == span && span_classify(local, pt, sm, r, r.tol - a.margin) == span;
    }
    const unsigned long long m = __ballot(vote);
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        masks[(int64_t)blockIdx.x * kSelWaves + w] = m;
        wave_votes[w] = (unsigned int)__popcll(m);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned int s = 0u;
#pragma unroll
        for (int j = 0; j < kSelWaves; ++j) s += wave_votes[j];
        totals[blockIdx.x] = s;
    }
    hist_fold(hist, kSelBins, kSelBlock, [&](int b) { return &counts[b]; });
}

// one block: offsets[b] = totals[0] + .. + totals[b - 1], *n_selected = the sum of all (at most 2^31 - 1 candidates: 32 bits hold it)
__global__ __launch_bounds__(kScanBlock) void span_scan_kernel(const uint32_t* __restrict__ totals, int64_t n_blocks, uint32_t* __restrict__ offsets,
                                                               unsigned long long* __restrict__ n_selected) {
    __shared__ uint32_t wave_sum[kScanBlock / 64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    uint32_t carry = 0u;
    for (int64_t base = 0; base < n_blocks; base += kScanBlock) {
        const int64_t b = base + threadIdx.x;
        const uint32_t v = b < n_blocks ? totals[b] : 0u;
        uint32_t incl = v;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t up = __shfl_up(incl, d, 64);
            if (lane >= d) incl += up;
        }
        if (lane == 63) wave_sum[w] = incl;
        __syncthreads();
        uint32_t before = 0u, chunk = 0u;
#pragma unroll
        for (int j = 0; j < kScanBlock / 64; ++j) {
            const uint32_t s = wave_sum[j];
            before += j < w ? s : 0u;
            chunk += s;
        }
        if (b < n_blocks) offsets[b] = carry + before + incl - v;
        carry += chunk;
        __syncthreads();  // the next chunk overwrites wave_sum
    }
    if (threadIdx.x == 0) *n_selected = carry;
}

__global__ __launch_bounds__(kSelBlock) void span_scatter_kernel(const unsigned long long* __restrict__ masks, const uint32_t* __restrict__ offsets,
                                                                 int64_t first_index, int64_t capacity, int64_t* __restrict__ indices) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int64_t rank = offsets[blockIdx.x];
    if (rank >= capacity) return;  // every later rank of the block is larger still
    unsigned long long mine = 0ull;
#pragma unroll
    for (int j = 0; j < kSelWaves; ++j) {
        const unsigned long long m = masks[(int64_t)blockIdx.x * kSelWaves + j];
        if (j < w) rank += __popcll(m);
        if (j == w) mine = m;
    }
    rank += __popcll(mine & ((1ull << lane) - 1ull));
    if (((mine >> lane) & 1ull) && rank < capacity) indices[rank] = first_index + (int64_t)blockIdx.x * kSelBlock + threadIdx.x;
}

}  // namespace slamdev
