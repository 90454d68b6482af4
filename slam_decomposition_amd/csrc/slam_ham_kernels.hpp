// slam_ham_kernels.hpp -- the kernels of the Hamiltonian templates around eval_ham (slam_ham.hpp); included by slam_ham_host.hip alone.
#pragma once
#include "slam_ham.hpp"

namespace slamdev {

// ---------------------------------------------------------------------------------------------------------------------------
// slam_ham_eval: one item per wavefront, grid-stride
// ---------------------------------------------------------------------------------------------------------------------------
// (two wavefronts per SIMD: with the unitary wanted and the any-argument sincos path the evaluation does not fit 128 registers)
__global__ void __launch_bounds__(kWave, 2) eval_ham_kernel(HamEvalArgs a) {
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const int lane = threadIdx.x;
    const int n = a.h.n;
    ham_prologue(lds, a.h);
    const int ent = ((lane & 7) * 8 + (lane >> 3)) * 2;  // entry (r, c) of a row-major 8x8
    for (int64_t m = blockIdx.x; m < a.n_items; m += gridDim.x) {
#pragma unroll
        for (int s = 0; s < kQ3Slots; ++s) {
            const int i = 2 * lane + s;
            lds[kQ3OffX + i] = i < n ? a.x[m * n + i] : 0.0;
        }
        lds_fence();
        const double2 t = q3_item_entry<false>(a.targets, (int64_t)a.target_of[m], lane, ent);
        double wr = 0.0, wi = 0.0;
        const double f = eval_ham<true, true>(lds, t.x, t.y, n, a.h.t_index, a.h.dim, a.cost_kind, wr, wi);
        if (lane == 0) a.loss[m] = f;
        if (a.grad && lane < n) a.grad[m * n + lane] = lds[kQ3OffG + lane];
        if (a.unitary) *reinterpret_cast<double2*>(a.unitary + m * 128 + ent) = make_double2(wr, wi);
        lds_fence();
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// slam_ham_minimize: the optimizer body of the three-qubit templates around eval_ham
// ---------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kWave, 3) minimize_ham_kernel(HamArgs args) {
    constexpr bool STATE = false;
#define Q3_MIN_SETUP const int n = args.h.n;
#define Q3_MIN_PROLOGUE ham_prologue(lds, args.h);
#define Q3_MIN_EVAL eval_ham<false, false>(lds, tre, tim, n, args.h.t_index, args.h.dim, args.cost_kind, wre, wim)
#include "slam_q3_minimize.inc"
#undef Q3_MIN_SETUP
#undef Q3_MIN_PROLOGUE
#undef Q3_MIN_EVAL
}

}  // namespace slamdev
