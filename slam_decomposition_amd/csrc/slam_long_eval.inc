// slam_long_eval.inc -- body of eval_long_kernel / eval_long_mk_kernel (slam_long.hpp), included inside the kernel with the constant MK (MakhlinFunctionalCost) defined.
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const int lane = threadIdx.x;
    const int n = 6 * (a.k + 1);
    long_prologue(lds);
    const LongGateCols gcol = load_gate_cols(a.gates, a.k);
    for (int64_t item = blockIdx.x; item < a.n_items; item += gridDim.x) {
        const int64_t tgt = a.target_of[item];
#pragma unroll
        for (int s = 0; s < kLongSlots; ++s) {
            const int i = 2 * lane + s;
            lds[kLongOffX + i] = (i < n) ? a.x[item * n + i] : 0.0;
        }
        lds_fence();
        double tre[4], tim[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const double2 t = *reinterpret_cast<const double2*>(a.targets + tgt * 32 + (lane & 3) * 2 + 8 * r);
            tre[r] = t.x;
            tim[r] = t.y;
        }
        double f;
        if constexpr (MK) {
            double gT[3];
            mk_target_g(a.targets + tgt * 32 + (lane & 3) * 2, lane & 3, gT);
            f = eval_long<true, true>(lds, tre, tim, gcol, a.k, a.cost_kind, false, gT);
        } else {
            f = eval_long<true>(lds, tre, tim, gcol, a.k, a.cost_kind, false);
        }
        if (lane == 0) a.loss[item] = f;
        if (a.grad) {
#pragma unroll
            for (int s = 0; s < kLongSlots; ++s) {
                const int i = 2 * lane + s;
                if (i < n) a.grad[item * n + i] = lds[kLongOffG + i];
            }
        }
        if (a.unitary && lane < 16) {
            // W = Pre_{L-1}, column-major in LDS -> row-major (re, im) out
            const double2 e = reinterpret_cast<const double2*>(lds + kLongOffPre)[a.k * 16 + lane];  // element (r = lane & 3, col = lane >> 2)
            const int r = lane & 3, cc = lane >> 2;
            a.unitary[item * 32 + (r * 4 + cc) * 2] = e.x;
            a.unitary[item * 32 + (r * 4 + cc) * 2 + 1] = e.y;
        }
        lds_fence();
    }
