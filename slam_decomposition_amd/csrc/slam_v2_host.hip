// slam_v2_host.hip -- host side of libslamhip.so, parametrised-gate unit: slam_v2_* (CircuitTemplateV2, src/slam/basisv2.py:27-299) on the
// kernels of slam_v2.hpp.  The span loop's bookkeeping kernels are enqueued through slam_hip.hip (slam_host.hpp).
#include "slam_host.hpp"
#include "slam_v2.hpp"

namespace {

template <int K, int QN>
constexpr size_t v2_lds_bytes() { return sizeof(double) * CfgV2<K, QN>::LDS_DOUBLES; }

int v2_stage_maps(slam_ctx* c, int k, const int32_t* gate_seq, const V2GateMap** d_out) {
    if (c->v2_gates_host.empty()) return fail(SLAM_ERR_STATE, "no parametrised gates: call slam_v2_set_gates first");
    if (!gate_seq) return fail(SLAM_ERR_INVALID, "gate_seq is NULL");
    V2GateMap tmp[SLAM_MAX_SPAN_EVAL];
    for (int j = 0; j < k; ++j) {
        if (gate_seq[j] < 0 || gate_seq[j] >= (int)c->v2_gates_host.size())
            return fail(SLAM_ERR_INVALID, "gate_seq[%d] = %d outside the parametrised gate table (%d gates)", j, gate_seq[j], (int)c->v2_gates_host.size());
        tmp[j] = c->v2_gates_host[(size_t)gate_seq[j]];
    }
    HIP_TRY(c->v2_maps.reserve(sizeof(V2GateMap) * SLAM_MAX_SPAN_EVAL));
    HIP_TRY(hipMemcpyAsync(c->v2_maps.p, tmp, sizeof(V2GateMap) * (size_t)k, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));  // tmp is a stack buffer
    *d_out = c->v2_maps.as<V2GateMap>();
    return SLAM_OK;
}

template <int K, int QN>
int v2_launch_eval(slam_ctx* c, const V2GateMap* d_maps, const double* d_x, const int32_t* d_tof, int64_t M, double* d_loss, double* d_grad,
                   double* d_unitary) {
    const size_t lds = v2_lds_bytes<K, QN>();
    { int rc = kernel_per_cu(c, reinterpret_cast<const void*>(&eval_v2_kernel<K, QN>), lds, nullptr); if (rc) return rc; }
    EvalV2Args<K, QN> a{};
    a.targets = c->targets.as<double>();
    a.x = d_x;
    a.target_of = d_tof;
    a.n_items = M;
    a.loss = d_loss;
    a.grad = d_grad;
    a.unitary = d_unitary;
    a.cost_kind = c->cost_kind;
    a.maps = d_maps;
    hipLaunchKernelGGL((eval_v2_kernel<K, QN>), dim3((unsigned)((M + kQuadsPerWave - 1) / kQuadsPerWave)), dim3(kWave), lds, c->stream, a);
    HIP_TRY(hipGetLastError());
    return SLAM_OK;
}

struct V2Stage {
    bool bounded;        // some parameter has a finite bound (or is fixed): projected steps; else plain BFGS
    bool riswap_like;    // every gate of the span: only the angle a moves, phi_c = b = 0
    bool count_on_device = false;  // the kernel reads the stage's target count from its control block (n_active = upper bound)
    int k = 0;
    double exit_loss;
    const V2GateMap* d_maps;
    const int32_t* d_active;
    int32_t n_active;
    const double* d_x0;
    const double* d_bounds;  // init_lo | init_hi | bound_lo | bound_hi, n each
    const slam_opt_params* prm;
};

constexpr int kV2HmemWavesPerCu = 8;  // wavefronts per CU whose inverse Hessian lives in device memory (v2_hmem slices)

template <int K, int QN, int GQ, bool FREE>
int v2_launch_minimize_gq(slam_ctx* c, const V2Stage& sgt) {
    const size_t lds = v2_lds_bytes<K, QN>();
    // attribute + occupancy once per context and instantiation (both were runtime calls inside every stage launch of the
    // span loop's chain)
    int per_cu = 0;
    { int rc = kernel_per_cu(c, reinterpret_cast<const void*>(&minimize_v2_kernel<K, QN, GQ, FREE>), lds, &per_cu); if (rc) return rc; }
    constexpr int n = CfgV2<K, QN>::N;
    MinimizeV2Args<K, QN> a{};
    fill_stage_common(a, c, sgt.prm, sgt.exit_loss);
    a.targets = c->targets.as<double>();
    a.active = sgt.d_active;
    a.n_active = sgt.count_on_device ? -1 : sgt.n_active;
    a.x0 = sgt.d_x0;
    a.init_lo = sgt.d_bounds;
    a.init_hi = sgt.d_bounds + n;
    a.bound_lo = sgt.d_bounds + 2 * n;
    a.bound_hi = sgt.d_bounds + 3 * n;
    a.maps = sgt.d_maps;
    a.ctl = stage_ctl(c, K);
    a.bounded = sgt.bounded ? 1 : 0;
    if (c->v2_cons_n[K] > 0) {
        if (c->v2_cons_n[K] != n) return fail(SLAM_ERR_STATE, "the cost constraint of span %d was set for %d parameters, the template has %d (set the gates first)", K, c->v2_cons_n[K], n);
        if (FREE) return fail(SLAM_ERR_STATE, "internal: constrained stage dispatched to the unbounded kernel");
        a.cons_w = c->v2_cons_w[K].as<double>();
        // results are feasible: the multiplier loop ends with c <= tol against a right-hand side lowered by tol
        a.cons_tol = 1e-8 * (1.0 + std::fabs(c->v2_cons_max[K]));
        a.cons_max = c->v2_cons_max[K] - a.cons_tol;
        a.cons_rho = c->v2_cons_rho[K];
        a.bounded = 1;
    }
    // persistent wavefronts: never more than can be resident; every quad pulls items from the stage's queue
    const int64_t M = (int64_t)sgt.n_active * sgt.prm->restarts;
    int64_t blocks = (M + kQuadsPerWave - 1) / kQuadsPerWave;
    // (in-memory metric: at most kV2HmemWavesPerCu wavefronts per CU -- the bound v2_decompose_body sizes v2_hmem with up front, so the
    // per-stage reserve below can never grow the buffer in the middle of a chain: ADVICE r4)
    const int64_t cap = (int64_t)(v2_h_in_memory<K, QN>() && per_cu > kV2HmemWavesPerCu ? kV2HmemWavesPerCu : per_cu) * c->compute_units;
    if (blocks > cap) blocks = cap;
    if constexpr (v2_h_in_memory<K, QN>()) {
        HIP_TRY(c->v2_hmem.reserve((size_t)blocks * v2_h_floats_per_wave<K, QN>() * sizeof(float)));
        a.hmem = c->v2_hmem.as<float>();
    }
    HIP_TRY(hipEventRecord(c->ev_a[K], c->stream));
    hipLaunchKernelGGL((minimize_v2_kernel<K, QN, GQ, FREE>), dim3((unsigned)blocks), dim3(kWave), lds, c->stream, a);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(c->ev_b[K], c->stream));
    return SLAM_OK;
}

// gate sub-class of the stage (slam_v2.hpp): one parameter per gate that only moves the angle a, phi_c = b = 0 (RiSwapGate)
template <int K, int QN>
int v2_launch_minimize(slam_ctx* c, const V2Stage& sgt) {
    if constexpr (QN == 1 && K <= 3) {
        if (sgt.riswap_like && !sgt.bounded && c->v2_cons_n[K] == 0) return v2_launch_minimize_gq<K, QN, 1, true>(c, sgt);  // RiSwapGate class, plain BFGS
        if (sgt.riswap_like) return v2_launch_minimize_gq<K, QN, 1, false>(c, sgt);
    }
    if (!sgt.bounded && c->v2_cons_n[K] == 0) return v2_launch_minimize_gq<K, QN, 0, true>(c, sgt);  // general gates, plain BFGS
    return v2_launch_minimize_gq<K, QN, 0, false>(c, sgt);
}

// spans 1..3 with 1, 2 or 4 parameters per gate; spans 4 and 5 (the reference's default maximum_span_guess = 5,
// basisv2.py:35) where the packed inverse Hessian still fits one wavefront's 512 registers: n <= 41 parameters
#define SLAM_V2_DISPATCH(FN, ...)                                                                             \
    do {                                                                                                      \
        const int key = k * 10 + c->v2_qn;                                                                    \
        switch (key) {                                                                                        \
            case 11: rc = FN<1, 1>(__VA_ARGS__); break;                                                       \
            case 12: rc = FN<1, 2>(__VA_ARGS__); break;                                                       \
            case 14: rc = FN<1, 4>(__VA_ARGS__); break;                                                       \
            case 21: rc = FN<2, 1>(__VA_ARGS__); break;                                                       \
            case 22: rc = FN<2, 2>(__VA_ARGS__); break;                                                       \
            case 24: rc = FN<2, 4>(__VA_ARGS__); break;                                                       \
            case 31: rc = FN<3, 1>(__VA_ARGS__); break;                                                       \
            case 32: rc = FN<3, 2>(__VA_ARGS__); break;                                                       \
            case 34: rc = FN<3, 4>(__VA_ARGS__); break;                                                       \
            case 41: rc = FN<4, 1>(__VA_ARGS__); break;                                                       \
            case 42: rc = FN<4, 2>(__VA_ARGS__); break;                                                       \
            case 51: rc = FN<5, 1>(__VA_ARGS__); break;                                                       \
            default: rc = fail(SLAM_ERR_UNSUPPORTED, "parametrised-gate templates: spans 1..3 with 1, 2 or 4 parameters per gate, span 4 with 1 or 2, span 5 with 1 (got span %d, %d)", \
                               k, c->v2_qn);                                                                  \
        }                                                                                                     \
    } while (0)

int v2_eval_body(slam_ctx* c, int k, const int32_t* gate_seq, const double* x, const int32_t* target_of, int64_t M, double* loss,
                 double* grad, double* unitary) {
    if (!c) return fail(SLAM_ERR_INVALID, "ctx is NULL");
    if (c->cost_kind == SLAM_COST_MAKHLIN)
        return fail(SLAM_ERR_UNSUPPORTED, "parametrised-gate templates do not run MakhlinFunctionalCost (SLAM_COST_MAKHLIN)");
    HIP_TRY(hipSetDevice(c->device));
    if (c->n_targets <= 0) return fail(SLAM_ERR_STATE, "no targets: call slam_set_targets first");
    if (k < 1 || k > SLAM_V2_MAX_SPAN) return fail(SLAM_ERR_UNSUPPORTED, "parametrised-gate templates support spans 1..%d (got %d)", SLAM_V2_MAX_SPAN, k);
    if (M < 0) return fail(SLAM_ERR_INVALID, "M < 0");
    if (M == 0) return SLAM_OK;
    if (!x || !target_of || !loss) return fail(SLAM_ERR_INVALID, "x, target_of and loss must be non-NULL");
    const V2GateMap* d_maps = nullptr;
    int rc = v2_stage_maps(c, k, gate_seq, &d_maps);
    if (rc) return rc;
    const int n = 6 * (k + 1) + c->v2_qn * k;
    EvalBufs d{};
    rc = stage_eval_inputs(c, x, target_of, M, n, grad != nullptr, unitary != nullptr, &d);
    if (rc) return rc;
    SLAM_V2_DISPATCH(v2_launch_eval, c, d_maps, d.x, d.target_of, M, d.loss, d.grad, d.unitary);
    if (rc) return rc;
    rc = enqueue_eval_readback(c, M, n, loss, grad, unitary);
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(c->stream));
    return SLAM_OK;
}

int v2_minimize_body(slam_ctx* c, int k, const int32_t* gate_seq, const int32_t* active, int64_t n_active, const double* x0,
                     const double* init_lo, const double* init_hi, const double* bound_lo, const double* bound_hi,
                     const slam_opt_params* prm, double exit_loss, double* best_loss, double* best_x, int32_t* best_restart,
                     double* item_loss, int32_t* item_iters, int32_t* item_status, int32_t* item_evals) {
    if (!c) return fail(SLAM_ERR_INVALID, "ctx is NULL");
    if (c->cost_kind == SLAM_COST_MAKHLIN)
        return fail(SLAM_ERR_UNSUPPORTED, "parametrised-gate templates do not run MakhlinFunctionalCost (SLAM_COST_MAKHLIN)");
    HIP_TRY(hipSetDevice(c->device));
    if (c->n_targets <= 0) return fail(SLAM_ERR_STATE, "no targets: call slam_set_targets first");
    if (k < 1 || k > SLAM_V2_MAX_SPAN) return fail(SLAM_ERR_UNSUPPORTED, "parametrised-gate templates support spans 1..%d (got %d)", SLAM_V2_MAX_SPAN, k);
    int rc = check_params(prm);
    if (rc) return rc;
    if (!active) n_active = c->n_targets;
    if (n_active <= 0) return n_active == 0 ? SLAM_OK : fail(SLAM_ERR_INVALID, "n_active < 0");
    if (!best_loss || !best_x) return fail(SLAM_ERR_INVALID, "best_loss and best_x must be non-NULL");
    if (!init_lo || !init_hi) return fail(SLAM_ERR_INVALID, "init_lo and init_hi must be non-NULL");
    const V2GateMap* d_maps = nullptr;
    rc = v2_stage_maps(c, k, gate_seq, &d_maps);
    if (rc) return rc;
    const int n = 6 * (k + 1) + c->v2_qn * k;
    const int32_t* d_active = nullptr;
    const double* d_x0 = nullptr;
    bool bounded = false;
    rc = stage_family_inputs(c, k, n, active, n_active, x0, init_lo, init_hi, bound_lo, bound_hi, prm, &d_active, &d_x0, &bounded);
    if (rc) return rc;
    bool riswap_like = c->v2_qn == 1;
    for (int j = 0; j < k && riswap_like; ++j) {
        const V2GateMap& gm = c->v2_gates_host[(size_t)gate_seq[j]];
        riswap_like = gm.sel[1] < 0 && gm.sel[2] < 0 && gm.offset[1] == 0.0 && gm.offset[2] == 0.0;  // phi_c = 0, b = 0 (phi_g: no effect then)
    }
    V2Stage sgt{bounded, riswap_like, false, k, exit_loss, d_maps, d_active, (int32_t)n_active, d_x0, c->v2_bounds.as<double>(), prm};
    SLAM_V2_DISPATCH(v2_launch_minimize, c, sgt);
    if (rc) return rc;
    return finish_single_stage(c, k, n, n_active, prm, exit_loss, best_loss, best_x, best_restart, item_loss, item_iters, item_status, item_evals);
}

// The span loop of a CircuitTemplateV2 (optimizer.py:233-303) enqueued as ONE chain, like decompose_body: results reset +
// first stage's active list, then per span the V2 optimizer kernel (target count from the device) and the shared epilogue
// kernel (reduction over restarts, merge into the running best -- rows of n_k parameters into rows of nmax --, compaction).
int v2_decompose_body(slam_ctx* c, int64_t first, int64_t count, int k_min, int k_max, const int32_t* gate_seqs, const double* init_lo,
                      const double* init_hi, const double* bound_lo, const double* bound_hi, const slam_opt_params* prm,
                      double success_threshold, FetchReq* fetch) {
    if (!c) return fail(SLAM_ERR_INVALID, "ctx is NULL");
    if (c->cost_kind == SLAM_COST_MAKHLIN)
        return fail(SLAM_ERR_UNSUPPORTED, "parametrised-gate templates do not run MakhlinFunctionalCost (SLAM_COST_MAKHLIN)");
    HIP_TRY(hipSetDevice(c->device));
    if (c->n_targets <= 0) return fail(SLAM_ERR_STATE, "no targets: call slam_set_targets first");
    if (c->v2_gates_host.empty()) return fail(SLAM_ERR_STATE, "no parametrised gates: call slam_v2_set_gates first");
    if (k_min < 1 || k_max < k_min || k_max > SLAM_V2_MAX_SPAN) return fail(SLAM_ERR_UNSUPPORTED, "parametrised-gate templates support spans 1..%d (got [%d, %d])", SLAM_V2_MAX_SPAN, k_min, k_max);
    int rc = check_params(prm);
    if (rc) return rc;
    if (!gate_seqs || !init_lo || !init_hi) return fail(SLAM_ERR_INVALID, "gate_seqs, init_lo and init_hi must be non-NULL");
    if (first < 0 || count <= 0 || first + count > c->n_targets) return fail(SLAM_ERR_INVALID, "target window outside the resident batch");
    const int qn = c->v2_qn;
    const int nmax = 6 * (k_max + 1) + qn * k_max;
    // per span: gate maps and (init_lo | init_hi | bound_lo | bound_hi), staged once
    std::vector<V2GateMap> maps;
    std::vector<double> b;
    std::vector<size_t> map_off, b_off;
    std::vector<bool> bounded_k, riswap_k;
    {
        const int32_t* gs = gate_seqs;
        size_t po = 0;  // offset into the caller's concatenated per-parameter arrays
        for (int k = k_min; k <= k_max; ++k) {
            const int n = 6 * (k + 1) + qn * k;
            map_off.push_back(maps.size());
            bool rl = qn == 1;
            for (int j = 0; j < k; ++j) {
                if (gs[j] < 0 || gs[j] >= (int)c->v2_gates_host.size()) return fail(SLAM_ERR_INVALID, "gate_seqs: index %d outside the parametrised gate table", gs[j]);
                const V2GateMap& gm = c->v2_gates_host[(size_t)gs[j]];
                maps.push_back(gm);
                rl = rl && gm.sel[1] < 0 && gm.sel[2] < 0 && gm.offset[1] == 0.0 && gm.offset[2] == 0.0;
            }
            riswap_k.push_back(rl);
            b_off.push_back(b.size());
            bool bd = false;
            for (int part = 0; part < 4; ++part)
                for (int i = 0; i < n; ++i) {
                    double v;
                    if (part == 0) v = init_lo[po + i];
                    else if (part == 1) v = init_hi[po + i];
                    else if (part == 2) v = bound_lo ? bound_lo[po + i] : -INFINITY;
                    else v = bound_hi ? bound_hi[po + i] : INFINITY;
                    if (part < 2 && !std::isfinite(v)) return fail(SLAM_ERR_INVALID, "start range of parameter %d at span %d must be finite", i, k);
                    if (part >= 2 && std::isfinite(v)) bd = true;
                    b.push_back(v);
                }
            for (int i = 0; i < n; ++i) {
                if (!(init_lo[po + i] <= init_hi[po + i])) return fail(SLAM_ERR_INVALID, "start range of parameter %d at span %d: lo > hi", i, k);
                if (bound_lo && bound_hi && !(bound_lo[po + i] <= bound_hi[po + i])) return fail(SLAM_ERR_INVALID, "bounds of parameter %d at span %d: lo > hi", i, k);
            }
            bounded_k.push_back(bd);
            po += (size_t)n;
            gs += k;
        }
    }
    HIP_TRY(c->v2_maps.reserve(sizeof(V2GateMap) * maps.size()));
    HIP_TRY(c->v2_bounds.reserve(b.size() * sizeof(double)));
    HIP_TRY(hipMemcpyAsync(c->v2_maps.p, maps.data(), sizeof(V2GateMap) * maps.size(), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(c->v2_bounds.p, b.data(), b.size() * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));  // local buffers
    const int64_t N = count, M = N * (int64_t)prm->restarts;
    if (M > 0x7fff0000LL) return fail(SLAM_ERR_INVALID, "too many work items in one stage (%lld)", (long long)M);
    rc = ensure_results_n(c, nmax);
    if (rc) return rc;
    HIP_TRY(c->active.reserve(N * sizeof(int32_t)));
    HIP_TRY(c->active2.reserve(N * sizeof(int32_t)));
    HIP_TRY(c->item_rec.reserve(M * sizeof(ItemRec)));
    HIP_TRY(c->item_x.reserve(M * nmax * sizeof(double)));
    {
        // inverse Hessians of the long templates (v2_h_in_memory: more than 8 parameter slots per lane) live in device memory, one slice
        // per resident wavefront: sized HERE for the longest span of the loop -- growing the buffer between two stages of the chain
        // would free it under the stage in flight (hipFree synchronises the device: ADVICE r3)
        size_t need = 0;
        for (int k = k_min; k <= k_max; ++k) {
            const int na = (6 * (k + 1) + c->v2_qn * k + 3) / 4;
            if (na <= 8) continue;
            int64_t blocks = (M + kQuadsPerWave - 1) / kQuadsPerWave;
            const int64_t cap = (int64_t)kV2HmemWavesPerCu * c->compute_units;  // the launch's own bound (v2_launch_minimize_gq)
            if (blocks > cap) blocks = cap;
            const size_t bytes = (size_t)blocks * (size_t)(na * (na + 1) / 2 * 4 * kWave) * sizeof(float);  // == v2_h_floats_per_wave<K, QN>()
            need = bytes > need ? bytes : need;
        }
        if (need) HIP_TRY(c->v2_hmem.reserve(need));
    }
    HIP_TRY(c->stage_loss.reserve(N * sizeof(double)));
    HIP_TRY(c->stage_x.reserve(N * nmax * sizeof(double)));
    HIP_TRY(c->stage_restart.reserve(N * sizeof(int32_t)));
    HIP_TRY(c->solved.reserve(N * sizeof(int32_t)));
    HIP_TRY(c->stage_targets.reserve((size_t)N * 32 * sizeof(double)));
    HIP_TRY(hipEventRecord(c->ev_t0, c->stream));
    rc = enqueue_init_results(c, c->stream, c->active.as<int32_t>(), first, N, k_min, 0);
    if (rc) return rc;
    DevBuf* cur = &c->active;
    DevBuf* nxt = &c->active2;
    for (int k = k_min, si = 0; k <= k_max; ++k, ++si) {
        const int n = 6 * (k + 1) + qn * k;
        V2Stage sgt{bounded_k[(size_t)si], riswap_k[(size_t)si], true, k, success_threshold, c->v2_maps.as<V2GateMap>() + map_off[(size_t)si],
                    cur->as<int32_t>(), (int32_t)N, nullptr, c->v2_bounds.as<double>() + b_off[(size_t)si], prm};
        SLAM_V2_DISPATCH(v2_launch_minimize, c, sgt);
        if (rc) return rc;
        const SpanLoopStep step{success_threshold, true, k < k_max, success_threshold, nxt->as<int32_t>()};
        ReduceArgs r = build_reduce_args(c, k, n, cur->as<int32_t>(), prm, success_threshold, true);  // (rows of c->result_nmax = nmax)
        r.ordered = 1;  // whatever the flags: the winner is the restart the reference's sequential loop breaks at
        rc = enqueue_stage_epilogue(c, N, build_epilogue_args(c, k, r, step));
        if (rc) return rc;
        DevBuf* t = cur; cur = nxt; nxt = t;
    }
    rc = enqueue_loop_end(c, fetch, nmax, first, count);
    if (rc) return rc;
    rc = wait_loop_end(c, fetch);
    if (rc) return rc;
    return collect_stats(c, k_min, k_max, c->h_ctl, prm->restarts);
}

}  // namespace

extern "C" {

int slam_v2_decompose_range(slam_ctx* ctx, int64_t first, int64_t count, int k_min, int k_max, const int32_t* gate_seqs, const double* init_lo,
                            const double* init_hi, const double* bound_lo, const double* bound_hi, const slam_opt_params* params,
                            double success_threshold, double* best_loss, double* best_x, int32_t* best_cycles) {
    FetchReq fr{best_loss, best_x, best_cycles};
    return drained(ctx, v2_decompose_body(ctx, first, count, k_min, k_max, gate_seqs, init_lo, init_hi, bound_lo, bound_hi, params, success_threshold,
                                          (best_loss || best_x || best_cycles) ? &fr : nullptr));
}

int slam_v2_set_gates(slam_ctx* ctx, const slam_v2_gate* gates, int32_t n_gates) {
    if (!ctx) return fail(SLAM_ERR_INVALID, "ctx is NULL");
    if (!gates || n_gates <= 0 || n_gates > SLAM_MAX_GATES) return fail(SLAM_ERR_INVALID, "n_gates must be in 1..%d", SLAM_MAX_GATES);
    const int qn = gates[0].n_params;
    if (qn != 1 && qn != 2 && qn != 4) return fail(SLAM_ERR_UNSUPPORTED, "parametrised gates take 1, 2 or 4 parameters (got %d)", qn);
    std::vector<V2GateMap> tmp((size_t)n_gates);
    for (int g = 0; g < n_gates; ++g) {
        if (gates[g].n_params != qn) return fail(SLAM_ERR_UNSUPPORTED, "all parametrised gates of a template must take the same number of parameters");
        for (int r = 0; r < 4; ++r) {
            if (gates[g].sel[r] < -1 || gates[g].sel[r] >= qn) return fail(SLAM_ERR_INVALID, "gate %d: sel[%d] = %d outside [-1, %d)", g, r, gates[g].sel[r], qn);
            if (!std::isfinite(gates[g].scale[r]) || !std::isfinite(gates[g].offset[r])) return fail(SLAM_ERR_INVALID, "gate %d: non-finite map", g);
            tmp[(size_t)g].sel[r] = gates[g].sel[r];
            tmp[(size_t)g].scale[r] = gates[g].sel[r] < 0 ? 0.0 : gates[g].scale[r];
            tmp[(size_t)g].offset[r] = gates[g].offset[r];
            tmp[(size_t)g].pad[r] = 0;
        }
    }
    ctx->v2_gates_host.swap(tmp);
    ctx->v2_qn = qn;
    for (int k = 0; k <= SLAM_V2_MAX_SPAN; ++k) ctx->v2_cons_n[k] = 0;  // a constraint belongs to the gate table it was set for
    return SLAM_OK;
}

int slam_v2_set_constraint(slam_ctx* ctx, int k, const double* weights, int n, double cost_max) {
    if (!ctx) return fail(SLAM_ERR_INVALID, "ctx is NULL");
    HIP_TRY(hipSetDevice(ctx->device));
    if (k < 1 || k > SLAM_V2_MAX_SPAN) return fail(SLAM_ERR_UNSUPPORTED, "parametrised-gate templates support spans 1..%d (got %d)", SLAM_V2_MAX_SPAN, k);
    if (!weights || n == 0) {  // remove_constraint (basisv2.py:202-204)
        ctx->v2_cons_n[k] = 0;
        return SLAM_OK;
    }
    if (ctx->v2_gates_host.empty()) return fail(SLAM_ERR_STATE, "no parametrised gates: call slam_v2_set_gates first");
    const int want = 6 * (k + 1) + ctx->v2_qn * k;
    if (n != want) return fail(SLAM_ERR_INVALID, "span %d with %d parameters per gate has %d parameters (got %d weights)", k, ctx->v2_qn, want, n);
    if (!std::isfinite(cost_max)) return fail(SLAM_ERR_INVALID, "cost_max must be finite");
    double w2max = 0.0;
    for (int i = 0; i < n; ++i) {
        if (!std::isfinite(weights[i])) return fail(SLAM_ERR_INVALID, "weights[%d] is not finite", i);
        w2max = std::max(w2max, weights[i] * weights[i]);
    }
    if (!(w2max > 0.0)) return fail(SLAM_ERR_INVALID, "a cost constraint needs a non-zero weight");
    HIP_TRY(ctx->v2_cons_w[k].reserve((size_t)n * sizeof(double)));
    HIP_TRY(hipMemcpyAsync(ctx->v2_cons_w[k].p, weights, (size_t)n * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));  // the caller's buffer
    ctx->v2_cons_n[k] = n;
    ctx->v2_cons_max[k] = cost_max;
    ctx->v2_cons_rho[k] = 30.0 / w2max;
    return SLAM_OK;
}

int slam_v2_eval_loss_grad(slam_ctx* ctx, int k, const int32_t* gate_seq, const double* x, const int32_t* target_of, int64_t M,
                           double* loss, double* grad, double* unitary) {
    return drained(ctx, v2_eval_body(ctx, k, gate_seq, x, target_of, M, loss, grad, unitary));
}

int slam_v2_minimize_stage(slam_ctx* ctx, int k, const int32_t* gate_seq, const int32_t* active, int64_t n_active, const double* x0,
                           const double* init_lo, const double* init_hi, const double* bound_lo, const double* bound_hi,
                           const slam_opt_params* params, double exit_loss, double* best_loss, double* best_x, int32_t* best_restart,
                           double* item_loss, int32_t* item_iters, int32_t* item_status, int32_t* item_evals) {
    return drained(ctx, v2_minimize_body(ctx, k, gate_seq, active, n_active, x0, init_lo, init_hi, bound_lo, bound_hi, params, exit_loss,
                                         best_loss, best_x, best_restart, item_loss, item_iters, item_status, item_evals));
}

int slam_v2_minimize_stage_trace(slam_ctx* ctx, int k, const int32_t* gate_seq, const int32_t* active, int64_t n_active, const double* x0,
                                 const double* init_lo, const double* init_hi, const double* bound_lo, const double* bound_hi,
                                 const slam_opt_params* params, double exit_loss, int32_t trace_cap, double* best_loss, double* best_x,
                                 int32_t* best_restart, double* item_loss, int32_t* item_iters, int32_t* item_status, double* trace_loss,
                                 double* trace_x) {
    return minimize_stage_trace(
        ctx, active, n_active, params, trace_cap, trace_loss, trace_x,
        [&](int* n) {
            if (k < 1 || k > SLAM_V2_MAX_SPAN) return fail(SLAM_ERR_UNSUPPORTED, "parametrised-gate templates support spans 1..%d (got %d)", SLAM_V2_MAX_SPAN, k);
            *n = 6 * (k + 1) + ctx->v2_qn * k;
            return (int)SLAM_OK;
        },
        [&] {
            return slam_v2_minimize_stage(ctx, k, gate_seq, active, n_active, x0, init_lo, init_hi, bound_lo, bound_hi, params, exit_loss, best_loss, best_x,
                                          best_restart, item_loss, item_iters, item_status, nullptr);
        });
}

}  // extern "C"
