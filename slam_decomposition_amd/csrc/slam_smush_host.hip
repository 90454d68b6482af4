// slam_smush_host.hip -- host side of libslamhip.so, parallel-drive unit: slam_smush_* (CircuitTemplateV2(param_vec_expand=...),
// ConversionGainSmushGate) on the kernels of slam_smush.hpp.  The reduction over restarts is enqueued through slam_hip.hip (slam_host.hpp).
#include "slam_host.hpp"
#include "slam_smush.hpp"

static_assert(sizeof(SmushMap) == sizeof(slam_smush_gate), "SmushMap mirrors slam_smush_gate");
static_assert(kSmushMaxSlices == SLAM_SMUSH_MAX_SLICES && kSmushMaxSpan == SLAM_SMUSH_MAX_SPAN && kSmushNP == SLAM_SMUSH_MAX_N, "smush limits");
namespace {

int smush_check(slam_ctx* c, int k) {
    if (!c) return fail(SLAM_ERR_INVALID, "ctx is NULL");
    if (c->cost_kind == SLAM_COST_MAKHLIN)
        return fail(SLAM_ERR_UNSUPPORTED, "smush-gate templates do not run MakhlinFunctionalCost (SLAM_COST_MAKHLIN)");
    if (c->smush_gates_host.empty()) return fail(SLAM_ERR_STATE, "no smush gates: call slam_smush_set_gates first");
    if (k < 1 || k > SLAM_SMUSH_MAX_SPAN) return fail(SLAM_ERR_UNSUPPORTED, "smush-gate templates support spans 1..%d (got %d)", SLAM_SMUSH_MAX_SPAN, k);
    const int n = 6 * (k + 1) + c->smush_qn * k;
    if (n > SLAM_SMUSH_MAX_N)
        return fail(SLAM_ERR_UNSUPPORTED, "span %d with %d parameters per gate has %d parameters: at most %d", k, c->smush_qn, n, SLAM_SMUSH_MAX_N);
    return SLAM_OK;
}

int smush_stage_maps(slam_ctx* c, int k, const int32_t* gate_seq, const SmushMap** d_out) {
    if (!gate_seq) return fail(SLAM_ERR_INVALID, "gate_seq is NULL");
    std::vector<SmushMap> tmp((size_t)k);
    for (int j = 0; j < k; ++j) {
        if (gate_seq[j] < 0 || gate_seq[j] >= (int)c->smush_gates_host.size())
            return fail(SLAM_ERR_INVALID, "gate_seq[%d] = %d outside the smush gate table (%d gates)", j, gate_seq[j], (int)c->smush_gates_host.size());
        tmp[(size_t)j] = c->smush_gates_host[(size_t)gate_seq[j]];
    }
    HIP_TRY(c->smush_maps.reserve(sizeof(SmushMap) * SLAM_SMUSH_MAX_SPAN));
    HIP_TRY(hipMemcpyAsync(c->smush_maps.p, tmp.data(), sizeof(SmushMap) * (size_t)k, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));  // tmp is a local buffer
    *d_out = c->smush_maps.as<SmushMap>();
    return SLAM_OK;
}

int smush_eval_body(slam_ctx* c, int k, const int32_t* gate_seq, const double* x, const int32_t* target_of, int64_t M, double* loss,
                    double* grad, double* unitary) {
    int rc = smush_check(c, k);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(c->device));
    if (c->n_targets <= 0) return fail(SLAM_ERR_STATE, "no targets: call slam_set_targets first");
    if (M < 0) return fail(SLAM_ERR_INVALID, "M < 0");
    if (M == 0) return SLAM_OK;
    if (!x || !target_of || !loss) return fail(SLAM_ERR_INVALID, "x, target_of and loss must be non-NULL");
    const SmushMap* d_maps = nullptr;
    rc = smush_stage_maps(c, k, gate_seq, &d_maps);
    if (rc) return rc;
    const int n = 6 * (k + 1) + c->smush_qn * k;
    EvalBufs d{};
    rc = stage_eval_inputs(c, x, target_of, M, n, grad != nullptr, unitary != nullptr, &d);
    if (rc) return rc;
    SmushEvalArgs a{};
    a.targets = c->targets.as<double>();
    a.x = d.x;
    a.target_of = d.target_of;
    a.n_items = M;
    a.loss = d.loss;
    a.grad = d.grad;
    a.unitary = d.unitary;
    a.cost_kind = c->cost_kind;
    a.maps = d_maps;
    a.k = k;
    a.qn = c->smush_qn;
    { rc = kernel_per_cu(c, reinterpret_cast<const void*>(&eval_smush_kernel), kSmLdsBytes, nullptr); if (rc) return rc; }
    const int64_t blocks = std::min<int64_t>(M, (int64_t)std::max(1, c->compute_units) * 16);
    hipLaunchKernelGGL(eval_smush_kernel, dim3((unsigned)blocks), dim3(kWave), kSmLdsBytes, c->stream, a);
    HIP_TRY(hipGetLastError());
    rc = enqueue_eval_readback(c, M, n, loss, grad, unitary);
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(c->stream));
    return SLAM_OK;
}

int smush_minimize_body(slam_ctx* c, int k, const int32_t* gate_seq, const int32_t* active, int64_t n_active, const double* x0,
                        const double* init_lo, const double* init_hi, const double* bound_lo, const double* bound_hi,
                        const slam_opt_params* prm, double exit_loss, double* best_loss, double* best_x, int32_t* best_restart,
                        double* item_loss, int32_t* item_iters, int32_t* item_status, int32_t* item_evals) {
    int rc = smush_check(c, k);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(c->device));
    if (c->n_targets <= 0) return fail(SLAM_ERR_STATE, "no targets: call slam_set_targets first");
    rc = check_params(prm);
    if (rc) return rc;
    if (!active) n_active = c->n_targets;
    if (n_active <= 0) return n_active == 0 ? SLAM_OK : fail(SLAM_ERR_INVALID, "n_active < 0");
    if (!best_loss || !best_x) return fail(SLAM_ERR_INVALID, "best_loss and best_x must be non-NULL");
    if (!init_lo || !init_hi) return fail(SLAM_ERR_INVALID, "init_lo and init_hi must be non-NULL");
    const int n = 6 * (k + 1) + c->smush_qn * k;
    const int64_t M = n_active * (int64_t)prm->restarts;
    const SmushMap* d_maps = nullptr;
    rc = smush_stage_maps(c, k, gate_seq, &d_maps);
    if (rc) return rc;
    const int32_t* d_active = nullptr;
    const double* d_x0 = nullptr;
    bool bounded = false;
    rc = stage_family_inputs(c, k, n, active, n_active, x0, init_lo, init_hi, bound_lo, bound_hi, prm, &d_active, &d_x0, &bounded);
    if (rc) return rc;
    int per_cu = 0;
    { rc = kernel_per_cu(c, reinterpret_cast<const void*>(&minimize_smush_kernel), kSmLdsBytes, &per_cu); if (rc) return rc; }
    const int64_t resident = (int64_t)per_cu * std::max(1, c->compute_units);
    int64_t blocks = std::min<int64_t>(M, resident);
    if (blocks < 1) blocks = 1;
    HIP_TRY(c->smush_hmem.reserve((size_t)resident * (size_t)SLAM_SMUSH_MAX_N * kSmushNP * sizeof(float)));
    SmushArgs a{};
    fill_stage_common(a, c, prm, exit_loss);
    a.targets = c->targets.as<double>();
    a.active = d_active;
    a.n_active = (int32_t)n_active;
    a.x0 = d_x0;
    a.init_lo = c->v2_bounds.as<double>();
    a.init_hi = a.init_lo + n;
    a.bound_lo = a.init_lo + 2 * n;
    a.bound_hi = a.init_lo + 3 * n;
    a.maps = d_maps;
    a.k = k;
    a.qn = c->smush_qn;
    a.bounded = bounded ? 1 : 0;
    a.ctl = stage_ctl(c, k);
    a.hmem = c->smush_hmem.as<float>();
    HIP_TRY(hipEventRecord(c->ev_a[k], c->stream));
    hipLaunchKernelGGL(minimize_smush_kernel, dim3((unsigned)blocks), dim3(kWave), kSmLdsBytes, c->stream, a);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(c->ev_b[k], c->stream));
    return finish_single_stage(c, k, n, n_active, prm, exit_loss, best_loss, best_x, best_restart, item_loss, item_iters, item_status, item_evals);
}

}  // namespace

extern "C" {

int slam_smush_set_gates(slam_ctx* ctx, const slam_smush_gate* gates, int32_t n_gates) {
    if (!ctx) return fail(SLAM_ERR_INVALID, "ctx is NULL");
    if (!gates || n_gates <= 0 || n_gates > SLAM_MAX_GATES) return fail(SLAM_ERR_INVALID, "n_gates must be in 1..%d", SLAM_MAX_GATES);
    const int qn = gates[0].n_params;
    if (qn < 1 || qn > SLAM_SMUSH_MAX_N - 12) return fail(SLAM_ERR_UNSUPPORTED, "smush gates take 1..%d parameters (got %d)", SLAM_SMUSH_MAX_N - 12, qn);
    std::vector<SmushMap> tmp((size_t)n_gates);
    for (int g = 0; g < n_gates; ++g) {
        const slam_smush_gate& s = gates[g];
        if (s.n_params != qn) return fail(SLAM_ERR_UNSUPPORTED, "all smush gates of a template must take the same number of parameters");
        if (s.n_slices < 1 || s.n_slices > SLAM_SMUSH_MAX_SLICES)
            return fail(SLAM_ERR_UNSUPPORTED, "gate %d: %d time slices, 1..%d are supported", g, s.n_slices, SLAM_SMUSH_MAX_SLICES);
        if (!std::isfinite(s.t)) return fail(SLAM_ERR_INVALID, "gate %d: pulse time is not finite", g);
        SmushMap& m = tmp[(size_t)g];
        std::memset(&m, 0, sizeof(m));
        m.qn = qn;
        m.n_slices = s.n_slices;
        m.t = s.t;
        const int nraw = 2 + 2 * s.n_slices;
        for (int r = 0; r < SLAM_SMUSH_RAW; ++r) {
            const bool used = r < nraw;
            if (used && (s.sel[r] < -1 || s.sel[r] >= qn)) return fail(SLAM_ERR_INVALID, "gate %d: sel[%d] = %d outside [-1, %d)", g, r, s.sel[r], qn);
            if (used && (!std::isfinite(s.scale[r]) || !std::isfinite(s.offset[r]))) return fail(SLAM_ERR_INVALID, "gate %d: non-finite map", g);
            m.sel[r] = used ? s.sel[r] : -1;
            m.scale[r] = (used && s.sel[r] >= 0) ? s.scale[r] : 0.0;
            m.offset[r] = used ? s.offset[r] : 0.0;
        }
    }
    ctx->smush_gates_host.swap(tmp);
    ctx->smush_qn = qn;
    return SLAM_OK;
}

int slam_smush_eval_loss_grad(slam_ctx* ctx, int k, const int32_t* gate_seq, const double* x, const int32_t* target_of, int64_t M,
                              double* loss, double* grad, double* unitary) {
    return drained(ctx, smush_eval_body(ctx, k, gate_seq, x, target_of, M, loss, grad, unitary));
}

int slam_smush_minimize_stage(slam_ctx* ctx, int k, const int32_t* gate_seq, const int32_t* active, int64_t n_active, const double* x0,
                              const double* init_lo, const double* init_hi, const double* bound_lo, const double* bound_hi,
                              const slam_opt_params* params, double exit_loss, double* best_loss, double* best_x, int32_t* best_restart,
                              double* item_loss, int32_t* item_iters, int32_t* item_status, int32_t* item_evals) {
    return drained(ctx, smush_minimize_body(ctx, k, gate_seq, active, n_active, x0, init_lo, init_hi, bound_lo, bound_hi, params, exit_loss,
                                            best_loss, best_x, best_restart, item_loss, item_iters, item_status, item_evals));
}

int slam_smush_minimize_stage_trace(slam_ctx* ctx, int k, const int32_t* gate_seq, const int32_t* active, int64_t n_active, const double* x0,
                                    const double* init_lo, const double* init_hi, const double* bound_lo, const double* bound_hi,
                                    const slam_opt_params* params, double exit_loss, int32_t trace_cap, double* best_loss, double* best_x,
                                    int32_t* best_restart, double* item_loss, int32_t* item_iters, int32_t* item_status, double* trace_loss,
                                    double* trace_x) {
    return minimize_stage_trace(
        ctx, active, n_active, params, trace_cap, trace_loss, trace_x,
        [&](int* n) {
            const int rc = smush_check(ctx, k);
            if (rc) return rc;
            *n = 6 * (k + 1) + ctx->smush_qn * k;
            return (int)SLAM_OK;
        },
        [&] {
            return slam_smush_minimize_stage(ctx, k, gate_seq, active, n_active, x0, init_lo, init_hi, bound_lo, bound_hi, params, exit_loss, best_loss,
                                             best_x, best_restart, item_loss, item_iters, item_status, nullptr);
        });
}

}  // extern "C"
