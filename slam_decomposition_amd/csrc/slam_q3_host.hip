// slam_q3_host.hip -- host side of the three-qubit templates (slam_q3.hpp): slam_q3_eval, slam_q3_minimize.  Both are self-contained:
// gates, targets and parameters come from the host with every call, the context lends its device and its stream, and its resident 4x4
// targets, gate table, results and statistics are not touched.
#include "slam_host.hpp"
#include "slam_q3.hpp"

namespace {

// The template description shared by both entry points, checked before anything touches the device.  *edge_bits: the packed edges.
int check_template(const double* gates, int32_t n_gates, int32_t k, const int32_t* gate_index, const int32_t* edges, uint64_t* edge_bits) {
    if (k < 1 || k > SLAM_Q3_MAX_SPAN) return fail(SLAM_ERR_UNSUPPORTED, "three-qubit templates take 1..%d gates (got %d)", SLAM_Q3_MAX_SPAN, k);
    if (!gates) return fail(SLAM_ERR_INVALID, "gates is NULL");
    if (n_gates < 1 || n_gates > SLAM_MAX_GATES) return fail(SLAM_ERR_INVALID, "n_gates must be in 1..%d (got %d)", SLAM_MAX_GATES, n_gates);
    if (!gate_index) return fail(SLAM_ERR_INVALID, "gate_index is NULL");
    if (!edges) return fail(SLAM_ERR_INVALID, "edges is NULL");
    uint64_t bits = 0;
    for (int j = 0; j < k; ++j) {
        if (gate_index[j] < 0 || gate_index[j] >= n_gates)
            return fail(SLAM_ERR_INVALID, "gate_index[%d] = %d outside the gate table (n_gates = %d)", j, gate_index[j], n_gates);
        const int a = edges[2 * j], b = edges[2 * j + 1];
        if (a < 0 || a > 2 || b < 0 || b > 2 || a == b)
            return fail(SLAM_ERR_INVALID, "edges[%d] = (%d, %d): an edge is an ordered pair of distinct qubits from {0, 1, 2}", j, a, b);
        bits |= (uint64_t)(a | (b << 2)) << (4 * j);
    }
    for (int64_t i = 0; i < (int64_t)n_gates * 32; ++i)
        if (!std::isfinite(gates[i])) return fail(SLAM_ERR_INVALID, "gates: entry %lld is not finite", (long long)i);
    *edge_bits = bits;
    return SLAM_OK;
}

int check_cost(int32_t cost_kind) {
    if (cost_kind == SLAM_COST_MAKHLIN) return fail(SLAM_ERR_UNSUPPORTED, "MakhlinFunctionalCost: Weyl chamber only for 2Q gates");
    if (cost_kind != SLAM_COST_BASIC && cost_kind != SLAM_COST_SQUARE) return fail(SLAM_ERR_INVALID, "unknown cost kind %d", cost_kind);
    return SLAM_OK;
}

// the gate of every position, in order: [k][4][4][2] on the device
int stage_q3_gates(slam_ctx* c, DevBuf& d, const double* gates, int32_t k, const int32_t* gate_index) {
    std::vector<double> h((size_t)k * 32);
    for (int j = 0; j < k; ++j) std::memcpy(h.data() + 32 * j, gates + (size_t)gate_index[j] * 32, 32 * sizeof(double));
    HIP_TRY(d.reserve(h.size() * sizeof(double)));
    HIP_TRY(hipMemcpyAsync(d.p, h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));  // (h leaves scope)
    return SLAM_OK;
}

int upload(slam_ctx* c, DevBuf& d, const void* src, size_t bytes) {
    HIP_TRY(d.reserve(bytes));
    HIP_TRY(hipMemcpyAsync(d.p, src, bytes, hipMemcpyHostToDevice, c->stream));
    return SLAM_OK;
}

int q3_eval(slam_ctx* c, const double* gates, int32_t k, const int32_t* gate_index, uint64_t edge_bits, const double* targets, int64_t n_targets,
            const double* x, const int32_t* target_of, int64_t M, int32_t cost_kind, double* loss, double* grad, double* unitary) {
    const int n = 9 + 6 * k;
    HIP_TRY(hipSetDevice(c->device));
    { int rc = kernel_per_cu(c, reinterpret_cast<const void*>(&eval_q3_kernel), kQ3LdsBytes, nullptr); if (rc) return rc; }
    DevBuf d_gates, d_targets, d_x, d_tof, d_loss, d_grad, d_unitary;
    { int rc = stage_q3_gates(c, d_gates, gates, k, gate_index); if (rc) return rc; }
    { int rc = upload(c, d_targets, targets, (size_t)n_targets * 128 * sizeof(double)); if (rc) return rc; }
    { int rc = upload(c, d_x, x, (size_t)M * n * sizeof(double)); if (rc) return rc; }
    { int rc = upload(c, d_tof, target_of, (size_t)M * sizeof(int32_t)); if (rc) return rc; }
    HIP_TRY(d_loss.reserve((size_t)M * sizeof(double)));
    if (grad) HIP_TRY(d_grad.reserve((size_t)M * n * sizeof(double)));
    if (unitary) HIP_TRY(d_unitary.reserve((size_t)M * 128 * sizeof(double)));
    Q3EvalArgs a{};
    a.targets = d_targets.as<double>();
    a.x = d_x.as<double>();
    a.target_of = d_tof.as<int32_t>();
    a.n_items = M;
    a.loss = d_loss.as<double>();
    a.grad = grad ? d_grad.as<double>() : nullptr;
    a.unitary = unitary ? d_unitary.as<double>() : nullptr;
    a.cost_kind = cost_kind;
    a.gates = d_gates.as<double>();
    a.edges = edge_bits;
    a.k = k;
    int64_t blocks = M;
    const int64_t cap = (int64_t)16 * c->compute_units;
    if (blocks > cap) blocks = cap;
    hipLaunchKernelGGL(eval_q3_kernel, dim3((unsigned)blocks), dim3(kWave), kQ3LdsBytes, c->stream, a);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(loss, d_loss.p, (size_t)M * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (grad) HIP_TRY(hipMemcpyAsync(grad, d_grad.p, (size_t)M * n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (unitary) HIP_TRY(hipMemcpyAsync(unitary, d_unitary.p, (size_t)M * 128 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return SLAM_OK;
}

int q3_minimize(slam_ctx* c, const double* gates, int32_t k, const int32_t* gate_index, uint64_t edge_bits, const double* targets, int64_t N,
                int32_t cost_kind, const slam_opt_params* prm, double exit_loss, const double* x0, double* best_loss, double* best_x,
                int32_t* best_restart, double* item_loss, int32_t* item_iters, int32_t* item_status, int32_t* item_evals, double* item_x,
                double* kernel_ms) {
    const int n = 9 + 6 * k;
    const int R = prm->restarts;
    const int64_t M = N * (int64_t)R;
    HIP_TRY(hipSetDevice(c->device));
    int per_cu = 0;
    { int rc = kernel_per_cu(c, reinterpret_cast<const void*>(&minimize_q3_kernel), kQ3LdsBytes, &per_cu); if (rc) return rc; }
    int64_t blocks = (int64_t)per_cu * c->compute_units;  // persistent wavefronts, one item each at a time
    if (blocks > M) blocks = M;
    if (blocks < 1) blocks = 1;
    DevBuf d_gates, d_targets, d_x0, d_ctl, d_solved, d_rec, d_x, d_hmem;
    { int rc = stage_q3_gates(c, d_gates, gates, k, gate_index); if (rc) return rc; }
    { int rc = upload(c, d_targets, targets, (size_t)N * 128 * sizeof(double)); if (rc) return rc; }
    if (x0) { int rc = upload(c, d_x0, x0, (size_t)M * n * sizeof(double)); if (rc) return rc; }
    StageCtl h_ctl{};
    h_ctl.n_active = (int32_t)N;
    { int rc = upload(c, d_ctl, &h_ctl, sizeof(StageCtl)); if (rc) return rc; }
    HIP_TRY(d_solved.reserve((size_t)N * sizeof(int32_t)));
    HIP_TRY(hipMemsetAsync(d_solved.p, 0, (size_t)N * sizeof(int32_t), c->stream));
    HIP_TRY(d_rec.reserve((size_t)M * sizeof(ItemRec)));
    HIP_TRY(d_x.reserve((size_t)M * n * sizeof(double)));
    HIP_TRY(d_hmem.reserve((size_t)blocks * (size_t)n * kQ3HStride * sizeof(float)));
    Q3Args a{};
    a.targets = d_targets.as<double>();
    a.x0 = x0 ? d_x0.as<double>() : nullptr;
    a.ctl = d_ctl.as<StageCtl>();
    a.restarts = R;
    a.maxiter = prm->maxiter;
    a.gtol = prm->gtol;
    a.stop_loss = prm->stop_loss;
    a.gtol_far = prm->gtol_far;
    a.far_loss = prm->far_loss;
    a.exit_loss = exit_loss;
    a.seed = prm->seed;
    a.target_base = prm->target_base;
    a.flags = prm->flags & (SLAM_FLAG_EARLY_EXIT | SLAM_FLAG_ORDERED);
    a.cost_kind = cost_kind;
    a.solved = d_solved.as<int32_t>();
    a.item_rec = d_rec.as<ItemRec>();
    a.item_x = d_x.as<double>();
    a.gates = d_gates.as<double>();
    a.edges = edge_bits;
    a.k = k;
    a.hmem = d_hmem.as<float>();
    Event e0, e1;
    HIP_TRY(hipEventCreate(&e0.h));
    HIP_TRY(hipEventCreate(&e1.h));
    HIP_TRY(hipEventRecord(e0, c->stream));
    hipLaunchKernelGGL(minimize_q3_kernel, dim3((unsigned)blocks), dim3(kWave), kQ3LdsBytes, c->stream, a);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(e1, c->stream));
    std::vector<ItemRec> rec((size_t)M);
    std::vector<double> xs((size_t)M * n);
    HIP_TRY(hipMemcpyAsync(rec.data(), d_rec.p, (size_t)M * sizeof(ItemRec), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(xs.data(), d_x.p, (size_t)M * n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (kernel_ms) {
        float ms = 0.0f;
        HIP_TRY(hipEventElapsedTime(&ms, e0, e1));
        *kernel_ms = ms;
    }
    // per target the reduction over its restarts: ordered -- the lowest-index restart below exit_loss; otherwise, and when none is,
    // the smallest loss (ties: the lowest index)
    const bool ordered = (prm->flags & SLAM_FLAG_ORDERED) != 0;
    for (int64_t t = 0; t < N; ++t) {
        int win = -1;
        if (ordered)
            for (int r = 0; r < R && win < 0; ++r)
                if (rec[t * R + r].loss < exit_loss) win = r;
        if (win < 0) {
            win = 0;
            for (int r = 1; r < R; ++r)
                if (rec[t * R + r].loss < rec[t * R + win].loss) win = r;
        }
        if (best_loss) best_loss[t] = rec[t * R + win].loss;
        if (best_restart) best_restart[t] = win;
        if (best_x) std::memcpy(best_x + t * n, xs.data() + (t * R + win) * n, (size_t)n * sizeof(double));
    }
    for (int64_t m = 0; m < M; ++m) {
        if (item_loss) item_loss[m] = rec[m].loss;
        if (item_iters) item_iters[m] = rec[m].iters;
        if (item_status) item_status[m] = rec[m].status;
        if (item_evals) item_evals[m] = rec[m].evals;
    }
    if (item_x) std::memcpy(item_x, xs.data(), xs.size() * sizeof(double));
    return SLAM_OK;
}

}  // namespace

extern "C" {

int slam_q3_eval(slam_ctx* ctx, const double* gates, int32_t n_gates, int32_t k, const int32_t* gate_index, const int32_t* edges,
                 const double* targets, int64_t n_targets, const double* x, const int32_t* target_of, int64_t M, int32_t cost_kind,
                 double* loss, double* grad, double* unitary) {
    uint64_t edge_bits = 0;
    { int rc = check_template(gates, n_gates, k, gate_index, edges, &edge_bits); if (rc) return rc; }
    { int rc = check_cost(cost_kind); if (rc) return rc; }
    if (!targets || n_targets <= 0) return fail(SLAM_ERR_INVALID, "targets: at least one 8x8 target is required");
    if (!x || !target_of || !loss) return fail(SLAM_ERR_INVALID, "x, target_of and loss are required");
    if (M <= 0 || M > 0x7fff0000LL) return fail(SLAM_ERR_INVALID, "M must be in 1..%lld (got %lld)", 0x7fff0000LL, (long long)M);
    for (int64_t m = 0; m < M; ++m)
        if (target_of[m] < 0 || target_of[m] >= n_targets)
            return fail(SLAM_ERR_INVALID, "target_of[%lld] = %d outside the targets (n_targets = %lld)", (long long)m, target_of[m], (long long)n_targets);
    if (!ctx) return fail(SLAM_ERR_INVALID, "ctx is NULL");
    return drained(ctx, q3_eval(ctx, gates, k, gate_index, edge_bits, targets, n_targets, x, target_of, M, cost_kind, loss, grad, unitary));
}

int slam_q3_minimize(slam_ctx* ctx, const double* gates, int32_t n_gates, int32_t k, const int32_t* gate_index, const int32_t* edges,
                     const double* targets, int64_t n_targets, int32_t cost_kind, const slam_opt_params* params, double exit_loss,
                     const double* x0, double* best_loss, double* best_x, int32_t* best_restart, double* item_loss, int32_t* item_iters,
                     int32_t* item_status, int32_t* item_evals, double* item_x, double* kernel_ms) {
    uint64_t edge_bits = 0;
    { int rc = check_template(gates, n_gates, k, gate_index, edges, &edge_bits); if (rc) return rc; }
    { int rc = check_cost(cost_kind); if (rc) return rc; }
    { int rc = check_params(params); if (rc) return rc; }
    if (!targets || n_targets <= 0) return fail(SLAM_ERR_INVALID, "targets: at least one 8x8 target is required");
    if (n_targets * (int64_t)params->restarts > 0x7fff0000LL)
        return fail(SLAM_ERR_INVALID, "too many work items in one stage (%lld)", (long long)(n_targets * (int64_t)params->restarts));
    if (!(exit_loss == exit_loss)) return fail(SLAM_ERR_INVALID, "exit_loss is NaN");
    if (!ctx) return fail(SLAM_ERR_INVALID, "ctx is NULL");
    return drained(ctx, q3_minimize(ctx, gates, k, gate_index, edge_bits, targets, n_targets, cost_kind, params, exit_loss, x0, best_loss, best_x,
                                    best_restart, item_loss, item_iters, item_status, item_evals, item_x, kernel_ms));
}

}  // extern "C"
