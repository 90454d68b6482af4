// slam_q3_host.hip -- host side of the three-qubit templates (slam_q3.hpp): slam_q3_eval, slam_q3_minimize and their mixed-arity
// siblings slam_q3m_eval, slam_q3m_minimize, and the state objectives slam_q3s_eval, slam_q3s_minimize (mutual information of a start
// state carried through the template: the STATE instantiations of the same kernels).  All are self-contained: gates, targets and parameters come from the host with every
// call, the context lends its device and its stream, and its resident 4x4 targets, gate table, results and statistics are not touched.
// A checked template is a Q3Plan; the mixed kernels run only for a plan with a three-qubit position.
#include "slam_host.hpp"
#include "slam_q3.hpp"

namespace {

static_assert(SLAM_Q3_MAX_GATES3 == kQ3MaxGates3 && SLAM_Q3_MAX_GATES3 >= 2 && SLAM_Q3_MAX_GATES3 <= 4, "the gate index of a position has two bits");
static_assert(SLAM_Q3_MAX_SPAN == kQ3MaxSpan, "header and kernel disagree");

// The template description shared by both entry points, checked before anything touches the device.  *edge_bits: the packed edges.
struct Q3Plan {
    int k = 0, n = 0;
    bool mixed = false;           // a position has arity 3
    bool state = false;           // slam_q3s_*: the items are 8-vectors (start states), not 8x8 targets
    uint64_t edge_bits = 0;       // Q3Args::edges
    uint64_t ext_bits = 0;        // Q3MArgs::ext
    std::vector<double> gates2;   // [k][4][4][2]: the 4x4 of every position (zeros at a three-qubit position)
    const double* gates3 = nullptr;
    int n_gates3 = 0;
};

void fill_plan(Q3Plan& p, const double* gates, int32_t k, const int32_t* gate_index, uint64_t edge_bits) {
    p.k = k;
    p.n = 9 + 6 * k;
    p.edge_bits = edge_bits;
    p.gates2.resize((size_t)k * 32);
    for (int j = 0; j < k; ++j) std::memcpy(p.gates2.data() + 32 * j, gates + (size_t)gate_index[j] * 32, 32 * sizeof(double));
}

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

// The mixed description: per position an arity, an index into the table of that arity and three qubits (the third ignored at arity 2).
int check_mixed(const double* gates2, int32_t n_gates2, const double* gates3, int32_t n_gates3, int32_t k, const int32_t* arity,
                const int32_t* gate_index, const int32_t* qubits, Q3Plan* plan) {
    if (k < 1 || k > SLAM_Q3_MAX_SPAN) return fail(SLAM_ERR_UNSUPPORTED, "three-qubit templates take 1..%d gates (got %d)", SLAM_Q3_MAX_SPAN, k);
    if (n_gates2 < 0 || n_gates2 > SLAM_MAX_GATES) return fail(SLAM_ERR_INVALID, "n_gates2 must be in 0..%d (got %d)", SLAM_MAX_GATES, n_gates2);
    if (n_gates3 < 0) return fail(SLAM_ERR_INVALID, "n_gates3 is negative (%d)", n_gates3);
    if (n_gates3 > SLAM_Q3_MAX_GATES3)
        return fail(SLAM_ERR_UNSUPPORTED, "a template takes at most %d distinct three-qubit gates (got %d)", SLAM_Q3_MAX_GATES3, n_gates3);
    if (n_gates2 > 0 && !gates2) return fail(SLAM_ERR_INVALID, "gates2 is NULL");
    if (n_gates3 > 0 && !gates3) return fail(SLAM_ERR_INVALID, "gates3 is NULL");
    if (!arity) return fail(SLAM_ERR_INVALID, "arity is NULL");
    if (!gate_index) return fail(SLAM_ERR_INVALID, "gate_index is NULL");
    if (!qubits) return fail(SLAM_ERR_INVALID, "qubits is NULL");
    uint64_t bits = 0, ext = 0;
    int n = 9;
    bool mixed = false;
    for (int j = 0; j < k; ++j) {
        if (arity[j] != 2 && arity[j] != 3) return fail(SLAM_ERR_INVALID, "arity[%d] = %d: a position holds a two- or a three-qubit gate", j, arity[j]);
        const bool three = arity[j] == 3;
        const int n_tab = three ? n_gates3 : n_gates2;
        if (gate_index[j] < 0 || gate_index[j] >= n_tab)
            return fail(SLAM_ERR_INVALID, "gate_index[%d] = %d outside the table of %d-qubit gates (%d entries)", j, gate_index[j], arity[j], n_tab);
        const int a = qubits[3 * j], b = qubits[3 * j + 1], c = three ? qubits[3 * j + 2] : 3;
        if (a < 0 || a > 2 || b < 0 || b > 2 || a == b || (three && (c < 0 || c > 2 || c == a || c == b)))
            return fail(SLAM_ERR_INVALID, "qubits[%d] = (%d, %d, %d): arity %d takes that many distinct qubits from {0, 1, 2}, in order", j,
                        qubits[3 * j], qubits[3 * j + 1], qubits[3 * j + 2], arity[j]);
        bits |= (uint64_t)(a | (b << 2)) << (4 * j);
        ext |= (uint64_t)(c | ((three ? gate_index[j] : 0) << 2)) << (4 * j);
        n += 3 * arity[j];
        mixed = mixed || three;
    }
    if (n > kQ3N) return fail(SLAM_ERR_UNSUPPORTED, "three-qubit templates take at most %d parameters (got 9 + 3 * the arities = %d)", kQ3N, n);
    for (int64_t i = 0; i < (int64_t)n_gates2 * 32; ++i)
        if (!std::isfinite(gates2[i])) return fail(SLAM_ERR_INVALID, "gates2: entry %lld is not finite", (long long)i);
    for (int64_t i = 0; i < (int64_t)n_gates3 * 128; ++i)
        if (!std::isfinite(gates3[i])) return fail(SLAM_ERR_INVALID, "gates3: entry %lld is not finite", (long long)i);
    plan->k = k;
    plan->n = n;
    plan->mixed = mixed;
    plan->edge_bits = bits;
    plan->ext_bits = ext;
    plan->gates2.assign((size_t)k * 32, 0.0);
    for (int j = 0; j < k; ++j)
        if (arity[j] == 2) std::memcpy(plan->gates2.data() + 32 * j, gates2 + (size_t)gate_index[j] * 32, 32 * sizeof(double));
    plan->gates3 = gates3;
    plan->n_gates3 = n_gates3;
    return SLAM_OK;
}

int check_cost(int32_t cost_kind) {
    if (cost_kind == SLAM_COST_MAKHLIN) return fail(SLAM_ERR_UNSUPPORTED, "MakhlinFunctionalCost: Weyl chamber only for 2Q gates");
    if (cost_kind != SLAM_COST_BASIC && cost_kind != SLAM_COST_SQUARE) return fail(SLAM_ERR_INVALID, "unknown cost kind %d", cost_kind);
    return SLAM_OK;
}

int check_state_cost(int32_t cost_kind) {
    if (cost_kind != SLAM_COST_MUTUAL_INFO && cost_kind != SLAM_COST_MUTUAL_INFO_SQUARE)
        return fail(SLAM_ERR_INVALID, "cost kind %d: the state objectives are SLAM_COST_MUTUAL_INFO (%d) and SLAM_COST_MUTUAL_INFO_SQUARE (%d)", cost_kind,
                    SLAM_COST_MUTUAL_INFO, SLAM_COST_MUTUAL_INFO_SQUARE);
    return SLAM_OK;
}

// start states [n_states][8][2]: finite, of unit norm to 1e-9
int check_states(const double* states, int64_t n_states) {
    if (!states || n_states <= 0) return fail(SLAM_ERR_INVALID, "states: at least one state of 8 amplitudes is required");
    if (n_states > 0x7fff0000LL) return fail(SLAM_ERR_INVALID, "too many states (%lld)", (long long)n_states);
    for (int64_t s = 0; s < n_states; ++s) {
        double norm2 = 0.0;
        for (int i = 0; i < 16; ++i) {
            const double v = states[s * 16 + i];
            if (!std::isfinite(v)) return fail(SLAM_ERR_INVALID, "states[%lld]: entry %d is not finite", (long long)s, i);
            norm2 += v * v;
        }
        if (!(std::fabs(norm2 - 1.0) <= 1e-9)) return fail(SLAM_ERR_INVALID, "states[%lld]: |psi|^2 = %.17g is not 1 to 1e-9", (long long)s, norm2);
    }
    return SLAM_OK;
}

// the 4x4 of every position, in order: [k][4][4][2] on the device; for a mixed plan the table of three-qubit gates too
int stage_q3_gates(slam_ctx* c, DevBuf& d, DevBuf& d3, const Q3Plan& p) {
    HIP_TRY(d.reserve(p.gates2.size() * sizeof(double)));
    HIP_TRY(hipMemcpyAsync(d.p, p.gates2.data(), p.gates2.size() * sizeof(double), hipMemcpyHostToDevice, c->stream));
    if (p.mixed) {
        HIP_TRY(d3.reserve((size_t)p.n_gates3 * 128 * sizeof(double)));
        HIP_TRY(hipMemcpyAsync(d3.p, p.gates3, (size_t)p.n_gates3 * 128 * sizeof(double), hipMemcpyHostToDevice, c->stream));
    }
    return SLAM_OK;
}

int check_eval_items(const double* targets, int64_t n_targets, const double* x, const int32_t* target_of, int64_t M, const double* loss) {
    if (!targets || n_targets <= 0) return fail(SLAM_ERR_INVALID, "targets: at least one 8x8 target is required");
    if (!x || !target_of || !loss) return fail(SLAM_ERR_INVALID, "x, target_of and loss are required");
    if (M <= 0 || M > 0x7fff0000LL) return fail(SLAM_ERR_INVALID, "M must be in 1..%lld (got %lld)", 0x7fff0000LL, (long long)M);
    for (int64_t m = 0; m < M; ++m)
        if (target_of[m] < 0 || target_of[m] >= n_targets)
            return fail(SLAM_ERR_INVALID, "target_of[%lld] = %d outside the targets (n_targets = %lld)", (long long)m, target_of[m], (long long)n_targets);
    return SLAM_OK;
}

int check_minimize_stage(const slam_opt_params* params, const double* targets, int64_t n_targets, double exit_loss) {
    { int rc = check_params(params); if (rc) return rc; }
    if (!targets || n_targets <= 0) return fail(SLAM_ERR_INVALID, "targets: at least one 8x8 target is required");
    if (n_targets * (int64_t)params->restarts > 0x7fff0000LL)
        return fail(SLAM_ERR_INVALID, "too many work items in one stage (%lld)", (long long)(n_targets * (int64_t)params->restarts));
    if (!(exit_loss == exit_loss)) return fail(SLAM_ERR_INVALID, "exit_loss is NaN");
    return SLAM_OK;
}

// explicit start points x0[n_targets * restarts * n], as the two-qubit stage checks them (slam_hip.hip, upload_stage_x0): the
// optimizer's evaluation takes its sines and cosines from the table path, which is valid for |x| < 2e8 only
int check_stage_x0(const double* x0, int64_t count) {
    if (!x0) return SLAM_OK;
    for (int64_t i = 0; i < count; ++i)
        if (!(x0[i] > -1e8 && x0[i] < 1e8)) return fail(SLAM_ERR_INVALID, "x0[%lld] = %g: explicit seeds must be finite with |x| < 1e8", (long long)i, x0[i]);
    return SLAM_OK;
}

int upload(slam_ctx* c, DevBuf& d, const void* src, size_t bytes) {
    HIP_TRY(d.reserve(bytes));
    HIP_TRY(hipMemcpyAsync(d.p, src, bytes, hipMemcpyHostToDevice, c->stream));
    return SLAM_OK;
}

int q3_eval(slam_ctx* c, const Q3Plan& plan, const double* targets, int64_t n_targets, const double* x, const int32_t* target_of, int64_t M,
            int32_t cost_kind, double* loss, double* grad, double* unitary) {
    const int n = plan.n;
    const void* kernel = plan.state ? (plan.mixed ? reinterpret_cast<const void*>(&eval_q3_kernel<true, true>) : reinterpret_cast<const void*>(&eval_q3_kernel<false, true>))
                                    : (plan.mixed ? reinterpret_cast<const void*>(&eval_q3_kernel<true>) : reinterpret_cast<const void*>(&eval_q3_kernel<false>));
    const size_t lds_bytes = plan.mixed ? kQ3MLdsBytes : kQ3LdsBytes;
    const size_t item_doubles = plan.state ? 16 : 128;  // a state [8][2] or a target / unitary [8][8][2]
    HIP_TRY(hipSetDevice(c->device));
    { int rc = kernel_per_cu(c, kernel, lds_bytes, nullptr); if (rc) return rc; }
    DevBuf d_gates, d_gates3, d_targets, d_x, d_tof, d_loss, d_grad, d_unitary;
    { int rc = stage_q3_gates(c, d_gates, d_gates3, plan); if (rc) return rc; }
    { int rc = upload(c, d_targets, targets, (size_t)n_targets * item_doubles * sizeof(double)); if (rc) return rc; }
    { int rc = upload(c, d_x, x, (size_t)M * n * sizeof(double)); if (rc) return rc; }
    { int rc = upload(c, d_tof, target_of, (size_t)M * sizeof(int32_t)); if (rc) return rc; }
    HIP_TRY(d_loss.reserve((size_t)M * sizeof(double)));
    if (grad) HIP_TRY(d_grad.reserve((size_t)M * n * sizeof(double)));
    if (unitary) HIP_TRY(d_unitary.reserve((size_t)M * item_doubles * sizeof(double)));
    Q3MEvalArgs a{};
    a.targets = d_targets.as<double>();
    a.x = d_x.as<double>();
    a.target_of = d_tof.as<int32_t>();
    a.n_items = M;
    a.loss = d_loss.as<double>();
    a.grad = grad ? d_grad.as<double>() : nullptr;
    a.unitary = unitary ? d_unitary.as<double>() : nullptr;
    a.cost_kind = cost_kind;
    a.gates = d_gates.as<double>();
    a.edges = plan.edge_bits;
    a.k = plan.k;
    a.gates3 = d_gates3.as<double>();
    a.ext = plan.ext_bits;
    a.n_gates3 = plan.n_gates3;
    a.n = n;
    int64_t blocks = M;
    const int64_t cap = (int64_t)16 * c->compute_units;
    if (blocks > cap) blocks = cap;
    if (plan.state && plan.mixed) hipLaunchKernelGGL((eval_q3_kernel<true, true>), dim3((unsigned)blocks), dim3(kWave), kQ3MLdsBytes, c->stream, a);
    else if (plan.state) hipLaunchKernelGGL((eval_q3_kernel<false, true>), dim3((unsigned)blocks), dim3(kWave), kQ3LdsBytes, c->stream, static_cast<const Q3EvalArgs&>(a));
    else if (plan.mixed) hipLaunchKernelGGL(eval_q3_kernel<true>, dim3((unsigned)blocks), dim3(kWave), kQ3MLdsBytes, c->stream, a);
    else hipLaunchKernelGGL(eval_q3_kernel<false>, dim3((unsigned)blocks), dim3(kWave), kQ3LdsBytes, c->stream, static_cast<const Q3EvalArgs&>(a));
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(loss, d_loss.p, (size_t)M * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (grad) HIP_TRY(hipMemcpyAsync(grad, d_grad.p, (size_t)M * n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (unitary) HIP_TRY(hipMemcpyAsync(unitary, d_unitary.p, (size_t)M * item_doubles * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return SLAM_OK;
}

int q3_minimize(slam_ctx* c, const Q3Plan& plan, const double* targets, int64_t N, int32_t cost_kind, const slam_opt_params* prm, double exit_loss, const double* x0, double* best_loss, double* best_x,
                int32_t* best_restart, double* item_loss, int32_t* item_iters, int32_t* item_status, int32_t* item_evals, double* item_x,
                double* kernel_ms) {
    const int n = plan.n;
    const void* kernel = plan.state ? (plan.mixed ? reinterpret_cast<const void*>(&minimize_q3_kernel<true, true>) : reinterpret_cast<const void*>(&minimize_q3_kernel<false, true>))
                                    : (plan.mixed ? reinterpret_cast<const void*>(&minimize_q3_kernel<true>) : reinterpret_cast<const void*>(&minimize_q3_kernel<false>));
    const size_t lds_bytes = plan.mixed ? kQ3MLdsBytes : kQ3LdsBytes;
    const int R = prm->restarts;
    const int64_t M = N * (int64_t)R;
    HIP_TRY(hipSetDevice(c->device));
    int per_cu = 0;
    { int rc = kernel_per_cu(c, kernel, lds_bytes, &per_cu); if (rc) return rc; }
    int64_t blocks = (int64_t)per_cu * c->compute_units;  // persistent wavefronts, one item each at a time
    if (blocks > M) blocks = M;
    if (blocks < 1) blocks = 1;
    DevBuf d_gates, d_gates3, d_targets, d_x0, d_ctl, d_solved, d_rec, d_x, d_hmem;
    { int rc = stage_q3_gates(c, d_gates, d_gates3, plan); if (rc) return rc; }
    { int rc = upload(c, d_targets, targets, (size_t)N * (plan.state ? 16 : 128) * sizeof(double)); if (rc) return rc; }
    if (x0) { int rc = upload(c, d_x0, x0, (size_t)M * n * sizeof(double)); if (rc) return rc; }
    StageCtl h_ctl{};
    h_ctl.n_active = (int32_t)N;
    { int rc = upload(c, d_ctl, &h_ctl, sizeof(StageCtl)); if (rc) return rc; }
    HIP_TRY(d_solved.reserve((size_t)N * sizeof(int32_t)));
    HIP_TRY(hipMemsetAsync(d_solved.p, 0, (size_t)N * sizeof(int32_t), c->stream));
    HIP_TRY(d_rec.reserve((size_t)M * sizeof(ItemRec)));
    HIP_TRY(d_x.reserve((size_t)M * n * sizeof(double)));
    HIP_TRY(d_hmem.reserve((size_t)blocks * (size_t)n * kQ3HStride * sizeof(float)));
    Q3MArgs a{};
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
    a.edges = plan.edge_bits;
    a.k = plan.k;
    a.hmem = d_hmem.as<float>();
    a.gates3 = d_gates3.as<double>();
    a.ext = plan.ext_bits;
    a.n_gates3 = plan.n_gates3;
    a.n = n;
    Event e0, e1;
    HIP_TRY(hipEventCreate(&e0.h));
    HIP_TRY(hipEventCreate(&e1.h));
    HIP_TRY(hipEventRecord(e0, c->stream));
    if (plan.state && plan.mixed) hipLaunchKernelGGL((minimize_q3_kernel<true, true>), dim3((unsigned)blocks), dim3(kWave), kQ3MLdsBytes, c->stream, a);
    else if (plan.state) hipLaunchKernelGGL((minimize_q3_kernel<false, true>), dim3((unsigned)blocks), dim3(kWave), kQ3LdsBytes, c->stream, static_cast<const Q3Args&>(a));
    else if (plan.mixed) hipLaunchKernelGGL(minimize_q3_kernel<true>, dim3((unsigned)blocks), dim3(kWave), kQ3MLdsBytes, c->stream, a);
    else hipLaunchKernelGGL(minimize_q3_kernel<false>, dim3((unsigned)blocks), dim3(kWave), kQ3LdsBytes, c->stream, static_cast<const Q3Args&>(a));
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
    { int rc = check_eval_items(targets, n_targets, x, target_of, M, loss); if (rc) return rc; }
    if (!ctx) return fail(SLAM_ERR_INVALID, "ctx is NULL");
    Q3Plan plan;
    fill_plan(plan, gates, k, gate_index, edge_bits);
    return drained(ctx, q3_eval(ctx, plan, targets, n_targets, x, target_of, M, cost_kind, loss, grad, unitary));
}

int slam_q3m_eval(slam_ctx* ctx, const double* gates2, int32_t n_gates2, const double* gates3, int32_t n_gates3, int32_t k, const int32_t* arity,
                  const int32_t* gate_index, const int32_t* qubits, const double* targets, int64_t n_targets, const double* x,
                  const int32_t* target_of, int64_t M, int32_t cost_kind, double* loss, double* grad, double* unitary) {
    Q3Plan plan;
    { int rc = check_mixed(gates2, n_gates2, gates3, n_gates3, k, arity, gate_index, qubits, &plan); if (rc) return rc; }
    { int rc = check_cost(cost_kind); if (rc) return rc; }
    { int rc = check_eval_items(targets, n_targets, x, target_of, M, loss); if (rc) return rc; }
    if (!ctx) return fail(SLAM_ERR_INVALID, "ctx is NULL");
    return drained(ctx, q3_eval(ctx, plan, targets, n_targets, x, target_of, M, cost_kind, loss, grad, unitary));
}

int slam_q3_minimize(slam_ctx* ctx, const double* gates, int32_t n_gates, int32_t k, const int32_t* gate_index, const int32_t* edges,
                     const double* targets, int64_t n_targets, int32_t cost_kind, const slam_opt_params* params, double exit_loss,
                     const double* x0, double* best_loss, double* best_x, int32_t* best_restart, double* item_loss, int32_t* item_iters,
                     int32_t* item_status, int32_t* item_evals, double* item_x, double* kernel_ms) {
    uint64_t edge_bits = 0;
    { int rc = check_template(gates, n_gates, k, gate_index, edges, &edge_bits); if (rc) return rc; }
    { int rc = check_cost(cost_kind); if (rc) return rc; }
    { int rc = check_minimize_stage(params, targets, n_targets, exit_loss); if (rc) return rc; }
    { int rc = check_stage_x0(x0, n_targets * (int64_t)params->restarts * (9 + 6 * k)); if (rc) return rc; }
    if (!ctx) return fail(SLAM_ERR_INVALID, "ctx is NULL");
    Q3Plan plan;
    fill_plan(plan, gates, k, gate_index, edge_bits);
    return drained(ctx, q3_minimize(ctx, plan, targets, n_targets, cost_kind, params, exit_loss, x0, best_loss, best_x, best_restart, item_loss,
                                    item_iters, item_status, item_evals, item_x, kernel_ms));
}

int slam_q3m_minimize(slam_ctx* ctx, const double* gates2, int32_t n_gates2, const double* gates3, int32_t n_gates3, int32_t k,
                      const int32_t* arity, const int32_t* gate_index, const int32_t* qubits, const double* targets, int64_t n_targets,
                      int32_t cost_kind, const slam_opt_params* params, double exit_loss, const double* x0, double* best_loss, double* best_x,
                      int32_t* best_restart, double* item_loss, int32_t* item_iters, int32_t* item_status, int32_t* item_evals, double* item_x,
                      double* kernel_ms) {
    Q3Plan plan;
    { int rc = check_mixed(gates2, n_gates2, gates3, n_gates3, k, arity, gate_index, qubits, &plan); if (rc) return rc; }
    { int rc = check_cost(cost_kind); if (rc) return rc; }
    { int rc = check_minimize_stage(params, targets, n_targets, exit_loss); if (rc) return rc; }
    { int rc = check_stage_x0(x0, n_targets * (int64_t)params->restarts * plan.n); if (rc) return rc; }
    if (!ctx) return fail(SLAM_ERR_INVALID, "ctx is NULL");
    return drained(ctx, q3_minimize(ctx, plan, targets, n_targets, cost_kind, params, exit_loss, x0, best_loss, best_x, best_restart, item_loss,
                                    item_iters, item_status, item_evals, item_x, kernel_ms));
}

int slam_q3s_eval(slam_ctx* ctx, const double* gates2, int32_t n_gates2, const double* gates3, int32_t n_gates3, int32_t k, const int32_t* arity,
                  const int32_t* gate_index, const int32_t* qubits, const double* states, int64_t n_states, const double* x,
                  const int32_t* state_of, int64_t M, int32_t cost_kind, double* loss, double* grad, double* out_state) {
    Q3Plan plan;
    { int rc = check_mixed(gates2, n_gates2, gates3, n_gates3, k, arity, gate_index, qubits, &plan); if (rc) return rc; }
    { int rc = check_state_cost(cost_kind); if (rc) return rc; }
    { int rc = check_states(states, n_states); if (rc) return rc; }
    { int rc = check_eval_items(states, n_states, x, state_of, M, loss); if (rc) return rc; }
    if (!ctx) return fail(SLAM_ERR_INVALID, "ctx is NULL");
    plan.state = true;
    return drained(ctx, q3_eval(ctx, plan, states, n_states, x, state_of, M, cost_kind, loss, grad, out_state));
}

int slam_q3s_minimize(slam_ctx* ctx, const double* gates2, int32_t n_gates2, const double* gates3, int32_t n_gates3, int32_t k,
                      const int32_t* arity, const int32_t* gate_index, const int32_t* qubits, const double* states, int64_t n_states,
                      int32_t cost_kind, const slam_opt_params* params, double exit_loss, const double* x0, double* best_loss, double* best_x,
                      int32_t* best_restart, double* item_loss, int32_t* item_iters, int32_t* item_status, int32_t* item_evals, double* item_x,
                      double* kernel_ms) {
    Q3Plan plan;
    { int rc = check_mixed(gates2, n_gates2, gates3, n_gates3, k, arity, gate_index, qubits, &plan); if (rc) return rc; }
    { int rc = check_state_cost(cost_kind); if (rc) return rc; }
    { int rc = check_states(states, n_states); if (rc) return rc; }
    { int rc = check_minimize_stage(params, states, n_states, exit_loss); if (rc) return rc; }
    { int rc = check_stage_x0(x0, n_states * (int64_t)params->restarts * plan.n); if (rc) return rc; }
    if (!ctx) return fail(SLAM_ERR_INVALID, "ctx is NULL");
    plan.state = true;
    return drained(ctx, q3_minimize(ctx, plan, states, n_states, cost_kind, params, exit_loss, x0, best_loss, best_x, best_restart, item_loss,
                                    item_iters, item_status, item_evals, item_x, kernel_ms));
}

}  // extern "C"
