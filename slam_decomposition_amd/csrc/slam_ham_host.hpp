// slam_ham_host.hpp -- what the host units of the Hamiltonian templates share: slam_ham_host.hip (one exponential, slam_ham.hpp) and
// slam_hams_host.hip (time slices, slam_hams.hpp).  The checks of a description, the compression of dense term matrices into the
// per-entry contribution lists the kernels read, and the two drivers -- one evaluation launch, one optimizer stage -- as templates over
// the kernel's argument structure and the unit's plan.  A plan is a checked description: `dim`, `n`, and
// `int stage(slam_ctx*, int64_t wavefronts, Desc*)`, which puts what the kernel reads onto the device and fills the kernel's descriptor.
// Included after the unit's kernel header (the launch constants of slam_q3.hpp).
#pragma once
#include "slam_host.hpp"

namespace hamhost {

// dimensions, caps and pointers of a description, before anything touches the device
inline int check_shape(int32_t dim, int32_t n_params, int32_t n_terms, const double* matrices, const int32_t* s_index, const int32_t* phi_index,
                       int32_t t_index) {
    if (dim != 4 && dim != 8) return fail(SLAM_ERR_INVALID, "dim must be 4 or 8 (got %d)", dim);
    if (n_params < 1) return fail(SLAM_ERR_INVALID, "n_params must be positive (got %d)", n_params);
    if (n_params > SLAM_HAM_MAX_PARAMS) return fail(SLAM_ERR_UNSUPPORTED, "a Hamiltonian takes at most %d parameters (got %d)", SLAM_HAM_MAX_PARAMS, n_params);
    if (n_terms < 1) return fail(SLAM_ERR_INVALID, "n_terms must be positive (got %d)", n_terms);
    if (n_terms > SLAM_HAM_MAX_TERMS) return fail(SLAM_ERR_UNSUPPORTED, "a Hamiltonian takes at most %d terms (got %d)", SLAM_HAM_MAX_TERMS, n_terms);
    if (!matrices || !s_index || !phi_index) return fail(SLAM_ERR_INVALID, "matrices, s_index and phi_index are required");
    if (t_index < -1 || t_index >= n_params) return fail(SLAM_ERR_INVALID, "t_index = %d outside -1 .. %d", t_index, n_params - 1);
    return SLAM_OK;
}

// the index arrays of one Hamiltonian; `where` goes in front of the message ("" or "slice 3: ")
inline int check_indices(int32_t n_params, int32_t n_terms, const int32_t* s_index, const int32_t* phi_index, const char* where) {
    for (int k = 0; k < n_terms; ++k) {
        if (s_index[k] < 0 || s_index[k] >= n_params)
            return fail(SLAM_ERR_INVALID, "%ss_index[%d] = %d outside 0 .. %d", where, k, s_index[k], n_params - 1);
        if (phi_index[k] < -1 || phi_index[k] >= n_params)
            return fail(SLAM_ERR_INVALID, "%sphi_index[%d] = %d outside -1 .. %d", where, k, phi_index[k], n_params - 1);
    }
    return SLAM_OK;
}

inline int check_matrices(int32_t dim, int32_t n_terms, const double* matrices) {
    for (int64_t i = 0; i < (int64_t)n_terms * dim * dim * 2; ++i)
        if (!std::isfinite(matrices[i])) return fail(SLAM_ERR_INVALID, "matrices: entry %lld is not finite", (long long)i);
    return SLAM_OK;
}

// The entry lists of one Hamiltonian: w [64][2][2] and idx [64] (zeroed by the caller), lane = r | c << 3 of the 8x8; M[r][c] feeds
// entry (r, c) as it is and entry (c, r) conjugated.  merge_diagonal: the two halves of a phase-free term on a diagonal entry become
// one contribution of weight 2 Re M[r][r].
inline int compress_terms(int32_t dim, int32_t n_terms, const double* matrices, const int32_t* s_index, const int32_t* phi_index, bool merge_diagonal,
                          const char* where, double* w, uint32_t* idx) {
    int count[64] = {0};
    auto add = [&](int lane, double re, double im, int k, int half) {
        const int q = count[lane]++;
        if (q >= 2) return false;
        w[(lane * 2 + q) * 2] = re;
        w[(lane * 2 + q) * 2 + 1] = im;
        idx[lane] |= ((uint32_t)(s_index[k] + 1) | ((uint32_t)(phi_index[k] + 1) << 6) | ((uint32_t)half << 12)) << (16 * q);
        return true;
    };
    for (int k = 0; k < n_terms; ++k)
        for (int r = 0; r < dim; ++r)
            for (int c = 0; c < dim; ++c) {
                const double* m = matrices + (((size_t)k * dim + r) * dim + c) * 2;
                if (m[0] == 0.0 && m[1] == 0.0) continue;
                bool ok = true;
                if (merge_diagonal && r == c && phi_index[k] < 0) {
                    if (m[0] != 0.0) ok = add(r | (r << 3), 2.0 * m[0], 0.0, k, 0);
                } else {
                    ok = add(r | (c << 3), m[0], m[1], k, 0);
                    const int lane = c | (r << 3);
                    if (ok && !add(lane, m[0], -m[1], k, 1)) return fail(SLAM_ERR_UNSUPPORTED, "%sentry (%d, %d) of the Hamiltonian takes more than two contributions", where, lane & 7, lane >> 3);
                }
                if (!ok) return fail(SLAM_ERR_UNSUPPORTED, "%sentry (%d, %d) of the Hamiltonian takes more than two contributions", where, r, c);
            }
    return SLAM_OK;
}

inline int check_cost(int32_t cost_kind) {
    if (cost_kind != SLAM_COST_BASIC && cost_kind != SLAM_COST_SQUARE)
        return fail(SLAM_ERR_INVALID, "cost kind %d: the Hamiltonian templates take SLAM_COST_BASIC and SLAM_COST_SQUARE", cost_kind);
    return SLAM_OK;
}

inline int check_targets(const double* targets, int64_t n_targets, int dim) {
    if (!targets || n_targets <= 0) return fail(SLAM_ERR_INVALID, "targets: at least one %dx%d target is required", dim, dim);
    if (n_targets > 0x7fff0000LL) return fail(SLAM_ERR_INVALID, "too many targets (%lld)", (long long)n_targets);
    for (int64_t i = 0; i < n_targets * dim * dim * 2; ++i)
        if (!std::isfinite(targets[i])) return fail(SLAM_ERR_INVALID, "targets: entry %lld is not finite", (long long)i);
    return SLAM_OK;
}

// the rows of an evaluation call
inline int check_rows(const double* x, const int32_t* target_of, const double* loss, int64_t M, int64_t n_targets, int32_t n_params) {
    if (!x || !target_of || !loss) return fail(SLAM_ERR_INVALID, "x, target_of and loss are required");
    if (M <= 0 || M > 0x7fff0000LL) return fail(SLAM_ERR_INVALID, "M must be in 1..%lld (got %lld)", 0x7fff0000LL, (long long)M);
    for (int64_t m = 0; m < M; ++m)
        if (target_of[m] < 0 || target_of[m] >= n_targets)
            return fail(SLAM_ERR_INVALID, "target_of[%lld] = %d outside the targets (n_targets = %lld)", (long long)m, target_of[m], (long long)n_targets);
    for (int64_t i = 0; i < M * n_params; ++i)
        if (!std::isfinite(x[i])) return fail(SLAM_ERR_INVALID, "x: entry %lld is not finite", (long long)i);
    return SLAM_OK;
}

// the work items, exit_loss and start points of an optimizer stage (params have passed check_params)
inline int check_stage(const slam_opt_params* params, int64_t n_targets, double exit_loss, const double* x0, int32_t n_params) {
    if (n_targets * (int64_t)params->restarts > 0x7fff0000LL)
        return fail(SLAM_ERR_INVALID, "too many work items in one stage (%lld)", (long long)(n_targets * (int64_t)params->restarts));
    if (!(exit_loss == exit_loss)) return fail(SLAM_ERR_INVALID, "exit_loss is NaN");
    if (!x0) return fail(SLAM_ERR_INVALID, "x0 is required: the start points of a Hamiltonian template are drawn on the host");
    // (the optimizer's evaluation takes its sines and cosines from the table path, valid for |x| < 2e8 only)
    for (int64_t i = 0; i < n_targets * (int64_t)params->restarts * n_params; ++i)
        if (!(x0[i] > -1e8 && x0[i] < 1e8)) return fail(SLAM_ERR_INVALID, "x0[%lld] = %g: start points must be finite with |x| < 1e8", (long long)i, x0[i]);
    return SLAM_OK;
}

inline int upload(slam_ctx* c, DevBuf& d, const void* src, size_t bytes) {
    HIP_TRY(d.reserve(bytes));
    HIP_TRY(hipMemcpyAsync(d.p, src, bytes, hipMemcpyHostToDevice, c->stream));
    return SLAM_OK;
}

// the targets as 8x8 (dim = 4: the leading block, zeros elsewhere) onto the device; `padded` lives until the stream has drained
inline int stage_targets(slam_ctx* c, int dim, const double* targets, int64_t n_targets, std::vector<double>& padded, DevBuf& d_t) {
    const double* src = targets;
    if (dim == 4) {
        padded.assign((size_t)n_targets * 128, 0.0);
        for (int64_t t = 0; t < n_targets; ++t)
            for (int r = 0; r < 4; ++r) std::memcpy(padded.data() + t * 128 + r * 16, targets + t * 32 + r * 8, 8 * sizeof(double));
        src = padded.data();
    }
    return upload(c, d_t, src, (size_t)n_targets * 128 * sizeof(double));
}

// one evaluation launch: item per wavefront, grid-stride
template <class Args, class Plan>
int eval_run(slam_ctx* c, void (*kernel)(Args), Plan& plan, const double* targets, int64_t n_targets, const double* x, const int32_t* target_of, int64_t M,
             int32_t cost_kind, double* loss, double* grad, double* unitary) {
    const int n = plan.n, dim = plan.dim;
    HIP_TRY(hipSetDevice(c->device));
    { int rc = kernel_per_cu(c, reinterpret_cast<const void*>(kernel), kQ3LdsBytes, nullptr); if (rc) return rc; }
    int64_t blocks = M;
    const int64_t cap = (int64_t)16 * c->compute_units;
    if (blocks > cap) blocks = cap;
    DevBuf d_targets, d_x, d_tof, d_loss, d_grad, d_unitary;
    std::vector<double> padded;
    Args a{};
    { int rc = stage_targets(c, dim, targets, n_targets, padded, d_targets); if (rc) return rc; }
    { int rc = plan.stage(c, blocks, &a.h); if (rc) return rc; }
    { int rc = upload(c, d_x, x, (size_t)M * n * sizeof(double)); if (rc) return rc; }
    { int rc = upload(c, d_tof, target_of, (size_t)M * sizeof(int32_t)); if (rc) return rc; }
    HIP_TRY(d_loss.reserve((size_t)M * sizeof(double)));
    if (grad) HIP_TRY(d_grad.reserve((size_t)M * n * sizeof(double)));
    if (unitary) HIP_TRY(d_unitary.reserve((size_t)M * 128 * sizeof(double)));
    a.targets = d_targets.as<double>();
    a.x = d_x.as<double>();
    a.target_of = d_tof.as<int32_t>();
    a.n_items = M;
    a.loss = d_loss.as<double>();
    a.grad = grad ? d_grad.as<double>() : nullptr;
    a.unitary = unitary ? d_unitary.as<double>() : nullptr;
    a.cost_kind = cost_kind;
    hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(kWave), kQ3LdsBytes, c->stream, a);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(loss, d_loss.p, (size_t)M * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (grad) HIP_TRY(hipMemcpyAsync(grad, d_grad.p, (size_t)M * n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    std::vector<double> u8;
    if (unitary) {
        double* dst = unitary;
        if (dim == 4) {
            u8.resize((size_t)M * 128);
            dst = u8.data();
        }
        HIP_TRY(hipMemcpyAsync(dst, d_unitary.p, (size_t)M * 128 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    }
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (unitary && dim == 4)
        for (int64_t m = 0; m < M; ++m)
            for (int r = 0; r < 4; ++r) std::memcpy(unitary + m * 32 + r * 8, u8.data() + m * 128 + r * 16, 8 * sizeof(double));
    return SLAM_OK;
}

// one optimizer stage: persistent wavefronts, one item each at a time; the reduction over the restarts as slam_q3_minimize
template <class Args, class Plan>
int minimize_run(slam_ctx* c, void (*kernel)(Args), Plan& plan, const double* targets, int64_t N, int32_t cost_kind, const slam_opt_params* prm,
                 double exit_loss, const double* x0, double* best_loss, double* best_x, int32_t* best_restart, double* item_loss, int32_t* item_iters,
                 int32_t* item_status, int32_t* item_evals, double* item_x, double* kernel_ms) {
    const int n = plan.n;
    const int R = prm->restarts;
    const int64_t M = N * (int64_t)R;
    HIP_TRY(hipSetDevice(c->device));
    int per_cu = 0;
    { int rc = kernel_per_cu(c, reinterpret_cast<const void*>(kernel), kQ3LdsBytes, &per_cu); if (rc) return rc; }
    int64_t blocks = (int64_t)per_cu * c->compute_units;
    if (blocks > M) blocks = M;
    if (blocks < 1) blocks = 1;
    DevBuf d_targets, d_x0, d_ctl, d_solved, d_rec, d_x, d_hmem;
    std::vector<double> padded;
    Args a{};
    { int rc = stage_targets(c, plan.dim, targets, N, padded, d_targets); if (rc) return rc; }
    { int rc = plan.stage(c, blocks, &a.h); if (rc) return rc; }
    { int rc = upload(c, d_x0, x0, (size_t)M * n * sizeof(double)); if (rc) return rc; }
    StageCtl h_ctl{};
    h_ctl.n_active = (int32_t)N;
    { int rc = upload(c, d_ctl, &h_ctl, sizeof(StageCtl)); if (rc) return rc; }
    HIP_TRY(d_solved.reserve((size_t)N * sizeof(int32_t)));
    HIP_TRY(hipMemsetAsync(d_solved.p, 0, (size_t)N * sizeof(int32_t), c->stream));
    HIP_TRY(d_rec.reserve((size_t)M * sizeof(ItemRec)));
    HIP_TRY(d_x.reserve((size_t)M * n * sizeof(double)));
    HIP_TRY(d_hmem.reserve((size_t)blocks * (size_t)n * kQ3HStride * sizeof(float)));
    a.targets = d_targets.as<double>();
    a.x0 = d_x0.as<double>();
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
    a.hmem = d_hmem.as<float>();
    Event e0, e1;
    HIP_TRY(hipEventCreate(&e0.h));
    HIP_TRY(hipEventCreate(&e1.h));
    HIP_TRY(hipEventRecord(e0, c->stream));
    hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(kWave), kQ3LdsBytes, c->stream, a);
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
    // per target the reduction over its restarts, as slam_q3_minimize: ordered -- the lowest-index restart below exit_loss; otherwise,
    // and when none is, the smallest loss (ties: the lowest index)
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

}  // namespace hamhost
