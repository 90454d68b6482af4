// slam_ham_host.hip -- host side of the Hamiltonian templates (slam_ham.hpp, slam_ham_kernels.hpp): slam_ham_eval and slam_ham_minimize.  Both are
// self-contained: the Hamiltonian's description, targets and parameters come from the host with every call, the context lends its
// device and its stream, and nothing of it is touched or kept.  A checked description is a HamPlan: the dense term matrices compressed
// into the per-entry contribution lists the kernels read.  Checks and drivers are those of slam_ham_host.hpp.
#include "slam_host.hpp"
#include "slam_ham_kernels.hpp"
#include "slam_ham_host.hpp"

namespace {

using namespace hamhost;

static_assert(SLAM_HAM_MAX_TERMS == kHamMaxTerms && SLAM_HAM_MAX_PARAMS == kHamMaxParams, "header and kernel disagree");

struct HamPlan {
    int dim = 0, n = 0, t_index = -1;
    std::vector<double> w = std::vector<double>(256, 0.0);  // [64][2][2]
    std::vector<uint32_t> idx = std::vector<uint32_t>(64, 0u);
    DevBuf d_w, d_idx;

    // the entry lists onto the device
    int stage(slam_ctx* c, int64_t, HamDesc* desc) {
        { int rc = upload(c, d_w, w.data(), w.size() * sizeof(double)); if (rc) return rc; }
        { int rc = upload(c, d_idx, idx.data(), idx.size() * sizeof(uint32_t)); if (rc) return rc; }
        desc->w = d_w.as<double>();
        desc->idx = d_idx.as<uint32_t>();
        desc->n = n;
        desc->t_index = t_index;
        desc->dim = dim;
        return SLAM_OK;
    }
};

// everything about the description, before anything touches the device
int check_description(int32_t dim, int32_t n_params, int32_t n_terms, const double* matrices, const int32_t* s_index, const int32_t* phi_index,
                      int32_t t_index, HamPlan* plan) {
    { int rc = check_shape(dim, n_params, n_terms, matrices, s_index, phi_index, t_index); if (rc) return rc; }
    { int rc = check_indices(n_params, n_terms, s_index, phi_index, ""); if (rc) return rc; }
    { int rc = check_matrices(dim, n_terms, matrices); if (rc) return rc; }
    { int rc = compress_terms(dim, n_terms, matrices, s_index, phi_index, false, "", plan->w.data(), plan->idx.data()); if (rc) return rc; }
    plan->dim = dim;
    plan->n = n_params;
    plan->t_index = t_index;
    return SLAM_OK;
}

}  // namespace

extern "C" {

int slam_ham_eval(slam_ctx* ctx, int32_t dim, int32_t n_params, int32_t n_terms, const double* matrices, const int32_t* s_index,
                  const int32_t* phi_index, int32_t t_index, const double* targets, int64_t n_targets, const double* x, const int32_t* target_of,
                  int64_t M, int32_t cost_kind, double* loss, double* grad, double* unitary) {
    HamPlan plan;
    { int rc = check_description(dim, n_params, n_terms, matrices, s_index, phi_index, t_index, &plan); if (rc) return rc; }
    { int rc = check_cost(cost_kind); if (rc) return rc; }
    { int rc = check_targets(targets, n_targets, dim); if (rc) return rc; }
    { int rc = check_rows(x, target_of, loss, M, n_targets, n_params); if (rc) return rc; }
    if (!ctx) return fail(SLAM_ERR_INVALID, "ctx is NULL");
    return drained(ctx, eval_run<HamEvalArgs>(ctx, &eval_ham_kernel, plan, targets, n_targets, x, target_of, M, cost_kind, loss, grad, unitary));
}

int slam_ham_minimize(slam_ctx* ctx, int32_t dim, int32_t n_params, int32_t n_terms, const double* matrices, const int32_t* s_index,
                      const int32_t* phi_index, int32_t t_index, const double* targets, int64_t n_targets, int32_t cost_kind,
                      const slam_opt_params* params, double exit_loss, const double* x0, double* best_loss, double* best_x, int32_t* best_restart,
                      double* item_loss, int32_t* item_iters, int32_t* item_status, int32_t* item_evals, double* item_x, double* kernel_ms) {
    HamPlan plan;
    { int rc = check_description(dim, n_params, n_terms, matrices, s_index, phi_index, t_index, &plan); if (rc) return rc; }
    { int rc = check_cost(cost_kind); if (rc) return rc; }
    { int rc = check_params(params); if (rc) return rc; }
    { int rc = check_targets(targets, n_targets, dim); if (rc) return rc; }
    { int rc = check_stage(params, n_targets, exit_loss, x0, n_params); if (rc) return rc; }
    if (!ctx) return fail(SLAM_ERR_INVALID, "ctx is NULL");
    return drained(ctx, minimize_run<HamArgs>(ctx, &minimize_ham_kernel, plan, targets, n_targets, cost_kind, params, exit_loss, x0, best_loss, best_x,
                                              best_restart, item_loss, item_iters, item_status, item_evals, item_x, kernel_ms));
}

}  // extern "C"
