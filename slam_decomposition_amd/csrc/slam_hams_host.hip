// slam_hams_host.hip -- host side of the time-sliced Hamiltonian templates (slam_hams.hpp): slam_hams_eval and slam_hams_minimize, the
// slam_ham_* pair with n_slices index rows.  Self-contained calls on the checks and drivers of slam_ham_host.hpp.  A checked description
// is a HamsPlan: per slice the entry lists (a phase-free term's two halves on a diagonal entry merged into one contribution) and the set
// of parameters the slice reads; staging adds the wavefronts' workspace for the slices' eigenvectors.
#include "slam_host.hpp"
#include "slam_hams.hpp"
#include "slam_ham_host.hpp"

namespace {

using namespace hamhost;

static_assert(SLAM_HAMS_MAX_SLICES == kHamsMaxSlices, "header and kernel disagree");

struct HamsPlan {
    int dim = 0, n = 0, t_index = -1, n_slices = 0;
    std::vector<double> w;       // [S][64][2][2]
    std::vector<uint32_t> idx;   // [S][64]
    uint32_t reads[kHamsMaxSlices] = {0};
    DevBuf d_w, d_idx, d_work;

    int stage(slam_ctx* c, int64_t wavefronts, HamsDesc* desc) {
        { int rc = upload(c, d_w, w.data(), w.size() * sizeof(double)); if (rc) return rc; }
        { int rc = upload(c, d_idx, idx.data(), idx.size() * sizeof(uint32_t)); if (rc) return rc; }
        HIP_TRY(d_work.reserve((size_t)wavefronts * kHamsWorkDoubles * sizeof(double)));
        desc->w = d_w.as<double>();
        desc->idx = d_idx.as<uint32_t>();
        desc->work = d_work.as<double>();
        std::memcpy(desc->reads, reads, sizeof(reads));
        desc->n = n;
        desc->t_index = t_index;
        desc->dim = dim;
        desc->n_slices = n_slices;
        return SLAM_OK;
    }
};

// everything about the description, before anything touches the device
int check_description(int32_t dim, int32_t n_params, int32_t n_terms, int32_t n_slices, const double* matrices, const int32_t* s_index,
                      const int32_t* phi_index, int32_t t_index, HamsPlan* plan) {
    if (n_slices < 1 || n_slices > SLAM_HAMS_MAX_SLICES)
        return fail(n_slices < 1 ? SLAM_ERR_INVALID : SLAM_ERR_UNSUPPORTED, "n_slices must be in 1 .. %d (got %d)", SLAM_HAMS_MAX_SLICES, n_slices);
    { int rc = check_shape(dim, n_params, n_terms, matrices, s_index, phi_index, t_index); if (rc) return rc; }
    char where[32];
    for (int s = 0; s < n_slices; ++s) {
        std::snprintf(where, sizeof(where), "slice %d: ", s);
        int rc = check_indices(n_params, n_terms, s_index + (size_t)s * n_terms, phi_index + (size_t)s * n_terms, where);
        if (rc) return rc;
    }
    { int rc = check_matrices(dim, n_terms, matrices); if (rc) return rc; }
    plan->w.assign((size_t)n_slices * 256, 0.0);
    plan->idx.assign((size_t)n_slices * 64, 0u);
    for (int s = 0; s < n_slices; ++s) {
        std::snprintf(where, sizeof(where), "slice %d: ", s);
        const int32_t* si = s_index + (size_t)s * n_terms;
        const int32_t* pi = phi_index + (size_t)s * n_terms;
        int rc = compress_terms(dim, n_terms, matrices, si, pi, true, where, plan->w.data() + (size_t)s * 256, plan->idx.data() + (size_t)s * 64);
        if (rc) return rc;
        for (int k = 0; k < n_terms; ++k) {
            plan->reads[s] |= 1u << si[k];
            if (pi[k] >= 0) plan->reads[s] |= 1u << pi[k];
        }
    }
    plan->dim = dim;
    plan->n = n_params;
    plan->t_index = t_index;
    plan->n_slices = n_slices;
    return SLAM_OK;
}

}  // namespace

extern "C" {

int slam_hams_eval(slam_ctx* ctx, int32_t dim, int32_t n_params, int32_t n_terms, int32_t n_slices, const double* matrices, const int32_t* s_index,
                   const int32_t* phi_index, int32_t t_index, const double* targets, int64_t n_targets, const double* x, const int32_t* target_of,
                   int64_t M, int32_t cost_kind, double* loss, double* grad, double* unitary) {
    HamsPlan plan;
    { int rc = check_description(dim, n_params, n_terms, n_slices, matrices, s_index, phi_index, t_index, &plan); if (rc) return rc; }
    { int rc = check_cost(cost_kind); if (rc) return rc; }
    { int rc = check_targets(targets, n_targets, dim); if (rc) return rc; }
    { int rc = check_rows(x, target_of, loss, M, n_targets, n_params); if (rc) return rc; }
    if (!ctx) return fail(SLAM_ERR_INVALID, "ctx is NULL");
    return drained(ctx, eval_run<HamsEvalArgs>(ctx, &eval_hams_kernel, plan, targets, n_targets, x, target_of, M, cost_kind, loss, grad, unitary));
}

int slam_hams_minimize(slam_ctx* ctx, int32_t dim, int32_t n_params, int32_t n_terms, int32_t n_slices, const double* matrices,
                       const int32_t* s_index, const int32_t* phi_index, int32_t t_index, const double* targets, int64_t n_targets, int32_t cost_kind,
                       const slam_opt_params* params, double exit_loss, const double* x0, double* best_loss, double* best_x, int32_t* best_restart,
                       double* item_loss, int32_t* item_iters, int32_t* item_status, int32_t* item_evals, double* item_x, double* kernel_ms) {
    HamsPlan plan;
    { int rc = check_description(dim, n_params, n_terms, n_slices, matrices, s_index, phi_index, t_index, &plan); if (rc) return rc; }
    { int rc = check_cost(cost_kind); if (rc) return rc; }
    { int rc = check_params(params); if (rc) return rc; }
    { int rc = check_targets(targets, n_targets, dim); if (rc) return rc; }
    { int rc = check_stage(params, n_targets, exit_loss, x0, n_params); if (rc) return rc; }
    if (!ctx) return fail(SLAM_ERR_INVALID, "ctx is NULL");
    return drained(ctx, minimize_run<HamsArgs>(ctx, &minimize_hams_kernel, plan, targets, n_targets, cost_kind, params, exit_loss, x0, best_loss, best_x,
                                               best_restart, item_loss, item_iters, item_status, item_evals, item_x, kernel_ms));
}

}  // extern "C"
