// slam_geometry.hip -- host side of libslamhip.so, geometry unit: Weyl coordinates, span prediction, coverage and family lookups, the Haar
// sampler and its selection by template size, candidate basis-gate scores (slam_candidates.hpp), parallel-drive coverage samples and region lookups, the KAK decomposition and
// local-gate completion (slam_weyl.hpp, slam_sampler.hpp, slam_span_sampler.hpp, slam_pd.hpp, slam_kak.hpp; their kernels in
// slam_span_sampler.hpp and slam_geometry_kernels.hpp).
#include "slam_host.hpp"
#include "slam_sampler.hpp"
#include "slam_span_sampler.hpp"
#include "slam_geometry_kernels.hpp"
#include "slam_candidates.hpp"

// One device (or host) buffer carved into typed sections: add<T>(n) appends n elements of T at the next offset aligned to alignof(T),
// `total` is what to reserve, and a section gives its typed pointer from the buffer's base and its size in bytes.
template <class T>
struct Section {
    size_t off, bytes;
    T* at(void* base) const { return reinterpret_cast<T*>(static_cast<char*>(base) + off); }
};
struct Carver {
    size_t total = 0;
    template <class T>
    Section<T> add(size_t n) {
        const size_t off = (total + alignof(T) - 1) & ~(alignof(T) - 1);
        total = off + n * sizeof(T);
        return {off, n * sizeof(T)};
    }
};

// the window [first, first + count) of the resident targets; cap_int32: of at most 2^31 - 1 targets
static int check_window(const slam_ctx* ctx, int64_t first, int64_t count, bool cap_int32) {
    if (first < 0 || count < 0 || first + count > ctx->n_targets) return fail(SLAM_ERR_INVALID, "target window outside the resident batch");
    if (cap_int32 && count > 0x7fffffffLL) return fail(SLAM_ERR_INVALID, "too many targets in one call (%lld)", (long long)count);
    return SLAM_OK;
}

// what slam_coverage_lookup and slam_family_lookup ask of a row table in the same words (each has checks of its own in between)
static int check_table_start(const int32_t* table_offsets) {
    if (table_offsets[0] != 0) return fail(SLAM_ERR_INVALID, "table_offsets[0] must be 0 (got %d)", table_offsets[0]);
    return SLAM_OK;
}
static int check_row_kinds(const int32_t* kinds, int64_t E) {
    for (int64_t e = 0; e < E; ++e)
        if (kinds[e] != 0 && kinds[e] != 1) return fail(SLAM_ERR_INVALID, "kinds[%lld] = %d (0 = one gate, 1 = half-spaces)", (long long)e, kinds[e]);
    return SLAM_OK;
}

int enqueue_c1c2c3(slam_ctx* c, const double* d_unitaries, int64_t count, int ndigits, double* d_out) {
    hipLaunchKernelGGL(c1c2c3_kernel, dim3((unsigned)((count + 63) / 64)), dim3(64), 0, c->stream, d_unitaries, count, ndigits, d_out);
    HIP_TRY(hipGetLastError());
    return SLAM_OK;
}

// the caller's half-spaces (slam_predict_spans: point[4], bounds[k_max][14], tol) as the kernels' argument block
static SpanRegions span_regions(int k_max, const double* point, const double* bounds, double tol) {
    static_assert(sizeof(SpanRegions{}.bounds) / sizeof(SpanRegions{}.bounds[0]) == SLAM_MAX_SPAN_EVAL, "SpanRegions::bounds holds SLAM_MAX_SPAN_EVAL prefixes");
    SpanRegions r{};
    r.k_max = k_max;
    r.tol = tol;
    for (int j = 0; j < 4; ++j) r.point[j] = point[j];
    for (int k = 2; k <= k_max; ++k)
        for (int p = 0; p < kSpanPatterns; ++p) r.bounds[k - 1][p] = bounds[(size_t)(k - 1) * kSpanPatterns + p];
    return r;
}

int enqueue_span_predict(slam_ctx* c, int64_t first, int64_t count, int k_max, const double* point, const double* bounds, double tol,
                         int32_t* d_spans) {
    const SpanRegions r = span_regions(k_max, point, bounds, tol);
    hipLaunchKernelGGL(span_predict_kernel, dim3((unsigned)((count + 63) / 64)), dim3(64), 0, c->stream, c->targets.as<double>() + first * 32, count, r,
                       d_spans);
    HIP_TRY(hipGetLastError());
    return SLAM_OK;
}

// Weyl coordinates of `count` unitaries that are already in device memory
static int weyl_device(slam_ctx* ctx, const double* d_unitaries, int64_t count, int ndigits, double* out) {
    HIP_TRY(ctx->ev_weyl.reserve((size_t)count * 3 * sizeof(double)));
    int rc = enqueue_c1c2c3(ctx, d_unitaries, count, ndigits, ctx->ev_weyl.as<double>());
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(out, ctx->ev_weyl.p, (size_t)count * 3 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return SLAM_OK;
}

// KAK records of `count` unitaries that are already in device memory, unpacked into the caller's arrays
static int kak_device(slam_ctx* ctx, const double* d_unitaries, int64_t count, double* phase, double* a1, double* a2, double* c, double* b1,
                      double* b2) {
    HIP_TRY(ctx->ev_weyl.reserve((size_t)count * kKakRecord * sizeof(double)));
    hipLaunchKernelGGL(kak_kernel, dim3((unsigned)((count + kKakBlock - 1) / kKakBlock)), dim3(kKakBlock), 0, ctx->stream, d_unitaries, count,
                       ctx->ev_weyl.as<double>());
    HIP_TRY(hipGetLastError());
    std::vector<double> rec((size_t)count * kKakRecord);
    HIP_TRY(hipMemcpyAsync(rec.data(), ctx->ev_weyl.p, rec.size() * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    for (int64_t i = 0; i < count; ++i) {
        const double* r = rec.data() + (size_t)i * kKakRecord;
        phase[i] = r[0];
        std::memcpy(a1 + i * 8, r + 1, 8 * sizeof(double));
        std::memcpy(a2 + i * 8, r + 9, 8 * sizeof(double));
        std::memcpy(c + i * 3, r + 17, 3 * sizeof(double));
        std::memcpy(b1 + i * 8, r + 20, 8 * sizeof(double));
        std::memcpy(b2 + i * 8, r + 28, 8 * sizeof(double));
    }
    return SLAM_OK;
}

extern "C" {

int slam_kak(slam_ctx* ctx, const double* unitaries, int64_t count, double* phase, double* a1, double* a2, double* c, double* b1, double* b2) {
    if (!ctx) return fail(SLAM_ERR_INVALID, "ctx is NULL");
    if (count < 0) return fail(SLAM_ERR_INVALID, "count < 0");
    if (count > 0x7fffffffLL) return fail(SLAM_ERR_INVALID, "too many unitaries in one call (%lld)", (long long)count);
    if (count == 0) return SLAM_OK;
    if (!unitaries) return fail(SLAM_ERR_INVALID, "unitaries is NULL");
    if (!phase || !a1 || !a2 || !c || !b1 || !b2) return fail(SLAM_ERR_INVALID, "phase, a1, a2, c, b1 and b2 must be non-NULL");
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(ctx->ev_unitary.reserve((size_t)count * 32 * sizeof(double)));
    HIP_TRY(hipMemcpyAsync(ctx->ev_unitary.p, unitaries, (size_t)count * 32 * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    return kak_device(ctx, ctx->ev_unitary.as<double>(), count, phase, a1, a2, c, b1, b2);
}

int slam_targets_kak(slam_ctx* ctx, int64_t first, int64_t count, double* phase, double* a1, double* a2, double* c, double* b1, double* b2) {
    if (!ctx) return fail(SLAM_ERR_INVALID, "ctx is NULL");
    if (int rc = check_window(ctx, first, count, true)) return rc;
    if (count == 0) return SLAM_OK;
    if (!phase || !a1 || !a2 || !c || !b1 || !b2) return fail(SLAM_ERR_INVALID, "phase, a1, a2, c, b1 and b2 must be non-NULL");
    HIP_TRY(hipSetDevice(ctx->device));
    return kak_device(ctx, ctx->targets.as<double>() + first * 32, count, phase, a1, a2, c, b1, b2);
}

int slam_complete_locals(slam_ctx* ctx, int k, const int32_t* gate_seq, const double* x, const int32_t* target_of, int64_t M, double* x_out,
                         double* loss_out, double* gap_out) {
    if (!ctx) return fail(SLAM_ERR_INVALID, "ctx is NULL");
    if (ctx->n_targets <= 0) return fail(SLAM_ERR_STATE, "no targets: call slam_set_targets first");
    if (ctx->n_gates <= 0) return fail(SLAM_ERR_STATE, "no gates: call slam_set_gates first");
    if (k < 1 || k > SLAM_MAX_SPAN_EVAL) return fail(SLAM_ERR_UNSUPPORTED, "span must be in 1..%d (got %d)", SLAM_MAX_SPAN_EVAL, k);
    if (M < 0) return fail(SLAM_ERR_INVALID, "M < 0");
    if (M > 0x7fffffffLL) return fail(SLAM_ERR_INVALID, "too many items in one call (%lld)", (long long)M);
    if (M == 0) return SLAM_OK;
    if (!gate_seq) return fail(SLAM_ERR_INVALID, "gate_seq is NULL");
    if (!x || !target_of) return fail(SLAM_ERR_INVALID, "x and target_of must be non-NULL");
    if (!x_out || !loss_out || !gap_out) return fail(SLAM_ERR_INVALID, "x_out, loss_out and gap_out must be non-NULL");
    static_assert(sizeof(CompleteArgs{}.seq) / sizeof(int32_t) == SLAM_MAX_SPAN_EVAL, "CompleteArgs::seq holds SLAM_MAX_SPAN_EVAL gates");
    CompleteArgs a{};
    a.k = k;
    for (int j = 0; j < k; ++j) {
        if (gate_seq[j] < 0 || gate_seq[j] >= ctx->n_gates)
            return fail(SLAM_ERR_INVALID, "gate_seq[%d] = %d outside the gate table (n_gates = %d)", j, gate_seq[j], ctx->n_gates);
        a.seq[j] = gate_seq[j];
    }
    for (int64_t m = 0; m < M; ++m)
        if (target_of[m] < 0 || target_of[m] >= ctx->n_targets)
            return fail(SLAM_ERR_INVALID, "target_of[%lld] = %d outside [0, %lld)", (long long)m, target_of[m], (long long)ctx->n_targets);
    const size_t n = 6 * ((size_t)k + 1);
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(ctx->ev_x.reserve((size_t)M * n * sizeof(double)));
    HIP_TRY(ctx->ev_tof.reserve((size_t)M * sizeof(int32_t)));
    HIP_TRY(ctx->ev_grad.reserve((size_t)M * n * sizeof(double)));  // the completed rows
    HIP_TRY(ctx->ev_loss.reserve((size_t)M * 2 * sizeof(double)));  // losses, then gaps
    HIP_TRY(hipMemcpyAsync(ctx->ev_x.p, x, (size_t)M * n * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipMemcpyAsync(ctx->ev_tof.p, target_of, (size_t)M * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
    a.gates = ctx->gates.as<double>();
    a.targets = ctx->targets.as<double>();
    a.x = ctx->ev_x.as<double>();
    a.target_of = ctx->ev_tof.as<int32_t>();
    a.M = M;
    a.x_out = ctx->ev_grad.as<double>();
    a.loss_out = ctx->ev_loss.as<double>();
    a.gap_out = ctx->ev_loss.as<double>() + M;
    hipLaunchKernelGGL(complete_locals_kernel, dim3((unsigned)((M + kKakBlock - 1) / kKakBlock)), dim3(kKakBlock), 0, ctx->stream, a);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(x_out, ctx->ev_grad.p, (size_t)M * n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipMemcpyAsync(loss_out, a.loss_out, (size_t)M * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipMemcpyAsync(gap_out, a.gap_out, (size_t)M * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return SLAM_OK;
}

int slam_c1c2c3(slam_ctx* ctx, const double* unitaries, int64_t count, int ndigits, double* out) {
    if (!ctx) return fail(SLAM_ERR_INVALID, "ctx is NULL");
    if (count < 0) return fail(SLAM_ERR_INVALID, "count < 0");
    if (count == 0) return SLAM_OK;
    if (!unitaries || !out) return fail(SLAM_ERR_INVALID, "unitaries and out must be non-NULL");
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(ctx->ev_unitary.reserve((size_t)count * 32 * sizeof(double)));
    HIP_TRY(hipMemcpyAsync(ctx->ev_unitary.p, unitaries, (size_t)count * 32 * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    return weyl_device(ctx, ctx->ev_unitary.as<double>(), count, ndigits, out);
}

int slam_targets_c1c2c3(slam_ctx* ctx, int64_t first, int64_t count, int ndigits, double* out) {
    if (!ctx) return fail(SLAM_ERR_INVALID, "ctx is NULL");
    if (int rc = check_window(ctx, first, count, false)) return rc;
    if (count == 0) return SLAM_OK;
    if (!out) return fail(SLAM_ERR_INVALID, "out is NULL");
    HIP_TRY(hipSetDevice(ctx->device));
    return weyl_device(ctx, ctx->targets.as<double>() + first * 32, count, ndigits, out);
}

int slam_predict_spans(slam_ctx* ctx, int64_t first, int64_t count, int k_max, const double* point, const double* bounds, double tol,
                       int32_t* spans_out) {
    if (!ctx) return fail(SLAM_ERR_INVALID, "ctx is NULL");
    if (int rc = check_window(ctx, first, count, false)) return rc;
    if (k_max < 1 || k_max > SLAM_MAX_SPAN_EVAL) return fail(SLAM_ERR_INVALID, "k_max must be 1..%d (got %d)", SLAM_MAX_SPAN_EVAL, k_max);
    if (!point || (k_max > 1 && !bounds)) return fail(SLAM_ERR_INVALID, "point / bounds is NULL");
    if (count == 0) return SLAM_OK;
    if (!spans_out) return fail(SLAM_ERR_INVALID, "spans_out is NULL");
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(ctx->ev_weyl.reserve((size_t)count * sizeof(int32_t)));
    int rc = enqueue_span_predict(ctx, first, count, k_max, point, bounds, tol, ctx->ev_weyl.as<int32_t>());
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(spans_out, ctx->ev_weyl.p, (size_t)count * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return SLAM_OK;
}

int slam_coverage_lookup(slam_ctx* ctx, int64_t first, int64_t count, int32_t n_tables, const int32_t* table_offsets, const int32_t* kinds,
                         const double* points, const double* bounds, double tol, int64_t* counts_out, int32_t* entry_out) {
    if (!ctx) return fail(SLAM_ERR_INVALID, "ctx is NULL");
    if (int rc = check_window(ctx, first, count, true)) return rc;
    if (n_tables < 1) return fail(SLAM_ERR_INVALID, "n_tables must be >= 1 (got %d)", n_tables);
    if (!table_offsets) return fail(SLAM_ERR_INVALID, "table_offsets is NULL");
    if (int rc = check_table_start(table_offsets)) return rc;
    int32_t max_bins = 0;
    for (int32_t t = 0; t < n_tables; ++t) {
        if (table_offsets[t + 1] < table_offsets[t])
            return fail(SLAM_ERR_INVALID, "table_offsets must be non-decreasing (offsets[%d] = %d > offsets[%d] = %d)", t, table_offsets[t],
                        t + 1, table_offsets[t + 1]);
        if (table_offsets[t + 1] > 0x3fffffff) return fail(SLAM_ERR_INVALID, "too many coverage entries");
        const int32_t nb = table_offsets[t + 1] - table_offsets[t] + 2;
        if (nb > max_bins) max_bins = nb;
    }
    const int64_t E = table_offsets[n_tables];
    if (E > 0 && (!kinds || !points || !bounds)) return fail(SLAM_ERR_INVALID, "kinds / points / bounds is NULL");
    if (int rc = check_row_kinds(kinds, E)) return rc;
    if (!counts_out) return fail(SLAM_ERR_INVALID, "counts_out is NULL");
    const int64_t n_counts = E + 2 * (int64_t)n_tables;
    std::memset(counts_out, 0, (size_t)n_counts * sizeof(int64_t));
    if (count == 0) return SLAM_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    // one upload: offsets, kinds (int32), then points [E][4] and bounds [E][14] (doubles)
    Carver cv;
    const auto s_off = cv.add<int32_t>((size_t)n_tables + 1), s_kind = cv.add<int32_t>((size_t)E);
    const auto s_pt = cv.add<double>((size_t)E * 4), s_bd = cv.add<double>((size_t)E * kSpanPatterns);
    HIP_TRY(ctx->cov_table.reserve(cv.total));
    HIP_TRY(ctx->cov_counts.reserve((size_t)n_counts * sizeof(unsigned long long)));
    if (entry_out) HIP_TRY(ctx->cov_entries.reserve((size_t)n_tables * (size_t)count * sizeof(int32_t)));
    char* tb = ctx->cov_table.as<char>();
    HIP_TRY(hipMemcpyAsync(s_off.at(tb), table_offsets, s_off.bytes, hipMemcpyHostToDevice, ctx->stream));
    if (E > 0) {
        HIP_TRY(hipMemcpyAsync(s_kind.at(tb), kinds, s_kind.bytes, hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(hipMemcpyAsync(s_pt.at(tb), points, s_pt.bytes, hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(hipMemcpyAsync(s_bd.at(tb), bounds, s_bd.bytes, hipMemcpyHostToDevice, ctx->stream));
    }
    HIP_TRY(hipMemsetAsync(ctx->cov_counts.p, 0, (size_t)n_counts * sizeof(unsigned long long), ctx->stream));
    const int32_t lds_bins = max_bins < kCoverageLdsBins ? max_bins : kCoverageLdsBins;
    hipLaunchKernelGGL(coverage_lookup_kernel, dim3((unsigned)((count + kCoverageBlock - 1) / kCoverageBlock)), dim3(kCoverageBlock),
                       (size_t)lds_bins * sizeof(unsigned int), ctx->stream, ctx->targets.as<double>() + first * 32, count, n_tables,
                       s_off.at(tb), s_kind.at(tb), s_pt.at(tb), s_bd.at(tb), tol, lds_bins, ctx->cov_counts.as<unsigned long long>(),
                       entry_out ? ctx->cov_entries.as<int32_t>() : nullptr);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(counts_out, ctx->cov_counts.p, (size_t)n_counts * sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream));
    if (entry_out)
        HIP_TRY(hipMemcpyAsync(entry_out, ctx->cov_entries.p, (size_t)n_tables * (size_t)count * sizeof(int32_t), hipMemcpyDeviceToHost,
                               ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return SLAM_OK;
}

int slam_family_lookup(slam_ctx* ctx, int64_t first, int64_t count, int32_t n_members, const int32_t* table_offsets, const int32_t* kinds,
                       const double* points, const double* bounds, const int32_t* child_even, const int32_t* child_odd,
                       const double* durations, double cost_1q, double tol, int32_t policy, int64_t* counts_out, int64_t* base_counts_out,
                       int32_t* member_out, int32_t* gates_out) {
    if (!ctx) return fail(SLAM_ERR_INVALID, "ctx is NULL");
    if (int rc = check_window(ctx, first, count, true)) return rc;
    static_assert(SLAM_FAMILY_MAX_MEMBERS == kFamilyMaxMembers, "family size");
    if (n_members < 1 || n_members > SLAM_FAMILY_MAX_MEMBERS)
        return fail(SLAM_ERR_INVALID, "n_members must be in 1..%d (got %d)", SLAM_FAMILY_MAX_MEMBERS, n_members);
    if (!table_offsets || !kinds || !points || !bounds) return fail(SLAM_ERR_INVALID, "table_offsets / kinds / points / bounds is NULL");
    if (!child_even || !child_odd || !durations) return fail(SLAM_ERR_INVALID, "child_even / child_odd / durations is NULL");
    if (int rc = check_table_start(table_offsets)) return rc;
    for (int32_t m = 0; m < n_members; ++m)
        if (table_offsets[m + 1] <= table_offsets[m])
            return fail(SLAM_ERR_INVALID, "every member needs at least one row (offsets[%d] = %d, offsets[%d] = %d)", m, table_offsets[m], m + 1,
                        table_offsets[m + 1]);
    const int64_t E = table_offsets[n_members], E0 = table_offsets[1];
    if (E + E0 + 4 > kFamilyMaxBins) return fail(SLAM_ERR_INVALID, "too many coverage rows (%lld; at most %d bins)", (long long)E, kFamilyMaxBins);
    if (int rc = check_row_kinds(kinds, E)) return rc;
    for (int32_t m = 0; m < n_members; ++m) {
        // a child has a larger index than its parent: the kernel's one ascending pass over the members relies on it
        if (child_even[m] != -1 && (child_even[m] <= m || child_even[m] >= n_members))
            return fail(SLAM_ERR_INVALID, "child_even[%d] = %d must be -1 or in (%d, %d)", m, child_even[m], m, n_members);
        if (child_odd[m] != -1 && (child_odd[m] <= m || child_odd[m] >= n_members))
            return fail(SLAM_ERR_INVALID, "child_odd[%d] = %d must be -1 or in (%d, %d)", m, child_odd[m], m, n_members);
        if (!std::isfinite(durations[m])) return fail(SLAM_ERR_INVALID, "durations[%d] is not finite", m);
    }
    if (!std::isfinite(cost_1q) || !std::isfinite(tol)) return fail(SLAM_ERR_INVALID, "cost_1q and tol must be finite");
    if (policy != 0 && policy != 1) return fail(SLAM_ERR_INVALID, "policy must be 0 (the reference's walk) or 1 (best member), got %d", policy);
    if (!counts_out || !base_counts_out) return fail(SLAM_ERR_INVALID, "counts_out / base_counts_out is NULL");
    std::memset(counts_out, 0, (size_t)(E + 2) * sizeof(int64_t));
    std::memset(base_counts_out, 0, (size_t)(E0 + 2) * sizeof(int64_t));
    if (count == 0) return SLAM_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    // one upload: offsets, kinds, both child lists (int32), then points [E][4], bounds [E][14] and the rows' costs [E] (doubles).
    // The costs are computed here, once per row, so that the device compares the very doubles the caller sums.
    Carver cv;
    const auto s_off = cv.add<int32_t>((size_t)n_members + 1), s_kind = cv.add<int32_t>((size_t)E);
    const auto s_ce = cv.add<int32_t>((size_t)n_members), s_co = cv.add<int32_t>((size_t)n_members);
    const auto s_pt = cv.add<double>((size_t)E * 4), s_bd = cv.add<double>((size_t)E * kSpanPatterns), s_cs = cv.add<double>((size_t)E);
    std::vector<char> host(cv.total, 0);
    std::memcpy(s_off.at(host.data()), table_offsets, s_off.bytes);
    std::memcpy(s_kind.at(host.data()), kinds, s_kind.bytes);
    std::memcpy(s_ce.at(host.data()), child_even, s_ce.bytes);
    std::memcpy(s_co.at(host.data()), child_odd, s_co.bytes);
    std::memcpy(s_pt.at(host.data()), points, s_pt.bytes);
    std::memcpy(s_bd.at(host.data()), bounds, s_bd.bytes);
    double* row_cost = s_cs.at(host.data());
    for (int32_t m = 0; m < n_members; ++m)
        for (int32_t e = table_offsets[m]; e < table_offsets[m + 1]; ++e) {
            const double k = (double)(e - table_offsets[m] + 1);
            const double c1 = (k + 1.0) * cost_1q, c2 = k * durations[m];
            row_cost[e] = c1 + c2;  // (k + 1) cost_1q + k duration_m: two products and a sum, each rounded
        }
    const int64_t n_counts = E + 2 + E0 + 2;
    HIP_TRY(ctx->cov_table.reserve(cv.total));
    HIP_TRY(ctx->cov_counts.reserve((size_t)n_counts * sizeof(unsigned long long)));
    const bool want = member_out || gates_out;
    if (want) HIP_TRY(ctx->cov_entries.reserve(2 * (size_t)count * sizeof(int32_t)));
    char* tb = ctx->cov_table.as<char>();
    HIP_TRY(hipMemcpyAsync(tb, host.data(), cv.total, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipMemsetAsync(ctx->cov_counts.p, 0, (size_t)n_counts * sizeof(unsigned long long), ctx->stream));
    unsigned long long* d_counts = ctx->cov_counts.as<unsigned long long>();
    int32_t* d_member = want ? ctx->cov_entries.as<int32_t>() : nullptr;
    hipLaunchKernelGGL(family_lookup_kernel, dim3((unsigned)((count + kCoverageBlock - 1) / kCoverageBlock)), dim3(kCoverageBlock),
                       (size_t)n_counts * sizeof(unsigned int), ctx->stream, ctx->targets.as<double>() + first * 32, count, n_members,
                       s_off.at(tb), s_kind.at(tb), s_pt.at(tb), s_bd.at(tb), s_cs.at(tb), s_ce.at(tb), s_co.at(tb), tol, policy, d_counts,
                       d_counts + (E + 2), d_member, want ? d_member + count : nullptr);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(counts_out, d_counts, (size_t)(E + 2) * sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipMemcpyAsync(base_counts_out, d_counts + (E + 2), (size_t)(E0 + 2) * sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream));
    if (member_out) HIP_TRY(hipMemcpyAsync(member_out, d_member, (size_t)count * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    if (gates_out) HIP_TRY(hipMemcpyAsync(gates_out, d_member + count, (size_t)count * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return SLAM_OK;
}

int slam_candidate_scores(slam_ctx* ctx, int64_t first, int64_t count, int32_t n_candidates, const double* cand_coords, int32_t k_cap,
                          double tol, const int32_t* group_of, int32_t n_groups, int64_t* counts_out, int32_t* first_k_out,
                          double* kernel_ms_out) {
    static_assert(SLAM_CANDIDATE_MAX_K == kCandMaxK, "candidate k_cap");
    if (!ctx) return fail(SLAM_ERR_INVALID, "ctx is NULL");
    if (int rc = check_window(ctx, first, count, true)) return rc;
    if (n_candidates < 1 || n_candidates > SLAM_CANDIDATE_MAX_GATES)
        return fail(SLAM_ERR_INVALID, "n_candidates must be in 1..%d (got %d)", SLAM_CANDIDATE_MAX_GATES, n_candidates);
    if (k_cap < 1 || k_cap > SLAM_CANDIDATE_MAX_K) return fail(SLAM_ERR_INVALID, "k_cap must be in 1..%d (got %d)", SLAM_CANDIDATE_MAX_K, k_cap);
    if (!cand_coords) return fail(SLAM_ERR_INVALID, "cand_coords is NULL");
    for (int64_t j = 0; j < 3 * (int64_t)n_candidates; ++j)
        if (!std::isfinite(cand_coords[j])) return fail(SLAM_ERR_INVALID, "cand_coords[%lld] is not finite", (long long)j);
    if (!std::isfinite(tol)) return fail(SLAM_ERR_INVALID, "tol must be finite");
    if (n_groups < 1) return fail(SLAM_ERR_INVALID, "n_groups must be >= 1 (got %d)", n_groups);
    if (!group_of && n_groups != 1) return fail(SLAM_ERR_INVALID, "n_groups = %d needs group_of", n_groups);
    if (group_of)
        for (int64_t i = 0; i < count; ++i)
            if (group_of[i] < 0 || group_of[i] >= n_groups)
                return fail(SLAM_ERR_INVALID, "group_of[%lld] = %d outside [0, %d)", (long long)i, group_of[i], n_groups);
    if (!counts_out) return fail(SLAM_ERR_INVALID, "counts_out is NULL");
    const int64_t G = n_candidates, nb = (int64_t)k_cap + 2;
    const int64_t n_counts = (int64_t)n_groups * G * nb;
    if (n_counts > ((int64_t)1 << 31)) return fail(SLAM_ERR_INVALID, "n_groups x n_candidates x (k_cap + 2) = %lld counts: too many", (long long)n_counts);
    std::memset(counts_out, 0, (size_t)n_counts * sizeof(int64_t));
    if (kernel_ms_out) *kernel_ms_out = 0.0;
    if (count == 0) return SLAM_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    // one buffer: coordinates [G][3], alcove points [G][4], rows [G][k_cap - 1][14] (doubles), then the groups (int32)
    Carver cv;
    const auto s_crd = cv.add<double>((size_t)G * 3), s_pt = cv.add<double>((size_t)G * 4);
    const auto s_row = cv.add<double>((size_t)G * (size_t)(k_cap - 1) * kSpanPatterns);
    const auto s_grp = cv.add<int32_t>(group_of ? (size_t)count : 0);
    HIP_TRY(ctx->cov_table.reserve(cv.total));
    HIP_TRY(ctx->cov_counts.reserve((size_t)n_counts * sizeof(unsigned long long)));
    if (first_k_out) HIP_TRY(ctx->cov_entries.reserve((size_t)G * (size_t)count * sizeof(int32_t)));
    char* tb = ctx->cov_table.as<char>();
    HIP_TRY(hipMemcpyAsync(s_crd.at(tb), cand_coords, s_crd.bytes, hipMemcpyHostToDevice, ctx->stream));
    if (group_of) HIP_TRY(hipMemcpyAsync(s_grp.at(tb), group_of, s_grp.bytes, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipMemsetAsync(ctx->cov_counts.p, 0, (size_t)n_counts * sizeof(unsigned long long), ctx->stream));
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    if (kernel_ms_out) {
        HIP_TRY(hipEventCreate(&ev0));
        if (hipError_t e = hipEventCreate(&ev1); e != hipSuccess) {
            (void)hipEventDestroy(ev0);
            HIP_TRY(e);
        }
        (void)hipEventRecord(ev0, ctx->stream);
    }
    hipLaunchKernelGGL(candidate_rows_kernel, dim3((unsigned)((G + kCandRowsBlock - 1) / kCandRowsBlock)), dim3(kCandRowsBlock), 0, ctx->stream,
                       s_crd.at(tb), (int32_t)G, k_cap, s_pt.at(tb), s_row.at(tb));
    // candidates split over grid.y until the launch has about 2048 blocks: a circuit's few hundred targets still fill the device,
    // a large batch keeps one chunk (the target's Weyl coordinates are computed once per block)
    const int64_t t_blocks = (count + kCandBlock - 1) / kCandBlock;
    int64_t n_chunks = (2048 + t_blocks - 1) / t_blocks;
    const int64_t max_chunks = (G + 7) / 8;
    if (n_chunks > max_chunks) n_chunks = max_chunks;
    const int32_t chunk = (int32_t)((G + n_chunks - 1) / n_chunks);
    n_chunks = (G + chunk - 1) / chunk;
    hipLaunchKernelGGL(candidate_scores_kernel, dim3((unsigned)t_blocks, (unsigned)n_chunks), dim3(kCandBlock), 0, ctx->stream,
                       ctx->targets.as<double>() + first * 32, count, (int32_t)G, chunk, k_cap, s_pt.at(tb), s_row.at(tb), tol,
                       group_of ? s_grp.at(tb) : nullptr, ctx->cov_counts.as<unsigned long long>(),
                       first_k_out ? ctx->cov_entries.as<int32_t>() : nullptr);
    const hipError_t launch_err = hipGetLastError();
    if (kernel_ms_out) (void)hipEventRecord(ev1, ctx->stream);
    hipError_t err = launch_err;
    if (err == hipSuccess) err = hipMemcpyAsync(counts_out, ctx->cov_counts.p, (size_t)n_counts * sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream);
    if (err == hipSuccess && first_k_out)
        err = hipMemcpyAsync(first_k_out, ctx->cov_entries.p, (size_t)G * (size_t)count * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream);
    if (err == hipSuccess) err = hipStreamSynchronize(ctx->stream);
    if (kernel_ms_out) {
        float ms = 0.0f;
        if (err == hipSuccess) err = hipEventElapsedTime(&ms, ev0, ev1);
        *kernel_ms_out = (double)ms;
        (void)hipEventDestroy(ev0);
        (void)hipEventDestroy(ev1);
    }
    HIP_TRY(err);
    return SLAM_OK;
}

int slam_sample_haar(slam_ctx* ctx, uint64_t seed, int64_t first_index, int64_t n_targets) {
    if (!ctx) return fail(SLAM_ERR_INVALID, "ctx is NULL");
    if (n_targets <= 0 || n_targets > 0x7fffffffLL) return fail(SLAM_ERR_INVALID, "n_targets must be in 1..2^31-1");
    if (first_index < 0) return fail(SLAM_ERR_INVALID, "first_index < 0");
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(ctx->targets.reserve((size_t)n_targets * 32 * sizeof(double)));
    hipLaunchKernelGGL(haar_targets_kernel, dim3((unsigned)((n_targets + 127) / 128)), dim3(128), 0, ctx->stream,
                       ctx->targets.as<double>(), first_index, n_targets, seed);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    ctx->n_targets = n_targets;
    ctx->result_nmax = 0;
    ctx->result_filled = 0;
    return SLAM_OK;
}

int slam_sample_haar_indexed(slam_ctx* ctx, uint64_t seed, const int64_t* indices, int64_t n_targets) {
    if (!ctx) return fail(SLAM_ERR_INVALID, "ctx is NULL");
    if (n_targets <= 0 || n_targets > 0x7fffffffLL) return fail(SLAM_ERR_INVALID, "n_targets must be in 1..2^31-1");
    if (!indices) return fail(SLAM_ERR_INVALID, "indices is NULL");
    for (int64_t i = 0; i < n_targets; ++i)
        if (indices[i] < 0) return fail(SLAM_ERR_INVALID, "indices[%lld] < 0", (long long)i);
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(ctx->targets.reserve((size_t)n_targets * 32 * sizeof(double)));
    HIP_TRY(ctx->sel_indices.reserve((size_t)n_targets * sizeof(int64_t)));
    HIP_TRY(hipMemcpyAsync(ctx->sel_indices.p, indices, (size_t)n_targets * sizeof(int64_t), hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(haar_indexed_kernel, dim3((unsigned)((n_targets + 127) / 128)), dim3(128), 0, ctx->stream, ctx->targets.as<double>(),
                       ctx->sel_indices.as<int64_t>(), n_targets, seed);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    ctx->n_targets = n_targets;
    ctx->result_nmax = 0;
    ctx->result_filled = 0;
    return SLAM_OK;
}

int slam_haar_select_spans(slam_ctx* ctx, uint64_t seed, int64_t first_index, int64_t n_candidates, int k_max, const double* point,
                           const double* bounds, double tol, double margin, int32_t span_lo, int32_t span_hi, int64_t capacity,
                           int64_t* n_selected, int64_t* indices_out, int64_t* span_counts) {
    if (!ctx) return fail(SLAM_ERR_INVALID, "ctx is NULL");
    if (n_candidates < 0 || n_candidates > 0x7fffffffLL)
        return fail(SLAM_ERR_INVALID, "n_candidates must be in 0..2^31-1 (got %lld)", (long long)n_candidates);
    if (first_index < 0 || first_index > INT64_MAX - n_candidates) return fail(SLAM_ERR_INVALID, "first_index out of range (%lld)", (long long)first_index);
    if (k_max < 1 || k_max > SLAM_MAX_SPAN_EVAL) return fail(SLAM_ERR_INVALID, "k_max must be 1..%d (got %d)", SLAM_MAX_SPAN_EVAL, k_max);
    if (!point || (k_max > 1 && !bounds)) return fail(SLAM_ERR_INVALID, "point / bounds is NULL");
    if (!std::isfinite(tol)) return fail(SLAM_ERR_INVALID, "tol must be finite");
    if (!(margin >= 0.0) || !std::isfinite(margin)) return fail(SLAM_ERR_INVALID, "margin must be finite and >= 0 (got %g)", margin);
    if (span_lo > span_hi) return fail(SLAM_ERR_INVALID, "span_lo > span_hi (%d > %d)", span_lo, span_hi);
    if (span_lo < 0 || span_hi > k_max + 1) return fail(SLAM_ERR_INVALID, "spans must lie in 0..k_max + 1 = %d (got %d..%d)", k_max + 1, span_lo, span_hi);
    if (capacity < 0) return fail(SLAM_ERR_INVALID, "capacity < 0");
    if (!n_selected || (capacity > 0 && !indices_out)) return fail(SLAM_ERR_INVALID, "n_selected / indices_out is NULL");
    *n_selected = 0;
    if (n_candidates == 0) return SLAM_OK;
    static_assert(kSelBins == SLAM_MAX_SPAN_EVAL + 2, "one histogram bin per span, local and out of reach");
    HIP_TRY(hipSetDevice(ctx->device));
    const int64_t n_blocks = (n_candidates + kSelBlock - 1) / kSelBlock;
    const int64_t cap = capacity < n_candidates ? capacity : n_candidates;
    // sel_blocks: votes per block [n_blocks], their exclusive scan [n_blocks] (32 bits each), then the total (64 bits)
    Carver cv;
    const auto s_tot = cv.add<uint32_t>((size_t)n_blocks), s_scan = cv.add<uint32_t>((size_t)n_blocks);
    const auto s_sum = cv.add<unsigned long long>(1);
    HIP_TRY(ctx->sel_masks.reserve((size_t)n_blocks * kSelWaves * sizeof(unsigned long long)));
    HIP_TRY(ctx->sel_blocks.reserve(cv.total));
    HIP_TRY(ctx->sel_counts.reserve(kSelBins * sizeof(unsigned long long)));
    if (cap > 0) HIP_TRY(ctx->sel_indices.reserve((size_t)cap * sizeof(int64_t)));
    char* bl = ctx->sel_blocks.as<char>();
    HIP_TRY(hipMemsetAsync(ctx->sel_counts.p, 0, kSelBins * sizeof(unsigned long long), ctx->stream));
    const SpanRegions r = span_regions(k_max, point, bounds, tol);
    SelArgs a{};
    a.seed = seed;
    a.first_index = first_index;
    a.n = n_candidates;
    a.margin = margin;
    a.span_lo = span_lo;
    a.span_hi = span_hi;
    hipLaunchKernelGGL(haar_span_select_kernel, dim3((unsigned)n_blocks), dim3(kSelBlock), 0, ctx->stream, r, a,
                       ctx->sel_masks.as<unsigned long long>(), s_tot.at(bl), ctx->sel_counts.as<unsigned long long>());
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(span_scan_kernel, dim3(1), dim3(kScanBlock), 0, ctx->stream, s_tot.at(bl), n_blocks, s_scan.at(bl), s_sum.at(bl));
    HIP_TRY(hipGetLastError());
    if (cap > 0) {
        hipLaunchKernelGGL(span_scatter_kernel, dim3((unsigned)n_blocks), dim3(kSelBlock), 0, ctx->stream, ctx->sel_masks.as<unsigned long long>(),
                           s_scan.at(bl), first_index, cap, ctx->sel_indices.as<int64_t>());
        HIP_TRY(hipGetLastError());
    }
    unsigned long long total = 0, counts[kSelBins] = {0};
    HIP_TRY(hipMemcpyAsync(&total, s_sum.at(bl), sizeof(total), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipMemcpyAsync(counts, ctx->sel_counts.p, sizeof(counts), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    *n_selected = (int64_t)total;
    const int64_t copy = (int64_t)total < cap ? (int64_t)total : cap;
    if (copy > 0) {
        HIP_TRY(hipMemcpyAsync(indices_out, ctx->sel_indices.p, (size_t)copy * sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(hipStreamSynchronize(ctx->stream));
    }
    if (span_counts)
        for (int b = 0; b < k_max + 2; ++b) span_counts[b] += (int64_t)counts[b];
    return SLAM_OK;
}

int slam_get_targets(slam_ctx* ctx, int64_t first, int64_t count, double* out) {
    if (!ctx || !out) return fail(SLAM_ERR_INVALID, "NULL argument");
    if (int rc = check_window(ctx, first, count, false)) return rc;
    if (count == 0) return SLAM_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipMemcpyAsync(out, ctx->targets.as<double>() + first * 32, (size_t)count * 32 * sizeof(double),
                           hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return SLAM_OK;
}

// ---- parallel-drive coverage (slam_pd.hpp) ----------------------------------------------------------------------------------------
int slam_pd_sample(slam_ctx* ctx, double gc, double gg, double t, int32_t n_slices, int32_t k, double bound, uint64_t seed,
                   int64_t first_index, int64_t n_samples, const int64_t* indices, int ndigits, double* coords_out, double* params_out,
                   double* unitaries_out) {
    if (!ctx) return fail(SLAM_ERR_INVALID, "ctx is NULL");
    if (n_samples <= 0 || n_samples > 0x7fffffffLL) return fail(SLAM_ERR_INVALID, "n_samples must be in 1..2^31-1 (got %lld)", (long long)n_samples);
    if (!(t > 0.0) || !std::isfinite(t)) return fail(SLAM_ERR_INVALID, "t must be a finite positive pulse time (got %g)", t);
    if (!(bound > 0.0) || !std::isfinite(bound)) return fail(SLAM_ERR_INVALID, "bound must be finite and positive (got %g)", bound);
    if (!std::isfinite(gc) || !std::isfinite(gg)) return fail(SLAM_ERR_INVALID, "gc and gg must be finite");
    if (k < 1 || k > SLAM_PD_MAX_SPAN) return fail(SLAM_ERR_UNSUPPORTED, "k must be in 1..%d (got %d)", SLAM_PD_MAX_SPAN, k);
    if (n_slices < 1 || n_slices > SLAM_PD_MAX_SLICES)
        return fail(SLAM_ERR_UNSUPPORTED, "n_slices must be in 1..%d (got %d)", SLAM_PD_MAX_SLICES, n_slices);
    if (first_index < 0 || first_index > 0x7fffffffffffLL) return fail(SLAM_ERR_INVALID, "first_index out of range");
    if (indices)
        for (int64_t i = 0; i < n_samples; ++i)
            if (indices[i] < 0) return fail(SLAM_ERR_INVALID, "indices[%lld] < 0", (long long)i);
    if (!indices && first_index + n_samples > 0xffffffffLL) return fail(SLAM_ERR_INVALID, "sample indices beyond 2^32");
    static_assert(SLAM_PD_MAX_SPAN == kPdMaxSpan && SLAM_PD_MAX_SLICES == kPdMaxSlices, "slam_pd limits");
    HIP_TRY(hipSetDevice(ctx->device));
    PdSpec sp{};
    sp.gc = gc;
    sp.gg = gg;
    sp.tau = t / n_slices;
    sp.bound = bound;
    sp.n_slices = n_slices;
    sp.k = k;
    sp.n_params = 6 * (k - 1) + k * (2 + 2 * n_slices);
    sp.seed = seed;
    // staging: indices, then parameter rows, then unitaries
    Carver cv;
    const auto s_idx = cv.add<int64_t>(indices ? (size_t)n_samples : 0);
    const auto s_prm = cv.add<double>(params_out ? (size_t)n_samples * sp.n_params : 0);
    const auto s_uni = cv.add<double>(unitaries_out ? (size_t)n_samples * 32 : 0);
    HIP_TRY(ctx->pd_coords.reserve((size_t)n_samples * 3 * sizeof(double)));
    ctx->pd_n = 0;
    if (cv.total) HIP_TRY(ctx->pd_stage.reserve(cv.total));
    char* st = ctx->pd_stage.as<char>();
    if (indices) HIP_TRY(hipMemcpyAsync(s_idx.at(st), indices, s_idx.bytes, hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(pd_sample_kernel, dim3((unsigned)((n_samples + kPdBlock - 1) / kPdBlock)), dim3(kPdBlock), 0, ctx->stream, sp,
                       first_index, n_samples, indices ? s_idx.at(st) : nullptr, ndigits, ctx->pd_coords.as<double>(),
                       params_out ? s_prm.at(st) : nullptr, unitaries_out ? s_uni.at(st) : nullptr);
    HIP_TRY(hipGetLastError());
    if (coords_out)
        HIP_TRY(hipMemcpyAsync(coords_out, ctx->pd_coords.p, (size_t)n_samples * 3 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    if (params_out) HIP_TRY(hipMemcpyAsync(params_out, s_prm.at(st), s_prm.bytes, hipMemcpyDeviceToHost, ctx->stream));
    if (unitaries_out) HIP_TRY(hipMemcpyAsync(unitaries_out, s_uni.at(st), s_uni.bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    ctx->pd_n = n_samples;
    return SLAM_OK;
}

int slam_pd_extremes(slam_ctx* ctx, const double* directions, int32_t n_dirs, int64_t* index_out, double* coords_out) {
    if (!ctx) return fail(SLAM_ERR_INVALID, "ctx is NULL");
    if (ctx->pd_n <= 0) return fail(SLAM_ERR_STATE, "no resident samples: call slam_pd_sample first");
    if (n_dirs < 1 || n_dirs > SLAM_PD_MAX_DIRS) return fail(SLAM_ERR_INVALID, "n_dirs must be in 1..%d (got %d)", SLAM_PD_MAX_DIRS, n_dirs);
    if (!directions || !index_out || !coords_out) return fail(SLAM_ERR_INVALID, "NULL argument");
    for (int32_t d = 0; d < 3 * n_dirs; ++d)
        if (!std::isfinite(directions[d])) return fail(SLAM_ERR_INVALID, "directions must be finite");
    HIP_TRY(hipSetDevice(ctx->device));
    // staging: directions [n_dirs][3], keys [n_dirs], indices [n_dirs], coordinates [n_dirs][3]
    Carver cv;
    const auto s_dir = cv.add<double>((size_t)n_dirs * 3);
    const auto s_key = cv.add<unsigned long long>((size_t)n_dirs);
    const auto s_idx = cv.add<int64_t>((size_t)n_dirs);
    const auto s_crd = cv.add<double>((size_t)n_dirs * 3);
    HIP_TRY(ctx->pd_out.reserve(cv.total));
    char* b = ctx->pd_out.as<char>();
    HIP_TRY(hipMemcpyAsync(s_dir.at(b), directions, s_dir.bytes, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipMemsetAsync(s_key.at(b), 0, s_key.bytes, ctx->stream));
    const int64_t n = ctx->pd_n;
    hipLaunchKernelGGL(pd_extremes_kernel, dim3((unsigned)((n + kPdScanBlock - 1) / kPdScanBlock)), dim3(kPdScanBlock), 0, ctx->stream,
                       ctx->pd_coords.as<double>(), n, s_dir.at(b), n_dirs, s_key.at(b));
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(pd_gather_kernel, dim3((unsigned)((n_dirs + 63) / 64)), dim3(64), 0, ctx->stream, ctx->pd_coords.as<double>(),
                       s_key.at(b), n_dirs, s_idx.at(b), s_crd.at(b));
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(index_out, s_idx.at(b), s_idx.bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipMemcpyAsync(coords_out, s_crd.at(b), s_crd.bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return SLAM_OK;
}

int slam_pd_filter(slam_ctx* ctx, const double* facets, int32_t n_facets, double eps, int64_t capacity, int64_t* n_out, int64_t* index_out,
                   double* coords_out) {
    if (!ctx) return fail(SLAM_ERR_INVALID, "ctx is NULL");
    if (ctx->pd_n <= 0) return fail(SLAM_ERR_STATE, "no resident samples: call slam_pd_sample first");
    if (n_facets < 0 || n_facets > SLAM_PD_MAX_FACETS) return fail(SLAM_ERR_INVALID, "n_facets must be in 0..%d (got %d)", SLAM_PD_MAX_FACETS, n_facets);
    if (n_facets > 0 && !facets) return fail(SLAM_ERR_INVALID, "facets is NULL");
    if (!n_out || capacity < 0 || (capacity > 0 && (!index_out || !coords_out))) return fail(SLAM_ERR_INVALID, "bad output arguments");
    if (!(eps >= 0.0) || !std::isfinite(eps)) return fail(SLAM_ERR_INVALID, "eps must be finite and >= 0");
    for (int32_t f = 0; f < 4 * n_facets; ++f)
        if (!std::isfinite(facets[f])) return fail(SLAM_ERR_INVALID, "facets must be finite");
    HIP_TRY(hipSetDevice(ctx->device));
    const int64_t n = ctx->pd_n;
    // staging: facets [n_facets][4], the counter, indices [n], coordinates [n][3]
    Carver cv;
    const auto s_fac = cv.add<double>((size_t)n_facets * 4);
    const auto s_cnt = cv.add<unsigned int>(1);
    const auto s_idx = cv.add<int64_t>((size_t)n);
    const auto s_crd = cv.add<double>((size_t)n * 3);
    HIP_TRY(ctx->pd_out.reserve(cv.total));
    char* b = ctx->pd_out.as<char>();
    if (n_facets > 0) HIP_TRY(hipMemcpyAsync(s_fac.at(b), facets, s_fac.bytes, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipMemsetAsync(s_cnt.at(b), 0, s_cnt.bytes, ctx->stream));
    hipLaunchKernelGGL(pd_filter_kernel, dim3((unsigned)((n + kPdScanBlock - 1) / kPdScanBlock)), dim3(kPdScanBlock), 0, ctx->stream,
                       ctx->pd_coords.as<double>(), n, s_fac.at(b), n_facets, eps, s_cnt.at(b), s_idx.at(b), s_crd.at(b));
    HIP_TRY(hipGetLastError());
    unsigned int m = 0;
    HIP_TRY(hipMemcpyAsync(&m, s_cnt.at(b), sizeof(unsigned int), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    *n_out = (int64_t)m;
    const int64_t copy = (int64_t)m < capacity ? (int64_t)m : capacity;
    if (copy > 0) {
        HIP_TRY(hipMemcpyAsync(index_out, s_idx.at(b), (size_t)copy * sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(hipMemcpyAsync(coords_out, s_crd.at(b), (size_t)copy * 3 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(hipStreamSynchronize(ctx->stream));
    }
    return SLAM_OK;
}

int slam_region_lookup(slam_ctx* ctx, int64_t first, int64_t count, int32_t n_regions, const int32_t* region_offsets, const int32_t* kinds,
                       const int32_t* facet_offsets, const double* facets, const double* aux, double tol, int64_t* counts_out) {
    if (!ctx) return fail(SLAM_ERR_INVALID, "ctx is NULL");
    if (int rc = check_window(ctx, first, count, true)) return rc;
    if (n_regions < 1 || n_regions > SLAM_REGION_MAX) return fail(SLAM_ERR_INVALID, "n_regions must be in 1..%d (got %d)", SLAM_REGION_MAX, n_regions);
    if (!region_offsets || !counts_out) return fail(SLAM_ERR_INVALID, "region_offsets / counts_out is NULL");
    if (!std::isfinite(tol)) return fail(SLAM_ERR_INVALID, "tol must be finite");
    if (region_offsets[0] != 0) return fail(SLAM_ERR_INVALID, "region_offsets[0] must be 0");
    for (int32_t r = 0; r < n_regions; ++r)
        if (region_offsets[r + 1] < region_offsets[r] || region_offsets[r + 1] > 0x00ffffff)
            return fail(SLAM_ERR_INVALID, "region_offsets must be non-decreasing and below 2^24");
    const int32_t P = region_offsets[n_regions];
    if (P > 0 && (!kinds || !facet_offsets)) return fail(SLAM_ERR_INVALID, "kinds / facet_offsets is NULL");
    bool need_aux = false;
    for (int32_t p = 0; p < P; ++p) {
        if (kinds[p] < 0 || kinds[p] > 2) return fail(SLAM_ERR_INVALID, "kinds[%d] = %d (0 facets, 1 coverage bounds, 2 one gate)", p, kinds[p]);
        need_aux = need_aux || kinds[p] != 0;
    }
    if (P > 0 && facet_offsets[0] != 0) return fail(SLAM_ERR_INVALID, "facet_offsets[0] must be 0");
    for (int32_t p = 0; p < P; ++p)
        if (facet_offsets[p + 1] < facet_offsets[p] || facet_offsets[p + 1] > 0x00ffffff)
            return fail(SLAM_ERR_INVALID, "facet_offsets must be non-decreasing and below 2^24");
    const int64_t F = P > 0 ? facet_offsets[P] : 0;
    if (F > 0 && !facets) return fail(SLAM_ERR_INVALID, "facets is NULL");
    if (need_aux && !aux) return fail(SLAM_ERR_INVALID, "aux is NULL");
    const int64_t n_counts = 2 * (int64_t)n_regions + 1;
    std::memset(counts_out, 0, (size_t)n_counts * sizeof(int64_t));
    if (count == 0) return SLAM_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    // one upload: region offsets, kinds, facet offsets (int32), then facets [F][4] and aux [P][14] (doubles)
    Carver cv;
    const auto s_ro = cv.add<int32_t>((size_t)n_regions + 1), s_ki = cv.add<int32_t>((size_t)P), s_fo = cv.add<int32_t>((size_t)P + 1);
    const auto s_fa = cv.add<double>((size_t)F * 4), s_ax = cv.add<double>((size_t)P * kSpanPatterns);
    HIP_TRY(ctx->reg_table.reserve(cv.total));
    HIP_TRY(ctx->reg_counts.reserve((size_t)n_counts * sizeof(unsigned long long)));
    char* tb = ctx->reg_table.as<char>();
    HIP_TRY(hipMemcpyAsync(s_ro.at(tb), region_offsets, s_ro.bytes, hipMemcpyHostToDevice, ctx->stream));
    if (P > 0) {
        HIP_TRY(hipMemcpyAsync(s_ki.at(tb), kinds, s_ki.bytes, hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(hipMemcpyAsync(s_fo.at(tb), facet_offsets, s_fo.bytes, hipMemcpyHostToDevice, ctx->stream));
        if (F > 0) HIP_TRY(hipMemcpyAsync(s_fa.at(tb), facets, s_fa.bytes, hipMemcpyHostToDevice, ctx->stream));
        if (aux) HIP_TRY(hipMemcpyAsync(s_ax.at(tb), aux, s_ax.bytes, hipMemcpyHostToDevice, ctx->stream));
    }
    HIP_TRY(hipMemsetAsync(ctx->reg_counts.p, 0, (size_t)n_counts * sizeof(unsigned long long), ctx->stream));
    static_assert(SLAM_REGION_MAX == kRegionMax, "region table size");
    hipLaunchKernelGGL(region_lookup_kernel, dim3((unsigned)((count + kRegionBlock - 1) / kRegionBlock)), dim3(kRegionBlock), 0, ctx->stream,
                       ctx->targets.as<double>() + first * 32, count, n_regions, s_ro.at(tb), s_ki.at(tb), s_fo.at(tb), s_fa.at(tb), s_ax.at(tb),
                       tol, ctx->reg_counts.as<unsigned long long>());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(counts_out, ctx->reg_counts.p, (size_t)n_counts * sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return SLAM_OK;
}

}  // extern "C"
