// slam_hip.hip -- host side of libslamhip.so, core unit: error state, contexts, the fixed-gate templates and the decompose family
// (slam_v2_host.hip, slam_smush_host.hip, slam_geometry.hip and slam_comm.hip hold the other families; slam_host.hpp what they share).
// The C ABI is declared in include/slam_hip.h.
// gfx950 only; no torch, no CUDA compatibility layer.
#include "slam_host.hpp"
#define SLAM_STAGE_KERNELS  // this unit emits the bookkeeping kernels of slam_kernels.hpp
#include "slam_kernels.hpp"
#include "slam_long_kernels.hpp"

namespace {

thread_local std::string g_err;

}  // namespace

int fail(int code, const char* fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

// slam_comm.hip reports its errors through the same thread-local message (library-internal, not exported)
extern "C" __attribute__((visibility("hidden"))) void slam_set_last_error(const char* msg) { g_err = msg ? msg : ""; }

// Every API call leaves the context's stream drained: the per-span gate slots, the pinned staging buffers and
// DevBuf::reserve's hipFree rely on it.  A call that fails after it has enqueued work therefore waits for that work
// (ignoring the result: the error being reported is the first one) and forgets the cached gate slots.
int drained(slam_ctx* c, int rc) {
    if (rc != SLAM_OK && c && c->stream) {
        const std::string keep = g_err;
        (void)hipSetDevice(c->device);
        (void)hipStreamSynchronize(c->stream);
        for (hipStream_t st : c->spec_stream)
            if (st) (void)hipStreamSynchronize(st);
        for (const auto& h : c->helper)
            if (h && h->stream) (void)hipStreamSynchronize(h->stream);
        (void)hipGetLastError();
        for (auto& st : c->staged) st.valid = false;
        g_err = keep;
    }
    return rc;
}

namespace {

template <int K, int GC>
constexpr size_t lds_bytes() { return sizeof(double) * lds_doubles<K, GC>(); }

// copy G_1..G_K of this span, in order, into the context's small device buffer (stream-ordered)
int stage_gates(slam_ctx* c, int k, const int32_t* gate_seq, const double** d_out) {
    // One device slot per span k, cached: as long as the gate table and the span's sequence do not change (the
    // normal case: one basis, many batches) nothing is copied -- a copy inside the span loop's chain of kernels
    // costs as much as a kernel there (it waits its turn on a busy GPU).  Every API call ends with the stream
    // drained, so a slot is never rewritten under a running kernel.  The host side of a slot is pinned: a copy
    // from pageable memory would make the calling thread wait (spinning) for everything enqueued before it.
    double* dst = c->span_gates.as<double>() + (size_t)k * SLAM_MAX_SPAN_EVAL * 32;
    *d_out = dst;
    slam_ctx::StagedSeq& st = c->staged[k];
    if (st.valid && std::memcmp(st.seq, gate_seq, (size_t)k * sizeof(int32_t)) == 0) return SLAM_OK;
    double* tmp = c->h_gates + (size_t)k * SLAM_MAX_SPAN_EVAL * 32;
    for (int j = 0; j < k; ++j) std::memcpy(tmp + 32 * j, c->gates_host.data() + (size_t)gate_seq[j] * 32, 32 * sizeof(double));
    HIP_TRY(hipMemcpyAsync(dst, tmp, (size_t)k * 32 * sizeof(double), hipMemcpyHostToDevice, c->stream));
    std::memcpy(st.seq, gate_seq, (size_t)k * sizeof(int32_t));
    st.valid = true;
    return SLAM_OK;
}

// Structure class of the gates of one span (see slam_device.hpp: GC_*).  A launch uses the most
// general class any of its gates needs; entries below 1e-15 count as structural zeros.
int classify_gates(slam_ctx* c, int k, const int32_t* gate_seq) {
    const double tol = 1e-15;
    bool all_cx = true, all_x = true, all_xri = true, all_xri1 = true;
    for (int j = 0; j < k; ++j) {
        const double* g = c->gates_host.data() + (size_t)gate_seq[j] * 32;
        auto re = [&](int r, int s) { return g[(r * 4 + s) * 2]; };
        auto im = [&](int r, int s) { return g[(r * 4 + s) * 2 + 1]; };
        auto mag = [&](int r, int s) { return std::fabs(re(r, s)) + std::fabs(im(r, s)); };
        // qiskit CXGate: ones at (0,0), (1,3), (2,2), (3,1)
        bool cx = true;
        for (int r = 0; r < 4; ++r)
            for (int s = 0; s < 4; ++s) {
                const bool one = (r == 0 && s == 0) || (r == 1 && s == 3) || (r == 2 && s == 2) || (r == 3 && s == 1);
                if (std::fabs(re(r, s) - (one ? 1.0 : 0.0)) > tol || std::fabs(im(r, s)) > tol) cx = false;
            }
        all_cx = all_cx && cx;
        // X shape: non-zeros only inside the blocks on index pairs (0,3) and (1,2)
        bool x = true;
        for (int r = 0; r < 4; ++r)
            for (int s = 0; s < 4; ++s) {
                const bool inside = ((r == 0 || r == 3) && (s == 0 || s == 3)) || ((r == 1 || r == 2) && (s == 1 || s == 2));
                if (!inside && mag(r, s) > tol) x = false;
            }
        all_x = all_x && x;
        const bool xri = x && std::fabs(im(0, 0)) <= tol && std::fabs(im(3, 3)) <= tol && std::fabs(im(1, 1)) <= tol &&
                         std::fabs(im(2, 2)) <= tol && std::fabs(re(0, 3)) <= tol && std::fabs(re(3, 0)) <= tol &&
                         std::fabs(re(1, 2)) <= tol && std::fabs(re(2, 1)) <= tol;
        all_xri = all_xri && xri;
        // ... and the identity on the (0,3) block: RiSwapGate(alpha) (sqrt-iSWAP, iSWAP) leaves |00> and |11> alone
        all_xri1 = all_xri1 && xri && std::fabs(re(0, 0) - 1.0) <= tol && std::fabs(re(3, 3) - 1.0) <= tol && mag(0, 3) <= tol &&
                   mag(3, 0) <= tol;
    }
    if (all_cx) return GC_CX;
    if (all_xri1) return GC_XRI1;
    if (all_xri) return GC_XRI;
    if (all_x) return GC_XGEN;
    return GC_DENSE;
}

// f(std::integral_constant<int, GC_...>{}) for the structure class gc: the one place the classes are enumerated
template <class F>
int with_gate_class(int gc, F&& f) {
    if (gc == GC_CX) return f(std::integral_constant<int, GC_CX>{});
    if (gc == GC_XRI1) return f(std::integral_constant<int, GC_XRI1>{});
    if (gc == GC_XRI) return f(std::integral_constant<int, GC_XRI>{});
    if (gc == GC_XGEN) return f(std::integral_constant<int, GC_XGEN>{});
    return f(std::integral_constant<int, GC_DENSE>{});
}

template <int K, class Kernel>
int launch_eval(slam_ctx* c, Kernel kernel, size_t lds, const int32_t* gate_seq, const double* d_x, const int32_t* d_tof, int64_t M, double* d_loss,
                double* d_grad, double* d_unitary) {
    { int rc = kernel_per_cu(c, reinterpret_cast<const void*>(kernel), lds, nullptr); if (rc) return rc; }
    EvalArgs<K> a{};
    a.targets = c->targets.as<double>();
    a.x = d_x;
    a.target_of = d_tof;
    a.n_items = M;
    a.loss = d_loss;
    a.grad = d_grad;
    a.unitary = d_unitary;
    a.cost_kind = c->cost_kind;
    { int rc = stage_gates(c, K, gate_seq, &a.gates); if (rc) return rc; }
    const int64_t blocks = (M + kQuadsPerWave - 1) / kQuadsPerWave;
    hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(kWave), lds, c->stream, a);
    HIP_TRY(hipGetLastError());
    return SLAM_OK;
}

// the span's eval kernel; MakhlinFunctionalCost: the dense gate class whatever the gates' structure (one instantiation per span)
template <int K>
int launch_eval_gc(slam_ctx* c, int gc, const int32_t* gate_seq, const double* d_x, const int32_t* d_tof, int64_t M, double* d_loss, double* d_grad,
                   double* d_unitary) {
    if (c->cost_kind == SLAM_COST_MAKHLIN)
        return launch_eval<K>(c, &eval_mk_kernel<K>, lds_bytes<K, GC_DENSE>(), gate_seq, d_x, d_tof, M, d_loss, d_grad, d_unitary);
    return with_gate_class(gc, [&](auto g) -> int {
        constexpr int GC = decltype(g)::value;
        return launch_eval<K>(c, &eval_kernel<K, GC>, lds_bytes<K, GC>(), gate_seq, d_x, d_tof, M, d_loss, d_grad, d_unitary);
    });
}

struct StageLaunch {
    double exit_loss;               // a finished restart below this pre-empts its siblings
    const int32_t* gate_seq;
    const double* d_stage_targets;  // [n_active][32]
    const int32_t* d_active;        // original target index per slot, or nullptr = first_target + slot
    int32_t first_target;
    const double* d_x0;
    int64_t n_items_max;            // upper bound (grid sizing); the kernel reads the real count from ctl
    const slam_opt_params* prm;
    StageCtl* ctl;
};

// the optimizer kernel's argument block for one stage of one context
template <int K>
int build_minimize_args(slam_ctx* c, const StageLaunch& sl, MinimizeArgs<K>& a) {
    const slam_opt_params* prm = sl.prm;
    a = MinimizeArgs<K>{};
    fill_stage_common(a, c, prm, sl.exit_loss);
    a.targets = sl.d_stage_targets;
    a.orig = sl.d_active;
    a.first_target = sl.first_target;
    a.x0 = sl.d_x0;
    a.ctl = sl.ctl;
    if (prm->flags & SLAM_FLAG_NO_EXTERIOR) a.flags |= kFlagNoExterior;  // (the upper bits are internal: kFlagTrace, kFlagNoExterior)
    if (a.trace_loss) a.flags |= kFlagTrace;
    a.items_per_quad = prm->items_per_quad;
    { int rc = stage_gates(c, K, sl.gate_seq, &a.gates); if (rc) return rc; }
    return SLAM_OK;
}

// The per-span optimizer launch of spans 1..SLAM_MAX_SPAN_QUAD (minimize_kernel<K, GC>, minimize_mk_kernel<K>): the kernel's
// argument block, then whatever the kernel takes after it (tail).
template <int K, class Kernel, class... Tail>
int launch_persistent(slam_ctx* c, const StageLaunch& sl, Kernel kernel, size_t lds, Tail... tail) {
    int per_cu = 0;
    { int rc = kernel_per_cu(c, reinterpret_cast<const void*>(kernel), lds, &per_cu); if (rc) return rc; }
    const slam_opt_params* prm = sl.prm;
    MinimizeArgs<K> a;
    { int rc = build_minimize_args<K>(c, sl, a); if (rc) return rc; }
    // persistent wavefronts: never more blocks than can be resident, every quad pulls items.  The grid is
    // sized for the upper bound of the item count; the kernel derives the real launch shape (waves that
    // take part, chunk size) from the device-side target count and surplus waves exit at once.
    int64_t blocks = (sl.n_items_max + kQuadsPerWave - 1) / kQuadsPerWave;
    if (prm->items_per_quad > 1) {
        blocks = (sl.n_items_max + (int64_t)kQuadsPerWave * prm->items_per_quad - 1) / ((int64_t)kQuadsPerWave * prm->items_per_quad);
        if (blocks < 1) blocks = 1;
    }
    // leave a few wavefront slots free: with several batches in flight the bookkeeping kernels of the other streams
    // (reduce / compaction / epilogue) otherwise wait for the tail of this stage before they can even start
    const int64_t resident = (int64_t)per_cu * c->compute_units;
    const int64_t cap = resident - c->reserve_waves > 0 ? resident - c->reserve_waves : 1;
    if (blocks > cap) blocks = cap;
    HIP_TRY(hipEventRecord(c->ev_a[K], c->stream));
    hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(kWave), lds, c->stream, a, tail...);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(c->ev_b[K], c->stream));
    return SLAM_OK;
}

// MakhlinFunctionalCost: the dense gate class whatever the gates' structure
template <int K>
int launch_minimize_gc(slam_ctx* c, int gc, const StageLaunch& sl) {
    if (c->cost_kind == SLAM_COST_MAKHLIN) return launch_persistent<K>(c, sl, &minimize_mk_kernel<K>, lds_bytes<K, GC_DENSE>());
    return with_gate_class(gc, [&](auto g) -> int {
        constexpr int GC = decltype(g)::value;
        return launch_persistent<K>(c, sl, &minimize_kernel<K, GC>, lds_bytes<K, GC>(), (const MinimizeArgs<K>*)nullptr, 0);
    });
}

// templates of SLAM_MAX_SPAN_QUAD + 1 .. SLAM_MAX_SPAN_MINIMIZE gates: one wavefront per item (slam_long.hpp)
int launch_minimize_long(slam_ctx* c, const StageLaunch& sl, int k) {
    const bool mk = c->cost_kind == SLAM_COST_MAKHLIN;
    const void* kern = mk ? reinterpret_cast<const void*>(&minimize_long_mk_kernel) : reinterpret_cast<const void*>(&minimize_long_kernel);
    int per_cu = 0;
    { int rc = kernel_per_cu(c, kern, kLongLdsBytes, &per_cu); if (rc) return rc; }
    const int64_t resident = (int64_t)per_cu * c->compute_units;
    const slam_opt_params* prm = sl.prm;
    LongArgs a{};
    fill_stage_common(a, c, prm, sl.exit_loss);
    a.targets = sl.d_stage_targets;
    a.orig = sl.d_active;
    a.first_target = sl.first_target;
    a.x0 = sl.d_x0;
    a.ctl = sl.ctl;
    if (prm->flags & SLAM_FLAG_NO_EXTERIOR) a.flags |= kFlagNoExterior;
    a.k = k;
    { int rc = stage_gates(c, k, sl.gate_seq, &a.gates); if (rc) return rc; }
    int64_t blocks = sl.n_items_max;  // one item per wavefront at a time
    if (blocks > resident) blocks = resident;
    if (blocks < 1) blocks = 1;
    // (sized for the whole grid and the longest template once: growing it between two stages of a chain would free it under the stage in flight)
    HIP_TRY(c->long_hmem.reserve((size_t)resident * (size_t)(6 * (SLAM_MAX_SPAN_MINIMIZE + 1)) * kLongHStride * sizeof(float)));
    a.hmem = c->long_hmem.as<float>();
    HIP_TRY(hipEventRecord(c->ev_a[k], c->stream));
    if (mk) hipLaunchKernelGGL(minimize_long_mk_kernel, dim3((unsigned)blocks), dim3(kWave), kLongLdsBytes, c->stream, a);
    else hipLaunchKernelGGL(minimize_long_kernel, dim3((unsigned)blocks), dim3(kWave), kLongLdsBytes, c->stream, a);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(c->ev_b[k], c->stream));
    return SLAM_OK;
}

int launch_eval_long(slam_ctx* c, int k, const int32_t* gate_seq, const double* d_x, const int32_t* d_tof, int64_t M, double* d_loss, double* d_grad,
                     double* d_unitary) {
    const bool mk = c->cost_kind == SLAM_COST_MAKHLIN;
    const void* kern = mk ? reinterpret_cast<const void*>(&eval_long_mk_kernel) : reinterpret_cast<const void*>(&eval_long_kernel);
    { int rc = kernel_per_cu(c, kern, kLongLdsBytes, nullptr); if (rc) return rc; }
    LongEvalArgs a{};
    a.targets = c->targets.as<double>();
    a.x = d_x;
    a.target_of = d_tof;
    a.n_items = M;
    a.loss = d_loss;
    a.grad = d_grad;
    a.unitary = d_unitary;
    a.cost_kind = c->cost_kind;
    a.k = k;
    { int rc = stage_gates(c, k, gate_seq, &a.gates); if (rc) return rc; }
    int64_t blocks = M;
    const int64_t cap = (int64_t)8 * c->compute_units;
    if (blocks > cap) blocks = cap;
    if (mk) hipLaunchKernelGGL(eval_long_mk_kernel, dim3((unsigned)blocks), dim3(kWave), kLongLdsBytes, c->stream, a);
    else hipLaunchKernelGGL(eval_long_kernel, dim3((unsigned)blocks), dim3(kWave), kLongLdsBytes, c->stream, a);
    HIP_TRY(hipGetLastError());
    return SLAM_OK;
}

int check_gate_seq(slam_ctx* c, int k, const int32_t* gate_seq) {
    if (!gate_seq) return fail(SLAM_ERR_INVALID, "gate_seq is NULL");
    for (int j = 0; j < k; ++j)
        if (gate_seq[j] < 0 || gate_seq[j] >= c->n_gates)
            return fail(SLAM_ERR_INVALID, "gate_seq[%d] = %d outside the gate table (n_gates = %d)", j,
                        gate_seq[j], c->n_gates);
    return SLAM_OK;
}

}  // namespace

int check_params(const slam_opt_params* p) {
    if (!p) return fail(SLAM_ERR_INVALID, "params is NULL");
    if (p->restarts <= 0) return fail(SLAM_ERR_INVALID, "restarts must be > 0 (got %d)", p->restarts);
    if (p->maxiter < 0 || p->maxiter > SLAM_MAX_MAXITER)
        return fail(SLAM_ERR_INVALID, "maxiter must be in 0..%d (got %d)", SLAM_MAX_MAXITER, p->maxiter);
    if (p->target_base < 0 || p->target_base > 0x7fffffffLL) return fail(SLAM_ERR_INVALID, "target_base out of range");
    return SLAM_OK;
}

namespace {

// Work buffers of a stage with at most n_upper targets at span <= k_max.
int reserve_stage_buffers(slam_ctx* c, int64_t n_upper, int k_max, const slam_opt_params* prm) {
    const int n = 6 * (k_max + 1);
    const int64_t M = n_upper * (int64_t)prm->restarts;
    if (M > 0x7fff0000LL) return fail(SLAM_ERR_INVALID, "too many work items in one stage (%lld)", (long long)M);
    HIP_TRY(c->item_rec.reserve(M * sizeof(ItemRec)));
    HIP_TRY(c->item_x.reserve(M * n * sizeof(double)));
    HIP_TRY(c->stage_loss.reserve(n_upper * sizeof(double)));
    HIP_TRY(c->stage_x.reserve(n_upper * n * sizeof(double)));
    HIP_TRY(c->stage_restart.reserve(n_upper * sizeof(int32_t)));
    HIP_TRY(c->solved.reserve(n_upper * sizeof(int32_t)));
    HIP_TRY(c->stage_targets.reserve((size_t)n_upper * 32 * sizeof(double)));
    return SLAM_OK;
}

// Enqueues one span stage for the device-resident active list (d_active may be nullptr = identity): stage
// inputs, the optimizer kernel, the per-target reduction and (merge) the span loop's bookkeeping.  No host
// synchronisation: the stage's target count lives in its control block (stage_ctl(c, k)->n_active, at most
// n_upper), which must have been zeroed and published on the stream before.  Leaves per-slot results in
// ctx->stage_loss / stage_x / stage_restart and the per-item arrays.  loop: what follows the optimizer kernel inside the span loop
// (nullptr: single-stage call, reduce only).
int enqueue_stage(slam_ctx* c, int k, const int32_t* gate_seq, const int32_t* d_active, int64_t n_upper,
                  const double* d_x0, const slam_opt_params* prm, const SpanLoopStep* loop) {
    const int n = 6 * (k + 1);
    const int64_t M = n_upper * (int64_t)prm->restarts;
    if (M <= 0) return SLAM_OK;
    StageCtl* ctl = stage_ctl(c, k);
    const bool merge = loop != nullptr;
    if (!(loop && loop->inputs_ready)) {
        const int64_t nt = n_upper * 16;
        hipLaunchKernelGGL(stage_prepare_kernel, dim3((unsigned)((nt + 255) / 256)), dim3(256), 0, c->stream,
                           c->targets.as<double>(), d_active, ctl, c->stage_targets.as<double>(), c->solved.as<int32_t>());
        HIP_TRY(hipGetLastError());
    }
    const double* d_stage_targets = d_active ? c->stage_targets.as<double>() : c->targets.as<double>();
    // which finished restart stops its siblings: in ordered mode the one the reference's loop breaks at -- best
    // result below the success threshold (optimizer.py:287) -- otherwise one that reached stop_loss
    const double exit_loss = ((prm->flags & SLAM_FLAG_ORDERED) && loop) ? loop->exit_loss
                             : (((prm->flags & SLAM_FLAG_ORDERED) && c->stage_exit_loss >= 0.0) ? c->stage_exit_loss : prm->stop_loss);
    StageLaunch sl{exit_loss, gate_seq, d_stage_targets, d_active, 0, d_x0, M, prm, ctl};
    int rc;
    const int gc = classify_gates(c, k, gate_seq);
    static_assert(SLAM_MAX_SPAN_QUAD == 5, "one case per quad-per-item span");
    switch (k) {
        case 1: rc = launch_minimize_gc<1>(c, gc, sl); break;
        case 2: rc = launch_minimize_gc<2>(c, gc, sl); break;
        case 3: rc = launch_minimize_gc<3>(c, gc, sl); break;
        case 4: rc = launch_minimize_gc<4>(c, gc, sl); break;
        case 5: rc = launch_minimize_gc<5>(c, gc, sl); break;
        default:
            if (k < 1 || k > SLAM_MAX_SPAN_MINIMIZE) return fail(SLAM_ERR_UNSUPPORTED, "minimize supports spans 1..%d (got %d)", SLAM_MAX_SPAN_MINIMIZE, k);
            rc = launch_minimize_long(c, sl, k);  // SLAM_MAX_SPAN_QUAD < k: one wavefront per item
            break;
    }
    if (rc != SLAM_OK) return rc;

    const ReduceArgs r = build_reduce_args(c, k, n, d_active, prm, exit_loss, merge);
    if (loop) {
        const EpilogueArgs e = build_epilogue_args(c, k, r, *loop);
        return enqueue_stage_epilogue(c, n_upper, e);
    }
    // single-stage call: per-target reduction only
    const int rb = 256;
    hipLaunchKernelGGL(reduce_merge_kernel, dim3((unsigned)((n_upper + rb - 1) / rb)), dim3(rb), 0, c->stream, r);
    HIP_TRY(hipGetLastError());
    return SLAM_OK;
}

}  // namespace

// The counters of the control blocks h_ctl[k_min..k_max] added to the statistics.  Which blocks are left out is the caller's rule:
// none; the stages that had no targets; of those, only the ones that counted no evaluation either (the one-launch loops).
enum FoldSkip { FOLD_ALL, FOLD_SKIP_IDLE, FOLD_SKIP_IDLE_UNEVALUATED };
static void fold_counters(slam_stats& s, const StageCtl* h_ctl, int k_min, int k_max, int restarts, FoldSkip skip) {
    for (int k = k_min; k <= k_max; ++k) {
        const bool idle = h_ctl[k].n_active <= 0;
        if ((skip == FOLD_SKIP_IDLE && idle) || (skip == FOLD_SKIP_IDLE_UNEVALUATED && idle && h_ctl[k].evals == 0)) continue;
        s.evals[k] += (int64_t)h_ctl[k].evals;
        s.evals_accepted[k] += (int64_t)h_ctl[k].evals_accepted;
        s.evals_preempted[k] += (int64_t)h_ctl[k].evals_preempted;
        s.wave_rounds[k] += (int64_t)h_ctl[k].rounds;
        s.items[k] += (int64_t)h_ctl[k].n_active * restarts;
    }
}

// ---- shared with the other units (slam_host.hpp) ----
// After the stream has drained: fold the stages' control blocks and kernel brackets into the statistics.
int collect_stats(slam_ctx* c, int k_min, int k_max, const StageCtl* h_ctl, int restarts) {
    for (int k = k_min; k <= k_max; ++k) {
        if (h_ctl[k].n_active <= 0) continue;
        float ms = 0.f;
        HIP_TRY(hipEventElapsedTime(&ms, c->ev_a[k], c->ev_b[k]));
        c->stats.kernel_ms += ms;
        c->stats.kernel_ms_span[k] += ms;
        c->stats.kernel_launches += 1;
    }
    fold_counters(c->stats, h_ctl, k_min, k_max, restarts, FOLD_SKIP_IDLE);
    return SLAM_OK;
}

int enqueue_loop_end(slam_ctx* c, FetchReq* fetch, int nmax, int64_t first, int64_t count) {
    HIP_TRY(hipEventRecord(c->ev_t1, c->stream));
    if (fetch) {  // the results ride on the same wait as the span loop
        const int rc = enqueue_fetch_n(c, nmax, first, count, *fetch);
        if (rc) return rc;
    }
    HIP_TRY(hipMemcpyAsync(c->h_ctl, c->counters.p, sizeof(StageCtl) * (SLAM_MAX_SPAN_EVAL + 2), hipMemcpyDeviceToHost, c->stream));
    return SLAM_OK;
}

int wait_loop_end(slam_ctx* c, const FetchReq* fetch) {
    HIP_TRY(hipEventRecord(c->ev_done, c->stream));
    HIP_TRY(hipEventSynchronize(c->ev_done));  // sleep until the chain is done
    if (fetch) finish_fetch(c, *fetch);
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, c->ev_t0, c->ev_t1));
    c->stats.total_ms = ms;
    return SLAM_OK;
}

ReduceArgs build_reduce_args(slam_ctx* c, int k, int n, const int32_t* d_active, const slam_opt_params* prm, double exit_loss, bool merge) {
    ReduceArgs r{};
    r.slot_ev = (!merge && c->slot_ev_on) ? c->slot_ev.as<unsigned long long>() : nullptr;
    r.item_rec = c->item_rec.as<ItemRec>();
    r.item_x = c->item_x.as<double>();
    r.exit_loss = exit_loss;
    r.ordered = ((prm->flags & SLAM_FLAG_EARLY_EXIT) && (prm->flags & SLAM_FLAG_ORDERED)) ? 1 : 0;
    r.ctl = stage_ctl(c, k);
    r.restarts = prm->restarts;
    r.n = n;
    r.stage_loss = c->stage_loss.as<double>();
    r.stage_x = c->stage_x.as<double>();
    r.stage_restart = c->stage_restart.as<int32_t>();
    if (merge) {
        r.active = d_active;
        r.nmax = c->result_nmax;
        r.k = k;
        r.best_loss = c->best_loss.as<double>();
        r.best_x = c->best_x.as<double>();
        r.best_cycles = c->best_cycles.as<int32_t>();
        r.span_loss = c->span_loss.as<double>();
    }
    return r;
}

EpilogueArgs build_epilogue_args(slam_ctx* c, int k, const ReduceArgs& r, const SpanLoopStep& loop) {
    EpilogueArgs e{};
    e.r = r;
    e.has_next = loop.has_next ? 1 : 0;
    e.threshold = loop.threshold;
    e.active_out = loop.active_out;
    e.next = stage_ctl(c, k + 1);
    e.targets = c->targets.as<double>();
    e.stage_targets = c->stage_targets.as<double>();
    e.solved = c->solved.as<int32_t>();
    return e;
}

static int ensure_results(slam_ctx* c, int k_max) { return ensure_results_n(c, 6 * (k_max + 1)); }
int ensure_results_n(slam_ctx* c, int nmax) {
    const void* p0 = c->best_loss.p;
    const void* p1 = c->best_cycles.p;
    HIP_TRY(c->best_loss.reserve(c->n_targets * sizeof(double)));
    HIP_TRY(c->best_x.reserve(c->n_targets * (size_t)nmax * sizeof(double)));
    HIP_TRY(c->best_cycles.reserve(c->n_targets * sizeof(int32_t)));
    HIP_TRY(c->span_loss.reserve(c->n_targets * (size_t)kSpanLossStride * sizeof(double)));
    if (c->result_nmax != nmax || c->result_filled != c->n_targets || p0 != c->best_loss.p || p1 != c->best_cycles.p) {
        // new batch, new row width or new allocation: every target starts as "nothing found yet", so that a
        // window no call has decomposed reads as (+inf, -1) instead of uninitialised memory
        hipLaunchKernelGGL(fill_results_kernel, dim3((unsigned)((c->n_targets + 255) / 256)), dim3(256), 0, c->stream,
                           c->best_loss.as<double>(), c->best_cycles.as<int32_t>(), c->span_loss.as<double>(), c->n_targets);
        HIP_TRY(hipGetLastError());
        c->result_filled = c->n_targets;
    }
    c->result_nmax = nmax;
    return SLAM_OK;
}

static int enqueue_fetch(slam_ctx* ctx, int k_layout, int64_t first, int64_t count, FetchReq& fr) {
    return enqueue_fetch_n(ctx, 6 * (k_layout + 1), first, count, fr);
}
int enqueue_fetch_n(slam_ctx* ctx, int nmax, int64_t first, int64_t count, FetchReq& fr) {
    if (ctx->result_nmax != nmax || ctx->n_targets <= 0)
        return fail(SLAM_ERR_STATE, "no resident results with rows of %d parameters", nmax);
    if (first < 0 || count < 0 || first + count > ctx->n_targets)
        return fail(SLAM_ERR_INVALID, "target window outside the resident batch");
    const size_t N = (size_t)count;
    const size_t o = (size_t)first;
    fr.b_loss = N * sizeof(double);
    fr.b_x = N * nmax * sizeof(double);
    fr.b_cyc = N * sizeof(int32_t);
    if (N == 0) return SLAM_OK;
    const size_t need = fr.b_loss + fr.b_x + fr.b_cyc;
    char* h = nullptr;
    if (need <= (size_t)1 << 20) {
        if (need > ctx->h_stage.cap) HIP_TRY(ctx->h_stage.reserve(need + need / 4));
        h = static_cast<char*>(ctx->h_stage.p);
        fr.staged = true;
    }
    // (big windows: an extra host copy of tens of MB costs more than the runtime's own staging -- round 5 A/B with everything staged:
    //  the driver's command 14.8 -> 15.2 ms per step, 327 680 targets through the API 81.8 -> 83.3 ms)
    if (fr.best_loss)
        HIP_TRY(hipMemcpyAsync(h ? (void*)h : (void*)fr.best_loss, ctx->best_loss.as<double>() + o, fr.b_loss, hipMemcpyDeviceToHost, ctx->stream));
    if (fr.best_x)
        HIP_TRY(hipMemcpyAsync(h ? (void*)(h + fr.b_loss) : (void*)fr.best_x, ctx->best_x.as<double>() + o * nmax, fr.b_x, hipMemcpyDeviceToHost, ctx->stream));
    if (fr.best_cycles)
        HIP_TRY(hipMemcpyAsync(h ? (void*)(h + fr.b_loss + fr.b_x) : (void*)fr.best_cycles, ctx->best_cycles.as<int32_t>() + o, fr.b_cyc, hipMemcpyDeviceToHost, ctx->stream));
    return SLAM_OK;
}

void finish_fetch(slam_ctx* ctx, const FetchReq& fr) {
    if (!fr.staged) return;
    const char* h = static_cast<const char*>(ctx->h_stage.p);
    if (fr.best_loss) std::memcpy(fr.best_loss, h, fr.b_loss);
    if (fr.best_x) std::memcpy(fr.best_x, h + fr.b_loss, fr.b_x);
    if (fr.best_cycles) std::memcpy(fr.best_cycles, h + fr.b_loss + fr.b_x, fr.b_cyc);
}

// Per-item results of a single-stage call for the host: the records come over as they are and are unpacked into the
// caller's arrays (any of which may be NULL).  The stream is idle (the caller has waited for the stage).
int fetch_item_records(slam_ctx* c, int64_t M, double* item_loss, int32_t* item_iters, int32_t* item_status, int32_t* item_evals) {
    if (!(item_loss || item_iters || item_status || item_evals) || M <= 0) return SLAM_OK;
    std::vector<ItemRec> rec((size_t)M);
    HIP_TRY(hipMemcpyAsync(rec.data(), c->item_rec.p, (size_t)M * sizeof(ItemRec), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    for (int64_t i = 0; i < M; ++i) {
        if (item_loss) item_loss[i] = rec[(size_t)i].loss;
        if (item_iters) item_iters[i] = rec[(size_t)i].iters;
        if (item_status) item_status[i] = rec[(size_t)i].status;
        if (item_evals) item_evals[i] = rec[(size_t)i].evals;
    }
    return SLAM_OK;
}

int enqueue_set_n_active(slam_ctx* c, int k, int64_t n_active) {
    hipLaunchKernelGGL(set_n_active_kernel, dim3(1), dim3(1), 0, c->stream, stage_ctl(c, k), (int32_t)n_active);
    HIP_TRY(hipGetLastError());
    return SLAM_OK;
}

int enqueue_init_results(slam_ctx* c, hipStream_t stream, int32_t* d_active, int64_t first, int64_t n, int k_min, int list_mode) {
    hipLaunchKernelGGL(init_results_kernel, dim3((unsigned)(((d_active ? n * 16 : n) + 255) / 256)), dim3(256), 0, stream,
                       c->best_loss.as<double>(), c->best_cycles.as<int32_t>(), c->span_loss.as<double>(), d_active, first, n, stage_ctl(c, k_min),
                       c->targets.as<double>(), c->stage_targets.as<double>(), c->solved.as<int32_t>(), c->counters.as<StageCtl>(),
                       (int32_t)(sizeof(StageCtl) * (SLAM_MAX_SPAN_EVAL + 2) / 8), list_mode);
    HIP_TRY(hipGetLastError());
    return SLAM_OK;
}

int enqueue_stage_epilogue(slam_ctx* c, int64_t n_upper, const EpilogueArgs& e) {
    // reduction, bookkeeping, compaction and the next stage's inputs in ONE launch: a single workgroup for small
    // batches (ordered compaction without atomics), a grid of 256-thread workgroups beyond
    if (n_upper <= 2048) hipLaunchKernelGGL(stage_epilogue_kernel<256>, dim3(1), dim3(256), 0, c->stream, e);
    else if (n_upper <= kEpilogueMaxTargets) hipLaunchKernelGGL(stage_epilogue_kernel<1024>, dim3(1), dim3(1024), 0, c->stream, e);
    else hipLaunchKernelGGL(stage_epilogue_grid_kernel, dim3((unsigned)((n_upper + 255) / 256)), dim3(256), 0, c->stream, e);
    HIP_TRY(hipGetLastError());
    return SLAM_OK;
}

// (init_lo, init_hi, bound_lo, bound_hi) checked and packed into b[4 n]; *bounded: some bound is finite
static int pack_stage_bounds(int n, const double* init_lo, const double* init_hi, const double* bound_lo, const double* bound_hi, double* b, bool* bounded) {
    *bounded = false;
    for (int i = 0; i < n; ++i) {
        b[i] = init_lo[i];
        b[n + i] = init_hi[i];
        b[2 * n + i] = bound_lo ? bound_lo[i] : -INFINITY;
        b[3 * n + i] = bound_hi ? bound_hi[i] : INFINITY;
        if (!(b[i] <= b[n + i]) || !std::isfinite(b[i]) || !std::isfinite(b[n + i]))
            return fail(SLAM_ERR_INVALID, "start range of parameter %d must be finite with lo <= hi", i);
        if (!(b[2 * n + i] <= b[3 * n + i])) return fail(SLAM_ERR_INVALID, "bounds of parameter %d: lo > hi", i);
        *bounded = *bounded || std::isfinite(b[2 * n + i]) || std::isfinite(b[3 * n + i]);
    }
    return SLAM_OK;
}

// the caller's active list checked and copied into c->active (*d_active stays nullptr without one)
static int upload_stage_active(slam_ctx* c, const int32_t* active, int64_t n_active, const int32_t** d_active) {
    *d_active = nullptr;
    if (active) {
        for (int64_t s = 0; s < n_active; ++s)
            if (active[s] < 0 || active[s] >= c->n_targets)
                return fail(SLAM_ERR_INVALID, "active[%lld] = %d outside [0, %lld)", (long long)s, active[s], (long long)c->n_targets);
        HIP_TRY(c->active.reserve((size_t)n_active * sizeof(int32_t)));
        HIP_TRY(hipMemcpyAsync(c->active.p, active, (size_t)n_active * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
        *d_active = c->active.as<int32_t>();
    }
    return SLAM_OK;
}

// explicit start points x0[count] checked and copied into c->x0 (*d_x0 stays nullptr without them)
static int upload_stage_x0(slam_ctx* c, const double* x0, int64_t count, const double** d_x0) {
    *d_x0 = nullptr;
    if (x0) {
        // the optimizer kernel's range reduction covers |x| < 2e9; steps are <= 2 rad each
        for (int64_t i = 0; i < count; ++i)
            if (!(x0[i] > -1e8 && x0[i] < 1e8)) return fail(SLAM_ERR_INVALID, "x0[%lld] = %g: explicit seeds must be finite with |x| < 1e8", (long long)i, x0[i]);
        HIP_TRY(c->x0.reserve((size_t)count * sizeof(double)));
        HIP_TRY(hipMemcpyAsync(c->x0.p, x0, (size_t)count * sizeof(double), hipMemcpyHostToDevice, c->stream));
        *d_x0 = c->x0.as<double>();
    }
    return SLAM_OK;
}

int stage_family_inputs(slam_ctx* c, int k, int n, const int32_t* active, int64_t n_active, const double* x0, const double* init_lo,
                        const double* init_hi, const double* bound_lo, const double* bound_hi, const slam_opt_params* prm,
                        const int32_t** d_active, const double** d_x0, bool* bounded) {
    const int64_t M = n_active * (int64_t)prm->restarts;
    std::vector<double> b((size_t)4 * n);
    int rc = pack_stage_bounds(n, init_lo, init_hi, bound_lo, bound_hi, b.data(), bounded);
    if (rc) return rc;
    rc = upload_stage_active(c, active, n_active, d_active);
    if (rc) return rc;
    rc = upload_stage_x0(c, x0, M * n, d_x0);
    if (rc) return rc;
    HIP_TRY(c->v2_bounds.reserve(b.size() * sizeof(double)));
    HIP_TRY(hipMemcpyAsync(c->v2_bounds.p, b.data(), b.size() * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));  // b is a local buffer
    // stage buffers sized for n parameters per item (reserve_stage_buffers sizes for 6 (k + 1))
    HIP_TRY(c->item_rec.reserve(M * sizeof(ItemRec)));
    HIP_TRY(c->item_x.reserve(M * n * sizeof(double)));
    HIP_TRY(c->stage_loss.reserve(n_active * sizeof(double)));
    HIP_TRY(c->stage_x.reserve(n_active * n * sizeof(double)));
    HIP_TRY(c->stage_restart.reserve(n_active * sizeof(int32_t)));
    HIP_TRY(hipMemsetAsync(c->counters.p, 0, sizeof(StageCtl) * (SLAM_MAX_SPAN_EVAL + 2), c->stream));
    rc = enqueue_set_n_active(c, k, n_active);
    if (rc) return rc;
    HIP_TRY(c->solved.reserve((size_t)n_active * sizeof(int32_t)));
    HIP_TRY(hipMemsetAsync(c->solved.p, 0, (size_t)n_active * sizeof(int32_t), c->stream));
    return SLAM_OK;
}

int stage_eval_inputs(slam_ctx* c, const double* x, const int32_t* target_of, int64_t M, int n, bool want_grad, bool want_unitary, EvalBufs* d) {
    for (int64_t m = 0; m < M; ++m)
        if (target_of[m] < 0 || target_of[m] >= c->n_targets)
            return fail(SLAM_ERR_INVALID, "target_of[%lld] = %d outside [0, %lld)", (long long)m, target_of[m], (long long)c->n_targets);
    HIP_TRY(c->ev_x.reserve((size_t)M * n * sizeof(double)));
    HIP_TRY(c->ev_tof.reserve((size_t)M * sizeof(int32_t)));
    HIP_TRY(c->ev_loss.reserve((size_t)M * sizeof(double)));
    if (want_grad) HIP_TRY(c->ev_grad.reserve((size_t)M * n * sizeof(double)));
    if (want_unitary) HIP_TRY(c->ev_unitary.reserve((size_t)M * 32 * sizeof(double)));
    HIP_TRY(hipMemcpyAsync(c->ev_x.p, x, (size_t)M * n * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(c->ev_tof.p, target_of, (size_t)M * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    *d = EvalBufs{c->ev_x.as<double>(), c->ev_tof.as<int32_t>(), c->ev_loss.as<double>(), want_grad ? c->ev_grad.as<double>() : nullptr,
                  want_unitary ? c->ev_unitary.as<double>() : nullptr};
    return SLAM_OK;
}

int enqueue_eval_readback(slam_ctx* c, int64_t M, int n, double* loss, double* grad, double* unitary) {
    HIP_TRY(hipMemcpyAsync(loss, c->ev_loss.p, (size_t)M * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (grad) HIP_TRY(hipMemcpyAsync(grad, c->ev_grad.p, (size_t)M * n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (unitary) HIP_TRY(hipMemcpyAsync(unitary, c->ev_unitary.p, (size_t)M * 32 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    return SLAM_OK;
}

// single stage of a parametrised-gate family: per-target reduction only, no merge into resident results
static int enqueue_stage_reduce(slam_ctx* c, int k, int n, int64_t n_active, const slam_opt_params* prm, double exit_loss) {
    ReduceArgs r = build_reduce_args(c, k, n, nullptr, prm, exit_loss, false);
    r.ordered = 1;  // whatever the flags: the winner is the restart the reference's sequential loop breaks at (restarts below it always run to their end)
    r.slot_ev = nullptr;  // the evaluations stay in the stage's counters: these stages never run on a helper context of the overlapped loop
    hipLaunchKernelGGL(reduce_merge_kernel, dim3((unsigned)((n_active + 255) / 256)), dim3(256), 0, c->stream, r);
    HIP_TRY(hipGetLastError());
    return SLAM_OK;
}

int finish_single_stage(slam_ctx* c, int k, int n, int64_t n_active, const slam_opt_params* prm, double exit_loss, double* best_loss, double* best_x,
                        int32_t* best_restart, double* item_loss, int32_t* item_iters, int32_t* item_status, int32_t* item_evals) {
    int rc = enqueue_stage_reduce(c, k, n, n_active, prm, exit_loss);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(best_loss, c->stage_loss.p, (size_t)n_active * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(best_x, c->stage_x.p, (size_t)n_active * n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (best_restart) HIP_TRY(hipMemcpyAsync(best_restart, c->stage_restart.p, (size_t)n_active * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(c->h_ctl, c->counters.p, sizeof(StageCtl) * (SLAM_MAX_SPAN_EVAL + 2), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    rc = fetch_item_records(c, n_active * (int64_t)prm->restarts, item_loss, item_iters, item_status, item_evals);
    if (rc) return rc;
    return collect_stats(c, k, k, c->h_ctl, prm->restarts);
}

namespace {

// -----------------------------------------------------------------------------------------------------------------------
// Small batches: the whole span loop of a target in ONE wavefront (span_wave_kernel, slam_kernels.hpp) -- one launch per call, no
// stage barrier across targets, no bookkeeping launches.  Used when the batch is at most kWaveLoopTargetsPerSimd targets per SIMD,
// spans <= 3, ordered early exit, one gate structure class for all spans; SLAM_FLAG_STAGED forces the per-span launches.
// -----------------------------------------------------------------------------------------------------------------------
constexpr int kWaveLoopTargetsPerSimd = 1;

int launch_span_wave(slam_ctx* c, int gc, const WaveLoopArgs& a, int64_t count) {
    return with_gate_class(gc, [&](auto g) -> int {
        constexpr int GC = decltype(g)::value;
        const size_t lds = sizeof(double) * (size_t)(lds_doubles<3, GC>() + kWlLdsDoubles);
        { int rc = kernel_per_cu(c, reinterpret_cast<const void*>(&span_wave_kernel<GC>), lds, nullptr); if (rc) return rc; }
        const int64_t blocks = count;  // one wavefront per target
        hipLaunchKernelGGL((span_wave_kernel<GC>), dim3((unsigned)blocks), dim3(kWave), lds, c->stream, a);
        HIP_TRY(hipGetLastError());
        return SLAM_OK;
    });
}

// speculative spans: one launch per span, each on its own stream, then the merge (span_spec_kernel / span_merge_kernel)
template <int K>
int launch_span_spec(slam_ctx* c, int gc, const WaveLoopArgs& a, int64_t count, hipStream_t stream) {
    return with_gate_class(gc, [&](auto g) -> int {
        constexpr int GC = decltype(g)::value;
        const size_t lds = sizeof(double) * (size_t)(lds_doubles<K, GC>() + kWlLdsDoubles);
        { int rc = kernel_per_cu(c, reinterpret_cast<const void*>(&span_spec_kernel<K, GC>), lds, nullptr); if (rc) return rc; }
        hipLaunchKernelGGL((span_spec_kernel<K, GC>), dim3((unsigned)count), dim3(kWave), lds, stream, a);
        HIP_TRY(hipGetLastError());
        return SLAM_OK;
    });
}

constexpr int64_t kOverlapMaxItems = 1 << 17;  // four times what the chip holds at once (2048 wavefronts x 16 items)

// would decompose_overlapped (below) take this call?
bool overlap_eligible(const slam_ctx* c, int64_t count, int k_min, int k_max, const slam_opt_params* prm) {
    static const bool env_staged = std::getenv("SLAM_STAGED") != nullptr;
    static const bool env_off = []{ const char* e = std::getenv("SLAM_OVERLAP"); return e && e[0] == '0'; }();
    if ((prm->flags & SLAM_FLAG_STAGED) || env_staged || env_off) return false;
    if (c->cost_kind == SLAM_COST_MAKHLIN) return false;  // (per-span launches only: no MakhlinFunctionalCost instantiation of the side-by-side spans)
    if (!(prm->flags & SLAM_FLAG_EARLY_EXIT) || !(prm->flags & SLAM_FLAG_ORDERED)) return false;
    if (k_max <= k_min || k_max > 3 || c->trace_cap > 0) return false;
    if (prm->flags & SLAM_FLAG_OVERLAP) return true;
    return !(prm->flags & SLAM_FLAG_NO_OVERLAP) && count * (int64_t)prm->restarts <= kOverlapMaxItems;
}

// returns SLAM_OK and *taken = true when the call was served by the wave-loop kernel; *taken = false: not eligible (nothing enqueued)
int decompose_wave_loop(slam_ctx* c, int64_t first, int64_t count, int k_min, int k_max, const int32_t* gate_seqs, const slam_opt_params* prm,
                        double success_threshold, FetchReq* fetch, bool* taken) {
    *taken = false;
    if (prm->flags & SLAM_FLAG_STAGED) return SLAM_OK;
    if (c->cost_kind == SLAM_COST_MAKHLIN) return SLAM_OK;  // (no wave-loop instantiation for MakhlinFunctionalCost: the per-span launches)
    static const bool env_staged = std::getenv("SLAM_STAGED") != nullptr;  // (test runs: the whole suite through the per-span launches)
    static const bool env_no_wave = []{ const char* e = std::getenv("SLAM_WAVE_LOOP"); return e && e[0] == '0'; }();  // (A/B runs)
    if (env_staged || env_no_wave) return SLAM_OK;
    if (!(prm->flags & SLAM_FLAG_EARLY_EXIT) || !(prm->flags & SLAM_FLAG_ORDERED)) return SLAM_OK;
    if (k_max > 3 || c->trace_cap > 0) return SLAM_OK;
    if (count > (int64_t)kWaveLoopTargetsPerSimd * 4 * c->compute_units) return SLAM_OK;
    // a wavefront runs its target's restarts 16 at a time: with many restarts and few targets the per-span launches, which spread the
    // items over the whole chip, are faster (measured, CNOT, profiles/r4_wave_probe.txt: R = 32: 1024 targets 1.34 vs 1.63 ms, 16
    // targets 1.00 vs 0.81; R = 64: 1024 targets 2.01 vs 2.41, 256 targets 1.96 vs 1.44; R = 128: 1024 targets 3.52 vs 3.25)
    if (prm->restarts > 16 && !(prm->restarts <= 64 && count * (int64_t)prm->restarts >= 32768)) return SLAM_OK;
    // ... and with more than 16 restarts the spans side by side on the whole chip (decompose_overlapped) beat it where they may run
    // (tools/r4_wave_vs_overlap.py, 1024 targets: R = 32 1.29 -> 1.15 ms CNOT, 1.47 -> 1.31 sqrt(iSWAP); R = 64 2.01 -> 1.67, 2.26 -> 1.57;
    // with 16 restarts the wave kernels win: 0.90 vs 1.08, 512 targets 0.67 vs 0.75)
    if (prm->restarts > 16 && overlap_eligible(c, count, k_min, k_max, prm)) return SLAM_OK;
    int gc = -1;
    {
        const int32_t* gs = gate_seqs;
        for (int k = k_min; k <= k_max; ++k) {
            const int g = classify_gates(c, k, gs);
            if (gc >= 0 && g != gc) return SLAM_OK;  // (per-span classes differ: the per-span launches use each span's own class)
            gc = g;
            gs += k;
        }
    }
    // argument blocks of the spans (the kernels' own MinimizeArgs layout), staged through pinned memory
    const size_t need = sizeof(MinimizeArgs<1>) * (size_t)(SLAM_MAX_SPAN_EVAL + 1);
    HIP_TRY(c->mq_args.reserve(need));
    HIP_TRY(c->h_mq_args.reserve(need));
    MinimizeArgs<1>* h = static_cast<MinimizeArgs<1>*>(c->h_mq_args.p);
    const int32_t* gs = gate_seqs;
    for (int k = k_min; k <= k_max; ++k) {
        StageLaunch sl{success_threshold, gs, c->targets.as<double>(), nullptr, 0, nullptr, count * (int64_t)prm->restarts, prm, stage_ctl(c, k)};
        int rc;
        switch (k) {
            case 1: rc = build_minimize_args<1>(c, sl, *reinterpret_cast<MinimizeArgs<1>*>(&h[k])); break;
            case 2: rc = build_minimize_args<2>(c, sl, *reinterpret_cast<MinimizeArgs<2>*>(&h[k])); break;
            default: rc = build_minimize_args<3>(c, sl, *reinterpret_cast<MinimizeArgs<3>*>(&h[k])); break;
        }
        if (rc) return rc;
        gs += k;
    }
    *taken = true;
    HIP_TRY(hipEventRecord(c->ev_t0, c->stream));
    HIP_TRY(hipMemcpyAsync(c->mq_args.p, h, need, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemsetAsync(c->counters.p, 0, sizeof(StageCtl) * (SLAM_MAX_SPAN_EVAL + 2), c->stream));
    WaveLoopArgs a{};
    a.stage_args = c->mq_args.as<MinimizeArgs<1>>();
    a.ctl = c->counters.as<StageCtl>();
    a.k_min = k_min;
    a.k_max = k_max;
    a.first = (int32_t)first;
    a.count = (int32_t)count;
    a.threshold = success_threshold;
    a.best_loss = c->best_loss.as<double>();
    a.best_x = c->best_x.as<double>();
    a.best_cycles = c->best_cycles.as<int32_t>();
    a.span_loss = c->span_loss.as<double>();
    a.nmax = c->result_nmax;
    // every wavefront leaves a stage after this many rounds whatever happens: far above what R restarts of maxiter iterations
    // (each at most 1 + 21 line-search evaluations) can need when they run 16 at a time
    {
        const double need_rounds = ((double)prm->restarts / 16.0 + 1.0) * ((double)prm->maxiter + 2.0) * 22.0;
        a.round_cap = need_rounds > 4.0e9 ? 0xffffffffu : (uint32_t)need_rounds;
    }
    // speculative spans (see span_spec_kernel): all spans of all targets at once when the loop has more than one span.
    // SLAM_SPECULATE=0 keeps the one-wavefront-per-target loop (A/B runs, tests of that kernel).
    static const bool env_no_spec = []{ const char* e = std::getenv("SLAM_SPECULATE"); return e && e[0] == '0'; }();
    // Worth it while every (target, span) wavefront finds a SIMD of its own (measured, tools/r4_spec_probe.sh, CNOT x 16 restarts: 1
    // target 0.51 -> 0.28 ms, 256 targets 0.80 -> 0.55; at 1024 targets the k = 2 and k = 3 stages no longer fit beside each other
    // -- 256 + 304 registers -- and the two forms tie: 0.94 / 0.89 ms CNOT, 1.14 / 1.18 ms sqrt(iSWAP), where k = 3 is mostly wasted)
    const bool spec = k_max > k_min && !env_no_spec && count <= 2 * (int64_t)c->compute_units;
    int n_launch = 1;
    HIP_TRY(hipEventRecord(c->ev_a[0], c->stream));  // bracket 0: the whole call's optimizer work (kernel_ms)
    int rc;
    if (spec) {
        HIP_TRY(c->spec_loss.reserve(sizeof(double) * 3 * (size_t)count));
        HIP_TRY(c->spec_x.reserve(sizeof(double) * 3 * (size_t)count * (size_t)c->result_nmax));
        HIP_TRY(c->spec_ev.reserve(sizeof(unsigned long long) * 9 * (size_t)count));
        a.spec_loss = c->spec_loss.as<double>();
        a.spec_x = c->spec_x.as<double>();
        a.spec_ev = c->spec_ev.as<unsigned long long>();
        if (!c->spec_stream[0]) {
            for (int j = 0; j < 2; ++j) {
                HIP_TRY(hipStreamCreateWithFlags(&c->spec_stream[j].h, hipStreamNonBlocking));
                HIP_TRY(hipEventCreateWithFlags(&c->spec_join[j].h, hipEventDisableTiming));
            }
            HIP_TRY(hipEventCreateWithFlags(&c->spec_fork.h, hipEventDisableTiming));
        }
        HIP_TRY(hipEventRecord(c->spec_fork, c->stream));
        // the longest stage first, on the call's own stream; the others beside it
        int side = 0;
        for (int k = k_max; k >= k_min; --k) {
            hipStream_t st = c->stream;
            if (k != k_max) {
                st = c->spec_stream[side];
                HIP_TRY(hipStreamWaitEvent(st, c->spec_fork, 0));
            }
            HIP_TRY(hipEventRecord(c->ev_a[k], st));  // span k's own launch (the spans overlap in time: kernel_ms_span[k])
            switch (k) {
                case 1: rc = launch_span_spec<1>(c, gc, a, count, st); break;
                case 2: rc = launch_span_spec<2>(c, gc, a, count, st); break;
                default: rc = launch_span_spec<3>(c, gc, a, count, st); break;
            }
            if (rc) return rc;
            HIP_TRY(hipEventRecord(c->ev_b[k], st));
            if (k != k_max) {
                HIP_TRY(hipEventRecord(c->spec_join[side], st));
                HIP_TRY(hipStreamWaitEvent(c->stream, c->spec_join[side], 0));
                ++side;
            }
        }
        SpanMergeArgs mg{};
        mg.k_min = k_min;
        mg.k_max = k_max;
        mg.first = (int32_t)first;
        mg.count = (int32_t)count;
        mg.nmax = c->result_nmax;
        mg.threshold = success_threshold;
        for (int k = k_min; k <= k_max; ++k) {
            mg.loss[k] = a.spec_loss + (size_t)(k - 1) * count;
            mg.x[k] = a.spec_x + (size_t)(k - 1) * count * c->result_nmax;
            mg.xstride[k] = c->result_nmax;
            mg.xn[k] = 6 * (k + 1);
            mg.ev[k] = a.spec_ev + (size_t)(k - 1) * count * 3;
            mg.src_ctl[k] = nullptr;  // (the stage kernels add their rounds themselves)
        }
        mg.ctl = a.ctl;
        mg.best_loss = a.best_loss;
        mg.best_x = a.best_x;
        mg.best_cycles = a.best_cycles;
        mg.span_loss = a.span_loss;
        hipLaunchKernelGGL(span_merge_kernel, dim3((unsigned)((count + kWave - 1) / kWave)), dim3(kWave), 0, c->stream, mg);
        HIP_TRY(hipGetLastError());
        n_launch = (k_max - k_min + 1) + 1;
    } else {
        rc = launch_span_wave(c, gc, a, count);
        if (rc) return rc;
    }
    HIP_TRY(hipEventRecord(c->ev_b[0], c->stream));
    rc = enqueue_loop_end(c, fetch, c->result_nmax, first, count);
    if (rc) return rc;
    rc = wait_loop_end(c, fetch);
    if (rc) return rc;
    float kms = 0.f;
    HIP_TRY(hipEventElapsedTime(&kms, c->ev_a[0], c->ev_b[0]));
    c->stats.kernel_ms += kms;
    if (spec) {
        // one launch per span, side by side: every span's own bracket (they overlap: their sum exceeds kernel_ms)
        for (int k = k_min; k <= k_max; ++k) {
            float sk = 0.f;
            HIP_TRY(hipEventElapsedTime(&sk, c->ev_a[k], c->ev_b[k]));
            c->stats.kernel_ms_span[k] += sk;
        }
    } else {
        c->stats.kernel_ms_span[0] += kms;  // ONE launch for all spans: no per-span split exists -- booked under index 0
    }
    c->stats.kernel_launches += n_launch;
    fold_counters(c->stats, c->h_ctl, k_min, k_max, prm->restarts, FOLD_SKIP_IDLE_UNEVALUATED);
    return SLAM_OK;
}

// -----------------------------------------------------------------------------------------------------------------------
// Medium batches: the spans of the loop side by side.  The stages of a target do not use each other's results, only the decision
// whether they are needed (optimizer.py:301-303), and their start points are keyed by span -- so every span runs for ALL targets of
// the window at once, each as the ordinary per-span pipeline (stage inputs, optimizer kernel, per-target reduction: what
// slam_minimize_stage runs) on a helper context with its own stream and stage buffers, and span_merge_kernel then applies the loop's
// bookkeeping in span order.  Results are those of the staged launches bit for bit; the work of stages the loop would not have reached
// is wasted (booked as pre-empted evaluations), which is why this form is taken only while one call cannot fill the chip for long
// (targets x restarts <= kOverlapMaxItems and no SLAM_FLAG_NO_OVERLAP; measured, tools/r4_overlap_probe.py: CNOT 4096 x 16 2.84 -> 1.86 ms, 20 480 x 16 5.1 -> 4.9,
// sqrt(iSWAP) 65 536 x 32 18.1 -> 16.5) or when the caller asks for it (SLAM_FLAG_OVERLAP).
// -----------------------------------------------------------------------------------------------------------------------
__global__ void iota_kernel(int32_t* out, int32_t first, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = first + (int32_t)i;
}

int decompose_overlapped(slam_ctx* c, int64_t first, int64_t count, int k_min, int k_max, const int32_t* gate_seqs, const slam_opt_params* prm,
                         double success_threshold, FetchReq* fetch, bool* taken) {
    *taken = false;
    if (!overlap_eligible(c, count, k_min, k_max, prm)) return SLAM_OK;
    // helper contexts (one per span), created on first use; their targets are this context's (borrowed for the call)
    for (int k = k_min; k <= k_max; ++k) {
        if (!c->helper[k]) {
            slam_ctx* h = nullptr;
            int rc = slam_ctx_create(c->device, &h);
            if (rc) return rc;
            c->helper[k].reset(h);
            HIP_TRY(hipEventCreateWithFlags(&c->ov_join[k].h, hipEventDisableTiming));
        }
    }
    if (!c->ov_fork) HIP_TRY(hipEventCreateWithFlags(&c->ov_fork.h, hipEventDisableTiming));
    struct Unborrow {
        slam_ctx* c;
        ~Unborrow() {
            for (const auto& h : c->helper)
                if (h) {
                    h->targets.unborrow();
                    h->n_targets = 0;
                }
        }
    } unborrow{c};
    *taken = true;
    HIP_TRY(hipEventRecord(c->ev_t0, c->stream));
    HIP_TRY(hipMemsetAsync(c->counters.p, 0, sizeof(StageCtl) * (SLAM_MAX_SPAN_EVAL + 2), c->stream));
    HIP_TRY(hipEventRecord(c->ev_a[0], c->stream));  // bracket 0: the whole call's optimizer work (kernel_ms)
    HIP_TRY(hipEventRecord(c->ov_fork, c->stream));
    SpanMergeArgs mg{};
    const int32_t* gs = gate_seqs;
    // the spans are enqueued longest first (k_max ... k_min): each on its helper's stream
    const int32_t* seq_of[SLAM_MAX_SPAN_EVAL + 1] = {};
    for (int k = k_min; k <= k_max; ++k) {
        seq_of[k] = gs;
        gs += k;
    }
    for (int k = k_max; k >= k_min; --k) {
        slam_ctx* h = c->helper[k].get();
        h->targets.borrow(c->targets);
        h->n_targets = c->n_targets;
        if (h->helper_gates_version != c->gates_version) {
            h->gates_host = c->gates_host;
            h->n_gates = c->n_gates;
            for (auto& st : h->staged) st.valid = false;
            h->helper_gates_version = c->gates_version;
        }
        h->cost_kind = c->cost_kind;
        h->reserve_waves = c->reserve_waves;
        h->stage_exit_loss = success_threshold;  // ordered early exit at the loop's threshold (optimizer.py:287)
        h->slot_ev_on = true;
        HIP_TRY(h->active.reserve((size_t)count * sizeof(int32_t)));
        HIP_TRY(h->slot_ev.reserve((size_t)count * 3 * sizeof(unsigned long long)));
        int rc = reserve_stage_buffers(h, count, k, prm);
        if (rc) return rc;
        HIP_TRY(hipStreamWaitEvent(h->stream, c->ov_fork, 0));
        hipLaunchKernelGGL(iota_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, h->stream, h->active.as<int32_t>(), (int32_t)first, count);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemsetAsync(h->counters.p, 0, sizeof(StageCtl) * (SLAM_MAX_SPAN_EVAL + 2), h->stream));
        hipLaunchKernelGGL(set_n_active_kernel, dim3(1), dim3(1), 0, h->stream, stage_ctl(h, k), (int32_t)count);
        HIP_TRY(hipGetLastError());
        rc = enqueue_stage(h, k, seq_of[k], h->active.as<int32_t>(), count, nullptr, prm, nullptr);
        if (rc) return rc;
        HIP_TRY(hipEventRecord(c->ov_join[k], h->stream));
        HIP_TRY(hipStreamWaitEvent(c->stream, c->ov_join[k], 0));
        mg.loss[k] = h->stage_loss.as<double>();
        mg.x[k] = h->stage_x.as<double>();
        mg.xstride[k] = 6 * (k + 1);
        mg.xn[k] = 6 * (k + 1);
        mg.ev[k] = h->slot_ev.as<unsigned long long>();
        mg.src_ctl[k] = stage_ctl(h, k);
    }
    mg.k_min = k_min;
    mg.k_max = k_max;
    mg.first = (int32_t)first;
    mg.count = (int32_t)count;
    mg.nmax = c->result_nmax;
    mg.threshold = success_threshold;
    mg.ctl = c->counters.as<StageCtl>();
    mg.best_loss = c->best_loss.as<double>();
    mg.best_x = c->best_x.as<double>();
    mg.best_cycles = c->best_cycles.as<int32_t>();
    mg.span_loss = c->span_loss.as<double>();
    hipLaunchKernelGGL(span_merge_kernel, dim3((unsigned)((count + kWave - 1) / kWave)), dim3(kWave), 0, c->stream, mg);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(c->ev_b[0], c->stream));
    int rc = enqueue_loop_end(c, fetch, c->result_nmax, first, count);
    if (rc) return rc;
    rc = wait_loop_end(c, fetch);
    if (rc) return rc;
    float kms = 0.f;
    HIP_TRY(hipEventElapsedTime(&kms, c->ev_a[0], c->ev_b[0]));
    c->stats.kernel_ms += kms;
    for (int k = k_min; k <= k_max; ++k) {
        // every span's own optimizer launch, bracketed on its helper's stream by enqueue_stage (the spans overlap in time: the sum of
        // kernel_ms_span exceeds kernel_ms -- ADVICE r4: the whole used to be booked on the first span)
        float sk = 0.f;
        HIP_TRY(hipEventElapsedTime(&sk, c->helper[k]->ev_a[k], c->helper[k]->ev_b[k]));
        c->stats.kernel_ms_span[k] += sk;
    }
    c->stats.kernel_launches += 2 * (k_max - k_min + 1) + 1;
    fold_counters(c->stats, c->h_ctl, k_min, k_max, prm->restarts, FOLD_ALL);
    return SLAM_OK;
}

// h_list != nullptr: the batch is the explicit list of resident-target indices h_list[0..count) (first ignored)
int decompose_body(slam_ctx* c, int64_t first, int64_t count, int k_min, int k_max, const int32_t* gate_seqs,
                   const slam_opt_params* prm, double success_threshold, const int32_t* h_list, int k_layout,
                   FetchReq* fetch) {
    if (!c) return fail(SLAM_ERR_INVALID, "ctx is NULL");
    HIP_TRY(hipSetDevice(c->device));
    if (c->n_targets <= 0) return fail(SLAM_ERR_STATE, "no targets: call slam_set_targets first");
    if (c->n_gates <= 0) return fail(SLAM_ERR_STATE, "no gates: call slam_set_gates first");
    if (k_min < 1 || k_max < k_min) return fail(SLAM_ERR_INVALID, "bad span range [%d, %d]", k_min, k_max);
    if (k_max > SLAM_MAX_SPAN_MINIMIZE)
        return fail(SLAM_ERR_UNSUPPORTED, "minimize supports spans 1..%d (got k_max = %d)", SLAM_MAX_SPAN_MINIMIZE, k_max);
    int rc = check_params(prm);
    if (rc) return rc;
    {
        const int32_t* gs = gate_seqs;
        for (int k = k_min; k <= k_max; ++k) {
            rc = check_gate_seq(c, k, gs);
            if (rc) return rc;
            gs += k;
        }
    }
    if (h_list) {
        if (count <= 0) return fail(SLAM_ERR_INVALID, "empty target list");
        for (int64_t i = 0; i < count; ++i)
            if (h_list[i] < 0 || h_list[i] >= c->n_targets)
                return fail(SLAM_ERR_INVALID, "targets[%lld] = %d outside [0, %lld)", (long long)i, h_list[i], (long long)c->n_targets);
        first = 0;
    } else if (first < 0 || count <= 0 || first + count > c->n_targets)
        return fail(SLAM_ERR_INVALID, "target window [%lld, %lld) outside [0, %lld)", (long long)first,
                    (long long)(first + count), (long long)c->n_targets);
    if (k_layout == 0) k_layout = k_max;
    if (k_layout < k_max || k_layout > SLAM_MAX_SPAN_MINIMIZE) return fail(SLAM_ERR_INVALID, "k_layout must be in [k_max, %d]", SLAM_MAX_SPAN_MINIMIZE);
    if (c->result_nmax != 0 && c->result_nmax != 6 * (k_layout + 1) && (h_list || !(first == 0 && count == c->n_targets)))
        return fail(SLAM_ERR_STATE, "resident results were produced with a different k_max");
    rc = ensure_results(c, k_layout);
    if (rc) return rc;
    if (!h_list && k_layout == k_max) {
        bool taken = false;
        rc = decompose_wave_loop(c, first, count, k_min, k_max, gate_seqs, prm, success_threshold, fetch, &taken);
        if (rc || taken) return rc;
        rc = decompose_overlapped(c, first, count, k_min, k_max, gate_seqs, prm, success_threshold, fetch, &taken);
        if (rc || taken) return rc;
    }
    const int64_t N = count;
    HIP_TRY(c->active.reserve(N * sizeof(int32_t)));
    HIP_TRY(c->active2.reserve(N * sizeof(int32_t)));
    rc = reserve_stage_buffers(c, N, k_max, prm);
    if (rc) return rc;
    HIP_TRY(hipEventRecord(c->ev_t0, c->stream));
    const bool whole = !h_list && (first == 0 && count == c->n_targets);
    if (h_list) HIP_TRY(hipMemcpyAsync(c->active.p, h_list, (size_t)N * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    rc = enqueue_init_results(c, c->stream, whole ? (int32_t*)nullptr : c->active.as<int32_t>(), first, N, k_min, h_list ? 1 : 0);
    if (rc) return rc;

    // The whole span loop is enqueued at once: a stage's target count is produced on the device by the
    // previous stage's compaction (every stage is sized for N on the host; a stage without targets costs a
    // few empty launches), so the only host synchronisation is the one at the end.
    const int32_t* d_active = whole ? nullptr : c->active.as<int32_t>();  // nullptr = identity
    DevBuf* cur = &c->active;
    DevBuf* nxt = &c->active2;
    const int32_t* gs = gate_seqs;
    for (int k = k_min; k <= k_max; ++k) {
        // the first stage's inputs come from init_results_kernel, the later ones from the previous stage's epilogue
        SpanLoopStep step{success_threshold, true, k < k_max, success_threshold, nxt->as<int32_t>()};
        rc = enqueue_stage(c, k, gs, d_active, N, nullptr, prm, &step);
        if (rc) return rc;
        gs += k;
        if (k < k_max) {
            d_active = nxt->as<int32_t>();
            DevBuf* t = cur; cur = nxt; nxt = t;
        }
    }
    rc = enqueue_loop_end(c, fetch, 6 * (k_layout + 1), h_list ? 0 : first, h_list ? c->n_targets : count);
    if (rc) return rc;
    rc = wait_loop_end(c, fetch);
    if (rc) return rc;
    return collect_stats(c, k_min, k_max, c->h_ctl, prm->restarts);
}

int decompose_impl(slam_ctx* c, int64_t first, int64_t count, int k_min, int k_max, const int32_t* gate_seqs,
                   const slam_opt_params* prm, double success_threshold, const int32_t* h_list = nullptr, int k_layout = 0,
                   FetchReq* fetch = nullptr) {
    return drained(c, decompose_body(c, first, count, k_min, k_max, gate_seqs, prm, success_threshold, h_list, k_layout, fetch));
}


// -----------------------------------------------------------------------------------------------------------------------
// slam_decompose_multi: the span loops of SEVERAL contexts -- same device, same target window, each with its own gate table
// (e.g. the bases of a parametric-Hamiltonian sweep, BASELINE configs[4]) -- enqueued as ONE chain of kernels on the first
// context's stream: per span ONE multi-queue optimizer launch (minimize_kernel<K, GC, true>: a wavefront works on one
// sub-problem at a time, so gates stay scalar operands) and ONE epilogue launch for all of them.  Every context ends with the
// results its own slam_decompose_range call would have left (ordered early exit: bit for bit) -- which is why contexts whose gates
// fall into different structure classes get one optimizer launch PER CLASS (measured: the same item run through the GC_XRI1 and the
// GC_XRI instantiation ends 1e-14 apart -- the compiler contracts the surrounding products differently -- so a launch in the most
// general class of the group would not reproduce the per-context calls).
// -----------------------------------------------------------------------------------------------------------------------
template <int K, int GC>
int launch_minimize_multi(slam_ctx* lead, const MinimizeArgs<K>& common, const MinimizeArgs<K>* d_subs, int n, int64_t items_max_total) {
    const size_t lds = lds_bytes<K, GC>();
    int per_cu = 0;
    { int rc = kernel_per_cu(lead, reinterpret_cast<const void*>(&minimize_kernel<K, GC, true>), lds, &per_cu); if (rc) return rc; }
    int64_t blocks = (items_max_total + kQuadsPerWave - 1) / kQuadsPerWave;
    const int64_t resident = (int64_t)per_cu * lead->compute_units;
    const int64_t cap = resident > 0 ? resident : 1;
    if (blocks > cap) blocks = cap;
    if (blocks < n) blocks = n;  // every sub-problem has a wavefront that starts on it
    hipLaunchKernelGGL((minimize_kernel<K, GC, true>), dim3((unsigned)blocks), dim3(kWave), lds, lead->stream, common, d_subs, n);
    HIP_TRY(hipGetLastError());
    return SLAM_OK;
}

int decompose_multi_body(slam_ctx** cs, int n, int64_t first, int64_t count, int k_min, int k_max, const int32_t* gate_seqs,
                         const slam_opt_params* prm, double success_threshold) {
    if (!cs || n <= 0) return fail(SLAM_ERR_INVALID, "no contexts");
    slam_ctx* lead = cs[0];
    for (int i = 0; i < n; ++i) {
        if (!cs[i]) return fail(SLAM_ERR_INVALID, "ctxs[%d] is NULL", i);
        if (cs[i]->device != lead->device) return fail(SLAM_ERR_INVALID, "ctxs[%d] lives on device %d, ctxs[0] on %d", i, cs[i]->device, lead->device);
        for (int j = 0; j < i; ++j)
            if (cs[j] == cs[i]) return fail(SLAM_ERR_INVALID, "ctxs[%d] and ctxs[%d] are the same context", j, i);
        if (cs[i]->n_targets <= 0) return fail(SLAM_ERR_STATE, "ctxs[%d]: no targets", i);
        if (cs[i]->n_gates <= 0) return fail(SLAM_ERR_STATE, "ctxs[%d]: no gates", i);
        if (first < 0 || count <= 0 || first + count > cs[i]->n_targets)
            return fail(SLAM_ERR_INVALID, "ctxs[%d]: target window [%lld, %lld) outside [0, %lld)", i, (long long)first, (long long)(first + count), (long long)cs[i]->n_targets);
        if (cs[i]->cost_kind != lead->cost_kind) return fail(SLAM_ERR_INVALID, "ctxs[%d]: another cost function than ctxs[0]", i);
    }
    if (lead->cost_kind == SLAM_COST_MAKHLIN)
        return fail(SLAM_ERR_UNSUPPORTED, "slam_decompose_multi does not run MakhlinFunctionalCost (SLAM_COST_MAKHLIN): call slam_decompose_range per context");
    HIP_TRY(hipSetDevice(lead->device));
    if (k_min < 1 || k_max < k_min) return fail(SLAM_ERR_INVALID, "bad span range [%d, %d]", k_min, k_max);
    if (k_max > 3) return fail(SLAM_ERR_UNSUPPORTED, "slam_decompose_multi runs spans 1..3 (got k_max = %d)", k_max);
    int rc = check_params(prm);
    if (rc) return rc;
    if (!(prm->flags & SLAM_FLAG_EARLY_EXIT) || !(prm->flags & SLAM_FLAG_ORDERED))
        return fail(SLAM_ERR_INVALID, "slam_decompose_multi needs SLAM_FLAG_EARLY_EXIT | SLAM_FLAG_ORDERED (results independent of scheduling)");
    const int64_t N = count;
    for (int i = 0; i < n; ++i) {
        slam_ctx* c = cs[i];
        const int32_t* gs = gate_seqs;
        for (int k = k_min; k <= k_max; ++k) {
            rc = check_gate_seq(c, k, gs);
            if (rc) return rc;
            gs += k;
        }
        if (c->result_nmax != 0 && c->result_nmax != 6 * (k_max + 1) && !(first == 0 && count == c->n_targets))
            return fail(SLAM_ERR_STATE, "ctxs[%d]: resident results were produced with a different k_max", i);
        // (allocation and the first fill run on the context's own, idle stream; the lead's stream waits for them below)
        rc = ensure_results(c, k_max);
        if (rc) return rc;
        HIP_TRY(c->active.reserve(N * sizeof(int32_t)));
        HIP_TRY(c->active2.reserve(N * sizeof(int32_t)));
        rc = reserve_stage_buffers(c, N, k_max, prm);
        if (rc) return rc;
        if (c != lead) HIP_TRY(hipStreamSynchronize(c->stream));
    }
    // staging: per span n optimizer argument blocks + n epilogue argument blocks
    const size_t sz_ma = sizeof(MinimizeArgs<1>), sz_ep = sizeof(EpilogueArgs);
    static_assert(sizeof(MinimizeArgs<1>) == sizeof(MinimizeArgs<3>), "argument blocks of all spans have one layout");
    const size_t slot = (size_t)n * (sz_ma + sz_ep);
    const size_t need = slot * (size_t)(k_max + 1);
    HIP_TRY(lead->mq_args.reserve(need));
    HIP_TRY(lead->h_mq_args.reserve(need));
    HIP_TRY(hipEventRecord(lead->ev_t0, lead->stream));
    for (int i = 0; i < n; ++i) {
        slam_ctx* c = cs[i];
        const bool whole = (first == 0 && count == c->n_targets);
        rc = enqueue_init_results(c, lead->stream, whole ? (int32_t*)nullptr : c->active.as<int32_t>(), first, N, k_min, 0);
        if (rc) return rc;
    }
    std::vector<const int32_t*> d_active((size_t)n);
    std::vector<DevBuf*> cur((size_t)n), nxt((size_t)n);
    for (int i = 0; i < n; ++i) {
        const bool whole = (first == 0 && count == cs[i]->n_targets);
        d_active[(size_t)i] = whole ? nullptr : cs[i]->active.as<int32_t>();
        cur[(size_t)i] = &cs[i]->active;
        nxt[(size_t)i] = &cs[i]->active2;
    }
    const int32_t* gs = gate_seqs;
    for (int k = k_min; k <= k_max; ++k) {
        char* h = static_cast<char*>(lead->h_mq_args.p) + slot * (size_t)k;
        char* d = static_cast<char*>(lead->mq_args.p) + slot * (size_t)k;
        MinimizeArgs<1>* h_ma = reinterpret_cast<MinimizeArgs<1>*>(h);  // (one layout for every span)
        EpilogueArgs* h_ep = reinterpret_cast<EpilogueArgs*>(h + (size_t)n * sz_ma);
        // contexts ordered by the structure class of their gates: one contiguous run of argument blocks, one launch, per class
        std::vector<int> order((size_t)n), cls((size_t)n);
        for (int i = 0; i < n; ++i) { order[(size_t)i] = i; cls[(size_t)i] = classify_gates(cs[i], k, gs); }
        std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return cls[(size_t)a] < cls[(size_t)b]; });
        for (int slot_i = 0; slot_i < n; ++slot_i) {
            const int i = order[(size_t)slot_i];
            slam_ctx* c = cs[i];
            const double* d_stage_targets = d_active[(size_t)i] ? c->stage_targets.as<double>() : c->targets.as<double>();
            StageLaunch sl{success_threshold, gs, d_stage_targets, d_active[(size_t)i], 0, nullptr, N * (int64_t)prm->restarts, prm, stage_ctl(c, k)};
            switch (k) {
                case 1: rc = build_minimize_args<1>(c, sl, *reinterpret_cast<MinimizeArgs<1>*>(&h_ma[slot_i])); break;
                case 2: rc = build_minimize_args<2>(c, sl, *reinterpret_cast<MinimizeArgs<2>*>(&h_ma[slot_i])); break;
                default: rc = build_minimize_args<3>(c, sl, *reinterpret_cast<MinimizeArgs<3>*>(&h_ma[slot_i])); break;
            }
            if (rc) return rc;
            if (c != lead) HIP_TRY(hipStreamSynchronize(c->stream));  // (its gate slot may just have been staged on its own stream)
            SpanLoopStep step{success_threshold, true, k < k_max, success_threshold, nxt[(size_t)i]->as<int32_t>()};
            const ReduceArgs r = build_reduce_args(c, k, 6 * (k + 1), d_active[(size_t)i], prm, success_threshold, true);
            h_ep[slot_i] = build_epilogue_args(c, k, r, step);
        }
        HIP_TRY(hipMemcpyAsync(d, h, slot, hipMemcpyHostToDevice, lead->stream));
        HIP_TRY(hipEventRecord(lead->ev_a[k], lead->stream));
        for (int lo = 0; lo < n;) {
            const int gc = cls[(size_t)order[(size_t)lo]];
            int hi = lo;
            while (hi < n && cls[(size_t)order[(size_t)hi]] == gc) ++hi;
            const int cnt = hi - lo;
            const int64_t items_total = (int64_t)cnt * N * prm->restarts;
            auto launch = [&](auto kc) -> int {
                constexpr int KK = decltype(kc)::value;
                const MinimizeArgs<KK>& a0 = *reinterpret_cast<const MinimizeArgs<KK>*>(&h_ma[lo]);
                const MinimizeArgs<KK>* dsub = reinterpret_cast<const MinimizeArgs<KK>*>(d) + lo;
                return with_gate_class(gc, [&](auto g) -> int { return launch_minimize_multi<KK, decltype(g)::value>(lead, a0, dsub, cnt, items_total); });
            };
            switch (k) {
                case 1: rc = launch(std::integral_constant<int, 1>{}); break;
                case 2: rc = launch(std::integral_constant<int, 2>{}); break;
                case 3: rc = launch(std::integral_constant<int, 3>{}); break;
                default: return fail(SLAM_ERR_UNSUPPORTED, "slam_decompose_multi runs spans 1..3");
            }
            if (rc) return rc;
            lead->stats.kernel_launches += 1;
            lo = hi;
        }
        HIP_TRY(hipEventRecord(lead->ev_b[k], lead->stream));
        hipLaunchKernelGGL(stage_epilogue_multi_kernel, dim3((unsigned)((N + 255) / 256), (unsigned)n), dim3(256), 0, lead->stream,
                           reinterpret_cast<const EpilogueArgs*>(d + (size_t)n * sz_ma));
        HIP_TRY(hipGetLastError());
        gs += k;
        if (k < k_max)
            for (int i = 0; i < n; ++i) {
                d_active[(size_t)i] = nxt[(size_t)i]->as<int32_t>();
                DevBuf* t = cur[(size_t)i]; cur[(size_t)i] = nxt[(size_t)i]; nxt[(size_t)i] = t;
            }
    }
    HIP_TRY(hipEventRecord(lead->ev_t1, lead->stream));
    for (int i = 0; i < n; ++i)
        HIP_TRY(hipMemcpyAsync(cs[i]->h_ctl, cs[i]->counters.p, sizeof(StageCtl) * (SLAM_MAX_SPAN_EVAL + 2), hipMemcpyDeviceToHost, lead->stream));
    HIP_TRY(hipEventRecord(lead->ev_done, lead->stream));
    HIP_TRY(hipEventSynchronize(lead->ev_done));
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, lead->ev_t0, lead->ev_t1));
    lead->stats.total_ms = ms;
    // statistics: every context gets the evaluations / items of its own queues; the kernels' time goes to the leading context
    for (int i = 0; i < n; ++i) fold_counters(cs[i]->stats, cs[i]->h_ctl, k_min, k_max, prm->restarts, FOLD_SKIP_IDLE);
    for (int k = k_min; k <= k_max; ++k) {
        float kms = 0.f;
        HIP_TRY(hipEventElapsedTime(&kms, lead->ev_a[k], lead->ev_b[k]));
        lead->stats.kernel_ms += kms;
        lead->stats.kernel_ms_span[k] += kms;
    }
    return SLAM_OK;
}

int decompose_multi_impl(slam_ctx** cs, int n, int64_t first, int64_t count, int k_min, int k_max, const int32_t* gate_seqs,
                         const slam_opt_params* prm, double success_threshold) {
    const int rc = decompose_multi_body(cs, n, first, count, k_min, k_max, gate_seqs, prm, success_threshold);
    if (rc != SLAM_OK && cs)
        for (int i = 0; i < n; ++i)
            if (cs[i]) (void)drained(cs[i], rc);  // (the work sits on ctxs[0]'s stream; every context forgets its cached gate slots)
    return rc;
}

// ---- hardware queues, asked for when the library loads (include/slam_hip.h: slam_hw_queues_requested) ----
// The HIP runtime maps every stream of the process onto GPU_MAX_HW_QUEUES hardware queues (its default: 4) and reads that variable
// once, when its first call initialises it.  Streams that share a queue serialise, and the library lives on contexts that run side by
// side: each has its own stream, and the speculative / overlapped spans add streams inside a call.  So the library raises the variable
// itself, in the earliest constructor the toolchain gives a shared object (priorities up to 100 belong to the implementation).  No HIP
// call is made here: the runtime stays uninitialised until the first real entry point.
constexpr long HWQ_DEFAULT = 16, HWQ_MIN = 4, HWQ_MAX = 32;
int g_hw_queues = 0;  // the value in force after the constructor ran; 0 = switched off

// leading decimal digits as atoi reads them (what the runtime does with the variable); -1 = none
long env_number(const char* s) {
    if (!s) return -1;
    char* end = nullptr;
    const long v = std::strtol(s, &end, 10);
    return end == s ? -1 : v;
}

__attribute__((constructor(101))) void request_hw_queues() {
    long want = HWQ_DEFAULT;
    if (const char* own = std::getenv("SLAM_HW_QUEUES")) {
        char* end = nullptr;
        const long v = std::strtol(own, &end, 10);
        const bool whole = end != own && *end == '\0';
        if (whole && v == 0) return;  // the integrator keeps their own number
        if (whole && v >= HWQ_MIN && v <= HWQ_MAX) want = v;
    }
    const long have = env_number(std::getenv("GPU_MAX_HW_QUEUES"));
    if (have >= want) {  // never lowered; a value above HWQ_MAX is the caller's and is not written here
        g_hw_queues = have > 0x7fffffffL ? 0x7fffffff : (int)have;
        return;
    }
    char buf[8];
    snprintf(buf, sizeof(buf), "%ld", want);
    if (setenv("GPU_MAX_HW_QUEUES", buf, 1) == 0) g_hw_queues = (int)want;
    else g_hw_queues = have > 0 ? (int)have : 0;
}

}  // namespace

extern "C" {

int slam_hw_queues_requested(void) { return g_hw_queues; }

const char* slam_last_error(void) { return g_err.c_str(); }

const char* slam_version(void) { return "slamhip 0.4.0 (gfx950)"; }

int slam_abi_version(void) { return SLAM_ABI_VERSION; }

int slam_device_count(int* count) {
    if (!count) return fail(SLAM_ERR_INVALID, "count is NULL");
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) {
        *count = 0;
        return fail(SLAM_ERR_HIP, "hipGetDeviceCount failed: %s", hipGetErrorString(e));
    }
    *count = n;
    return SLAM_OK;
}

int slam_ctx_create(int device, slam_ctx** out) {
    if (!out) return fail(SLAM_ERR_INVALID, "out is NULL");
    *out = nullptr;
    int n = 0;
    HIP_TRY(hipGetDeviceCount(&n));
    if (device < 0 || device >= n) return fail(SLAM_ERR_INVALID, "device %d out of range (%d visible)", device, n);
    HIP_TRY(hipSetDevice(device));
    if (const char* e = std::getenv("SLAM_HOST_WAIT")) {
        // tuning knob: how the HIP runtime's own waits behave on this device (block / yield / spin)
        const unsigned fl = e[0] == 'b' ? hipDeviceScheduleBlockingSync : (e[0] == 'y' ? hipDeviceScheduleYield : hipDeviceScheduleSpin);
        if (hipSetDeviceFlags(fl) != hipSuccess) (void)hipGetLastError();
    }
    slam_ctx* c = new (std::nothrow) slam_ctx();
    if (!c) return fail(SLAM_ERR_NOMEM, "out of host memory");
    c->device = device;
    if (const char* e = std::getenv("SLAM_RESERVE_WAVES")) c->reserve_waves = std::atoi(e) > 0 ? std::atoi(e) : 0;
    hipError_t e = hipStreamCreateWithFlags(&c->stream.h, hipStreamNonBlocking);
    for (int k = 0; k <= SLAM_MAX_SPAN_EVAL && e == hipSuccess; ++k) {
        e = hipEventCreate(&c->ev_a[k].h);
        if (e == hipSuccess) e = hipEventCreate(&c->ev_b[k].h);
    }
    if (e == hipSuccess) e = hipEventCreate(&c->ev_t0.h);
    if (e == hipSuccess) e = hipEventCreate(&c->ev_t1.h);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&c->ev_done.h, hipEventBlockingSync | hipEventDisableTiming);

    if (e == hipSuccess) e = c->h_ctl.reserve(sizeof(StageCtl) * (SLAM_MAX_SPAN_EVAL + 2));
    if (e == hipSuccess) e = c->counters.reserve(sizeof(StageCtl) * (SLAM_MAX_SPAN_EVAL + 2));
    if (e == hipSuccess) e = c->span_gates.reserve((size_t)64 * SLAM_MAX_SPAN_EVAL * 32 * sizeof(double));
    if (e == hipSuccess) e = c->h_gates.reserve((size_t)64 * SLAM_MAX_SPAN_EVAL * 32 * sizeof(double));
    if (e == hipSuccess) {
        hipDeviceProp_t prop;
        e = hipGetDeviceProperties(&prop, device);
        if (e == hipSuccess) c->compute_units = prop.multiProcessorCount;
    }
    if (e != hipSuccess) {
        delete c;
        return fail(SLAM_ERR_HIP, "context setup failed: %s", hipGetErrorString(e));
    }
    *out = c;
    return SLAM_OK;
}

int slam_ctx_destroy(slam_ctx* ctx) {
    if (!ctx) return SLAM_OK;
    (void)hipSetDevice(ctx->device);
    if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
    delete ctx;
    return SLAM_OK;
}

int slam_ctx_device_info(slam_ctx* ctx, char* name, int name_len, int* compute_units, int* clock_khz) {
    if (!ctx) return fail(SLAM_ERR_INVALID, "ctx is NULL");
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, ctx->device));
    if (name && name_len > 0) {
        snprintf(name, (size_t)name_len, "%s (%s)", prop.name, prop.gcnArchName);
    }
    if (compute_units) *compute_units = prop.multiProcessorCount;
    if (clock_khz) *clock_khz = prop.clockRate;
    return SLAM_OK;
}

int slam_set_targets(slam_ctx* ctx, const double* targets, int64_t n_targets) {
    if (!ctx) return fail(SLAM_ERR_INVALID, "ctx is NULL");
    if (!targets || n_targets <= 0) return fail(SLAM_ERR_INVALID, "targets must be non-empty");
    if (n_targets > 0x7fffffffLL) return fail(SLAM_ERR_INVALID, "too many targets");
    HIP_TRY(hipSetDevice(ctx->device));
    const size_t bytes = (size_t)n_targets * 32 * sizeof(double);
    HIP_TRY(ctx->targets.reserve(bytes));
    HIP_TRY(hipMemcpyAsync(ctx->targets.p, targets, bytes, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    ctx->n_targets = n_targets;
    ctx->result_nmax = 0;
    ctx->result_filled = 0;
    return SLAM_OK;
}

int slam_set_gates(slam_ctx* ctx, const double* gates, int32_t n_gates) {
    if (!ctx) return fail(SLAM_ERR_INVALID, "ctx is NULL");
    if (!gates || n_gates <= 0 || n_gates > SLAM_MAX_GATES)
        return fail(SLAM_ERR_INVALID, "n_gates must be in 1..%d", SLAM_MAX_GATES);
    HIP_TRY(hipSetDevice(ctx->device));
    const size_t bytes = (size_t)n_gates * 32 * sizeof(double);
    HIP_TRY(ctx->gates.reserve(bytes));
    HIP_TRY(hipMemcpyAsync(ctx->gates.p, gates, bytes, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    ctx->gates_host.assign(gates, gates + (size_t)n_gates * 32);
    ctx->n_gates = n_gates;
    ++ctx->gates_version;
    for (auto& st : ctx->staged) st.valid = false;
    return SLAM_OK;
}

static int eval_body(slam_ctx* ctx, int k, const int32_t* gate_seq, const double* x, const int32_t* target_of,
                     int64_t M, double* loss, double* grad, double* unitary, double* weyl, int ndigits) {
    if (!ctx) return fail(SLAM_ERR_INVALID, "ctx is NULL");
    HIP_TRY(hipSetDevice(ctx->device));
    if (ctx->n_targets <= 0) return fail(SLAM_ERR_STATE, "no targets: call slam_set_targets first");
    if (ctx->n_gates <= 0) return fail(SLAM_ERR_STATE, "no gates: call slam_set_gates first");
    if (k < 1 || k > SLAM_MAX_SPAN_EVAL) return fail(SLAM_ERR_UNSUPPORTED, "span must be in 1..%d (got %d)", SLAM_MAX_SPAN_EVAL, k);
    if (M < 0) return fail(SLAM_ERR_INVALID, "M < 0");
    if (M == 0) return SLAM_OK;
    if (!x || !target_of || !loss) return fail(SLAM_ERR_INVALID, "x, target_of and loss must be non-NULL");
    int rc = check_gate_seq(ctx, k, gate_seq);
    if (rc) return rc;
    const int n = 6 * (k + 1);
    if (weyl) HIP_TRY(ctx->ev_weyl.reserve((size_t)M * 3 * sizeof(double)));
    EvalBufs d{};
    rc = stage_eval_inputs(ctx, x, target_of, M, n, grad != nullptr, unitary || weyl, &d);
    if (rc) return rc;
    const int gc = classify_gates(ctx, k, gate_seq);
    switch (k) {
        case 1: rc = launch_eval_gc<1>(ctx, gc, gate_seq, d.x, d.target_of, M, d.loss, d.grad, d.unitary); break;
        case 2: rc = launch_eval_gc<2>(ctx, gc, gate_seq, d.x, d.target_of, M, d.loss, d.grad, d.unitary); break;
        case 3: rc = launch_eval_gc<3>(ctx, gc, gate_seq, d.x, d.target_of, M, d.loss, d.grad, d.unitary); break;
        case 4: rc = launch_eval_gc<4>(ctx, gc, gate_seq, d.x, d.target_of, M, d.loss, d.grad, d.unitary); break;
        case 5: rc = launch_eval_gc<5>(ctx, gc, gate_seq, d.x, d.target_of, M, d.loss, d.grad, d.unitary); break;
        default: rc = launch_eval_long(ctx, k, gate_seq, d.x, d.target_of, M, d.loss, d.grad, d.unitary); break;  // SLAM_MAX_SPAN_QUAD < k: one wavefront per item
    }
    if (rc) return rc;
    rc = enqueue_eval_readback(ctx, M, n, loss, grad, unitary);
    if (rc) return rc;
    if (weyl) {
        // Weyl coordinates of the template unitaries without bringing the unitaries back (optimizer.py:85,103)
        rc = enqueue_c1c2c3(ctx, ctx->ev_unitary.as<double>(), M, ndigits, ctx->ev_weyl.as<double>());
        if (rc) return rc;
        HIP_TRY(hipMemcpyAsync(weyl, ctx->ev_weyl.p, (size_t)M * 3 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    }
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return SLAM_OK;
}

static int eval_impl(slam_ctx* ctx, int k, const int32_t* gate_seq, const double* x, const int32_t* target_of,
                     int64_t M, double* loss, double* grad, double* unitary, double* weyl = nullptr, int ndigits = 8) {
    return drained(ctx, eval_body(ctx, k, gate_seq, x, target_of, M, loss, grad, unitary, weyl, ndigits));
}

int slam_eval_loss_grad(slam_ctx* ctx, int k, const int32_t* gate_seq, const double* x, const int32_t* target_of,
                        int64_t M, double* loss, double* grad) {
    return eval_impl(ctx, k, gate_seq, x, target_of, M, loss, grad, nullptr);
}

int slam_eval_unitary(slam_ctx* ctx, int k, const int32_t* gate_seq, const double* x, const int32_t* target_of,
                      int64_t M, double* unitary, double* loss) {
    if (!unitary) return fail(SLAM_ERR_INVALID, "unitary is NULL");
    std::vector<double> tmp;
    if (!loss && M > 0) {
        tmp.resize((size_t)M);
        loss = tmp.data();
    }
    return eval_impl(ctx, k, gate_seq, x, target_of, M, loss, nullptr, unitary);
}

static int minimize_stage_body(slam_ctx* ctx, int k, const int32_t* gate_seq, const int32_t* active, int64_t n_active,
                        const double* x0, const slam_opt_params* params, double* best_loss, double* best_x,
                        int32_t* best_restart, double* item_loss, int32_t* item_iters, int32_t* item_status,
                        int32_t* item_evals) {
    if (!ctx) return fail(SLAM_ERR_INVALID, "ctx is NULL");
    HIP_TRY(hipSetDevice(ctx->device));
    if (ctx->n_targets <= 0) return fail(SLAM_ERR_STATE, "no targets: call slam_set_targets first");
    if (ctx->n_gates <= 0) return fail(SLAM_ERR_STATE, "no gates: call slam_set_gates first");
    if (k < 1 || k > SLAM_MAX_SPAN_MINIMIZE)
        return fail(SLAM_ERR_UNSUPPORTED, "minimize supports spans 1..%d (got %d)", SLAM_MAX_SPAN_MINIMIZE, k);
    int rc = check_params(params);
    if (rc) return rc;
    rc = check_gate_seq(ctx, k, gate_seq);
    if (rc) return rc;
    if (!active) n_active = ctx->n_targets;
    if (n_active < 0) return fail(SLAM_ERR_INVALID, "n_active < 0");
    if (n_active == 0) return SLAM_OK;
    if (!best_loss || !best_x) return fail(SLAM_ERR_INVALID, "best_loss and best_x must be non-NULL");
    const int n = 6 * (k + 1);
    const int64_t M = n_active * (int64_t)params->restarts;
    const int32_t* d_active = nullptr;
    rc = upload_stage_active(ctx, active, n_active, &d_active);
    if (rc) return rc;
    const double* d_x0 = nullptr;
    rc = upload_stage_x0(ctx, x0, M * n, &d_x0);
    if (rc) return rc;
    rc = reserve_stage_buffers(ctx, n_active, k, params);
    if (rc) return rc;
    HIP_TRY(hipEventRecord(ctx->ev_t0, ctx->stream));
    HIP_TRY(hipMemsetAsync(ctx->counters.p, 0, sizeof(StageCtl) * (SLAM_MAX_SPAN_EVAL + 2), ctx->stream));
    hipLaunchKernelGGL(set_n_active_kernel, dim3(1), dim3(1), 0, ctx->stream, stage_ctl(ctx, k), (int32_t)n_active);
    HIP_TRY(hipGetLastError());
    rc = enqueue_stage(ctx, k, gate_seq, d_active, n_active, d_x0, params, nullptr);
    if (rc) return rc;
    rc = enqueue_loop_end(ctx, nullptr, 0, 0, 0);
    if (rc) return rc;
    rc = wait_loop_end(ctx, nullptr);  // sleep until the stage is done; the copies below then find an idle stream
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(best_loss, ctx->stage_loss.p, (size_t)n_active * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipMemcpyAsync(best_x, ctx->stage_x.p, (size_t)n_active * n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    if (best_restart) HIP_TRY(hipMemcpyAsync(best_restart, ctx->stage_restart.p, (size_t)n_active * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    rc = fetch_item_records(ctx, M, item_loss, item_iters, item_status, item_evals);
    if (rc) return rc;
    return collect_stats(ctx, k, k, ctx->h_ctl, params->restarts);
}

int slam_minimize_stage(slam_ctx* ctx, int k, const int32_t* gate_seq, const int32_t* active, int64_t n_active,
                        const double* x0, const slam_opt_params* params, double* best_loss, double* best_x,
                        int32_t* best_restart, double* item_loss, int32_t* item_iters, int32_t* item_status,
                        int32_t* item_evals) {
    return drained(ctx, minimize_stage_body(ctx, k, gate_seq, active, n_active, x0, params, best_loss, best_x, best_restart,
                                            item_loss, item_iters, item_status, item_evals));
}

int slam_decompose_resident(slam_ctx* ctx, int k_min, int k_max, const int32_t* gate_seqs,
                            const slam_opt_params* params, double success_threshold) {
    if (!ctx) return fail(SLAM_ERR_INVALID, "ctx is NULL");
    return decompose_impl(ctx, 0, ctx->n_targets, k_min, k_max, gate_seqs, params, success_threshold);
}

int slam_decompose_range(slam_ctx* ctx, int64_t first, int64_t count, int k_min, int k_max,
                         const int32_t* gate_seqs, const slam_opt_params* params, double success_threshold) {
    if (!ctx) return fail(SLAM_ERR_INVALID, "ctx is NULL");
    return decompose_impl(ctx, first, count, k_min, k_max, gate_seqs, params, success_threshold);
}

int slam_decompose_list(slam_ctx* ctx, const int32_t* targets, int64_t count, int k_min, int k_max, int k_layout,
                        const int32_t* gate_seqs, const slam_opt_params* params, double success_threshold) {
    if (!ctx) return fail(SLAM_ERR_INVALID, "ctx is NULL");
    if (!targets) return fail(SLAM_ERR_INVALID, "targets is NULL");
    return decompose_impl(ctx, 0, count, k_min, k_max, gate_seqs, params, success_threshold, targets, k_layout);
}

// -----------------------------------------------------------------------------------------------------------------------
// slam_decompose_predicted: CircuitTemplate(use_polytopes=True) for a window of RESIDENT targets without a host step in between --
// the coverage lookup (span_predict_kernel), the per-size target lists (span_bucket_kernel) and ONE span loop in which the targets of
// size k join the loop at stage k.  carry = 0: a target runs at its own size only (exact regions: basis.py:95-100 returns
// range(k, k + 1)); carry = 1: targets that miss the threshold go on to the next size (regions widened by `tol`, lower bounds).
// Replaces the host's np.nonzero + one slam_decompose_list per size (round 4).
// -----------------------------------------------------------------------------------------------------------------------
int decompose_predicted_body(slam_ctx* c, int64_t first, int64_t count, int k_max, const double* point, const double* bounds, double tol,
                             int carry, const int32_t* gate_seqs, const slam_opt_params* prm, double success_threshold,
                             int64_t* n_local, int64_t* n_unreachable) {
    HIP_TRY(hipSetDevice(c->device));
    if (c->n_targets <= 0) return fail(SLAM_ERR_STATE, "no targets");
    if (c->n_gates <= 0) return fail(SLAM_ERR_STATE, "no gates");
    if (first < 0 || count <= 0 || first + count > c->n_targets) return fail(SLAM_ERR_INVALID, "target window outside the resident batch");
    if (k_max < 1 || k_max > SLAM_MAX_SPAN_MINIMIZE) return fail(SLAM_ERR_INVALID, "k_max must be 1..%d (got %d)", SLAM_MAX_SPAN_MINIMIZE, k_max);
    if (!point || (k_max > 1 && !bounds) || !gate_seqs) return fail(SLAM_ERR_INVALID, "point / bounds / gate_seqs is NULL");
    int rc = check_params(prm);
    if (rc) return rc;
    {
        const int32_t* gs = gate_seqs;
        for (int k = 1; k <= k_max; ++k) {
            rc = check_gate_seq(c, k, gs);
            if (rc) return rc;
            gs += k;
        }
    }
    if (c->result_nmax != 0 && c->result_nmax != 6 * (k_max + 1) && !(first == 0 && count == c->n_targets))
        return fail(SLAM_ERR_STATE, "resident results were produced with a different k_max");
    rc = ensure_results(c, k_max);
    if (rc) return rc;
    const int64_t N = count;
    HIP_TRY(c->active.reserve(N * sizeof(int32_t)));
    HIP_TRY(c->active2.reserve(N * sizeof(int32_t)));
    HIP_TRY(c->bucket_lists.reserve((size_t)k_max * N * sizeof(int32_t)));
    HIP_TRY(c->bucket_counts.reserve((size_t)(SLAM_MAX_SPAN_EVAL + 2) * sizeof(int32_t)));
    HIP_TRY(c->ev_weyl.reserve((size_t)N * sizeof(int32_t)));
    HIP_TRY(c->h_bucket_counts.reserve((SLAM_MAX_SPAN_EVAL + 2) * sizeof(int32_t)));
    rc = reserve_stage_buffers(c, N, k_max, prm);
    if (rc) return rc;
    HIP_TRY(hipEventRecord(c->ev_t0, c->stream));
    const int n_words = (int)(sizeof(StageCtl) * (SLAM_MAX_SPAN_EVAL + 2) / 8);
    hipLaunchKernelGGL(clear_ctl_kernel, dim3((unsigned)((n_words + 255) / 256)), dim3(256), 0, c->stream, c->counters.as<StageCtl>(), n_words,
                       c->bucket_counts.as<int32_t>(), SLAM_MAX_SPAN_EVAL + 2);
    HIP_TRY(hipGetLastError());
    int32_t* d_spans = c->ev_weyl.as<int32_t>();
    rc = enqueue_span_predict(c, first, N, k_max, point, bounds, tol, d_spans);
    if (rc) return rc;
    hipLaunchKernelGGL(span_bucket_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, c->stream, d_spans, first, N, (int32_t)k_max,
                       c->bucket_lists.as<int32_t>(), c->bucket_counts.as<int32_t>(), c->best_loss.as<double>(), c->best_cycles.as<int32_t>(),
                       c->span_loss.as<double>());
    HIP_TRY(hipGetLastError());
    DevBuf* cur = &c->active;
    DevBuf* nxt = &c->active2;
    const int32_t* gs = gate_seqs;
    for (int k = 1; k <= k_max; ++k) {
        // stage k's list: what the previous stage carried over (carry) + the targets of size k
        hipLaunchKernelGGL(stage_append_kernel, dim3(1), dim3(1024), 0, c->stream, c->bucket_lists.as<int32_t>() + (size_t)(k - 1) * N,
                           c->bucket_counts.as<int32_t>() + (k - 1), stage_ctl(c, k), cur->as<int32_t>());
        HIP_TRY(hipGetLastError());
        SpanLoopStep step{success_threshold, false, carry && k < k_max, success_threshold, nxt->as<int32_t>()};
        rc = enqueue_stage(c, k, gs, cur->as<int32_t>(), N, nullptr, prm, &step);
        if (rc) return rc;
        gs += k;
        DevBuf* t = cur; cur = nxt; nxt = t;
    }
    rc = enqueue_loop_end(c, nullptr, 0, 0, 0);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(c->h_bucket_counts, c->bucket_counts.p, (SLAM_MAX_SPAN_EVAL + 2) * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    rc = wait_loop_end(c, nullptr);
    if (rc) return rc;
    if (n_local) *n_local = c->h_bucket_counts[k_max];
    if (n_unreachable) *n_unreachable = c->h_bucket_counts[k_max + 1];
    return collect_stats(c, 1, k_max, c->h_ctl, prm->restarts);
}

int slam_decompose_predicted(slam_ctx* ctx, int64_t first, int64_t count, int k_max, const double* point, const double* bounds, double tol,
                             int carry, const int32_t* gate_seqs, const slam_opt_params* params, double success_threshold,
                             int64_t* n_local, int64_t* n_unreachable) {
    if (!ctx) return fail(SLAM_ERR_INVALID, "ctx is NULL");
    return drained(ctx, decompose_predicted_body(ctx, first, count, k_max, point, bounds, tol, carry, gate_seqs, params, success_threshold, n_local, n_unreachable));
}

int slam_fetch_results_range(slam_ctx* ctx, int k_max, int64_t first, int64_t count, double* best_loss,
                             double* best_x, int32_t* best_cycles) {
    if (!ctx) return fail(SLAM_ERR_INVALID, "ctx is NULL");
    HIP_TRY(hipSetDevice(ctx->device));
    FetchReq fr{best_loss, best_x, best_cycles};
    int rc = enqueue_fetch(ctx, k_max, first, count, fr);
    if (rc) return rc;
    HIP_TRY(hipEventRecord(ctx->ev_done, ctx->stream));
    HIP_TRY(hipEventSynchronize(ctx->ev_done));
    finish_fetch(ctx, fr);
    return SLAM_OK;
}

int slam_decompose_range_fetch(slam_ctx* ctx, int64_t first, int64_t count, int k_min, int k_max, const int32_t* gate_seqs,
                               const slam_opt_params* params, double success_threshold, double* best_loss, double* best_x,
                               int32_t* best_cycles) {
    if (!ctx) return fail(SLAM_ERR_INVALID, "ctx is NULL");
    FetchReq fr{best_loss, best_x, best_cycles};
    return decompose_impl(ctx, first, count, k_min, k_max, gate_seqs, params, success_threshold, nullptr, 0, &fr);
}

int slam_decompose_multi(slam_ctx** ctxs, int32_t n_ctx, int64_t first, int64_t count, int k_min, int k_max, const int32_t* gate_seqs,
                         const slam_opt_params* params, double success_threshold) {
    return decompose_multi_impl(ctxs, n_ctx, first, count, k_min, k_max, gate_seqs, params, success_threshold);
}

int slam_fetch_results(slam_ctx* ctx, int k_max, double* best_loss, double* best_x, int32_t* best_cycles) {
    if (!ctx) return fail(SLAM_ERR_INVALID, "ctx is NULL");
    return slam_fetch_results_range(ctx, k_max, 0, ctx->n_targets, best_loss, best_x, best_cycles);
}

int slam_decompose(slam_ctx* ctx, int k_min, int k_max, const int32_t* gate_seqs, const slam_opt_params* params,
                   double success_threshold, double* best_loss, double* best_x, int32_t* best_cycles) {
    if (!ctx) return fail(SLAM_ERR_INVALID, "ctx is NULL");
    int rc = decompose_impl(ctx, 0, ctx->n_targets, k_min, k_max, gate_seqs, params, success_threshold);
    if (rc) return rc;
    return slam_fetch_results(ctx, k_max, best_loss, best_x, best_cycles);
}

int slam_eval_c1c2c3(slam_ctx* ctx, int k, const int32_t* gate_seq, const double* x, int64_t M, int ndigits, double* out) {
    if (!out && M > 0) return fail(SLAM_ERR_INVALID, "out is NULL");
    std::vector<int32_t> tof((size_t)(M > 0 ? M : 0), 0);  // the loss is not wanted: any resident target will do
    std::vector<double> loss((size_t)(M > 0 ? M : 0));
    return eval_impl(ctx, k, gate_seq, x, tof.data(), M, loss.data(), nullptr, nullptr, out, ndigits);
}

int slam_fetch_span_losses(slam_ctx* ctx, int64_t first, int64_t count, double* out) {
    if (!ctx) return fail(SLAM_ERR_INVALID, "ctx is NULL");
    if (ctx->result_nmax == 0 || ctx->n_targets <= 0) return fail(SLAM_ERR_STATE, "no resident results");
    if (first < 0 || count < 0 || first + count > ctx->n_targets) return fail(SLAM_ERR_INVALID, "target window outside the resident batch");
    if (count == 0) return SLAM_OK;
    if (!out) return fail(SLAM_ERR_INVALID, "out is NULL");
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipMemcpyAsync(out, ctx->span_loss.as<double>() + first * kSpanLossStride, (size_t)count * kSpanLossStride * sizeof(double),
                           hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return SLAM_OK;
}

int slam_minimize_stage_trace(slam_ctx* ctx, int k, const int32_t* gate_seq, const int32_t* active, int64_t n_active,
                              const double* x0, const slam_opt_params* params, double exit_loss, int32_t trace_cap,
                              double* best_loss, double* best_x, int32_t* best_restart, double* item_loss,
                              int32_t* item_iters, int32_t* item_status, double* trace_loss, double* trace_x) {
    return minimize_stage_trace(
        ctx, active, n_active, params, trace_cap, trace_loss, trace_x,
        [&](int* n) {
            if (k < 1 || k > SLAM_MAX_SPAN_MINIMIZE) return fail(SLAM_ERR_UNSUPPORTED, "per-iteration traces are recorded for spans 1..%d (got %d)", SLAM_MAX_SPAN_MINIMIZE, k);
            *n = 6 * (k + 1);
            return (int)SLAM_OK;
        },
        [&] {
            ctx->stage_exit_loss = exit_loss;
            const int rc = slam_minimize_stage(ctx, k, gate_seq, active, n_active, x0, params, best_loss, best_x, best_restart, item_loss, item_iters,
                                               item_status, nullptr);
            ctx->stage_exit_loss = -1.0;
            return rc;
        });
}

int slam_set_cost(slam_ctx* ctx, int cost) {
    if (!ctx) return fail(SLAM_ERR_INVALID, "ctx is NULL");
    if (cost != SLAM_COST_BASIC && cost != SLAM_COST_SQUARE && cost != SLAM_COST_MAKHLIN)
        return fail(SLAM_ERR_INVALID, "Unrecognized Cost Function (%d)", cost);
    ctx->cost_kind = cost;
    return SLAM_OK;
}

int slam_synchronize(slam_ctx* ctx) {
    if (!ctx) return fail(SLAM_ERR_INVALID, "ctx is NULL");
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return SLAM_OK;
}

int slam_host_alloc(size_t bytes, void** ptr) {
    if (!ptr) return fail(SLAM_ERR_INVALID, "ptr is NULL");
    *ptr = nullptr;
    if (bytes == 0) return fail(SLAM_ERR_INVALID, "bytes == 0");
    HIP_TRY(hipHostMalloc(ptr, bytes, hipHostMallocPortable));
    return SLAM_OK;
}

int slam_host_free(void* ptr) {
    if (!ptr) return SLAM_OK;
    HIP_TRY(hipHostFree(ptr));
    return SLAM_OK;
}

int slam_get_stats(slam_ctx* ctx, slam_stats* out) {
    if (!ctx || !out) return fail(SLAM_ERR_INVALID, "NULL argument");
    *out = ctx->stats;
    return SLAM_OK;
}

int slam_reset_stats(slam_ctx* ctx) {
    if (!ctx) return fail(SLAM_ERR_INVALID, "ctx is NULL");
    ctx->stats = slam_stats{};
    return SLAM_OK;
}

int slam_ctx_device(slam_ctx* ctx, int* device) {
    if (!ctx || !device) return fail(SLAM_ERR_INVALID, "NULL argument");
    *device = ctx->device;
    return SLAM_OK;
}

int slam_best_loss_device_ptr(slam_ctx* ctx, void** ptr, int64_t* n) {
    if (!ctx || !ptr || !n) return fail(SLAM_ERR_INVALID, "NULL argument");
    if (!ctx->best_loss.p || ctx->n_targets <= 0) return fail(SLAM_ERR_STATE, "no resident results");
    *ptr = ctx->best_loss.p;
    *n = ctx->n_targets;
    return SLAM_OK;
}

int slam_metric_update_check(slam_ctx* ctx, int na, const float* h, const float* s, const float* w, const float* v, int64_t n_items,
                             float* h_shipped, float* h_vector) {
    if (!ctx) return fail(SLAM_ERR_INVALID, "ctx is NULL");
    if (na != 3 && na != 5 && na != 6) return fail(SLAM_ERR_UNSUPPORTED, "na must be 3, 5 or 6 (spans 1, 2, 3; got %d)", na);
    if (n_items < 0) return fail(SLAM_ERR_INVALID, "n_items < 0");
    if (n_items > (1 << 20)) return fail(SLAM_ERR_INVALID, "too many items in one call (%lld)", (long long)n_items);
    if (n_items == 0) return SLAM_OK;
    if (!h || !s || !w || !v) return fail(SLAM_ERR_INVALID, "h, s, w and v must be non-NULL");
    if (!h_shipped || !h_vector) return fail(SLAM_ERR_INVALID, "h_shipped and h_vector must be non-NULL");
    const size_t h_b = (size_t)n_items * (na * (na + 1) / 2) * 16 * sizeof(float), vec_b = (size_t)n_items * 4 * na * sizeof(float);
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(ctx->ev_x.reserve(h_b + 3 * vec_b));  // h, s, w, v
    HIP_TRY(ctx->ev_grad.reserve(2 * h_b));       // both results
    char* in = ctx->ev_x.as<char>();
    char* out = ctx->ev_grad.as<char>();
    HIP_TRY(hipMemcpyAsync(in, h, h_b, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipMemcpyAsync(in + h_b, s, vec_b, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipMemcpyAsync(in + h_b + vec_b, w, vec_b, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipMemcpyAsync(in + h_b + 2 * vec_b, v, vec_b, hipMemcpyHostToDevice, ctx->stream));
    const dim3 grid((unsigned)((n_items + kQuadsPerWave - 1) / kQuadsPerWave)), block(kWave);
    auto launch = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, grid, block, 0, ctx->stream, reinterpret_cast<const float*>(in), reinterpret_cast<const float*>(in + h_b),
                           reinterpret_cast<const float*>(in + h_b + vec_b), reinterpret_cast<const float*>(in + h_b + 2 * vec_b), n_items,
                           reinterpret_cast<float*>(out), reinterpret_cast<float*>(out + h_b));
    };
    if (na == 3) launch(metric_update_check_kernel<3>);
    else if (na == 5) launch(metric_update_check_kernel<5>);
    else launch(metric_update_check_kernel<6>);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(h_shipped, out, h_b, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipMemcpyAsync(h_vector, out + h_b, h_b, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return SLAM_OK;
}

}  // extern "C"
