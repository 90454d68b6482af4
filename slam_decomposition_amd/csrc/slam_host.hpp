// slam_host.hpp -- what the host units of libslamhip.so share (internal: not installed, not part of the C ABI).
// The units: slam_hip.hip (context, plain templates, the decompose family), slam_v2_host.hip, slam_smush_host.hip,
// slam_geometry.hip, slam_analytic.hip, slam_q3_host.hip, slam_ham_host.hip, slam_hams_host.hip and slam_comm.hip.  Every __global__ kernel is emitted by exactly one of them: a header that defines
// kernels (slam_kernels.hpp, slam_long_kernels.hpp, slam_geometry_kernels.hpp, ...) is included by its owner alone, and the headers that
// several units include (slam_weyl.hpp, slam_pd.hpp, slam_kak.hpp) hold __device__ functions only.  Where a unit needs another unit's
// kernel it calls the enqueue_* function of the owner declared below.  Everything declared here has hidden visibility.
#pragma once
#include "../../include/slam_hip.h"
#include "slam_types.hpp"

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <new>
#include <string>
#include <type_traits>
#include <algorithm>
#include <utility>
#include <vector>

using namespace slamdev;

#define SLAM_INTERNAL __attribute__((visibility("hidden")))

// records the calling thread's error message (slam_last_error) and returns `code`
SLAM_INTERNAL int fail(int code, const char* fmt, ...);

#define HIP_TRY(expr)                                                                            \
    do {                                                                                         \
        hipError_t _e = (expr);                                                                  \
        if (_e != hipSuccess)                                                                    \
            return fail(SLAM_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
    } while (0)

// The owners of a context's device resources: four small move-only types (declaring the moves deletes the copies), each empty until
// its resource exists, each releasing it in its destructor.

// growable device buffer; owns its allocation unless it borrows another buffer's (borrow / unborrow)
struct SLAM_INTERNAL DevBuf {
    void* p = nullptr;
    size_t cap = 0;
    bool borrowed = false;
    DevBuf() = default;
    DevBuf(DevBuf&& o) noexcept : p(o.p), cap(o.cap), borrowed(o.borrowed) { o.p = nullptr, o.cap = 0, o.borrowed = false; }
    DevBuf& operator=(DevBuf&& o) noexcept { std::swap(p, o.p), std::swap(cap, o.cap), std::swap(borrowed, o.borrowed); return *this; }
    ~DevBuf() { release(); }
    hipError_t reserve(size_t bytes) {
        if (bytes <= cap) return hipSuccess;
        if (borrowed) return hipErrorInvalidValue;  // the owner's allocation is not this buffer's to free
        if (p) {
            hipError_t e = hipFree(p);
            p = nullptr;
            cap = 0;
            if (e != hipSuccess) return e;
        }
        size_t want = bytes + bytes / 4 + 256;
        hipError_t e = hipMalloc(&p, want);
        if (e != hipSuccess) {
            want = bytes;
            e = hipMalloc(&p, want);
        }
        if (e == hipSuccess) cap = want;
        return e;
    }
    // a view of owner's allocation for as long as the owner keeps it; never freed from here
    void borrow(const DevBuf& owner) {
        release();
        p = owner.p;
        cap = owner.cap;
        borrowed = true;
    }
    void unborrow() { if (borrowed) release(); }
    template <class T>
    T* as() { return static_cast<T*>(p); }

private:
    void release() {
        if (p && !borrowed) (void)hipFree(p);
        p = nullptr;
        cap = 0;
        borrowed = false;
    }
};

// pinned host block of T (hipHostMallocDefault); reserve keeps the block when it is big enough, contents are not carried over
template <class T>
struct SLAM_INTERNAL PinnedBuf {
    T* p = nullptr;
    size_t cap = 0;  // bytes
    PinnedBuf() = default;
    PinnedBuf(PinnedBuf&& o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr, o.cap = 0; }
    PinnedBuf& operator=(PinnedBuf&& o) noexcept { std::swap(p, o.p), std::swap(cap, o.cap); return *this; }
    ~PinnedBuf() { if (p) (void)hipHostFree(p); }
    hipError_t reserve(size_t bytes) {
        if (bytes <= cap) return hipSuccess;
        if (p) (void)hipHostFree(p);
        p = nullptr;
        cap = 0;
        hipError_t e = hipHostMalloc(reinterpret_cast<void**>(&p), bytes, hipHostMallocDefault);
        if (e == hipSuccess) cap = bytes;
        return e;
    }
    operator T*() const { return p; }
};

// an event or a stream: created in place (&x.h) where it always was, converts to the raw handle
template <class T, hipError_t (*Destroy)(T)>
struct SLAM_INTERNAL Handle {
    T h = nullptr;
    Handle() = default;
    Handle(Handle&& o) noexcept : h(o.h) { o.h = nullptr; }
    Handle& operator=(Handle&& o) noexcept { std::swap(h, o.h); return *this; }
    ~Handle() { if (h) (void)Destroy(h); }
    operator T() const { return h; }
};
using Event = Handle<hipEvent_t, hipEventDestroy>;
using Stream = Handle<hipStream_t, hipStreamDestroy>;

// Declaration order is the teardown order, reversed: the streams come first, so every buffer, pinned block and event is released
// before the stream it was used on is destroyed; `helper` follows `targets`, so the helpers (which borrow targets inside a call) go first.
struct slam_ctx {
    int device = 0;
    Stream stream;
    Stream spec_stream[2];  // speculative spans (span_spec_kernel): two side streams
    Event ev_a[SLAM_MAX_SPAN_EVAL + 1], ev_b[SLAM_MAX_SPAN_EVAL + 1];  // optimizer-kernel bracket per span
    Event ev_t0, ev_t1;                          // whole-call bracket
    // The host waits for a finished span loop on a blocking-sync event: the waiting thread sleeps instead of
    // spinning, so that many contexts (one host thread each) can be in flight without the threads fighting
    // over cores.  (Measured: with spinning waits, 32 batches in flight run 30 % slower than 16.)
    Event ev_done;
    PinnedBuf<StageCtl> h_ctl;                   // the stages' control blocks, copied back once per call
    PinnedBuf<double> h_gates;                   // mirror of span_gates
    PinnedBuf<void> h_stage;                     // staging for result fetches (same reason: no spinning inside the
                                                 // runtime's pageable-copy path)
    int64_t n_targets = 0;
    int32_t n_gates = 0;
    DevBuf targets, gates;
    // stage work buffers
    DevBuf active, active2, x0;
    DevBuf item_rec, item_x;  // per work item: one 32-byte result record (slam_types.hpp: ItemRec), the parameter row
    DevBuf stage_loss, stage_x, stage_restart;
    // decompose results
    DevBuf best_loss, best_x, best_cycles, span_loss;
    DevBuf v2_hmem;              // inverse Hessians of the long parametrised-gate templates (slam_v2.hpp: v2_h_in_memory)
    DevBuf v2_maps, v2_bounds;   // slam_v2_*: staged gate maps [SLAM_MAX_SPAN_EVAL], (init_lo, init_hi, bound_lo, bound_hi)[n]
    std::vector<V2GateMap> v2_gates_host;
    int v2_qn = 0;
    // cost constraint per span (slam_v2_set_constraint): weights [n(k)] on the device, right-hand side; empty = none
    DevBuf v2_cons_w[SLAM_V2_MAX_SPAN + 1];
    int v2_cons_n[SLAM_V2_MAX_SPAN + 1] = {0};
    double v2_cons_max[SLAM_V2_MAX_SPAN + 1] = {0};
    double v2_cons_rho[SLAM_V2_MAX_SPAN + 1] = {0};  // penalty parameter of the multiplier method: 30 / max_i w_i^2
    DevBuf trace_loss, trace_x;  // slam_minimize_stage_trace
    int32_t trace_cap = 0;       // > 0 only inside slam_minimize_stage_trace
    double stage_exit_loss = -1.0;  // single-stage calls: >= 0 overrides stop_loss as the ordered early-exit level
    int32_t result_nmax = 0;
    int64_t result_filled = 0;  // targets whose resident results have been initialised (+inf / -1) for result_nmax
    DevBuf counters;  // StageCtl[SLAM_MAX_SPAN_EVAL + 2]: one control block per span stage (slam_types.hpp)
    DevBuf long_hmem;  // inverse Hessian approximations of the wavefront-per-item kernels: [resident wavefronts][n][128] floats
    DevBuf bucket_lists, bucket_counts;  // slam_decompose_predicted: per-size target lists [k_max][count], their sizes
    PinnedBuf<int32_t> h_bucket_counts;  // mirror of bucket_counts
    DevBuf solved;
    DevBuf stage_targets;
    DevBuf span_gates;  // 64 slots x [SLAM_MAX_SPAN_EVAL][32] doubles
    struct StagedSeq { bool valid = false; int32_t seq[SLAM_MAX_SPAN_EVAL] = {}; } staged[SLAM_MAX_SPAN_EVAL + 1];
    int cost_kind = 0;  // SLAM_COST_*
    std::vector<double> gates_host;
    int compute_units = 0;
    int reserve_waves = 0;  // wavefront slots the persistent optimizer grid leaves free for the span loop's bookkeeping kernels
    std::vector<std::pair<const void*, int>> launch_cache;  // kernel_per_cu: (kernel, resident workgroups per CU) of every kernel prepared so far
    // eval buffers
    DevBuf ev_x, ev_tof, ev_loss, ev_grad, ev_unitary, ev_weyl;
    DevBuf cov_table, cov_counts, cov_entries;  // slam_coverage_lookup: offsets / kinds / points / bounds, counts, entry per target
    slam_stats stats{};
    // speculative spans (span_spec_kernel): staging rows, fork / join events
    DevBuf spec_loss, spec_x, spec_ev;
    Event spec_fork, spec_join[2];
    // overlapped spans (decompose_overlapped): one helper context per span (own stream, own stage buffers; targets borrowed)
    std::unique_ptr<slam_ctx> helper[SLAM_MAX_SPAN_EVAL + 1];
    Event ov_fork, ov_join[SLAM_MAX_SPAN_EVAL + 1];
    DevBuf slot_ev;                 // (helper side) per-slot evaluation counts of its stage
    bool slot_ev_on = false;        // (helper side) single-stage reductions write slot_ev instead of the stage's counters
    uint64_t gates_version = 1;     // bumped by slam_set_gates
    uint64_t helper_gates_version = 0;  // (helper side) the owner's gates_version its gate table is a copy of
    // slam_decompose_multi (this context leads the call): the sub-problems' argument blocks / epilogue arguments per span, staged
    // through pinned memory
    DevBuf mq_args;
    PinnedBuf<void> h_mq_args;
    // slam_smush_* (slam_smush.hpp): gate table, staged maps of a span, inverse Hessians of the resident wavefronts
    std::vector<SmushMap> smush_gates_host;
    int smush_qn = 0;
    DevBuf smush_maps, smush_hmem;
    // slam_pd_* / slam_region_lookup (slam_pd.hpp): resident sample coordinates [pd_n][3], per-call staging, region tables
    DevBuf pd_coords, pd_stage, pd_out, reg_table, reg_counts;
    int64_t pd_n = 0;
    // slam_haar_select_spans (slam_span_sampler.hpp): ballot masks per wavefront; votes per block, their scan, the total; selected
    // indices (also the staged index list of slam_sample_haar_indexed); span histogram
    DevBuf sel_masks, sel_blocks, sel_indices, sel_counts;
};

// The one place a kernel with dynamic LDS is prepared.  First call for `fn` on this context: sets MaxDynamicSharedMemorySize = lds and
// asks the occupancy; every call: *per_cu (may be nullptr) = resident workgroups of 64 threads per CU, at least 1.  Keyed by the
// kernel's address and scanned linearly (a process sees a few dozen instantiations); a context is driven by one host thread at a time.
// lds must be the same on every call for fn (it is a function of the instantiation); 64 is kWave, the block size of every kernel
// launched through here.
inline int kernel_per_cu(slam_ctx* c, const void* fn, size_t lds, int* per_cu) {
    int v = 0;
    for (const auto& e : c->launch_cache)
        if (e.first == fn) { v = e.second; break; }
    if (v == 0) {
        HIP_TRY(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&v, fn, 64, lds));
        if (v < 1) v = 1;
        c->launch_cache.emplace_back(fn, v);
    }
    if (per_cu) *per_cu = v;
    return SLAM_OK;
}

// The stage fields that the optimizer kernels' argument blocks (MinimizeArgs, LongArgs, MinimizeV2Args, SmushArgs) spell the same way;
// everything family-specific (more flags, lists, bounds, hmem, ...) is the caller's.
template <class A>
void fill_stage_common(A& a, slam_ctx* c, const slam_opt_params* prm, double exit_loss) {
    a.restarts = prm->restarts;
    a.maxiter = prm->maxiter;
    a.gtol = prm->gtol;
    a.stop_loss = prm->stop_loss;
    a.gtol_far = prm->gtol_far;
    a.far_loss = prm->far_loss;
    a.exit_loss = exit_loss;
    a.seed = prm->seed;
    a.target_base = prm->target_base;
    a.flags = prm->flags & (SLAM_FLAG_EARLY_EXIT | SLAM_FLAG_ORDERED);
    a.cost_kind = c->cost_kind;
    a.solved = c->solved.as<int32_t>();
    a.item_rec = c->item_rec.as<ItemRec>();
    a.item_x = c->item_x.as<double>();
    a.trace_cap = c->trace_cap;
    a.trace_loss = c->trace_cap > 0 ? c->trace_loss.as<double>() : nullptr;
    a.trace_x = c->trace_cap > 0 ? c->trace_x.as<double>() : nullptr;
}

// ---- slam_hip.hip ----------------------------------------------------------------------------------------------------
// Every API call leaves the context's stream drained: the per-span gate slots, the pinned staging buffers and
// DevBuf::reserve's hipFree rely on it.  A call that fails after it has enqueued work therefore waits for that work
// (ignoring the result: the error being reported is the first one) and forgets the cached gate slots.
SLAM_INTERNAL int drained(slam_ctx* c, int rc);
SLAM_INTERNAL int check_params(const slam_opt_params* p);
inline StageCtl* stage_ctl(slam_ctx* c, int k) { return c->counters.as<StageCtl>() + k; }
// After the stream has drained: fold the stages' control blocks and kernel brackets into the statistics.
SLAM_INTERNAL int collect_stats(slam_ctx* c, int k_min, int k_max, const StageCtl* h_ctl, int restarts);
// Resident results with rows of nmax parameters: (re)allocated and, where new, filled with (+inf, -1).
SLAM_INTERNAL int ensure_results_n(slam_ctx* c, int nmax);

// Results of the window [first, first + count) on their way to the host: small windows go through pinned
// staging (asynchronous copies, no spinning inside the runtime's pageable path), big ones straight into the
// caller's arrays.  enqueue_fetch only enqueues; finish_fetch runs after the stream has drained.
struct FetchReq {
    double* best_loss;
    double* best_x;
    int32_t* best_cycles;
    size_t b_loss = 0, b_x = 0, b_cyc = 0;
    bool staged = false;
};

SLAM_INTERNAL int enqueue_fetch_n(slam_ctx* ctx, int nmax, int64_t first, int64_t count, FetchReq& fr);
SLAM_INTERNAL void finish_fetch(slam_ctx* ctx, const FetchReq& fr);

// Per-item results of a single-stage call for the host: the records come over as they are and are unpacked into the
// caller's arrays (any of which may be NULL).  The stream is idle (the caller has waited for the stage).
SLAM_INTERNAL int fetch_item_records(slam_ctx* c, int64_t M, double* item_loss, int32_t* item_iters, int32_t* item_status, int32_t* item_evals);

// The bookkeeping kernels (slam_kernels.hpp), enqueued on behalf of the other units:
// set_n_active_kernel on c's stream: stage k works on n_active targets
SLAM_INTERNAL int enqueue_set_n_active(slam_ctx* c, int k, int64_t n_active);
// init_results_kernel on `stream`: resets the results of the n targets of the window [first, first + n) -- of the list already in
// d_active with list_mode -- clears c's control blocks, publishes n as stage k_min's target count and, with d_active != nullptr,
// writes the first active list and gathers the first stage's targets
SLAM_INTERNAL int enqueue_init_results(slam_ctx* c, hipStream_t stream, int32_t* d_active, int64_t first, int64_t n, int k_min, int list_mode);
// the epilogue of a span-loop stage with at most n_upper targets on c's stream: picks the kernel by n_upper
SLAM_INTERNAL int enqueue_stage_epilogue(slam_ctx* c, int64_t n_upper, const EpilogueArgs& e);

// The end of a span loop, in two halves, so that a caller can enqueue a copy of its own between them.
// First half: records ev_t1, enqueues the fetch of the window [first, first + count) with rows of nmax parameters (fetch may be
// nullptr: nothing to fetch) and sends the control blocks to c->h_ctl.
SLAM_INTERNAL int enqueue_loop_end(slam_ctx* c, FetchReq* fetch, int nmax, int64_t first, int64_t count);
// Second half: records ev_done and sleeps until it has passed, completes the fetch, stats.total_ms = ev_t0 .. ev_t1.
SLAM_INTERNAL int wait_loop_end(slam_ctx* c, const FetchReq* fetch);

// What follows the optimizer kernel of a stage inside a span loop.
struct SpanLoopStep {
    double exit_loss;        // ordered early exit: the span loop's success threshold; otherwise params->stop_loss
    bool inputs_ready;       // the previous kernel of the chain already prepared this stage's inputs
    bool has_next;           // a longer span follows: compact the unsolved targets into active_out
    double threshold;
    int32_t* active_out;
};
// The argument blocks of the reduction over restarts of stage k (rows of n parameters; merge: into the resident results, rows of
// c->result_nmax) and of the span loop's epilogue around it.  A family that differs in a field overrides it after the call.
SLAM_INTERNAL ReduceArgs build_reduce_args(slam_ctx* c, int k, int n, const int32_t* d_active, const slam_opt_params* prm, double exit_loss, bool merge);
SLAM_INTERNAL EpilogueArgs build_epilogue_args(slam_ctx* c, int k, const ReduceArgs& r, const SpanLoopStep& loop);

// The staging of an evaluation call (slam_eval_*, slam_v2_eval_*, slam_smush_eval_*) of M items with rows of n parameters:
// target_of checked, the ev_* buffers reserved, x and target_of on their way to the device; the device pointers the kernel takes
// (grad / unitary: nullptr when not wanted)
struct EvalBufs {
    const double* x;
    const int32_t* target_of;
    double* loss;
    double* grad;
    double* unitary;
};
SLAM_INTERNAL int stage_eval_inputs(slam_ctx* c, const double* x, const int32_t* target_of, int64_t M, int n, bool want_grad, bool want_unitary,
                                    EvalBufs* d);
// ... and its results on their way back (grad, unitary: may be nullptr); no wait: the caller synchronises
SLAM_INTERNAL int enqueue_eval_readback(slam_ctx* c, int64_t M, int n, double* loss, double* grad, double* unitary);

// What the single-stage calls of the parametrised-gate families (slam_v2_*, slam_smush_*) do between "the arguments are valid" and
// "build the kernel's argument block", for stage k with rows of n parameters: the bounds checked, packed and uploaded to
// c->v2_bounds as (init_lo | init_hi | bound_lo | bound_hi)[n] (*bounded: some bound is finite), the active list and the start
// points checked and uploaded (*d_active / *d_x0 stay nullptr without them), the stage buffers reserved, the control blocks zeroed,
// n_active published and `solved` zeroed.
SLAM_INTERNAL int stage_family_inputs(slam_ctx* c, int k, int n, const int32_t* active, int64_t n_active, const double* x0, const double* init_lo,
                                      const double* init_hi, const double* bound_lo, const double* bound_hi, const slam_opt_params* prm,
                                      const int32_t** d_active, const double** d_x0, bool* bounded);
// after the optimizer kernel of stage k (rows of n parameters): the reduction over restarts (ordered winner rule), the results, the
// per-item records and the statistics brought back
SLAM_INTERNAL int finish_single_stage(slam_ctx* c, int k, int n, int64_t n_active, const slam_opt_params* prm, double exit_loss, double* best_loss,
                                      double* best_x, int32_t* best_restart, double* item_loss, int32_t* item_iters, int32_t* item_status,
                                      int32_t* item_evals);

// ---- slam_geometry.hip ------------------------------------------------------------------------------------------------
// c1c2c3_kernel on c's stream: Weyl coordinates of `count` unitaries in device memory into d_out[count][3]
SLAM_INTERNAL int enqueue_c1c2c3(slam_ctx* c, const double* d_unitaries, int64_t count, int ndigits, double* d_out);
// span_predict_kernel on c's stream: template sizes of the resident targets [first, first + count) into d_spans
SLAM_INTERNAL int enqueue_span_predict(slam_ctx* c, int64_t first, int64_t count, int k_max, const double* point, const double* bounds, double tol,
                                       int32_t* d_spans);

// ---- the three *_minimize_stage_trace entry points --------------------------------------------------------------------
// `span` checks k for the family and gives the template's parameter count; `stage` is the family's single-stage call, run with
// ctx->trace_cap set.
template <class Span, class Stage>
int minimize_stage_trace(slam_ctx* ctx, const int32_t* active, int64_t n_active, const slam_opt_params* params, int32_t trace_cap,
                         double* trace_loss, double* trace_x, Span span, Stage stage) {
    if (!ctx) return fail(SLAM_ERR_INVALID, "ctx is NULL");
    if (!params) return fail(SLAM_ERR_INVALID, "params is NULL");
    if (trace_cap <= 0 || !trace_loss || !trace_x) return fail(SLAM_ERR_INVALID, "trace buffers and trace_cap > 0 are required");
    int n = 0;
    int rc = span(&n);
    if (rc) return rc;
    if (!active) n_active = ctx->n_targets;
    if (n_active <= 0 || params->restarts <= 0) return fail(SLAM_ERR_INVALID, "nothing to trace");
    const int64_t M = n_active * (int64_t)params->restarts;
    const size_t rows = (size_t)M * (size_t)trace_cap;
    if (rows * (size_t)(n + 1) * sizeof(double) > ((size_t)4 << 30))
        return fail(SLAM_ERR_INVALID, "trace of %lld items x %d iterations exceeds 4 GiB: trace fewer targets at a time", (long long)M, trace_cap);
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(ctx->trace_loss.reserve(rows * sizeof(double)));
    HIP_TRY(ctx->trace_x.reserve(rows * n * sizeof(double)));
    // rows that no iteration reaches read as NaN
    HIP_TRY(hipMemsetAsync(ctx->trace_loss.p, 0xFF, rows * sizeof(double), ctx->stream));
    HIP_TRY(hipMemsetAsync(ctx->trace_x.p, 0xFF, rows * n * sizeof(double), ctx->stream));
    ctx->trace_cap = trace_cap;
    rc = stage();
    ctx->trace_cap = 0;
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(trace_loss, ctx->trace_loss.p, rows * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipMemcpyAsync(trace_x, ctx->trace_x.p, rows * n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return SLAM_OK;
}
