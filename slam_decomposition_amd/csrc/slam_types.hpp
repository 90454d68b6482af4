// slam_types.hpp -- plain-data types shared by the kernels and the host units of libslamhip: no kernel, no device function.
// The host's context (slam_host.hpp) and the argument blocks that cross a unit boundary are built from these, so a unit can
// enqueue another unit's kernel through a host function without including that kernel's header.
#pragma once
#include <stdint.h>

namespace slamdev {

// gate structure classes GC_* (slam_device.hpp)
constexpr int kGateClasses = 5;

// One finished (or dropped) work item: the five scalars of its result as ONE 32-byte record = one sector, written by one lane as two
// 16-byte stores (round 3 wrote them into five arrays: five partial-sector stores per item, WRITE_SIZE 2.2x the payload)
struct __attribute__((aligned(32))) ItemRec {
    double loss;
    int32_t iters;
    int32_t status;
    int32_t evals;   // all loss+gradient evaluations of the item
    int32_t acc;     // those whose point was accepted
    int32_t pad[2];
};
static_assert(sizeof(ItemRec) == 32, "ItemRec layout");

// Device-side control block of one span stage.  The span loop (optimizer.py:233-303) is enqueued as one
// chain of kernels without host round trips: the number of targets a stage works on is produced on the
// device by the previous stage's compaction, and every kernel of the stage reads it from here.
struct StageCtl {
    unsigned long long evals;    // += fused loss+gradient evaluations (reduce kernel)
    unsigned long long rounds;   // += lock-step evaluation rounds of every wavefront
    unsigned int work_counter;   // work queue of the optimizer kernel
    int32_t n_active;            // targets of this stage (written by init / the previous stage's compaction)
    unsigned long long evals_accepted;   // += evaluations whose point was accepted (initial point or Armijo step)
    unsigned long long evals_preempted;  // += evaluations of items that ended pre-empted by a sibling restart
    int32_t pad[6];
};
static_assert(sizeof(StageCtl) == 64, "StageCtl layout");

// ---------------------------------------------------------------------------------
// per-target reduction over restarts: argmin of item_loss (ties -> lowest restart), then the span loop's
// bookkeeping (TemplateOptimizer._run, optimizer.py:281-303): "if best_result is None or result.fun <
// best_result" the stage result replaces the target's best (loss, parameters, cycles).
// ---------------------------------------------------------------------------------
struct ReduceArgs {
    const ItemRec* item_rec;   // [n_active * R]
    const double* item_x;      // [n_active * R][n]
    double exit_loss;          // ordered == 1: the winner is the lowest-index restart below exit_loss (else the argmin)
    int32_t ordered;
    StageCtl* ctl;             // n_active; evals += sum of item_evals
    int32_t restarts;
    int32_t n;                 // parameters at this span
    double* stage_loss;        // [n_active]
    double* stage_x;           // [n_active][n]
    int32_t* stage_restart;    // [n_active]
    // merge into the resident results (best_loss == nullptr: single-stage call, no merge)
    const int32_t* active;     // [n_active] target index of each stage slot (nullptr = identity)
    int32_t nmax;
    int32_t k;
    double* best_loss;         // [n_targets]
    double* best_x;            // [n_targets][nmax]
    int32_t* best_cycles;      // [n_targets]
    double* span_loss;         // [n_targets][kSpanLossStride]: running best after span k at [k - 1] ("Cycle (k =...), Best Loss")
    // overlapped spans: the slot's evaluation counts (all, accepted, pre-empted) go here instead of into ctl -- the merge books them
    unsigned long long* slot_ev;  // [n_active][3] or nullptr
};

// stage_epilogue_kernel / stage_epilogue_grid_kernel (slam_kernels.hpp)
struct EpilogueArgs {
    ReduceArgs r;
    int32_t has_next;
    double threshold;
    int32_t* active_out;     // [n_upper] next stage's active list
    StageCtl* next;
    const double* targets;   // resident targets
    double* stage_targets;   // next stage's gathered targets
    int32_t* solved;
};

// slam_v2.hpp
struct V2GateMap {  // raw angle order: 0 a, 1 phi_c, 2 b, 3 phi_g
    double scale[4];
    double offset[4];
    int32_t sel[4];
    int32_t pad[4];
};
static_assert(sizeof(V2GateMap) == 96, "V2GateMap layout");

// slam_smush.hpp
constexpr int kSmushMaxSpan = 6;
constexpr int kSmushMaxLayers = kSmushMaxSpan + 1;
constexpr int kSmushMaxSlices = 58;                       // SLAM_SMUSH_MAX_SLICES
constexpr int kSmushRaw = 2 + 2 * kSmushMaxSlices;        // raw order: gc, gg, gx[0..N), gy[0..N)
constexpr int kSmushNP = 128;                             // n <= 128: lane l holds components 2 l, 2 l + 1

// device copy of slam_smush_gate (include/slam_hip.h): same layout
struct SmushMap {
    int32_t qn;
    int32_t n_slices;
    double t;
    int32_t sel[kSmushRaw];
    double scale[kSmushRaw];
    double offset[kSmushRaw];
};

}  // namespace slamdev
