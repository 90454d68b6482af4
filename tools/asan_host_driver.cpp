// AddressSanitizer driver for the HOST side of libslamhip (tools/asan_host.sh): runs every C-ABI entry point through
// the paths that need no GPU -- argument validation, error formatting, the thread-local message, context / communicator
// creation failing cleanly on a machine without a device -- under ASan + UBSan.  With a GPU present it still only uses
// these paths (it never launches a kernel).
#include "../include/slam_hip.h"

#include <cstdio>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <thread>
#include <vector>

static int fails = 0;
#define EXPECT(cond)                                                             \
    do {                                                                         \
        if (!(cond)) { std::printf("FAIL %s:%d  %s  [%s]\n", __FILE__, __LINE__, #cond, slam_last_error()); ++fails; } \
    } while (0)

int main() {
    EXPECT(std::strstr(slam_version(), "gfx950") != nullptr);
    {  // the load-time initialiser ran before main: off (SLAM_HW_QUEUES=0), or the variable holds what it reports, at least 4
        const int q = slam_hw_queues_requested();
        const char* e = std::getenv("GPU_MAX_HW_QUEUES");
        EXPECT(q == 0 || (q >= 4 && e && std::atoi(e) == q));
    }
    EXPECT(slam_device_count(nullptr) == SLAM_ERR_INVALID);
    int n = -1;
    const int rc_count = slam_device_count(&n);
    EXPECT(rc_count == SLAM_OK || (rc_count == SLAM_ERR_HIP && n == 0));
    EXPECT(slam_ctx_create(0, nullptr) == SLAM_ERR_INVALID);
    slam_ctx* ctx = nullptr;
    EXPECT(slam_ctx_create(-1, &ctx) != SLAM_OK && ctx == nullptr);
    EXPECT(slam_ctx_create(1 << 20, &ctx) != SLAM_OK && ctx == nullptr);
    EXPECT(std::strlen(slam_last_error()) > 0);
    // every entry point rejects a NULL context with a message, never a crash
    double d[64] = {0};
    int32_t i32[8] = {0};
    int64_t i64 = 0;
    slam_opt_params prm{};
    prm.restarts = 1;
    slam_stats st{};
    void* p = nullptr;
    EXPECT(slam_ctx_destroy(nullptr) == SLAM_OK);
    EXPECT(slam_ctx_device_info(nullptr, nullptr, 0, nullptr, nullptr) == SLAM_ERR_INVALID);
    EXPECT(slam_set_targets(nullptr, d, 1) == SLAM_ERR_INVALID);
    EXPECT(slam_sample_haar(nullptr, 1, 0, 1) == SLAM_ERR_INVALID);
    EXPECT(slam_get_targets(nullptr, 0, 1, d) == SLAM_ERR_INVALID);
    EXPECT(slam_sample_haar_indexed(nullptr, 1, &i64, 1) == SLAM_ERR_INVALID);
    EXPECT(slam_haar_select_spans(nullptr, 1, 0, 1, 3, d, d, 0.0, 0.0, 2, 3, 1, &i64, &i64, nullptr) == SLAM_ERR_INVALID);
    EXPECT(slam_c1c2c3(nullptr, d, 1, 8, d) == SLAM_ERR_INVALID);
    EXPECT(slam_targets_c1c2c3(nullptr, 0, 1, 8, d) == SLAM_ERR_INVALID);
    EXPECT(slam_kak(nullptr, d, 1, d, d, d, d, d, d) == SLAM_ERR_INVALID);
    EXPECT(slam_targets_kak(nullptr, 0, 1, d, d, d, d, d, d) == SLAM_ERR_INVALID);
    EXPECT(slam_complete_locals(nullptr, 1, i32, d, i32, 1, d, d, d) == SLAM_ERR_INVALID);
    EXPECT(slam_sqiswap_decompose(nullptr, 0, 1, d, i32, d, d) == SLAM_ERR_INVALID);
    EXPECT(std::strstr(slam_last_error(), "ctx is NULL") != nullptr);
    {  // slam_cx_decompose checks its gate and folds the host's factors before it needs a context: CXGate and its reduction as
       // Context.cx_decompose computes it (_ffi.cx_dress), so the whole of the host's share runs here
    const double cx_gate[32] = {
        1.0, 0.0, 0.0, 0.0, 0.0, 0.0,
        0.0, 0.0, 0.0, 0.0, 0.0, 0.0,
        0.0, 0.0, 1.0, 0.0, 0.0, 0.0,
        0.0, 0.0, 1.0, 0.0, 0.0, 0.0,
        0.0, 0.0, 1.0, 0.0, 0.0, 0.0,
        0.0, 0.0};
    const double cx_dress[99] = {
        5.5511151231257815e-17, -0.7071067811865476, 0.7071067811865476, -5.5511151231257815e-17, -0.7071067811865476, -5.5511151231257815e-17,
        5.5511151231257815e-17, 0.7071067811865476, 0.5, -0.5, -0.5, 0.5,
        0.5, 0.5, 0.5, 0.5, 6.312253112239643e-33, -1.0,
        0.0, 0.0, 0.0, 0.0, 6.312253112239643e-33, 1.0,
        -0.7071067811865476, -1.848816132009102e-33, -0.7071067811865476, -1.848816132009102e-33, 0.7071067811865476, -1.848816132009102e-33,
        -0.7071067811865476, 1.848816132009102e-33, -0.6532814824381884, 0.27059805007309845, -0.6532814824381883, 0.2705980500730985,
        0.6532814824381883, 0.2705980500730985, -0.6532814824381884, -0.27059805007309845, -0.9238795325112868, 0.0,
        0.0, -0.3826834323650897, 0.0, -0.3826834323650897, -0.9238795325112868, 0.0,
        0.6532814824381883, -0.27059805007309856, -0.6532814824381883, -0.27059805007309856, 0.6532814824381883, -0.27059805007309856,
        0.6532814824381883, 0.27059805007309856, 0.38268343236508995, 0.0, 0.0, -0.9238795325112868,
        0.0, -0.9238795325112868, 0.38268343236508995, 0.0, 0.7071067811865476, -5.5511151231257815e-17,
        -5.5511151231257815e-17, 0.7071067811865476, 5.5511151231257815e-17, 0.7071067811865476, 0.7071067811865476, 5.5511151231257815e-17,
        0.5, 0.5, 0.5, 0.5, -0.5, 0.5,
        0.5, -0.5, 0.0, 0.0, -6.312253112239643e-33, -1.0,
        6.312253112239643e-33, -1.0, 0.0, 0.0, 1.848816132009102e-33, -0.7071067811865476,
        1.848816132009102e-33, -0.7071067811865476, -1.848816132009102e-33, -0.7071067811865476, 1.848816132009102e-33, 0.7071067811865476,
        0.5000000000000001, 5.551115123125783e-17, 5.551115123125783e-17};
        EXPECT(slam_cx_decompose(nullptr, 0, 1, 0, cx_gate, cx_dress, d, i32, d, d) == SLAM_ERR_INVALID);
        EXPECT(std::strstr(slam_last_error(), "ctx is NULL") != nullptr);
        EXPECT(slam_cx_decompose(nullptr, 0, 1, 2, cx_gate, cx_dress, d, i32, d, d) == SLAM_ERR_INVALID);
        EXPECT(std::strstr(slam_last_error(), "family") != nullptr);
        EXPECT(slam_cx_decompose(nullptr, 0, 1, 1, cx_gate, cx_dress, d, i32, d, d) == SLAM_ERR_INVALID);  // the other family's class
        EXPECT(std::strstr(slam_last_error(), "coordinates") != nullptr);
        EXPECT(slam_cx_decompose(nullptr, 0, 1, 0, nullptr, cx_dress, d, i32, d, d) == SLAM_ERR_INVALID);
        double bad[SLAM_CX_DRESS];
        std::memcpy(bad, cx_dress, sizeof(bad));
        bad[3] += 1e-9;  // one factor off: the gate is not rebuilt
        EXPECT(slam_cx_decompose(nullptr, 0, 1, 0, cx_gate, bad, d, i32, d, d) == SLAM_ERR_INVALID);
        EXPECT(std::strstr(slam_last_error(), "rebuild the gate") != nullptr);
        std::memcpy(bad, cx_dress, sizeof(bad));
        bad[8 * 9 + 2] += 1e-9;  // a factor of CX21 off
        EXPECT(slam_cx_decompose(nullptr, 0, 1, 0, cx_gate, bad, d, i32, d, d) == SLAM_ERR_INVALID);
        EXPECT(std::strstr(slam_last_error(), "CX21") != nullptr);
        for (double& v : bad) v = 0.0;
        bad[96] = 0.5;
        EXPECT(slam_cx_decompose(nullptr, 0, 1, 0, cx_gate, bad, d, i32, d, d) == SLAM_ERR_INVALID);  // all-zero factors
        // slam_approx_decompose: the same check and fold, then its own arguments, then the context
        EXPECT(slam_approx_decompose(nullptr, 0, 1, 0, cx_gate, cx_dress, 0.99, -1, d, i32, d, d, d) == SLAM_ERR_INVALID);
        EXPECT(std::strstr(slam_last_error(), "ctx is NULL") != nullptr);
        EXPECT(slam_approx_decompose(nullptr, 0, 1, 0, cx_gate, cx_dress, 1.0, 3, d, i32, d, d, d) == SLAM_ERR_INVALID);
        EXPECT(std::strstr(slam_last_error(), "ctx is NULL") != nullptr);
        EXPECT(slam_approx_decompose(nullptr, 0, 1, 3, cx_gate, cx_dress, 0.99, -1, d, i32, d, d, d) == SLAM_ERR_INVALID);
        EXPECT(std::strstr(slam_last_error(), "family") != nullptr);
        EXPECT(slam_approx_decompose(nullptr, 0, 1, 0, cx_gate, bad, 0.99, -1, d, i32, d, d, d) == SLAM_ERR_INVALID);
        EXPECT(slam_approx_decompose(nullptr, 0, 1, 0, cx_gate, cx_dress, 0.0, -1, d, i32, d, d, d) == SLAM_ERR_INVALID);
        EXPECT(std::strstr(slam_last_error(), "basis_fidelity") != nullptr);
        EXPECT(slam_approx_decompose(nullptr, 0, 1, 0, cx_gate, cx_dress, 0.99, 4, d, i32, d, d, d) == SLAM_ERR_INVALID);
        EXPECT(std::strstr(slam_last_error(), "force_cycles") != nullptr);
    }
    {  // slam_b_decompose likewise: BerkeleyGate and its reduction as Context.b_decompose computes it (_ffi.b_dress)
        const double s = 0.38268343236508984, c = 0.9238795325112867;
        const double b_gate[32] = {
            c, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, s,
            0.0, 0.0, s, 0.0, 0.0, c, 0.0, 0.0,
            0.0, 0.0, 0.0, c, s, 0.0, 0.0, 0.0,
            0.0, s, 0.0, 0.0, 0.0, 0.0, c, 0.0};
        const double b_dress[SLAM_B_DRESS] = {
            1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0,
            1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0,
            1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0,
            1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0,
            0.5, 0.25, 0.0};
        EXPECT(slam_b_decompose(nullptr, 0, 1, b_gate, b_dress, d, i32, d, d) == SLAM_ERR_INVALID);
        EXPECT(std::strstr(slam_last_error(), "ctx is NULL") != nullptr);
        EXPECT(slam_b_decompose(nullptr, 0, 1, nullptr, b_dress, d, i32, d, d) == SLAM_ERR_INVALID);
        EXPECT(slam_b_decompose(nullptr, 0, 1, b_gate, nullptr, d, i32, d, d) == SLAM_ERR_INVALID);
        double bad[SLAM_B_DRESS];
        std::memcpy(bad, b_dress, sizeof(bad));
        bad[33] = 0.0;  // the CNOT class
        EXPECT(slam_b_decompose(nullptr, 0, 1, b_gate, bad, d, i32, d, d) == SLAM_ERR_INVALID);
        EXPECT(std::strstr(slam_last_error(), "coordinates") != nullptr);
        std::memcpy(bad, b_dress, sizeof(bad));
        bad[3] += 1e-9;  // one factor off: the gate is not rebuilt
        EXPECT(slam_b_decompose(nullptr, 0, 1, b_gate, bad, d, i32, d, d) == SLAM_ERR_INVALID);
        EXPECT(std::strstr(slam_last_error(), "rebuild the gate") != nullptr);
        for (double& v : bad) v = 0.0;
        bad[32] = 0.5;
        bad[33] = 0.25;
        EXPECT(slam_b_decompose(nullptr, 0, 1, b_gate, bad, d, i32, d, d) == SLAM_ERR_INVALID);  // all-zero factors
        EXPECT(slam_approx_decompose(nullptr, 0, 1, 2, b_gate, b_dress, 0.99, 2, d, i32, d, d, d) == SLAM_ERR_INVALID);
        EXPECT(std::strstr(slam_last_error(), "ctx is NULL") != nullptr);
        EXPECT(slam_approx_decompose(nullptr, 0, 1, 2, b_gate, b_dress, 0.99, 3, d, i32, d, d, d) == SLAM_ERR_INVALID);
        EXPECT(std::strstr(slam_last_error(), "force_cycles") != nullptr);
        EXPECT(slam_approx_decompose(nullptr, 0, 1, 2, b_gate, bad, 0.99, -1, d, i32, d, d, d) == SLAM_ERR_INVALID);
        const double fid[2] = {0.9, 1.0}, bad_fid[2] = {0.9, 1.5};
        EXPECT(slam_approx_counts(nullptr, 0, 1, 2, 2, fid, &i64, &i64) == SLAM_ERR_INVALID);
        EXPECT(std::strstr(slam_last_error(), "ctx is NULL") != nullptr);
        EXPECT(slam_approx_counts(nullptr, 0, 1, 2, 2, bad_fid, &i64, &i64) == SLAM_ERR_INVALID);
        EXPECT(std::strstr(slam_last_error(), "fidelities[1]") != nullptr);
        EXPECT(slam_approx_counts(nullptr, 0, 1, 2, 65, fid, &i64, &i64) == SLAM_ERR_INVALID);
        EXPECT(slam_approx_counts(nullptr, 0, 1, 3, 2, fid, &i64, &i64) == SLAM_ERR_INVALID);
    }
    {  // slam_sc_decompose, slam_sc_counts: CAN(1/2, 0.3, 0) and its reduction as Context.sc_decompose computes it (_ffi.sc_dress)
        const double c1 = 0.9510565162951535, s1 = 0.3090169943749474, c4 = 0.30901699437494745, s4 = 0.9510565162951535;
        const double sc_gate[32] = {
            c1, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, s1,
            0.0, 0.0, c4, 0.0, 0.0, s4, 0.0, 0.0,
            0.0, 0.0, 0.0, s4, c4, 0.0, 0.0, 0.0,
            0.0, s1, 0.0, 0.0, 0.0, 0.0, c1, 0.0};
        const double sc_dress[SLAM_SC_DRESS] = {
            1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0,
            1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0,
            1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0,
            1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0,
            0.5, 0.3, 0.0};
        const double fid[2] = {0.9, 1.0}, bad_fid[2] = {0.9, 1.5};
        EXPECT(slam_sc_decompose(nullptr, 0, 1, sc_gate, sc_dress, 0.99, -1, d, i32, d, d, d) == SLAM_ERR_INVALID);
        EXPECT(std::strstr(slam_last_error(), "ctx is NULL") != nullptr);
        EXPECT(slam_sc_counts(nullptr, 0, 1, sc_gate, sc_dress, 2, fid, &i64, &i64) == SLAM_ERR_INVALID);
        EXPECT(std::strstr(slam_last_error(), "ctx is NULL") != nullptr);
        EXPECT(slam_sc_decompose(nullptr, 0, 1, nullptr, sc_dress, 0.99, -1, d, i32, d, d, d) == SLAM_ERR_INVALID);
        EXPECT(slam_sc_counts(nullptr, 0, 1, sc_gate, nullptr, 2, fid, &i64, &i64) == SLAM_ERR_INVALID);
        double bad[SLAM_SC_DRESS];
        std::memcpy(bad, sc_dress, sizeof(bad));
        bad[32] = 0.25;  // off the line
        EXPECT(slam_sc_decompose(nullptr, 0, 1, sc_gate, bad, 0.99, -1, d, i32, d, d, d) == SLAM_ERR_INVALID);
        EXPECT(std::strstr(slam_last_error(), "coordinates") != nullptr);
        std::memcpy(bad, sc_dress, sizeof(bad));
        bad[33] = 0.6;  // beyond the iSWAP end of the line
        EXPECT(slam_sc_counts(nullptr, 0, 1, sc_gate, bad, 2, fid, &i64, &i64) == SLAM_ERR_INVALID);
        EXPECT(std::strstr(slam_last_error(), "coordinates") != nullptr);
        bad[33] = 0.2;  // another gate of the line
        EXPECT(slam_sc_decompose(nullptr, 0, 1, sc_gate, bad, 0.99, -1, d, i32, d, d, d) == SLAM_ERR_INVALID);
        EXPECT(std::strstr(slam_last_error(), "rebuild the gate") != nullptr);
        std::memcpy(bad, sc_dress, sizeof(bad));
        bad[3] += 1e-9;  // one factor off: the gate is not rebuilt
        EXPECT(slam_sc_decompose(nullptr, 0, 1, sc_gate, bad, 0.99, -1, d, i32, d, d, d) == SLAM_ERR_INVALID);
        EXPECT(std::strstr(slam_last_error(), "rebuild the gate") != nullptr);
        EXPECT(slam_sc_decompose(nullptr, 0, 1, sc_gate, sc_dress, 0.0, -1, d, i32, d, d, d) == SLAM_ERR_INVALID);
        EXPECT(std::strstr(slam_last_error(), "basis_fidelity") != nullptr);
        EXPECT(slam_sc_decompose(nullptr, 0, 1, sc_gate, sc_dress, 0.99, 4, d, i32, d, d, d) == SLAM_ERR_INVALID);
        EXPECT(std::strstr(slam_last_error(), "force_cycles") != nullptr);
        EXPECT(slam_sc_counts(nullptr, 0, 1, sc_gate, sc_dress, 2, bad_fid, &i64, &i64) == SLAM_ERR_INVALID);
        EXPECT(std::strstr(slam_last_error(), "fidelities[1]") != nullptr);
        EXPECT(slam_sc_counts(nullptr, 0, 1, sc_gate, sc_dress, 65, fid, &i64, &i64) == SLAM_ERR_INVALID);
    }
    {  // slam_sqiswap_approx_decompose, slam_sqiswap_approx_counts: no gate to reduce, the fidelity and the size come first
        const double fid[2] = {0.9, 1.0}, bad_fid[2] = {0.9, 1.5};
        EXPECT(slam_sqiswap_approx_decompose(nullptr, 0, 1, 0.99, -1, d, i32, d, d, d) == SLAM_ERR_INVALID);
        EXPECT(std::strstr(slam_last_error(), "ctx is NULL") != nullptr);
        EXPECT(slam_sqiswap_approx_decompose(nullptr, 0, 1, 0.99, 3, nullptr, nullptr, nullptr, nullptr, nullptr) == SLAM_ERR_INVALID);
        EXPECT(std::strstr(slam_last_error(), "ctx is NULL") != nullptr);
        EXPECT(slam_sqiswap_approx_decompose(nullptr, 0, 1, 0.0, -1, d, i32, d, d, d) == SLAM_ERR_INVALID);
        EXPECT(std::strstr(slam_last_error(), "basis_fidelity") != nullptr);
        EXPECT(slam_sqiswap_approx_decompose(nullptr, 0, 1, 0.99, 4, d, i32, d, d, d) == SLAM_ERR_INVALID);
        EXPECT(std::strstr(slam_last_error(), "force_cycles") != nullptr);
        EXPECT(slam_sqiswap_approx_counts(nullptr, 0, 1, 2, fid, &i64, &i64) == SLAM_ERR_INVALID);
        EXPECT(std::strstr(slam_last_error(), "ctx is NULL") != nullptr);
        EXPECT(slam_sqiswap_approx_counts(nullptr, 0, 1, 2, bad_fid, &i64, &i64) == SLAM_ERR_INVALID);
        EXPECT(std::strstr(slam_last_error(), "fidelities[1]") != nullptr);
        EXPECT(slam_sqiswap_approx_counts(nullptr, 0, 1, 65, fid, &i64, &i64) == SLAM_ERR_INVALID);
        EXPECT(slam_sqiswap_approx_counts(nullptr, 0, 1, 2, nullptr, &i64, &i64) == SLAM_ERR_INVALID);
    }
    EXPECT(slam_predict_spans(nullptr, 0, 1, 3, d, d, 0.0, i32) == SLAM_ERR_INVALID);
    EXPECT(slam_coverage_lookup(nullptr, 0, 1, 1, i32, i32, d, d, 0.0, &i64, i32) == SLAM_ERR_INVALID);
    EXPECT(slam_family_lookup(nullptr, 0, 1, 1, i32, i32, d, d, i32, i32, d, 0.1, 1e-7, 0, &i64, &i64, i32, i32) == SLAM_ERR_INVALID);
    EXPECT(slam_candidate_scores(nullptr, 0, 1, 1, d, 8, 1e-7, nullptr, 1, &i64, i32, nullptr) == SLAM_ERR_INVALID);
    EXPECT(std::strstr(slam_last_error(), "ctx is NULL") != nullptr);
    EXPECT(slam_pd_sample(nullptr, 1.0, 0.0, 1.0, 4, 1, 1.0, 0, 0, 1, nullptr, 8, d, nullptr, nullptr) == SLAM_ERR_INVALID);
    EXPECT(slam_pd_extremes(nullptr, d, 1, &i64, d) == SLAM_ERR_INVALID);
    EXPECT(slam_pd_filter(nullptr, d, 1, 0.0, 0, &i64, nullptr, nullptr) == SLAM_ERR_INVALID);
    EXPECT(slam_region_lookup(nullptr, 0, 1, 1, i32, i32, i32, d, d, 1e-7, &i64) == SLAM_ERR_INVALID);
    EXPECT(slam_eval_c1c2c3(nullptr, 1, i32, d, 1, 8, d) == SLAM_ERR_INVALID);
    EXPECT(slam_set_gates(nullptr, d, 1) == SLAM_ERR_INVALID);
    EXPECT(slam_eval_loss_grad(nullptr, 1, i32, d, i32, 1, d, d) == SLAM_ERR_INVALID);
    EXPECT(slam_eval_unitary(nullptr, 1, i32, d, i32, 1, d, d) == SLAM_ERR_INVALID);
    EXPECT(slam_minimize_stage(nullptr, 1, i32, nullptr, 0, nullptr, &prm, d, d, i32, d, i32, i32, i32) == SLAM_ERR_INVALID);
    EXPECT(slam_minimize_stage_trace(nullptr, 1, i32, nullptr, 0, nullptr, &prm, 1e-10, 4, d, d, i32, d, i32, i32, d, d) == SLAM_ERR_INVALID);
    EXPECT(slam_decompose(nullptr, 1, 3, i32, &prm, 1e-10, d, d, i32) == SLAM_ERR_INVALID);
    EXPECT(slam_decompose_resident(nullptr, 1, 3, i32, &prm, 1e-10) == SLAM_ERR_INVALID);
    EXPECT(slam_decompose_range(nullptr, 0, 1, 1, 3, i32, &prm, 1e-10) == SLAM_ERR_INVALID);
    EXPECT(slam_decompose_range_fetch(nullptr, 0, 1, 1, 3, i32, &prm, 1e-10, d, d, i32) == SLAM_ERR_INVALID);
    EXPECT(slam_decompose_list(nullptr, i32, 1, 1, 3, 3, i32, &prm, 1e-10) == SLAM_ERR_INVALID);
    EXPECT(slam_decompose_multi(nullptr, 0, 0, 1, 1, 3, i32, &prm, 1e-10) == SLAM_ERR_INVALID);
    { slam_ctx* none[2] = {nullptr, nullptr}; EXPECT(slam_decompose_multi(none, 2, 0, 1, 1, 3, i32, &prm, 1e-10) == SLAM_ERR_INVALID); }
    EXPECT(slam_abi_version() == SLAM_ABI_VERSION);
    EXPECT(slam_fetch_results(nullptr, 3, d, d, i32) == SLAM_ERR_INVALID);
    EXPECT(slam_fetch_results_range(nullptr, 3, 0, 1, d, d, i32) == SLAM_ERR_INVALID);
    EXPECT(slam_fetch_span_losses(nullptr, 0, 1, d) == SLAM_ERR_INVALID);
    slam_v2_gate vg{};
    vg.n_params = 1;
    EXPECT(slam_v2_set_gates(nullptr, &vg, 1) == SLAM_ERR_INVALID);
    EXPECT(slam_v2_set_constraint(nullptr, 1, d, 13, 1.0) == SLAM_ERR_INVALID);
    EXPECT(slam_v2_eval_loss_grad(nullptr, 1, i32, d, i32, 1, d, d, d) == SLAM_ERR_INVALID);
    EXPECT(slam_v2_minimize_stage(nullptr, 1, i32, nullptr, 1, nullptr, d, d, nullptr, nullptr, &prm, 1e-10, d, d, i32, d, i32, i32, i32) == SLAM_ERR_INVALID);
    EXPECT(slam_v2_decompose_range(nullptr, 0, 1, 1, 1, i32, d, d, nullptr, nullptr, &prm, 1e-10, d, d, i32) == SLAM_ERR_INVALID);
    EXPECT(slam_v2_minimize_stage_trace(nullptr, 1, i32, nullptr, 1, nullptr, d, d, nullptr, nullptr, &prm, 1e-10, 4, d, d, i32, d, i32, i32, d, d) == SLAM_ERR_INVALID);
    {
        static slam_smush_gate sg{};
        sg.n_params = 8;
        sg.n_slices = 4;
        sg.t = 1.0;
        EXPECT(slam_smush_set_gates(nullptr, &sg, 1) == SLAM_ERR_INVALID);
        EXPECT(slam_smush_eval_loss_grad(nullptr, 1, i32, d, i32, 1, d, d, d) == SLAM_ERR_INVALID);
        EXPECT(slam_smush_minimize_stage(nullptr, 1, i32, nullptr, 1, nullptr, d, d, nullptr, nullptr, &prm, 1e-10, d, d, i32, d, i32, i32, i32) ==
               SLAM_ERR_INVALID);
        EXPECT(slam_smush_minimize_stage_trace(nullptr, 1, i32, nullptr, 1, nullptr, d, d, nullptr, nullptr, &prm, 1e-10, 4, d, d, i32, d, i32, i32, d,
                                               d) == SLAM_ERR_INVALID);
    }
    {  // slam_q3_eval, slam_q3_minimize: the template, the cost kind and the pointers are checked before the context
        const int32_t gi[2] = {0, 0}, ed[4] = {0, 1, 1, 2}, bad_gi[2] = {0, 1}, bad_ed[4] = {0, 1, 2, 2}, far_ed[4] = {0, 3, 1, 2};
        static double t8[128] = {0}, x3[21] = {0}, g3[21], u3[128];
        EXPECT(slam_q3_eval(nullptr, d, 1, 2, gi, ed, t8, 1, x3, i32, 1, SLAM_COST_BASIC, d, g3, u3) == SLAM_ERR_INVALID);
        EXPECT(std::strstr(slam_last_error(), "ctx is NULL") != nullptr);
        EXPECT(slam_q3_eval(nullptr, d, 1, 0, gi, ed, t8, 1, x3, i32, 1, SLAM_COST_BASIC, d, g3, u3) == SLAM_ERR_UNSUPPORTED);
        EXPECT(slam_q3_eval(nullptr, d, 1, SLAM_Q3_MAX_SPAN + 1, gi, ed, t8, 1, x3, i32, 1, SLAM_COST_BASIC, d, g3, u3) == SLAM_ERR_UNSUPPORTED);
        EXPECT(std::strstr(slam_last_error(), "1..15") != nullptr);
        EXPECT(slam_q3_eval(nullptr, nullptr, 1, 2, gi, ed, t8, 1, x3, i32, 1, SLAM_COST_BASIC, d, g3, u3) == SLAM_ERR_INVALID);
        EXPECT(slam_q3_eval(nullptr, d, 1, 2, nullptr, ed, t8, 1, x3, i32, 1, SLAM_COST_BASIC, d, g3, u3) == SLAM_ERR_INVALID);
        EXPECT(slam_q3_eval(nullptr, d, 1, 2, gi, nullptr, t8, 1, x3, i32, 1, SLAM_COST_BASIC, d, g3, u3) == SLAM_ERR_INVALID);
        EXPECT(slam_q3_eval(nullptr, d, 1, 2, bad_gi, ed, t8, 1, x3, i32, 1, SLAM_COST_BASIC, d, g3, u3) == SLAM_ERR_INVALID);
        EXPECT(std::strstr(slam_last_error(), "gate_index[1]") != nullptr);
        EXPECT(slam_q3_eval(nullptr, d, 1, 2, gi, bad_ed, t8, 1, x3, i32, 1, SLAM_COST_BASIC, d, g3, u3) == SLAM_ERR_INVALID);
        EXPECT(std::strstr(slam_last_error(), "edges[1]") != nullptr);
        EXPECT(slam_q3_eval(nullptr, d, 1, 2, gi, far_ed, t8, 1, x3, i32, 1, SLAM_COST_BASIC, d, g3, u3) == SLAM_ERR_INVALID);
        EXPECT(std::strstr(slam_last_error(), "edges[0]") != nullptr);
        EXPECT(slam_q3_eval(nullptr, d, 1, 2, gi, ed, t8, 1, x3, i32, 1, SLAM_COST_MAKHLIN, d, g3, u3) == SLAM_ERR_UNSUPPORTED);
        EXPECT(std::strstr(slam_last_error(), "Weyl chamber only for 2Q gates") != nullptr);
        EXPECT(slam_q3_eval(nullptr, d, 1, 2, gi, ed, t8, 1, x3, i32, 1, 7, d, g3, u3) == SLAM_ERR_INVALID);
        EXPECT(slam_q3_eval(nullptr, d, 1, 2, gi, ed, nullptr, 1, x3, i32, 1, SLAM_COST_BASIC, d, g3, u3) == SLAM_ERR_INVALID);
        EXPECT(slam_q3_eval(nullptr, d, 1, 2, gi, ed, t8, 1, nullptr, i32, 1, SLAM_COST_BASIC, d, g3, u3) == SLAM_ERR_INVALID);
        EXPECT(slam_q3_eval(nullptr, d, 1, 2, gi, ed, t8, 1, x3, i32, 0, SLAM_COST_BASIC, d, g3, u3) == SLAM_ERR_INVALID);
        { const int32_t tof[1] = {1}; EXPECT(slam_q3_eval(nullptr, d, 1, 2, gi, ed, t8, 1, x3, tof, 1, SLAM_COST_BASIC, d, g3, u3) == SLAM_ERR_INVALID); }
        EXPECT(std::strstr(slam_last_error(), "target_of[0]") != nullptr);
        EXPECT(slam_q3_minimize(nullptr, d, 1, 2, gi, ed, t8, 1, SLAM_COST_SQUARE, &prm, 1e-10, nullptr, d, g3, i32, d, i32, i32, i32, nullptr, nullptr) ==
               SLAM_ERR_INVALID);
        EXPECT(std::strstr(slam_last_error(), "ctx is NULL") != nullptr);
        EXPECT(slam_q3_minimize(nullptr, d, 1, 16, gi, ed, t8, 1, SLAM_COST_BASIC, &prm, 1e-10, nullptr, d, g3, i32, d, i32, i32, i32, nullptr, nullptr) ==
               SLAM_ERR_UNSUPPORTED);
        EXPECT(slam_q3_minimize(nullptr, d, 1, 2, gi, bad_ed, t8, 1, SLAM_COST_BASIC, &prm, 1e-10, nullptr, d, g3, i32, d, i32, i32, i32, nullptr, nullptr) ==
               SLAM_ERR_INVALID);
        EXPECT(slam_q3_minimize(nullptr, d, 1, 2, gi, ed, t8, 1, SLAM_COST_MAKHLIN, &prm, 1e-10, nullptr, d, g3, i32, d, i32, i32, i32, nullptr, nullptr) ==
               SLAM_ERR_UNSUPPORTED);
        EXPECT(slam_q3_minimize(nullptr, d, 1, 2, gi, ed, t8, 1, SLAM_COST_BASIC, nullptr, 1e-10, nullptr, d, g3, i32, d, i32, i32, i32, nullptr, nullptr) ==
               SLAM_ERR_INVALID);
        EXPECT(std::strstr(slam_last_error(), "params is NULL") != nullptr);
        EXPECT(slam_q3_minimize(nullptr, d, 1, 2, gi, ed, nullptr, 1, SLAM_COST_BASIC, &prm, 1e-10, nullptr, d, g3, i32, d, i32, i32, i32, nullptr, nullptr) ==
               SLAM_ERR_INVALID);
        EXPECT(slam_q3_minimize(nullptr, d, 1, 2, gi, ed, t8, 0, SLAM_COST_BASIC, &prm, 1e-10, nullptr, d, g3, i32, d, i32, i32, i32, nullptr, nullptr) ==
               SLAM_ERR_INVALID);
        {  // explicit start points [1][restarts = 1][21]: every entry is read, the first and the last are refused unless finite with |x| < 1e8
            const double bad[3] = {std::numeric_limits<double>::quiet_NaN(), std::numeric_limits<double>::infinity(), 1e12};
            for (int at : {0, 20})
                for (double v : bad) {
                    double xb[21] = {0};
                    xb[at] = v;
                    EXPECT(slam_q3_minimize(nullptr, d, 1, 2, gi, ed, t8, 1, SLAM_COST_BASIC, &prm, 1e-10, xb, d, g3, i32, d, i32, i32, i32, nullptr,
                                            nullptr) == SLAM_ERR_INVALID);
                    EXPECT(std::strstr(slam_last_error(), "explicit seeds must be finite with |x| < 1e8") != nullptr);
                    EXPECT(std::strstr(slam_last_error(), at ? "x0[20]" : "x0[0]") != nullptr);
                }
            double ok[21] = {0};
            ok[0] = 9.9e7;
            ok[20] = -9.9e7;
            EXPECT(slam_q3_minimize(nullptr, d, 1, 2, gi, ed, t8, 1, SLAM_COST_BASIC, &prm, 1e-10, ok, d, g3, i32, d, i32, i32, i32, nullptr, nullptr) ==
                   SLAM_ERR_INVALID);
            EXPECT(std::strstr(slam_last_error(), "ctx is NULL") != nullptr);
        }
    }
    {  // slam_q3m_eval, slam_q3m_minimize: arities, qubits, table indices and the caps are checked before the context
        const int32_t ar[2] = {3, 2}, gi[2] = {1, 0}, qb[6] = {0, 1, 2, 1, 2, 7}, bad_ar[2] = {3, 4}, bad_gi[2] = {2, 0}, bad_qb[6] = {0, 1, 1, 1, 2, 0};
        static double g3m[SLAM_Q3_MAX_GATES3 + 1][128] = {{0}}, t8[128] = {0}, x3[24] = {0}, gr[24], u3[128];
        const double* g3 = &g3m[0][0];
        EXPECT(slam_q3m_eval(nullptr, d, 1, g3, 2, 2, ar, gi, qb, t8, 1, x3, i32, 1, SLAM_COST_BASIC, d, gr, u3) == SLAM_ERR_INVALID);
        EXPECT(std::strstr(slam_last_error(), "ctx is NULL") != nullptr);
        EXPECT(slam_q3m_eval(nullptr, d, 1, g3, 2, 0, ar, gi, qb, t8, 1, x3, i32, 1, SLAM_COST_BASIC, d, gr, u3) == SLAM_ERR_UNSUPPORTED);
        EXPECT(slam_q3m_eval(nullptr, d, 1, g3, 2, SLAM_Q3_MAX_SPAN + 1, ar, gi, qb, t8, 1, x3, i32, 1, SLAM_COST_BASIC, d, gr, u3) == SLAM_ERR_UNSUPPORTED);
        EXPECT(slam_q3m_eval(nullptr, d, 1, g3, SLAM_Q3_MAX_GATES3 + 1, 2, ar, gi, qb, t8, 1, x3, i32, 1, SLAM_COST_BASIC, d, gr, u3) == SLAM_ERR_UNSUPPORTED);
        EXPECT(std::strstr(slam_last_error(), "distinct three-qubit gates") != nullptr);
        EXPECT(slam_q3m_eval(nullptr, d, 1, g3, 2, 2, bad_ar, gi, qb, t8, 1, x3, i32, 1, SLAM_COST_BASIC, d, gr, u3) == SLAM_ERR_INVALID);
        EXPECT(std::strstr(slam_last_error(), "arity[1]") != nullptr);
        EXPECT(slam_q3m_eval(nullptr, d, 1, g3, 2, 2, ar, bad_gi, qb, t8, 1, x3, i32, 1, SLAM_COST_BASIC, d, gr, u3) == SLAM_ERR_INVALID);
        EXPECT(std::strstr(slam_last_error(), "gate_index[0]") != nullptr);
        EXPECT(slam_q3m_eval(nullptr, d, 1, g3, 2, 2, ar, gi, bad_qb, t8, 1, x3, i32, 1, SLAM_COST_BASIC, d, gr, u3) == SLAM_ERR_INVALID);
        EXPECT(std::strstr(slam_last_error(), "qubits[0]") != nullptr);
        EXPECT(slam_q3m_eval(nullptr, d, 1, nullptr, 2, 2, ar, gi, qb, t8, 1, x3, i32, 1, SLAM_COST_BASIC, d, gr, u3) == SLAM_ERR_INVALID);
        EXPECT(slam_q3m_eval(nullptr, d, 1, g3, 2, 2, nullptr, gi, qb, t8, 1, x3, i32, 1, SLAM_COST_BASIC, d, gr, u3) == SLAM_ERR_INVALID);
        EXPECT(slam_q3m_eval(nullptr, d, 1, g3, 2, 2, ar, gi, nullptr, t8, 1, x3, i32, 1, SLAM_COST_BASIC, d, gr, u3) == SLAM_ERR_INVALID);
        EXPECT(slam_q3m_eval(nullptr, d, 1, g3, 2, 2, ar, gi, qb, t8, 1, x3, i32, 1, SLAM_COST_MAKHLIN, d, gr, u3) == SLAM_ERR_UNSUPPORTED);
        EXPECT(slam_q3m_eval(nullptr, d, 1, g3, 2, 2, ar, gi, qb, nullptr, 1, x3, i32, 1, SLAM_COST_BASIC, d, gr, u3) == SLAM_ERR_INVALID);
        EXPECT(slam_q3m_eval(nullptr, d, 1, g3, 2, 2, ar, gi, qb, t8, 1, x3, i32, 0, SLAM_COST_BASIC, d, gr, u3) == SLAM_ERR_INVALID);
        {  // eleven three-qubit positions: 108 parameters
            int32_t ar11[11], gi11[11], qb11[33];
            for (int j = 0; j < 11; ++j) { ar11[j] = 3; gi11[j] = 0; qb11[3 * j] = 2; qb11[3 * j + 1] = 0; qb11[3 * j + 2] = 1; }
            EXPECT(slam_q3m_eval(nullptr, nullptr, 0, g3, 1, 11, ar11, gi11, qb11, t8, 1, x3, i32, 1, SLAM_COST_BASIC, d, gr, u3) == SLAM_ERR_UNSUPPORTED);
            EXPECT(std::strstr(slam_last_error(), "108") != nullptr);
            EXPECT(slam_q3m_eval(nullptr, nullptr, 0, g3, 1, 10, ar11, gi11, qb11, t8, 1, x3, i32, 1, SLAM_COST_BASIC, d, gr, u3) == SLAM_ERR_INVALID);
            EXPECT(std::strstr(slam_last_error(), "ctx is NULL") != nullptr);
        }
        EXPECT(slam_q3m_minimize(nullptr, d, 1, g3, 2, 2, ar, gi, qb, t8, 1, SLAM_COST_SQUARE, &prm, 1e-10, nullptr, d, gr, i32, d, i32, i32, i32, nullptr,
                                 nullptr) == SLAM_ERR_INVALID);
        EXPECT(std::strstr(slam_last_error(), "ctx is NULL") != nullptr);
        EXPECT(slam_q3m_minimize(nullptr, d, 1, g3, 2, 16, ar, gi, qb, t8, 1, SLAM_COST_BASIC, &prm, 1e-10, nullptr, d, gr, i32, d, i32, i32, i32, nullptr,
                                 nullptr) == SLAM_ERR_UNSUPPORTED);
        EXPECT(slam_q3m_minimize(nullptr, d, 1, g3, 2, 2, bad_ar, gi, qb, t8, 1, SLAM_COST_BASIC, &prm, 1e-10, nullptr, d, gr, i32, d, i32, i32, i32, nullptr,
                                 nullptr) == SLAM_ERR_INVALID);
        EXPECT(slam_q3m_minimize(nullptr, d, 1, g3, 2, 2, ar, gi, bad_qb, t8, 1, SLAM_COST_BASIC, &prm, 1e-10, nullptr, d, gr, i32, d, i32, i32, i32, nullptr,
                                 nullptr) == SLAM_ERR_INVALID);
        EXPECT(slam_q3m_minimize(nullptr, d, 1, g3, 2, 2, ar, gi, qb, t8, 1, SLAM_COST_MAKHLIN, &prm, 1e-10, nullptr, d, gr, i32, d, i32, i32, i32, nullptr,
                                 nullptr) == SLAM_ERR_UNSUPPORTED);
        EXPECT(slam_q3m_minimize(nullptr, d, 1, g3, 2, 2, ar, gi, qb, t8, 1, SLAM_COST_BASIC, nullptr, 1e-10, nullptr, d, gr, i32, d, i32, i32, i32, nullptr,
                                 nullptr) == SLAM_ERR_INVALID);
        EXPECT(std::strstr(slam_last_error(), "params is NULL") != nullptr);
        EXPECT(slam_q3m_minimize(nullptr, d, 1, g3, 2, 2, ar, gi, qb, t8, 0, SLAM_COST_BASIC, &prm, 1e-10, nullptr, d, gr, i32, d, i32, i32, i32, nullptr,
                                 nullptr) == SLAM_ERR_INVALID);
        {  // explicit start points [1][1][24] (n from the arities), as above
            const double bad[3] = {std::numeric_limits<double>::quiet_NaN(), -std::numeric_limits<double>::infinity(), -1e12};
            for (int at : {0, 23})
                for (double v : bad) {
                    double xb[24] = {0};
                    xb[at] = v;
                    EXPECT(slam_q3m_minimize(nullptr, d, 1, g3, 2, 2, ar, gi, qb, t8, 1, SLAM_COST_BASIC, &prm, 1e-10, xb, d, gr, i32, d, i32, i32, i32,
                                             nullptr, nullptr) == SLAM_ERR_INVALID);
                    EXPECT(std::strstr(slam_last_error(), "explicit seeds must be finite with |x| < 1e8") != nullptr);
                    EXPECT(std::strstr(slam_last_error(), at ? "x0[23]" : "x0[0]") != nullptr);
                }
            double ok[24] = {0};
            ok[0] = -9.9e7;
            ok[23] = 9.9e7;
            EXPECT(slam_q3m_minimize(nullptr, d, 1, g3, 2, 2, ar, gi, qb, t8, 1, SLAM_COST_BASIC, &prm, 1e-10, ok, d, gr, i32, d, i32, i32, i32, nullptr,
                                     nullptr) == SLAM_ERR_INVALID);
            EXPECT(std::strstr(slam_last_error(), "ctx is NULL") != nullptr);
        }
    }
    {  // slam_q3s_eval, slam_q3s_minimize: the cost kind and the states (finite, unit norm to 1e-9) too are checked before the context
        const int32_t ar[2] = {3, 2}, gi[2] = {1, 0}, qb[6] = {0, 1, 2, 1, 2, 7}, bad_ar[2] = {3, 4}, bad_qb[6] = {0, 1, 1, 1, 2, 0};
        static double g3m[2][128] = {{0}}, x3[24] = {0}, gr[24], vout[16];
        const double* g3 = &g3m[0][0];
        double st2[2][16] = {{0}};
        st2[0][6] = 1.0;                               // |011>
        st2[1][1] = st2[1][15] = std::sqrt(0.5);       // (i |000> + i |111>) / sqrt 2
        const double* st = &st2[0][0];
        for (int32_t kind : {SLAM_COST_MUTUAL_INFO, SLAM_COST_MUTUAL_INFO_SQUARE}) {
            EXPECT(slam_q3s_eval(nullptr, d, 1, g3, 2, 2, ar, gi, qb, st, 2, x3, i32, 1, kind, d, gr, vout) == SLAM_ERR_INVALID);
            EXPECT(std::strstr(slam_last_error(), "ctx is NULL") != nullptr);
        }
        for (int32_t kind : {SLAM_COST_BASIC, SLAM_COST_SQUARE, SLAM_COST_MAKHLIN, 5, -1}) {
            EXPECT(slam_q3s_eval(nullptr, d, 1, g3, 2, 2, ar, gi, qb, st, 2, x3, i32, 1, kind, d, gr, vout) == SLAM_ERR_INVALID);
            EXPECT(std::strstr(slam_last_error(), "SLAM_COST_MUTUAL_INFO") != nullptr);
            EXPECT(slam_q3s_minimize(nullptr, d, 1, g3, 2, 2, ar, gi, qb, st, 2, kind, &prm, 1e-10, nullptr, d, gr, i32, d, i32, i32, i32, nullptr,
                                     nullptr) == SLAM_ERR_INVALID);
        }
        for (double v : {std::numeric_limits<double>::quiet_NaN(), std::numeric_limits<double>::infinity(), 1.0 + 1e-8, 0.0}) {
            double sb[2][16];
            std::memcpy(sb, st2, sizeof sb);
            sb[1][15] = v;  // (the last entry of the last state: all of the array is read)
            EXPECT(slam_q3s_eval(nullptr, d, 1, g3, 2, 2, ar, gi, qb, &sb[0][0], 2, x3, i32, 1, SLAM_COST_MUTUAL_INFO, d, gr, vout) == SLAM_ERR_INVALID);
            EXPECT(std::strstr(slam_last_error(), "states[1]") != nullptr);
            EXPECT(slam_q3s_minimize(nullptr, d, 1, g3, 2, 2, ar, gi, qb, &sb[0][0], 2, SLAM_COST_MUTUAL_INFO, &prm, 1e-10, nullptr, d, gr, i32, d, i32, i32,
                                     i32, nullptr, nullptr) == SLAM_ERR_INVALID);
            EXPECT(std::strstr(slam_last_error(), "states[1]") != nullptr);
        }
        EXPECT(slam_q3s_eval(nullptr, d, 1, g3, 2, 2, ar, gi, qb, nullptr, 2, x3, i32, 1, SLAM_COST_MUTUAL_INFO, d, gr, vout) == SLAM_ERR_INVALID);
        EXPECT(slam_q3s_eval(nullptr, d, 1, g3, 2, 2, ar, gi, qb, st, 0, x3, i32, 1, SLAM_COST_MUTUAL_INFO, d, gr, vout) == SLAM_ERR_INVALID);
        EXPECT(slam_q3s_eval(nullptr, d, 1, g3, 2, 2, ar, gi, qb, st, 2, nullptr, i32, 1, SLAM_COST_MUTUAL_INFO, d, gr, vout) == SLAM_ERR_INVALID);
        EXPECT(slam_q3s_eval(nullptr, d, 1, g3, 2, 2, ar, gi, qb, st, 2, x3, i32, 0, SLAM_COST_MUTUAL_INFO, d, gr, vout) == SLAM_ERR_INVALID);
        { const int32_t sof[1] = {2}; EXPECT(slam_q3s_eval(nullptr, d, 1, g3, 2, 2, ar, gi, qb, st, 2, x3, sof, 1, SLAM_COST_MUTUAL_INFO, d, gr, vout) == SLAM_ERR_INVALID); }
        // what the mixed pair checks
        EXPECT(slam_q3s_eval(nullptr, d, 1, g3, 2, SLAM_Q3_MAX_SPAN + 1, ar, gi, qb, st, 2, x3, i32, 1, SLAM_COST_MUTUAL_INFO, d, gr, vout) == SLAM_ERR_UNSUPPORTED);
        EXPECT(slam_q3s_eval(nullptr, d, 1, g3, 2, 2, bad_ar, gi, qb, st, 2, x3, i32, 1, SLAM_COST_MUTUAL_INFO, d, gr, vout) == SLAM_ERR_INVALID);
        EXPECT(std::strstr(slam_last_error(), "arity[1]") != nullptr);
        EXPECT(slam_q3s_eval(nullptr, d, 1, g3, 2, 2, ar, gi, bad_qb, st, 2, x3, i32, 1, SLAM_COST_MUTUAL_INFO, d, gr, vout) == SLAM_ERR_INVALID);
        EXPECT(slam_q3s_eval(nullptr, d, 1, nullptr, 2, 2, ar, gi, qb, st, 2, x3, i32, 1, SLAM_COST_MUTUAL_INFO, d, gr, vout) == SLAM_ERR_INVALID);
        EXPECT(slam_q3s_minimize(nullptr, d, 1, g3, 2, 2, ar, gi, qb, st, 2, SLAM_COST_MUTUAL_INFO_SQUARE, &prm, 1e-10, nullptr, d, gr, i32, d, i32, i32, i32,
                                 nullptr, nullptr) == SLAM_ERR_INVALID);
        EXPECT(std::strstr(slam_last_error(), "ctx is NULL") != nullptr);
        EXPECT(slam_q3s_minimize(nullptr, d, 1, g3, 2, 16, ar, gi, qb, st, 2, SLAM_COST_MUTUAL_INFO, &prm, 1e-10, nullptr, d, gr, i32, d, i32, i32, i32, nullptr,
                                 nullptr) == SLAM_ERR_UNSUPPORTED);
        EXPECT(slam_q3s_minimize(nullptr, d, 1, g3, 2, 2, ar, gi, qb, st, 2, SLAM_COST_MUTUAL_INFO, nullptr, 1e-10, nullptr, d, gr, i32, d, i32, i32, i32, nullptr,
                                 nullptr) == SLAM_ERR_INVALID);
        EXPECT(std::strstr(slam_last_error(), "params is NULL") != nullptr);
        EXPECT(slam_q3s_minimize(nullptr, d, 1, g3, 2, 2, ar, gi, qb, nullptr, 2, SLAM_COST_MUTUAL_INFO, &prm, 1e-10, nullptr, d, gr, i32, d, i32, i32, i32, nullptr,
                                 nullptr) == SLAM_ERR_INVALID);
        {  // explicit start points [2][restarts = 1][24]: the last entry is read
            double xb[48] = {0};
            xb[47] = 1e12;
            EXPECT(slam_q3s_minimize(nullptr, d, 1, g3, 2, 2, ar, gi, qb, st, 2, SLAM_COST_MUTUAL_INFO, &prm, 1e-10, xb, d, gr, i32, d, i32, i32, i32, nullptr,
                                     nullptr) == SLAM_ERR_INVALID);
            EXPECT(std::strstr(slam_last_error(), "x0[47]") != nullptr);
            xb[47] = 9.9e7;
            EXPECT(slam_q3s_minimize(nullptr, d, 1, g3, 2, 2, ar, gi, qb, st, 2, SLAM_COST_MUTUAL_INFO, &prm, 1e-10, xb, d, gr, i32, d, i32, i32, i32, nullptr,
                                     nullptr) == SLAM_ERR_INVALID);
            EXPECT(std::strstr(slam_last_error(), "ctx is NULL") != nullptr);
        }
    }
    {  // slam_ham_eval, slam_ham_minimize: the description, the cost kind, targets, items and start points are checked before the context
        static double mats[17][64][2] = {{{0}}}, tg[2][64][2] = {{{0}}}, xh[3][2] = {{0}}, x0h[2][3][2] = {{{0}}}, lossh[3], gradh[6], uh[3][64][2];
        mats[0][2 * 4 + 1][0] = 1.0;  // (dim = 4: M_0[2][1]; read as dim = 8 the same doubles are M_0[1][1])
        mats[1][3 * 4 + 0][0] = 1.0;
        const double* m = &mats[0][0][0];
        const double* t = &tg[0][0][0];
        const double* x = &xh[0][0];
        const double* x0 = &x0h[0][0][0];
        const int32_t si[17] = {0, 1}, pi[17] = {-1, -1}, tof[3] = {0, 1, 0};
        slam_opt_params hp = prm;
        hp.restarts = 3;
        hp.maxiter = 10;
        auto ev = [&](int32_t dim, int32_t n, int32_t k, const double* mm, const int32_t* s, const int32_t* p, int32_t ti, const double* tt, int64_t nt,
                      const double* xx, const int32_t* to, int64_t M, int32_t cost) {
            return slam_ham_eval(nullptr, dim, n, k, mm, s, p, ti, tt, nt, xx, to, M, cost, lossh, gradh, &uh[0][0][0]);
        };
        auto mn = [&](int32_t dim, int32_t n, int32_t k, const double* mm, const int32_t* s, const int32_t* p, int32_t ti, const double* tt, int64_t nt,
                      int32_t cost, const slam_opt_params* pp, const double* xx0) {
            return slam_ham_minimize(nullptr, dim, n, k, mm, s, p, ti, tt, nt, cost, pp, 1e-10, xx0, d, gradh, i32, d, i32, i32, i32, nullptr, nullptr);
        };
        for (int32_t dim : {4, 8})
            for (int32_t cost : {SLAM_COST_BASIC, SLAM_COST_SQUARE}) {
                EXPECT(ev(dim, 2, 2, m, si, pi, -1, t, 2, x, tof, 3, cost) == SLAM_ERR_INVALID);
                EXPECT(std::strstr(slam_last_error(), "ctx is NULL") != nullptr);
                EXPECT(mn(dim, 2, 2, m, si, pi, 1, t, 2, cost, &hp, x0) == SLAM_ERR_INVALID);
                EXPECT(std::strstr(slam_last_error(), "ctx is NULL") != nullptr);
            }
        for (int32_t dim : {0, 2, 5, 16}) {
            EXPECT(ev(dim, 2, 2, m, si, pi, -1, t, 2, x, tof, 3, 0) == SLAM_ERR_INVALID);
            EXPECT(std::strstr(slam_last_error(), "dim must be") != nullptr);
            EXPECT(mn(dim, 2, 2, m, si, pi, -1, t, 2, 0, &hp, x0) == SLAM_ERR_INVALID);
        }
        EXPECT(ev(4, SLAM_HAM_MAX_PARAMS + 1, 2, m, si, pi, -1, t, 2, x, tof, 3, 0) == SLAM_ERR_UNSUPPORTED);
        EXPECT(mn(4, SLAM_HAM_MAX_PARAMS + 1, 2, m, si, pi, -1, t, 2, 0, &hp, x0) == SLAM_ERR_UNSUPPORTED);
        EXPECT(ev(4, 2, SLAM_HAM_MAX_TERMS + 1, m, si, pi, -1, t, 2, x, tof, 3, 0) == SLAM_ERR_UNSUPPORTED);
        EXPECT(mn(4, 2, SLAM_HAM_MAX_TERMS + 1, m, si, pi, -1, t, 2, 0, &hp, x0) == SLAM_ERR_UNSUPPORTED);
        EXPECT(ev(4, 0, 2, m, si, pi, -1, t, 2, x, tof, 3, 0) == SLAM_ERR_INVALID);
        EXPECT(ev(4, 2, 0, m, si, pi, -1, t, 2, x, tof, 3, 0) == SLAM_ERR_INVALID);
        EXPECT(ev(4, 2, 2, nullptr, si, pi, -1, t, 2, x, tof, 3, 0) == SLAM_ERR_INVALID);
        EXPECT(ev(4, 2, 2, m, nullptr, pi, -1, t, 2, x, tof, 3, 0) == SLAM_ERR_INVALID);
        EXPECT(ev(4, 2, 2, m, si, nullptr, -1, t, 2, x, tof, 3, 0) == SLAM_ERR_INVALID);
        {  // index arrays out of range
            const int32_t s_hi[2] = {0, 2}, s_lo[2] = {-1, 0}, p_hi[2] = {-1, 2}, p_lo[2] = {-2, 0};
            EXPECT(ev(4, 2, 2, m, s_hi, pi, -1, t, 2, x, tof, 3, 0) == SLAM_ERR_INVALID);
            EXPECT(std::strstr(slam_last_error(), "s_index[1]") != nullptr);
            EXPECT(ev(4, 2, 2, m, s_lo, pi, -1, t, 2, x, tof, 3, 0) == SLAM_ERR_INVALID);
            EXPECT(ev(4, 2, 2, m, si, p_hi, -1, t, 2, x, tof, 3, 0) == SLAM_ERR_INVALID);
            EXPECT(std::strstr(slam_last_error(), "phi_index[1]") != nullptr);
            EXPECT(mn(4, 2, 2, m, si, p_lo, -1, t, 2, 0, &hp, x0) == SLAM_ERR_INVALID);
            EXPECT(ev(4, 2, 2, m, si, pi, 2, t, 2, x, tof, 3, 0) == SLAM_ERR_INVALID);
            EXPECT(mn(4, 2, 2, m, si, pi, -2, t, 2, 0, &hp, x0) == SLAM_ERR_INVALID);
            EXPECT(std::strstr(slam_last_error(), "t_index") != nullptr);
            const int32_t to_bad[3] = {0, 2, 0};
            EXPECT(ev(4, 2, 2, m, si, pi, -1, t, 2, x, to_bad, 3, 0) == SLAM_ERR_INVALID);
            EXPECT(std::strstr(slam_last_error(), "target_of[1]") != nullptr);
        }
        for (double v : {std::numeric_limits<double>::quiet_NaN(), std::numeric_limits<double>::infinity()}) {
            static double mb[2][64][2], tb[2][64][2], xb[3][2], x0b[2][3][2];
            std::memcpy(mb, mats, sizeof mb);
            mb[1][63][1] = v;  // (the last entry read at dim = 8: all of the array is looked at)
            EXPECT(ev(8, 2, 2, &mb[0][0][0], si, pi, -1, t, 2, x, tof, 3, 0) == SLAM_ERR_INVALID);
            EXPECT(std::strstr(slam_last_error(), "matrices") != nullptr);
            EXPECT(mn(8, 2, 2, &mb[0][0][0], si, pi, -1, t, 2, 0, &hp, x0) == SLAM_ERR_INVALID);
            std::memcpy(tb, tg, sizeof tb);
            tb[1][63][1] = v;
            EXPECT(ev(8, 2, 2, m, si, pi, -1, &tb[0][0][0], 2, x, tof, 3, 0) == SLAM_ERR_INVALID);
            EXPECT(std::strstr(slam_last_error(), "targets") != nullptr);
            EXPECT(mn(8, 2, 2, m, si, pi, -1, &tb[0][0][0], 2, 0, &hp, x0) == SLAM_ERR_INVALID);
            std::memcpy(xb, xh, sizeof xb);
            xb[2][1] = v;
            EXPECT(ev(4, 2, 2, m, si, pi, -1, t, 2, &xb[0][0], tof, 3, 0) == SLAM_ERR_INVALID);
            EXPECT(std::strstr(slam_last_error(), "x: entry 5") != nullptr);
            std::memcpy(x0b, x0h, sizeof x0b);
            x0b[1][2][1] = v;
            EXPECT(mn(4, 2, 2, m, si, pi, -1, t, 2, 0, &hp, &x0b[0][0][0]) == SLAM_ERR_INVALID);
            EXPECT(std::strstr(slam_last_error(), "x0[11]") != nullptr);
        }
        {  // three terms on one entry
            static double m3[3][16][2] = {{{0}}};
            m3[0][9][0] = m3[1][9][0] = m3[2][9][0] = 1.0;
            const int32_t s3[3] = {0, 1, 0}, p3[3] = {-1, -1, 1};
            EXPECT(ev(4, 2, 3, &m3[0][0][0], s3, p3, -1, t, 2, x, tof, 3, 0) == SLAM_ERR_UNSUPPORTED);
            EXPECT(std::strstr(slam_last_error(), "more than two contributions") != nullptr);
        }
        for (int32_t kind : {SLAM_COST_MAKHLIN, SLAM_COST_MUTUAL_INFO, SLAM_COST_MUTUAL_INFO_SQUARE, 5, -1}) {
            EXPECT(ev(4, 2, 2, m, si, pi, -1, t, 2, x, tof, 3, kind) == SLAM_ERR_INVALID);
            EXPECT(std::strstr(slam_last_error(), "cost kind") != nullptr);
            EXPECT(mn(4, 2, 2, m, si, pi, -1, t, 2, kind, &hp, x0) == SLAM_ERR_INVALID);
        }
        EXPECT(ev(4, 2, 2, m, si, pi, -1, nullptr, 2, x, tof, 3, 0) == SLAM_ERR_INVALID);
        EXPECT(ev(4, 2, 2, m, si, pi, -1, t, 0, x, tof, 3, 0) == SLAM_ERR_INVALID);
        EXPECT(ev(4, 2, 2, m, si, pi, -1, t, 2, nullptr, tof, 3, 0) == SLAM_ERR_INVALID);
        EXPECT(ev(4, 2, 2, m, si, pi, -1, t, 2, x, nullptr, 3, 0) == SLAM_ERR_INVALID);
        EXPECT(ev(4, 2, 2, m, si, pi, -1, t, 2, x, tof, 0, 0) == SLAM_ERR_INVALID);
        EXPECT(mn(4, 2, 2, m, si, pi, -1, t, 2, 0, nullptr, x0) == SLAM_ERR_INVALID);
        EXPECT(std::strstr(slam_last_error(), "params is NULL") != nullptr);
        EXPECT(mn(4, 2, 2, m, si, pi, -1, t, 2, 0, &hp, nullptr) == SLAM_ERR_INVALID);
        EXPECT(std::strstr(slam_last_error(), "x0 is required") != nullptr);
    }
    {  // slam_hams_eval, slam_hams_minimize: the per-slice index rows and entry lists, the diagonal merge, everything before the context
        static double mats[4][16][2] = {{{0}}}, tg[2][16][2] = {{{0}}}, xh[3][4] = {{0}}, x0h[2][3][4] = {{{0}}}, lossh[3], gradh[12], uh[3][16][2];
        mats[0][2 * 4 + 1][0] = 1.0;
        mats[1][3 * 4 + 0][0] = 1.0;
        mats[2][0][0] = mats[2][1 * 4 + 1][0] = 0.5;  // two diagonal terms that share entry (0, 0)
        mats[3][0][0] = mats[3][2 * 4 + 2][0] = 0.5;
        const double* m = &mats[0][0][0];
        const double* t = &tg[0][0][0];
        constexpr int S = SLAM_HAMS_MAX_SLICES;
        int32_t si[S][4], pi[S][4];
        for (int s = 0; s < S; ++s)
            for (int k = 0; k < 4; ++k) {
                si[s][k] = (k + s) % 4;
                pi[s][k] = k < 2 ? (s % 2 ? 3 : -1) : -1;
            }
        const int32_t tof[3] = {0, 1, 0};
        slam_opt_params hp = prm;
        hp.restarts = 3;
        hp.maxiter = 10;
        auto ev = [&](int32_t n, int32_t k, int32_t slices, const int32_t* s, const int32_t* p, int32_t ti, int32_t cost) {
            return slam_hams_eval(nullptr, 4, n, k, slices, m, s, p, ti, t, 2, &xh[0][0], tof, 3, cost, lossh, gradh, &uh[0][0][0]);
        };
        auto mn = [&](int32_t n, int32_t k, int32_t slices, const int32_t* s, const int32_t* p, int32_t ti, int32_t cost, const double* xx0) {
            return slam_hams_minimize(nullptr, 4, n, k, slices, m, s, p, ti, t, 2, cost, &hp, 1e-10, xx0, d, gradh, i32, d, i32, i32, i32, nullptr, nullptr);
        };
        for (int32_t slices = 1; slices <= S; ++slices) {  // good descriptions: the context is looked at last
            EXPECT(ev(4, 4, slices, &si[0][0], &pi[0][0], 3, SLAM_COST_SQUARE) == SLAM_ERR_INVALID);
            EXPECT(std::strstr(slam_last_error(), "ctx is NULL") != nullptr);
            EXPECT(mn(4, 4, slices, &si[0][0], &pi[0][0], -1, SLAM_COST_BASIC, &x0h[0][0][0]) == SLAM_ERR_INVALID);
            EXPECT(std::strstr(slam_last_error(), "ctx is NULL") != nullptr);
        }
        EXPECT(ev(4, 4, 0, &si[0][0], &pi[0][0], -1, 0) == SLAM_ERR_INVALID);
        EXPECT(ev(4, 4, S + 1, &si[0][0], &pi[0][0], -1, 0) == SLAM_ERR_UNSUPPORTED);
        EXPECT(std::strstr(slam_last_error(), "n_slices") != nullptr);
        EXPECT(mn(4, 4, -3, &si[0][0], &pi[0][0], -1, 0, &x0h[0][0][0]) == SLAM_ERR_INVALID);
        {  // an index out of range in the last slice only; a diagonal term on a phase is not merged
            int32_t sb[S][4], pb[S][4];
            std::memcpy(sb, si, sizeof sb);
            std::memcpy(pb, pi, sizeof pb);
            sb[S - 1][3] = 4;
            EXPECT(ev(4, 4, S, &sb[0][0], &pi[0][0], -1, 0) == SLAM_ERR_INVALID);
            EXPECT(std::strstr(slam_last_error(), "slice 7: s_index[3]") != nullptr);
            EXPECT(ev(4, 4, S - 1, &sb[0][0], &pi[0][0], -1, 0) == SLAM_ERR_INVALID);
            EXPECT(std::strstr(slam_last_error(), "ctx is NULL") != nullptr);
            pb[2][2] = pb[2][3] = 0;
            EXPECT(mn(4, 4, S, &si[0][0], &pb[0][0], -1, 0, &x0h[0][0][0]) == SLAM_ERR_UNSUPPORTED);
            EXPECT(std::strstr(slam_last_error(), "slice 2: entry (0, 0)") != nullptr);
        }
        EXPECT(ev(4, 4, 2, &si[0][0], &pi[0][0], -1, SLAM_COST_MAKHLIN) == SLAM_ERR_INVALID);
        x0h[1][2][3] = std::numeric_limits<double>::infinity();
        EXPECT(mn(4, 4, 2, &si[0][0], &pi[0][0], -1, 0, &x0h[0][0][0]) == SLAM_ERR_INVALID);
        EXPECT(std::strstr(slam_last_error(), "x0[23]") != nullptr);
        EXPECT(mn(4, 4, 2, &si[0][0], &pi[0][0], -1, 0, nullptr) == SLAM_ERR_INVALID);
    }
    EXPECT(slam_set_cost(nullptr, 0) == SLAM_ERR_INVALID);
    EXPECT(slam_synchronize(nullptr) == SLAM_ERR_INVALID);
    EXPECT(slam_get_stats(nullptr, &st) == SLAM_ERR_INVALID);
    EXPECT(slam_reset_stats(nullptr) == SLAM_ERR_INVALID);
    EXPECT(slam_best_loss_device_ptr(nullptr, &p, &i64) == SLAM_ERR_INVALID);
    { float f32[1] = {0.0f}; EXPECT(slam_metric_update_check(nullptr, 3, f32, f32, f32, f32, 1, f32, f32) == SLAM_ERR_INVALID); }
    { int dev = 0; EXPECT(slam_ctx_device(nullptr, &dev) == SLAM_ERR_INVALID); }
    // communicator: bad arguments; without RCCL or without a device creation fails with a message
    slam_comm* comm = nullptr;
    char id[SLAM_COMM_ID_BYTES] = {0};
    EXPECT(slam_comm_get_unique_id(nullptr) == SLAM_ERR_INVALID);
    EXPECT(slam_comm_init(0, 0, 1, nullptr, &comm) == SLAM_ERR_INVALID);
    EXPECT(slam_comm_init(0, 2, 2, id, &comm) == SLAM_ERR_INVALID && comm == nullptr);
    EXPECT(slam_comm_init(0, 0, 1, id, nullptr) == SLAM_ERR_INVALID);
    EXPECT(slam_comm_destroy(nullptr) == SLAM_OK);
    EXPECT(slam_comm_rank(nullptr, nullptr, nullptr) == SLAM_ERR_INVALID);
    EXPECT(slam_comm_allreduce_f64(nullptr, d, 1, SLAM_OP_MIN) == SLAM_ERR_INVALID);
    EXPECT(slam_comm_barrier(nullptr) == SLAM_ERR_INVALID);
    EXPECT(slam_comm_merge_begin(nullptr, 1) == SLAM_ERR_INVALID);
    EXPECT(slam_comm_merge_add(nullptr, nullptr, 0, 0, 0) == SLAM_ERR_INVALID);
    EXPECT(slam_comm_merge_add_host(nullptr, d, 1, 0) == SLAM_ERR_INVALID);
    EXPECT(slam_allreduce_min(nullptr, 1e-8, &i64, d, 1) == SLAM_ERR_INVALID);
    // the message is thread-local: concurrent failing calls do not trample each other
    std::vector<std::thread> th;
    for (int t = 0; t < 8; ++t)
        th.emplace_back([t] {
            for (int r = 0; r < 200; ++r) {
                slam_ctx* c = nullptr;
                if (slam_ctx_create(-1 - t, &c) == SLAM_OK) ++fails;
                char want[32];
                std::snprintf(want, sizeof(want), "device %d ", -1 - t);
                if (slam_device_count(nullptr) != SLAM_ERR_INVALID) ++fails;
                (void)want;
            }
        });
    for (auto& x : th) x.join();
    std::printf(fails ? "asan host driver: %d FAILURES\n" : "asan host driver: ok\n", fails);
    return fails ? 1 : 0;
}
