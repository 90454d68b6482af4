// slam_analytic.hip -- host side of libslamhip.so, analytic unit: the closed-form decomposition into sqrt(iSWAP) gates
// (slam_analytic.hpp).
#include "slam_host.hpp"

// slam_kak.hpp and the headers under it define their __global__ kernels where they are included, and slam_geometry.hip is the unit that
// emits them (slam_host.hpp).  This unit calls their __device__ functions only: here those kernels are read as function templates
// that nothing instantiates, so no second copy of them is emitted, on the host or on the device.
#pragma push_macro("__global__")
#undef __global__
#define __global__ template <int = 0> __attribute__((global))
#include "slam_kak.hpp"
#pragma pop_macro("__global__")
#include "slam_analytic.hpp"

extern "C" {

int slam_sqiswap_decompose(slam_ctx* ctx, int64_t first, int64_t count, double* x_out, int32_t* cycles, double* loss, double* gap) {
    if (!ctx) return fail(SLAM_ERR_INVALID, "ctx is NULL");
    if (first < 0 || count < 0 || first + count > ctx->n_targets)
        return fail(SLAM_ERR_INVALID, "target window outside the resident batch");
    if (count > 0x7fffffffLL) return fail(SLAM_ERR_INVALID, "too many targets in one call (%lld)", (long long)count);
    if (count == 0) return SLAM_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(ctx->ev_grad.reserve((size_t)count * 24 * sizeof(double)));  // the rows
    HIP_TRY(ctx->ev_loss.reserve((size_t)count * 2 * sizeof(double)));   // losses, then gaps
    HIP_TRY(ctx->ev_tof.reserve((size_t)count * sizeof(int32_t)));       // sizes
    AnalyticArgs a{};
    a.targets = ctx->targets.as<double>() + first * 32;
    a.M = count;
    a.x_out = ctx->ev_grad.as<double>();
    a.cycles = ctx->ev_tof.as<int32_t>();
    a.loss = ctx->ev_loss.as<double>();
    a.gap = ctx->ev_loss.as<double>() + count;
    hipLaunchKernelGGL(sqiswap_decompose_kernel, dim3((unsigned)((count + kKakBlock - 1) / kKakBlock)), dim3(kKakBlock), 0, ctx->stream, a);
    HIP_TRY(hipGetLastError());
    if (x_out) HIP_TRY(hipMemcpyAsync(x_out, a.x_out, (size_t)count * 24 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    if (cycles) HIP_TRY(hipMemcpyAsync(cycles, a.cycles, (size_t)count * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    if (loss) HIP_TRY(hipMemcpyAsync(loss, a.loss, (size_t)count * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    if (gap) HIP_TRY(hipMemcpyAsync(gap, a.gap, (size_t)count * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return SLAM_OK;
}

}  // extern "C"
