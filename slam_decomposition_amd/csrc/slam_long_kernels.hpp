// slam_long_kernels.hpp -- the four __global__ kernels of the wavefront-per-item templates (slam_long.hpp holds their device
// functions, which slam_smush.hpp uses too).  Included by ONE unit, slam_hip.hip.
#pragma once
#include "slam_long.hpp"

namespace slamdev {

// ---------------------------------------------------------------------------------------------------------------------------
// slam_eval_loss_grad / slam_eval_unitary for 6 .. 16 gates: one item per wavefront
// ---------------------------------------------------------------------------------------------------------------------------
// The kernel bodies live in slam_long_eval.inc / slam_long_minimize.inc and are included into the BasicCost / SquareCost kernel and its
// MakhlinFunctionalCost twin with the constant MK (if constexpr).  (A shared forceinline body template instead changed the register
// allocation of the existing kernels: it is simplified once on its own before it is inlined -- eval_long_kernel 181 -> 180 VGPRs,
// minimize_long_kernel 246 -> 251 VGPRs and 125 -> 115 SGPR spills, with other instructions.)
__global__ void __launch_bounds__(kWave, 2) eval_long_kernel(LongEvalArgs a) {
    constexpr bool MK = false;
#include "slam_long_eval.inc"
}
// MakhlinFunctionalCost (SLAM_COST_MAKHLIN)
__global__ void __launch_bounds__(kWave, 2) eval_long_mk_kernel(LongEvalArgs a) {
    constexpr bool MK = true;
#include "slam_long_eval.inc"
}

// ---------------------------------------------------------------------------------------------------------------------------
// Quasi-Newton minimisation (the iteration of minimize_body / oracle/bfgs_port.py), one item per wavefront, persistent wavefronts
// pulling (restart-major) queue positions.  Lane l holds components 2l and 2l + 1 of x, g, p; the fp32 inverse Hessian approximation
// H (n rows of kLongHStride floats in device memory, this wavefront's slice) is read row by row as float2 per lane: since H is
// symmetric, lane l's two COLUMNS give its two components of H v, and a row is one coalesced 8 n-byte access of the wavefront.
// ---------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kWave, 2) minimize_long_kernel(LongArgs args) {
    constexpr bool MK = false;
#include "slam_long_minimize.inc"
}
// MakhlinFunctionalCost (SLAM_COST_MAKHLIN)
__global__ void __launch_bounds__(kWave, 2) minimize_long_mk_kernel(LongArgs args) {
    constexpr bool MK = true;
#include "slam_long_minimize.inc"
}

}  // namespace slamdev
