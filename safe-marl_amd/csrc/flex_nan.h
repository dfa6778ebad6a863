// flex_nan.h — the NaN-propagating ReLU and clamp of the kernels that stand in for torch.relu / torch.clamp: csrc/actor.hip and
// csrc/flexenv.hip through actor_r16.h, csrc/qmix.hip, and the environment-action clamps of csrc/gauss.hip (gauss_env_action) and
// csrc/rollout.hip (agent_sum_explore_kernel).
#ifndef FLEX_NAN_H
#define FLEX_NAN_H
#include <hip/hip_runtime.h>

// ReLU and clamp that hand a NaN on, as torch.relu / torch.clamp do (fmaxf / fminf return the other operand: a NaN observation
// would come out as a finite action): IEEE 754-2019 maximum / minimum, one v_maximum3_f32 / v_minimum3_f32 each on gfx950.
// Finite values: the same bits as fmaxf(v, 0) / fminf(fmaxf(v, lo), hi).
__device__ __forceinline__ float relu_nan(float v) { return __builtin_elementwise_maximum(v, 0.0f); }
__device__ __forceinline__ float clamp_nan(float v, float lo, float hi) {
    return __builtin_elementwise_minimum(__builtin_elementwise_maximum(v, lo), hi);
}

#endif
