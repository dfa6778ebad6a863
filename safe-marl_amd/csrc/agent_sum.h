// agent_sum.h — the agent-summed action selection of matd3.py:92-97 / iddpg.py:66-71 under util.py:57-64 for ONE (environment,
// action component): csrc/rollout.hip (agent_sum_explore_kernel, one thread per pair) and csrc/flexenv.hip (the selection phase
// of the summed rollout burst, lanes 0 .. 2 act_dim - 1 of a wavefront for its own two environments).  One body, so that the
// two forms round in the same places: the burst equals the three launches per step bit for bit
// (tests/test_summed_burst_gpu.py).  Below it the form with per-sample log-stds, shared in the same way by csrc/gauss.hip
// (gauss_sum_explore_kernel) and the Gaussian summed burst (tests/test_gauss_burst_gpu.py).
#ifndef FLEX_AGENT_SUM_H
#define FLEX_AGENT_SUM_H
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "flex_nan.h"

// `m`: component k of agent 0's mean of the environment (agents `ad` floats apart); `eps`: this pair's standard-normal draw or
// NULL (no exploration: the summed mean itself, util.py:75-77 behind matd3.py:94-96); `std`: component k's exp of the
// agent-summed log-std (only read with eps).  `action` / `env_action` (may be NULL): component k of agent 0's row of the
// environment — every agent gets the one action and translate_action of it (util.py:125-128).
__device__ __forceinline__ void agent_sum_select(const float* m, int n, int ad, const float* eps,
                                                 const float* std, float act_low, float act_high,
                                                 float* action, float* env_action) {
    float s = m[0];
    for (int i = 1; i < n; ++i) s = __fadd_rn(s, m[i * ad]);                            // ((m0 + m1) + m2) + ...
    const float y = eps ? tanhf(__fadd_rn(s, __fmul_rn(*eps, *std))) : s;              // tanh(loc + eps * scale)
    const float span = act_high - act_low;
    const float c = clamp_nan(y, act_low, act_high);                                   // th.clamp: a NaN action stays NaN
    const float ev = __fadd_rn(__fmul_rn(__fmul_rn(0.5f, __fadd_rn(c, 1.0f)), span), act_low);
    for (int i = 0; i < n; ++i) action[i * ad] = y;
    if (env_action)
        for (int i = 0; i < n; ++i) env_action[i * ad] = ev;
}

// translate_action (util.py:125-128) with the roundings of scale_action's tensor ops; a NaN action stays NaN, as through th.clamp
__device__ __forceinline__ float gauss_env_action(float y, float lo, float hi) {
    const float c = clamp_nan(y, lo, hi);
    return __fadd_rn(__fmul_rn(__fmul_rn(0.5f, __fadd_rn(c, 1.0f)), hi - lo), lo);
}

// The same selection with per-sample log-stds (gaussian_policy): csrc/gauss.hip (gauss_sum_explore_kernel, one thread per pair)
// and the selection phase of the Gaussian summed rollout burst (csrc/flexenv.hip), one body for the same reason.  `m`, `l`:
// component k of agent 0's mean and log-std of the environment; means and log-stds are summed in agent order, each add rounded
// on its own, y = tanhf(s + eps * expf(ls)) with product and sum rounded separately.
__device__ __forceinline__ void gauss_sum_select(const float* m, const float* l, int n, int ad, float eps, float act_low,
                                                 float act_high, float* action, float* env_action) {
    float s = m[0], ls = l[0];
    for (int i = 1; i < n; ++i) {                                                        // ((x0 + x1) + x2) + ...
        s = __fadd_rn(s, m[i * ad]);
        ls = __fadd_rn(ls, l[i * ad]);
    }
    const float y = tanhf(__fadd_rn(s, __fmul_rn(eps, expf(ls))));                     // tanh(loc + eps * scale)
    for (int i = 0; i < n; ++i) action[i * ad] = y;
    if (env_action) {
        const float ev = gauss_env_action(y, act_low, act_high);
        for (int i = 0; i < n; ++i) env_action[i * ad] = ev;
    }
}

#endif
