// ppo.hip — the PPO update of IPPO / MAPPO around the networks: GAE, the clipped policy loss and the clipped value loss,
// each with its gradient, in a handful of launches (gfx950).  Boundary: include/flexnet.h (flexnet_ppo_*).
//
// madrl/learning_algorithms/ppo.py:14-69 behind model.py:308-323.  The tensors are [rows, n] fp32 with n <= 8: launch- and
// dependency-bound, like the DDPG value loss of tdloss.hip whose statistics pass and finish this file reuses.
//   gae:     r^ = BatchNorm1d(n)(reward);  delta_i = r^_i + gamma V_old(s'_i) m_i - V_old(s_i);
//            A_i = delta_i + gamma lambda m_i A_{i + stride},  m_i = 1 - done_i where last_step_i, else 1;
//            A^ = BatchNorm1d(n)(A) when normalize_advantages.  Both modules' running statistics move as nn.BatchNorm1d
//            moves them.  The recurrence is a composition of affine maps x -> b_i + a_i x: a chain is a reverse scan.
//   policy:  mu = sum over agents of the means;  log p = sum_k log N(act_k; mu_k, sigma_k);  ratio = exp(log p - old);
//            loss = -mean(min(ratio A^, clamp(ratio, 1 -+ eps) A^));  d loss / d means (the same for every agent).
//            ONE body, two instantiations: sigma from a fixed log_std [a] (flexnet_ppo_policy_loss), or from the Gaussian
//            actors' log_stds [rows, n, a], summed over agents per row like the means, with d loss / d log_stds besides
//            (flexnet_ppo_policy_loss_rows, declared in flexnet.h's Gaussian section).
//   value:   ret = r^ + gamma (1 - done) V(s');  vc = old + clamp(V - old, -+eps);
//            loss = coef mean(max((V - ret)^2, (vc - ret)^2));  d loss / d V.
// Pointwise values are formed in fp32 in the order the tensor composition forms them (so branch decisions agree with it);
// the scan state and every sum are fp64 in a fixed order.  No atomics: the same inputs give the same bits.
//
// Subgradients at ties, as PyTorch's: th.min / th.max of two tensors hand HALF of the incoming gradient to each argument
// where they are equal; th.clamp passes the gradient where lo <= x <= hi, both ends included.  So a ratio inside the clip
// range (surr1 == surr2) gets 1/2 + 1/2 of d/d ratio, a ratio outside it with A^ == 0 gets 1/2 of it (times A^ = 0), and a
// value exactly eps away from the old one still passes the clipped branch's gradient.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>
#include "flexnet.h"
#include "flex_launch.h"
#include "flex_reduce.h"
#include "flex_td.h"

#define PPO_THREADS 256
#define PPO_BLOCKS FLEXNET_PPO_BLOCKS        // per-block partial sums of the losses
#define PPO_WS_REWARD 0                      // workspace (doubles): reward statistics | advantage statistics | loss partials
#define PPO_WS_ADV (FLEXNET_TD_WS_FLOATS / 2)
#define PPO_WS_LOSS FLEXNET_TD_WS_FLOATS
#define PPO_LANE_MAX_STEPS 256               // chains up to this long: one lane walks the chain
#define PPO_LANE_MIN_CHAINS 16384            // ... and longer ones when there are this many (every CU busy anyway)

// the FlexTdLossArgs view of one of the two BatchNorm modules (tdloss.hip's statistics pass / td_finish work on it)
__host__ __device__ static inline FlexTdLossArgs ppo_bn_view(const FlexPpoGaeArgs& a, const FlexPpoBatchNorm& bn, const float* x,
                                                             int ws_off) {
    FlexTdLossArgs t = {};
    t.rows = (int32_t)a.rows; t.n_agents = a.n_agents; t.normalise = bn.enabled;
    t.bn_eps = bn.eps; t.bn_momentum = bn.momentum;
    t.reward = x;
    t.bn_weight = bn.weight; t.bn_bias = bn.bias;
    t.running_mean = bn.running_mean; t.running_var = bn.running_var; t.num_batches_tracked = bn.num_batches_tracked;
    t.workspace = a.workspace + 2 * ws_off; t.workspace_floats = FLEXNET_TD_WS_FLOATS;
    return t;
}

struct PpoStep { float a, b; };      // A_i = b + a A_next

// delta and the recurrence's factor of row `row`, agent j; writes the normalised reward
__device__ __forceinline__ PpoStep ppo_step(const FlexPpoGaeArgs& a, int64_t row, int j, float mean, float scale, float shift) {
    const int64_t idx = row * a.n_agents + j;
    const float m = a.last_step[row] != 0.0f ? 1.0f - a.done[row] : 1.0f;
    const float rn = a.reward_bn.enabled ? (a.reward[idx] - mean) * scale + shift : a.reward[idx];
    a.reward_norm[idx] = rn;
    PpoStep s;
    s.b = rn + a.gamma * a.old_next_values[idx] * m - a.old_values[idx];       // ppo.py:49
    s.a = a.gamma * a.lambda_ * m;                                             // ppo.py:50
    return s;
}

// one lane per chain (env e, agent j): rows e, e + stride, ... walked from the last one back
__global__ __launch_bounds__(PPO_THREADS) void ppo_gae_lane_kernel(FlexPpoGaeArgs a, int64_t chains) {
    const int64_t c = (int64_t)blockIdx.x * PPO_THREADS + threadIdx.x;
    if (c >= chains) return;
    const int n = a.n_agents;
    const int64_t e = c / n;
    const int j = (int)(c - e * n);
    float mean, scale, shift;
    td_column_affine(ppo_bn_view(a, a.reward_bn, a.reward, PPO_WS_REWARD), j, mean, scale, shift);
    const int64_t steps = (a.rows - e + a.chain_stride - 1) / a.chain_stride;
    double adv = 0.0;
    for (int64_t t = steps - 1; t >= 0; --t) {
        const int64_t row = t * a.chain_stride + e;
        const PpoStep s = ppo_step(a, row, j, mean, scale, shift);
        adv = (double)s.b + (double)s.a * adv;
        a.advantages[row * n + j] = (float)adv;
    }
}

// one wavefront per chain: tiles of 64 steps from the end of the chain back; lane 0 holds the LAST step of its tile, so the
// successor of lane l is lane l - 1 and the reverse scan is an inclusive scan in lane order over the maps x -> b + a x
__global__ __launch_bounds__(64) void ppo_gae_wave_kernel(FlexPpoGaeArgs a) {
    const int lane = threadIdx.x, n = a.n_agents;
    const int64_t c = blockIdx.x;
    const int64_t e = c / n;
    const int j = (int)(c - e * n);
    float mean, scale, shift;
    td_column_affine(ppo_bn_view(a, a.reward_bn, a.reward, PPO_WS_REWARD), j, mean, scale, shift);
    const int64_t steps = (a.rows - e + a.chain_stride - 1) / a.chain_stride;
    double carry = 0.0;                                   // the advantage of the step after this tile
    for (int64_t end = steps; end > 0; end -= 64) {
        const int64_t t = end - 1 - lane;
        double fa = 1.0, fb = 0.0;                        // the identity map in the lanes past the chain's start
        if (t >= 0) {
            const PpoStep s = ppo_step(a, t * a.chain_stride + e, j, mean, scale, shift);
            fa = (double)s.a; fb = (double)s.b;
        }
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const double pa = __shfl_up(fa, off, 64), pb = __shfl_up(fb, off, 64);
            if (lane >= off) { fb = fb + fa * pb; fa = fa * pa; }
        }
        const double adv = fb + fa * carry;
        if (t >= 0) a.advantages[(t * a.chain_stride + e) * n + j] = (float)adv;
        carry = __shfl(adv, 63, 64);
    }
}

// A^ = BatchNorm(A) with the batch statistics of the second statistics pass; block 0 then moves BOTH modules' running
// statistics (they depend on the workspace alone)
__global__ __launch_bounds__(PPO_THREADS) void ppo_gae_finish_kernel(FlexPpoGaeArgs a) {
    __shared__ float mean_s[TD_NA], scale_s[TD_NA], shift_s[TD_NA];
    const int tid = threadIdx.x, n = a.n_agents;
    const FlexTdLossArgs av = ppo_bn_view(a, a.adv_bn, a.advantages, PPO_WS_ADV);
    if (a.adv_bn.enabled) {
        if (tid < TD_NA) {
            float m, sc, sh;
            td_column_affine(av, tid, m, sc, sh);
            mean_s[tid] = m; scale_s[tid] = sc; shift_s[tid] = sh;
        }
        __syncthreads();
        const int64_t total = a.rows * n;
        for (int64_t idx = (int64_t)blockIdx.x * PPO_THREADS + tid; idx < total; idx += (int64_t)gridDim.x * PPO_THREADS) {
            const int j = (int)(idx % n);
            a.advantages_norm[idx] = (a.advantages[idx] - mean_s[j]) * scale_s[j] + shift_s[j];
        }
    }
    if (blockIdx.x == 0 && tid < 64) {
        if (a.reward_bn.enabled) td_finish(ppo_bn_view(a, a.reward_bn, a.reward, PPO_WS_REWARD), 0, tid);
        if (a.adv_bn.enabled) td_finish(av, 0, tid);
    }
}

static bool ppo_bn_ok(const FlexPpoBatchNorm& bn) {
    return !bn.enabled || ((bn.running_mean == nullptr) == (bn.running_var == nullptr));
}

extern "C" int flexnet_ppo_gae(const FlexPpoGaeArgs* a, void* stream) {
    if (!a || a->rows < 1 || a->n_agents < 1 || a->chain_stride < 1 || !a->reward || !a->old_values || !a->old_next_values ||
        !a->done || !a->last_step || !a->reward_norm || !a->advantages || !a->workspace ||
        a->workspace_floats < FLEXNET_PPO_WS_FLOATS || !flex_aligned(a->workspace, 8) ||
        (a->adv_bn.enabled && !a->advantages_norm) || !ppo_bn_ok(a->reward_bn) || !ppo_bn_ok(a->adv_bn))
        return FLEXNET_EINVAL;
    if (a->n_agents > TD_NA || a->rows > (int64_t)INT32_MAX / TD_NA) return FLEXNET_EUNSUPPORTED;
    hipStream_t s = (hipStream_t)stream;
    if (a->reward_bn.enabled) flex_td_launch_stats(ppo_bn_view(*a, a->reward_bn, a->reward, PPO_WS_REWARD), s);
    const int64_t per_agent = a->chain_stride < a->rows ? a->chain_stride : a->rows;
    const int64_t chains = per_agent * a->n_agents;
    const int64_t steps = (a->rows + a->chain_stride - 1) / a->chain_stride;
    if (steps <= PPO_LANE_MAX_STEPS || chains >= PPO_LANE_MIN_CHAINS)
        hipLaunchKernelGGL(ppo_gae_lane_kernel, dim3((unsigned)((chains + PPO_THREADS - 1) / PPO_THREADS)), dim3(PPO_THREADS), 0, s,
                           *a, chains);
    else
        hipLaunchKernelGGL(ppo_gae_wave_kernel, dim3((unsigned)chains), dim3(64), 0, s, *a);
    if (a->adv_bn.enabled) flex_td_launch_stats(ppo_bn_view(*a, a->adv_bn, a->advantages, PPO_WS_ADV), s);
    if (a->adv_bn.enabled || a->reward_bn.enabled) {
        const int64_t total = a->rows * a->n_agents;
        int64_t blocks = a->adv_bn.enabled ? (total + PPO_THREADS - 1) / PPO_THREADS : 1;
        if (blocks > 1024) blocks = 1024;
        hipLaunchKernelGGL(ppo_gae_finish_kernel, dim3((unsigned)blocks), dim3(PPO_THREADS), 0, s, *a);
    }
    return flex_launch_status();
}


// th.min / th.max / th.clamp hand a NaN on (fminf / fmaxf would drop it and report a finite loss for a diverged run)
__device__ __forceinline__ float ppo_minf(float a, float b) { return (a < b || a != a) ? a : b; }
__device__ __forceinline__ float ppo_maxf(float a, float b) { return (a > b || a != a) ? a : b; }
__device__ __forceinline__ float ppo_clampf(float x, float lo, float hi) { return x < lo ? lo : (x > hi ? hi : x); }

// ---- the two losses: one thread per row, per-block partial sums (fp64, fixed tree), a one-wavefront finish ---------------
__global__ __launch_bounds__(64) void ppo_loss_finish_kernel(const double* partial, double scale, float* loss) {
    flex_loss_finish(partial, PPO_BLOCKS, scale, loss);
}

// Normal(mu, sd).log_prob(x) = -(x - mu)^2 inv2var - logc, and its d / d mu = (x - mu) invvar
__device__ __forceinline__ void ppo_normal(float sd, float& inv2var, float& invvar, float& logc) {
    const float var = sd * sd;
    inv2var = 1.0f / (2.0f * var); invvar = 1.0f / var;
    logc = logf(sd) + 0.918938533204672742f;           // log(std) + log(sqrt(2 pi))
}

// The policy loss, ONE body: A = FlexPpoPolicyArgs (the fixed-std policy: log_std [a], already summed over the agents, so the
// Normal's constants are formed once in front of the row loop) or FlexPpoPolicyRowsArgs (learned log-stds [rows, n, a], summed
// over the agents per row like the means: the constants are formed per row, and d_log_stds comes out besides d_means).
template <class A>
__device__ __forceinline__ void ppo_policy(const A& a) {
    constexpr bool ROWS = std::is_same_v<A, FlexPpoPolicyRowsArgs>;
    const int n = a.n_agents, na = a.act_dim;
    const float lo = 1.0f - a.eps_clip, hi = 1.0f + a.eps_clip;
    const float inv = 1.0f / (float)(a.rows * n);
    float inv2var[FLEXNET_MAX_ACT], invvar[FLEXNET_MAX_ACT], logc[FLEXNET_MAX_ACT];
    if constexpr (!ROWS) {
#pragma unroll
        for (int k = 0; k < FLEXNET_MAX_ACT; ++k) ppo_normal(k < na ? expf(a.log_std[k]) : 1.0f, inv2var[k], invvar[k], logc[k]);
    }
    double acc = 0.0;
    for (int64_t b = (int64_t)blockIdx.x * PPO_THREADS + threadIdx.x; b < a.rows; b += (int64_t)PPO_BLOCKS * PPO_THREADS) {
        const float* mp = a.means + b * n * na;
        const float* ap = a.actions + b * n * na;
        const float* lp = nullptr;
        if constexpr (ROWS) lp = a.log_stds + b * n * na;
        float mu[FLEXNET_MAX_ACT], g[FLEXNET_MAX_ACT], gl[FLEXNET_MAX_ACT];
#pragma unroll
        for (int k = 0; k < FLEXNET_MAX_ACT; ++k) {
            float s = 0.0f, l = 0.0f;
            if (k < na) {
                s = mp[k];
                if constexpr (ROWS) l = lp[k];
                for (int i = 1; i < n; ++i) {           // agent order, as the pointwise adds of the composition
                    s += mp[i * na + k];
                    if constexpr (ROWS) l += lp[i * na + k];
                }
            }
            mu[k] = s; g[k] = 0.0f; gl[k] = 0.0f;
            if constexpr (ROWS) ppo_normal(expf(l), inv2var[k], invvar[k], logc[k]);
        }
        for (int i = 0; i < n; ++i) {
            float logp = 0.0f, old = 0.0f;
#pragma unroll
            for (int k = 0; k < FLEXNET_MAX_ACT; ++k)
                if (k < na) {
                    const float x = ap[i * na + k], d = x - mu[k];
                    logp += -(d * d) * inv2var[k] - logc[k];
                    old += x;                                          // model.py:313: old_log_prob_a IS the action
                }
            if (a.old_log_prob) old = a.old_log_prob[b * n + i];
            const float ratio = expf(logp - old);
            const float adv = a.advantages[b * n + i];
            const bool inside = ratio >= lo && ratio <= hi;
            const float clipped = ppo_clampf(ratio, lo, hi);
            const float s1 = ratio * adv, s2 = clipped * adv;
            acc += (double)ppo_minf(s1, s2);
            // th.min: half the gradient to each argument at a tie; th.clamp: gradient inside [lo, hi], ends included
            const float w1 = s1 < s2 ? 1.0f : (s1 == s2 ? 0.5f : 0.0f);
            const float w2 = (1.0f - w1) * (inside ? 1.0f : 0.0f);
            const float dlogp = -inv * (w1 + w2) * adv * ratio;        // d loss / d log p[b, i]
            if (a.ratio) a.ratio[b * n + i] = ratio;
#pragma unroll
            for (int k = 0; k < FLEXNET_MAX_ACT; ++k)
                if (k < na) {
                    const float d = ap[i * na + k] - mu[k];
                    g[k] += dlogp * d * invvar[k];
                    if constexpr (ROWS) gl[k] += dlogp * (d * d * invvar[k] - 1.0f);   // d log p / d log_std = (x - mu)^2 / var - 1
                }
        }
        float* dp = a.d_means + b * n * na;
        float* dl = nullptr;
        if constexpr (ROWS) dl = a.d_log_stds ? a.d_log_stds + b * n * na : nullptr;
        for (int i = 0; i < n; ++i)
#pragma unroll
            for (int k = 0; k < FLEXNET_MAX_ACT; ++k)
                if (k < na) {                                          // the sums over agents hand them to every agent
                    dp[i * na + k] = g[k];
                    if (dl) dl[i * na + k] = gl[k];
                }
    }
    flex_block_sum_f64<PPO_THREADS>(acc, reinterpret_cast<double*>(a.workspace) + PPO_WS_LOSS);
}

__global__ __launch_bounds__(PPO_THREADS) void ppo_policy_kernel(FlexPpoPolicyArgs a) { ppo_policy(a); }
__global__ __launch_bounds__(PPO_THREADS) void ppo_policy_rows_kernel(FlexPpoPolicyRowsArgs a) { ppo_policy(a); }

// the policy loss of both forms: the kernel, then the finish
template <class A, class K>
static int ppo_policy_launch(const A* a, K kernel, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(kernel, dim3(PPO_BLOCKS), dim3(PPO_THREADS), 0, s, *a);
    hipLaunchKernelGGL(ppo_loss_finish_kernel, dim3(1), dim3(64), 0, s, reinterpret_cast<const double*>(a->workspace) + PPO_WS_LOSS,
                       -1.0 / ((double)a->rows * a->n_agents), a->loss);
    return flex_launch_status();
}

extern "C" int flexnet_ppo_policy_loss(const FlexPpoPolicyArgs* a, void* stream) {
    if (!a || a->rows < 1 || a->n_agents < 1 || a->act_dim < 1 || !a->means || !a->log_std || !a->actions || !a->advantages ||
        !a->loss || !a->d_means || !a->workspace || a->workspace_floats < FLEXNET_PPO_WS_FLOATS ||
        !flex_aligned(a->workspace, 8))
        return FLEXNET_EINVAL;
    if (a->n_agents > FLEXNET_MAX_AGENTS || a->act_dim > FLEXNET_MAX_ACT) return FLEXNET_EUNSUPPORTED;
    return ppo_policy_launch(a, ppo_policy_kernel, stream);
}

extern "C" int flexnet_ppo_policy_loss_rows(const FlexPpoPolicyRowsArgs* a, void* stream) {
    if (!a || a->rows < 1 || a->n_agents < 1 || a->act_dim < 1 || !a->means || !a->log_stds || !a->actions || !a->advantages ||
        !a->loss || !a->d_means || !a->workspace || a->workspace_floats < FLEXNET_PPO_WS_FLOATS ||
        !flex_aligned(a->workspace, 8))
        return FLEXNET_EINVAL;
    if (a->n_agents > FLEXNET_MAX_AGENTS || a->act_dim > FLEXNET_MAX_ACT || a->rows >= ((int64_t)1 << 28))
        return FLEXNET_EUNSUPPORTED;
    return ppo_policy_launch(a, ppo_policy_rows_kernel, stream);
}

__global__ __launch_bounds__(PPO_THREADS) void ppo_value_kernel(FlexPpoValueArgs a) {
    const int n = a.n_agents;
    const int64_t total = a.rows * n;
    const float c2 = 2.0f * a.value_loss_coef / (float)total;
    double acc = 0.0;
    for (int64_t idx = (int64_t)blockIdx.x * PPO_THREADS + threadIdx.x; idx < total; idx += (int64_t)PPO_BLOCKS * PPO_THREADS) {
        const int64_t b = idx / n;
        const float v = a.values[idx], old = a.old_values[idx];
        const float ret = a.reward_norm[idx] + (a.gamma * (1.0f - a.done[b])) * a.next_values[idx];     // ppo.py:53
        const float d = v - old;
        const bool inside = d >= -a.eps_clip && d <= a.eps_clip;
        const float vc = old + ppo_clampf(d, -a.eps_clip, a.eps_clip);
        const float e1 = v - ret, e2 = vc - ret;
        const float s1 = e1 * e1, s2 = e2 * e2;
        acc += (double)ppo_maxf(s1, s2);
        // th.max: half the gradient to each argument at a tie; th.clamp: gradient inside [-eps, eps], ends included
        const float w1 = s1 > s2 ? 1.0f : (s1 == s2 ? 0.5f : 0.0f);
        const float w2 = (1.0f - w1) * (inside ? 1.0f : 0.0f);
        a.d_values[idx] = c2 * (w1 * e1 + w2 * e2);
        if (a.returns) a.returns[idx] = ret;
    }
    flex_block_sum_f64<PPO_THREADS>(acc, reinterpret_cast<double*>(a.workspace) + PPO_WS_LOSS);
}

extern "C" int flexnet_ppo_value_loss(const FlexPpoValueArgs* a, void* stream) {
    if (!a || a->rows < 1 || a->n_agents < 1 || !a->values || !a->old_values || !a->next_values || !a->reward_norm || !a->done ||
        !a->loss || !a->d_values || !a->workspace || a->workspace_floats < FLEXNET_PPO_WS_FLOATS ||
        !flex_aligned(a->workspace, 8))
        return FLEXNET_EINVAL;
    if (a->n_agents > FLEXNET_MAX_AGENTS) return FLEXNET_EUNSUPPORTED;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(ppo_value_kernel, dim3(PPO_BLOCKS), dim3(PPO_THREADS), 0, s, *a);
    hipLaunchKernelGGL(ppo_loss_finish_kernel, dim3(1), dim3(64), 0, s, reinterpret_cast<const double*>(a->workspace) + PPO_WS_LOSS,
                       (double)a->value_loss_coef / ((double)a->rows * a->n_agents), a->loss);
    return flex_launch_status();
}
