// gauss.hip — the learned log-std head of the Gaussian actors and what consumes per-row standard deviations (gfx950).
// Boundary: include/flexnet.h (flexnet_gauss_*).
//
// madrl/agents/{rnn,mlp}_agent_gaussian.py: log_std = MIN + 0.5 (MAX - MIN) (tanh(W h + b) + 1) on the actor's hidden state
// h [rows, 64], W [a, 64] with a <= 8.
//   head forward:   reads h ONCE (16-byte loads) in the 32-rows-per-wavefront layout of flex_mfma_tile.h: lane (row i, half
//                   hf) holds 32 of its row's 64 units, the a dot products are VALU chains over those 32 and one exchange
//                   with the other half; the 2 KB of weights are two addresses per wavefront load (L1).  Half 0 stores
//                   log_std and t = tanh(u); half 1 runs the optional exploration epilogue of maddpg.py:88 under
//                   util.py:56-64, action = tanh(mean + exp(log_std) noise), and translate_action (util.py:125-128).
//                   HBM-bound at update size: 42 MB of h at 163 840 rows.
//   head backward:  d_u = d_log_std 0.5 (MAX - MIN) (1 - t^2);  d_h = d_u W in the same layout (16-byte stores).  dW / db
//                   are flexnet_wgrad(d_u, h) with its column sums.
//   per-agent heads: head forward / backward with the weights of agent r % n for row r (shared_params: False), on the actors'
//                   work map — a wavefront owns 32 rows of one agent — so that the weights stay uniform per wavefront;
//                   eager calls only, like the actors they follow.  The SAME two bodies as the shared
//                   head's (templates over the argument struct), without the exploration epilogue.
//   sum explore:    the agent-summed selection of iddpg.py:64-70 / matd3.py:91-98 with per-sample log-stds, one thread per
//                   (environment, action component), every fp32 rounding where the tensor composition has it.
// (PPO's policy loss on per-row log-stds, flexnet_ppo_policy_loss_rows, is an instantiation of ppo.hip's one body and lives there.)
// No LDS, no scratch, no atomics: the same inputs give the same bits.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>
#include "flexnet.h"
#include "flex_launch.h"
#include "flex_mfma_tile.h"
#include "flex_nan.h"
#include "agent_sum.h"

#define GAUSS_THREADS 256
#define GAUSS_ROWS (GAUSS_THREADS / 2)       // 32 rows per wavefront
#define GAUSS_MAX_ROWS ((int64_t)1 << 30)

// (gauss_env_action — translate_action, util.py:125-128 — and the agent-summed selection live in agent_sum.h: the rollout burst
//  of csrc/flexenv.hip runs the same bodies)

// ---- the head, both ways: ONE body each, a template over the argument struct (A = FlexGaussHeadArgs or, shared_params: False,
// FlexGaussHeadUnsharedArgs).  The forms differ in the row map, in where W and b come from and in the exploration epilogue,
// which only the shared form has; per row the arithmetic — and so the bits — are the same code.
struct GaussRow { int64_t row; bool ok; int ag; };

// shared weights: consecutive rows, 32 per wavefront
__device__ __forceinline__ GaussRow gauss_row(const FlexGaussHeadArgs& a, int i) {
    const int64_t row = (int64_t)blockIdx.x * GAUSS_ROWS + (threadIdx.x >> 6) * 32 + i;
    return {row, row < a.rows, 0};
}
// per-agent weights, the actors' work map: a wavefront owns 32 samples of ONE agent (rows s * n + ag), a work-group is four
// wavefronts of agent blockIdx.x % n, so W and b are one uniform pointer per work-group out of the tables
__device__ __forceinline__ GaussRow gauss_row(const FlexGaussHeadUnsharedArgs& a, int i) {
    const int n = a.n_agents, ag = blockIdx.x % n;
    const int64_t s = ((int64_t)(blockIdx.x / n) * (GAUSS_THREADS / 64) + (threadIdx.x >> 6)) * 32 + i;
    return {s * n + ag, s < a.rows / n, ag};
}
__device__ __forceinline__ const float* gauss_pick(const float* p, int) { return p; }
__device__ __forceinline__ const float* gauss_pick(const float* const (&p)[FLEXNET_MAX_AGENTS], int ag) { return p[ag]; }

template <class A>
__device__ __forceinline__ void gauss_head_forward(const A& a) {
    const int lane = threadIdx.x & 63, i = lane & 31, hf = lane >> 5;
    const GaussRow m = gauss_row(a, i);
    const int64_t row = m.row;
    const bool ok = m.ok;
    const int na = a.act_dim;
    const float* W = gauss_pick(a.w, m.ag);
    const float* B = gauss_pick(a.b, m.ag);
    tv16 x0, x1;
#pragma unroll
    for (int r = 0; r < 16; ++r) { x0[r] = 0.0f; x1[r] = 0.0f; }
    if (ok) {
        const float* hr = a.h + row * SH + 4 * hf;
        x0 = load_tile(hr);
        x1 = load_tile(hr + 32);
    }
    const float half_span = 0.5f * (a.log_std_max - a.log_std_min);
    float ls[FLEXNET_MAX_ACT], t[FLEXNET_MAX_ACT];
#pragma unroll
    for (int k = 0; k < FLEXNET_MAX_ACT; ++k) {
        ls[k] = 0.0f; t[k] = 0.0f;
        if (k < na) {                                   // (the same for every lane: the exchange below is wavefront-wide)
            const float* wr = W + k * SH + 4 * hf;
            float p0 = 0.0f, p1 = 0.0f;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const tv4 w0 = ld4(wr + 8 * q), w1 = ld4(wr + 32 + 8 * q);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    p0 = fmaf(x0[4 * q + j], w0[j], p0);
                    p1 = fmaf(x1[4 * q + j], w1[j], p1);
                }
            }
            const float p = p0 + p1;
            float u = p + other_half(p);                // (an fp32 add commutes: both halves hold the same bits)
            if (B) u += B[k];
            t[k] = tanhf(u);
            ls[k] = a.log_std_min + half_span * (t[k] + 1.0f);
        }
    }
    if (!ok) return;
    if (hf == 0) {
        float* lo = a.log_std + row * na;
#pragma unroll
        for (int k = 0; k < FLEXNET_MAX_ACT; ++k)
            if (k < na) lo[k] = ls[k];
        if (a.t) {
            float* to = a.t + row * na;
#pragma unroll
            for (int k = 0; k < FLEXNET_MAX_ACT; ++k)
                if (k < na) to[k] = t[k];
        }
    } else if constexpr (std::is_same_v<A, FlexGaussHeadArgs>) {      // the exploration epilogue: the shared form's alone
        if (!a.action) return;
        const float* mp = a.means + row * na;
        const float* np_ = a.noise + row * na;
        float* ao = a.action + row * na;
#pragma unroll
        for (int k = 0; k < FLEXNET_MAX_ACT; ++k)
            if (k < na) {
                const float y = tanhf(__fadd_rn(mp[k], __fmul_rn(np_[k], expf(ls[k]))));      // tanh(loc + eps * scale)
                ao[k] = y;
                if (a.env_action) a.env_action[row * na + k] = gauss_env_action(y, a.action_low, a.action_high);
            }
    }
}

template <class A>
__device__ __forceinline__ void gauss_head_backward(const A& a) {
    const int lane = threadIdx.x & 63, i = lane & 31, hf = lane >> 5;
    const GaussRow m = gauss_row(a, i);
    if (!m.ok) return;                                  // (no exchange between lanes in this kernel)
    const int64_t row = m.row;
    const int na = a.act_dim;
    const float* W = gauss_pick(a.w, m.ag);
    const float half_span = 0.5f * (a.log_std_max - a.log_std_min);
    float du[FLEXNET_MAX_ACT];
#pragma unroll
    for (int k = 0; k < FLEXNET_MAX_ACT; ++k) {
        du[k] = 0.0f;
        if (k < na) {
            const float tt = a.t[row * na + k];
            du[k] = a.d_log_std[row * na + k] * (half_span * (1.0f - tt * tt));
        }
    }
    if (hf == 0 && a.d_u) {
#pragma unroll
        for (int k = 0; k < FLEXNET_MAX_ACT; ++k)
            if (k < na) a.d_u[row * na + k] = du[k];
    }
    if (!a.d_h) return;
    // The lane's two tiles one after the other (per element the same chain of FMAs over k, so the same bits): with both sets of
    // accumulators live the body, inlined into its kernels, takes 82 VGPRs and 5 waves per SIMD where the kernels had 7.
    float* dr = a.d_h + row * SH + 4 * hf;
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        tv16 g;
#pragma unroll
        for (int r = 0; r < 16; ++r) g[r] = 0.0f;
#pragma unroll
        for (int k = 0; k < FLEXNET_MAX_ACT; ++k)
            if (k < na) {
                const float* wr = W + k * SH + 4 * hf + 32 * t;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const tv4 w = ld4(wr + 8 * q);
#pragma unroll
                    for (int j = 0; j < 4; ++j) g[4 * q + j] = fmaf(du[k], w[j], g[4 * q + j]);
                }
            }
        store_tile(dr + 32 * t, g, true);
    }
}

__global__ __launch_bounds__(GAUSS_THREADS) void gauss_head_forward_kernel(FlexGaussHeadArgs a) { gauss_head_forward(a); }
__global__ __launch_bounds__(GAUSS_THREADS) void gauss_head_backward_kernel(FlexGaussHeadArgs a) { gauss_head_backward(a); }
__global__ __launch_bounds__(GAUSS_THREADS) void gauss_head_unshared_forward_kernel(FlexGaussHeadUnsharedArgs a) {
    gauss_head_forward(a);
}
__global__ __launch_bounds__(GAUSS_THREADS) void gauss_head_unshared_backward_kernel(FlexGaussHeadUnsharedArgs a) {
    gauss_head_backward(a);
}

static int gauss_head_check(const FlexGaussHeadArgs* a) {
    if (!a || a->rows < 0 || a->act_dim < 1 || !a->w) return FLEXNET_EINVAL;
    if (a->hid != FLEXNET_HID || a->act_dim > FLEXNET_MAX_ACT || a->rows > GAUSS_MAX_ROWS || !flex_aligned(a->w, 16))
        return FLEXNET_EUNSUPPORTED;
    return FLEXNET_OK;
}

extern "C" int flexnet_gauss_head_forward(const FlexGaussHeadArgs* a, void* stream) {
    const int rc = gauss_head_check(a);
    if (rc != FLEXNET_OK) return rc;
    const bool explore = a->means || a->noise || a->action || a->env_action;
    if (!a->h || !a->log_std || (explore && !(a->means && a->noise && a->action)) ||
        (a->env_action && !(a->action_high >= a->action_low)))
        return FLEXNET_EINVAL;
    if (!flex_aligned(a->h, 16)) return FLEXNET_EUNSUPPORTED;
    if (a->rows == 0) return FLEXNET_OK;
    const unsigned blocks = (unsigned)((a->rows + GAUSS_ROWS - 1) / GAUSS_ROWS);
    hipLaunchKernelGGL(gauss_head_forward_kernel, dim3(blocks), dim3(GAUSS_THREADS), 0, (hipStream_t)stream, *a);
    return flex_launch_status();
}

extern "C" int flexnet_gauss_head_backward(const FlexGaussHeadArgs* a, void* stream) {
    const int rc = gauss_head_check(a);
    if (rc != FLEXNET_OK) return rc;
    if (!a->d_log_std || !a->t || !(a->d_u || a->d_h)) return FLEXNET_EINVAL;
    if (a->d_h && !flex_aligned(a->d_h, 16)) return FLEXNET_EUNSUPPORTED;
    if (a->rows == 0) return FLEXNET_OK;
    const unsigned blocks = (unsigned)((a->rows + GAUSS_ROWS - 1) / GAUSS_ROWS);
    hipLaunchKernelGGL(gauss_head_backward_kernel, dim3(blocks), dim3(GAUSS_THREADS), 0, (hipStream_t)stream, *a);
    return flex_launch_status();
}

// ---- shared_params: False: every agent's own head (FlexGaussHeadUnsharedArgs) ------------------------------------------------
static int gauss_head_unshared_check(const FlexGaussHeadUnsharedArgs* a) {
    if (!a || a->rows < 0 || a->act_dim < 1 || a->n_agents < 1) return FLEXNET_EINVAL;
    if (a->hid != FLEXNET_HID || a->act_dim > FLEXNET_MAX_ACT || a->n_agents > FLEXNET_MAX_AGENTS || a->rows > GAUSS_MAX_ROWS)
        return FLEXNET_EUNSUPPORTED;
    if (a->rows % a->n_agents != 0) return FLEXNET_EINVAL;
    bool aligned = true;
    for (int k = 0; k < a->n_agents; ++k) {
        if (!a->w[k] || ((a->b[k] != nullptr) != (a->b[0] != nullptr))) return FLEXNET_EINVAL;
        aligned = aligned && flex_aligned(a->w[k], 16);
    }
    return aligned ? FLEXNET_OK : FLEXNET_EUNSUPPORTED;
}

static unsigned gauss_head_unshared_grid(const FlexGaussHeadUnsharedArgs* a) {
    const int64_t batch = a->rows / a->n_agents;
    return (unsigned)(((batch + GAUSS_ROWS - 1) / GAUSS_ROWS) * a->n_agents);
}

extern "C" int flexnet_gauss_head_unshared_forward(const FlexGaussHeadUnsharedArgs* a, void* stream) {
    const int rc = gauss_head_unshared_check(a);
    if (rc != FLEXNET_OK) return rc;
    if (!a->h || !a->log_std) return FLEXNET_EINVAL;
    if (!flex_aligned(a->h, 16)) return FLEXNET_EUNSUPPORTED;
    if (a->rows == 0) return FLEXNET_OK;
    hipLaunchKernelGGL(gauss_head_unshared_forward_kernel, dim3(gauss_head_unshared_grid(a)), dim3(GAUSS_THREADS), 0,
                       (hipStream_t)stream, *a);
    return flex_launch_status();
}

extern "C" int flexnet_gauss_head_unshared_backward(const FlexGaussHeadUnsharedArgs* a, void* stream) {
    const int rc = gauss_head_unshared_check(a);
    if (rc != FLEXNET_OK) return rc;
    if (!a->d_log_std || !a->t || !(a->d_u || a->d_h)) return FLEXNET_EINVAL;
    if (a->d_h && !flex_aligned(a->d_h, 16)) return FLEXNET_EUNSUPPORTED;
    if (a->rows == 0) return FLEXNET_OK;
    hipLaunchKernelGGL(gauss_head_unshared_backward_kernel, dim3(gauss_head_unshared_grid(a)), dim3(GAUSS_THREADS), 0,
                       (hipStream_t)stream, *a);
    return flex_launch_status();
}

// ---- agent-summed exploration with per-sample log-stds: one thread per (environment, action component) ------------------
__global__ __launch_bounds__(256) void gauss_sum_explore_kernel(FlexGaussSumArgs a) {
    const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;          // (64-bit: the last block of a grid near 2^31)
    if (tid >= (int64_t)a.n_envs * a.act_dim) return;
    const int n = a.n_agents, ad = a.act_dim;
    const int64_t e = tid / ad;
    const int k = (int)(tid - e * ad);
    const int64_t at = e * n * ad + k;
    gauss_sum_select(a.means + at, a.log_stds + at, n, ad, a.eps[tid], a.act_low, a.act_high, a.action + at,
                     a.env_action ? a.env_action + at : nullptr);
}

extern "C" int flexnet_gauss_sum_explore(const FlexGaussSumArgs* a, void* stream) {
    if (!a || a->n_envs < 0 || a->n_agents < 1 || a->act_dim < 1 || !a->means || !a->log_stds || !a->eps || !a->action ||
        !(a->act_high >= a->act_low))
        return FLEXNET_EINVAL;
    if (a->n_agents > FLEXNET_MAX_AGENTS || a->act_dim > FLEXNET_MAX_ACT) return FLEXNET_EUNSUPPORTED;
    if (a->n_envs == 0) return FLEXNET_OK;
    const int64_t tot = (int64_t)a->n_envs * a->act_dim;
    if (tot > 0x7fffffff) return FLEXNET_EUNSUPPORTED;
    hipLaunchKernelGGL(gauss_sum_explore_kernel, dim3((int)((tot + 255) / 256)), dim3(256), 0, (hipStream_t)stream, *a);
    return flex_launch_status();
}
