// critic_unshared_twin.hip — MATD3's twin critics under `shared_params: False` (madrl/models/matd3.py:24-27: one MLPCritic of
// (o + a) n + n + 1 columns per agent; matd3.py:74-82: agent i's critic twice on its row, the trailing twin flag at 0 and at 1)
// for a whole batch in one launch per direction (gfx950).  Boundary: include/flexnet.h (FlexCriticUnsharedTwinArgs /
// FlexCriticUnsharedTwinBwdArgs).  Reference arithmetic: madrl/critics/mlp_critic.py:28-35 per agent and head.
//
// Work map and stages: flex_agent_tile.h, as critic_unshared.hip uses them — a wavefront per 32 samples of ONE agent, the weights
// read where the modules keep them through per-agent pointer tables, the first layer's input described by blocks.  The backward's
// stages of a head and the entry points' checks are the ones critic_unshared.hip runs: critic_unshared_stages.h.  What is new
// is the flag column: every fc1.weight is [64, w1 + n_id + w2 + 1], and the first layer — the block products, the bias and the
// agent's own id column, where critic_unshared.hip spends its time — is formed ONCE per row.  That is head 0's pre-activation
// z1; head 1's is z1 + fc1_w[a][:, last].  The rest runs per head.
//
// Forward: z1 (saved once), then per head LayerNorm, ReLU -> x (saved per head), fc2, ReLU, fc3 -> q [heads, b, n] — the memory
// of the reference's cat([values1, values2], 0).  The kernel is compiled per head count with the head loop unrolled (left
// as a loop it held 318 registers, one wavefront per SIMD; unrolled, two); head 0 runs the same operations in the same
// order in both, and no fp32 operation is reassociated: its bits are a one-head launch's.
// Backward, from dq [heads, b, n] and the saves, per head: z2 = fc2(x) is RECOMPUTED, dz2 (stored for the weight gradient),
// dx = dz2 @ fc2_w from the LDS copy of fc2_w, LayerNorm / ReLU backward (at_ln_relu_backward; head 1 adds the flag column back
// to z1 through its `s_add`) -> that head's dz1.  Out: dz1_sum = head 0's dz1 + head 1's — fc1's weight and input gradients are
// linear in it and are taken once; d_flag, the sum of head 1's dz1 over the agent's rows, is the flag column of d_fc1_w[a]; the
// optional own-block input gradient comes from head 0's dz1 only (matd3.py:123-125: the policy loss reads the first head).  The
// per-agent [64] sums and d_fc3_b are per-lane sums folded per work-group in a fixed order and summed over work-groups by a
// second launch: no atomics, bit-reproducible.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "critic_unshared_stages.h"

#define CT_VECS 7                                // d_ln_w | d_ln_b | d_fc1_b | d_fc2_b | d_fc3_w | d_flag | d_fc3_b (element 0)
#define CT_PITCH (CT_VECS * SH)                  // a work-group's partial row

static_assert(FLEXNET_CRITIC_UNSHARED_TWIN_WS_FLOATS >= FLEXNET_MAX_AGENTS * AT_MAX_BLOCKS * CT_PITCH, "workspace macro");

// (The kernels' names begin with twin_: build.kernel_resources filters on a name's beginning, and "critic_unshared" is
// critic_unshared.hip's four.)
// one kernel with or without the saves: the no-grad launch and the training forward give the same bits
template <int HEADS>
__global__ __launch_bounds__(64 * AT_W) void twin_critic_unshared_forward_kernel(FlexCriticUnsharedTwinArgs a) {
    const bool SAVE = a.save_z1 != nullptr;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, i = lane & 31, h = lane >> 5;
    const int n = a.n_agents;
    const int ag = blockIdx.x % n;
    const int64_t batch = a.rows / n;
    const int64_t s0 = ((int64_t)(blockIdx.x / n) * AT_W + wave) * 32;
    if (s0 >= batch) return;                                   // (the kernel has no barrier)
    const bool ok = s0 + i < batch;
    const int64_t s = ok ? s0 + i : batch - 1;                 // the last partial tile re-reads a valid sample
    const int64_t row = s * n + ag;
    const int n_id = a.agent_id ? n : 0;
    const int ld1 = a.w1 + n_id + a.w2 + 1;                    // ... | the twin flag's column
    const float* W1 = a.fc1_w[ag];

    // which blocks take the wide loads: uniform over the work-group (the agent's offsets and weights)
    const float* x1b = a.x1 + (int64_t)ag * a.x1_agent_off;
    const float* x2b = a.x2 + (int64_t)ag * a.x2_agent_off;
    const bool wrows = at_aligned(W1, 8) && (ld1 & 1) == 0;
    const bool xv1 = at_aligned(x1b, 16) && (a.x1_pitch & 3) == 0;
    const bool xv2 = a.w2 > 0 && at_aligned(x2b, 16) && (a.x2_pitch & 3) == 0;
    const bool wv2 = wrows && ((a.w1 + n_id) & 1) == 0;

    tv16 z[2] = {zero_tile(), zero_tile()};
    at_fc1_block_wide(z, x1b + s * a.x1_pitch, W1 + (int64_t)i * ld1, W1 + (int64_t)(32 + i) * ld1, a.w1, h, xv1, wrows);
    if (a.w2 > 0)
        at_fc1_block_wide(z, x2b + s * a.x2_pitch, W1 + (int64_t)i * ld1 + a.w1 + n_id, W1 + (int64_t)(32 + i) * ld1 + a.w1 + n_id,
                          a.w2, h, xv2, wv2);
    // + bias + the agent's own id column -> z1 (saved once: head 0's pre-activation)
    at_add_bias_id(z, a.fc1_b[ag], a.agent_id ? W1 + a.w1 + ag : nullptr, ld1, h);
    if (SAVE) {
        store_tile(a.save_z1 + row * SH + 4 * h, z[0], ok);
        store_tile(a.save_z1 + row * SH + 32 + 4 * h, z[1], ok);
    }
    const float* W2 = a.fc2_w[ag];
    const float* b2 = a.fc2_b[ag];
    const float* w3 = a.fc3_w[ag];
    const float* flag = W1 + (ld1 - 1);
#pragma unroll
    for (int hd = 0; hd < HEADS; ++hd) {
        const int64_t hrow = (int64_t)hd * a.rows + row;
        tv16 x[2] = {z[0], z[1]};
        if (hd == 1) {                                         // the flag input is 1: + its column
#pragma unroll
            for (int t = 0; t < 2; ++t) {
#pragma unroll
                for (int r = 0; r < 16; ++r) x[t][r] += flag[(int64_t)(32 * t + TILE_U(r, h)) * ld1];
            }
        }
        at_layernorm_relu(x, a.layernorm, a.ln_w[ag], a.ln_b[ag], a.ln_eps, h);
        if (SAVE) {
            store_tile(a.save_x + hrow * SH + 4 * h, x[0], ok);
            store_tile(a.save_x + hrow * SH + 32 + 4 * h, x[1], ok);
        }
        // fc2, ReLU, fc3: the lane sums its 32 units, the two halves of a row meet
        float p = 0.0f;
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            tv16 z2 = bias_tile(b2 + 32 * t, h);
            z2 = layer_tile(W2 + (int64_t)(32 * t + i) * SH + 4 * h, z2, x[0], x[1]);
#pragma unroll
            for (int r = 0; r < 16; ++r) p += w3[32 * t + TILE_U(r, h)] * fmaxf(z2[r], 0.0f);
        }
        const float q = (p + other_half(p)) + a.fc3_b[ag][0];
        if (ok && h == 0) a.q[hrow] = q;
    }
}

// ---- backward ---------------------------------------------------------------------------------------------------------
// PG: with the parameter sums and dz2 (the value loss); without, only dz1_sum and d_x2_own come out (`critic_frozen`)
template <bool PG>
__global__ __launch_bounds__(64 * AT_W) void twin_critic_unshared_backward_kernel(FlexCriticUnsharedTwinBwdArgs a,
                                                                                  int blocks_per_agent) {
    __shared__ __attribute__((aligned(16))) float s_lnw[SH], s_b2[SH], s_w3[SH], s_flag[SH];
    __shared__ __attribute__((aligned(16))) float s_own[SH * FLEXNET_MAX_ACT];
    // fc2_w of the agent (rows for z2, columns for dx); after the tile loop the same memory is the fold buffer
    __shared__ __attribute__((aligned(16))) float s_buf[AT_W * 64 * AT_FOLD];
    static_assert(SH * AT_WP <= AT_W * 64 * AT_FOLD, "the fc2_w tile lives in the fold buffer");
    float (*fold)[64][AT_FOLD] = reinterpret_cast<float (*)[64][AT_FOLD]>(s_buf);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, i = lane & 31, h = lane >> 5;
    const int n = a.n_agents;
    const int ag = blockIdx.x % n, kb = blockIdx.x / n;
    const int64_t batch = a.rows / n;
    const int64_t tiles = (batch + 31) / 32;
    const int n_id = a.agent_id ? n : 0;
    const int ld1 = a.w1 + n_id + a.w2 + 1;
    const int ow = a.d_x2_own ? a.own_w : 0;
    cu_stage_agent(s_buf, s_own, s_lnw, s_b2, s_w3, s_flag, a.fc1_w[ag],
                   a.fc1_w[ag] + a.w1 + n_id + a.own_first + (int64_t)ag * a.own_step, ld1, ow, a.layernorm, a.ln_w[ag],
                   a.fc2_w[ag], a.fc2_b[ag], a.fc3_w[ag], tid);

    tv16 acc_g[2], acc_b[2], acc_d[2], acc_b2[2], acc_w3[2], acc_f[2];
    float acc_b3 = 0.0f;
    if (PG) cu_zero_sums(acc_g, acc_b, acc_d, acc_b2, acc_w3, acc_f);
#pragma unroll 1
    for (int64_t tile = (int64_t)kb * AT_W + wave; tile < tiles; tile += (int64_t)blocks_per_agent * AT_W) {
        bool ok;
        const int64_t row = at_loop_sample(tile, i, batch, ok) * n + ag;
        tv16 dsum[2] = {zero_tile(), zero_tile()};             // head 0's dz1, then + head 1's
#pragma unroll 1
        for (int hd = 0; hd < a.heads; ++hd) {
            __asm__ volatile("" ::: "memory");                 // (as at_loop_sample, for the head loop's invariant LDS reads)
            const int64_t hrow = (int64_t)hd * a.rows + row;
            const float dqv = ok ? a.dq[hrow] : 0.0f;          // a dead row's dq is zero: so is everything below

            const tv16 XS[2] = {load_tile(a.x + hrow * SH + 4 * h), load_tile(a.x + hrow * SH + 32 + 4 * h)};
            tv16 dz2[2], dx[2];
            cu_head_dz2<PG>(XS, dqv, s_buf, s_b2, s_w3, dz2, acc_w3, acc_b2, PG ? a.dz2 + hrow * SH : nullptr, i, h, ok);
            if (PG) acc_b3 += dqv;
            cu_head_dx(s_buf, dz2, dx, i, h);
            // LayerNorm / ReLU backward; ReLU's mask from the forward's own output.  Head 1's pre-activation is z1 + the flag
            // column (`s_add`).  The stage's own store is off (its `ok` false): dz1_sum is stored once, below.
            tv16 dzv[2];
            at_ln_relu_backward<PG, false>(a.z1 + row * SH, hd ? s_flag : nullptr, XS, nullptr, dx, s_lnw, a.layernorm, a.ln_eps,
                                           a.dz1_sum + row * SH, h, false, acc_g, acc_b, acc_d, dzv);
#pragma unroll
            for (int t = 0; t < 2; ++t) {
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    dsum[t][e] += dzv[t][e];
                    if (PG && hd == 1) acc_f[t][e] += dzv[t][e];
                }
            }
            // the own-action gradient is head 0's dz1 alone
            if (ow > 0 && hd == 0) cu_own_block(s_own, dzv, a.d_x2_own + row * ow, ow, i, h, ok);
        }
        store_tile(a.dz1_sum + row * SH + 4 * h, dsum[0], ok);
        store_tile(a.dz1_sum + row * SH + 32 + 4 * h, dsum[1], ok);
    }
    if (!PG) return;

    float* out = a.workspace + ((int64_t)ag * blocks_per_agent + kb) * CT_PITCH;
    __syncthreads();                                           // every wavefront is done with the fc2_w tile
    at_fold(fold, out, tid, acc_g, acc_b, acc_d, acc_b2, acc_w3, acc_f);
    cu_fold_fc3_b(fold, out + 6 * SH, acc_b3, tid);
}

// the second launch: block = CT_VECS * agent + vector
__global__ __launch_bounds__(64 * FLEX_RED_G) void twin_critic_unshared_reduce_kernel(FlexCriticUnsharedTwinBwdArgs a,
                                                                                      int blocks_per_agent) {
    int ag, vec, ex;
    float sum;
    if (!at_reduce_agent(a.workspace, CT_VECS, blocks_per_agent, ag, vec, ex, sum)) return;
    if (vec == 0) { if (a.layernorm) a.d_ln_w[ag * SH + ex] = sum; }
    else if (vec == 1) { if (a.layernorm) a.d_ln_b[ag * SH + ex] = sum; }
    else if (vec == 2) a.d_fc1_b[ag * SH + ex] = sum;
    else if (vec == 3) a.d_fc2_b[ag * SH + ex] = sum;
    else if (vec == 4) a.d_fc3_w[ag * SH + ex] = sum;
    else if (vec == 5) a.d_flag[ag * SH + ex] = sum;
    else if (ex == 0) a.d_fc3_b[ag] = sum;
}

// ---- entry points: the checks are critic_unshared_stages.h's ---------------------------------------------------------------
extern "C" int flexnet_critic_unshared_twin_forward(const FlexCriticUnsharedTwinArgs* a, void* stream) {
    if (!a) return FLEXNET_EINVAL;
    const int rc = cu_check_forward(a, a->heads);
    if (rc != FLEXNET_OK) return rc;
    if (a->rows == 0) return FLEXNET_OK;
    const int64_t groups = at_groups(a->rows / a->n_agents);
    const dim3 grid((unsigned)(groups * a->n_agents)), block(64 * AT_W);
    if (a->heads == 2) hipLaunchKernelGGL(twin_critic_unshared_forward_kernel<2>, grid, block, 0, (hipStream_t)stream, *a);
    else hipLaunchKernelGGL(twin_critic_unshared_forward_kernel<1>, grid, block, 0, (hipStream_t)stream, *a);
    return flex_launch_status();
}

extern "C" int flexnet_critic_unshared_twin_backward(const FlexCriticUnsharedTwinBwdArgs* a, void* stream) {
    if (!a) return FLEXNET_EINVAL;
    const int rc = cu_check_backward(a, a->dz1_sum, a->d_flag != nullptr, a->heads);
    if (rc != FLEXNET_OK) return rc;
    if (a->rows == 0) return FLEXNET_OK;
    const bool pg = a->param_grads != 0;
    const int64_t bpa = at_blocks_per_agent(a->rows / a->n_agents);
    if (pg && bpa * a->n_agents * CT_PITCH > a->workspace_floats) return FLEXNET_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)(bpa * a->n_agents)), block(64 * AT_W);
    if (pg) {
        hipLaunchKernelGGL(twin_critic_unshared_backward_kernel<true>, grid, block, 0, s, *a, (int)bpa);
        hipLaunchKernelGGL(twin_critic_unshared_reduce_kernel, dim3(CT_VECS * a->n_agents), dim3(64 * FLEX_RED_G), 0, s, *a,
                           (int)bpa);
    } else {
        hipLaunchKernelGGL(twin_critic_unshared_backward_kernel<false>, grid, block, 0, s, *a, (int)bpa);
    }
    return flex_launch_status();
}
