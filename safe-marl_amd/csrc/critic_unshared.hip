// critic_unshared.hip — the critics of `shared_params: False` (madrl/models/model.py:124-138: one MLPCritic per agent) for a
// whole batch in one launch per direction (gfx950).  Boundary: include/flexnet.h (FlexCriticUnsharedArgs /
// FlexCriticUnsharedBwdArgs).  Reference arithmetic: madrl/critics/mlp_critic.py:28-35 per agent on the input rows of
// maddpg.py:33-54, mappo.py:34-62, ippo.py:34-59 and iddpg.py:32-59.
//
// Work map and the stages shared with actor_unshared.hip and actor_mlp.hip: flex_agent_tile.h.  The backward's own stages — the LDS
// prologue, a head's dz2 and dx, the own-block product, the d_fc3_b fold — and the entry points' checks are shared with
// critic_unshared_twin.hip: critic_unshared_stages.h (which also says why the forward's head is not among them).  The weights
// are read where the modules keep them, through per-agent pointer tables.
//
// The first layer's input is never materialised: agent a's row of sample s is [x1 block | onehot(a) | x2 block], each block
// `base + s * pitch + a * agent_off` (agent_off 0: the block is shared by the sample's agents).  The id block is not read —
// agent a adds its own column w1 + a of its fc1.
//
// Forward: fc1 over the blocks + bias + id column -> z1 (saved), LayerNorm, ReLU -> x (saved), fc2, ReLU, fc3 -> q [b, n].
// Backward, from dq and the two saves: z2 = fc2(x) is RECOMPUTED (64 matrix-core steps per tile against a [rows, 64] tensor
// written and read back), dz2 and dz1 come out for the weight gradients (flexnet_wgrad_batched), dx = dz2 @ fc2_w on the
// matrix cores from an LDS copy of fc2_w, LayerNorm / ReLU backward (at_ln_relu_backward), and the optional own-block input
// gradient d_x2_own = dz1 @ fc1_w[a][:, own columns].  The per-agent [64] sums (d_ln_w, d_ln_b, d_fc1_b, d_fc2_b, d_fc3_w) and
// d_fc3_b are per-lane sums folded per work-group in a fixed order and summed over work-groups by a second launch: no
// atomics, bit-reproducible.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "critic_unshared_stages.h"

#define CU_VECS 6                                // d_ln_w | d_ln_b | d_fc1_b | d_fc2_b | d_fc3_w | d_fc3_b (element 0)
#define CU_PITCH (CU_VECS * SH)                  // a work-group's partial row

static_assert(FLEXNET_CRITIC_UNSHARED_WS_FLOATS >= FLEXNET_MAX_AGENTS * AT_MAX_BLOCKS * CU_PITCH, "workspace macro");

// (one kernel with or without the saves: the no-grad launch and the training forward give the same bits)
__global__ __launch_bounds__(64 * AT_W) void critic_unshared_forward_kernel(FlexCriticUnsharedArgs a) {
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
    const int ld1 = a.w1 + n_id + a.w2;
    const float* W1 = a.fc1_w[ag];
    const float* b1 = a.fc1_b[ag];

    tv16 x[2] = {zero_tile(), zero_tile()};
    at_fc1_block(x, a.x1 + s * a.x1_pitch + (int64_t)ag * a.x1_agent_off, W1 + (int64_t)i * ld1, W1 + (int64_t)(32 + i) * ld1,
                 a.w1, h);
    if (a.w2 > 0)
        at_fc1_block(x, a.x2 + s * a.x2_pitch + (int64_t)ag * a.x2_agent_off, W1 + (int64_t)i * ld1 + a.w1 + n_id,
                     W1 + (int64_t)(32 + i) * ld1 + a.w1 + n_id, a.w2, h);
    // + bias + the agent's own id column -> z1 (saved), LayerNorm, ReLU -> x (saved)
    at_add_bias_id(x, b1, a.agent_id ? W1 + a.w1 + ag : nullptr, ld1, h);
    if (SAVE) {
        store_tile(a.save_z1 + row * SH + 4 * h, x[0], ok);
        store_tile(a.save_z1 + row * SH + 32 + 4 * h, x[1], ok);
    }
    at_layernorm_relu(x, a.layernorm, a.ln_w[ag], a.ln_b[ag], a.ln_eps, h);
    if (SAVE) {
        store_tile(a.save_x + row * SH + 4 * h, x[0], ok);
        store_tile(a.save_x + row * SH + 32 + 4 * h, x[1], ok);
    }
    // fc2, ReLU, fc3: the lane sums its 32 units, the two halves of a row meet
    const float* W2 = a.fc2_w[ag];
    const float* b2 = a.fc2_b[ag];
    const float* w3 = a.fc3_w[ag];
    float p = 0.0f;
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        tv16 z2 = bias_tile(b2 + 32 * t, h);
        z2 = layer_tile(W2 + (int64_t)(32 * t + i) * SH + 4 * h, z2, x[0], x[1]);
#pragma unroll
        for (int r = 0; r < 16; ++r) p += w3[32 * t + TILE_U(r, h)] * fmaxf(z2[r], 0.0f);
    }
    const float q = (p + other_half(p)) + a.fc3_b[ag][0];
    if (ok && h == 0) a.q[row] = q;
}

// ---- backward ---------------------------------------------------------------------------------------------------------
// PG: with the parameter sums and dz2 (the value loss); without, only dz1 and d_x2_own come out (`critic_frozen`)
template <bool PG>
__global__ __launch_bounds__(64 * AT_W) void critic_unshared_backward_kernel(FlexCriticUnsharedBwdArgs a, int blocks_per_agent) {
    __shared__ __attribute__((aligned(16))) float s_lnw[SH], s_b2[SH], s_w3[SH];
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
    const int ld1 = a.w1 + n_id + a.w2;
    const int ow = a.d_x2_own ? a.own_w : 0;
    cu_stage_agent(s_buf, s_own, s_lnw, s_b2, s_w3, nullptr, a.fc1_w[ag],
                   a.fc1_w[ag] + a.w1 + n_id + a.own_first + (int64_t)ag * a.own_step, ld1, ow, a.layernorm, a.ln_w[ag],
                   a.fc2_w[ag], a.fc2_b[ag], a.fc3_w[ag], tid);

    tv16 acc_g[2], acc_b[2], acc_d[2], acc_b2[2], acc_w3[2];
    float acc_b3 = 0.0f;
    if (PG) cu_zero_sums(acc_g, acc_b, acc_d, acc_b2, acc_w3);
#pragma unroll 1
    for (int64_t tile = (int64_t)kb * AT_W + wave; tile < tiles; tile += (int64_t)blocks_per_agent * AT_W) {
        bool ok;
        const int64_t row = at_loop_sample(tile, i, batch, ok) * n + ag;
        const float dqv = ok ? a.dq[row] : 0.0f;               // a dead row's dq is zero: so is everything below

        const tv16 XS[2] = {load_tile(a.x + row * SH + 4 * h), load_tile(a.x + row * SH + 32 + 4 * h)};
        tv16 dz2[2], dx[2];
        cu_head_dz2<PG>(XS, dqv, s_buf, s_b2, s_w3, dz2, acc_w3, acc_b2, PG ? a.dz2 + row * SH : nullptr, i, h, ok);
        if (PG) acc_b3 += dqv;
        cu_head_dx(s_buf, dz2, dx, i, h);
        // LayerNorm / ReLU backward; ReLU's mask from the forward's own output
        tv16 dzv[2];
        at_ln_relu_backward<PG, false>(a.z1 + row * SH, nullptr, XS, nullptr, dx, s_lnw, a.layernorm, a.ln_eps, a.dz1 + row * SH,
                                       h, ok, acc_g, acc_b, acc_d, dzv);
        if (ow > 0) cu_own_block(s_own, dzv, a.d_x2_own + row * ow, ow, i, h, ok);
    }
    if (!PG) return;

    float* out = a.workspace + ((int64_t)ag * blocks_per_agent + kb) * CU_PITCH;
    __syncthreads();                                           // every wavefront is done with the fc2_w tile
    at_fold(fold, out, tid, acc_g, acc_b, acc_d, acc_b2, acc_w3);
    cu_fold_fc3_b(fold, out + 5 * SH, acc_b3, tid);
}

// the second launch: block = CU_VECS * agent + vector
__global__ __launch_bounds__(64 * FLEX_RED_G) void critic_unshared_reduce_kernel(FlexCriticUnsharedBwdArgs a, int blocks_per_agent) {
    int ag, vec, ex;
    float sum;
    if (!at_reduce_agent(a.workspace, CU_VECS, blocks_per_agent, ag, vec, ex, sum)) return;
    if (vec == 0) { if (a.layernorm) a.d_ln_w[ag * SH + ex] = sum; }
    else if (vec == 1) { if (a.layernorm) a.d_ln_b[ag * SH + ex] = sum; }
    else if (vec == 2) a.d_fc1_b[ag * SH + ex] = sum;
    else if (vec == 3) a.d_fc2_b[ag * SH + ex] = sum;
    else if (vec == 4) a.d_fc3_w[ag * SH + ex] = sum;
    else if (ex == 0) a.d_fc3_b[ag] = sum;
}

// ---- entry points: the checks are critic_unshared_stages.h's ---------------------------------------------------------------
extern "C" int flexnet_critic_unshared_forward(const FlexCriticUnsharedArgs* a, void* stream) {
    if (!a) return FLEXNET_EINVAL;
    const int rc = cu_check_forward(a);
    if (rc != FLEXNET_OK) return rc;
    if (a->rows == 0) return FLEXNET_OK;
    const int64_t groups = at_groups(a->rows / a->n_agents);
    hipLaunchKernelGGL(critic_unshared_forward_kernel, dim3((unsigned)(groups * a->n_agents)), dim3(64 * AT_W), 0,
                       (hipStream_t)stream, *a);
    return flex_launch_status();
}

extern "C" int flexnet_critic_unshared_backward(const FlexCriticUnsharedBwdArgs* a, void* stream) {
    if (!a) return FLEXNET_EINVAL;
    const int rc = cu_check_backward(a, a->dz1);
    if (rc != FLEXNET_OK) return rc;
    if (a->rows == 0) return FLEXNET_OK;
    const bool pg = a->param_grads != 0;
    const int64_t bpa = at_blocks_per_agent(a->rows / a->n_agents);
    if (pg && bpa * a->n_agents * CU_PITCH > a->workspace_floats) return FLEXNET_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)(bpa * a->n_agents)), block(64 * AT_W);
    if (pg) {
        hipLaunchKernelGGL(critic_unshared_backward_kernel<true>, grid, block, 0, s, *a, (int)bpa);
        hipLaunchKernelGGL(critic_unshared_reduce_kernel, dim3(CU_VECS * a->n_agents), dim3(64 * FLEX_RED_G), 0, s, *a, (int)bpa);
    } else {
        hipLaunchKernelGGL(critic_unshared_backward_kernel<false>, grid, block, 0, s, *a, (int)bpa);
    }
    return flex_launch_status();
}
