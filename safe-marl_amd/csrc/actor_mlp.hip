// actor_mlp.hip — the MLP actor of `agent_type: mlp` (madrl/agents/mlp_agent.py:20-32, mlp_agent_gaussian.py: fc1 -> LayerNorm ->
// ReLU -> fc2 -> ReLU = h -> fc3) for a whole batch in one launch per direction (gfx950), in both of its forms: ONE set of
// weights under `shared_params: True` (FlexActorMlpArgs / FlexActorMlpBwdArgs) and one MLPAgent / MLPAgentGaussian per agent
// under `shared_params: False` (madrl/models/model.py:124-138; FlexActorMlpUnsharedArgs / FlexActorMlpUnsharedBwdArgs).
// Boundary: include/flexnet.h.  The entry points are for eager calls: the host side never launches them on a capturing stream
// (nets.mlp_actor_allowed).
//
// Work map and the stages shared with actor_unshared.hip and critic_unshared.hip: flex_agent_tile.h.
// The forward and the backward are ONE body each, a template over the argument struct: the two forms differ only in where a
// weight pointer comes from, and am_pick hides that.  With one set of weights the agent only picks the id column of fc1 and the
// row of the per-agent sums.  With per-agent weights every parameter is a table of the modules' own tensors (as in
// actor_unshared.hip; no stacked copy), read through one uniform pointer per work-group, and under agent_id agent a adds only
// its own column obs_dim + a of its fc1_w[a].
//
// Forward: fc1 over the observation columns (read where the caller keeps them, [b, n, obs_dim] without id columns, clamped
// scalar loads) + bias + the agent's id column -> z1 (saved), LayerNorm, ReLU -> x (saved), fc2, ReLU -> h (always written),
// fc3 with the A operand's rows past act_dim zero -> means [rows, act_dim].
// Backward, from d_means, the optional d_h and the three saves: dh = d_means @ fc3_w (+ d_h) on the matrix cores (K = 8: one
// group of four steps per tile), dz2 = dh [h > 0], dx = dz2 @ fc2_w from an LDS copy of fc2_w, LayerNorm / ReLU backward as
// csrc/lnrelu.hip -> dz1.  The [64] sums and d_fc3_b are per-lane sums over one agent's rows, folded per work-group in a fixed
// order and summed over work-groups by a second launch: no atomics, bit-reproducible.  That second launch is where the two
// forms part.  One set of weights sums d_ln_w, d_ln_b, d_fc1_b, d_fc2_b and d_fc3_b over EVERY agent's work-groups and adds
// the per-agent sums of dz1; per-agent weights sum each vector over ONE agent's work-groups into [n, 64] / [n, act_dim].
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "flexnet.h"
#include "flex_launch.h"
#include "flex_agent_tile.h"

#define AM_VECS 5                                // d_ln_w | d_ln_b | sum of dz1 | d_fc2_b | d_fc3_b (elements 0 .. act_dim)
#define AM_PITCH (AM_VECS * SH)                  // a work-group's partial row

static_assert(FLEXNET_ACTOR_MLP_WS_FLOATS >= FLEXNET_MAX_AGENTS * AT_MAX_BLOCKS * AM_PITCH, "workspace macro");
static_assert(FLEXNET_ACTOR_MLP_UNSHARED_WS_FLOATS >= FLEXNET_MAX_AGENTS * AT_MAX_BLOCKS * AM_PITCH, "workspace macro");
static_assert(FLEXNET_MAX_ACT == 8, "the heads' eight outputs are the first k-group of a tile: registers 0..3 of both lane halves");

// agent `ag`'s pointer of a weight field: the field itself with one set of weights, entry `ag` of a table of per-agent ones
__device__ __forceinline__ const float* am_pick(const float* p, int) { return p; }
__device__ __forceinline__ const float* am_pick(const float* const (&p)[FLEXNET_MAX_AGENTS], int ag) { return p[ag]; }

// ---- forward: A = FlexActorMlpArgs or FlexActorMlpUnsharedArgs --------------------------------------------------------------
// (one body with or without the saves: the no-grad launch and the training forward give the same bits)
template <class A>
__device__ __forceinline__ void am_forward(const A& a) {
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
    const int ld1 = a.obs_dim + (a.agent_id ? n : 0);
    const float* W1 = am_pick(a.fc1_w, ag);
    const float* B1 = am_pick(a.fc1_b, ag);

    tv16 x[2] = {zero_tile(), zero_tile()};
    at_fc1_block(x, a.obs + row * a.obs_dim, W1 + (int64_t)i * ld1, W1 + (int64_t)(32 + i) * ld1, a.obs_dim, h);
    // + bias + the agent's id column (of its own fc1, where the weights are per agent) -> z1 (saved), LayerNorm, ReLU -> x (saved)
    at_add_bias_id(x, B1, a.agent_id ? W1 + a.obs_dim + ag : nullptr, ld1, h);
    if (SAVE) {
        store_tile(a.save_z1 + row * SH + 4 * h, x[0], ok);
        store_tile(a.save_z1 + row * SH + 32 + 4 * h, x[1], ok);
    }
    at_layernorm_relu(x, a.layernorm, am_pick(a.ln_w, ag), am_pick(a.ln_b, ag), a.ln_eps, h);
    if (SAVE) {
        store_tile(a.save_x + row * SH + 4 * h, x[0], ok);
        store_tile(a.save_x + row * SH + 32 + 4 * h, x[1], ok);
    }
    // fc2, ReLU -> h: the function's second result, and the backward's third save
    const float* W2 = am_pick(a.fc2_w, ag);
    const float* B2 = am_pick(a.fc2_b, ag);
    tv16 hh[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        hh[t] = bias_tile(B2 + 32 * t, h);
        hh[t] = layer_tile(W2 + (int64_t)(32 * t + i) * SH + 4 * h, hh[t], x[0], x[1]);
#pragma unroll
        for (int r = 0; r < 16; ++r) hh[t][r] = fmaxf(hh[t][r], 0.0f);
        store_tile(a.h + row * SH + 32 * t + 4 * h, hh[t], ok);
    }
    // fc3
    const bool live = i < a.act_dim;
    const float* B3 = am_pick(a.fc3_b, ag);
    tv16 m = zero_tile();
    at_head(m, am_pick(a.fc3_w, ag) + (int64_t)(live ? i : 0) * SH + 4 * h, live, hh);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int c = 4 * h + j;
        if (ok && c < a.act_dim) a.means[row * a.act_dim + c] = m[j] + B3[c];
    }
}

__global__ __launch_bounds__(64 * AT_W) void actor_mlp_forward_kernel(FlexActorMlpArgs a) { am_forward(a); }
__global__ __launch_bounds__(64 * AT_W) void mlp_unshared_actor_forward_kernel(FlexActorMlpUnsharedArgs a) { am_forward(a); }

// ---- backward: A = FlexActorMlpBwdArgs or FlexActorMlpUnsharedBwdArgs ---------------------------------------------------------
// Leaves a work-group's five partial vectors, over its agent's rows, in row (agent, work-group) of the workspace.
template <class A>
__device__ __forceinline__ void am_backward(const A& a, int blocks_per_agent) {
    __shared__ __attribute__((aligned(16))) float s_lnw[SH];
    __shared__ __attribute__((aligned(16))) float s_w3[FLEXNET_MAX_ACT * SH];      // the agent's fc3_w, rows past act_dim zero
    // the agent's fc2_w (columns for dx); after the tile loop the same memory is the fold buffer
    __shared__ __attribute__((aligned(16))) float s_buf[AT_W * 64 * AT_FOLD];
    static_assert(SH * AT_WP <= AT_W * 64 * AT_FOLD, "the fc2_w tile lives in the fold buffer");
    float (*fold)[64][AT_FOLD] = reinterpret_cast<float (*)[64][AT_FOLD]>(s_buf);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, i = lane & 31, h = lane >> 5;
    const int n = a.n_agents;
    const int ag = blockIdx.x % n, kb = blockIdx.x / n;
    const int64_t batch = a.rows / n;
    const int64_t tiles = (batch + 31) / 32;
    const int na = a.act_dim;
    at_stage_weight(s_buf, am_pick(a.fc2_w, ag), SH, tid);
    at_stage_head(s_w3, am_pick(a.fc3_w, ag), na, tid);
    if (tid < SH) s_lnw[tid] = a.layernorm ? am_pick(a.ln_w, ag)[tid] : 1.0f;
    __syncthreads();

    tv16 acc_g[2], acc_b[2], acc_d[2], acc_b2[2];
    float acc_b3[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        acc_g[t] = zero_tile(); acc_b[t] = zero_tile(); acc_d[t] = zero_tile(); acc_b2[t] = zero_tile();
    }
#pragma unroll 1
    for (int64_t tile = (int64_t)kb * AT_W + wave; tile < tiles; tile += (int64_t)blocks_per_agent * AT_W) {
        bool ok;
        const int64_t row = at_loop_sample(tile, i, batch, ok) * n + ag;
        // the lane's four of its row's d_means: c = 4 h + j (a dead row's are zero: so is everything below)
        float dm[4];
        at_head_grad(dm, a.d_means + row * na, na, h, ok);
#pragma unroll
        for (int j = 0; j < 4; ++j) acc_b3[j] += dm[j];
        // dh = d_means @ fc3_w (+ d_h), dz2 = dh [h > 0]
        tv16 dz2[2];
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            tv16 dh = zero_tile();
            if (a.d_h && ok) dh = load_tile(a.d_h + row * SH + 32 * t + 4 * h);
            dh = at_head_transposed(s_w3 + 32 * t + i, h, dh, dm);
            const tv16 hv = load_tile(a.h + row * SH + 32 * t + 4 * h);
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                dz2[t][e] = hv[e] > 0.0f ? dh[e] : 0.0f;
                acc_b2[t][e] += dz2[t][e];
            }
            store_tile(a.dz2 + row * SH + 32 * t + 4 * h, dz2[t], ok);
        }
        // dx = dz2 @ fc2_w: never stored
        tv16 dx[2] = {zero_tile(), zero_tile()};
#pragma unroll
        for (int to = 0; to < 2; ++to) {
            const float* wc = s_buf + (32 * to) * AT_WP + i;
            dx[0] = transposed_tile(wc, AT_WP, h, dx[0], dz2[to]);
            dx[1] = transposed_tile(wc + 32, AT_WP, h, dx[1], dz2[to]);
        }
        // LayerNorm / ReLU backward; ReLU's mask from the forward's own output
        const tv16 XS[2] = {load_tile(a.x + row * SH + 4 * h), load_tile(a.x + row * SH + 32 + 4 * h)};
        tv16 dzv[2];
        at_ln_relu_backward<true, false>(a.z1 + row * SH, nullptr, XS, nullptr, dx, s_lnw, a.layernorm, a.ln_eps, a.dz1 + row * SH,
                                         h, ok, acc_g, acc_b, acc_d, dzv);
    }

    float* out = a.workspace + ((int64_t)ag * blocks_per_agent + kb) * AM_PITCH;
    __syncthreads();                                           // every wavefront is done with the fc2_w tile
    at_fold(fold, out, tid, acc_g, acc_b, acc_d, acc_b2);
    // d_fc3_b: lane half hh of a row holds its d_means 4 hh .. 4 hh + 3
#pragma unroll
    for (int j = 0; j < 4; ++j) fold[wave][lane][j] = acc_b3[j];
    __syncthreads();
    if (tid < SH) {
        float sum = 0.0f;
        if (tid < FLEXNET_MAX_ACT) {
            for (int wv = 0; wv < AT_W; ++wv)
                for (int ii = 0; ii < 32; ++ii) sum += fold[wv][32 * (tid >> 2) + ii][tid & 3];
        }
        out[4 * SH + tid] = sum;
    }
}

__global__ __launch_bounds__(64 * AT_W) void actor_mlp_backward_kernel(FlexActorMlpBwdArgs a, int blocks_per_agent) {
    am_backward(a, blocks_per_agent);
}
__global__ __launch_bounds__(64 * AT_W) void mlp_unshared_actor_backward_kernel(FlexActorMlpUnsharedBwdArgs a, int blocks_per_agent) {
    am_backward(a, blocks_per_agent);
}

// ---- the second launch: the work-groups' partial rows summed in a fixed order; one kernel per form ------------------------------
// One set of weights, element ex.  Blocks 0 .. 4: a vector over every agent's rows (d_ln_w, d_ln_b, d_fc1_b, d_fc2_b,
// d_fc3_b); block 5 + a: the sum of dz1 over agent a's rows.
__global__ __launch_bounds__(64 * FLEX_RED_G) void actor_mlp_reduce_kernel(FlexActorMlpBwdArgs a, int blocks_per_agent) {
    const int ex = threadIdx.x & 63;
    const int vec = blockIdx.x < AM_VECS ? blockIdx.x : 2;
    const int ag = blockIdx.x < AM_VECS ? 0 : blockIdx.x - AM_VECS;
    const int rows = blockIdx.x < AM_VECS ? blocks_per_agent * a.n_agents : blocks_per_agent;
    float sum;
    if (!flex_reduce_rows(a.workspace + (int64_t)ag * blocks_per_agent * AM_PITCH + vec * SH + ex, AM_PITCH, rows, true, sum))
        return;
    if (blockIdx.x >= AM_VECS) a.d_dz1_agent[ag * SH + ex] = sum;
    else if (vec == 0) { if (a.layernorm) a.d_ln_w[ex] = sum; }
    else if (vec == 1) { if (a.layernorm) a.d_ln_b[ex] = sum; }
    else if (vec == 2) a.d_fc1_b[ex] = sum;
    else if (vec == 3) a.d_fc2_b[ex] = sum;
    else if (ex < a.act_dim) a.d_fc3_b[ex] = sum;
}

// Per-agent weights: block = AM_VECS * agent + vector (vector 2, the sum of dz1 over the agent's rows, is its d_fc1_b)
__global__ __launch_bounds__(64 * FLEX_RED_G) void mlp_unshared_actor_reduce_kernel(FlexActorMlpUnsharedBwdArgs a, int blocks_per_agent) {
    int ag, vec, ex;
    float sum;
    if (!at_reduce_agent(a.workspace, AM_VECS, blocks_per_agent, ag, vec, ex, sum)) return;
    if (vec == 0) { if (a.layernorm) a.d_ln_w[ag * SH + ex] = sum; }
    else if (vec == 1) { if (a.layernorm) a.d_ln_b[ag * SH + ex] = sum; }
    else if (vec == 2) a.d_fc1_b[ag * SH + ex] = sum;
    else if (vec == 3) a.d_fc2_b[ag * SH + ex] = sum;
    else if (ex < a.act_dim) a.d_fc3_b[ag * a.act_dim + ex] = sum;
}

// ---- entry points: checks, the grid, the launches on the caller's stream; nothing else ---------------------------------------
// (the two forms check their pointers apart: fields against table entries, in the order include/flexnet.h documents)
static int am_check_shape(int rows, int n, int obs_dim, int act_dim, int hid) {
    if (rows < 0 || n < 1 || obs_dim < 1 || act_dim < 1 || rows % n != 0) return FLEXNET_EINVAL;
    if (hid != FLEXNET_HID || n > FLEXNET_MAX_AGENTS || obs_dim > FLEXNET_MAX_OBS || act_dim > FLEXNET_MAX_ACT)
        return FLEXNET_EUNSUPPORTED;
    return FLEXNET_OK;
}

extern "C" int flexnet_actor_mlp_forward(const FlexActorMlpArgs* a, void* stream) {
    if (!a) return FLEXNET_EINVAL;
    if (!a->obs || !a->fc1_w || !a->fc1_b || !a->fc2_w || !a->fc2_b || !a->fc3_w || !a->fc3_b || !a->means || !a->h)
        return FLEXNET_EINVAL;
    if (a->layernorm && (!a->ln_w || !a->ln_b)) return FLEXNET_EINVAL;
    const int rc = am_check_shape(a->rows, a->n_agents, a->obs_dim, a->act_dim, a->hid);
    if (rc != FLEXNET_OK) return rc;
    if ((a->save_z1 != nullptr) != (a->save_x != nullptr)) return FLEXNET_EINVAL;       // both or none (h is always written)
    bool aligned = flex_aligned(a->fc2_w, 16) && flex_aligned(a->fc3_w, 16) && flex_aligned(a->h, 16);
    if (a->save_z1) aligned = aligned && flex_aligned(a->save_z1, 16) && flex_aligned(a->save_x, 16);
    if (!aligned) return FLEXNET_EUNSUPPORTED;
    if (a->rows == 0) return FLEXNET_OK;
    const int64_t groups = at_groups(a->rows / a->n_agents);
    hipLaunchKernelGGL(actor_mlp_forward_kernel, dim3((unsigned)(groups * a->n_agents)), dim3(64 * AT_W), 0,
                       (hipStream_t)stream, *a);
    return flex_launch_status();
}

extern "C" int flexnet_actor_mlp_backward(const FlexActorMlpBwdArgs* a, void* stream) {
    if (!a) return FLEXNET_EINVAL;
    if (!a->d_means || !a->z1 || !a->x || !a->h || !a->fc2_w || !a->fc3_w || !a->dz1 || !a->dz2 || !a->d_fc1_b ||
        !a->d_fc2_b || !a->d_fc3_b || !a->d_dz1_agent || !a->workspace)
        return FLEXNET_EINVAL;
    if (a->layernorm && (!a->ln_w || !a->d_ln_w || !a->d_ln_b)) return FLEXNET_EINVAL;
    const int rc = am_check_shape(a->rows, a->n_agents, a->obs_dim, a->act_dim, a->hid);
    if (rc != FLEXNET_OK) return rc;
    const int64_t bpa = at_blocks_per_agent(a->rows / a->n_agents);
    if (bpa * a->n_agents * AM_PITCH > a->workspace_floats) return FLEXNET_EINVAL;
    if (!(flex_aligned(a->z1, 16) && flex_aligned(a->x, 16) && flex_aligned(a->h, 16) && flex_aligned(a->dz1, 16) &&
          flex_aligned(a->dz2, 16) && flex_aligned(a->d_h, 16)))
        return FLEXNET_EUNSUPPORTED;
    if (a->rows == 0) return FLEXNET_OK;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(actor_mlp_backward_kernel, dim3((unsigned)(bpa * a->n_agents)), dim3(64 * AT_W), 0, s, *a, (int)bpa);
    hipLaunchKernelGGL(actor_mlp_reduce_kernel, dim3(AM_VECS + a->n_agents), dim3(64 * FLEX_RED_G), 0, s, *a, (int)bpa);
    return flex_launch_status();
}

extern "C" int flexnet_actor_mlp_unshared_forward(const FlexActorMlpUnsharedArgs* a, void* stream) {
    if (!a) return FLEXNET_EINVAL;
    if (!a->obs || !a->means || !a->h) return FLEXNET_EINVAL;
    const int rc = am_check_shape(a->rows, a->n_agents, a->obs_dim, a->act_dim, a->hid);
    if (rc != FLEXNET_OK) return rc;
    if ((a->save_z1 != nullptr) != (a->save_x != nullptr)) return FLEXNET_EINVAL;       // both or none (h is always written)
    bool aligned = flex_aligned(a->h, 16);
    for (int k = 0; k < a->n_agents; ++k) {
        if (!a->fc1_w[k] || !a->fc1_b[k] || !a->fc2_w[k] || !a->fc2_b[k] || !a->fc3_w[k] || !a->fc3_b[k] ||
            (a->layernorm && (!a->ln_w[k] || !a->ln_b[k])))
            return FLEXNET_EINVAL;
        aligned = aligned && flex_aligned(a->fc2_w[k], 16) && flex_aligned(a->fc3_w[k], 16);
    }
    if (a->save_z1) aligned = aligned && flex_aligned(a->save_z1, 16) && flex_aligned(a->save_x, 16);
    if (!aligned) return FLEXNET_EUNSUPPORTED;
    if (a->rows == 0) return FLEXNET_OK;
    const int64_t groups = at_groups(a->rows / a->n_agents);
    hipLaunchKernelGGL(mlp_unshared_actor_forward_kernel, dim3((unsigned)(groups * a->n_agents)), dim3(64 * AT_W), 0,
                       (hipStream_t)stream, *a);
    return flex_launch_status();
}

extern "C" int flexnet_actor_mlp_unshared_backward(const FlexActorMlpUnsharedBwdArgs* a, void* stream) {
    if (!a) return FLEXNET_EINVAL;
    if (!a->d_means || !a->z1 || !a->x || !a->h || !a->dz1 || !a->dz2 || !a->d_fc1_b || !a->d_fc2_b || !a->d_fc3_b || !a->workspace)
        return FLEXNET_EINVAL;
    if (a->layernorm && (!a->d_ln_w || !a->d_ln_b)) return FLEXNET_EINVAL;
    const int rc = am_check_shape(a->rows, a->n_agents, a->obs_dim, a->act_dim, a->hid);
    if (rc != FLEXNET_OK) return rc;
    for (int k = 0; k < a->n_agents; ++k) {
        if (!a->fc2_w[k] || !a->fc3_w[k] || (a->layernorm && !a->ln_w[k])) return FLEXNET_EINVAL;
    }
    const int64_t bpa = at_blocks_per_agent(a->rows / a->n_agents);
    if (bpa * a->n_agents * AM_PITCH > a->workspace_floats) return FLEXNET_EINVAL;
    if (!(flex_aligned(a->z1, 16) && flex_aligned(a->x, 16) && flex_aligned(a->h, 16) && flex_aligned(a->dz1, 16) &&
          flex_aligned(a->dz2, 16) && flex_aligned(a->d_h, 16)))
        return FLEXNET_EUNSUPPORTED;
    if (a->rows == 0) return FLEXNET_OK;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(mlp_unshared_actor_backward_kernel, dim3((unsigned)(bpa * a->n_agents)), dim3(64 * AT_W), 0, s, *a, (int)bpa);
    hipLaunchKernelGGL(mlp_unshared_actor_reduce_kernel, dim3(AM_VECS * a->n_agents), dim3(64 * FLEX_RED_G), 0, s, *a, (int)bpa);
    return flex_launch_status();
}
