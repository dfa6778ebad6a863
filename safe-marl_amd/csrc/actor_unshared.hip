// actor_unshared.hip — the RNN actors of `shared_params: False` (madrl/models/model.py:124-138: one RNNAgent per agent) for a
// whole batch in ONE launch, forward and backward (gfx950).  Boundary: include/flexnet.h (FlexActorUnsharedArgs /
// FlexActorUnsharedBwdArgs).  Reference arithmetic: madrl/agents/rnn_agent.py:25-33 per agent.
//
// Work map and the stages shared with critic_unshared.hip and actor_mlp.hip: flex_agent_tile.h (one wavefront owns 32 samples
// of ONE agent, a work-group is four wavefronts of the same agent: their weight reads share the CU's cache).  The weights are
// read where the modules keep them, through per-agent pointer tables in the argument struct.
//
// Forward: fc1 over the observation columns, + bias + the agent's OWN id column, LayerNorm, ReLU, GRUCell (r, z, n), fc2; with
// the six training saves of FlexActorArgs.  Backward: gru.hip's fused arithmetic (gate gradients, dx = d_gi @ W_ih on the
// matrix cores and never stored, LayerNorm / ReLU / bias backward) on this map; the [n_agents, 64] parameter sums are per-lane
// sums folded per work-group in a fixed order and summed over work-groups by a second launch: no atomics, bit-reproducible.
// A second backward kernel from the same body (flexnet_actor_unshared_backward_hn) starts dh' from d_hn, the gradient the
// per-agent log-std heads of RNNAgentGaussian modules send to the new hidden state; it is launched eagerly only.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "flexnet.h"
#include "flex_launch.h"
#include "flex_agent_tile.h"

#define AU_VECS 3                                // d_ln_w | d_ln_b | d_fc1_b
#define AU_PITCH (AU_VECS * SH)                  // a work-group's partial row

static_assert(FLEXNET_ACTOR_UNSHARED_WS_FLOATS >= FLEXNET_MAX_AGENTS * AT_MAX_BLOCKS * AU_PITCH, "workspace macro");

__device__ __forceinline__ float au_sigmoid(float x) { return 1.0f / (1.0f + expf(-x)); }

// the sum of two bias vectors over the lane's units
__device__ __forceinline__ tv16 au_bias2_tile(const float* b0, const float* b1, int h) {
    tv16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = b0[TILE_U(r, h)] + b1[TILE_U(r, h)];
    return acc;
}

// (one kernel with or without the saves: the inference launch and the training forward give the same bits)
__global__ __launch_bounds__(64 * AT_W) void actor_unshared_forward_kernel(FlexActorUnsharedArgs a) {
    const bool SAVE = a.save_z1 != nullptr;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, i = lane & 31, h = lane >> 5;
    const int n = a.n_agents, ad = a.act_dim, od = a.obs_dim;
    const int ag = blockIdx.x % n;
    const int64_t batch = a.rows / n;
    const int64_t s0 = ((int64_t)(blockIdx.x / n) * AT_W + wave) * 32;
    if (s0 >= batch) return;                                   // (the kernel has no barrier)
    const bool ok = s0 + i < batch;
    const int64_t s = ok ? s0 + i : batch - 1;                 // the last partial tile re-reads a valid sample
    const int64_t row = s * n + ag;
    const int ld1 = od + (a.agent_id ? n : 0);
    const float* W1 = a.fc1_w[ag];
    const float* b1 = a.fc1_b[ag];
    const float* Wih = a.w_ih[ag];
    const float* Whh = a.w_hh[ag];
    const float* bih = a.b_ih[ag];
    const float* bhh = a.b_hh[ag];

    // fc1 over the observation columns -> z1 (saved BEFORE the bias: the backward adds it again), + bias + the agent's own id
    // column, LayerNorm, ReLU -> x (saved).  The block product is at_fc1_block's text, kept in the kernel: through the function
    // this launch measured 1.5 % slower at 163 840 rows (profiles/agent_tile_shared_bench.txt).
    tv16 x[2] = {zero_tile(), zero_tile()};
    {
        const float* op = a.obs + row * od;
        const float* w0 = W1 + (int64_t)i * ld1;
        const float* w1 = W1 + (int64_t)(32 + i) * ld1;
        for (int c0 = 0; c0 < od; c0 += 8) {
            float o[4], wa[4], wb[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int c = c0 + 4 * h + j;
                const bool in = c < od;
                const int cc = in ? c : od - 1;                // (clamped: no load past the row)
                const float ov = op[cc], av = w0[cc], bv = w1[cc];
                o[j] = in ? ov : 0.0f; wa[j] = in ? av : 0.0f; wb[j] = in ? bv : 0.0f;
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                x[0] = TILE_MFMA(wa[j], o[j], x[0]);
                x[1] = TILE_MFMA(wb[j], o[j], x[1]);
            }
        }
    }
    if (SAVE) {
        store_tile(a.save_z1 + row * SH + 4 * h, x[0], ok);
        store_tile(a.save_z1 + row * SH + 32 + 4 * h, x[1], ok);
    }
    at_add_bias_id(x, b1, a.agent_id ? W1 + od + ag : nullptr, ld1, h);
    at_layernorm_relu(x, a.layernorm, a.ln_w[ag], a.ln_b[ag], a.ln_eps, h);
    if (SAVE) {
        store_tile(a.save_x + row * SH + 4 * h, x[0], ok);
        store_tile(a.save_x + row * SH + 32 + 4 * h, x[1], ok);
    }

    // GRUCell, 32 units at a time: r and z sum both products in one accumulator, the candidate keeps W_hn h + b_hn apart
    const tv16 hp[2] = {load_tile(a.hidden_in + row * SH + 4 * h), load_tile(a.hidden_in + row * SH + 32 + 4 * h)};
    tv16 hn[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const int ub = 32 * t;
        tv16 gr = au_bias2_tile(bih + ub, bhh + ub, h);
        gr = layer_tile(Wih + (int64_t)(ub + i) * SH + 4 * h, gr, x[0], x[1]);
        gr = layer_tile(Whh + (int64_t)(ub + i) * SH + 4 * h, gr, hp[0], hp[1]);
        tv16 gz = au_bias2_tile(bih + SH + ub, bhh + SH + ub, h);
        gz = layer_tile(Wih + (int64_t)(SH + ub + i) * SH + 4 * h, gz, x[0], x[1]);
        gz = layer_tile(Whh + (int64_t)(SH + ub + i) * SH + 4 * h, gz, hp[0], hp[1]);
        tv16 gin = bias_tile(bih + 2 * SH + ub, h);
        gin = layer_tile(Wih + (int64_t)(2 * SH + ub + i) * SH + 4 * h, gin, x[0], x[1]);
        tv16 ghn = bias_tile(bhh + 2 * SH + ub, h);
        ghn = layer_tile(Whh + (int64_t)(2 * SH + ub + i) * SH + 4 * h, ghn, hp[0], hp[1]);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const float rg = au_sigmoid(gr[r]), zg = au_sigmoid(gz[r]);
            const float ng = tanhf(gin[r] + rg * ghn[r]);
            gr[r] = rg; gz[r] = zg; gin[r] = ng;
            hn[t][r] = (1.0f - zg) * ng + zg * hp[t][r];
        }
        if (SAVE) {
            store_tile(a.save_r + row * SH + ub + 4 * h, gr, ok);
            store_tile(a.save_z + row * SH + ub + 4 * h, gz, ok);
            store_tile(a.save_n + row * SH + ub + 4 * h, gin, ok);
            store_tile(a.save_hn + row * SH + ub + 4 * h, ghn, ok);
        }
        store_tile(a.hidden_out + row * SH + ub + 4 * h, hn[t], ok);
    }

    // fc2
    const bool live = i < ad;
    tv16 m = zero_tile();
    at_head(m, a.fc2_w[ag] + (int64_t)(live ? i : 0) * SH + 4 * h, live, hn);
    const float* b2 = a.fc2_b[ag];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int k = 4 * h + j;
        if (ok && k < ad) a.means[row * ad + k] = m[j] + b2[k];
    }
}

// ---- backward ---------------------------------------------------------------------------------------------------------
// (the body of both backward kernels: WITH_HN = the variant that starts dh' from d_hn, the gradient the per-agent log-std heads
// send to the new hidden state; without it the body is the kernel as it always was)
template <bool WITH_HN>
__device__ __forceinline__ void au_backward_body(const FlexActorUnsharedBwdArgs& a, const float* d_hn, int blocks_per_agent) {
    __shared__ __attribute__((aligned(16))) float s_add[SH], s_lnw[SH];
    __shared__ __attribute__((aligned(16))) float s_w2[FLEXNET_MAX_ACT * SH];
    // W_ih of the agent, read by the dx chains from ONE base register (with the weights in global memory the compiler kept a
    // 64-bit address per chain step live across the tile loop and spilled); after the loop the same memory is the fold buffer
    __shared__ float s_wih[3 * SH * AT_WP];
    static_assert(AT_W * 64 * AT_FOLD <= 3 * SH * AT_WP, "the fold buffer lives in the W_ih tile");
    float (*fold)[64][AT_FOLD] = reinterpret_cast<float (*)[64][AT_FOLD]>(s_wih);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, i = lane & 31, h = lane >> 5;
    const int n = a.n_agents, ad = a.act_dim, od = a.obs_dim;
    const int ag = blockIdx.x % n, kb = blockIdx.x / n;
    const int64_t batch = a.rows / n;
    const int64_t tiles = (batch + 31) / 32;
    const int ld1 = od + (a.agent_id ? n : 0);
    at_stage_weight(s_wih, a.w_ih[ag], 3 * SH, tid);
    at_stage_head(s_w2, a.fc2_w[ag], ad, tid);
    if (tid < SH) {
        s_add[tid] = at_unit_add(a.fc1_b[ag], a.agent_id ? a.fc1_w[ag] + od + ag : nullptr, ld1, tid);
        s_lnw[tid] = a.layernorm ? a.ln_w[ag][tid] : 1.0f;
    }
    __syncthreads();

    tv16 acc_g[2] = {zero_tile(), zero_tile()}, acc_b[2] = {zero_tile(), zero_tile()},
         acc_d[2] = {zero_tile(), zero_tile()};
#pragma unroll 1
    for (int64_t tile = (int64_t)kb * AT_W + wave; tile < tiles; tile += (int64_t)blocks_per_agent * AT_W) {
        bool ok;
        const int64_t row = at_loop_sample(tile, i, batch, ok) * n + ag;

        // dh' = d_means @ fc2_w: four steps per 32 units (the outputs past act_dim are zero rows)
        tv16 dh[2] = {zero_tile(), zero_tile()};
        if (WITH_HN && ok) {                                      // (+ d_hn: the accumulators start from it)
            dh[0] = load_tile(d_hn + row * SH + 4 * h);
            dh[1] = load_tile(d_hn + row * SH + 32 + 4 * h);
        }
        float dm[4];
        at_head_grad(dm, a.d_means + row * ad, ad, h, ok);
        dh[0] = at_head_transposed(s_w2 + i, h, dh[0], dm);
        dh[1] = at_head_transposed(s_w2 + 32 + i, h, dh[1], dm);
        // gate gradients (a dead row's dh' is zero: so is everything below)
        tv16 dgi[3][2];
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const int64_t at = row * SH + 32 * t + 4 * h;
            const tv16 R = load_tile(a.r + at), Z = load_tile(a.z + at), N = load_tile(a.n + at), HN = load_tile(a.hn + at),
                       HP = load_tile(a.h_prev + at);
            tv16 dnr;
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const float g = dh[t][e];
                const float dn = g * (1.0f - Z[e]) * (1.0f - N[e] * N[e]);
                const float dz = g * (HP[e] - N[e]) * Z[e] * (1.0f - Z[e]);
                const float dr = dn * HN[e] * R[e] * (1.0f - R[e]);
                dgi[0][t][e] = dr; dgi[1][t][e] = dz; dgi[2][t][e] = dn;
                dnr[e] = dn * R[e];
            }
            float* gi = a.d_gi + row * (3 * SH) + 32 * t + 4 * h;
            float* gh = a.d_gh + row * (3 * SH) + 32 * t + 4 * h;
            store_tile(gi, dgi[0][t], ok); store_tile(gi + SH, dgi[1][t], ok); store_tile(gi + 2 * SH, dgi[2][t], ok);
            store_tile(gh, dgi[0][t], ok); store_tile(gh + SH, dgi[1][t], ok); store_tile(gh + 2 * SH, dnr, ok);
        }
        // dx = d_gi @ W_ih: never stored
        tv16 dx[2] = {zero_tile(), zero_tile()};
#pragma unroll
        for (int G = 0; G < 3; ++G) {
#pragma unroll
            for (int to = 0; to < 2; ++to) {
                const float* wc = s_wih + (SH * G + 32 * to) * AT_WP + i;
                dx[0] = transposed_tile(wc, AT_WP, h, dx[0], dgi[G][to]);
                dx[1] = transposed_tile(wc + 32, AT_WP, h, dx[1], dgi[G][to]);
            }
        }
        // LayerNorm / ReLU / bias backward; ReLU's mask from the forward's own output
        tv16 dzv[2];
        at_ln_relu_backward<true, true>(a.z1 + row * SH, s_add, nullptr, a.x + row * SH, dx, s_lnw, a.layernorm, a.ln_eps,
                                        a.dz + row * SH, h, ok, acc_g, acc_b, acc_d, dzv);
    }

    __syncthreads();                                           // every wavefront is done with the W_ih tile
    at_fold(fold, a.workspace + ((int64_t)ag * blocks_per_agent + kb) * AU_PITCH, tid, acc_g, acc_b, acc_d);
}

__global__ __launch_bounds__(64 * AT_W) void actor_unshared_backward_kernel(FlexActorUnsharedBwdArgs a, int blocks_per_agent) {
    au_backward_body<false>(a, nullptr, blocks_per_agent);
}

__global__ __launch_bounds__(64 * AT_W) void actor_hn_unshared_backward_kernel(FlexActorUnsharedBwdArgs a, const float* d_hn,
                                                                             int blocks_per_agent) {
    au_backward_body<true>(a, d_hn, blocks_per_agent);
}

// the second launch: block = AU_VECS * agent + vector
__global__ __launch_bounds__(64 * FLEX_RED_G) void actor_unshared_reduce_kernel(FlexActorUnsharedBwdArgs a, int blocks_per_agent) {
    int ag, vec, ex;
    float sum;
    if (!at_reduce_agent(a.workspace, AU_VECS, blocks_per_agent, ag, vec, ex, sum)) return;
    if (vec == 0) { if (a.layernorm) a.d_ln_w[ag * SH + ex] = sum; }
    else if (vec == 1) { if (a.layernorm) a.d_ln_b[ag * SH + ex] = sum; }
    else a.d_fc1_b[ag * SH + ex] = sum;
}

// ---- entry points -----------------------------------------------------------------------------------------------------
static int au_check_shape(int rows, int n, int od, int ad) {
    if (n < 1 || od < 1 || ad < 1 || rows % n != 0) return FLEXNET_EINVAL;
    if (n > FLEXNET_MAX_AGENTS || od > FLEXNET_MAX_OBS || ad > FLEXNET_MAX_ACT) return FLEXNET_EUNSUPPORTED;
    return FLEXNET_OK;
}

extern "C" int flexnet_actor_unshared_forward(const FlexActorUnsharedArgs* a, void* stream) {
    if (!a || a->rows < 0) return FLEXNET_EINVAL;
    if (!a->obs || !a->hidden_in || !a->means || !a->hidden_out) return FLEXNET_EINVAL;
    const int rc = au_check_shape(a->rows, a->n_agents, a->obs_dim, a->act_dim);
    if (rc != FLEXNET_OK) return rc;
    bool aligned = flex_aligned(a->hidden_in, 16) && flex_aligned(a->hidden_out, 16);
    for (int k = 0; k < a->n_agents; ++k) {
        if (!a->fc1_w[k] || !a->fc1_b[k] || !a->w_ih[k] || !a->w_hh[k] || !a->b_ih[k] || !a->b_hh[k] || !a->fc2_w[k] ||
            !a->fc2_b[k] || (a->layernorm && (!a->ln_w[k] || !a->ln_b[k])))
            return FLEXNET_EINVAL;
        aligned = aligned && flex_aligned(a->w_ih[k], 16) && flex_aligned(a->w_hh[k], 16) && flex_aligned(a->fc2_w[k], 16);
    }
    const int saves = (a->save_z1 != nullptr) + (a->save_x != nullptr) + (a->save_r != nullptr) + (a->save_z != nullptr) +
                      (a->save_n != nullptr) + (a->save_hn != nullptr);
    if (saves != 0 && saves != 6) return FLEXNET_EINVAL;                      // all six or none
    if (saves) aligned = aligned && flex_aligned(a->save_z1, 16) && flex_aligned(a->save_x, 16) && flex_aligned(a->save_r, 16) &&
                         flex_aligned(a->save_z, 16) && flex_aligned(a->save_n, 16) && flex_aligned(a->save_hn, 16);
    if (!aligned) return FLEXNET_EUNSUPPORTED;
    if (a->rows == 0) return FLEXNET_OK;
    const int64_t groups = at_groups(a->rows / a->n_agents);
    const dim3 grid((unsigned)(groups * a->n_agents)), block(64 * AT_W);
    hipLaunchKernelGGL(actor_unshared_forward_kernel, grid, block, 0, (hipStream_t)stream, *a);
    return flex_launch_status();
}

// (d_hn NULL: flexnet_actor_unshared_backward; else its variant)
static int au_backward(const FlexActorUnsharedBwdArgs* a, const float* d_hn, void* stream) {
    if (!a || a->rows < 0) return FLEXNET_EINVAL;
    if (!a->d_means || !a->r || !a->z || !a->n || !a->hn || !a->h_prev || !a->z1 || !a->x || !a->d_gi || !a->d_gh || !a->dz ||
        !a->d_fc1_b || !a->workspace || (a->layernorm && (!a->d_ln_w || !a->d_ln_b)))
        return FLEXNET_EINVAL;
    const int rc = au_check_shape(a->rows, a->n_agents, a->obs_dim, a->act_dim);
    if (rc != FLEXNET_OK) return rc;
    bool aligned = flex_aligned(a->r, 16) && flex_aligned(a->z, 16) && flex_aligned(a->n, 16) && flex_aligned(a->hn, 16) &&
                   flex_aligned(a->h_prev, 16) && flex_aligned(a->z1, 16) && flex_aligned(a->x, 16) && flex_aligned(a->d_gi, 16) &&
                   flex_aligned(a->d_gh, 16) && flex_aligned(a->dz, 16);
    for (int k = 0; k < a->n_agents; ++k) {
        if (!a->fc1_w[k] || !a->fc1_b[k] || !a->w_ih[k] || !a->fc2_w[k] || (a->layernorm && !a->ln_w[k])) return FLEXNET_EINVAL;
    }
    if (!aligned || !flex_aligned(d_hn, 16)) return FLEXNET_EUNSUPPORTED;
    if (a->rows == 0) return FLEXNET_OK;
    const int64_t bpa = at_blocks_per_agent(a->rows / a->n_agents);
    if (bpa * a->n_agents * AU_PITCH > a->workspace_floats) return FLEXNET_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    if (d_hn)
        hipLaunchKernelGGL(actor_hn_unshared_backward_kernel, dim3((unsigned)(bpa * a->n_agents)), dim3(64 * AT_W), 0, s, *a, d_hn,
                           (int)bpa);
    else
        hipLaunchKernelGGL(actor_unshared_backward_kernel, dim3((unsigned)(bpa * a->n_agents)), dim3(64 * AT_W), 0, s, *a, (int)bpa);
    hipLaunchKernelGGL(actor_unshared_reduce_kernel, dim3(AU_VECS * a->n_agents), dim3(64 * FLEX_RED_G), 0, s, *a, (int)bpa);
    return flex_launch_status();
}

extern "C" int flexnet_actor_unshared_backward(const FlexActorUnsharedBwdArgs* a, void* stream) {
    return au_backward(a, nullptr, stream);
}

extern "C" int flexnet_actor_unshared_backward_hn(const FlexActorUnsharedBwdArgs* a, const float* d_hn, void* stream) {
    if (!d_hn) return FLEXNET_EINVAL;
    return au_backward(a, d_hn, stream);
}
