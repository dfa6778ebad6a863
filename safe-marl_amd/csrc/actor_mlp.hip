// actor_mlp.hip — the MLP actor of `agent_type: mlp` (madrl/agents/mlp_agent.py:20-32, mlp_agent_gaussian.py: fc1 -> LayerNorm ->
// ReLU -> fc2 -> ReLU = h -> fc3) for a whole batch in one launch per direction (gfx950), in both of its forms: ONE set of
// weights under `shared_params: True` (FlexActorMlpArgs / FlexActorMlpBwdArgs) and one MLPAgent / MLPAgentGaussian per agent
// under `shared_params: False` (madrl/models/model.py:124-138; FlexActorMlpUnsharedArgs / FlexActorMlpUnsharedBwdArgs).
// Boundary: include/flexnet.h.  The entry points are for eager calls: the host side never launches them on a capturing stream
// (nets.mlp_actor_allowed).
//
// Work map (critic_unshared.hip's): one wavefront owns 32 samples of ONE agent — rows r = s * n_agents + a of the [b * n, .]
// tensors — on flex_mfma_tile.h's transposed fp32 scheme; a work-group is four wavefronts of the same agent, blockIdx.x % n.
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
#include "flex_mfma_tile.h"
#include "flex_reduce.h"

#define AM_W 4                                   // wavefronts per work-group (one per SIMD)
#define AM_MAX_BLOCKS 128                        // backward work-groups per agent (the two FLEXNET_ACTOR_MLP*_WS_FLOATS)
#define AM_VECS 5                                // d_ln_w | d_ln_b | sum of dz1 | d_fc2_b | d_fc3_b (elements 0 .. act_dim)
#define AM_PITCH (AM_VECS * SH)                  // a work-group's partial row
#define AM_FOLD 33                               // pitch of a lane's 32 sums in the fold buffer
#define AM_WP 72                                 // pitch of an fc2_w row in LDS: the two lane halves hit disjoint banks

static_assert(FLEXNET_ACTOR_MLP_WS_FLOATS >= FLEXNET_MAX_AGENTS * AM_MAX_BLOCKS * AM_PITCH, "workspace macro");
static_assert(FLEXNET_ACTOR_MLP_UNSHARED_WS_FLOATS >= FLEXNET_MAX_AGENTS * AM_MAX_BLOCKS * AM_PITCH, "workspace macro");
static_assert(FLEXNET_MAX_ACT == 8, "the heads' eight outputs are the first k-group of a tile: registers 0..3 of both lane halves");

__device__ __forceinline__ tv16 am_zero_tile() {
    tv16 t;
#pragma unroll
    for (int r = 0; r < 16; ++r) t[r] = 0.0f;
    return t;
}

// agent `ag`'s pointer of a weight field: the field itself with one set of weights, entry `ag` of a table of per-agent ones
__device__ __forceinline__ const float* am_pick(const float* p, int) { return p; }
__device__ __forceinline__ const float* am_pick(const float* const (&p)[FLEXNET_MAX_AGENTS], int ag) { return p[ag]; }

// x += W[:, 0 .. width) @ xp[0 .. width) for the lane's row (critic_unshared.hip's cu_fc1_block): MFMA step j of a group of
// eight columns takes the pair (c + j, c + 4 + j); `w0` / `w1` = the lane's two weight rows.  (Clamped: no load past a row,
// no alignment asked of it.)
__device__ __forceinline__ void am_fc1_block(tv16* x, const float* xp, const float* w0, const float* w1, int width, int h) {
    for (int c0 = 0; c0 < width; c0 += 8) {
        float o[4], wa[4], wb[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int c = c0 + 4 * h + j;
            const bool in = c < width;
            const int cc = in ? c : width - 1;
            const float ov = xp[cc], av = w0[cc], bv = w1[cc];
            o[j] = in ? ov : 0.0f; wa[j] = in ? av : 0.0f; wb[j] = in ? bv : 0.0f;
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            x[0] = TILE_MFMA(wa[j], o[j], x[0]);
            x[1] = TILE_MFMA(wb[j], o[j], x[1]);
        }
    }
}

// ---- forward: A = FlexActorMlpArgs or FlexActorMlpUnsharedArgs --------------------------------------------------------------
// (one body with or without the saves: the no-grad launch and the training forward give the same bits)
template <class A>
__device__ __forceinline__ void am_forward(const A& a) {
    const bool SAVE = a.save_z1 != nullptr;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, i = lane & 31, h = lane >> 5;
    const int n = a.n_agents;
    const int ag = blockIdx.x % n;
    const int64_t batch = a.rows / n;
    const int64_t s0 = ((int64_t)(blockIdx.x / n) * AM_W + wave) * 32;
    if (s0 >= batch) return;                                   // (the kernel has no barrier)
    const bool ok = s0 + i < batch;
    const int64_t s = ok ? s0 + i : batch - 1;                 // the last partial tile re-reads a valid sample
    const int64_t row = s * n + ag;
    const int ld1 = a.obs_dim + (a.agent_id ? n : 0);
    const float* W1 = am_pick(a.fc1_w, ag);
    const float* B1 = am_pick(a.fc1_b, ag);

    tv16 x[2] = {am_zero_tile(), am_zero_tile()};
    am_fc1_block(x, a.obs + row * a.obs_dim, W1 + (int64_t)i * ld1, W1 + (int64_t)(32 + i) * ld1, a.obs_dim, h);
    // + bias + the agent's id column (of its own fc1, where the weights are per agent)
#pragma unroll
    for (int t = 0; t < 2; ++t) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int u = 32 * t + TILE_U(r, h);
            float add = B1[u];
            if (a.agent_id) add += W1[(int64_t)u * ld1 + a.obs_dim + ag];
            x[t][r] += add;
        }
    }
    if (SAVE) {
        store_tile(a.save_z1 + row * SH + 4 * h, x[0], ok);
        store_tile(a.save_z1 + row * SH + 32 + 4 * h, x[1], ok);
    }
    if (a.layernorm) {
        const float* LW = am_pick(a.ln_w, ag);
        const float* LB = am_pick(a.ln_b, ag);
        float mean, rstd;
        row_stats(x[0], x[1], a.ln_eps, mean, rstd);
#pragma unroll
        for (int t = 0; t < 2; ++t) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int u = 32 * t + TILE_U(r, h);
                x[t][r] = ((x[t][r] - mean) * rstd) * LW[u] + LB[u];
            }
        }
    }
#pragma unroll
    for (int t = 0; t < 2; ++t) {
#pragma unroll
        for (int r = 0; r < 16; ++r) x[t][r] = fmaxf(x[t][r], 0.0f);
    }
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
    // fc3: rows past act_dim of the A operand are zero; output c = 4 h + r sits in accumulator register r < 4
    const bool live = i < a.act_dim;
    const float* w3 = am_pick(a.fc3_w, ag) + (int64_t)(live ? i : 0) * SH + 4 * h;
    const float* B3 = am_pick(a.fc3_b, ag);
    tv16 m = am_zero_tile();
#pragma unroll
    for (int kt = 0; kt < 2; ++kt) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const tv4 w = ld4(w3 + 32 * kt + 8 * q);
#pragma unroll
            for (int j = 0; j < 4; ++j) m = TILE_MFMA(live ? w[j] : 0.0f, hh[kt][4 * q + j], m);
        }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int c = 4 * h + j;
        if (ok && c < a.act_dim) a.means[row * a.act_dim + c] = m[j] + B3[c];
    }
}

__global__ __launch_bounds__(64 * AM_W) void actor_mlp_forward_kernel(FlexActorMlpArgs a) { am_forward(a); }
__global__ __launch_bounds__(64 * AM_W) void mlp_unshared_actor_forward_kernel(FlexActorMlpUnsharedArgs a) { am_forward(a); }

// ---- backward: A = FlexActorMlpBwdArgs or FlexActorMlpUnsharedBwdArgs ---------------------------------------------------------
// Leaves a work-group's five partial vectors, over its agent's rows, in row (agent, work-group) of the workspace.
template <class A>
__device__ __forceinline__ void am_backward(const A& a, int blocks_per_agent) {
    __shared__ __attribute__((aligned(16))) float s_lnw[SH];
    __shared__ __attribute__((aligned(16))) float s_w3[FLEXNET_MAX_ACT * SH];      // the agent's fc3_w, rows past act_dim zero
    // the agent's fc2_w (columns for dx); after the tile loop the same memory is the fold buffer
    __shared__ __attribute__((aligned(16))) float s_buf[AM_W * 64 * AM_FOLD];
    static_assert(SH * AM_WP <= AM_W * 64 * AM_FOLD, "the fc2_w tile lives in the fold buffer");
    float (*fold)[64][AM_FOLD] = reinterpret_cast<float (*)[64][AM_FOLD]>(s_buf);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, i = lane & 31, h = lane >> 5;
    const int n = a.n_agents;
    const int ag = blockIdx.x % n, kb = blockIdx.x / n;
    const int64_t batch = a.rows / n;
    const int64_t tiles = (batch + 31) / 32;
    const int na = a.act_dim;
    {
        const float* W2 = am_pick(a.fc2_w, ag);
        const float* W3 = am_pick(a.fc3_w, ag);
        for (int idx = tid; idx < SH * SH; idx += 64 * AM_W) s_buf[(idx >> 6) * AM_WP + (idx & 63)] = W2[idx];
        for (int idx = tid; idx < FLEXNET_MAX_ACT * SH; idx += 64 * AM_W) s_w3[idx] = idx < na * SH ? W3[idx] : 0.0f;
        if (tid < SH) s_lnw[tid] = a.layernorm ? am_pick(a.ln_w, ag)[tid] : 1.0f;
    }
    __syncthreads();

    tv16 acc_g[2], acc_b[2], acc_d[2], acc_b2[2];
    float acc_b3[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        acc_g[t] = am_zero_tile(); acc_b[t] = am_zero_tile(); acc_d[t] = am_zero_tile(); acc_b2[t] = am_zero_tile();
    }
#pragma unroll 1
    for (int64_t tile = (int64_t)kb * AM_W + wave; tile < tiles; tile += (int64_t)blocks_per_agent * AM_W) {
        // (a compiler fence, as in critic_unshared.hip: without it the loop-invariant LDS reads of the weights are hoisted out
        // of the tile loop into registers the kernel does not have, and spill)
        __asm__ volatile("" ::: "memory");
        const int64_t s0 = tile * 32;
        const bool ok = s0 + i < batch;
        const int64_t s = ok ? s0 + i : batch - 1;
        const int64_t row = s * n + ag;
        // the lane's four of its row's d_means: c = 4 h + j (a dead row's are zero: so is everything below)
        float dm[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int c = 4 * h + j;
            const float v = a.d_means[row * na + (c < na ? c : na - 1)];
            dm[j] = ok && c < na ? v : 0.0f;
            acc_b3[j] += dm[j];
        }
        // dh = d_means @ fc3_w (+ d_h), dz2 = dh [h > 0]
        tv16 dz2[2];
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            tv16 dh = am_zero_tile();
            if (a.d_h && ok) dh = load_tile(a.d_h + row * SH + 32 * t + 4 * h);
#pragma unroll
            for (int j = 0; j < 4; ++j) dh = TILE_MFMA(s_w3[(4 * h + j) * SH + 32 * t + i], dm[j], dh);
            const tv16 hv = load_tile(a.h + row * SH + 32 * t + 4 * h);
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                dz2[t][e] = hv[e] > 0.0f ? dh[e] : 0.0f;
                acc_b2[t][e] += dz2[t][e];
            }
            store_tile(a.dz2 + row * SH + 32 * t + 4 * h, dz2[t], ok);
        }
        // dx = dz2 @ fc2_w: never stored
        tv16 dx[2] = {am_zero_tile(), am_zero_tile()};
#pragma unroll
        for (int to = 0; to < 2; ++to) {
            const float* wc = s_buf + (32 * to) * AM_WP + i;
            dx[0] = transposed_tile(wc, AM_WP, h, dx[0], dz2[to]);
            dx[1] = transposed_tile(wc + 32, AM_WP, h, dx[1], dz2[to]);
        }
        // LayerNorm / ReLU backward (csrc/lnrelu.hip's arithmetic); ReLU's mask from the forward's own output
        const tv16 XS[2] = {load_tile(a.x + row * SH + 4 * h), load_tile(a.x + row * SH + 32 + 4 * h)};
        tv16 xh[2] = {load_tile(a.z1 + row * SH + 4 * h), load_tile(a.z1 + row * SH + 32 + 4 * h)};
        float rstd = 1.0f;
        if (a.layernorm) {
            float mean;
            row_stats(xh[0], xh[1], a.ln_eps, mean, rstd);
#pragma unroll
            for (int t = 0; t < 2; ++t) {
#pragma unroll
                for (int e = 0; e < 16; ++e) xh[t][e] = (xh[t][e] - mean) * rstd;
            }
        }
        tv16 dzv[2];
        float s1 = 0.0f, s2 = 0.0f;
#pragma unroll
        for (int t = 0; t < 2; ++t) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const tv4 gw = ld4(s_lnw + 32 * t + 8 * q + 4 * h);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int e = 4 * q + j;
                    const float dy = XS[t][e] > 0.0f ? dx[t][e] : 0.0f;
                    acc_g[t][e] = fmaf(dy, xh[t][e], acc_g[t][e]);
                    acc_b[t][e] += dy;
                    const float dxh = dy * gw[j];
                    dzv[t][e] = dxh;
                    s1 += dxh;
                    s2 = fmaf(dxh, xh[t][e], s2);
                }
            }
        }
        if (a.layernorm) {
            const float m1 = (s1 + other_half(s1)) * (1.0f / SH), m2 = (s2 + other_half(s2)) * (1.0f / SH);
#pragma unroll
            for (int t = 0; t < 2; ++t) {
#pragma unroll
                for (int e = 0; e < 16; ++e) dzv[t][e] = rstd * (dzv[t][e] - m1 - xh[t][e] * m2);
            }
        }
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            store_tile(a.dz1 + row * SH + 32 * t + 4 * h, dzv[t], ok);
#pragma unroll
            for (int e = 0; e < 16; ++e) acc_d[t][e] += dzv[t][e];
        }
    }

    // work-group fold, fixed order: wavefronts in index order, rows in index order.  Register r of tile t in lane (i, h) is
    // unit 32 t + TILE_U(r, h) of one row.
    float* out = a.workspace + ((int64_t)ag * blocks_per_agent + kb) * AM_PITCH;
    __syncthreads();                                           // every wavefront is done with the fc2_w tile
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const tv16* src = q == 0 ? acc_g : q == 1 ? acc_b : q == 2 ? acc_d : acc_b2;
#pragma unroll
        for (int t = 0; t < 2; ++t) {
#pragma unroll
            for (int r = 0; r < 16; ++r) fold[wave][lane][16 * t + r] = src[t][r];
        }
        __syncthreads();
        if (tid < SH) {
            const int t = tid >> 5, w = tid & 31, uh = (w >> 2) & 1, r = 4 * (w >> 3) + (w & 3);
            float sum = 0.0f;
            for (int wv = 0; wv < AM_W; ++wv)
                for (int ii = 0; ii < 32; ++ii) sum += fold[wv][32 * uh + ii][16 * t + r];
            out[q * SH + tid] = sum;
        }
        __syncthreads();
    }
    // d_fc3_b: lane half hh of a row holds its d_means 4 hh .. 4 hh + 3
#pragma unroll
    for (int j = 0; j < 4; ++j) fold[wave][lane][j] = acc_b3[j];
    __syncthreads();
    if (tid < SH) {
        float sum = 0.0f;
        if (tid < FLEXNET_MAX_ACT) {
            for (int wv = 0; wv < AM_W; ++wv)
                for (int ii = 0; ii < 32; ++ii) sum += fold[wv][32 * (tid >> 2) + ii][tid & 3];
        }
        out[4 * SH + tid] = sum;
    }
}

__global__ __launch_bounds__(64 * AM_W) void actor_mlp_backward_kernel(FlexActorMlpBwdArgs a, int blocks_per_agent) {
    am_backward(a, blocks_per_agent);
}
__global__ __launch_bounds__(64 * AM_W) void mlp_unshared_actor_backward_kernel(FlexActorMlpUnsharedBwdArgs a, int blocks_per_agent) {
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

// Per-agent weights, element ex of every work-group's partial row of ONE agent: block = AM_VECS * agent + vector (vector 2, the
// sum of dz1 over the agent's rows, is its d_fc1_b)
__global__ __launch_bounds__(64 * FLEX_RED_G) void mlp_unshared_actor_reduce_kernel(FlexActorMlpUnsharedBwdArgs a, int blocks_per_agent) {
    const int ex = threadIdx.x & 63;
    const int ag = blockIdx.x / AM_VECS, vec = blockIdx.x % AM_VECS;
    float sum;
    if (!flex_reduce_rows(a.workspace + (int64_t)ag * blocks_per_agent * AM_PITCH + vec * SH + ex, AM_PITCH, blocks_per_agent,
                          true, sum))
        return;
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
    const int64_t batch = a->rows / a->n_agents;
    const int64_t groups = ((batch + 31) / 32 + AM_W - 1) / AM_W;
    hipLaunchKernelGGL(actor_mlp_forward_kernel, dim3((unsigned)(groups * a->n_agents)), dim3(64 * AM_W), 0,
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
    const int64_t batch = a->rows / a->n_agents;
    int64_t bpa = ((batch + 31) / 32 + AM_W - 1) / AM_W;
    if (bpa > AM_MAX_BLOCKS) bpa = AM_MAX_BLOCKS;
    if (bpa * a->n_agents * AM_PITCH > a->workspace_floats) return FLEXNET_EINVAL;
    if (!(flex_aligned(a->z1, 16) && flex_aligned(a->x, 16) && flex_aligned(a->h, 16) && flex_aligned(a->dz1, 16) &&
          flex_aligned(a->dz2, 16) && flex_aligned(a->d_h, 16)))
        return FLEXNET_EUNSUPPORTED;
    if (a->rows == 0) return FLEXNET_OK;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(actor_mlp_backward_kernel, dim3((unsigned)(bpa * a->n_agents)), dim3(64 * AM_W), 0, s, *a, (int)bpa);
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
    const int64_t batch = a->rows / a->n_agents;
    const int64_t groups = ((batch + 31) / 32 + AM_W - 1) / AM_W;
    hipLaunchKernelGGL(mlp_unshared_actor_forward_kernel, dim3((unsigned)(groups * a->n_agents)), dim3(64 * AM_W), 0,
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
    const int64_t batch = a->rows / a->n_agents;
    int64_t bpa = ((batch + 31) / 32 + AM_W - 1) / AM_W;
    if (bpa > AM_MAX_BLOCKS) bpa = AM_MAX_BLOCKS;
    if (bpa * a->n_agents * AM_PITCH > a->workspace_floats) return FLEXNET_EINVAL;
    if (!(flex_aligned(a->z1, 16) && flex_aligned(a->x, 16) && flex_aligned(a->h, 16) && flex_aligned(a->dz1, 16) &&
          flex_aligned(a->dz2, 16) && flex_aligned(a->d_h, 16)))
        return FLEXNET_EUNSUPPORTED;
    if (a->rows == 0) return FLEXNET_OK;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(mlp_unshared_actor_backward_kernel, dim3((unsigned)(bpa * a->n_agents)), dim3(64 * AM_W), 0, s, *a, (int)bpa);
    hipLaunchKernelGGL(mlp_unshared_actor_reduce_kernel, dim3(AM_VECS * a->n_agents), dim3(64 * FLEX_RED_G), 0, s, *a, (int)bpa);
    return flex_launch_status();
}
