// critic_unshared_stages.h — the stages critic_unshared.hip and critic_unshared_twin.hip share, on flex_agent_tile.h's work map
// and in its idiom: functions on tiles and plain pointers, no argument struct, no LDS of their own (the kernel declares its
// buffers and passes them); where the two families differ the difference is a template bool or an argument.  A critic head
// is LayerNorm, ReLU, fc2, ReLU, fc3 on a first-layer output: the plain kernels run one per row, the twin kernels one per
// head of a row, so a head's backward up to dx, the own-block product behind it and the work-group's prologue and d_fc3_b
// fold are written once here.  Every stage keeps the statements of the kernel bodies it was cut from in their order: each
// element's fp32 chain is the same sequence of operations.  Then the entry points' argument checks, as templates over the
// argument struct.
// (The FORWARD's head — ten lines behind the first layer — stays in each forward kernel.  The compiler finishes a function
// before it inlines it: fc3's weights are then addressed from one base with constant offsets, no longer through the unit
// indices LayerNorm's loads already hold, and critic_unshared_forward_kernel comes out at 124 registers and three
// wavefronts per SIMD where it has 155 and two — another kernel, with another speed, and not this header's business.)
#ifndef CRITIC_UNSHARED_STAGES_H
#define CRITIC_UNSHARED_STAGES_H
#include "flexnet.h"
#include "flex_launch.h"
#include "flex_agent_tile.h"

#define CU_MAX_W1 (FLEXNET_MAX_AGENTS * FLEXNET_MAX_OBS)
#define CU_MAX_W2 (FLEXNET_MAX_AGENTS * FLEXNET_MAX_ACT)

// ---- backward ---------------------------------------------------------------------------------------------------------
// The agent's weights into LDS, by the whole work-group, with the barrier behind them: fc2_w into `s_buf` (rows for z2,
// columns for dx), the own-block columns of fc1_w (`own_cols` = fc1_w + the block's first column; `ld1` = fc1_w's row
// length) as s_own[u * 8 + c], zero past `ow`, the LayerNorm weight (ones without LayerNorm), fc2_b, fc3_w and — `s_flag` not
// NULL — fc1_w's last column.
__device__ __forceinline__ void cu_stage_agent(float* s_buf, float* s_own, float* s_lnw, float* s_b2, float* s_w3, float* s_flag,
                                               const float* fc1_w, const float* own_cols, int ld1, int ow, bool layernorm,
                                               const float* ln_w, const float* fc2_w, const float* fc2_b, const float* fc3_w,
                                               int tid) {
    at_stage_weight(s_buf, fc2_w, SH, tid);
    for (int idx = tid; idx < SH * FLEXNET_MAX_ACT; idx += 64 * AT_W) {
        const int u = idx >> 3, c = idx & 7;
        s_own[idx] = c < ow ? own_cols[(int64_t)u * ld1 + c] : 0.0f;
    }
    if (tid < SH) {
        s_lnw[tid] = layernorm ? ln_w[tid] : 1.0f;
        s_b2[tid] = fc2_b[tid];
        s_w3[tid] = fc3_w[tid];
        if (s_flag) s_flag[tid] = fc1_w[(int64_t)tid * ld1 + (ld1 - 1)];
    }
    __syncthreads();
}

template <class... P>
__device__ __forceinline__ void cu_zero_sums(P&... acc) {
#pragma unroll
    for (int t = 0; t < 2; ++t) ((acc[t] = zero_tile()), ...);
}

// z2 = fc2(x) again from the forward's ReLU output `XS`, dz2 = dq w3 [z2 > 0].  PG: the per-lane sums acc_w3 (d_fc3_w) and
// acc_b2 (d_fc2_b) are kept and dz2 is stored to `dz2_64`, its row.
template <bool PG>
__device__ __forceinline__ void cu_head_dz2(const tv16 (&XS)[2], float dqv, const float* s_buf, const float* s_b2,
                                            const float* s_w3, tv16 (&dz2)[2], tv16 (&acc_w3)[2], tv16 (&acc_b2)[2],
                                            float* dz2_64, int i, int h, bool ok) {
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        tv16 z2 = bias_tile(s_b2 + 32 * t, h);
        z2 = layer_tile(s_buf + (32 * t + i) * AT_WP + 4 * h, z2, XS[0], XS[1]);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const tv4 w3 = ld4(s_w3 + 32 * t + 8 * q + 4 * h);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int e = 4 * q + j;
                const float hv = fmaxf(z2[e], 0.0f);
                const float d = z2[e] > 0.0f ? dqv * w3[j] : 0.0f;
                dz2[t][e] = d;
                if (PG) {
                    acc_w3[t][e] = fmaf(dqv, hv, acc_w3[t][e]);
                    acc_b2[t][e] += d;
                }
            }
        }
        if (PG) store_tile(dz2_64 + 32 * t + 4 * h, dz2[t], ok);
    }
}

// dx = dz2 @ fc2_w from the LDS copy: never stored
__device__ __forceinline__ void cu_head_dx(const float* s_buf, const tv16 (&dz2)[2], tv16 (&dx)[2], int i, int h) {
    dx[0] = zero_tile();
    dx[1] = zero_tile();
#pragma unroll
    for (int to = 0; to < 2; ++to) {
        const float* wc = s_buf + (32 * to) * AT_WP + i;
        dx[0] = transposed_tile(wc, AT_WP, h, dx[0], dz2[to]);
        dx[1] = transposed_tile(wc + 32, AT_WP, h, dx[1], dz2[to]);
    }
}

// d_x2_own = dz1 @ the own-block columns (cu_stage_agent's s_own) -> `d_own`, the row's `ow` outputs: the A operand's rows
// past ow are zero; output c = 4 h + r sits in accumulator register r < 4
__device__ __forceinline__ void cu_own_block(const float* s_own, const tv16 (&dzv)[2], float* d_own, int ow, int i, int h,
                                             bool ok) {
    tv16 m = zero_tile();
    const bool live = i < FLEXNET_MAX_ACT;
    const float* wo = s_own + (live ? i : 0);
#pragma unroll
    for (int t = 0; t < 2; ++t) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float w = wo[(32 * t + 8 * q + 4 * h + j) * FLEXNET_MAX_ACT];
                m = TILE_MFMA(live ? w : 0.0f, dzv[t][4 * q + j], m);
            }
        }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int c = 4 * h + j;
        if (ok && c < ow) d_own[c] = m[j];
    }
}

// d_fc3_b behind at_fold, into `out_vec`, the work-group's last vector (element 0; the rest zero): both halves of a row hold
// its dq, half 0 counts
__device__ __forceinline__ void cu_fold_fc3_b(float (*fold)[64][AT_FOLD], float* out_vec, float acc_b3, int tid) {
    fold[tid >> 6][tid & 63][0] = acc_b3;
    __syncthreads();
    if (tid < SH) {
        float sum = 0.0f;
        if (tid == 0) {
            for (int wv = 0; wv < AT_W; ++wv)
                for (int ii = 0; ii < 32; ++ii) sum += fold[wv][ii][0];
        }
        out_vec[tid] = sum;
    }
}

// ---- the entry points' checks, in the order the two families answer them -------------------------------------------------
static inline int cu_check_shape(int rows, int n, int w1, int w2, int heads = 1) {
    if (rows < 0 || n < 1 || w1 < 1 || w2 < 0 || rows % n != 0 || heads < 1 || heads > 2) return FLEXNET_EINVAL;
    if (n > FLEXNET_MAX_AGENTS || w1 > CU_MAX_W1 || w2 > CU_MAX_W2) return FLEXNET_EUNSUPPORTED;
    return FLEXNET_OK;
}

// a forward's arguments, up to the launch (A: FlexCriticUnsharedArgs / FlexCriticUnsharedTwinArgs)
template <class A>
static int cu_check_forward(const A* a, int heads = 1) {
    if (!a->x1 || !a->q || (a->w2 > 0 && !a->x2)) return FLEXNET_EINVAL;
    if (a->x1_pitch < 0 || a->x2_pitch < 0 || a->x1_agent_off < 0 || a->x2_agent_off < 0) return FLEXNET_EINVAL;
    const int rc = cu_check_shape(a->rows, a->n_agents, a->w1, a->w2, heads);
    if (rc != FLEXNET_OK) return rc;
    bool aligned = true;
    for (int k = 0; k < a->n_agents; ++k) {
        if (!a->fc1_w[k] || !a->fc1_b[k] || !a->fc2_w[k] || !a->fc2_b[k] || !a->fc3_w[k] || !a->fc3_b[k] ||
            (a->layernorm && (!a->ln_w[k] || !a->ln_b[k])))
            return FLEXNET_EINVAL;
        aligned = aligned && flex_aligned(a->fc2_w[k], 16);
    }
    if ((a->save_z1 != nullptr) != (a->save_x != nullptr)) return FLEXNET_EINVAL;       // both or none
    if (a->save_z1) aligned = aligned && flex_aligned(a->save_z1, 16) && flex_aligned(a->save_x, 16);
    return aligned ? FLEXNET_OK : FLEXNET_EUNSUPPORTED;
}

// a backward's arguments, up to the empty batch (A: the two BwdArgs): `dz1` = the struct's first-layer gradient output,
// `more_sums` = the parameter-gradient buffers only this family has are all there
template <class A>
static int cu_check_backward(const A* a, const float* dz1, bool more_sums = true, int heads = 1) {
    if (!a->dq || !a->z1 || !a->x || !dz1) return FLEXNET_EINVAL;
    const bool pg = a->param_grads != 0;
    if (pg && (!a->dz2 || !a->d_fc1_b || !a->d_fc2_b || !a->d_fc3_w || !a->d_fc3_b || !more_sums || !a->workspace ||
               (a->layernorm && (!a->d_ln_w || !a->d_ln_b))))
        return FLEXNET_EINVAL;
    const int rc = cu_check_shape(a->rows, a->n_agents, a->w1, a->w2, heads);
    if (rc != FLEXNET_OK) return rc;
    if (a->d_x2_own) {
        if (a->own_w < 1 || a->own_first < 0 || a->own_step < 0 ||
            a->own_first + (a->n_agents - 1) * a->own_step + a->own_w > a->w2)
            return FLEXNET_EINVAL;
        if (a->own_w > FLEXNET_MAX_ACT) return FLEXNET_EUNSUPPORTED;
    }
    const bool aligned = flex_aligned(a->z1, 16) && flex_aligned(a->x, 16) && flex_aligned(dz1, 16) && (!pg || flex_aligned(a->dz2, 16));
    for (int k = 0; k < a->n_agents; ++k) {
        if (!a->fc1_w[k] || !a->fc2_w[k] || !a->fc2_b[k] || !a->fc3_w[k] || (a->layernorm && !a->ln_w[k])) return FLEXNET_EINVAL;
    }
    return aligned ? FLEXNET_OK : FLEXNET_EUNSUPPORTED;
}

#endif
