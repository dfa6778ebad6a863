// attn_critic.hip — MAAC's attention critic (madrl/critics/maac_critic.py:86-159, continuous branch, one attention head, no
// input BatchNorm) for a whole batch in one launch per direction (gfx950).  Boundary: include/flexnet.h (FlexAttnCriticArgs /
// FlexAttnCriticBwdArgs).
//
// Work map: attention couples the agents of a sample, so one wavefront owns 32 SAMPLES with all their agents — rows
// r = s * n_agents + j of the [b * n, .] tensors — on flex_mfma_tile.h's transposed fp32 scheme; lane (sample i, half h) holds
// 32 of a row's 64 units.  A work-group is four independent wavefronts: no barrier, no LDS.
//
// Forward, two phases per wavefront.  Phase 1, per agent j: sa_j = LeakyReLU(enc_j [o_j | a_j]) with the observation and the
// action read as two blocks where the caller keeps them, key_j = K sa_j, val_j = LeakyReLU(V sa_j + b_V); the three go to the
// caller's staging tensors.  Phase 2, per agent i: s_i, sel_i = Q s_i, the logits sel_i . key_j over j != i (a per-lane
// 32-term sum plus the other half), softmax of the scaled logits with the maximum subtracted, other_i = sum_j w_ij val_j,
// q_i = critic_i([sa_i | other_i]), b_i = bias_i(s_i), out q_i - b_i.  Every lane reads back exactly the staging elements it
// wrote itself (the same units of the same rows), so the two phases need no synchronisation beyond a thread's own program
// order.  The regulariser's sums of squared unscaled logits leave as one partial per wavefront and agent and are summed in a
// fixed order by a second launch: no atomics, bit-reproducible.
//
// Backward, from dq [b, n] and the forward's saves, again two phases: per agent i the critic head back to d_sa_i (direct) and
// d_other_i, the softmax back to the logit gradients, and with param_grads the selector / state-encoder / bias-head path; per
// agent j the gradients every OTHER agent's attention sent to key_j and val_j, gathered by loads (no read-modify-write), and
// the encoder's pre-activation gradient.  param_grads = 1 emits the gradients at the seven pre-activations for
// flexnet_wgrad_batched (whose column sums are the [64] bias gradients) and the two output layers' bias gradients, +- the sum of
// dq over the samples, through one fp64 partial per wavefront and a second launch; param_grads = 0 emits d_act alone.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "flexnet.h"
#include "flex_launch.h"
#include "flex_mfma_tile.h"
#include "flex_reduce.h"

#define AC_W 4                                   // wavefronts per work-group (one per SIMD)
#define AC_SLOPE 0.01f                           // nn.LeakyReLU()'s negative slope
#define AC_SCALE 0.125f                          // 1 / sqrt(64): the key size of the one head

__device__ __forceinline__ float attn_critic_lrelu(float x) { return x > 0.0f ? x : x * AC_SLOPE; }
__device__ __forceinline__ float attn_critic_slope(float y) { return y > 0.0f ? 1.0f : AC_SLOPE; }      // from the OUTPUT's sign

// The FORWARD's dot products are no single fp32 chain.  The softmax carries a logit's rounding into the attention weights
// (times 8 at unit-scale logits, times 64 and more between near-tied saturated ones), and the logit is the end of three chained
// layers (encoder, extractor, sel . key), each of which would add a K-term chain's rounding.  So every group of four MFMA steps
// (eight terms) starts from zero and is folded into an fp64 sum per unit: a layer's output is the fp32 rounding of a sum whose
// own error is that of eight-term chains.  (v_mfma_f32_32x32x2_f32 itself is exact fp32; the fold is VALU work beside it.)
struct dv16 {                                    // (sixteen separate doubles, not one 32-register tuple)
    double v[16];
    __device__ __forceinline__ double& operator[](int r) { return v[r]; }
    __device__ __forceinline__ const double& operator[](int r) const { return v[r]; }
};

__device__ __forceinline__ dv16 attn_critic_dzero() {
    dv16 t;
#pragma unroll
    for (int r = 0; r < 16; ++r) t[r] = 0.0;
    return t;
}

__device__ __forceinline__ void attn_critic_fold(dv16& sum, const tv16& part) {
#pragma unroll
    for (int r = 0; r < 16; ++r) sum[r] += (double)part[r];
}

__device__ __forceinline__ double other_half_d(double v) { return __shfl_xor(v, 32, 64); }

// x += W[:, c0 .. c0 + width) @ xp[0 .. width) for the lane's row: MFMA step j of a group of eight columns takes the pair
// (c + j, c + 4 + j); `w0` / `w1` = the lane's two weight rows at the block's first column.  (Clamped: no load past a row.)
__device__ __forceinline__ void attn_critic_block(dv16* x, const float* xp, const float* w0, const float* w1, int width, int h) {
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
        tv16 p0 = zero_tile(), p1 = zero_tile();
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            p0 = TILE_MFMA(wa[j], o[j], p0);
            p1 = TILE_MFMA(wb[j], o[j], p1);
        }
        attn_critic_fold(x[0], p0);
        attn_critic_fold(x[1], p1);
        __builtin_amdgcn_sched_barrier(0);                     // (one group's partials live at a time: no spills)
    }
}

// acc += W[32 outputs, 64 columns] @ in, folded every eight terms (layer_tile's operand order).  `wrow` as layer_tile's.
__device__ __forceinline__ void attn_critic_tile(dv16& acc, const float* wrow, const tv16& in0, const tv16& in1) {
#pragma unroll
    for (int kt = 0; kt < 2; ++kt) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const tv4 w = ld4(wrow + 32 * kt + 8 * q);
            tv16 p = zero_tile();
#pragma unroll
            for (int j = 0; j < 4; ++j) p = TILE_MFMA(w[j], kt ? in1[4 * q + j] : in0[4 * q + j], p);
            attn_critic_fold(acc, p);
            __builtin_amdgcn_sched_barrier(0);                 // (one group's partial live at a time: no spills)
        }
    }
}

__device__ __forceinline__ void attn_critic_load(tv16* t, const float* row, int h) {
    t[0] = load_tile(row + 4 * h);
    t[1] = load_tile(row + 32 + 4 * h);
}

__device__ __forceinline__ void attn_critic_store(float* row, const tv16* t, int h, bool ok) {
    store_tile(row + 4 * h, t[0], ok);
    store_tile(row + 32 + 4 * h, t[1], ok);
}

// the lane's row of x . y over its 64 units (both halves end with the same number)
__device__ __forceinline__ float attn_critic_dot(const tv16* x, const tv16* y) {
    float p = 0.0f;
#pragma unroll
    for (int t = 0; t < 2; ++t) {
#pragma unroll
        for (int r = 0; r < 16; ++r) p = fmaf(x[t][r], y[t][r], p);
    }
    return p + other_half(p);
}

// ... summed in fp64 (the forward's logits): what is left is each product's own fp32 rounding, not a 32-term chain's
__device__ __forceinline__ double attn_critic_dot_d(const tv16* x, const tv16* y) {
    double p = 0.0;
#pragma unroll
    for (int t = 0; t < 2; ++t) {
#pragma unroll
        for (int r = 0; r < 16; ++r) p += (double)(x[t][r] * y[t][r]);
    }
    return p + other_half_d(p);
}

// out = W [64, 64 columns at pitch ld] @ in (+ bias, or none), both tiles: the forward's folded sums, rounded once
__device__ __forceinline__ void attn_critic_layer(tv16* out, const float* W, int ld, const float* bias, const tv16* in, int i, int h) {
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        dv16 acc = attn_critic_dzero();
        attn_critic_tile(acc, W + (int64_t)(32 * t + i) * ld + 4 * h, in[0], in[1]);
#pragma unroll
        for (int r = 0; r < 16; ++r) out[t][r] = (float)(bias ? acc[r] + (double)bias[32 * t + TILE_U(r, h)] : acc[r]);
    }
}

// acc += W[:, k0 .. k0 + 64)^T @ d for W [64, ld]: the input gradient of a layer, both tiles
__device__ __forceinline__ void attn_critic_layer_t(tv16* acc, const float* W, int ld, int k0, const tv16* d, int i, int h) {
#pragma unroll
    for (int to = 0; to < 2; ++to) {
        const float* wc = W + (int64_t)(32 * to) * ld + k0 + i;
        acc[0] = transposed_tile(wc, ld, h, acc[0], d[to]);
        acc[1] = transposed_tile(wc + 32, ld, h, acc[1], d[to]);
    }
}

// (one kernel with or without the saves: the no-grad launch and the training forward give the same bits)
__global__ __launch_bounds__(64 * AC_W) void attn_critic_forward_kernel(FlexAttnCriticArgs a) {
    const bool SAVE = a.save_s != nullptr;
    const int n = a.n_agents, o = a.obs_dim, ad = a.act_dim, ld = o + ad;
    const int64_t tile = (int64_t)blockIdx.x * AC_W + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);     // (scalar)
    const int64_t s0 = tile * 32;
    if (s0 >= a.batch) return;                                 // (the kernel has no barrier)
    // The lane's indices are formed anew, from the lane counter itself, for every agent of either phase: then no vector register
    // lives through both loops, and the dozen 64-bit row addresses derived from the indices are formed where they are used —
    // carried along, they would spill.  The last partial tile re-reads a valid sample.
#define AC_LANE()                                                                  \
    int lane;                                                                      \
    __asm__ volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(lane));   \
    const int i = lane & 31, h = lane >> 5;                                         \
    const bool ok = s0 + i < a.batch;                                              \
    const int64_t s = ok ? s0 + i : a.batch - 1

    // phase 1: every agent's encoding, key and value
#pragma unroll 1
    for (int j = 0; j < n; ++j) {
        AC_LANE();
        const int64_t row = s * n + j;
        // (the shared extractors' row addresses are formed anew per agent: hoisted out of the loop, the lane's sixteen 64-bit
        // addresses per matrix are what would spill)
        const float* key_w = a.key_w;
        const float* val_w = a.val_w;
        __asm__ volatile("" : "+s"(key_w), "+s"(val_w));
        const float* W = a.enc_w[j];
        const float* b = a.enc_b[j];
        dv16 xd[2] = {attn_critic_dzero(), attn_critic_dzero()};
        attn_critic_block(xd, a.obs + row * o, W + (int64_t)i * ld, W + (int64_t)(32 + i) * ld, o, h);
        attn_critic_block(xd, a.act + row * ad, W + (int64_t)i * ld + o, W + (int64_t)(32 + i) * ld + o, ad, h);
        tv16 x[2];
#pragma unroll
        for (int t = 0; t < 2; ++t) {
#pragma unroll
            for (int r = 0; r < 16; ++r) x[t][r] = attn_critic_lrelu((float)(xd[t][r] + (double)b[32 * t + TILE_U(r, h)]));
        }
        attn_critic_store(a.sa + row * SH, x, h, ok);
        tv16 y[2];
        attn_critic_layer(y, key_w, SH, nullptr, x, i, h);
        attn_critic_store(a.key + row * SH, y, h, ok);
        attn_critic_layer(y, val_w, SH, a.val_b, x, i, h);
#pragma unroll
        for (int t = 0; t < 2; ++t) {
#pragma unroll
            for (int r = 0; r < 16; ++r) y[t][r] = attn_critic_lrelu(y[t][r]);
        }
        attn_critic_store(a.val + row * SH, y, h, ok);
    }

    // phase 2: every agent's attention over the others, its critic head and its bias head
#pragma unroll 1
    for (int ai = 0; ai < n; ++ai) {
        __asm__ volatile("" ::: "memory");
        AC_LANE();
        const int64_t row = s * n + ai;
        tv16 sx[2];
        {
            const float* W = a.senc_w[ai];
            const float* b = a.senc_b[ai];
            dv16 xd[2] = {attn_critic_dzero(), attn_critic_dzero()};
            attn_critic_block(xd, a.obs + row * o, W + (int64_t)i * o, W + (int64_t)(32 + i) * o, o, h);
#pragma unroll
            for (int t = 0; t < 2; ++t) {
#pragma unroll
                for (int r = 0; r < 16; ++r) sx[t][r] = attn_critic_lrelu((float)(xd[t][r] + (double)b[32 * t + TILE_U(r, h)]));
            }
        }
        tv16 sel[2];
        const float* sel_w = a.sel_w;
        __asm__ volatile("" : "+s"(sel_w));                    // (as the key and value extractors above)
        attn_critic_layer(sel, sel_w, SH, nullptr, sx, i, h);
        if (SAVE) attn_critic_store(a.save_sel + row * SH, sel, h, ok);
        // the bias head on s_i
        double bp = 0.0;
        {
            const float* W = a.b1_w[ai];
            const float* b = a.b1_b[ai];
            const float* w2 = a.b2_w[ai];
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                dv16 acc = attn_critic_dzero();
                attn_critic_tile(acc, W + (int64_t)(32 * t + i) * SH + 4 * h, sx[0], sx[1]);
                tv16 z;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    z[r] = attn_critic_lrelu((float)(acc[r] + (double)b[32 * t + TILE_U(r, h)]));
                    bp = fma((double)w2[32 * t + TILE_U(r, h)], (double)z[r], bp);
                }
                if (SAVE) store_tile(a.save_hb + row * SH + 32 * t + 4 * h, z, ok);
            }
        }
        const double bias = (bp + other_half_d(bp)) + (double)a.b2_b[ai][0];
        if (SAVE) attn_critic_store(a.save_s + row * SH, sx, h, ok);
        // the logits and their distance to the largest stay in fp64: between near-tied saturated logits the difference is
        // all that matters, and it is far below an fp32 ulp of either
        float l[FLEXNET_MAX_AGENTS];
        double pd[FLEXNET_MAX_AGENTS];
        float regp = 0.0f;
        double mx = -1.0e300;
#pragma unroll
        for (int j = 0; j < FLEXNET_MAX_AGENTS; ++j) {
            l[j] = 0.0f;
            pd[j] = 0.0;
            if (j < n && j != ai) {
                tv16 k[2];
                attn_critic_load(k, a.key + (s * n + j) * SH, h);
                pd[j] = attn_critic_dot_d(sel, k);
                const float p = (float)pd[j];
                regp = fmaf(p, p, regp);
                mx = fmax(mx, pd[j]);
            }
            __builtin_amdgcn_sched_barrier(0);                 // (one agent's key tiles live at a time)
        }
        float den = 0.0f;
#pragma unroll
        for (int j = 0; j < FLEXNET_MAX_AGENTS; ++j) {
            if (j < n && j != ai) {
                l[j] = expf((float)((pd[j] - mx) * (double)AC_SCALE));
                den += l[j];
            }
        }
        const float inv = 1.0f / den;
        tv16 oth[2] = {zero_tile(), zero_tile()};
#pragma unroll
        for (int j = 0; j < FLEXNET_MAX_AGENTS; ++j) {
            if (j < n && j != ai) {
                l[j] *= inv;
                tv16 v[2];
                attn_critic_load(v, a.val + (s * n + j) * SH, h);
#pragma unroll
                for (int t = 0; t < 2; ++t) {
#pragma unroll
                    for (int r = 0; r < 16; ++r) oth[t][r] = fmaf(l[j], v[t][r], oth[t][r]);
                }
            }
            __builtin_amdgcn_sched_barrier(0);                 // (one agent's value tiles live at a time)
            if (SAVE && ok && j < n) a.save_w[(s * n + ai) * n + j] = l[j];        // (both halves: the same number)
        }
        if (SAVE) attn_critic_store(a.save_other + row * SH, oth, h, ok);
        tv16 sa[2];
        attn_critic_load(sa, a.sa + row * SH, h);
        // the critic head on [sa_i | other_i]
        double qp = 0.0;
        {
            const float* W = a.c1_w[ai];
            const float* b = a.c1_b[ai];
            const float* w2 = a.c2_w[ai];
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                dv16 acc = attn_critic_dzero();
                attn_critic_tile(acc, W + (int64_t)(32 * t + i) * (2 * SH) + 4 * h, sa[0], sa[1]);
                attn_critic_tile(acc, W + (int64_t)(32 * t + i) * (2 * SH) + SH + 4 * h, oth[0], oth[1]);
                tv16 z;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    z[r] = attn_critic_lrelu((float)(acc[r] + (double)b[32 * t + TILE_U(r, h)]));
                    qp = fma((double)w2[32 * t + TILE_U(r, h)], (double)z[r], qp);
                }
                if (SAVE) store_tile(a.save_hc + row * SH + 32 * t + 4 * h, z, ok);
            }
        }
        const double q = (qp + other_half_d(qp)) + (double)a.c2_b[ai][0];
        if (ok && h == 0) a.q[row] = (float)(q - bias);
        // the regulariser's partial: the live samples of this wavefront, one half of each row
        const float total = flex_wave_sum(ok && h == 0 ? regp : 0.0f);
        if (lane == 0) a.workspace[tile * n + ai] = total;
    }
}
#undef AC_LANE

// reg[i] = 1e-3 * (sum over the wavefronts' partials, in index order) / (b (n - 1)): one work-group
__global__ __launch_bounds__(64 * FLEX_RED_G) void attn_critic_reg_kernel(FlexAttnCriticArgs a, int tiles) {
    const int ex = threadIdx.x & 63;
    const bool active = ex < a.n_agents;
    float sum;
    if (!flex_reduce_rows(a.workspace + (active ? ex : 0), a.n_agents, tiles, active, sum)) return;
    a.reg[ex] = 1.0e-3f * (sum / ((float)a.batch * (float)(a.n_agents - 1)));
}

// ---- backward ---------------------------------------------------------------------------------------------------------
// PG: the gradients at the seven pre-activations (the value loss); without, d_act alone (the policy loss, critic frozen)
template <bool PG>
__global__ __launch_bounds__(64 * AC_W) void attn_critic_backward_kernel(FlexAttnCriticBwdArgs a) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, i = lane & 31, h = lane >> 5;
    const int n = a.n_agents, o = a.obs_dim, ad = a.act_dim, ld = o + ad;
    const int64_t tile = (int64_t)blockIdx.x * AC_W + wave;
    const int64_t s0 = tile * 32;
    if (s0 >= a.batch) return;                                 // (the kernel has no barrier)
    const bool ok = s0 + i < a.batch;
    const int64_t s = ok ? s0 + i : a.batch - 1;

    // phase A, per agent i: the critic head back to d_sa_i (direct) and d_other_i, the softmax back to the logits
#pragma unroll 1
    for (int ai = 0; ai < n; ++ai) {
        __asm__ volatile("" ::: "memory");
        const int64_t row = s * n + ai;
        const float dqv = ok ? a.dq[row] : 0.0f;               // a dead row's dq is zero: so is everything below
        tv16 dzc[2];
        {
            tv16 hc[2];
            attn_critic_load(hc, a.hc + row * SH, h);
            const float* w2 = a.c2_w[ai];
#pragma unroll
            for (int t = 0; t < 2; ++t) {
#pragma unroll
                for (int r = 0; r < 16; ++r) dzc[t][r] = dqv * w2[32 * t + TILE_U(r, h)] * attn_critic_slope(hc[t][r]);
            }
        }
        if (PG) {
            attn_critic_store(a.dz_c + row * SH, dzc, h, ok);
            // the output layers' bias gradients are +- the sum of dq over the samples: one fp64 partial per wavefront and agent
            // (a sum of signed terms far larger than their total: fp32 partial sums would each round at the terms' scale)
            double total = h == 0 ? (double)dqv : 0.0;
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) total += __shfl_xor(total, off, 64);
            if (lane == 0) reinterpret_cast<double*>(a.workspace)[tile * n + ai] = total;
        }
        tv16 dsa[2] = {zero_tile(), zero_tile()}, dot[2] = {zero_tile(), zero_tile()};
        attn_critic_layer_t(dsa, a.c1_w[ai], 2 * SH, 0, dzc, i, h);
        attn_critic_layer_t(dot, a.c1_w[ai], 2 * SH, SH, dzc, i, h);
        attn_critic_store(a.g_direct + row * SH, dsa, h, ok);
        attn_critic_store(a.g_other + row * SH, dot, h, ok);
        // d w_ij = d_other_i . val_j, parked in g_dl;  d l_ij = w_ij (d w_ij - sum_k w_ik d w_ik) / sqrt(64) replaces it below
        // (every lane reads back what it wrote itself; both halves of a row write the same number)
        float mean = 0.0f;
#pragma unroll 1
        for (int j = 0; j < n; ++j) {
            if (j == ai) continue;
            tv16 v[2];
            attn_critic_load(v, a.val + (s * n + j) * SH, h);
            const float dw = attn_critic_dot(dot, v);
            mean = fmaf(a.w[(s * n + ai) * n + j], dw, mean);
            if (ok) a.g_dl[(s * n + ai) * n + j] = dw;
        }
        if (PG) {
            // the selector, the bias head and the state encoder
            tv16 dsel[2] = {zero_tile(), zero_tile()};
#pragma unroll 1
            for (int j = 0; j < n; ++j) {
                if (j == ai) continue;
                const int64_t at = (s * n + ai) * n + j;
                const float dl = ok ? a.w[at] * (a.g_dl[at] - mean) * AC_SCALE : 0.0f;
                if (ok) a.g_dl[at] = dl;
                tv16 k[2];
                attn_critic_load(k, a.key + (s * n + j) * SH, h);
#pragma unroll
                for (int t = 0; t < 2; ++t) {
#pragma unroll
                    for (int r = 0; r < 16; ++r) dsel[t][r] = fmaf(dl, k[t][r], dsel[t][r]);
                }
            }
            attn_critic_store(a.d_sel + row * SH, dsel, h, ok);
            tv16 dzb[2];
            {
                tv16 hb[2];
                attn_critic_load(hb, a.hb + row * SH, h);
                const float* w2 = a.b2_w[ai];
#pragma unroll
                for (int t = 0; t < 2; ++t) {
#pragma unroll
                    for (int r = 0; r < 16; ++r) dzb[t][r] = -dqv * w2[32 * t + TILE_U(r, h)] * attn_critic_slope(hb[t][r]);
                }
            }
            attn_critic_store(a.dz_b + row * SH, dzb, h, ok);
            tv16 ds[2] = {zero_tile(), zero_tile()};
            attn_critic_layer_t(ds, a.sel_w, SH, 0, dsel, i, h);
            attn_critic_layer_t(ds, a.b1_w[ai], SH, 0, dzb, i, h);
            tv16 sx[2];
            attn_critic_load(sx, a.s + row * SH, h);
#pragma unroll
            for (int t = 0; t < 2; ++t) {
#pragma unroll
                for (int r = 0; r < 16; ++r) ds[t][r] *= attn_critic_slope(sx[t][r]);
            }
            attn_critic_store(a.dz_s + row * SH, ds, h, ok);
        } else {
#pragma unroll 1
            for (int j = 0; j < n; ++j) {
                if (j == ai) continue;
                const int64_t at = (s * n + ai) * n + j;
                if (ok) a.g_dl[at] = a.w[at] * (a.g_dl[at] - mean) * AC_SCALE;
            }
        }
    }

    // phase B, per agent j: what the other agents' attention sent to key_j and val_j, then the encoder
#pragma unroll 1
    for (int j = 0; j < n; ++j) {
        __asm__ volatile("" ::: "memory");
        const int64_t row = s * n + j;
        tv16 dval[2] = {zero_tile(), zero_tile()}, dkey[2] = {zero_tile(), zero_tile()};
#pragma unroll 1
        for (int ai = 0; ai < n; ++ai) {
            if (ai == j) continue;
            const float wij = a.w[(s * n + ai) * n + j], dlij = ok ? a.g_dl[(s * n + ai) * n + j] : 0.0f;
            tv16 g[2], q[2];
            attn_critic_load(g, a.g_other + (s * n + ai) * SH, h);
            attn_critic_load(q, a.sel + (s * n + ai) * SH, h);
#pragma unroll
            for (int t = 0; t < 2; ++t) {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    dval[t][r] = fmaf(wij, g[t][r], dval[t][r]);
                    dkey[t][r] = fmaf(dlij, q[t][r], dkey[t][r]);
                }
            }
        }
        {
            tv16 v[2];
            attn_critic_load(v, a.val + row * SH, h);
#pragma unroll
            for (int t = 0; t < 2; ++t) {
#pragma unroll
                for (int r = 0; r < 16; ++r) dval[t][r] *= attn_critic_slope(v[t][r]);
            }
        }
        if (PG) {
            attn_critic_store(a.d_key + row * SH, dkey, h, ok);
            attn_critic_store(a.dz_v + row * SH, dval, h, ok);
        }
        tv16 dsa[2];
        attn_critic_load(dsa, a.g_direct + row * SH, h);
        attn_critic_layer_t(dsa, a.key_w, SH, 0, dkey, i, h);
        attn_critic_layer_t(dsa, a.val_w, SH, 0, dval, i, h);
        {
            tv16 sa[2];
            attn_critic_load(sa, a.sa + row * SH, h);
#pragma unroll
            for (int t = 0; t < 2; ++t) {
#pragma unroll
                for (int r = 0; r < 16; ++r) dsa[t][r] *= attn_critic_slope(sa[t][r]);
            }
        }
        if (PG) {
            attn_critic_store(a.dz_sa + row * SH, dsa, h, ok);
        } else {
            // d_act_j = dz_sa_j @ the action columns of enc_j: the A operand's rows past act_dim are zero; output c = 4 h + r
            // sits in accumulator register r < 4
            tv16 m = zero_tile();
            const bool live = i < ad;
            const float* wo = a.enc_w[j] + o + (live ? i : 0);
#pragma unroll
            for (int t = 0; t < 2; ++t) {
#pragma unroll
                for (int q = 0; q < 4; ++q) {
#pragma unroll
                    for (int jj = 0; jj < 4; ++jj) {
                        const float wv = wo[(int64_t)(32 * t + 8 * q + 4 * h + jj) * ld];
                        m = TILE_MFMA(live ? wv : 0.0f, dsa[t][4 * q + jj], m);
                    }
                }
            }
#pragma unroll
            for (int jj = 0; jj < 4; ++jj) {
                const int c = 4 * h + jj;
                if (ok && c < ad) a.d_act[row * ad + c] = m[jj];
            }
        }
    }
}

// d_c2_b[i] = the sum of the wavefronts' fp64 partials of dq[:, i], d_b2_b[i] = minus it (out = q - b): one work-group per
// agent, strided sums folded by a halving tree through LDS — a fixed order
#define AC_SUM_T 256
__global__ __launch_bounds__(AC_SUM_T) void attn_critic_dq_sum_kernel(FlexAttnCriticBwdArgs a, int tiles) {
    __shared__ double red[AC_SUM_T];
    const int tid = threadIdx.x, ag = blockIdx.x;
    const double* p = reinterpret_cast<const double*>(a.workspace) + ag;
    double t = 0.0;
    for (int k = tid; k < tiles; k += AC_SUM_T) t += p[(int64_t)k * a.n_agents];
    red[tid] = t;
    __syncthreads();
    for (int sft = AC_SUM_T / 2; sft > 0; sft >>= 1) {
        if (tid < sft) red[tid] += red[tid + sft];
        __syncthreads();
    }
    if (tid == 0) {
        a.d_c2_b[ag] = (float)red[0];
        a.d_b2_b[ag] = -(float)red[0];
    }
}

// ---- entry points -----------------------------------------------------------------------------------------------------
static int attn_critic_check_shape(int64_t batch, int n, int o, int ad) {
    if (batch < 0 || n < 1 || o < 1 || ad < 1) return FLEXNET_EINVAL;
    if (n < 2 || n > FLEXNET_MAX_AGENTS || o > FLEXNET_MAX_OBS || o % 4 != 0 || ad > FLEXNET_MAX_ACT ||
        batch > FLEXNET_ATTN_CRITIC_MAX_BATCH)
        return FLEXNET_EUNSUPPORTED;
    return FLEXNET_OK;
}

extern "C" int flexnet_attn_critic_forward(const FlexAttnCriticArgs* a, void* stream) {
    if (!a) return FLEXNET_EINVAL;
    if (!a->obs || !a->act || !a->key_w || !a->sel_w || !a->val_w || !a->val_b || !a->sa || !a->key || !a->val || !a->q ||
        !a->reg || !a->workspace)
        return FLEXNET_EINVAL;
    const int rc = attn_critic_check_shape(a->batch, a->n_agents, a->obs_dim, a->act_dim);
    if (rc != FLEXNET_OK) return rc;
    bool aligned = flex_aligned(a->key_w, 16) && flex_aligned(a->sel_w, 16) && flex_aligned(a->val_w, 16) &&
                   flex_aligned(a->sa, 16) && flex_aligned(a->key, 16) && flex_aligned(a->val, 16);
    for (int k = 0; k < a->n_agents; ++k) {
        if (!a->enc_w[k] || !a->enc_b[k] || !a->senc_w[k] || !a->senc_b[k] || !a->c1_w[k] || !a->c1_b[k] || !a->c2_w[k] ||
            !a->c2_b[k] || !a->b1_w[k] || !a->b1_b[k] || !a->b2_w[k] || !a->b2_b[k])
            return FLEXNET_EINVAL;
        aligned = aligned && flex_aligned(a->c1_w[k], 16) && flex_aligned(a->b1_w[k], 16);
    }
    const int saves = (a->save_s != nullptr) + (a->save_sel != nullptr) + (a->save_other != nullptr) + (a->save_hc != nullptr) +
                      (a->save_hb != nullptr) + (a->save_w != nullptr);
    if (saves != 0 && saves != 6) return FLEXNET_EINVAL;                               // all or none
    if (saves)
        aligned = aligned && flex_aligned(a->save_s, 16) && flex_aligned(a->save_sel, 16) && flex_aligned(a->save_other, 16) &&
                  flex_aligned(a->save_hc, 16) && flex_aligned(a->save_hb, 16);
    const int64_t tiles = (a->batch + 31) / 32;
    if (a->workspace_floats < tiles * a->n_agents) return FLEXNET_EINVAL;
    if (!aligned) return FLEXNET_EUNSUPPORTED;
    if (a->batch == 0) return FLEXNET_OK;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(attn_critic_forward_kernel, dim3((unsigned)((tiles + AC_W - 1) / AC_W)), dim3(64 * AC_W), 0, s, *a);
    hipLaunchKernelGGL(attn_critic_reg_kernel, dim3(1), dim3(64 * FLEX_RED_G), 0, s, *a, (int)tiles);
    return flex_launch_status();
}

extern "C" int flexnet_attn_critic_backward(const FlexAttnCriticBwdArgs* a, void* stream) {
    if (!a) return FLEXNET_EINVAL;
    if (!a->dq || !a->sa || !a->key || !a->val || !a->sel || !a->hc || !a->w || !a->key_w || !a->val_w || !a->g_direct ||
        !a->g_other || !a->g_dl)
        return FLEXNET_EINVAL;
    const bool pg = a->param_grads != 0;
    if (pg && (!a->s || !a->hb || !a->sel_w || !a->dz_c || !a->dz_b || !a->dz_s || !a->d_sel || !a->d_key || !a->dz_v || !a->dz_sa ||
               !a->d_c2_b || !a->d_b2_b || !a->workspace))
        return FLEXNET_EINVAL;
    if (!pg && !a->d_act) return FLEXNET_EINVAL;
    const int rc = attn_critic_check_shape(a->batch, a->n_agents, a->obs_dim, a->act_dim);
    if (rc != FLEXNET_OK) return rc;
    bool aligned = flex_aligned(a->sa, 16) && flex_aligned(a->key, 16) && flex_aligned(a->val, 16) && flex_aligned(a->sel, 16) &&
                   flex_aligned(a->hc, 16) && flex_aligned(a->g_direct, 16) && flex_aligned(a->g_other, 16);
    if (pg)
        aligned = aligned && flex_aligned(a->s, 16) && flex_aligned(a->hb, 16) && flex_aligned(a->dz_c, 16) &&
                  flex_aligned(a->dz_b, 16) && flex_aligned(a->dz_s, 16) && flex_aligned(a->d_sel, 16) &&
                  flex_aligned(a->d_key, 16) && flex_aligned(a->dz_v, 16) && flex_aligned(a->dz_sa, 16);
    for (int k = 0; k < a->n_agents; ++k) {
        if (!a->enc_w[k] || !a->c1_w[k] || !a->c2_w[k] || (pg && (!a->b1_w[k] || !a->b2_w[k]))) return FLEXNET_EINVAL;
    }
    const int64_t tiles = (a->batch + 31) / 32;
    if (pg && a->workspace_floats < 2 * tiles * a->n_agents) return FLEXNET_EINVAL;
    if (pg && !flex_aligned(a->workspace, 8)) return FLEXNET_EUNSUPPORTED;
    if (!aligned) return FLEXNET_EUNSUPPORTED;
    if (a->batch == 0) return FLEXNET_OK;
    const dim3 grid((unsigned)((tiles + AC_W - 1) / AC_W)), block(64 * AC_W);
    hipStream_t s = (hipStream_t)stream;
    if (pg) {
        hipLaunchKernelGGL(attn_critic_backward_kernel<true>, grid, block, 0, s, *a);
        hipLaunchKernelGGL(attn_critic_dq_sum_kernel, dim3(a->n_agents), dim3(AC_SUM_T), 0, s, *a, (int)tiles);
    } else {
        hipLaunchKernelGGL(attn_critic_backward_kernel<false>, grid, block, 0, s, *a);
    }
    return flex_launch_status();
}
