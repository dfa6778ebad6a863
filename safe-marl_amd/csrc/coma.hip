// coma.hip — COMA's counterfactual baseline (madrl/models/coma.py:137-149) and its policy loss (coma.py:180-188), gfx950.
// Boundary: include/flexnet.h (flexnet_coma_baseline / flexnet_coma_policy_loss).
//
// Critic row (b, i) is [o_1 .. o_n | o_i | onehot(i) | a_1 .. a_n]; the caller hands over its fc1 pre-activation z1[b, i] on
// the actions taken.  The baseline's row (s, b, i) differs from it in agent i's own act_dim action columns only:
//     z(s, b, i) = z1[b, i] + W_act[:, i a : (i + 1) a] (sampled[s, b, i] - act[b, i])
// — a rank-act_dim update of 64 values instead of an 889-wide product, and nothing of [s b n, 889] is ever formed.
//
// One wavefront (one work-group) owns 32 samples of ONE agent, so the whole tile shares the action block of W_act and the
// update is act_dim / 2 steps of v_mfma_f32_32x32x2_f32 per 32 units (A = the block's columns, B = the rows' differences,
// C = z1) against the 64 steps of fc2.  z1, the block's columns and fc2's weights (64 registers per lane: the whole
// matrix over the wavefront) stay in registers while the wavefront walks its rows through the s draws; LayerNorm's
// parameters, fc2's bias and fc3 sit in LDS.  The tail is flex_mfma_tile.h's transposed scheme, as in sqddpg.hip.  Lane
// (row, half 0) sums its row's values over s = 0, 1, .. in that order: no atomics, bit-reproducible.  Forward only — the
// baseline enters the loss detached (coma.py:180).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "flexnet.h"
#include "flex_launch.h"
#include "flex_mfma_tile.h"
#include "flex_reduce.h"

#define CM_THREADS 256
#define CM_BLOCKS FLEXNET_COMA_BLOCKS

// the draws' differences of the lane's row for pass s: component 2 kk + h in d[kk]
__device__ __forceinline__ void cm_load_delta(const FlexComaBaselineArgs& a, int64_t s, int64_t row, int h, const float* own,
                                              float* d) {
    const float* sp = a.sampled + (s * a.batch * a.n_agents + row) * a.act_dim;
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
        const int c = 2 * kk + h;
        d[kk] = c < a.act_dim ? sp[c] - own[kk] : 0.0f;
    }
}

__global__ __launch_bounds__(64) void coma_baseline_kernel(FlexComaBaselineArgs a) {
    __shared__ __attribute__((aligned(16))) float s_lnw[SH], s_lnb[SH], s_b2[SH], s_w3[SH];
    const int lane = threadIdx.x, i = lane & 31, h = lane >> 5;
    const int n = a.n_agents, ad = a.act_dim, nka = n * ad;
    const int ag = blockIdx.x % n;
    const int64_t b0 = (int64_t)(blockIdx.x / n) * 32;
    const bool ok = b0 + i < a.batch;
    const int64_t b = ok ? b0 + i : a.batch - 1;              // the last partial tile re-reads a valid sample
    const int64_t row = b * n + ag;

    s_lnw[lane] = a.layernorm ? a.ln_w[lane] : 1.0f;
    s_lnb[lane] = a.layernorm ? a.ln_b[lane] : 0.0f;
    s_b2[lane] = a.fc2_b[lane];
    s_w3[lane] = a.fc3_w[lane];

    // resident: z1 of the row, fc2 as the A operand, the agent's action block of W_act, the action taken
    tv16 z[2];
    tv4 w2[2][2][4];
    float wa[2][4], own[4];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const float* zp = a.z1 + row * SH + 32 * t + 4 * h;
        const float* wr = a.fc2_w + (32 * t + i) * SH + 4 * h;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const tv4 u = ld4(zp + 8 * q);
#pragma unroll
            for (int j = 0; j < 4; ++j) z[t][4 * q + j] = u[j];
            w2[t][0][q] = ld4(wr + 8 * q);
            w2[t][1][q] = ld4(wr + 32 + 8 * q);
        }
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
            const int c = 2 * kk + h;
            wa[t][kk] = c < ad ? a.w_act[(32 * t + i) * nka + ag * ad + c] : 0.0f;
        }
    }
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
        const int c = 2 * kk + h;
        own[kk] = c < ad ? a.act[row * ad + c] : 0.0f;
    }
    __syncthreads();
    const float b3 = a.fc3_b[0];
    const int ns = a.sample_size;
    const int first = a.q ? -1 : 0;                            // pass -1: the unmodified row
    float d[4] = {0.0f, 0.0f, 0.0f, 0.0f}, dn[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    if (first == 0) cm_load_delta(a, 0, row, h, own, d);
    float acc = 0.0f;
    for (int s = first; s < ns; ++s) {
        if (s + 1 < ns) cm_load_delta(a, s + 1, row, h, own, dn);          // in flight behind this pass's arithmetic
        tv16 zs[2] = {z[0], z[1]};
        if (s >= 0) {
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) {
                if (2 * kk < ad) {
                    zs[0] = TILE_MFMA(wa[0][kk], d[kk], zs[0]);
                    zs[1] = TILE_MFMA(wa[1][kk], d[kk], zs[1]);
                }
            }
        }
        float mean = 0.0f, rstd = 1.0f;
        if (a.layernorm) row_stats(zs[0], zs[1], a.ln_eps, mean, rstd);
#pragma unroll
        for (int t = 0; t < 2; ++t) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const tv4 g = ld4(s_lnw + 32 * t + 8 * q + 4 * h), be = ld4(s_lnb + 32 * t + 8 * q + 4 * h);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float v = zs[t][4 * q + j];
                    const float y = a.layernorm ? ((v - mean) * rstd) * g[j] + be[j] : v;
                    zs[t][4 * q + j] = fmaxf(y, 0.0f);
                }
            }
        }
        tv16 z2[2] = {bias_tile(s_b2, h), bias_tile(s_b2 + 32, h)};
#pragma unroll
        for (int kt = 0; kt < 2; ++kt) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    z2[0] = TILE_MFMA(w2[0][kt][q][j], zs[kt][4 * q + j], z2[0]);
                    z2[1] = TILE_MFMA(w2[1][kt][q][j], zs[kt][4 * q + j], z2[1]);
                }
            }
        }
        float p = 0.0f;
#pragma unroll
        for (int t = 0; t < 2; ++t) {
#pragma unroll
            for (int r2 = 0; r2 < 16; ++r2) p += s_w3[32 * t + TILE_U(r2, h)] * fmaxf(z2[t][r2], 0.0f);
        }
        const float q = (p + other_half(p)) + b3;
        if (s >= 0) {
            acc += q;
            if (a.q_sampled && ok && h == 0) a.q_sampled[(int64_t)s * a.batch * n + row] = q;
        } else if (ok && h == 0) {
            a.q[row] = q;
        }
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) d[kk] = dn[kk];
    }
    if (ok && h == 0) a.baseline[row] = acc / (float)ns;
}

// ---- policy loss: one thread per (sample, agent), per-block partial sums (fp64, fixed tree), a one-wavefront finish ------
__global__ __launch_bounds__(CM_THREADS) void coma_policy_kernel(FlexComaPolicyArgs a) {
    const int na = a.act_dim, tid = threadIdx.x;
    const int64_t total = a.rows * a.n_agents;
    const float inv = 1.0f / (float)total;
    double acc = 0.0;
    for (int64_t r = (int64_t)blockIdx.x * CM_THREADS + tid; r < total; r += (int64_t)CM_BLOCKS * CM_THREADS) {
        const float adv = a.advantages ? a.advantages[r] : a.q[r] - a.baseline[r];
        const float dlogp = -inv * adv;                                  // d loss / d log p[b, i]
        float logp = 0.0f;
        for (int k = 0; k < na; ++k) {
            const int64_t e = r * na + k;
            // Normal(mu, exp(log_std)).log_prob: -(x - mu)^2 / (2 var) - log_std - log(sqrt(2 pi))
            const float ls = a.log_stds[a.log_std_uniform ? 0 : e];
            const float sd = expf(ls), var = sd * sd;
            const float m = a.avail ? (a.avail[e] == 0.0f ? 0.0f : 1.0f) : 1.0f;
            const float df = a.actions[e] - a.means[e];
            logp += m * (-(df * df) / (2.0f * var) - ls - 0.918938533204672742f);
            a.d_means[e] = dlogp * m * df / var;
            if (a.d_log_stds) a.d_log_stds[e] = dlogp * m * (df * df / var - 1.0f);
        }
        if (a.log_prob) a.log_prob[r] = logp;
        acc += (double)(adv * logp);
    }
    flex_block_sum_f64<CM_THREADS>(acc, reinterpret_cast<double*>(a.workspace));
}

__global__ __launch_bounds__(64) void coma_loss_finish_kernel(const double* partial, double scale, float* loss) {
    flex_loss_finish(partial, CM_BLOCKS, scale, loss);
}

// ---- entry points -----------------------------------------------------------------------------------------------------
extern "C" int flexnet_coma_baseline(const FlexComaBaselineArgs* a, void* stream) {
    if (!a || a->batch < 0 || !a->z1 || !a->w_act || !a->act || !a->sampled || !a->fc2_w || !a->fc2_b || !a->fc3_w ||
        !a->fc3_b || !a->baseline)
        return FLEXNET_EINVAL;
    if (a->layernorm && (!a->ln_w || !a->ln_b)) return FLEXNET_EINVAL;
    if (a->n_agents < 1 || a->n_agents > FLEXNET_MAX_AGENTS || a->act_dim < 1 || a->act_dim > 8 ||
        a->n_agents * a->act_dim > 32 || a->sample_size < 1 || a->batch * a->n_agents > (int64_t)INT32_MAX)
        return FLEXNET_EUNSUPPORTED;
    if (!flex_aligned(a->z1, 16) || !flex_aligned(a->fc2_w, 16)) return FLEXNET_EUNSUPPORTED;
    if (a->batch == 0) return FLEXNET_OK;
    const int64_t tiles = (a->batch + 31) / 32 * a->n_agents;
    hipLaunchKernelGGL(coma_baseline_kernel, dim3((unsigned)tiles), dim3(64), 0, (hipStream_t)stream, *a);
    return flex_launch_status();
}

extern "C" int flexnet_coma_policy_loss(const FlexComaPolicyArgs* a, void* stream) {
    if (!a || a->rows < 1 || a->n_agents < 1 || a->act_dim < 1 || !a->means || !a->log_stds || !a->actions ||
        (!a->advantages && (!a->q || !a->baseline)) || !a->loss || !a->d_means || !a->workspace ||
        a->workspace_floats < FLEXNET_COMA_WS_FLOATS || !flex_aligned(a->workspace, 8))
        return FLEXNET_EINVAL;
    if (a->n_agents > FLEXNET_MAX_AGENTS || a->act_dim > FLEXNET_MAX_ACT) return FLEXNET_EUNSUPPORTED;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(coma_policy_kernel, dim3(CM_BLOCKS), dim3(CM_THREADS), 0, s, *a);
    hipLaunchKernelGGL(coma_loss_finish_kernel, dim3(1), dim3(64), 0, s, reinterpret_cast<const double*>(a->workspace),
                       -1.0 / ((double)a->rows * a->n_agents), a->loss);
    return flex_launch_status();
}
