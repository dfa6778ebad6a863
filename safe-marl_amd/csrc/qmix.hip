// qmix.hip — the QMIX mixer of FACMADDPG (madrl/critics/qmix.py:53-81), forward and backward (gfx950).
// Boundary: include/flexnet.h (flexnet_qmix_forward / flexnet_qmix_backward).
//
// Shipped configuration (facmaddpg.yaml): hypernet_layers 2, hypernet_embed 64, mixing_embed_dim 64, q_embed_dim 1, not
// gated, no skip connections.  Per sample, with the global state x [S] (S = n * obs_size):
//     h1 = [relu(Ww1_0 x + b) | relu(Wwf_0 x + b) | Wb1 x + b | relu(WV_0 x + b)]          (S -> 4 x 64, ONE GEMM)
//     w1 = |Ww1_2 h1[0:64] + b| (64 n), wf = |Wwf_2 h1[64:128] + b| (64), v = WV_2 h1[192:256] + b
//     hidden[e] = elu(sum_i q_i w1[i, e] + h1[128 + e]);  q_tot = sum_e hidden[e] wf[e] + v
//
// One wavefront owns 32 samples end to end.  Every layer is evaluated in flex_mfma_tile.h's transposed scheme on
// v_mfma_f32_32x32x2_f32 (exact fp32): A = weights (rows = output units), B = activations (columns = the wavefront's 32
// samples), so lane (sample s, half h) ends a layer holding units 8 q + 4 h + j of its sample in accumulator register
// 4 q + j — exactly what the next layer's B operand wants.
// The first layer reads the state rows and the weight rows with one 16-byte load per lane and group of eight inputs;
// the weights (4 x 64 x S floats, 737 KB at S = 720) are shared by every wavefront and served from L2 / L1.  The
// per-sample hypernetwork outputs w1 [64 n] and wf [64] never leave the registers: the mixing is done on the
// accumulators (w1 tile t of agent t / 2 holds embed units of the same lane positions as h1's hyper_b_1 tile).
//
// Saved for the backward: h1 [B, 256] (post-activation; hyper_b_1's block is linear) — 1 KB per sample written once by
// the forward instead of recomputing the S -> 256 GEMM (93 % of the forward's multiply-adds).  The backward re-forms the
// second layers from h1 (64 -> 64 n, 64 -> 64: 7 % of the work) and writes dL/d(w1 pre-abs) [B, 64 n], dL/d(wf pre-abs)
// [B, 64] and the first-layer pre-activation gradients [B, 256]; the weight gradients are flexnet_wgrad reductions of
// those against h1 and the state (fixed order).  No atomics, no LDS, no cross-wavefront communication: bit-reproducible.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "flexnet.h"
#include "flex_launch.h"
#include "flex_mfma_tile.h"
#include "flex_nan.h"

#define QM_WAVES 4                                   // wavefronts per block: 128 samples
#define QM_E FLEXNET_QMIX_EMBED                      // 64

__device__ __forceinline__ float sgnf(float x) { return x > 0.0f ? 1.0f : (x < 0.0f ? -1.0f : 0.0f); }  // torch.sign

// ---- forward ------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64 * QM_WAVES, 1) void qmix_forward_kernel(FlexQmixArgs a) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int i = lane & 31, h = lane >> 5;
    const int64_t s0 = ((int64_t)blockIdx.x * QM_WAVES + wave) * 32;
    if (s0 >= a.batch) return;
    const int64_t smp = s0 + i;
    const bool ok = smp < a.batch;
    const int64_t row = ok ? smp : a.batch - 1;                 // the last partial tile re-reads a valid row
    const int S = a.state_dim, n = a.n_agents;

    // first layer: four S -> 64 heads as one S -> 256 product; tile t = head t / 2, units 32 (t & 1) .. + 31
    const float* wm[4] = {a.w1_0_w, a.wf_0_w, a.b1_w, a.v_0_w};
    const float* bm[4] = {a.w1_0_b, a.wf_0_b, a.b1_b, a.v_0_b};
    tv16 acc[8];
    const float* wr[8];
#pragma unroll
    for (int t = 0; t < 8; ++t) {
        acc[t] = bias_tile_or_zero(bm[t >> 1] + 32 * (t & 1), h);
        wr[t] = wm[t >> 1] + (int64_t)(32 * (t & 1) + i) * S + 4 * h;
    }
    const float* xr = a.state + row * a.ld_state + 4 * h;
    tv4 xb = ld4(xr), wb[8];
#pragma unroll
    for (int t = 0; t < 8; ++t) wb[t] = ld4(wr[t]);
    for (int k0 = 0; k0 < S; k0 += 8) {
        // next group's operands in flight while this group's 32 MFMAs issue
        const int kn = k0 + 8 < S ? k0 + 8 : k0;
        const tv4 xn = ld4(xr + kn);
        tv4 wn[8];
#pragma unroll
        for (int t = 0; t < 8; ++t) wn[t] = ld4(wr[t] + kn);
#pragma unroll
        for (int t = 0; t < 8; ++t) {
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[t] = TILE_MFMA(wb[t][j], xb[j], acc[t]);
        }
        xb = xn;
#pragma unroll
        for (int t = 0; t < 8; ++t) wb[t] = wn[t];
    }
#pragma unroll
    for (int t = 0; t < 8; ++t) {
        if ((t >> 1) != 2) {                                    // hyper_b_1 is a single linear layer
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[t][r] = relu_nan(acc[t][r]);     // a NaN weight must reach q_tot, as torch.relu's does
        }
    }
    if (a.h1) {
        float* hr = a.h1 + smp * (4 * QM_E) + 4 * h;
#pragma unroll
        for (int t = 0; t < 8; ++t) store_tile(hr + 32 * t, acc[t], ok);
    }

    // mixing: sum_i q_i |w1[i, e]| over the agents in order, then + b1, elu
    tv16 hs[2];
#pragma unroll
    for (int eh = 0; eh < 2; ++eh) {
        hs[eh] = tv16{};
        for (int ag = 0; ag < n; ++ag) {
            const float qa = a.agent_qs[row * n + ag];
            const int ob = ag * QM_E + 32 * eh;
            const tv16 w = layer_tile(a.w1_2_w + (int64_t)(ob + i) * QM_E + 4 * h, bias_tile_or_zero(a.w1_2_b + ob, h),
                                             acc[0], acc[1]);
#pragma unroll
            for (int r = 0; r < 16; ++r) hs[eh][r] += qa * fabsf(w[r]);
        }
    }
    float part = 0.0f;
#pragma unroll
    for (int eh = 0; eh < 2; ++eh) {
        const tv16 wf = layer_tile(a.wf_2_w + (32 * eh + i) * QM_E + 4 * h, bias_tile_or_zero(a.wf_2_b + 32 * eh, h),
                                          acc[2], acc[3]);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const float x = hs[eh][r] + acc[4 + eh][r];
            const float hid = x > 0.0f ? x : expm1f(x);
            part += hid * fabsf(wf[r]);
        }
    }
    float vp = 0.0f;                                            // V.2: 64 -> 1 in the lanes, halves combined below
#pragma unroll
    for (int t = 0; t < 2; ++t) {
#pragma unroll
        for (int r = 0; r < 16; ++r) vp += a.v_2_w[32 * t + TILE_U(r, h)] * acc[6 + t][r];
    }
    const float part_o = other_half(part), vp_o = other_half(vp);
    if (h == 0 && ok) a.q_tot[smp] = (part + part_o) + ((vp + vp_o) + a.v_2_b[0]);
}

// ---- backward -----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64 * QM_WAVES, 1) void qmix_backward_kernel(FlexQmixArgs a) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int i = lane & 31, h = lane >> 5;
    const int64_t s0 = ((int64_t)blockIdx.x * QM_WAVES + wave) * 32;
    if (s0 >= a.batch) return;
    const int64_t smp = s0 + i;
    const bool ok = smp < a.batch;
    const int64_t row = ok ? smp : a.batch - 1;
    const int n = a.n_agents;
    const bool pg = a.want_param_grads != 0;
    const float* hr = a.h1 + row * (4 * QM_E) + 4 * h;
    const tv16 h0 = load_tile(hr), h1t = load_tile(hr + 32);
    const tv16 h2 = load_tile(hr + 64), h3 = load_tile(hr + 96);
    const float g = a.d_q_tot[row];

    // re-formed forward: wf (pre-abs) and the mixing's pre-activation
    tv16 wf[2], dh[2];
#pragma unroll
    for (int eh = 0; eh < 2; ++eh)
        wf[eh] = layer_tile(a.wf_2_w + (32 * eh + i) * QM_E + 4 * h, bias_tile_or_zero(a.wf_2_b + 32 * eh, h), h2, h3);
#pragma unroll
    for (int eh = 0; eh < 2; ++eh) {
        tv16 hs = tv16{};
        for (int ag = 0; ag < n; ++ag) {
            const float qa = a.agent_qs[row * n + ag];
            const int ob = ag * QM_E + 32 * eh;
            const tv16 w = layer_tile(a.w1_2_w + (int64_t)(ob + i) * QM_E + 4 * h, bias_tile_or_zero(a.w1_2_b + ob, h), h0, h1t);
#pragma unroll
            for (int r = 0; r < 16; ++r) hs[r] += qa * fabsf(w[r]);
        }
        const tv16 b1 = load_tile(hr + 128 + 32 * eh);
        tv16 dwf;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const float x = hs[r] + b1[r];
            const float hid = x > 0.0f ? x : expm1f(x);
            dwf[r] = g * hid * sgnf(wf[eh][r]);                  // d(wf pre-abs)
            dh[eh][r] = g * fabsf(wf[eh][r]) * (x > 0.0f ? 1.0f : expf(x));   // d(hidden pre-activation) = d b1
        }
        wf[eh] = dwf;
    }
    float* pr = a.d_pre1 + smp * (4 * QM_E) + 4 * h;
    if (pg) {
        store_tile(a.d_wf + smp * QM_E + 4 * h, wf[0], ok);
        store_tile(a.d_wf + smp * QM_E + 32 + 4 * h, wf[1], ok);
        store_tile(pr + 128, dh[0], ok);
        store_tile(pr + 160, dh[1], ok);
    }

    // d agent_qs, d(w1 pre-abs) and its input gradient into h1[0:64]
    tv16 dx0 = tv16{}, dx1 = tv16{};
    for (int ag = 0; ag < n; ++ag) {
        const float qa = a.agent_qs[row * n + ag];
        float dqp = 0.0f;
#pragma unroll
        for (int eh = 0; eh < 2; ++eh) {
            const int ob = ag * QM_E + 32 * eh;
            const tv16 w = layer_tile(a.w1_2_w + (int64_t)(ob + i) * QM_E + 4 * h, bias_tile_or_zero(a.w1_2_b + ob, h), h0, h1t);
            tv16 dw;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                dqp += dh[eh][r] * fabsf(w[r]);
                dw[r] = dh[eh][r] * qa * sgnf(w[r]);
            }
            if (pg) {
                store_tile(a.d_w1 + smp * (n * QM_E) + ob + 4 * h, dw, ok);
                dx0 = transposed_tile(a.w1_2_w + (int64_t)ob * QM_E + i, QM_E, h, dx0, dw);
                dx1 = transposed_tile(a.w1_2_w + (int64_t)ob * QM_E + 32 + i, QM_E, h, dx1, dw);
            }
        }
        const float tot = dqp + other_half(dqp);
        if (h == 0 && ok) a.d_agent_qs[smp * n + ag] = tot;
    }
    if (!pg) return;
    // ReLU masks, torch's threshold_backward: zero where h1 <= 0, so a NaN unit hands its gradient on; hyper_w_final's input
    // gradient; V: d h1[192 + u] = g V2[u]
    tv16 d2 = tv16{}, d3 = tv16{};
#pragma unroll
    for (int eh = 0; eh < 2; ++eh) {
        d2 = transposed_tile(a.wf_2_w + (32 * eh) * QM_E + i, QM_E, h, d2, wf[eh]);
        d3 = transposed_tile(a.wf_2_w + (32 * eh) * QM_E + 32 + i, QM_E, h, d3, wf[eh]);
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        dx0[r] = h0[r] <= 0.0f ? 0.0f : dx0[r];
        dx1[r] = h1t[r] <= 0.0f ? 0.0f : dx1[r];
        d2[r] = h2[r] <= 0.0f ? 0.0f : d2[r];
        d3[r] = h3[r] <= 0.0f ? 0.0f : d3[r];
    }
    store_tile(pr, dx0, ok);
    store_tile(pr + 32, dx1, ok);
    store_tile(pr + 64, d2, ok);
    store_tile(pr + 96, d3, ok);
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const tv16 hv = load_tile(hr + 192 + 32 * t);
        tv16 dv;
#pragma unroll
        for (int r = 0; r < 16; ++r) dv[r] = hv[r] <= 0.0f ? 0.0f : g * a.v_2_w[32 * t + TILE_U(r, h)];
        store_tile(pr + 192 + 32 * t, dv, ok);
    }
}

// ---- entry points -------------------------------------------------------------------------------------------------
// FLEXNET_EINVAL for missing tensors, FLEXNET_EUNSUPPORTED for shapes / layouts outside the kernel; both before any HIP call
static int qmix_check(const FlexQmixArgs* a, bool backward) {
    if (!a || a->batch < 0) return FLEXNET_EINVAL;
    if (!a->agent_qs || !a->w1_2_w || !a->w1_2_b || !a->wf_2_w || !a->wf_2_b || !a->v_2_w || !a->v_2_b)
        return FLEXNET_EINVAL;
    if (!backward && (!a->state || !a->q_tot || !a->w1_0_w || !a->w1_0_b || !a->wf_0_w || !a->wf_0_b || !a->b1_w ||
                      !a->b1_b || !a->v_0_w || !a->v_0_b))
        return FLEXNET_EINVAL;
    if (backward && (!a->h1 || !a->d_q_tot || !a->d_agent_qs ||
                     (a->want_param_grads && (!a->d_w1 || !a->d_wf || !a->d_pre1))))
        return FLEXNET_EINVAL;
    const int S = a->state_dim;
    if (a->n_agents < 1 || a->n_agents > FLEXNET_MAX_AGENTS || S < 16 || S > FLEXNET_QMIX_MAX_STATE || S % 16 != 0)
        return FLEXNET_EUNSUPPORTED;
    if (!backward && (a->ld_state < S || a->ld_state % 4 != 0 || !flex_aligned(a->state, 16) || !flex_aligned(a->w1_0_w, 16) ||
                      !flex_aligned(a->wf_0_w, 16) || !flex_aligned(a->b1_w, 16) || !flex_aligned(a->v_0_w, 16)))
        return FLEXNET_EUNSUPPORTED;
    if (!flex_aligned(a->w1_2_w, 16) || !flex_aligned(a->wf_2_w, 16) || (a->h1 && !flex_aligned(a->h1, 16)))
        return FLEXNET_EUNSUPPORTED;
    if (backward && a->want_param_grads &&
        (!flex_aligned(a->d_w1, 16) || !flex_aligned(a->d_wf, 16) || !flex_aligned(a->d_pre1, 16)))
        return FLEXNET_EUNSUPPORTED;
    return FLEXNET_OK;
}

static inline int qm_blocks(int64_t batch) { return (int)((batch + 32 * QM_WAVES - 1) / (32 * QM_WAVES)); }

extern "C" int flexnet_qmix_forward(const FlexQmixArgs* a, void* stream) {
    const int rc = qmix_check(a, false);
    if (rc != FLEXNET_OK || a->batch == 0) return rc;
    hipLaunchKernelGGL(qmix_forward_kernel, dim3(qm_blocks(a->batch)), dim3(64 * QM_WAVES), 0, (hipStream_t)stream, *a);
    return flex_launch_status();
}

extern "C" int flexnet_qmix_backward(const FlexQmixArgs* a, void* stream) {
    const int rc = qmix_check(a, true);
    if (rc != FLEXNET_OK || a->batch == 0) return rc;
    hipLaunchKernelGGL(qmix_backward_kernel, dim3(qm_blocks(a->batch)), dim3(64 * QM_WAVES), 0, (hipStream_t)stream, *a);
    return flex_launch_status();
}
