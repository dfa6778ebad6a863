// flex_mfma_tile.h — the transposed fp32 matrix-core tile scheme of qmix.hip, sqddpg.hip, coma.hip, gauss.hip, attn_critic.hip,
// actor_unshared.hip, critic_unshared.hip and actor_mlp.hip: A = weights (rows = output units), B = the wavefront's 32 rows
// (v_mfma_f32_32x32x2_f32, exact fp32).  Lane (row i = lane & 31, half h = lane >> 5) holds 32 of its row's 64 units as two
// accumulator tiles; register r of tile t is unit 32 t + TILE_U(r, h) — exactly what the next layer's B operand wants when MFMA
// step (q, j) takes the k-pair (8 q + j, 8 q + 4 + j).  The per-agent work map of the last three and the stages they share on
// it: flex_agent_tile.h.  (critic.hip / actor.hip keep their own register map: actor_r16.h.)
#ifndef FLEX_MFMA_TILE_H
#define FLEX_MFMA_TILE_H
#include <hip/hip_runtime.h>
#include "flexnet.h"

typedef float tv16 __attribute__((ext_vector_type(16)));
typedef float tv4 __attribute__((ext_vector_type(4)));

#define SH FLEXNET_HID                                      // 64: the MLPCritic's hidden width, two tiles
#define TILE_MFMA(a_, b_, c_) __builtin_amdgcn_mfma_f32_32x32x2f32((a_), (b_), (c_), 0, 0, 0)
#define TILE_U(r, h) (8 * ((r) >> 2) + 4 * (h) + ((r) & 3))     // unit of accumulator register r in lane half h

__device__ __forceinline__ tv4 ld4(const float* p) { return *reinterpret_cast<const tv4*>(p); }
__device__ __forceinline__ void st4(float* p, tv4 v) { *reinterpret_cast<tv4*>(p) = v; }
__device__ __forceinline__ float other_half(float v) { return __shfl_xor(v, 32, 64); }

__device__ __forceinline__ tv16 zero_tile() {
    tv16 t;
#pragma unroll
    for (int r = 0; r < 16; ++r) t[r] = 0.0f;
    return t;
}

// accumulators start from the bias of their units
__device__ __forceinline__ tv16 bias_tile(const float* b, int h) {
    tv16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = b[TILE_U(r, h)];
    return acc;
}

// ... NULL: a zero tile.  (Its own body, not a wrapper round bias_tile: that changed qmix.hip's instruction stream.)
__device__ __forceinline__ tv16 bias_tile_or_zero(const float* b, int h) {
    tv16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = b ? b[TILE_U(r, h)] : 0.0f;
    return acc;
}

// out[o][s] = acc + sum_k W[o][k] in[k][s] for the 32 outputs o = obase + lane row and k over 64 inputs held as two
// tiles of accumulator layout (in0: inputs 0..31, in1: 32..63).  `wrow` = W + (obase + i) * 64 + 4 h.
__device__ __forceinline__ tv16 layer_tile(const float* wrow, tv16 acc, const tv16& in0, const tv16& in1) {
#pragma unroll
    for (int kt = 0; kt < 2; ++kt) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const tv4 w = ld4(wrow + 32 * kt + 8 * q);
#pragma unroll
            for (int j = 0; j < 4; ++j) acc = TILE_MFMA(w[j], kt ? in1[4 * q + j] : in0[4 * q + j], acc);
        }
    }
    return acc;
}

// The transposed product: acc[k][s] += sum_o W[o][k] d[o][s] for k = kbase + lane row and o over the 32 outputs of the
// tile `d` (accumulator layout).  `wcol` = W + obase * ld + kbase + i.
__device__ __forceinline__ tv16 transposed_tile(const float* wcol, int ld, int h, tv16 acc, const tv16& d) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
#pragma unroll
        for (int j = 0; j < 4; ++j) acc = TILE_MFMA(wcol[(8 * q + 4 * h + j) * ld], d[4 * q + j], acc);
    }
    return acc;
}

__device__ __forceinline__ void store_tile(float* row, const tv16& t, bool ok) {      // row = base + unit offset + 4 h
    if (!ok) return;
#pragma unroll
    for (int q = 0; q < 4; ++q) st4(row + 8 * q, tv4{t[4 * q], t[4 * q + 1], t[4 * q + 2], t[4 * q + 3]});
}

__device__ __forceinline__ tv16 load_tile(const float* row) {
    tv16 t;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const tv4 v = ld4(row + 8 * q);
#pragma unroll
        for (int j = 0; j < 4; ++j) t[4 * q + j] = v[j];
    }
    return t;
}

// LayerNorm statistics of the lane's row over its 64 units (both halves end with the same pair).  The mean is summed pairwise,
// as critic.hip's critic_ln_inplace does: as many additions as a running sum, log2(64) roundings instead of 63 — and exact on a
// row whose units are all equal, where rstd = eps^-1/2 multiplies whatever the mean is off by
__device__ __forceinline__ void row_stats(const tv16& z0, const tv16& z1, float eps, float& mean, float& rstd) {
    float ps[16];
#pragma unroll
    for (int r2 = 0; r2 < 16; ++r2) ps[r2] = z0[r2] + z1[r2];
#pragma unroll
    for (int w = 8; w >= 1; w >>= 1) {
#pragma unroll
        for (int r2 = 0; r2 < w; ++r2) ps[r2] += ps[r2 + w];
    }
    const float p = ps[0];
    mean = (p + other_half(p)) * (1.0f / SH);
    float v = 0.0f;
#pragma unroll
    for (int r2 = 0; r2 < 16; ++r2) {
        const float d0 = z0[r2] - mean, d1 = z1[r2] - mean;
        v += d0 * d0 + d1 * d1;
    }
    rstd = rsqrtf((v + other_half(v)) * (1.0f / SH) + eps);
}

#endif
