// critic_mfma.h — the MLPCritic tail on the fp32 matrix cores in the transposed scheme shared by sqddpg.hip and coma.hip:
// A = weights, B = the wavefront's 32 rows (v_mfma_f32_32x32x2_f32).  Lane (row i = lane & 31, half h = lane >> 5) holds
// 32 of its row's 64 hidden units as two accumulator tiles; register r of tile t is unit 32 t + SU(r, h).
#ifndef CRITIC_MFMA_H
#define CRITIC_MFMA_H
#include <hip/hip_runtime.h>
#include "flexnet.h"

typedef float sv16 __attribute__((ext_vector_type(16)));
typedef float sv4 __attribute__((ext_vector_type(4)));

#define SH FLEXNET_HID                                      // 64
#define SQMFMA(a_, b_, c_) __builtin_amdgcn_mfma_f32_32x32x2f32((a_), (b_), (c_), 0, 0, 0)
#define SU(r, h) (8 * ((r) >> 2) + 4 * (h) + ((r) & 3))     // unit of accumulator register r in lane half h

__device__ __forceinline__ sv4 ld4(const float* p) { return *reinterpret_cast<const sv4*>(p); }
__device__ __forceinline__ float other_half(float v) { return __shfl_xor(v, 32, 64); }

__device__ __forceinline__ sv16 bias_tile(const float* b, int h) {
    sv16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = b[SU(r, h)];
    return acc;
}

// out[o][s] = acc + sum_k W[o][k] in[k][s], 32 outputs o, k over 64 inputs as two accumulator-layout tiles
__device__ __forceinline__ sv16 layer_tile(const float* wrow, sv16 acc, const sv16& in0, const sv16& in1) {
#pragma unroll
    for (int kt = 0; kt < 2; ++kt) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const sv4 w = ld4(wrow + 32 * kt + 8 * q);
#pragma unroll
            for (int j = 0; j < 4; ++j) acc = SQMFMA(w[j], kt ? in1[4 * q + j] : in0[4 * q + j], acc);
        }
    }
    return acc;
}

// LayerNorm statistics of the lane's row over its 64 units (both halves end with the same pair)
__device__ __forceinline__ void row_stats(const sv16& z0, const sv16& z1, float eps, float& mean, float& rstd) {
    float p = 0.0f;
#pragma unroll
    for (int r2 = 0; r2 < 16; ++r2) p += z0[r2] + z1[r2];
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
