// flex_reduce.h — the deterministic reductions the learner kernels share, each summed in a FIXED order.
//
// flex_reduce_rows: the second stage of the two-stage reductions of critic.hip, wgrad.hip, lnrelu.hip and sqddpg.hip:
// element e of `rows` partial rows (one per thread block of the first stage, `pitch` floats apart).  A thread block of
// 64 x FLEX_RED_G threads takes 64 consecutive elements: thread (ex, gy) walks rows gy, gy + G, gy + 2G, ... with four
// loads in flight into four accumulators, the G group sums are folded through LDS in index order.  The result is valid
// in the threads with gy == 0 (the others return false).
//
// flex_block_sum_f64 / flex_partials_sum_f64 / flex_loss_finish: the fp64 sum behind a reported loss (ppo.hip, coma.hip,
// tdloss.hip): per-block partial sums by a halving tree through LDS, then one wavefront over the partials.
#ifndef FLEX_REDUCE_H
#define FLEX_REDUCE_H
#include <hip/hip_runtime.h>
#include <stdint.h>

#define FLEX_RED_G 16

// `src` already points at this thread's element (e = blockIdx.x * 64 + ex); `active` = e is a real element.
__device__ __forceinline__ bool flex_reduce_rows(const float* src, int64_t pitch, int rows, bool active, float& sum) {
    __shared__ float part[FLEX_RED_G][64];
    const int ex = threadIdx.x & 63, gy = threadIdx.x >> 6;
    float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f, s3 = 0.0f;
    if (active) {
        int b = gy;
        for (; b + 3 * FLEX_RED_G < rows; b += 4 * FLEX_RED_G) {
            s0 += src[(int64_t)b * pitch];
            s1 += src[(int64_t)(b + FLEX_RED_G) * pitch];
            s2 += src[(int64_t)(b + 2 * FLEX_RED_G) * pitch];
            s3 += src[(int64_t)(b + 3 * FLEX_RED_G) * pitch];
        }
        for (; b < rows; b += FLEX_RED_G) s0 += src[(int64_t)b * pitch];
    }
    part[gy][ex] = (s0 + s1) + (s2 + s3);
    __syncthreads();
    if (gy != 0 || !active) return false;
    float t = 0.0f;
#pragma unroll
    for (int k = 0; k < FLEX_RED_G; ++k) t += part[k][ex];
    sum = t;
    return true;
}

// First stage of a loss sum: the block's THREADS values folded by a halving tree through LDS, into partial[blockIdx.x].
template <int THREADS>
__device__ __forceinline__ void flex_block_sum_f64(double v, double* partial) {
    __shared__ double red[THREADS];
    const int tid = threadIdx.x;
    red[tid] = v;
    __syncthreads();
    for (int sft = THREADS / 2; sft > 0; sft >>= 1) {
        if (tid < sft) red[tid] += red[tid + sft];
        __syncthreads();
    }
    if (tid == 0) partial[blockIdx.x] = red[0];
}

// Second stage, one wavefront: lane l adds the partials of blocks l, l + 64, ..., then a fixed xor-shuffle tree; the total
// is returned in every lane.
__device__ __forceinline__ double flex_partials_sum_f64(const double* partial, int nblocks, int lane) {
    double t = 0.0;
    for (int b = lane; b < nblocks; b += 64) t += partial[b];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) t += __shfl_xor(t, off, 64);
    return t;
}

// The body of a one-wavefront finish kernel: *loss = scale * (sum of the nblocks partials)
__device__ __forceinline__ void flex_loss_finish(const double* partial, int nblocks, double scale, float* loss) {
    const int lane = threadIdx.x;
    const double t = flex_partials_sum_f64(partial, nblocks, lane);
    if (lane == 0) *loss = (float)(t * scale);
}

#endif
