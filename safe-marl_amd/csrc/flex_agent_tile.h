// flex_agent_tile.h — the per-agent work map of actor_unshared.hip, critic_unshared.hip and actor_mlp.hip on flex_mfma_tile.h's
// transposed scheme, and the stages the three run on it.  One wavefront owns 32 samples of ONE agent — rows r = s * n_agents + a
// of the caller's [b * n, .] tensors — so the whole tile multiplies with that agent's weights; a work-group is AT_W wavefronts
// of agent blockIdx.x % n.  Forward: the first layer's block product, + bias + the agent's own id column, LayerNorm, ReLU, the
// 64 -> <= 8 head.  Backward: a [k 64, 64] weight staged in LDS, LayerNorm / ReLU backward with its per-lane parameter sums,
// the work-group fold of those sums in a fixed order, and the second launch that sums the work-groups' rows of one agent.
// The functions take tiles by reference and plain pointers, never an argument struct, and declare no LDS of their own: a kernel
// declares its buffers and passes them.  Where the kernels differ the difference is a template bool or an argument.
#ifndef FLEX_AGENT_TILE_H
#define FLEX_AGENT_TILE_H
#include "flex_mfma_tile.h"
#include "flex_reduce.h"

#define AT_W 4                                   // wavefronts per work-group (one per SIMD)
#define AT_MAX_BLOCKS 128                        // backward work-groups per agent (the FLEXNET_*_WS_FLOATS macros)
#define AT_FOLD 33                               // pitch of a lane's 32 sums in the fold buffer
#define AT_WP 72                                 // pitch of a weight row in LDS: the two lane halves (four rows apart) hit disjoint banks

// work-groups per agent: the forward's grid; the backward's, capped (past the cap a wavefront walks several tiles)
static inline int64_t at_groups(int64_t batch) { return ((batch + 31) / 32 + AT_W - 1) / AT_W; }
static inline int64_t at_blocks_per_agent(int64_t batch) {
    const int64_t bpa = at_groups(batch);
    return bpa > AT_MAX_BLOCKS ? AT_MAX_BLOCKS : bpa;
}

// x += W[:, c0 .. c0 + width) @ xp[0 .. width) for the lane's row: MFMA step j of a group of eight columns takes the pair
// (c + j, c + 4 + j); `w0` / `w1` = the lane's two weight rows at the block's first column.  (Clamped: no load past a row, no
// alignment asked of it.)
__device__ __forceinline__ void at_fc1_block(tv16 (&x)[2], const float* xp, const float* w0, const float* w1, int width, int h) {
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

typedef float tv2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ bool at_aligned(const void* p, uintptr_t bytes) { return (reinterpret_cast<uintptr_t>(p) & (bytes - 1)) == 0; }

// at_fc1_block with wide loads where the operands allow them, for the whole groups of eight columns; the rest (and everything
// where they do not) goes through at_fc1_block itself.  The lane's four inputs of a group are consecutive (c0 + 4 h + j): one
// 16-byte load where `xv` (the row 16-byte aligned), and each weight row's four are two 8-byte loads where `wv` (the rows
// 8-byte aligned: an even row length and first column).  The same values meet the same MFMA steps in the same order: the bits
// are at_fc1_block's.  Five loads per group instead of twelve: at 746 columns the first layer is bound by its load count.
// (critic_unshared_twin.hip's; critic_unshared.hip's forward calls at_fc1_block.)
__device__ __forceinline__ void at_fc1_block_wide(tv16 (&x)[2], const float* xp, const float* w0, const float* w1, int width, int h,
                                                  bool xv, bool wv) {
    int c0 = 0;
    if (xv || wv) {
        const int full = width & ~7;
        for (; c0 < full; c0 += 8) {
            const int c = c0 + 4 * h;
            float o[4], wa[4], wb[4];
            if (xv) {
                const tv4 v = ld4(xp + c);
#pragma unroll
                for (int j = 0; j < 4; ++j) o[j] = v[j];
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) o[j] = xp[c + j];
            }
            if (wv) {
                const tv2 a0 = *reinterpret_cast<const tv2*>(w0 + c), a1 = *reinterpret_cast<const tv2*>(w0 + c + 2);
                const tv2 b0 = *reinterpret_cast<const tv2*>(w1 + c), b1 = *reinterpret_cast<const tv2*>(w1 + c + 2);
                wa[0] = a0[0]; wa[1] = a0[1]; wa[2] = a1[0]; wa[3] = a1[1];
                wb[0] = b0[0]; wb[1] = b0[1]; wb[2] = b1[0]; wb[3] = b1[1];
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) { wa[j] = w0[c + j]; wb[j] = w1[c + j]; }
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                x[0] = TILE_MFMA(wa[j], o[j], x[0]);
                x[1] = TILE_MFMA(wb[j], o[j], x[1]);
            }
        }
    }
    if (c0 < width) at_fc1_block(x, xp + c0, w0 + c0, w1 + c0, width - c0, h);
}

// what unit u's first-layer output gains past the product: its bias + the agent's own id column (`id_col` = fc1_w + the
// column, NULL without agent_id; `ld1` = fc1_w's row length)
__device__ __forceinline__ float at_unit_add(const float* b1, const float* id_col, int ld1, int u) {
    float add = b1[u];
    if (id_col) add += id_col[(int64_t)u * ld1];
    return add;
}

__device__ __forceinline__ void at_add_bias_id(tv16 (&x)[2], const float* b1, const float* id_col, int ld1, int h) {
#pragma unroll
    for (int t = 0; t < 2; ++t) {
#pragma unroll
        for (int r = 0; r < 16; ++r) x[t][r] += at_unit_add(b1, id_col, ld1, 32 * t + TILE_U(r, h));
    }
}

// LayerNorm (where `layernorm`), ReLU
__device__ __forceinline__ void at_layernorm_relu(tv16 (&x)[2], bool layernorm, const float* lw, const float* lb, float eps, int h) {
    if (layernorm) {
        float mean, rstd;
        row_stats(x[0], x[1], eps, mean, rstd);
#pragma unroll
        for (int t = 0; t < 2; ++t) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int u = 32 * t + TILE_U(r, h);
                x[t][r] = ((x[t][r] - mean) * rstd) * lw[u] + lb[u];
            }
        }
    }
#pragma unroll
    for (int t = 0; t < 2; ++t) {
#pragma unroll
        for (int r = 0; r < 16; ++r) x[t][r] = fmaxf(x[t][r], 0.0f);
    }
}

// The head 64 -> <= 8 outputs, m += W @ in: the A operand's rows past the head's width are zero (`live` = lane row i below it;
// `wrow` = W + (live ? i : 0) * 64 + 4 h); output c = 4 h + r sits in accumulator register r < 4.  (The caller's accumulator by
// reference: returned by value, actor_unshared.hip's forward took 220 registers for 192 and lost a wavefront per SIMD.)
__device__ __forceinline__ void at_head(tv16& m, const float* wrow, bool live, const tv16 (&in)[2]) {
#pragma unroll
    for (int kt = 0; kt < 2; ++kt) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const tv4 w = ld4(wrow + 32 * kt + 8 * q);
#pragma unroll
            for (int j = 0; j < 4; ++j) m = TILE_MFMA(live ? w[j] : 0.0f, in[kt][4 * q + j], m);
        }
    }
}

// ---- backward ---------------------------------------------------------------------------------------------------------
// a [rows, 64] weight into LDS at pitch AT_WP, by the whole work-group
__device__ __forceinline__ void at_stage_weight(float* dst, const float* W, int rows, int tid) {
    for (int idx = tid; idx < rows * SH; idx += 64 * AT_W) dst[(idx >> 6) * AT_WP + (idx & 63)] = W[idx];
}

// a head's weight [width, 64] into its LDS copy [FLEXNET_MAX_ACT, 64], rows past `width` zero
__device__ __forceinline__ void at_stage_head(float* dst, const float* W, int width, int tid) {
    for (int idx = tid; idx < FLEXNET_MAX_ACT * SH; idx += 64 * AT_W) dst[idx] = idx < width * SH ? W[idx] : 0.0f;
}

// The head of a backward's tile loop: the sample of lane row i in `tile`; a partial tile's dead rows (`ok` false) re-read the
// last valid sample.  (Behind a compiler fence: without it the loop-invariant LDS reads of the staged weight — up to 192 values
// per lane — are hoisted out of the tile loop into registers the kernel does not have, and spill.)
__device__ __forceinline__ int64_t at_loop_sample(int64_t tile, int i, int64_t batch, bool& ok) {
    __asm__ volatile("" ::: "memory");
    const int64_t s0 = tile * 32;
    ok = s0 + i < batch;
    return ok ? s0 + i : batch - 1;
}

// the lane's four of its row's gradient of the head's `width` outputs (`d_row` = its row): c = 4 h + j; zero past the width and
// on a dead row (clamped: no load past the row)
__device__ __forceinline__ void at_head_grad(float (&dm)[4], const float* d_row, int width, int h, bool ok) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int c = 4 * h + j;
        const bool in = c < width;
        const float v = d_row[in ? c : width - 1];
        dm[j] = (in && ok) ? v : 0.0f;
    }
}

// dh += dm @ W (the transpose of at_head; one group of four steps): `wcol` = at_stage_head's copy of W + the lane's unit
__device__ __forceinline__ tv16 at_head_transposed(const float* wcol, int h, tv16 dh, const float (&dm)[4]) {
#pragma unroll
    for (int j = 0; j < 4; ++j) dh = TILE_MFMA(wcol[(4 * h + j) * SH], dm[j], dh);
    return dh;
}

// LayerNorm / ReLU (/ bias) backward of one tile pair, csrc/lnrelu.hip's arithmetic: from the saved first-layer output
// (`z1_64` = its row), the forward's own ReLU output (`XS`, or NULL: each tile loaded from `x_64` as its turn comes) and dx, the
// gradient of the first layer's output -> dzv, stored to `dz_64`.  `s_add` (NULL: none): z1 was saved before its bias and id
// column, which are added back here.  `s_lnw`: the LayerNorm weight in LDS, ones without LayerNorm.  ACC: the per-lane
// parameter sums acc_g (d_ln_w), acc_b (d_ln_b) and acc_d (the sum of dzv) are kept; MASK: dy and acc_d are masked with `ok`.
template <bool ACC, bool MASK>
__device__ __forceinline__ void at_ln_relu_backward(const float* z1_64, const float* s_add, const tv16* XS, const float* x_64,
                                                    const tv16 (&dx)[2], const float* s_lnw, bool layernorm, float eps,
                                                    float* dz_64, int h, bool ok, tv16 (&acc_g)[2], tv16 (&acc_b)[2],
                                                    tv16 (&acc_d)[2], tv16 (&dzv)[2]) {
    tv16 xh[2];
    float rstd = 1.0f;
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        xh[t] = load_tile(z1_64 + 32 * t + 4 * h);
        if (s_add) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const tv4 ad4 = ld4(s_add + 32 * t + 8 * q + 4 * h);
#pragma unroll
                for (int j = 0; j < 4; ++j) xh[t][4 * q + j] += ad4[j];
            }
        }
    }
    if (layernorm) {
        float mean;
        row_stats(xh[0], xh[1], eps, mean, rstd);
#pragma unroll
        for (int t = 0; t < 2; ++t) {
#pragma unroll
            for (int e = 0; e < 16; ++e) xh[t][e] = (xh[t][e] - mean) * rstd;
        }
    }
    float s1 = 0.0f, s2 = 0.0f;
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const tv16 xs = XS ? XS[t] : load_tile(x_64 + 32 * t + 4 * h);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const tv4 gw = ld4(s_lnw + 32 * t + 8 * q + 4 * h);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int e = 4 * q + j;
                const float dy = (xs[e] > 0.0f && (!MASK || ok)) ? dx[t][e] : 0.0f;
                if (ACC) {
                    acc_g[t][e] = fmaf(dy, xh[t][e], acc_g[t][e]);
                    acc_b[t][e] += dy;
                }
                const float dxh = dy * gw[j];
                dzv[t][e] = dxh;
                s1 += dxh;
                s2 = fmaf(dxh, xh[t][e], s2);
            }
        }
    }
    if (layernorm) {
        const float m1 = (s1 + other_half(s1)) * (1.0f / SH), m2 = (s2 + other_half(s2)) * (1.0f / SH);
#pragma unroll
        for (int t = 0; t < 2; ++t) {
#pragma unroll
            for (int e = 0; e < 16; ++e) dzv[t][e] = rstd * (dzv[t][e] - m1 - xh[t][e] * m2);
        }
    }
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        store_tile(dz_64 + 32 * t + 4 * h, dzv[t], ok);
        if (ACC) {
#pragma unroll
            for (int e = 0; e < 16; ++e) acc_d[t][e] += (!MASK || ok) ? dzv[t][e] : 0.0f;
        }
    }
}

// Work-group fold of one tile pair of per-lane sums into 64 sums, fixed order: wavefronts in index order, rows in index order.
// Register r of tile t in lane (i, h) is unit 32 t + TILE_U(r, h) of one row.  By the whole work-group; `fold` is free on entry
// (a barrier behind its last other use) and again on return.
__device__ __forceinline__ void at_fold_pair(float (*fold)[64][AT_FOLD], const tv16 (&src)[2], float* out, int tid) {
    const int lane = tid & 63, wave = tid >> 6;
#pragma unroll
    for (int t = 0; t < 2; ++t) {
#pragma unroll
        for (int r = 0; r < 16; ++r) fold[wave][lane][16 * t + r] = src[t][r];
    }
    __syncthreads();
    if (tid < SH) {
        const int t = tid >> 5, w = tid & 31, uh = (w >> 2) & 1, r = 4 * (w >> 3) + (w & 3);
        float sum = 0.0f;
        for (int wv = 0; wv < AT_W; ++wv)
            for (int ii = 0; ii < 32; ++ii) sum += fold[wv][32 * uh + ii][16 * t + r];
        out[tid] = sum;
    }
    __syncthreads();
}

// ... of a list of them into consecutive vectors of the work-group's partial row
template <class... P>
__device__ __forceinline__ void at_fold(float (*fold)[64][AT_FOLD], float* out, int tid, const P&... acc) {
    int q = 0;
    (at_fold_pair(fold, acc, out + SH * q++, tid), ...);
}

// The second launch: element ex of vector `vec` of every work-group's partial row (`vecs` vectors of 64) of ONE agent, summed
// in a fixed order: block = vecs * agent + vector.  False: this thread holds no sum.
__device__ __forceinline__ bool at_reduce_agent(const float* workspace, int vecs, int blocks_per_agent, int& ag, int& vec, int& ex,
                                                float& sum) {
    ex = threadIdx.x & 63;
    ag = blockIdx.x / vecs;
    vec = blockIdx.x % vecs;
    return flex_reduce_rows(workspace + (int64_t)ag * blocks_per_agent * (vecs * SH) + vec * SH + ex, vecs * SH, blocks_per_agent,
                            true, sum);
}

#endif
