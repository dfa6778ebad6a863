// sqddpg.hip — SQDDPG's Shapley-value critic (madrl/models/sqddpg.py:35-104), coalition draw, forward and backward
// (gfx950).  Boundary: include/flexnet.h (flexnet_sqddpg_draw / flexnet_sqddpg_forward / flexnet_sqddpg_backward).
//
// Group g = (b, s) of the b * ns coalition groups holds a permutation: pos[g, i] is the position of agent i.  Critic row
// (b, s, i) is fc1 of [obs_0 .. obs_{n-1} | onehot(i) | block p = act[b, agent at p] if p <= pos[g, i] else 0], so
//     z1 = z_shared[b] + z_id[i] + W_act x,     x[p a + k] = act[b, gc[g, p], k] for p <= pos[g, i], else 0
// with z_shared = W_obs obs + b1 formed once per sample by the caller.  The kernel never materialises the 745-wide rows:
// each row's z1 starts from z_shared + z_id and takes the coalition-masked action block (n a <= 32 columns) as up to 16
// steps of v_mfma_f32_32x32x2_f32; LayerNorm, ReLU, fc2 (fp32 MFMA), ReLU and fc3 follow in flex_mfma_tile.h's transposed
// scheme (A = weights, B = the wavefront's 32 rows; lane (row i, half h) ends a layer holding units 8 q + 4 h + j).
//
// One wavefront (one work-group) owns a chunk of whole samples (`spc` of them, <= 64 / n and about 256 rows): it walks the
// chunk's rows in tiles of 32 and lane (sample, agent) sums its rows' q over s in order, so phi = mean_s q and S = sum_i phi
// need no atomics and are bit-reproducible.  The backward recomputes the forward per tile and stages a1 / dz2 / dz1 / x
// in LDS ([row][unit], 32 rows) to reduce over rows: dW2 and dW_act as MFMA outer products with the rows as the k
// dimension, the bias / LayerNorm / fc3 / id-column sums as one lane per unit.  Parameter gradients are per-wavefront
// partials of a persistent grid (at most FLEXNET_SQDDPG_BWD_GRID wavefronts) in a workspace, summed in a fixed order by
// flex_reduce_rows.  Nothing of width 64 per row goes to HBM.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "flexnet.h"
#include "flex_reduce.h"
#include "flex_launch.h"
#include "flex_mfma_tile.h"

#define SQ_LP 68                                            // LDS row pitch (floats) of the [row][unit] stages
#define SQ_XP 33                                            // LDS row pitch of the action stage [row][k]
#define SQ_MAXK 32                                          // n a <= 32: one MFMA k tile for dW_act

// workspace row of one wavefront's parameter-gradient partials (floats)
#define SQW_W2 0                                            // dW2 [64][64]
#define SQW_B2 4096                                         // db2 [64]
#define SQW_G 4160                                          // d LayerNorm weight [64]
#define SQW_BE 4224                                         // d LayerNorm bias [64]
#define SQW_W3 4288                                         // dW3 [64]
#define SQW_B3 4352                                         // db3 (element 0 of 64)
#define SQW_ID 4416                                         // d z_id [8][64]
#define SQW_WA 4928                                         // dW_act [64][32]
static_assert(SQW_WA + SH * SQ_MAXK == FLEXNET_SQDDPG_WS_ROW, "workspace row layout");

struct SqRow {            // one row of the tile, as lane (i, h) sees it
    int64_t b;            // sample
    int64_t g;            // coalition group b * ns + s
    int ag;               // agent
    int own;              // pos[g, ag]
    bool ok;              // a real row of the chunk
};

__device__ __forceinline__ SqRow sq_row(const FlexSqddpgArgs& a, int64_t b0, int rows, int lr) {
    SqRow r;
    r.ok = lr < rows;
    if (!r.ok) lr = rows - 1;                               // the last partial tile re-reads a valid row
    const int R = a.sample_size * a.n_agents;
    const int ls = lr / R, rem = lr - ls * R, s = rem / a.n_agents;
    r.ag = rem - s * a.n_agents;
    r.b = b0 + ls;
    r.g = r.b * a.sample_size + s;
    r.own = a.pos[r.g * a.n_agents + r.ag];
    return r;
}

// the coalition-masked action input x[k] of the row, k = p a + c: act[b, agent at position p, c] for p <= own, else 0
__device__ __forceinline__ float sq_x(const FlexSqddpgArgs& a, const SqRow& r, int k) {
    const int n = a.n_agents, ad = a.act_dim;
    if (k >= n * ad) return 0.0f;
    const int p = k / ad, c = k - p * ad;
    if (p > r.own) return 0.0f;
    int who = 0;
#pragma unroll
    for (int j = 0; j < FLEXNET_MAX_AGENTS; ++j)
        if (j < n && a.pos[r.g * n + j] == p) who = j;
    return a.act[(r.b * n + who) * ad + c];
}

struct SqFwd { tv16 z[2], xh[2], a1[2], z2[2]; float rstd; };

// z1 -> LayerNorm -> ReLU -> fc2 of the lane's row; returns the pre-activation z2 (and what the backward needs)
__device__ __forceinline__ void sq_forward_row(const FlexSqddpgArgs& a, const SqRow& r, int i, int h, float* xs, SqFwd& f) {
    const int nk = (a.n_agents * a.act_dim + 1) & ~1;
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const float* zs = a.z_shared + r.b * SH + 32 * t + 4 * h;
        const float* zi = a.z_id + r.ag * SH + 32 * t + 4 * h;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const tv4 u = ld4(zs + 8 * q), v = ld4(zi + 8 * q);
#pragma unroll
            for (int j = 0; j < 4; ++j) f.z[t][4 * q + j] = u[j] + v[j];
        }
    }
    for (int kk = 0; kk < nk; kk += 2) {                    // W_act x: lane half h feeds column kk + h
        const int k = kk + h;
        const float xv = sq_x(a, r, k);
        if (xs) xs[i * SQ_XP + k] = xv;
        const int nka = a.n_agents * a.act_dim;
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const float w = k < nka ? a.w_act[(32 * t + i) * nka + k] : 0.0f;
            f.z[t] = TILE_MFMA(w, xv, f.z[t]);
        }
    }
    float mean = 0.0f, rstd = 1.0f;
    if (a.layernorm) row_stats(f.z[0], f.z[1], a.ln_eps, mean, rstd);
    f.rstd = rstd;
#pragma unroll
    for (int t = 0; t < 2; ++t) {
#pragma unroll
        for (int r2 = 0; r2 < 16; ++r2) {
            const int u = 32 * t + TILE_U(r2, h);
            const float xh = a.layernorm ? (f.z[t][r2] - mean) * rstd : f.z[t][r2];
            const float y = a.layernorm ? xh * a.ln_w[u] + a.ln_b[u] : xh;
            f.xh[t][r2] = xh;
            f.a1[t][r2] = fmaxf(y, 0.0f);
        }
    }
#pragma unroll
    for (int t = 0; t < 2; ++t)
        f.z2[t] = layer_tile(a.fc2_w + (32 * t + i) * SH + 4 * h, bias_tile(a.fc2_b + 32 * t, h), f.a1[0], f.a1[1]);
}

// rows of the chunk's sample `ls` and agent `ag` inside tile [t0, t0 + 32): s in [lo, hi]
__device__ __forceinline__ void sq_s_range(int base, int n, int ns, int t0, int& lo, int& hi) {
    lo = t0 > base ? (t0 - base + n - 1) / n : 0;
    const int top = t0 + 31 - base;
    hi = top < 0 ? -1 : top / n;
    if (hi > ns - 1) hi = ns - 1;
}

// ---- coalition draw -------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint64_t sq_mix(uint64_t x) {          // splitmix64 finaliser
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}

// one uniform permutation per group (Fisher-Yates on a nibble-packed array): pos[g, agent] = position
__global__ __launch_bounds__(256) void sqddpg_draw_kernel(FlexSqddpgDrawArgs a) {
    const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (g >= a.groups) return;
    const int n = a.n_agents;
    const uint64_t key = sq_mix(sq_mix((uint64_t)a.rng_state[0]) ^ (uint64_t)a.rng_state[1]) ^ (uint64_t)g * 0xD1B54A32D192ED03ull;
    uint32_t perm = 0;                                     // perm nibble p = agent at position p
#pragma unroll
    for (int p = 0; p < FLEXNET_MAX_AGENTS; ++p) perm |= (uint32_t)p << (4 * p);
    for (int k = n - 1; k > 0; --k) {
        const uint64_t r = sq_mix(key + (uint64_t)k * 0x9E3779B97F4A7C15ull);
        const int j = (int)(((r >> 32) * (uint64_t)(k + 1)) >> 32);        // uniform in [0, k]
        const uint32_t vk = (perm >> (4 * k)) & 15u, vj = (perm >> (4 * j)) & 15u;
        perm &= ~((15u << (4 * k)) | (15u << (4 * j)));
        perm |= (vj << (4 * k)) | (vk << (4 * j));
    }
    uint32_t pos = 0;
#pragma unroll
    for (int p = 0; p < FLEXNET_MAX_AGENTS; ++p)
        if (p < n) pos |= (uint32_t)p << (4 * ((perm >> (4 * p)) & 15u));
#pragma unroll
    for (int i = 0; i < FLEXNET_MAX_AGENTS; ++i)
        if (i < n) a.pos[g * n + i] = (int32_t)((pos >> (4 * i)) & 15u);
}

// ---- forward ----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64, 1) void sqddpg_forward_kernel(FlexSqddpgArgs a, int spc) {
    __shared__ float qs[32];
    __shared__ float ph[64];
    const int lane = threadIdx.x, i = lane & 31, h = lane >> 5;
    const int n = a.n_agents, ns = a.sample_size, R = ns * n;
    const int64_t b0 = (int64_t)blockIdx.x * spc;
    const int nb = (int)(a.batch - b0 < spc ? a.batch - b0 : spc);
    const int rows = nb * R;
    const bool owner = lane < nb * n;                      // lane (ls, agent) sums its rows' q
    const int ls = lane / n, lag = lane - (lane / n) * n, base = ls * R + lag;
    float acc = 0.0f;
    for (int t0 = 0; t0 < rows; t0 += 32) {
        const SqRow r = sq_row(a, b0, rows, t0 + i);
        SqFwd f;
        sq_forward_row(a, r, i, h, nullptr, f);
        float p = 0.0f;
#pragma unroll
        for (int t = 0; t < 2; ++t) {
#pragma unroll
            for (int r2 = 0; r2 < 16; ++r2) p += a.fc3_w[32 * t + TILE_U(r2, h)] * fmaxf(f.z2[t][r2], 0.0f);
        }
        const float q = (p + other_half(p)) + a.fc3_b[0];
        if (h == 0) {
            qs[i] = q;
            if (a.q && r.ok) a.q[b0 * R + t0 + i] = q;
        }
        __syncthreads();
        if (owner) {
            int lo, hi;
            sq_s_range(base, n, ns, t0, lo, hi);
            for (int s = lo; s <= hi; ++s) acc += qs[base + s * n - t0];
        }
        __syncthreads();
    }
    const float phi = acc / (float)ns;
    if (owner) {
        ph[lane] = phi;
        if (a.phi) a.phi[b0 * n + lane] = phi;
    }
    __syncthreads();
    if (a.s && owner && lag == 0) {
        float s = 0.0f;
        for (int j = 0; j < n; ++j) s += ph[lane + j];
        a.s[b0 + ls] = s;
    }
}

// ---- backward ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64, 1) void sqddpg_backward_kernel(FlexSqddpgArgs a, int spc, int64_t chunks) {
    __shared__ float s_a1[32 * SQ_LP];                      // a1, later dy
    __shared__ float s_dz2[32 * SQ_LP];                     // dz2, later dy * xhat
    __shared__ float s_dz1[32 * SQ_LP];                     // dq * a2, later dz1
    __shared__ float s_x[32 * SQ_XP];                       // the rows' action inputs
    __shared__ float s_dq[32];
    __shared__ int s_meta[32];                              // agent | (sample in chunk << 4) | (own position << 12); -1: no row
    __shared__ float s_da[32 * 8];                          // d act_own of the rows
    const int lane = threadIdx.x, i = lane & 31, h = lane >> 5;
    const int n = a.n_agents, ns = a.sample_size, R = ns * n, ad = a.act_dim, nka = n * ad;
    const bool pg = a.want_param_grads != 0;
    const float inv_ns = 1.0f / (float)ns;
    tv16 dw2[4], dwa[2];
#pragma unroll
    for (int t = 0; t < 4; ++t) dw2[t] = tv16{};
    dwa[0] = tv16{};
    dwa[1] = tv16{};
    float c_b2 = 0.0f, c_w3 = 0.0f, c_g = 0.0f, c_be = 0.0f, c_b3 = 0.0f;   // lane = unit
    float c_id[FLEXNET_MAX_AGENTS];
#pragma unroll
    for (int j = 0; j < FLEXNET_MAX_AGENTS; ++j) c_id[j] = 0.0f;

    for (int64_t c = blockIdx.x; c < chunks; c += gridDim.x) {
        const int64_t b0 = c * spc;
        const int nb = (int)(a.batch - b0 < spc ? a.batch - b0 : spc);
        const int rows = nb * R;
        const bool owner = lane < nb * n;
        const int ls = lane / n, lag = lane - (lane / n) * n, base = ls * R + lag;
        float da_acc[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) da_acc[k] = 0.0f;
        float zs_acc = 0.0f;                                 // d z_shared of the current sample, lane = unit
        int zs_cur = 0;
        for (int t0 = 0; t0 < rows; t0 += 32) {
            const SqRow r = sq_row(a, b0, rows, t0 + i);
            SqFwd f;
            sq_forward_row(a, r, i, h, pg ? s_x : nullptr, f);
            float dq = 0.0f;
            if (r.ok) {
                dq = a.d_phi[r.b * n + r.ag] * inv_ns;
                if (a.d_q) dq += a.d_q[b0 * R + t0 + i];
            }
            // fc3, ReLU, fc2^T
            tv16 dz2[2], da1[2];
#pragma unroll
            for (int t = 0; t < 2; ++t) {
#pragma unroll
                for (int r2 = 0; r2 < 16; ++r2)
                    dz2[t][r2] = f.z2[t][r2] > 0.0f ? dq * a.fc3_w[32 * t + TILE_U(r2, h)] : 0.0f;
            }
            da1[0] = tv16{};
            da1[1] = tv16{};
#pragma unroll
            for (int ot = 0; ot < 2; ++ot) {
#pragma unroll
                for (int kt = 0; kt < 2; ++kt)
                    da1[kt] = transposed_tile(a.fc2_w + (32 * ot) * SH + 32 * kt + i, SH, h, da1[kt], dz2[ot]);
            }
            if (pg) {
#pragma unroll
                for (int t = 0; t < 2; ++t) {
#pragma unroll
                    for (int r2 = 0; r2 < 16; ++r2) {
                        const int u = 32 * t + TILE_U(r2, h);
                        s_a1[i * SQ_LP + u] = f.a1[t][r2];
                        s_dz2[i * SQ_LP + u] = dz2[t][r2];
                        s_dz1[i * SQ_LP + u] = dq * fmaxf(f.z2[t][r2], 0.0f);
                    }
                }
                if (h == 0) s_dq[i] = dq;
            }
            // ReLU and LayerNorm backward -> dz1 (in place in da1)
            float m1 = 0.0f, m2 = 0.0f;
#pragma unroll
            for (int t = 0; t < 2; ++t) {
#pragma unroll
                for (int r2 = 0; r2 < 16; ++r2) {
                    const int u = 32 * t + TILE_U(r2, h);
                    const float dy = f.a1[t][r2] > 0.0f ? da1[t][r2] : 0.0f;
                    da1[t][r2] = dy;
                    if (a.layernorm) {
                        const float dx = dy * a.ln_w[u];
                        m1 += dx;
                        m2 += dx * f.xh[t][r2];
                    }
                }
            }
            if (a.layernorm) {
                m1 = (m1 + other_half(m1)) * (1.0f / SH);
                m2 = (m2 + other_half(m2)) * (1.0f / SH);
            }
            __syncthreads();
            if (pg) {
                // dW2 += dz2^T a1 over the tile's rows (MFMA k = rows); column sums of dz2 and dq a2
#pragma unroll
                for (int st = 0; st < 16; ++st) {
                    const int row = 2 * st + h;
#pragma unroll
                    for (int ot = 0; ot < 2; ++ot) {
                        const float av = s_dz2[row * SQ_LP + 32 * ot + i];
#pragma unroll
                        for (int kt = 0; kt < 2; ++kt)
                            dw2[2 * ot + kt] = TILE_MFMA(av, s_a1[row * SQ_LP + 32 * kt + i], dw2[2 * ot + kt]);
                    }
                }
                for (int row = 0; row < 32; ++row) {
                    c_b2 += s_dz2[row * SQ_LP + lane];
                    c_w3 += s_dz1[row * SQ_LP + lane];
                    c_b3 += s_dq[row];
                }
            }
            __syncthreads();
            // stage 2: dy, dy * xhat, dz1
#pragma unroll
            for (int t = 0; t < 2; ++t) {
#pragma unroll
                for (int r2 = 0; r2 < 16; ++r2) {
                    const int u = 32 * t + TILE_U(r2, h);
                    const float dy = da1[t][r2];
                    float dz1 = dy;
                    if (a.layernorm) dz1 = f.rstd * (dy * a.ln_w[u] - m1 - f.xh[t][r2] * m2);
                    if (pg) {
                        s_a1[i * SQ_LP + u] = dy;
                        s_dz2[i * SQ_LP + u] = dy * f.xh[t][r2];
                    }
                    s_dz1[i * SQ_LP + u] = dz1;
                }
            }
            if (h == 0) s_meta[i] = r.ok ? (r.ag | ((int)(r.b - b0) << 4) | (r.own << 12)) : -1;
            __syncthreads();
            if (pg) {
#pragma unroll
                for (int st = 0; st < 16; ++st) {
                    const int row = 2 * st + h;
                    const float xv = i < nka ? s_x[row * SQ_XP + i] : 0.0f;
#pragma unroll
                    for (int ot = 0; ot < 2; ++ot) dwa[ot] = TILE_MFMA(s_dz1[row * SQ_LP + 32 * ot + i], xv, dwa[ot]);
                }
            }
            for (int row = 0; row < 32; ++row) {           // lane = unit: the rows in order
                const int m = s_meta[row];
                if (m < 0) break;
                const float v = s_dz1[row * SQ_LP + lane];
                if (pg) {
                    c_be += s_a1[row * SQ_LP + lane];
                    c_g += s_dz2[row * SQ_LP + lane];
#pragma unroll
                    for (int j = 0; j < FLEXNET_MAX_AGENTS; ++j) c_id[j] += (m & 15) == j ? v : 0.0f;
                }
                if (a.d_z_shared) {
                    const int smp = (m >> 4) & 255;
                    if (smp != zs_cur) {
                        a.d_z_shared[(b0 + zs_cur) * SH + lane] = zs_acc;
                        zs_acc = 0.0f;
                        zs_cur = smp;
                    }
                    zs_acc += v;
                }
            }
            if (a.d_act_own) {
                // row i, components c = h, h + 2, ...: W_act[:, own block]^T dz1
                const int m = s_meta[i];
                if (m >= 0) {
                    const int own = (m >> 12) & 15;
                    for (int cc = h; cc < ad; cc += 2) {
                        const float* wc = a.w_act + own * ad + cc;
                        float d = 0.0f;
                        for (int u = 0; u < SH; ++u) d += wc[u * nka] * s_dz1[i * SQ_LP + u];
                        s_da[i * 8 + cc] = d;
                    }
                }
                __syncthreads();
                if (owner) {
                    int lo, hi;
                    sq_s_range(base, n, ns, t0, lo, hi);
                    for (int s = lo; s <= hi; ++s) {
                        const int row = base + s * n - t0;
#pragma unroll
                        for (int cc = 0; cc < 8; ++cc)
                            if (cc < ad) da_acc[cc] += s_da[row * 8 + cc];
                    }
                }
            }
            __syncthreads();
        }
        if (a.d_z_shared) a.d_z_shared[(b0 + zs_cur) * SH + lane] = zs_acc;
        if (a.d_act_own && owner) {
#pragma unroll
            for (int cc = 0; cc < 8; ++cc)
                if (cc < ad) a.d_act_own[((b0 + ls) * n + lag) * ad + cc] = da_acc[cc];
        }
    }
    if (!pg) return;
    float* w = a.workspace + (int64_t)blockIdx.x * FLEXNET_SQDDPG_WS_ROW;
#pragma unroll
    for (int ot = 0; ot < 2; ++ot) {
#pragma unroll
        for (int kt = 0; kt < 2; ++kt) {
#pragma unroll
            for (int r2 = 0; r2 < 16; ++r2) w[SQW_W2 + (32 * ot + TILE_U(r2, h)) * SH + 32 * kt + i] = dw2[2 * ot + kt][r2];
        }
#pragma unroll
        for (int r2 = 0; r2 < 16; ++r2) w[SQW_WA + (32 * ot + TILE_U(r2, h)) * SQ_MAXK + i] = dwa[ot][r2];
    }
    w[SQW_B2 + lane] = c_b2;
    w[SQW_G + lane] = c_g;
    w[SQW_BE + lane] = c_be;
    w[SQW_W3 + lane] = c_w3;
    w[SQW_B3 + lane] = c_b3;
#pragma unroll
    for (int j = 0; j < FLEXNET_MAX_AGENTS; ++j) w[SQW_ID + j * SH + lane] = c_id[j];
}

// fixed-order sum of the wavefronts' partial rows into the parameter gradients
__global__ __launch_bounds__(64 * FLEX_RED_G) void sqddpg_reduce_kernel(FlexSqddpgArgs a, int parts) {
    const int e = blockIdx.x * 64 + (threadIdx.x & 63);
    float v;
    if (!flex_reduce_rows(a.workspace + e, FLEXNET_SQDDPG_WS_ROW, parts, e < FLEXNET_SQDDPG_WS_ROW, v)) return;
    const int n = a.n_agents, nka = n * a.act_dim;
    if (e < SQW_B2) a.d_fc2_w[e] = v;
    else if (e < SQW_G) a.d_fc2_b[e - SQW_B2] = v;
    else if (e < SQW_BE) { if (a.layernorm) a.d_ln_w[e - SQW_G] = v; }
    else if (e < SQW_W3) { if (a.layernorm) a.d_ln_b[e - SQW_BE] = v; }
    else if (e < SQW_B3) a.d_fc3_w[e - SQW_W3] = v;
    else if (e < SQW_ID) { if (e == SQW_B3) a.d_fc3_b[0] = v; }
    else if (e < SQW_WA) { if (e - SQW_ID < n * SH) a.d_z_id[e - SQW_ID] = v; }
    else {
        const int u = (e - SQW_WA) / SQ_MAXK, k = (e - SQW_WA) - u * SQ_MAXK;
        if (k < nka) a.d_w_act[u * nka + k] = v;
    }
}

// ---- entry points -----------------------------------------------------------------------------------------------------
// samples per wavefront chunk: about 256 rows, at most 64 / n samples (one lane per (sample, agent))
static inline int sq_spc(const FlexSqddpgArgs* a) {
    const int R = a->sample_size * a->n_agents;
    int s = 256 / R;
    if (s > 64 / a->n_agents) s = 64 / a->n_agents;
    return s < 1 ? 1 : s;
}

static int sqddpg_check(const FlexSqddpgArgs* a, bool backward) {
    if (!a || a->batch < 0 || !a->z_shared || !a->z_id || !a->w_act || !a->act || !a->pos || !a->fc2_w || !a->fc2_b ||
        !a->fc3_w || !a->fc3_b)
        return FLEXNET_EINVAL;
    if (a->layernorm && (!a->ln_w || !a->ln_b)) return FLEXNET_EINVAL;
    if (!backward && !a->phi && !a->q && !a->s) return FLEXNET_EINVAL;
    if (backward && (!a->d_phi || (a->want_param_grads && (!a->workspace || !a->d_z_id || !a->d_w_act || !a->d_fc2_w ||
                                                           !a->d_fc2_b || !a->d_fc3_w || !a->d_fc3_b ||
                                                           (a->layernorm && (!a->d_ln_w || !a->d_ln_b))))))
        return FLEXNET_EINVAL;
    if (a->n_agents < 1 || a->n_agents > FLEXNET_MAX_AGENTS || a->act_dim < 1 || a->act_dim > 8 ||
        a->n_agents * a->act_dim > SQ_MAXK || a->sample_size < 1 || a->sample_size * a->n_agents > 4096)
        return FLEXNET_EUNSUPPORTED;
    if (!flex_aligned(a->z_shared, 16) || !flex_aligned(a->z_id, 16) || !flex_aligned(a->fc2_w, 16)) return FLEXNET_EUNSUPPORTED;
    return FLEXNET_OK;
}

extern "C" int flexnet_sqddpg_draw(const FlexSqddpgDrawArgs* a, void* stream) {
    if (!a || a->groups < 0 || !a->rng_state || !a->pos) return FLEXNET_EINVAL;
    if (a->n_agents < 1 || a->n_agents > FLEXNET_MAX_AGENTS) return FLEXNET_EUNSUPPORTED;
    if (a->groups == 0) return FLEXNET_OK;
    hipLaunchKernelGGL(sqddpg_draw_kernel, dim3((unsigned)((a->groups + 255) / 256)), dim3(256), 0, (hipStream_t)stream, *a);
    return flex_launch_status();
}

extern "C" int flexnet_sqddpg_forward(const FlexSqddpgArgs* a, void* stream) {
    const int rc = sqddpg_check(a, false);
    if (rc != FLEXNET_OK || a->batch == 0) return rc;
    const int spc = sq_spc(a);
    const int64_t chunks = (a->batch + spc - 1) / spc;
    hipLaunchKernelGGL(sqddpg_forward_kernel, dim3((unsigned)chunks), dim3(64), 0, (hipStream_t)stream, *a, spc);
    return flex_launch_status();
}

extern "C" int flexnet_sqddpg_backward(const FlexSqddpgArgs* a, void* stream) {
    const int rc = sqddpg_check(a, true);
    if (rc != FLEXNET_OK || a->batch == 0) return rc;
    const int spc = sq_spc(a);
    const int64_t chunks = (a->batch + spc - 1) / spc;
    const int grid = (int)(chunks < FLEXNET_SQDDPG_BWD_GRID ? chunks : FLEXNET_SQDDPG_BWD_GRID);
    hipLaunchKernelGGL(sqddpg_backward_kernel, dim3(grid), dim3(64), 0, (hipStream_t)stream, *a, spc, chunks);
    if (hipGetLastError() != hipSuccess) return FLEXNET_EHIP;
    if (a->want_param_grads) {
        hipLaunchKernelGGL(sqddpg_reduce_kernel, dim3((FLEXNET_SQDDPG_WS_ROW + 63) / 64), dim3(64 * FLEX_RED_G), 0,
                           (hipStream_t)stream, *a, grid);
        if (hipGetLastError() != hipSuccess) return FLEXNET_EHIP;
    }
    return FLEXNET_OK;
}
