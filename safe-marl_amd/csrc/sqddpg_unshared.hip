// sqddpg_unshared.hip — SQDDPG's Shapley-value critic with `shared_params: False` (madrl/models/sqddpg.py:63-104, the else
// branch at :94-100: row (b, s, i) goes through critic i), forward and backward (gfx950).  Boundary: include/flexnet.h
// (flexnet_sqddpg_unshared_forward / flexnet_sqddpg_unshared_backward).
//
// The arithmetic of a row is sqddpg.hip's, in the same order: z1 = z_shared[b, i] + z_id[i] + W_act_i x with the
// coalition-masked action block x as up to 16 steps of v_mfma_f32_32x32x2_f32, LayerNorm (or none), ReLU, fc2 on the matrix
// cores, ReLU, fc3 (flex_mfma_tile.h's transposed scheme: A = weights, B = the wavefront's 32 rows).  What differs is the work
// map.  sqddpg.hip mixes a sample's agents inside a 32-row tile; here the A operand differs per agent, so tiles are
// agent-homogeneous: one wavefront (one work-group) owns a chunk of `spc` whole samples of ONE agent (blockIdx.y), its rows
// ordered (sample, s).  Lane `ls` owns sample `ls` and sums that sample's q over s in order: phi = mean_s q needs no atomics and
// is bit-reproducible.  Every weight is read where its module keeps it, through the per-agent pointer tables of the arguments
// (critic_unshared.hip's idiom); the action and id columns of fc1.weight are read in place at the weight's row pitch.
//
// The backward recomputes the forward per tile and stages a1 / dz2 / dz1 / x in LDS to reduce over rows, as sqddpg.hip does.
// Parameter gradients are per-wavefront partials of a persistent grid PER AGENT (at most FLEXNET_SQDDPG_UNSHARED_BWD_GRID
// wavefronts) in a workspace, summed in a fixed order by flex_reduce_rows.  Nothing of width 64 per row goes to HBM.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "flexnet.h"
#include "flex_reduce.h"
#include "flex_launch.h"
#include "flex_mfma_tile.h"

#define AS_LP 68                                            // LDS row pitch (floats) of the [row][unit] stages
#define AS_XP 33                                            // LDS row pitch of the action stage [row][k]
#define AS_MAXK 32                                          // n a <= 32: one MFMA k tile for dW_act
#define AS_WAVES_PER_CU 4                                   // backward wavefronts kept resident per CU

// workspace row of one wavefront's parameter-gradient partials (floats)
#define ASW_W2 0                                            // dW2 [64][64]
#define ASW_B2 4096                                         // db2 [64]
#define ASW_G 4160                                          // d LayerNorm weight [64]
#define ASW_BE 4224                                         // d LayerNorm bias [64]
#define ASW_W3 4288                                         // dW3 [64]
#define ASW_B3 4352                                         // db3 (element 0 of 64)
#define ASW_ID 4416                                         // d z_id [64]
#define ASW_WA 4480                                         // dW_act [64][32]
static_assert(ASW_WA + SH * AS_MAXK == FLEXNET_SQDDPG_UNSHARED_WS_ROW, "workspace row layout");

typedef FlexSqddpgUnsharedArgs AsArgs;

// A work-group has ONE agent: the [64] vectors of its critic are staged in LDS once (floats from the stage's base)
#define ASC_ID 0                                            // z_id: the agent's own id column of fc1.weight
#define ASC_LNW 64                                          // LayerNorm weight, bias (1, 0 without LayerNorm: not read)
#define ASC_LNB 128
#define ASC_B2 192                                          // fc2.bias
#define ASC_W3 256                                          // fc3.weight
#define ASC_FLOATS 320

__device__ __forceinline__ void as_stage(float* sc, const AsArgs& a, int ag, int lane) {
    sc[ASC_ID + lane] = a.w_id[ag][lane * (int)a.ld_fc1];
    sc[ASC_LNW + lane] = a.layernorm ? a.ln_w[ag][lane] : 1.0f;
    sc[ASC_LNB + lane] = a.layernorm ? a.ln_b[ag][lane] : 0.0f;
    sc[ASC_B2 + lane] = a.fc2_b[ag][lane];
    sc[ASC_W3 + lane] = a.fc3_w[ag][lane];
    __syncthreads();
}

struct AsRow {            // one row of the tile, as lane (i, h) sees it
    int64_t b;            // sample
    int64_t g;            // coalition group b * ns + s
    int own;              // pos[g, agent]
    uint32_t perm;        // nibble p = the agent at position p of the group
    bool ok;              // a real row of the chunk
};

__device__ __forceinline__ AsRow as_row(const AsArgs& a, int ag, int64_t b0, int rows, int lr) {
    AsRow r;
    r.ok = lr < rows;
    if (!r.ok) lr = rows - 1;                               // the last partial tile re-reads a valid row
    const int ls = lr / a.sample_size, s = lr - ls * a.sample_size;
    r.b = b0 + ls;
    r.g = r.b * a.sample_size + s;
    const int32_t* pg = a.pos + r.g * a.n_agents;
    r.own = pg[ag];
    r.perm = 0;
#pragma unroll
    for (int j = 0; j < FLEXNET_MAX_AGENTS; ++j) {          // (agents past n repeat agent n - 1: the same nibble again)
        const int jj = j < a.n_agents ? j : a.n_agents - 1;
        r.perm |= (uint32_t)jj << (4 * (pg[jj] & 7));
    }
    return r;
}

// the coalition-masked action input x[k] of the row, k = p a + c: act[b, agent at position p, c] for p <= own, else 0
__device__ __forceinline__ float as_x(const AsArgs& a, const AsRow& r, int k) {
    const int n = a.n_agents, ad = a.act_dim;
    if (k >= n * ad) return 0.0f;
    const int p = k / ad, c = k - p * ad;
    if (p > r.own) return 0.0f;
    int who = (int)((r.perm >> (4 * p)) & 15u);
    if (who >= n) who = n - 1;                              // (only a `pos` that is no permutation gets here: stay inside act)
    return a.act[(r.b * n + who) * ad + c];
}

struct AsFwd { tv16 z[2], xh[2], a1[2], z2[2]; float rstd; };

// z1 -> LayerNorm -> ReLU -> fc2 of the lane's row through critic `ag`; returns the pre-activation z2 (and what the backward
// needs)
__device__ __forceinline__ void as_forward_row(const AsArgs& a, int ag, const float* sc, const AsRow& r, int i, int h, float* xs,
                                               AsFwd& f) {
    const int nka = a.n_agents * a.act_dim, nk = (nka + 1) & ~1;
    const int ld = (int)a.ld_fc1;
    const float* wa = a.w_act[ag];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const float* zs = a.z_shared + (r.b * a.n_agents + ag) * SH + 32 * t + 4 * h;
        const float* zi = sc + ASC_ID + 32 * t + 4 * h;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const tv4 u = ld4(zs + 8 * q), v = ld4(zi + 8 * q);
#pragma unroll
            for (int j = 0; j < 4; ++j) f.z[t][4 * q + j] = u[j] + v[j];
        }
    }
    for (int kk = 0; kk < nk; kk += 2) {                    // W_act x: lane half h feeds column kk + h
        const int k = kk + h;
        const float xv = as_x(a, r, k);
        if (xs) xs[i * AS_XP + k] = xv;
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const float w = k < nka ? wa[(32 * t + i) * ld + k] : 0.0f;
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
            const float y = a.layernorm ? xh * sc[ASC_LNW + u] + sc[ASC_LNB + u] : xh;
            f.xh[t][r2] = xh;
            f.a1[t][r2] = fmaxf(y, 0.0f);
        }
    }
    const float* W2 = a.fc2_w[ag];
#pragma unroll
    for (int t = 0; t < 2; ++t)
        f.z2[t] = layer_tile(W2 + (32 * t + i) * SH + 4 * h, bias_tile(sc + ASC_B2 + 32 * t, h), f.a1[0], f.a1[1]);
}

// rows of the chunk's sample `ls` (rows base .. base + ns - 1) inside tile [t0, t0 + 32): s in [lo, hi]
__device__ __forceinline__ void as_s_range(int base, int ns, int t0, int& lo, int& hi) {
    lo = t0 > base ? t0 - base : 0;
    hi = t0 + 31 - base;
    if (hi > ns - 1) hi = ns - 1;
}

// ---- forward ----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64, 1) void agent_sqddpg_forward_kernel(AsArgs a, int spc) {
    __shared__ float qs[32];
    __shared__ __attribute__((aligned(16))) float sc[ASC_FLOATS];
    const int lane = threadIdx.x, i = lane & 31, h = lane >> 5;
    const int n = a.n_agents, ns = a.sample_size, ag = blockIdx.y;
    as_stage(sc, a, ag, lane);
    const int64_t b0 = (int64_t)blockIdx.x * spc;
    const int nb = (int)(a.batch - b0 < spc ? a.batch - b0 : spc);
    const int rows = nb * ns;
    const bool owner = lane < nb;                          // lane ls sums its sample's q
    const int base = lane * ns;
    const float* w3 = sc + ASC_W3;
    const float b3 = a.fc3_b[ag][0];
    float acc = 0.0f;
    for (int t0 = 0; t0 < rows; t0 += 32) {
        const AsRow r = as_row(a, ag, b0, rows, t0 + i);
        AsFwd f;
        as_forward_row(a, ag, sc, r, i, h, nullptr, f);
        float p = 0.0f;
#pragma unroll
        for (int t = 0; t < 2; ++t) {
#pragma unroll
            for (int r2 = 0; r2 < 16; ++r2) p += w3[32 * t + TILE_U(r2, h)] * fmaxf(f.z2[t][r2], 0.0f);
        }
        const float q = (p + other_half(p)) + b3;
        if (h == 0) {
            qs[i] = q;
            if (a.q && r.ok) a.q[r.g * n + ag] = q;
        }
        __syncthreads();
        if (owner) {
            int lo, hi;
            as_s_range(base, ns, t0, lo, hi);
            for (int s = lo; s <= hi; ++s) acc += qs[base + s - t0];
        }
        __syncthreads();
    }
    if (a.phi && owner) a.phi[(b0 + lane) * n + ag] = acc / (float)ns;
}

// ---- backward ---------------------------------------------------------------------------------------------------------
// PG: with the parameter gradients (the value loss); without, only d_z_shared and d_act_own come out (`frozen`)
template <bool PG>
__global__ __launch_bounds__(64, 1) void agent_sqddpg_backward_kernel(AsArgs a, int spc, int chunks, int grid) {
    __shared__ float s_a1[32 * AS_LP];                      // a1, later dy
    __shared__ float s_dz2[32 * AS_LP];                     // dz2, later dy * xhat
    __shared__ float s_dz1[32 * AS_LP];                     // dq * a2, later dz1
    __shared__ float s_x[32 * AS_XP];                       // the rows' action inputs
    __shared__ float s_dq[32];
    __shared__ int s_meta[32];                              // sample in chunk | (own position << 8); -1: no row
    __shared__ float s_da[64 * 8];                          // d act_own of the tile's 32 rows; at a chunk's end of its <= 64 samples
    __shared__ __attribute__((aligned(16))) float sc[ASC_FLOATS];
    const int lane = threadIdx.x, i = lane & 31, h = lane >> 5;
    const int n = a.n_agents, ns = a.sample_size, ad = a.act_dim, nka = n * ad, ag = blockIdx.y;
    constexpr bool pg = PG;
    const float inv_ns = 1.0f / (float)ns;
    const int ld = (int)a.ld_fc1;
#pragma unroll
    for (int k = 0; k < 8; ++k) s_da[64 * k + lane] = 0.0f;  // components >= act_dim stay zero: they are summed, never stored
    as_stage(sc, a, ag, lane);
    const float* wa = a.w_act[ag];
    const float* W2 = a.fc2_w[ag];
    const float* w3 = sc + ASC_W3;
    const float* lnw = sc + ASC_LNW;
    tv16 dw2[4], dwa[2];
#pragma unroll
    for (int t = 0; t < 4; ++t) dw2[t] = tv16{};
    dwa[0] = tv16{};
    dwa[1] = tv16{};
    float c_b2 = 0.0f, c_w3 = 0.0f, c_g = 0.0f, c_be = 0.0f, c_b3 = 0.0f, c_id = 0.0f;   // lane = unit

    for (int c = blockIdx.x; c < chunks; c += grid) {
        const int64_t b0 = (int64_t)c * spc;
        const int nb = (int)(a.batch - b0 < spc ? a.batch - b0 : spc);
        const int rows = nb * ns;
        const bool owner = lane < nb;
        const int base = lane * ns;
        float da_acc[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) da_acc[k] = 0.0f;
        float zs_acc = 0.0f;                                 // d z_shared of the current sample, lane = unit
        int zs_cur = 0;
        for (int t0 = 0; t0 < rows; t0 += 32) {
            const AsRow r = as_row(a, ag, b0, rows, t0 + i);
            AsFwd f;
            as_forward_row(a, ag, sc, r, i, h, pg ? s_x : nullptr, f);
            float dq = 0.0f;
            if (r.ok) {
                dq = a.d_phi[r.b * n + ag] * inv_ns;
                if (a.d_q) dq += a.d_q[r.g * n + ag];
            }
            // fc3, ReLU, fc2^T
            tv16 dz2[2], da1[2];
#pragma unroll
            for (int t = 0; t < 2; ++t) {
#pragma unroll
                for (int r2 = 0; r2 < 16; ++r2)
                    dz2[t][r2] = f.z2[t][r2] > 0.0f ? dq * w3[32 * t + TILE_U(r2, h)] : 0.0f;
            }
            da1[0] = tv16{};
            da1[1] = tv16{};
#pragma unroll
            for (int ot = 0; ot < 2; ++ot) {
#pragma unroll
                for (int kt = 0; kt < 2; ++kt)
                    da1[kt] = transposed_tile(W2 + (32 * ot) * SH + 32 * kt + i, SH, h, da1[kt], dz2[ot]);
            }
            if (pg) {
#pragma unroll
                for (int t = 0; t < 2; ++t) {
#pragma unroll
                    for (int r2 = 0; r2 < 16; ++r2) {
                        const int u = 32 * t + TILE_U(r2, h);
                        s_a1[i * AS_LP + u] = f.a1[t][r2];
                        s_dz2[i * AS_LP + u] = dz2[t][r2];
                        s_dz1[i * AS_LP + u] = dq * fmaxf(f.z2[t][r2], 0.0f);
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
                        const float dx = dy * lnw[u];
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
                        const float av = s_dz2[row * AS_LP + 32 * ot + i];
#pragma unroll
                        for (int kt = 0; kt < 2; ++kt)
                            dw2[2 * ot + kt] = TILE_MFMA(av, s_a1[row * AS_LP + 32 * kt + i], dw2[2 * ot + kt]);
                    }
                }
                for (int row = 0; row < 32; ++row) {
                    c_b2 += s_dz2[row * AS_LP + lane];
                    c_w3 += s_dz1[row * AS_LP + lane];
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
                    if (a.layernorm) dz1 = f.rstd * (dy * lnw[u] - m1 - f.xh[t][r2] * m2);
                    if (pg) {
                        s_a1[i * AS_LP + u] = dy;
                        s_dz2[i * AS_LP + u] = dy * f.xh[t][r2];
                    }
                    s_dz1[i * AS_LP + u] = dz1;
                }
            }
            if (h == 0) s_meta[i] = r.ok ? ((int)(r.b - b0) | (r.own << 8)) : -1;
            __syncthreads();
            if (pg) {
#pragma unroll
                for (int st = 0; st < 16; ++st) {
                    const int row = 2 * st + h;
                    const float xv = i < nka ? s_x[row * AS_XP + i] : 0.0f;
#pragma unroll
                    for (int ot = 0; ot < 2; ++ot) dwa[ot] = TILE_MFMA(s_dz1[row * AS_LP + 32 * ot + i], xv, dwa[ot]);
                }
            }
            for (int row = 0; row < 32; ++row) {           // lane = unit: the rows in order
                const int m = __builtin_amdgcn_readfirstlane(s_meta[row]);     // (uniform: the branches below are scalar)
                if (m < 0) break;
                const float v = s_dz1[row * AS_LP + lane];
                if (pg) {
                    c_be += s_a1[row * AS_LP + lane];
                    c_g += s_dz2[row * AS_LP + lane];
                    c_id += v;
                }
                if (a.d_z_shared) {
                    const int smp = m & 255;
                    if (smp != zs_cur) {
                        a.d_z_shared[((b0 + zs_cur) * n + ag) * SH + lane] = zs_acc;
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
                    const int own = (m >> 8) & 15;
                    for (int cc = h; cc < ad; cc += 2) {
                        const float* wc = wa + own * ad + cc;
                        float d = 0.0f;
#pragma unroll 4
                        for (int u = 0; u < SH; ++u) d += wc[u * ld] * s_dz1[i * AS_LP + u];
                        s_da[i * 8 + cc] = d;
                    }
                }
                __syncthreads();
                if (owner) {
                    int lo, hi;
                    as_s_range(base, ns, t0, lo, hi);
                    for (int s = lo; s <= hi; ++s) {
                        const int row = base + s - t0;
#pragma unroll
                        for (int cc = 0; cc < 8; ++cc) da_acc[cc] += s_da[row * 8 + cc];
                    }
                }
            }
            __syncthreads();
        }
        if (a.d_z_shared) a.d_z_shared[((b0 + zs_cur) * n + ag) * SH + lane] = zs_acc;
        if (a.d_act_own) {                                   // through s_da ([sample][8]): a uniform loop over the components
#pragma unroll
            for (int cc = 0; cc < 8; ++cc) s_da[lane * 8 + cc] = da_acc[cc];
            __syncthreads();
            if (owner) {
                float* out = a.d_act_own + ((b0 + lane) * n + ag) * ad;
                int cc = 0;                                    // (act_dim >= 1)
#pragma clang loop unroll(disable) vectorize(disable)
                do out[cc] = s_da[lane * 8 + cc]; while (++cc < ad);
            }
            __syncthreads();
        }
    }
    if (!pg) return;
    float* w = a.workspace + ((int64_t)ag * grid + blockIdx.x) * FLEXNET_SQDDPG_UNSHARED_WS_ROW;
#pragma unroll
    for (int ot = 0; ot < 2; ++ot) {
#pragma unroll
        for (int kt = 0; kt < 2; ++kt) {
#pragma unroll
            for (int r2 = 0; r2 < 16; ++r2) w[ASW_W2 + (32 * ot + TILE_U(r2, h)) * SH + 32 * kt + i] = dw2[2 * ot + kt][r2];
        }
#pragma unroll
        for (int r2 = 0; r2 < 16; ++r2) w[ASW_WA + (32 * ot + TILE_U(r2, h)) * AS_MAXK + i] = dwa[ot][r2];
    }
    w[ASW_B2 + lane] = c_b2;
    w[ASW_G + lane] = c_g;
    w[ASW_BE + lane] = c_be;
    w[ASW_W3 + lane] = c_w3;
    w[ASW_B3 + lane] = c_b3;
    w[ASW_ID + lane] = c_id;
}

// fixed-order sum of an agent's wavefronts' partial rows into its parameter gradients (blockIdx.y = agent)
__global__ __launch_bounds__(64 * FLEX_RED_G) void agent_sqddpg_reduce_kernel(AsArgs a, int parts) {
    const int e = blockIdx.x * 64 + (threadIdx.x & 63), ag = blockIdx.y;
    float v;
    if (!flex_reduce_rows(a.workspace + (int64_t)ag * parts * FLEXNET_SQDDPG_UNSHARED_WS_ROW + e, FLEXNET_SQDDPG_UNSHARED_WS_ROW,
                          parts, e < FLEXNET_SQDDPG_UNSHARED_WS_ROW, v))
        return;
    const int nka = a.n_agents * a.act_dim;
    if (e < ASW_B2) a.d_fc2_w[ag * SH * SH + e] = v;
    else if (e < ASW_G) a.d_fc2_b[ag * SH + e - ASW_B2] = v;
    else if (e < ASW_BE) { if (a.layernorm) a.d_ln_w[ag * SH + e - ASW_G] = v; }
    else if (e < ASW_W3) { if (a.layernorm) a.d_ln_b[ag * SH + e - ASW_BE] = v; }
    else if (e < ASW_B3) a.d_fc3_w[ag * SH + e - ASW_W3] = v;
    else if (e < ASW_ID) { if (e == ASW_B3) a.d_fc3_b[ag] = v; }
    else if (e < ASW_WA) a.d_z_id[ag * SH + e - ASW_ID] = v;
    else {
        const int u = (e - ASW_WA) / AS_MAXK, k = (e - ASW_WA) - u * AS_MAXK;
        if (k < nka) a.d_w_act[(ag * SH + u) * nka + k] = v;
    }
}

// ---- entry points -----------------------------------------------------------------------------------------------------
// samples per wavefront chunk: about 256 rows of one agent, at most 64 samples (one lane per sample)
static inline int as_spc(const AsArgs* a) {
    int s = 256 / a->sample_size;
    if (s > 64) s = 64;
    return s < 1 ? 1 : s;
}

static int as_check(const AsArgs* a, bool backward) {
    if (!a || a->batch < 0 || !a->z_shared || !a->act || !a->pos) return FLEXNET_EINVAL;
    if (a->n_agents < 1 || a->n_agents > FLEXNET_MAX_AGENTS || a->act_dim < 1 || a->act_dim > 8 ||
        a->n_agents * a->act_dim > AS_MAXK || a->sample_size < 1 || a->sample_size * a->n_agents > 4096)
        return FLEXNET_EUNSUPPORTED;
    if (a->ld_fc1 < a->n_agents * a->act_dim) return FLEXNET_EINVAL;
    if (a->ld_fc1 > (1 << 20)) return FLEXNET_EUNSUPPORTED;       // 32-bit offsets into fc1.weight
    for (int i = 0; i < a->n_agents; ++i) {
        if (!a->w_act[i] || !a->w_id[i] || !a->fc2_w[i] || !a->fc2_b[i] || !a->fc3_w[i] || !a->fc3_b[i]) return FLEXNET_EINVAL;
        if (a->layernorm && (!a->ln_w[i] || !a->ln_b[i])) return FLEXNET_EINVAL;
    }
    if (!backward && !a->phi && !a->q) return FLEXNET_EINVAL;
    if (backward && (!a->d_phi || (a->want_param_grads && (!a->workspace || !a->d_z_id || !a->d_w_act || !a->d_fc2_w ||
                                                           !a->d_fc2_b || !a->d_fc3_w || !a->d_fc3_b ||
                                                           (a->layernorm && (!a->d_ln_w || !a->d_ln_b))))))
        return FLEXNET_EINVAL;
    if (!flex_aligned(a->z_shared, 16)) return FLEXNET_EUNSUPPORTED;
    for (int i = 0; i < a->n_agents; ++i)
        if (!flex_aligned(a->fc2_w[i], 16)) return FLEXNET_EUNSUPPORTED;
    return FLEXNET_OK;
}

extern "C" int flexnet_sqddpg_unshared_forward(const FlexSqddpgUnsharedArgs* a, void* stream) {
    const int rc = as_check(a, false);
    if (rc != FLEXNET_OK || a->batch == 0) return rc;
    const int spc = as_spc(a);
    const int64_t chunks = (a->batch + spc - 1) / spc;
    if (chunks > 0x7fffffff) return FLEXNET_EUNSUPPORTED;
    hipLaunchKernelGGL(agent_sqddpg_forward_kernel, dim3((unsigned)chunks, (unsigned)a->n_agents), dim3(64), 0,
                       (hipStream_t)stream, *a, spc);
    return flex_launch_status();
}

extern "C" int flexnet_sqddpg_unshared_backward(const FlexSqddpgUnsharedArgs* a, void* stream) {
    const int rc = as_check(a, true);
    if (rc != FLEXNET_OK || a->batch == 0) return rc;
    const int spc = as_spc(a);
    const int64_t chunks = (a->batch + spc - 1) / spc;
    if (chunks > 0x7fffffff) return FLEXNET_EUNSUPPORTED;
    // one agent's persistent grid: its share of the wavefronts the device keeps resident, at most what the workspace holds
    const int cus = flex_cu_count();
    if (cus < 1) return FLEXNET_EHIP;
    int64_t grid = ((int64_t)cus * AS_WAVES_PER_CU + a->n_agents - 1) / a->n_agents;
    if (grid > FLEXNET_SQDDPG_UNSHARED_BWD_GRID) grid = FLEXNET_SQDDPG_UNSHARED_BWD_GRID;
    if (grid > chunks) grid = chunks;
    if (a->want_param_grads)
        hipLaunchKernelGGL(agent_sqddpg_backward_kernel<true>, dim3((unsigned)grid, (unsigned)a->n_agents), dim3(64), 0,
                           (hipStream_t)stream, *a, spc, (int)chunks, (int)grid);
    else
        hipLaunchKernelGGL(agent_sqddpg_backward_kernel<false>, dim3((unsigned)grid, (unsigned)a->n_agents), dim3(64), 0,
                           (hipStream_t)stream, *a, spc, (int)chunks, (int)grid);
    if (hipGetLastError() != hipSuccess) return FLEXNET_EHIP;
    if (a->want_param_grads) {
        hipLaunchKernelGGL(agent_sqddpg_reduce_kernel, dim3((FLEXNET_SQDDPG_UNSHARED_WS_ROW + 63) / 64, (unsigned)a->n_agents),
                           dim3(64 * FLEX_RED_G), 0, (hipStream_t)stream, *a, (int)grid);
        if (hipGetLastError() != hipSuccess) return FLEXNET_EHIP;
    }
    return FLEXNET_OK;
}
