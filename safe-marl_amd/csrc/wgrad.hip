// wgrad.hip — weight gradients of the learner's linear layers: C[m, n] = sum_k A[k, m] * B[k, n] with k = the batch
// (gfx950).  Boundary: include/flexnet.h (flexnet_wgrad, flexnet_wgrad_batched).
//
// The reference's update (madrl/utils/trainer.py:62-111 -> loss.backward()) spends its GEMM time on exactly this
// shape: dW = dY^T X for fc1 / GRUCell / fc2 of rnn_agent.py:13-33 and fc1 of mlp_critic.py:5-34, where the summed
// dimension is the batch (32 768 samples, x agents = 163 840 rows) and the output is at most 192 x 745.  Library
// split-K kernels reach 10-15 TFLOP/s there.  Here both operands are read in their stored [k, .] layout straight
// into the operand registers of v_mfma_f32_32x32x2_f32 (exact fp32 products, fp32 accumulation): lane l of a
// wavefront supplies row k0 + (l >> 5) and columns MT * (l & 31) .. + MT - 1 of A — one vector load, coalesced over
// the half-wavefront — so register t of that load is the A operand of M-tile t (the tile's row index i is column
// MT * i + t: a permutation undone when the result is written).  B alike.  A wavefront owns the whole
// [32 MT, 32 NT] output block over its share of k, so every element of A and B is read once per column chunk and the
// kernel runs at the HBM / matrix-core balance point (7 loaded floats per 10 MFMAs for [64, 160]).
// Partial blocks are folded over the thread block's four wavefronts in LDS (fixed order), written as register images
// to the workspace and summed over thread blocks in a fixed order by wgrad_reduce_kernel: bit-reproducible.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "flexnet.h"
#include "flex_launch.h"
#include "flex_reduce.h"
#include "critic_finish.h"

typedef float v16f __attribute__((ext_vector_type(16)));
typedef float v4f __attribute__((ext_vector_type(4)));
typedef float v2f __attribute__((ext_vector_type(2)));

#define WG_WAVES 4
#ifndef WG_UNROLL
#define WG_UNROLL(MT, NT) ((MT) * (NT) >= 10 ? 2 : 4)   // k steps (2 rows each) whose loads are issued together
#endif
#ifndef WG_DEPTH
#define WG_DEPTH(MT, NT) 2                              // register buffers in rotation
#endif
#define WG_IMG(MT, NT) ((MT) * (NT) * 1024)

#define WG_CS_FLOATS (520 * 192)      // head of the workspace: per-block column sums of A

struct WgradK {
    const float* a;
    const float* b;
    float* c;
    float* ws;                       // register images, after the column-sum area
    float* cs;                       // column-sum partials [slabs][32 MT], or NULL
    float* colsum;
    int64_t k, lda, ldb, a_floats, b_floats;
    int32_t m, n, rows_per_block, slabs, accumulate, ldc;
    // second input block (TWO instantiations): B = [b | b2], columns n .. n + n2 - 1 of the result go to c2
    const float* b2;
    float* c2;
    int64_t ldb2, b2_floats;
    int32_t n2, ldc2;
    const int64_t* b_cell;           // B's first row inside a larger row store (device cell), or NULL
};

__device__ __forceinline__ __amdgpu_buffer_rsrc_t wg_rsrc(const float* base, int64_t floats) {
    const int64_t bytes = floats > 0 ? floats * 4 : 0;
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(base), 0, bytes > 0x7ffffff0ll ? 0x7ffffff0 : (int)bytes, 0x00027000);
}

// W consecutive floats at byte offset `off` (out of range: zeros)
template <int W>
__device__ __forceinline__ void wg_load(__amdgpu_buffer_rsrc_t r, int off, float* out) {
    if constexpr (W == 1) {
        out[0] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r, off, 0, 0));
    } else if constexpr (W == 2) {
        const v2f v = __builtin_bit_cast(v2f, __builtin_amdgcn_raw_buffer_load_b64(r, off, 0, 0));
        out[0] = v.x; out[1] = v.y;
    } else if constexpr (W >= 4) {
        const v4f v = __builtin_bit_cast(v4f, __builtin_amdgcn_raw_buffer_load_b128(r, off, 0, 0));
        out[0] = v.x; out[1] = v.y; out[2] = v.z; out[3] = v.w;
        if constexpr (W > 4) wg_load<W - 4>(r, off + 16, out + 4);
    } else {
        wg_load<2>(r, off, out);
        wg_load<1>(r, off + 8, out + 2);
    }
}

template <int MT, int NT, bool CS, bool TWO = false>
__global__ __launch_bounds__(64 * WG_WAVES, 2) void wgrad_kernel(WgradK p) {
#include "wgrad_block.h"
}

// ---- flexnet_wgrad_batched: up to FLEXNET_WGRAD_MAX_BATCH problems of one shape class (MT, NT) per launch; the problem is
// grid dimension z and its parameters are entry z of a table in the kernel arguments (no host-to-device copy) ---------------
struct WgradB {
    const float* a;
    const float* b;
    float* c;
    float* ws;
    float* cs;
    float* colsum;
    int64_t k, lda, ldb, a_floats, b_floats;
    int32_t m, n, rows_per_block, slabs, accumulate, ldc;
};
struct WgradBatchK {
    WgradB p[FLEXNET_WGRAD_MAX_BATCH];
};
static_assert(sizeof(WgradBatchK) <= 4096, "the table travels in the kernel arguments");

__device__ __forceinline__ WgradK wg_problem(const WgradB& e) {
    WgradK p;
    p.a = e.a; p.b = e.b; p.c = e.c; p.ws = e.ws; p.cs = e.cs; p.colsum = e.colsum;
    p.k = e.k; p.lda = e.lda; p.ldb = e.ldb; p.a_floats = e.a_floats; p.b_floats = e.b_floats;
    p.m = e.m; p.n = e.n; p.rows_per_block = e.rows_per_block; p.slabs = e.slabs; p.accumulate = e.accumulate; p.ldc = e.ldc;
    p.b2 = nullptr; p.c2 = nullptr; p.ldb2 = 0; p.b2_floats = 0; p.n2 = 0; p.ldc2 = 0; p.b_cell = nullptr;
    return p;
}

// the grid spans the class's largest problem: the blocks past this problem's own slabs / column chunks leave at once
template <int MT, int NT>
__global__ __launch_bounds__(64 * WG_WAVES, 2) void wgrad_batched_kernel(WgradBatchK t) {
    const WgradK p = wg_problem(t.p[blockIdx.z]);
    if ((int)blockIdx.x >= p.slabs || (int)blockIdx.y * (32 * NT) >= p.n) return;
    constexpr bool CS = true, TWO = false;           // (column-sum partials are written for every problem; the second stage asks)
#include "wgrad_block.h"
}

// element e of the slabs' register images, summed in a fixed order, stored at its place in C; the thread blocks past
// the image (column chunk 0 only, when column sums were asked for) sum the blocks' column-sum partials the same way
// RIDER (flexnet_wgrad_critic_finish): the finish blocks of flexnet_critic_td_backward ride behind this launch's own blocks
// (row 0 of the grid) — same thread-block shape, nothing shared with them but the launch
#define WG_RED FLEX_RED_G
template <int MT, int NT, bool RIDER = false>
__global__ __launch_bounds__(64 * WG_RED) void wgrad_reduce_kernel(WgradK p, CriticFinishK f) {
    constexpr int IMG_BLOCKS = WG_IMG(MT, NT) / 64;
    float sum;
    if constexpr (RIDER) {
        const int own = IMG_BLOCKS + (p.cs ? (32 * MT + 63) / 64 : 0);
        if ((int)blockIdx.x >= own) {
            if (blockIdx.y == 0 && (int)blockIdx.x - own < f.blocks) critic_finish_block(f, blockIdx.x - own);
            return;
        }
    }
    if (blockIdx.x >= IMG_BLOCKS) {
        if (blockIdx.y != 0) return;
        const int m = (blockIdx.x - IMG_BLOCKS) * 64 + (threadIdx.x & 63);
        if (!flex_reduce_rows(p.cs + m, 32 * MT, p.slabs, m < 32 * MT, sum) || m >= p.m) return;
        p.colsum[m] = p.accumulate ? p.colsum[m] + sum : sum;
        return;
    }
    const int e = blockIdx.x * 64 + (threadIdx.x & 63);        // < WG_IMG: the grid covers it exactly
    if (!flex_reduce_rows(p.ws + (int64_t)blockIdx.y * p.slabs * WG_IMG(MT, NT) + e, WG_IMG(MT, NT), p.slabs, true, sum)) return;
    // register image -> matrix position (v_mfma_f32_32x32x2_f32 result layout, tile rows / columns interleaved)
    const int l = e & 63, r = (e >> 6) & 15, t = e >> 10;
    const int ti = t / NT, tj = t - ti * NT;
    const int i = (r & 3) + 8 * (r >> 2) + 4 * (l >> 5), j = l & 31;
    const int m = MT * i + ti, n = blockIdx.y * (32 * NT) + NT * j + tj;
    if (m >= p.m) return;
    float* dst;
    if (n < p.n) dst = p.c + (int64_t)m * p.ldc + n;
    else if (n - p.n < p.n2) dst = p.c2 + (int64_t)m * p.ldc2 + (n - p.n);       // (n2 = 0 without a second block)
    else return;
    *dst = p.accumulate ? *dst + sum : sum;
}

// wgrad_reduce_kernel's sums in its order, per problem
template <int MT, int NT>
__global__ __launch_bounds__(64 * WG_RED) void wgrad_batched_reduce_kernel(WgradBatchK t) {
    constexpr int IMG_BLOCKS = WG_IMG(MT, NT) / 64;
    const WgradB& p = t.p[blockIdx.z];
    if ((int)blockIdx.y * (32 * NT) >= p.n) return;
    float sum;
    if (blockIdx.x >= IMG_BLOCKS) {
        if (blockIdx.y != 0 || !p.colsum) return;
        const int m = (blockIdx.x - IMG_BLOCKS) * 64 + (threadIdx.x & 63);
        if (!flex_reduce_rows(p.cs + m, 32 * MT, p.slabs, m < 32 * MT, sum) || m >= p.m) return;
        p.colsum[m] = p.accumulate ? p.colsum[m] + sum : sum;
        return;
    }
    const int e = blockIdx.x * 64 + (threadIdx.x & 63);
    if (!flex_reduce_rows(p.ws + (int64_t)blockIdx.y * p.slabs * WG_IMG(MT, NT) + e, WG_IMG(MT, NT), p.slabs, true, sum)) return;
    const int l = e & 63, r = (e >> 6) & 15, tt = e >> 10;
    const int ti = tt / NT, tj = tt - ti * NT;
    const int i = (r & 3) + 8 * (r >> 2) + 4 * (l >> 5), j = l & 31;
    const int m = MT * i + ti, n = blockIdx.y * (32 * NT) + NT * j + tj;
    if (m >= p.m || n >= p.n) return;
    float* dst = p.c + (int64_t)m * p.ldc + n;
    *dst = p.accumulate ? *dst + sum : sum;
}

template <int MT, int NT>
static int wgrad_batched_launch(const WgradBatchK& t, int count, int slabs, int chunks, bool any_cs, hipStream_t s) {
    hipLaunchKernelGGL((wgrad_batched_kernel<MT, NT>), dim3(slabs, chunks, count), dim3(64 * WG_WAVES), 0, s, t);
    const int cs_blocks = any_cs ? (32 * MT + 63) / 64 : 0;
    hipLaunchKernelGGL((wgrad_batched_reduce_kernel<MT, NT>), dim3(WG_IMG(MT, NT) / 64 + cs_blocks, chunks, count), dim3(64 * WG_RED),
                       0, s, t);
    return flex_launch_status();
}

template <int MT, int NT>
static int wgrad_launch(WgradK p, int chunks, hipStream_t s, const CriticFinishK* rider) {
    if (p.b2) {
        if constexpr (MT == 2 && NT == 5) {
            if (p.cs) hipLaunchKernelGGL((wgrad_kernel<MT, NT, true, true>), dim3(p.slabs, chunks), dim3(64 * WG_WAVES), 0, s, p);
            else hipLaunchKernelGGL((wgrad_kernel<MT, NT, false, true>), dim3(p.slabs, chunks), dim3(64 * WG_WAVES), 0, s, p);
        } else return FLEXNET_EUNSUPPORTED;
    } else if (p.cs) hipLaunchKernelGGL((wgrad_kernel<MT, NT, true>), dim3(p.slabs, chunks), dim3(64 * WG_WAVES), 0, s, p);
    else hipLaunchKernelGGL((wgrad_kernel<MT, NT, false>), dim3(p.slabs, chunks), dim3(64 * WG_WAVES), 0, s, p);
    // the column-sum blocks ride at the end of every grid row; those of column chunks > 0 return at once
    const int cs_blocks = p.cs ? (32 * MT + 63) / 64 : 0;
    if (rider) {
        if constexpr (MT == 2 && NT == 5)
            hipLaunchKernelGGL((wgrad_reduce_kernel<MT, NT, true>), dim3(WG_IMG(MT, NT) / 64 + cs_blocks + rider->blocks, chunks),
                               dim3(64 * WG_RED), 0, s, p, *rider);
        else return FLEXNET_EUNSUPPORTED;
    } else {
        CriticFinishK none;
        none.blocks = 0;                                          // (never read without RIDER)
        hipLaunchKernelGGL((wgrad_reduce_kernel<MT, NT>), dim3(WG_IMG(MT, NT) / 64 + cs_blocks, chunks), dim3(64 * WG_RED), 0, s, p, none);
    }
    return flex_launch_status();
}

// argument checks and the shape class of one problem
static int wgrad_class(const FlexWgradArgs* a, int* mt_out, int* nt_out, int* chunks_out) {
    if (!a || !a->a || !a->b || !a->c || !a->workspace || a->k < 0 || a->m < 1 || a->n < 1) return FLEXNET_EINVAL;
    if (a->lda < a->m || a->ldb < a->n || (a->ldc != 0 && a->ldc < a->n)) return FLEXNET_EINVAL;
    if (a->m > 192 || a->lda >= (1 << 24) || a->ldb >= (1 << 24)) return FLEXNET_EUNSUPPORTED;
    const bool two = a->b2 != nullptr || a->n2 != 0;
    if (two && (!a->b2 || !a->c2 || a->n2 < 1 || a->ldb2 < a->n2 || (a->ldc2 != 0 && a->ldc2 < a->n2))) return FLEXNET_EINVAL;
    const int mt = a->m <= 32 ? 1 : a->m <= 64 ? 2 : 6;
    const int nt = a->n <= 32 ? 1 : a->n <= 64 ? 2 : (mt == 6 ? 2 : 5);
    if (two && (mt != 2 || nt != 5 || a->n % nt != 0 || a->ldb2 >= (1 << 24))) return FLEXNET_EUNSUPPORTED;
    const int n_all = a->n + (two ? a->n2 : 0);
    *mt_out = mt; *nt_out = nt; *chunks_out = (n_all + 32 * nt - 1) / (32 * nt);
    return FLEXNET_OK;
}

// the kernels' view of one problem; `launch_chunks`: the column chunks of everything that shares the launch
static int wgrad_prepare(const FlexWgradArgs* a, int mt, int nt, int chunks, int launch_chunks, WgradK* out) {
    const bool two = a->b2 != nullptr || a->n2 != 0;
    const int64_t img = (int64_t)mt * nt * 1024;
    // thread blocks: about two per CU over all column chunks, at least 64 rows each, within the workspace
    const int64_t ws_floats = a->workspace_floats - WG_CS_FLOATS;
    if (ws_floats < chunks * img) return FLEXNET_EINVAL;
    int64_t slabs = (a->k + 63) / 64;
    // never more than two blocks per CU in total: with 515 blocks the last three ran as a second round (62 -> 3x us at
    // [32 768, 64] x [32 768, 720])
    const int64_t want = 512 / launch_chunks > 0 ? 512 / launch_chunks : 1;
    if (slabs > want) slabs = want;
    if (slabs * chunks * img > ws_floats) slabs = ws_floats / (chunks * img);
    if (slabs > 520) slabs = 520;
    if (slabs < 1) slabs = 1;
    int64_t rpb = (a->k + slabs - 1) / slabs;
    rpb = (rpb + 7) & ~(int64_t)7;
    if (rpb < 8) rpb = 8;
    int64_t ldmax = a->lda > a->ldb ? a->lda : a->ldb;
    if (two && a->ldb2 > ldmax) ldmax = a->ldb2;
    if (rpb * ldmax * 4 >= 0x7fffffffll) return FLEXNET_EUNSUPPORTED;
    slabs = a->k > 0 ? (a->k + rpb - 1) / rpb : 1;
    WgradK p;
    p.a = a->a; p.b = a->b; p.c = a->c; p.ws = a->workspace + WG_CS_FLOATS;
    p.cs = a->colsum ? a->workspace : nullptr; p.colsum = a->colsum;
    p.k = a->k; p.lda = a->lda; p.ldb = a->ldb;
    p.a_floats = a->k > 0 ? (a->k - 1) * a->lda + a->m : 0;
    p.b_floats = a->k > 0 ? (a->k - 1) * a->ldb + a->n : 0;
    p.m = a->m; p.n = a->n; p.rows_per_block = (int)rpb; p.slabs = (int)slabs; p.accumulate = a->accumulate;
    p.ldc = a->ldc > 0 ? a->ldc : a->n;
    p.b2 = two ? a->b2 : nullptr; p.c2 = two ? a->c2 : nullptr; p.ldb2 = two ? a->ldb2 : 0;
    p.b2_floats = two && a->k > 0 ? (a->k - 1) * a->ldb2 + a->n2 : 0;
    p.n2 = two ? a->n2 : 0; p.ldc2 = two ? (a->ldc2 > 0 ? a->ldc2 : a->n2) : 0;
    p.b_cell = a->b_row_cell;
    *out = p;
    return FLEXNET_OK;
}

static int wgrad_run(const FlexWgradArgs* a, void* stream, const CriticFinishK* rider) {
    int mt, nt, chunks;
    int rc = wgrad_class(a, &mt, &nt, &chunks);
    if (rc != FLEXNET_OK) return rc;
    WgradK p;
    rc = wgrad_prepare(a, mt, nt, chunks, chunks, &p);
    if (rc != FLEXNET_OK) return rc;
    hipStream_t s = (hipStream_t)stream;
    switch (mt * 10 + nt) {
        case 11: return wgrad_launch<1, 1>(p, chunks, s, rider);
        case 12: return wgrad_launch<1, 2>(p, chunks, s, rider);
        case 15: return wgrad_launch<1, 5>(p, chunks, s, rider);
        case 21: return wgrad_launch<2, 1>(p, chunks, s, rider);
        case 22: return wgrad_launch<2, 2>(p, chunks, s, rider);
        case 25: return wgrad_launch<2, 5>(p, chunks, s, rider);
        case 61: return wgrad_launch<6, 1>(p, chunks, s, rider);
        case 62: return wgrad_launch<6, 2>(p, chunks, s, rider);
    }
    return FLEXNET_EUNSUPPORTED;
}

// `count` independent problems (include/flexnet.h): every check of every problem first, then one first-stage and one
// second-stage launch per shape class present, classes in the order of wgrad_run's switch, problems in the caller's order.
extern "C" int flexnet_wgrad_batched(const FlexWgradArgs* problems, int32_t count, void* stream) {
    if (!problems || count < 1 || count > FLEXNET_WGRAD_MAX_BATCH) return FLEXNET_EINVAL;
    int cls[FLEXNET_WGRAD_MAX_BATCH], chunks[FLEXNET_WGRAD_MAX_BATCH];
    for (int i = 0; i < count; ++i) {
        const FlexWgradArgs* a = problems + i;
        int mt, nt;
        const int rc = wgrad_class(a, &mt, &nt, &chunks[i]);
        if (rc != FLEXNET_OK) return rc;
        if (a->b2 || a->n2 != 0 || a->b_row_cell) return FLEXNET_EUNSUPPORTED;
        if (a->workspace_floats < 0) return FLEXNET_EINVAL;
        cls[i] = mt * 10 + nt;
    }
    for (int i = 0; i < count; ++i)                               // every problem its own workspace slice
        for (int j = 0; j < i; ++j) {
            const float *bi = problems[i].workspace, *ei = bi + problems[i].workspace_floats;
            const float *bj = problems[j].workspace, *ej = bj + problems[j].workspace_floats;
            if (bi < ej && bj < ei) return FLEXNET_EINVAL;
        }
    static const int classes[8] = {11, 12, 15, 21, 22, 25, 61, 62};
    WgradBatchK tables[8];
    int members[8], grid_x[8], grid_y[8];
    bool any_cs[8];
    for (int c = 0; c < 8; ++c) {
        int total = 0;
        members[c] = 0; grid_x[c] = 0; grid_y[c] = 0; any_cs[c] = false;
        for (int i = 0; i < count; ++i) if (cls[i] == classes[c]) total += chunks[i];
        for (int i = 0; i < count; ++i) {
            if (cls[i] != classes[c]) continue;
            WgradK p;
            const int rc = wgrad_prepare(problems + i, classes[c] / 10, classes[c] % 10, chunks[i], total, &p);
            if (rc != FLEXNET_OK) return rc;
            WgradB& e = tables[c].p[members[c]++];
            e.a = p.a; e.b = p.b; e.c = p.c; e.ws = p.ws; e.colsum = p.colsum;
            e.cs = problems[i].workspace;                     // (the partials are written either way: one instantiation per class)
            e.k = p.k; e.lda = p.lda; e.ldb = p.ldb; e.a_floats = p.a_floats; e.b_floats = p.b_floats;
            e.m = p.m; e.n = p.n; e.rows_per_block = p.rows_per_block; e.slabs = p.slabs; e.accumulate = p.accumulate; e.ldc = p.ldc;
            if (p.slabs > grid_x[c]) grid_x[c] = p.slabs;
            if (chunks[i] > grid_y[c]) grid_y[c] = chunks[i];
            any_cs[c] = any_cs[c] || p.cs != nullptr;
        }
        for (int i = members[c]; i < FLEXNET_WGRAD_MAX_BATCH; ++i) tables[c].p[i] = WgradB{};
    }
    hipStream_t s = (hipStream_t)stream;
    for (int c = 0; c < 8; ++c) {
        if (!members[c]) continue;
        int rc = FLEXNET_EUNSUPPORTED;
        switch (classes[c]) {
            case 11: rc = wgrad_batched_launch<1, 1>(tables[c], members[c], grid_x[c], grid_y[c], any_cs[c], s); break;
            case 12: rc = wgrad_batched_launch<1, 2>(tables[c], members[c], grid_x[c], grid_y[c], any_cs[c], s); break;
            case 15: rc = wgrad_batched_launch<1, 5>(tables[c], members[c], grid_x[c], grid_y[c], any_cs[c], s); break;
            case 21: rc = wgrad_batched_launch<2, 1>(tables[c], members[c], grid_x[c], grid_y[c], any_cs[c], s); break;
            case 22: rc = wgrad_batched_launch<2, 2>(tables[c], members[c], grid_x[c], grid_y[c], any_cs[c], s); break;
            case 25: rc = wgrad_batched_launch<2, 5>(tables[c], members[c], grid_x[c], grid_y[c], any_cs[c], s); break;
            case 61: rc = wgrad_batched_launch<6, 1>(tables[c], members[c], grid_x[c], grid_y[c], any_cs[c], s); break;
            case 62: rc = wgrad_batched_launch<6, 2>(tables[c], members[c], grid_x[c], grid_y[c], any_cs[c], s); break;
        }
        if (rc != FLEXNET_OK) return rc;
    }
    return FLEXNET_OK;
}

extern "C" int flexnet_wgrad(const FlexWgradArgs* a, void* stream) { return wgrad_run(a, stream, nullptr); }

// The critic's first-layer weight gradient with the finish of flexnet_critic_td_backward riding in its second-stage launch
// (include/flexnet.h): call flexnet_critic_td_backward_phases(critic, td, 1, stream) first — this is its phase 2 plus
// flexnet_wgrad(w), one launch fewer.  Only for the [64, 5 n] form the critic's first layer takes (else FLEXNET_EUNSUPPORTED,
// nothing launched: the caller falls back to the two separate calls).
extern "C" int flexnet_wgrad_critic_finish(const FlexWgradArgs* w, const FlexCriticTailArgs* critic, const FlexTdLossArgs* td, void* stream) {
    if (!w || !critic || !td) return FLEXNET_EINVAL;
    const int mt = w->m <= 32 ? 1 : w->m <= 64 ? 2 : 6;
    const int nt = w->n <= 32 ? 1 : w->n <= 64 ? 2 : (mt == 6 ? 2 : 5);
    if (mt != 2 || nt != 5) return FLEXNET_EUNSUPPORTED;
    CriticFinishK k;
    const int rc = critic_finish_prepare(critic, td, &k);
    if (rc != FLEXNET_OK) return rc;
    return wgrad_run(w, stream, &k);
}
