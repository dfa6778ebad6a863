// episodes.hip — a batch of whole episodes out of the slab rings in one launch (gfx950): flexnet_gather_episodes.
// Boundary: include/flexnet.h (FlexEpisodeGatherArgs).  Reference: utils/replay_buffer.py:44-50 (EpisodeReplayBuffer.get_batch:
// the drawn episodes' transitions, concatenated in the drawn order).
// Pure data movement; the floor is the HBM writes of state and next_state (2 x rows x n x obs_dim x 4 bytes).  An episode of
// environment e is the strided rows (c0 + j, e) of the time-major rings, so no two output rows share a source run: a block
// of ONE wavefront owns FLEXNET_EPISODE_ROWS consecutive OUTPUT rows, finds the first one's episode by bisection of the
// table's offsets (uniform: scalar loads) and walks on from there.  Stacked observations are formed as in
// gather_window_kernel (the gather is the im2col): the history + 1 slabs of 32-byte records one output row reaches into —
// n_agents x 32 B contiguous per slab — are staged in LDS by 16-byte loads, and state and next_state of the row are both
// formed from them; they leave as 16-byte stores where a row is a whole number of them (n_agents * history even), as 8-byte
// stores otherwise.
// Measured history of the launch at tools/episodic_bench.py's shape (32 680 rows x 5 agents, history 24; 328 MB read +
// written): 256 threads per block, every record pair read straight from cache, 64-bit index arithmetic 175 us; the same with
// the records staged in LDS 169 us (so it was not the scattered reads); one wavefront per block, so that four to six times as
// many rows are in flight per CU, 136 us; a row's hidden-state and small-record loads issued before the staging barrier
// instead of field after field 120 us = 2.7 TB/s, a third of the HBM peak.  What is left is each row's own chain (table,
// loads, barrier, stores) at 4 wavefronts per SIMD; the tensor composition of the same batch takes 1.4 ms.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "flexnet.h"
#include "flex_launch.h"

#define EPISODE_THREADS 64            // one wavefront per block: many rows in flight per CU hide each row's chain of loads
#define EPISODE_MAX_H 32           // histories the staging buffer holds (flexnet_gather_window's limit)

typedef float ep_f2 __attribute__((ext_vector_type(2)));
typedef float ep_f4 __attribute__((ext_vector_type(4)));

// `w` floats from src to dst by the whole block: 16-byte units where both ends allow it
__device__ __forceinline__ void episode_copy(float* dst, const float* src, int w, int tid) {
    if ((w & 3) == 0 && (((uintptr_t)dst | (uintptr_t)src) & 15) == 0) {
        for (int i = tid; i < (w >> 2); i += EPISODE_THREADS)
            reinterpret_cast<ep_f4*>(dst)[i] = reinterpret_cast<const ep_f4*>(src)[i];
    } else {
        for (int i = tid; i < w; i += EPISODE_THREADS) dst[i] = src[i];
    }
}

// two neighbouring floats (an even index x of one agent's 6 * H stacked row) out of the staged records: slot h = x / 6 is
// staged slab h + shift (shift 0: the observation of slab c, 1: of slab c + 1), live if it is no older than the episode
template <int HC>
__device__ __forceinline__ ep_f2 stacked_pair(const float* rec, int shift, int agent, int pitch, int x, int H, float older) {
    const int h = x / 6, f = x - 6 * h, back = (HC ? HC : H) - 1 - h;
    const ep_f2 v = *reinterpret_cast<const ep_f2*>(rec + (h + shift) * pitch + agent * 8 + f);
    return (float)back <= older ? v : ep_f2{0.0f, 0.0f};
}

// stacked observations [n, 6 * H] into dst (V floats per store: 4 or 2) from the H + 1 staged slabs c - (H - 1) .. c + 1.
// HC: the history as a compile-time constant (24: the reference's; the divisions then cost a multiply), 0: H at run time.
template <int V, int HC>
__device__ __forceinline__ void episode_stack(float* dst, const float* rec, int shift, int n, int H, int tid) {
    const int Hc = HC ? HC : H, w = 6 * Hc, units = n * w / V, pitch = n * 8;
    const float* own = rec + (Hc - 1 + shift) * pitch + 6;              // `older` of agent 0 in the observation's own slab
    for (int u = tid; u < units; u += EPISODE_THREADS) {
        const int x0 = u * V, a = x0 / w, x = x0 - a * w;              // (V = 4: w = 6 H may be no multiple of 4 — the second
        const float older = own[a * 8];                                //  pair may then belong to the next agent)
        const ep_f2 p0 = stacked_pair<HC>(rec, shift, a, pitch, x, H, older);
        if (V == 2) {
            *reinterpret_cast<ep_f2*>(dst + x0) = p0;
        } else {
            int a1 = a, x1 = x + 2;
            if (x1 >= w) { a1 = a + 1; x1 = 0; }
            const float older1 = a1 == a ? older : own[a1 * 8];
            const ep_f2 p1 = stacked_pair<HC>(rec, shift, a1, pitch, x1, H, older1);
            *reinterpret_cast<ep_f4*>(dst + x0) = ep_f4{p0.x, p0.y, p1.x, p1.y};
        }
    }
}

template <int V, int HC>
__global__ __launch_bounds__(EPISODE_THREADS) void gather_episodes_kernel(FlexEpisodeGatherArgs a) {
    // the feature records one output row reaches into: slabs c - (H - 1) .. c + 1 of its environment, n x 32 B each
    __shared__ __attribute__((aligned(16))) float rec[(EPISODE_MAX_H + 1) * FLEXNET_MAX_AGENTS * 8];
    const int tid = threadIdx.x;
    const int64_t row0 = (int64_t)blockIdx.x * FLEXNET_EPISODE_ROWS;
    if (row0 >= a.rows) return;
    // the episode of the block's first row: the last one whose offset is <= row0 (offsets ascend from 0: checked on the host)
    int lo = 0, hi = a.n_episodes - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (a.episodes[4 * (int64_t)mid + 3] <= row0) lo = mid; else hi = mid - 1;
    }
    int ep = lo;
    const int n = a.n_agents, N = a.n_envs, slabs = a.slabs;
    const int no = n * a.obs_dim, nh = n * a.hid_dim, na = n * a.act_dim;
    const bool quick = (nh & 3) == 0 && (nh >> 2) <= 2 * EPISODE_THREADS && na + n + 2 <= EPISODE_THREADS &&
                       ((((uintptr_t)a.hid_ring) | ((uintptr_t)a.last_hid) | ((uintptr_t)a.hid)) & 15) == 0;
    for (int r = 0; r < FLEXNET_EPISODE_ROWS; ++r) {
        const int64_t row = row0 + r;
        if (row >= a.rows) return;
        while (ep + 1 < a.n_episodes && a.episodes[4 * (int64_t)(ep + 1) + 3] <= row) ++ep;
        const int64_t c0 = a.episodes[4 * (int64_t)ep], env64 = a.episodes[4 * (int64_t)ep + 1];
        const int64_t len = a.episodes[4 * (int64_t)ep + 2], j = row - a.episodes[4 * (int64_t)ep + 3];
        if (j < 0 || j >= len || env64 < 0 || env64 >= N || c0 < 0) continue;      // (a table the host check would refuse)
        const int env = (int)env64;
        const int cm0 = (int)((c0 + j) % slabs), cm1 = cm0 + 1 >= slabs ? 0 : cm0 + 1;   // physical slabs: uniform, once per row
        const int64_t s0 = (int64_t)cm0 * N + env, s1 = (int64_t)cm1 * N + env;          // ring rows of the two slabs
        // A row's loads all go out before the first of them is waited for: the hidden states and the small record into
        // registers here, the feature records into LDS below (one memory latency per row instead of one per field; `quick`
        // is uniform: what two 16-byte loads and one float per lane hold, n_agents x 64 hidden units and <= 8 actions do)
        ep_f4 h0[2] = {}, h1[2] = {};
        float sm = 0.0f;
        const float* small = a.small_ring + s0 * a.small_w;
        if (quick) {
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                const int i = tid + EPISODE_THREADS * k;
                if (i < (nh >> 2)) {
                    h0[k] = reinterpret_cast<const ep_f4*>(a.hid_ring + s0 * nh)[i];
                    h1[k] = reinterpret_cast<const ep_f4*>(a.hid_ring + s1 * nh)[i];
                }
            }
            if (tid < na + n + 2) sm = small[tid];
        }
        if (a.row_ring) {
            // (everything that decides a `continue` / `return` above is uniform over the block: the barriers are reached by all)
            const int H = HC ? HC : a.history, pitch = n * 8, per = n * 2;
            const int64_t npairs = (int64_t)N * n, ea = (int64_t)env * n;
            __syncthreads();                                            // the previous row's readers are done
            for (int t = tid; t < (H + 1) * per; t += EPISODE_THREADS) {
                const int st = t / per, q = t - st * per;
                int sl = cm0 - (H - 1) + st;                            // in (-slabs, slabs]: H <= slabs - 1 (checked on the host)
                sl = sl < 0 ? sl + slabs : (sl >= slabs ? sl - slabs : sl);
                *reinterpret_cast<ep_f4*>(rec + st * pitch + 4 * q) =
                    *reinterpret_cast<const ep_f4*>(a.row_ring + (sl * npairs + ea) * 8 + 4 * q);
            }
            __syncthreads();
            episode_stack<V, HC>(a.state + row * no, rec, 0, n, H, tid);
            episode_stack<V, HC>(a.next_state + row * no, rec, 1, n, H, tid);
        } else {
            episode_copy(a.state + row * no, a.obs_ring + s0 * no, no, tid);
            episode_copy(a.next_state + row * no, a.obs_ring + s1 * no, no, tid);
        }
        if (quick) {
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                const int i = tid + EPISODE_THREADS * k;
                if (i < (nh >> 2)) {
                    reinterpret_cast<ep_f4*>(a.last_hid + row * nh)[i] = h0[k];
                    reinterpret_cast<ep_f4*>(a.hid + row * nh)[i] = h1[k];
                }
            }
            if (tid < na) a.action[row * na + tid] = sm;
            else if (tid < na + n) a.reward[row * n + (tid - na)] = sm;
            else if (tid == na + n) a.done[row] = sm;
            else if (tid == na + n + 1) a.last_step[row] = sm;
        } else {
            episode_copy(a.last_hid + row * nh, a.hid_ring + s0 * nh, nh, tid);
            episode_copy(a.hid + row * nh, a.hid_ring + s1 * nh, nh, tid);
            for (int i = tid; i < na + n + 2; i += EPISODE_THREADS) {
                const float v = small[i];
                if (i < na) a.action[row * na + i] = v;
                else if (i < na + n) a.reward[row * n + (i - na)] = v;
                else if (i == na + n) a.done[row] = v;
                else a.last_step[row] = v;
            }
        }
        if (a.v_ring) episode_copy(a.value + row * n, a.v_ring + s0 * n, n, tid);
        if (a.nv_ring) episode_copy(a.next_value + row * n, a.nv_ring + s0 * n, n, tid);
        if (a.lp_ring) episode_copy(a.log_prob_a + row * na, a.lp_ring + s0 * na, na, tid);
    }
}

extern "C" int flexnet_gather_episodes(const FlexEpisodeGatherArgs* a, void* stream) {
    if (!a || !a->hid_ring || !a->small_ring || !a->episodes || !a->episodes_host || (a->row_ring != nullptr) == (a->obs_ring != nullptr))
        return FLEXNET_EINVAL;
    if (!a->state || !a->next_state || !a->last_hid || !a->hid || !a->action || !a->reward || !a->done || !a->last_step)
        return FLEXNET_EINVAL;
    if ((a->v_ring != nullptr) != (a->value != nullptr) || (a->nv_ring != nullptr) != (a->next_value != nullptr) ||
        (a->lp_ring != nullptr) != (a->log_prob_a != nullptr))
        return FLEXNET_EINVAL;
    if (a->n_episodes < 1 || a->rows < 1 || a->n_envs < 1 || a->n_agents < 1 || a->obs_dim < 1 || a->hid_dim < 1 || a->act_dim < 1 ||
        a->slabs < 2 || a->history < 0 || (int64_t)a->small_w < (int64_t)a->n_agents * a->act_dim + a->n_agents + 2)
        return FLEXNET_EINVAL;
    if (a->row_ring ? (a->history < 1 || a->obs_dim != 6 * a->history) : a->history != 0) return FLEXNET_EINVAL;
    // a slab's observation reaches history - 1 slabs back, next_state one slab on: an episode of L steps needs L + history slabs
    const int64_t reach = a->row_ring ? a->history : 1;
    int64_t at = 0;
    for (int32_t i = 0; i < a->n_episodes; ++i) {
        const int64_t* e = a->episodes_host + 4 * (int64_t)i;
        if (e[0] < 0 || e[1] < 0 || e[1] >= a->n_envs || e[2] < 1 || e[2] + reach > a->slabs || e[3] != at || e[3] >= a->rows)
            return FLEXNET_EINVAL;
        at += e[2];
    }
    if (at != a->rows) return FLEXNET_EINVAL;
    const int64_t blocks = (a->rows + FLEXNET_EPISODE_ROWS - 1) / FLEXNET_EPISODE_ROWS;
    if (blocks > 0x7fffffffll) return FLEXNET_EUNSUPPORTED;
    // what the staging buffer holds, and 32-bit sizes of one row
    if (a->row_ring && (a->history > EPISODE_MAX_H || a->n_agents > FLEXNET_MAX_AGENTS || !flex_aligned(a->row_ring, 16)))
        return FLEXNET_EUNSUPPORTED;
    if ((int64_t)a->n_agents * a->obs_dim > 0x7fffffffll / 8 || (int64_t)a->n_agents * a->hid_dim > 0x7fffffffll / 8)
        return FLEXNET_EUNSUPPORTED;
    if (!flex_aligned(a->state, 8) || !flex_aligned(a->next_state, 8) || (a->row_ring && !flex_aligned(a->row_ring, 8)))
        return FLEXNET_EUNSUPPORTED;
    const bool wide = a->row_ring && (((int64_t)a->n_agents * a->obs_dim) & 3) == 0 && flex_aligned(a->state, 16) &&
                      flex_aligned(a->next_state, 16);
    const dim3 grid((unsigned)blocks), block(EPISODE_THREADS);
    hipStream_t st = (hipStream_t)stream;
    if (wide && a->history == 24) hipLaunchKernelGGL((gather_episodes_kernel<4, 24>), grid, block, 0, st, *a);
    else if (wide) hipLaunchKernelGGL((gather_episodes_kernel<4, 0>), grid, block, 0, st, *a);
    else hipLaunchKernelGGL((gather_episodes_kernel<2, 0>), grid, block, 0, st, *a);
    return flex_launch_status();
}
