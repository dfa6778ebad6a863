// wgrad_block.h — the body of wgrad.hip's first-stage kernels, included INSIDE a kernel whose scope provides MT, NT, CS, TWO and the
// problem `p` (a WgradK): wgrad_kernel and wgrad_batched_kernel share this text and nothing else, so that the batched form adds
// no instruction to wgrad_kernel.  (No include guard: it is a fragment, included once per kernel.)
    __shared__ float fold[WG_IMG(MT, NT)];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t k0 = (int64_t)blockIdx.x * p.rows_per_block;
    const int64_t left = p.k - k0;
    const int rows = left < p.rows_per_block ? (int)left : p.rows_per_block;
    const int n0 = blockIdx.y * (32 * NT);
    // buffer views of this block's rows: anything past them (other blocks' rows, the end of the allocation) reads 0
    int64_t fa = (int64_t)rows * p.lda, fb = (int64_t)rows * p.ldb - n0;
    const int64_t ea = p.a_floats - k0 * p.lda, eb = p.b_floats - k0 * p.ldb - n0;
    if (ea < fa) fa = ea;
    if (eb < fb) fb = eb;
    const __amdgpu_buffer_rsrc_t ra = wg_rsrc(p.a + k0 * p.lda, fa);
    const float* const pb = p.b + (p.b_cell ? *p.b_cell * p.ldb : 0);
    const __amdgpu_buffer_rsrc_t rb = wg_rsrc(pb + k0 * p.ldb + n0, fb);
    // TWO: a lane's NT columns lie in b (virtual column < n) or in b2 (n is a multiple of NT: never astride); it loads
    // from both views every step with the offset of the other one out of range (-> zeros) and keeps its own
    int64_t fb2 = 0;
    if (TWO) {
        fb2 = (int64_t)rows * p.ldb2;
        const int64_t eb2 = p.b2_floats - k0 * p.ldb2;
        if (eb2 < fb2) fb2 = eb2;
    }
    const __amdgpu_buffer_rsrc_t rb2 = wg_rsrc(TWO ? p.b2 + k0 * p.ldb2 : p.b, TWO ? fb2 : 0);

    v16f acc[MT][NT];
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int j = 0; j < NT; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.0f;

    // step s of the block: rows 2 s, 2 s + 1; wavefront w takes steps w, w + 4, ...
    const int col = lane & 31, half = lane >> 5;
    const int steps = (rows + 1) >> 1;
    const int lda4 = (int)p.lda * 4, ldb4 = (int)p.ldb * 4;
    int offa = (2 * wave + half) * lda4 + col * (MT * 4);
    int offb = (2 * wave + half) * ldb4 + col * (NT * 4);
    const int stepa = 2 * WG_WAVES * lda4, stepb = 2 * WG_WAVES * ldb4;
    // (offsets are advanced as unsigned numbers: an out-of-range lane starts at 2^31 and stays past every view, whose
    // size is below 2^31 bytes by the dispatcher's check on rows_per_block)
    unsigned offb2 = 0x80000000u, stepb2 = 0;
    bool in_b2 = false;
    if (TWO) {
        const int vcol = n0 + NT * col - p.n;            // this lane's first column, counted from the start of b2
        in_b2 = vcol >= 0;
        stepb2 = 2 * WG_WAVES * (unsigned)p.ldb2 * 4u;
        if (in_b2) {
            offb2 = (unsigned)((2 * wave + half) * (int)p.ldb2 * 4 + vcol * 4);
            offb = (int)0x80000000u;
        }
    }
    const int mine = steps > wave ? (steps - wave + WG_WAVES - 1) / WG_WAVES : 0;

    constexpr int U = WG_UNROLL(MT, NT);
    constexpr int D = WG_DEPTH(MT, NT);
    float av[D][U][MT], bv[D][U][NT];
    float bw[TWO ? D : 1][TWO ? U : 1][NT];
    float csum[MT];                  // this lane's share of sum_k A[k, MT * col + i] (the bias gradient)
#pragma unroll
    for (int i = 0; i < MT; ++i) csum[i] = 0.0f;
    const bool want_cs = CS && blockIdx.y == 0;
    if (TWO) {
#pragma unroll
        for (int d = 0; d < D; ++d)
#pragma unroll
            for (int u = 0; u < U; ++u)
#pragma unroll
                for (int j = 0; j < NT; ++j) { bv[d][u][j] = 0.0f; bw[d][u][j] = 0.0f; }
    }
    auto issue = [&](int buf) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
            wg_load<MT>(ra, offa, av[buf][u]);
            offa += stepa;
            if constexpr (TWO) {
                // both views, unconditionally: the view a column chunk does not touch is out of range for every lane and its
                // loads return zeros without memory traffic.  (Skipping them with `if (has1)` / `if (has2)` put uniform
                // branches — and the waits behind them — into the prefetch: 51.2 -> 47.2 us at [32 768, 64] x [720 | 20].)
                wg_load<NT>(rb, offb, bv[buf][u]);
                wg_load<NT>(rb2, (int)offb2, bw[buf][u]);
                offb = (int)((unsigned)offb + (unsigned)stepb);
                offb2 += stepb2;
            } else {
                wg_load<NT>(rb, offb, bv[buf][u]);
                offb += stepb;
            }
        }
    };
    auto multiply = [&](int buf) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
            float bsel[NT];
#pragma unroll
            for (int j = 0; j < NT; ++j) bsel[j] = (TWO && in_b2) ? bw[TWO ? buf : 0][TWO ? u : 0][j] : bv[buf][u][j];
#pragma unroll
            for (int i = 0; i < MT; ++i)
#pragma unroll
                for (int j = 0; j < NT; ++j) {
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[buf][u][i], bsel[j], acc[i][j], 0, 0, 0);
                }
        }
        if (CS) {                    // (every column chunk adds; only chunk 0 stores)
#pragma unroll
            for (int u = 0; u < U; ++u)
#pragma unroll
                for (int i = 0; i < MT; ++i) csum[i] += av[buf][u][i];
        }
    };
    // D register buffers in rotation, D - 1 groups of loads in flight behind the one being multiplied.  Rows past the
    // block's end lie outside the buffer views and load 0 (0 * 0 adds nothing), so the trip count is rounded up to a
    // whole rotation and the loads issued past the last group are harmless.
    const int groups = (mine + U - 1) / U;
    if (groups > 0) {
#pragma unroll
        for (int d = 0; d < D - 1; ++d) issue(d);
        for (int g = 0; g < groups; g += D) {
#pragma unroll
            for (int d = 0; d < D; ++d) {
                // the loads of the group D - 1 ahead go out BEFORE this group's products and stay there: left alone, the
                // instruction scheduler sinks them to a few MFMAs before their use (to shorten register lifetimes), which
                // turns the prefetch distance from a whole group (~1500 cycles of MFMA) into ~500 and the loop latency-bound
                issue((d + D - 1) % D);
                __builtin_amdgcn_sched_barrier(0);
                multiply(d);
                __builtin_amdgcn_sched_barrier(0);
            }
        }
    }

    if (want_cs) {                   // lanes l and l + 32 hold the same columns; then the four wavefronts in order
        __shared__ float cfold[WG_WAVES][32 * MT];
#pragma unroll
        for (int i = 0; i < MT; ++i) {
            const float s = csum[i] + __shfl_xor(csum[i], 32);
            if (half == 0) cfold[wave][col * MT + i] = s;
        }
        __syncthreads();
        for (int e = threadIdx.x; e < 32 * MT; e += 64 * WG_WAVES) {
            float s = cfold[0][e];
#pragma unroll
            for (int w = 1; w < WG_WAVES; ++w) s += cfold[w][e];
            p.cs[(int64_t)blockIdx.x * (32 * MT) + e] = s;
        }
    }

    // fold the four wavefronts' register images in LDS, wavefront 0 first
#pragma unroll
    for (int w = 0; w < WG_WAVES; ++w) {
        if (wave == w) {
#pragma unroll
            for (int i = 0; i < MT; ++i)
#pragma unroll
                for (int j = 0; j < NT; ++j)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int e = ((i * NT + j) * 16 + r) * 64 + lane;
                        if (w == 0) fold[e] = acc[i][j][r];
                        else if (w < WG_WAVES - 1) fold[e] += acc[i][j][r];
                        else acc[i][j][r] += fold[e];
                    }
        }
        __syncthreads();
    }
    if (wave != WG_WAVES - 1) return;
    float* out = p.ws + ((int64_t)blockIdx.y * p.slabs + blockIdx.x) * WG_IMG(MT, NT);
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int j = 0; j < NT; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) out[((i * NT + j) * 16 + r) * 64 + lane] = acc[i][j][r];
