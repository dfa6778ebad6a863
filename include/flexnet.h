/* flexnet.h — C ABI of the learner-side kernels of the flexibility-provision hot path (gfx950).
 *
 * The reference's actor is a PyTorch module evaluated once per environment step and agent:
 *     madrl/agents/rnn_agent.py:13-33  RNNAgent: fc1 -> LayerNorm -> ReLU -> GRUCell -> fc2
 *     madrl/models/model.py:102-140    Model.policy: obs (+ one-hot agent id) -> means, hidden
 * flexnet_actor_forward is that forward pass (inference: no autograd graph) for a whole batch of rows in ONE launch:
 * row r is agent r % n_agents of sample r / n_agents, exactly the [b * n, .] reshape of model.py:110-112.
 * Weights are passed in the layout of the reference's state_dict (row-major [out, in]); the kernel re-lays them out
 * in LDS itself, so a state_dict loaded from the reference works unchanged.
 *
 * Plain pointers and sizes only; every pointer is DEVICE memory (fp32); asynchronous on `stream` (a hipStream_t).
 * Return 0 or a negative FLEXNET_E* code for API errors.
 */
#ifndef FLEXNET_H
#define FLEXNET_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FLEXNET_OK 0
#define FLEXNET_EINVAL (-1)
#define FLEXNET_EHIP (-2)
#define FLEXNET_EUNSUPPORTED (-3)  /* shape outside what the fused kernel holds in LDS: the caller keeps its own path */

#define FLEXNET_HID 64             /* hid_size of madrl/args/default.yaml:33; the kernel maps one lane to one unit */
#define FLEXNET_MAX_OBS 144        /* obs_size = 6 * history (env:370-403), history <= 24 */
#define FLEXNET_MAX_AGENTS 8
#define FLEXNET_MAX_ACT 8

typedef struct {
    int32_t rows;              /* b * n_agents */
    int32_t n_agents;
    int32_t obs_dim;           /* <= FLEXNET_MAX_OBS */
    int32_t act_dim;           /* <= FLEXNET_MAX_ACT */
    int32_t agent_id;          /* 1: fc1 has n_agents one-hot id columns after the obs_dim observation columns (model.py:105-108) */
    int32_t layernorm;         /* args.layernorm (rnn_agent.py:19-20,27-28) */
    float ln_eps;              /* nn.LayerNorm default 1e-5 */
    int32_t variant;           /* 0: matrix-core kernel (v_mfma_f32_32x32x2_f32); 1: the VALU kernel (kept as cross-check) */
    const float* obs;          /* [rows, obs_dim] */
    const float* hidden_in;    /* [rows, 64] */
    const float* fc1_w;        /* [64, obs_dim (+ n_agents)] */
    const float* fc1_b;        /* [64] */
    const float* ln_w;         /* [64] (ignored without layernorm) */
    const float* ln_b;         /* [64] */
    const float* w_ih;         /* [192, 64]  GRUCell.weight_ih, gate order r, z, n */
    const float* w_hh;         /* [192, 64] */
    const float* b_ih;         /* [192] */
    const float* b_hh;         /* [192] */
    const float* fc2_w;        /* [act_dim, 64] */
    const float* fc2_b;        /* [act_dim] */
    float* means;              /* out [rows, act_dim]  (fc2 output: the action mean, rnn_agent.py:32) */
    float* hidden_out;         /* out [rows, 64]       (GRU state, rnn_agent.py:31) */
    /* optional exploration epilogue (all three NULL to skip): utils/util.py:57-64 select_action in training mode with
     * the fixed std of model.py:121-123, and utils/util.py:125-128 translate_action's arithmetic */
    const float* noise;        /* [rows, act_dim] standard normal draws */
    float* action;             /* out [rows, act_dim]  tanh(mean + std * noise) */
    float* env_action;         /* out [rows, act_dim]  0.5 * (clamp(action, low, high) + 1) * (high - low) + low */
    float std, action_low, action_high, pad1;
    /* Alternative to `noise` (leave that NULL): the kernel draws the standard normal numbers itself — Philox4x32-10 keyed
     * by rng_state[0] (seed) with counter (row, action group, rng_state[1] = step), Box-Muller on 24-bit uniforms.  The
     * caller (or flexnet_rollout_pack, given the same pointer) advances rng_state[1] between launches.  variant 0 only. */
    const uint64_t* rng_state; /* device [2] or NULL */
    /* Inputs in a slab ring (the replay ring of flexnet_rollout_pack, written in place by the environment kernel):
     * with `cursor` non-NULL the launch reads obs + cursor[0] * obs_slab_stride and hidden_in + cursor[0] *
     * hid_slab_stride (strides in floats; cursor[0] is read on the device, so the launch replays from a HIP graph). */
    const int64_t* cursor;     /* device [1] or NULL */
    int64_t obs_slab_stride;
    int64_t hid_slab_stride;
    int64_t* cursor_out;       /* device [1] or NULL: one lane writes the slab index this launch read there (never read by
                                  this launch) — the cell the environment's step launch takes its slab from when it files
                                  the transition itself (FLEX_STEP_REPLAY_SINK, include/flexenv.h) */
    /* Training forward (variant 0): what the backward pass of rnn_agent.py:25-33 needs, stored on the way ([rows, 64]
     * each, all six or none): fc1's raw output (before bias / id column / LayerNorm), the GRU input x = ReLU(LayerNorm(.)),
     * the gates r, z, n and the hidden part of the candidate, W_hn h + b_hn.  flexnet_gru_backward consumes them. */
    float* save_z1;
    float* save_x;
    float* save_r;
    float* save_z;
    float* save_n;
    float* save_hn;
    int64_t ring_slabs;        /* flexenv_rollout_burst only (include/flexenv.h): slabs of the two input rings, for the wrap of
                                  the slab index from one step of the burst to the next; 0 elsewhere */
    /* Observations read IN PLACE from an environment's history (include/flexenv.h: flexenv_obs_source; FLEX_STEP_OBS_ROWS):
     * with obs_pushed non-NULL row r's observation is the obs_dim CONTIGUOUS floats at
     *     obs + r * obs_row_stride + ((obs_pushed[(r / n_agents) * obs_pushed_stride] - 1) mod obs_slots + 1) * obs_slot_w
     * (the last obs_slots rows of a mirror ring: no wrap, zeros where the episode had not begun) instead of obs + r * obs_dim;
     * `cursor` / the slab strides then apply to hidden_in only.  obs_slots * obs_slot_w == obs_dim. */
    const int32_t* obs_pushed; /* device, or NULL: obs is [rows, obs_dim] */
    int32_t obs_row_stride, obs_pushed_stride, obs_slots, obs_slot_w;
} FlexActorArgs;

/* rnn_agent.py:25-33 + model.py:102-116 for all rows. */
int flexnet_actor_forward(const FlexActorArgs* args, void* stream);

/* Pointwise backward of the GRUCell and of fc2's input (rnn_agent.py:30-32) for a training batch, from the tensors
 * flexnet_actor_forward saved: with h' = (1 - z) n + z h,
 *     dh'  = d_means @ fc2_w (+ d_hidden_out)
 *     dn~  = dh' (1 - z) (1 - n^2)      dz~ = dh' (h - n) z (1 - z)      dr~ = dn~ (W_hn h + b_hn) r (1 - r)
 *     d_gi = [dr~ | dz~ | dn~]  [rows, 192]   (gradient of W_ih x + b_ih; W_hh's first 128 rows see the same dr~, dz~)
 *     d_gh = [dr~ | dz~ | dn~ r] [rows, 192]  (gradient of W_hh h + b_hh)
 * Weight and bias gradients are then flexnet_wgrad products of d_gi / d_gh with x and h; dx = d_gi @ W_ih.  The previous
 * hidden state takes no gradient (a replayed tensor). */
typedef struct {
    int32_t rows;
    int32_t act_dim;           /* <= FLEXNET_MAX_ACT */
    const float* d_means;      /* [rows, act_dim] */
    const float* d_hidden;     /* [rows, 64] or NULL: gradient arriving at the new hidden state directly */
    const float* fc2_w;        /* [act_dim, 64] */
    const float* r;            /* saved by flexnet_actor_forward */
    const float* z;
    const float* n;
    const float* hn;
    const float* h_prev;       /* [rows, 64] */
    float* d_gi;               /* out [rows, 192] */
    float* d_gh;               /* out [rows, 192] */
    /* Round 3, optional (dz NULL: the pointwise pass above): the first layer's backward in the same launch —
     * dx = d_gi @ W_ih on the matrix cores (never stored), then the backward of x = ReLU(LayerNorm(z1 + fc1.bias + id column
     * of row % n_agents)) (rnn_agent.py:25-29; flexnet_lnrelu_backward's arithmetic): dz [rows, 64] (the gradient of fc1's
     * raw output: flexnet_wgrad against the observations gives fc1's weight gradient) and the four parameter gradients, the
     * id-column sums written through strides (e.g. straight into fc1's gradient: agent stride 1, unit stride its row pitch). */
    const float* w_ih;         /* [192, 64] */
    const float* z1;           /* [rows, 64]  save_z1 of flexnet_actor_forward */
    const float* x;            /* [rows, 64]  save_x, or NULL: ReLU's mask is then recomputed from z1 */
    const float* fc1_w;        /* [64, fc1_ld]: the id columns are read in place (agent_id) */
    const float* fc1_b;        /* [64] or NULL */
    const float* ln_w;         /* [64] (layernorm) */
    const float* ln_b;
    float* dz;                 /* out [rows, 64] */
    float* d_ln_w;             /* out [64] or NULL */
    float* d_ln_b;
    float* d_fc1_b;
    float* d_id;               /* out, n_agents x 64 elements through the two strides below, or NULL */
    float* workspace;          /* >= FLEXNET_LNRELU_WS_FLOATS floats */
    int64_t workspace_floats;
    int64_t d_id_agent_stride, d_id_unit_stride;
    int32_t fc1_ld, obs_dim, n_agents, agent_id, layernorm;
    float ln_eps;
} FlexGruBwdArgs;

int flexnet_gru_backward(const FlexGruBwdArgs* args, void* stream);

/* The centralised critic (madrl/critics/mlp_critic.py:5-34: fc1 -> LayerNorm -> ReLU -> fc2 -> ReLU -> fc3) AFTER its
 * first layer: the caller forms fc1's output z1 from column blocks (maddpg.py:38-54 repeats every agent's observation
 * n times in fc1's input; one GEMM per sample instead of n), these two entry points do the rest — forward, and the
 * backward pass that autograd would otherwise spread over some fifteen kernels.  One lane per hidden unit.
 * Gradient outputs of the backward call are ACCUMULATED into (atomics): the caller zeroes them. */
typedef struct {
    int32_t rows;              /* b * n_agents */
    int32_t layernorm;         /* args.layernorm (mlp_critic.py:12-13,27-28) */
    float ln_eps;
    int32_t variant;           /* 0: matrix-core kernels for the forward and the dz1-only backward; 1: the VALU kernels */
    const float* z1;           /* [rows, 64]  fc1 output; or NULL: z1[r] = z_shared[r / n_agents] + z_id[r % n_agents] */
    const float* ln_w;         /* [64] */
    const float* ln_b;         /* [64] */
    const float* fc2_w;        /* [64, 64] */
    const float* fc2_b;        /* [64] */
    const float* fc3_w;        /* [1, 64] */
    const float* fc3_b;        /* [1] */
    float* q;                  /* out [rows]  (mlp_critic.py:31: v) */
    /* backward only (NULL for the forward call) */
    const float* dq;           /* [rows]      dLoss/dq */
    float* dz1;                /* out [rows, 64] */
    float* d_ln_w;             /* += [64]   (d_fc2_w == NULL: no parameter gradients at all, dz1 only) */
    float* d_ln_b;             /* += [64] */
    float* d_fc2_w;            /* += [64, 64] */
    float* d_fc2_b;            /* += [64] */
    float* d_fc3_w;            /* += [64] */
    float* d_fc3_b;            /* += [1] */
    const float* z_shared;     /* [rows / n_agents, 64]  the part of fc1's output all agents of a sample share (maddpg.py:38-54) */
    const float* z_id;         /* [n_agents, 64]         fc1's one-hot id columns, transposed */
    int32_t n_agents;          /* used with z_shared */
    int32_t overwrite_grads;   /* backward, fixed-order path only: the six parameter gradients are STORED, not added to
                                * (no zero fill by the caller); with the atomic path set: FLEXNET_EINVAL */
    float* d_z_shared;         /* backward, composed input: out [rows / n_agents, 64] = sum over a sample's agents of dz1, or NULL
                                * (set: the contents of dz1 after the call are unspecified, see variant_pgrad32) */
    float* d_z_id;             /* backward, composed input: out [n_agents, 64] = sum over samples of dz1, or NULL (both or none;
                                * needs the workspace) */
    float* workspace;          /* backward: scratch for the per-block partial sums, or NULL */
    int64_t workspace_floats;  /* >= FLEXNET_CRITIC_WS_FLOATS: the parameter gradients are then reduced in a fixed order
                                * (bit-reproducible) by a second small launch; otherwise with atomics */
    int32_t d_z_id_agent_stride;   /* d_z_id element (agent i, unit u) is stored at i * agent_stride + u * unit_stride floats; */
    int32_t d_z_id_unit_stride;    /* 0, 0 = the dense [n_agents, 64] layout (64, 1).  (1, fc1 row length) writes the id */
                                   /* columns of fc1.weight's gradient in place */
    int32_t z_id_agent_stride;     /* the same for the INPUT z_id: (1, fc1 row length) reads the id columns of fc1.weight where */
    int32_t z_id_unit_stride;      /* they are (every kernel stages the [n_agents, 64] table in LDS once per block) */
    /* dz1-only matrix-core backward (d_fc2_w == NULL, variant 0, rows >= 65 536) of a loss that is a scaled mean of q
     * (the policy loss -mean Q(s, pi(s)), maddpg.py:104-107): every row's dLoss/dq is `dq_value` (`dq` is not read), and
     * the kernel — which recomputes the forward anyway — also returns q_mean_scale * sum(q) in *q_mean_out (fixed-order
     * sums, fp64 partials in the workspace).  The two come together; set elsewhere: FLEXNET_EUNSUPPORTED. */
    int32_t dq_uniform;
    float dq_value;
    float q_mean_scale;
    int32_t variant_pgrad32;       /* backward WITH parameter gradients on the matrix cores (rows >= 65 536, fixed-order workspace):
                                    * 0 = 16-row tiles, two wavefronts per SIMD (round 3) — on a composed input with d_z_shared
                                    *     set, in its sample-major form: d_z_shared and d_z_id come out of the backward kernel
                                    *     itself and `dz1` is NOT written (scratch the caller still provides);
                                    * 1 = the 32-row kernel, one wavefront per SIMD, dz1 stored and folded by a second kernel;
                                    * 2 = 16-row tiles over consecutive rows, dz1 stored and folded (cross-checks, A/B) */
    float* q_mean_out;             /* NULL: no sum of q */
} FlexCriticTailArgs;

#define FLEXNET_CRITIC_WS_FLOATS (1024 * 4416)

int flexnet_critic_tail_forward(const FlexCriticTailArgs* args, void* stream);
int flexnet_critic_tail_backward(const FlexCriticTailArgs* args, void* stream);

/* Weight gradient of a linear layer over a tall batch: C[m, n] = sum_k A[k, m] * B[k, n] (A = dLoss/dY, B = the
 * layer's input, k = the batch rows) — what loss.backward() of madrl/utils/trainer.py:62-111 computes for fc1 / the
 * GRUCell / fc2 of rnn_agent.py:13-33 and fc1 of mlp_critic.py:5-34.  fp32 products and sums on the matrix cores
 * (v_mfma_f32_32x32x2_f32), summed over k in a fixed order: bit-reproducible.  m <= 192; else FLEXNET_EUNSUPPORTED. */
typedef struct {
    int64_t k;                 /* rows summed over */
    int64_t lda, ldb;          /* row pitch of A and B in floats (>= m, n): column slices of wider records are fine */
    int64_t workspace_floats;  /* >= FLEXNET_WGRAD_WS_FLOATS */
    int32_t m, n;
    int32_t accumulate;        /* 1: C += result */
    int32_t ldc;               /* row pitch of C in floats; 0 = n (dense).  A column block of a wider weight gradient works */
    const float* a;            /* [k, m] */
    const float* b;            /* [k, n] */
    float* c;                  /* out [m, n] */
    float* workspace;
    float* colsum;             /* out [m] = sum_k A[k, m] (the layer's bias gradient), or NULL */
    /* optional second input block (NULL / 0: none): B is then the column concatenation [b | b2] read in place from its two
     * homes — the critic's observation block and action block, mlp_critic.py:25 after maddpg.py:47-54 — and the result
     * columns n .. n + n2 - 1 go to c2.  One launch instead of two.  n must be a multiple of the kernel's lane width
     * for this shape (5 for 32 < m <= 64 and n > 64; anything else: FLEXNET_EUNSUPPORTED, make two calls). */
    const float* b2;           /* [k, n2] */
    float* c2;                 /* out [m, n2] */
    int64_t ldb2;              /* row pitch of b2 */
    int32_t n2;
    int32_t ldc2;              /* row pitch of c2; 0 = n2 */
    /* optional (NULL: none): B's rows are read in place from a larger row store — the replay's stacked-observation ring —
     * starting at row *b_row_cell (device int64, read by the kernel: a replayed HIP graph follows the sampled window without
     * a copy of it); `b` is then the store's base, rows *b_row_cell .. + k - 1 must lie inside it. */
    const int64_t* b_row_cell;
} FlexWgradArgs;

#define FLEXNET_WGRAD_WS_FLOATS (520 * 12288 + 520 * 192)

int flexnet_wgrad(const FlexWgradArgs* args, void* stream);

/* `count` independent problems C_i = A_i^T B_i in one call — the per-agent weight gradients of `shared_params: False`
 * (madrl/models/model.py:124-138: one RNNAgent and one MLPCritic per agent, each with its own fc1 / GRUCell / fc2 or fc1 / fc2
 * of rnn_agent.py:13-33 and mlp_critic.py:5-34).  One first-stage and one second-stage launch per shape class present (the
 * kernel instantiation flexnet_wgrad picks from m and n), the problem index a grid dimension, the per-problem parameters a
 * table in the kernel arguments: no host-to-device copy.  Row pitches as in flexnet_wgrad — agent i's rows of an interleaved
 * [b, n_agents, .] tensor (a = base + width * i, lda = width * n_agents) and a column block of a wider C are ordinary
 * problems; `colsum` and `accumulate` are per problem.  Every problem brings its own workspace slice (any size from
 * 520 * 192 + one register image per column chunk; a short one lowers that problem's parallelism): overlapping slices
 * are FLEXNET_EINVAL.  Thread blocks per problem come from the launch's total, about two per CU over the whole class.  Sums
 * in a fixed order: bit-reproducible, and count == 1 gives the bits of flexnet_wgrad on the same arguments.
 * b2 / c2, b_row_cell and the critic-finish rider do not exist here: FLEXNET_EUNSUPPORTED.  count outside
 * 1..FLEXNET_WGRAD_MAX_BATCH: FLEXNET_EINVAL.  Every check of every problem comes before the first launch. */
#define FLEXNET_WGRAD_MAX_BATCH (4 * FLEXNET_MAX_AGENTS)
int flexnet_wgrad_batched(const FlexWgradArgs* problems, int32_t count, void* stream);

/* The actor's first-layer epilogue at update batches (rnn_agent.py:25-29 with the one-hot id columns of
 * model.py:105-108 folded in): out = relu(LayerNorm(z + bias + id_cols[r % n_agents])) for z = obs @ W_obs^T, and the
 * backward of that chain with its four parameter gradients (OVERWRITTEN, summed in a fixed order). */
typedef struct {
    int32_t rows, n_agents;
    int32_t layernorm;         /* args.layernorm */
    float ln_eps;
    const float* z;            /* [rows, 64] */
    const float* bias;         /* [64] or NULL */
    const float* id_cols;      /* [n_agents, 64] (fc1.weight[:, obs:obs+n] transposed) or NULL */
    const float* ln_w;         /* [64] */
    const float* ln_b;         /* [64] */
    float* out;                /* forward: [rows, 64] */
    /* backward only */
    const float* dout;         /* [rows, 64] */
    float* dz;                 /* out [rows, 64] */
    float* d_bias;             /* out [64] or NULL */
    float* d_id;               /* out [n_agents, 64] or NULL */
    float* d_ln_w;             /* out [64] or NULL */
    float* d_ln_b;             /* out [64] or NULL */
    float* workspace;
    int64_t workspace_floats;  /* >= FLEXNET_LNRELU_WS_FLOATS */
} FlexLnReluArgs;

#define FLEXNET_LNRELU_WS_FLOATS (1024 * 704)

int flexnet_lnrelu_forward(const FlexLnReluArgs* args, void* stream);
int flexnet_lnrelu_backward(const FlexLnReluArgs* args, void* stream);

/* clip_grad_norm_(params, max_norm) followed by torch.optim.RMSprop.step() (alpha, eps; no momentum, not centred, no
 * weight decay — madrl/utils/trainer.py:34-35,86-90,103-107) for all tensors of one network in two small launches. */
#define FLEXNET_OPT_MAX_TENSORS 16
#define FLEXNET_OPT_MAX_ELEMENTS (1 << 20)
#define FLEXNET_OPT_WS_FLOATS 64
typedef struct {
    int32_t n_tensors;         /* <= FLEXNET_OPT_MAX_TENSORS; tensors whose gradient is None are simply not listed */
    float lr, alpha, eps;
    float max_norm;            /* <= 0: no clipping.  optim.clip_and_step never sends it: clip_grad_norm_ zeroes the gradients at
                                * 0 and turns them round below it, and the wrapper takes the PyTorch calls there.  A NaN norm
                                * reaches every gradient, as torch.clamp hands it on */
    float one_minus_alpha;     /* 1 - alpha rounded from the caller's double, as RMSprop forms it; 0: 1.0f - alpha */
    float* total_norm;         /* out [1]: the pre-clip 2-norm over all listed gradients, or NULL */
    float* workspace;          /* FLEXNET_OPT_WS_FLOATS floats of scratch */
    int64_t numel[FLEXNET_OPT_MAX_TENSORS];      /* a tensor of no elements has no address: not listed either */
    float* param[FLEXNET_OPT_MAX_TENSORS];
    float* grad[FLEXNET_OPT_MAX_TENSORS];        /* scaled in place by the clip factor, as clip_grad_norm_ does */
    float* square_avg[FLEXNET_OPT_MAX_TENSORS];  /* RMSprop state */
    float* step[FLEXNET_OPT_MAX_TENSORS];        /* RMSprop's per-tensor step counter (fp32 scalar, += 1) or NULL */
} FlexClipRmspropArgs;

int flexnet_clip_rmsprop(const FlexClipRmspropArgs* args, void* stream);

/* The value loss of madrl/models/maddpg.py:100-123 behind model.py:308-323's reward normalisation, and its gradient:
 *     r = BatchNorm1d(n)(reward) [train mode];  ret = r + gamma (1 - done) next_q;  loss = mean((ret - q)^2);
 *     dq = dLoss/dq = -2 (ret - q) / (rows n).   The module's running statistics move as nn.BatchNorm1d moves them.
 * With q == NULL (and next_q, dq, loss NULL, normalise = 1) only the statistics pass runs: the running statistics are
 * updated, nothing else — a get_loss call that does not use the value loss still owes the module that update. */
typedef struct {
    int32_t rows, n_agents;    /* [rows, n_agents] tensors; n_agents <= FLEXNET_MAX_AGENTS */
    int32_t normalise;         /* args.reward_normalisation */
    float gamma, bn_eps, bn_momentum;
    const float* reward;       /* [rows, n] raw */
    const float* done;         /* [rows] 0/1 */
    const float* next_q;       /* [rows, n] bootstrap values (no gradient) */
    const float* q;            /* [rows, n] */
    const float* bn_weight;    /* [n] or NULL (1) */
    const float* bn_bias;      /* [n] or NULL (0) */
    float* running_mean;       /* [n] updated in place, or NULL */
    float* running_var;        /* [n] */
    int64_t* num_batches_tracked; /* += 1, or NULL */
    float* dq;                 /* out [rows, n] */
    float* loss;               /* out [1] */
    float* workspace;          /* 8-byte aligned */
    int64_t workspace_floats;  /* >= FLEXNET_TD_WS_FLOATS */
    /* Reward statistics over MORE than this call's rows (data-parallel ranks): run flexnet_td_stats, sum the
     * first FLEXNET_TD_STAT_DOUBLES doubles of the workspace over the ranks (one all-reduce of 8 KB), then make the call
     * with stats_ready = 1 and stat_rows = the rows those sums cover.  0 / 0: the call computes its own statistics. */
    int32_t stats_ready;
    int32_t pad0;
    int64_t stat_rows;
} FlexTdLossArgs;

#define FLEXNET_TD_WS_FLOATS (2 * (64 * 2 * 8 + 1024))
#define FLEXNET_TD_STAT_DOUBLES (64 * 2 * 8)   /* per-block partial sums and sums of squares of the reward columns */

int flexnet_td_loss(const FlexTdLossArgs* args, void* stream);
/* The statistics pass alone (args->reward, rows, n_agents, workspace): per-block partial column sums into the workspace. */
int flexnet_td_stats(const FlexTdLossArgs* args, void* stream);

/* The value loss AND the critic's backward in one pass (maddpg.py:100-123 over mlp_critic.py:25-33): the matrix-core
 * backward kernel recomputes the tail's forward anyway, so it forms q, the TD error, dLoss/dq and the loss partial sums
 * itself — no forward launch of the tail, no q / dq round trip.  `critic`: as for flexnet_critic_tail_backward, `dq`
 * unused; `td`: as for flexnet_td_loss with rows * n_agents == critic->rows; td->q and td->dq are optional OUTPUTS here
 * ([rows * n_agents] each, NULL = not stored).  Covers what the matrix-core backward covers (variant 0, parameter
 * gradients through the fixed-order workspace path, critic->rows >= 65 536); otherwise FLEXNET_EUNSUPPORTED and the caller
 * makes the two separate calls around a forward. */
int flexnet_critic_td_backward(const FlexCriticTailArgs* critic, const FlexTdLossArgs* td, void* stream);
/* The same in separately launchable phases, for callers that overlap the small launches with independent work on another
 * stream (round 5: the statistics pass beside the first-layer GEMM, the finish beside the first layer's weight gradient):
 * phases = 1: the statistics pass (unless td->stats_ready) and the backward kernel; 2: the finish launch (parameter
 * gradients from the partial rows, loss, running statistics) — it needs phase 1 of the same arguments complete on its stream
 * and nothing of flexnet_wgrad's; 3: both, = flexnet_critic_td_backward. */
int flexnet_critic_td_backward_phases(const FlexCriticTailArgs* critic, const FlexTdLossArgs* td, int32_t phases, void* stream);
/* Phase 2 of the above riding in the second-stage launch of the critic's first-layer weight gradient (round 5): what
 * flexnet_critic_td_backward_phases(critic, td, 2, stream) followed by flexnet_wgrad(w, stream) compute, in one launch fewer
 * (model.py:43-50 runs ten value sub-updates per event; a replayed graph's small launches each wait for the one before).
 * Needs phase 1 of the same (critic, td) complete on `stream`.  Only the weight gradient of a 64-unit layer over more than
 * 64 input columns carries the rider: FLEXNET_EUNSUPPORTED otherwise, with nothing launched. */
int flexnet_wgrad_critic_finish(const FlexWgradArgs* w, const FlexCriticTailArgs* critic, const FlexTdLossArgs* td, void* stream);

/* out[0] = scale * sum(x[0 .. n)) in a FIXED order (fp64 partial sums of 64 blocks, one-wavefront finish): the scalar
 * means the losses report — policy_loss = -Q(s, pi(s)).mean() (madrl/models/maddpg.py:107), the entropy of
 * utils/trainer.py:48-56 — without ATen's multi-block reduction, whose global semaphore does not survive a HIP-graph
 * replay on this stack.  No memset, no atomics. */
typedef struct {
    int64_t n;                 /* elements, >= 1 */
    float scale;               /* 1 / n for a mean */
    int32_t pad0;
    const float* x;            /* [n] contiguous */
    float* out;                /* out [1] */
    float* workspace;          /* 8-byte aligned, >= FLEXNET_SUM_WS_FLOATS floats */
    int64_t workspace_floats;
} FlexSumArgs;

#define FLEXNET_SUM_WS_FLOATS (2 * 64)

int flexnet_scaled_sum(const FlexSumArgs* args, void* stream);

/* One vector step's bookkeeping of the rollout (madrl/models/model.py:230-262 per environment, utils/replay_buffer.py:
 * 23-27) in ONE launch.  The replay ring is slab-structured — slab k holds, for every environment of vector step k,
 * the observation the policy acted on, the hidden state it started from, and (once the step has run) its action,
 * reward, done and last_step flags:
 *     obs_ring   [slabs, N, n * obs_dim]      obs(k)
 *     hid_ring   [slabs, N, n * 64]           hidden state going INTO step k (model.py:211,259; zero after a terminal step)
 *     small_ring [slabs, N, small_w]          [action n*act | reward n | done | last_step | pad]
 * Every observation is stored ONCE: the next_state of a transition in slab k is obs(k + 1), the `hid` of model.py:241 is
 * the hidden state of slab k + 1 (zeroed where done = 1 — where the TD target multiplies the bootstrap value by zero
 * anyway, maddpg.py:117) and `last_hid` is the slab's own.  This launch, after step k ran:
 *     slab k     <- action, reward, done (last_step = done; the caller flags the final step of a horizon, model.py:229)
 *     slab k + 1 <- obs_next (skipped when NULL: the environment kernel wrote it there itself, FLEX_STEP_OBS_RING of
 *                   include/flexenv.h), hid_new * (1 - done)
 *     hid_state  <- hid_new * (1 - done)      (hand-over to a policy that does not read the ring; skipped when NULL)
 *     statistics += this step's info / reward / failure sums (fixed-order block sums)
 * Slab indices live on the device (the launch replays from a HIP graph) in two cells, each written by exactly one kernel
 * of the step so that no launch reads a cell it also writes: cursor[0] = the slab the policy reads (advanced HERE, by one
 * lane, when cursor_stepped), cursor[1] = the slab being filled next (advanced by the environment's step kernel,
 * flexenv_set_step_counter, before this launch).  Without an environment counter (cursor_stepped = 0) this launch reads
 * cursor[0] and a one-thread launch behind it advances both cells. */
typedef struct {
    int32_t n_envs, n_agents, obs_dim, act_dim;
    int32_t slabs;             /* ring capacity in slabs, >= 2 */
    int32_t small_w;           /* floats per small record: >= n_agents * act_dim + n_agents + 2 */
    int32_t info_w;            /* columns of `info` (7) */
    int32_t cursor_stepped;    /* 1: cursor[1] was already advanced for this step by flexenv_step; 0: see above */
    const float* action;       /* [N, n, act_dim]  what the replay keeps (model.py:232) */
    const double* reward;      /* [N]   one reward per environment, stored once per agent */
    const float* obs_next;     /* [N, n, obs_dim], or NULL (already in the ring) */
    const uint8_t* done;       /* [N] */
    const float* hid_new;      /* [N, n, 64] */
    const double* info;        /* [N, info_w] or NULL */
    const uint8_t* failed;     /* [N] or NULL */
    float* obs_ring;
    float* hid_ring;
    float* small_ring;
    float* hid_state;          /* out [N, n, 64] or NULL; may alias hid_new */
    int64_t* cursor;           /* [2]: physical slab indices, see above */
    double* info_sum;          /* [info_w] or NULL */
    double* rew_sum;           /* [1] */
    double* fail_sum;          /* [1] or NULL */
    int64_t* rng_state;        /* [2] or NULL: {seed, step}; step += 1 (the actor kernel's noise stream, flexnet_actor_forward) */
} FlexRolloutPackArgs;

int flexnet_rollout_pack(const FlexRolloutPackArgs* args, void* stream);

/* Agent-summed exploration of MATD3 / IDDPG (matd3.py:92-97 + utils/util.py:57-64, iddpg.py:66-71): the policy means of a
 * sample are summed over the AGENT axis, ONE action tanh(sum + std * eps) is drawn and every agent receives it; the env is
 * fed translate_action of it (util.py:125-128).  One launch for what the tensor composition spreads over ~40:
 *     y[e, k]          = tanh(((m[e,0,k] + m[e,1,k]) + ...) + eps[e, k] * std[k])
 *     action[e, i, k]  = y[e, k]
 *     env_action[e, i, k] = 0.5 (clamp(y, low, high) + 1) (high - low) + low
 * every step rounded to fp32 in the order the tensor operations round it (bit-identical to them). */
typedef struct {
    int32_t n_envs, n_agents, act_dim, pad0;
    float act_low, act_high;
    const float* means;        /* [N, n, a] */
    const float* eps;          /* [N, a] standard normal draws; NULL: no exploration, action = the summed mean (no tanh) */
    const float* std;          /* [a] exp of the agent-summed log-std */
    float* action;             /* out [N, n, a] */
    float* env_action;         /* out [N, n, a], or NULL (bootstrap actions of a value loss: no environment behind them) */
} FlexAgentSumArgs;

int flexnet_agent_sum_explore(const FlexAgentSumArgs* args, void* stream);

/* The shared part of the centralised critic's first layer (madrl/critics/mlp_critic.py:25-26 on the input of
 * madrl/models/maddpg.py:33-54) as ONE launch on the matrix cores, exact fp32 (csrc/linear.hip: weights stationary in
 * registers, inputs straight from memory into MFMA operands):
 *     out[b, 0:64] = bias + x1[b, 0:k1] W[:, c1:c1+k1]^T + x2[b, 0:k2] W[:, c2:c2+k2]^T
 * x1 = every agent's observation ([b, n * obs_dim], row pitch ld1), x2 = every agent's action ([b, n * act_dim]; k2 = 0:
 * none), W = fc1.weight as stored ([64, ldw], the id columns between the two blocks are skipped).  k1 a multiple of 8 (an
 * 8-column input piece never straddles the two blocks); k2, ld1, ld2 multiples of 4; x1 / x2 / out 16-byte aligned; at most
 * 768 input columns (k1 + k2 rounded up to a multiple of 32: the weights stay in the registers of eight wavefronts);
 * otherwise FLEXNET_EUNSUPPORTED (the caller keeps the two library GEMMs), nothing launched.  Bit-reproducible: every output
 * is a fixed-order sum of eight matrix-core accumulations. */
typedef struct {
    int64_t rows;
    int32_t k1, k2, ld1, ld2, ldw, c1, c2, pad0;
    const float* x1;           /* [rows, ld1] */
    const float* x2;           /* [rows, ld2] or NULL */
    const float* w;            /* [64, ldw] */
    const float* bias;         /* [64] */
    float* out;                /* out [rows, 64] */
    const int64_t* x1_row_cell; /* optional (NULL: none): as FlexWgradArgs.b_row_cell — x1 is the base of a row store, the rows
                                  of this call start at row *x1_row_cell (device int64) */
} FlexLinear2Args;
int flexnet_linear2(const FlexLinear2Args* args, void* stream);

/* Stacked observations of a replay window out of the ROW ring (include/flexenv.h: FLEX_STEP_OBS_RING) — the gather of the
 * window IS the im2col: the replay keeps every feature row once, [slabs][N][n_agents][FLEX_ROW_FLOATS] =
 * [Pd, Qd, Ppv, V, price, E, older, 0], and output row i (global slot first_slot + i: slab (slot / N) mod slabs, environment
 * slot mod N) becomes env:387-401's [n_agents, 6 * history] observation of that slab:
 *     dst[i][a][h * 6 + f] = row_ring[slab - (history - 1 - h)][env][a][f]   if history - 1 - h <= older(slab, env, a)
 *                          = 0                                              otherwise (before the episode began)
 * (slab indices modulo `slabs`).  The caller keeps the history - 1 slabs behind every window it asks for intact. */
typedef struct {
    const float* row_ring;
    float* dst;                /* out [rows, n_agents * 6 * history], 8-byte aligned */
    int64_t rows;
    int64_t first_slot;
    int32_t n_envs, n_agents, history, slabs;
} FlexWindowArgs;
int flexnet_gather_window(const FlexWindowArgs* args, void* stream);

/* A batch of whole EPISODES out of the slab rings (episodic replay, utils/replay_buffer.py:44-50: the chosen episodes'
 * transitions concatenated in the drawn order) in ONE launch.  Episode i of the table is (first slab counter c0,
 * environment e, length L, first output row off): for j < L, output row off + j of every field is what the window of one
 * transition at global slot (c0 + j) * n_envs + e holds —
 *     state / next_state  the stacked observations of slabs c0 + j and c0 + j + 1: from row_ring by flexnet_gather_window's
 *                         rule (history >= 1, obs_dim = 6 * history), or copied from obs_ring (history = 0);
 *     last_hid / hid      hid_ring at those two slabs;   action | reward | done | last_step   the small record of slab c0 + j;
 *     value / next_value / log_prob_a   v_ring / nv_ring / lp_ring at slab c0 + j, each where ring AND output are given
 * (slab indices modulo `slabs`).  Plain copies.  The table is handed over twice: `episodes` on the device for the kernel,
 * `episodes_host` — the host's mirror of the same [n_episodes][4] int64 — for the checks, so that nothing is read back.
 * The offsets must tile the batch: off[0] = 0, off[i + 1] = off[i] + L[i], the last one ending at `rows`.
 * FLEXNET_EINVAL before any HIP call: a missing ring, table or output (or both / neither of row_ring and obs_ring, a filed
 * ring without its output or the reverse), n_episodes / rows / a dimension < 1, small_w < n_agents * act_dim + n_agents + 2,
 * history not matching the ring (row_ring: obs_dim != 6 * history or history < 1; obs_ring: history != 0), and per episode
 * c0 < 0, e outside [0, n_envs), L < 1, L + history exceeding what `slabs` holds, an offset that is not the running sum, a total
 * other than `rows`.  FLEXNET_EUNSUPPORTED: rows >= 2^31 / FLEXNET_EPISODE_ROWS blocks, with row_ring history > 32 or n_agents >
 * FLEXNET_MAX_AGENTS or a row_ring that is not 16-byte aligned, state / next_state not 8-byte aligned. */
#define FLEXNET_EPISODE_ROWS 4                 /* output rows per thread block */
typedef struct {
    const float* row_ring;                     /* [slabs][n_envs][n_agents * 8], or NULL */
    const float* obs_ring;                     /* [slabs][n_envs][n_agents * obs_dim], or NULL */
    const float* hid_ring;                     /* [slabs][n_envs][n_agents * hid_dim] */
    const float* small_ring;                   /* [slabs][n_envs][small_w] */
    const float* v_ring;                       /* [slabs][n_envs][n_agents], optional */
    const float* nv_ring;                      /* [slabs][n_envs][n_agents], optional */
    const float* lp_ring;                      /* [slabs][n_envs][n_agents * act_dim], optional */
    const int64_t* episodes;                   /* device [n_episodes][4]: c0, e, L, off */
    const int64_t* episodes_host;              /* host mirror of the same table */
    float* state;                              /* out [rows, n_agents * obs_dim] */
    float* next_state;
    float* last_hid;                           /* out [rows, n_agents * hid_dim] */
    float* hid;
    float* action;                             /* out [rows, n_agents * act_dim] */
    float* reward;                             /* out [rows, n_agents] */
    float* done;                               /* out [rows] */
    float* last_step;                          /* out [rows] */
    float* value;                              /* out [rows, n_agents], with v_ring */
    float* next_value;                         /* out [rows, n_agents], with nv_ring */
    float* log_prob_a;                         /* out [rows, n_agents * act_dim], with lp_ring */
    int64_t rows;
    int32_t n_episodes, n_envs, n_agents, history, obs_dim, hid_dim, act_dim, small_w, slabs, pad0;
} FlexEpisodeGatherArgs;
int flexnet_gather_episodes(const FlexEpisodeGatherArgs* args, void* stream);

/* Replay-window refresh: up to FLEXNET_GATHER_MAX_JOBS strided row copies in one launch.  A sampled window of the slab
 * ring (utils/replay_buffer.py:17-21: consecutive transitions) becomes the contiguous static batch a captured sub-update
 * reads; each field is one job (two where the window crosses the ring's seam). */
#define FLEXNET_GATHER_MAX_JOBS 12
typedef struct {
    int32_t n_jobs, pad0;
    const float* src[FLEXNET_GATHER_MAX_JOBS];
    float* dst[FLEXNET_GATHER_MAX_JOBS];
    int64_t rows[FLEXNET_GATHER_MAX_JOBS];
    int32_t width[FLEXNET_GATHER_MAX_JOBS];        /* floats per row */
    int32_t src_stride[FLEXNET_GATHER_MAX_JOBS];   /* floats between rows */
    int32_t dst_stride[FLEXNET_GATHER_MAX_JOBS];
} FlexGatherArgs;

int flexnet_gather_rows(const FlexGatherArgs* args, void* stream);
/* The same launch carrying the reward-statistics pass of the value loss (= flexnet_td_stats(td), model.py:308-323) as extra
 * blocks (round 5): jobs reward_job .. reward_job + reward_jobs - 1 (one, or two for a window that wraps the ring's seam)
 * are the copies of the [td->rows, td->n_agents] reward rows; the statistics are taken from the rows those jobs read, in the
 * partition flexnet_td_stats uses (bit-identical sums), into td->workspace.  The consumer then runs with stats_ready = 1. */
int flexnet_gather_rows_td(const FlexGatherArgs* args, int32_t reward_job, int32_t reward_jobs, const FlexTdLossArgs* td, void* stream);

/* The refresh of a captured sub-update's static batch with the window's first slot read from DEVICE memory (round 5): the
 * form of flexnet_gather_rows a HIP graph can hold — one graph then runs ALL the value sub-updates of an update event
 * (model.py:47-50), each refreshing its batch from its own cell of a device array of window starts, instead of one graph
 * launch per sub-update with a host-side refresh in between (8 us of graph hand-over each).
 * Job j copies rows [start + row_off[j], + rows[j]) (taken modulo ring_rows: a window may wrap the ring's seam) of a ring
 * whose rows are src_stride[j] floats apart, columns base[j] .. + width[j] - 1, into the contiguous dst[j]; cell[k] <-
 * start modulo cell_mod[k] (the in-place windows' first-row cells, nets.RING_VIEWS).  td != NULL: the reward-statistics pass
 * rides in the launch as in flexnet_gather_rows_td, on job reward_job. */
#define FLEXNET_WINDOW_MAX_JOBS 8
#define FLEXNET_WINDOW_MAX_CELLS 4
typedef struct {
    int32_t n_jobs, n_cells;
    const int64_t* start;                                  /* device: the window's first global slot (>= 0) */
    int64_t ring_rows;                                     /* rows of every ring the jobs read (slabs * n_envs) */
    const float* base[FLEXNET_WINDOW_MAX_JOBS];            /* ring row 0, first column of the job */
    float* dst[FLEXNET_WINDOW_MAX_JOBS];
    int64_t rows[FLEXNET_WINDOW_MAX_JOBS];
    int64_t row_off[FLEXNET_WINDOW_MAX_JOBS];
    int32_t width[FLEXNET_WINDOW_MAX_JOBS];
    int32_t src_stride[FLEXNET_WINDOW_MAX_JOBS];
    int64_t* cell[FLEXNET_WINDOW_MAX_CELLS];
    int64_t cell_mod[FLEXNET_WINDOW_MAX_CELLS];
    int32_t reward_job, pad0;                              /* used with td only */
} FlexWindowRefreshArgs;

int flexnet_window_refresh(const FlexWindowRefreshArgs* args, const FlexTdLossArgs* td /* NULL: none */, void* stream);
/* flexnet_clip_rmsprop(opt) followed by flexnet_window_refresh(refresh, td) without a launch for the refresh: inside an update
 * event's graph the optimiser step that ends one value sub-update is followed by the refresh for the next, which depends on
 * nothing the step computes — its copy blocks ride in the norm launch, its statistics blocks in the step launch, where they
 * read the rewards from the copy just made: td->reward must be dst[reward_job] (FLEXNET_EINVAL otherwise).  The caller
 * guarantees that nothing still reads what the refresh writes (trainer.py:81-108 order: the loss's kernels are done). */
int flexnet_clip_rmsprop_refresh(const FlexClipRmspropArgs* opt, const FlexWindowRefreshArgs* refresh, const FlexTdLossArgs* td, void* stream);

/* QMIX mixer of FACMADDPG (madrl/critics/qmix.py:53-81) in the shipped configuration (facmaddpg.yaml: two-layer
 * hypernetworks of width FLEXNET_QMIX_EMBED, mixing_embed_dim FLEXNET_QMIX_EMBED, q_embed_dim 1, not gated, no skip
 * connections).  Weights in the layout of the reference's state_dict.  One wavefront per 32 samples on
 * v_mfma_f32_32x32x2_f32 (exact fp32); no atomics, bit-reproducible, no allocation or host synchronisation.
 * forward:  q_tot [B] from agent_qs [B, n] and state [B, ld_state]; with h1 non-NULL also the first-layer outputs
 *           [B, 256] = [relu(hyper_w_1.0) | relu(hyper_w_final.0) | hyper_b_1 | relu(V.0)] the backward reads.
 * backward: d_agent_qs [B, n] from d_q_tot [B], agent_qs and h1; with want_param_grads also d_w1 [B, 64 n] (gradient of
 *           hyper_w_1.2's output, before abs), d_wf [B, 64] (hyper_w_final.2's output) and d_pre1 [B, 256] (the four
 *           first-layer pre-activations, in h1's column order): the parameter gradients are flexnet_wgrad reductions of
 *           those against h1 and the state.  The backward does not read the state or the first-layer weights.
 * n_agents 1..FLEXNET_MAX_AGENTS, state_dim a multiple of 16 up to FLEXNET_QMIX_MAX_STATE, ld_state a multiple of 4,
 * float4-read tensors 16-byte aligned; else FLEXNET_EUNSUPPORTED (missing tensors: FLEXNET_EINVAL), before any HIP call. */
#define FLEXNET_QMIX_EMBED 64
#define FLEXNET_QMIX_MAX_STATE 1024
typedef struct {
    int64_t batch;             /* B */
    int64_t ld_state;          /* row pitch of state in floats */
    int32_t n_agents;
    int32_t state_dim;         /* S = n_agents * obs_size */
    int32_t want_param_grads;  /* backward: 1 = also d_w1, d_wf, d_pre1 */
    int32_t pad0;
    const float* agent_qs;     /* [B, n] */
    const float* state;        /* [B, ld_state] (forward) */
    const float* w1_0_w;       /* hyper_w_1.0: [64, S], [64] */
    const float* w1_0_b;
    const float* w1_2_w;       /* hyper_w_1.2: [64 n, 64], [64 n] */
    const float* w1_2_b;
    const float* wf_0_w;       /* hyper_w_final.0: [64, S], [64] */
    const float* wf_0_b;
    const float* wf_2_w;       /* hyper_w_final.2: [64, 64], [64] */
    const float* wf_2_b;
    const float* b1_w;         /* hyper_b_1: [64, S], [64] */
    const float* b1_b;
    const float* v_0_w;        /* V.0: [64, S], [64] */
    const float* v_0_b;
    const float* v_2_w;        /* V.2: [1, 64], [1] */
    const float* v_2_b;
    float* q_tot;              /* forward out [B] */
    float* h1;                 /* forward out (optional) / backward in [B, 256] */
    const float* d_q_tot;      /* backward in [B] */
    float* d_agent_qs;         /* backward out [B, n] */
    float* d_w1;               /* backward out [B, 64 n] */
    float* d_wf;               /* backward out [B, 64] */
    float* d_pre1;             /* backward out [B, 256] */
} FlexQmixArgs;

int flexnet_qmix_forward(const FlexQmixArgs* args, void* stream);
int flexnet_qmix_backward(const FlexQmixArgs* args, void* stream);

/* SQDDPG's Shapley-value critic (madrl/models/sqddpg.py:35-104) with a shared MLPCritic, agent_id, hid 64, ReLU.
 * Group g = b * sample_size + s holds a permutation of the agents: pos[g, i] = position of agent i.  Critic row (b, s, i)
 * has first layer z1 = z_shared[b] + z_id[i] + sum over agents j with pos[g, j] <= pos[g, i] of
 * W_act[:, block pos[g, j]] act[b, j] (the reference's coalition-ordered action blocks), then the MLPCritic tail.
 * draw:     one uniform permutation per group from the counter-based stream rng_state = [seed, step] (int64, device);
 *           the caller advances step.  No host synchronisation.
 * forward:  phi [b, n] = mean over s of q, s [b] = sum_i phi (agent order), q [b, ns, n] (each optional, not all NULL).
 * backward: from d_phi [b, n] (and optionally d_q [b, ns, n]) recomputes the forward and writes d_z_shared [b, 64] and
 *           d_act_own [b, n, a] (agent i's own action, the other agents' actions detached) where non-NULL; with
 *           want_param_grads the gradients of z_id, W_act, the LayerNorm, fc2 and fc3, through `workspace`
 *           (FLEXNET_SQDDPG_BWD_GRID * FLEXNET_SQDDPG_WS_ROW floats) and a fixed-order reduction.
 * No atomics: bit-reproducible.  n_agents 1..FLEXNET_MAX_AGENTS, act_dim 1..8 with n * act_dim <= 32, sample_size >= 1
 * with sample_size * n <= 4096, z_shared / z_id / fc2_w 16-byte aligned; else FLEXNET_EUNSUPPORTED.  Missing tensors:
 * FLEXNET_EINVAL.  Both before any HIP call. */
#define FLEXNET_SQDDPG_WS_ROW 6976
#define FLEXNET_SQDDPG_BWD_GRID 1024
typedef struct {
    int64_t groups;            /* b * sample_size */
    int32_t n_agents;
    int32_t pad0;
    const int64_t* rng_state;  /* [seed, step] */
    int32_t* pos;              /* out [groups, n] */
} FlexSqddpgDrawArgs;

typedef struct {
    int64_t batch;             /* b */
    int32_t n_agents;
    int32_t act_dim;
    int32_t sample_size;       /* ns */
    int32_t layernorm;
    float ln_eps;
    int32_t want_param_grads;  /* backward */
    const float* z_shared;     /* [b, 64]: W_obs obs_all + fc1.bias */
    const float* z_id;         /* [n, 64]: the id columns of fc1.weight, transposed */
    const float* w_act;        /* [64, n a]: the action columns of fc1.weight */
    const float* act;          /* [b, n, a] */
    const int32_t* pos;        /* [b ns, n] */
    const float* ln_w;         /* [64], [64] (layernorm) */
    const float* ln_b;
    const float* fc2_w;        /* [64, 64], [64] */
    const float* fc2_b;
    const float* fc3_w;        /* [1, 64], [1] */
    const float* fc3_b;
    float* q;                  /* forward out [b, ns, n] (optional) */
    float* phi;                /* forward out [b, n] (optional) */
    float* s;                  /* forward out [b] (optional) */
    const float* d_phi;        /* backward in [b, n] */
    const float* d_q;          /* backward in [b, ns, n] (optional) */
    float* d_z_shared;         /* backward out [b, 64] (optional) */
    float* d_act_own;          /* backward out [b, n, a] (optional) */
    float* d_z_id;             /* backward out, want_param_grads: [n, 64] */
    float* d_w_act;            /* [64, n a] */
    float* d_ln_w;             /* [64], [64] (layernorm) */
    float* d_ln_b;
    float* d_fc2_w;            /* [64, 64], [64] */
    float* d_fc2_b;
    float* d_fc3_w;            /* [64], [1] */
    float* d_fc3_b;
    float* workspace;          /* FLEXNET_SQDDPG_BWD_GRID * FLEXNET_SQDDPG_WS_ROW floats */
} FlexSqddpgArgs;

int flexnet_sqddpg_draw(const FlexSqddpgDrawArgs* args, void* stream);
int flexnet_sqddpg_forward(const FlexSqddpgArgs* args, void* stream);
int flexnet_sqddpg_backward(const FlexSqddpgArgs* args, void* stream);

/* SQDDPG with shared_params False: one MLPCritic per agent (csrc/sqddpg_unshared.hip).  Row (b, s, i) goes through critic i:
 *     z1 = z_shared[b, i] + z_id[i] + W_act_i x,     x as above from pos,
 * with z_shared[b, i] = W_obs_i obs_all[b] + b1_i formed by the caller ([b, n, 64]) and z_id[i] critic i's OWN id column (no
 * other id column of critic i ever meets a 1).  The weights are read where the modules keep them, through per-agent pointer
 * tables: w_act[i] points at the first action column of critic i's fc1.weight and w_id[i] at its id column i, both with the
 * row pitch ld_fc1 (floats).  One wavefront owns a chunk of whole samples of ONE agent (the agent is a grid dimension); lane
 * `ls` sums its sample's q over s in order.
 * forward:  q [b, ns, n] and phi [b, n] (each optional, not both NULL), the layouts of flexnet_sqddpg_forward.  S = sum_i phi
 *           is the caller's (a sample's agents live in different work-groups).
 * backward: from d_phi [b, n] (and optionally d_q) recomputes the forward and writes d_z_shared [b, n, 64] and d_act_own
 *           [b, n, a] where non-NULL; with want_param_grads, per agent, d_z_id [n, 64], d_w_act [n, 64, n a], d_ln_w / d_ln_b
 *           (layernorm) / d_fc2_b / d_fc3_w [n, 64], d_fc2_w [n, 64, 64], d_fc3_b [n], through per-wavefront partials of a
 *           persistent grid per agent in `workspace` and a fixed-order reduction.  The grid of one agent is at most
 *           FLEXNET_SQDDPG_UNSHARED_BWD_GRID wavefronts; `workspace` holds n_agents * FLEXNET_SQDDPG_UNSHARED_BWD_GRID *
 *           FLEXNET_SQDDPG_UNSHARED_WS_ROW floats.
 * No atomics: bit-reproducible.  Limits as flexnet_sqddpg_*: n_agents 1..FLEXNET_MAX_AGENTS, act_dim 1..8 with n * act_dim <=
 * 32, sample_size >= 1 with sample_size * n <= 4096, z_shared and every fc2_w 16-byte aligned; else FLEXNET_EUNSUPPORTED.  A
 * missing tensor or table entry (of agents 0..n-1), batch < 0, ld_fc1 < n * act_dim: FLEXNET_EINVAL.  Both before any HIP
 * call. */
#define FLEXNET_SQDDPG_UNSHARED_WS_ROW 6528
#define FLEXNET_SQDDPG_UNSHARED_BWD_GRID 256
typedef struct {
    int64_t batch;             /* b */
    int32_t n_agents;
    int32_t act_dim;
    int32_t sample_size;       /* ns */
    int32_t layernorm;
    float ln_eps;
    int32_t want_param_grads;  /* backward */
    int64_t ld_fc1;            /* floats between the rows of every fc1.weight */
    const float* z_shared;     /* [b, n, 64]: W_obs_i obs_all + fc1_i.bias */
    const float* act;          /* [b, n, a] */
    const int32_t* pos;        /* [b ns, n] */
    const float* w_act[FLEXNET_MAX_AGENTS];    /* per agent: fc1.weight + first action column, [64, n a] at pitch ld_fc1 */
    const float* w_id[FLEXNET_MAX_AGENTS];     /* fc1.weight + the agent's own id column, [64] at pitch ld_fc1 */
    const float* ln_w[FLEXNET_MAX_AGENTS];     /* [64] (layernorm) */
    const float* ln_b[FLEXNET_MAX_AGENTS];
    const float* fc2_w[FLEXNET_MAX_AGENTS];    /* [64, 64] */
    const float* fc2_b[FLEXNET_MAX_AGENTS];    /* [64] */
    const float* fc3_w[FLEXNET_MAX_AGENTS];    /* [1, 64] */
    const float* fc3_b[FLEXNET_MAX_AGENTS];    /* [1] */
    float* q;                  /* forward out [b, ns, n] (optional) */
    float* phi;                /* forward out [b, n] (optional) */
    const float* d_phi;        /* backward in [b, n] */
    const float* d_q;          /* backward in [b, ns, n] (optional) */
    float* d_z_shared;         /* backward out [b, n, 64] (optional) */
    float* d_act_own;          /* backward out [b, n, a] (optional) */
    float* d_z_id;             /* backward out, want_param_grads: [n, 64] */
    float* d_w_act;            /* [n, 64, n a] */
    float* d_ln_w;             /* [n, 64] each (layernorm) */
    float* d_ln_b;
    float* d_fc2_w;            /* [n, 64, 64] */
    float* d_fc2_b;            /* [n, 64] */
    float* d_fc3_w;            /* [n, 64] */
    float* d_fc3_b;            /* [n] */
    float* workspace;          /* n_agents * FLEXNET_SQDDPG_UNSHARED_BWD_GRID * FLEXNET_SQDDPG_UNSHARED_WS_ROW floats */
} FlexSqddpgUnsharedArgs;

int flexnet_sqddpg_unshared_forward(const FlexSqddpgUnsharedArgs* args, void* stream);
int flexnet_sqddpg_unshared_backward(const FlexSqddpgUnsharedArgs* args, void* stream);

/* ---- PPO (IPPO / MAPPO): madrl/learning_algorithms/ppo.py:14-69 around the networks (csrc/ppo.hip) ----------------
 * [rows, n_agents] fp32 tensors, n_agents <= FLEXNET_MAX_AGENTS.  Fixed-order reductions, no atomics: bit-reproducible.
 * gae:    reward_norm = BatchNorm(reward) (reward_bn.enabled, else a copy);
 *         delta_i = reward_norm_i + gamma old_next_values_i m_i - old_values_i,  m_i = last_step_i ? 1 - done_i : 1;
 *         advantages_i = delta_i + gamma lambda_ m_i advantages_{i + chain_stride} (0 past the last row): row i continues
 *         into row i + chain_stride — 1: one chain over the batch; N: a time-major window of N environments, N chains.
 *         With adv_bn.enabled also advantages_norm = BatchNorm(advantages).  An enabled module's running statistics
 *         move as a training-mode nn.BatchNorm1d moves them (pointers may be NULL: no tracking).
 *         One lane per chain for chains of up to 256 steps (or >= 16384 chains), else one wavefront per chain scanning
 *         64 steps at a time; any rows / chain_stride >= 1.
 * policy: mu = sum over agents of means;  log p[b, i] = sum_k log N(actions[b, i, k]; mu[b, k], exp(log_std[k]));
 *         ratio = exp(log p - old) with old = old_log_prob[b, i], or sum_k actions[b, i, k] when old_log_prob is NULL
 *         (model.py:313);  loss = -mean(min(ratio A, clamp(ratio, 1 - eps, 1 + eps) A));  d_means = d loss / d means.
 * value:  ret = reward_norm + gamma (1 - done) next_values;  vc = old_values + clamp(values - old_values, -eps, eps);
 *         loss = coef mean(max((values - ret)^2, (vc - ret)^2));  d_values = d loss / d values.
 * Ties: min / max give half of the gradient to each argument where they are equal; clamp passes the gradient on
 * [lo, hi], ends included (PyTorch's subgradients).
 * Missing tensors, a short or misaligned workspace: FLEXNET_EINVAL; n_agents / act_dim beyond the maxima, rows >= 2^28:
 * FLEXNET_EUNSUPPORTED.  Both before any HIP call. */
#define FLEXNET_PPO_BLOCKS 256
#define FLEXNET_PPO_WS_FLOATS (2 * FLEXNET_TD_WS_FLOATS + 2 * FLEXNET_PPO_BLOCKS)
typedef struct {
    int32_t enabled;           /* normalise with this module */
    float eps, momentum;
    int32_t pad0;
    const float* weight;       /* [n] or NULL (1) */
    const float* bias;         /* [n] or NULL (0) */
    float* running_mean;       /* [n] updated in place, or NULL */
    float* running_var;
    int64_t* num_batches_tracked; /* += 1, or NULL */
} FlexPpoBatchNorm;

typedef struct {
    int64_t rows;
    int64_t chain_stride;      /* >= 1 */
    int32_t n_agents;
    float gamma, lambda_;
    int32_t pad0;
    const float* reward;       /* [rows, n] raw */
    const float* old_values;   /* [rows, n] */
    const float* old_next_values;
    const float* done;         /* [rows] 0/1 */
    const float* last_step;    /* [rows] 0/1 */
    FlexPpoBatchNorm reward_bn;
    FlexPpoBatchNorm adv_bn;
    float* reward_norm;        /* out [rows, n] */
    float* advantages;         /* out [rows, n] */
    float* advantages_norm;    /* out [rows, n] (adv_bn.enabled) */
    float* workspace;          /* 8-byte aligned */
    int64_t workspace_floats;  /* >= FLEXNET_PPO_WS_FLOATS */
} FlexPpoGaeArgs;

typedef struct {
    int64_t rows;
    int32_t n_agents, act_dim; /* act_dim <= FLEXNET_MAX_ACT */
    float eps_clip;
    int32_t pad0;
    const float* means;        /* [rows, n, a] */
    const float* log_std;      /* [a]: the agent-summed log-std of the fixed-std policy */
    const float* actions;      /* [rows, n, a] */
    const float* old_log_prob; /* [rows, n] or NULL */
    const float* advantages;   /* [rows, n] */
    float* loss;               /* out [1] */
    float* d_means;            /* out [rows, n, a] */
    float* ratio;              /* out [rows, n] (optional) */
    float* workspace;
    int64_t workspace_floats;  /* >= FLEXNET_PPO_WS_FLOATS */
} FlexPpoPolicyArgs;

typedef struct {
    int64_t rows;
    int32_t n_agents;
    float gamma, eps_clip, value_loss_coef;
    const float* values;       /* [rows, n] */
    const float* old_values;   /* [rows, n] */
    const float* next_values;  /* [rows, n] V(s') of the current network, no gradient */
    const float* reward_norm;  /* [rows, n] from flexnet_ppo_gae */
    const float* done;         /* [rows] */
    float* loss;               /* out [1] */
    float* d_values;           /* out [rows, n] */
    float* returns;            /* out [rows, n] (optional) */
    float* workspace;
    int64_t workspace_floats;  /* >= FLEXNET_PPO_WS_FLOATS */
} FlexPpoValueArgs;

int flexnet_ppo_gae(const FlexPpoGaeArgs* args, void* stream);
int flexnet_ppo_policy_loss(const FlexPpoPolicyArgs* args, void* stream);
int flexnet_ppo_value_loss(const FlexPpoValueArgs* args, void* stream);

/* ---- COMA (madrl/models/coma.py:126-189, continuous branch; csrc/coma.hip) -----------------------------------------
 * baseline: the counterfactual baseline of coma.py:137-149 with a shared MLPCritic, agent_id, hid 64, ReLU.  Critic row
 *         (b, i) is [o_1 .. o_n | o_i | onehot(i) | a_1 .. a_n]; z1 [b n, 64] is its fc1 pre-activation (before the
 *         LayerNorm) on the actions taken.  Row (s, b, i) of the baseline replaces agent i's own action by the draw
 *         sampled[s, b, i], so its pre-activation is z1[b, i] + w_act[:, i a : (i + 1) a] (sampled[s, b, i] - act[b, i]):
 *         a rank-act_dim update, then the MLPCritic tail.  baseline [b, n] = mean over s (summed in the order s = 0, 1, ..:
 *         bit-reproducible); q_sampled [s, b, n] and q [b, n] (the tail of the unmodified z1, from the same pass) are
 *         optional.  Forward only: the baseline enters the loss detached (coma.py:180).
 *         n_agents 1..FLEXNET_MAX_AGENTS, act_dim 1..8 with n * act_dim <= 32, sample_size >= 1, z1 / fc2_w 16-byte
 *         aligned, batch * n < 2^31; else FLEXNET_EUNSUPPORTED.  Missing tensors: FLEXNET_EINVAL.  Both before any HIP call.
 * policy: adv = advantages[b, i] when given, else q[b, i] - baseline[b, i];
 *         log p[b, i] = sum_k avail[b, i, k] log N(actions[b, i, k]; means[b, i, k], exp(log_stds[b, i, k])) (per-agent
 *         means, util.py:42-44 and coma.py:183-185; avail NULL: every action available; log_std_uniform: log_stds is ONE
 *         element);  loss = -mean(adv log p);  d_means = d loss / d means and, where non-NULL, d_log_stds.  Sums in fp64 in
 *         a fixed order.  n_agents <= FLEXNET_MAX_AGENTS, act_dim <= FLEXNET_MAX_ACT. */
#define FLEXNET_COMA_BLOCKS 256
#define FLEXNET_COMA_WS_FLOATS (2 * FLEXNET_COMA_BLOCKS)
typedef struct {
    int64_t batch;             /* b */
    int32_t n_agents;
    int32_t act_dim;
    int32_t sample_size;       /* s */
    int32_t layernorm;
    float ln_eps;
    int32_t pad0;
    const float* z1;           /* [b n, 64] */
    const float* w_act;        /* [64, n a]: the action columns of fc1.weight */
    const float* act;          /* [b, n, a] */
    const float* sampled;      /* [s, b, n, a] */
    const float* ln_w;         /* [64], [64] (layernorm) */
    const float* ln_b;
    const float* fc2_w;        /* [64, 64], [64] */
    const float* fc2_b;
    const float* fc3_w;        /* [1, 64], [1] */
    const float* fc3_b;
    float* baseline;           /* out [b, n] */
    float* q_sampled;          /* out [s, b, n] (optional) */
    float* q;                  /* out [b, n] (optional) */
} FlexComaBaselineArgs;

typedef struct {
    int64_t rows;              /* b */
    int32_t n_agents, act_dim;
    int32_t log_std_uniform;
    int32_t pad0;
    const float* means;        /* [rows, n, a] */
    const float* log_stds;     /* [rows, n, a], or one element (log_std_uniform) */
    const float* actions;      /* [rows, n, a] */
    const float* avail;        /* [rows, n, a] or NULL */
    const float* q;            /* [rows, n] */
    const float* baseline;     /* [rows, n] */
    const float* advantages;   /* [rows, n] or NULL (q - baseline) */
    float* loss;               /* out [1] */
    float* d_means;            /* out [rows, n, a] */
    float* d_log_stds;         /* out [rows, n, a] (optional) */
    float* log_prob;           /* out [rows, n] (optional) */
    float* workspace;          /* 8-byte aligned */
    int64_t workspace_floats;  /* >= FLEXNET_COMA_WS_FLOATS */
} FlexComaPolicyArgs;

int flexnet_coma_baseline(const FlexComaBaselineArgs* args, void* stream);
int flexnet_coma_policy_loss(const FlexComaPolicyArgs* args, void* stream);

/* ---- Gaussian actors (madrl/agents/{rnn,mlp}_agent_gaussian.py, gaussian_policy: True; csrc/gauss.hip) -------------
 * head forward:  u = h w^T + b;  t = tanh(u);  log_std = log_std_min + 0.5 (log_std_max - log_std_min) (t + 1) for
 *         h [rows, 64], w [a, 64].  With means / noise / action (all three, [rows, a]) the exploration of maddpg.py:88
 *         under util.py:56-64 runs in the same launch: action = tanh(means + exp(log_std) noise), and env_action (optional)
 *         = translate_action of it (util.py:125-128).  No log-probability comes back.
 * head backward: d_u = d_log_std 0.5 (log_std_max - log_std_min) (1 - t^2) [rows, a];  d_h = d_u w [rows, 64].  Either
 *         output may be NULL.  dw / db: flexnet_wgrad(d_u, h) with its colsum.
 *         hid == FLEXNET_HID, act_dim <= FLEXNET_MAX_ACT, rows <= 2^30, h / w / d_h 16-byte aligned; else
 *         FLEXNET_EUNSUPPORTED.  Missing tensors: FLEXNET_EINVAL.  Both before any HIP call.
 * sum explore:   the agent-summed selection of iddpg.py:64-70 / matd3.py:91-98 with per-sample standard deviations:
 *         y[e, k] = tanh(((m[e,0,k] + m[e,1,k]) + ..) + exp((ls[e,0,k] + ls[e,1,k]) + ..) eps[e, k]), handed to every
 *         agent, and env_action (optional) = translate_action of it.  n_agents <= FLEXNET_MAX_AGENTS, act_dim <=
 *         FLEXNET_MAX_ACT, n_envs * act_dim < 2^31; else FLEXNET_EUNSUPPORTED.
 * ppo rows:      (csrc/ppo.hip: the other instantiation of flexnet_ppo_policy_loss's one kernel body, with that file's
 *         helpers and finish.)  flexnet_ppo_policy_loss with log_stds [rows, n, a], summed over agents per row like the means:
 *         sigma[b, k] = exp(sum_i log_stds[b, i, k]);  besides d_means, d_log_stds[b, i, k] = sum_j dloss/dlogp[b, j]
 *         ((actions[b, j, k] - mu[b, k])^2 / sigma[b, k]^2 - 1) for every agent i (optional).  Same workspace, fp64 block
 *         sums and finish, same ties.  n_agents / act_dim beyond the maxima, rows >= 2^28: FLEXNET_EUNSUPPORTED. */
typedef struct {
    int64_t rows;
    int32_t act_dim;           /* <= FLEXNET_MAX_ACT */
    int32_t hid;               /* FLEXNET_HID */
    float log_std_min, log_std_max;
    float action_low, action_high;
    const float* h;            /* [rows, 64] (forward) */
    const float* w;            /* [a, 64] */
    const float* b;            /* [a] or NULL (forward) */
    float* log_std;            /* out [rows, a] (forward) */
    float* t;                  /* forward: out [rows, a], optional; backward: in */
    const float* means;        /* [rows, a]: with noise and action, the exploration epilogue */
    const float* noise;        /* [rows, a] standard normal draws */
    float* action;             /* out [rows, a] */
    float* env_action;         /* out [rows, a] (optional) */
    const float* d_log_std;    /* [rows, a] (backward) */
    float* d_u;                /* out [rows, a] (backward, optional) */
    float* d_h;                /* out [rows, 64] (backward, optional) */
} FlexGaussHeadArgs;

typedef struct {
    int32_t n_envs, n_agents, act_dim, pad0;
    float act_low, act_high;
    const float* means;        /* [n_envs, n, a] */
    const float* log_stds;     /* [n_envs, n, a] */
    const float* eps;          /* [n_envs, a] standard normal draws */
    float* action;             /* out [n_envs, n, a] */
    float* env_action;         /* out [n_envs, n, a] (optional) */
} FlexGaussSumArgs;

typedef struct {
    int64_t rows;
    int32_t n_agents, act_dim; /* act_dim <= FLEXNET_MAX_ACT */
    float eps_clip;
    int32_t pad0;
    const float* means;        /* [rows, n, a] */
    const float* log_stds;     /* [rows, n, a] */
    const float* actions;      /* [rows, n, a] */
    const float* old_log_prob; /* [rows, n] or NULL */
    const float* advantages;   /* [rows, n] */
    float* loss;               /* out [1] */
    float* d_means;            /* out [rows, n, a] */
    float* d_log_stds;         /* out [rows, n, a] (optional) */
    float* ratio;              /* out [rows, n] (optional) */
    float* workspace;
    int64_t workspace_floats;  /* >= FLEXNET_PPO_WS_FLOATS */
} FlexPpoPolicyRowsArgs;

int flexnet_gauss_head_forward(const FlexGaussHeadArgs* args, void* stream);
int flexnet_gauss_head_backward(const FlexGaussHeadArgs* args, void* stream);
int flexnet_gauss_sum_explore(const FlexGaussSumArgs* args, void* stream);
int flexnet_ppo_policy_loss_rows(const FlexPpoPolicyRowsArgs* args, void* stream);

/* ---- shared_params: False (madrl/models/model.py:124-138: one RNNAgent per agent; csrc/actor_unshared.hip) ------------
 * flexnet_actor_forward's computation (rnn_agent.py:25-33, the arithmetic of its variant 0) with PER-AGENT weights: row r of
 * the [rows, .] tensors is agent r % n_agents of sample r / n_agents, and agent i's rows use fc1_w[i], fc1_b[i], ... — the
 * modules' own parameter tensors through pointer tables, no stacked copy.  Under agent_id, fc1_w[i] is [64, obs_dim +
 * n_agents] and only its OWN id column obs_dim + i enters (the other one-hot entries are zero).  One wavefront owns 32
 * samples of one agent on v_mfma_f32_32x32x2_f32 (exact fp32).  No exploration epilogue, ring cursor or in-place
 * observations.  The six save_* tensors are those of FlexActorArgs (all six or none).
 * backward: flexnet_gru_backward's fused arithmetic on the same map, from d_means and the saves: d_gi, d_gh [rows, 192], dz
 *         [rows, 64] (dx = d_gi @ w_ih[i] on the matrix cores, never stored), and d_ln_w, d_ln_b (layernorm), d_fc1_b as
 *         [n_agents, 64], each summed over the agent's rows in a fixed order through `workspace`: no atomics,
 *         bit-reproducible.  Agent i's id column of fc1's gradient equals d_fc1_b[i]; its other id columns are zero.  The
 *         weight gradients are flexnet_wgrad products per agent through its row pitches (a = d_gi + 192 i, lda = 192 n, ...).
 * hid 64, ReLU, obs_dim <= FLEXNET_MAX_OBS, n_agents <= FLEXNET_MAX_AGENTS, act_dim <= FLEXNET_MAX_ACT, fp32, contiguous,
 * the [rows, 64] / [rows, 192] tensors and w_ih / w_hh / fc2_w 16-byte aligned; else FLEXNET_EUNSUPPORTED.  Missing
 * tensors, rows % n_agents != 0, a short workspace: FLEXNET_EINVAL.  Both before any HIP call. */
#define FLEXNET_ACTOR_UNSHARED_WS_FLOATS (FLEXNET_MAX_AGENTS * 128 * 192)
typedef struct {
    int32_t rows;              /* b * n_agents */
    int32_t n_agents;
    int32_t obs_dim;
    int32_t act_dim;
    int32_t agent_id;
    int32_t layernorm;
    float ln_eps;
    int32_t pad0;
    const float* obs;          /* [rows, obs_dim] */
    const float* hidden_in;    /* [rows, 64] */
    const float* fc1_w[FLEXNET_MAX_AGENTS];    /* per agent: [64, obs_dim (+ n_agents)] */
    const float* fc1_b[FLEXNET_MAX_AGENTS];    /* [64] */
    const float* ln_w[FLEXNET_MAX_AGENTS];     /* [64] (layernorm) */
    const float* ln_b[FLEXNET_MAX_AGENTS];
    const float* w_ih[FLEXNET_MAX_AGENTS];     /* [192, 64], gate order r, z, n */
    const float* w_hh[FLEXNET_MAX_AGENTS];
    const float* b_ih[FLEXNET_MAX_AGENTS];     /* [192] */
    const float* b_hh[FLEXNET_MAX_AGENTS];
    const float* fc2_w[FLEXNET_MAX_AGENTS];    /* [act_dim, 64] */
    const float* fc2_b[FLEXNET_MAX_AGENTS];    /* [act_dim] */
    float* means;              /* out [rows, act_dim] */
    float* hidden_out;         /* out [rows, 64] */
    float* save_z1;            /* out [rows, 64] each, all six or none (FlexActorArgs.save_*) */
    float* save_x;
    float* save_r;
    float* save_z;
    float* save_n;
    float* save_hn;
} FlexActorUnsharedArgs;

typedef struct {
    int32_t rows;
    int32_t n_agents;
    int32_t obs_dim;
    int32_t act_dim;
    int32_t agent_id;
    int32_t layernorm;
    float ln_eps;
    int32_t pad0;
    const float* d_means;      /* [rows, act_dim] */
    const float* r;            /* the forward's saves, [rows, 64] each */
    const float* z;
    const float* n;
    const float* hn;
    const float* h_prev;       /* [rows, 64]: the forward's hidden_in */
    const float* z1;
    const float* x;
    const float* fc1_w[FLEXNET_MAX_AGENTS];
    const float* fc1_b[FLEXNET_MAX_AGENTS];
    const float* ln_w[FLEXNET_MAX_AGENTS];     /* (layernorm) */
    const float* w_ih[FLEXNET_MAX_AGENTS];
    const float* fc2_w[FLEXNET_MAX_AGENTS];
    float* d_gi;               /* out [rows, 192] */
    float* d_gh;               /* out [rows, 192] */
    float* dz;                 /* out [rows, 64] */
    float* d_ln_w;             /* out [n_agents, 64] (layernorm) */
    float* d_ln_b;
    float* d_fc1_b;            /* out [n_agents, 64] */
    float* workspace;
    int64_t workspace_floats;  /* >= FLEXNET_ACTOR_UNSHARED_WS_FLOATS */
} FlexActorUnsharedBwdArgs;

int flexnet_actor_unshared_forward(const FlexActorUnsharedArgs* args, void* stream);
int flexnet_actor_unshared_backward(const FlexActorUnsharedBwdArgs* args, void* stream);

/* ---- shared_params: False, the critics (madrl/models/model.py:124-138: one MLPCritic per agent; csrc/critic_unshared.hip) ---
 * Every agent's own MLPCritic (madrl/critics/mlp_critic.py:28-35: fc1 -> LayerNorm -> ReLU -> fc2 -> ReLU -> fc3) in one entry
 * point per direction, with PER-AGENT weights through pointer tables (the modules' own tensors, no stacked copy).  Row
 * s * n_agents + a of the [rows, .] tensors is agent a of sample s; q is [b, n_agents].  One wavefront owns 32 samples of one
 * agent on v_mfma_f32_32x32x2_f32 (exact fp32).
 * The first layer's input is described by blocks and never materialised.  Every agent's fc1.weight is [64, w1 + n_id + w2] with
 * the column order [x1 | id columns | x2] (n_id = n_agents under agent_id, else 0); agent a's row of sample s reads
 *     x1 + s * x1_pitch + a * x1_agent_off  (w1 floats)   and   x2 + s * x2_pitch + a * x2_agent_off  (w2 floats, w2 = 0: none)
 * — an agent offset of 0 is a block shared by the sample's agents.  The id block is not read: agent a adds its own column
 * w1 + a.  The four input rows of the reference:
 *     maddpg.py:33-54   x1 = obs [b, n o] shared,     x2 = act [b, n a] shared  (the others' actions detached by the caller)
 *     mappo.py:34-62    x1 = obs [b, n o] shared,     no x2
 *     ippo.py:34-59     x1 = obs [b, n, o] per agent, no x2
 *     iddpg.py:32-59    x1 = obs [b, n, o] per agent, x2 = act [b, n, a] per agent
 * forward: q, and with both save_* set z1 (fc1's output with bias and id column) and x (after LayerNorm and ReLU).  The launch
 *         with and without the saves gives the same bits.
 * backward: from dq [b, n] and the two saves (fc2's output is recomputed): dz1 [rows, 64]; with param_grads also dz2
 *         [rows, 64] and the per-agent sums d_ln_w, d_ln_b (layernorm), d_fc1_b, d_fc2_b, d_fc3_w as [n_agents, 64] and d_fc3_b
 *         [n_agents], each summed over the agent's rows in a fixed order through `workspace` and a second launch: no atomics,
 *         bit-reproducible.  The weight gradients are flexnet_wgrad_batched problems through row pitches: d_fc2_w[a] =
 *         dz2[a]^T x[a], d_fc1_w[a] = dz1[a]^T [x1 | x2] into column blocks; agent a's id column of d_fc1_w equals d_fc1_b[a], its
 *         other id columns are zero.  param_grads = 0 (the policy loss against frozen critics) writes dz1 and d_x2_own only.
 *         d_x2_own (optional) [b, n_agents, own_w] = dz1[s, a, :] @ fc1_w[a][:, w1 + n_id + own_first + a * own_step .. + own_w):
 *         the gradient of agent a's OWN action block (maddpg: own_first 0, own_step act_dim; iddpg: 0, 0).  Observations take
 *         no gradient.
 * hid 64, ReLU, fp32, n_agents <= FLEXNET_MAX_AGENTS, w1 <= FLEXNET_MAX_AGENTS * FLEXNET_MAX_OBS, w2 <= FLEXNET_MAX_AGENTS *
 * FLEXNET_MAX_ACT, own_w <= FLEXNET_MAX_ACT, the [rows, 64] tensors and fc2_w 16-byte aligned; else FLEXNET_EUNSUPPORTED.
 * Missing tensors, rows % n_agents != 0, one save without the other, an own block outside x2, a short workspace:
 * FLEXNET_EINVAL.  Both before any HIP call. */
#define FLEXNET_CRITIC_UNSHARED_WS_FLOATS (FLEXNET_MAX_AGENTS * 128 * 384)
typedef struct {
    int32_t rows;              /* b * n_agents */
    int32_t n_agents;
    int32_t w1, w2;
    int32_t agent_id;
    int32_t layernorm;
    float ln_eps;
    int32_t pad0;
    const float* x1;
    const float* x2;           /* NULL with w2 = 0 */
    int64_t x1_pitch, x2_pitch;            /* floats between samples */
    int64_t x1_agent_off, x2_agent_off;    /* floats between a sample's agents; 0: shared */
    const float* fc1_w[FLEXNET_MAX_AGENTS];    /* per agent: [64, w1 + n_id + w2] */
    const float* fc1_b[FLEXNET_MAX_AGENTS];    /* [64] */
    const float* ln_w[FLEXNET_MAX_AGENTS];     /* [64] (layernorm) */
    const float* ln_b[FLEXNET_MAX_AGENTS];
    const float* fc2_w[FLEXNET_MAX_AGENTS];    /* [64, 64] */
    const float* fc2_b[FLEXNET_MAX_AGENTS];    /* [64] */
    const float* fc3_w[FLEXNET_MAX_AGENTS];    /* [1, 64] */
    const float* fc3_b[FLEXNET_MAX_AGENTS];    /* [1] */
    float* q;                  /* out [b, n_agents] */
    float* save_z1;            /* out [rows, 64] each, both or none */
    float* save_x;
} FlexCriticUnsharedArgs;

typedef struct {
    int32_t rows;
    int32_t n_agents;
    int32_t w1, w2;
    int32_t agent_id;
    int32_t layernorm;
    float ln_eps;
    int32_t param_grads;       /* 0: dz1 and d_x2_own only, no gradient buffer is touched */
    const float* dq;           /* [b, n_agents] */
    const float* z1;           /* the forward's saves */
    const float* x;
    const float* fc1_w[FLEXNET_MAX_AGENTS];
    const float* ln_w[FLEXNET_MAX_AGENTS];     /* (layernorm) */
    const float* fc2_w[FLEXNET_MAX_AGENTS];
    const float* fc2_b[FLEXNET_MAX_AGENTS];
    const float* fc3_w[FLEXNET_MAX_AGENTS];
    float* dz1;                /* out [rows, 64] */
    float* dz2;                /* out [rows, 64] (param_grads) */
    float* d_ln_w;             /* out [n_agents, 64] (param_grads and layernorm) */
    float* d_ln_b;
    float* d_fc1_b;            /* out [n_agents, 64] (param_grads) */
    float* d_fc2_b;
    float* d_fc3_w;
    float* d_fc3_b;            /* out [n_agents] */
    float* d_x2_own;           /* out [b, n_agents, own_w], or NULL */
    int32_t own_first, own_step, own_w, pad1;
    float* workspace;          /* (param_grads) */
    int64_t workspace_floats;  /* >= FLEXNET_CRITIC_UNSHARED_WS_FLOATS */
} FlexCriticUnsharedBwdArgs;

int flexnet_critic_unshared_forward(const FlexCriticUnsharedArgs* args, void* stream);
int flexnet_critic_unshared_backward(const FlexCriticUnsharedBwdArgs* args, void* stream);

/* ---- shared_params: False, MATD3's twin critics (madrl/models/matd3.py:24-27, 74-82; csrc/critic_unshared_twin.hip) ---------
 * The per-agent critics above with MATD3's trailing twin-flag input: every agent's fc1.weight is [64, w1 + n_id + w2 + 1] with
 * the column order [x1 | id columns | x2 | flag], and agent a's critic is evaluated on its row with the flag at 0 (head 0) and
 * at 1 (head 1).  The input blocks, pitches and agent offsets are FlexCriticUnsharedArgs's (matd3.py:33-66 builds maddpg.py's
 * row: x1 = obs [b, n o] shared, x2 = act [b, n a] shared).  The first layer — block products, bias, own id column — is formed
 * ONCE per row and is head 0's pre-activation z1; head 1's is z1 + fc1_w[a][:, last].  Per head: LayerNorm (optional), ReLU,
 * fc2 on the matrix cores, ReLU, fc3.  Same work map: one wavefront owns 32 samples of one agent on v_mfma_f32_32x32x2_f32.
 * FOR EAGER CALLS ONLY: no caller in this project launches either entry point on a stream that is being captured.
 * forward: heads = 1 or 2; q is [heads, b, n_agents] — the memory of the reference's cat([values1, values2], 0).  With both
 *         save_* set: z1 [rows, 64] (head 0's only) and x [heads, rows, 64].  The launch with and without the saves gives the
 *         same bits, and head 0 of a heads = 2 launch equals a heads = 1 launch bit for bit.
 * backward: from dq [heads, b, n_agents] and the saves, per head: fc2's output recomputed, dz2, dx = dz2 @ fc2_w, LayerNorm /
 *         ReLU backward -> that head's dz1.  Always written: dz1_sum [rows, 64], the heads' dz1 added (head 0 first) — d_fc1_w's
 *         x1 and x2 column blocks are flexnet_wgrad_batched problems on it.  With param_grads also dz2 [heads, rows, 64]
 *         (d_fc2_w[a] = dz2[:, a]^T x[:, a] is ONE problem of heads * b rows: in [heads, b, n, 64] agent a's rows keep the pitch
 *         64 n across the head boundary), the per-agent sums d_ln_w, d_ln_b (layernorm), d_fc1_b, d_fc2_b, d_fc3_w as
 *         [n_agents, 64] and d_fc3_b [n_agents], each over both heads, and d_flag [n_agents, 64]: the sum of head 1's dz1 over
 *         the agent's rows, which is the flag column of d_fc1_w[a].  Every sum in a fixed order through `workspace` and a second
 *         launch: no atomics, bit-reproducible.  Agent a's id column of d_fc1_w equals d_fc1_b[a], its other id columns are zero.
 *         d_x2_own (optional) [b, n_agents, own_w] is taken from head 0's dz1 ONLY (matd3.py:123-125: the policy loss reads the
 *         first head) against fc1_w[a][:, w1 + n_id + own_first + a * own_step .. + own_w).  heads = 1, param_grads = 0 is that
 *         policy pass: it writes dz1_sum and d_x2_own only.
 * Limits and their split as above: sizes and alignment FLEXNET_EUNSUPPORTED; missing tensors, rows % n_agents != 0, one save
 * without the other, heads outside {1, 2}, an own block outside x2, a short workspace FLEXNET_EINVAL.  Both before any HIP
 * call. */
#define FLEXNET_CRITIC_UNSHARED_TWIN_WS_FLOATS (FLEXNET_MAX_AGENTS * 128 * 448)
typedef struct {
    int32_t rows;              /* b * n_agents */
    int32_t n_agents;
    int32_t w1, w2;
    int32_t agent_id;
    int32_t layernorm;
    float ln_eps;
    int32_t heads;             /* 1: the flag at 0 only; 2: both */
    const float* x1;
    const float* x2;           /* NULL with w2 = 0 */
    int64_t x1_pitch, x2_pitch;            /* floats between samples */
    int64_t x1_agent_off, x2_agent_off;    /* floats between a sample's agents; 0: shared */
    const float* fc1_w[FLEXNET_MAX_AGENTS];    /* per agent: [64, w1 + n_id + w2 + 1] */
    const float* fc1_b[FLEXNET_MAX_AGENTS];    /* [64] */
    const float* ln_w[FLEXNET_MAX_AGENTS];     /* [64] (layernorm) */
    const float* ln_b[FLEXNET_MAX_AGENTS];
    const float* fc2_w[FLEXNET_MAX_AGENTS];    /* [64, 64] */
    const float* fc2_b[FLEXNET_MAX_AGENTS];    /* [64] */
    const float* fc3_w[FLEXNET_MAX_AGENTS];    /* [1, 64] */
    const float* fc3_b[FLEXNET_MAX_AGENTS];    /* [1] */
    float* q;                  /* out [heads, b, n_agents] */
    float* save_z1;            /* out [rows, 64]; both saves or none */
    float* save_x;             /* out [heads, rows, 64] */
} FlexCriticUnsharedTwinArgs;

typedef struct {
    int32_t rows;
    int32_t n_agents;
    int32_t w1, w2;
    int32_t agent_id;
    int32_t layernorm;
    float ln_eps;
    int32_t param_grads;       /* 0: dz1_sum and d_x2_own only, no gradient buffer is touched */
    int32_t heads;
    int32_t pad0;
    const float* dq;           /* [heads, b, n_agents] */
    const float* z1;           /* the forward's saves: [rows, 64] */
    const float* x;            /* [heads, rows, 64] */
    const float* fc1_w[FLEXNET_MAX_AGENTS];
    const float* ln_w[FLEXNET_MAX_AGENTS];     /* (layernorm) */
    const float* fc2_w[FLEXNET_MAX_AGENTS];
    const float* fc2_b[FLEXNET_MAX_AGENTS];
    const float* fc3_w[FLEXNET_MAX_AGENTS];
    float* dz1_sum;            /* out [rows, 64] */
    float* dz2;                /* out [heads, rows, 64] (param_grads) */
    float* d_ln_w;             /* out [n_agents, 64] (param_grads and layernorm) */
    float* d_ln_b;
    float* d_fc1_b;            /* out [n_agents, 64] (param_grads) */
    float* d_fc2_b;
    float* d_fc3_w;
    float* d_fc3_b;            /* out [n_agents] */
    float* d_flag;             /* out [n_agents, 64]: the flag column of d_fc1_w */
    float* d_x2_own;           /* out [b, n_agents, own_w], or NULL */
    int32_t own_first, own_step, own_w, pad1;
    float* workspace;          /* (param_grads) */
    int64_t workspace_floats;  /* >= FLEXNET_CRITIC_UNSHARED_TWIN_WS_FLOATS */
} FlexCriticUnsharedTwinBwdArgs;

int flexnet_critic_unshared_twin_forward(const FlexCriticUnsharedTwinArgs* args, void* stream);
int flexnet_critic_unshared_twin_backward(const FlexCriticUnsharedTwinBwdArgs* args, void* stream);

/* ---- agent_type: mlp under shared_params: True (madrl/agents/mlp_agent.py:20-32, mlp_agent_gaussian.py; csrc/actor_mlp.hip) ----
 * The MLP actor (fc1 -> LayerNorm -> ReLU -> fc2 -> ReLU = h -> fc3: the MLPCritic's layers with act_dim outputs) in one entry
 * point per direction, with ONE set of weights.  Row s * n_agents + a of the [rows, .] tensors is agent a of sample s.  One
 * wavefront owns 32 samples of one agent on v_mfma_f32_32x32x2_f32 (exact fp32): the agent only selects the id column of fc1
 * and the row of the per-agent sums.  The Gaussian agent's `mean` head goes in the fc3 slot.
 * FOR EAGER CALLS ONLY: no caller in this project launches either entry point on a stream that is being captured into a HIP
 * graph ("the capture rule").
 * forward: obs is [b, n_agents, obs_dim] WITHOUT id columns, read in place with scalar loads (no alignment or width asked of a
 *         row); under agent_id, fc1_w is [64, obs_dim + n_agents] and agent a adds its column obs_dim + a.  Out: means
 *         [rows, act_dim] and h [rows, 64] (always: the module's second result), and with both save_* set z1 (fc1's output
 *         with bias and id column) and x (after LayerNorm and ReLU).  The launch with and without the saves gives the same bits.
 * backward: from d_means [rows, act_dim], the optional d_h [rows, 64] (the gradient the Gaussian agent's log-std head sends to
 *         h) and the saves z1, x, h:  dh = d_means @ fc3_w (+ d_h);  dz2 = dh [h > 0];  dx = dz2 @ fc2_w (matrix cores, never
 *         stored);  LayerNorm / ReLU backward with csrc/lnrelu.hip's arithmetic -> dz1.  Out: dz1, dz2 [rows, 64]; d_ln_w, d_ln_b
 *         (layernorm), d_fc1_b, d_fc2_b [64], d_fc3_b [act_dim]; d_dz1_agent [n_agents, 64], the sum of dz1 over each agent's
 *         rows — the id columns of fc1's gradient, transposed.  Every sum in a fixed order through `workspace` and a second
 *         launch: no atomics, bit-reproducible.  The weight gradients are three flexnet_wgrad_batched problems: d_fc1_w[:, :obs_dim]
 *         = dz1^T obs, d_fc2_w = dz2^T x, d_fc3_w = d_means^T h.  Observations take no gradient.
 * hid == FLEXNET_HID, ReLU, fp32, n_agents <= FLEXNET_MAX_AGENTS, obs_dim <= FLEXNET_MAX_OBS, act_dim <= FLEXNET_MAX_ACT, the
 * [rows, 64] tensors, fc2_w and fc3_w 16-byte aligned; else FLEXNET_EUNSUPPORTED.  Missing tensors, rows % n_agents != 0, one
 * save without the other, LayerNorm without its pair, a short workspace: FLEXNET_EINVAL.  Both before any HIP call; after the
 * checks an entry point computes its grid and launches on `stream`, nothing else. */
#define FLEXNET_ACTOR_MLP_WS_FLOATS (FLEXNET_MAX_AGENTS * 128 * 320)
typedef struct {
    int32_t rows;              /* b * n_agents */
    int32_t n_agents;
    int32_t obs_dim;
    int32_t act_dim;
    int32_t agent_id;
    int32_t layernorm;
    float ln_eps;
    int32_t hid;               /* FLEXNET_HID */
    const float* obs;          /* [rows, obs_dim] */
    const float* fc1_w;        /* [64, obs_dim (+ n_agents)] */
    const float* fc1_b;        /* [64] */
    const float* ln_w;         /* [64] (layernorm) */
    const float* ln_b;
    const float* fc2_w;        /* [64, 64] */
    const float* fc2_b;        /* [64] */
    const float* fc3_w;        /* [act_dim, 64] */
    const float* fc3_b;        /* [act_dim] */
    float* means;              /* out [rows, act_dim] */
    float* h;                  /* out [rows, 64] */
    float* save_z1;            /* out [rows, 64] each, both or none */
    float* save_x;
} FlexActorMlpArgs;

typedef struct {
    int32_t rows;
    int32_t n_agents;
    int32_t obs_dim;
    int32_t act_dim;
    int32_t agent_id;
    int32_t layernorm;
    float ln_eps;
    int32_t hid;
    const float* d_means;      /* [rows, act_dim] */
    const float* d_h;          /* [rows, 64] or NULL */
    const float* z1;           /* the forward's saves */
    const float* x;
    const float* h;            /* the forward's h */
    const float* ln_w;         /* (layernorm) */
    const float* fc2_w;
    const float* fc3_w;
    float* dz1;                /* out [rows, 64] */
    float* dz2;                /* out [rows, 64] */
    float* d_ln_w;             /* out [64] (layernorm) */
    float* d_ln_b;
    float* d_fc1_b;            /* out [64] */
    float* d_fc2_b;            /* out [64] */
    float* d_fc3_b;            /* out [act_dim] */
    float* d_dz1_agent;        /* out [n_agents, 64] */
    float* workspace;
    int64_t workspace_floats;  /* >= FLEXNET_ACTOR_MLP_WS_FLOATS */
} FlexActorMlpBwdArgs;

int flexnet_actor_mlp_forward(const FlexActorMlpArgs* args, void* stream);
int flexnet_actor_mlp_backward(const FlexActorMlpBwdArgs* args, void* stream);

/* ---- agent_type: mlp under shared_params: False (madrl/models/model.py:124-138: one MLPAgent / MLPAgentGaussian per agent;
 * csrc/actor_mlp.hip's per-agent form) ----
 * flexnet_actor_mlp_*'s computation and work map with PER-AGENT weights: row s * n_agents + a of the [rows, .] tensors is agent a
 * of sample s and uses fc1_w[a], fc1_b[a], ... — the modules' own parameter tensors through pointer tables, no stacked copy.  A
 * wavefront owns 32 samples of one agent; a work-group's agent, blockIdx.x % n_agents, selects the weights.  Under agent_id,
 * fc1_w[a] is [64, obs_dim + n_agents] and only its OWN id column obs_dim + a enters (the other one-hot entries are zero).  The
 * Gaussian agent's `mean` head goes in the fc3 slot.
 * FOR EAGER CALLS ONLY, like flexnet_actor_mlp_*: no caller in this project launches either entry point on a stream that is
 * being captured into a HIP graph.
 * forward: means [rows, act_dim] and h [rows, 64] always; with both save_* set also z1 and x.  Same bits with and without.
 * backward: from d_means, the optional d_h [rows, 64] and the saves z1, x, h: dz1, dz2 [rows, 64]; per agent d_ln_w, d_ln_b
 *         (layernorm), d_fc1_b, d_fc2_b as [n_agents, 64] and d_fc3_b as [n_agents, act_dim], each summed over the agent's rows
 *         in a fixed order through `workspace` and a second launch: no atomics, bit-reproducible.  Agent a's id column of
 *         d_fc1_w[a] equals d_fc1_b[a]; its other id columns are zero.  The weight gradients are three flexnet_wgrad_batched
 *         problems per agent through its row pitch (a = dz1 + 64 a, lda = 64 n_agents, ...), all in one call.
 * Limits and return codes are flexnet_actor_mlp_*'s: hid == FLEXNET_HID, ReLU, fp32, n_agents <= FLEXNET_MAX_AGENTS, obs_dim <=
 * FLEXNET_MAX_OBS, act_dim <= FLEXNET_MAX_ACT, the [rows, 64] tensors and every fc2_w / fc3_w 16-byte aligned; else
 * FLEXNET_EUNSUPPORTED.  Missing tensors or table entries, rows % n_agents != 0, one save without the other, LayerNorm without
 * its pair, a short workspace: FLEXNET_EINVAL.  Both before any HIP call; then the grid and the launches on `stream`. */
#define FLEXNET_ACTOR_MLP_UNSHARED_WS_FLOATS (FLEXNET_MAX_AGENTS * 128 * 320)
typedef struct {
    int32_t rows;              /* b * n_agents */
    int32_t n_agents;
    int32_t obs_dim;
    int32_t act_dim;
    int32_t agent_id;
    int32_t layernorm;
    float ln_eps;
    int32_t hid;               /* FLEXNET_HID */
    const float* obs;          /* [rows, obs_dim] */
    const float* fc1_w[FLEXNET_MAX_AGENTS];    /* per agent: [64, obs_dim (+ n_agents)] */
    const float* fc1_b[FLEXNET_MAX_AGENTS];    /* [64] */
    const float* ln_w[FLEXNET_MAX_AGENTS];     /* [64] (layernorm) */
    const float* ln_b[FLEXNET_MAX_AGENTS];
    const float* fc2_w[FLEXNET_MAX_AGENTS];    /* [64, 64] */
    const float* fc2_b[FLEXNET_MAX_AGENTS];    /* [64] */
    const float* fc3_w[FLEXNET_MAX_AGENTS];    /* [act_dim, 64] */
    const float* fc3_b[FLEXNET_MAX_AGENTS];    /* [act_dim] */
    float* means;              /* out [rows, act_dim] */
    float* h;                  /* out [rows, 64] */
    float* save_z1;            /* out [rows, 64] each, both or none */
    float* save_x;
} FlexActorMlpUnsharedArgs;

typedef struct {
    int32_t rows;
    int32_t n_agents;
    int32_t obs_dim;
    int32_t act_dim;
    int32_t agent_id;
    int32_t layernorm;
    float ln_eps;
    int32_t hid;
    const float* d_means;      /* [rows, act_dim] */
    const float* d_h;          /* [rows, 64] or NULL */
    const float* z1;           /* the forward's saves */
    const float* x;
    const float* h;            /* the forward's h */
    const float* ln_w[FLEXNET_MAX_AGENTS];     /* (layernorm) */
    const float* fc2_w[FLEXNET_MAX_AGENTS];
    const float* fc3_w[FLEXNET_MAX_AGENTS];
    float* dz1;                /* out [rows, 64] */
    float* dz2;                /* out [rows, 64] */
    float* d_ln_w;             /* out [n_agents, 64] (layernorm) */
    float* d_ln_b;
    float* d_fc1_b;            /* out [n_agents, 64] */
    float* d_fc2_b;            /* out [n_agents, 64] */
    float* d_fc3_b;            /* out [n_agents, act_dim] */
    float* workspace;
    int64_t workspace_floats;  /* >= FLEXNET_ACTOR_MLP_UNSHARED_WS_FLOATS */
} FlexActorMlpUnsharedBwdArgs;

int flexnet_actor_mlp_unshared_forward(const FlexActorMlpUnsharedArgs* args, void* stream);
int flexnet_actor_mlp_unshared_backward(const FlexActorMlpUnsharedBwdArgs* args, void* stream);

/* ---- gaussian_policy: True under shared_params: False: every agent's own log-std head (csrc/gauss.hip) ----
 * flexnet_gauss_head_*'s arithmetic with PER-AGENT weights: row r of the [rows, .] tensors uses w[r % n_agents] and
 * b[r % n_agents] (pointer tables of the modules' own tensors; b all set or all NULL).  A wavefront owns 32 rows of one agent,
 * so the weights are one uniform pointer per wavefront.  There is no exploration epilogue in this form.
 * forward: log_std [rows, act_dim], and t = tanh(u) (optional).
 * backward: from d_log_std and t: d_u [rows, act_dim] and d_h [rows, 64], either optional.  dw_a / db_a are
 *         flexnet_wgrad_batched problems with the column sum, operands d_u and h at agent a's row pitch.
 * hid == FLEXNET_HID, act_dim <= FLEXNET_MAX_ACT, n_agents <= FLEXNET_MAX_AGENTS, rows <= 2^30, h / d_h / every w 16-byte
 * aligned; else FLEXNET_EUNSUPPORTED.  Missing tensors or table entries, rows % n_agents != 0: FLEXNET_EINVAL.  Both before any
 * HIP call.  Launched eagerly only, like the actors they follow. */
typedef struct {
    int64_t rows;              /* b * n_agents */
    int32_t n_agents;
    int32_t act_dim;           /* <= FLEXNET_MAX_ACT */
    int32_t hid;               /* FLEXNET_HID */
    int32_t pad0;
    float log_std_min, log_std_max;
    const float* h;            /* [rows, 64] (forward) */
    const float* w[FLEXNET_MAX_AGENTS];        /* per agent: [a, 64] */
    const float* b[FLEXNET_MAX_AGENTS];        /* [a], or all NULL (forward) */
    float* log_std;            /* out [rows, a] (forward) */
    float* t;                  /* forward: out [rows, a], optional; backward: in */
    const float* d_log_std;    /* [rows, a] (backward) */
    float* d_u;                /* out [rows, a] (backward, optional) */
    float* d_h;                /* out [rows, 64] (backward, optional) */
} FlexGaussHeadUnsharedArgs;

int flexnet_gauss_head_unshared_forward(const FlexGaussHeadUnsharedArgs* args, void* stream);
int flexnet_gauss_head_unshared_backward(const FlexGaussHeadUnsharedArgs* args, void* stream);

/* flexnet_actor_unshared_backward with the gradient the per-agent log-std heads send to the NEW hidden state: d_hn [rows, 64]
 * (16-byte aligned, not NULL) is added to dh' = d_means @ fc2_w[a] before the gate gradients — what the shared-weight node does
 * with its hidden-state gradient.  A compile-time variant of the same kernel body: flexnet_actor_unshared_backward itself is
 * untouched.  Same checks and return codes; d_hn NULL: FLEXNET_EINVAL.  Launched eagerly only. */
int flexnet_actor_unshared_backward_hn(const FlexActorUnsharedBwdArgs* args, const float* d_hn, void* stream);

/* ---- MAAC: the attention critic (madrl/critics/maac_critic.py:86-159, continuous branch; csrc/attn_critic.hip) ----------------
 * ONE critic for all agents: per agent j an encoder of [o_j | a_j] (enc: [64, obs_dim + act_dim]), a state encoder of o_j
 * (senc: [64, obs_dim]), a critic head on [sa_j | other_j] (c1: [64, 128], c2: [1, 64]) and a bias head on s_j (b1: [64, 64],
 * b2: [1, 64]), all with LeakyReLU(0.01), through per-agent pointer tables; the key, selector and value extractors of the one
 * attention head ([64, 64]; the value extractor with a bias) are shared.  obs is [b, n, obs_dim], act [b, n, act_dim], both
 * contiguous and never concatenated; row s * n_agents + j of the [b n, 64] tensors is agent j of sample s.  One wavefront owns
 * 32 samples with all their agents on v_mfma_f32_32x32x2_f32 (exact fp32).
 * forward: q [b, n] = critic_i - bias_i, and reg [n] = 1e-3 * mean over (samples, other agents) of the UNSCALED logits squared,
 *         through one partial per wavefront and agent in `workspace` (>= ceil(b / 32) * n floats) and a second launch that sums
 *         them in index order: no atomics, bit-reproducible.  sa, key, val are staging tensors the launch always writes (and
 *         the backward reads); the six save_* are all set or all NULL, and q / reg are the same bits either way.
 * backward: from dq [b, n] and what the forward left.  param_grads = 1: the gradients at the seven pre-activations, [b n, 64]
 *         each — dz_sa (encoder), dz_s (state encoder), d_key, d_sel, dz_v (extractors), dz_c (critic fc1), dz_b (bias fc1) —
 *         for flexnet_wgrad_batched, whose column sums are the [64] bias gradients, and d_c2_b / d_b2_b [n] = +- the sum of dq
 *         over the samples (one fp64 partial per wavefront in `workspace`, summed in a fixed order by a second launch); actions take
 *         no gradient.  param_grads = 0:
 *         d_act [b, n, act_dim] alone (the critic frozen).  g_direct, g_other [b n, 64] and g_dl [b, n, n] are scratch.  The
 *         regulariser takes no backward.
 * n_agents 2..FLEXNET_MAX_AGENTS, obs_dim <= FLEXNET_MAX_OBS and a multiple of 4, act_dim <= FLEXNET_MAX_ACT, b <=
 * FLEXNET_ATTN_CRITIC_MAX_BATCH, hid 64, fp32, the [b n, 64] tensors and every [64, 64] / [64, 128] weight 16-byte aligned; else
 * FLEXNET_EUNSUPPORTED.  Missing tensors, some saves without the others, a short workspace: FLEXNET_EINVAL.  Both before any
 * HIP call.  Launched eagerly only (never on a capturing stream). */
#define FLEXNET_ATTN_CRITIC_MAX_BATCH (1 << 24)
typedef struct {
    int64_t batch;             /* b */
    int32_t n_agents;
    int32_t obs_dim;
    int32_t act_dim;
    int32_t pad0;
    const float* obs;          /* [b, n, obs_dim] */
    const float* act;          /* [b, n, act_dim] */
    const float* enc_w[FLEXNET_MAX_AGENTS];    /* per agent: [64, obs_dim + act_dim] */
    const float* enc_b[FLEXNET_MAX_AGENTS];    /* [64] */
    const float* senc_w[FLEXNET_MAX_AGENTS];   /* [64, obs_dim] */
    const float* senc_b[FLEXNET_MAX_AGENTS];
    const float* c1_w[FLEXNET_MAX_AGENTS];     /* [64, 128] */
    const float* c1_b[FLEXNET_MAX_AGENTS];
    const float* c2_w[FLEXNET_MAX_AGENTS];     /* [1, 64] */
    const float* c2_b[FLEXNET_MAX_AGENTS];     /* [1] */
    const float* b1_w[FLEXNET_MAX_AGENTS];     /* [64, 64] */
    const float* b1_b[FLEXNET_MAX_AGENTS];
    const float* b2_w[FLEXNET_MAX_AGENTS];     /* [1, 64] */
    const float* b2_b[FLEXNET_MAX_AGENTS];     /* [1] */
    const float* key_w;        /* [64, 64] */
    const float* sel_w;
    const float* val_w;
    const float* val_b;        /* [64] */
    float* sa;                 /* out [b n, 64]: staging, always written */
    float* key;
    float* val;
    float* q;                  /* out [b, n] */
    float* reg;                /* out [n] */
    float* save_s;             /* out [b n, 64] each, and save_w [b, n, n]: all six or none */
    float* save_sel;
    float* save_other;
    float* save_hc;
    float* save_hb;
    float* save_w;
    float* workspace;
    int64_t workspace_floats;  /* >= ceil(b / 32) * n_agents */
} FlexAttnCriticArgs;

typedef struct {
    int64_t batch;
    int32_t n_agents;
    int32_t obs_dim;
    int32_t act_dim;
    int32_t param_grads;       /* 1: the seven pre-activation gradients; 0: d_act alone */
    const float* dq;           /* [b, n] */
    const float* sa;           /* the forward's staging tensors and saves */
    const float* key;
    const float* val;
    const float* s;            /* (param_grads) */
    const float* sel;
    const float* hc;
    const float* hb;           /* (param_grads) */
    const float* w;            /* [b, n, n] */
    const float* enc_w[FLEXNET_MAX_AGENTS];
    const float* c1_w[FLEXNET_MAX_AGENTS];
    const float* c2_w[FLEXNET_MAX_AGENTS];
    const float* b1_w[FLEXNET_MAX_AGENTS];     /* (param_grads) */
    const float* b2_w[FLEXNET_MAX_AGENTS];     /* (param_grads) */
    const float* key_w;
    const float* sel_w;        /* (param_grads) */
    const float* val_w;
    float* g_direct;           /* scratch [b n, 64] */
    float* g_other;            /* scratch [b n, 64] */
    float* g_dl;               /* scratch [b, n, n] */
    float* dz_c;               /* out [b n, 64] each (param_grads) */
    float* dz_b;
    float* dz_s;
    float* d_sel;
    float* d_key;
    float* dz_v;
    float* dz_sa;
    float* d_act;              /* out [b, n, act_dim] (param_grads == 0) */
    float* d_c2_b;             /* out [n] each (param_grads): the bias gradients of critic_fc2 and bias_fc2, +- sum_b dq */
    float* d_b2_b;
    float* workspace;          /* (param_grads) 8-byte aligned: it holds doubles */
    int64_t workspace_floats;  /* >= 2 * ceil(b / 32) * n_agents */
} FlexAttnCriticBwdArgs;

int flexnet_attn_critic_forward(const FlexAttnCriticArgs* args, void* stream);
int flexnet_attn_critic_backward(const FlexAttnCriticBwdArgs* args, void* stream);

#ifdef __cplusplus
}
#endif
#endif
