"""MADDPG / SAFEMADDPG on device-resident batches, with the reference's class and method names
(madrl/models/model.py, maddpg.py, safemaddpg.py) so that ``PGTrainer(args, MADDPG, env, logger)``
and reference state_dicts keep working.

What is different from the reference, by design:
  * every method takes batches of any size (thousands of envs), never assumes batch 1;
  * a replay batch is already a tuple of device tensors (replay_buffer.DeviceReplayBuffer): there is no
    numpy -> tensor -> device ``unpack_data`` round trip per sub-update (model.py:308-323);
  * the centralised critic does not materialise its [B*n, n*(o+a)+n] input (maddpg.py:33-76); it forms
    fc1's output from the column blocks of fc1.weight — the observation block once per sample instead
    of n times — which is the same affine map up to fp32 summation order;
  * the rollout steps N environments per iteration without a host sync (``train_process`` on a
    VecFlexProvisionEnv) and the soft target update is one fused ``torch._foreach`` call.
The N=1 path through ``FlexibilityProvisionEnv`` reproduces the reference's cadence exactly.
"""
from __future__ import annotations

import os

import numpy as np
import torch as th
import torch.nn as nn

from .nets import (WGRAD_MIN_ROWS, AttentionCritic, attn_critic, CriticTail, critic_first_layer, critic_td_loss, critic_td_loss_supported, critic_policy_loss,
                   critic_policy_loss_supported, expand_agents, MLPAgent, MLPAgentGaussian, MLPCritic, mlp_burst_actor_args, mlp_burst_declines, mlp_test_actor_args, RNNAgent, RNNAgentGaussian, critic_policy_supported, critic_replayed_supported,
                   critic_tail_supported, fused_actor_forward, fused_actor_forward_unshared, actor_unshared_supported,
                   actor_mlp_declines, actor_mlp_train, fused_actor_forward_mlp, mlp_actor_allowed,
                   actor_mlp_unshared_declines, actor_mlp_unshared_train, fused_actor_forward_mlp_unshared,
                   gauss_head_unshared_declines, gauss_log_std_unshared,
                   actor_unshared_train, critic_unshared_supported, critic_unshared_train, fused_critic_forward_unshared,
                   critic_unshared_twin_supported, critic_unshared_twin_train, fused_critic_forward_unshared_twin,
                   tall_linear, td_loss, td_loss_supported, wide_batch_linear,
                   batchnorm_stats_supported, batchnorm_update_running_stats, sync_batchnorm, QMixer,
                   sqddpg_draw, sqddpg_fused_config, sqddpg_shapley_fused, sqddpg_shapley_unshared, sqddpg_unshared_config,
                   unshared_critics_switch, ppo_gae, ppo_policy_loss, ppo_value_loss,
                   coma_baseline, coma_baseline_torch, coma_fused_config, coma_policy_loss, coma_rows)
from .replay_buffer import Transition
from .util import _graph_audit, graph_capture, prep_obs, scale_action, select_action, translate_action, mean_all, note_fallback


class RolloutGraph:
    """One vector step of the rollout — policy forward, exploration noise, action scaling, the fused env kernel,
    the transition into the slab replay ring, statistics, hand-over of the hidden state — captured ONCE as a HIP graph
    and replayed per step.  Eagerly this is ~25 tiny kernels whose launch cost (0.36 ms) dwarfs the 14 us env kernel; as
    a graph it is one launch.  Everything the graph touches is a static tensor owned here, by the env or by the ring.

    The observation the policy reads IS the env's own output buffer (``env.obs``): the ring already holds it (the pack
    kernel of the step that produced it wrote it into the next slab), so nothing is handed over or copied twice."""

    def __init__(self, model, env, buf):
        self.model, self.env, self.buf = model, env, buf
        N, n, o, a, h = env.n_envs, model.n_, model.obs_dim, model.act_dim, model.hid_dim
        dev = model.device
        # Row mode (round 4): where the env's step kernel files observations itself (ring I/O below) the replay keeps every
        # feature ROW once and the policy kernels read the stacked observation in place from the env's own history —
        # nothing copies a [n, 6 H] window per step any more; elsewhere (general bodies) slabs hold stacked observations
        self.history = getattr(getattr(env, "vec", env), "history", None)
        self.rows_capable = bool(hasattr(env, "obs_source") and hasattr(env, "set_obs_ring") and env.obs.is_cuda
                                 and self.history and o == 6 * self.history)
        if not buf.slab_mode:
            if buf.store is not None:
                raise RuntimeError("replay buffer already holds field-by-field transitions; the graph rollout needs slab mode")
            buf.alloc_slabs(N, n, o, a, h)                    # (re-made in row mode by _configure_env where that applies)
        if (buf.n_envs, buf.n_agents, buf.obs_dim, buf.act_dim, buf.hid_dim) != (N, n, o, a, h):
            raise RuntimeError("replay buffer was allocated for another environment batch")
        self._obs = env.obs                         # [N, n, o]: written by the env kernel, read by the policy (tensor mode)
        self._hid = th.zeros(N, n, h, device=dev)
        self._info_sum = th.zeros(env.info.shape[1], dtype=th.float64, device=dev)
        self._rew_sum = th.zeros((), dtype=th.float64, device=dev)
        self._fail_sum = th.zeros((), dtype=th.float64, device=dev)
        self.std = float(model.args.fixed_policy_std)
        # gaussian_policy: the standard deviation is an output of the policy, per row — the kernels that carry ONE constant std
        # (the actor kernel's exploration epilogue and everything built on it: ring I/O, sink, burst) are not used; the
        # general bodies draw from the log-stds Model.policy returns and neither ``std`` nor ``summed_std`` is consulted.  (The one
        # exception is opt-in: ``gauss_burst`` below, the agent-summed burst with the log-std head in its policy phase.)
        self.gaussian = bool(model.args.gaussian_policy)
        self.graph = None
        self.bursts = {}                                       # k -> graph of k bodies (run())
        self._torch_noise = False
        self.rng_state = th.zeros(2, dtype=th.int64, device=dev)           # [seed, step] of the actor kernel's noise stream
        self.rng_state[0] = int(th.randint(0, 2 ** 62, (1,)).item())
        self.plain = type(model).get_actions is MADDPG.get_actions and bool(model.args.action_enforcebound)
        self.avail = th.ones(N, n, a, device=dev)             # every action is available (env:721-730)
        # MATD3 / IDDPG with the bound enforced: their agent-summed action selection (matd3.py:92-97, iddpg.py:66-71 over
        # util.py:57-64) and translate_action as ONE launch behind the fused policy — bit-identical to get_actions +
        # env_action (same draws from torch's generator, every fp32 rounding in the same place), ~40 launches fewer per step
        self.summed = (type(model).__name__ in ("MATD3", "IDDPG", "FACMADDPG", "SQDDPG", "IPPO", "MAPPO", "COMA")
                       and type(model).get_actions in (MATD3.get_actions, IDDPG.get_actions)
                       and bool(model.args.action_enforcebound) and bool(model.args.continuous) and a > 1
                       and env.obs.is_cuda and model.fused_inference and model.args.shared_params)
        if self.summed:
            if not self.gaussian:
                self.std_sum = model.summed_std(self.avail.device)
            self.act_pol_buf = th.zeros(N, n, a, device=dev)
            self.env_act_buf = th.zeros(N, n, a, device=dev)
        # plain MADDPG on the GPU: policy + exploration in one HIP launch, ring write + hand-over + statistics in another
        self.safe = type(model).__name__ == "SAFEMADDPG"       # + the safety projection between policy and env
        # (the actor kernel's exploration epilogue IS tanh(mean + std * noise), util.py:57-64: without action_enforcebound
        # the reference adds unbounded noise, util.py:66-74, and the general body below runs select_action itself)
        self._fast = (type(model).__name__ in ("MADDPG", "SAFEMADDPG") and model.fused_inference
                     and model.args.shared_params and env.obs.is_cuda and model.args.agent_type == "rnn" and h == 64
                     and o <= 144 and bool(model.args.action_enforcebound) and not self.gaussian)
        # ring write / hand-over / statistics in ONE launch of this project's kernel (fixed-order block sums): no ATen
        # reduction is ever captured into the rollout graph, whatever the algorithm
        self.packable = env.obs.is_cuda and h == 64 and o <= 144 and n <= 8 and a <= 8 and (n * o) % 4 == 0
        if self.safe:
            self.predictor = tuple(th.as_tensor(x, dtype=th.float64, device=dev).contiguous() for x in model.predictor)
        self.env_calls = None                                  # env.calls after this object's last step (continuity check)
        # The env's step kernel advances the slab the step fills (cursor[1]) itself (one lane): no launch of its own.
        self.cursor_stepped = 1 if (hasattr(env, "set_step_counter") and env.obs.is_cuda) else 0
        # Ring I/O (the fused path): the env kernel writes its observation straight into the slab after the cursor, the
        # actor kernel reads observation and hidden state from the slab at the cursor — the observation is written once,
        # where the replay keeps it, and never copied.
        self.ring_io = bool(self._fast and self.cursor_stepped and self.rows_capable)
        # Sink (ring I/O + an env that files transitions): the env step kernel also writes the small record, the masked
        # hidden state and the per-environment statistics — a vector step is TWO launches, policy and environment, and no
        # bookkeeping kernel.  Cursor cells then follow the two-kernel protocol of include/flexenv.h: cursor[0] is read by
        # the policy and written by the env step (slab to read next), cursor[1] is read by the env step and written by the
        # policy (slab it just read).
        # ... within the sink's own limits (flexenv_set_replay_sink: action row <= 32 floats, recurrent row <= 384 floats —
        # seven agents x 64 units is 448 — and the two-environments-per-wavefront instantiation, i.e. <= 32 PQ buses);
        # outside them the pack kernel files the transition (three launches per step)
        n_bus = getattr(getattr(env, "vec", env), "n_bus", None)       # (a wrapped env without it: not eligible — pack path)
        two_per_wave = n_bus is not None and n_bus - 1 <= 32
        self.sink = bool(self.ring_io and hasattr(env, "set_replay_sink") and n * a <= 32 and n * h <= 384 and two_per_wave)
        # MATD3 / IDDPG with the one-launch action selection (`summed`): the same ring I/O and sink — policy kernel (slab at the
        # cursor -> means, new hidden state), agent_sum_explore_kernel (-> the action the replay keeps, the env's action), env
        # step (files the transition): three launches, no pack kernel, the observation written once (round 3)
        summed_sink_shape = bool(self.summed and self.cursor_stepped and self.rows_capable
                                 and hasattr(env, "set_replay_sink") and n * a <= 32 and n * h <= 384
                                 and two_per_wave and h == 64 and o <= 144
                                 and os.environ.get("FLEX_SUMMED_SINK", "1") != "0")
        self.summed_sink = bool(summed_sink_shape and not self.gaussian)
        # gaussian_policy with a shared RNNAgentGaussian (include/flexenv.h: flexenv_rollout_burst_summed_gauss): the summed
        # burst below with the log-std head evaluated in the policy phase and per-sample log-stds in the selection — the env
        # configured as for `summed_sink`, every vector step (a single one too) through the one launch.  Off unless
        # FLEX_GAUSS_BURST=1: the general body stays what a Gaussian RolloutGraph runs by default.
        self.gauss_burst = bool(summed_sink_shape and self.gaussian and isinstance(model.policy_dicts[0], RNNAgentGaussian)
                                and n <= 5 and o % 4 == 0 and a == 4
                                and hasattr(getattr(env, "vec", env), "rollout_burst_summed_gauss")
                                and os.environ.get("FLEX_SUMMED_BURST", "1") != "0"
                                and os.environ.get("FLEX_GAUSS_BURST", "0") == "1")
        # agent_type mlp with a shared MLPAgent (include/flexenv.h: flexenv_rollout_burst_summed_mlp): the same two launches with
        # the MLP's second layer where the GRU cell stands — one form only, as `gauss_burst`: every vector step, a single one
        # too, through the one launch, the env configured as for `summed_sink`.  On by default for the fixed std (without it
        # body() hands the MLP agent to the RNN's kernel, which declines, and the trainer falls back to the eager loop:
        # FLEX_MLP_BURST=0 keeps exactly that); an MLPAgentGaussian needs FLEX_GAUSS_BURST=1 as well, as the RNN's Gaussian
        # burst does.  The launch belongs to the burst family of csrc/flexenv.hip and is captured like its siblings — the
        # capture rule of csrc/actor_mlp.hip (nets.mlp_actor_allowed) concerns that file's entry points, which this body never
        # calls.
        agent0 = model.policy_dicts[0]
        self.mlp_burst = bool(summed_sink_shape
                              and ((type(agent0) is MLPAgent and not self.gaussian)
                                   or (type(agent0) is MLPAgentGaussian and self.gaussian
                                       and os.environ.get("FLEX_GAUSS_BURST", "0") == "1"))
                              and model.args.hid_size == 64 and model.args.hid_activation == "relu"
                              and n <= 5 and o % 4 == 0 and a == 4
                              and hasattr(getattr(env, "vec", env), "rollout_burst_summed_mlp")
                              and os.environ.get("FLEX_SUMMED_BURST", "1") != "0"
                              and os.environ.get("FLEX_MLP_BURST", "1") != "0")
        if self.mlp_burst:
            self.summed_sink = False                  # (the three-launch form is the RNN agent's: there is no second form here)
        # agent_type mlp under MADDPG / SAFEMADDPG (include/flexenv.h: flexenv_rollout_burst_mlp): the plain burst below — in-kernel
        # noise stream, exploration epilogue, SAFEMADDPG's projection as a phase of the launch — with the MLP's policy tiles.  One
        # form only, as `mlp_burst`: every vector step, a single one too, through the one launch; the env configured as for `sink`
        # with the noise stream's aux_counter, the replay in row mode.  `fast` stays off (it is the RNN agent's two-launch body),
        # and without this flag (FLEX_MLP_BURST=0) the general body at the bottom of body() runs Model.policy as before.
        own_get_actions = SAFEMADDPG.get_actions if self.safe else MADDPG.get_actions
        # SAFEMADDPG.intended_actions inside the burst launches (include/flexenv.h: flexenv_rollout_burst_routed) is opt-in:
        # FLEX_INTENDED_LAUNCH=1, read here.  With it both burst forms below admit that routing and body() hands the launch
        # the routing in force at each call (the buffers are the same for both); without it they exclude it as before.
        self.intended_launch = bool(self.safe and os.environ.get("FLEX_INTENDED_LAUNCH", "0") == "1")
        self.mlp_plain_burst = bool(type(model).__name__ in ("MADDPG", "SAFEMADDPG")
                                    and type(model).get_actions is own_get_actions
                                    and bool(model.args.action_enforcebound) and not self.gaussian
                                    and model.fused_inference and model.args.shared_params and env.obs.is_cuda
                                    and type(agent0) is MLPAgent
                                    and model.args.hid_size == 64 and model.args.hid_activation == "relu" and h == 64
                                    and n <= 5 and o % 4 == 0 and o <= 144 and (not self.safe or a == 4)
                                    and n * a <= 32 and n * h <= 384 and two_per_wave
                                    and self.rows_capable and self.cursor_stepped and hasattr(env, "set_replay_sink")
                                    and hasattr(getattr(env, "vec", env), "rollout_burst_mlp")
                                    and not (self.safe and model.intended_actions and not self.intended_launch)
                                    and os.environ.get("FLEX_ROLLOUT_BURST", "1") != "0"
                                    and os.environ.get("FLEX_MLP_BURST", "1") != "0")
        if self.mlp_plain_burst:
            self.means_buf = th.zeros(N * n, a, device=dev)
            self.burst_env_act = th.zeros(N * n, a, device=dev)
            if self.safe:
                self.burst_adjusted = th.zeros(N, 4 * n, dtype=th.float64, device=dev)
                self.burst_safe_env_act = th.zeros(N, 4 * n, device=dev)
        if self.sink or self.summed_sink or self.gauss_burst or self.mlp_burst or self.mlp_plain_burst:
            self.act_buf = th.zeros(N * n, a, device=dev)
            self.hid_buf = th.zeros(N * n, h, device=dev)
            self.acc = th.zeros(N, 10, dtype=th.float64, device=dev)
        # Burst launch (round 3): with the sink, plain MADDPG (nothing between policy and environment) and at most five
        # agents — a block's sixteen environments are then at most five 16-row policy tiles, what one CU's LDS-resident
        # weights serve — run(m) is ONE persistent launch per m steps (include/flexenv.h: flexenv_rollout_burst).
        # SAFEMADDPG: the safety projection is a phase of the same launch (each wavefront projects its own two environments)
        self.burst_launch = bool(self.sink and n <= 5 and o % 4 == 0 and hasattr(getattr(env, "vec", env), "rollout_burst")
                                 and (not self.safe or a == 4) and os.environ.get("FLEX_ROLLOUT_BURST", "1") != "0")
        if self.burst_launch:
            self.means_buf = th.zeros(N * n, a, device=dev)
            self.burst_env_act = th.zeros(N * n, a, device=dev)
            if self.safe:
                self.burst_adjusted = th.zeros(N, 4 * n, dtype=th.float64, device=dev)
                self.burst_safe_env_act = th.zeros(N, 4 * n, device=dev)
        # The same launch for the agent-summed algorithms (include/flexenv.h: flexenv_rollout_burst_summed): the policy hands
        # on its means, each wavefront sums those of its own two environments and selects the one action (the arithmetic of
        # flexnet_agent_sum_explore) in front of its step.  The draws stay in torch's generator: one [k, N, 1, a] call per
        # burst of k steps.  FLEX_SUMMED_BURST=0: three launches per step, graphs of 16 / 8 / 4 / 2 bodies.
        self.summed_burst = bool(self.summed_sink and n <= 5 and o % 4 == 0 and a == 4
                                 and hasattr(getattr(env, "vec", env), "rollout_burst_summed")
                                 and os.environ.get("FLEX_SUMMED_BURST", "1") != "0")
        if self.summed_burst or self.gauss_burst or self.mlp_burst:
            self.means_buf = th.zeros(N * n, a, device=dev)
        if self.gauss_burst or (self.mlp_burst and self.gaussian):
            self.log_stds_buf = th.zeros(N * n, a, device=dev)
        self._configure_env()

    def _configure_env(self):
        """Point the env's device-side hooks at this object's ring for the mode in force (fast / general body, in-kernel
        or torch noise): called at construction and whenever a test flips ``fast`` or ``torch_noise``."""
        env, buf = self.env, self.buf
        if not self.cursor_stepped:
            return
        N, n, o = env.n_envs, self.model.n_, self.model.obs_dim
        # the replay's layout follows the mode: feature rows where the env files observations itself, stacked slabs otherwise
        if bool(self.ring_active) != bool(buf.row_mode):
            if buf.k != 0 or buf.length != 0:
                raise RuntimeError("the rollout body changed between ring I/O and tensor hand-over with transitions in the replay")
            buf.alloc_slabs(N, n, o, self.model.act_dim, self.model.hid_dim, history=self.history if self.ring_active else None)
        if self.ring_active:
            self.obs_src = env.obs_source()                 # the policy kernels read the stacked observation in place
        row_stride = N * n * buf.ROW_W
        if self.sink_active:
            env.set_step_counter(None)                      # the env step sets cursor[0] itself in this mode
            env.set_obs_ring(buf.cursor[1:], row_stride, buf.slabs)
            env.set_replay_sink(self.act_buf, self.hid_buf, buf.small_ring, buf.hid_ring, self.acc, cursor_out=buf.cursor[0:1],
                                aux_counter=None if (self._torch_noise or self.summed_sink or self.gauss_burst or self.mlp_burst)
                                else self.rng_state[1:2])         # (mlp_plain_burst: always the noise stream's counter)
        else:
            env.set_step_counter(buf.cursor[1:], buf.slabs)
            if self.ring_active:
                env.set_obs_ring(buf.cursor, row_stride, buf.slabs)
            if hasattr(env, "set_replay_sink"):
                env.set_replay_sink(None, None, None, None, None)

    @property
    def fast(self):
        return self._fast

    @fast.setter
    def fast(self, value):
        if self.mlp_plain_burst and value:
            raise RuntimeError("fast is the RNN agent's two-launch body: the MLP agent's rollout has the burst launch only")
        self._fast = bool(value)
        self._configure_env()

    @property
    def torch_noise(self):
        return self._torch_noise

    @torch_noise.setter
    def torch_noise(self, value):
        if self.mlp_plain_burst and value:
            raise RuntimeError("torch_noise: the MLP agent's burst draws in the kernel and has no second form")
        self._torch_noise = bool(value)
        self._configure_env()

    @property
    def sink_active(self):
        return (self.sink and self.fast) or self.summed_sink or self.gauss_burst or self.mlp_burst or self.mlp_plain_burst

    @property
    def fused_burst(self):
        if self.summed_burst or self.gauss_burst or self.mlp_burst:       # (their draws are torch's own: torch_noise gates the plain form only)
            return True
        if self.mlp_plain_burst:                                          # (one form only; its setters refuse torch_noise and fast)
            return True
        return (self.burst_launch and self.sink_active and not self._torch_noise
                # (that routing transposes in torch, unless FLEX_INTENDED_LAUNCH=1 put it into the launch)
                and not (self.safe and self.model.intended_actions and not self.intended_launch))

    @property
    def _burst_form(self):
        """What run() keys its burst graphs by, next to their length: ``fused_burst``, or — truthy as well — the name of the
        routed launch's intended form, so that a graph recorded under one routing is never replayed under the other."""
        fused = self.fused_burst
        return "intended" if fused and self.intended_launch and self.model.intended_actions else fused

    # episode statistics: block sums of the pack kernel, or (sink) the env step's per-environment running sums, added up
    # when asked for (outside any graph)
    @property
    def info_sum(self):
        return self.acc[:, :self._info_sum.numel()].sum(0) if self.sink_active else self._info_sum

    @property
    def rew_sum(self):
        return self.acc[:, 7].sum() if self.sink_active else self._rew_sum

    @property
    def fail_sum(self):
        return self.acc[:, 8].sum() if self.sink_active else self._fail_sum

    @property
    def ring_active(self):
        # (tests switch `fast` off to run the general body on the same object)
        return (self.ring_io and self.fast) or self.summed_sink or self.gauss_burst or self.mlp_burst or self.mlp_plain_burst

    @property
    def obs(self):
        """The observation the next policy evaluation reads: [N, n, o]."""
        if self.ring_active:                                # (a materialised copy: the policy kernels read the env's history)
            return self.env.obs_view().view(self.env.n_envs, self.model.n_, self.model.obs_dim)
        return self._obs

    @property
    def hid(self):
        """The hidden state the next policy evaluation starts from: [N, n, h]."""
        if self.ring_active:
            return self.buf.hid_ring[self.buf.k % self.buf.slabs].view(self.env.n_envs, self.model.n_, self.model.hid_dim)
        return self._hid

    def _pack(self, action, hid):
        """model.py:230-262 for every environment in one launch (include/flexnet.h: flexnet_rollout_pack)."""
        from . import _lib
        m, env, buf = self.model, self.env, self.buf
        a = _lib.FlexRolloutPackArgs()
        a.n_envs, a.n_agents, a.obs_dim, a.act_dim = env.n_envs, m.n_, m.obs_dim, m.act_dim
        a.slabs, a.small_w, a.info_w, a.cursor_stepped = buf.slabs, buf.small_w, env.info.shape[1], self.cursor_stepped
        for name, t in (("action", action), ("reward", env.reward), ("obs_next", None if self.ring_active else env.obs),
                        ("done", env.done), ("hid_new", hid), ("info", env.info), ("failed", env.failed),
                        ("obs_ring", buf.row_ring if buf.row_mode else buf.obs_ring), ("hid_ring", buf.hid_ring),
                        ("small_ring", buf.small_ring),
                        ("hid_state", None if self.ring_active else self._hid), ("cursor", buf.cursor),
                        ("info_sum", self._info_sum), ("rew_sum", self._rew_sum), ("fail_sum", self._fail_sum)):
            if t is not None:
                assert t.is_contiguous()
                setattr(a, name, t.data_ptr())
        if not self.torch_noise:
            a.rng_state = self.rng_state.data_ptr()       # next step of the actor kernel's noise stream
        _lib.launch("flexnet_rollout_pack", a)

    def last_transition(self):
        """Views of the transition the last step wrote (tests, debugging): the slab before the cursor."""
        buf = self.buf
        N = self.env.n_envs
        return buf.slab_window((buf.k - 1) * N, N)

    def body(self, burst=0):
        """One vector step (``burst`` = 0), or ``burst`` of them in the fused launch (``fused_burst`` configurations only)."""
        m, env = self.model, self.env
        N = env.n_envs
        if burst and not self.fused_burst:
            raise RuntimeError("rollout burst launch outside its configuration")
        if self.fast:
            with th.no_grad():
                # exploration noise: drawn by the actor kernel from its own Philox stream (seeded from torch's generator
                # when this object was built; the pack kernel advances the step counter), or — torch_noise, used by the
                # tests that compare with the PyTorch glue draw for draw — by torch.randn.  Inside a HIP graph torch.randn
                # costs a launch plus two seed/offset fill kernels per replay.
                buf = self.buf
                noise = th.randn(N, m.n_, m.act_dim, device=env.obs.device) if self.torch_noise else None
                # ring I/O: the hidden state from the slab at the cursor, the stacked observation IN PLACE from the env's history
                ring = dict(ring_cursor=buf.cursor, obs_slab_stride=0, hid_slab_stride=buf.hid_ring.stride(0),
                            obs_source=self.obs_src) if self.ring_active else {}
                obs_in = self._obs                           # (ring I/O: only its shape is used)
                hid_in = buf.hid_ring[0].view(N, m.n_, m.hid_dim) if self.ring_active else self._hid
                if self.sink_active:           # static outputs the env step reads back (registered with its replay sink)
                    ring.update(cursor_out=buf.cursor[1:], out=dict(hidden_out=self.hid_buf, action=self.act_buf))
                if burst:
                    # policy and environment for `burst` steps in one persistent launch (include/flexenv.h:
                    # flexenv_rollout_burst): the policy call's arguments, handed to the env's launch instead of its own
                    ring["out"].update(means=self.means_buf, env_action=self.burst_env_act)
                    vec = env.vec if hasattr(env, "vec") else env
                    safety = None
                    if self.safe:          # safemaddpg.py:90-111 inside the launch: what the three-launch body below calls
                        s_p, s_q, beta = self.predictor
                        safety = dict(s_p=s_p, s_q=s_q, beta=beta, v_min=m.V_min, v_max=m.V_max, adjusted=self.burst_adjusted,
                                      env_action=self.burst_safe_env_act, act_low=m.args.action_low, act_high=m.args.action_high)
                        if self.intended_launch:       # (flexenv_rollout_burst_routed: the routing in force at this call)
                            safety["routing"] = int(bool(m.intended_actions))
                    ring.update(ring_slabs=buf.slabs,
                                launch=lambda args: vec.rollout_burst(args, burst, buf.row_ring, safety=safety))
                out = fused_actor_forward(m.policy_dicts[0], obs_in, hid_in, m.n_, m.args.agent_id, noise=noise,
                                          std=self.std, low=m.args.action_low, high=m.args.action_high,
                                          rng_state=None if self.torch_noise else self.rng_state, **ring)
                if out is None:
                    raise RuntimeError("the fused actor kernel declined a configuration RolloutGraph.fast admitted")
                if burst:
                    return
                _, hid, action, env_action = out
                if self.safe:
                    # safemaddpg.py:90-111: the proposed action goes through the safety layer (HIP closed form,
                    # flexenv_safety_project); the replay keeps the policy's own action (model.py:232)
                    vec = env.vec if hasattr(env, "vec") else env
                    # ... and the env's action (translate_action of the adjusted vector) comes out of the same launch
                    if m.intended_actions:        # (not the reference's routing: SAFEMADDPG.intended_actions)
                        adj, _ = vec.safety_project(action.view(N, m.n_, m.act_dim), *self.predictor, m.V_min, m.V_max,
                                                    want_hit=False)
                        env_action = m.env_action(adj)
                    else:
                        _, _, env_action = vec.safety_project(action.view(N, m.n_, m.act_dim), *self.predictor, m.V_min, m.V_max,
                                                              env_action_range=(m.args.action_low, m.args.action_high),
                                                              want_hit=False)
                env.step(env_action.view(N, m.n_, m.act_dim), fuse_obs=True, auto_reset=True,
                         obs_ring=buf.row_ring if self.ring_active else None, replay_sink=self.sink_active)
                if not self.sink_active:
                    self._pack(action, hid)
                return
        if self.mlp_plain_burst:
            if self.safe and m.intended_actions and not self.intended_launch:
                raise RuntimeError("SAFEMADDPG.intended_actions was switched on after construction: that routing is not in "
                                   "the MLP agent's burst launch, which has no second form")
            # the MLP policy with its exploration epilogue (noise drawn in the kernel: torch's generator is not touched), the
            # safety projection (SAFEMADDPG) and the environment for `burst` steps — or ONE step: the same launch, there is no
            # second form — in one persistent launch (include/flexenv.h: flexenv_rollout_burst_mlp).  Model.policy is not called.
            buf, k = self.buf, burst or 1
            vec = env.vec if hasattr(env, "vec") else env
            args, mlp = mlp_burst_actor_args(m.policy_dicts[0], N, m.n_, m.obs_dim, m.args.agent_id, ring_cursor=buf.cursor,
                                             cursor_out=buf.cursor[1:], obs_source=self.obs_src, ring_slabs=buf.slabs,
                                             hidden_out=self.hid_buf, means=self.means_buf, rng_state=self.rng_state,
                                             std=self.std, action_low=m.args.action_low, action_high=m.args.action_high)
            # (what the epilogue writes: the action the sink files, the action the step — or the projection — reads)
            args.action, args.env_action = self.act_buf.data_ptr(), self.burst_env_act.data_ptr()
            safety = None
            if self.safe:                  # safemaddpg.py:90-111 inside the launch, as in the RNN agent's burst
                s_p, s_q, beta = self.predictor
                safety = dict(s_p=s_p, s_q=s_q, beta=beta, v_min=m.V_min, v_max=m.V_max, adjusted=self.burst_adjusted,
                              env_action=self.burst_safe_env_act, act_low=m.args.action_low, act_high=m.args.action_high)
                if self.intended_launch:       # (flexenv_rollout_burst_routed: the routing in force at this call)
                    safety["routing"] = int(bool(m.intended_actions))
            vec.rollout_burst_mlp(args, mlp, k, buf.row_ring, safety=safety)
            return
        if self.gauss_burst:
            with th.no_grad():
                # policy with both heads, per-sample selection and environment for `burst` steps — or ONE step: the same launch,
                # there is no second form — in one persistent launch (include/flexenv.h: flexenv_rollout_burst_summed_gauss);
                # the draws of all its steps from ONE call of the function _summed_exploration_rows draws a step's from
                import torch.distributions.normal as tdn      # (looked up at call time, as summed_exploration does)
                buf, k = self.buf, burst or 1
                agent = m.policy_dicts[0]
                eps = tdn._standard_normal((k, N, 1, m.act_dim), th.float32, self.act_buf.device)
                vec = env.vec if hasattr(env, "vec") else env

                def launch(args):
                    # (what the selection phase writes: the action the sink files, the action the step reads)
                    args.action, args.env_action = self.act_buf.data_ptr(), self.env_act_buf.data_ptr()
                    vec.rollout_burst_summed_gauss(args, k, buf.row_ring, eps, agent.log_std.weight, agent.log_std.bias,
                                                   self.log_stds_buf, agent.args.LOG_STD_MIN, agent.args.LOG_STD_MAX,
                                                   m.args.action_low, m.args.action_high)

                out = fused_actor_forward(agent, self._obs, buf.hid_ring[0].view(N, m.n_, m.hid_dim), m.n_, m.args.agent_id,
                                          ring_cursor=buf.cursor, obs_slab_stride=0, obs_source=self.obs_src,
                                          hid_slab_stride=buf.hid_ring.stride(0), cursor_out=buf.cursor[1:],
                                          out=dict(hidden_out=self.hid_buf, means=self.means_buf), ring_slabs=buf.slabs,
                                          launch=launch)
                if out is None:
                    raise RuntimeError("the fused actor kernel declined a configuration RolloutGraph.gauss_burst admitted")
            return
        if self.mlp_burst:
            with th.no_grad():
                # the MLP policy, selection and environment for `burst` steps — or ONE step: the same launch, there is no second
                # form — in one persistent launch (include/flexenv.h: flexenv_rollout_burst_summed_mlp); the draws of all its
                # steps from ONE call of the function summed_exploration draws a step's from.  Model.policy is not called.
                import torch.distributions.normal as tdn      # (looked up at call time, as summed_exploration does)
                buf, k = self.buf, burst or 1
                agent = m.policy_dicts[0]
                eps = tdn._standard_normal((k, N, 1, m.act_dim), th.float32, self.act_buf.device)
                vec = env.vec if hasattr(env, "vec") else env
                args, mlp = mlp_burst_actor_args(agent, N, m.n_, m.obs_dim, m.args.agent_id, ring_cursor=buf.cursor,
                                                 cursor_out=buf.cursor[1:], obs_source=self.obs_src, ring_slabs=buf.slabs,
                                                 hidden_out=self.hid_buf, means=self.means_buf)
                # (what the selection phase writes: the action the sink files, the action the step reads)
                args.action, args.env_action = self.act_buf.data_ptr(), self.env_act_buf.data_ptr()
                if self.gaussian:
                    vec.rollout_burst_summed_mlp(args, mlp, k, buf.row_ring, eps, m.args.action_low, m.args.action_high,
                                                 log_std_w=agent.log_std.weight, log_std_b=agent.log_std.bias,
                                                 log_stds=self.log_stds_buf, log_std_min=agent.args.LOG_STD_MIN,
                                                 log_std_max=agent.args.LOG_STD_MAX)
                else:
                    vec.rollout_burst_summed_mlp(args, mlp, k, buf.row_ring, eps, m.args.action_low, m.args.action_high,
                                                 std=m.summed_std(eps.device))
            return
        if self.summed and self.summed_sink:
            with th.no_grad():
                buf = self.buf
                outs, hook = dict(hidden_out=self.hid_buf), {}
                if burst:
                    # policy, action selection and environment for `burst` steps in one persistent launch (include/flexenv.h:
                    # flexenv_rollout_burst_summed): the policy call's arguments, handed to the env's launch instead of its
                    # own, and the draws of all its steps from ONE call of the function summed_exploration draws a step's from
                    import torch.distributions.normal as tdn      # (looked up at call time, as summed_exploration does)
                    eps = tdn._standard_normal((burst, N, 1, m.act_dim), th.float32, self.act_buf.device)
                    vec = env.vec if hasattr(env, "vec") else env
                    outs.update(means=self.means_buf)

                    def launch(args):
                        # (what the selection phase writes: the action the sink files, the action the step reads)
                        args.action, args.env_action = self.act_buf.data_ptr(), self.env_act_buf.data_ptr()
                        vec.rollout_burst_summed(args, burst, buf.row_ring, eps, m.summed_std(eps.device), m.args.action_low,
                                                 m.args.action_high)

                    hook = dict(ring_slabs=buf.slabs, launch=launch)
                out = fused_actor_forward(m.policy_dicts[0], self._obs,
                                          buf.hid_ring[0].view(N, m.n_, m.hid_dim), m.n_, m.args.agent_id,
                                          ring_cursor=buf.cursor, obs_slab_stride=0, obs_source=self.obs_src,
                                          hid_slab_stride=buf.hid_ring.stride(0), cursor_out=buf.cursor[1:],
                                          out=outs, **hook)
                if out is None:
                    raise RuntimeError("the fused actor kernel declined a configuration RolloutGraph.summed_sink admitted")
                if burst:
                    return
                summed_exploration(m, out[0].view(N, m.n_, m.act_dim), env_action=self.env_act_buf,
                                   action_out=self.act_buf.view(N, m.n_, m.act_dim))
                env.step(self.env_act_buf, fuse_obs=True, auto_reset=True, obs_ring=buf.row_ring, replay_sink=True)
            return
        if self.summed:
            with th.no_grad():
                means, log_stds, hid = m.policy(self.obs, last_hid=self.hid)
                summed_exploration(m, means.to(th.float32), env_action=self.env_act_buf, action_out=self.act_pol_buf,
                                   log_stds=log_stds if self.gaussian else None)
                env.step(self.env_act_buf, fuse_obs=True, auto_reset=True)
                self._pack(self.act_pol_buf, hid.reshape(N, m.n_, -1).to(th.float32).contiguous())
            return
        with th.no_grad():
            if self.plain and self.gaussian:
                means, log_stds, hid = m.policy(self.obs, last_hid=self.hid)
                action = action_pol = th.tanh(means + log_stds.exp() * th.randn_like(means))    # util.py:57-64, per-row std
            elif self.plain:
                means, _, hid = m.policy(self.obs, last_hid=self.hid)
                action = action_pol = th.tanh(means + self.std * th.randn_like(means))          # util.py:57-64
            else:
                # MATD3 / IDDPG (agent-summed action selection, matd3.py:88-111, iddpg.py:66-71): their own get_actions,
                # exactly as the eager loop calls it; the replay keeps the restore-masked action (model.py:232)
                action, action_pol, _, _, hid = m.get_actions(self.obs, status="train", exploration=True,
                                                              actions_avail=self.avail, target=False, last_hid=self.hid)
                action_pol = action_pol.expand(N, m.n_, m.act_dim)
            env.step(m.env_action(action), fuse_obs=True, auto_reset=True)
            self._pack(action_pol.to(th.float32).contiguous(), hid.reshape(N, m.n_, -1).to(th.float32).contiguous())

    def step(self):
        """One vector step: a graph replay (or the eager body before capture) plus the host mirror of the ring cursor.
        Returns the physical slab the step completed."""
        if self.graph is not None:
            self.graph.replay()
        else:
            self.body()
        return self.buf.stepped()

    BURSTS = (16, 8, 4, 2)
    BURST_MAX = 96                                       # fused burst launch: steps per launch (an episode of the env)

    def run(self, m):
        """``m`` consecutive vector steps with nothing for the host to do in between: graphs of 16 / 8 / 4 / 2 bodies
        (captured on first use, sharing the one-step graph's memory pool) and single steps for the rest.  Every body
        finds its slabs through the device-side cursors, so k bodies in one graph are k replays of the one-step graph
        minus k - 1 graph launches (~8 us of idle GPU each at 4096 envs).  Returns the slabs completed, in order."""
        done = []
        for k in (self.burst_chunks(m) if self.graph is not None else [1] * m):
            if k == 1:
                done.append(self.step())
                continue
            g = self.bursts.get((k, self._burst_form))      # (keyed by the body's form too: a flag flipped after capture()
            if g is None:                                    #  must not replay a graph recorded for the other body)
                g = self._capture_burst(k)
            g.replay()
            done.extend(self.buf.stepped() for _ in range(k))
        return done

    def burst_chunks(self, m):
        """The graph sizes run(m) replays, in order (1 = the one-step graph)."""
        out = []
        while m > 0:
            if self.fused_burst:
                k = max(1, min(m, self.BURST_MAX, self.buf.slabs - 1))     # (a burst stays below the ring's size)
            else:
                k = next((b for b in self.BURSTS if b <= m), 1)
            out.append(k)
            m -= k
        return out

    def _capture_burst(self, k, collect=True):
        """A graph of ``k`` bodies, sharing the one-step graph's memory pool.  Recording launches nothing: the environment,
        the ring and the cursors are untouched (the bodies were warmed up when the one-step graph was captured); only the
        env's host-side call counter would move."""
        calls = getattr(self.env, "calls", None)
        g = th.cuda.CUDAGraph()
        with graph_capture(g, collect=collect, pool=self.graph.pool()):
            if self.fused_burst:
                self.body(burst=k)
            else:
                for _ in range(k):
                    self.body()
        if calls is not None:
            self.env.calls = calls
        self.bursts[(k, self._burst_form)] = g
        return g

    def capture(self, lengths=None):
        """Warm-up + capture.  The warm-up steps are real steps of the environment; the ring cursor and the statistics
        they moved are put back afterwards (the slabs they wrote are overwritten by the steps that follow).
        ``lengths``: the run lengths the caller will ask run() for (the training loop knows its schedule: the distances
        between update events and episode ends) — with the one-launch burst every length is a graph of its own, and they are
        all recorded NOW rather than inside somebody's timed region; other lengths are recorded at first use."""
        import os
        if not self.packable:
            raise RuntimeError("observation / hidden sizes outside flexnet_rollout_pack: the statistics would go through "
                               "ATen reductions, which must not be captured into a HIP graph (DESIGN.md §6)")
        cursor0 = self.buf.cursor.clone()
        if os.environ.get("FLEX_GRAPH_AUDIT") == "1":
            from .util import audit_graph_body
            self.audit = audit_graph_body(self.body)
        side = th.cuda.Stream()
        side.wait_stream(th.cuda.current_stream())
        # The warm-up runs the body the capture will run: paths that stand aside for a capture (nets.mlp_actor_allowed) stand
        # aside here too.  Otherwise the module loop they fall back to would run for the first time INSIDE the capture, and a
        # library GEMM's first call of a process sets its handle and workspace up with calls a capturing stream forbids.
        with th.cuda.stream(side), _graph_audit():
            for _ in range(3):
                self.body()                      # warm-up on a side stream, as graph capture requires
        th.cuda.current_stream().wait_stream(side)
        g = th.cuda.CUDAGraph()
        with graph_capture(g):
            self.body()
        self.graph = g
        self.bursts = {}
        # every burst size NOW, not at first use: a first use falls into somebody's timed region (a 16-body capture is
        # milliseconds of host work — BENCH_r02's SAFEMADDPG leg, timed from the second episode on, carried the 8 / 4 / 2
        # captures and read 0.366 ms per vector step on the driver's box against 0.25-0.32 on others)
        if self.fused_burst:
            sizes = sorted({k for m in (lengths or ()) for k in self.burst_chunks(int(m)) if k > 1})
        else:
            sizes = list(self.BURSTS)
        import gc
        gc.collect()
        for k in sizes:
            self._capture_burst(k, collect=False)
        self.buf.cursor.copy_(cursor0)

    def release(self):
        """Undo what construction set up on the env and the replay buffer (capture failed: the eager rollout takes over and
        writes the buffer field by field, so the env's device-side hooks must not point at a ring any more)."""
        env = self.env
        if self.cursor_stepped:
            env.set_step_counter(None)
            if hasattr(env, "set_obs_ring"):
                env.set_obs_ring(None, 0, 0)
            if hasattr(env, "set_replay_sink"):
                env.set_replay_sink(None, None, None, None, None)
        self.graph, self.bursts = None, {}
        self.buf.release_slabs()

    def start_episode(self, first_obs=None):
        """``first_obs`` given: a hard reset happened (env.reset()); the stream restarts in the ring and the hidden state
        is zero.  None: the environments continue where the last step left them (those that terminated restarted
        inside that launch, their hidden state was zeroed by the pack kernel)."""
        if first_obs is not None:
            if not self.ring_active and first_obs.data_ptr() != self._obs.data_ptr():
                self._obs.copy_(first_obs)
            self._hid.zero_()
            self.buf.begin_stream(first_obs)
        self._info_sum.zero_(); self._rew_sum.zero_(); self._fail_sum.zero_()
        if self.sink or self.summed_sink or self.gauss_burst or self.mlp_burst or self.mlp_plain_burst:
            self.acc.zero_()


class _GraphSafe:
    """``graph_safe_updates`` of an algorithm whose sub-updates may be captured into a HIP graph: the declared value on the class;
    on a model, False under ``shared_params: False`` — the per-agent critics' gradient path holds ATen bias and LayerNorm
    reductions (util.GRAPH_DENYLIST), so those sub-updates run eagerly."""

    def __init__(self, value):
        self.value = bool(value)

    def __get__(self, obj, owner=None):
        return self.value if obj is None else bool(self.value and obj.args.shared_params)


def episode_stats(sums, length):
    """The reference's ``mean_test_*`` keys from per-episode sums, as model.py:285-306 forms them: every figure summed over an
    episode's steps, divided by THAT episode's length ``t + 1``, then averaged over the episodes (accumulated in episode order,
    as the reference's loop does).  ``sums`` [N, 10]: info[0..6] (``_lib.INFO_KEYS``), reward, steps with voltage_penalty > 0,
    solver_failed; ``length`` [N].  ``mean_test_reward`` is the reference's: its running sum takes info["reward"] AND the
    step's reward (model.py:286-290: the info key collides with the reward's own), so it is their sum — ``evaluate_on``
    reports the step reward alone.  Besides the reference's keys: ``mean_test_violation_rate`` (share of an episode's steps with
    any bus voltage outside its band) and ``mean_test_solver_failed``."""
    from ._lib import INFO_KEYS
    sums = np.asarray(sums, dtype=np.float64).reshape(-1, 10)
    length = np.asarray(length).reshape(-1)
    if sums.shape[0] != length.shape[0] or sums.shape[0] < 1 or (length < 1).any():
        raise ValueError("episode_stats: sums [N, 10] and length [N] >= 1 of the same N >= 1 episodes")
    per = sums / length.astype(np.float64)[:, None]                  # model.py:297-298
    per[:, 7] = (sums[:, 0] + sums[:, 7]) / length                   # model.py:286-290
    mean = np.cumsum(per, axis=0)[-1] / float(sums.shape[0])         # model.py:299-305, in episode order
    stat = {"mean_test_" + k: float(mean[i]) for i, k in enumerate(INFO_KEYS) if k != "reward"}
    stat["mean_test_reward"] = float(mean[7])
    stat["mean_test_violation_rate"] = float(mean[8])
    stat["mean_test_solver_failed"] = float(mean[9])
    return stat


def one_launch_declines(model):
    """None where ``Model.test_episodes`` may take the single launch (flexenv_test_episodes for a shared RNN actor,
    flexenv_test_episodes_mlp for a shared MLP one), else the reason — decided from the model's class and arguments, whatever
    the device, and from two switches of the process environment, read at every call: FLEX_MLP_TEST_LAUNCH=1 admits the MLP
    agent (unset or 0: it keeps the loop), FLEX_INTENDED_LAUNCH=1 admits SAFEMADDPG with ``intended_actions``
    (flexenv_test_episodes_routed; unset or 0: it keeps the loop)."""
    args = model.args
    if not args.shared_params:
        return "shared_params is False: the launch stages one shared actor"
    # agent_type mlp (include/flexenv.h: flexenv_test_episodes_mlp) is opt-in: FLEX_MLP_TEST_LAUNCH=1, read at every call
    mlp = (args.agent_type == "mlp" and type(model.policy_dicts[0]) in (MLPAgent, MLPAgentGaussian)
           and os.environ.get("FLEX_MLP_TEST_LAUNCH", "0") == "1")
    if not mlp and (args.agent_type != "rnn" or not isinstance(model.policy_dicts[0], RNNAgent)):
        hint = " (FLEX_MLP_TEST_LAUNCH=1 admits a shared MLP agent)" if args.agent_type == "mlp" else ""
        return f"agent_type {args.agent_type}: the launch holds the RNN actor's tiles" + hint
    if args.hid_size != 64 or args.hid_activation != "relu":
        return f"hid_size {args.hid_size} / hid_activation {args.hid_activation}: the tiles are built for 64 relu units"
    if model.obs_dim > 144 or model.obs_dim % 4:
        return f"obs_size {model.obs_dim}: the tiles hold up to 144 columns, a multiple of 4"
    if model.n_ > 5:
        return f"{model.n_} agents: a block's policy tiles hold sixteen environments of at most 5"
    if model.act_dim != 4:
        return f"action_dim {model.act_dim}: the environment step reads four controls per building"
    if not args.action_enforcebound:
        return "action_enforcebound is False: the launch's test mode is tanh(mean)"
    own = type(model).get_actions
    if own is SAFEMADDPG.get_actions:
        if model.intended_actions and os.environ.get("FLEX_INTENDED_LAUNCH", "0") != "1":
            return "SAFEMADDPG with intended_actions: that routing is not in the launch"
        return None
    if own is MADDPG.get_actions or own is MATD3.get_actions or own is IDDPG.get_actions:
        return None
    return f"{type(model).__name__}.get_actions is none of MADDPG's, SAFEMADDPG's, MATD3's or IDDPG's"


class TestEpisodes:
    """What ``Model.test_episodes`` returns: ``sums`` [N, 10] and ``length`` [N] (NumPy), ``trace`` (dict of NumPy arrays, or
    None), ``launch`` (True: the single launch ran; False: the loop) and ``stat()``."""
    __test__ = False               # (not a pytest class)

    def __init__(self, out, first, launch):
        host = {k: v.cpu().numpy() for k, v in {**out, **first}.items()}
        self.sums, self.length = host.pop("sums"), host.pop("length")
        self.trace = host or None
        self.launch = bool(launch)

    def stat(self):
        return episode_stats(self.sums, self.length)


class Model(nn.Module):
    """model.py:10-323, the parts the MADDPG path uses."""

    def __init__(self, args):
        super().__init__()
        self.args = args
        self.device = th.device("cuda" if th.cuda.is_available() and self.args.cuda else "cpu")
        self.n_ = self.args.agent_num
        self.hid_dim = self.args.hid_size
        self.obs_dim = self.args.obs_size
        self.act_dim = self.args.action_dim
        self.Transition = Transition
        self.batchnorm = nn.BatchNorm1d(self.n_)
        self.fused_inference = True      # no-grad policy passes on the GPU go through csrc/actor.hip

    # -- construction ------------------------------------------------------------------------------
    def construct_model(self):
        """Critic first, then policy: the order of the draws from torch's generator."""
        self.construct_value_net()
        self.construct_policy_net()

    def build_nets(self, target_net):
        """What every algorithm's __init__ does: the nets, their initialisation, the target and its first reload."""
        self.construct_model()
        self.apply(self.init_weights)
        if target_net is not None:
            self.target_net = target_net
            self.reload_params_to_target()

    def build_value_dicts(self, input_shape):
        """``value_dicts`` for critics of ``input_shape`` columns plus the id columns under agent_id: one critic under
        shared_params, else one per agent."""
        input_shape += self.n_ if self.args.agent_id else 0
        count = 1 if self.args.shared_params else self.n_
        self.value_dicts = nn.ModuleList([MLPCritic(input_shape, 1, self.args) for _ in range(count)])

    def construct_policy_net(self):
        """model.py:145-169"""
        input_shape = self.obs_dim + self.n_ if self.args.agent_id else self.obs_dim
        if self.args.gaussian_policy:                     # learned log-std heads (model.py:152-159)
            Agent = {"mlp": MLPAgentGaussian, "rnn": RNNAgentGaussian}[self.args.agent_type]
        else:
            Agent = {"mlp": MLPAgent, "rnn": RNNAgent}[self.args.agent_type]
        count = 1 if self.args.shared_params else self.n_
        self.policy_dicts = nn.ModuleList([Agent(input_shape, self.args) for _ in range(count)])

    def init_weights(self, m):
        """model.py:174-182"""
        if type(m) == nn.Linear:
            if self.args.init_type == "normal":
                nn.init.normal_(m.weight, 0.0, self.args.init_std)
            elif self.args.init_type == "orthogonal":
                nn.init.orthogonal_(m.weight, gain=nn.init.calculate_gain(self.args.hid_activation))

    def reload_params_to_target(self):
        """model.py:22-26 (+ the mixer where the algorithm has one)"""
        self.target_net.policy_dicts.load_state_dict(self.policy_dicts.state_dict())
        self.target_net.value_dicts.load_state_dict(self.value_dicts.state_dict())
        if getattr(self.args, "mixer", False):
            self.target_net.mixer.load_state_dict(self.mixer.state_dict())

    def update_target(self):
        """model.py:28-38: theta' <- (1 - target_lr) theta' + target_lr theta over every state_dict entry
        of the policy and value nets and, with args.mixer, the mixer (floating entries; the nets hold no buffers)."""
        with th.no_grad():
            nets = ["policy_dicts", "value_dicts"] + (["mixer"] if getattr(self.args, "mixer", False) else [])
            tgt = [t for k in nets for t in getattr(self.target_net, k).state_dict().values()]
            src = [t for k in nets for t in getattr(self, k).state_dict().values()]
            th._foreach_mul_(tgt, 1 - self.args.target_lr)
            th._foreach_add_(tgt, src, alpha=self.args.target_lr)

    # -- policy ----------------------------------------------------------------------------------------
    def policy(self, obs, schedule=None, last_act=None, last_hid=None, info={}, stat={}):
        """model.py:102-140. obs [b, n, o] -> means [b, n, a], log_stds, hiddens [b, n, hid]."""
        b = obs.size(0)
        fused = None
        gauss = bool(self.args.gaussian_policy)      # log_stds [b, n, a] from the agents' log-std heads (model.py:119-120,135-136)
        mlp = self.args.shared_params and isinstance(self.policy_dicts[0], MLPAgent)
        standing_aside = False
        if mlp and obs.is_cuda and self.fused_inference:
            # agent_type mlp: csrc/actor_mlp.hip, one launch without a graph and one autograd node with one — for eager calls.
            # While a HIP graph is captured (or audited for a capture) the composition below runs, and nothing is noted.
            agent, out = self.policy_dicts[0], None
            standing_aside = not mlp_actor_allowed()
            if not standing_aside and not th.is_grad_enabled():
                if getattr(agent, "fused_inference", True):
                    out = fused_actor_forward_mlp(agent, obs, self.n_, self.args.agent_id)
            elif (not standing_aside and b * self.n_ >= WGRAD_MIN_ROWS and getattr(agent, "fused_training", True)
                  and not obs.requires_grad):
                why = actor_mlp_declines(agent, obs, self.n_, self.args.agent_id)
                if why is None:
                    out = actor_mlp_train(agent, obs, self.n_, self.args.agent_id)
                else:
                    note_fallback("actor_forward", "update pass: " + why)
            if out is not None:
                means, hiddens = out[0].view(b, self.n_, -1), out[1].view(b, self.n_, -1)
                if gauss:                             # the mean head ran in the fc3 slot; csrc/gauss.hip reads h
                    return means, agent.log_std_of(out[1]).view(b, self.n_, -1), hiddens
                return means, self._log_stds_like(means), hiddens
        if self.args.shared_params and obs.is_cuda and not th.is_grad_enabled() and self.fused_inference and not mlp:
            # rollout steps and bootstrap targets: one HIP launch instead of the module's ten kernels
            fused = fused_actor_forward(self.policy_dicts[0], obs, last_hid, self.n_, self.args.agent_id)
        if fused is not None:
            means = fused[0].view(b, self.n_, -1)
            hiddens = fused[1].view(b, self.n_, -1)
            if gauss:                                 # the mean head ran in the fc2 slot; the log-std head reads the new hidden state
                return means, self.policy_dicts[0].log_std_of(fused[1]).view(b, self.n_, -1), hiddens
            return means, self._log_stds_like(means), hiddens
        if (self.args.shared_params and obs.is_cuda and th.is_grad_enabled() and self.fused_inference
                and b * self.n_ >= WGRAD_MIN_ROWS and isinstance(self.policy_dicts[0], RNNAgent)):
            # update batches: no id concat (the id block of fc1 is an addend per agent), fused LayerNorm/ReLU pass
            out = self.policy_dicts[0].forward_update(obs.reshape(b * self.n_, -1), last_hid, self.n_, self.args.agent_id)
            if out is not None:
                means, hiddens = out[0].view(b, self.n_, -1), out[2].view(b, self.n_, -1)
                if gauss:
                    return means, out[1].view(b, self.n_, -1), hiddens
                return means, self._log_stds_like(means), hiddens
        per_agent_eager = not self.args.shared_params and (gauss or isinstance(self.policy_dicts[0], MLPAgent))
        if per_agent_eager and obs.is_cuda and self.fused_inference:
            # one MLP or Gaussian actor per agent: csrc/actor_mlp.hip's per-agent form, or csrc/actor_unshared.hip with the gradient at the
            # new hidden state, and csrc/gauss.hip's per-agent heads — for eager calls.  While a HIP graph is captured (or audited
            # for a capture) the loop below runs, and nothing is noted.
            out = self._policy_per_agent_eager(obs, last_hid, gauss)
            if out is not None:
                return out
        if not self.args.shared_params and obs.is_cuda and self.fused_inference and not per_agent_eager:
            # one RNN actor per agent with the fixed std (model.py:124-138): one launch over all of them (csrc/actor_unshared.hip)
            # instead of the loop below, captures included.
            out = None
            if not th.is_grad_enabled():
                out = fused_actor_forward_unshared(self.policy_dicts, obs, last_hid)
            elif b * self.n_ >= WGRAD_MIN_ROWS and not last_hid.requires_grad:
                if actor_unshared_supported(self.policy_dicts, obs, self.args.agent_id):
                    out = actor_unshared_train(self.policy_dicts, obs, last_hid)
                else:
                    note_fallback("actor_unshared", f"update pass: agent_type {self.args.agent_type}, hid {self.args.hid_size}, "
                                                    f"act {self.args.hid_activation}, obs {tuple(obs.shape)} {obs.dtype}")
            if out is not None:
                means = out[0].view(b, self.n_, -1)
                return means, self._log_stds_like(means), out[1].view(b, self.n_, -1)
        if (gauss and obs.is_cuda and not standing_aside and self.args.shared_params
                and not isinstance(self.policy_dicts[0], RNNAgent)):
            note_fallback("gaussian_policy", f"agent_type {self.args.agent_type}, shared_params {self.args.shared_params}")
        obs = self.with_ids(obs)
        if self.args.shared_params:
            means, log_stds, hiddens = self.policy_dicts[0](obs.reshape(b * self.n_, -1), last_hid)
            means = means.view(b, self.n_, -1)
            hiddens = hiddens.view(b, self.n_, -1)
            if gauss:
                return means, log_stds.view(b, self.n_, -1), hiddens
        else:
            outs = [pol(obs[:, i, :], last_hid[:, i, :]) for i, pol in enumerate(self.policy_dicts)]
            means = th.stack([o[0] for o in outs], dim=1)
            hiddens = th.stack([o[2] for o in outs], dim=1)
            if gauss:
                return means, th.stack([o[1] for o in outs], dim=1), hiddens
        # fixed_policy_std (model.py:121-123): log(1.0) = 0 at the default config
        return means, self._log_stds_like(means), hiddens

    def _policy_per_agent_eager(self, obs, last_hid, gauss):
        """``policy`` under ``shared_params: False`` for MLP agents and for Gaussian agents of either type, on GPU tensors: the
        launch under no_grad, the autograd node with gradients from WGRAD_MIN_ROWS actor rows, and for Gaussian agents the
        per-agent head node on the ``h`` / new hidden state either returns.  None where the per-agent loop runs: silently while
        a HIP graph is captured or audited (``mlp_actor_allowed``), below the threshold and with a switch off
        (``fused_inference`` / ``fused_training`` on any agent); after a note where the configuration declines."""
        agents = list(self.policy_dicts)
        b, n = obs.size(0), self.n_
        if not mlp_actor_allowed():
            return None
        mlp = isinstance(agents[0], MLPAgent)
        out = None
        if not th.is_grad_enabled():
            if all(getattr(g, "fused_inference", True) for g in agents):
                out = fused_actor_forward_mlp_unshared(agents, obs) if mlp else fused_actor_forward_unshared(agents, obs, last_hid)
        elif (b * n >= WGRAD_MIN_ROWS and not obs.requires_grad and all(getattr(g, "fused_training", True) for g in agents)
              and (mlp or not last_hid.requires_grad)):
            if mlp:
                why = actor_mlp_unshared_declines(agents, obs, self.args.agent_id)
                if why is None:
                    out = actor_mlp_unshared_train(agents, obs)
                else:
                    note_fallback("actor_mlp_unshared", "update pass: " + why)
            elif actor_unshared_supported(agents, obs, self.args.agent_id, kind=type(agents[0])):
                out = actor_unshared_train(agents, obs, last_hid)
            else:
                note_fallback("actor_unshared", f"update pass: agent_type {self.args.agent_type}, hid {self.args.hid_size}, "
                                                f"act {self.args.hid_activation}, obs {tuple(obs.shape)} {obs.dtype}")
        if out is None:
            return None
        means, hiddens = out[0].view(b, n, -1), out[1].view(b, n, -1)
        if not gauss:
            return means, self._log_stds_like(means), hiddens
        why = gauss_head_unshared_declines(agents, out[1])
        if why is None:
            return means, gauss_log_std_unshared(agents, out[1]).view(b, n, -1), hiddens
        note_fallback("gauss_head", "per-agent heads: " + why)
        return means, th.stack([g.log_std_of(hiddens[:, i]) for i, g in enumerate(agents)], dim=1), hiddens

    def _log_stds_like(self, means):
        """fixed_policy_std (model.py:121-123) as a broadcast view of ONE cached element per device — a fill kernel per
        policy call otherwise; nothing downstream writes into it."""
        cache = self.__dict__.setdefault("_log_std_cache", {})
        if means.device not in cache:
            log_std = float(np.log(self.args.fixed_policy_std))
            # the entropy of N(mean, std) does not depend on the mean: with the fixed std it is ONE number
            cache[means.device] = (th.full((1,), log_std, dtype=means.dtype, device=means.device),
                                   th.full((), 0.5 + 0.5 * float(np.log(2.0 * np.pi)) + log_std, dtype=means.dtype,
                                           device=means.device))
        out = cache[means.device][0].expand_as(means)
        out._flex_entropy = cache[means.device][1]        # mean entropy of Normal(means, exp(out)) (util.py:35-36)
        return out

    def summed_std(self, device):
        """exp(sum over agents of the fixed log-std) [a], the standard deviation of the agent-summed action selection: the
        tensor ops' own arithmetic, once per device."""
        cache = self.__dict__.setdefault("_std_sum_cache", {})
        if device not in cache:
            n, a = self.n_, self.act_dim
            with th.no_grad():
                ls = self._log_stds_like(th.zeros(1, n, a, device=device))
                cache[device] = _sum_agents(ls.expand(1, n, a)).exp().reshape(a).to(th.float32).contiguous()
        return cache[device]

    # -- pieces the algorithms' critics and losses share ---------------------------------------------------
    def with_ids(self, rows):
        """[b, n, w] -> [b, n, w + n]: onehot(i) behind agent i's columns (under agent_id)."""
        if self.args.agent_id:
            ids = th.eye(self.n_, device=rows.device, dtype=rows.dtype).expand(rows.size(0), -1, -1)
            rows = th.cat((rows, ids), dim=-1)
        return rows

    # algorithms whose per-agent critics (shared_params False) csrc/critic_unshared.hip covers: their `value` is one MLPCritic
    # per agent on rows made of an observation block, the id columns and an optional action block
    unshared_critic_kernel = False
    # ... and those that take it only under FLEX_UNSHARED_CRITICS=1 (nets.unshared_critics_switch, read at every call)
    unshared_critic_opt_in = False

    def unshared_values(self, obs, act, shared, critic_frozen=False):
        """The per-agent critics of ``shared_params: False`` on the blocks obs [b, n, o] / act [b, n, a] or None in one launch
        per direction (nets.fused_critic_forward_unshared without a graph at any size, the node nets._CriticUnsharedFn with
        one from WGRAD_MIN_ROWS rows): [b, n, 1], or None where the per-agent loop runs — the CPU, ``fused_inference`` off,
        small batches with a graph (silently) and configurations the kernel declines (after a ``critic_unshared`` note)."""
        takes = self.unshared_critic_kernel or (self.unshared_critic_opt_in and unshared_critics_switch())
        if not (takes and not self.args.shared_params and obs.is_cuda and self.fused_inference):
            return None
        b, n = obs.size(0), self.n_
        critics = list(self.value_dicts)
        with_grad = th.is_grad_enabled() and ((act is not None and act.requires_grad) or obs.requires_grad
                                              or any(p.requires_grad for c in critics for p in c.parameters()))
        if not with_grad:
            q = fused_critic_forward_unshared(critics, obs, None if act is None else act.detach(), shared)
        elif b * n < WGRAD_MIN_ROWS:
            return None
        elif critic_unshared_supported(critics, obs, act, shared, train=True):
            q = critic_unshared_train(critics, obs, act, shared, param_grads=not critic_frozen)
        else:
            self.note_unfused("critic_unshared")
            return None
        return None if q is None else q.view(b, n, 1)

    def row_values(self, rows, tall):
        """The critic on materialised rows [b, n, w] -> [b, n, 1]: the shared one on all of them, else agent i's on row i.
        ``tall``: update batches on the GPU take the shared critic's first layer with the batch-reduced weight gradient of
        csrc/wgrad.hip (the library's dW = dY^T X over 163 840 rows took 0.8 ms) and the rest in the fused tail kernels."""
        if not self.args.shared_params:
            return th.stack([net(rows[:, i, :], None)[0] for i, net in enumerate(self.value_dicts)], dim=1)
        b, net = rows.size(0), self.value_dicts[0]
        rows = rows.reshape(b * self.n_, -1)
        if tall and rows.is_cuda and rows.shape[0] >= WGRAD_MIN_ROWS:
            v, _ = net.forward_from_hidden(tall_linear(rows, net.fc1.weight, net.fc1.bias), need_hidden=False)
        else:
            v, _ = net(rows, None)
        return v.view(b, self.n_, -1)

    def policy_term(self, advantages):
        """-mean of the (normalize_advantages: batch-normalised) advantages [b, n]."""
        if self.args.normalize_advantages:
            advantages = self.batchnorm(advantages)
        return mean_all(advantages, sign=-1.0)

    def next_actions(self, next_state, actions_avail, hids, exploration=False, **kw):
        """The restored next actions of a TD target, for a caller under no_grad: from the behaviour policy (double_q) or
        the target policy.  ``kw``: ``clip`` / ``need_log_prob`` where the algorithm's get_actions takes them."""
        return self.get_actions(next_state, status="train", exploration=exploration, actions_avail=actions_avail,
                                target=not self.args.double_q, last_hid=hids, **kw)[1]

    def note_unfused(self, kernel):
        note_fallback(kernel, f"shared_params {self.args.shared_params}, agent_id {self.args.agent_id}, "
                              f"hid {self.args.hid_size}, agents {self.n_}, act_dim {self.act_dim}")

    # -- update cadence (model.py:40-71) -----------------------------------------------------------
    on_policy = False                # IPPO / MAPPO / COMA: the replay is cleared after every update event (model.py:54-57)

    def _unfiled_columns(self, n_envs):
        """What the vectorised rollout files for log_prob_a / value / next_value: constants nobody reads (the DDPG losses)."""
        return dict(log_prob_a=0.0, value=0.0, next_value=0.0)

    def transition_update(self, trainer, trans, stat):
        if self.args.replay:
            if trans is not None:
                trainer.replay_buffer.add_experience(trans)
            replay_cond = trainer.steps > self.args.replay_warmup \
                and len(trainer.replay_buffer.buffer) >= trainer.effective_batch_size() \
                and trainer.steps % self.args.behaviour_update_freq == 0
            if replay_cond:
                if self.on_policy:                        # old values of every transition the event's windows may read
                    self.begin_update_event(trainer)
                if hasattr(trainer, "replay_event"):      # same sub-updates in the same order, software-pipelined
                    trainer.replay_event(stat, self.args.value_update_epochs, self.args.policy_update_epochs)
                else:
                    for _ in range(self.args.value_update_epochs):
                        trainer.value_replay_process(stat)
                    for _ in range(self.args.policy_update_epochs):
                        trainer.policy_replay_process(stat)
                if getattr(self.args, "mixer", False):              # model.py:51-53: after the value and policy steps
                    for _ in range(self.args.mixer_update_epochs):
                        trainer.mixer_replay_process(stat)
                if self.on_policy:                        # model.py:54-57: the data of an on-policy update is used once
                    trainer.replay_buffer.clear()
        else:
            raise NotImplementedError("the MADDPG path always replays (default.yaml:22)")
        if self.args.target and trainer.steps % self.args.target_update_freq == 0:
            self.update_target()

    def episode_update(self, trainer, stat, episode=None):
        """model.py:73-86, the replay branch of ``episodic: True``: the episode joins the replay (``episode``: the list of its
        Transitions, one environment; the vectorised rollouts have filed theirs through ``end_block``), and an update event
        — value sub-updates, policy sub-updates, the mixer's, each on a fresh batch of whole episodes — fires when
        ``trainer.episodes`` is past ``replay_warmup``, a multiple of ``behaviour_update_freq``, and the replay holds a batch
        of episodes.  With a vectorised env ``trainer.episodes`` counts blocks (replay_buffer.EpisodeReplayBuffer).
        Quirks kept from the reference: ``update_target`` is called from transition_update only (model.py:68-71), so in
        episodic mode the target network stays at its initial copy; the on-policy classes' replay is NOT cleared here —
        their episodic mode is batch_size = replay_buffer_size = behaviour_update_freq (default.yaml:1); and without a
        replay the reference reads a buffer that does not exist (model.py:87-97), which raises here.
        On-policy classes: ``begin_update_event`` files value / next_value (/ log_prob_a) of the replay's transitions
        before the first batch is gathered — for every transition in the ring, so outside the on-policy triple, blocks
        older than the last update are re-valued by the current critic."""
        if not self.args.replay:
            raise NotImplementedError("episodic updates without a replay read a buffer the reference never builds (model.py:87-97)")
        if episode is not None:
            trainer.replay_buffer.add_experience(episode)
        replay_cond = trainer.episodes > self.args.replay_warmup \
            and len(trainer.replay_buffer.buffer) >= trainer.effective_batch_size() \
            and trainer.episodes % self.args.behaviour_update_freq == 0
        if replay_cond:
            if self.on_policy:
                self.begin_update_event(trainer)
            for _ in range(self.args.value_update_epochs):
                trainer.value_replay_process(stat)
            for _ in range(self.args.policy_update_epochs):
                trainer.policy_replay_process(stat)
            if getattr(self.args, "mixer", False):
                for _ in range(self.args.mixer_update_epochs):
                    trainer.mixer_replay_process(stat)

    # -- batches -----------------------------------------------------------------------------------------
    def _tensor_batch(self, batch):
        """A Transition of per-sample tuples (trainer.py:68) as a Transition of device tensors; tensors pass through."""
        if not isinstance(batch.reward, th.Tensor):
            batch = Transition(*[th.stack([th.as_tensor(np.asarray(x), dtype=th.float32) for x in f]).to(self.device)
                                 for f in batch])
            # model.py:312-320 concatenates the [1, n, x] per-step arrays along axis 0
            batch = Transition(*[f.squeeze(1) if f.dim() == 4 else f for f in batch])
        return batch

    def unpack_data(self, batch, normalise_reward=True):
        """model.py:308-323.  ``batch`` is a Transition of device tensors (replay_buffer.window) or, for
        callers written against the reference, a Transition of per-sample tuples (trainer.py:68).
        ``normalise_reward=False`` hands the raw reward on: the caller applies the BatchNorm itself (the fused value
        loss does, together with the running-statistics update — exactly once per get_loss call either way)."""
        batch = self._tensor_batch(batch)
        reward = batch.reward.float()
        if self.args.reward_normalisation and normalise_reward:
            # train-mode batch statistics (running stats still update).  The affine pair is in no optimiser
            # (trainer.py:34-35), so its gradient is never used: taking it out of the graph removes a
            # batch-norm backward over [batch, n] that cost 31 % of a value sub-update.
            # The reward columns of a packed replay row are a strided slice: the statistics kernel reads them 3x
            # slower than a contiguous copy (41 vs 14 us for [32768, 5]), so copy first.
            with th.no_grad():
                reward = sync_batchnorm(self.batchnorm, reward.contiguous())     # (= self.batchnorm(reward) on one rank)
        done = batch.done.float().view(-1, 1)
        last_step = batch.last_step.float().view(-1, 1)
        # model.py:313 fills log_prob_a from batch.action; nothing downstream reads it
        return (batch.state, batch.action, batch.action, batch.value, batch.next_value, reward, batch.next_state,
                done, last_step, batch.action_avail, batch.last_hid, batch.hid)

    # -- rollouts ------------------------------------------------------------------------------------------
    def train_process(self, stat, trainer):
        if hasattr(trainer.env, "handle"):          # VecFlexProvisionEnv: batched, sync-free rollout
            return self._train_process_vec(stat, trainer)
        return self._train_process_single(stat, trainer)

    def _train_process_single(self, stat, trainer):
        """model.py:198-267 on a reference-style env (lists of numpy observations, one env)."""
        env = trainer.env
        stat_train = {"mean_train_reward": 0}
        state, _ = env.reset()
        last_hid = self.policy_dicts[0].init_hidden()
        avail = th.tensor(env.get_avail_actions())
        t = 0
        episodic, episode = bool(getattr(self.args, "episodic", False)), []
        for t in range(self.args.max_steps):
            state_ = prep_obs(state).to(self.device).contiguous().view(1, self.n_, self.obs_dim)
            action, action_pol, log_prob_a, _, hid = self.get_actions(state_, status="train", exploration=True,
                                                                      actions_avail=avail, target=False, last_hid=last_hid)
            value = self.value(state_, action_pol)
            _, actual = translate_action(self.args, action, env)
            reward, done, info = env.step(actual)
            next_state = env.get_obs()
            next_state_ = prep_obs(next_state).to(self.device).contiguous().view(1, self.n_, self.obs_dim)
            _, next_action_pol, _, _, _ = self.get_actions(next_state_, status="train", exploration=True,
                                                           actions_avail=avail, target=False, last_hid=hid)
            next_value = self.value(next_state_, next_action_pol)
            done_ = done or t == self.args.max_steps - 1
            trans = Transition(state, action_pol.detach().cpu().numpy(), log_prob_a.detach().cpu().numpy(),
                               value.detach().cpu().numpy(), next_value.detach().cpu().numpy(),
                               np.array([reward] * env.get_num_of_agents()), next_state, done, done_,
                               env.get_avail_actions(), last_hid.detach().cpu().numpy(), hid.detach().cpu().numpy())
            if episodic:                                  # model.py:243-246: collected, no update inside the episode
                episode.append(trans)
            else:
                self.transition_update(trainer, trans, stat)
            for k, v in info.items():
                stat_train["mean_train_" + k] = stat_train.get("mean_train_" + k, 0) + v
            stat_train["mean_train_reward"] += reward
            trainer.steps += 1
            if done_:
                break
            state, last_hid = next_state, hid
        trainer.episodes += 1
        for k, v in stat_train.items():
            if k.split("_")[0] == "mean":
                stat_train[k] = v / float(t + 1)
        stat.update(stat_train)
        if episodic:                                      # model.py:265-266
            self.episode_update(trainer, stat, episode)

    def _train_process_vec(self, stat, trainer):
        """The same rollout over N environments at once.  One "episode" is ``episode_limit - 1`` vector
        steps (what one reference episode executes); environments that terminate early
        (solver failure) are auto-reset by mask.  Nothing in the loop reads a device value on the host;
        statistics are accumulated on the device and fetched once at the end."""
        env = trainer.env
        args = self.args
        N = env.n_envs
        horizon = min(args.max_steps, env.episode_limit - 1)
        if self._use_rollout_graph(trainer):
            return self._train_process_graph(stat, trainer, horizon)
        obs = env.reset().clone()
        last_hid = th.zeros(N, self.n_, self.hid_dim, device=self.device)
        info_sum = th.zeros(env.info.shape[1], dtype=th.float64, device=self.device)
        rew_sum = th.zeros((), dtype=th.float64, device=self.device)
        fail_sum = th.zeros((), dtype=th.float64, device=self.device)
        buf = trainer.replay_buffer
        buf.const_shapes = {"log_prob_a": (self.n_, self.act_dim), "value": (self.n_, 1), "next_value": (self.n_, 1),
                            "action_avail": (self.n_, self.act_dim)}
        std = float(self.args.fixed_policy_std)
        for t in range(horizon):
            with th.no_grad():
                # exploration of select_action (util.py:57-64): tanh(N(mean, std)); every action is available
                # (env:721-730), so the restore mask is the identity and log_prob — unused by the DDPG losses — is
                # not formed.  SAFEMADDPG routes through get_actions for its safety layer.
                if type(self).get_actions is MADDPG.get_actions and self.args.action_enforcebound and self.args.gaussian_policy:
                    means, log_stds, hid = self.policy(obs, last_hid=last_hid)
                    action = action_pol = th.tanh(means + log_stds.exp() * th.randn_like(means))
                elif type(self).get_actions is MADDPG.get_actions and self.args.action_enforcebound:
                    means, _, hid = self.policy(obs, last_hid=last_hid)
                    action = action_pol = th.tanh(means + std * th.randn_like(means))
                else:
                    avail = th.ones(N, self.n_, self.act_dim, device=self.device)
                    action, action_pol, _, _, hid = self.get_actions(obs, status="train", exploration=True,
                                                                     actions_avail=avail, target=False, last_hid=last_hid)
                actual = self.env_action(action)
            # one launch: step + get_obs, and envs that terminate restart in place (their row of env.obs is then
            # the first observation of the new episode; the terminal transition is masked by `done` in the loss)
            reward, done, info = env.step(actual, fuse_obs=True, auto_reset=True)
            next_obs = env.obs
            donef = done.float()
            last_step = donef if t < horizon - 1 else th.ones_like(donef)       # model.py:229
            buf.add_batch(state=obs, action=action_pol, **self._unfiled_columns(N),
                          reward=reward.float().unsqueeze(1).expand(N, self.n_), next_state=next_obs, done=donef,
                          last_step=last_step, action_avail=1.0, last_hid=last_hid, hid=hid)
            if not getattr(args, "episodic", False):
                self.transition_update(trainer, None, stat)
            info_sum += info.sum(0)
            rew_sum += reward.sum()
            fail_sum += env.failed.sum()
            trainer.steps += 1
            # next iteration: terminated envs have restarted; they get a zero hidden state
            obs = next_obs.clone()
            last_hid = hid * (1.0 - donef).view(N, 1, 1)
        trainer.episodes += 1
        denom = float(N * horizon)
        vals = th.cat([info_sum, rew_sum.view(1), fail_sum.view(1)]).cpu().numpy() / denom
        from ._lib import INFO_KEYS
        for i, k in enumerate(INFO_KEYS):
            stat["mean_train_" + k] = float(vals[i])
        stat["mean_train_reward"] = float(vals[-2])
        stat["mean_train_solver_failed"] = float(vals[-1])
        if getattr(args, "episodic", False):              # the block's episodes into the table, then model.py:265-266
            buf.end_block(horizon)
            self.episode_update(trainer, stat)

    def _use_rollout_graph(self, trainer):
        """HIP-graph rollout: CUDA device, not switched off by the trainer.  MADDPG and SAFEMADDPG take the fused two-kernel
        body, MATD3 and IDDPG the general body around their own get_actions; if capture fails the eager loop runs."""
        if not getattr(trainer, "graph_rollout", True) or self.device.type != "cuda":
            return False
        if type(self).__name__ == "SAFEMADDPG":          # the graph body knows the reference's safety-layer order only
            return type(self).get_actions is SAFEMADDPG.get_actions and bool(self.args.action_enforcebound)
        return True                                      # MADDPG: fused path; MATD3 / IDDPG / others: their get_actions

    def _run_lengths(self, steps, horizon):
        """Every run length the loop of _train_process_graph will ask the rollout for, from step counter ``steps`` on: the
        schedule repeats once the counter's phase against the update frequencies repeats at an episode start."""
        freqs = [int(self.args.behaviour_update_freq)] + ([int(self.args.target_update_freq)] if self.args.target else [])
        freqs = [f for f in freqs if f > 0 and not getattr(self.args, "episodic", False)]      # (episodic: nothing interrupts a block)
        period = int(np.lcm.reduce(freqs)) if freqs else 1
        seen, lengths, s = set(), set(), int(steps)
        while s % period not in seen and len(seen) < 4096:
            seen.add(s % period)
            t = 0
            while t < horizon:
                m = min([horizon - t] + [(-s) % f + 1 for f in freqs])
                lengths.add(m)
                t += m
                s += m
        return sorted(lengths)

    def _train_process_graph(self, stat, trainer, horizon):
        env, buf = trainer.env, trainer.replay_buffer
        N = env.n_envs
        rg = getattr(self, "_rollout_graph", None)
        if rg is None or rg.env is not env or rg.buf is not buf:
            rg = None
            try:
                rg = RolloutGraph(self, env, buf)
                rg.start_episode(env.reset())             # the warm-up steps of capture() need a live episode
                rg.capture(lengths=self._run_lengths(trainer.steps, horizon))
            except Exception as exc:                      # capture unsupported here: fall back to the eager loop
                import warnings
                warnings.warn(f"rollout graph capture failed ({exc}); using the eager rollout")
                trainer.graph_rollout = False
                if rg is not None:
                    rg.release()                          # env hooks off, slab ring dropped: add_batch works again
                elif getattr(buf, "slab_mode", False) and buf.length == 0:
                    buf.release_slabs()
                return self._train_process_vec(stat, trainer)
            object.__setattr__(self, "_rollout_graph", rg)
        # model.py:208 resets the environment at the start of every episode.  Here an episode of `horizon` vector steps
        # ends with every environment terminated and restarted IN the last launch (fresh draws from the same reset
        # stream), so the next episode continues from that state: same distribution, and the replay ring stays one
        # unbroken stream (next_state of slab k is slab k + 1).  A hard reset happens when that is not the case: the
        # first episode, environments out of phase (a solver failure restarted some mid-episode), or anybody else having
        # stepped / reset the env since (evaluation).
        if rg.env_calls == getattr(env, "calls", None) and getattr(rg, "in_phase", False):
            rg.start_episode(None)
        else:
            rg.start_episode(env.reset())
        small = buf.small_ring
        last_col = self.n_ * self.act_dim + self.n_ + 1
        # model.py:215-262 steps, then asks transition_update whether an update is due — which it is only when the step
        # counter reaches a multiple of behaviour_update_freq / target_update_freq (model.py:43-50).  The steps up to the
        # next such multiple (or the end of the episode) need nothing from the host and go out as bursts.
        freqs = [int(self.args.behaviour_update_freq)] + ([int(self.args.target_update_freq)] if self.args.target else [])
        episodic = bool(getattr(self.args, "episodic", False))
        if episodic:                                      # no update event interrupts a block: it is a single run
            freqs = []
        t = 0
        while t < horizon:
            s0 = trainer.steps
            m = min([horizon - t] + [(-s0) % f + 1 for f in freqs if f > 0])
            slabs = rg.run(m)
            t += m
            if t == horizon:                                                  # model.py:229: last_step on the final step
                small[slabs[-1], :, last_col] = 1.0
            trainer.steps = s0 + m - 1
            if not episodic:
                self.transition_update(trainer, None, stat)
            trainer.steps += 1
        trainer.episodes += 1
        vals = th.cat([rg.info_sum, rg.rew_sum.view(1), rg.fail_sum.view(1), env.done.double().sum().view(1)]).cpu().numpy()
        rg.in_phase = bool(vals[-1] == N)                 # everybody terminated (and restarted) in the last launch
        rg.env_calls = getattr(env, "calls", None)
        vals = vals[:-1] / float(N * horizon)
        from ._lib import INFO_KEYS
        for i, k in enumerate(INFO_KEYS):
            stat["mean_train_" + k] = float(vals[i])
        stat["mean_train_reward"] = float(vals[-2])
        stat["mean_train_solver_failed"] = float(vals[-1])
        if episodic:                                      # the block's episodes into the table, then model.py:265-266
            buf.end_block(horizon)
            self.episode_update(trainer, stat)

    def env_action(self, action):
        """translate_action (util.py:121-130) kept on the device: [N, n, a] in the env's range.  MATD3 samples ONE
        action from the agent-summed mean (matd3.py:92-97) — in the reference that [1,1,a] tensor cannot even be
        reshaped by env:260; here every agent receives it, which is what its restore_actions broadcast implies."""
        action = action.detach()
        if action.dim() == 3 and action.size(1) == 1 and self.n_ > 1:
            action = action.expand(-1, self.n_, -1)
        return scale_action(self.args, action).reshape(-1, self.n_, self.act_dim)

    def evaluation(self, stat, trainer):
        """model.py:269-306 (test-mode rollouts; next-row f1 of SURVEY §8f)."""
        env = trainer.env
        if hasattr(env, "handle"):
            return self._evaluation_vec(stat, trainer)
        stat_test = {}
        for _ in range(self.args.num_eval_episodes):
            epi = {"mean_test_reward": 0}
            state, _ = env.reset()
            last_hid = self.policy_dicts[0].init_hidden()
            avail = th.tensor(env.get_avail_actions())
            t = 0
            for t in range(self.args.max_steps):
                state_ = prep_obs(state).to(self.device).contiguous().view(1, self.n_, self.obs_dim)
                with th.no_grad():
                    action, _, _, _, hid = self.get_actions(state_, status="test", exploration=False,
                                                            actions_avail=avail, target=False, last_hid=last_hid)
                _, actual = translate_action(self.args, action, env)
                reward, done, info = env.step(actual)
                done_ = done or t == self.args.max_steps - 1
                next_state = env.get_obs()
                for k, v in info.items():
                    epi["mean_test_" + k] = epi.get("mean_test_" + k, 0) + v
                epi["mean_test_reward"] += reward
                if done_:
                    break
                state, last_hid = next_state, hid
            for k, v in epi.items():
                stat_test[k] = stat_test.get(k, 0) + v / float(t + 1)
        for k, v in stat_test.items():
            stat[k] = v / float(self.args.num_eval_episodes)

    # a caller's switch: the periodic evaluation of a vectorised trainer as per-episode statistics (test_episodes below, the
    # reference's own arithmetic: model.py:285-306) instead of evaluate_on's means over env-steps
    one_launch_eval = False

    def _evaluation_vec(self, stat, trainer):
        if self.one_launch_eval:
            stat.update(self.test_episodes(trainer.env).stat())
        else:
            stat.update(self.evaluate_on(trainer.env))

    def evaluate_on(self, env, spec=None):
        """model.py:269-306 on every environment of ``env`` (a VecFlexProvisionEnv, not necessarily the trainer's): one
        test-mode episode each — tanh(mean), no exploration (util.py:79-82) — and the reference's ``mean_test_*`` keys,
        averaged over environments and steps.  ``spec``: injected episode draws (VecFlexProvisionEnv.reset), so that
        different policies are compared on the SAME episodes.  Besides the reference's keys: ``mean_test_violation_rate``
        = share of env-steps with any bus voltage outside [v_min, v_max] (voltage_penalty > 0, env:685) and
        ``mean_test_solver_failed``."""
        bound = self.__dict__.get("env", None)
        rebind = bound is not None and (bound.vec if hasattr(bound, "vec") else bound) is not env
        if rebind:                    # SAFEMADDPG projects against the env it is bound to (safemaddpg.py:143-172)
            self.__dict__["env"] = env
        try:
            return self._evaluate_on(env, spec)
        finally:
            if rebind:
                self.__dict__["env"] = bound

    def _evaluate_on(self, env, spec):
        N = env.n_envs
        horizon = min(self.args.max_steps, env.episode_limit - 1)
        obs = env.reset(spec=spec).clone()
        viol_sum = th.zeros((), dtype=th.float64, device=self.device)
        fail_sum = th.zeros((), dtype=th.float64, device=self.device)
        last_hid = th.zeros(N, self.n_, self.hid_dim, device=self.device)
        avail = th.ones(N, self.n_, self.act_dim, device=self.device)
        info_sum = th.zeros(env.info.shape[1], dtype=th.float64, device=self.device)
        rew_sum = th.zeros((), dtype=th.float64, device=self.device)
        # plain MADDPG in test mode is tanh(mean) (util.py:79-82) -> translate_action: the actor kernel's epilogue with a zero
        # standard deviation, one launch instead of the policy plus a dozen pointwise ones
        fused = (type(self).get_actions is MADDPG.get_actions and self.fused_eval and self.fused_inference
                 and self.args.shared_params and env.obs.is_cuda and self.args.agent_type == "rnn" and self.hid_dim == 64
                 and self.obs_dim <= 144 and bool(self.args.action_enforcebound))
        zero_noise = th.zeros(N, self.n_, self.act_dim, device=self.device) if fused else None
        for t in range(horizon):
            with th.no_grad():
                out = fused_actor_forward(self.policy_dicts[0], obs, last_hid, self.n_, self.args.agent_id, noise=zero_noise,
                                          std=0.0, low=self.args.action_low, high=self.args.action_high) if fused else None
                if out is not None:
                    hid, actual = out[1].view(N, self.n_, -1), out[3].view(N, self.n_, self.act_dim)
                else:
                    action, _, _, _, hid = self.get_actions(obs, status="test", exploration=False, actions_avail=avail,
                                                            target=False, last_hid=last_hid)
                    actual = self.env_action(action)
            reward, done, info = env.step(actual, fuse_obs=True, auto_reset=True)
            info_sum += info.sum(0)
            rew_sum += reward.sum()
            viol_sum += (info[:, 5] > 0).sum()
            fail_sum += env.failed.sum()
            donef = done.float()
            obs = env.obs.clone()
            last_hid = hid * (1.0 - donef).view(N, 1, 1)
        vals = th.cat([info_sum, rew_sum.view(1), viol_sum.view(1), fail_sum.view(1)]).cpu().numpy() / float(N * horizon)
        from ._lib import INFO_KEYS
        stat = {}
        for i, k in enumerate(INFO_KEYS):
            stat["mean_test_" + k] = float(vals[i])
        stat["mean_test_reward"] = float(vals[-3])
        stat["mean_test_violation_rate"] = float(vals[-2])
        stat["mean_test_solver_failed"] = float(vals[-1])
        return stat

    def test_episodes(self, env, spec=None, trace=False, one_launch=None, steps=None):
        """One test-mode episode per environment of ``env`` (model.py:269-306: tanh(mean), no exploration) with a record PER
        EPISODE: ``.sums`` [N, 10] (info[0..6], reward, steps with voltage_penalty > 0, solver_failed, each summed over the
        episode's own steps in step order), ``.length`` [N] (an episode ends with its first ``done`` or after ``steps`` steps,
        default min(max_steps, episode_limit - 1)), ``.stat()`` (``episode_stats``) and, with ``trace``, ``.trace``: the per-step
        arrays of include/flexenv.h FlexTestOut plus ``v0`` / ``agent0`` / ``row0``, the state the reset left.  Nothing is
        accumulated or traced for an environment behind its episode's end; ``env`` is left to be reset by the caller.
        ``one_launch``: None takes the single launch (flexenv_test_episodes) where ``one_launch_declines`` has no objection and
        the tensors are on the GPU, else the loop; False the loop; True raises ValueError with the reason where it declines.
        ``spec``: injected episode draws, as in ``evaluate_on``."""
        vec = env.vec if hasattr(env, "vec") else env
        why = one_launch_declines(self)
        if why is None and not vec.obs.is_cuda:
            why = "the environment is not on a GPU"
        if one_launch and why is not None:
            raise ValueError("test_episodes(one_launch=True): " + why)
        steps = min(self.args.max_steps, vec.episode_limit - 1) if steps is None else int(steps)
        if steps < 1:
            raise ValueError("steps must be >= 1")
        bound = self.__dict__.get("env", None)
        rebind = bound is not None and (bound.vec if hasattr(bound, "vec") else bound) is not vec
        if rebind:                    # SAFEMADDPG projects against the env it is bound to (safemaddpg.py:143-172)
            self.__dict__["env"] = vec
        try:
            with th.no_grad():
                res = None
                if why is None and one_launch is not False:
                    res = self._test_episodes_launch(vec, spec, trace, steps)
                    if res is None and one_launch:
                        raise ValueError("test_episodes(one_launch=True): the library declined the shape")
                if res is None:
                    res = self._test_episodes_loop(vec, spec, trace, steps)
                return res
        finally:
            if rebind:
                self.__dict__["env"] = bound

    def _test_snapshot(self, vec, trace):
        if not trace:
            return {}
        return dict(v0=vec.peek("V"), row0=vec.peek("ROW"),
                    agent0=th.stack([vec.peek(f) for f in ("E", "PRED", "CH", "DIS", "QPV")], dim=-1))

    def _fused_test_policy(self):
        """Where test mode is the actor kernel's epilogue with a zero standard deviation (what _evaluate_on takes for MADDPG);
        SAFEMADDPG's reference routing puts the safety launch behind the same call."""
        own = type(self).get_actions
        safe = own is SAFEMADDPG.get_actions and not self.intended_actions and self.act_dim == 4
        return ((own is MADDPG.get_actions or safe) and self.fused_eval and self.fused_inference and self.args.shared_params
                and self.args.agent_type == "rnn" and self.hid_dim == 64 and self.obs_dim <= 144
                and bool(self.args.action_enforcebound)), safe

    def _test_episodes_loop(self, vec, spec, trace, steps):
        """The loop form of test_episodes: every algorithm, agent type and shared_params value; the launch's record, step by step."""
        N, n, a = vec.n_envs, self.n_, self.act_dim
        obs = vec.reset(spec=spec)
        out = vec.test_out(steps, trace)
        first = self._test_snapshot(vec, trace)
        fused, safe = self._fused_test_policy()
        fused = fused and obs.is_cuda
        last_hid = th.zeros(N, n, self.hid_dim, device=self.device)
        avail = th.ones(N, n, a, device=self.device)
        zero_noise = th.zeros(N, n, a, device=self.device) if fused else None
        alive = th.ones(N, dtype=th.bool, device=self.device)
        for t in range(steps):
            res = fused_actor_forward(self.policy_dicts[0], obs, last_hid, n, self.args.agent_id, noise=zero_noise, std=0.0,
                                      low=self.args.action_low, high=self.args.action_high) if fused else None
            if res is not None and safe:
                hid = res[1].view(N, n, -1)
                actual = vec.safety_project(res[2].view(N, n, a), *self.predictor, self.V_min, self.V_max,
                                            env_action_range=(self.args.action_low, self.args.action_high),
                                            want_hit=False)[2].view(N, n, a)
            elif res is not None:
                hid, actual = res[1].view(N, n, -1), res[3].view(N, n, a)
            else:
                action, _, _, _, hid = self.get_actions(obs, status="test", exploration=False, actions_avail=avail,
                                                        target=False, last_hid=last_hid)
                actual = self.env_action(action).to(th.float32).contiguous()
            reward, done, info = vec.step(actual, fuse_obs=True)
            failed = vec.failed
            col = alive.view(N, 1)
            fig = th.cat([info, reward.view(N, 1), (info[:, 5:6] > 0).double(), failed.view(N, 1).double()], dim=1)
            out["sums"] += th.where(col, fig, th.zeros_like(fig))
            out["length"] += alive.to(th.int32)
            if trace:
                flags = 4 + (done != 0).to(th.uint8) + 2 * (failed != 0).to(th.uint8)
                agent = th.stack([vec.peek(f) for f in ("E", "PRED", "CH", "DIS", "QPV")], dim=-1)
                for k, val in (("actions", actual.reshape(N, n, 4)), ("v", vec.peek("V")), ("agent", agent), ("row", vec.peek("ROW")),
                               ("reward", reward), ("info", info), ("flags", flags)):
                    dst = out[k][t]
                    dst.copy_(th.where(alive.view([N] + [1] * (dst.dim() - 1)), val, th.zeros_like(dst)))
            alive = alive & (done == 0)
            obs, last_hid = vec.obs, hid
        return TestEpisodes(out, first, launch=False)

    def _test_episodes_launch(self, vec, spec, trace, steps):
        """flexenv_test_episodes on the model's shared RNN actor — flexenv_test_episodes_mlp on a shared MLP one
        (``one_launch_declines`` admitted it); None where the library declines the shape."""
        N, n, a = vec.n_envs, self.n_, self.act_dim
        obs = vec.reset(spec=spec)                 # (pushes every first observation: the launch reads the history in place)
        out = vec.test_out(steps, trace)
        first = self._test_snapshot(vec, trace)
        own = type(self).get_actions
        safety = None
        if own is SAFEMADDPG.get_actions:
            s_p, s_q, beta = (th.as_tensor(x, dtype=th.float64, device=vec.device).contiguous() for x in self.predictor)
            safety = dict(s_p=s_p, s_q=s_q, beta=beta, v_min=self.V_min, v_max=self.V_max,
                          adjusted=th.empty(N, 4 * n, dtype=th.float64, device=vec.device),
                          env_action=th.empty(N, 4 * n, dtype=th.float32, device=vec.device),
                          act_low=self.args.action_low, act_high=self.args.action_high)
            if self.intended_actions:          # (one_launch_declines admitted it: FLEX_INTENDED_LAUNCH=1)
                safety["routing"] = 1
        summed = own is MATD3.get_actions or own is IDDPG.get_actions
        agent = self.policy_dicts[0]
        if type(agent) in (MLPAgent, MLPAgentGaussian):
            # (parameters the kernels cannot read through a raw pointer — not fp32, not contiguous: the loop, as the RNN form)
            if mlp_burst_declines(agent, n, self.obs_dim, self.args.agent_id) is not None:
                return None
            # no carried state and no GRU tensors: the output head in the fc2 slot, h of every step in `hid`
            hid = th.empty(N * n, 64, device=vec.device)
            means, action, env_action = (th.empty(N * n, a, device=vec.device) for _ in range(3))
            args, mlp = mlp_test_actor_args(agent, N, n, self.obs_dim, self.args.agent_id, hid, means, action, env_action,
                                            self.args.action_low, self.args.action_high)
            if vec.test_episodes(args, steps, summed=summed, safety=safety, out=out, mlp=mlp) is None:
                return None
            return TestEpisodes(out, first, launch=True)
        done = []
        res = fused_actor_forward(self.policy_dicts[0], obs.view(N, n, -1), th.zeros(N * n, 64, device=vec.device), n,
                                  self.args.agent_id, noise=th.zeros(N, n, a, device=vec.device), std=0.0,
                                  low=self.args.action_low, high=self.args.action_high,
                                  launch=lambda args: done.append(vec.test_episodes(args, steps, summed=summed, safety=safety, out=out)))
        if res is None or not done or done[0] is None:
            return None
        return TestEpisodes(out, first, launch=True)


class MADDPG(Model):
    """maddpg.py:7-123."""

    def __init__(self, args, target_net=None):
        super().__init__(args)
        self.build_nets(target_net)
        self.batchnorm = nn.BatchNorm1d(self.args.agent_num).to(self.device)      # maddpg.py:16

    def construct_value_net(self):
        """maddpg.py:18-27: input (obs+act)*n + n."""
        self.build_value_dicts((self.obs_dim + self.act_dim) * self.n_)

    # replay fields each loss reads (get_loss below; MATD3 and SAFEMADDPG read the same ones): a graphed sub-update
    # refreshes only these columns of its static batch
    # (reward in both: unpack_data's batch-norm running statistics move on every get_loss call, model.py:308-323)
    graph_safe_updates = _GraphSafe(True)       # trainer._graphed_sub_update: the gradient path uses no multi-block PyTorch reduction
    unshared_critic_kernel = True
    update_fields = {"policy": ("state", "reward", "last_hid"),
                     "value": ("state", "action", "reward", "next_state", "done", "hid"),
                     # trainer.replay_event with the bootstrap values filed per transition first (round 3)
                     "value_cached": ("state", "action", "reward", "done", "next_value"),
                     "bootstrap": ("next_state", "hid")}

    def value(self, obs, act, critic_frozen=False):
        """maddpg.py:33-76.  Row i of the reference's critic input is
        [obs_0..obs_{n-1} | onehot(i) | act_0..act_{n-1}] with act_j detached for j != i.  fc1 of that row is
        W_obs @ obs_all + W_id[:, i] + W_act @ act_all(detached) + W_act[:, block i] @ (act_i - act_i.detach()) + b:
        the first and third terms are shared by the n rows of a sample, the last one is zero-valued and only
        carries agent i's own-action gradient.  Returns [b, n, 1].  ``critic_frozen``: the caller differentiates w.r.t. the
        actions only (the policy loss of a policy sub-update) — one autograd node, no critic-parameter gradients."""
        b, n, o, a = obs.size(0), self.n_, self.obs_dim, self.act_dim
        if (critic_frozen and self.args.shared_params and self.args.agent_id and act.requires_grad and th.is_grad_enabled()
                and critic_policy_supported(self.value_dicts[0], obs.reshape(b, n * o), act, n)):
            return CriticTail.apply_policy(obs.reshape(b, n * o), act, self.value_dicts[0]).view(b, n, 1)
        v = self.unshared_values(obs, act, True, critic_frozen)            # non-shared critics: csrc/critic_unshared.hip
        if v is not None:
            return v
        act_det = act.detach()
        own = act - act_det if act.requires_grad else None                # zeros that carry d/d act_i
        values = []
        nets = self.value_dicts if not self.args.shared_params else [self.value_dicts[0]] * 1
        if self.args.shared_params:
            net = self.value_dicts[0]
            W, bias = net.fc1.weight, net.fc1.bias
            W_obs = W[:, :n * o]
            off = n * o
            if self.args.agent_id:
                W_id = W[:, off:off + n]                                  # [hid, n]
                off += n
            W_act = W[:, off:off + n * a]
            act_cols = act_det.reshape(b, n * a)
            obs_cols = obs.reshape(b, n * o)
            if (not act.requires_grad and self.args.agent_id and th.is_grad_enabled() and W.requires_grad
                    and critic_replayed_supported(net, obs_cols, act_cols, n)):
                # value loss on replayed actions: the whole critic as one autograd node (nets._CriticReplayedFn)
                return CriticTail.apply_replayed(obs_cols, act_cols, n, net).view(b, n, 1)
            if not th.is_grad_enabled() or not (W.requires_grad or act.requires_grad or obs.requires_grad):
                # bootstrap targets: no graph — one launch of csrc/linear.hip at update sizes (nets.critic_first_layer), else
                # two library GEMMs (the bias rides the first, the second accumulates)
                with th.no_grad():
                    shared = critic_first_layer(bias, obs_cols, act_cols, W, off)
            else:
                shared = wide_batch_linear(obs_cols, W_obs) + wide_batch_linear(act_cols, W_act) + bias      # [b, hid]
            if not act.requires_grad and self.args.agent_id and critic_tail_supported(net, shared):
                # replayed actions (value loss, bootstrap target): every row is shared[b] + the agent's id column; the
                # fused tail composes it on the fly instead of reading a materialised [b * n, hid] tensor
                return CriticTail.apply_composed(shared, W_id.t(), net).view(b, n, 1)
            h = shared.unsqueeze(1).expand(b, n, -1)
            if self.args.agent_id:
                h = h + W_id.t().unsqueeze(0)                             # [1, n, hid]
            if act.requires_grad:      # zero-valued term that only carries d/d act_i: nothing to add for replayed actions
                h = h + th.einsum("bia,hia->bih", own, W_act.view(-1, n, a))
            v, _ = net.forward_from_hidden(h.reshape(b * n, -1), need_hidden=False)
            return v.view(b, n, 1)
        for i, net in enumerate(nets):                                    # non-shared critics: plain input rows
            acts_i = act_det.clone()
            acts_i[:, i] = act[:, i]
            ids = th.eye(n, device=obs.device, dtype=obs.dtype)[i].expand(b, -1)
            parts = [obs.reshape(b, n * o)] + ([ids] if self.args.agent_id else []) + [acts_i.reshape(b, n * a)]
            v, _ = net(th.cat(parts, dim=-1), None)
            values.append(v)
        return th.stack(values, dim=1)

    def get_actions(self, state, status, exploration, actions_avail, target=False, last_hid=None):
        """maddpg.py:78-98 (continuous branch)."""
        pol = self.target_net.policy if (target and self.args.target) else self.policy
        means, log_stds, hiddens = pol(state, last_hid=last_hid)
        actions, log_prob_a = select_action(self.args, means, status=status, exploration=exploration,
                                            info={"log_std": log_stds})
        if getattr(actions_avail, "_flex_const", None) == 1.0:      # every action available (env:721-730): the mask is 1
            restore_actions = actions
        else:
            restore_mask = 1.0 - (actions_avail.to(means.device) == 0).float()
            restore_actions = restore_mask * actions
        return actions, restore_actions, log_prob_a, (means, log_stds), hiddens

    bootstrap_from_batch = False     # set by trainer.replay_event while it captures / replays value sub-updates on filed values
    bootstrap_cacheable = True       # get_loss below honours bootstrap_from_batch (a subclass with its own get_loss says False)

    def bootstrap_values(self, next_state, actions_avail, hids):
        """Q'(s', pi(s')) [b, n] of maddpg.py:108-111: the next action from the behaviour policy (double_q) or the target
        policy, valued by the target critic; no gradient (maddpg.py:110,115: .detach())."""
        with th.no_grad():
            next_actions = self.next_actions(next_state, actions_avail, hids)
            return self.target_net.value(next_state, next_actions).view(-1, self.n_)

    def get_loss(self, batch, need="both"):
        """maddpg.py:100-123: policy_loss = -Q(s, pi(s)).mean(); value_loss = (r + gamma (1-done) Q'(s', pi(s')) - Q(s,a))^2.mean().

        The reference evaluates both losses in every sub-update and uses one (trainer.py:84,101).  ``need`` =
        "value" / "policy" evaluates only the graph that loss needs — same loss value, same gradients, about half
        the forward work and no backward through the unused half; "both" is the reference's call."""
        # value loss alone on the GPU: reward normalisation, TD target, loss and dLoss/dQ are csrc/tdloss.hip
        on_gpu = (isinstance(batch.reward, th.Tensor) and batch.reward.is_cuda and self.fused_inference
                  and th.is_grad_enabled())
        fused_td = need == "value" and on_gpu
        # the policy loss never reads the reward: all the normalisation owes is the module's running statistics
        stats_only = (need == "policy" and on_gpu and self.args.reward_normalisation
                      and batchnorm_stats_supported(self.batchnorm, batch.reward))
        state, actions, _, _, _, rewards, next_state, done, _, actions_avail, last_hids, hids = \
            self.unpack_data(batch, normalise_reward=not (fused_td or stats_only))
        if stats_only:
            batchnorm_update_running_stats(self.batchnorm, rewards)
        policy_loss = value_loss = None
        action_out = None
        if need in ("both", "policy"):
            _, actions_pol, _, action_out, _ = self.get_actions(state, status="train", exploration=False,
                                                                actions_avail=actions_avail, target=False,
                                                                last_hid=last_hids)
            # need == "policy": a policy sub-update — only the policy optimiser's parameters take this loss's gradient
            # (utils/trainer.py:99-108), so the critic is differentiated w.r.t. the actions alone
            policy_loss = self._critic_policy_loss(state, actions_pol) if need == "policy" else None
            if policy_loss is None:
                advantages = self.value(state, actions_pol, critic_frozen=(need == "policy")).view(-1, self.n_)
                policy_loss = self.policy_term(advantages)
        if need in ("both", "value"):
            if self.bootstrap_from_batch and need == "value":
                # trainer.replay_event filed Q'(s', pi(s')) for this window already (bootstrap_values below, on the same
                # networks: they do not change between the value sub-updates of one update event)
                next_values = batch.next_value.view(-1, self.n_)
            else:
                next_values = self.bootstrap_values(next_state, actions_avail, hids)
            bn = self.batchnorm if self.args.reward_normalisation else None
            if fused_td:
                # update batches: Q(s, a), the TD error and the critic's whole backward in one pass (nets._CriticTdLossFn)
                value_loss = self._critic_td_loss(state, actions, next_values, rewards, done, bn)
                if value_loss is not None:
                    return policy_loss, value_loss, action_out
            values = self.value(state, actions).view(-1, self.n_)
            if fused_td and td_loss_supported(values, next_values, rewards, done, bn):
                value_loss = td_loss(values, next_values, rewards, done, self.args.gamma, bn)
            else:
                if fused_td and bn is not None:                 # the raw reward was handed on: normalise it here
                    with th.no_grad():
                        rewards = sync_batchnorm(bn, rewards.contiguous())
                returns = rewards + self.args.gamma * (1 - done) * next_values
                assert returns.size() == values.size()
                value_loss = mean_all((returns - values).pow(2))
        return policy_loss, value_loss, action_out


def _maddpg_critic_td_loss(self, state, actions, next_values, rewards, done, bn):
    """MADDPG.value + the value loss + the critic's backward as one node, or None where that node does not apply."""
    if not (self.args.shared_params and self.args.agent_id and not actions.requires_grad and self.fused_td_backward
            and type(self).value is MADDPG.value):          # (IDDPG / MATD3 bring their own critic input layout)
        return None
    b, n = state.size(0), self.n_
    net = self.value_dicts[0]
    obs_cols, act_cols = state.reshape(b, n * self.obs_dim), actions.reshape(b, n * self.act_dim)
    if not critic_td_loss_supported(net, obs_cols, act_cols, n, next_values, rewards, done, bn):
        return None
    return critic_td_loss(obs_cols, act_cols, n, net, next_values, rewards, done, self.args.gamma, bn)


def _maddpg_critic_policy_loss(self, state, actions_pol):
    """-mean Q(s, pi(s)) with the critic frozen (a policy sub-update) as one node, or None where that node does not apply."""
    if not (self.args.shared_params and self.args.agent_id and self.fused_td_backward and not self.args.normalize_advantages
            and type(self).value is MADDPG.value and isinstance(actions_pol, th.Tensor) and actions_pol.is_cuda
            and self.fused_inference):
        return None
    b, n = state.size(0), self.n_
    net = self.value_dicts[0]
    obs_cols = state.reshape(b, n * self.obs_dim)
    if not critic_policy_loss_supported(net, obs_cols, actions_pol, n):
        return None
    return critic_policy_loss(obs_cols, actions_pol, net, sign=-1.0)


def _fc1_reads_in_place(self, net):
    """``net``'s first layer is the [64, obs | act | ids] one whose product flexnet_linear2 forms from the ring in place."""
    n, fc1 = self.n_, getattr(net, "fc1", None)
    return ((n * self.obs_dim) % 8 == 0 and (n * self.act_dim) % 4 == 0 and n * (self.obs_dim + self.act_dim) <= 768
            and fc1 is not None and fc1.weight.shape == (64, n * (self.obs_dim + self.act_dim) + n))


def _maddpg_reads_state_in_place(self, bs):
    """True iff a value sub-update on filed bootstrap values ("value_cached") touches ``batch.state`` ONLY through
    nets._CriticTdLossFn — whose first layer (flexnet_linear2) and weight gradient (flexnet_wgrad) can read the window in place
    from the replay's stacked-observation ring (nets.RING_VIEWS; trainer._static_batch then hands a NaN placeholder instead of
    a gathered copy).  The conditions are those of _maddpg_critic_td_loss / nets.critic_td_loss_supported that do not depend on
    the batch's values; a subclass with its own get_loss / value / critic input layout (MATD3, IDDPG) answers False."""
    from .nets import CRITIC_TD_MIN_ROWS, CRITIC_VARIANT
    import safe_marl_amd.nets as _nets
    return bool(type(self).get_loss is MADDPG.get_loss and type(self)._critic_td_loss is _maddpg_critic_td_loss
                and type(self).value is MADDPG.value and self.args.shared_params and self.args.agent_id
                and self.fused_td_backward and self.fused_inference and _nets.CRITIC_FC1_FUSED
                and bs * self.n_ >= CRITIC_TD_MIN_ROWS and CRITIC_VARIANT == 0 and _nets.CRITIC_PGRAD32 == 0
                and _fc1_reads_in_place(self, self.value_dicts[0]))


def _maddpg_reads_next_state_in_place(self, bs):
    """The same question for the graph that files the bootstrap values (MADDPG.bootstrap_values on "next_state", "hid"): the
    policy's fused inference pass (nets.fused_actor_forward) and the target critic's first layer without a graph
    (nets.critic_first_layer) are the only readers of ``next_state``."""
    import safe_marl_amd.nets as _nets
    n = self.n_
    tgt = getattr(self, "target_net", None)
    if tgt is None or type(self).bootstrap_values is not MADDPG.bootstrap_values or type(self).policy is not Model.policy:
        return False
    agent = self.policy_dicts[0]
    a = agent.args
    return bool(type(self).get_actions is MADDPG.get_actions and type(tgt).value is MADDPG.value and self.args.shared_params
                and self.args.agent_id and self.fused_inference and tgt.fused_inference and _nets.CRITIC_FC1_FUSED
                and isinstance(agent, _nets.RNNAgent) and a.hid_size == 64 and a.hid_activation == "relu"
                and self.obs_dim <= 144 and n <= 8 and a.action_dim <= 8
                and _fc1_reads_in_place(self, tgt.value_dicts[0]) and bs * n >= 65536)


MADDPG.reads_state_in_place = _maddpg_reads_state_in_place
MADDPG.reads_next_state_in_place = _maddpg_reads_next_state_in_place
MADDPG._critic_td_loss = _maddpg_critic_td_loss
MADDPG._critic_policy_loss = _maddpg_critic_policy_loss
MADDPG.fused_eval = True                  # (tests switch it off to compare the evaluation with the tensor composition)
MADDPG.fused_td_backward = True          # (tests switch it off to compare with the forward / td_loss / backward sequence)


def _summed_exploration_rows(model, means, log_stds, env_action, action_out):
    """summed_exploration with per-sample log-stds (gaussian_policy): one launch of flexnet_gauss_sum_explore."""
    import torch.distributions.normal as tdn
    from . import _lib
    b, n, a = means.shape
    means = means.contiguous()
    log_stds = log_stds.detach().to(th.float32).expand(b, n, a).contiguous()
    eps = tdn._standard_normal((b, 1, a), means.dtype, means.device)
    out = action_out if action_out is not None else th.empty(b, n, a, dtype=th.float32, device=means.device)
    k = _lib.FlexGaussSumArgs()
    k.n_envs, k.n_agents, k.act_dim = b, n, a
    k.act_low, k.act_high = float(model.args.action_low), float(model.args.action_high)
    k.means, k.log_stds, k.eps, k.action = means.data_ptr(), log_stds.data_ptr(), eps.data_ptr(), out.data_ptr()
    if env_action is not None:
        k.env_action = env_action.data_ptr()
    _lib.launch("flexnet_gauss_sum_explore", k)
    return out


def summed_exploration(model, means, env_action=None, action_out=None, log_stds=None):
    """tanh(sum over agents of the means + exp(sum of log-stds) * eps), the ONE action of matd3.py:92-97 / iddpg.py:66-71
    under util.py:57-64, handed to every agent: [b, n, a] (and, with ``env_action``, translate_action of it) from one launch
    of flexnet_agent_sum_explore.  eps is Normal.rsample's own draw; every fp32 rounding sits where the tensor ops have it.
    ``log_stds`` [b, n, a] without a ``_flex_entropy`` attribute (learned, per sample): flexnet_gauss_sum_explore instead of
    the constant ``summed_std``."""
    if log_stds is not None and getattr(log_stds, "_flex_entropy", None) is None:
        return _summed_exploration_rows(model, means, log_stds, env_action, action_out)
    import torch.distributions.normal as tdn      # (looked up at call time: the very function Normal.rsample calls)
    from . import _lib
    b, n, a = means.shape
    std = model.summed_std(means.device)
    means = means.contiguous()
    eps = tdn._standard_normal((b, 1, a), means.dtype, means.device)
    out = action_out if action_out is not None else th.empty(b, n, a, dtype=th.float32, device=means.device)
    k = _lib.FlexAgentSumArgs()
    k.n_envs, k.n_agents, k.act_dim = b, n, a
    k.act_low, k.act_high = float(model.args.action_low), float(model.args.action_high)
    k.means, k.eps, k.std, k.action = means.data_ptr(), eps.data_ptr(), std.data_ptr(), out.data_ptr()
    if env_action is not None:
        k.env_action = env_action.data_ptr()
    _lib.launch("flexnet_agent_sum_explore", k)
    return out


class _SumBroadcastAgentsFn(th.autograd.Function):
    """y[b, i, :] = ((x[b, 0] + x[b, 1]) + ...) for every agent i — matd3.py:94-97's agent-summed mean handed back to every
    agent (nets.expand_agents of _sum_agents) — and its gradient, which is the same operation on the incoming gradient; one
    launch each way instead of 2 (n - 1) pointwise adds."""

    @staticmethod
    def forward(ctx, x, model):
        ctx.model = model
        return _sum_broadcast(model, x)

    @staticmethod
    def backward(ctx, g):
        return _sum_broadcast(ctx.model, g.contiguous()), None


def _sum_broadcast(model, x):
    from . import _lib
    b, n, a = x.shape
    x = x.contiguous()
    out = th.empty(b, n, a, dtype=th.float32, device=x.device)
    k = _lib.FlexAgentSumArgs()
    k.n_envs, k.n_agents, k.act_dim = b, n, a
    k.means, k.action = x.data_ptr(), out.data_ptr()
    _lib.launch("flexnet_agent_sum_explore", k)
    return out


def _summed_mean_applies(model, means, status, exploration, actions_avail):
    """Training mode without exploration (the losses' policy evaluations): the summed mean to every agent, one launch."""
    return (status == "train" and not exploration and means.is_cuda and means.dtype == th.float32 and means.dim() == 3
            and means.size(-1) > 1 and getattr(actions_avail, "_flex_const", None) == 1.0
            and getattr(model, "fused_inference", False))


def _summed_exploration_applies(model, means, status, exploration, actions_avail, need_log_prob):
    """The one-launch form covers exactly: training-mode exploration with the bound enforced, every action available (the
    constant mask of the vectorised paths), no gradient through the means, nobody asking for the log-probability."""
    return (not need_log_prob and status == "train" and exploration and bool(model.args.action_enforcebound)
            and means.is_cuda and means.dtype == th.float32 and means.dim() == 3 and means.size(-1) > 1
            and not means.requires_grad and getattr(actions_avail, "_flex_const", None) == 1.0
            and getattr(model, "fused_inference", False))


def _sum_agents(x):
    """x.sum(dim=1, keepdim=True) over the (small) agent axis as n - 1 pointwise adds: the same numbers up to fp32
    summation order, and no ATen reduce_kernel in a captured rollout graph (util.GRAPH_DENYLIST is strict about those)."""
    parts = x.unbind(1)
    out = parts[0]
    for p in parts[1:]:
        out = out + p
    return out.unsqueeze(1)


def _summed_get_actions(self, obs, status, exploration, actions_avail, target, last_hid, need_log_prob, clip=False,
                        mask_unavailable=False):
    """The agent-summed action selection of matd3.py:88-111 and iddpg.py:61-83 (continuous branch): the means are summed over
    the AGENT axis before sampling (matd3.py:94-97), and the one action goes to every agent.  ``need_log_prob=False`` (the
    losses and the vectorised rollout never read it): exploration in one launch where ``_summed_exploration_applies``.
    ``mask_unavailable``: MATD3 zeroes the means and log-stds of unavailable actions first; ``clip``: its target smoothing."""
    pol = self.target_net.policy if (target and self.args.target) else self.policy
    means, log_stds, hiddens = pol(obs, last_hid=last_hid)
    if _summed_exploration_applies(self, means, status, exploration, actions_avail, need_log_prob):
        restore_actions = summed_exploration(self, means, log_stds=log_stds)
        return restore_actions[:, :1], restore_actions, None, (means, log_stds), hiddens
    if _summed_mean_applies(self, means, status, exploration, actions_avail):
        restore_actions = _SumBroadcastAgentsFn.apply(means, self)
        return restore_actions[:, :1], restore_actions, None, (means, log_stds), hiddens
    avail = actions_avail
    if mask_unavailable:
        avail = avail.to(means.device)
        means = means.masked_fill(avail == 0, 0.0)
        log_stds = log_stds.masked_fill(avail == 0, 0.0)
    if means.size(-1) > 1:                                              # matd3.py:94-96: sum over dim=1 (agents)
        means_, log_stds_ = _sum_agents(means), _sum_agents(log_stds)
    else:
        means_, log_stds_ = means, log_stds
    actions, log_prob_a = select_action(self.args, means_, status=status, exploration=exploration,
                                        info={"clip": clip, "log_std": log_stds_})
    if getattr(actions_avail, "_flex_const", None) == 1.0 and actions.size(1) == 1:
        # every action available (env:721-730): the mask is 1; the agent-summed action goes to every agent
        restore_actions = expand_agents(actions, self.n_)
    else:                               # (the mask reaches the device only here, unless MATD3 moved it above)
        restore_actions = (1.0 - (avail.to(means.device) == 0).float()) * actions
    return actions, restore_actions, log_prob_a, (means, log_stds), hiddens


class MATD3(MADDPG):
    """madrl/models/matd3.py:8-149: twin centralised critics realised as ONE shared network with
    a trailing 0/1 input flag (matd3.py:64-67), clipped-double-Q target min(Q1', Q2') (matd3.py:139-140) and a
    value loss averaged over the twins (matd3.py:148).  Bug-compatible with the reference's action selection, which
    sums the policy means over the AGENT axis before sampling (matd3.py:92-97)."""
    bootstrap_cacheable = False      # own get_loss (min of twins, target-smoothing noise drawn inside): values are per sub-update
    unshared_critic_kernel = False   # (its fc1 holds the flag column: not csrc/critic_unshared.hip's row)
    unshared_twin_kernel = True      # per-agent twin critics (shared_params False): csrc/critic_unshared_twin.hip

    # since round 2 the GPU path of both losses reduces only through this project's fixed-order kernels (twin critic
    # nodes, flexnet_td_loss, flexnet_scaled_sum, pointwise agent sums): sub-updates replay as HIP graphs like MADDPG's
    graph_safe_updates = _GraphSafe(True)

    def construct_value_net(self):
        """matd3.py:18-27: the MADDPG critic input plus the twin flag."""
        self.build_value_dicts((self.obs_dim + self.act_dim) * self.n_ + 1)

    def value(self, obs, act, critic_frozen=False, first_head_only=False):
        """matd3.py:33-86: returns cat([Q1, Q2], dim=0) of shape [2b, n, 1] (``first_head_only``: Q1 alone, [b, n, 1] — all
        the policy loss reads, matd3.py:121).  Same column-block evaluation as MADDPG.value; the twin flag only adds
        fc1.weight's last column to the second head's pre-activation."""
        if not self.args.shared_params:
            return self.unshared_twin_values(obs, act, critic_frozen, first_head_only)
        b, n, o, a = obs.size(0), self.n_, self.obs_dim, self.act_dim
        net = self.value_dicts[0]
        W, bias = net.fc1.weight, net.fc1.bias
        obs_cols = obs.reshape(b, n * o)
        if self.args.agent_id and obs.is_cuda:
            # GPU paths as single autograd nodes / fused tails (nets.py), every reduction in this project's kernels
            if (critic_frozen and first_head_only and act.requires_grad and th.is_grad_enabled()
                    and critic_policy_supported(net, obs_cols, act, n)):
                return CriticTail.apply_policy(obs_cols, act, net).view(b, n, 1)
            act_cols = act.detach().reshape(b, n * a)
            if (not act.requires_grad and th.is_grad_enabled() and W.requires_grad
                    and critic_replayed_supported(net, obs_cols, act_cols, n)):
                if W.shape[1] == n * o + n + n * a + 1 and self.fused_twin:
                    # both heads as one node: fc1's output formed once, its weight gradient taken once (nets._CriticReplayedTwinFn)
                    return CriticTail.apply_replayed_twin(obs_cols, act_cols, n, net).view(2 * b, n, 1)
                q1 = CriticTail.apply_replayed(obs_cols, act_cols, n, net)
                q2 = CriticTail.apply_replayed(obs_cols, act_cols, n, net, twin=True)
                return th.cat([q1.view(b, n, 1), q2.view(b, n, 1)], dim=0)
            if not th.is_grad_enabled() and critic_tail_supported(net, obs_cols.new_empty(1, self.hid_dim)):
                off = n * o
                shared = th.addmm(bias, obs_cols, W[:, :off].t())
                shared.addmm_(act_cols, W[:, off + n:off + n + n * a].t())
                ids = W[:, off:off + n].t()
                q1 = CriticTail.apply_composed(shared, ids, net)
                q2 = CriticTail.apply_composed(shared, ids + W[:, -1], net)
                return th.cat([q1.view(b, n, 1), q2.view(b, n, 1)], dim=0)
        act_det = act.detach()
        own = act - act_det
        off = n * o
        h = wide_batch_linear(obs_cols, W[:, :off]) + bias
        h = h.unsqueeze(1).expand(b, n, -1)
        if self.args.agent_id:
            h = h + W[:, off:off + n].t().unsqueeze(0)
            off += n
        W_act = W[:, off:off + n * a]
        h = h + (act_det.reshape(b, n * a) @ W_act.t()).unsqueeze(1)
        if act.requires_grad:
            h = h + th.einsum("bia,hia->bih", own, W_act.view(-1, n, a))
        flag = W[:, off + n * a]                                            # column of the 0/1 twin flag
        v1, _ = net.forward_from_hidden(h.reshape(b * n, -1), need_hidden=False)
        if first_head_only:
            return v1.view(b, n, 1)
        v2, _ = net.forward_from_hidden((h + flag).reshape(b * n, -1), need_hidden=False)
        return th.cat([v1.view(b, n, 1), v2.view(b, n, 1)], dim=0)

    def unshared_twin_values(self, obs, act, critic_frozen=False, first_head_only=False):
        """matd3.py:74-82 under ``shared_params: False``: agent i's own critic on its row, the twin flag at 0 and at 1 ->
        cat([Q1, Q2], 0) [2b, n, 1] (``first_head_only``: Q1, [b, n, 1]).  On the GPU with ``fused_inference``
        csrc/critic_unshared_twin.hip forms the first layer once per row: one launch without gradients at any size
        (nets.fused_critic_forward_unshared_twin), the node nets._CriticUnsharedTwinFn from WGRAD_MIN_ROWS rows with them.
        Elsewhere — the CPU, small batches with gradients, both heads of an action that takes a gradient, configurations the
        kernel declines (after a ``critic_unshared_twin`` note) — the per-agent loop as a tensor composition that carries the
        own-action gradient as MADDPG.value's loop does."""
        b, n, o, a = obs.size(0), self.n_, self.obs_dim, self.act_dim
        critics = list(self.value_dicts)
        heads = 1 if first_head_only else 2
        if self.unshared_twin_kernel and obs.is_cuda and self.fused_inference:
            with_grad = th.is_grad_enabled() and (act.requires_grad or obs.requires_grad
                                                  or any(p.requires_grad for c in critics for p in c.parameters()))
            q = None
            if not with_grad:
                q = fused_critic_forward_unshared_twin(critics, obs, act.detach(), heads)
            elif b * n >= WGRAD_MIN_ROWS and not (act.requires_grad and heads == 2):
                if critic_unshared_twin_supported(critics, obs, act, heads, train=True):
                    q = critic_unshared_twin_train(critics, obs, act, heads, param_grads=not critic_frozen)
                else:
                    self.note_unfused("critic_unshared_twin")
            if q is not None:
                return q.view(heads * b, n, 1)
        act_det = act.detach()
        obs_cols = obs.reshape(b, n * o)
        values1, values2 = [], []
        for i, net in enumerate(critics):
            acts_i = act_det
            if act.requires_grad:                                         # the others' actions detached (matd3.py:46-53)
                acts_i = act_det.clone()
                acts_i[:, i] = act[:, i]
            W = net.fc1.weight
            h = obs_cols @ W[:, :n * o].t() + net.fc1.bias
            off = n * o
            if self.args.agent_id:
                h = h + W[:, off + i]
                off += n
            h = h + acts_i.reshape(b, n * a) @ W[:, off:off + n * a].t()
            values1.append(net.forward_from_hidden(h, need_hidden=False)[0])
            if not first_head_only:
                values2.append(net.forward_from_hidden(h + W[:, off + n * a], need_hidden=False)[0])
        v1 = th.stack(values1, dim=1)
        if first_head_only:
            return v1
        return th.cat([v1, th.stack(values2, dim=1)], dim=0)

    def get_actions(self, obs, status, exploration, actions_avail, target=False, last_hid=None, clip=False, need_log_prob=True):
        """matd3.py:88-111 (continuous branch): the agent-summed selection on means masked where unavailable."""
        return _summed_get_actions(self, obs, status, exploration, actions_avail, target, last_hid, need_log_prob,
                                   clip=clip, mask_unavailable=True)

    def get_loss(self, batch, need="both"):
        """matd3.py:113-149.  ``need`` = "value" / "policy" (what a sub-update asks for) on the GPU: the reward BatchNorm
        and both TD terms through flexnet_td_loss (batch statistics once, running statistics moved once), the policy loss
        through the first head's action-gradient node; "both" is the reference's call."""
        on_gpu = (isinstance(batch.reward, th.Tensor) and batch.reward.is_cuda and self.fused_inference
                  and th.is_grad_enabled() and need in ("value", "policy") and self.args.reward_normalisation
                  and batchnorm_stats_supported(self.batchnorm, batch.reward))
        state, actions, _, _, _, rewards, next_state, done, _, actions_avail, last_hids, hids = \
            self.unpack_data(batch, normalise_reward=not on_gpu)
        b = state.size(0)
        policy_loss = value_loss = action_out = None
        if need in ("both", "policy"):
            if on_gpu:                      # the policy loss never reads the reward: the module's bookkeeping only
                batchnorm_update_running_stats(self.batchnorm, rewards)
            _, actions_pol, _, action_out, _ = self.get_actions(state, status="train", exploration=False,
                                                                actions_avail=actions_avail, target=False,
                                                                last_hid=last_hids)
            if on_gpu:
                advantages = self.value(state, actions_pol, critic_frozen=True, first_head_only=True).reshape(-1, self.n_)
            else:
                advantages = self.value(state, actions_pol)[:b].reshape(-1, self.n_)      # first head only
            policy_loss = self.policy_term(advantages)
        if need in ("both", "value"):
            with th.no_grad():
                next_actions = self.next_actions(next_state, actions_avail, hids, exploration=True, clip=True,
                                                 need_log_prob=False)
                nxt = self.target_net.value(next_state, next_actions)
                next_min = th.min(nxt[:b].reshape(-1, self.n_), nxt[b:].reshape(-1, self.n_))
            cur = self.value(state, actions)
            values1, values2 = cur[:b].reshape(-1, self.n_), cur[b:].reshape(-1, self.n_)
            if on_gpu and td_loss_supported(values1, next_min, rewards, done, self.batchnorm):
                # matd3.py:141-148: both twins against the same normalised return; the second term must not move the
                # BatchNorm's running statistics again
                value_loss = 0.5 * (td_loss(values1, next_min, rewards, done, self.args.gamma, self.batchnorm)
                                    + td_loss(values2, next_min, rewards, done, self.args.gamma, self.batchnorm,
                                              update_stats=False))
            else:
                if on_gpu:                  # the raw reward was handed on: normalise it here
                    with th.no_grad():
                        rewards = sync_batchnorm(self.batchnorm, rewards.contiguous())
                returns = rewards + self.args.gamma * (1 - done) * next_min
                assert returns.size() == values1.size() == values2.size()
                value_loss = 0.5 * (mean_all((returns - values1).pow(2)) + mean_all((returns - values2).pow(2)))
        return policy_loss, value_loss, action_out


MATD3.fused_twin = True             # (tests switch it off to compare with the two single-head nodes)


class IDDPG(MADDPG):
    """madrl/models/iddpg.py:7-83 with the loss of madrl/learning_algorithms/ddpg.py:14-37:
    independent critics Q_i(o_i, a_i) on the agent's own observation and action (plus its one-hot id), the same
    DDPG losses as MADDPG, and the agent-summed action selection it shares with MATD3 (iddpg.py:66-71)."""

    graph_safe_updates = _GraphSafe(True)       # as MATD3: no PyTorch reduction is left on the GPU path of either loss

    def construct_value_net(self):
        """iddpg.py:17-26"""
        self.build_value_dicts(self.obs_dim + self.act_dim)

    def value(self, obs, act, critic_frozen=False):
        """iddpg.py:32-59: rows [o_i | onehot(i) | a_i] -> [b, n, 1]."""
        v = self.unshared_values(obs, act, False, critic_frozen)
        if v is not None:
            return v
        return self.row_values(th.cat((self.with_ids(obs), act), dim=-1), True)

    def get_actions(self, state, status, exploration, actions_avail, target=False, last_hid=None, need_log_prob=True):
        """iddpg.py:61-83 (continuous branch): the means are summed over the agent axis before sampling."""
        return _summed_get_actions(self, state, status, exploration, actions_avail, target, last_hid, need_log_prob)


class SAFEMADDPG(MADDPG):
    """safemaddpg.py:14-299: MADDPG whose get_actions passes the proposed action through the safety layer.

    The reference solves a Pyomo QP with Gurobi per call (safemaddpg.py:176-299) using a pickled sklearn
    regressor (safemaddpg.py:27); here the layer is the HIP closed-form projection
    (``flexenv_safety_project``) and the regressor's row sums come from ``safety_signal.fit_voltage_predictor``
    (or any (s_p, s_q, beta) triple the caller passes as ``predictor``)."""

    def __init__(self, args, env, target_net=None, predictor=None):
        super().__init__(args, target_net)
        self.env = env
        self.V_min = args.v_min
        self.V_max = args.v_max
        self.solver_interventions = 0
        self.solver_infeasible = 0
        if predictor is None:
            from .safety_signal import fit_voltage_predictor
            vec = env.vec if hasattr(env, "vec") else env
            predictor = fit_voltage_predictor(vec.net, device=vec.device).building_terms(vec.net)
        self.predictor = predictor          # (s_p [n], s_q [n], beta [n]) per building

    def safety_layer_optimization(self, proposed_actions):
        """safemaddpg.py:176-299 on every env of the batch: returns [B, 4n] type-major adjusted actions."""
        vec = self.env.vec if hasattr(self.env, "vec") else self.env
        s_p, s_q, beta = self.predictor
        adjusted, hit = vec.safety_project(proposed_actions.detach().reshape(-1, self.n_, self.act_dim),
                                           s_p, s_q, beta, self.V_min, self.V_max)
        self._last_intervened = hit
        return adjusted

    def get_actions(self, state, status, exploration, actions_avail, target=False, last_hid=None):
        """safemaddpg.py:90-111.  During a loss evaluation (batch != env batch) the reference solves the QP on
        batch element 0 against the live env and discards the result (safemaddpg.py:118-121);
        that call is skipped here — it has no observable effect."""
        actions, restore_actions, log_prob_a, action_out, hiddens = super().get_actions(
            state, status, exploration, actions_avail, target, last_hid)
        vec = self.env.vec if hasattr(self.env, "vec") else self.env
        if state.size(0) != vec.n_envs:
            return actions, restore_actions, log_prob_a, action_out, hiddens
        adjusted = self.safety_layer_optimization(restore_actions).to(th.float32)   # safemaddpg.py:106-109
        return adjusted, restore_actions, log_prob_a, action_out, hiddens

    # NOT the reference's behaviour (off by default; no parity claim is made with it on).  The reference hands the safety
    # layer's type-major physical-unit vector (safemaddpg.py:297) through translate_action (util.py:125-128: clamp to [0, 1],
    # then 0.5 (a + 1)) to an env that re-reads it agent-major as raw values (env:268-274) — SURVEY A13.  Every entry then
    # arrives >= 0.5: the load reduction is clipped to its maximum, charging and discharging cancel at their maxima, and q
    # lands in [0.5, 0.5 + c] pu, so the policy cannot move the environment (tools/learning_curve.py: the test reward of
    # SAFEMADDPG stays within 3e-4 of -0.097 from the untrained policy to episode 400, at either batch size).  With
    # ``intended_actions`` the adjusted (percentage, charge, discharge, q) of building i reaches the env as is, agent-major:
    # what safemaddpg.py:90-111 evidently means to do.
    intended_actions = False

    def env_action(self, action):
        if self.intended_actions:
            return action.detach().reshape(-1, self.act_dim, self.n_).transpose(1, 2).to(th.float32).contiguous()
        # the type-major flat vector is re-read agent-major by env.step (safemaddpg.py:297 vs env:268-274, A13)
        return scale_action(self.args, action.detach()).reshape(-1, self.n_, self.act_dim)


class FACMADDPG(IDDPG):
    """madrl/models/facmaddpg.py:9-114: IDDPG's per-agent critic Q_i(o_i, a_i) and agent-summed action selection
    (facmaddpg.py:36-83, inherited unchanged), mixed into Q_tot(s, Q_1..Q_n) by a QMIX mixer over the global state
    (madrl/critics/qmix.py; nets.QMixer, csrc/qmix.hip on the GPU).  The value loss is on Q_tot against the reward of
    agent 0 (facmaddpg.py:106); the policy loss is IDDPG's, without the mixer.  The mixer has an optimiser of its own
    (trainer.mixer_replay_process, args.mixer)."""

    graph_safe_updates = False       # sub-updates run eagerly (the mixer's losses are not audited for graph capture)
    unshared_critic_kernel = False   # (unshared critics keep the per-agent loop ...
    unshared_critic_opt_in = True    # ... unless FLEX_UNSHARED_CRITICS=1: then IDDPG's rows through csrc/critic_unshared.hip)
    bootstrap_cacheable = False      # own get_loss: the bootstrap target is Q_tot', not per-agent values

    def construct_value_net(self):
        """facmaddpg.py:19-30"""
        super().construct_value_net()
        self.mixer = QMixer(self.args)

    def get_loss(self, batch, need="both"):
        """facmaddpg.py:85-114.  ``need`` = "value" (gradients for the critic: the mixer is differentiated w.r.t. its input
        only), "mixer" (gradients for the mixer: the critic's values enter as data), "policy", or "both" (the reference's
        call).  The value and mixer sub-updates step on the same loss."""
        state, actions, _, _, _, rewards, next_state, done, _, actions_avail, last_hids, hids = self.unpack_data(batch)
        b, n = state.size(0), self.n_
        policy_loss = value_loss = action_out = None
        if need in ("both", "policy"):
            _, actions_pol, _, action_out, _ = self.get_actions(state, status="train", exploration=False,
                                                                actions_avail=actions_avail, target=False,
                                                                last_hid=last_hids)
            # (a policy sub-update takes the own-action gradient alone: the per-agent kernels skip the critics' parameter gradients)
            policy_loss = self.policy_term(self.value(state, actions_pol, critic_frozen=(need == "policy")).contiguous().view(-1, n))
        if need in ("both", "value", "mixer"):
            with th.no_grad():
                # double_q: the next actions from the behaviour policy (facmaddpg.py:90-93), valued by the target critic
                # and mixed by the target mixer on s' (facmaddpg.py:99-102)
                next_actions = self.next_actions(next_state, actions_avail, hids)
                next_values = self.target_net.value(next_state, next_actions).contiguous().view(-1, n)
                next_q_tot = self.target_net.mixer(next_values, next_state.reshape(b, n * self.obs_dim)).view(-1, 1)
            if need == "mixer":
                with th.no_grad():
                    values = self.value(state, actions).contiguous().view(-1, n)
            else:
                values = self.value(state, actions).contiguous().view(-1, n)
            q_tot = self.mixer(values, state.reshape(b, n * self.obs_dim), param_grads=(need != "value")).view(-1, 1)
            returns = rewards[:, 0:1] + self.args.gamma * (1 - done) * next_q_tot
            assert returns.size() == q_tot.size()
            value_loss = mean_all((returns - q_tot).pow(2))
        return policy_loss, value_loss, action_out


class SQDDPG(MADDPG):
    """madrl/models/sqddpg.py:8-158: MADDPG's centralised critic (same construction and state_dict keys) valued on sampled
    coalitions.  For each of ``sample_size`` uniformly random agent orders per sample, row (b, s, i) of the critic holds every
    observation, the actions of the agents placed at or before agent i (in coalition order; the others' actions detached)
    and onehot(i); phi[b, i] = mean over s is agent i's Shapley estimate.  The policy loss is -mean(phi), the value loss is
    on S = sum_i phi with the target S' of the target critic, every term on FRESH coalitions.  Action selection is IDDPG's
    agent-summed one (sqddpg.py:109-129).  On the GPU, csrc/sqddpg.hip draws the coalitions and runs the critic without
    materialising the [b ns n, 745] rows (nets.sqddpg_shapley_fused); elsewhere the reference's composition
    (``marginal_contribution_torch``)."""

    graph_safe_updates = False       # sub-updates run eagerly (fresh coalitions per call; not audited for graph capture)
    unshared_critic_kernel = False   # (unshared critics run the composition; FLEX_UNSHARED_CRITICS=1: csrc/sqddpg_unshared.hip)
    bootstrap_cacheable = False      # own get_loss: the target term draws its own coalitions in every value sub-update
    get_actions = IDDPG.get_actions  # the same function object (RolloutGraph.summed checks identity)
    coalition_source = None          # tests: callable(role, groups) -> pos [groups, n], role "policy" / "value" / "target"

    def __init__(self, args, target_net=None):
        super().__init__(args, target_net)
        self.sample_size = int(args.sample_size)
        self._coalition_rng = None

    # -- coalitions ------------------------------------------------------------------------------------
    def draw_coalitions(self, role, batch_size, device):
        """pos [b ns, n]: pos[g, i] is the position of agent i in coalition group g = b ns + s (the raw th.multinomial
        output of sqddpg.py:35-40).  ``coalition_source`` when set; on the GPU the device draw of csrc/sqddpg.hip from a
        [seed, step] stream seeded from torch's generator (no host synchronisation after the first call); else
        th.multinomial as the reference."""
        groups = batch_size * self.sample_size
        n = self.n_
        if self.coalition_source is not None:
            return self.coalition_source(role, groups).to(device)
        if device.type == "cuda" and self.fused_inference:
            if self._coalition_rng is None or self._coalition_rng.device != device:
                seed = int(th.randint(0, 2 ** 62, (1,)).item())
                self._coalition_rng = th.tensor([seed, 0], dtype=th.int64, device=device)
            return sqddpg_draw(groups, n, self._coalition_rng)
        weights = th.full((groups, n), 1.0 / n, dtype=th.float64, device=device)
        return th.multinomial(weights, n, replacement=False)

    def coalition_maps(self, pos, batch_size):
        """sqddpg.py:35-61 from the drawn positions: (subcoalition map, grand coalitions, individual map), each
        [b, ns, n, n].  individual[.., i, p] = 1 at p = pos[g, i]; subcoalition[.., i, p] = 1 for p <= pos[g, i];
        grand[.., i, p] = the agent at position p (the same for every i)."""
        b, ns, n = batch_size, self.sample_size, self.n_
        pos = pos.long().reshape(b * ns, n)
        individual = th.zeros(b * ns * n, n, device=pos.device).scatter_(1, pos.reshape(-1, 1), 1.0).view(b, ns, n, n)
        subcoalition = th.matmul(individual, th.tril(th.ones(n, n, device=pos.device)))
        grand = th.empty_like(pos).scatter_(1, pos, th.arange(n, device=pos.device).expand(b * ns, n))
        grand = grand.view(b, ns, 1, n).expand(b, ns, n, n)
        return subcoalition, grand, individual

    def marginal_contribution_torch(self, obs, act, pos):
        """sqddpg.py:63-104 on given coalitions: the critic's values [b, ns, n, 1] of the materialised rows
        [obs_0 .. obs_{n-1} | block p = act of the agent at position p if p <= pos[g, i] else 0 | onehot(i)]."""
        b, ns, n, o, a = obs.size(0), self.sample_size, self.n_, self.obs_dim, self.act_dim
        subcoalition, grand, individual = self.coalition_maps(pos, b)
        acts = act.view(b, 1, 1, n, a).expand(b, ns, n, n, a).gather(3, grand.unsqueeze(-1).expand(b, ns, n, n, a))
        others = (subcoalition - individual).unsqueeze(-1)
        acts = (acts * others).detach() + acts * individual.unsqueeze(-1)          # only agent i's own action keeps its gradient
        rows = th.cat((obs.reshape(b, 1, 1, n * o).expand(b, ns, n, n * o), acts.reshape(b, ns, n, n * a)), dim=-1)
        return self.row_values(self.with_ids(rows.reshape(b * ns, n, -1)), False).reshape(b, ns, n, 1)

    def _fused(self, act):
        if not act.is_cuda:
            return False
        ok = (self.args.shared_params and self.fused_inference and act.dtype == th.float32
              and sqddpg_fused_config(self.value_dicts[0], self.n_, self.act_dim, self.sample_size))
        if not ok:
            self.note_unfused("sqddpg")
        return ok

    def _unshared_kernel(self, obs, act):
        """Per-agent critics (shared_params False) on GPU tensors under FLEX_UNSHARED_CRITICS=1: whether
        csrc/sqddpg_unshared.hip covers the call; a decline leaves a ``sqddpg_unshared`` note."""
        ok = (self.fused_inference and act.dtype == th.float32 and obs.dtype == th.float32 and obs.is_cuda
              and sqddpg_unshared_config(self.value_dicts, self.n_, self.act_dim, self.sample_size))
        if not ok:
            self.note_unfused("sqddpg_unshared")
        return ok

    def shapley_values(self, obs, act, pos, want_q=False, frozen=False):
        """(phi [b, n], values [b, ns, n, 1] or None) on the coalitions ``pos``; ``frozen``: no critic-parameter gradients."""
        b, n = obs.size(0), self.n_
        if not self.args.shared_params and act.is_cuda and unshared_critics_switch():
            # opt-in (the default keeps the composition and its "sqddpg" note): one critic per agent in csrc/sqddpg_unshared.hip
            if self._unshared_kernel(obs, act):
                phi, q = sqddpg_shapley_unshared(self.value_dicts, obs.reshape(b, n * self.obs_dim), act, pos,
                                                 self.sample_size, want_q=want_q, frozen=frozen)
                return phi, (q.unsqueeze(-1) if want_q else None)
        elif self._fused(act):
            phi, q = sqddpg_shapley_fused(self.value_dicts[0], obs.reshape(b, n * self.obs_dim), act.to(th.float32),
                                          pos, self.sample_size, want_q=want_q, frozen=frozen)
            return phi, (q.unsqueeze(-1) if want_q else None)
        values = self.marginal_contribution_torch(obs, act, pos)
        return values.mean(dim=1).reshape(b, n), values

    def value(self, obs, act, critic_frozen=False):
        """sqddpg.py:106-107: the critic's values [b, ns, n, 1] on fresh coalitions."""
        pos = self.draw_coalitions("value", obs.size(0), obs.device)
        return self.shapley_values(obs, act, pos, want_q=True, frozen=critic_frozen)[1]

    marginal_contribution = value

    def get_loss(self, batch, need="both"):
        """sqddpg.py:131-158.  ``need`` = "value" (the value and target terms), "policy" (the policy term, critic frozen) or
        "both" (the reference's call: policy, value and target coalitions drawn in that order)."""
        state, actions, _, _, _, rewards, next_state, done, _, actions_avail, last_hids, hids = self.unpack_data(batch)
        b, dev = state.size(0), state.device
        policy_loss = value_loss = action_out = None
        if need in ("both", "policy"):
            _, actions_pol, _, action_out, _ = self.get_actions(state, status="train", exploration=False,
                                                                actions_avail=actions_avail, target=False,
                                                                last_hid=last_hids)
            pos = self.draw_coalitions("policy", b, dev)
            policy_loss = self.policy_term(self.shapley_values(state, actions_pol, pos, frozen=(need == "policy"))[0])
        if need in ("both", "value"):
            pos = self.draw_coalitions("value", b, dev)
            pos_next = self.draw_coalitions("target", b, dev)
            tgt = self.target_net if self.args.target else self
            with th.no_grad():
                # double_q: the next actions from the behaviour policy (sqddpg.py:136-139)
                next_actions = self.next_actions(next_state, actions_avail, hids)
                next_phi, _ = tgt.shapley_values(next_state, next_actions, pos_next)
                next_sum = next_phi.sum(dim=-1, keepdim=True)
            phi, _ = self.shapley_values(state, actions, pos)
            returns = rewards + self.args.gamma * (1 - done) * next_sum
            value_loss = mean_all((returns - phi.sum(dim=-1, keepdim=True)).pow(2))
        return policy_loss, value_loss, action_out


class _PPO:
    """madrl/learning_algorithms/ppo.py:7-10: what the reference's ``self.rl`` holds beside the loss — the BatchNorm of the
    advantages.  A plain object: the module stays outside the model's state_dict, as in the reference."""

    def __init__(self, args, device):
        self.args = args
        self.batchnorm = nn.BatchNorm1d(args.agent_num).to(device)


class IPPO(Model):
    """madrl/models/ippo.py:9-83 with the loss of madrl/learning_algorithms/ppo.py:14-69: the fixed-std RNN policy with the
    agent-summed action selection of IDDPG, independent state-value nets V_i(o_i) (plus the one-hot id), GAE on the values
    filed with the data, the clipped surrogate and the clipped value loss.  On the GPU the loss around the networks is
    csrc/ppo.hip (nets.ppo_gae / ppo_policy_loss / ppo_value_loss); elsewhere the tensor composition of the same formulas.

    ``gae_chain_stride``: row i of a batch continues into row i + stride.  1 is the reference's layout (a batch is one
    chain); the trainer sets it to the number of environments, whose pooled windows are whole vector steps, time-major.
    ``args.ppo_consistent_ratio`` (off by default, NOT the reference): the old log-probability is the loss's own
    log-density under the parameters that collected the data, instead of the action (model.py:313)."""

    on_policy = True
    graph_safe_updates = False       # sub-updates run eagerly
    unshared_critic_kernel = True
    gae_chain_stride = 1
    fused_ppo = True                 # (tests switch it off to compare with the tensor composition)
    get_actions = IDDPG.get_actions  # ippo.py:61-79 (continuous branch): the same function object
    FILE_ROWS = 131072               # rows per pass of begin_update_event

    def __init__(self, args, target_net=None):
        super().__init__(args)
        if not args.continuous:
            raise NotImplementedError("discrete control is outside the flexibility-provision hot path")
        self.build_nets(target_net)
        object.__setattr__(self, "rl", _PPO(self.args, self.device))
        self.consistent_ratio = bool(getattr(args, "ppo_consistent_ratio", False))
        self.last_terms = {}

    def construct_value_net(self):
        """ippo.py:19-28: a V(s), input obs + id."""
        self.build_value_dicts(self.obs_dim)

    def value(self, obs, act=None):
        """ippo.py:34-59: rows [o_i | onehot(i)] -> [b, n, 1]; ``act`` is ignored."""
        v = self.unshared_values(obs, None, False)
        if v is not None:
            return v
        return self.row_values(self.with_ids(obs), self.fused_inference)

    def _unfiled_columns(self, n_envs):
        """Real columns: begin_update_event files the values (and the consistent log-probability) into them."""
        z = th.zeros(n_envs, self.n_, 1, device=self.device)
        out = dict(value=z, next_value=z, log_prob_a=0.0)
        if self.consistent_ratio:
            out["log_prob_a"] = th.zeros(n_envs, self.n_, self.act_dim, device=self.device)
        return out

    # -- old values --------------------------------------------------------------------------------------------------
    def log_density(self, means, log_stds, actions):
        """ppo.py:19-28: log N(actions; agent-summed means, exp(agent-summed log-stds)) [b, n, a]."""
        from torch.distributions.normal import Normal
        if means.size(-1) > 1:
            means, log_stds = means.sum(dim=1, keepdim=True), log_stds.sum(dim=1, keepdim=True)
        return Normal(means, log_stds.exp(), validate_args=False).log_prob(actions)

    def begin_update_event(self, trainer):
        """Files ``value`` = V(s) and ``next_value`` = V(s') of every transition in the replay, in tall passes, before the
        first sub-update of an update event — for the vectorised rollouts, which do not value each step as model.py:218,226
        does.  Nothing has trained since the replay was last cleared, so these are the values the per-step route would have
        stored (tests/test_ppo_cpu.py).  With ``ppo_consistent_ratio`` the log-density column is filed the same way, on
        either route."""
        buf = trainer.replay_buffer
        vec = getattr(trainer.env, "n_envs", 1) > 1 or buf.slab_mode
        if not (vec or self.consistent_ratio):
            return
        if buf.slab_mode:
            buf.enable_filed_columns(log_prob=self.consistent_ratio)
        N = max(1, getattr(trainer.env, "n_envs", 1))
        chunk = max(N, self.FILE_ROWS // (N * self.n_) * N)
        with th.no_grad():
            for start, count in buf.contiguous_runs():
                for c in range(start, start + count, chunk):
                    m = min(chunk, start + count - c)
                    w = buf.window(c, m)
                    cols = {}
                    if vec:
                        cols["value"] = self.value(w.state, None).reshape(m, self.n_, 1)
                        cols["next_value"] = self.value(w.next_state, None).reshape(m, self.n_, 1)
                    if self.consistent_ratio:
                        means, log_stds, _ = self.policy(w.state, last_hid=w.last_hid)
                        lp = self.log_density(means, log_stds, w.action)
                        cols["log_prob_a"] = lp[:, :buf.field_rows("log_prob_a")]
                    buf.file_columns(c, m, **cols)

    # -- loss ----------------------------------------------------------------------------------------------------------
    def get_loss(self, batch, need="both"):
        """ppo.py:14-69 -> (policy_loss, value_loss, (means, log_stds)).  ``need`` = "value" / "policy" builds only that
        loss's graph; the reward and advantage BatchNorms move once per call whichever it is, as in the reference, which
        evaluates both losses every time."""
        args, n = self.args, self.n_
        batch = self._tensor_batch(batch)
        state, actions, _, old_values, old_next_values, rewards, next_state, done, last_step, actions_avail, last_hids, _ = \
            self.unpack_data(batch, normalise_reward=False)
        fused = bool(self.fused_ppo and self.fused_inference)
        reward_bn = self.batchnorm if args.reward_normalisation else None
        adv_bn = self.rl.batchnorm if args.normalize_advantages else None
        reward_norm, advantages, advantages_norm = ppo_gae(
            rewards, old_values, old_next_values, done, last_step, args.gamma, args.lambda_, self.gae_chain_stride,
            reward_bn, adv_bn, fused=fused)
        terms = dict(advantages=advantages, advantages_norm=advantages_norm, reward_norm=reward_norm)
        policy_loss = value_loss = action_out = None
        if need in ("both", "policy"):
            means, log_stds, _ = self.policy(state, last_hid=last_hids)
            action_out = (means, log_stds)
            old = batch.log_prob_a if self.consistent_ratio else None
            policy_loss, terms["ratios"] = ppo_policy_loss(means, log_stds, actions, old, advantages_norm, args.eps_clip,
                                                           actions_avail, fused=fused)
        if need in ("both", "value"):
            values = self.value(state, None).contiguous().view(-1, n)
            with th.no_grad():
                next_values = self.value(next_state, None).contiguous().view(-1, n)
            value_loss, terms["returns"] = ppo_value_loss(values, old_values, next_values, reward_norm, done, args.gamma,
                                                          args.eps_clip, args.value_loss_coef, fused=fused)
        self.last_terms = terms          # (tests and tools read the intermediates of the last call)
        return policy_loss, value_loss, action_out


class MAPPO(IPPO):
    """madrl/models/mappo.py:9-89: IPPO whose value nets see every agent's observation, V_i(o_1..o_n, onehot(i))."""

    def construct_value_net(self):
        """mappo.py:19-28"""
        self.build_value_dicts(self.obs_dim * self.n_)

    def value(self, obs, act=None):
        """mappo.py:34-62: rows [o_1 .. o_n | onehot(i)] -> [b, n, 1].  The n rows of a sample differ in the id column only,
        so the shared net's first layer is formed ONCE per sample and the id column added per agent — on the GPU by the
        critic's first-layer and tail kernels (as MADDPG.value on replayed actions)."""
        b, n, o = obs.size(0), self.n_, self.obs_dim
        obs_cols = obs.reshape(b, n * o)
        if self.args.shared_params:
            net = self.value_dicts[0]
            W, bias = net.fc1.weight, net.fc1.bias
            if obs.is_cuda and self.fused_inference and b * n >= WGRAD_MIN_ROWS:
                if th.is_grad_enabled() and W.requires_grad:
                    shared = wide_batch_linear(obs_cols, W[:, :n * o]) + bias
                else:
                    shared = th.addmm(bias, obs_cols, W[:, :n * o].t())
                if self.args.agent_id and critic_tail_supported(net, shared):
                    return CriticTail.apply_composed(shared, W[:, n * o:n * o + n].t(), net).view(b, n, 1)
                h = shared.unsqueeze(1).expand(b, n, -1)
                if self.args.agent_id:
                    h = h + W[:, n * o:n * o + n].t().unsqueeze(0)
                v, _ = net.forward_from_hidden(h.reshape(b * n, -1), need_hidden=False)
                return v.view(b, n, 1)
        v = self.unshared_values(obs, None, True)       # per-agent critics: the shared observation block, not n copies of it
        if v is not None:
            return v
        return self.row_values(self.with_ids(obs_cols.unsqueeze(1).expand(b, n, n * o)), False)


class COMA(Model):
    """madrl/models/coma.py:9-189 (continuous branch): a centralised critic Q_i on rows [o_1 .. o_n | o_i | onehot(i) |
    a_1 .. a_n] and the counterfactual baseline — for every sample and agent the mean of the critic over ``sample_size``
    draws of that agent's action from its own policy, everybody else's action kept.  The policy loss is
    -mean((Q - baseline).detach() log p) with the per-agent log-density, the value loss the one-step TD error against the
    target critic.  Action selection is IDDPG's agent-summed one (coma.py:104-124).  On-policy: the replay is cleared after
    every update event (model.py:56).

    On the GPU the first layer is assembled from fc1's column blocks (the all-observation and action blocks once per sample,
    the own-observation block per row, the id column per agent), the baseline is one launch of csrc/coma.hip on that
    pre-activation (nets.coma_baseline: nothing of [s b n, 889] is formed) and the policy loss another
    (nets.coma_policy_loss); elsewhere the reference's composition on materialised rows."""

    on_policy = True
    graph_safe_updates = False       # sub-updates run eagerly
    get_actions = IDDPG.get_actions  # coma.py:104-124 (continuous branch): the same function object
    sample_source = None             # tests: callable(means, std, s) -> the draws [s, b, n, a] of coma.py:141

    def __init__(self, args, target_net=None):
        super().__init__(args)
        if not args.continuous:
            raise NotImplementedError("discrete control is outside the flexibility-provision hot path")
        self.build_nets(target_net)
        # coma.py:17: ONE module for the reward normalisation of unpack_data and (normalize_advantages) the advantages
        self.batchnorm = nn.BatchNorm1d(self.args.agent_num).to(self.device)
        self.sample_size = int(args.sample_size)
        self.last_terms = {}

    def construct_value_net(self):
        """coma.py:19-35"""
        self.build_value_dicts((self.n_ + 1) * self.obs_dim + self.n_ * self.act_dim)

    def begin_update_event(self, trainer):
        """Nothing to file: COMA reads no stored value / log-probability column."""

    # -- critic --------------------------------------------------------------------------------------------------------
    def first_layer(self, obs, act):
        """fc1 of the shared critic on the rows of coma.py:41-78, [b n, hid], from fc1.weight's column blocks: the
        all-observation and action blocks once per sample, the own-observation block per row, the id column per agent — the
        same affine map up to fp32 summation order, without the [b n, 889] input."""
        b, n, o, a = obs.size(0), self.n_, self.obs_dim, self.act_dim
        net = self.value_dicts[0]
        W, bias = net.fc1.weight, net.fc1.bias
        c_act = (n + 1) * o + (n if self.args.agent_id else 0)
        obs_cols, act_cols = obs.reshape(b, n * o), act.detach().reshape(b, n * a)
        if not th.is_grad_enabled() or not W.requires_grad:
            with th.no_grad():
                shared = critic_first_layer(bias, obs_cols, act_cols, W, c_act)
        else:
            shared = wide_batch_linear(obs_cols, W[:, :n * o]) + wide_batch_linear(act_cols, W[:, c_act:c_act + n * a]) + bias
        z = shared.unsqueeze(1) + tall_linear(obs.reshape(b * n, o), W[:, n * o:(n + 1) * o]).view(b, n, -1)
        if self.args.agent_id:
            z = z + W[:, (n + 1) * o:(n + 1) * o + n].t().unsqueeze(0)
        return z.reshape(b * n, -1)

    def _composed(self, t):
        return bool(self.args.shared_params and t.is_cuda and t.dtype == th.float32 and self.fused_inference)

    def value(self, obs, act):
        """coma.py:41-102 (continuous branch): ``act`` [b, n, a] -> [b, n, 1]; the baseline's form, ``act`` [s b, n, n a]
        with row-specific actions -> [s b, n, 1] (the reference's view of the same values in the same order)."""
        per_row = obs.size(0) != act.size(0)
        b, n = obs.size(0), self.n_
        if not per_row and self._composed(obs) and b * n >= WGRAD_MIN_ROWS:
            v, _ = self.value_dicts[0].forward_from_hidden(self.first_layer(obs, act), need_hidden=False)
            return v.view(b, n, 1)
        return self.row_values(coma_rows(obs, act, self.args.agent_id, per_row), False)

    def draw_samples(self, means, std):
        """coma.py:139-141: ``sample_size`` draws of every agent's action from its own policy, [s, b, n, a]."""
        s = self.sample_size
        if self.sample_source is not None:
            return self.sample_source(means, std, s).to(means.device)
        return th.normal(means.unsqueeze(0).expand(s, *means.shape), std.unsqueeze(0).expand(s, *means.shape))

    def _fused(self, state):
        if not (state.is_cuda and self.fused_inference):
            return False
        ok = (self.args.shared_params and state.dtype == th.float32
              and coma_fused_config(self.value_dicts[0], self.n_, self.act_dim))
        if not ok:
            self.note_unfused("coma")
        return ok

    # -- loss ----------------------------------------------------------------------------------------------------------
    def get_loss(self, batch, need="both"):
        """coma.py:126-189 -> (policy_loss, value_loss, (means, log_stds)).  ``need`` = "value": the value loss alone (no
        draws, no baseline); "policy": the policy loss with the critic frozen; "both": the reference's call."""
        args, n = self.args, self.n_
        batch = self._tensor_batch(batch)
        state, actions, _, _, _, rewards, next_state, done, _, actions_avail, last_hids, hids = self.unpack_data(batch)
        fused = self._fused(state)
        net = self.value_dicts[0]
        terms = {}
        policy_loss = value_loss = action_out = None
        values = z1 = None
        if fused:
            with th.set_grad_enabled(th.is_grad_enabled() and need != "policy"):
                z1 = self.first_layer(state, actions)
        if need in ("both", "value"):
            if fused:
                values = net.forward_from_hidden(z1, need_hidden=False)[0].view(-1, n)
            else:
                values = self.value(state, actions).view(-1, n)
        if need in ("both", "policy"):
            means, log_stds, _ = self.policy(state, last_hid=last_hids)
            action_out = (means, log_stds)
            with th.no_grad():
                sampled = self.draw_samples(means.detach(), log_stds.detach().exp())
                if fused:
                    baselines, _, q = coma_baseline(net, z1.detach(), actions, sampled, want_values=values is None)
                    q = values.detach() if values is not None else q
                else:
                    nets = net if args.shared_params else self.value_dicts
                    baselines, _ = coma_baseline_torch(nets, state, actions, sampled, args.agent_id)
                    q = values.detach() if values is not None else self.value(state, actions).view(-1, n)
                advantages = None
                if args.normalize_advantages:
                    advantages = self.batchnorm(q - baselines)
            policy_loss, terms["log_prob_a"] = coma_policy_loss(means, log_stds, actions, actions_avail, q, baselines,
                                                                advantages, fused=fused)
            terms.update(sampled=sampled, baselines=baselines, values=q)
        if need in ("both", "value"):
            with th.no_grad():
                # double_q: the next actions from the behaviour policy (coma.py:133-136), valued by the target critic
                next_actions = self.next_actions(next_state, actions_avail, hids)
                tgt = self.target_net if args.target else self
                next_values = tgt.value(next_state, next_actions).view(-1, n)
            returns = rewards + args.gamma * (1 - done) * next_values
            assert returns.size() == values.size()
            value_loss = mean_all((returns - values).pow(2))
            terms.update(values=values.detach(), next_values=next_values, returns=returns)
        self.last_terms = terms          # (tests and tools read the intermediates of the last call)
        return policy_loss, value_loss, action_out


def _sum_last(x):
    """x.sum(dim=-1) over the (small) action axis as pointwise adds, like ``_sum_agents``: the same numbers up to fp32 summation
    order, and no ATen reduce_kernel in a captured rollout graph."""
    parts = x.unbind(-1)
    out = parts[0]
    for p in parts[1:]:
        out = out + p
    return out


class MAAC(Model):
    """madrl/models/maac.py:9-119 (continuous branch): soft actor-critic with ONE attention critic for all agents
    (nets.AttentionCritic, whatever ``shared_params`` says) and the Gaussian agents of ``agent_type``; ``gaussian_policy`` is
    forced, as alg_args/maac.yaml does.  Off-policy with transition replay, like MADDPG.

    The reference's quirks are kept: both action selections of ``get_loss`` explore, the next actions come from the TARGET
    policy, the agent-summed means and log-stds give ONE action and one log-density per sample that every agent shares
    (maac.py:70-80 — unlike IDDPG's the means are not masked), the TD target carries the ``soft`` / ``reward_scale`` entropy
    term, and the attention regulariser is added to the POLICY loss only — whose optimiser holds no critic parameter, so the
    regulariser never moves anything and is formed without a graph outside ``need="both"``.

    On the GPU the critic is csrc/attn_critic.hip through ``nets.attn_critic`` (eager calls only); elsewhere, and for
    ``need="both"`` — the reference's single call — the tensor composition."""

    graph_safe_updates = False       # sub-updates run eagerly
    noise_source = None              # tests: callable(role, shape) -> the standard-normal draw of "behaviour" / "target"

    def __init__(self, args, target_net=None):
        if not args.gaussian_policy:
            args = args._replace(gaussian_policy=True)
        super().__init__(args)
        if not args.continuous:
            raise NotImplementedError("discrete control is outside the flexibility-provision hot path")
        self.build_nets(target_net)
        self.batchnorm = nn.BatchNorm1d(self.args.agent_num).to(self.device)      # maac.py:16
        self.last_terms = {}

    def construct_value_net(self):
        """maac.py:38-39"""
        self.value_dicts = nn.ModuleList([AttentionCritic(self.args)])

    def update_target(self):
        """model.py:28-38; with norm_in the critic holds BatchNorm counters, which are copied."""
        if not self.args.norm_in:
            return super().update_target()
        with th.no_grad():
            for k in ("policy_dicts", "value_dicts"):
                src = getattr(self, k).state_dict()
                for name, t in getattr(self.target_net, k).state_dict().items():
                    if t.is_floating_point():
                        t.mul_(1 - self.args.target_lr).add_(src[name], alpha=self.args.target_lr)
                    else:
                        t.copy_(src[name])

    # -- critic ---------------------------------------------------------------------------------------------------------
    def critic(self, obs, act, critic_frozen=False, composed=False):
        """(q - b [b, n], regulariser [n]) of the attention critic.  ``critic_frozen``: the caller differentiates w.r.t. the
        actions only and the regulariser comes back detached; ``composed``: the tensor composition whatever the device."""
        net = self.value_dicts[0]
        if composed or not self.fused_inference:
            return net(obs, act)
        return attn_critic(net, obs, act, critic_frozen=critic_frozen)

    def value(self, obs, act, critic_frozen=False):
        """maac.py:45-64: [b + 1, n] — the values, and the regulariser as the last row."""
        q, reg = self.critic(obs, act, critic_frozen)
        return th.cat((q, reg.view(1, -1)), dim=0)

    # -- actions --------------------------------------------------------------------------------------------------------
    def _explore(self, means, log_stds, role):
        """util.py:56-64 on a recorded draw: Normal.rsample is loc + eps * scale."""
        from torch.distributions.normal import Normal
        std = log_stds.exp()
        eps = self.noise_source(role, tuple(means.shape)).to(means.device, means.dtype)
        x_t = means + eps * std
        y_t = th.tanh(x_t)
        return y_t, Normal(means, std, validate_args=False).log_prob(x_t) - th.log(1 - y_t.pow(2) + 1e-6)

    def get_actions(self, state, status, exploration, actions_avail, target=False, last_hid=None):
        """maac.py:66-90 (continuous branch): actions [b, 1, a], restored actions [b, n, a], log_prob_a [b, n]."""
        pol = self.target_net.policy if (target and self.args.target) else self.policy
        means, log_stds, hiddens = pol(state, last_hid=last_hid)
        if means.size(-1) > 1:
            means_, log_stds_ = _sum_agents(means), _sum_agents(log_stds)
        else:
            means_, log_stds_ = means, log_stds
        if (self.noise_source is not None and status == "train" and exploration and self.args.action_enforcebound):
            actions, log_prob_a = self._explore(means_, log_stds_, "target" if target else "behaviour")
        else:
            actions, log_prob_a = select_action(self.args, means_, status=status, exploration=exploration,
                                                info={"log_std": log_stds_})
        if getattr(actions_avail, "_flex_const", None) == 1.0 and actions.size(1) == 1:
            # every action available (env:721-730): the mask is 1
            restore_actions = expand_agents(actions, self.n_)
            if log_prob_a is not None:
                log_prob_a = _sum_last(log_prob_a).expand(-1, self.n_)
        else:
            restore_mask = 1.0 - (actions_avail.to(means.device) == 0).float()
            if log_prob_a is not None:
                log_prob_a = _sum_last(restore_mask * log_prob_a)
            restore_actions = restore_mask * actions
        return actions, restore_actions, log_prob_a, (means, log_stds), hiddens

    # -- loss -----------------------------------------------------------------------------------------------------------
    def get_loss(self, batch, need="both"):
        """maac.py:92-119 -> (policy_loss, value_loss, (means, log_stds)).  ``need`` = "value": the value loss alone — the
        behaviour policy's draw still enters the TD target through its log-density, without a graph: only the value
        optimiser's parameters take this loss's gradient; "policy": the policy loss with the critic frozen and the regulariser
        from a pass without a graph; "both": the reference's call, one graph through everything, on the composition."""
        args, n = self.args, self.n_
        batch = self._tensor_batch(batch)
        state, actions, _, _, _, rewards, next_state, done, _, actions_avail, last_hids, hids = self.unpack_data(batch)
        both = need == "both"
        tgt = self.target_net if args.target else self
        terms = {}
        policy_loss = value_loss = action_out = None
        with th.set_grad_enabled(th.is_grad_enabled() and need != "value"):
            _, actions_pol, log_prob_a, action_out, _ = self.get_actions(
                state, status="train", exploration=True, actions_avail=actions_avail, target=False, last_hid=last_hids)
        terms["log_prob_a"] = log_prob_a.detach()
        if need in ("both", "value"):
            with th.no_grad():
                _, next_actions, _, _, _ = self.get_actions(next_state, status="train", exploration=True,
                                                            actions_avail=actions_avail, target=True, last_hid=hids)
                next_values = tgt.critic(next_state, next_actions, composed=both)[0]
        if both:
            values, attn_reg = self.critic(state, actions.detach(), composed=True)
        elif need == "value":
            values, attn_reg = self.critic(state, actions.detach())
        else:
            with th.no_grad():
                attn_reg = self.critic(state, actions.detach())[1]
        terms["attn_reg"] = attn_reg.detach()
        if need in ("both", "policy"):
            advantages = self.critic(state, actions_pol, critic_frozen=not both, composed=both)[0]
            if args.normalize_advantages:
                advantages = self.batchnorm(advantages)
            if args.soft:
                policy_loss = log_prob_a / args.reward_scale - advantages
            else:
                policy_loss = -advantages.detach() * log_prob_a
            policy_loss = mean_all(policy_loss + attn_reg)
        if need in ("both", "value"):
            assert values.size() == next_values.size() == log_prob_a.size()
            returns = rewards + args.gamma * (1 - done) * next_values.detach() - args.soft * log_prob_a / args.reward_scale
            value_loss = mean_all((returns - values).pow(2))
            terms.update(values=values.detach(), next_values=next_values, returns=returns.detach())
        self.last_terms = terms          # (tests and tools read the intermediates of the last call)
        return policy_loss, value_loss, (action_out if need != "value" else None)
