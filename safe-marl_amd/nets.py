"""Actor and critic networks of the MADDPG path, same parameter names and shapes as the reference so
state_dicts interchange (actor 34 948 params, critic 52 097 params at the default config).
Training (autograd) runs through PyTorch-ROCm; the actor's INFERENCE pass — every rollout step and every
bootstrap target — is one fused HIP launch (csrc/actor.hip, include/flexnet.h) through ``fused_actor_forward``."""
from __future__ import annotations

import ctypes as C
import math
import os
import torch as th
import torch.nn as nn
import torch.nn.functional as F

from . import _lib
from .util import in_graph_audit, note_fallback


def _find_fused_gru():
    """ATen's pointwise GRU cell, what nn.GRUCell dispatches to on the GPU after its two gate GEMMs (ATen RNN.cpp)."""
    try:
        return th.ops.aten._thnn_fused_gru_cell.default
    except (AttributeError, RuntimeError):
        return None


_FUSED_GRU = _find_fused_gru()


def _gru_cell(x, hx, rnn):
    """nn.GRUCell as ATen composes it on the GPU, for update batches: the biases ride the gate GEMMs (their gradients
    are then column sums taken inside csrc/wgrad.hip's pass over the gate gradients) instead of entering the pointwise
    cell, whose backward would reduce them with two more passes over [rows, 192]."""
    gi = tall_linear(x, rnn.weight_ih, rnn.bias_ih)
    gh = tall_linear(hx, rnn.weight_hh, rnn.bias_hh)
    return _FUSED_GRU(gi, gh, hx, None, None)[0]


def _activation(name):
    if name == "relu":
        return F.relu
    if name == "tanh":
        return th.tanh
    raise ValueError(name)


class RNNAgent(nn.Module):
    """madrl/agents/rnn_agent.py:13-33: fc1 -> LayerNorm -> act -> GRUCell -> fc2; forward returns
    (action mean, None, new hidden)."""

    def __init__(self, input_shape, args):
        super().__init__()
        self.args = args
        self.fc1 = nn.Linear(input_shape, args.hid_size)
        if args.layernorm:
            self.layernorm = nn.LayerNorm(args.hid_size)
        self.rnn = nn.GRUCell(args.hid_size, args.hid_size)
        self._build_heads(args)
        self._act = _activation(args.hid_activation)

    def _build_heads(self, args):
        """What follows the GRU cell (RNNAgentGaussian: ``mean`` and ``log_std``; ``fc2`` is then a property over ``mean`` —
        an ``self.fc2 = ...`` in __init__ would collide with it)."""
        self.fc2 = nn.Linear(args.hid_size, args.action_dim)

    def init_hidden(self):
        return self.fc1.weight.new_zeros(1, self.args.agent_num, self.args.hid_size)

    def forward(self, inputs, hidden_state):
        if th.is_grad_enabled() and inputs.is_cuda and not inputs.requires_grad and inputs.dim() == 2:
            x = wide_batch_linear(inputs, self.fc1.weight) + self.fc1.bias     # split-K weight gradient at update batches
        else:
            x = self.fc1(inputs)
        if self.args.layernorm:
            x = self.layernorm(x)
        x, hx = self._act(x), hidden_state.reshape(-1, self.args.hid_size)
        if (th.is_grad_enabled() and x.is_cuda and x.dim() == 2 and x.shape[0] >= WGRAD_MIN_ROWS
                and x.dtype == th.float32 and _FUSED_GRU is not None):
            # update batches (163 840 rows): the GRUCell as PyTorch composes it on the GPU — two gate GEMMs and the
            # fused pointwise cell — with the three weight gradients (W_ih, W_hh, fc2) from csrc/wgrad.hip
            r = self.rnn
            h = _gru_cell(x, hx, r)
            return tall_linear(h, self.fc2.weight, self.fc2.bias), None, h
        h = self.rnn(x, hx)
        return self.fc2(h), None, h

    def forward_update(self, obs, hidden_state, n_agents, agent_id):
        """The same forward for an update batch on the GPU, from observations WITHOUT the one-hot id columns: row r is
        agent r % n_agents (model.py:110-112), fc1's id block enters as a per-agent addend.  Returns None when the
        configuration is outside what csrc/lnrelu.hip covers (the caller concatenates the ids and calls forward)."""
        o = obs.shape[1]
        W = self.fc1.weight
        hx0 = hidden_state.reshape(-1, self.args.hid_size)
        if actor_train_supported(self, obs, n_agents, agent_id) and not hx0.requires_grad and hx0.dtype == th.float32:
            # one autograd node: fused matrix-core forward, hand-written backward (csrc/actor.hip, gru.hip, wgrad.hip, lnrelu.hip)
            ln = self.layernorm if self.args.layernorm else None
            r = self.rnn
            means, h = self._train_node().apply(obs, hx0, n_agents, bool(agent_id), W, self.fc1.bias,
                                                None if ln is None else ln.weight, None if ln is None else ln.bias,
                                                _ln_eps(self), r.weight_ih, r.weight_hh, r.bias_ih, r.bias_hh,
                                                self.fc2.weight, self.fc2.bias)
            return means, None, h
        if not (obs.is_cuda and obs.dtype == th.float32 and lnrelu_supported(self, n_agents) and _FUSED_GRU is not None
                and W.shape[1] == o + (n_agents if agent_id else 0) and obs.shape[0] % n_agents == 0):
            if obs.is_cuda:
                note_fallback("actor_update_pass", f"hid {self.args.hid_size}, act {self.args.hid_activation}, agents "
                                                   f"{n_agents}, dtype {obs.dtype}")
            return None
        z = wide_batch_linear(obs, W[:, :o]) if not obs.requires_grad else tall_linear(obs, W[:, :o])
        ln = self.layernorm if self.args.layernorm else None
        x = _LnReluFn.apply(z, self.fc1.bias, W[:, o:].t() if agent_id else None, None if ln is None else ln.weight,
                            None if ln is None else ln.bias, _ln_eps(self), n_agents)
        r, hx = self.rnn, hidden_state.reshape(-1, self.args.hid_size)
        h = _gru_cell(x, hx, r)
        return tall_linear(h, self.fc2.weight, self.fc2.bias), None, h

    def _train_node(self):
        """The autograd node of the fused update pass (the Gaussian agent's also takes a gradient at the hidden state)."""
        return _ActorTrainFn


class MLPAgent(nn.Module):
    """madrl/agents/mlp_agent.py:5-32 (agent_type: mlp): fc1 -> LayerNorm -> act -> fc2 -> act -> fc3; forward returns
    (action mean, None, h).  This ``forward`` is the tensor composition; on the GPU under ``shared_params`` ``Model.policy``
    takes csrc/actor_mlp.hip instead (``fused_actor_forward_mlp`` / ``actor_mlp_train``) wherever no HIP graph is being
    captured, and under ``shared_params: False`` csrc/actor_mlp.hip's per-agent form over all the agents' modules
    (``fused_actor_forward_mlp_unshared`` / ``actor_mlp_unshared_train``).  ``fused_inference`` / ``fused_training`` (read with getattr, default True): the two switches of those paths."""

    def __init__(self, input_shape, args):
        super().__init__()
        self.args = args
        self.fc1 = nn.Linear(input_shape, args.hid_size)
        if args.layernorm:
            self.layernorm = nn.LayerNorm(args.hid_size)
        self.fc2 = nn.Linear(args.hid_size, args.hid_size)
        self._build_heads(args)
        self._act = _activation(args.hid_activation)

    def _build_heads(self, args):
        """What follows fc2 (MLPAgentGaussian: ``mean`` and ``log_std``; ``fc3`` is then a property over ``mean``)."""
        self.fc3 = nn.Linear(args.hid_size, args.action_dim)

    def init_hidden(self):
        return self.fc1.weight.new_zeros(1, self.args.hid_size)

    def forward(self, inputs, hidden_state):
        x = self.fc1(inputs)
        if self.args.layernorm:
            x = self.layernorm(x)
        h = self._act(self.fc2(self._act(x)))
        return self.fc3(h), None, h


def gauss_log_std_torch(h, weight, bias, lo, hi):
    """rnn_agent_gaussian.py:37-39: lo + 0.5 (hi - lo) (tanh(h W^T + b) + 1), the tensor composition."""
    return lo + 0.5 * (hi - lo) * (th.tanh(F.linear(h, weight, bias)) + 1)


def _gauss_head_fill(a, rows, weight, lo, hi):
    """The fields FlexGaussHeadArgs and FlexGaussHeadUnsharedArgs share (``weight``: the head's, or any agent's)."""
    a.rows, a.act_dim, a.hid = rows, weight.shape[0], weight.shape[1]
    a.log_std_min, a.log_std_max = float(lo), float(hi)
    return a


def _gauss_head_args(h, weight, lo, hi):
    a = _gauss_head_fill(_lib.FlexGaussHeadArgs(), h.shape[0], weight, lo, hi)
    a.w = weight.data_ptr()
    return a


def _gauss_head_backward_launch(entry, a, d_log_std, t, want_d_h):
    """(d_u [rows, a], d_h [rows, 64] or None) from either form's backward entry point on its filled struct ``a``."""
    d_log_std = d_log_std.contiguous()
    d_u = th.empty_like(t)
    d_h = th.empty(t.shape[0], a.hid, dtype=th.float32, device=t.device) if want_d_h else None
    a.d_log_std, a.t, a.d_u = d_log_std.data_ptr(), t.data_ptr(), d_u.data_ptr()
    if d_h is not None:
        a.d_h = d_h.data_ptr()
    _lib.launch(entry, a)
    return d_u, d_h


def gauss_head_supported(h, weight, bias=None):
    """What csrc/gauss.hip covers: fp32 GPU rows of 64 hidden units, at most FLEXNET_MAX_ACT outputs."""
    return (h.is_cuda and h.dim() == 2 and all(t is None or (t.is_cuda and t.dtype == th.float32) for t in (h, weight, bias))
            and h.shape[1] == weight.shape[1] and h.is_contiguous() and h.data_ptr() % 16 == 0)


def gauss_head_forward(h, weight, bias, lo, hi, means=None, noise=None, low=0.0, high=1.0, want_t=True):
    """One launch of flexnet_gauss_head_forward, no graph: (log_std [rows, a], t = tanh(u) or None) and, with ``means`` and
    ``noise`` [rows, a], also (action = tanh(means + exp(log_std) noise), env_action) — the per-agent exploration of
    maddpg.py:88 under util.py:56-64 with translate_action (util.py:125-128).  None where the library declines.
    (The epilogue is an entry of the library for callers that hold the noise; the learner's own paths draw in tensor
    operations next to torch's generator, so today only the tests call it.)"""
    if (means is None) != (noise is None):
        raise ValueError("gauss_head_forward: the exploration epilogue needs both `means` and `noise`")
    h, weight = h.detach().contiguous(), weight.detach().contiguous()
    rows, na = h.shape[0], weight.shape[0]
    log_std = th.empty(rows, na, dtype=th.float32, device=h.device)
    t = th.empty_like(log_std) if want_t else None
    a = _gauss_head_args(h, weight, lo, hi)
    a.h, a.log_std = h.data_ptr(), log_std.data_ptr()
    keep = [h, weight]
    if bias is not None:
        keep.append(bias.detach().contiguous())
        a.b = keep[-1].data_ptr()
    if t is not None:
        a.t = t.data_ptr()
    action = env_action = None
    if noise is not None:
        keep += [means.detach().reshape(rows, na).to(th.float32).contiguous(), noise.reshape(rows, na).to(th.float32).contiguous()]
        action, env_action = th.empty_like(log_std), th.empty_like(log_std)
        a.means, a.noise, a.action, a.env_action = keep[-2].data_ptr(), keep[-1].data_ptr(), action.data_ptr(), env_action.data_ptr()
        a.action_low, a.action_high = float(low), float(high)
    if not _lib.try_launch("flexnet_gauss_head_forward", a):
        return None
    return (log_std, t, action, env_action) if noise is not None else (log_std, t)


def gauss_head_backward(d_log_std, t, weight, lo, hi, want_d_h=True):
    """One launch of flexnet_gauss_head_backward: (d_u [rows, a], d_h [rows, 64] or None)."""
    weight = weight.detach().contiguous()
    return _gauss_head_backward_launch("flexnet_gauss_head_backward", _gauss_head_args(t, weight, lo, hi), d_log_std, t, want_d_h)


class _GaussHeadFn(th.autograd.Function):
    """The log-std head of the Gaussian agents as one node: csrc/gauss.hip both ways, the weight and bias gradients from one
    pass of csrc/wgrad.hip over d_u."""

    @staticmethod
    def forward(ctx, h, weight, bias, lo, hi):
        out = gauss_head_forward(h, weight, bias, lo, hi, want_t=any(ctx.needs_input_grad[:3]))
        if out is None:
            raise _lib.FlexLibraryError("flexnet_gauss_head_forward declined a configuration gauss_log_std admitted")
        log_std, t = out
        if t is not None:
            ctx.save_for_backward(h, weight, t)
        ctx.lo, ctx.hi, ctx.has_bias = float(lo), float(hi), bias is not None
        return log_std

    @staticmethod
    def backward(ctx, d_log_std):
        h, weight, t = ctx.saved_tensors
        d_u, d_h = gauss_head_backward(d_log_std, t, weight, ctx.lo, ctx.hi, want_d_h=ctx.needs_input_grad[0])
        dw = db = None
        want_db = ctx.has_bias and ctx.needs_input_grad[2]
        if ctx.needs_input_grad[1]:
            hd = h.detach()
            if tall_wgrad_supported(d_u, hd):
                if want_db:
                    db = th.empty(d_u.shape[1], dtype=th.float32, device=d_u.device)
                dw = tall_wgrad(d_u, hd, colsum=db)
            else:
                dw = d_u.t() @ hd
        if want_db and db is None:
            db = d_u.sum(0)
        return d_h, dw, db, None, None


def gauss_log_std(h, weight, bias, lo, hi):
    """log_std [rows, a] of the Gaussian agents' head on ``h`` [rows, hid]: csrc/gauss.hip on the GPU (hid 64, a <= 8, fp32),
    the tensor composition elsewhere."""
    if gauss_head_supported(h, weight, bias):
        if weight.shape[1] == _lib.FLEXNET_HID and weight.shape[0] <= _lib.FLEXNET_MAX_ACT and h.shape[0] >= 1:
            return _GaussHeadFn.apply(h, weight, bias, lo, hi)
        note_fallback("gauss_head", f"hid {weight.shape[1]}, act_dim {weight.shape[0]}")
    elif h.is_cuda:
        note_fallback("gauss_head", f"dtype {h.dtype}, shape {tuple(h.shape)}")
    return gauss_log_std_torch(h, weight, bias, lo, hi)


class RNNAgentGaussian(RNNAgent):
    """madrl/agents/rnn_agent_gaussian.py:7-40: the RNN agent with the heads ``mean`` and ``log_std`` in place of ``fc2``;
    forward returns (mean, log_std, new hidden) with log_std = MIN + 0.5 (MAX - MIN) (tanh(log_std(h)) + 1).  The ``mean``
    head sits where the fixed-std agent has ``fc2``, so the fused actor kernels serve it unchanged; the log-std head is
    csrc/gauss.hip on the hidden state they return."""

    def _build_heads(self, args):
        self.mean = nn.Linear(args.hid_size, args.action_dim)
        self.log_std = nn.Linear(args.hid_size, args.action_dim)

    @property
    def fc2(self):
        # a CLASS property: found before nn.Module.__getattr__ looks among the registered submodules, so the kernels' wrappers
        # read agent.fc2.weight / .bias as the mean head's, and no "fc2.*" key enters the state_dict
        return self.mean

    def log_std_of(self, h):
        return gauss_log_std(h, self.log_std.weight, self.log_std.bias, self.args.LOG_STD_MIN, self.args.LOG_STD_MAX)

    def forward(self, inputs, hidden_state):
        mean, _, h = super().forward(inputs, hidden_state)
        return mean, self.log_std_of(h), h

    def forward_update(self, obs, hidden_state, n_agents, agent_id):
        out = super().forward_update(obs, hidden_state, n_agents, agent_id)
        if out is None:
            return None
        return out[0], self.log_std_of(out[2]), out[2]

    def _train_node(self):
        return _ActorTrainHidFn


class MLPAgentGaussian(MLPAgent):
    """madrl/agents/mlp_agent_gaussian.py:7-41 (agent_type: mlp): the MLP agent with the heads ``mean`` and ``log_std`` in
    place of ``fc3``; forward returns (mean, log_std, h).  The ``mean`` head sits where the fixed-std agent has ``fc3``, so
    csrc/actor_mlp.hip serves it unchanged; on that path the log-std head is csrc/gauss.hip on the ``h`` it returns."""

    def _build_heads(self, args):
        self.mean = nn.Linear(args.hid_size, args.action_dim)
        self.log_std = nn.Linear(args.hid_size, args.action_dim)

    @property
    def fc3(self):
        # a CLASS property (as RNNAgentGaussian.fc2): the base class reads self.fc3 as the mean head, and no "fc3.*" key
        # enters the state_dict
        return self.mean

    def log_std_of(self, h):
        return gauss_log_std(h, self.log_std.weight, self.log_std.bias, self.args.LOG_STD_MIN, self.args.LOG_STD_MAX)

    def forward(self, inputs, hidden_state):
        mean, _, h = super().forward(inputs, hidden_state)
        log_std = gauss_log_std_torch(h, self.log_std.weight, self.log_std.bias, self.args.LOG_STD_MIN, self.args.LOG_STD_MAX)
        return mean, log_std, h


class MLPCritic(nn.Module):
    """madrl/critics/mlp_critic.py:5-34: fc1 -> LayerNorm -> act -> fc2 -> act -> fc3; returns (v, h).

    ``forward_from_hidden`` takes the pre-LayerNorm first-layer activation directly: the centralised
    critic's input repeats every agent's observation n times (maddpg.py:38-39), so the caller forms
    fc1's output from its column blocks once per sample instead of n times (learner.MADDPG.value)."""

    def __init__(self, input_shape, output_shape, args):
        super().__init__()
        self.args = args
        self.fc1 = nn.Linear(input_shape, args.hid_size)
        if args.layernorm:
            self.layernorm = nn.LayerNorm(args.hid_size)
        self.fc2 = nn.Linear(args.hid_size, args.hid_size)
        self.fc3 = nn.Linear(args.hid_size, output_shape)
        self._act = _activation(args.hid_activation)

    def init_hidden(self):
        return self.fc1.weight.new_zeros(1, self.args.hid_size)

    def forward_from_hidden(self, x, need_hidden=True):
        """``need_hidden=False`` (the MADDPG losses only use v): on the GPU the whole tail — LayerNorm, ReLU, fc2, ReLU,
        fc3 and, when a graph is recorded, their backward — is two HIP launches (csrc/critic.hip)."""
        if not need_hidden and critic_tail_supported(self, x):
            return CriticTail.apply(x, self), None
        if self.args.layernorm:
            x = self.layernorm(x)
        h = self._act(self.fc2(self._act(x)))
        return self.fc3(h), h

    def forward(self, inputs, hidden_state):
        return self.forward_from_hidden(self.fc1(inputs))


# FlexActorArgs.variant when the caller names none (include/flexnet.h: 0 = the library's choice by size; tests pin 2 / 3)
ACTOR_VARIANT = 0


def fused_actor_forward(agent, obs, hidden, n_agents, agent_id, noise=None, std=1.0, low=0.0, high=1.0, variant=None,
                        rng_state=None, ring_cursor=None, obs_slab_stride=0, hid_slab_stride=0, cursor_out=None,
                        out=None, ring_slabs=0, launch=None, obs_source=None):
    """rnn_agent.py:25-33 + model.py:102-116 without an autograd graph, in one HIP launch.

    ``obs`` [b, n, obs_dim] fp32 on the GPU WITHOUT the one-hot id columns (the kernel adds fc1's id column of
    row r % n itself), ``hidden`` [b, n, 64] or [b * n, 64].  Returns (means [b * n, act], hidden [b * n, 64]) or
    None when the configuration is not one the kernel covers (the caller then uses the module).  With ``noise``
    [b, n, act] (standard normal draws) the exploration epilogue runs in the same launch and two more tensors come
    back: action = tanh(mean + std * noise) (util.py:57-64) and the environment's action (util.py:125-128).  With
    ``rng_state`` (int64 device tensor [seed, step]) instead of ``noise`` the kernel draws the normal numbers itself
    (Philox4x32-10 + Box-Muller, csrc/actor.hip actor_noise4); the caller advances ``rng_state[1]`` per call —
    flexnet_rollout_pack does when handed the same tensor.  With ``ring_cursor`` (int64 device tensor) ``obs`` and ``hidden``
    are slab 0 of two slab rings and the launch reads slab ``ring_cursor[0]`` of each (strides in floats), resolved on the
    device — the rollout graph's way of reading the observation where the environment kernel wrote it.
    ``launch`` (with ``ring_slabs``): called with the filled FlexActorArgs INSTEAD of flexnet_actor_forward — the rollout
    burst, which runs this policy evaluation inside the environment's persistent launch (flex_env.rollout_burst).
    ``obs_source`` (a ``_lib.FlexObsSource``, VecFlexProvisionEnv.obs_source()): the observations are read IN PLACE from
    the environment's history (``obs`` then only gives the shape [b, n, obs_dim]; it is not read)."""
    a = agent.args
    if not (isinstance(agent, RNNAgent) and a.hid_size == 64 and a.hid_activation == "relu" and obs.is_cuda
            and obs.dtype == th.float32 and obs.shape[-1] <= 144 and n_agents <= 8 and a.action_dim <= 8):
        if obs.is_cuda:
            note_fallback("actor_forward", f"{type(agent).__name__}, hid {a.hid_size}, act {a.hid_activation}, obs "
                                           f"{obs.shape[-1]}, agents {n_agents}, dtype {obs.dtype}")
        return None
    rows = obs.shape[0] * obs.shape[1]
    obs_dim = obs.shape[-1]
    obs = obs.contiguous()
    rv = ring_view_of(obs)
    if rv is not None:
        # a placeholder of the replay's stacked-observation ring (RING_VIEWS): the observations are read in place — the ring's
        # base plus, through the kernel's cursor mechanism, the window's first row from the device cell
        if ring_cursor is not None or obs_source is not None or rv[0].shape[1] != obs.shape[1] * obs.shape[2]:
            raise RuntimeError("fused_actor_forward: an in-place window of the stacked-observation ring cannot be combined with a ring cursor")
        ring_cursor, obs_slab_stride, hid_slab_stride, cursor_out = rv[1], rv[0].shape[1], 0, None
        obs = rv[0]
    hidden = hidden.reshape(rows, 64).to(th.float32).contiguous()
    rvh = ring_view_of(hidden)
    if rvh is not None:
        # the hidden states of the same window, in place from the replay's hidden-state ring (same cell: same ring geometry)
        if rv is None or rvh[1] is not rv[1] or rvh[0].shape[1] != n_agents * 64:
            raise RuntimeError("fused_actor_forward: hidden states are read in place only together with the observations of the same window")
        hid_slab_stride = rvh[0].shape[1]
        hidden = rvh[0]
    means = (out or {}).get("means")
    if means is None:
        means = th.empty(rows, a.action_dim, dtype=th.float32, device=obs.device)
    hid_out = (out or {}).get("hidden_out")
    if hid_out is None:
        hid_out = th.empty(rows, 64, dtype=th.float32, device=obs.device)
    args = _lib.FlexActorArgs()
    args.rows, args.n_agents, args.obs_dim, args.act_dim = rows, n_agents, obs_dim, a.action_dim
    args.agent_id, args.layernorm, args.ln_eps = int(bool(agent_id)), int(bool(a.layernorm)), _ln_eps(agent)
    args.variant = int(ACTOR_VARIANT if variant is None else variant)
    action = env_action = None
    explore = noise is not None or rng_state is not None
    if noise is not None:
        noise = noise.reshape(rows, a.action_dim).to(th.float32).contiguous()
    elif rng_state is not None:
        if not (rng_state.is_cuda and rng_state.dtype == th.int64 and rng_state.numel() == 2 and rng_state.is_contiguous()):
            raise ValueError("rng_state must be a contiguous int64 device tensor [seed, step]")
        args.rng_state = rng_state.data_ptr()
    if ring_cursor is not None:
        args.cursor, args.obs_slab_stride, args.hid_slab_stride = ring_cursor.data_ptr(), int(obs_slab_stride), int(hid_slab_stride)
        if cursor_out is not None:
            args.cursor_out = cursor_out.data_ptr()
    if explore:
        action, env_action = (out or {}).get("action"), (out or {}).get("env_action")
        if env_action is None:
            env_action = th.empty_like(means)
        if action is None:
            action = th.empty_like(means)
        args.std, args.action_low, args.action_high = float(std), float(low), float(high)
    ln = agent.layernorm if a.layernorm else None
    for name, t in (("obs", obs), ("hidden_in", hidden), ("fc1_w", agent.fc1.weight), ("fc1_b", agent.fc1.bias),
                    ("ln_w", ln.weight if ln is not None else None), ("ln_b", ln.bias if ln is not None else None),
                    ("w_ih", agent.rnn.weight_ih), ("w_hh", agent.rnn.weight_hh), ("b_ih", agent.rnn.bias_ih),
                    ("b_hh", agent.rnn.bias_hh), ("fc2_w", agent.fc2.weight), ("fc2_b", agent.fc2.bias),
                    ("means", means), ("hidden_out", hid_out), ("noise", noise), ("action", action),
                    ("env_action", env_action)):
        if t is not None and not t.is_contiguous():
            note_fallback("actor_forward", f"non-contiguous {name}")
            return None
        setattr(args, name, None if t is None else t.data_ptr())
    args.ring_slabs = int(ring_slabs)
    if obs_source is not None:
        args.obs, args.obs_pushed = obs_source.ring, obs_source.pushed
        args.obs_row_stride, args.obs_pushed_stride = obs_source.row_stride, obs_source.pushed_stride
        args.obs_slots, args.obs_slot_w = obs_source.slots, obs_source.slot_w
    if launch is not None:
        launch(args)
        return (means, hid_out, action, env_action) if explore else (means, hid_out)
    if not _lib.try_launch("flexnet_actor_forward", args):
        note_fallback("actor_forward", "FLEXNET_EUNSUPPORTED from flexnet_actor_forward")
        return None
    return (means, hid_out, action, env_action) if explore else (means, hid_out)


# ---- plumbing that every fused family below shares ------------------------------------------------------------------------------
_SCRATCH = {}


def _scratch(name, device, numel, dtype=th.float32):
    """The per-device scratch of one kernel family: ``numel`` elements of ``dtype``, allocated once per (name, device) and kept
    (it never shrinks).  Calls of one family are expected on one stream at a time (the update's); a family whose calls may
    run on several streams puts the stream into its ``name``."""
    key = (name, device)
    if key not in _SCRATCH:
        _SCRATCH[key] = th.empty(numel, dtype=dtype, device=device)
    return _SCRATCH[key]


def _ln_eps(module):
    """LayerNorm's eps of an agent or critic module (without LayerNorm the library's default: no kernel reads it then)."""
    return float(module.layernorm.eps) if module.args.layernorm else 1e-5


NOT_FP32_DEVICE = "a parameter is not a contiguous fp32 device tensor"


def _params_decline(params):
    """``NOT_FP32_DEVICE`` unless every parameter the kernels read through a raw pointer is a contiguous fp32 device tensor
    (None, an absent LayerNorm pair, passes), else None."""
    for p in params:
        if p is not None and not (p.is_cuda and p.dtype == th.float32 and p.is_contiguous()):
            return NOT_FP32_DEVICE
    return None


def _fill_tables(a, names, params, n):
    """Writes ``params[i][k]`` of agent i < n into entry i of the pointer table ``names[k]`` of the ctypes struct ``a`` (None:
    a null pointer); a table the struct does not have is skipped, so one list of names serves a family's forward and backward
    structs."""
    for k, name in enumerate(names):
        table = getattr(a, name, None)
        if table is not None:
            for i in range(n):
                p = params[i][k]
                table[i] = None if p is None else p.data_ptr()


def _regroup_params(saved, n, width, has_ln, ln_slots=(2, 3)):
    """Per-agent parameter lists of ``width`` entries from ``saved``, the flat run of n agents' parameters that a node gave
    ``save_for_backward`` without its None entries: without LayerNorm the ``ln_slots`` of every agent come back as None."""
    absent = () if has_ln else ln_slots
    per = width - len(absent)
    out = []
    for i in range(n):
        it = iter(saved[per * i:per * (i + 1)])
        out.append([None if k in absent else next(it) for k in range(width)])
    return out


def _fused_inference(key, why, on_gpu, entry, launch):
    """The protocol of every ``fused_*_forward*`` below.  ``why``: the reason its kernel does not cover the call, or None;
    a decline is noted under ``key`` on GPU tensors only (on the CPU the caller's composition is simply what runs).  Else
    ``launch()`` under no_grad, whose None — the library answered FLEXNET_EUNSUPPORTED from ``entry`` — is noted too.  Returns
    the launch's result, or None for "run the composition"."""
    if why is not None:
        if on_gpu:
            note_fallback(key, why)
        return None
    with th.no_grad():
        out = launch()
    if out is None:
        note_fallback(key, f"FLEXNET_EUNSUPPORTED from {entry}")
    return out


WGRAD_MIN_ROWS = 2048         # below this the library GEMM is launch-bound either way


# the finish of the fused value loss rides in the first-layer weight gradient's second-stage launch (FLEX_WGRAD_FINISH_RIDER=0:
# two launches, the A/B switch)
WGRAD_FINISH_RIDER = os.environ.get("FLEX_WGRAD_FINISH_RIDER", "1") != "0"


def tall_wgrad_supported(dy, x):
    return (dy.is_cuda and x.is_cuda and dy.dtype == th.float32 and x.dtype == th.float32 and dy.dim() == 2
            and x.dim() == 2 and dy.shape[0] == x.shape[0] and 1 <= dy.shape[1] <= 192 and x.shape[1] >= 1
            and (dy.shape[0] <= 1 or (dy.stride(1) == 1 and x.stride(1) == 1 and dy.stride(0) >= dy.shape[1]
                                      and x.stride(0) >= x.shape[1] and max(dy.stride(0), x.stride(0)) < (1 << 24))))


def tall_wgrad(dy, x, out=None, accumulate=False, colsum=None, x2=None, out2=None, critic_finish=None):
    """dW[m, n] = sum_k dy[k, m] * x[k, n] (csrc/wgrad.hip: include/flexnet.h flexnet_wgrad) — the weight gradient of
    y = x @ W.T over a tall batch.  Row-strided views (column slices of the packed replay rows) are read in place.
    The workspace is per device: calls are expected on one stream at a time (the update's).
    ``x2`` / ``out2``: a second input block of the same layer (out2 = dy.T @ x2) — in the same launch where the kernel
    takes [x | x2] as one operand (64 output rows, x wider than 64 columns and a multiple of 5), else a second call.
    ``critic_finish`` = (FlexCriticTailArgs, FlexTdLossArgs): phase 2 of flexnet_critic_td_backward_phases rides in this
    call's second-stage launch (flexnet_wgrad_critic_finish) — or is launched on its own first where the rider does not apply."""
    k, m = dy.shape
    n = x.shape[1]
    if x2 is not None and not (32 < m <= 64 and n > 64 and n % 5 == 0 and k > 1 and tall_wgrad_supported(dy, x2)
                               and out2.stride(1) == 1):
        tall_wgrad(dy, x2, out=out2, accumulate=accumulate)
        x2 = None
    if k <= 1:
        dy, x = dy.contiguous(), x.contiguous()
    if out is None:
        out = th.empty(m, n, dtype=th.float32, device=dy.device)
    elif out.shape != (m, n) or out.dtype != th.float32 or (m > 1 and (out.stride(1) != 1 or out.stride(0) < n)):
        raise ValueError("tall_wgrad: `out` must be an fp32 [m, n] tensor or a column block of a wider one")
    ws = _scratch("wgrad", dy.device, _lib.FLEXNET_WGRAD_WS_FLOATS)
    a = _lib.FlexWgradArgs()
    a.k, a.m, a.n = k, m, n
    a.lda, a.ldb = (dy.stride(0), x.stride(0)) if k > 1 else (m, n)
    a.a, a.b, a.c = dy.data_ptr(), x.data_ptr(), out.data_ptr()
    rv = ring_view_of(x)
    if rv is not None:           # in place from the replay's stacked-observation ring (RING_VIEWS)
        if x.stride(0) != rv[0].shape[1] or k <= 1:
            raise RuntimeError("tall_wgrad: a placeholder of the stacked-observation ring must be read as whole rows")
        a.b, a.b_row_cell = rv[0].data_ptr(), rv[1].data_ptr()
    a.workspace, a.workspace_floats, a.accumulate = ws.data_ptr(), ws.numel(), int(accumulate)
    a.ldc = out.stride(0) if m > 1 else n
    if colsum is not None:          # [m] <- sum_k dy[k, :], the bias gradient, from the same pass over dy
        a.colsum = colsum.data_ptr()
    if x2 is not None:
        a.b2, a.c2, a.ldb2, a.n2, a.ldc2 = x2.data_ptr(), out2.data_ptr(), x2.stride(0), x2.shape[1], out2.stride(0)
    if critic_finish is not None:
        if WGRAD_FINISH_RIDER and _lib.try_launch("flexnet_wgrad_critic_finish", a, *critic_finish):
            return out
        _lib.launch("flexnet_critic_td_backward_phases", *critic_finish, 2)
    _lib.launch("flexnet_wgrad", a)
    return out


_WGRAD_BATCH_WS = {}


def _wgrad_class(m, n):
    """csrc/wgrad.hip's shape class of an [m, n] result: (MT, NT, column chunks, floats per register image)."""
    mt = 1 if m <= 32 else 2 if m <= 64 else 6
    nt = 1 if n <= 32 else 2 if n <= 64 else (2 if mt == 6 else 5)
    return mt, nt, (n + 32 * nt - 1) // (32 * nt), mt * nt * 1024


def tall_wgrad_batched(problems):
    """Independent weight gradients out_i = dy_i^T x_i in ONE flexnet_wgrad_batched call (csrc/wgrad.hip: one first-stage and
    one second-stage launch per shape class instead of two launches per problem).  ``problems``: (dy, x, out, colsum or None)
    with ``tall_wgrad_supported(dy, x)`` and ``out`` an fp32 [m, n] tensor or a column block of a wider one — agent i's rows
    ``t.view(b, n, w)[:, i]`` of an interleaved tensor are an ordinary problem.  Every problem gets its own slice of a per-device
    workspace, sized for the thread blocks the library will choose for it (a shorter slice would only lower that number).  More
    problems than FLEXNET_WGRAD_MAX_BATCH go in several calls.  Bit-reproducible."""
    for c0 in range(0, len(problems), _lib.FLEXNET_WGRAD_MAX_BATCH):
        _wgrad_batched_call(problems[c0:c0 + _lib.FLEXNET_WGRAD_MAX_BATCH])


def _wgrad_batched_call(problems):
    dev = problems[0][0].device
    classes = [_wgrad_class(dy.shape[1], x.shape[1]) for dy, x, _, _ in problems]
    launch_chunks = {}
    for mt, nt, chunks, _ in classes:
        launch_chunks[(mt, nt)] = launch_chunks.get((mt, nt), 0) + chunks
    need = []
    for (dy, _, _, _), (mt, nt, chunks, img) in zip(problems, classes):
        slabs = max(1, min((dy.shape[0] + 63) // 64, max(1, 512 // launch_chunks[(mt, nt)]), 520))
        need.append(_lib.FLEXNET_WGRAD_CS_FLOATS + slabs * chunks * img)
    total = sum(need)
    ws = _WGRAD_BATCH_WS.get(dev)
    if ws is None or ws.numel() < total:
        ws = _WGRAD_BATCH_WS[dev] = th.empty(total, dtype=th.float32, device=dev)
    table = (_lib.FlexWgradArgs * len(problems))()
    at, keep = 0, []
    for a, (dy, x, out, colsum), floats in zip(table, problems, need):
        k, m = dy.shape
        n = x.shape[1]
        if k <= 1:                        # (a single row's pitch is arbitrary: dense copies, as tall_wgrad)
            dy, x = dy.contiguous(), x.contiguous()
            keep += [dy, x]
        if (not tall_wgrad_supported(dy, x) or out.shape != (m, n) or out.dtype != th.float32
                or (m > 1 and (out.stride(1) != 1 or out.stride(0) < n))):
            raise ValueError("tall_wgrad_batched: fp32 [k, m <= 192] x [k, n] problems into [m, n] blocks")
        a.k, a.m, a.n = k, m, n
        a.lda, a.ldb = (dy.stride(0), x.stride(0)) if k > 1 else (m, n)
        a.a, a.b, a.c = dy.data_ptr(), x.data_ptr(), out.data_ptr()
        a.ldc = out.stride(0) if m > 1 else n
        if colsum is not None:
            a.colsum = colsum.data_ptr()
        a.workspace, a.workspace_floats = ws.data_ptr() + 4 * at, floats
        at += floats
    _lib.launch("flexnet_wgrad_batched", table, len(problems))


class _TallLinear(th.autograd.Function):
    """y = x @ W.T (+ b) for a tall x: the library GEMM forward and for dx, csrc/wgrad.hip for dW."""

    @staticmethod
    def forward(ctx, x, w, b):
        ctx.save_for_backward(x, w)
        ctx.has_bias = b is not None
        return th.addmm(b, x, w.t()) if b is not None else x @ w.t()

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        dx = dw = db = None
        want_db = ctx.has_bias and ctx.needs_input_grad[2]
        if ctx.needs_input_grad[1]:
            if tall_wgrad_supported(dy, x):
                if want_db:
                    db = th.empty(dy.shape[1], dtype=th.float32, device=dy.device)
                dw = tall_wgrad(dy, x, colsum=db)
            else:
                dw = dy.t() @ x
        if ctx.needs_input_grad[0]:
            dx = dy @ w
        if want_db and db is None:
            db = dy.sum(0)
        return dx, dw, db


def tall_linear(x, w, b=None):
    """F.linear for [rows, in] inputs; rows >= WGRAD_MIN_ROWS on the GPU take the hand-written weight gradient."""
    if x.is_cuda and x.dim() == 2 and x.shape[0] >= WGRAD_MIN_ROWS and w.shape[0] <= 192 and x.dtype == th.float32:
        return _TallLinear.apply(x, w, b)
    return F.linear(x, w, b)


# In-place windows of the replay's stacked-observation ring (replay_buffer.DeviceReplayBuffer.enable_stacked_ring; round 5).
# A captured sub-update needs static addresses, so until round 4 every sub-update began by gathering its window's stacked
# observations into a static batch (flexnet_gather_window: 23 us at 32 768 samples, 79 us at 131 072 — a tenth of an update event
# at the reference's sample reuse, each observation expanded ~6 times).  With the ring kept stacked (every slab expanded ONCE,
# when it enters the replay) the window is a contiguous run of ring rows, and the kernels that read observations take the ring's
# base plus a DEVICE cell holding the window's first row (FlexLinear2Args.x1_row_cell, FlexWgradArgs.b_row_cell): the graph is
# static, the window moves.  The static batch's `state` tensor is then a placeholder full of NaN, registered here by its
# data pointer: a consumer that does not know the ring reads NaN, not yesterday's observations.
RING_VIEWS = {}              # placeholder data_ptr -> (ring tensor [rows, width], device int64 cell)


def register_ring_view(placeholder, ring, cell):
    """``placeholder`` (a NaN-filled [rows, width] tensor that stands where a gathered window used to be) is read as rows
    cell[0] .. of ``ring`` by the kernels that know how.  Entries whose placeholder has been freed are dropped first: they
    hold a view of their ring, and a dropped trainer's 2.9 GB ring must not outlive it."""
    import weakref
    for key in [k for k, v in RING_VIEWS.items() if v[2]() is None]:
        del RING_VIEWS[key]
    RING_VIEWS[placeholder.data_ptr()] = (ring, cell, weakref.ref(placeholder))


def ring_view_of(t):
    """(ring, cell) if ``t`` is (a whole-row view of) a registered placeholder, else None."""
    if not RING_VIEWS or not t.is_cuda:
        return None
    key = t.data_ptr()
    rv = RING_VIEWS.get(key)
    if rv is None:
        return None
    if rv[2]() is None:          # the placeholder is gone (its trainer was dropped): the address may be anybody's now
        del RING_VIEWS[key]
        return None
    return rv


LINEAR2_MIN_ROWS = 8192      # below: the library call (a launch of this kernel loads 189 KB of weights into every CU's registers)
LINEAR2_MAX_ROWS = 65536     # above: the library pair again — measured (tools/linear_bench.py, profiles/r05f_linear_bench.txt): 39.6 vs
#                              40-47 us at 32 768 rows, 41.4 vs 71.4 at 36 864, but 138 vs 128 at 131 072 (both within 10 % of what the
#                              fp32 matrix pipe sustains at the clock it holds under this load; the kernel's launch cost is lower, its slope
#                              slightly higher)
CRITIC_FC1_FUSED = True      # (tests switch it off to compare with the two library GEMMs)


def critic_first_layer(bias, obs2d, act2d, W, c_act):
    """``bias + obs2d @ W[:, :no].T + act2d @ W[:, c_act:c_act + na].T`` — the shared part of the centralised critic's
    first layer (mlp_critic.py:25-26 on maddpg.py:33-54's input).  On the GPU at update sizes: ONE launch of
    csrc/linear.hip (include/flexnet.h: flexnet_linear2 — weights stationary in registers, exact fp32 on the matrix cores, no
    second pass over the [b, 64] result; round 5); otherwise the two library GEMMs of rounds 1-4."""
    no, na_ = obs2d.shape[1], act2d.shape[1]
    rv = ring_view_of(obs2d)
    if rv is not None and (th.is_grad_enabled() or obs2d.stride(0) != no or rv[0].shape[1] != no):
        raise RuntimeError("critic_first_layer: a placeholder of the stacked-observation ring reached a path that cannot read it in place")
    ok = (CRITIC_FC1_FUSED and obs2d.is_cuda and obs2d.dtype == th.float32 and act2d.dtype == th.float32 and W.dtype == th.float32
          and (rv is not None or LINEAR2_MIN_ROWS <= obs2d.shape[0] <= LINEAR2_MAX_ROWS) and W.shape[0] == 64 and no % 8 == 0 and na_ % 4 == 0
          and obs2d.stride(0) % 4 == 0 and act2d.stride(0) % 4 == 0
          and obs2d.stride(1) == 1 and act2d.stride(1) == 1 and W.stride(1) == 1 and bias.is_contiguous()
          and not th.is_grad_enabled())
    if ok:
        out = th.empty(obs2d.shape[0], 64, dtype=th.float32, device=obs2d.device)
        a = _lib.FlexLinear2Args()
        a.rows, a.k1, a.k2 = obs2d.shape[0], no, na_
        a.ld1, a.ld2, a.ldw, a.c1, a.c2 = obs2d.stride(0), act2d.stride(0), W.stride(0), 0, int(c_act)
        a.x1, a.x2, a.w, a.bias, a.out = obs2d.data_ptr(), act2d.data_ptr(), W.data_ptr(), bias.data_ptr(), out.data_ptr()
        if rv is not None:
            a.x1, a.x1_row_cell = rv[0].data_ptr(), rv[1].data_ptr()
        if _lib.try_launch("flexnet_linear2", a):
            return out
        if rv is not None:
            raise RuntimeError("flexnet_linear2 declined an in-place window of the stacked-observation ring (FLEXNET_EUNSUPPORTED)")
        note_fallback("critic_fc1", "FLEXNET_EUNSUPPORTED from flexnet_linear2")
    if rv is not None:
        raise RuntimeError("critic_first_layer: an in-place window of the stacked-observation ring needs the fused kernel")
    shared = th.addmm(bias, obs2d, W[:, :no].t())
    shared.addmm_(act2d, W[:, c_act:c_act + na_].t())
    return shared


def _td_workspace(device):
    """Per-device fp64 scratch of csrc/tdloss.hip (statistics partials)."""
    return _scratch("td", device, _lib.FLEXNET_TD_WS_FLOATS // 2, th.float64)


# Cross-rank reward statistics ("or all-reduce 2 x 5 moments"; off unless the trainer switches it on):
# model.py:321-322 normalises the reward with BATCH statistics; with data-parallel ranks each rank's batch is a shard, and
# the full-batch statistics are the sums over the ranks of the per-rank sums.  GPU path: the statistics pass of
# csrc/tdloss.hip leaves its per-block partial sums in the workspace, ONE all-reduce of those 8 KB makes them global
# (flexnet_td_stats -> all-reduce -> the call with stats_ready / stat_rows); CPU path: sync_batchnorm below.
# The switch lives on the BatchNorm MODULE (``bn.flex_sync_ranks``, set by the trainer that owns the model): a second
# trainer in the same process (bench legs, an evaluation trainer, tests) cannot change the behaviour of the first one,
# and a trainer's graphed and eager paths read the same flag (it used to be a module global).


def set_reward_bn_sync(bn, on):
    if bn is not None:
        object.__setattr__(bn, "flex_sync_ranks", bool(on))


def _sync_active(bn):
    import torch.distributed as dist
    return (bn is not None and getattr(bn, "flex_sync_ranks", False) and dist.is_available() and dist.is_initialized()
            and dist.get_world_size() > 1)


# Reward statistics filed ahead of the loss (round 5).  The trainer's captured value sub-update refreshes its static batch with
# ONE gather launch per window; the statistics pass of the fused value loss needs the batch's rewards only, so it rides in that
# launch (flexnet_gather_rows_td) instead of being the graph's own 6.5-us launch between the first-layer product and the
# backward kernel.  Protocol: the trainer OFFERS the static reward tensor (offer_td_stats) before the warm-up steps;
# _CriticTdLossFn.forward, meeting that tensor, takes the offer — stats_ready = 1, no statistics launch — and records that it
# did; the trainer then keeps the rider for every refresh of that batch (TransReplayBuffer.gather(td=...)) or withdraws it.
TD_OFFERS = {}              # data_ptr of a static [rows, n] reward tensor -> {"taken": bool}


def offer_td_stats(reward):
    """Offer to file the reward statistics of ``reward`` (a static batch tensor) with every refresh of it.  Returns
    (record, FlexTdLossArgs for the rider); record["taken"] says after a loss has run whether the fused value loss used them."""
    import weakref
    r2 = reward.reshape(reward.shape[0], -1)
    rec = {"taken": False, "ref": weakref.ref(reward)}        # (a dead tensor's address may be handed out again: checked on use)
    TD_OFFERS[r2.data_ptr()] = rec
    rows, n = r2.shape
    ws = _td_workspace(r2.device)
    a = _lib.FlexTdLossArgs()
    a.rows, a.n_agents, a.normalise, a.reward = rows, n, 1, r2.data_ptr()
    a.workspace, a.workspace_floats = ws.data_ptr(), 2 * ws.numel()
    return rec, a


def withdraw_td_stats(reward):
    TD_OFFERS.pop(reward.reshape(reward.shape[0], -1).data_ptr(), None)


def _td_sync_stats(a, ws, bn):
    """If cross-rank statistics are on for ``bn``: statistics pass, all-reduce of the partial sums, and mark ``a``
    (FlexTdLossArgs) so that the call that follows uses them instead of computing its own.  ``ws``: the fp64 workspace
    tensor of ``a``."""
    if not (a.normalise and _sync_active(bn)):
        return
    import torch.distributed as dist
    _lib.launch("flexnet_td_stats", a)
    dist.all_reduce(ws[:_lib.FLEXNET_TD_STAT_DOUBLES], op=dist.ReduceOp.SUM)
    a.stats_ready, a.stat_rows = 1, int(a.rows) * dist.get_world_size()


def sync_batchnorm(bn, x):
    """``bn(x)`` of a training-mode nn.BatchNorm1d on [rows, n] with the batch statistics taken over ALL ranks' rows (equal
    shards): normalised output, running statistics and num_batches_tracked moved as the module moves them.  Plain tensor
    ops (the eager / CPU path); without an initialised process group of more than one rank it is ``bn(x)``."""
    if not (_sync_active(bn) and bn.training):
        return bn(x)
    import torch.distributed as dist
    xd = x.double()
    mom = th.cat([xd.sum(0), (xd * xd).sum(0)])
    dist.all_reduce(mom, op=dist.ReduceOp.SUM)
    rows = x.shape[0] * dist.get_world_size()
    n = x.shape[1]
    mean = mom[:n] / rows
    var = (mom[n:] / rows - mean * mean).clamp_min(0.0)
    out = (xd - mean) / th.sqrt(var + bn.eps)
    if bn.affine:
        out = out * bn.weight.double() + bn.bias.double()
    if bn.track_running_stats:
        with th.no_grad():
            m = bn.momentum
            unbiased = var * rows / (rows - 1) if rows > 1 else var
            bn.running_mean.mul_(1 - m).add_((m * mean).to(bn.running_mean.dtype))
            bn.running_var.mul_(1 - m).add_((m * unbiased).to(bn.running_var.dtype))
            bn.num_batches_tracked += 1
    return out.to(x.dtype)


class _TdLossFn(th.autograd.Function):
    """mean((BatchNorm(reward) + gamma (1 - done) next_q - q)^2) (maddpg.py:100-123 behind model.py:308-323) with its
    gradient w.r.t. q, in three small launches (csrc/tdloss.hip); the BatchNorm module's running statistics are
    updated in place as its own forward would."""

    @staticmethod
    def forward(ctx, q, next_q, reward, done, gamma, bn, update_stats=True):
        rows, n = reward.shape
        q2, nq, r, d = q.reshape(rows, n).contiguous(), next_q.reshape(rows, n).contiguous(), reward.contiguous(), \
            done.reshape(rows).contiguous()
        dq = th.empty_like(q2)
        loss = th.empty((), dtype=th.float32, device=q.device)
        ws = _td_workspace(q.device)
        a = _lib.FlexTdLossArgs()
        a.rows, a.n_agents, a.normalise, a.gamma = rows, n, int(bn is not None), float(gamma)
        a.reward, a.done, a.next_q, a.q = r.data_ptr(), d.data_ptr(), nq.data_ptr(), q2.data_ptr()
        if bn is not None:
            a.bn_eps, a.bn_momentum = float(bn.eps), float(bn.momentum)
            if bn.affine:
                a.bn_weight, a.bn_bias = bn.weight.data_ptr(), bn.bias.data_ptr()
            if bn.track_running_stats and update_stats:
                a.running_mean, a.running_var = bn.running_mean.data_ptr(), bn.running_var.data_ptr()
                a.num_batches_tracked = bn.num_batches_tracked.data_ptr()
        a.dq, a.loss = dq.data_ptr(), loss.data_ptr()
        a.workspace, a.workspace_floats = ws.data_ptr(), 2 * ws.numel()
        _td_sync_stats(a, ws, bn)
        _lib.launch("flexnet_td_loss", a)
        ctx.save_for_backward(dq)
        ctx.q_shape = q.shape
        return loss

    @staticmethod
    def backward(ctx, grad_loss):
        (dq,) = ctx.saved_tensors
        from .util import is_unit_seed
        if is_unit_seed(grad_loss):                   # the trainer's root gradient: dq is the answer as it stands
            return dq.view(ctx.q_shape), None, None, None, None, None, None
        return (dq * grad_loss).view(ctx.q_shape), None, None, None, None, None, None


def td_loss_supported(q, next_q, reward, done, bn):
    """The fused value loss covers fp32 GPU tensors, up to 8 agents, and a BatchNorm1d in training mode with momentum
    (or no normalisation at all)."""
    ok = (q.is_cuda and q.dtype == th.float32 and next_q.dtype == th.float32 and reward.dtype == th.float32
          and done.dtype == th.float32 and reward.dim() == 2 and 1 <= reward.shape[1] <= 8 and reward.shape[0] >= 1
          and q.numel() == reward.numel() and next_q.numel() == reward.numel() and done.numel() == reward.shape[0]
          and not next_q.requires_grad)
    if bn is not None:
        ok = ok and bn.training and bn.momentum is not None and isinstance(bn, nn.BatchNorm1d) \
            and bn.num_features == reward.shape[1] and (not bn.track_running_stats or bn.running_mean.dtype == th.float32)
    return bool(ok)


def batchnorm_update_running_stats(bn, x):
    """What a training-mode ``bn(x)`` does to ``running_mean`` / ``running_var`` / ``num_batches_tracked``, without the
    normalised output (csrc/tdloss.hip statistics pass): for get_loss calls that normalise the reward only for the
    module's bookkeeping (the policy loss never reads it, model.py:308-323)."""
    rows, n = x.shape
    x = x.contiguous()
    ws = _td_workspace(x.device)
    a = _lib.FlexTdLossArgs()
    a.rows, a.n_agents, a.normalise = rows, n, 1
    a.bn_eps, a.bn_momentum = float(bn.eps), float(bn.momentum)
    a.reward = x.data_ptr()
    a.running_mean, a.running_var = bn.running_mean.data_ptr(), bn.running_var.data_ptr()
    a.num_batches_tracked = bn.num_batches_tracked.data_ptr()
    a.workspace, a.workspace_floats = ws.data_ptr(), 2 * ws.numel()
    _td_sync_stats(a, ws, bn)
    _lib.launch("flexnet_td_loss", a)


def batchnorm_stats_supported(bn, x):
    return bool(x.is_cuda and x.dtype == th.float32 and x.dim() == 2 and 1 <= x.shape[1] <= 8 and x.shape[0] >= 1
                and isinstance(bn, nn.BatchNorm1d) and bn.training and bn.momentum is not None and bn.track_running_stats
                and bn.num_features == x.shape[1] and bn.running_mean.dtype == th.float32)


def td_loss(q, next_q, reward, done, gamma, bn=None, update_stats=True):
    """``update_stats=False``: the same batch-statistics normalisation without moving the module's running statistics
    (a second loss term on the same normalised reward, matd3.py:141-148)."""
    return _TdLossFn.apply(q, next_q, reward, done, gamma, bn, update_stats)


def _lnrelu_workspace(device):
    """Per-device scratch of csrc/lnrelu.hip's backward and of the first layer's backward inside csrc/gru.hip (same partials)."""
    return _scratch("lnrelu", device, _lib.FLEXNET_LNRELU_WS_FLOATS)


def _lnrelu_args(z, bias, id_cols, ln_w, ln_b, eps, n_agents):
    a = _lib.FlexLnReluArgs()
    a.rows, a.n_agents, a.layernorm, a.ln_eps = z.shape[0], n_agents, int(ln_w is not None), float(eps)
    a.z = z.data_ptr()
    a.bias = None if bias is None else bias.data_ptr()
    a.id_cols = None if id_cols is None else id_cols.data_ptr()
    if ln_w is not None:
        a.ln_w, a.ln_b = ln_w.data_ptr(), ln_b.data_ptr()
    return a


class _LnReluFn(th.autograd.Function):
    """relu(LayerNorm(z + bias + id_cols[r % n])) (rnn_agent.py:25-29 after the fc1 GEMM) with a hand-written backward
    (csrc/lnrelu.hip): dz and the gradients of bias, id columns and the LayerNorm pair in two launches."""

    @staticmethod
    def forward(ctx, z, bias, id_cols, ln_w, ln_b, eps, n_agents):
        z = z.contiguous()
        id_cols = None if id_cols is None else id_cols.contiguous()
        out = th.empty_like(z)
        a = _lnrelu_args(z, bias, id_cols, ln_w, ln_b, eps, n_agents)
        a.out = out.data_ptr()
        _lib.launch("flexnet_lnrelu_forward", a)
        ctx.eps, ctx.n_agents = eps, n_agents
        ctx.save_for_backward(z, bias, id_cols, ln_w, ln_b)
        return out

    @staticmethod
    def backward(ctx, dout):
        z, bias, id_cols, ln_w, ln_b = ctx.saved_tensors
        dout = dout.contiguous()
        dz = th.empty_like(z)
        small = th.empty(3 + ctx.n_agents, 64, dtype=th.float32, device=z.device)
        a = _lnrelu_args(z, bias, id_cols, ln_w, ln_b, ctx.eps, ctx.n_agents)
        a.dout, a.dz = dout.data_ptr(), dz.data_ptr()
        if ln_w is not None:
            a.d_ln_w, a.d_ln_b = small[0].data_ptr(), small[1].data_ptr()
        if bias is not None:
            a.d_bias = small[2].data_ptr()
        if id_cols is not None:
            a.d_id = small[3:].data_ptr()
        ws = _lnrelu_workspace(z.device)
        a.workspace, a.workspace_floats = ws.data_ptr(), ws.numel()
        _lib.launch("flexnet_lnrelu_backward", a)
        return (dz, None if bias is None else small[2], None if id_cols is None else small[3:],
                None if ln_w is None else small[0], None if ln_w is None else small[1], None, None)


# the first layer's backward inside the gate-gradient launch (csrc/gru.hip, gru_backward_fused_kernel); False: the round-2
# composition (pointwise gate gradients, library GEMM for dx, csrc/lnrelu.hip) — kept as the cross-check of tests/test_gru_gpu.py
GRU_BWD_FUSED = True
_DEBUG_KEEP = None                # tools/gru_diag.py: a dict that receives the backward's dz


class _ActorTrainFn(th.autograd.Function):
    """The whole actor of rnn_agent.py:25-33 for an update batch as ONE autograd node: the forward is the fused
    matrix-core kernel of csrc/actor.hip (fc1 -> LayerNorm -> ReLU -> GRUCell -> fc2 chained through registers) with its
    `save_*` outputs, the backward is csrc/gru.hip (gate gradients, fc2's input gradient folded in), csrc/wgrad.hip for
    every weight / bias gradient, one library GEMM for dx and csrc/lnrelu.hip for the first layer's epilogue.  Replaces
    the composition fc1 GEMM + lnrelu + two gate GEMMs + ATen's pointwise GRU cell + fc2 GEMM (309 us forward at 163 840
    rows) and their autograd backward.  Observations and the previous hidden state are replayed tensors: no gradient."""

    @staticmethod
    def forward(ctx, obs, hidden, n_agents, agent_id, fc1_w, fc1_b, ln_w, ln_b, ln_eps, w_ih, w_hh, b_ih, b_hh, fc2_w, fc2_b):
        rows, o = obs.shape
        act_dim = fc2_w.shape[0]
        obs, hidden = obs.contiguous(), hidden.contiguous()
        means = th.empty(rows, act_dim, dtype=th.float32, device=obs.device)
        hid_out = th.empty(rows, 64, dtype=th.float32, device=obs.device)
        saved = th.empty(6, rows, 64, dtype=th.float32, device=obs.device)          # z1 | x | r | z | n | hn
        a = _lib.FlexActorArgs()
        a.rows, a.n_agents, a.obs_dim, a.act_dim = rows, n_agents, o, act_dim
        a.agent_id, a.layernorm, a.ln_eps, a.variant = int(bool(agent_id)), int(ln_w is not None), float(ln_eps), 0
        for name, t in (("obs", obs), ("hidden_in", hidden), ("fc1_w", fc1_w), ("fc1_b", fc1_b), ("ln_w", ln_w), ("ln_b", ln_b),
                        ("w_ih", w_ih), ("w_hh", w_hh), ("b_ih", b_ih), ("b_hh", b_hh), ("fc2_w", fc2_w), ("fc2_b", fc2_b),
                        ("means", means), ("hidden_out", hid_out), ("save_z1", saved[0]), ("save_x", saved[1]),
                        ("save_r", saved[2]), ("save_z", saved[3]), ("save_n", saved[4]), ("save_hn", saved[5])):
            if t is not None:
                if not t.is_contiguous():
                    raise ValueError(f"actor training forward: {name} must be contiguous")
                setattr(a, name, t.data_ptr())
        _lib.launch("flexnet_actor_forward", a)
        ctx.n_agents, ctx.agent_id, ctx.ln_eps = n_agents, bool(agent_id), float(ln_eps)
        ctx.save_for_backward(obs, hidden, hid_out, saved, fc1_w, fc1_b, ln_w, ln_b, w_ih, fc2_w)
        if not getattr(ctx, "hid_grad", False):
            ctx.mark_non_differentiable(hid_out)      # the new hidden state is returned for the caller's bookkeeping only
        ctx.set_materialize_grads(False)              # ... and must not cost a [rows, 64] zero fill per backward
        return means, hid_out

    @staticmethod
    def backward(ctx, d_means, _d_hid):
        obs, hidden, hid_out, saved, fc1_w, fc1_b, ln_w, ln_b, w_ih, fc2_w = ctx.saved_tensors
        rows, o = obs.shape
        n, dev = ctx.n_agents, obs.device
        if d_means is None:                           # (_ActorTrainHidFn: the gradient arrived at the hidden state alone)
            d_means = th.zeros(rows, fc2_w.shape[0], dtype=th.float32, device=dev)
        d_means = d_means.contiguous()
        d_gi = th.empty(rows, 192, dtype=th.float32, device=dev)
        d_gh = th.empty(rows, 192, dtype=th.float32, device=dev)
        g = _lib.FlexGruBwdArgs()
        g.rows, g.act_dim = rows, fc2_w.shape[0]
        g.d_means, g.fc2_w = d_means.data_ptr(), fc2_w.data_ptr()
        g.r, g.z, g.n, g.hn = saved[2].data_ptr(), saved[3].data_ptr(), saved[4].data_ptr(), saved[5].data_ptr()
        g.h_prev, g.d_gi, g.d_gh = hidden.data_ptr(), d_gi.data_ptr(), d_gh.data_ptr()
        if _d_hid is not None:                        # (_ActorTrainHidFn: the log-std head's gradient at the new hidden state)
            _d_hid = _d_hid.contiguous()
            g.d_hidden = _d_hid.data_ptr()
        fused = GRU_BWD_FUSED
        if fused:
            # ... and the first layer's backward in the same launch (round 3): dx = d_gi @ W_ih on the matrix cores, never
            # stored; LayerNorm / ReLU / bias / id columns backward; the id-column sums land in fc1's gradient through strides
            dz = th.empty(rows, 64, dtype=th.float32, device=dev)
            small = th.empty(3, 64, dtype=th.float32, device=dev)
            d_fc1_w = th.empty_like(fc1_w)
            ws = _lnrelu_workspace(dev)
            g.w_ih, g.z1, g.fc1_w, g.dz = w_ih.data_ptr(), saved[0].data_ptr(), fc1_w.data_ptr(), dz.data_ptr()
            g.x = saved[1].data_ptr()                  # ReLU's mask: the forward's own output
            g.fc1_b = fc1_b.data_ptr() if fc1_b is not None else None
            g.fc1_ld, g.obs_dim, g.n_agents, g.agent_id = fc1_w.shape[1], o, n, int(ctx.agent_id)
            g.layernorm, g.ln_eps = int(ln_w is not None), ctx.ln_eps
            if ln_w is not None:
                g.ln_w, g.ln_b, g.d_ln_w, g.d_ln_b = ln_w.data_ptr(), ln_b.data_ptr(), small[0].data_ptr(), small[1].data_ptr()
            g.d_fc1_b = small[2].data_ptr()
            if ctx.agent_id:
                g.d_id = d_fc1_w.data_ptr() + 4 * o
                g.d_id_agent_stride, g.d_id_unit_stride = 1, fc1_w.shape[1]
            g.workspace, g.workspace_floats = ws.data_ptr(), ws.numel()
        _lib.launch("flexnet_gru_backward", g)
        # fc2: weight and bias gradients from one pass over d_means
        d_fc2_b = th.empty(fc2_w.shape[0], dtype=th.float32, device=dev)
        d_fc2_w = tall_wgrad(d_means, hid_out, colsum=d_fc2_b)
        # GRUCell: W_ih sees [dr | dz | dn], W_hh sees [dr | dz | dn r]; the biases are the column sums of the same passes
        d_b_ih = th.empty(192, dtype=th.float32, device=dev)
        d_w_ih = tall_wgrad(d_gi, saved[1], colsum=d_b_ih)
        d_b_hh = th.empty(192, dtype=th.float32, device=dev)
        d_w_hh = tall_wgrad(d_gh, hidden, colsum=d_b_hh)
        if fused:
            if _DEBUG_KEEP is not None:
                _DEBUG_KEEP["dz"] = dz
            tall_wgrad(dz, obs, out=d_fc1_w[:, :o])
            has_ln = ln_w is not None
            return (None, None, None, None, d_fc1_w, small[2], small[0] if has_ln else None, small[1] if has_ln else None, None,
                    d_w_ih, d_w_hh, d_b_ih, d_b_hh, d_fc2_w, d_fc2_b)
        # first layer: dx = d_gi @ W_ih, then the LayerNorm / ReLU / bias / id-column epilogue backward and fc1's weight
        dx = d_gi @ w_ih
        dz = th.empty(rows, 64, dtype=th.float32, device=dev)
        small = th.empty(3 + n, 64, dtype=th.float32, device=dev)
        id_cols = fc1_w[:, o:].t().contiguous() if ctx.agent_id else None
        la = _lnrelu_args(saved[0], fc1_b, id_cols, ln_w, ln_b, ctx.ln_eps, n)
        la.dout, la.dz = dx.data_ptr(), dz.data_ptr()
        if ln_w is not None:
            la.d_ln_w, la.d_ln_b = small[0].data_ptr(), small[1].data_ptr()
        la.d_bias = small[2].data_ptr()
        if id_cols is not None:
            la.d_id = small[3:].data_ptr()
        ws = _lnrelu_workspace(dev)
        la.workspace, la.workspace_floats = ws.data_ptr(), ws.numel()
        _lib.launch("flexnet_lnrelu_backward", la)
        if _DEBUG_KEEP is not None:
            _DEBUG_KEEP["dz"] = dz
        d_fc1_w = th.empty_like(fc1_w)
        tall_wgrad(dz, obs, out=d_fc1_w[:, :o])
        if ctx.agent_id:
            d_fc1_w[:, o:] = small[3:].t()
        has_ln = ln_w is not None
        return (None, None, None, None, d_fc1_w, small[2], small[0] if has_ln else None, small[1] if has_ln else None, None,
                d_w_ih, d_w_hh, d_b_ih, d_b_hh, d_fc2_w, d_fc2_b)


class _ActorTrainHidFn(_ActorTrainFn):
    """_ActorTrainFn whose new hidden state takes a gradient too (FlexGruBwdArgs.d_hidden): the Gaussian agent's log-std
    head reads it, and autograd sums that head's d_h with nothing else — the mean head's share is formed inside the kernel."""

    @staticmethod
    def forward(ctx, *args):
        ctx.hid_grad = True
        return _ActorTrainFn.forward(ctx, *args)


def actor_train_supported(agent, obs, n_agents, agent_id):
    """What the fused training pass covers: the RNN agent at 64 hidden units with ReLU, fp32 GPU rows >= WGRAD_MIN_ROWS."""
    a = agent.args
    W = agent.fc1.weight
    return (isinstance(agent, RNNAgent) and obs.is_cuda and obs.dtype == th.float32 and obs.dim() == 2
            and a.hid_size == 64 and a.hid_activation == "relu" and obs.shape[1] <= 144 and 1 <= n_agents <= 8
            and a.action_dim <= 8 and obs.shape[0] >= WGRAD_MIN_ROWS and obs.shape[0] % n_agents == 0
            and W.shape[1] == obs.shape[1] + (n_agents if agent_id else 0) and not obs.requires_grad
            and getattr(agent, "fused_training", True) and getattr(agent, "fused_epilogue", True))


_UNSHARED_TABLES = ("fc1_w", "fc1_b", "ln_w", "ln_b", "w_ih", "w_hh", "b_ih", "b_hh", "fc2_w", "fc2_b")
ACTOR_UNSHARED_MAX_ROWS = 1 << 26        # csrc/wgrad.hip addresses a block's rows through 32-bit byte offsets


def _unshared_params(agent):
    """The ten parameters of one RNNAgent in ``_UNSHARED_TABLES`` order (the LayerNorm pair None without layernorm)."""
    ln = agent.layernorm if agent.args.layernorm else None
    r = agent.rnn
    return (agent.fc1.weight, agent.fc1.bias, None if ln is None else ln.weight, None if ln is None else ln.bias,
            r.weight_ih, r.weight_hh, r.bias_ih, r.bias_hh, agent.fc2.weight, agent.fc2.bias)


def _unshared_declines(agents, obs, agent_id, kind=None):
    """Why csrc/actor_unshared.hip does not cover these per-agent actors on ``obs`` [b, n, obs_dim], or None.  ``kind``: the one
    class every agent must be — RNNAgent (default), or RNNAgentGaussian, whose ``mean`` head sits in the fc2 slot."""
    kind = RNNAgent if kind is None else kind
    n, o = len(agents), obs.shape[-1]
    a = agents[0].args
    if not (obs.is_cuda and obs.dtype == th.float32 and obs.dim() == 3 and obs.shape[1] == n):
        return f"obs {tuple(obs.shape)} {obs.dtype} for {n} agents"
    if not (a.hid_size == 64 and a.hid_activation == "relu" and o <= 144 and 1 <= n <= 8 and a.action_dim <= 8):
        return f"hid {a.hid_size}, act {a.hid_activation}, obs {o}, agents {n}, actions {a.action_dim}"
    if obs.shape[0] * n >= ACTOR_UNSHARED_MAX_ROWS:
        return f"{obs.shape[0] * n} rows"
    for i, agent in enumerate(agents):
        if type(agent) is not kind:
            return f"agent {i} is a {type(agent).__name__}"
        if agent.fc1.weight.shape[1] != o + (n if agent_id else 0):
            return f"agent {i}: fc1 takes {agent.fc1.weight.shape[1]} columns, obs {o}, agent_id {bool(agent_id)}"
        if not (getattr(agent, "fused_training", True) and getattr(agent, "fused_epilogue", True)):
            return f"agent {i}: fused passes switched off"
        why = _params_decline(_unshared_params(agent))
        if why is not None:
            return f"agent {i}: {why}"
    return None


def actor_unshared_supported(agents, obs, agent_id, train=True, kind=None):
    """``actor_train_supported``'s conditions for EVERY agent of a ``shared_params: False`` model (obs [b, n, obs_dim]), and
    ``type(agent) is kind`` (RNNAgent); ``train``: also the row threshold of the hand-written weight gradients."""
    return (_unshared_declines(agents, obs, agent_id, kind) is None and not obs.requires_grad
            and (not train or obs.shape[0] * obs.shape[1] >= WGRAD_MIN_ROWS))


def _unshared_args(cls, params, rows, n, o, act_dim, agent_id, ln_eps):
    a = cls()
    a.rows, a.n_agents, a.obs_dim, a.act_dim = rows, n, o, act_dim
    a.agent_id, a.layernorm, a.ln_eps = int(bool(agent_id)), int(params[0][2] is not None), float(ln_eps)
    _fill_tables(a, _UNSHARED_TABLES, params, n)
    return a


def _unshared_launch_forward(params, obs, hidden, n, agent_id, ln_eps, saved=None):
    """One flexnet_actor_unshared_forward launch on obs [rows, o], hidden [rows, 64] (both contiguous); (means, hidden) or None
    when the library answers FLEXNET_EUNSUPPORTED."""
    rows, o = obs.shape
    act_dim = params[0][8].shape[0]
    means = th.empty(rows, act_dim, dtype=th.float32, device=obs.device)
    hid_out = th.empty(rows, 64, dtype=th.float32, device=obs.device)
    a = _unshared_args(_lib.FlexActorUnsharedArgs, params, rows, n, o, act_dim, agent_id, ln_eps)
    a.obs, a.hidden_in, a.means, a.hidden_out = obs.data_ptr(), hidden.data_ptr(), means.data_ptr(), hid_out.data_ptr()
    if saved is not None:
        for k, name in enumerate(("save_z1", "save_x", "save_r", "save_z", "save_n", "save_hn")):
            setattr(a, name, saved[k].data_ptr())
    if not _lib.try_launch("flexnet_actor_unshared_forward", a):
        return None
    return means, hid_out


def fused_actor_forward_unshared(agents, obs, hidden):
    """model.py:124-138 (one RNNAgent per agent) without an autograd graph, in ONE HIP launch (csrc/actor_unshared.hip) instead
    of the loop's ten kernels per agent.  ``obs`` [b, n, obs_dim] WITHOUT the one-hot id columns (agent i's own id column of
    its fc1 is added by the kernel), ``hidden`` [b, n, 64] or [b * n, 64].  Returns (means [b * n, act], hidden [b * n, 64]) in
    the caller's row order, or None after ``note_fallback("actor_unshared", ...)`` when it declines on GPU tensors."""
    agents = list(agents)
    n, o = len(agents), obs.shape[-1]
    agent_id = agents[0].fc1.weight.shape[1] != o
    why = _unshared_declines(agents, obs, agent_id, RNNAgentGaussian if type(agents[0]) is RNNAgentGaussian else None)
    if why is None and hidden.dtype != th.float32:
        why = f"hidden {hidden.dtype}"

    def launch():
        rows = obs.shape[0] * n
        return _unshared_launch_forward([_unshared_params(g) for g in agents], obs.reshape(rows, o).contiguous(),
                                        hidden.reshape(rows, 64).contiguous(), n, agent_id, _ln_eps(agents[0]))
    return _fused_inference("actor_unshared", why, obs.is_cuda, "flexnet_actor_unshared_forward", launch)


class _ActorUnsharedTrainFn(th.autograd.Function):
    """The per-agent actors of ``shared_params: False`` for an update batch as ONE autograd node (csrc/actor_unshared.hip): the
    fused forward with its saves, one backward launch for the gate gradients, dx and the first layer's epilogue of every agent,
    then csrc/wgrad.hip per agent through row pitches (rows a, a + n, ... of the [rows, .] tensors are agent a's), the 4 n
    products as one flexnet_wgrad_batched call.  The id block
    of agent a's fc1 gradient is zero except its own column a, which is its bias gradient (the one-hot input).  Observations
    and the previous hidden state take no gradient; the new hidden state is non-differentiable.  Bit-reproducible."""

    @staticmethod
    def forward(ctx, obs, hidden, n_agents, agent_id, ln_eps, *flat):
        rows, o = obs.shape
        params = [flat[10 * i:10 * i + 10] for i in range(n_agents)]
        obs, hidden = obs.contiguous(), hidden.contiguous()
        saved = th.empty(6, rows, 64, dtype=th.float32, device=obs.device)          # z1 | x | r | z | n | hn
        out = _unshared_launch_forward(params, obs, hidden, n_agents, agent_id, ln_eps, saved)
        if out is None:
            _lib.check(_lib.FLEXNET_EUNSUPPORTED, "flexnet_actor_unshared_forward")
        means, hid_out = out
        ctx.n_agents, ctx.agent_id, ctx.ln_eps = n_agents, bool(agent_id), float(ln_eps)
        ctx.has_ln = params[0][2] is not None
        ctx.save_for_backward(obs, hidden, hid_out, saved, *[p for p in flat if p is not None])
        if not getattr(ctx, "hid_grad", False):
            ctx.mark_non_differentiable(hid_out)
        ctx.set_materialize_grads(False)
        return means, hid_out

    @staticmethod
    def backward(ctx, d_means, d_hid):
        obs, hidden, hid_out, saved = ctx.saved_tensors[:4]
        n, dev, has_ln = ctx.n_agents, obs.device, ctx.has_ln
        params = _regroup_params(ctx.saved_tensors[4:], n, 10, has_ln)
        rows, o = obs.shape
        b, act_dim = rows // n, params[0][8].shape[0]
        if d_means is None and d_hid is None:
            return (None,) * (5 + 10 * n)
        d_means = th.zeros(rows, act_dim, dtype=th.float32, device=dev) if d_means is None else d_means.contiguous()
        d_gi = th.empty(rows, 192, dtype=th.float32, device=dev)
        d_gh = th.empty(rows, 192, dtype=th.float32, device=dev)
        dz = th.empty(rows, 64, dtype=th.float32, device=dev)
        small = th.empty(3, n, 64, dtype=th.float32, device=dev)                   # d_ln_w | d_ln_b | d_fc1_b
        ws = _scratch("actor_unshared", dev, _lib.FLEXNET_ACTOR_UNSHARED_WS_FLOATS)
        g = _unshared_args(_lib.FlexActorUnsharedBwdArgs, params, rows, n, o, act_dim, ctx.agent_id, ctx.ln_eps)
        g.d_means, g.h_prev = d_means.data_ptr(), hidden.data_ptr()
        g.z1, g.x, g.r, g.z, g.n, g.hn = (saved[k].data_ptr() for k in range(6))
        g.d_gi, g.d_gh, g.dz = d_gi.data_ptr(), d_gh.data_ptr(), dz.data_ptr()
        g.d_ln_w, g.d_ln_b, g.d_fc1_b = small[0].data_ptr(), small[1].data_ptr(), small[2].data_ptr()
        g.workspace, g.workspace_floats = ws.data_ptr(), ws.numel()
        if d_hid is None:
            _lib.launch("flexnet_actor_unshared_backward", g)
        else:                                        # (_ActorUnsharedTrainHidFn: the log-std heads' gradient at the new hidden state)
            if not mlp_actor_allowed():
                raise RuntimeError("flexnet_actor_unshared_backward_hn is launched eagerly only (nets.mlp_actor_allowed)")
            d_hid = d_hid.contiguous()
            _lib.launch("flexnet_actor_unshared_backward_hn", g, C.c_void_p(d_hid.data_ptr()))
        # the weight gradients: four csrc/wgrad.hip products per agent, each over the agent's rows through the row pitch, all in
        # ONE flexnet_wgrad_batched call; the GRU's and fc2's bias gradients are the column sums of the same passes
        ld = params[0][0].shape[1]
        d_fc1_w = th.zeros(n, 64, ld, dtype=th.float32, device=dev) if ctx.agent_id else th.empty(n, 64, ld, dtype=th.float32, device=dev)
        d_w_ih, d_w_hh = th.empty(2, n, 192, 64, dtype=th.float32, device=dev).unbind(0)
        d_b_ih, d_b_hh = th.empty(2, n, 192, dtype=th.float32, device=dev).unbind(0)
        d_fc2_w = th.empty(n, act_dim, 64, dtype=th.float32, device=dev)
        d_fc2_b = th.empty(n, act_dim, dtype=th.float32, device=dev)
        obs3, hid3, hout3, x3 = obs.view(b, n, o), hidden.view(b, n, 64), hid_out.view(b, n, 64), saved[1].view(b, n, 64)
        dm3, dgi3, dgh3, dz3 = d_means.view(b, n, act_dim), d_gi.view(b, n, 192), d_gh.view(b, n, 192), dz.view(b, n, 64)
        problems = []
        for i in range(n):
            problems += [(dm3[:, i], hout3[:, i], d_fc2_w[i], d_fc2_b[i]), (dgi3[:, i], x3[:, i], d_w_ih[i], d_b_ih[i]),
                         (dgh3[:, i], hid3[:, i], d_w_hh[i], d_b_hh[i]), (dz3[:, i], obs3[:, i], d_fc1_w[i, :, :o], None)]
        tall_wgrad_batched(problems)
        if ctx.agent_id:
            th.diagonal(d_fc1_w[:, :, o:], dim1=0, dim2=2).copy_(small[2].t())     # [64, n]: agent i's own id column
        grads = []
        for i in range(n):
            grads += [d_fc1_w[i], small[2, i], small[0, i] if has_ln else None, small[1, i] if has_ln else None,
                      d_w_ih[i], d_w_hh[i], d_b_ih[i], d_b_hh[i], d_fc2_w[i], d_fc2_b[i]]
        return (None, None, None, None, None, *grads)


class _ActorUnsharedTrainHidFn(_ActorUnsharedTrainFn):
    """_ActorUnsharedTrainFn whose new hidden state takes a gradient too (flexnet_actor_unshared_backward_hn): the Gaussian
    agents' per-agent log-std heads read it (``_GaussHeadUnsharedFn``); the mean heads' share is formed inside the kernel.  For
    eager calls only (``mlp_actor_allowed``)."""

    @staticmethod
    def forward(ctx, *args):
        ctx.hid_grad = True
        return _ActorUnsharedTrainFn.forward(ctx, *args)


def actor_unshared_train(agents, obs, hidden):
    """The node on obs [b, n, obs_dim] / hidden [b, n, 64] (``actor_unshared_supported`` holds): (means, hidden) as [b * n, .].
    For RNNAgentGaussian modules the new hidden state carries the log-std heads' gradient back."""
    agents = list(agents)
    n, o = len(agents), obs.shape[-1]
    agent_id = agents[0].fc1.weight.shape[1] != o
    flat = [p for g in agents for p in _unshared_params(g)]
    node = _ActorUnsharedTrainHidFn if type(agents[0]) is RNNAgentGaussian else _ActorUnsharedTrainFn
    return node.apply(obs.reshape(-1, o), hidden.reshape(-1, 64), n, agent_id, _ln_eps(agents[0]), *flat)


# ---- the per-agent critics of shared_params: False (csrc/critic_unshared.hip) ------------------------------------------------
_CRITIC_UNSHARED_TABLES = ("fc1_w", "fc1_b", "ln_w", "ln_b", "fc2_w", "fc2_b", "fc3_w", "fc3_b")


def _critic_unshared_params(critic):
    """The eight parameters of one MLPCritic in ``_CRITIC_UNSHARED_TABLES`` order (the LayerNorm pair None without layernorm)."""
    ln = critic.layernorm if critic.args.layernorm else None
    return (critic.fc1.weight, critic.fc1.bias, None if ln is None else ln.weight, None if ln is None else ln.bias,
            critic.fc2.weight, critic.fc2.bias, critic.fc3.weight, critic.fc3.bias)


def _critic_unshared_widths(x1, x2, shared):
    """(w1, w2) of the first layer's blocks: x1 [b, n, o] / x2 [b, n, a] (or None) as ONE block per sample (``shared``: every
    agent's critic reads [b, n o] — maddpg.py:33-54, mappo.py:34-62) or as agent i's own row (ippo.py:34-59, iddpg.py:32-59)."""
    n = x1.shape[1]
    w1 = x1.shape[2] * (n if shared else 1)
    w2 = 0 if x2 is None else x2.shape[2] * (n if shared else 1)
    return w1, w2


def _critic_unshared_family(heads):
    """What the two families of per-agent critic kernels differ in on the host — the plain one (``heads`` None,
    csrc/critic_unshared.hip) and MATD3's twins (csrc/critic_unshared_twin.hip): (forward struct, backward struct, the entry
    points' stem, the ``note_fallback`` / ``_scratch`` key, the workspace's floats).  The twins' fc1 has one column more: the flag."""
    if heads is None:
        return (_lib.FlexCriticUnsharedArgs, _lib.FlexCriticUnsharedBwdArgs, "flexnet_critic_unshared", "critic_unshared",
                _lib.FLEXNET_CRITIC_UNSHARED_WS_FLOATS)
    return (_lib.FlexCriticUnsharedTwinArgs, _lib.FlexCriticUnsharedTwinBwdArgs, "flexnet_critic_unshared_twin",
            "critic_unshared_twin", _lib.FLEXNET_CRITIC_UNSHARED_TWIN_WS_FLOATS)


def _critic_unshared_declines(critics, x1, x2, shared, heads=None, names=("x1", "x2")):
    """Why the per-agent critic kernels do not cover these critics on the blocks x1 [b, n, o], x2 [b, n, a] / None
    (csrc/critic_unshared.hip), or — ``heads`` 1 or 2 — why csrc/critic_unshared_twin.hip does not: the same conditions with
    the twin flag's column behind the blocks in fc1, the action block required, the rows counted per head, outside a graph
    capture."""
    n = len(critics)
    flag = int(heads is not None)                    # the twin flag's column behind fc1's blocks
    if flag and x2 is None:
        return f"no {names[1]} block"
    for name, t in zip(names, (x1, x2)):
        if t is not None and not (t.is_cuda and t.dtype == th.float32 and t.dim() == 3 and t.shape[1] == n
                                  and t.shape[0] == x1.shape[0]):
            return f"{name} {tuple(t.shape)} {t.dtype} for {n} agents"
    w1, w2 = _critic_unshared_widths(x1, x2, shared)
    if flag and heads not in (1, 2):
        return f"{heads} heads"
    if not (1 <= n <= _lib.FLEXNET_MAX_AGENTS and 1 <= w1 <= _lib.FLEXNET_MAX_AGENTS * _lib.FLEXNET_MAX_OBS
            and w2 <= _lib.FLEXNET_MAX_AGENTS * _lib.FLEXNET_MAX_ACT and (x2 is None or 1 <= x2.shape[2] <= _lib.FLEXNET_MAX_ACT)):
        return f"agents {n}, first block {w1}, second block {w2}"
    rows = (heads if flag else 1) * x1.shape[0] * n
    if rows >= ACTOR_UNSHARED_MAX_ROWS:
        return f"{rows} rows"
    if flag and (th.cuda.is_current_stream_capturing() or in_graph_audit()):
        return "the entry points are launched eagerly only"
    for i, c in enumerate(critics):
        if type(c) is not MLPCritic:
            return f"critic {i} is a {type(c).__name__}"
        a = c.args
        if not (a.hid_size == 64 and a.hid_activation == "relu" and c.fc3.out_features == 1):
            return f"critic {i}: hid {a.hid_size}, act {a.hid_activation}, out {c.fc3.out_features}"
        if c.fc1.weight.shape[1] not in (w1 + w2 + flag, w1 + n + w2 + flag):
            return (f"critic {i}: fc1 takes {c.fc1.weight.shape[1]} columns, blocks {w1} + {w2}{' + the flag' if flag else ''}, "
                    f"{n} agents")
        if c.fc1.weight.shape[1] != critics[0].fc1.weight.shape[1] or bool(a.layernorm) != bool(critics[0].args.layernorm):
            return f"critic {i} differs from critic 0 in its input width or LayerNorm"
        if not getattr(c, "fused_tail", True):
            return f"critic {i}: fused passes switched off"
        why = _params_decline(_critic_unshared_params(c))
        if why is not None:
            return f"critic {i}: {why}"
    return None


def critic_unshared_supported(critics, x1, x2=None, shared=False, train=False):
    """What csrc/critic_unshared.hip covers: every module ``type(...) is MLPCritic`` with 64 hidden units, ReLU and one output,
    fp32 contiguous device tensors, at most FLEXNET_MAX_AGENTS agents, blocks of at most FLEXNET_MAX_AGENTS * FLEXNET_MAX_OBS
    and FLEXNET_MAX_AGENTS * FLEXNET_MAX_ACT columns; ``train``: also the row threshold of the hand-written weight gradients."""
    critics = list(critics)
    return (_critic_unshared_declines(critics, x1, x2, shared) is None and not x1.requires_grad
            and (not train or x1.shape[0] * x1.shape[1] >= WGRAD_MIN_ROWS))


def _critic_unshared_args(cls, params, x1, x2, shared, ln_eps, heads=None):
    """The head of either family's forward or backward struct ``cls``: the shape, the switches and the pointer tables."""
    b, n, _ = x1.shape
    w1, w2 = _critic_unshared_widths(x1, x2, shared)
    flag = int(heads is not None)
    a = cls()
    a.rows, a.n_agents, a.w1, a.w2 = b * n, n, w1, w2
    if flag:
        a.heads = heads
    a.agent_id, a.layernorm, a.ln_eps = int(params[0][0].shape[1] != w1 + w2 + flag), int(params[0][2] is not None), float(ln_eps)
    _fill_tables(a, _CRITIC_UNSHARED_TABLES, params, n)
    return a


def _critic_unshared_launch_forward(params, x1, x2, shared, ln_eps, saved=None, heads=None):
    """One flexnet_critic_unshared_forward launch on contiguous x1 [b, n, o] / x2 [b, n, a] or None: q [b, n]; or — ``heads``
    1 or 2 — one flexnet_critic_unshared_twin_forward launch: q [heads, b, n].  None when the library answers
    FLEXNET_EUNSUPPORTED.  ``saved`` = (z1 [b n, 64], x [b n, 64] or [heads, b n, 64])."""
    b, n, o = x1.shape
    cls, _, entry = _critic_unshared_family(heads)[:3]
    q = th.empty((b, n) if heads is None else (heads, b, n), dtype=th.float32, device=x1.device)
    a = _critic_unshared_args(cls, params, x1, x2, shared, ln_eps, heads)
    a.x1, a.x1_pitch, a.x1_agent_off = x1.data_ptr(), n * o, 0 if shared else o
    if x2 is not None:
        a.x2, a.x2_pitch, a.x2_agent_off = x2.data_ptr(), n * x2.shape[2], 0 if shared else x2.shape[2]
    a.q = q.data_ptr()
    if saved is not None:
        a.save_z1, a.save_x = saved[0].data_ptr(), saved[1].data_ptr()
    if not _lib.try_launch(entry + "_forward", a):
        return None
    return q


def fused_critic_forward_unshared(critics, x1, x2=None, shared=False):
    """model.py:124-138 (one MLPCritic per agent) without an autograd graph, in ONE HIP launch (csrc/critic_unshared.hip) at
    any batch size, instead of the loop's clone / eye / cat and ten kernels per agent.  ``x1`` [b, n, o] (observations) and
    ``x2`` [b, n, a] (actions) or None are the blocks of the first layer's input, never concatenated: ``shared`` — every agent's
    critic reads all of them ([o_1 .. o_n | onehot(i) | a_1 .. a_n]), else agent i's reads its own ([o_i | onehot(i) | a_i]).
    Returns q [b, n], or None after ``note_fallback("critic_unshared", ...)`` when it declines on GPU tensors."""
    critics = list(critics)
    why = _critic_unshared_declines(critics, x1, x2, shared)

    def launch():
        return _critic_unshared_launch_forward([_critic_unshared_params(c) for c in critics], x1.contiguous(),
                                               None if x2 is None else x2.contiguous(), shared, _ln_eps(critics[0]))
    return _fused_inference("critic_unshared", why, x1.is_cuda, "flexnet_critic_unshared_forward", launch)


class _CriticUnsharedFn(th.autograd.Function):
    """The per-agent critics of ``shared_params: False`` for an update batch as ONE autograd node (csrc/critic_unshared.hip): the
    fused forward with its two saves (fc1's output and the first activation; fc2's output is recomputed), one backward launch
    for dz1, dz2, the per-agent vector sums and the own-action gradient, then ONE flexnet_wgrad_batched call for every agent's
    d_fc1_w (its x1 block and its x2 block as two problems into column slices) and d_fc2_w.  The id block of agent a's fc1
    gradient is zero except its own column a, which is its bias gradient (the one-hot input).  ``x1`` takes no gradient; ``x2``
    takes the gradient of agent i's own action block only — maddpg.py:47-54 detaches the others, iddpg.py has no others.
    ``param_grads`` False: the critics are frozen (the policy sub-update), no parameter gradient is formed.  Bit-reproducible.
    (``ctx.heads``, set by _CriticUnsharedTwinFn alone: the twin family's launches on the same plumbing.)"""

    @staticmethod
    def forward(ctx, x1, x2, shared, ln_eps, param_grads, *flat):
        b, n, _ = x1.shape
        heads = ctx.heads = getattr(ctx, "heads", None)
        params = [flat[8 * i:8 * i + 8] for i in range(n)]
        x1 = x1.contiguous()
        x2 = None if x2 is None else x2.contiguous()
        saved = th.empty(1 + (heads or 1), b * n, 64, dtype=th.float32, device=x1.device)     # z1 | x (per head)
        q = _critic_unshared_launch_forward(params, x1, x2, shared, ln_eps, (saved[0], saved[1:]), heads)
        if q is None:
            _lib.check(_lib.FLEXNET_EUNSUPPORTED, _critic_unshared_family(heads)[2] + "_forward")
        ctx.shared, ctx.ln_eps, ctx.param_grads = bool(shared), float(ln_eps), bool(param_grads)
        ctx.has_ln, ctx.has_x2 = params[0][2] is not None, x2 is not None
        ctx.save_for_backward(x1, saved, *([x2] if x2 is not None else []), *[p for p in flat if p is not None])
        ctx.set_materialize_grads(False)
        return q

    @staticmethod
    def backward(ctx, dq):
        x1, saved = ctx.saved_tensors[:2]
        rest = ctx.saved_tensors[2:]
        x2 = None
        if ctx.has_x2:
            x2, rest = rest[0], rest[1:]
        b, n, _ = x1.shape
        dev, has_ln, shared, heads = x1.device, ctx.has_ln, ctx.shared, ctx.heads
        _, cls, entry, key, ws_floats = _critic_unshared_family(heads)
        flag = int(heads is not None)
        hb = (heads or 1) * b                        # the rows per agent of dz2 and x: [heads, b, n, 64] keeps the pitch 64 n
        params = _regroup_params(rest, n, 8, has_ln)
        if dq is None:
            return (None,) * (5 + 8 * n)
        if flag and th.cuda.is_current_stream_capturing():
            raise RuntimeError(f"{entry}_backward is launched eagerly only")
        rows = b * n
        pg = ctx.param_grads and any(ctx.needs_input_grad[5:])
        want_x2 = x2 is not None and ctx.needs_input_grad[1]
        dq = dq.contiguous()
        dz1 = th.empty(rows, 64, dtype=th.float32, device=dev)                # (the twins': head 0's + head 1's)
        g = _critic_unshared_args(cls, params, x1, x2, shared, ctx.ln_eps, heads)
        g.param_grads = int(pg)
        g.dq, g.z1, g.x = dq.data_ptr(), saved[0].data_ptr(), saved[1].data_ptr()
        setattr(g, "dz1_sum" if flag else "dz1", dz1.data_ptr())
        d_x2 = None
        if want_x2:
            act_dim = x2.shape[2]
            d_x2 = th.empty(b, n, act_dim, dtype=th.float32, device=dev)
            g.d_x2_own, g.own_first, g.own_step, g.own_w = d_x2.data_ptr(), 0, act_dim if shared else 0, act_dim
        if pg:
            dz2 = th.empty(hb * n, 64, dtype=th.float32, device=dev)
            sums = ("d_ln_w", "d_ln_b", "d_fc1_b", "d_fc2_b", "d_fc3_w") + (("d_flag",) if flag else ())
            small = th.empty(len(sums), n, 64, dtype=th.float32, device=dev)
            d_fc3_b = th.empty(n, 1, dtype=th.float32, device=dev)
            ws = _scratch(key, dev, ws_floats)
            g.dz2, g.d_fc3_b = dz2.data_ptr(), d_fc3_b.data_ptr()
            for k, name in enumerate(sums):
                setattr(g, name, small[k].data_ptr())
            g.workspace, g.workspace_floats = ws.data_ptr(), ws.numel()
        _lib.launch(entry + "_backward", g)
        if not pg:
            return (None, d_x2, None, None, None) + (None,) * (8 * n)
        # the weight gradients: per agent d_fc1_w's x1 block and its x2 block from dz1 over the agent's b rows (the twins' heads
        # share the first layer's input), and d_fc2_w over its heads * b rows, each through the row pitch — one
        # flexnet_wgrad_batched call
        w1, w2 = g.w1, g.w2
        ld = params[0][0].shape[1]
        n_id = ld - w1 - w2 - flag
        d_fc1_w = (th.zeros if n_id else th.empty)(n, 64, ld, dtype=th.float32, device=dev)
        d_fc2_w = th.empty(n, 64, 64, dtype=th.float32, device=dev)
        dz1_3, dz2_3, x_3 = dz1.view(b, n, 64), dz2.view(hb, n, 64), saved[1:].view(hb, n, 64)
        problems = []
        for i in range(n):
            problems.append((dz1_3[:, i], x1.view(b, w1) if shared else x1[:, i], d_fc1_w[i, :, :w1], None))
            if x2 is not None:
                problems.append((dz1_3[:, i], x2.view(b, w2) if shared else x2[:, i], d_fc1_w[i, :, w1 + n_id:w1 + n_id + w2], None))
            problems.append((dz2_3[:, i], x_3[:, i], d_fc2_w[i], None))
        tall_wgrad_batched(problems)
        if n_id:
            th.diagonal(d_fc1_w[:, :, w1:w1 + n], dim1=0, dim2=2).copy_(small[2].t())     # [64, n]: agent i's own id column
        if flag:
            d_fc1_w[:, :, ld - 1] = small[5]                                                # the flag column (zero with one head)
        grads = []
        for i in range(n):
            grads += [d_fc1_w[i], small[2, i], small[0, i] if has_ln else None, small[1, i] if has_ln else None,
                      d_fc2_w[i], small[3, i], small[4, i].view(1, 64), d_fc3_b[i]]
        return (None, d_x2, None, None, None, *grads)


def critic_unshared_train(critics, x1, x2=None, shared=False, param_grads=True):
    """The node on the blocks x1 [b, n, o] / x2 [b, n, a] or None (``critic_unshared_supported(..., train=True)`` holds): q [b, n]."""
    critics = list(critics)
    flat = [p for c in critics for p in _critic_unshared_params(c)]
    return _CriticUnsharedFn.apply(x1, x2, shared, _ln_eps(critics[0]), param_grads, *flat)


# ---- MATD3's per-agent twin critics of shared_params: False (csrc/critic_unshared_twin.hip): eager calls only -------------------
# The checks, the launch and the node are the plain family's above with ``heads`` set: obs / act are maddpg.py's shared blocks.
def critic_unshared_twin_supported(critics, obs, act, heads=2, train=False):
    """What csrc/critic_unshared_twin.hip covers: ``critic_unshared_supported``'s conditions on the blocks obs [b, n, o] (shared)
    and act [b, n, a] (shared), fc1 taking the flag column behind them, outside a graph capture; ``train``: also the row
    threshold of the hand-written weight gradients."""
    critics = list(critics)
    return (_critic_unshared_declines(critics, obs, act, True, heads, ("obs", "act")) is None and not obs.requires_grad
            and (not train or obs.shape[0] * obs.shape[1] >= WGRAD_MIN_ROWS))


def fused_critic_forward_unshared_twin(critics, obs, act, heads=2):
    """matd3.py:74-82 (agent i's own critic on its row, the twin flag at 0 and at 1) without an autograd graph, in ONE HIP
    launch (csrc/critic_unshared_twin.hip) at any batch size: the first layer is formed once per row and the second head adds
    fc1.weight's last column.  ``obs`` [b, n, o], ``act`` [b, n, a].  Returns q [heads, b, n] — cat([Q1, Q2], 0) — or None
    after ``note_fallback("critic_unshared_twin", ...)`` when it declines on GPU tensors."""
    critics = list(critics)
    why = _critic_unshared_declines(critics, obs, act, True, heads, ("obs", "act")) if obs.is_cuda else "CPU tensors"

    def launch():
        return _critic_unshared_launch_forward([_critic_unshared_params(c) for c in critics], obs.contiguous(), act.contiguous(),
                                               True, _ln_eps(critics[0]), heads=heads)
    return _fused_inference("critic_unshared_twin", why, obs.is_cuda, "flexnet_critic_unshared_twin_forward", launch)


class _CriticUnsharedTwinFn(_CriticUnsharedFn):
    """MATD3's per-agent twin critics for an update batch as ONE autograd node (csrc/critic_unshared_twin.hip), on
    _CriticUnsharedFn's plumbing: the fused forward with its saves (fc1's output once, the first activation per head), the
    backward launches for dz1_sum, dz2, the per-agent vector sums, the flag column's gradient and the own-action gradient, then
    ONE flexnet_wgrad_batched call: per agent d_fc1_w's obs block and action block from dz1_sum (both heads share the first
    layer's input), and d_fc2_w as one problem of heads * b rows.  The id block of agent a's fc1 gradient is zero except its
    own column a, which is its bias gradient; its flag column is d_flag[a].  ``obs`` takes no gradient; ``act`` takes the
    gradient of agent i's own action block through the FIRST head only — with heads = 2 and an action that requires a gradient
    the node refuses.  ``param_grads`` False: the critics are frozen (the policy sub-update).  For eager calls only.
    Bit-reproducible."""

    @staticmethod
    def forward(ctx, obs, act, heads, ln_eps, param_grads, *flat):
        ctx.heads = int(heads)
        return _CriticUnsharedFn.forward(ctx, obs, act, True, ln_eps, param_grads, *flat)


def critic_unshared_twin_train(critics, obs, act, heads=2, param_grads=True):
    """The node on obs [b, n, o] / act [b, n, a] (``critic_unshared_twin_supported(..., train=True)`` holds): q [heads, b, n]."""
    critics = list(critics)
    if heads == 2 and act.requires_grad:
        raise RuntimeError("critic_unshared_twin_train: the action gradient is the first head's (heads = 1)")
    flat = [p for c in critics for p in _critic_unshared_params(c)]
    return _CriticUnsharedTwinFn.apply(obs, act, heads, _ln_eps(critics[0]), param_grads, *flat)


# ---- the MLP actor of agent_type mlp under shared_params (csrc/actor_mlp.hip): eager calls only --------------------------------
def mlp_actor_allowed():
    """The capture rule of csrc/actor_mlp.hip: its entry points are launched eagerly only.  False while the
    current stream is capturing a HIP graph and while ``util.audit_graph_body`` runs a body on behalf of a capture site (the
    audit must see what the capture will see); the MLP agent then runs the tensor composition, silently — nothing is
    misconfigured.  Both the inference launch and the training node consult this one function."""
    return not (in_graph_audit() or th.cuda.is_current_stream_capturing())


def _actor_mlp_params(agent):
    """The eight parameters of an MLPAgent in FlexActorMlpArgs order (the LayerNorm pair None without layernorm; the Gaussian
    agent's ``mean`` head in the fc3 slot, through its class property)."""
    ln = agent.layernorm if agent.args.layernorm else None
    return (agent.fc1.weight, agent.fc1.bias, None if ln is None else ln.weight, None if ln is None else ln.bias,
            agent.fc2.weight, agent.fc2.bias, agent.fc3.weight, agent.fc3.bias)


def actor_mlp_declines(agent, obs, n_agents, agent_id):
    """Why csrc/actor_mlp.hip does not cover ``agent`` on ``obs`` [b, n, obs_dim] / [b * n, obs_dim] (no id columns), or None."""
    if type(agent) not in (MLPAgent, MLPAgentGaussian):
        return f"a {type(agent).__name__}"
    a, o = agent.args, obs.shape[-1]
    if not (obs.is_cuda and obs.dtype == th.float32 and obs.dim() in (2, 3)):
        return f"obs {tuple(obs.shape)} {obs.dtype} on {obs.device.type}"
    if not (a.hid_size == _lib.FLEXNET_HID and a.hid_activation == "relu"):
        return f"hid {a.hid_size}, act {a.hid_activation}"
    if not (1 <= o <= _lib.FLEXNET_MAX_OBS and 1 <= n_agents <= _lib.FLEXNET_MAX_AGENTS and 1 <= a.action_dim <= _lib.FLEXNET_MAX_ACT):
        return f"obs {o}, agents {n_agents}, actions {a.action_dim}"
    rows = obs.numel() // o
    if rows % n_agents != 0 or rows >= ACTOR_UNSHARED_MAX_ROWS or (obs.dim() == 3 and obs.shape[1] != n_agents):
        return f"obs {tuple(obs.shape)} for {n_agents} agents"
    if agent.fc1.weight.shape[1] != o + (n_agents if agent_id else 0):
        return f"fc1 takes {agent.fc1.weight.shape[1]} columns, obs {o}, agent_id {bool(agent_id)}"
    return _params_decline(_actor_mlp_params(agent))


def actor_mlp_supported(agent, obs, n_agents, agent_id):
    """What csrc/actor_mlp.hip covers: ``type(agent)`` MLPAgent or MLPAgentGaussian with 64 hidden units and ReLU, fp32
    contiguous device tensors, obs_dim <= 144, at most 8 agents and 8 actions, fc1 of obs_dim (+ n) columns."""
    return actor_mlp_declines(agent, obs, n_agents, agent_id) is None


def _actor_mlp_head(cls, rows, n, o, act_dim, agent_id, ln_w, ln_eps):
    if not mlp_actor_allowed():
        raise RuntimeError("csrc/actor_mlp.hip is launched eagerly only (nets.mlp_actor_allowed): never under a capture")
    a = cls()
    a.rows, a.n_agents, a.obs_dim, a.act_dim, a.hid = rows, n, o, act_dim, _lib.FLEXNET_HID
    a.agent_id, a.layernorm, a.ln_eps = int(bool(agent_id)), int(ln_w is not None), float(ln_eps)
    return a


def _actor_mlp_launch_forward(params, obs, n, agent_id, ln_eps, saved=None):
    """One flexnet_actor_mlp_forward launch on contiguous obs [rows, o]: (means [rows, a], h [rows, 64]), or None when the
    library answers FLEXNET_EUNSUPPORTED."""
    rows, o = obs.shape
    act_dim = params[6].shape[0]
    means = th.empty(rows, act_dim, dtype=th.float32, device=obs.device)
    h = th.empty(rows, 64, dtype=th.float32, device=obs.device)
    a = _actor_mlp_head(_lib.FlexActorMlpArgs, rows, n, o, act_dim, agent_id, params[2], ln_eps)
    for name, p in zip(("fc1_w", "fc1_b", "ln_w", "ln_b", "fc2_w", "fc2_b", "fc3_w", "fc3_b"), params):
        setattr(a, name, None if p is None else p.data_ptr())
    a.obs, a.means, a.h = obs.data_ptr(), means.data_ptr(), h.data_ptr()
    if saved is not None:
        a.save_z1, a.save_x = saved[0].data_ptr(), saved[1].data_ptr()
    if not _lib.try_launch("flexnet_actor_mlp_forward", a):
        return None
    return means, h


def fused_actor_forward_mlp(agent, obs, n_agents, agent_id):
    """mlp_agent.py:20-32 + model.py:102-116 without an autograd graph, in ONE HIP launch (csrc/actor_mlp.hip) at any batch
    size, instead of the module's ten kernels.  ``obs`` [b, n, obs_dim] WITHOUT the one-hot id columns (the kernel adds fc1's id
    column of row r % n itself).  Returns (means [b * n, act], h [b * n, 64]), or None after ``note_fallback("actor_forward",
    ...)`` when it declines on GPU tensors.  Never called under a capture (``mlp_actor_allowed``)."""
    why = actor_mlp_declines(agent, obs, n_agents, agent_id)

    def launch():
        return _actor_mlp_launch_forward(_actor_mlp_params(agent), obs.reshape(-1, obs.shape[-1]).contiguous(), n_agents, agent_id,
                                         _ln_eps(agent))
    return _fused_inference("actor_forward", why, obs.is_cuda, "flexnet_actor_mlp_forward", launch)


def mlp_burst_declines(agent, n_agents, obs_dim, agent_id):
    """Why the burst's MLP policy phase (csrc/actor_r16.h: actor_r16_burst's MLP) does not cover the shared ``agent``, or None."""
    if type(agent) not in (MLPAgent, MLPAgentGaussian):
        return f"a {type(agent).__name__}"
    a = agent.args
    if not (a.hid_size == _lib.FLEXNET_HID and a.hid_activation == "relu"):
        return f"hid {a.hid_size}, act {a.hid_activation}"
    if agent.fc1.weight.shape[1] != obs_dim + (n_agents if agent_id else 0):
        return f"fc1 takes {agent.fc1.weight.shape[1]} columns, obs {obs_dim}, agent_id {bool(agent_id)}"
    return _params_decline(_actor_mlp_params(agent))


def _mlp_launch_args(agent, n_envs, n_agents, obs_dim, agent_id, outputs):
    """What the MLP forms of the persistent launches share: ``mlp_burst_declines`` (raises on a reason — the caller admitted the
    configuration, and there is no other form to fall back to), a FlexActorArgs with the shapes, the first layer, the LayerNorm
    pair, the output head (``fc3``, the Gaussian agent's ``mean``) in the fc2 slot and ``outputs`` (name -> contiguous tensor),
    no GRU tensors and no ``hidden_in``; and the FlexBurstMlp with the second layer."""
    why = mlp_burst_declines(agent, n_agents, obs_dim, agent_id)
    if why is not None:
        raise RuntimeError(f"the burst's MLP policy does not cover this agent: {why}")
    fc1_w, fc1_b, ln_w, ln_b, fc2_w, fc2_b, head_w, head_b = _actor_mlp_params(agent)
    args = _lib.FlexActorArgs()
    args.rows, args.n_agents, args.obs_dim, args.act_dim = n_envs * n_agents, n_agents, obs_dim, agent.args.action_dim
    args.agent_id, args.layernorm, args.ln_eps = int(bool(agent_id)), int(ln_w is not None), _ln_eps(agent)
    for name, t in (("fc1_w", fc1_w), ("fc1_b", fc1_b), ("ln_w", ln_w), ("ln_b", ln_b), ("fc2_w", head_w), ("fc2_b", head_b),
                    *outputs.items()):
        if t is not None and not t.is_contiguous():
            raise RuntimeError(f"the burst's MLP policy: non-contiguous {name}")
        setattr(args, name, None if t is None else t.data_ptr())
    mlp = _lib.FlexBurstMlp()
    mlp.fc2_w, mlp.fc2_b = fc2_w.data_ptr(), fc2_b.data_ptr()
    return args, mlp


def mlp_burst_actor_args(agent, n_envs, n_agents, obs_dim, agent_id, ring_cursor, cursor_out, obs_source, ring_slabs, hidden_out,
                         means, rng_state=None, std=None, action_low=None, action_high=None):
    """The ring-form FlexActorArgs of the rollout burst for a shared MLPAgent (include/flexenv.h:
    flexenv_rollout_burst_summed_mlp) — the sibling of what ``fused_actor_forward(..., launch=...)`` fills for the RNN agent:
    same ring, cursor and ``obs_source`` fields, the output head (``fc3``, the Gaussian agent's ``mean``) in the fc2 slot, no GRU
    tensors and no ``hidden_in``.  ``rng_state`` (with ``std``, ``action_low``, ``action_high``): what the exploration epilogue
    of flexenv_rollout_burst_mlp needs — the noise stream's [seed, step] cell, the fixed std and the action range; the agent-summed
    forms leave them out.  Returns (args, FlexBurstMlp with the second layer).  Raises when the agent is outside what
    the launch covers: the caller admitted the configuration, and there is no other form to fall back to."""
    args, mlp = _mlp_launch_args(agent, n_envs, n_agents, obs_dim, agent_id, dict(means=means, hidden_out=hidden_out))
    args.cursor, args.cursor_out = ring_cursor.data_ptr(), cursor_out.data_ptr()
    args.obs_slab_stride, args.hid_slab_stride, args.ring_slabs = 0, 0, int(ring_slabs)
    args.obs, args.obs_pushed = obs_source.ring, obs_source.pushed
    args.obs_row_stride, args.obs_pushed_stride = obs_source.row_stride, obs_source.pushed_stride
    args.obs_slots, args.obs_slot_w = obs_source.slots, obs_source.slot_w
    if rng_state is not None:
        if not (rng_state.dtype == th.int64 and rng_state.numel() == 2 and rng_state.is_contiguous()):
            raise ValueError("rng_state must be a contiguous int64 tensor [seed, step]")
        if std is None or action_low is None or action_high is None:
            raise ValueError("the exploration epilogue needs std, action_low and action_high next to rng_state")
        args.rng_state = rng_state.data_ptr()
        args.std, args.action_low, args.action_high = float(std), float(action_low), float(action_high)
    return args, mlp


def mlp_test_actor_args(agent, n_envs, n_agents, obs_dim, agent_id, hidden_out, means, action, env_action, action_low, action_high):
    """The test-form FlexActorArgs of flexenv_test_episodes_mlp for a shared MLPAgent / MLPAgentGaussian (include/flexenv.h):
    the policy of ``mlp_burst_actor_args`` — same checks, the output head in the fc2 slot, no GRU tensors, no ``hidden_in`` —
    without ring, cursor cells and noise stream (the launch reads the observation in place from the environment's own
    history), with the four tensors every step writes: ``means`` / ``action`` / ``env_action`` [rows, act_dim] and ``hidden_out``
    [rows, 64], and the action range of the test epilogue.  Returns (args, FlexBurstMlp with the second layer); raises as
    ``mlp_burst_actor_args`` does."""
    why = mlp_burst_declines(agent, n_agents, obs_dim, agent_id)          # (first: an agent outside the launch, whatever the tensors)
    if why is not None:
        raise RuntimeError(f"the burst's MLP policy does not cover this agent: {why}")
    rows, a = n_envs * n_agents, agent.args.action_dim
    for name, t, w in (("hidden_out", hidden_out, _lib.FLEXNET_HID), ("means", means, a), ("action", action, a),
                       ("env_action", env_action, a)):
        if not (t.is_cuda and t.dtype == th.float32 and t.numel() == rows * w):
            raise ValueError(f"mlp_test_actor_args: {name} must be an fp32 device tensor of {rows * w} elements")
    args, mlp = _mlp_launch_args(agent, n_envs, n_agents, obs_dim, agent_id,
                                 dict(means=means, hidden_out=hidden_out, action=action, env_action=env_action))
    args.std, args.action_low, args.action_high = 0.0, float(action_low), float(action_high)
    return args, mlp


def _actor_mlp_node_forward(ctx, launch_forward, entry, params, keep, obs, n_agents, agent_id, ln_eps, hid_grad):
    """What the ``forward`` of the two MLP-actor nodes share: ``launch_forward`` (``_actor_mlp_launch_forward`` or its per-agent
    form, whose entry point is ``entry``) on ``params`` with the saves z1 | x, then the bookkeeping — obs, h, the saves and
    ``keep`` (the weights the backward reads) saved, h non-differentiable unless ``hid_grad``, no zero-filled gradients."""
    obs = obs.contiguous()
    saved = th.empty(2, obs.shape[0], 64, dtype=th.float32, device=obs.device)               # z1 | x
    out = launch_forward(params, obs, n_agents, agent_id, ln_eps, saved)
    if out is None:
        _lib.check(_lib.FLEXNET_EUNSUPPORTED, entry)
    means, h = out
    ctx.n_agents, ctx.agent_id, ctx.ln_eps = n_agents, bool(agent_id), float(ln_eps)
    ctx.save_for_backward(obs, h, saved, *keep)
    if not hid_grad:
        ctx.mark_non_differentiable(h)
    ctx.set_materialize_grads(False)
    return means, h


def _actor_mlp_node_backward_args(cls, ctx, ws, act_dim, ln_w, d_means, d_h):
    """What the ``backward`` of the two MLP-actor nodes share: d_means made dense (zeros where only h took a gradient), dz1 | dz2
    allocated, and ``cls`` (FlexActorMlpBwdArgs or its per-agent form) filled up to the weight pointers and the vector sums'
    outputs, which differ: the sizes and switches, d_means, the optional d_h, the three saves, dz1, dz2 and the workspace
    ``ws``.  Returns (args, d_means, dz, d_h); the caller holds d_h until the launch."""
    obs, h, saved = ctx.saved_tensors[:3]
    rows, o = obs.shape
    dev = obs.device
    d_means = th.zeros(rows, act_dim, dtype=th.float32, device=dev) if d_means is None else d_means.contiguous()
    dz = th.empty(2, rows, 64, dtype=th.float32, device=dev)                               # dz1 | dz2
    g = _actor_mlp_head(cls, rows, ctx.n_agents, o, act_dim, ctx.agent_id, ln_w, ctx.ln_eps)
    g.d_means, g.z1, g.x, g.h = d_means.data_ptr(), saved[0].data_ptr(), saved[1].data_ptr(), h.data_ptr()
    if d_h is not None:
        d_h = d_h.contiguous()
        g.d_h = d_h.data_ptr()
    g.dz1, g.dz2 = dz[0].data_ptr(), dz[1].data_ptr()
    g.workspace, g.workspace_floats = ws.data_ptr(), ws.numel()
    return g, d_means, dz, d_h


class _ActorMlpTrainFn(th.autograd.Function):
    """The MLP actor of ``agent_type: mlp`` for an update batch as ONE autograd node (csrc/actor_mlp.hip): the fused forward with
    its saves (z1, x; h is its second result), one backward launch for dz1, dz2 and every vector sum, then ONE
    flexnet_wgrad_batched call for d_fc1_w's observation block, d_fc2_w and d_fc3_w.  The id block of fc1's gradient is the
    per-agent sums of dz1.  ``hid_grad``: h takes a gradient too (the Gaussian agent's log-std head reads it; the mean head's
    share is formed inside the kernel), else it is non-differentiable.  Observations take no gradient.  Bit-reproducible."""

    @staticmethod
    def forward(ctx, obs, n_agents, agent_id, ln_eps, hid_grad, fc1_w, fc1_b, ln_w, ln_b, fc2_w, fc2_b, fc3_w, fc3_b):
        return _actor_mlp_node_forward(ctx, _actor_mlp_launch_forward, "flexnet_actor_mlp_forward",
                                       (fc1_w, fc1_b, ln_w, ln_b, fc2_w, fc2_b, fc3_w, fc3_b), (fc1_w, ln_w, fc2_w, fc3_w),
                                       obs, n_agents, agent_id, ln_eps, hid_grad)

    @staticmethod
    def backward(ctx, d_means, d_h):
        obs, h, saved, fc1_w, ln_w, fc2_w, fc3_w = ctx.saved_tensors
        if d_means is None and d_h is None:
            return (None,) * 13
        o = obs.shape[1]
        n, dev, act_dim, has_ln = ctx.n_agents, obs.device, fc3_w.shape[0], ln_w is not None
        small = th.empty(4, 64, dtype=th.float32, device=dev)                              # d_ln_w | d_ln_b | d_fc1_b | d_fc2_b
        d_fc3_b = th.empty(act_dim, dtype=th.float32, device=dev)
        d_id = th.empty(n, 64, dtype=th.float32, device=dev)
        ws = _scratch("actor_mlp", dev, _lib.FLEXNET_ACTOR_MLP_WS_FLOATS)
        g, d_means, dz, d_h = _actor_mlp_node_backward_args(_lib.FlexActorMlpBwdArgs, ctx, ws, act_dim, ln_w, d_means, d_h)
        g.fc2_w, g.fc3_w = fc2_w.data_ptr(), fc3_w.data_ptr()
        if has_ln:
            g.ln_w, g.d_ln_w, g.d_ln_b = ln_w.data_ptr(), small[0].data_ptr(), small[1].data_ptr()
        g.d_fc1_b, g.d_fc2_b, g.d_fc3_b, g.d_dz1_agent = small[2].data_ptr(), small[3].data_ptr(), d_fc3_b.data_ptr(), d_id.data_ptr()
        _lib.launch("flexnet_actor_mlp_backward", g)
        d_fc1_w = th.empty_like(fc1_w)
        d_fc2_w = th.empty_like(fc2_w)
        d_fc3_w = th.empty_like(fc3_w)
        tall_wgrad_batched([(dz[0], obs, d_fc1_w[:, :o], None), (dz[1], saved[1], d_fc2_w, None), (d_means, h, d_fc3_w, None)])
        if ctx.agent_id:
            d_fc1_w[:, o:] = d_id.t()
        return (None, None, None, None, None, d_fc1_w, small[2], small[0] if has_ln else None, small[1] if has_ln else None,
                d_fc2_w, small[3], d_fc3_w, d_fc3_b)


def actor_mlp_train(agent, obs, n_agents, agent_id):
    """The node on obs [b, n, obs_dim] / [b * n, obs_dim] (``actor_mlp_supported`` holds, ``mlp_actor_allowed()``, obs takes no
    gradient): (means [b * n, act], h [b * n, 64]); for the Gaussian agent h carries the log-std head's gradient back."""
    return _ActorMlpTrainFn.apply(obs.reshape(-1, obs.shape[-1]), n_agents, bool(agent_id), _ln_eps(agent),
                                  type(agent) is MLPAgentGaussian, *_actor_mlp_params(agent))


# ---- the MLP actors of agent_type mlp under shared_params False (csrc/actor_mlp.hip's per-agent form): eager calls only -------
_ACTOR_MLP_TABLES = ("fc1_w", "fc1_b", "ln_w", "ln_b", "fc2_w", "fc2_b", "fc3_w", "fc3_b")


def _one_configuration(agents):
    """None when every agent is of agent 0's class and configuration (the kernels take ONE set of sizes and switches), else why
    not."""
    first = agents[0]
    a0 = first.args

    def key(g):
        a = g.args
        eps = float(g.layernorm.eps) if a.layernorm else None
        return (a.hid_size, a.hid_activation, bool(a.layernorm), eps, a.action_dim, tuple(g.fc1.weight.shape),
                getattr(a, "LOG_STD_MIN", None), getattr(a, "LOG_STD_MAX", None))
    for i, g in enumerate(agents):
        if type(g) is not type(first):
            return f"agent {i} is a {type(g).__name__}, agent 0 a {type(first).__name__}"
        if g.args is not a0 and key(g) != key(first):
            return f"agent {i} is configured unlike agent 0"
    return None


def actor_mlp_unshared_declines(agents, obs, agent_id):
    """Why csrc/actor_mlp.hip's per-agent form does not cover these per-agent MLP actors on ``obs`` [b, n, obs_dim] (no id columns), or
    None: ``actor_mlp_declines``'s predicates for every agent, and all agents of one class and one configuration."""
    agents = list(agents)
    n = len(agents)
    if not (obs.dim() == 3 and obs.shape[1] == n):
        return f"obs {tuple(obs.shape)} for {n} agents"
    why = _one_configuration(agents)
    if why is not None:
        return why
    for i, g in enumerate(agents):
        why = actor_mlp_declines(g, obs, n, agent_id)
        if why is not None:
            return f"agent {i}: {why}"
    return None


def actor_mlp_unshared_supported(agents, obs, agent_id):
    """What csrc/actor_mlp.hip's per-agent form covers: ``actor_mlp_supported`` for every agent, all of one class and configuration."""
    return actor_mlp_unshared_declines(agents, obs, agent_id) is None


def _actor_mlp_unshared_launch_forward(params, obs, n, agent_id, ln_eps, saved=None):
    """One flexnet_actor_mlp_unshared_forward launch on contiguous obs [rows, o]: (means [rows, a], h [rows, 64]), or None when
    the library answers FLEXNET_EUNSUPPORTED.  ``params``: per agent, the eight tensors in ``_ACTOR_MLP_TABLES`` order."""
    rows, o = obs.shape
    act_dim = params[0][6].shape[0]
    means = th.empty(rows, act_dim, dtype=th.float32, device=obs.device)
    h = th.empty(rows, 64, dtype=th.float32, device=obs.device)
    a = _actor_mlp_head(_lib.FlexActorMlpUnsharedArgs, rows, n, o, act_dim, agent_id, params[0][2], ln_eps)
    _fill_tables(a, _ACTOR_MLP_TABLES, params, n)
    a.obs, a.means, a.h = obs.data_ptr(), means.data_ptr(), h.data_ptr()
    if saved is not None:
        a.save_z1, a.save_x = saved[0].data_ptr(), saved[1].data_ptr()
    if not _lib.try_launch("flexnet_actor_mlp_unshared_forward", a):
        return None
    return means, h


def fused_actor_forward_mlp_unshared(agents, obs):
    """model.py:124-138 with one MLPAgent (or MLPAgentGaussian) per agent, without an autograd graph, in ONE HIP launch
    (csrc/actor_mlp.hip's per-agent form) instead of the loop's ten kernels per agent.  ``obs`` [b, n, obs_dim] WITHOUT the one-hot id
    columns (agent i's own id column of its fc1 is added by the kernel).  Returns (means [b * n, act], h [b * n, 64]), or None
    after ``note_fallback("actor_mlp_unshared", ...)`` when it declines on GPU tensors.  Never called under a capture
    (``mlp_actor_allowed``)."""
    agents = list(agents)
    n, o = len(agents), obs.shape[-1]
    agent_id = agents[0].fc1.weight.shape[1] != o
    why = actor_mlp_unshared_declines(agents, obs, agent_id)

    def launch():
        return _actor_mlp_unshared_launch_forward([_actor_mlp_params(g) for g in agents], obs.reshape(-1, o).contiguous(), n,
                                                  agent_id, _ln_eps(agents[0]))
    return _fused_inference("actor_mlp_unshared", why, obs.is_cuda, "flexnet_actor_mlp_unshared_forward", launch)


class _ActorMlpUnsharedTrainFn(th.autograd.Function):
    """The per-agent MLP actors of ``shared_params: False`` for an update batch as ONE autograd node over all agents' parameters
    (csrc/actor_mlp.hip's per-agent form): the fused forward with its saves (z1, x; h is its second result), one backward launch for
    dz1, dz2 and every agent's vector sums, then the 3 n weight gradients — per agent d_fc1_w's observation block, d_fc2_w and
    d_fc3_w over the agent's rows through the row pitch — as ONE flexnet_wgrad_batched call.  The id block of agent a's fc1
    gradient is zero except its own column a, which is its bias gradient (the one-hot input).  ``hid_grad``: h takes a gradient
    too (the Gaussian agents' log-std heads read it), else it is non-differentiable.  Observations take no gradient.
    Bit-reproducible."""

    @staticmethod
    def forward(ctx, obs, n_agents, agent_id, ln_eps, hid_grad, *flat):
        params = [flat[8 * i:8 * i + 8] for i in range(n_agents)]
        ctx.has_ln = params[0][2] is not None
        keep = [p for q in params for p in (q[0], q[2], q[4], q[6]) if p is not None]        # fc1_w, ln_w, fc2_w, fc3_w
        return _actor_mlp_node_forward(ctx, _actor_mlp_unshared_launch_forward, "flexnet_actor_mlp_unshared_forward",
                                       params, keep, obs, n_agents, agent_id, ln_eps, hid_grad)

    @staticmethod
    def backward(ctx, d_means, d_h):
        obs, h, saved = ctx.saved_tensors[:3]
        n, dev, has_ln = ctx.n_agents, obs.device, ctx.has_ln
        if d_means is None and d_h is None:
            return (None,) * (5 + 8 * n)
        kept = _regroup_params(ctx.saved_tensors[3:], n, 4, has_ln, ln_slots=(1,))           # fc1_w, ln_w, fc2_w, fc3_w
        rows, o = obs.shape
        b, act_dim, ld = rows // n, kept[0][3].shape[0], kept[0][0].shape[1]
        small = th.empty(4, n, 64, dtype=th.float32, device=dev)                           # d_ln_w | d_ln_b | d_fc1_b | d_fc2_b
        d_fc3_b = th.empty(n, act_dim, dtype=th.float32, device=dev)
        ws = _scratch("actor_mlp_unshared", dev, _lib.FLEXNET_ACTOR_MLP_UNSHARED_WS_FLOATS)
        g, d_means, dz, d_h = _actor_mlp_node_backward_args(_lib.FlexActorMlpUnsharedBwdArgs, ctx, ws, act_dim, kept[0][1],
                                                            d_means, d_h)
        _fill_tables(g, ("fc1_w", "ln_w", "fc2_w", "fc3_w"), kept, n)                      # (the backward has no fc1_w table)
        if has_ln:
            g.d_ln_w, g.d_ln_b = small[0].data_ptr(), small[1].data_ptr()
        g.d_fc1_b, g.d_fc2_b, g.d_fc3_b = small[2].data_ptr(), small[3].data_ptr(), d_fc3_b.data_ptr()
        _lib.launch("flexnet_actor_mlp_unshared_backward", g)
        d_fc1_w = (th.zeros if ctx.agent_id else th.empty)(n, 64, ld, dtype=th.float32, device=dev)
        d_fc2_w = th.empty(n, 64, 64, dtype=th.float32, device=dev)
        d_fc3_w = th.empty(n, act_dim, 64, dtype=th.float32, device=dev)
        obs3, h3, x3 = obs.view(b, n, o), h.view(b, n, 64), saved[1].view(b, n, 64)
        dm3, dz1_3, dz2_3 = d_means.view(b, n, act_dim), dz[0].view(b, n, 64), dz[1].view(b, n, 64)
        problems = []
        for i in range(n):
            problems += [(dz1_3[:, i], obs3[:, i], d_fc1_w[i, :, :o], None), (dz2_3[:, i], x3[:, i], d_fc2_w[i], None),
                         (dm3[:, i], h3[:, i], d_fc3_w[i], None)]
        tall_wgrad_batched(problems)                                                       # 3 n <= 24 problems: one call
        if ctx.agent_id:
            th.diagonal(d_fc1_w[:, :, o:], dim1=0, dim2=2).copy_(small[2].t())             # [64, n]: agent i's own id column
        grads = []
        for i in range(n):
            grads += [d_fc1_w[i], small[2, i], small[0, i] if has_ln else None, small[1, i] if has_ln else None,
                      d_fc2_w[i], small[3, i], d_fc3_w[i], d_fc3_b[i]]
        return (None, None, None, None, None, *grads)


def actor_mlp_unshared_train(agents, obs):
    """The node on obs [b, n, obs_dim] (``actor_mlp_unshared_supported`` holds, ``mlp_actor_allowed()``, obs takes no gradient):
    (means [b * n, act], h [b * n, 64]); for the Gaussian agents h carries the log-std heads' gradient back."""
    agents = list(agents)
    n, o = len(agents), obs.shape[-1]
    agent_id = agents[0].fc1.weight.shape[1] != o
    flat = [p for g in agents for p in _actor_mlp_params(g)]
    return _ActorMlpUnsharedTrainFn.apply(obs.reshape(-1, o), n, agent_id, _ln_eps(agents[0]),
                                          type(agents[0]) is MLPAgentGaussian, *flat)


# ---- every agent's own log-std head under shared_params False (csrc/gauss.hip): eager calls only -------------------------------
def gauss_head_unshared_declines(agents, h):
    """Why flexnet_gauss_head_unshared_* does not cover the ``log_std`` heads of these per-agent Gaussian agents on ``h``
    [b * n, 64], or None: ``gauss_log_std``'s predicates for every head, and all agents of one class and configuration."""
    agents = list(agents)
    n = len(agents)
    if not all(type(g) in (RNNAgentGaussian, MLPAgentGaussian) for g in agents):
        return "an agent without a log_std head"
    why = _one_configuration(agents)
    if why is not None:
        return why
    if not (h.is_cuda and h.dtype == th.float32 and h.dim() == 2 and h.shape[1] == _lib.FLEXNET_HID and h.shape[0] % n == 0
            and 1 <= n <= _lib.FLEXNET_MAX_AGENTS and h.shape[0] <= (1 << 30)):
        return f"h {tuple(h.shape)} {h.dtype} on {h.device.type} for {n} agents"
    for i, g in enumerate(agents):
        w, b = g.log_std.weight, g.log_std.bias
        if not (w.shape[1] == _lib.FLEXNET_HID and 1 <= w.shape[0] <= _lib.FLEXNET_MAX_ACT):
            return f"agent {i}: hid {w.shape[1]}, act_dim {w.shape[0]}"
        why = _params_decline((w, b))
        if why is not None:
            return f"agent {i}: {why}"
    return None


def gauss_head_unshared_supported(agents, h):
    return gauss_head_unshared_declines(agents, h) is None


def _gauss_head_unshared_args(rows, n, ws, lo, hi):
    if not mlp_actor_allowed():
        raise RuntimeError("flexnet_gauss_head_unshared_* are launched eagerly only (nets.mlp_actor_allowed): never under a capture")
    a = _gauss_head_fill(_lib.FlexGaussHeadUnsharedArgs(), rows, ws[0], lo, hi)
    a.n_agents = n
    for i in range(n):
        a.w[i] = ws[i].data_ptr()
    return a


class _GaussHeadUnsharedFn(th.autograd.Function):
    """The log-std heads of per-agent Gaussian agents (RNN or MLP) on the actors' ``h`` [b * n, 64] as ONE node: row r uses agent
    r % n's head; csrc/gauss.hip's per-agent kernels both ways, and every head's weight and bias gradient — d_u^T h and d_u's
    column sums over the agent's rows through the row pitch — as the n problems of one flexnet_wgrad_batched call.
    Bit-reproducible."""

    @staticmethod
    def forward(ctx, h, n_agents, lo, hi, *flat):
        h = h.contiguous()
        ws, bs = flat[0::2], flat[1::2]
        rows, na = h.shape[0], ws[0].shape[0]
        log_std = th.empty(rows, na, dtype=th.float32, device=h.device)
        want_t = any(ctx.needs_input_grad)
        t = th.empty_like(log_std) if want_t else None
        a = _gauss_head_unshared_args(rows, n_agents, ws, lo, hi)
        for i in range(n_agents):
            a.b[i] = bs[i].data_ptr()
        a.h, a.log_std = h.data_ptr(), log_std.data_ptr()
        if t is not None:
            a.t = t.data_ptr()
        _lib.launch("flexnet_gauss_head_unshared_forward", a)
        if t is not None:
            ctx.save_for_backward(h, t, *ws)
        ctx.n_agents, ctx.lo, ctx.hi = n_agents, float(lo), float(hi)
        return log_std

    @staticmethod
    def backward(ctx, d_log_std):
        h, t = ctx.saved_tensors[:2]
        ws = ctx.saved_tensors[2:]
        n, rows, na, dev = ctx.n_agents, t.shape[0], t.shape[1], t.device
        d_u, d_h = _gauss_head_backward_launch("flexnet_gauss_head_unshared_backward",
                                               _gauss_head_unshared_args(rows, n, ws, ctx.lo, ctx.hi), d_log_std, t,
                                               ctx.needs_input_grad[0])
        dw = th.empty(n, na, 64, dtype=th.float32, device=dev)
        db = th.empty(n, na, dtype=th.float32, device=dev)
        b = rows // n
        du3, h3 = d_u.view(b, n, na), h.detach().view(b, n, 64)
        tall_wgrad_batched([(du3[:, i], h3[:, i], dw[i], db[i]) for i in range(n)])
        grads = []
        for i in range(n):
            grads += [dw[i], db[i]]
        return (d_h, None, None, None, *grads)


def gauss_log_std_unshared(agents, h):
    """log_std [b * n, a] of per-agent Gaussian agents on the actors' ``h`` [b * n, 64] (``gauss_head_unshared_supported``
    holds, ``mlp_actor_allowed()``)."""
    agents = list(agents)
    a0 = agents[0].args
    flat = [p for g in agents for p in (g.log_std.weight, g.log_std.bias)]
    return _GaussHeadUnsharedFn.apply(h, len(agents), a0.LOG_STD_MIN, a0.LOG_STD_MAX, *flat)


def lnrelu_supported(agent, n_agents):
    """Configurations csrc/lnrelu.hip covers: 64 hidden units, ReLU, at most FLEXNET_MAX_AGENTS id columns."""
    a = agent.args
    return (a.hid_size == 64 and a.hid_activation == "relu" and 1 <= n_agents <= 8
            and getattr(agent, "fused_epilogue", True))


class _WideBatchLinear(th.autograd.Function):
    """y = x @ W.T for a tall x [B, K] (B ~ 1e4..1e5) and a small W [N, K], x without gradient.  The weight gradient
    dW = dy.T @ x has only N*K/tile output tiles (23 workgroups for 64 x 720) and a reduction over the whole batch:
    the library kernel leaves 90 % of the chip idle (250 us at batch 32 768).  Split-K by hand: the batch is cut into
    S slabs, one batched GEMM forms S partial dW, their sum is the gradient (S * 23 workgroups)."""

    SLABS = 16

    @staticmethod
    def forward(ctx, x, w):
        ctx.save_for_backward(x, w)
        return x @ w.t()

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        dw = dx = None
        if ctx.needs_input_grad[1]:
            b = x.shape[0]
            s = _WideBatchLinear.SLABS
            if b >= WGRAD_MIN_ROWS and tall_wgrad_supported(dy, x):
                dw = tall_wgrad(dy, x)
            elif b % s == 0 and b >= 4096:
                dw = th.bmm(dy.reshape(s, b // s, -1).transpose(1, 2), x.reshape(s, b // s, -1)).sum(0)
            else:
                dw = dy.t() @ x
        if ctx.needs_input_grad[0]:
            dx = dy @ w
        return dx, dw


def wide_batch_linear(x, w):
    return _WideBatchLinear.apply(x, w)


def _critic_config_ok(critic):
    """The MLPCritic configuration csrc/critic.hip (and the tail inside csrc/sqddpg.hip) implements: 64 hidden units, ReLU,
    one output."""
    a = critic.args
    return a.hid_size == 64 and a.hid_activation == "relu" and critic.fc3.out_features == 1


def critic_tail_supported(critic, x):
    a = critic.args
    ok = (x.is_cuda and x.dtype == th.float32 and x.dim() == 2 and x.shape[1] == 64 and _critic_config_ok(critic)
          and getattr(critic, "fused_tail", True))
    if x.is_cuda and not ok and getattr(critic, "fused_tail", True):
        note_fallback("critic_tail", f"hid {a.hid_size}, act {a.hid_activation}, out {critic.fc3.out_features}, dtype {x.dtype}")
    return ok


CRITIC_VARIANT = 0              # 0: matrix-core forward / dz1-only backward (csrc/critic.hip); 1: the VALU kernels
CRITIC_PGRAD32 = 0              # matrix-core backward WITH parameter gradients: 0 = 16-row tiles, two wavefronts per SIMD;
#                                 1 = the 32-row kernel it replaced (tests and tools/critic_bench.py compare the two)


def _tail_params(critic):
    """(ln_w, ln_b, w2, b2, w3, b3, eps) of an MLPCritic: the tail's arguments, in the order every critic node takes them."""
    ln = critic.layernorm if critic.args.layernorm else None
    return (None if ln is None else ln.weight, None if ln is None else ln.bias, critic.fc2.weight, critic.fc2.bias,
            critic.fc3.weight, critic.fc3.bias, _ln_eps(critic))


def _critic_args(z1, ln_w, ln_b, w2, b2, w3, b3, eps):
    a = _lib.FlexCriticTailArgs()
    a.rows, a.layernorm, a.ln_eps, a.variant = z1.shape[0], int(ln_w is not None), float(eps), CRITIC_VARIANT
    a.variant_pgrad32 = CRITIC_PGRAD32
    a.z1 = z1.data_ptr()
    if ln_w is not None:
        a.ln_w, a.ln_b = ln_w.data_ptr(), ln_b.data_ptr()
    a.fc2_w, a.fc2_b, a.fc3_w, a.fc3_b = w2.data_ptr(), b2.data_ptr(), w3.data_ptr(), b3.data_ptr()
    return a


def _composed_args(shared, n, W, no, tail, dense_ids=None):
    """``_critic_args`` for the composed input z1[b, i] = shared[b] + id column i (``tail``: _tail_params' tuple).  The
    id-column table is ``dense_ids`` [n, 64] if given, else columns no .. no + n - 1 of fc1.weight ``W`` read where they are
    (the kernels stage the table in LDS through the two strides: no transposed copy per call)."""
    args = _critic_args(shared, *tail)
    args.rows, args.z1, args.z_shared, args.n_agents = shared.shape[0] * n, None, shared.data_ptr(), n
    if dense_ids is not None:
        args.z_id = dense_ids.data_ptr()
    else:
        args.z_id = W[:, no:no + n].data_ptr()
        args.z_id_agent_stride, args.z_id_unit_stride = 1, W.stride(0)
    return args


def _critic_workspace(device):
    """Per-device scratch for the backward kernel's per-block partial sums (18 MB, allocated once)."""
    return _scratch("critic", device, _lib.FLEXNET_CRITIC_WS_FLOATS)


def _bind_workspace(args, device, overwrite=False):
    """With the workspace the backward kernel reduces the parameter gradients in a fixed-order second stage; ``overwrite``:
    that stage STORES them (no zero fill of the slab needed) instead of adding to what is there."""
    ws = _critic_workspace(device)
    args.workspace, args.workspace_floats, args.overwrite_grads = ws.data_ptr(), ws.numel(), int(overwrite)


# The tail's six parameter gradients are written into ONE slab (one allocation, one zero fill where they are accumulated):
# FlexCriticTailArgs field -> (first float, shape), in the order fc2.weight, fc2.bias, fc3.weight, LayerNorm weight and
# bias, fc3.bias
_TAIL_GRADS = {}
_TAIL_FLOATS = 0
for _name, _shape in (("d_fc2_w", (64, 64)), ("d_fc2_b", (64,)), ("d_fc3_w", (1, 64)), ("d_ln_w", (64,)), ("d_ln_b", (64,)),
                      ("d_fc3_b", (1,))):
    _TAIL_GRADS[_name] = (_TAIL_FLOATS, _shape)
    _TAIL_FLOATS += math.prod(_shape)


def _new_tail_grads(device, zero=False, heads=None):
    """An empty slab ([heads, floats] with ``heads``); ``zero``: zero-filled, for the kernels that accumulate into it."""
    shape = (_TAIL_FLOATS,) if heads is None else (heads, _TAIL_FLOATS)
    return (th.zeros if zero else th.empty)(shape, dtype=th.float32, device=device)


def _bind_tail_grads(args, slab):
    """Point the d_* fields of ``args`` into ``slab`` (one head's); the LayerNorm pair only where there is a LayerNorm."""
    base = slab.data_ptr()
    for name, (first, _) in _TAIL_GRADS.items():
        if args.layernorm or name not in ("d_ln_w", "d_ln_b"):
            setattr(args, name, base + 4 * first)


def _split_tail_grads(slab, has_ln):
    """The six gradients of a slab in autograd-return order (ln_w, ln_b, w2, b2, w3, b3), None for an absent LayerNorm."""
    def part(name):
        first, shape = _TAIL_GRADS[name]
        g = slab[first:first + math.prod(shape)]
        return g.view(shape) if len(shape) > 1 else g
    return ((part("d_ln_w") if has_ln else None), (part("d_ln_b") if has_ln else None), part("d_fc2_w"), part("d_fc2_b"),
            part("d_fc3_w"), part("d_fc3_b"))


def _sum_rows(x):
    """x[0] + ... + x[n - 1] with n - 1 pointwise adds: no ATen reduction in a captured graph."""
    tot = x[0]
    for i in range(1, x.shape[0]):
        tot = tot + x[i]
    return tot


def _fc1_grad(dW, d_shared, obs2d, act2d, n, d_id=None, flag_rows=None, critic_finish=None):
    """Fill fc1's weight gradient ``dW`` [64, obs | n id columns | act | trailing columns] from ``d_shared`` [b, 64] and
    return its bias gradient (the column sum from the same pass).  ``d_id`` [n, 64]: the id-column sums, transposed into the
    id block (None: the tail's backward wrote them there through its strides).  Trailing columns see no input: zero —
    except, with ``flag_rows`` [n, 64] (both heads of the twin critic), the last one: the flag column sees every agent's row
    of the second head, the sum of its id-column gradients.  ``critic_finish``: tall_wgrad's rider."""
    no, na_ = obs2d.shape[1], act2d.shape[1]
    end = no + n + na_
    d_bias = th.empty(64, dtype=th.float32, device=dW.device)
    # the observation block and the action block of dW from one launch (the action block rides in the last column chunk)
    tall_wgrad(d_shared, obs2d, out=dW[:, :no], colsum=d_bias, x2=act2d, out2=dW[:, no + n:end], critic_finish=critic_finish)
    if d_id is not None:
        dW[:, no:no + n] = d_id.t()
    if flag_rows is not None:
        dW[:, -1] = _sum_rows(flag_rows)
        if dW.shape[1] > end + 1:
            dW[:, end:-1] = 0.0
    elif dW.shape[1] > end:
        dW[:, end:] = 0.0
    return d_bias


class _CriticTailFn(th.autograd.Function):
    """q = fc3(relu(fc2(relu(LayerNorm(z1))))) (mlp_critic.py:27-31) with a hand-written backward: gradients for z1 and
    for the six parameter tensors of the tail."""

    @staticmethod
    def forward(ctx, z1, *tail):
        z1 = z1.contiguous()
        q = th.empty(z1.shape[0], 1, dtype=th.float32, device=z1.device)
        args = _critic_args(z1, *tail)
        args.q = q.data_ptr()
        _lib.launch("flexnet_critic_tail_forward", args)
        ctx.eps = tail[6]
        ctx.save_for_backward(z1, *tail[:6])
        return q

    @staticmethod
    def backward(ctx, dq):
        z1, *tail = ctx.saved_tensors
        dq = dq.contiguous()
        dz1 = th.empty_like(z1)
        args = _critic_args(z1, *tail, ctx.eps)
        args.dq, args.dz1 = dq.data_ptr(), dz1.data_ptr()
        if not any(ctx.needs_input_grad[1:7]):
            # the policy loss differentiates through a critic whose parameters take no step: dz1 only
            _lib.launch("flexnet_critic_tail_backward", args)
            return (dz1,) + (None,) * 7
        grads = _new_tail_grads(z1.device, zero=True)      # one zero-fill for all six
        _bind_tail_grads(args, grads)
        _bind_workspace(args, z1.device)
        _lib.launch("flexnet_critic_tail_backward", args)
        return (dz1, *_split_tail_grads(grads, tail[0] is not None), None)


class _CriticTailComposedFn(th.autograd.Function):
    """The same tail on z1[b, i] = shared[b] + id_cols[i] (the critic's first-layer output when no agent's own-action
    gradient is needed, maddpg.py:38-54) without materialising the [b * n, 64] tensor on the way in."""

    @staticmethod
    def forward(ctx, shared, id_cols, *tail):
        shared = shared.contiguous()
        n = id_cols.shape[0]
        q = th.empty(shared.shape[0] * n, 1, dtype=th.float32, device=shared.device)
        args = _composed_args(shared, n, None, 0, tail, dense_ids=id_cols)
        if not id_cols.is_contiguous():          # fc1.weight's id columns, transposed view: read in place through strides
            args.z_id_agent_stride, args.z_id_unit_stride = id_cols.stride(0), id_cols.stride(1)
        args.q = q.data_ptr()
        _lib.launch("flexnet_critic_tail_forward", args)
        ctx.eps = tail[6]
        ctx.save_for_backward(shared, id_cols, *tail[:6])
        return q

    @staticmethod
    def backward(ctx, dq):
        shared, id_cols, *tail = ctx.saved_tensors
        id_cols = id_cols.contiguous()
        n = id_cols.shape[0]
        dev = shared.device
        dq = dq.contiguous()
        dz1 = th.empty(shared.shape[0] * n, 64, dtype=th.float32, device=dev)
        grads = _new_tail_grads(dev, zero=True)
        args = _composed_args(shared, n, None, 0, (*tail, ctx.eps), dense_ids=id_cols)
        args.dq, args.dz1 = dq.data_ptr(), dz1.data_ptr()
        _bind_tail_grads(args, grads)
        _bind_workspace(args, dev)
        d_shared = th.empty_like(shared)
        d_id = th.empty(n, 64, dtype=th.float32, device=dev)
        args.d_z_shared, args.d_z_id = d_shared.data_ptr(), d_id.data_ptr()
        _lib.launch("flexnet_critic_tail_backward", args)
        return (d_shared, d_id, *_split_tail_grads(grads, tail[0] is not None), None)


class _CriticReplayedFn(th.autograd.Function):
    """The WHOLE shared-parameter critic on replayed (gradient-free) inputs, maddpg.py:33-76 + mlp_critic.py:25-33, as
    one autograd node: q[b, i] = tail(obs_all[b] W_obs^T + act_all[b] W_act^T + bias + W_id[:, i]).  Forward: two GEMMs
    (the second accumulates) and the composed tail kernel.  Backward: the tail backward kernel, two reductions of dz1,
    and fc1's weight gradient written block by block into ONE [64, in] tensor by csrc/wgrad.hip (its bias gradient is the
    column sum from the same pass) — instead of three column-slice gradients that autograd zero-fills, scatters and
    adds, plus a separate bias reduction."""

    @staticmethod
    def forward(ctx, obs2d, act2d, n_agents, W, bias, ln_w, ln_b, w2, b2, w3, b3, eps, twin=False):
        no = obs2d.shape[1]
        shared = critic_first_layer(bias, obs2d, act2d, W, no + n_agents)
        # twin (matd3.py:64-67): the second head is the same network with the trailing 0/1 input flag set — fc1's last
        # column joins every agent's id column
        id_cols = (W[:, no:no + n_agents] + W[:, -1:]).t().contiguous() if twin else None
        ctx.twin = bool(twin)
        q = th.empty(shared.shape[0] * n_agents, 1, dtype=th.float32, device=shared.device)
        args = _composed_args(shared, n_agents, W, no, (ln_w, ln_b, w2, b2, w3, b3, eps), dense_ids=id_cols)
        args.q = q.data_ptr()
        _lib.launch("flexnet_critic_tail_forward", args)
        ctx.eps, ctx.n_agents = eps, n_agents
        ctx.save_for_backward(obs2d, act2d, shared, id_cols, W, ln_w, ln_b, w2, b2, w3, b3)
        return q

    @staticmethod
    def backward(ctx, dq):
        obs2d, act2d, shared, id_cols, W, *tail = ctx.saved_tensors      # (id_cols: twin only)
        n = ctx.n_agents
        no = obs2d.shape[1]
        dev = shared.device
        dq = dq.contiguous()
        dz1 = th.empty(shared.shape[0] * n, 64, dtype=th.float32, device=dev)
        # the six tail gradients are STORED by the fixed-order second stage (overwrite_grads): no zero fill
        grads = _new_tail_grads(dev)
        args = _composed_args(shared, n, W, no, (*tail, ctx.eps), dense_ids=id_cols)
        args.dq, args.dz1 = dq.data_ptr(), dz1.data_ptr()
        _bind_tail_grads(args, grads)
        _bind_workspace(args, dev, overwrite=True)
        d_shared = th.empty_like(shared)                    # dz1 folded onto its two sources by the same call
        dW = th.empty_like(W)
        if ctx.twin:
            d_id = th.empty(n, 64, dtype=th.float32, device=dev)
        else:                                               # ... the id-column sums straight into dW[:, no:no + n]
            d_id = dW[:, no:no + n]
            args.d_z_id_agent_stride, args.d_z_id_unit_stride = 1, W.shape[1]
        args.d_z_shared, args.d_z_id = d_shared.data_ptr(), d_id.data_ptr()
        _lib.launch("flexnet_critic_tail_backward", args)
        d_bias = _fc1_grad(dW, d_shared, obs2d, act2d, n, d_id=d_id if ctx.twin else None)
        if ctx.twin and W.shape[1] > no + n + act2d.shape[1]:
            dW[:, -1] = _sum_rows(d_id)      # the flag column sees every agent's row: the sum of the id-column gradients
        return (None, None, None, dW, d_bias, *_split_tail_grads(grads, tail[0] is not None), None, None)


class _CriticReplayedTwinFn(th.autograd.Function):
    """Both heads of MATD3's twin critic (matd3.py:33-86: ONE network, the second head with the trailing 0/1 input flag set)
    on replayed inputs as one node: fc1's output on [obs | act] is the same for both heads — only the id-column table
    differs (the flag column joins it) — so it is formed once, the tail runs forward and backward per head, and fc1's weight
    gradient is taken ONCE on the sum of the two heads' input gradients.  Returns cat([Q1, Q2]) as [2 rows, 1]."""

    @staticmethod
    def forward(ctx, obs2d, act2d, n_agents, W, bias, *tail):
        n = n_agents
        no = obs2d.shape[1]
        shared = critic_first_layer(bias, obs2d, act2d, W, no + n)
        id2 = (W[:, no:no + n] + W[:, -1:]).t().contiguous()
        rows = shared.shape[0] * n
        q = th.empty(2 * rows, 1, dtype=th.float32, device=shared.device)
        for h in range(2):
            args = _composed_args(shared, n, W, no, tail, dense_ids=id2 if h else None)
            args.q = q[h * rows:].data_ptr()
            _lib.launch("flexnet_critic_tail_forward", args)
        ctx.eps, ctx.n_agents = tail[6], n
        ctx.save_for_backward(obs2d, act2d, shared, id2, W, *tail[:6])
        return q

    @staticmethod
    def backward(ctx, dq):
        obs2d, act2d, shared, id2, W, *tail = ctx.saved_tensors
        n = ctx.n_agents
        no = obs2d.shape[1]
        rows = shared.shape[0] * n
        dev = shared.device
        dq = dq.contiguous()
        dz1 = th.empty(rows, 64, dtype=th.float32, device=dev)                 # (per head, consumed inside its call)
        grads = _new_tail_grads(dev, heads=2)
        d_shared = th.empty((2,) + tuple(shared.shape), dtype=th.float32, device=dev)
        d_id = th.empty(2, n, 64, dtype=th.float32, device=dev)
        for h in range(2):
            args = _composed_args(shared, n, W, no, (*tail, ctx.eps), dense_ids=id2 if h else None)
            args.dq, args.dz1 = dq[h * rows:].data_ptr(), dz1.data_ptr()
            _bind_tail_grads(args, grads[h])
            _bind_workspace(args, dev, overwrite=True)
            args.d_z_shared, args.d_z_id = d_shared[h].data_ptr(), d_id[h].data_ptr()
            _lib.launch("flexnet_critic_tail_backward", args)
        gsum = grads[0] + grads[1]
        dsum = d_shared[0] + d_shared[1]
        isum = d_id[0] + d_id[1]
        dW = th.empty_like(W)
        d_bias = _fc1_grad(dW, dsum, obs2d, act2d, n, d_id=isum, flag_rows=d_id[1])
        return (None, None, None, dW, d_bias, *_split_tail_grads(gsum, tail[0] is not None), None)


# Measured and NOT adopted (round 5; VERDICT r04 item 1b asked for the small launches to be folded into their neighbours): the
# value sub-update's small launches BESIDE its matrix work on a second stream — the reward-statistics pass (6.7 us, needs only
# the batch's rewards) while the first-layer product runs, the finish launch (5.4 us: parameter gradients from the partial
# rows, loss, running statistics) while the first layer's weight gradient runs; neither needs the other's output.  Under
# HIP-graph capture the fork and join become graph edges, and every cross-branch edge of a replayed graph costs 4-9 us of idle
# time on this runtime: kernel time 396 -> 370 us per value sub-update, span 404 -> 401 (profiles/r05g4_update_timeline.txt).
# One stream is the default; FLEX_TD_FORK=1 keeps the two-stream form reachable (same kernels, same bits:
# tests/test_critic_gpu.py).
TD_FORK = os.environ.get("FLEX_TD_FORK", "0") == "1"
_SIDE_STREAMS = {}


def _side_stream(device):
    s = _SIDE_STREAMS.get(device)
    if s is None:
        s = _SIDE_STREAMS[device] = th.cuda.Stream(device=device)
    return s


class _CriticTdLossFn(th.autograd.Function):
    """mean((BatchNorm(reward) + gamma (1 - done) Q'(s', pi'(s')) - Q(s, a))^2) for the shared-parameter critic on replayed
    inputs — maddpg.py:100-123 over maddpg.py:33-76 + mlp_critic.py:25-33 — with the critic's backward run IN the forward
    (include/flexnet.h: flexnet_critic_td_backward): the matrix-core backward kernel recomputes the tail's forward anyway,
    so it forms q, the TD error, dLoss/dq and the loss itself.  No forward launch of the tail, no q / dq tensors, no
    td_apply launch; every parameter gradient of the critic is ready when the loss is, and ``backward`` hands them over
    (times the incoming gradient unless that is util.unit_seed).  The BatchNorm module's running statistics move as its
    own training-mode forward would move them."""

    @staticmethod
    def forward(ctx, obs2d, act2d, n_agents, W, bias, ln_w, ln_b, w2, b2, w3, b3, eps, next_q, reward, done, gamma, bn):
        n = n_agents
        no = obs2d.shape[1]
        dev = obs2d.device
        nq, r, d = next_q.reshape(-1, n).contiguous(), reward.contiguous(), done.reshape(-1).contiguous()
        t = _td_args(r, d, nq, gamma, bn, update_stats=True)
        _td_sync_stats(t, _td_workspace(r.device), bn)
        offer = TD_OFFERS.get(r.data_ptr())
        if offer is not None and offer["ref"]() is None:
            del TD_OFFERS[r.data_ptr()]
            offer = None
        if offer is not None and t.normalise and not t.stats_ready:
            t.stats_ready, offer["taken"] = 1, True           # filed by the launch that refreshed this batch (offer_td_stats)
        fork = TD_FORK
        main = th.cuda.current_stream(dev)
        side = _side_stream(dev) if fork else None
        if fork and t.normalise and not t.stats_ready:
            # the statistics pass beside the first-layer product (it needs the rewards only)
            side.wait_stream(main)
            _lib.launch("flexnet_td_stats", t, stream=side)
            t.stats_ready = 1
        shared = critic_first_layer(bias, obs2d, act2d, W, no + n)
        if fork:
            main.wait_stream(side)
        dz1 = th.empty(shared.shape[0] * n, 64, dtype=th.float32, device=dev)
        grads = _new_tail_grads(dev)
        args = _composed_args(shared, n, W, no, (ln_w, ln_b, w2, b2, w3, b3, eps))
        args.dz1 = dz1.data_ptr()
        _bind_tail_grads(args, grads)
        _bind_workspace(args, dev, overwrite=True)
        d_shared = th.empty_like(shared)
        dW = th.empty_like(W)
        args.d_z_shared, args.d_z_id = d_shared.data_ptr(), dW[:, no:no + n].data_ptr()
        args.d_z_id_agent_stride, args.d_z_id_unit_stride = 1, W.shape[1]
        loss = th.empty((), dtype=th.float32, device=dev)
        t.loss = loss.data_ptr()
        sm = args.variant_pgrad32 == 0          # (the 16-row kernel writes d_z_shared itself: the finish does not feed the weight gradient)
        if fork and sm:
            _lib.launch("flexnet_critic_td_backward_phases", args, t, 1)
            side.wait_stream(main)
            _lib.launch("flexnet_critic_td_backward_phases", args, t, 2, stream=side)
            d_bias = _fc1_grad(dW, d_shared, obs2d, act2d, n)
            main.wait_stream(side)
        elif sm:
            # the finish (phase 2) depends on the backward kernel alone: it rides in the weight gradient's second-stage launch
            _lib.launch("flexnet_critic_td_backward_phases", args, t, 1)
            d_bias = _fc1_grad(dW, d_shared, obs2d, act2d, n, critic_finish=(args, t))
        else:
            _lib.launch("flexnet_critic_td_backward", args, t)
            d_bias = _fc1_grad(dW, d_shared, obs2d, act2d, n)
        ctx.has_ln = ln_w is not None
        ctx.save_for_backward(dW, d_bias, grads)
        return loss

    @staticmethod
    def backward(ctx, g):
        from .util import is_unit_seed
        dW, d_bias, grads = ctx.saved_tensors
        if not is_unit_seed(g):
            dW, d_bias, grads = dW * g, d_bias * g, grads * g
        return (None, None, None, dW, d_bias, *_split_tail_grads(grads, ctx.has_ln)) + (None,) * 6


def _td_args(reward, done, next_q, gamma, bn, update_stats=True):
    """FlexTdLossArgs for [rows, n] tensors (q / dq / loss left to the caller); the workspace is per device."""
    rows, n = reward.shape
    ws = _td_workspace(reward.device)
    a = _lib.FlexTdLossArgs()
    a.rows, a.n_agents, a.normalise, a.gamma = rows, n, int(bn is not None), float(gamma)
    a.reward, a.done, a.next_q = reward.data_ptr(), done.data_ptr(), next_q.data_ptr()
    if bn is not None:
        a.bn_eps, a.bn_momentum = float(bn.eps), float(bn.momentum)
        if bn.affine:
            a.bn_weight, a.bn_bias = bn.weight.data_ptr(), bn.bias.data_ptr()
        if bn.track_running_stats and update_stats:
            a.running_mean, a.running_var = bn.running_mean.data_ptr(), bn.running_var.data_ptr()
            a.num_batches_tracked = bn.num_batches_tracked.data_ptr()
    a.workspace, a.workspace_floats = ws.data_ptr(), 2 * ws.numel()
    return a


CRITIC_TD_MIN_ROWS = 65536          # csrc/critic.hip CRITIC_MFMA_MIN_ROWS: below it the matrix-core backward is not used


def critic_td_loss_supported(critic, obs2d, act2d, n_agents, next_q, reward, done, bn):
    """What flexnet_critic_td_backward covers: the replayed-input critic node's configuration at matrix-core batch sizes,
    an fc1 without trailing extra columns, the fused value loss's tensors, gradients wanted."""
    W = critic.fc1.weight
    return (critic_replayed_supported(critic, obs2d, act2d, n_agents) and th.is_grad_enabled() and W.requires_grad
            and obs2d.shape[0] * n_agents >= CRITIC_TD_MIN_ROWS and CRITIC_VARIANT == 0
            and W.shape[1] == obs2d.shape[1] + n_agents + act2d.shape[1]
            and reward.dim() == 2 and reward.shape == (obs2d.shape[0], n_agents)
            and td_loss_supported(reward, next_q, reward, done, bn))


def critic_td_loss(obs2d, act2d, n_agents, critic, next_q, reward, done, gamma, bn):
    return _CriticTdLossFn.apply(obs2d, act2d, n_agents, critic.fc1.weight, critic.fc1.bias, *_tail_params(critic),
                                 next_q, reward, done, gamma, bn)


class _ExpandAgentsFn(th.autograd.Function):
    """x [b, 1, a] -> [b, n, a] (the agent-summed action of matd3.py:92-97 / iddpg.py:66-71 handed to every agent); the
    backward sums over the agent axis with n - 1 pointwise adds instead of ATen's reduce_kernel (a captured HIP graph
    must not hold one)."""

    @staticmethod
    def forward(ctx, x, n):
        ctx.n = n
        return x.expand(-1, n, -1)

    @staticmethod
    def backward(ctx, g):
        parts = g.unbind(1)
        tot = parts[0]
        for p in parts[1:]:
            tot = tot + p
        return tot.unsqueeze(1), None


def expand_agents(x, n):
    return _ExpandAgentsFn.apply(x, n) if x.requires_grad else x.expand(-1, n, -1)


def _policy_args(obs2d, act, W, bias, tail):
    """The forward set-up of the two policy-loss nodes: fc1 on [obs | the policy's own actions] — value-wise every row is
    shared[b] + W_id[:, i], the own-action term is zero-valued — and the composed tail's arguments on it."""
    b, n, na_ = act.shape
    no = obs2d.shape[1]
    shared = critic_first_layer(bias, obs2d, act.reshape(b, n * na_), W, no + n)
    return shared, _composed_args(shared, n, W, no, tail)


def _policy_d_act(dz1, W, dims):
    """d act[b, i] = dz1[b, i] @ W_act[:, block i]: row i of a sample carries agent i's own action block only."""
    b, n, na_, no = dims
    W_act = W[:, no + n:no + n + n * na_].reshape(64, n, na_)
    return th.einsum("bih,hia->bia", dz1.view(b, n, 64), W_act)


class _CriticPolicyFn(th.autograd.Function):
    """The shared-parameter critic inside the POLICY loss, maddpg.py:33-76 + maddpg.py:104-107: q[b, i] on the policy's own
    actions, differentiated w.r.t. those actions only (row i of a sample carries agent i's own action block; the other
    agents' blocks are detached, maddpg.py:47-54).  Value-wise every row is still shared[b] + W_id[:, i] — the own-action
    term is zero-valued — so the forward is two GEMMs and the composed tail kernel; the backward is the tail's dz1-only
    kernel and d act[b, i] = dz1[b, i] @ W_act[:, block i].  The critic's parameters get no gradient from this node: it
    is used where only the policy optimiser steps (utils/trainer.py:99-108 steps the policy on the policy loss)."""

    @staticmethod
    def forward(ctx, obs2d, act, W, bias, *tail):
        shared, args = _policy_args(obs2d, act, W, bias, tail)
        q = th.empty(args.rows, 1, dtype=th.float32, device=shared.device)
        args.q = q.data_ptr()
        _lib.launch("flexnet_critic_tail_forward", args)
        ctx.eps, ctx.dims = tail[6], (*act.shape, obs2d.shape[1])
        ctx.save_for_backward(shared, W, *tail[:6])
        return q

    @staticmethod
    def backward(ctx, dq):
        shared, W, *tail = ctx.saved_tensors
        b, n, na_, no = ctx.dims
        dq = dq.contiguous()
        dz1 = th.empty(b * n, 64, dtype=th.float32, device=shared.device)
        args = _composed_args(shared, n, W, no, (*tail, ctx.eps))
        args.dq, args.dz1 = dq.data_ptr(), dz1.data_ptr()
        _lib.launch("flexnet_critic_tail_backward", args)
        return (None, _policy_d_act(dz1, W, ctx.dims)) + (None,) * 9


class _CriticPolicyLossFn(th.autograd.Function):
    """sign * mean(Q(s, pi(s))) over all [b, n] entries for the shared-parameter critic, differentiated w.r.t. the policy's
    actions only — the policy loss of maddpg.py:104-107 as ONE node.  The gradient of a mean is a constant, so the critic
    needs no forward pass of its own: the dz1-only backward kernel (which recomputes the forward) runs in this node's
    ``forward`` with a uniform dLoss/dq and also returns the sum of q, i.e. the loss.  No tail forward launch, no loss
    reduction launches; ``backward`` hands the stored action gradient over."""

    @staticmethod
    def forward(ctx, obs2d, act, W, bias, ln_w, ln_b, w2, b2, w3, b3, eps, sign):
        shared, args = _policy_args(obs2d, act, W, bias, (ln_w, ln_b, w2, b2, w3, b3, eps))
        rows = args.rows
        dz1 = th.empty(rows, 64, dtype=th.float32, device=shared.device)
        loss = th.empty((), dtype=th.float32, device=shared.device)
        args.dz1 = dz1.data_ptr()
        args.dq_uniform, args.dq_value, args.q_mean_scale, args.q_mean_out = 1, sign / rows, sign / rows, loss.data_ptr()
        _bind_workspace(args, shared.device)
        _lib.launch("flexnet_critic_tail_backward", args)
        ctx.save_for_backward(_policy_d_act(dz1, W, (*act.shape, obs2d.shape[1])))
        return loss

    @staticmethod
    def backward(ctx, g):
        from .util import is_unit_seed
        (d_act,) = ctx.saved_tensors
        return (None, d_act if is_unit_seed(g) else d_act * g) + (None,) * 10


def critic_policy_loss_supported(critic, obs2d, act, n_agents):
    return (critic_policy_supported(critic, obs2d, act, n_agents) and CRITIC_VARIANT == 0
            and act.shape[0] * n_agents >= CRITIC_TD_MIN_ROWS and act.requires_grad and th.is_grad_enabled())


def critic_policy_loss(obs2d, act, critic, sign=-1.0):
    return _CriticPolicyLossFn.apply(obs2d, act, critic.fc1.weight, critic.fc1.bias, *_tail_params(critic), float(sign))


def critic_policy_supported(critic, obs2d, act, n_agents):
    W = critic.fc1.weight
    return (obs2d.is_cuda and obs2d.dtype == th.float32 and act.dtype == th.float32 and act.dim() == 3
            and _critic_config_ok(critic) and getattr(critic, "fused_tail", True)
            and 1 <= n_agents <= 8 and not obs2d.requires_grad and act.shape[1] == n_agents
            and W.shape[1] in (obs2d.shape[1] + n_agents + n_agents * act.shape[2],
                               obs2d.shape[1] + n_agents + n_agents * act.shape[2] + 1))      # + MATD3's twin flag column


def critic_replayed_supported(critic, obs2d, act2d, n_agents):
    W = critic.fc1.weight
    return (obs2d.is_cuda and obs2d.dtype == th.float32 and act2d.dtype == th.float32
            and _critic_config_ok(critic) and getattr(critic, "fused_tail", True)
            and 1 <= n_agents <= 8 and not obs2d.requires_grad and not act2d.requires_grad
            and obs2d.shape[0] >= WGRAD_MIN_ROWS and W.shape[1] in (obs2d.shape[1] + n_agents + act2d.shape[1],
                                                                    obs2d.shape[1] + n_agents + act2d.shape[1] + 1)
            and all(x.dim() == 2 and x.stride(1) == 1 and x.shape[1] <= x.stride(0) < (1 << 24) for x in (obs2d, act2d)))


class CriticTail:
    @staticmethod
    def apply_policy(obs2d, act, critic):
        return _CriticPolicyFn.apply(obs2d, act, critic.fc1.weight, critic.fc1.bias, *_tail_params(critic))

    @staticmethod
    def apply_replayed_twin(obs2d, act2d, n_agents, critic):
        return _CriticReplayedTwinFn.apply(obs2d, act2d, n_agents, critic.fc1.weight, critic.fc1.bias, *_tail_params(critic))

    @staticmethod
    def apply_replayed(obs2d, act2d, n_agents, critic, twin=False):
        return _CriticReplayedFn.apply(obs2d, act2d, n_agents, critic.fc1.weight, critic.fc1.bias, *_tail_params(critic), twin)

    @staticmethod
    def apply_composed(shared, id_cols, critic):
        return _CriticTailComposedFn.apply(shared, id_cols, *_tail_params(critic))

    @staticmethod
    def apply(z1, critic):
        return _CriticTailFn.apply(z1, *_tail_params(critic))


# ---- QMIX mixer of FACMADDPG (madrl/critics/qmix.py) ---------------------------------------------------------------------
QMIX_PARAMS = ("hyper_w_1.0.weight", "hyper_w_1.0.bias", "hyper_w_1.2.weight", "hyper_w_1.2.bias",
               "hyper_w_final.0.weight", "hyper_w_final.0.bias", "hyper_w_final.2.weight", "hyper_w_final.2.bias",
               "hyper_b_1.weight", "hyper_b_1.bias", "V.0.weight", "V.0.bias", "V.2.weight", "V.2.bias")


class QMixer(nn.Module):
    """madrl/critics/qmix.py:6-81, same parameter names and shapes (a reference state_dict loads).  On the GPU, in the shipped
    configuration (two-layer hypernetworks of width 64, mixing_embed_dim 64, q_embed_dim 1, not gated, no skip connections),
    forward and backward are csrc/qmix.hip plus flexnet_wgrad reductions (one autograd node, _QmixFn); elsewhere the
    reference's PyTorch composition (``forward_torch``)."""

    def __init__(self, args):
        super().__init__()
        self.args = args
        self.n_agents = args.agent_num
        self.state_dim = args.obs_size * args.agent_num
        self.embed_dim = args.mixing_embed_dim
        self.q_embed_dim = getattr(args, "q_embed_dim", 1)
        out1 = self.embed_dim * self.n_agents * self.q_embed_dim
        self.hyper_w_1 = nn.Linear(self.state_dim, out1)
        self.hyper_w_final = nn.Linear(self.state_dim, self.embed_dim)
        if getattr(args, "hypernet_layers", 1) > 1:
            assert args.hypernet_layers == 2, "Only 1 or 2 hypernet_layers is supported atm!"
            he = args.hypernet_embed
            self.hyper_w_1 = nn.Sequential(nn.Linear(self.state_dim, he), nn.ReLU(), nn.Linear(he, out1))
            self.hyper_w_final = nn.Sequential(nn.Linear(self.state_dim, he), nn.ReLU(), nn.Linear(he, self.embed_dim))
        if getattr(args, "hyper_initialization_nonzeros", 0) > 0:          # qmix.py:35-40, as written there
            std = args.hyper_initialization_nonzeros ** -0.5
            self.hyper_w_1.weight.data.normal_(std=std)
            self.hyper_w_1.bias.data.normal_(std=std)
            self.hyper_w_final.weight.data.normal_(std=std)
            self.hyper_w_final.bias.data.normal_(std=std)
        self.hyper_b_1 = nn.Linear(self.state_dim, self.embed_dim)
        self.V = nn.Sequential(nn.Linear(self.state_dim, self.embed_dim), nn.ReLU(), nn.Linear(self.embed_dim, 1))
        if getattr(args, "gated", False):
            self.gate = nn.Parameter(th.ones(size=(1,)) * 0.5)

    def fused_config(self):
        """The configuration csrc/qmix.hip implements (include/flexnet.h: flexnet_qmix_forward)."""
        a = self.args
        return (getattr(a, "hypernet_layers", 1) == 2 and a.hypernet_embed == 64 and self.embed_dim == 64
                and self.q_embed_dim == 1 and not getattr(a, "gated", False) and not getattr(a, "skip_connections", False)
                and 1 <= self.n_agents <= 8 and self.state_dim % 16 == 0 and 16 <= self.state_dim <= 1024)

    def fused_supported(self, agent_qs, states):
        if not (agent_qs.is_cuda and states.is_cuda):
            return False
        ok = (self.fused_config() and agent_qs.dtype == th.float32 and states.dtype == th.float32
              and not states.requires_grad and all(p.dtype == th.float32 and p.is_cuda for p in self.parameters()))
        if not ok:
            note_fallback("qmix", f"hypernet_layers {getattr(self.args, 'hypernet_layers', 1)}, state {self.state_dim}, "
                                  f"agents {self.n_agents}, gated {getattr(self.args, 'gated', False)}, "
                                  f"skip {getattr(self.args, 'skip_connections', False)}")
        return ok

    def forward(self, agent_qs, states, param_grads=True):
        """q_tot [bs, 1, 1] (qmix.py:53-81).  ``param_grads=False``: the caller differentiates w.r.t. ``agent_qs`` only (a value
        sub-update, whose optimiser holds the critic): the mixer's parameters take no gradient from this call."""
        bs = agent_qs.size(0)
        if self.fused_supported(agent_qs, states):
            q = agent_qs.reshape(bs, self.n_agents)
            x = states.reshape(bs, self.state_dim)
            params = dict(self.named_parameters())
            ws = [params[k] if param_grads else params[k].detach() for k in QMIX_PARAMS]
            save = th.is_grad_enabled() and (q.requires_grad or any(w.requires_grad for w in ws))
            return _QmixFn.apply(q, x, save, *ws).view(bs, 1, 1)
        return self.forward_torch(agent_qs, states, param_grads)

    def forward_torch(self, agent_qs, states, param_grads=True):
        """qmix.py:53-81 as written there."""
        params = {k: (v if param_grads else v.detach()) for k, v in self.named_parameters()}
        return self._forward_torch_with(agent_qs, states, params)

    def _forward_torch_with(self, agent_qs, states, p):
        bs = agent_qs.size(0)
        states = states.reshape(-1, self.state_dim)
        agent_qs = agent_qs.reshape(-1, 1, self.n_agents * self.q_embed_dim)

        def lin(x, name):
            return F.linear(x, p[name + ".weight"], p[name + ".bias"])

        def head(x, name):
            if isinstance(getattr(self, name), nn.Sequential):
                return lin(F.relu(lin(x, name + ".0")), name + ".2")
            return lin(x, name)

        w1 = th.abs(head(states, "hyper_w_1"))
        b1 = lin(states, "hyper_b_1")
        w1 = w1.view(-1, self.n_agents * self.q_embed_dim, self.embed_dim)
        b1 = b1.view(-1, 1, self.embed_dim)
        hidden = F.elu(th.bmm(agent_qs, w1) + b1)
        w_final = th.abs(head(states, "hyper_w_final")).view(-1, self.embed_dim, 1)
        v = head(states, "V").view(-1, 1, 1)
        s = agent_qs.sum(dim=2, keepdim=True) if getattr(self.args, "skip_connections", False) else 0
        if getattr(self.args, "gated", False):
            y = th.bmm(hidden, w_final) * p["gate"] + v + s
        else:
            y = th.bmm(hidden, w_final) + v + s
        return y.view(bs, -1, 1)


def _qmix_args(q, x, ws):
    a = _lib.FlexQmixArgs()
    a.batch, a.n_agents, a.state_dim = q.shape[0], q.shape[1], x.shape[1]
    a.ld_state = x.stride(0) if x.shape[0] > 1 else x.shape[1]
    a.agent_qs, a.state = q.data_ptr(), x.data_ptr()
    names = ("w1_0_w", "w1_0_b", "w1_2_w", "w1_2_b", "wf_0_w", "wf_0_b", "wf_2_w", "wf_2_b", "b1_w", "b1_b", "v_0_w",
             "v_0_b", "v_2_w", "v_2_b")
    for name, w in zip(names, ws):
        setattr(a, name, w.data_ptr())
    return a


def _wgrad_into(dy, x, out, colsum):
    """out = dy^T x, colsum = sum over rows of dy: csrc/wgrad.hip (fixed order) where it applies."""
    if tall_wgrad_supported(dy, x):
        tall_wgrad(dy, x, out=out, colsum=colsum)
    else:
        out.copy_(dy.t() @ x)
        colsum.copy_(dy.sum(0))


class _QmixFn(th.autograd.Function):
    """QMixer.forward in the shipped configuration: flexnet_qmix_forward (saving the first-layer outputs h1 [B, 256]),
    flexnet_qmix_backward (d agent_qs, and the per-sample gradients of the second-layer outputs and first-layer
    pre-activations when a mixer parameter needs its gradient) and the batch reductions dW = dY^T X of csrc/wgrad.hip."""

    @staticmethod
    def forward(ctx, q, x, save, *ws):
        q = q.contiguous()
        if x.stride(-1) != 1 or (x.shape[0] > 1 and x.stride(0) % 4 != 0) or x.data_ptr() % 16 != 0:
            x = x.contiguous()
            if x.data_ptr() % 16 != 0:          # already contiguous on a base that is not: contiguous() hands the view back
                x = x.clone()
        ws = [w.contiguous() for w in ws]
        B = q.shape[0]
        out = th.empty(B, dtype=th.float32, device=q.device)
        h1 = th.empty(B, 4 * _lib.FLEXNET_QMIX_EMBED, dtype=th.float32, device=q.device) if save else None
        a = _qmix_args(q, x, ws)
        a.q_tot = out.data_ptr()
        if h1 is not None:
            a.h1 = h1.data_ptr()
        _lib.launch("flexnet_qmix_forward", a)
        if save:
            ctx.save_for_backward(q, x, h1, *ws)
        return out

    @staticmethod
    def backward(ctx, g):
        q, x, h1, *ws = ctx.saved_tensors
        B, n = q.shape
        E = _lib.FLEXNET_QMIX_EMBED
        want_w = any(ctx.needs_input_grad[3:])
        g = g.reshape(B).contiguous()
        dq = th.empty(B, n, dtype=th.float32, device=q.device)
        a = _qmix_args(q, x, ws)
        a.h1, a.d_q_tot, a.d_agent_qs = h1.data_ptr(), g.data_ptr(), dq.data_ptr()
        if want_w:
            d_w1 = th.empty(B, E * n, dtype=th.float32, device=q.device)
            d_wf = th.empty(B, E, dtype=th.float32, device=q.device)
            d_pre1 = th.empty(B, 4 * E, dtype=th.float32, device=q.device)
            a.want_param_grads, a.d_w1, a.d_wf, a.d_pre1 = 1, d_w1.data_ptr(), d_wf.data_ptr(), d_pre1.data_ptr()
        _lib.launch("flexnet_qmix_backward", a)
        grads = [None] * len(ws)
        if want_w:
            S = x.shape[1]
            dev = q.device
            d1w = th.empty(4 * E, S, dtype=th.float32, device=dev)            # the four first layers, h1's unit order
            d1b = th.empty(4 * E, dtype=th.float32, device=dev)
            for c0 in (0, 2 * E):                                             # flexnet_wgrad: m <= 192 per call
                _wgrad_into(d_pre1[:, c0:c0 + 2 * E], x, d1w[c0:c0 + 2 * E], d1b[c0:c0 + 2 * E])
            dw12 = th.empty(E * n, E, dtype=th.float32, device=dev)
            db12 = th.empty(E * n, dtype=th.float32, device=dev)
            for c0 in range(0, E * n, 160):
                c1 = min(c0 + 160, E * n)
                _wgrad_into(d_w1[:, c0:c1], h1[:, 0:E], dw12[c0:c1], db12[c0:c1])
            dwf2 = th.empty(E, E, dtype=th.float32, device=dev)
            dbf2 = th.empty(E, dtype=th.float32, device=dev)
            _wgrad_into(d_wf, h1[:, E:2 * E], dwf2, dbf2)
            dv2 = th.empty(1, E, dtype=th.float32, device=dev)
            dbv2 = th.empty(1, dtype=th.float32, device=dev)
            _wgrad_into(g.view(B, 1), h1[:, 3 * E:4 * E], dv2, dbv2)
            # QMIX_PARAMS order: hyper_w_1.0, hyper_w_1.2, hyper_w_final.0, hyper_w_final.2, hyper_b_1, V.0, V.2
            grads = [d1w[0:E], d1b[0:E], dw12, db12, d1w[E:2 * E], d1b[E:2 * E], dwf2, dbf2,
                     d1w[2 * E:3 * E], d1b[2 * E:3 * E], d1w[3 * E:4 * E], d1b[3 * E:4 * E], dv2, dbv2]
            grads = [gr if need else None for gr, need in zip(grads, ctx.needs_input_grad[3:])]
        return (dq if ctx.needs_input_grad[0] else None, None, None, *grads)


# ---- SQDDPG's Shapley-value critic (madrl/models/sqddpg.py:35-104) -------------------------------------------------------
def sqddpg_fused_config(critic, n_agents, act_dim, sample_size):
    """The configuration csrc/sqddpg.hip implements (include/flexnet.h: flexnet_sqddpg_forward): a shared MLPCritic with hid
    64, ReLU and one output, the agent id columns, n <= 8 agents, act_dim <= 8 with n * act_dim <= 32."""
    return (_critic_config_ok(critic) and bool(critic.args.agent_id)
            and 1 <= n_agents <= 8 and 1 <= act_dim <= 8 and n_agents * act_dim <= 32 and sample_size >= 1
            and sample_size * n_agents <= 4096)


def sqddpg_draw(groups, n_agents, rng_state):
    """One uniform random permutation per coalition group on the device: pos [groups, n] (int32), pos[g, i] = position of
    agent i.  The stream is rng_state = [seed, step] (int64, device); the step advances on the device after the draw."""
    pos = th.empty(groups, n_agents, dtype=th.int32, device=rng_state.device)
    a = _lib.FlexSqddpgDrawArgs()
    a.groups, a.n_agents, a.rng_state, a.pos = groups, n_agents, rng_state.data_ptr(), pos.data_ptr()
    _lib.launch("flexnet_sqddpg_draw", a)
    rng_state[1:2].add_(1)
    return pos


def _sqddpg_args(z_shared, z_id, w_act, act, pos, ns, eps, layernorm, ps):
    a = _lib.FlexSqddpgArgs()
    a.batch, a.n_agents, a.act_dim = act.shape
    a.sample_size, a.layernorm, a.ln_eps = ns, int(layernorm), eps
    a.z_shared, a.z_id, a.w_act, a.act, a.pos = (z_shared.data_ptr(), z_id.data_ptr(), w_act.data_ptr(), act.data_ptr(),
                                                 pos.data_ptr())
    ln_w, ln_b, fc2_w, fc2_b, fc3_w, fc3_b = ps
    if layernorm:
        a.ln_w, a.ln_b = ln_w.data_ptr(), ln_b.data_ptr()
    a.fc2_w, a.fc2_b, a.fc3_w, a.fc3_b = fc2_w.data_ptr(), fc2_b.data_ptr(), fc3_w.data_ptr(), fc3_b.data_ptr()
    return a


class _SqddpgFn(th.autograd.Function):
    """phi [b, n] = mean over the ns coalitions of the critic's value of each agent's coalition row, and (want_q) the rows'
    values q [b, ns, n]: flexnet_sqddpg_forward / flexnet_sqddpg_backward.  Inputs: z_shared [b, 64] (fc1 of the
    observations + bias), z_id [n, 64], w_act [64, n a], act [b, n, a] (only agent i's own action takes a gradient from row
    (b, s, i)), pos [b ns, n]; then the tail's parameters."""

    @staticmethod
    def forward(ctx, z_shared, z_id, w_act, act, pos, ns, eps, layernorm, want_q, ln_w, ln_b, fc2_w, fc2_b, fc3_w, fc3_b):
        ctx.set_materialize_grads(False)
        z_shared, z_id, w_act, act = z_shared.contiguous(), z_id.contiguous(), w_act.contiguous(), act.contiguous()
        pos = pos.to(th.int32).contiguous()
        ps = [None if p is None else p.contiguous() for p in (ln_w, ln_b, fc2_w, fc2_b, fc3_w, fc3_b)]
        b, n, _ = act.shape
        phi = th.empty(b, n, dtype=th.float32, device=act.device)
        q = th.empty(b, ns, n, dtype=th.float32, device=act.device) if want_q else phi.new_empty(0)
        k = _sqddpg_args(z_shared, z_id, w_act, act, pos, ns, eps, layernorm, ps)
        k.phi = phi.data_ptr()
        if want_q:
            k.q = q.data_ptr()
        _lib.launch("flexnet_sqddpg_forward", k)
        ctx.ns, ctx.eps, ctx.layernorm = ns, eps, layernorm
        ctx.save_for_backward(z_shared, z_id, w_act, act, pos, *[p if p is not None else phi.new_empty(0) for p in ps])
        if not want_q:
            ctx.mark_non_differentiable(q)
        return phi, q

    @staticmethod
    def backward(ctx, d_phi, d_q):
        z_shared, z_id, w_act, act, pos, *ps = ctx.saved_tensors
        if not ctx.layernorm:
            ps[0] = ps[1] = None
        b, n, ad = act.shape
        dev = act.device
        need = ctx.needs_input_grad
        want_w = any(need[1:3]) or any(need[9:])
        d_phi = th.zeros(b, n, dtype=th.float32, device=dev) if d_phi is None else d_phi.contiguous()
        k = _sqddpg_args(z_shared, z_id, w_act, act, pos, ctx.ns, ctx.eps, ctx.layernorm, ps)
        k.d_phi = d_phi.data_ptr()
        if d_q is not None and d_q.numel() == b * ctx.ns * n:
            d_q = d_q.contiguous()
            k.d_q = d_q.data_ptr()
        dz = th.empty(b, 64, dtype=th.float32, device=dev) if need[0] else None
        da = th.empty(b, n, ad, dtype=th.float32, device=dev) if need[3] else None
        if dz is not None:
            k.d_z_shared = dz.data_ptr()
        if da is not None:
            k.d_act_own = da.data_ptr()
        grads = [None] * 8
        if want_w:
            ws = _scratch("sqddpg", dev, _lib.FLEXNET_SQDDPG_BWD_GRID * _lib.FLEXNET_SQDDPG_WS_ROW)
            grads = [th.empty(n, 64, device=dev), th.empty(64, n * ad, device=dev), th.zeros(64, device=dev),
                     th.zeros(64, device=dev), th.empty(64, 64, device=dev), th.empty(64, device=dev),
                     th.empty(1, 64, device=dev), th.empty(1, device=dev)]
            k.want_param_grads = 1
            k.workspace = ws.data_ptr()
            for name, t in zip(("d_z_id", "d_w_act", "d_ln_w", "d_ln_b", "d_fc2_w", "d_fc2_b", "d_fc3_w", "d_fc3_b"), grads):
                setattr(k, name, t.data_ptr())
        _lib.launch("flexnet_sqddpg_backward", k)
        gz_id, gw_act, *gp = [g if nd else None for g, nd in zip(grads, (need[1], need[2]) + tuple(need[9:]))]
        return (dz, gz_id, gw_act, da, None, None, None, None, None, *gp)


def sqddpg_shapley_fused(critic, obs2d, act, pos, ns, want_q=False, frozen=False):
    """(phi [b, n], q [b, ns, n] or None) of madrl/models/sqddpg.py:63-104 through csrc/sqddpg.hip.  fc1's observation
    block and bias form z_shared once per sample (tall_linear: flexnet_wgrad for dW_obs / db1); the reference's row layout
    [obs | coalition actions | onehot(i)] fixes the column blocks.  ``frozen``: the critic's parameters take no gradient
    (a policy sub-update)."""
    b, n, ad = act.shape
    W, bias = critic.fc1.weight, critic.fc1.bias
    *tail, eps = _tail_params(critic)
    if frozen:
        W, bias = W.detach(), bias.detach()
        tail = [None if p is None else p.detach() for p in tail]
    no = obs2d.shape[1]
    z_shared = tall_linear(obs2d, W[:, :no], bias)
    w_act = W[:, no:no + n * ad]
    z_id = W[:, no + n * ad:no + n * ad + n].t()
    phi, q = _SqddpgFn.apply(z_shared, z_id, w_act, act, pos, ns, eps, tail[0] is not None, want_q, *tail)
    return phi, (q if want_q else None)


# ---- SQDDPG with shared_params False: one critic per agent (csrc/sqddpg_unshared.hip) ------------------------------------------
def unshared_critics_switch():
    """FLEX_UNSHARED_CRITICS=1: FACMADDPG's and SQDDPG's per-agent critics (shared_params False) take the HIP kernels instead of
    the per-agent loop / the tensor composition.  Opt-in, and read from the environment at every call."""
    return os.environ.get("FLEX_UNSHARED_CRITICS", "") == "1"


def sqddpg_unshared_config(critics, n_agents, act_dim, sample_size):
    """The configuration csrc/sqddpg_unshared.hip implements (include/flexnet.h: flexnet_sqddpg_unshared_forward): one
    ``type(...) is MLPCritic`` per agent with hid 64, ReLU, one output and the agent id columns, all of one input width and one
    LayerNorm setting, fp32 contiguous device parameters, n <= 8 agents, act_dim <= 8 with n * act_dim <= 32."""
    critics = list(critics)
    if not (len(critics) == n_agents and 1 <= n_agents <= 8 and 1 <= act_dim <= 8 and n_agents * act_dim <= 32
            and sample_size >= 1 and sample_size * n_agents <= 4096):
        return False
    for c in critics:
        if type(c) is not MLPCritic or not (_critic_config_ok(c) and c.args.agent_id and getattr(c, "fused_tail", True)):
            return False
        if (c.fc1.weight.shape[1] != critics[0].fc1.weight.shape[1] or c.fc1.weight.shape[1] <= n_agents * act_dim + n_agents
                or bool(c.args.layernorm) != bool(critics[0].args.layernorm)):
            return False
        if _params_decline(_critic_unshared_params(c)) is not None:
            return False
    return True


class _SqddpgZSharedFn(th.autograd.Function):
    """z_shared [b, n, 64] of the per-agent critics: z_shared[:, i] = obs2d @ W_i[:, :no].T + b_i, one library GEMM on the
    stacked observation columns.  Backward: every agent's dW_obs (into the first ``no`` columns of a full-width zero gradient
    of its fc1.weight) and db in ONE flexnet_wgrad_batched call — agent i's rows dz[:, i] are an ordinary problem at row pitch
    64 n — from WGRAD_MIN_ROWS samples, the library GEMM below.  Inputs: obs2d [b, no], no, then (fc1.weight, fc1.bias) per
    agent."""

    @staticmethod
    def forward(ctx, obs2d, no, *wb):
        ws, bs = wb[0::2], wb[1::2]
        wcat = th.cat([w[:, :no] for w in ws], 0)
        z = th.addmm(th.cat(bs), obs2d, wcat.t())
        ctx.no, ctx.ld = no, ws[0].shape[1]
        ctx.save_for_backward(obs2d, wcat if obs2d.requires_grad else obs2d.new_empty(0))
        return z.view(obs2d.shape[0], len(ws), 64)

    @staticmethod
    def backward(ctx, dz):
        obs2d, wcat = ctx.saved_tensors
        dz = dz.contiguous()
        b, n, _ = dz.shape
        no, need = ctx.no, ctx.needs_input_grad
        grads = [None] * (2 * n)
        if any(need[2:]):
            gw = th.zeros(n, 64, ctx.ld, dtype=th.float32, device=dz.device)
            if b >= WGRAD_MIN_ROWS and tall_wgrad_supported(dz[:, 0], obs2d):
                gb = th.empty(n, 64, dtype=th.float32, device=dz.device)
                tall_wgrad_batched([(dz[:, i], obs2d, gw[i][:, :no], gb[i]) for i in range(n)])
            else:
                gw[:, :, :no] = (dz.view(b, n * 64).t() @ obs2d).view(n, 64, no)
                gb = dz.sum(0)
            for i in range(n):
                grads[2 * i], grads[2 * i + 1] = (gw[i] if need[2 + 2 * i] else None), (gb[i] if need[3 + 2 * i] else None)
        dx = dz.view(b, n * 64) @ wcat if need[0] else None
        return (dx, None, *grads)


_SQU_PER_AGENT = 7           # fc1.weight, then the tail: ln_w, ln_b, fc2_w, fc2_b, fc3_w, fc3_b


def _sqddpg_unshared_args(z_shared, act, pos, ns, eps, layernorm, no, ps):
    a = _lib.FlexSqddpgUnsharedArgs()
    a.batch, a.n_agents, a.act_dim = act.shape
    n, nka = act.shape[1], act.shape[1] * act.shape[2]
    a.sample_size, a.layernorm, a.ln_eps = ns, int(layernorm), eps
    a.ld_fc1 = ps[0][0].stride(0)
    a.z_shared, a.act, a.pos = z_shared.data_ptr(), act.data_ptr(), pos.data_ptr()
    for i, (w, ln_w, ln_b, fc2_w, fc2_b, fc3_w, fc3_b) in enumerate(ps):
        # the action columns and the agent's own id column of fc1.weight, read in place at the weight's row pitch
        a.w_act[i], a.w_id[i] = w.data_ptr() + 4 * no, w.data_ptr() + 4 * (no + nka + i)
        if layernorm:
            a.ln_w[i], a.ln_b[i] = ln_w.data_ptr(), ln_b.data_ptr()
        a.fc2_w[i], a.fc2_b[i], a.fc3_w[i], a.fc3_b[i] = fc2_w.data_ptr(), fc2_b.data_ptr(), fc3_w.data_ptr(), fc3_b.data_ptr()
    return a


class _SqddpgUnsharedFn(th.autograd.Function):
    """_SqddpgFn for one critic per agent: phi [b, n] and (want_q) q [b, ns, n] with row (b, s, i) through critic i —
    flexnet_sqddpg_unshared_forward / flexnet_sqddpg_unshared_backward.  Inputs: z_shared [b, n, 64] (_SqddpgZSharedFn), act
    [b, n, a] (only agent i's own action takes a gradient from row (b, s, i)), pos [b ns, n], ``no`` = fc1's observation columns;
    then per agent fc1.weight and the tail's parameters.  fc1.weight's gradient from here is zero outside its action columns and
    the agent's own id column."""

    @staticmethod
    def forward(ctx, z_shared, act, pos, ns, eps, layernorm, want_q, no, *flat):
        ctx.set_materialize_grads(False)
        z_shared, act = z_shared.contiguous(), act.contiguous()
        pos = pos.to(th.int32).contiguous()
        b, n, _ = act.shape
        ps = [list(flat[_SQU_PER_AGENT * i:_SQU_PER_AGENT * (i + 1)]) for i in range(n)]
        phi = th.empty(b, n, dtype=th.float32, device=act.device)
        q = th.empty(b, ns, n, dtype=th.float32, device=act.device) if want_q else phi.new_empty(0)
        k = _sqddpg_unshared_args(z_shared, act, pos, ns, eps, layernorm, no, ps)
        k.phi = phi.data_ptr()
        if want_q:
            k.q = q.data_ptr()
        _lib.launch("flexnet_sqddpg_unshared_forward", k)
        ctx.ns, ctx.eps, ctx.layernorm, ctx.no = ns, eps, layernorm, no
        ctx.save_for_backward(z_shared, act, pos, *[p for agent in ps for p in agent if p is not None])
        if not want_q:
            ctx.mark_non_differentiable(q)
        return phi, q

    @staticmethod
    def backward(ctx, d_phi, d_q):
        z_shared, act, pos, *saved = ctx.saved_tensors
        b, n, ad = act.shape
        ps = _regroup_params(saved, n, _SQU_PER_AGENT, ctx.layernorm, ln_slots=(1, 2))
        dev, no, nka = act.device, ctx.no, n * ad
        need = ctx.needs_input_grad
        d_phi = th.zeros(b, n, dtype=th.float32, device=dev) if d_phi is None else d_phi.contiguous()
        k = _sqddpg_unshared_args(z_shared, act, pos, ctx.ns, ctx.eps, ctx.layernorm, no, ps)
        k.d_phi = d_phi.data_ptr()
        if d_q is not None and d_q.numel() == b * ctx.ns * n:
            d_q = d_q.contiguous()
            k.d_q = d_q.data_ptr()
        dz = th.empty(b, n, 64, dtype=th.float32, device=dev) if need[0] else None
        da = th.empty(b, n, ad, dtype=th.float32, device=dev) if need[1] else None
        if dz is not None:
            k.d_z_shared = dz.data_ptr()
        if da is not None:
            k.d_act_own = da.data_ptr()
        out = [None] * (_SQU_PER_AGENT * n)
        want_w = any(need[8:])
        if want_w:
            ws = _scratch(("sqddpg_unshared", n), dev,
                          n * _lib.FLEXNET_SQDDPG_UNSHARED_BWD_GRID * _lib.FLEXNET_SQDDPG_UNSHARED_WS_ROW)
            g = dict(d_z_id=th.empty(n, 64, device=dev), d_w_act=th.empty(n, 64, nka, device=dev),
                     d_ln_w=th.zeros(n, 64, device=dev), d_ln_b=th.zeros(n, 64, device=dev),
                     d_fc2_w=th.empty(n, 64, 64, device=dev), d_fc2_b=th.empty(n, 64, device=dev),
                     d_fc3_w=th.empty(n, 64, device=dev), d_fc3_b=th.empty(n, device=dev))
            k.want_param_grads = 1
            k.workspace = ws.data_ptr()
            for name, t in g.items():
                setattr(k, name, t.data_ptr())
        _lib.launch("flexnet_sqddpg_unshared_backward", k)
        if want_w:
            gw = th.zeros(n, 64, ps[0][0].shape[1], dtype=th.float32, device=dev)
            gw[:, :, no:no + nka] = g["d_w_act"]
            gw[:, :, no + nka:no + nka + n].diagonal(dim1=0, dim2=2).copy_(g["d_z_id"].t())
            for i in range(n):
                per = [gw[i], g["d_ln_w"][i] if ctx.layernorm else None, g["d_ln_b"][i] if ctx.layernorm else None,
                       g["d_fc2_w"][i], g["d_fc2_b"][i], g["d_fc3_w"][i].view(1, 64), g["d_fc3_b"][i:i + 1]]
                for j, t in enumerate(per):
                    if need[8 + _SQU_PER_AGENT * i + j]:
                        out[_SQU_PER_AGENT * i + j] = t
        return (dz, da, None, None, None, None, None, None, *out)


def sqddpg_shapley_unshared(critics, obs2d, act, pos, ns, want_q=False, frozen=False):
    """(phi [b, n], q [b, ns, n] or None) of madrl/models/sqddpg.py:63-104 with one critic per agent (its else branch at
    :94-100) through csrc/sqddpg_unshared.hip.  z_shared [b, n, 64] comes from obs2d [b, n o] and each critic's observation
    columns and bias (_SqddpgZSharedFn); the reference's row layout [obs | coalition actions | onehot(i)] fixes the column
    blocks of every fc1.  ``frozen``: no critic parameter takes a gradient (a policy sub-update)."""
    critics = list(critics)
    no = obs2d.shape[1]
    wb, flat = [], []
    for c in critics:
        w, bias = c.fc1.weight, c.fc1.bias
        *tail, eps = _tail_params(c)
        if frozen:
            w, bias = w.detach(), bias.detach()
            tail = [None if p is None else p.detach() for p in tail]
        wb += [w, bias]
        flat += [w, *tail]
    z_shared = _SqddpgZSharedFn.apply(obs2d, no, *wb)
    phi, q = _SqddpgUnsharedFn.apply(z_shared, act, pos, ns, eps, bool(critics[0].args.layernorm), want_q, no, *flat)
    return phi, (q if want_q else None)


# ---- PPO (IPPO / MAPPO): madrl/learning_algorithms/ppo.py:14-69 around the networks ---------------------------------------
# Three pieces, each as a fused launch sequence of csrc/ppo.hip on the GPU and as the tensor composition of the same
# formulas everywhere else (CPU, fp64, more than 8 agents, a masked action_avail, cross-rank BatchNorm statistics): the
# composition is also what the GPU tests compare the kernels with.
def _loss_workspace(family, device, floats):
    """The fp64 statistics and loss partials of one call of ``family`` ("ppo", "coma"), read by that call's own finish launch: one
    workspace per (family, device, stream), so calls on different streams never share one (calls on one stream run in order)."""
    return _scratch((family, th.cuda.current_stream(device).cuda_stream), device, floats // 2, th.float64)


class _FusedLossFn(th.autograd.Function):
    """A loss whose gradients came out of the forward launch: ``apply(loss, x_1, dx_1, x_2, dx_2, ...)`` is ``loss`` with
    d loss / d x_k = dx_k (csrc/ppo.hip's losses, csrc/coma.hip's policy loss)."""

    @staticmethod
    def forward(ctx, loss, *pairs):
        ctx.save_for_backward(*pairs[1::2])
        return loss

    @staticmethod
    def backward(ctx, g):
        from .util import is_unit_seed
        unit = is_unit_seed(g)                          # the trainer's root gradient: the stored ones are the answer
        out = [None]
        for k, dx in enumerate(ctx.saved_tensors):
            out += [(dx if unit else dx * g) if ctx.needs_input_grad[1 + 2 * k] else None, None]
        return tuple(out)


def ppo_gae_torch(reward_norm, old_values, old_next_values, done, last_step, gamma, lambda_, chain_stride=1):
    """ppo.py:44-52 on chains: row i continues into row i + chain_stride.  The loop runs over the steps of a chain, every
    chain of the batch at once (stride 1: the reference's literal loop over the rows); each chain sees the literal loop's
    operations in the literal loop's order."""
    rows, n = reward_norm.shape
    stride = int(chain_stride)
    if stride < 1 or rows % stride != 0:
        raise ValueError(f"a batch of {rows} rows is not a whole number of steps of {stride} chains")
    steps = rows // stride
    done, last_step = done.reshape(steps, stride, 1), last_step.reshape(steps, stride, 1)
    mask = th.where(last_step != 0, 1.0 - done, th.ones_like(done))
    r, v, nv = (x.reshape(steps, stride, n) for x in (reward_norm, old_values, old_next_values))
    out = th.empty_like(r)
    last = 0
    for t in reversed(range(steps)):
        deltas = r[t] + gamma * nv[t] * mask[t] - v[t]
        last = deltas + gamma * lambda_ * last * mask[t]
        out[t] = last
    return out.reshape(rows, n)


def ppo_fused_supported(bns, *tensors):
    """csrc/ppo.hip covers fp32 CUDA tensors of up to 8 agents and training-mode BatchNorm1d modules with a momentum whose
    statistics are this rank's own (cross-rank statistics take the composition: sync_batchnorm)."""
    ok = all(t is None or (t.is_cuda and t.dtype == th.float32) for t in tensors)
    for bn in bns:
        if bn is not None:
            ok = ok and isinstance(bn, nn.BatchNorm1d) and bn.training and bn.momentum is not None and not _sync_active(bn) \
                and bn.num_features <= 8 and (not bn.track_running_stats or bn.running_mean.dtype == th.float32)
    return bool(ok)


def _ppo_bn_args(dst, bn):
    if bn is None:
        return
    dst.enabled, dst.eps, dst.momentum = 1, float(bn.eps), float(bn.momentum)
    if bn.affine:
        dst.weight, dst.bias = bn.weight.data_ptr(), bn.bias.data_ptr()
    if bn.track_running_stats:
        dst.running_mean, dst.running_var = bn.running_mean.data_ptr(), bn.running_var.data_ptr()
        dst.num_batches_tracked = bn.num_batches_tracked.data_ptr()


def ppo_gae(reward, old_values, old_next_values, done, last_step, gamma, lambda_, chain_stride=1, reward_bn=None, adv_bn=None,
            fused=True):
    """(reward_norm, advantages, advantages_norm) [rows, n], no gradient: the reward through ``reward_bn`` (None: as it is),
    GAE along the chains, the advantages through ``adv_bn`` (None: advantages_norm is advantages).  Both modules' running
    statistics move once, as their training-mode forward moves them."""
    rows, n = reward.shape
    stride = int(chain_stride)
    if stride < 1 or rows % stride != 0:
        raise ValueError(f"a batch of {rows} rows is not a whole number of steps of {stride} chains")
    old_values, old_next_values = old_values.reshape(rows, n), old_next_values.reshape(rows, n)
    done, last_step = done.reshape(rows), last_step.reshape(rows)
    with th.no_grad():
        if fused and n <= 8 and ppo_fused_supported((reward_bn, adv_bn), reward, old_values, old_next_values, done, last_step):
            r, v, nv, d, ls = (x.contiguous() for x in (reward, old_values, old_next_values, done, last_step))
            rn, adv = th.empty_like(r), th.empty_like(r)
            advn = th.empty_like(r) if adv_bn is not None else adv
            ws = _loss_workspace("ppo", r.device, _lib.FLEXNET_PPO_WS_FLOATS)
            a = _lib.FlexPpoGaeArgs()
            a.rows, a.chain_stride, a.n_agents, a.gamma, a.lambda_ = rows, stride, n, float(gamma), float(lambda_)
            a.reward, a.old_values, a.old_next_values, a.done, a.last_step = (x.data_ptr() for x in (r, v, nv, d, ls))
            _ppo_bn_args(a.reward_bn, reward_bn)
            _ppo_bn_args(a.adv_bn, adv_bn)
            a.reward_norm, a.advantages, a.advantages_norm = rn.data_ptr(), adv.data_ptr(), advn.data_ptr()
            a.workspace, a.workspace_floats = ws.data_ptr(), 2 * ws.numel()
            if _lib.try_launch("flexnet_ppo_gae", a):
                return rn, adv, advn
        if fused and reward.is_cuda:
            note_fallback("ppo_gae", f"agents {n}, dtype {reward.dtype}, cross-rank statistics or an evaluation-mode BatchNorm")
        rn = sync_batchnorm(reward_bn, reward.contiguous()) if reward_bn is not None else reward
        adv = ppo_gae_torch(rn, old_values, old_next_values, done, last_step, gamma, lambda_, stride)
        advn = sync_batchnorm(adv_bn, adv) if adv_bn is not None else adv
        return rn, adv, advn


def ppo_policy_loss_torch(means, log_stds, actions, old_log_prob, advantages, eps_clip, actions_avail=None):
    """ppo.py:19-33,36,57-61: (loss, ratios [rows, n]).  ``old_log_prob`` [rows, n, a] is summed over the action dimension
    here, as the reference sums it (model.py:313 hands the ACTION over in its place)."""
    from torch.distributions.normal import Normal
    if means.size(-1) > 1:
        means_, log_stds_ = means.sum(dim=1, keepdim=True), log_stds.sum(dim=1, keepdim=True)
    else:
        means_, log_stds_ = means, log_stds
    log_prob_a = Normal(means_, log_stds_.exp(), validate_args=False).log_prob(actions)
    if actions_avail is not None and getattr(actions_avail, "_flex_const", None) != 1.0:
        restore_mask = 1.0 - (actions_avail == 0).to(means.dtype)
        log_prob_a, old_log_prob = restore_mask * log_prob_a, restore_mask * old_log_prob
    log_prob_a, old_log_prob = log_prob_a.sum(dim=-1), old_log_prob.sum(dim=-1)
    ratios = th.exp(log_prob_a - old_log_prob.detach())
    assert ratios.size() == advantages.size()
    surr1 = ratios * advantages.detach()
    surr2 = th.clamp(ratios, 1 - eps_clip, 1 + eps_clip) * advantages.detach()
    return -th.min(surr1, surr2).mean(), ratios


def ppo_value_loss_torch(values, old_values, next_values, reward_norm, done, gamma, eps_clip, value_loss_coef):
    """ppo.py:53,63-68: (loss, returns [rows, n])."""
    returns = reward_norm + gamma * (1 - done.reshape(-1, 1)) * next_values.detach()
    assert old_values.size() == values.size()
    values_clipped = old_values + th.clamp(values - old_values, -eps_clip, eps_clip)
    surr1 = (values - returns).pow(2)
    surr2 = (values_clipped - returns).pow(2)
    return value_loss_coef * th.max(surr1, surr2).mean(), returns


def _ppo_policy_loss_fused(means, log_stds, actions, old_log_prob, advantages, eps_clip, every=True, per_row=None):
    """(loss, ratios) through csrc/ppo.hip's policy loss, or None where the configuration is not the kernel's or the library
    declines: flexnet_ppo_policy_loss for a fixed-std policy's log_stds (marked ``_flex_entropy``; the kernel takes the
    agent-summed log-std of one row), flexnet_ppo_policy_loss_rows for learned ones [rows, n, a], whose gradient comes out too.
    ``per_row`` given: that form whatever the configuration, so that the library itself answers."""
    rows, n, na = means.shape
    if per_row is None:
        per_row = getattr(log_stds, "_flex_entropy", None) is None
        if not (every and n <= 8 and na <= 8 and na > 1 and means.is_cuda and actions.shape == means.shape
                and ppo_fused_supported((), means, actions, advantages, old_log_prob, log_stds if per_row else None)
                and (not per_row or log_stds.shape == means.shape)):
            return None
    with th.no_grad():
        m, act, adv = means.detach().contiguous(), actions.contiguous(), advantages.reshape(rows, n).contiguous()
        if per_row:
            ls = log_stds.detach().expand_as(m).contiguous()
        else:
            ls = log_stds.detach()[:1].sum(dim=1).reshape(na).contiguous()        # the agent-summed log-std of one row
        old = old_log_prob.sum(dim=-1).expand(rows, n).contiguous() if old_log_prob is not None else None
        loss = th.empty((), dtype=th.float32, device=m.device)
        d_means, ratio = th.empty_like(m), th.empty(rows, n, dtype=th.float32, device=m.device)
        grads = (means, d_means)
        ws = _loss_workspace("ppo", m.device, _lib.FLEXNET_PPO_WS_FLOATS)
        a = _lib.FlexPpoPolicyRowsArgs() if per_row else _lib.FlexPpoPolicyArgs()
        a.rows, a.n_agents, a.act_dim, a.eps_clip = rows, n, na, float(eps_clip)
        a.means, a.actions, a.advantages = m.data_ptr(), act.data_ptr(), adv.data_ptr()
        setattr(a, "log_stds" if per_row else "log_std", ls.data_ptr())
        if old is not None:
            a.old_log_prob = old.data_ptr()
        a.loss, a.d_means, a.ratio = loss.data_ptr(), d_means.data_ptr(), ratio.data_ptr()
        if per_row and log_stds.requires_grad:
            grads += (log_stds, th.empty_like(m))
            a.d_log_stds = grads[-1].data_ptr()
        a.workspace, a.workspace_floats = ws.data_ptr(), 2 * ws.numel()
        if not _lib.try_launch("flexnet_ppo_policy_loss_rows" if per_row else "flexnet_ppo_policy_loss", a):
            return None
    return _FusedLossFn.apply(loss, *grads), ratio


def ppo_policy_loss(means, log_stds, actions, old_log_prob, advantages, eps_clip, actions_avail=None, fused=True):
    """(loss, ratios [rows, n] detached) of ppo.py:19-36,57-61.  ``old_log_prob``: [rows, n, a] as stored (summed here), or
    None for the reference's own choice, the action (model.py:313)."""
    rows, n, na = means.shape
    every = actions_avail is None or getattr(actions_avail, "_flex_const", None) == 1.0
    if fused:
        out = _ppo_policy_loss_fused(means, log_stds, actions, old_log_prob, advantages, eps_clip, every)
        if out is not None:
            return out
        if means.is_cuda:
            note_fallback("ppo_policy_loss", f"agents {n}, act_dim {na}, dtype {means.dtype}, every action available: {every}")
    loss, ratios = ppo_policy_loss_torch(means, log_stds, actions, actions if old_log_prob is None else old_log_prob,
                                         advantages, eps_clip, actions_avail)
    return loss, ratios.detach()


def ppo_value_loss(values, old_values, next_values, reward_norm, done, gamma, eps_clip, value_loss_coef, fused=True):
    """(loss, returns [rows, n]) of ppo.py:53,63-68; gradient w.r.t. ``values`` only."""
    rows, n = reward_norm.shape
    values2, old_values, next_values = values.reshape(rows, n), old_values.reshape(rows, n), next_values.reshape(rows, n).detach()
    if fused and n <= 8 and values.is_cuda and ppo_fused_supported((), values2, old_values, next_values, reward_norm, done):
        with th.no_grad():
            v, ov, nv, rn, d = (x.detach().contiguous() for x in (values2, old_values, next_values, reward_norm, done.reshape(rows)))
            loss = th.empty((), dtype=th.float32, device=v.device)
            d_values, returns = th.empty_like(v), th.empty_like(v)
            ws = _loss_workspace("ppo", v.device, _lib.FLEXNET_PPO_WS_FLOATS)
            a = _lib.FlexPpoValueArgs()
            a.rows, a.n_agents, a.gamma, a.eps_clip, a.value_loss_coef = rows, n, float(gamma), float(eps_clip), float(value_loss_coef)
            a.values, a.old_values, a.next_values, a.reward_norm, a.done = (x.data_ptr() for x in (v, ov, nv, rn, d))
            a.loss, a.d_values, a.returns = loss.data_ptr(), d_values.data_ptr(), returns.data_ptr()
            a.workspace, a.workspace_floats = ws.data_ptr(), 2 * ws.numel()
            ran = _lib.try_launch("flexnet_ppo_value_loss", a)
        if ran:
            return _FusedLossFn.apply(loss, values, d_values.view(values.shape)), returns
    if fused and values.is_cuda:
        note_fallback("ppo_value_loss", f"agents {n}, dtype {values.dtype}")
    loss, returns = ppo_value_loss_torch(values2, old_values, next_values, reward_norm, done, gamma, eps_clip, value_loss_coef)
    return loss, returns.detach()


# ---- COMA (madrl/models/coma.py:126-189): the counterfactual baseline and the policy loss -----------------------------------
# The baseline as the launch of csrc/coma.hip on the GPU (from the first-layer pre-activation of the rows on the actions
# taken: no [s b n, width] input exists) and as the reference's materialising composition everywhere else (CPU, fp64,
# configurations the kernel does not cover); the composition is also what the GPU tests compare the kernel with.
def coma_rows(obs, act, agent_id=True, per_row=False):
    """coma.py:41-78 (continuous branch): the critic's input rows [.., n, (n + 1) o + n + n a] =
    [o_1 .. o_n | o_i | onehot(i) | actions].  ``obs`` [b, n, o]; ``act`` [b, n, a] (every row of a sample sees the same n
    actions) or, with ``per_row``, [m b, n, n a] (row-specific actions, the observations repeated m times: the baseline's
    merged actions)."""
    b, n, o = obs.shape
    m = act.size(0) // b
    parts = [obs.reshape(b, 1, n * o).expand(b, n, n * o), obs]
    if agent_id:
        parts.append(th.eye(n, device=obs.device, dtype=obs.dtype).expand(b, n, n))
    inp = th.cat(parts, dim=-1)
    if per_row:
        inp = inp.unsqueeze(0).expand(m, b, n, inp.size(-1)).reshape(m * b, n, -1)
        acts = act.reshape(m * b, n, -1)
    else:
        acts = act.reshape(b, 1, -1).expand(b, n, act[0].numel())
    return th.cat((inp, acts), dim=-1)


def coma_merged_actions(act, sampled):
    """coma.py:142-147: [s b, n, n a] — row (s, b, i) holds the actions taken with agent i's own replaced by its draw."""
    s, b, n, a = sampled.shape
    mask = th.eye(n, device=act.device, dtype=act.dtype).view(1, 1, n, n, 1)
    merged = act.view(1, b, 1, n, a) * (1.0 - mask) + sampled.view(s, b, 1, n, a) * mask
    return merged.reshape(s * b, n, n * a)


def coma_baseline_torch(critics, obs, act, sampled, agent_id=True, s_chunk=None):
    """(baseline [b, n], q_sampled [s, b, n]) of coma.py:139-149 as the reference forms them: the [s b n, width] rows are
    materialised and handed to the critic (``critics``: the shared MLPCritic, or one per agent).  ``s_chunk``: that many
    draws at a time (the full set is 23 GB at the trainer's batch)."""
    s, b, n, _ = sampled.shape
    out = []
    step = s if s_chunk is None else int(s_chunk)
    for s0 in range(0, s, step):
        rows = coma_rows(obs, coma_merged_actions(act, sampled[s0:s0 + step]), agent_id, per_row=True)
        if isinstance(critics, nn.Module) and not isinstance(critics, nn.ModuleList):
            v = critics(rows.reshape(-1, rows.size(-1)), None)[0]
        else:
            v = th.stack([net(rows[:, i, :], None)[0] for i, net in enumerate(critics)], dim=1)
        out.append(v.reshape(-1, b, n))
    q_sampled = th.cat(out, dim=0)
    return q_sampled.mean(dim=0), q_sampled


def coma_fused_config(critic, n_agents, act_dim):
    """The configuration csrc/coma.hip implements (sqddpg_fused_config's): a shared MLPCritic with hid 64, ReLU and one
    output, the agent id columns, n <= 8 agents, act_dim <= 8 with n * act_dim <= 32."""
    return sqddpg_fused_config(critic, n_agents, act_dim, 1)


def coma_act_columns(critic, n_agents, act_dim):
    """The action columns [64, n a] of fc1.weight in COMA's row layout (the last n a columns)."""
    return critic.fc1.weight[:, critic.fc1.in_features - n_agents * act_dim:]


def coma_baseline(critic, z1, act, sampled, want_q=False, want_values=False, fused=True):
    """(baseline [b, n], q_sampled [s, b, n] or None, values [b, n] or None), no gradient, from ``z1`` [b n, hid] — fc1's
    pre-activation of the rows on the actions taken: row (s, b, i) is the tail of z1[b, i] + W_act,i (sampled[s, b, i] -
    act[b, i]).  ``values`` is the tail of z1 itself.  On the GPU one launch of csrc/coma.hip; otherwise (and with
    ``fused=False``) the same update as tensor operations."""
    s, b, n, a = sampled.shape
    with th.no_grad():
        w_act = coma_act_columns(critic, n, a)
        *tail, eps = _tail_params(critic)
        if fused and z1.is_cuda:
            if z1.dtype == th.float32 and sampled.dtype == th.float32 and coma_fused_config(critic, n, a):
                z1c, actc, smp, wa = z1.contiguous(), act.to(th.float32).contiguous(), sampled.contiguous(), w_act.contiguous()
                ps = [None if p is None else p.detach().contiguous() for p in tail]
                base = th.empty(b, n, dtype=th.float32, device=z1.device)
                qs = th.empty(s, b, n, dtype=th.float32, device=z1.device) if want_q else None
                q = th.empty(b, n, dtype=th.float32, device=z1.device) if want_values else None
                k = _lib.FlexComaBaselineArgs()
                k.batch, k.n_agents, k.act_dim, k.sample_size = b, n, a, s
                k.layernorm, k.ln_eps = int(ps[0] is not None), float(eps)
                k.z1, k.w_act, k.act, k.sampled = z1c.data_ptr(), wa.data_ptr(), actc.data_ptr(), smp.data_ptr()
                if ps[0] is not None:
                    k.ln_w, k.ln_b = ps[0].data_ptr(), ps[1].data_ptr()
                k.fc2_w, k.fc2_b, k.fc3_w, k.fc3_b = (p.data_ptr() for p in ps[2:])
                k.baseline = base.data_ptr()
                if qs is not None:
                    k.q_sampled = qs.data_ptr()
                if q is not None:
                    k.q = q.data_ptr()
                if _lib.try_launch("flexnet_coma_baseline", k):
                    return base, qs, q
            note_fallback("coma", f"hid {critic.args.hid_size}, act {critic.args.hid_activation}, agent_id "
                                  f"{critic.args.agent_id}, agents {n}, act_dim {a}, dtype {z1.dtype}")
        delta = (sampled - act.unsqueeze(0)).to(z1.dtype)                                   # [s, b, n, a]
        z = z1.view(1, b, n, -1) + th.einsum("sbia,hia->sbih", delta, w_act.reshape(-1, n, a))
        qs = critic.forward_from_hidden(z.reshape(s * b * n, -1), need_hidden=False)[0].reshape(s, b, n)
        q = critic.forward_from_hidden(z1, need_hidden=False)[0].reshape(b, n) if want_values else None
        return qs.mean(dim=0), (qs if want_q else None), q


def coma_policy_loss_torch(means, log_stds, actions, actions_avail, advantages):
    """coma.py:132,183-188: (loss, log_prob_a [b, n] after the mask and the sum over the action dimension)."""
    from torch.distributions.normal import Normal
    log_prob_a = Normal(means, log_stds.exp(), validate_args=False).log_prob(actions)
    if actions_avail is not None and getattr(actions_avail, "_flex_const", None) != 1.0:
        log_prob_a = (1.0 - (actions_avail == 0).to(means.dtype)) * log_prob_a
    log_prob_a = log_prob_a.sum(dim=-1)
    assert log_prob_a.size() == advantages.size()
    return (-advantages.detach() * log_prob_a).mean(), log_prob_a


def coma_policy_loss(means, log_stds, actions, actions_avail, values=None, baseline=None, advantages=None, fused=True):
    """(loss, log_prob_a [b, n] detached) of coma.py:180-188: -mean(adv log p) with adv = ``advantages`` when given (the
    normalised ones), else ``values`` - ``baseline``; nothing but the means and the log-stds takes a gradient."""
    rows, n, na = means.shape
    every = actions_avail is None or getattr(actions_avail, "_flex_const", None) == 1.0
    uniform = getattr(log_stds, "_flex_entropy", None) is not None
    given = [t for t in (values, baseline, advantages) if t is not None]
    if (fused and means.is_cuda and n <= 8 and na <= 8 and actions.shape == means.shape
            and all(t.is_cuda and t.dtype == th.float32 for t in [means, actions, log_stds] + given)
            and (every or (actions_avail.is_cuda and actions_avail.shape == means.shape))):
        with th.no_grad():
            m, act = means.detach().contiguous(), actions.contiguous()
            ls = log_stds.detach() if uniform else log_stds.detach().expand_as(m).contiguous()
            loss = th.empty((), dtype=th.float32, device=m.device)
            d_means = th.empty_like(m)
            want_dl = log_stds.requires_grad and not uniform
            d_log_stds = th.empty_like(m) if want_dl else m.new_empty(0)
            logp = th.empty(rows, n, dtype=th.float32, device=m.device)
            ws = _loss_workspace("coma", m.device, _lib.FLEXNET_COMA_WS_FLOATS)
            k = _lib.FlexComaPolicyArgs()
            k.rows, k.n_agents, k.act_dim, k.log_std_uniform = rows, n, na, int(uniform)
            k.means, k.log_stds, k.actions = m.data_ptr(), ls.data_ptr(), act.data_ptr()
            keep = []
            if not every:
                keep.append(actions_avail.to(th.float32).contiguous())
                k.avail = keep[-1].data_ptr()
            if advantages is not None:
                keep.append(advantages.detach().reshape(rows, n).contiguous())
                k.advantages = keep[-1].data_ptr()
            else:
                keep += [values.detach().reshape(rows, n).contiguous(), baseline.detach().reshape(rows, n).contiguous()]
                k.q, k.baseline = keep[-2].data_ptr(), keep[-1].data_ptr()
            k.loss, k.d_means, k.log_prob = loss.data_ptr(), d_means.data_ptr(), logp.data_ptr()
            if want_dl:
                k.d_log_stds = d_log_stds.data_ptr()
            k.workspace, k.workspace_floats = ws.data_ptr(), 2 * ws.numel()
            ran = _lib.try_launch("flexnet_coma_policy_loss", k)
        if ran:
            return _FusedLossFn.apply(loss, means, d_means, log_stds, d_log_stds), logp
    if fused and means.is_cuda:
        note_fallback("coma_policy_loss", f"agents {n}, act_dim {na}, dtype {means.dtype}")
    adv = advantages if advantages is not None else values - baseline
    loss, logp = coma_policy_loss_torch(means, log_stds, actions, actions_avail, adv.reshape(rows, n))
    return loss, logp.detach()


# ---- MAAC: the attention critic (madrl/critics/maac_critic.py; csrc/attn_critic.hip) ----------------------------------------
class AttentionCritic(nn.Module):
    """madrl/critics/maac_critic.py:6-159 (continuous branch): ONE critic for all agents.  Per agent an encoder of
    [o_j | a_j], an encoder of o_i, a critic head on [sa_i | other_i] and a bias head on s_i; shared key, selector and value
    extractors per attention head.  Agent i attends over the other n - 1 agents: logits sel_i . key_j, scaled by
    1 / sqrt(attend_dim), softmax, other_i = sum_j w_ij val_j.  The state_dict keys are the reference's.

    ``forward(obs [b, n, o], act [b, n, a])`` -> (q - b [b, n], regulariser [n]): the regulariser is 1e-3 times the sum over
    heads of the mean of the UNSCALED logits squared (maac_critic.py:125-134, 154).  ``pre``: a list that receives every
    LeakyReLU pre-activation, [b, n, .] each (tests clear the samples where one of them ties at zero)."""

    def __init__(self, args):
        super().__init__()
        self.args = args
        self.hidden_dim, self.attend_heads, self.nagents = args.hid_size, args.attend_heads, args.agent_num
        assert self.hidden_dim % self.attend_heads == 0
        if not args.continuous:
            raise NotImplementedError("discrete control is outside the flexibility-provision hot path")
        sdim, adim, hid = args.obs_size, args.action_dim, self.hidden_dim
        self.norm_in = bool(args.norm_in)
        self.critic_encoders, self.critics = nn.ModuleList(), nn.ModuleList()
        self.biases, self.state_encoders = nn.ModuleList(), nn.ModuleList()
        for _ in range(self.nagents):
            enc = nn.Sequential()
            if self.norm_in:
                enc.add_module("enc_bn", nn.BatchNorm1d(sdim + adim, affine=False))
            enc.add_module("enc_fc1", nn.Linear(sdim + adim, hid))
            enc.add_module("enc_nl", nn.LeakyReLU())
            self.critic_encoders.append(enc)
            critic = nn.Sequential()
            critic.add_module("critic_fc1", nn.Linear(2 * hid, hid))
            critic.add_module("critic_nl", nn.LeakyReLU())
            critic.add_module("critic_fc2", nn.Linear(hid, 1))
            self.critics.append(critic)
            bias = nn.Sequential()
            bias.add_module("bias_fc1", nn.Linear(hid, hid))
            bias.add_module("bias_nl", nn.LeakyReLU())
            bias.add_module("bias_fc2", nn.Linear(hid, 1))
            self.biases.append(bias)
            senc = nn.Sequential()
            if self.norm_in:
                senc.add_module("s_enc_bn", nn.BatchNorm1d(sdim, affine=False))
            senc.add_module("s_enc_fc1", nn.Linear(sdim, hid))
            senc.add_module("s_enc_nl", nn.LeakyReLU())
            self.state_encoders.append(senc)
        attend_dim = hid // self.attend_heads
        self.key_extractors, self.selector_extractors, self.value_extractors = nn.ModuleList(), nn.ModuleList(), nn.ModuleList()
        for _ in range(self.attend_heads):
            self.key_extractors.append(nn.Linear(hid, attend_dim, bias=False))
            self.selector_extractors.append(nn.Linear(hid, attend_dim, bias=False))
            self.value_extractors.append(nn.Sequential(nn.Linear(hid, attend_dim), nn.LeakyReLU()))

    def forward(self, obs, act, pre=None):
        n = self.nagents
        sa_in = th.cat((obs, act), dim=-1)
        lrelu = F.leaky_relu

        def first(seq, x, bn, fc):
            if self.norm_in:
                x = getattr(seq, bn)(x)
            return getattr(seq, fc)(x)

        z_sa = th.stack([first(e, sa_in[:, j], "enc_bn", "enc_fc1") for j, e in enumerate(self.critic_encoders)], dim=1)
        z_s = th.stack([first(e, obs[:, i], "s_enc_bn", "s_enc_fc1") for i, e in enumerate(self.state_encoders)], dim=1)
        sa, s = lrelu(z_sa), lrelu(z_s)                                              # [b, n, hid]
        diag = th.eye(n, dtype=th.bool, device=obs.device)
        others, reg, z_vals = [], 0.0, []
        for k_ext, s_ext, v_ext in zip(self.key_extractors, self.selector_extractors, self.value_extractors):
            keys, sels, z_v = k_ext(sa), s_ext(s), v_ext[0](sa)                      # [b, n, d]
            z_vals.append(z_v)
            logits = th.matmul(sels, keys.transpose(1, 2))                           # [b, i, j]
            reg = reg + logits.masked_fill(diag, 0.0).pow(2).sum(dim=(0, 2)) / (logits.shape[0] * (n - 1))
            w = (logits / math.sqrt(keys.shape[-1])).masked_fill(diag, float("-inf")).softmax(dim=-1)
            others.append(th.matmul(w, lrelu(z_v)))
        critic_in = th.cat([sa] + others, dim=-1)
        z_c = th.stack([c.critic_fc1(critic_in[:, i]) for i, c in enumerate(self.critics)], dim=1)
        z_b = th.stack([m.bias_fc1(s[:, i]) for i, m in enumerate(self.biases)], dim=1)
        q = th.cat([c.critic_fc2(lrelu(z_c[:, i])) for i, c in enumerate(self.critics)], dim=1)
        bb = th.cat([m.bias_fc2(lrelu(z_b[:, i])) for i, m in enumerate(self.biases)], dim=1)
        if pre is not None:
            pre += [z_sa, z_s, z_c, z_b] + z_vals
        return q - bb, 1e-3 * reg


_ATTN_CRITIC_TABLES = ("enc_w", "enc_b", "senc_w", "senc_b", "c1_w", "c1_b", "c2_w", "c2_b", "b1_w", "b1_b", "b2_w", "b2_b")
_ATTN_CRITIC_SHARED = ("key_w", "sel_w", "val_w", "val_b")
# call classes that take csrc/attn_critic.hip by default (each is gated by its own measurement);
# FLEX_ATTN_CRITIC_FUSED=0: none does — the A/B switch of tools/maac_bench.py and profiles/maac_bench.txt
ATTN_CRITIC_FUSED = {k: os.environ.get("FLEX_ATTN_CRITIC_FUSED", "1") != "0" for k in ("no_grad", "value", "policy")}


def _attn_critic_params(critic):
    """The parameters of an AttentionCritic in FlexAttnCriticArgs order: twelve per agent, then the four shared ones."""
    flat = []
    for e, se, c, bm in zip(critic.critic_encoders, critic.state_encoders, critic.critics, critic.biases):
        flat += [e.enc_fc1.weight, e.enc_fc1.bias, se.s_enc_fc1.weight, se.s_enc_fc1.bias, c.critic_fc1.weight, c.critic_fc1.bias,
                 c.critic_fc2.weight, c.critic_fc2.bias, bm.bias_fc1.weight, bm.bias_fc1.bias, bm.bias_fc2.weight, bm.bias_fc2.bias]
    v = critic.value_extractors[0][0]
    return flat + [critic.key_extractors[0].weight, critic.selector_extractors[0].weight, v.weight, v.bias]


def attn_critic_declines(critic, obs, act):
    """Why csrc/attn_critic.hip does not cover ``critic`` on obs [b, n, o] / act [b, n, a], or None."""
    if type(critic) is not AttentionCritic:
        return f"a {type(critic).__name__}"
    n = critic.nagents
    if critic.attend_heads != 1 or critic.norm_in or critic.hidden_dim != _lib.FLEXNET_HID:
        return f"attend_heads {critic.attend_heads}, norm_in {critic.norm_in}, hid {critic.hidden_dim}"
    for name, t in (("obs", obs), ("act", act)):
        if not (t.is_cuda and t.dtype == th.float32 and t.dim() == 3 and t.shape[1] == n and t.shape[0] == obs.shape[0]):
            return f"{name} {tuple(t.shape)} {t.dtype} on {t.device.type} for {n} agents"
    b, _, o = obs.shape
    a = act.shape[2]
    if not (2 <= n <= _lib.FLEXNET_MAX_AGENTS and 1 <= o <= _lib.FLEXNET_MAX_OBS and o % 4 == 0 and 1 <= a <= _lib.FLEXNET_MAX_ACT
            and o == critic.args.obs_size and a == critic.args.action_dim):
        return f"agents {n}, obs {o}, actions {a}"
    if not 1 <= b <= _lib.FLEXNET_ATTN_CRITIC_MAX_BATCH:
        return f"{b} samples"
    if not getattr(critic, "fused", True):
        return "fused passes switched off"
    return _params_decline(_attn_critic_params(critic))


def _attn_critic_tables(k, flat, n):
    """The pointers of ``flat`` (``_attn_critic_params``' order) into the forward's or the backward's struct ``k``."""
    _fill_tables(k, _ATTN_CRITIC_TABLES, [flat[12 * i:12 * i + 12] for i in range(n)], n)
    names = {f[0] for f in k._fields_}
    for c, name in enumerate(_ATTN_CRITIC_SHARED):
        if name in names:
            setattr(k, name, flat[12 * n + c].data_ptr())


def _attn_critic_eager_only():
    if not mlp_actor_allowed():
        raise RuntimeError("csrc/attn_critic.hip is launched eagerly only (nets.mlp_actor_allowed): never under a capture")


def _attn_critic_launch_forward(flat, obs, act, saves=None):
    """One flexnet_attn_critic_forward call on contiguous obs [b, n, o] / act [b, n, a]: (q [b, n], reg [n], stage [3, b n, 64]
    = sa | key | val), or None when the library answers FLEXNET_EUNSUPPORTED.  ``saves`` = (five [5, b n, 64], w [b, n, n])."""
    _attn_critic_eager_only()
    b, n, o = obs.shape
    dev = obs.device
    stage = th.empty(3, b * n, 64, dtype=th.float32, device=dev)
    q = th.empty(b, n, dtype=th.float32, device=dev)
    reg = th.empty(n, dtype=th.float32, device=dev)
    ws = th.empty(((b + 31) // 32) * n, dtype=th.float32, device=dev)
    k = _lib.FlexAttnCriticArgs()
    k.batch, k.n_agents, k.obs_dim, k.act_dim = b, n, o, act.shape[2]
    k.obs, k.act = obs.data_ptr(), act.data_ptr()
    _attn_critic_tables(k, flat, n)
    k.sa, k.key, k.val = (stage[c].data_ptr() for c in range(3))
    k.q, k.reg, k.workspace, k.workspace_floats = q.data_ptr(), reg.data_ptr(), ws.data_ptr(), ws.numel()
    if saves is not None:
        five, w = saves
        k.save_s, k.save_sel, k.save_other, k.save_hc, k.save_hb = (five[c].data_ptr() for c in range(5))
        k.save_w = w.data_ptr()
    if not _lib.try_launch("flexnet_attn_critic_forward", k):
        return None
    return q, reg, stage


def fused_attn_critic_forward(critic, obs, act):
    """maac_critic.py:86-159 without an autograd graph in ONE launch (and the regulariser's small second one) at any batch
    size: (q - b [b, n], regulariser [n]), or None after ``note_fallback("maac", ...)`` when it declines on GPU tensors.
    Never called under a capture (``mlp_actor_allowed``)."""
    why = attn_critic_declines(critic, obs, act)

    def launch():
        return _attn_critic_launch_forward(_attn_critic_params(critic), obs.contiguous(), act.contiguous())
    out = _fused_inference("maac", why, obs.is_cuda, "flexnet_attn_critic_forward", launch)
    return None if out is None else (out[0], out[1])


class _AttnCriticFn(th.autograd.Function):
    """The attention critic for an update batch as ONE autograd node (csrc/attn_critic.hip): the fused forward with its saves
    and one backward launch.  ``param_grads`` (the value sub-update; the actions carry no gradient): the gradients at the seven
    pre-activations, then flexnet_wgrad_batched for every weight — per agent the encoder's observation and action blocks, the
    state encoder, the critic head's two blocks and the bias head's first layer over the agent's rows through the row pitch,
    the two [1, 64] output layers against dq's column, and K, Q, V over all b n rows — with the [64] bias gradients as the
    column sums of the same passes; the output layers' bias gradients, +- the sum of dq, come from the backward launch.  Without (the policy sub-update, critic frozen): d_act alone.  The regulariser is returned
    detached: no optimiser ever steps a parameter on it.  Bit-reproducible."""

    @staticmethod
    def forward(ctx, obs, act, param_grads, *flat):
        b, n, _ = obs.shape
        obs, act = obs.contiguous(), act.contiguous()
        five = th.empty(5, b * n, 64, dtype=th.float32, device=obs.device)             # s | sel | other | hc | hb
        w = th.empty(b, n, n, dtype=th.float32, device=obs.device)
        out = _attn_critic_launch_forward(flat, obs, act, (five, w))
        if out is None:
            _lib.check(_lib.FLEXNET_EUNSUPPORTED, "flexnet_attn_critic_forward")
        q, reg, stage = out
        ctx.param_grads = bool(param_grads)
        ctx.save_for_backward(obs, act, stage, five, w, *flat)
        ctx.mark_non_differentiable(reg)
        ctx.set_materialize_grads(False)
        return q, reg

    @staticmethod
    def backward(ctx, dq, _dreg):
        obs, act, stage, five, w = ctx.saved_tensors[:5]
        flat = ctx.saved_tensors[5:]
        b, n, o = obs.shape
        a = act.shape[2]
        none = (None,) * (3 + len(flat))
        if dq is None:
            return none
        _attn_critic_eager_only()
        dev, rows = obs.device, b * n
        pg = ctx.param_grads and any(ctx.needs_input_grad[3:])
        want_act = ctx.needs_input_grad[1]
        dq = dq.contiguous()
        scratch = th.empty(2, rows, 64, dtype=th.float32, device=dev)
        g_dl = th.empty(b, n, n, dtype=th.float32, device=dev)

        def args(param_grads):
            k = _lib.FlexAttnCriticBwdArgs()
            k.batch, k.n_agents, k.obs_dim, k.act_dim, k.param_grads = b, n, o, a, int(param_grads)
            k.dq, k.w = dq.data_ptr(), w.data_ptr()
            k.sa, k.key, k.val = (stage[c].data_ptr() for c in range(3))
            k.s, k.sel, _, k.hc, k.hb = (five[c].data_ptr() for c in range(5))
            _attn_critic_tables(k, flat, n)
            k.g_direct, k.g_other, k.g_dl = scratch[0].data_ptr(), scratch[1].data_ptr(), g_dl.data_ptr()
            return k

        d_act = None
        if want_act:
            d_act = th.empty(b, n, a, dtype=th.float32, device=dev)
            k = args(False)
            k.d_act = d_act.data_ptr()
            _lib.launch("flexnet_attn_critic_backward", k)
        if not pg:
            return (None, d_act) + none[2:]
        g = th.empty(7, rows, 64, dtype=th.float32, device=dev)       # dz_c | dz_b | dz_s | d_sel | d_key | dz_v | dz_sa
        k = args(True)
        k.dz_c, k.dz_b, k.dz_s, k.d_sel, k.d_key, k.dz_v, k.dz_sa = (g[c].data_ptr() for c in range(7))
        d_out_b = th.empty(2, n, 1, dtype=th.float32, device=dev)     # critic_fc2.bias | bias_fc2.bias: +- sum_b dq
        ws = th.empty(2 * ((b + 31) // 32) * n, dtype=th.float32, device=dev)          # (fp64 partials)
        k.d_c2_b, k.d_b2_b, k.workspace, k.workspace_floats = d_out_b[0].data_ptr(), d_out_b[1].data_ptr(), ws.data_ptr(), ws.numel()
        _lib.launch("flexnet_attn_critic_backward", k)
        dz_c, dz_b, dz_s, d_sel, d_key, dz_v, dz_sa = (g[c].view(b, n, 64) for c in range(7))
        sa, s3, other, hc, hb = stage[0].view(b, n, 64), five[0].view(b, n, 64), five[2].view(b, n, 64), \
            five[3].view(b, n, 64), five[4].view(b, n, 64)
        new = lambda *shape: th.empty(*shape, dtype=th.float32, device=dev)      # noqa: E731
        d_enc_w, d_senc_w, d_c1_w, d_b1_w = new(n, 64, o + a), new(n, 64, o), new(n, 64, 128), new(n, 64, 64)
        d_vec = new(4, n, 64)                                                     # d_enc_b | d_senc_b | d_c1_b | d_b1_b
        d_out_w = new(2, n, 1, 64)                                                # critic_fc2 | bias_fc2 (sign below)
        d_kqv, d_val_b = new(3, 64, 64), new(64)
        problems = []
        for i in range(n):
            problems += [(dz_sa[:, i], obs[:, i], d_enc_w[i, :, :o], d_vec[0, i]), (dz_sa[:, i], act[:, i], d_enc_w[i, :, o:], None),
                         (dz_s[:, i], obs[:, i], d_senc_w[i], d_vec[1, i]),
                         (dz_c[:, i], sa[:, i], d_c1_w[i, :, :64], d_vec[2, i]), (dz_c[:, i], other[:, i], d_c1_w[i, :, 64:], None),
                         (dz_b[:, i], s3[:, i], d_b1_w[i], d_vec[3, i]),
                         (dq[:, i:i + 1], hc[:, i], d_out_w[0, i], None), (dq[:, i:i + 1], hb[:, i], d_out_w[1, i], None)]
        problems += [(g[4], stage[0], d_kqv[0], None), (g[3], five[0], d_kqv[1], None), (g[5], stage[0], d_kqv[2], d_val_b)]
        tall_wgrad_batched(problems)
        d_out_w[1].neg_()                                             # out = q - b: the bias head's output layer sees -dq
        grads = []
        for i in range(n):
            grads += [d_enc_w[i], d_vec[0, i], d_senc_w[i], d_vec[1, i], d_c1_w[i], d_vec[2, i], d_out_w[0, i], d_out_b[0, i],
                      d_b1_w[i], d_vec[3, i], d_out_w[1, i], d_out_b[1, i]]
        grads += [d_kqv[0], d_kqv[1], d_kqv[2], d_val_b]
        return (None, d_act, None, *grads)


def attn_critic_train(critic, obs, act, param_grads=True):
    """The node on obs [b, n, o] / act [b, n, a] (``attn_critic_declines`` is None): (q - b [b, n], regulariser [n] detached)."""
    return _AttnCriticFn.apply(obs, act, param_grads, *_attn_critic_params(critic))


def attn_critic(critic, obs, act, critic_frozen=False):
    """(q - b [b, n], regulariser [n]) of an AttentionCritic on obs [b, n, o] / act [b, n, a].  On GPU tensors, for EAGER calls
    (``mlp_actor_allowed``: while a HIP graph is captured or audited the composition runs, silently): csrc/attn_critic.hip —
    the forward launch under no_grad at any batch size, the node ``_AttnCriticFn`` with gradients from WGRAD_MIN_ROWS rows
    (``critic_frozen``: d_act only, else parameter gradients only) — or, after ``note_fallback("maac", ...)``, the module's own
    composition where the kernel declines.  On the CPU the composition, silently.  With the node the regulariser comes back
    detached."""
    if not obs.is_cuda or not mlp_actor_allowed():
        return critic(obs, act)
    with_grad = th.is_grad_enabled() and (act.requires_grad or obs.requires_grad or any(p.requires_grad for p in critic.parameters()))
    kind = "no_grad" if not with_grad else "policy" if critic_frozen else "value"
    if not ATTN_CRITIC_FUSED[kind] or (with_grad and obs.shape[0] * obs.shape[1] < WGRAD_MIN_ROWS):
        return critic(obs, act)
    if not with_grad:
        out = fused_attn_critic_forward(critic, obs, act)
        return out if out is not None else critic(obs, act)
    why = attn_critic_declines(critic, obs, act)
    if why is None and (obs.requires_grad or (act.requires_grad and not critic_frozen)):
        why = "gradients for the observations, or for actions and parameters at once"
    if why is not None:
        note_fallback("maac", "update pass: " + why)
        return critic(obs, act)
    return attn_critic_train(critic, obs, act, param_grads=not critic_frozen)
