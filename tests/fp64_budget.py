"""The fp64 error budget of the shared actor and critic kernels, as a plain helper module.

A HIP kernel is held against the fp64 evaluation of the module it replaces (``ref64``: a ``.double()`` copy of the module on
the ``.double()`` inputs), and its error may not exceed ``MARGIN`` times the error the fp32 PyTorch composition makes against
the same fp64 numbers on the same inputs, plus ``FLOOR_ULPS`` fp32 ulps of the tensor's scale (``within_budget``).  The
yardstick is measured in the test that uses it, never taken from a kernel.  ``families`` names the inputs at which the kernels'
LayerNorm, gate and ReLU code can go wrong without zero-mean, unit-scale inputs noticing; ``clear_ties`` removes from a
gradient comparison the rows whose ReLU side is arbitrary in any fp32 form.

The compositions below (``actor_plain``, ``mlp_actor_plain``, ``lnrelu_plain``, ``critic_tail_plain``, ``critic_plain``,
``critic_first_layer_plain``, ``coma_baseline_plain``, ``sqddpg_plain``, ``qmix_plain``) are the layers of nets.RNNAgent /
nets.MLPAgent / nets.MLPCritic / nets.QMixer written with torch.nn.functional alone, in whatever dtype the module has: the modules' own forward takes the
project's HIP weight-gradient kernels at update sizes (the mixer's: csrc/qmix.hip on any GPU tensors), which neither the yardstick nor the fp64 reference may.
tests/test_fp64_budget_cpu.py pins them to the modules' forward (1e-12 in fp64)."""
import copy
from typing import NamedTuple

import torch as th
import torch.nn.functional as F

MARGIN = 3.0          # tests/test_qmix_gpu.py's factor for the same comparison: two correct fp32 evaluations that differ in
#                       summation order have errors of the same magnitude, a wrong term shows as a ratio of 10 or more
FLOOR_ULPS = 8.0      # the gate path h' = (1 - z) n + z h: three transcendental evaluations of about 1 ulp each plus the
#                       combining arithmetic; on small cases err_t can be near zero by luck
ULP = 2.0 ** -24
TINY = 1.1754944e-38  # fp32's smallest normal: a reference that is exactly zero asks for exactly zero
TIE_CAP = 0.02


def ref64(module):
    """The plain high-precision reference: a deep copy of ``module`` (or of each module of a list) in fp64."""
    if isinstance(module, (list, tuple)):
        return [ref64(m) for m in module]
    return copy.deepcopy(module).double()


def within_budget(kernel, torch32, ref, *, margin=MARGIN, floor_ulps=FLOOR_ULPS, name):
    """assert max|kernel - ref| <= margin * max|torch32 - ref| + floor_ulps * 2^-24 * max(max|ref|, tiny) for one tensor; the
    figures are printed in one line whether or not the assertion holds.  A kernel value that is not finite where the
    reference is fails (NaN compares false)."""
    ref = ref.detach().double()
    assert kernel.shape == ref.shape and torch32.shape == ref.shape, (name, kernel.shape, torch32.shape, ref.shape)
    if ref.numel() == 0:
        return 0.0
    err_k = float((kernel.detach().double() - ref).abs().max())
    err_t = float((torch32.detach().double() - ref).abs().max())
    scale = float(ref.abs().max())
    ratio = err_k / err_t if err_t > 0 else (0.0 if err_k == 0 else float("inf"))
    line = f"fp64-budget {name} err_k={err_k:.3e} err_t={err_t:.3e} ratio={ratio:.3g} scale={scale:.3e}"
    print(line)
    bound = margin * err_t + floor_ulps * ULP * max(scale, TINY)
    assert err_k <= bound, f"{line} bound={bound:.3e}"
    return ratio


# ---------------------------------------------------------------------------------------------------------------------------
# modules under test

def make_agent(obs_dim, n_agents, act_dim, layernorm=True, device="cpu", seed=0):
    """tests/test_actor_gpu.py's agent: every parameter 0.3 randn, not the tiny default init — every term matters."""
    import types
    from safe_marl_amd.nets import RNNAgent
    th.manual_seed(seed)
    args = types.SimpleNamespace(hid_size=64, layernorm=layernorm, action_dim=act_dim, agent_num=n_agents, hid_activation="relu")
    agent = RNNAgent(obs_dim + n_agents, args)
    with th.no_grad():
        for p in agent.parameters():
            p.copy_(th.randn_like(p) * 0.3)
    return agent.to(device)


def make_critic(layernorm=True, device="cpu", seed=0, in_features=745):
    """tests/test_critic_gpu.py's critic: every parameter 0.2 randn."""
    import types
    from safe_marl_amd.nets import MLPCritic
    th.manual_seed(seed)
    c = MLPCritic(in_features, 1, types.SimpleNamespace(hid_size=64, layernorm=layernorm, hid_activation="relu", agent_id=True))
    with th.no_grad():
        for p in c.parameters():
            p.copy_(th.randn_like(p) * 0.2)
    return c.to(device)


def make_mlp_agent(obs_dim, n_agents, act_dim, layernorm=True, device="cpu", seed=0):
    """An MLPAgent (agent_type mlp) with ``make_agent``'s parameters: every one 0.3 randn."""
    import types
    from safe_marl_amd.nets import MLPAgent
    th.manual_seed(seed)
    args = types.SimpleNamespace(hid_size=64, layernorm=layernorm, action_dim=act_dim, agent_num=n_agents, hid_activation="relu")
    agent = MLPAgent(obs_dim + n_agents, args)
    with th.no_grad():
        for p in agent.parameters():
            p.copy_(th.randn_like(p) * 0.3)
    return agent.to(device)


def make_mixer(n_agents, obs_size, device="cpu", seed=0, zero_rows=False):
    """A nets.QMixer in the shipped configuration (two-layer hypernetworks, embed 64, not gated, no skip) with
    tests/test_qmix_gpu.py's parameters: every one 0.1 randn, drawn on the CPU.  ``zero_rows`` as there: exact zeros in rows of
    hyper_w_1.2 and hyper_w_final.2, whose outputs then are exactly zero on every sample — abs' sign(0) = 0 must come through."""
    from safe_marl_amd.nets import QMixer
    from safe_marl_amd.util import convert
    th.manual_seed(seed)
    m = QMixer(convert(dict(agent_num=n_agents, obs_size=obs_size, mixing_embed_dim=64, hypernet_layers=2, hypernet_embed=64,
                            hyper_initialization_nonzeros=0, gated=False, skip_connections=False)))
    with th.no_grad():
        for p in m.parameters():
            p.copy_(th.randn_like(p) * 0.1)
        if zero_rows:
            m.hyper_w_1[2].weight[::7].zero_()
            m.hyper_w_1[2].bias[::7].zero_()
            m.hyper_w_final[2].weight[::5].zero_()
            m.hyper_w_final[2].bias[::5].zero_()
    return m.to(device)


# ---------------------------------------------------------------------------------------------------------------------------
# the plain compositions

def with_ids(obs, n_agents):
    """[rows, obs_dim] -> [rows, obs_dim + n]: the one-hot id block of model.py:105-108, row r being agent r % n."""
    eye = th.eye(n_agents, dtype=obs.dtype, device=obs.device)
    return th.cat((obs, eye[th.arange(obs.shape[0], device=obs.device) % n_agents]), -1)


def layer_norm_running_sum(z, weight, bias, eps):
    """LayerNorm over 64 units with the statistics accumulated in the dtype of ``z`` one addend after the other in the order of
    the tile scheme's lanes before their repair (csrc/flex_mfma_tile.h ``row_stats``): lane half h holds units 8 q + 4 h + j of
    both 32-unit tiles and adds z0[r] + z1[r] for r = 0 .. 15 onto a running sum; the two halves meet at the end.  The mean of
    64 equal values then is off by an ulp or two and rstd = eps^-1/2 multiplies that: the third wrong evaluation
    tests/test_fp64_budget_cpu.py has the budget reject."""
    r = th.arange(16, device=z.device)
    halves = []
    for h in range(2):
        u = 8 * (r // 4) + 4 * h + (r % 4)
        halves.append((z[:, u], z[:, 32 + u]))
    part = []
    for z0, z1 in halves:
        p = th.zeros_like(z[:, 0])
        for k in range(16):
            p = p + (z0[:, k] + z1[:, k])
        part.append(p)
    mean = ((part[0] + part[1]) * (1.0 / 64)).unsqueeze(1)
    part = []
    for z0, z1 in halves:
        v = th.zeros_like(z[:, 0])
        for k in range(16):
            d0, d1 = z0[:, k] - mean[:, 0], z1[:, k] - mean[:, 0]
            v = v + (d0 * d0 + d1 * d1)
        part.append(v)
    rstd = th.rsqrt((part[0] + part[1]) * (1.0 / 64) + eps).unsqueeze(1)
    return ((z - mean) * rstd) * weight + bias


def _first_layer(module, obs, n_agents, agent_id, agent_index):
    """fc1 of rows [rows, obs_dim] without the id columns: the id column of agent r % n (or ``agent_index``) added."""
    W = module.fc1.weight
    o = obs.shape[1]
    z = F.linear(obs, W[:, :o], module.fc1.bias)
    if agent_id:
        ids = W[:, o:].t()
        z = z + (ids[th.arange(obs.shape[0], device=obs.device) % n_agents] if agent_index is None else ids[agent_index])
    return z


def mlp_actor_plain(agent, obs, n_agents, agent_id=True, agent_index=None, running_sum=False):
    """mlp_agent.py:20-32 on rows [rows, obs_dim] without the id columns: (means, h, first ReLU's pre-activation, second
    ReLU's).  Row r is agent r % n_agents, or every row agent ``agent_index``.  ``running_sum``: ``layer_norm_running_sum``
    in LayerNorm's place."""
    pre1 = _first_layer(agent, obs, n_agents, agent_id, agent_index)
    if agent.args.layernorm:
        ln = agent.layernorm
        pre1 = (layer_norm_running_sum if running_sum else lambda z, w, b, e: F.layer_norm(z, (64,), w, b, e))(
            pre1, ln.weight, ln.bias, ln.eps)
    pre2 = F.linear(th.relu(pre1), agent.fc2.weight, agent.fc2.bias)
    h = th.relu(pre2)
    return F.linear(h, agent.fc3.weight, agent.fc3.bias), h, pre1, pre2


def actor_plain(agent, obs, hidden, n_agents, agent_id=True, ln_units=64, drop_id_of=None, agent_index=None):
    """rnn_agent.py:25-33 on rows [rows, obs_dim] without the id columns: (means, new hidden, ReLU pre-activation).  Row r is
    agent r % n_agents, or every row agent ``agent_index`` (one of the per-agent modules of shared_params False on its rows).
    ``ln_units`` / ``drop_id_of``: the two wrong evaluations tests/test_fp64_budget_cpu.py has the budget reject — LayerNorm's
    mean taken over fewer units, one agent's id-column addend left out."""
    W = agent.fc1.weight
    o = obs.shape[1]
    z = F.linear(obs, W[:, :o], agent.fc1.bias)
    if agent_id:
        ids = W[:, o:].t()
        if drop_id_of is not None:
            ids = ids.clone()
            ids[drop_id_of] = 0.0
        z = z + (ids[th.arange(obs.shape[0], device=obs.device) % n_agents] if agent_index is None else ids[agent_index])
    if agent.args.layernorm:
        ln = agent.layernorm
        if ln_units == 64:
            pre = F.layer_norm(z, (64,), ln.weight, ln.bias, ln.eps)
        else:
            mean = z[:, :ln_units].mean(1, keepdim=True)
            var = (z - mean).square().mean(1, keepdim=True)
            pre = (z - mean) * th.rsqrt(var + ln.eps) * ln.weight + ln.bias
    else:
        pre = z
    h = agent.rnn(th.relu(pre), hidden.reshape(-1, 64))
    return agent.fc2(h), h, pre


def lnrelu_plain(z, bias, ids, ln_w, ln_b, n_agents, eps=1e-5):
    """relu(LayerNorm(z + bias + id column)) (tests/test_lnrelu_gpu.py's ``_reference``): (output, ReLU pre-activation)."""
    x = z
    if bias is not None:
        x = x + bias
    if ids is not None:
        x = (x.view(-1, n_agents, 64) + ids.unsqueeze(0)).reshape(-1, 64)
    if ln_w is not None:
        x = F.layer_norm(x, (64,), ln_w, ln_b, eps)
    return th.relu(x), x


def critic_tail_plain(critic, z):
    """mlp_critic.py:27-31 from the first layer's output: (q, first ReLU's pre-activation, second ReLU's)."""
    pre1 = z
    if critic.args.layernorm:
        ln = critic.layernorm
        pre1 = F.layer_norm(z, (64,), ln.weight, ln.bias, ln.eps)
    pre2 = F.linear(th.relu(pre1), critic.fc2.weight, critic.fc2.bias)
    return F.linear(th.relu(pre2), critic.fc3.weight, critic.fc3.bias), pre1, pre2


def critic_plain(critic, rows):
    """mlp_critic.py:27-35 on materialised input rows [rows, in_features]: (q [rows, 1], first ReLU's pre-activation, second
    ReLU's)."""
    return critic_tail_plain(critic, F.linear(rows, critic.fc1.weight, critic.fc1.bias))


CRITIC_FORMS = {"maddpg": (True, True), "mappo": (True, False), "ippo": (False, False), "iddpg": (False, True)}   # (shared, x2)


def critic_rows(obs, act, i, form, agent_id=True):
    """Agent i's critic input rows [b, width] of tests/test_critic_unshared_gpu.py's four forms from obs [b, n, o] and act
    [b, n, a]: [o_1 .. o_n | onehot(i) | a_1 .. a_n] (maddpg.py:33-54, the other agents' actions detached; mappo without the
    actions) or [o_i | onehot(i) | a_i] (iddpg.py:32-59; ippo without the action)."""
    shared, has_act = CRITIC_FORMS[form]
    b, n, _ = obs.shape
    parts = [obs.reshape(b, -1) if shared else obs[:, i]]
    if agent_id:
        parts.append(F.one_hot(th.full((b,), i, device=obs.device), n).to(obs.dtype))
    if has_act:
        if shared:
            own = th.zeros(1, n, 1, dtype=act.dtype, device=act.device)
            own[0, i, 0] = 1.0
            parts.append((act.detach() * (1.0 - own) + act * own).reshape(b, -1))
        else:
            parts.append(act[:, i])
    return th.cat(parts, 1)


def coma_baseline_plain(critic, z1, act, sampled):
    """coma.py:139-149 from fc1's pre-activation ``z1`` [b n, 64] of the rows on the actions taken (COMA's row layout: the
    action columns are fc1.weight's last n a): z(s, b, i) = z1[b, i] + W_act[:, i a:(i + 1) a] (sampled[s, b, i] - act[b, i]),
    then the tail.  Returns (baseline [b, n], q_sampled [s, b, n], values [b, n], the pre-activations of the sampled rows and
    of the rows themselves: four tensors [.., 64])."""
    s, b, n, a = sampled.shape
    w_act = critic.fc1.weight[:, critic.fc1.in_features - n * a:].reshape(-1, n, a)                 # [64, n, a]
    delta = sampled - act.unsqueeze(0)
    z = z1.view(1, b, n, -1) + (delta.unsqueeze(-2) * w_act.permute(1, 0, 2)).sum(-1)               # [s, b, n, 64]
    qs, pre1, pre2 = critic_tail_plain(critic, z.reshape(s * b * n, -1))
    q, vpre1, vpre2 = critic_tail_plain(critic, z1)
    qs = qs.reshape(s, b, n)
    return qs.mean(0), qs, q.reshape(b, n), (pre1, pre2, vpre1, vpre2)


def sqddpg_plain(critic, obs, act, pos, ns):
    """sqddpg.py:63-104 on the coalitions ``pos`` [b ns, n] (pos[g, i]: the position of agent i in group g = b ns + s): the
    critic on the materialised rows [obs_1 .. obs_n | block p = the action of the agent at position p if p <= pos[g, i],
    else 0 | onehot(i)], only agent i's own action keeping its gradient.  obs [b, n, o], act [b, n, a].  Returns (phi [b, n],
    q [b, ns, n], first ReLU's pre-activation, second ReLU's — [b ns n, 64] each)."""
    b, n, a = act.shape
    dev = act.device
    pos = pos.long().view(b, ns, n)
    who = th.empty_like(pos).scatter_(2, pos, th.arange(n, device=dev).expand(b, ns, n))           # the agent at position p
    ordered = act.unsqueeze(1).expand(b, ns, n, a).gather(2, who.unsqueeze(-1).expand(b, ns, n, a)).unsqueeze(2)
    p = th.arange(n, device=dev).view(1, 1, 1, n)
    own = (p == pos.unsqueeze(-1)).to(act.dtype).unsqueeze(-1)                                      # [b, ns, i, p, 1]
    before = (p < pos.unsqueeze(-1)).to(act.dtype).unsqueeze(-1)
    acts = ordered.detach() * before + ordered * own                                                # [b, ns, i, p, a]
    rows = th.cat((obs.reshape(b, 1, 1, -1).expand(b, ns, n, -1), acts.reshape(b, ns, n, n * a),
                   th.eye(n, dtype=act.dtype, device=dev).expand(b, ns, n, n)), -1)
    q, pre1, pre2 = critic_plain(critic, rows.reshape(b * ns * n, -1))
    q = q.view(b, ns, n)
    return q.mean(1), q, pre1, pre2


QMIX_RELU_HEADS = ("hyper_w_1", "hyper_w_final", "V")
QMIX_WRONG = ("abs_grad_one_at_zero", "drop_last_agent", "elu_slope_one")


def qmix_plain(mixer, agent_qs, states, wrong=None, taps=None):
    """qmix.py:53-81 (nets.QMixer.forward_torch) in the shipped configuration on agent_qs [B, n] and states [B, S], in the
    module's dtype: (q_tot [B], the pre-activations whose side of a kink is arbitrary in fp32 — the first-layer outputs of the
    three ReLU heads hyper_w_1, hyper_w_final, V, [B, 64] each, then the outputs of hyper_w_1 [B, 64 n] and hyper_w_final
    [B, 64] before ``abs``).  ELU is C1 at 0: no tie.  ``taps``: a dict that receives the two linear taps, ``b1`` [B, 64] and
    ``v`` [B, 1] (with the pre-activations, every bias gradient's per-sample addends are a gradient into one of these).
    ``wrong``: one of QMIX_WRONG, the wrong evaluations tests/test_fp64_budget_cpu.py has the budget reject — abs' gradient
    taken as +1 where its argument is exactly zero, the last agent's term left out of the mixing sum, ELU's slope taken as 1 on
    its negative branch (values unchanged: only the backward is wrong)."""
    assert wrong is None or wrong in QMIX_WRONG, wrong
    n, B = mixer.n_agents, agent_qs.shape[0]
    x, q = states.reshape(B, -1), agent_qs.reshape(B, n)

    def first(head):
        return F.linear(x, head[0].weight, head[0].bias)

    def absolute(t):
        if wrong == "abs_grad_one_at_zero":
            return t.abs() + (t == 0).to(t.dtype) * (t - t.detach())
        return t.abs()

    pre_w1, pre_wf, pre_v = (first(getattr(mixer, name)) for name in QMIX_RELU_HEADS)
    out_w1 = F.linear(F.relu(pre_w1), mixer.hyper_w_1[2].weight, mixer.hyper_w_1[2].bias)
    out_wf = F.linear(F.relu(pre_wf), mixer.hyper_w_final[2].weight, mixer.hyper_w_final[2].bias)
    v = F.linear(F.relu(pre_v), mixer.V[2].weight, mixer.V[2].bias)
    b1 = F.linear(x, mixer.hyper_b_1.weight, mixer.hyper_b_1.bias)
    w1 = absolute(out_w1).view(B, n, 64)
    if wrong == "drop_last_agent":
        mix = th.bmm(q[:, None, :n - 1], w1[:, :n - 1])
    else:
        mix = th.bmm(q[:, None, :], w1)
    z = mix + b1.view(B, 1, 64)
    hidden = F.elu(z)
    if wrong == "elu_slope_one":
        hidden = hidden.detach() + (z - z.detach())
    q_tot = th.bmm(hidden, absolute(out_wf).view(B, 64, 1)) + v.view(B, 1, 1)
    if taps is not None:
        taps.update(b1=b1, v=v)
    return q_tot.view(B), [pre_w1, pre_wf, pre_v, out_w1, out_wf]


# the bias gradients of the mixer as sums over the samples: index into qmix_plain's pre-activations, or the name of a tap
QMIX_BIAS_ADDENDS = {"hyper_w_1.0.bias": 0, "hyper_w_final.0.bias": 1, "V.0.bias": 2, "hyper_w_1.2.bias": 3,
                     "hyper_w_final.2.bias": 4, "hyper_b_1.bias": "b1", "V.2.bias": "v"}


def qmix_run(mixer, agent_qs, states, w, dtype, wrong=None):
    """One training pass of ``qmix_plain`` with the loss (q_tot w).sum(), everything cast to ``dtype`` (``mixer`` already is):
    (q_tot, d agent_qs, {parameter name: gradient}, {bias name: fb.row_sum_rounding of its per-sample addends}, the
    pre-activations detached)."""
    q = agent_qs.detach().to(dtype).requires_grad_(True)
    taps = {}
    q_tot, pre = qmix_plain(mixer, q, states.detach().to(dtype), wrong=wrong, taps=taps)
    loss = (q_tot * w.detach().to(dtype)).sum()
    params = dict(mixer.named_parameters())
    where = {name: (pre[k] if isinstance(k, int) else taps[k]) for name, k in QMIX_BIAS_ADDENDS.items()}
    addends = th.autograd.grad(loss, list(where.values()), retain_graph=True)
    floors = {name: row_sum_rounding(a).reshape(params[name].shape) for name, a in zip(where, addends)}
    grads = th.autograd.grad(loss, [q] + list(params.values()))
    return q_tot.detach(), grads[0], dict(zip(params, grads[1:])), floors, [p.detach() for p in pre]


def critic_first_layer_plain(critic, obs_cols, act_cols, n_agents):
    """maddpg.py:33-76 on replayed actions: fc1 of [obs_all | onehot(i) | act_all] for every agent i of every sample, from
    fc1's column blocks: [b * n, 64]."""
    W = critic.fc1.weight
    no, na = obs_cols.shape[1], act_cols.shape[1]
    shared = F.linear(obs_cols, W[:, :no]) + F.linear(act_cols, W[:, no + n_agents:no + n_agents + na]) + critic.fc1.bias
    return (shared.unsqueeze(1) + W[:, no:no + n_agents].t().unsqueeze(0)).reshape(-1, 64)


def td_loss_plain(q, next_q, reward, done, gamma, bn):
    """maddpg.py:100-123 behind model.py:308-323: mean((BatchNorm(reward) + gamma (1 - done) next_q - q)^2), the BatchNorm on
    batch statistics (training mode)."""
    if bn is not None:
        reward = F.batch_norm(reward, None, None, bn.weight, bn.bias, True, 0.0, bn.eps)
    returns = reward + gamma * (1.0 - done.view(-1, 1)) * next_q
    return (returns - q).square().mean()


def gate_rounding(agent, obs, hidden, n_agents, noise, std, agent_index=None):
    """What fp32 rounding in the hidden half of the GRU's gate pre-activations alone does to the actor's four outputs, element
    by element, to first order at the fp64 evaluation (``agent`` and inputs in fp64) — errors that a correct fp32 kernel
    reaches whatever its summation order.  It matters on rows with a large hidden state (the saturated family, |h| = 40); on
    0.5 randn rows it comes to a fraction of an ulp.

    The hidden half of gate unit j's pre-activation on row r is a sum of 64 terms w_jk h_rk of mean square t^2 = mean_k (w_jk
    h_rk)^2.  The partial sum after k terms has mean square k t^2 and its rounding is uniform within 2^-24 of it, variance
    (2^-24)^2 k t^2 / 3; summed over k: sigma = 2^-24 * 64 t / sqrt(6), one for each of a_r, a_z and gh_n (the x half, |x| of
    order 1, adds nothing to speak of).  The three roundings of a unit and those of different units are independent, so their
    effects add in quadrature.  With h' = n + z (h - n), n = tanh(gi_n + r gh_n):
        s_h^2   = [z (1 - z) (h - n) sigma_z]^2 + [(1 - z)(1 - n^2)]^2 ([r sigma_n]^2 + [r (1 - r) gh_n sigma_r]^2)  [rows, 64]
        s_m^2   = fc2_w^2 s_h^2    (only units whose gates are in transition contribute)                             [rows, act]
        d_h = 3 s_h,  d_means = 3 s_m,  d_action = (1 - action^2) d_means,  d_env_action = d_action / 2      (3 sigma)
    On unsaturated rows the gates' slopes spread the rounding over every row alike and the fp32 composition's own error is the
    yardstick.  On saturated rows it falls on the few (row, unit) pairs in transition, the largest error of a small batch is
    one element's, and two correct evaluations then differ there by more than the margin of 3 — which is never widened.  A
    tensor's floor is the largest of its elements' figures, so a tensor none of whose elements hangs on a gate in transition
    (an action behind a saturated tanh) keeps 8 ulps."""
    import math
    with th.no_grad():
        means, _, pre = actor_plain(agent, obs, hidden, n_agents, agent_index=agent_index)
        h = hidden.reshape(-1, 64)
        rnn = agent.rnn
        gi = F.linear(th.relu(pre), rnn.weight_ih, rnn.bias_ih)
        gh = F.linear(h, rnn.weight_hh, rnn.bias_hh)
        sigma = ULP * 64.0 / math.sqrt(6.0) * (h.square() @ rnn.weight_hh.square().t() / 64.0).sqrt()       # [rows, 192]
        r, z = th.sigmoid(gi[:, :64] + gh[:, :64]), th.sigmoid(gi[:, 64:128] + gh[:, 64:128])
        gh_n = gh[:, 128:]
        n = th.tanh(gi[:, 128:] + r * gh_n)
        var_h = (z * (1 - z) * (h - n) * sigma[:, 64:128]).square() + ((1 - z) * (1 - n * n)).square() * (
            (r * sigma[:, 128:]).square() + (r * (1 - r) * gh_n * sigma[:, :64]).square())
        d_m = 3.0 * (var_h @ agent.fc2.weight.square().t()).sqrt()
        action = th.tanh(means + std * noise.to(means.dtype))
        d_a = (1 - action * action) * d_m
    return {"hidden": 3.0 * var_h.sqrt(), "means": d_m, "action": d_a, "env_action": 0.5 * d_a}


def row_sum_rounding(addends):
    """What fp32 rounding of the partial sums alone does to a gradient that is a sum over rows, element by element: ``addends``
    [rows, ...] are the fp64 terms whose sum over dim 0 is the gradient (a bias gradient's are the rows of dL/d pre-activation).

    The N rows' terms of an element have mean m and variance v, so the partial sum after k terms, in whatever order the rows
    are taken, has mean square k^2 m^2 + k (1 - k / N) v (the drift to the sum N m that is known, and a random walk tied to it at
    both ends); its rounding is uniform within 2^-24 of it (gate_rounding's model; half an ulp is between 2^-25 and 2^-24 of
    the value, so measured running sums have 0.74 of this sigma), variance (2^-24)^2 (k^2 m^2 + k (1 - k / N) v) / 3.  Summed
    over k up to N: sigma = 2^-24 sqrt((m^2 N^3 / 3 + v N^2 / 6) / 3), which for terms of zero mean and mean square t^2 (m^2 of
    the order t^2 / N) is 2^-24 N t / sqrt(6) — a running sum, the least accurate order a correct fp32 kernel
    may use (the tile kernels keep a running sum per lane or per work-group over its tiles and fold those in a tree, which lies
    between this and a balanced tree).  The figure is 3 sigma.  It matters where the terms cancel: the gradient, and with it
    the 8-ulp floor, is then far smaller than the partial sums, and the fp32 composition — a tree sum — can come out with an
    error of a fraction of an ulp by luck (d_fc3.bias, one number, over 257 rows: 2e-10 on a gradient of 7e-3, a running
    sum's sigma 8e-9).  Where nothing cancels (v = 0) it is sqrt(N) / 3 ulps of the gradient N m: 10 ulps at 1 000 rows.
    tests/test_fp64_budget_cpu.py holds the derivation against running fp32 sums with and without drift, and that a budget
    with this floor still rejects a gradient off by 1e-5 of itself."""
    import math
    a = addends.detach().double()
    n = float(a.shape[0])
    return 3.0 * ULP * ((a.mean(0).square() * n ** 3 / 3.0 + a.var(0, unbiased=False) * n ** 2 / 6.0) / 3.0).sqrt()


def tail_sum_floors(g_q, g_pre1, g_pre2, pre1, pre2, ln):
    """``row_sum_rounding`` of the vector-sum gradients of an MLPCritic's tail from the fp64 reference's row gradients: ``g_q``
    [rows, 1], ``g_pre1`` / ``g_pre2`` [rows, 64] = dL / d(q, first ReLU's pre-activation, second ReLU's) with the
    pre-activations themselves; ``ln`` the fp64 LayerNorm or None.  {parameter name: floor, shaped as the parameter}."""
    out = {"fc3.bias": row_sum_rounding(g_q).reshape(1), "fc3.weight": row_sum_rounding(g_q * th.relu(pre2)).reshape(1, 64),
           "fc2.bias": row_sum_rounding(g_pre2)}
    if ln is not None:
        out["layernorm.bias"] = row_sum_rounding(g_pre1)
        out["layernorm.weight"] = row_sum_rounding(g_pre1 * (pre1 - ln.bias) / ln.weight)       # dL/dy xhat
    return out


def floor_ulps(extra, ref):
    """FLOOR_ULPS plus the largest figure of an element-wise floor ``extra`` (or None) in ulps of the scale of ``ref``: what
    ``within_budget`` takes as ``floor_ulps``."""
    if extra is None:
        return FLOOR_ULPS
    return FLOOR_ULPS + float(extra.max()) / (ULP * max(float(ref.detach().abs().max()), TINY))


def run_with_grads(forward, params, upstream):
    """One training pass: ``forward()`` returns a tuple of tensors, ``upstream`` the same number of gradients fed into them
    (None: none into that output); returns (outputs detached, {name: gradient}) for the named parameters ``params`` (a
    parameter the pass does not reach reports None)."""
    outs = forward()
    loss = sum((o * u).sum() for o, u in zip(outs, upstream) if u is not None)
    grads = th.autograd.grad(loss, list(params.values()), allow_unused=True)
    return tuple(o.detach() for o in outs), dict(zip(params, grads))


def cast(t, dtype=th.float64):
    return None if t is None else t.detach().to(dtype)


# ---------------------------------------------------------------------------------------------------------------------------
# ties

def tie_rows(preacts, eps=1e-5):
    """Rows of the fp64 pre-activations [rows, units] (one tensor per ReLU layer) with an entry within ``eps`` of zero, exact
    zeros excepted: there the side of ReLU's kink is arbitrary in any fp32 form."""
    tie = None
    for pre in preacts:
        t = ((pre.abs() < eps) & (pre != 0)).any(1)
        tie = t if tie is None else tie | t
    return tie


def clear_ties(ref_module, inputs, upstream, eps=1e-5):
    """tests/test_qmix_gpu.py's ``_clear_ties`` for the actor and the critic tail: rows with a ReLU pre-activation within
    ``eps`` of zero in fp64 (the LayerNorm output of the first layer; for the critic the fc2 output too) get zero upstream
    gradient, IN PLACE in every tensor of ``upstream`` (each [rows, ...]).  ``ref_module``: an fp64 RNNAgent with ``inputs``
    (obs rows without ids, hidden, n_agents), an fp64 MLPCritic with ``inputs`` (z,), or any callable that returns the list of
    fp64 pre-activations of ``inputs``.  Returns the share of rows cleared; the caller asserts it is at most TIE_CAP (a
    condition on the inputs, not a measurement).  Forward comparisons clear nothing."""
    from safe_marl_amd.nets import MLPCritic, RNNAgent
    with th.no_grad():
        if isinstance(ref_module, RNNAgent):
            preacts = [actor_plain(ref_module, *inputs)[2]]
        elif isinstance(ref_module, MLPCritic):
            preacts = list(critic_tail_plain(ref_module, *inputs)[1:])
        else:
            preacts = list(ref_module(*inputs))
        tie = tie_rows(preacts, eps)
        for u in (upstream if isinstance(upstream, (list, tuple)) else [upstream]):
            u.view(tie.shape[0], -1)[tie] = 0
    return float(tie.double().mean())


# ---------------------------------------------------------------------------------------------------------------------------
# input families

class Family(NamedTuple):
    name: str
    inputs: tuple         # (obs [rows, obs_dim], hidden [rows, 64]) for the RNN actor, (obs [rows, obs_dim],) for a module with
    #                       its own first layer and no state ("mlp"), (z [rows, 64],) for the direct entry points
    params: dict          # parameter changes the family needs: {"fc1.bias": ("add", 30.0)} / {"ln_b": ("fill", -10.0)}
    groups: object = None  # mixed: int64 [rows], the index into MIXED_OF[kind] of each row's family


MIXED_OF = {"actor": ("plain", "reset", "saturated"), "mlp": ("plain", "reset"), "z": ("plain", "reset", "offset", "constant")}
CONSTANT_BIAS = 2.7   # not a dyadic fraction: 2.7 k is inexact in fp32 for most k, so a running sum of equal addends rounds
CONSTANT_PARAMS = {"fc1.weight": ("fill", 0.0), "fc1.bias": ("fill", CONSTANT_BIAS)}


def _actor_inputs(name, rows, obs_dim, g, dev):
    if name == "reset":
        return th.zeros(rows, obs_dim, device=dev), th.zeros(rows, 64, device=dev)
    if name == "saturated":
        hid = 40.0 * th.sign(th.randn(rows, 64, device=dev, generator=g))
        return 8.0 * th.randn(rows, obs_dim, device=dev, generator=g), hid
    return 0.5 * th.randn(rows, obs_dim, device=dev, generator=g), 0.5 * th.randn(rows, 64, device=dev, generator=g)


def _mlp_inputs(name, rows, obs_dim, g, dev):
    if name == "reset":
        return (th.zeros(rows, obs_dim, device=dev),)
    return (0.5 * th.randn(rows, obs_dim, device=dev, generator=g),)


def _z_inputs(name, rows, g, dev):
    if name == "reset":
        return th.zeros(rows, 64, device=dev)
    z = 0.5 * th.randn(rows, 64, device=dev, generator=g)
    if name == "offset":
        return z + 30.0
    if name == "constant":
        return z[:, :1].mul(4.0).expand(rows, 64).contiguous()
    return z


def families(rows, n_agents, obs_dim, generator, kind=None):
    """The named input families for ``rows`` = samples x ``n_agents`` rows, drawn from ``generator`` on its device.  ``kind``
    "actor" (the default with an ``obs_dim``): the RNN actor's, inputs (obs, hidden); "mlp": a module with its own first layer
    and no state (nets.MLPAgent; nets.MLPCritic on materialised rows, ``obs_dim`` then the width the test draws), inputs
    (obs,); "z" (the default with ``obs_dim`` None): the direct entry points' (csrc/lnrelu.hip without bias or ids, the critic
    tail, csrc/coma.hip), inputs (z,).

    plain      0.5 randn.
    reset      inputs exactly zero: the workload's own first step.
    offset     the row mean about 70 times the row spread: fc1.bias += 30 on the module, a +30 common term on z.
    constant   the 64 LayerNorm inputs of a row all equal, bit for bit: variance exactly zero, rstd = eps^-1/2.  On z: one
               draw per row repeated.  On a module: fc1.weight (its id columns and, for the SQDDPG and COMA critics, its
               action block are part of it) filled with 0, fc1.bias with CONSTANT_BIAS, inputs plain.
    saturated  (RNN actor only) hidden = 40 sign(randn), obs = 8 randn: gate pre-activations of several tens.
    dead       ln_b = -10: every ReLU unit of every row is off.
    mixed      the families that are inputs alone (MIXED_OF) interleaved row by row, so that one 16-row or 32-row tile
               holds rows of each kind; ``groups`` says which.  (offset, constant on a module and dead are parameter
               changes: they hold for a whole batch and cannot be interleaved.)"""
    dev = generator.device
    if kind is None:
        kind = "z" if obs_dim is None else "actor"
    draw = {"z": lambda nm: (_z_inputs(nm, rows, generator, dev),),
            "mlp": lambda nm: _mlp_inputs(nm, rows, obs_dim, generator, dev),
            "actor": lambda nm: _actor_inputs(nm, rows, obs_dim, generator, dev)}[kind]
    out = {"plain": Family("plain", draw("plain"), {}), "reset": Family("reset", draw("reset"), {})}
    if kind == "z":
        out["offset"] = Family("offset", draw("offset"), {})
        out["constant"] = Family("constant", draw("constant"), {})
    else:
        out["offset"] = Family("offset", draw("plain"), {"fc1.bias": ("add", 30.0)})
        if kind == "actor":
            out["saturated"] = Family("saturated", draw("saturated"), {})
    out["dead"] = Family("dead", draw("plain"), {"ln_b": ("fill", -10.0)})
    names = MIXED_OF[kind]
    groups = th.arange(rows, device=dev) % len(names)
    parts = [out[nm].inputs if nm != "plain" else draw("plain") for nm in names]
    mixed = []
    for k in range(len(parts[0])):
        t = parts[0][k].clone()
        for j in range(1, len(names)):
            t[groups == j] = parts[j][k][groups == j]
        mixed.append(t)
    out["mixed"] = Family("mixed", tuple(mixed), {}, groups)
    if kind != "z":
        # (plain's own inputs, no further draw: whatever a test draws after this call is what it was before this family existed)
        out["constant"] = Family("constant", out["plain"].inputs, dict(CONSTANT_PARAMS))
    return out


QMIX_FAMILIES = ("plain", "reset", "dead", "zeros", "elu_neg", "elu_deep", "big_q", "mixed")
QMIX_MIXED_OF = ("plain", "reset", "elu_neg", "big_q")


def qmix_families(B, n, S, generator):
    """The mixer's named input families for ``B`` samples of ``n`` agents and a state of ``S``: inputs (agent_qs [B, n],
    states [B, S], loss weights w [B]) from ONE set of base draws q = randn, x = 0.3 randn, w = randn / B (the scales of
    tests/test_qmix_gpu.py), on the generator's device.

    plain     the base draws.
    reset     state exactly zero: the first-layer outputs are the biases, the first-layer weight gradients exactly zero.
    dead      the three ReLU heads' first-layer biases filled with -10: every hidden unit off, w1 = |hyper_w_1.2.bias|,
              gradients into the .0 layers of those heads exactly zero.
    zeros     a mixer made with ``zero_rows=True`` (``params`` says so: {"zero_rows": ...}, for ``make_mixer``); the inputs
              are plain's.
    elu_neg   q = -4 |randn|: every mixing unit on ELU's exponential branch, a few units deep.
    elu_deep  q = -300 - |randn|: hidden = -1 to the last bit, the slope exp(x) underflows.
    big_q     q = 100 randn: hundreds per unit on the linear branch, deep saturation on the other.
    mixed     plain, reset, elu_neg, big_q interleaved sample by sample (``groups``: which), so that one 32-sample tile holds
              each kind.  (dead and zeros are parameter changes; elu_deep has no gradient to compare.)"""
    dev = generator.device
    q = th.randn(B, n, device=dev, generator=generator)
    x = 0.3 * th.randn(B, S, device=dev, generator=generator)
    w = th.randn(B, device=dev, generator=generator) / B
    qs = {"plain": q, "reset": q, "elu_neg": -4.0 * q.abs(), "elu_deep": -300.0 - q.abs(), "big_q": 100.0 * q}
    xs = {"reset": th.zeros_like(x)}
    dead = {f"{head}.0.bias": ("fill", -10.0) for head in QMIX_RELU_HEADS}
    out = {name: Family(name, (qs[name], xs.get(name, x), w.clone()), {}) for name in qs}
    out["dead"] = Family("dead", (q, x, w.clone()), dead)
    out["zeros"] = Family("zeros", (q, x, w.clone()), {"zero_rows": ("make", True)})
    groups = th.arange(B, device=dev) % len(QMIX_MIXED_OF)
    mq, mx = q.clone(), x.clone()
    for j, name in enumerate(QMIX_MIXED_OF):
        mq[groups == j] = qs[name][groups == j]
        mx[groups == j] = xs.get(name, x)[groups == j]
    out["mixed"] = Family("mixed", (mq, mx, w.clone()), {}, groups)
    return out


def qmix_clear_ties(mixer64, states, w, eps=1e-5):
    """``clear_ties`` per SAMPLE for the mixer: w[b] = 0 IN PLACE where sample b has one of ``qmix_plain``'s pre-activations
    within ``eps`` of zero in fp64 (exact zeros excepted); the agent q-values play no part in them.  Returns the share."""
    zeros = th.zeros(states.shape[0], mixer64.n_agents, dtype=th.float64, device=states.device)
    return clear_ties(lambda x: qmix_plain(mixer64, zeros, x)[1], (states.double(),), [w], eps)


def apply_params(module, family):
    """Make the family's parameter changes on ``module`` (an RNNAgent, an MLPAgent, an MLPCritic or a QMixer, or a list of
    them: every one; ``ln_b`` is its LayerNorm's bias; a "make" entry is for the module's constructor, not for here)."""
    if isinstance(module, (list, tuple)):
        for m in module:
            apply_params(m, family)
        return module
    with th.no_grad():
        for key, (op, value) in family.params.items():
            if op == "make":
                continue
            p = module.layernorm.bias if key == "ln_b" else dict(module.named_parameters())[key]
            if op == "add":
                p.add_(value)
            else:
                p.fill_(value)
    return module
