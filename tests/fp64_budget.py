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
tests/test_fp64_budget_cpu.py pins them to the modules' forward (1e-12 in fp64).

The last part holds what has no module: csrc/ppo.hip (``gae_plain``, ``policy_loss_plain``, ``value_loss_plain``), csrc/gauss.hip's
log-std head (``gauss_head_plain``) and the stand-alone csrc/tdloss.hip (``td_run``) against the ``nets`` compositions of the same
formulas in fp64, with their input families (``gae_families``, ``policy_families``, ``value_families``, ``gauss_families``,
``td_families``), the elements whose side of a clip end is arbitrary (``policy_clear_kinks``, ``value_keep``) and the one floor
derived for them (``policy_loss_rounding``).

At the end, the two hand-written GEMMs: csrc/wgrad.hip (``wgrad_plain``, ``wgrad_families``, ``wgrad_floors``) and csrc/linear.hip
(``linear2_plain``, ``linear2_families``, ``linear2_sum_rounding``), with the floor of a sum of products
(``product_sum_rounding``; ``ordered_sum_rounding`` where the order of the addends matters, ``equal_addend_drift`` where they are
all equal) and the shapes both their GPU tests and the CPU test run.

Last, what every sub-update ends in and every reported loss goes through: csrc/optim.hip (``clip_rmsprop_plain`` with OPTIM_WRONG,
``optim_layouts``, ``optim_families``) and csrc/tdloss.hip's scalar mean (``mean_input``, ``mean_within_bound``: a bound derived
for a sum held in fp64, not a budget) for tests/test_optim_fp64_gpu.py."""
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


# ---------------------------------------------------------------------------------------------------------------------------
# csrc/ppo.hip, csrc/gauss.hip and the stand-alone csrc/tdloss.hip (tests/test_ppo_fp64_gpu.py, test_gauss_fp64_gpu.py,
# test_tdloss_fp64_gpu.py): the plain compositions with their wrong evaluations, and the input families.  Every family is drawn
# from a CPU generator, so that tests/test_fp64_budget_cpu.py holds conditions on the very cases the GPU tests run.

GAMMA, LAM = 0.99, 0.95
POLICY_EPS = 0.2
KINK = 1e-5
GAE_WRONG = ("mask_everywhere", "drop_carry_64", "biased_running_var")
GAE_FAMILIES = ("plain", "all_terminal", "open_sum", "tile_edges", "gamma0", "failure", "mixed")
GAE_MIXED_OF = ("plain", "all_terminal", "open_sum", "tile_edges")        # the FLAGS of these, chain by chain
FAILURE_REWARD, FAILURE_SPREAD = -200.0, 0.05
POLICY_FAMILIES = ("plain", "on_mean", "zero_adv", "clipped_out", "ends_min", "ends_max", "wide", "mixed")
POLICY_MIXED_OF = ("plain", "on_mean", "zero_adv", "clipped_out")         # (ends and wide are held in the rms form: not mixed in)
POLICY_RMS = ("ends_min", "ends_max", "wide")
VALUE_FAMILIES = ("plain", "eps0", "all_done")
GAUSS_FAMILIES = ("plain", "reset", "saturated", "flat", "wide_noise", "mixed")
GAUSS_MIXED_OF = ("plain", "reset", "saturated")
GAUSS_SATURATED = 25.0     # |u| of every saturated element in fp64: tanh is 1 to the last bit of fp64 beyond 19.1
LOG_STD_RANGES = ((0.0, 0.5), (-5.0, 2.0))
TD_FAMILIES = ("plain", "failure")


def bn_module(n, dtype=th.float32, device="cpu", seed=0):
    """tests/test_ppo_gpu.py's BatchNorm1d: affine parameters and running statistics that are not the initial ones."""
    g = th.Generator().manual_seed(seed)
    bn = th.nn.BatchNorm1d(n)
    with th.no_grad():
        bn.weight.copy_(1 + 0.1 * th.randn(n, generator=g))
        bn.bias.copy_(0.1 * th.randn(n, generator=g))
        bn.running_mean.copy_(th.randn(n, generator=g))
        bn.running_var.copy_(1 + th.rand(n, generator=g))
    return bn.to(dtype).to(device)


def fixed_log_stds(means, log_std):
    """The fixed-std policy's log_stds as the learner hands them over (tests/test_ppo_gpu.py's ``_log_stds``): ONE number
    expanded to the shape of ``means``, marked ``_flex_entropy``.  ``log_std``: a tensor whose first element is taken (in its
    own precision: the fp32 number is the input of every form)."""
    c = log_std.reshape(-1)[:1].detach().to(dtype=means.dtype, device=means.device)
    ls = c.expand_as(means)
    ls._flex_entropy = th.zeros((), device=means.device)
    return ls


def gae_chain_loop(reward_norm, old_values, old_next_values, done, last_step, gamma, lam, stride, wrong=None):
    """ppo.py:44-52 chain by chain, literally, in the dtype of its inputs: chain e is rows e, e + stride, ... and need not be as
    long as the others (``rows % stride != 0``: include/flexnet.h allows it, nets.ppo_gae_torch does not).  The loop runs over
    the steps from the last one back, each chain meeting ppo_gae_torch's operations in ppo_gae_torch's order.  ``wrong``:
    "mask_everywhere", m = 1 - done on every row instead of on last steps alone; "drop_carry_64", the advantage of the next
    step is not handed over at every 64th step counted from the chain's end (a wavefront scan that loses its carry between
    tiles)."""
    rows, n = reward_norm.shape
    per = min(int(stride), rows)
    done, last_step = done.reshape(rows, 1), last_step.reshape(rows, 1)
    mask = 1.0 - done if wrong == "mask_everywhere" else th.where(last_step != 0, 1.0 - done, th.ones_like(done))
    steps_of = (rows - th.arange(per) + stride - 1) // stride                          # chain e has this many steps
    out = th.empty_like(reward_norm)
    nxt = th.zeros(per, n, dtype=reward_norm.dtype)
    for t in reversed(range(int(steps_of.max()))):
        lo, hi = t * stride, min((t + 1) * stride, rows)
        k = hi - lo
        carry = nxt[:k]
        if wrong == "drop_carry_64":
            carry = th.where(((steps_of[:k] - 1 - t) % 64 == 0).view(k, 1), th.zeros_like(carry), carry)
        deltas = reward_norm[lo:hi] + gamma * old_next_values[lo:hi] * mask[lo:hi] - old_values[lo:hi]
        cur = deltas + gamma * lam * carry * mask[lo:hi]
        out[lo:hi] = cur
        nxt = th.zeros_like(nxt)
        nxt[:k] = cur
    return out


def gae_plain(reward, old_values, old_next_values, done, last_step, gamma, lam, stride, reward_bn=None, adv_bn=None, wrong=None):
    """nets.ppo_gae(..., fused=False) — the reward through its BatchNorm, GAE along the chains, the advantages through theirs —
    with both modules' running statistics beside the three tensors: {"reward_norm", "advantages", "advantages_norm",
    "reward_bn.running_mean", "reward_bn.running_var", "adv_bn.running_mean", ..., "reward_bn.num_batches_tracked", ...}.  The
    modules are moved as their training-mode forward moves them.  Ragged chains and the wrong evaluations (GAE_WRONG;
    "biased_running_var": the running variance moved by the biased batch variance) take ``gae_chain_loop`` between the modules."""
    from safe_marl_amd.nets import ppo_gae
    assert wrong is None or wrong in GAE_WRONG, wrong
    rows = reward.shape[0]
    before = {key: bn.running_var.clone() for key, bn in (("reward_bn", reward_bn), ("adv_bn", adv_bn)) if bn is not None}
    with th.no_grad():
        if wrong in (None, "biased_running_var") and rows % stride == 0:
            rn, adv, advn = ppo_gae(reward, old_values, old_next_values, done, last_step, gamma, lam, stride, reward_bn, adv_bn,
                                    fused=False)
        else:
            rn = reward_bn(reward) if reward_bn is not None else reward
            adv = gae_chain_loop(rn, old_values, old_next_values, done, last_step, gamma, lam, stride, wrong)
            advn = adv_bn(adv) if adv_bn is not None else adv
        out = {"reward_norm": rn, "advantages": adv, "advantages_norm": advn}
        for key, bn, x in (("reward_bn", reward_bn, reward), ("adv_bn", adv_bn, adv)):
            if bn is None:
                continue
            if wrong == "biased_running_var":
                bn.running_var.copy_((1 - bn.momentum) * before[key] + bn.momentum * x.var(0, unbiased=False))
            out[key + ".running_mean"], out[key + ".running_var"] = bn.running_mean.clone(), bn.running_var.clone()
            out[key + ".num_batches_tracked"] = bn.num_batches_tracked.clone()
    return out


def steps_from_end(rows, stride):
    """int64 [rows]: how many steps of its chain follow row r (0: the chain's last step), and the chain's length."""
    r = th.arange(rows)
    e = r % stride
    steps_of = (rows - e + stride - 1) // stride
    return steps_of - 1 - r // stride, steps_of


def gae_families(rows, n, stride, generator):
    """The named input families of GAE on ``rows`` rows of ``n`` agents in chains ``stride`` apart: inputs (reward, old_values,
    old_next_values, done, last_step), ``params`` {"gamma", "lam"}, from ONE set of base draws (tests/test_ppo_gpu.py's scales:
    reward 0.05 randn - 0.03, values randn, a last step on 8 % of the rows).

    plain         done on half of ALL rows, drawn independently of last_step: all four (done, last) combinations occur, and
                  done = 1 on a row that is not a last step must change nothing.
    all_terminal  last = done = 1 on every row: A = delta.
    open_sum      no last step (done as plain's: it must not matter), gamma = lambda = 1: suffix sums over the whole chain.
    tile_edges    last = done = 1 exactly at the steps that fall on lanes 0 and 63 of every 64-step tile counted from the
                  chain's end, and at the chain's first and last step; 0 elsewhere.
    gamma0        plain's inputs with gamma = 0.
    failure       plain's with reward column 0 exactly FAILURE_REWARD on every row (variance exactly zero) and column 1
                  FAILURE_REWARD + FAILURE_SPREAD randn (|mean| / std = 4 000: the workload's own extreme, a column of
                  failure rewards).
    mixed         the flags of GAE_MIXED_OF interleaved chain by chain (``groups`` [rows]: which), plain's gamma and lambda."""
    g = generator
    r = 0.05 * th.randn(rows, n, generator=g) - 0.03
    v, nv = th.randn(rows, n, generator=g), th.randn(rows, n, generator=g)
    last = (th.rand(rows, generator=g) < 0.08).float()
    done = (th.rand(rows, generator=g) < 0.5).float()
    spread = th.randn(rows, generator=g)
    after, steps_of = steps_from_end(rows, stride)
    edge = ((after % 64 == 0) | (after % 64 == 63) | (after == steps_of - 1)).float()
    ones, zeros = th.ones(rows), th.zeros(rows)
    flags = {"plain": (done, last), "all_terminal": (ones, ones), "open_sum": (done, zeros), "tile_edges": (edge, edge)}
    std = {"gamma": GAMMA, "lam": LAM}
    out = {name: Family(name, (r, v, nv, d.clone(), l.clone()), dict(std)) for name, (d, l) in flags.items()}
    out["open_sum"] = out["open_sum"]._replace(params={"gamma": 1.0, "lam": 1.0})
    out["gamma0"] = Family("gamma0", (r, v, nv, done.clone(), last.clone()), {"gamma": 0.0, "lam": LAM})
    rf = r.clone()
    rf[:, 0] = FAILURE_REWARD
    if n > 1:
        rf[:, 1] = FAILURE_REWARD + FAILURE_SPREAD * spread
    out["failure"] = Family("failure", (rf, v, nv, done.clone(), last.clone()), dict(std))
    groups = (th.arange(rows) % stride) % len(GAE_MIXED_OF)
    md, ml = done.clone(), last.clone()
    for j, name in enumerate(GAE_MIXED_OF):
        md[groups == j], ml[groups == j] = flags[name][0][groups == j], flags[name][1][groups == j]
    out["mixed"] = Family("mixed", (r, v, nv, md, ml), dict(std), groups)
    return out


def _log_density64(means, log_stds, actions):
    """log p [rows, n] in fp64 of ``actions`` [rows, n, a] under the agent-summed Gaussian of ``means`` / ``log_stds``."""
    import math
    mu, ls = means.double().sum(1, keepdim=True), log_stds.double().sum(1, keepdim=True)
    return (-(actions.double() - mu).square() / (2.0 * th.exp(2.0 * ls)) - ls - 0.5 * math.log(2.0 * math.pi)).sum(-1)


def _stored_log_prob(logp, a):
    """A stored log-density [rows, n, a] in fp32 whose sum over the action dimension is ``logp`` [rows, n] (fp64)."""
    return (logp / a).unsqueeze(-1).expand(*logp.shape, a).float().contiguous()


def policy_families(rows, n, a, generator, per_row=True, log_std_range=LOG_STD_RANGES[0]):
    """The named input families of the PPO policy loss on ``rows`` rows of ``n`` agents and ``a`` action components: inputs
    (means, log_stds, actions, old_log_prob — each [rows, n, a] —, advantages [rows, n]), ``params`` {"eps_clip"}.  ``per_row``
    False: every log-std is one number (the fixed-std policy; the test hands ``fixed_log_stds`` of it over).  One action for
    every agent of a row (ippo.py:72-73).  old_log_prob is the fp64 log-density plus 0.1 randn unless said otherwise.

    plain        tests/test_gauss_head_gpu.py's centred regime: ratios of order one on both sides of the clip range; every
                 seventh row's advantages exactly zero.
    on_mean      means on a grid of 2^-10 (their sum is exact in any order and any precision) and the action bit-equal to the
                 agent-summed mean: d = 0, d_means exactly zero, d_log_stds = -sum of dlogp.
    zero_adv     every advantage 0: the loss and both gradients exactly zero.
    clipped_out  old = log p - sign(adv): every ratio e or 1 / e on the side where the clipped branch is the smaller and has no
                 gradient; no advantage is zero.  Gradients exactly zero, the loss the clipped surrogate.
    ends_min / ends_max  every agent's log-std at the lower / upper end of ``log_std_range``.  Means and actions are plain's
                 times the summed standard deviation exp(n end), so that the standardised residual stays of order one while
                 log p is of order n a |end|.
    wide         the large-ratio regime of test_ppo_policy_loss_rows_with_large_ratios: uncentred means, old = the action.
    mixed        POLICY_MIXED_OF interleaved row by row (``groups``: which)."""
    import math
    g = generator
    rnd = lambda *s: th.randn(*s, generator=g)
    m0, l0, z, e, adv = rnd(rows, n, a), rnd(rows, n, a), rnd(rows, 1, a), rnd(rows, n), rnd(rows, n)
    mw, lw = rnd(rows, n, a), rnd(rows, n, a)
    adv0 = adv.clone()
    adv0[::7] = 0.0

    def log_stds_of(t):
        return t if per_row else t[:1, :1, :1].expand(rows, n, a).contiguous()

    def finish(name, means, log_stds, one, advantages, old=None, shift=None):
        actions = one.expand(rows, n, a).contiguous()
        if old is None:
            logp = _log_density64(means, log_stds, actions)
            old = _stored_log_prob(logp + (0.1 * e.double() if shift is None else shift), a)
        return Family(name, (means, log_stds, actions, old, advantages.clone()), {"eps_clip": POLICY_EPS})

    means = -0.9 / n + 0.1 / n ** 0.5 * m0
    ls = log_stds_of(0.15 / n ** 0.5 * l0 - 0.05 / n)
    one = means.sum(1, keepdim=True) + 0.25 * z
    out = {"plain": finish("plain", means, ls, one, adv0)}
    grid = (means * 1024.0).round() / 1024.0
    out["on_mean"] = finish("on_mean", grid, ls, grid.sum(1, keepdim=True), adv0)
    out["zero_adv"] = finish("zero_adv", means, ls, one, th.zeros_like(adv))
    nz = th.where(adv == 0, th.ones_like(adv), adv)
    out["clipped_out"] = finish("clipped_out", means, ls, one, nz, shift=-th.sign(nz).double())
    for name, end in zip(("ends_min", "ends_max"), log_std_range):
        sd = math.exp(n * end)
        me = (means.double() * sd).float()
        out[name] = finish(name, me, th.full((rows, n, a), float(end)), (me.sum(1, keepdim=True).double() + sd * 0.25 * z.double()).float(),
                           adv0)
    wm = 0.3 * mw
    wone = wm.sum(1, keepdim=True) + 0.7 * z
    out["wide"] = finish("wide", wm, log_stds_of(0.15 * lw - 0.05), wone, adv, old=wone.expand(rows, n, a).contiguous())
    groups = th.arange(rows) % len(POLICY_MIXED_OF)
    mixed = [t.clone() for t in out["plain"].inputs]
    for j, name in enumerate(POLICY_MIXED_OF):
        for k, t in enumerate(out[name].inputs):
            mixed[k][groups == j] = t[groups == j]
    out["mixed"] = Family("mixed", tuple(mixed), {"eps_clip": POLICY_EPS}, groups)
    return out


def policy_clear_kinks(inputs, eps_clip, eps=KINK):
    """An element (row, agent) has a kink when its fp64 ratio lies within ``eps`` (relative) of 1 - eps_clip or 1 + eps_clip with
    a non-zero advantage: on which side of clamp's end it falls is arbitrary in any fp32 form.  Their advantages are set to
    zero IN PLACE (a zero gradient in every form).  Returns the share; the caller asserts it is at most TIE_CAP."""
    means, log_stds, actions, old, adv = inputs
    ratio = th.exp(_log_density64(means, log_stds, actions) - old.double().sum(-1))
    kink = (((ratio / (1.0 - eps_clip) - 1.0).abs() < eps) | ((ratio / (1.0 + eps_clip) - 1.0).abs() < eps)) & (adv != 0)
    adv[kink] = 0.0
    return float(kink.double().mean())


POLICY_WRONG = ("no_minus_one",)


def policy_loss_plain(inputs, eps_clip, dtype, fixed=False, wrong=None):
    """nets.ppo_policy_loss_torch on a family's ``inputs`` cast to ``dtype``, with autograd: {"loss", "ratio", "d_means",
    "d_log_stds"} (the last only for per-row log-stds; ``fixed``: ``fixed_log_stds`` of the first one).  ``wrong``
    "no_minus_one": d log p / d log_std taken as (x - mu)^2 / var, without the - 1 of the density's normalisation (values
    unchanged: only the backward is wrong)."""
    import math
    from safe_marl_amd.nets import ppo_policy_loss_torch
    assert wrong is None or wrong in POLICY_WRONG, wrong
    means, log_stds, actions, old, adv = (t.detach().to(dtype) for t in inputs)
    m = means.clone().requires_grad_(True)
    ls = fixed_log_stds(m, inputs[1]) if fixed else log_stds.clone().requires_grad_(True)
    if wrong is None:
        loss, ratio = ppo_policy_loss_torch(m, ls, actions, old, adv, eps_clip)
    else:
        mu, s = m.sum(1, keepdim=True), ls.sum(1, keepdim=True)
        logp = (-(actions - mu).square() / (2 * s.exp().square()) - s.detach() - math.log(math.sqrt(2 * math.pi))).sum(-1)
        ratio = th.exp(logp - old.sum(-1))
        loss = -th.min(ratio * adv, th.clamp(ratio, 1 - eps_clip, 1 + eps_clip) * adv).mean()
    grads = th.autograd.grad(loss, [m] if fixed else [m, ls])
    out = {"loss": loss.detach(), "ratio": ratio.detach(), "d_means": grads[0]}
    if not fixed:
        out["d_log_stds"] = grads[1]
    return out


def value_families(rows, n, generator):
    """The PPO value loss's families: inputs (values, old_values, next_values, reward_norm [rows, n], done [rows]), ``params``
    {"eps_clip"}.

    plain     tests/test_ppo_gpu.py's ``_value_inputs``: V = old + 0.5 randn, eps_clip 0.5, with its constructed rows — every
              16th exactly on the upper clip boundary, the next on the lower one, the next a tie surr1 == surr2 outside the
              range (all exact in fp32: old in quarters, no bootstrap).
    eps0      plain's with eps_clip = 0: the clip range is the point V = old; every 16th row from the fourth has V == old,
              bit for bit (inside the closed range, and a tie).
    all_done  plain's with done = 1 on every row: the return is the normalised reward."""
    g = generator
    old = th.randn(rows, n, generator=g)
    values = old + 0.5 * th.randn(rows, n, generator=g)
    nv, rn = th.randn(rows, n, generator=g), th.randn(rows, n, generator=g)
    done = (th.rand(rows, generator=g) < 0.05).float()
    eps = 0.5
    for k in range(3):
        old[k::16] = (old[k::16] * 4).round() / 4
    values[0::16] = old[0::16] + eps
    values[1::16] = old[1::16] - eps
    values[2::16] = old[2::16] + 1.5
    done[2::16] = 1.0
    rn[2::16] = old[2::16] + 1.0              # V - ret = 0.5, vc - ret = old + 0.5 - ret = -0.5
    out = {"plain": Family("plain", (values, old, nv, rn, done), {"eps_clip": eps})}
    v0 = values.clone()
    v0[3::16] = old[3::16]
    out["eps0"] = Family("eps0", (v0, old, nv, rn, done), {"eps_clip": 0.0})
    out["all_done"] = Family("all_done", (values, old, nv, rn, th.ones_like(done)), {"eps_clip": eps})
    return out


VALUE_WRONG = ("clamp_open",)


def value_loss_plain(inputs, eps_clip, gamma, coef, dtype, wrong=None):
    """nets.ppo_value_loss_torch on a family's ``inputs`` cast to ``dtype``, with autograd: {"loss", "d_values", "returns"}.
    ``wrong`` "clamp_open": clamp's gradient cut AT its ends (V exactly eps_clip away from the old value), where th.clamp
    passes it."""
    from safe_marl_amd.nets import ppo_value_loss_torch
    assert wrong is None or wrong in VALUE_WRONG, wrong
    values, old, nv, rn, done = (t.detach().to(dtype) for t in inputs)
    v = values.clone().requires_grad_(True)
    vv = v
    if wrong == "clamp_open":
        vv = th.where((v - old).abs() == eps_clip, v.detach(), v)
        returns = rn + gamma * (1 - done.reshape(-1, 1)) * nv
        clipped = old + th.clamp(vv - old, -eps_clip, eps_clip)
        loss = coef * th.max((v - returns).pow(2), (clipped - returns).pow(2)).mean()
    else:
        loss, returns = ppo_value_loss_torch(v, old, nv, rn, done, gamma, eps_clip, coef)
    (gv,) = th.autograd.grad(loss, [v])
    return {"loss": loss.detach(), "d_values": gv, "returns": returns.detach()}


def value_keep(inputs, eps_clip, gamma, eps=KINK):
    """bool [rows, n]: the elements whose d_values is compared.  Left out, as arbitrary in any fp32 form: |V - old| within
    ``eps`` of eps_clip without being exactly on it (which side of clamp's end), and — OUTSIDE the clip range, where the
    clipped branch has no gradient — |s1 - s2| <= eps max(s1, s2) without s1 == s2 (which of the two squares is th.max's).
    Inside the range the clipped value is V up to a rounding and both branches carry the same gradient: nothing is arbitrary
    there.  All in fp64; the constructed boundary and tie rows are exact and stay.  The caller holds 1 - mean to TIE_CAP."""
    values, old, nv, rn, done = (t.double() for t in inputs)
    d = values - old
    ret = rn + gamma * (1 - done.reshape(-1, 1)) * nv
    s1, s2 = (values - ret).square(), (old + th.clamp(d, -eps_clip, eps_clip) - ret).square()
    near_clip = ((d.abs() - eps_clip).abs() < eps) & (d.abs() != eps_clip)
    near_tie = (d.abs() > eps_clip) & ((s1 - s2).abs() <= eps * th.maximum(s1, s2)) & (s1 != s2)
    return ~(near_clip | near_tie)


GAUSS_WRONG = ("one_minus_t",)


def gauss_head_plain(inputs, lo, hi, dtype, low=0.0, high=1.0, wrong=None):
    """nets.gauss_log_std_torch with the exploration epilogue (maddpg.py:88 under util.py:56-64, translate_action
    util.py:125-128) and autograd, on a family's ``inputs`` (h [rows, 64], w, b, means, noise, d_log_std [rows, a]) cast to
    ``dtype``.  w [a, 64] / b [a]: the shared head; w [n, a, 64] / b [n, a]: every agent's own, row r through head r % n.
    {"log_std", "t", "action", "env_action", "d_h", "d_w", "d_b", "d_u"}.  ``wrong`` "one_minus_t": d_u with 1 - t in place of
    1 - t^2 (values unchanged)."""
    assert wrong is None or wrong in GAUSS_WRONG, wrong
    h, w, b, means, noise, d_ls = (t.detach().to(dtype) for t in inputs)
    h, w, b = (t.clone().requires_grad_(True) for t in (h, w, b))
    if w.dim() == 3:
        n = w.shape[0]
        hv = h.view(-1, n, h.shape[1])
        u = th.stack([F.linear(hv[:, i], w[i], b[i]) for i in range(n)], 1).reshape(h.shape[0], -1)
    else:
        u = F.linear(h, w, b)
    t = th.tanh(u)
    tt = t if wrong is None else t.detach() + (u - u.detach()) * (1 - t.detach())
    log_std = lo + 0.5 * (hi - lo) * (tt + 1)
    action = th.tanh(means + log_std.exp() * noise)
    env = 0.5 * (th.clamp(action, min=low, max=high) + 1.0) * (high - low) + low
    d_h, d_w, d_b, d_u = th.autograd.grad(log_std, (h, w, b, u), d_ls)
    return {"log_std": log_std.detach(), "t": t.detach(), "action": action.detach(), "env_action": env.detach(), "d_h": d_h,
            "d_w": d_w, "d_b": d_b, "d_u": d_u}


def _gauss_u64(h, w, b):
    if w.dim() == 3:
        n = w.shape[0]
        return (th.einsum("bnk,nak->bna", h.double().view(-1, n, 64), w.double()) + b.double()).reshape(h.shape[0], -1)
    return h.double() @ w.double().t() + b.double()


def gauss_families(rows, a, generator, n=None, attempts=400):
    """The log-std head's families on ``rows`` rows of 64 hidden units and ``a`` outputs: inputs (h, w, b, means, noise,
    d_log_std); ``n``: per-agent heads (w [n, a, 64], row r through head r % n, ``rows`` a multiple of n).  ``params``
    {"range": (lo, hi)} where the family fixes it, {} where the test takes LOG_STD_RANGES.

    plain       h 0.5 randn, weights and bias 0.1 randn, means, noise and the upstream gradient randn.
    reset       h = 0: u = b.
    saturated   h = 40 sign(randn), weights 0.3 randn; a row is drawn again until every |u| of it is at least
                GAUSS_SATURATED in fp64: t = +-1 to the last bit, log_std exactly an end of the range, d_u and d_h exactly zero.
    flat        plain's inputs with lo == hi: log_std constant, every gradient exactly zero.
    wide_noise  plain's with the range (-5, 2) and noise 4 randn: the actions saturate and env_action sits on both clamp ends.
    mixed       GAUSS_MIXED_OF interleaved row by row — per-agent heads: sample by sample — under saturated's weights
                (``groups``: which), so that one 32-row tile holds each kind."""
    g = generator
    rnd = lambda *s: th.randn(*s, generator=g)
    wshape, bshape = ((a, 64), (a,)) if n is None else ((n, a, 64), (n, a))
    h, w, b = 0.5 * rnd(rows, 64), 0.1 * rnd(*wshape), 0.1 * rnd(*bshape)
    means, noise, d_ls = rnd(rows, a), rnd(rows, a), rnd(rows, a)
    ws = 0.3 * rnd(*wshape)
    hs = 40.0 * th.sign(rnd(rows, 64))
    for _ in range(attempts):
        again = (_gauss_u64(hs, ws, b).abs() < GAUSS_SATURATED).any(1)
        if not again.any():
            break
        fresh = 40.0 * th.sign(rnd(rows, 64))
        hs[again] = fresh[again]
    else:
        raise AssertionError(f"no saturated draw of {rows} rows, {a} outputs in {attempts} attempts")
    out = {"plain": Family("plain", (h, w, b, means, noise, d_ls), {}),
           "reset": Family("reset", (th.zeros_like(h), w, b, means, noise, d_ls), {}),
           "saturated": Family("saturated", (hs, ws, b, means, noise, d_ls), {}),
           "flat": Family("flat", (h, w, b, means, noise, d_ls), {"range": (0.25, 0.25)}),
           "wide_noise": Family("wide_noise", (h, w, b, means, 4.0 * noise, d_ls), {"range": LOG_STD_RANGES[1]})}
    groups = (th.arange(rows) if n is None else th.arange(rows) // n) % len(GAUSS_MIXED_OF)
    hm = h.clone()
    hm[groups == 1] = 0.0
    hm[groups == 2] = hs[groups == 2]
    out["mixed"] = Family("mixed", (hm, ws, b, means, noise, d_ls), {}, groups)
    return out


def td_families(rows, n, generator):
    """The stand-alone TD loss's families: inputs (q, next_q, reward [rows, n], done [rows]).  plain: tests/test_tdloss_gpu.py's
    reward 3 randn - 5; failure: ``gae_families``' reward columns 0 and 1 (exactly FAILURE_REWARD; FAILURE_REWARD +
    FAILURE_SPREAD randn), the rest plain's."""
    g = generator
    reward = 3.0 * th.randn(rows, n, generator=g) - 5.0
    done = (th.rand(rows, generator=g) < 0.1).float()
    nq, q = th.randn(rows, n, generator=g), th.randn(rows, n, generator=g)
    spread = th.randn(rows, generator=g)
    rf = reward.clone()
    rf[:, 0] = FAILURE_REWARD
    if n > 1:
        rf[:, 1] = FAILURE_REWARD + FAILURE_SPREAD * spread
    return {"plain": Family("plain", (q, nq, reward, done), {}), "failure": Family("failure", (q, nq, rf, done), {})}


def td_run(inputs, gamma, bn, dtype):
    """``td_loss_plain`` through a training-mode BatchNorm1d module ``bn`` (already in ``dtype``, or None), which is moved as its
    forward moves it, with autograd: {"loss", "dq", and with a module "running_mean", "running_var", "num_batches_tracked"}."""
    q, nq, reward, done = (t.detach().to(dtype) for t in inputs)
    q = q.clone().requires_grad_(True)
    with th.no_grad():
        r = bn(reward) if bn is not None else reward
    loss = td_loss_plain(q, nq, r, done, gamma, None)
    (dq,) = th.autograd.grad(loss, [q])
    out = {"loss": loss.detach(), "dq": dq}
    if bn is not None:
        out.update(running_mean=bn.running_mean.clone(), running_var=bn.running_var.clone(),
                   num_batches_tracked=bn.num_batches_tracked.clone())
    return out


def within_budget_rms(kernel, torch32, ref, *, name, margin=4.0, floor_ulps=4.0):
    """The rms form of tests/test_gauss_head_gpu.py::test_ppo_policy_loss_rows_with_large_ratios, with that test's factors:
    rms(kernel - ref) <= 4 rms(torch32 - ref) + 4 * 2^-24 rms(ref).  Where log p - old is of order ten or more the LARGEST
    error of an output is the half-ulp luck of its one largest exponent, for the kernel and the composition alike; an arithmetic
    that lost accuracy at large arguments would raise every large element's error, hence the rms."""
    ref = ref.detach().double()
    assert kernel.shape == ref.shape and torch32.shape == ref.shape, (name, kernel.shape, torch32.shape, ref.shape)
    rms = lambda x: float(x.double().square().mean().sqrt())
    err_k, err_t, scale = rms(kernel.detach().double() - ref), rms(torch32.detach().double() - ref), rms(ref)
    ratio = err_k / err_t if err_t > 0 else (0.0 if err_k == 0 else float("inf"))
    line = f"fp64-budget {name} [rms] err_k={err_k:.3e} err_t={err_t:.3e} ratio={ratio:.3g} scale={scale:.3e}"
    print(line)
    bound = margin * err_t + floor_ulps * ULP * max(scale, TINY)
    assert err_k <= bound, f"{line} bound={bound:.3e}"
    return ratio


def policy_loss_rounding(inputs, eps_clip):
    """What fp32 rounding of the exponent's argument alone does to the policy LOSS — one number, a mean over rows n elements
    whose terms cancel — to first order at the fp64 evaluation: errors that a correct fp32 evaluation reaches whatever its
    order of operations.  (The gradients and the ratio are tensors: their fp32 yardstick is a maximum over many elements and
    needs no such floor.  The loss of the fp32 composition can come out within a fraction of an ulp by luck, and the advantages
    are zero-mean, so the loss — the scale of the 8-ulp floor — is far smaller than its terms.)

    ratio = exp(x), x = log p - old.  log p is a sum of a terms T_k = d_k^2 / (2 var_k) + log sigma_k + log sqrt(2 pi), old a sum
    of a stored components, each accumulated in fp32: a partial sum P is rounded within 2^-24 |P| (uniform: variance
    (2^-24 P)^2 / 3, ``gate_rounding``'s model; measured sums have 0.74 of this sigma), every term carries two such roundings
    of its own (the quotient, the sum with its constants), and the difference log p - old one more.  Behind them, the fp32 sums
    over the agents: mu (partial sums M_i; d x / d mu_k = d_k / var_k) and the log-std (partial sums L_i;
    d x / d ls_k = d_k^2 / var_k - 1).  So
        var x = (2^-24)^2 / 3 * (sum_k P_k^2 + 2 sum_k T_k^2 + sum_k O_k^2 + x^2
                                 + sum_k (d_k / var_k)^2 sum_i M_ik^2 + sum_k (d_k^2 / var_k - 1)^2 sum_i L_ik^2).
    An element's surrogate min(ratio A, clamp(ratio) A) moves by w A ratio dx, w = 1 where the unclipped branch is the smaller
    one or the ratio is inside the range, 0 where the clipped branch is; its own product and exponential add three roundings of
    2^-24 |s|.  Where the elements' roundings are independent the loss, their mean, has
        sigma_i^2 = sum_i ((w_i A_i ratio_i)^2 var x_i + (2^-24)^2 s_i^2) / (rows n)^2.
    They are not all independent: what the rows share — the density's constants where the log-std is one number (the fixed-std
    policy, a head at an end of its range), and the partial sums of terms T_k that are those constants plus a small square —
    is rounded the same way in every element, and a common dx moves the loss by dx mean_i(w_i A_i ratio_i), which does not
    average out (the clipped elements are missing from the mean on one side of each sign of A: 1.4 % of the ratios' scale at
    eps_clip 0.2 with ratios exp(0.1 randn)).  The fp32 composition's dx has a mean of 0.2 to 0.6 of its root mean square on
    the families of ``policy_families``; the figure allows all of it to be common:
        sigma_c = rms_i(sqrt(var x_i)) |mean_i(w_i A_i ratio_i)|,    3 sqrt(sigma_i^2 + sigma_c^2).
    tests/test_fp64_budget_cpu.py holds it against the fp32 composition's own loss over many draws, and that a budget with
    this floor still rejects a loss with one row left out."""
    import math
    means, log_stds, actions, old, adv = (t.detach().double() for t in inputs)
    mu, ls = means.sum(1, keepdim=True), log_stds.sum(1, keepdim=True)
    var = th.exp(2.0 * ls)
    d = actions - mu                                                                   # [rows, n, a]
    terms = d.square() / (2.0 * var) + ls + 0.5 * math.log(2.0 * math.pi)
    x = -terms.sum(-1) - old.sum(-1)
    m_sq = means.cumsum(1).square().sum(1, keepdim=True)                               # [rows, 1, a]
    l_sq = log_stds.cumsum(1).square().sum(1, keepdim=True)
    var_x = (ULP ** 2 / 3.0) * (terms.cumsum(-1).square().sum(-1) + 2.0 * terms.square().sum(-1) + old.cumsum(-1).square().sum(-1)
                                + x.square() + ((d / var).square() * m_sq).sum(-1) + ((d.square() / var - 1.0).square() * l_sq).sum(-1))
    ratio = th.exp(x)
    s1, s2 = ratio * adv, th.clamp(ratio, 1.0 - eps_clip, 1.0 + eps_clip) * adv
    w = (s1 <= s2).double()
    sigma2 = ((w * adv * ratio).square() * var_x + ULP ** 2 * th.minimum(s1, s2).square()).sum() / float(adv.numel()) ** 2
    common2 = var_x.mean() * (w * adv * ratio).mean().square()
    return 3.0 * (sigma2 + common2).sqrt()


# ---------------------------------------------------------------------------------------------------------------------------
# csrc/wgrad.hip (flexnet_wgrad, flexnet_wgrad_batched) and csrc/linear.hip (flexnet_linear2): tests/test_wgrad_fp64_gpu.py and
# tests/test_linear_fp64_gpu.py.  The plain products with their wrong evaluations, the floor of a sum of products, the families
# (CPU generator: tests/test_fp64_budget_cpu.py holds the conditions on the very cases) and the shapes both files run.

WGRAD_WRONG = ("drop_last_row", "drop_slab_tail", "colsum_per_chunk")
LINEAR2_WRONG = ("drop_last_action_piece", "bias_twice")
WGRAD_FAMILIES = ("plain", "offset", "constant", "halves", "zero_x", "zero_dy", "mixed")
LINEAR2_FAMILIES = ("plain", "offset", "constant", "halves", "zero_x", "mixed")
WGRAD_MIXED_OF = ("plain", "zero", "x30")
CONSTANT_X = 1.3
HALVES_X = 30.0
# (k, m, n) per shape class (MT, NT) of csrc/wgrad.hip's dispatcher, on both sides of m = 32/33, 64/65 and n = 32/33, 64/65,
# 160/161 (the column-chunk step of NT = 5) and 128/129 (that of NT = 2 under MT = 6)
WGRAD_SHAPES = {
    (1, 1): [(1, 1, 1), (9, 32, 32)],
    (1, 2): [(65, 32, 33), (130, 4, 64)],
    (1, 5): [(129, 32, 65), (515, 7, 161)],
    (2, 1): [(63, 33, 32), (257, 64, 20)],
    (2, 2): [(64, 64, 64), (2051, 33, 33)],
    (2, 5): [(2049, 64, 160), (1003, 64, 321), (513, 40, 149)],
    (6, 1): [(66, 65, 32), (2050, 192, 1)],
    (6, 2): [(7, 192, 65), (2053, 100, 64), (300, 65, 129)],
}
WGRAD_CAP_SHAPE = (32777, 64, 20)       # 513 64-row slabs against the cap of 512: 72-row blocks, the last one of 17 rows
WGRAD_CAP_FAMILIES = ("plain", "constant")
WGRAD_TWO_SHAPES = ((2049, 64, 720, 20), (515, 64, 75, 161))       # (k, m, n | n2): the second input block, class [2, 5]
WGRAD_TWO_FAMILIES = ("plain", "halves", "mixed")
LINEAR2_ROWS = (1, 31, 32, 33, 97, 2049)
LINEAR2_WIDTHS = ((8, 0), (8, 4), (144, 4), (248, 8), (256, 8), (432, 12), (504, 8), (512, 8), (720, 20), (736, 32), (768, 0))
LINEAR2_ID_COLUMNS = 5


def wgrad_chunks(m, n):
    """The column chunks of csrc/wgrad.hip's shape class of an [m, n] result (nets._wgrad_class)."""
    from safe_marl_amd.nets import _wgrad_class
    return _wgrad_class(m, n)[2]


def linear2_ss(k1, k2):
    """The ``SS`` instantiation flexnet_linear2's entry point picks: 32-column super-steps per wavefront of eight."""
    return ((k1 + k2 + 31) // 32 + 7) // 8


def wgrad_plain(dy, x, wrong=None):
    """(dW, db) = (dy^T x, the column sum of dy) in the dtype given.  ``wrong``: one of WGRAD_WRONG, the wrong evaluations
    tests/test_fp64_budget_cpu.py has the budget reject — the sum over rows 0 .. k - 2 ("drop_last_row"); the rows past the last
    multiple of 8 of every 64-row slab left out, which only a partial last slab has ("drop_slab_tail": a block that rounds its
    rows DOWN to whole 8-row groups); the column sum times the column chunks of the shape class ("colsum_per_chunk": every chunk
    accumulates it in the kernel and only chunk 0 may store)."""
    assert wrong is None or wrong in WGRAD_WRONG, wrong
    k = dy.shape[0]
    if wrong == "drop_last_row":
        dy, x = dy[:k - 1], x[:k - 1]
    elif wrong == "drop_slab_tail":
        r = th.arange(k, device=dy.device)
        slab_rows = (k - 64 * (r // 64)).clamp(max=64)
        keep = (r % 64) < (slab_rows // 8) * 8
        dy, x = dy[keep], x[keep]
    c, cs = dy.t() @ x, dy.sum(0)
    if wrong == "colsum_per_chunk":
        cs = cs * wgrad_chunks(dy.shape[1], x.shape[1])
    return c, cs


def linear2_plain(bias, x1, x2, W, c1, c2, wrong=None):
    """include/flexnet.h's formula of flexnet_linear2 in the dtype given: bias + x1 W[:, c1:c1+k1]^T + x2 W[:, c2:c2+k2]^T (x2
    None or of no columns: no second block).  ``wrong``: one of LINEAR2_WRONG — the last four action columns left out, the bias
    added twice."""
    assert wrong is None or wrong in LINEAR2_WRONG, wrong
    k1 = x1.shape[1]
    k2 = 0 if x2 is None else x2.shape[1]
    out = bias + x1 @ W[:, c1:c1 + k1].t()
    if wrong == "drop_last_action_piece":
        k2 = max(k2 - 4, 0)
    if k2 > 0:
        out = out + x2[:, :k2] @ W[:, c2:c2 + k2].t()
    if wrong == "bias_twice":
        out = out + bias
    return out


def ordered_sum_rounding(segments):
    """``row_sum_rounding`` for addends that are NOT exchangeable along the summed dimension: ``segments`` lists, in summation
    order, (L, mean, variance) of runs of L addends each of which is exchangeable in itself.  The partial sum j addends into a
    run that starts at the prefix P (the sum of the runs before it) has mean square (P + j m)^2 + j (1 - j / L) v; summed over
    the run: L P^2 + P m L^2 + m^2 L^3 / 3 + v L^2 / 6.  One run is row_sum_rounding's own figure.  It is what a running fp32 sum
    IN THIS ORDER does, the least accurate order a correct kernel may use: where the first half of the addends is +30 and the
    second -30 the partial sums reach 15 N on a result of order sqrt(N), which the exchangeable form (partial sums of order
    30 sqrt(N)) does not know — tests/test_fp64_budget_cpu.py's running sum failed the ``halves`` family with it."""
    total, prefix = None, None
    for L, mean, var in segments:
        L = float(L)
        p = th.zeros_like(mean) if prefix is None else prefix
        s = L * p.square() + p * mean * L ** 2 + mean.square() * L ** 3 / 3.0 + var * L ** 2 / 6.0
        total = s if total is None else total + s
        prefix = p + L * mean
    return 3.0 * ULP * (total / 3.0).sqrt()


def equal_addend_drift(mean, var, n):
    """What a running fp32 sum of ``n`` EQUAL addends c loses beyond ``row_sum_rounding``, element by element (zero where the
    addends of an element are not all equal: ``var`` above 1e-12 of ``mean``^2).  row_sum_rounding takes the roundings of the
    partial sums to be independent and adds them in quadrature: sqrt(n) / 3 ulps of the sum.  With equal addends they are not:
    a partial sum inside the binade [2^b, 2^(b+1)) is a multiple of u_b = 2^(b-23), so S + c is rounded by the same amount
    e_b(c), |e_b| <= u_b / 2, at every step inside that binade, and the 2^b / c steps of a binade add LINEARLY.  The binades
    below the last one, 2^B <= n c, contribute a geometric series, 2^(2B-24) / (3 c), the last one (n c - 2^B) / c steps of
    2^(B-24): in all 2^(B-24) (2^B / 3 + n c - 2^B) / c, up to n / 3 ulps of the sum.  tests/test_fp64_budget_cpu.py's running
    sum of the ``constant`` family was off by 458 ulps at 2 049 rows (sqrt(n) / 3: 15) and by 2 440 at 32 777, inside this
    figure (683 and 11 580).  A kernel that keeps a running sum per thread block over a few hundred rows and folds the blocks in
    a tree stays far inside it; the row-order running sum is the least accurate order a correct kernel may use."""
    c = mean.detach().double().abs()
    s = float(n) * c
    safe = s.clamp(min=TINY)
    top = th.exp2(th.floor(th.log2(safe)))
    drift = top * ULP * (top / 3.0 + (safe - top)) / c.clamp(min=TINY)
    equal = (var <= 1e-12 * c.square()) & (c > 0)
    return th.where(equal, drift, th.zeros_like(drift))


def product_sum_rounding(dy, x, split=None):
    """``row_sum_rounding`` of the addends dy[:, m, None] * x[:, None, n] of dW = dy^T x, [m, n], without materialising them: the
    mean over rows of the addends is dy^T x / k and their second moment (dy^2)^T (x^2) / k, two fp64 GEMMs.  ``split``: the
    rows [0, split) and [split, k) are two runs of ``ordered_sum_rounding`` (the ``halves`` family, whose order matters).  Elements
    whose addends are all equal (the ``constant`` family) get ``equal_addend_drift`` on top."""
    d, xx = dy.detach().double(), x.detach().double()
    k = d.shape[0]
    bounds = [0, k] if split is None or split <= 0 or split >= k else [0, int(split), k]
    segments = []
    for lo, hi in zip(bounds[:-1], bounds[1:]):
        L = float(hi - lo)
        mean = d[lo:hi].t() @ xx[lo:hi] / L
        second = d[lo:hi].square().t() @ xx[lo:hi].square() / L
        segments.append((L, mean, (second - mean.square()).clamp_(min=0.0)))
    floor = ordered_sum_rounding(segments)
    if len(segments) == 1:
        floor = floor + equal_addend_drift(segments[0][1], segments[0][2], k)
    return floor


def linear2_sum_rounding(x1, x2, W, c1, c2, split=None):
    """The same floor for flexnet_linear2's output [rows, 64]: element (r, u) is a sum over the N = k1 + k2 input columns of
    x[r, c] W[u, column of c] (the bias is one more addend: one rounding, inside FLOOR_ULPS).  ``split``: a column count, as
    ``product_sum_rounding``'s row count."""
    k1 = x1.shape[1]
    k2 = 0 if x2 is None else x2.shape[1]
    xs = x1 if k2 == 0 else th.cat((x1, x2), 1)
    ws = W[:, c1:c1 + k1] if k2 == 0 else th.cat((W[:, c1:c1 + k1], W[:, c2:c2 + k2]), 1)
    return product_sum_rounding(xs.t(), ws.t(), split)


def wgrad_floors(fam):
    """(floor of dW [m, n], floor of the column sum [m]) of a ``wgrad_families`` case, element by element."""
    dy, x = fam.inputs
    d = dy.detach().double()
    return (product_sum_rounding(dy, x, fam.params.get("split")),
            row_sum_rounding(dy) + equal_addend_drift(d.mean(0), d.var(0, unbiased=False), d.shape[0]))


def wgrad_families(k, m, n, generator):
    """The named input families of dW = dy^T x over ``k`` rows, inputs (dy [k, m], x [k, n]), from a CPU generator.

    plain      randn for both operands.
    offset     x = randn + 30: every addend of an element has a mean (30 dy) far above what is left after the rows cancel.
    constant   dy = CONSTANT_BIAS, x = CONSTANT_X everywhere: nothing cancels and a running sum drifts.
    halves     dy = 1 + 0.1 randn; x = +30 + 0.5 randn on the first ceil(k / 2) rows, -30 + 0.5 randn on the rest: partial sums
               of order 15 k, a result of order sqrt(k).  ``params["split"]`` is the row where the sign turns: the order
               matters to the floor (``ordered_sum_rounding``).
    zero_x     x exactly zero: dW must be exactly zero (within_budget's TINY floor); the column sum is plain's.
    zero_dy    dy exactly zero: dW and the column sum exactly zero.
    mixed      x's rows cycle plain / zero / 30 x plain (``groups``), so one 8-row group and one 64-row slab hold each kind;
               dy is plain's."""
    g = generator
    dy, x = th.randn(k, m, generator=g), th.randn(k, n, generator=g)
    half = (k + 1) // 2
    sign = th.where(th.arange(k) < half, 1.0, -1.0).view(k, 1)
    hdy = 1.0 + 0.1 * th.randn(k, m, generator=g)
    hx = HALVES_X * sign + 0.5 * th.randn(k, n, generator=g)
    groups = th.arange(k) % len(WGRAD_MIXED_OF)
    mx = x.clone()
    mx[groups == 1] = 0.0
    mx[groups == 2] *= 30.0
    return {"plain": Family("plain", (dy, x), {}),
            "offset": Family("offset", (dy, x + 30.0), {}),
            "constant": Family("constant", (th.full((k, m), CONSTANT_BIAS), th.full((k, n), CONSTANT_X)), {}),
            "halves": Family("halves", (hdy, hx), {"split": half}),
            "zero_x": Family("zero_x", (dy, th.zeros(k, n)), {}),
            "zero_dy": Family("zero_dy", (th.zeros(k, m), x), {}),
            "mixed": Family("mixed", (dy, mx), {}, groups)}


def linear2_families(rows, k1, k2, generator):
    """The named input families of flexnet_linear2 on ``rows`` rows: inputs (bias [64], x1 [rows, k1], x2 [rows, k2], W [64, k1 +
    LINEAR2_ID_COLUMNS + k2]) with c1 = 0, c2 = k1 + LINEAR2_ID_COLUMNS; the id columns of W hold NaN (the kernel must skip
    them).  The families are ``wgrad_families``' on the input rows, the summed dimension being the N = k1 + k2 columns:

    plain      x randn, W 0.3 randn, bias randn.
    offset     x = randn + 30.
    constant   x = CONSTANT_X everywhere and W = CONSTANT_BIAS / 8 everywhere: every output is N equal addends and the bias.
    halves     W = 1 + 0.1 randn; x = +30 + 0.5 randn in the first ceil(N / 2) columns, -30 + 0.5 randn in the rest
               (``params["split"]``: that column count).
    zero_x     x exactly zero: the output is the bias, bit for bit.
    mixed      the rows cycle plain / zero / 30 x plain (``groups``): one 32-row tile holds each kind."""
    g = generator
    N, ldw = k1 + k2, k1 + LINEAR2_ID_COLUMNS + k2
    c2 = k1 + LINEAR2_ID_COLUMNS

    def weights(cols):
        W = th.full((64, ldw), float("nan"))
        W[:, :k1], W[:, c2:] = cols[:, :k1], cols[:, k1:]
        return W

    def parts(xs):
        return xs[:, :k1].contiguous(), xs[:, k1:].contiguous()

    bias = th.randn(64, generator=g)
    xs = th.randn(rows, N, generator=g)
    W = weights(0.3 * th.randn(64, N, generator=g))
    half = (N + 1) // 2
    sign = th.where(th.arange(N) < half, 1.0, -1.0).view(1, N)
    hW = weights(1.0 + 0.1 * th.randn(64, N, generator=g))
    hx = HALVES_X * sign + 0.5 * th.randn(rows, N, generator=g)
    groups = th.arange(rows) % len(WGRAD_MIXED_OF)
    mx = xs.clone()
    mx[groups == 1] = 0.0
    mx[groups == 2] *= 30.0
    return {"plain": Family("plain", (bias, *parts(xs), W), {}),
            "offset": Family("offset", (bias, *parts(xs + 30.0), W), {}),
            "constant": Family("constant", (bias, *parts(th.full((rows, N), CONSTANT_X)), weights(th.full((64, N), CONSTANT_BIAS / 8))), {}),
            "halves": Family("halves", (bias, *parts(hx), hW), {"split": half}),
            "zero_x": Family("zero_x", (bias, *parts(th.zeros(rows, N)), W), {}),
            "mixed": Family("mixed", (bias, *parts(mx), W), {}, groups)}


def wgrad_case(k, m, n):
    """``wgrad_families`` of one shape from the seed both tests/test_wgrad_fp64_gpu.py and tests/test_fp64_budget_cpu.py use."""
    return wgrad_families(k, m, n, th.Generator().manual_seed(1000003 * k + 1009 * m + n))


def wgrad_cases():
    """Every (shape class, (k, m, n), family names) the GPU test runs: WGRAD_SHAPES on every family, the cap shape, and the
    two-block shapes with x = [x | x2] as one operand."""
    out = [(cls, shape, WGRAD_FAMILIES) for cls, shapes in WGRAD_SHAPES.items() for shape in shapes]
    out.append(((2, 1), WGRAD_CAP_SHAPE, WGRAD_CAP_FAMILIES))
    return out + [((2, 5), (k, m, n + n2), WGRAD_TWO_FAMILIES) for k, m, n, n2 in WGRAD_TWO_SHAPES]


def linear2_case(rows, k1, k2):
    """``linear2_families`` of one shape from the seed both tests/test_linear_fp64_gpu.py and the CPU test use."""
    return linear2_families(rows, k1, k2, th.Generator().manual_seed(1000003 * rows + 1009 * k1 + k2))


# ---------------------------------------------------------------------------------------------------------------------------
# csrc/optim.hip (flexnet_clip_rmsprop through optim.clip_and_step) and the scalar mean of csrc/tdloss.hip (flexnet_scaled_sum
# through util.mean_all): tests/test_optim_fp64_gpu.py.  The plain step with its wrong evaluations, the tensor layouts on both
# sides of the kernel's own sizes (16 384 threads, four elements each per trip: 65 536 flat elements), the families (CPU
# generator: tests/test_fp64_budget_cpu.py holds the conditions on the very cases) and the derived bound of a mean.

OPTIM_LR, OPTIM_ALPHA, OPTIM_EPS = 1e-3, 0.99, 1e-5          # trainer.py:34-35
OPTIM_THREADS, OPTIM_PASS = 16384, 65536                     # csrc/optim.hip: OPT_BLOCKS * OPT_THREADS, times OPT_UNROLL
OPTIM_WRONG = ("eps_inside_root", "v_from_unclipped", "no_margin", "per_tensor_clip", "norm_first_pass_only")
OPTIM_FAMILIES = ("plain", "warm", "inactive", "tiny", "clip_margin", "large", "zero", "zero_warm")
OPTIM_FAMILY_LAYOUTS = ("actor", "pass+1", "three_passes")   # where every family runs; every layout runs plain and warm
ACTOR_SHAPES = [(64, 149), (64,), (64,), (64,), (192, 64), (192, 64), (192,), (192,), (4, 64), (4,)]   # tests/test_optim_gpu.py
CRITIC_SHAPES = [(64, 745), (64,), (64,), (64,), (64, 64), (64,), (1, 64), (1,)]
MEAN_SIZES = (1, 2, 255, 256, 257, 16383, 16384, 16385, 32767, 32768, 32769, 100003)
MEAN_INPUTS = ("randn", "randn+1000", "constant")


def optim_layouts():
    """{name: element counts per tensor, in order} for the optimiser step's flat index space.  ``pass+1``: the first element
    of the second trip of both loops is a tensor of its own; ``cap``: FLEXNET_OPT_MAX_TENSORS tensors and
    FLEXNET_OPT_MAX_ELEMENTS elements at once."""
    import math
    t, p = OPTIM_THREADS, OPTIM_PASS
    return {"one": [1], "sixteen_ones": [1] * 16,
            "actor": [math.prod(s) for s in ACTOR_SHAPES], "critic": [math.prod(s) for s in CRITIC_SHAPES],
            "threads-1": [t - 1], "threads": [t], "threads+1": [t + 1],
            "pass-1": [1, t - 1, 7, p - t - 8], "pass": [1, t - 1, 7, p - t - 7], "pass+1": [1, t - 1, 7, p - t - 7, 1],
            "three_passes": [3, 70001, 1, 69996, 16], "cap": [1] * 15 + [2 ** 20 - 15]}


def clip_rmsprop_plain(params, grads, square_avgs, max_norm, lr, alpha, eps, wrong=None):
    """clip_grad_norm_(params, max_norm) followed by RMSprop(lr, alpha, eps).step() (no momentum, not centred, no weight
    decay) on lists of tensors, in their dtype and modifying none: (norm, new params, clipped grads, new square_avgs) with
        norm = the 2-norm over every gradient;  coef = clamp(max_norm / (norm + 1e-6), max=1);  g = g coef;
        v = alpha v + (1 - alpha) g^2;  p = p - lr g / (sqrt(v) + eps).
    ``max_norm`` <= 0 is that formula too (PyTorch's: the gradients come out zero, or turned round).  ``wrong``: one of
    OPTIM_WRONG, the wrong evaluations tests/test_fp64_budget_cpu.py has the budget reject — sqrt(v + eps); v moved by the
    unclipped gradient; the coefficient without its 1e-6; every tensor clipped by its own norm; the norm over the first
    OPTIM_PASS flat elements alone (a loop that loses its second trip)."""
    assert wrong is None or wrong in OPTIM_WRONG, wrong
    if len(grads) == 0:
        return th.zeros(()), [], [], []
    seen = grads
    if wrong == "norm_first_pass_only" and sum(g.numel() for g in grads) > OPTIM_PASS:
        seen = [th.cat([g.reshape(-1) for g in grads])[:OPTIM_PASS]]
    norm = th.linalg.vector_norm(th.stack([th.linalg.vector_norm(g) for g in seen]))

    def coefficient(nrm):
        return th.clamp(max_norm / (nrm if wrong == "no_margin" else nrm + 1e-6), max=1.0)

    coef = coefficient(norm)
    new_p, new_g, new_v = [], [], []
    for p, g, v in zip(params, grads, square_avgs):
        gc = g * (coefficient(th.linalg.vector_norm(g)) if wrong == "per_tensor_clip" else coef)
        moved_by = g if wrong == "v_from_unclipped" else gc
        vn = alpha * v + (1.0 - alpha) * moved_by * moved_by
        avg = (vn + eps).sqrt() if wrong == "eps_inside_root" else vn.sqrt() + eps
        new_p.append(p - lr * (gc / avg))
        new_g.append(gc)
        new_v.append(vn)
    return norm, new_p, new_g, new_v


def optim_families(layout, generator):
    """The named input families of one optimiser step on tensors of ``layout`` elements each (flat: the kernels know no
    shapes), inputs (params, grads, square_avgs) as lists, ``params["max_norm"]`` the clip, from ONE set of base draws per
    tensor on a CPU generator: p = 0.1 randn (every family's parameters), g = randn, r = rand.  ``warm`` state of a gradient
    x: v = (0.5 + r) x^2, what the running average has near after many such steps.

    plain        g, state zero (a first step: sqrt(v) = |g| / 10).
    warm         g, state warm.
    inactive     1e-3 g, warm: the norm is below max_norm 1 up to 10^6 elements, the coefficient exactly 1.
    tiny         1e-6 g, state zero: sqrt(v) = 1e-7 |g| is far below eps, the step is lr g / eps.
    clip_margin  g scaled (in fp64) to a norm of 2e-3, warm, max_norm 1e-3: the 1e-6 is 5e-4 of the coefficient.
    large        1e15 g, warm: squares near the top of fp32 — the sum over 2^20 of them is still in range.
    zero         g exactly zero, state zero: nothing may move, and 0 / (0 + eps) is no NaN.
    zero_warm    g exactly zero, the state warm(randn): v decays by alpha, the parameters stay."""
    def draw(fn, scale=1.0):
        return [scale * fn(n, generator=generator) for n in layout]

    p, g, r = draw(th.randn, 0.1), draw(th.randn), draw(th.rand)

    def warm(xs):
        return [(0.5 + ri) * x * x for ri, x in zip(r, xs)]

    def scaled(c):
        return [c * x for x in g]

    zeros = [th.zeros(n) for n in layout]
    norm = float(th.cat(g).double().norm())
    margin = [(x.double() * (2e-3 / norm)).float() for x in g]
    fam = lambda name, gr, v, max_norm=1.0: Family(name, (p, gr, v), {"max_norm": max_norm})
    return {"plain": fam("plain", g, zeros), "warm": fam("warm", g, warm(g)),
            "inactive": fam("inactive", scaled(1e-3), warm(scaled(1e-3))),
            "tiny": fam("tiny", scaled(1e-6), zeros),
            "clip_margin": fam("clip_margin", margin, warm(margin), 1e-3),
            "large": fam("large", scaled(1e15), warm(scaled(1e15))),
            "zero": fam("zero", zeros, zeros), "zero_warm": fam("zero_warm", zeros, warm(g))}


def optim_case(layout_name):
    """``optim_families`` of one named layout from the seed both tests/test_optim_fp64_gpu.py and the CPU test use."""
    layouts = optim_layouts()
    return optim_families(layouts[layout_name], th.Generator().manual_seed(1009 * list(layouts).index(layout_name) + 7))


def optim_run(fam, dtype, wrong=None, device="cpu"):
    """``clip_rmsprop_plain`` of a family's inputs cast to ``dtype`` with the trainer's RMSprop settings:
    {"norm": ..., "param": [...], "grad": [...], "square_avg": [...]}."""
    p, g, v = ([t.to(device=device, dtype=dtype) for t in ts] for ts in fam.inputs)
    out = clip_rmsprop_plain(p, g, v, fam.params["max_norm"], OPTIM_LR, OPTIM_ALPHA, OPTIM_EPS, wrong=wrong)
    return dict(zip(("norm", "param", "grad", "square_avg"), out))


def optim_within_budget(kernel, torch32, ref, *, name):
    """``within_budget`` on the norm and, tensor by tensor, on every parameter, gradient and square_avg of three results of
    ``optim_run``'s form; the list of ratios."""
    ratios = [within_budget(kernel["norm"], torch32["norm"], ref["norm"], name=f"{name} norm")]
    for key in ("param", "grad", "square_avg"):
        assert len(kernel[key]) == len(torch32[key]) == len(ref[key]), (name, key)
        for t, (k, y, r) in enumerate(zip(kernel[key], torch32[key], ref[key])):
            ratios.append(within_budget(k.reshape(-1), y.reshape(-1), r.reshape(-1), name=f"{name} {key}[{t}]"))
    return ratios


def mean_input(kind, n, generator):
    """One of MEAN_INPUTS, fp32 [n]: randn, randn + 1000 (the mean 1 000 times the spread: a running fp32 sum loses the spread),
    CONSTANT_BIAS everywhere (equal addends: a running fp32 sum drifts)."""
    assert kind in MEAN_INPUTS, kind
    if kind == "constant":
        return th.full((n,), CONSTANT_BIAS)
    x = th.randn(n, generator=generator)
    return x + 1000.0 if kind == "randn+1000" else x


def mean_within_bound(out, x, sign=1.0, *, name):
    """assert |out - m| <= 2^-23 |m| + 2^-52 sum|x| for ``out`` = sign * mean(x) of fp32 ``x``, m that mean in fp64 of the fp32
    numbers; the figures are printed in one line either way.  Derived, not measured, for a sum held in fp64 (csrc/tdloss.hip:
    flexnet_scaled_sum): the fp32 ``scale`` = sign / n and the final cast to fp32 each round by at most 2^-24 of the result;
    an fp64 sum of n addends in any order is within (n - 1) 2^-53 sum|x| of the exact one, so times 1 / n within 2^-53 sum|x| —
    doubled here.  A sum held in fp32 cannot meet it on inputs whose mean is far above their spread."""
    xd = x.detach().double().reshape(-1).cpu()
    m = float(sign) * float(xd.sum()) / xd.numel()
    err = abs(float(out) - m)
    bound = 2.0 ** -23 * abs(m) + 2.0 ** -52 * float(xd.abs().sum())
    line = f"fp64-mean {name} err={err:.3e} bound={bound:.3e} mean={m:.9e}"
    print(line)
    assert err <= bound, line
    return err
