"""flexenv_rollout_burst_mlp: the rollout of MADDPG / SAFEMADDPG with a shared MLP actor (agent_type: mlp) as ONE persistent launch
per run of steps — fc1, LayerNorm, ReLU, the 64 -> 64 layer and the head on the matrix cores, the exploration epilogue on the
kernel's own noise stream, SAFEMADDPG's projection, environment step with the replay sink.  k steps against k one-step launches
bit for bit; the noise stream and the epilogue against the RNN agent's burst bit for bit, and against the NumPy restatement of
the stream; the policy against fp64 on the project's error budget and against the agent-summed MLP burst bit for bit; the safety
phase against the stand-alone projection; the environment against a twin stepped launch by launch; replayed graphs; refusals on
a live handle; training; and the switch."""
import os
import sys
import warnings

import numpy as np
import pytest
import torch

from . import fp64_budget as fb

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = {77: None, 531: [3, 17, 28], 64: None}       # 77 x 5 agents: the tail block's second group is partly filled; 531 x 3
RNG0 = (1234, 5)                                       # [seed, step] every run starts its noise stream from
_WORLD = {}


def _env(n_envs, buildings=None, safe=False):
    from safe_marl_amd.flex_env import VecFlexProvisionEnv
    from safe_marl_amd.network import create_network
    from safe_marl_amd.series import make_synthetic_series
    env_args = {} if buildings is None else {"buildings": buildings, "pv_nodes": buildings, "ess_nodes": buildings}
    key = tuple(buildings or ())
    if key not in _WORLD:
        net = create_network(env_args)
        _WORLD[key] = (net, make_synthetic_series(net, n_days=30))
    net, series = _WORLD[key]
    if safe:
        env_args = dict(env_args, alg="safemaddpg")
    return VecFlexProvisionEnv(env_args, n_envs, device="cuda:0", net=net, series=series, seed=9, warm_start=True)


def _alg_args(alg, env, **over):
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    from train_maddpg import DEFAULT_ALG_ARGS, PPO_ALG_ARGS
    a = dict(DEFAULT_ALG_ARGS)
    if alg == "ippo":
        a.update(PPO_ALG_ARGS)
    a.update(alg=alg, agent_num=env.n_agents, obs_size=env.obs_size, state_size=env.state_size, action_dim=4, v_min=0.9,
             v_max=1.1, agent_type="mlp")
    a.update(over)
    return a


def _predictor(n):
    """A voltage predictor that makes the safety layer intervene for some buildings and not for others: the sensitivities of
    tests/test_rollout_gpu.py's, the intercepts from below the band's lower edge (0.9: the first building's predicted voltage is
    outside it whenever its net load is positive) up to that test's 0.915."""
    return (torch.full((n,), -0.08, dtype=torch.float64), torch.full((n,), -0.05, dtype=torch.float64),
            torch.linspace(0.895, 0.915, n, dtype=torch.float64))


def _spec(n_envs, na):
    rng = np.random.default_rng(4)
    return dict(day=rng.integers(0, 20, n_envs).astype(np.int32), hour=rng.integers(0, 24, n_envs).astype(np.int32),
                interval=rng.integers(0, 4, n_envs).astype(np.int32), e0=0.0125 + 0.001 * rng.random((n_envs, na)),
                a0=0.5 + 0.5 * rng.random((n_envs, 4 * na)))


def _rollout(alg, n_envs, monkeypatch, **over):
    """A model of ``alg`` with the MLP agent (``agent_type`` in ``over`` for the RNN's), the policy's parameters times ten (every
    layer matters), its RolloutGraph on an env reset to _spec, the noise stream at RNG0."""
    from safe_marl_amd import learner
    from safe_marl_amd.replay_buffer import TransReplayBuffer
    from safe_marl_amd.util import convert
    for k in ("FLEX_MLP_BURST", "FLEX_ROLLOUT_BURST", "FLEX_SUMMED_BURST", "FLEX_GAUSS_BURST"):
        monkeypatch.delenv(k, raising=False)
    safe = alg == "safemaddpg"
    env = _env(n_envs, SHAPES[n_envs], safe)
    args = convert(_alg_args(alg, env, **over))
    torch.manual_seed(21)
    np.random.seed(21)
    if safe:
        m = learner.SAFEMADDPG(args, env, predictor=_predictor(env.n_agents)).cuda()
    else:
        m = {"maddpg": learner.MADDPG, "ippo": learner.IPPO}[alg](args).cuda()
    with torch.no_grad():
        for p in m.policy_dicts.parameters():
            p.mul_(10.0)
    rg = learner.RolloutGraph(m, env, TransReplayBuffer(n_envs * 128, device="cuda"))
    rg.start_episode(env.reset(spec=_spec(n_envs, env.n_agents)))
    rg.rng_state.copy_(torch.tensor(RNG0, dtype=torch.int64))
    return rg, env


def _mlp_rollout(alg, n_envs, monkeypatch, **over):
    from safe_marl_amd.nets import MLPAgent
    rg, env = _rollout(alg, n_envs, monkeypatch, **over)
    assert type(rg.model.policy_dicts[0]) is MLPAgent
    assert rg.mlp_plain_burst and not rg.fast and not rg.mlp_burst and not rg.summed
    assert rg.sink_active and rg.ring_active and rg.fused_burst and rg.buf.row_mode
    return rg, env


def _steps(rg, bursts):
    for k in bursts:
        rg.body(burst=k)
        for _ in range(k or 1):
            rg.buf.stepped()
    torch.cuda.synchronize()


def _launch_outputs(rg):
    names = ["acc", "act_buf", "hid_buf", "means_buf", "burst_env_act"]
    if rg.safe:
        names += ["burst_adjusted", "burst_safe_env_act"]
    return names


@pytest.mark.parametrize("alg,n_envs,steps,over", [("maddpg", 77, 10, {}), ("maddpg", 531, 10, {}), ("safemaddpg", 77, 10, {}),
                                                   ("safemaddpg", 531, 10, {}), ("maddpg", 77, 10, {"layernorm": False}),
                                                   ("safemaddpg", 77, 1, {})])
def test_k_steps_equal_k_one_step_launches_bit_for_bit(alg, n_envs, steps, over, monkeypatch):
    """Eager body(burst=k) against k body() calls of a second model built from the same seeds — the same launch with one step —
    from the same rng_state: a batch that is no multiple of a block's sixteen environments (77: the tail block's second group
    holds five of its eight), five and three agents (partly filled policy tiles), with and without LayerNorm.  Every ring, both
    cursor cells, the noise position, the statistics, the launch's outputs and the environments' own state: identical bits."""
    runs = []
    for bursts in ((steps,), (0,) * steps):
        rg, env = _mlp_rollout(alg, n_envs, monkeypatch, **over)
        assert bool(rg.model.args.layernorm) == over.get("layernorm", True) and steps < rg.buf.slabs
        _steps(rg, bursts)
        runs.append((rg, env))
    (a, ea), (b, eb) = runs
    for p, q in zip(a.model.policy_dicts.parameters(), b.model.policy_dicts.parameters()):
        assert torch.equal(p, q)
    assert a.buf.k == b.buf.k == steps
    assert torch.equal(a.buf.cursor, b.buf.cursor)
    assert a.buf.cursor.tolist() == [steps % a.buf.slabs, (steps - 1) % a.buf.slabs]
    assert a.rng_state.tolist() == b.rng_state.tolist() == [RNG0[0], RNG0[1] + steps]
    for ring in ("row_ring", "hid_ring", "small_ring"):
        assert torch.equal(getattr(a.buf, ring), getattr(b.buf, ring)), ring
    for name in _launch_outputs(a):
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    for name in ("reward", "done", "info", "failed"):
        assert torch.equal(getattr(ea, name), getattr(eb, name)), name
    assert torch.equal(ea.get_state(), eb.get_state())
    assert torch.equal(ea.obs_view().clone(), eb.obs_view().clone())
    assert float(a.acc[:, 7].abs().sum().item()) > 0              # a non-zero reward sum
    assert torch.isfinite(a.buf.small_ring).all() and torch.isfinite(a.hid_buf).all()
    assert float(a.hid_buf.abs().max().item()) > 0 and float(a.buf.hid_ring.abs().max().item()) > 0
    assert float(a.act_buf.std().item()) > 0.01 and float(a.act_buf.abs().max().item()) <= 1.0


def test_noise_stream_and_epilogue_are_the_rnn_bursts_bit_for_bit(monkeypatch):
    """Head weight zero and the bias kept, in the MLPAgent's fc3 and in an RNNAgent's fc2: both policies' means are the bias, so
    from one rng_state the action and the env action of flexenv_rollout_burst_mlp equal those of flexenv_rollout_burst bit for
    bit — at each of three consecutive one-step launches (equal actions: the twin environments stay in step), which holds the
    counter layout (global row, action group, step) and the two-parity buffer — and of one three-step launch of each form, read
    from the replay's rows."""
    bias = torch.tensor([0.3, -0.2, 0.1, 0.45], device="cuda")
    for bursts in ((1, 1, 1), (3,)):
        sides = []
        for agent_type in ("mlp", "rnn"):
            rg, env = _rollout("maddpg", 77, monkeypatch, agent_type=agent_type)
            assert rg.fused_burst and rg.mlp_plain_burst == (agent_type == "mlp") and rg.fast == (agent_type == "rnn")
            agent = rg.model.policy_dicts[0]
            head = agent.fc3 if agent_type == "mlp" else agent.fc2
            with torch.no_grad():
                head.weight.zero_()
                head.bias.copy_(bias)
            sides.append((rg, env))
        (a, ea), (b, eb) = sides
        n = ea.n_agents
        for t, k in enumerate(bursts):
            _steps(a, (k,))
            _steps(b, (k,))
            assert torch.equal(a.means_buf, bias.expand(77 * n, 4)) and torch.equal(b.means_buf, a.means_buf)
            assert torch.equal(a.act_buf, b.act_buf), t
            assert torch.equal(a.burst_env_act, b.burst_env_act), t
            assert float(a.act_buf.std().item()) > 0.01
            assert a.rng_state.tolist() == b.rng_state.tolist()
        assert a.rng_state.tolist() == [RNG0[0], RNG0[1] + 3] and a.buf.k == b.buf.k == 3
        acts = a.buf.small_ring[:3, :, :4 * n]
        assert torch.equal(acts, b.buf.small_ring[:3, :, :4 * n])
        assert not torch.equal(acts[0], acts[1]) and not torch.equal(acts[1], acts[2])
        assert torch.equal(ea.reward, eb.reward) and torch.equal(ea.get_state(), eb.get_state())


@pytest.mark.parametrize("alg,n_envs", [("maddpg", 77), ("safemaddpg", 531)])
def test_noise_with_real_weights(alg, n_envs, monkeypatch):
    """action against tanh(means + std z) with z from the NumPy restatement of actor_noise4 (tests/test_actor_gpu.py) at the
    launch's own means, within that file's tolerance for the same comparison (2e-5: fast_tanh against torch.tanh); env_action is
    translate_action of the stored action, exactly.  Two one-step launches: steps RNG0[1] and RNG0[1] + 1 of the stream."""
    from safe_marl_amd.util import scale_action
    from .test_actor_gpu import _noise_restatement
    rg, env = _mlp_rollout(alg, n_envs, monkeypatch)
    rows = n_envs * env.n_agents
    for t in range(2):
        _steps(rg, (1,))
        z = torch.from_numpy(_noise_restatement(RNG0[0], RNG0[1] + t, rows, 4)).float().cuda()
        want = torch.tanh(rg.means_buf + rg.std * z)
        assert rg.std > 0 and float(z.std().item()) > 0.9
        assert (rg.act_buf - want).abs().max().item() < 2e-5, t
        assert torch.equal(rg.burst_env_act, scale_action(rg.model.args, rg.act_buf).to(torch.float32)), t


def _references(rg, obs):
    """(means, h) of the shared agent on ``obs`` [N, n, o] fp32: the fp64 reference — a deep copy of the module in fp64 on the fp32
    observations with the id columns — and the fp32 yardstick, tests/fp64_budget.py's plain composition.  Neither from the kernel."""
    m = rg.model
    agent, n = m.policy_dicts[0], m.n_
    agent_id = bool(m.args.agent_id)
    rows = obs.reshape(-1, obs.shape[-1]).contiguous()
    with torch.no_grad():
        inputs = fb.with_ids(rows, n) if agent_id else rows
        out64 = fb.ref64(agent)(inputs.double(), None)
        out32 = fb.mlp_actor_plain(agent, rows, n, agent_id)
    return (out64[0], out64[2]), (out32[0], out32[1])


@pytest.mark.parametrize("alg,n_envs,steps,over", [("maddpg", 531, 10, {}), ("safemaddpg", 77, 10, {}),
                                                   ("maddpg", 77, 1, {"layernorm": False}), ("maddpg", 77, 1, {"agent_id": False})])
def test_policy_against_fp64(alg, n_envs, steps, over, monkeypatch):
    """One-step launches from the reset state: before each the observation the policy phase will read is materialised, after it
    means and h (hid_buf: what the phase stored, before the sink's mask) are held to the budget of tests/fp64_budget.py at its
    defaults — MARGIN times the fp32 composition's own error plus 8 ulps of the tensor's scale.  No element is excluded."""
    rg, env = _mlp_rollout(alg, n_envs, monkeypatch, **over)
    assert bool(rg.model.args.layernorm) == over.get("layernorm", True)
    assert bool(rg.model.args.agent_id) == over.get("agent_id", True)
    for t in range(steps):
        obs = rg.obs.clone()
        _steps(rg, (0,))
        (m64, h64), (m32, h32) = _references(rg, obs)
        name = f"mlp-plain-burst {alg} {n_envs}x{env.n_agents} {over or ''} step {t}"
        assert float(h64.abs().max()) > 0 and float(m64.abs().max()) > 0
        fb.within_budget(rg.hid_buf, h32, h64, name=name + " h")
        fb.within_budget(rg.means_buf, m32, m64, name=name + " means")


@pytest.mark.parametrize("n_envs", [77, 531])
def test_policy_phase_is_the_summed_mlp_bursts(n_envs, monkeypatch):
    """The same weights under IPPO through flexenv_rollout_burst_summed_mlp on the same observations (the reset state): the same
    means and the same h, bit for bit — it is the same policy phase, whatever the epilogue behind it."""
    a, ea = _mlp_rollout("maddpg", n_envs, monkeypatch)
    b, eb = _rollout("ippo", n_envs, monkeypatch)
    assert b.mlp_burst and not b.mlp_plain_burst
    b.model.policy_dicts.load_state_dict(a.model.policy_dicts.state_dict())
    assert torch.equal(a.obs.clone(), b.obs.clone())
    _steps(a, (1,))
    _steps(b, (1,))
    assert float(a.means_buf.abs().max().item()) > 0 and float(a.hid_buf.abs().max().item()) > 0
    assert torch.equal(a.means_buf, b.means_buf)
    assert torch.equal(a.hid_buf, b.hid_buf)


@pytest.mark.parametrize("alg,n_envs", [("maddpg", 77), ("maddpg", 531), ("safemaddpg", 77), ("safemaddpg", 531)])
def test_environment_and_safety_match_a_twin_stepped_launch_by_launch(alg, n_envs, monkeypatch):
    """A twin env reset with the same spec, launch by launch over six one-step launches: SAFEMADDPG's safe_env_action and adjusted
    equal the stand-alone safety_project of the twin (in the state the launch's projection saw) on the stored action, bit for bit,
    and the layer intervenes; the twin stepped on the launch's env action (the projected one under SAFEMADDPG) has the burst's
    reward, done, row records and state, bit for bit; the replay keeps the policy's own action."""
    steps = 6
    rg, env = _mlp_rollout(alg, n_envs, monkeypatch)
    m, buf, n = rg.model, rg.buf, env.n_agents
    twin = _env(n_envs, SHAPES[n_envs], rg.safe)
    twin.reset(spec=_spec(n_envs, n))
    ring = torch.zeros(steps + 1, n_envs, n * buf.ROW_W, device="cuda")
    cursor = torch.zeros(2, dtype=torch.int64, device="cuda")
    twin.set_obs_ring(cursor, n_envs * n * buf.ROW_W, steps + 1)
    hits = 0
    for t in range(steps):
        _steps(rg, (1,))
        action = rg.act_buf.view(n_envs, n, 4)
        small = buf.small_ring[t]
        assert torch.equal(small[:, :4 * n].reshape(n_envs, n, 4), action), t          # the policy's own action
        if rg.safe:
            adj, hit, env_action = twin.safety_project(action, *m.predictor, m.V_min, m.V_max,
                                                       env_action_range=(m.args.action_low, m.args.action_high))
            assert torch.equal(rg.burst_adjusted, adj), t
            assert torch.equal(rg.burst_safe_env_act, env_action), t
            hits += int(hit.sum().item())
        else:
            env_action = rg.burst_env_act
        twin.step(env_action.view(n_envs, n, 4).contiguous(), auto_reset=True, obs_ring=ring)
        cursor += 1
        assert torch.equal(small[:, 4 * n:5 * n], twin.reward.to(torch.float32)[:, None].expand(n_envs, n)), t
        assert torch.equal(small[:, 5 * n], twin.done.to(torch.float32)), t
        assert torch.equal(env.reward, twin.reward) and torch.equal(env.done, twin.done), t
    torch.cuda.synchronize()
    assert not rg.safe or hits > 0
    assert torch.equal(buf.row_ring[1:steps + 1], ring[1:steps + 1])
    assert torch.equal(env.get_state(), twin.get_state())
    assert torch.equal(env.obs_view().clone(), twin.obs_view().clone())
    assert float(ring[1:].abs().sum().item()) > 0


@pytest.mark.parametrize("alg", ["maddpg", "safemaddpg"])
def test_replayed_graphs_equal_eager_calls(alg, monkeypatch):
    """capture(lengths=[10]) records one graph of one burst launch whose body launches the new kernel and none of the stand-alone
    policy, projection or step launches; two replays of it and one of the one-step graph leave what the eager calls
    body(burst=10) x 2 and body() leave from the same state, bit for bit; the noise differs from replay to replay."""
    from safe_marl_amd.util import audit_graph_body
    n_envs, runs = 64, []
    for graphed in (True, False):
        rg, env = _mlp_rollout(alg, n_envs, monkeypatch)
        acts = []
        if graphed:
            rg.capture(lengths=[10])
            assert sorted(k for k, _ in rg.bursts) == [10] and all(fused for _, fused in rg.bursts)
            cursor0 = rg.buf.cursor.clone()
            audit = audit_graph_body(lambda: rg.body(burst=10))
            rg.buf.cursor.copy_(cursor0)
            assert len([k for k in audit if "plain_mlp" in k and "flex_rollout_burst_kernel" in k]) == 1, audit
            assert not any(s in k for k in audit for s in ("sum_explore", "flex_step_kernel", "gauss_head", "actor_r16", "actor_mlp",
                                                           "rollout_pack", "flex_safety_kernel")), audit
            rg.start_episode(env.reset(spec=_spec(n_envs, env.n_agents)))
            rg.rng_state.copy_(torch.tensor(RNG0, dtype=torch.int64))
            assert rg.buf.k == 0
            calls = env.calls
            for _ in range(2):
                rg.run(10)
                torch.cuda.synchronize()
                acts.append(rg.act_buf.clone())
            rg.step()
            torch.cuda.synchronize()
            assert env.calls == calls                             # (replays make no host-side call)
        else:
            for _ in range(2):
                _steps(rg, (10,))
                acts.append(rg.act_buf.clone())
            _steps(rg, (0,))
        assert not torch.equal(acts[0], acts[1])
        runs.append((rg, env, acts))
    (a, ea, xa), (b, eb, xb) = runs
    slabs = a.buf.slabs
    assert a.buf.k == b.buf.k == 21 and a.buf.cursor.tolist() == b.buf.cursor.tolist() == [21 % slabs, 20 % slabs]
    assert a.rng_state.tolist() == b.rng_state.tolist() == [RNG0[0], RNG0[1] + 21]
    assert torch.equal(xa[0], xb[0]) and torch.equal(xa[1], xb[1])
    for ring in ("row_ring", "hid_ring", "small_ring"):
        assert torch.equal(getattr(a.buf, ring), getattr(b.buf, ring)), ring
    for name in _launch_outputs(a):
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    assert torch.equal(ea.get_state(), eb.get_state()) and torch.equal(ea.reward, eb.reward)


def test_entry_refuses_what_it_cannot_run(monkeypatch):
    """flexenv_rollout_burst_mlp's argument checks on a live handle: a burst as long as the ring, a sink without the aux counter
    (the agent-summed forms' sink), a sink whose aux counter is not the noise stream's, an explicit noise tensor, an env without
    the sink — FLEX_EINVAL, nothing launched, cursor cells and noise position untouched; then a burst runs."""
    from safe_marl_amd import _lib, nets
    rg, env = _mlp_rollout("maddpg", 64, monkeypatch)
    _steps(rg, (5,))
    cursor, calls, buf = rg.buf.cursor.clone(), env.calls, rg.buf
    refuse = pytest.raises(_lib.FlexLibraryError, match="flexenv_rollout_burst_mlp failed with code -22")
    with refuse:
        rg.body(burst=buf.slabs)                                  # steps >= slabs
    for aux in (None, torch.zeros(1, dtype=torch.int64, device="cuda")):
        env.set_replay_sink(rg.act_buf, rg.hid_buf, buf.small_ring, buf.hid_ring, rg.acc, cursor_out=buf.cursor[0:1],
                            aux_counter=aux)
        with refuse:
            rg.body(burst=4)
    rg._configure_env()
    real = nets.mlp_burst_actor_args

    def with_noise(*a, **k):
        args, mlp = real(*a, **k)
        args.noise = rg.means_buf.data_ptr()
        return args, mlp

    from safe_marl_amd import learner
    monkeypatch.setattr(learner, "mlp_burst_actor_args", with_noise)
    with refuse:
        rg.body(burst=4)
    monkeypatch.setattr(learner, "mlp_burst_actor_args", real)
    env.set_replay_sink(None, None, None, None, None)             # sink off
    with refuse:
        rg.body(burst=4)
    env.calls = calls
    rg._configure_env()                                           # the sink back on: the next burst runs
    torch.cuda.synchronize()
    assert torch.equal(rg.buf.cursor, cursor) and rg.rng_state.tolist() == [RNG0[0], RNG0[1] + 5]
    _steps(rg, (6,))
    assert rg.buf.k == 11 and rg.buf.cursor.tolist() == [11 % buf.slabs, 10 % buf.slabs]
    assert rg.rng_state.tolist() == [RNG0[0], RNG0[1] + 11]


@pytest.mark.parametrize("alg", ["maddpg", "safemaddpg"])
def test_training_rolls_out_through_the_burst(alg, monkeypatch):
    """PGTrainer at 64 envs, two train_process calls.  By default: no "capture failed" warning, the trainer keeps its graph
    rollout through RolloutGraph.mlp_plain_burst, losses and gradient norms are finite, the policy's weights move, and FALLBACKS
    gains no note beyond those of the same run with FLEX_MLP_BURST=0 — with which the flag is off and training still runs."""
    from safe_marl_amd import learner
    from safe_marl_amd.trainer import PGTrainer
    from safe_marl_amd.util import FALLBACKS, convert
    gained = {}
    for flag in ("0", "1"):
        monkeypatch.setenv("FLEX_MLP_BURST", flag)
        env = _env(64, None, alg == "safemaddpg")
        a = _alg_args(alg, env, behaviour_update_freq=60, target_update_freq=120)      # (one update event per episode, at step 60)
        torch.manual_seed(3)
        np.random.seed(3)
        tr = PGTrainer(convert(a), {"maddpg": learner.MADDPG, "safemaddpg": learner.SAFEMADDPG}[alg], env, None,
                       replay_capacity=64 * 96 * 2)
        m = tr.behaviour_net
        w0 = {k: v.detach().clone() for k, v in m.policy_dicts.state_dict().items()}
        before = dict(FALLBACKS)
        stat = {}
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            for _ in range(2):
                m.train_process(stat, tr)
        torch.cuda.synchronize()
        gained[flag] = {k for k, v in FALLBACKS.items() if v != before.get(k, 0)}
        assert tr.steps == 190
        rg = getattr(m, "_rollout_graph", None)
        if flag == "1":
            assert not any("rollout graph capture failed" in str(x.message) for x in w), [str(x.message) for x in w]
            assert tr.graph_rollout and rg.mlp_plain_burst and rg.fused_burst and rg.sink_active and rg.buf.row_mode
            assert rg.buf.k == 190 and rg.bursts and all(fused for _, fused in rg.bursts)
        else:                                                     # the rollout this configuration had before the burst
            assert rg is None or not (rg.mlp_plain_burst or rg.fused_burst or rg.sink_active)
        seen = {k: float(v) for k, v in stat.items() if "loss" in k or "grad_norm" in k}
        assert any("value_loss" in k for k in seen) and any("policy_loss" in k for k in seen), sorted(stat)
        assert all(np.isfinite(v) for v in seen.values()), seen
        assert all(torch.isfinite(p).all() for p in m.parameters())
        assert all(not torch.equal(v, w0[k]) for k, v in m.policy_dicts.state_dict().items())
    assert gained["1"] <= gained["0"], gained


def test_example_in_a_fresh_process():
    """examples/train_maddpg.py --agent-type mlp --alg maddpg in a process of its own: the rollout runs no library GEMM any more, so
    the update captures' warm-up must run what the captures run (the module composition of the MLP agent) — otherwise the
    library's first call of the process falls into a capture, where its set-up is refused and the process ends.  The run reports
    the new rollout and no fall-back beyond the composition's note."""
    import json
    import subprocess
    env = {k: v for k, v in os.environ.items() if k not in ("FLEX_MLP_BURST", "FLEX_ROLLOUT_BURST")}
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "train_maddpg.py"), "--alg", "maddpg", "--agent-type", "mlp",
                          "--envs", "64", "--episodes", "1"], capture_output=True, text=True, timeout=300, cwd=ROOT, env=env)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    res = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("{")][-1])
    assert res["rollout"] == "flexenv_rollout_burst_mlp" and res["agent_type"] == "mlp"
    assert set(res["fallbacks"]) <= {"actor_forward"}, res["fallbacks"]
    for k in ("mean_train_value_loss", "mean_train_policy_loss", "mean_train_reward"):
        assert np.isfinite(res["stat"][k]), (k, res["stat"])
