"""flexenv_rollout_burst_summed_mlp: the rollout of the agent-summed algorithms with a shared MLP actor (agent_type: mlp) as ONE
persistent launch per run of steps — fc1, LayerNorm, ReLU, the 64 -> 64 layer and the head on the matrix cores, agent-summed
selection (fixed std, or the Gaussian heads with FLEX_GAUSS_BURST=1), environment step with the replay sink.  k steps against k
one-step launches bit for bit; the policy against fp64 on the project's error budget; the Gaussian form's mean path against the
fixed-std form and its log-std head against fp64; the selection against flexnet_agent_sum_explore / flexnet_gauss_sum_explore;
the environment against a twin stepped launch by launch; replayed graphs; refusals; training; and the switch."""
import os
import sys
import warnings

import numpy as np
import pytest
import torch

from . import fp64_budget as fb

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAPE_STEPS = 123
BURSTS = (40, 23, 60)                         # (every episode ends at step 96: the restarts fall inside the third burst)
SHAPES = {77: [5], 531: [3, 17, 28], 203: [3, 9, 17, 28], 4100: None}


def _env(n_envs, buildings=None, device="cuda:0"):
    from safe_marl_amd.flex_env import VecFlexProvisionEnv
    from safe_marl_amd.network import create_network
    from safe_marl_amd.series import make_synthetic_series
    env_args = {} if buildings is None else {"buildings": buildings, "pv_nodes": buildings, "ess_nodes": buildings}
    net = create_network(env_args)
    series = make_synthetic_series(net, n_days=30)
    return VecFlexProvisionEnv(env_args, n_envs, device=device, net=net, series=series, seed=9, warm_start=True)


def _trainer(alg, n_envs, buildings=None, gaussian=False, **over):
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    from train_maddpg import DEFAULT_ALG_ARGS, PPO_ALG_ARGS
    from safe_marl_amd import learner
    from safe_marl_amd.trainer import PGTrainer
    from safe_marl_amd.util import convert
    env = _env(n_envs, buildings)
    a = dict(DEFAULT_ALG_ARGS)
    if alg == "ippo":
        a.update(PPO_ALG_ARGS)
    a.update(alg=alg, agent_num=env.n_agents, obs_size=env.obs_size, state_size=env.state_size, action_dim=4,
             behaviour_update_freq=30, batch_size=4, agent_type="mlp", gaussian_policy=gaussian)
    a.update(over)
    torch.manual_seed(3)
    np.random.seed(3)
    cls = {"matd3": learner.MATD3, "ippo": learner.IPPO}[alg]
    return PGTrainer(convert(a), cls, env, None, replay_capacity=n_envs * 96 * 2)


class _Tape:
    """torch.distributions.normal._standard_normal served from a fixed tape [123, N, 1, 4]: a launch's one draw of k steps
    (shape (k, N, 1, 4), k = 1 for a single step) gets rows pos .. pos + k - 1 and pos advances.  Every other shape goes to the
    real function."""

    def __init__(self, n_envs):
        import torch.distributions.normal as tdn
        self.real = tdn._standard_normal
        g = torch.Generator(device="cuda").manual_seed(11)
        self.tape = torch.randn(TAPE_STEPS, n_envs, 1, 4, device="cuda", generator=g)
        self.n_envs, self.pos, self.calls = n_envs, 0, 0

    def __call__(self, shape, dtype, device):
        shape = tuple(shape)
        if len(shape) == 4 and shape[1:] == (self.n_envs, 1, 4):
            out = self.tape[self.pos:self.pos + shape[0]]
            assert out.shape[0] == shape[0]
            self.pos += shape[0]
            self.calls += 1
            return out
        return self.real(shape, dtype, device)


def _spec(n_envs, na):
    rng = np.random.default_rng(4)
    return dict(day=rng.integers(0, 20, n_envs).astype(np.int32), hour=rng.integers(0, 24, n_envs).astype(np.int32),
                interval=rng.integers(0, 4, n_envs).astype(np.int32), e0=0.0125 + 0.001 * rng.random((n_envs, na)),
                a0=0.5 + 0.5 * rng.random((n_envs, 4 * na)))


def _rollout(alg, n_envs, monkeypatch, tape=None, gaussian=False, **over):
    """An MLP trainer, the policy's parameters times ten (every layer matters), reset to _spec."""
    import torch.distributions.normal as tdn
    from safe_marl_amd.learner import RolloutGraph
    from safe_marl_amd.nets import MLPAgent, MLPAgentGaussian
    monkeypatch.delenv("FLEX_MLP_BURST", raising=False)
    monkeypatch.setenv("FLEX_GAUSS_BURST", "1" if gaussian else "0")
    if tape is not None:
        monkeypatch.setattr(tdn, "_standard_normal", tape)
    tr = _trainer(alg, n_envs, SHAPES.get(n_envs), gaussian, **over)
    m = tr.behaviour_net
    assert type(m.policy_dicts[0]) is (MLPAgentGaussian if gaussian else MLPAgent)
    with torch.no_grad():
        for p in m.policy_dicts.parameters():
            p.mul_(10.0)
    rg = RolloutGraph(m, tr.env, tr.replay_buffer)
    assert rg.summed and rg.mlp_burst and rg.gaussian == gaussian
    assert not rg.summed_sink and not rg.summed_burst and not rg.gauss_burst and not rg.fast
    assert rg.sink_active and rg.ring_active and rg.fused_burst and rg.buf.row_mode
    rg.start_episode(tr.env.reset(spec=_spec(n_envs, tr.env.n_agents)))
    if tape is not None:
        tape.pos = tape.calls = 0
    return rg, tr


@pytest.mark.parametrize("alg,n_envs,gaussian", [("ippo", 77, False), ("ippo", 531, False), ("ippo", 203, False),
                                                 ("ippo", 4100, False), ("matd3", 531, False), ("ippo", 531, True),
                                                 ("ippo", 77, True)])
def test_k_steps_equal_k_one_step_launches_bit_for_bit(alg, n_envs, gaussian, monkeypatch):
    """Eager body(burst=k) for k = 40, 23, 60 against 123 body() calls of a second trainer — the same launch with one step — on
    one noise tape: a batch that is not a multiple of a block's sixteen environments (tail block, empty second group), more
    blocks than CUs (4100 -> 257), one / three / four / five agents (partly filled policy tiles), the episodes' restart inside
    the last burst.  Every ring, cursor, statistic and the environments' own state: identical bits."""
    tape = _Tape(n_envs)
    runs = []
    for bursts in (BURSTS, (0,) * TAPE_STEPS):
        rg, tr = _rollout(alg, n_envs, monkeypatch, tape, gaussian)
        assert max(BURSTS) < rg.buf.slabs
        for k in bursts:
            rg.body(burst=k)                                      # (one _standard_normal call and one launch each)
            for _ in range(k or 1):
                rg.buf.stepped()
        torch.cuda.synchronize()
        assert tape.pos == TAPE_STEPS == sum(BURSTS) and tape.calls == len(bursts)
        runs.append((rg, tr))
    (a, ta), (b, tb) = runs
    na = ta.env.n_agents
    assert a.buf.k == b.buf.k == TAPE_STEPS
    assert torch.equal(a.buf.cursor, b.buf.cursor)
    assert a.buf.cursor.tolist() == [TAPE_STEPS % a.buf.slabs, (TAPE_STEPS - 1) % a.buf.slabs]
    for ring in ("row_ring", "hid_ring", "small_ring"):
        assert torch.equal(getattr(a.buf, ring), getattr(b.buf, ring)), ring
    for name in ("acc", "act_buf", "hid_buf", "means_buf", "env_act_buf") + (("log_stds_buf",) if gaussian else ()):
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    for name in ("reward", "done", "info", "failed"):
        assert torch.equal(getattr(ta.env, name), getattr(tb.env, name)), name
    assert torch.equal(ta.env.obs_view().clone(), tb.env.obs_view().clone())
    assert float(a.acc[:, 7].abs().sum().item()) > 0              # a non-zero reward sum
    assert torch.isfinite(a.buf.small_ring).all() and torch.isfinite(a.hid_buf).all()
    assert float(a.hid_buf.abs().max().item()) > 0 and float(a.buf.hid_ring.abs().max().item()) > 0
    # the ONE action of an environment in every agent's row
    act = a.act_buf.view(n_envs, na, 4)
    assert torch.equal(act, act[:, :1].expand(n_envs, na, 4))


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


@pytest.mark.parametrize("n_envs,steps,over", [(531, 10, {}), (77, 10, {}), (77, 1, {"layernorm": False}),
                                               (77, 1, {"agent_id": False})])
def test_policy_against_fp64(n_envs, steps, over, monkeypatch):
    """One-step launches from the reset state: before each the observation the policy phase will read is materialised, after it
    means and h (hid_buf: what the phase stored, before the sink's mask) are held to the budget of tests/fp64_budget.py at its
    defaults — MARGIN times the fp32 composition's own error plus 8 ulps of the tensor's scale.  No element is excluded."""
    rg, tr = _rollout("ippo", n_envs, monkeypatch, _Tape(n_envs), **over)
    assert bool(rg.model.args.layernorm) == over.get("layernorm", True)
    assert bool(rg.model.args.agent_id) == over.get("agent_id", True)
    for t in range(steps):
        obs = rg.obs.clone()
        rg.body()
        rg.buf.stepped()
        torch.cuda.synchronize()
        (m64, h64), (m32, h32) = _references(rg, obs)
        name = f"mlp-burst {n_envs}x{tr.env.n_agents} {over or ''} step {t}"
        assert float(h64.abs().max()) > 0 and float(m64.abs().max()) > 0
        fb.within_budget(rg.hid_buf, h32, h64, name=name + " h")
        fb.within_budget(rg.means_buf, m32, m64, name=name + " means")


def _one_step(n_envs, gaussian, monkeypatch):
    tape = _Tape(n_envs)
    rg, tr = _rollout("ippo", n_envs, monkeypatch, tape, gaussian)
    rg.body(burst=1)
    rg.buf.stepped()
    torch.cuda.synchronize()
    return rg, tr, tape


def _shared_step(gaussian):
    mp = pytest.MonkeyPatch()                     # (the switches and the tape are read while the step runs: undone right after)
    try:
        return _one_step(531, gaussian, mp)
    finally:
        mp.undo()


@pytest.fixture(scope="module")
def one_step():
    """One one-step burst of the fixed-std form from the reset state at 531 x 3, shared read-only."""
    return _shared_step(False)


@pytest.fixture(scope="module")
def one_step_gauss():
    """The same of the Gaussian form, shared (read-only) by the head and the selection tests."""
    return _shared_step(True)


def test_heads_do_not_disturb_each_other(one_step_gauss, monkeypatch):
    """The Gaussian form against the fixed-std form of the same entry point on the same first two layers with `mean` as the
    head (a constant std in place of the log-std head): the same means and the same h, bit for bit — the added columns of the
    head's image touch no other column's accumulator; log_stds against the head evaluated in fp64 on the launch's own h, within
    tests/test_gauss_burst_gpu.py's bound for it: max|kernel - fp64| <= 4 max|torch fp32 - fp64| + 4 * 2^-24 max|fp64|."""
    from safe_marl_amd.nets import gauss_log_std_torch, mlp_burst_actor_args
    rg, tr, tape = one_step_gauss
    n_envs = tr.env.n_envs
    rh, th_ = _rollout("ippo", n_envs, monkeypatch, gaussian=True)
    for p, q in zip(rh.model.policy_dicts.parameters(), rg.model.policy_dicts.parameters()):
        assert torch.equal(p, q)
    m, buf = rh.model, rh.buf
    agent = m.policy_dicts[0]
    eps = tape.tape[0:1].contiguous()
    args, mlp = mlp_burst_actor_args(agent, n_envs, m.n_, m.obs_dim, m.args.agent_id, ring_cursor=buf.cursor,
                                     cursor_out=buf.cursor[1:], obs_source=rh.obs_src, ring_slabs=buf.slabs,
                                     hidden_out=rh.hid_buf, means=rh.means_buf)
    assert args.fc2_w == agent.mean.weight.data_ptr()
    args.action, args.env_action = rh.act_buf.data_ptr(), rh.env_act_buf.data_ptr()
    th_.env.rollout_burst_summed_mlp(args, mlp, 1, buf.row_ring, eps, m.args.action_low, m.args.action_high,
                                     std=torch.ones(4, device="cuda"))
    torch.cuda.synchronize()
    assert float(rg.means_buf.abs().max().item()) > 0 and float(rg.hid_buf.abs().max().item()) > 0
    assert torch.equal(rg.means_buf, rh.means_buf)
    assert torch.equal(rg.hid_buf, rh.hid_buf)
    assert rh.buf.cursor.tolist() == rg.buf.cursor.tolist() == [1, 0]
    # the log-std head
    agent = rg.model.policy_dicts[0]
    lo, hi = agent.args.LOG_STD_MIN, agent.args.LOG_STD_MAX
    h = rg.hid_buf.detach()
    w, b = agent.log_std.weight.detach(), agent.log_std.bias.detach()
    f32 = gauss_log_std_torch(h, w, b, lo, hi).double()
    f64 = gauss_log_std_torch(h.double(), w.double(), b.double(), lo, hi)
    got = rg.log_stds_buf.double()
    assert got.shape == f64.shape == (n_envs * tr.env.n_agents, 4)
    err, own = (got - f64).abs().max().item(), (f32 - f64).abs().max().item()
    bound = 4.0 * own + 4.0 * 2.0 ** -24 * f64.abs().max().item()
    print(f"log_stds: kernel error {err:.3e}, fp32 composition error {own:.3e}, bound {bound:.3e}")
    assert float(rg.log_stds_buf.std().item()) > 0.01
    assert float(rg.log_stds_buf.min().item()) >= lo and float(rg.log_stds_buf.max().item()) <= hi
    assert err <= bound, (err, own, bound)


@pytest.mark.parametrize("form", ["one_step", "one_step_gauss"])
def test_selection_is_the_stand_alone_kernels(form, request):
    """flexnet_agent_sum_explore (fixed std) / flexnet_gauss_sum_explore (Gaussian) on the launch's own means (and log-stds) and
    that step's draws: the action the sink filed, the action buffer and the environment's action agree with it bit for bit, and
    every agent of an environment got the one action."""
    from safe_marl_amd import _lib
    rg, tr, tape = request.getfixturevalue(form)
    assert rg.gaussian == (form == "one_step_gauss")
    N, n = tr.env.n_envs, tr.env.n_agents
    m = rg.model
    eps = tape.tape[0].contiguous()
    action, env_action = torch.empty(N, n, 4, device="cuda"), torch.empty(N, n, 4, device="cuda")
    if rg.gaussian:
        k = _lib.FlexGaussSumArgs()
        k.log_stds = rg.log_stds_buf.data_ptr()
    else:
        k = _lib.FlexAgentSumArgs()
        std = m.summed_std(eps.device)
        k.std = std.data_ptr()
    k.n_envs, k.n_agents, k.act_dim = N, n, 4
    k.act_low, k.act_high = float(m.args.action_low), float(m.args.action_high)
    k.means, k.eps = rg.means_buf.data_ptr(), eps.data_ptr()
    k.action, k.env_action = action.data_ptr(), env_action.data_ptr()
    _lib.launch("flexnet_gauss_sum_explore" if rg.gaussian else "flexnet_agent_sum_explore", k)
    torch.cuda.synchronize()
    assert torch.equal(rg.act_buf.view(N, n, 4), action)
    assert torch.equal(rg.env_act_buf.view(N, n, 4), env_action)
    assert torch.equal(rg.buf.small_ring[0, :, :4 * n].reshape(N, n, 4), action)
    assert torch.equal(action, action[:, :1].expand(N, n, 4))
    assert float(action.std().item()) > 0.01 and float(action.abs().max().item()) <= 1.0


@pytest.mark.parametrize("n_envs", [77, 531])
def test_environment_matches_a_twin_stepped_launch_by_launch(n_envs, monkeypatch):
    """A twin env reset with the same spec and stepped one flexenv_step launch at a time on translate_action of the actions the
    burst filed in small_ring reproduces the burst's row records, rewards and dones bit for bit over 30 steps."""
    from safe_marl_amd.util import scale_action
    steps = 30
    rg, tr = _rollout("ippo", n_envs, monkeypatch, _Tape(n_envs))
    rg.body(burst=steps)
    for _ in range(steps):
        rg.buf.stepped()
    torch.cuda.synchronize()
    n, buf, m = tr.env.n_agents, rg.buf, rg.model
    twin = _env(n_envs, SHAPES[n_envs])
    twin.reset(spec=_spec(n_envs, n))
    ring = torch.zeros(steps + 1, n_envs, n * buf.ROW_W, device="cuda")
    cursor = torch.zeros(2, dtype=torch.int64, device="cuda")
    twin.set_obs_ring(cursor, n_envs * n * buf.ROW_W, steps + 1)
    for t in range(steps):
        small = buf.small_ring[t]
        action = small[:, :4 * n].reshape(n_envs, n, 4)
        env_action = scale_action(m.args, action).to(torch.float32).contiguous()      # translate_action, on the device
        twin.step(env_action, auto_reset=True, obs_ring=ring)
        cursor += 1
        assert torch.equal(small[:, 4 * n:5 * n], twin.reward.to(torch.float32)[:, None].expand(n_envs, n)), t
        assert torch.equal(small[:, 5 * n], twin.done.to(torch.float32)), t
    torch.cuda.synchronize()
    assert torch.equal(buf.row_ring[1:steps + 1], ring[1:steps + 1])
    assert torch.equal(tr.env.reward, twin.reward) and torch.equal(tr.env.done, twin.done)
    assert torch.equal(tr.env.obs_view().clone(), twin.obs_view().clone())
    assert float(ring[1:].abs().sum().item()) > 0


def test_mlp_burst_as_replayed_graphs(monkeypatch):
    """capture(lengths=[40]) records one graph of one burst launch; its body launches the new kernel and none of the stand-alone
    policy, selection or step launches; two replays walk ring and cursor cells by 80 steps with fresh draws each."""
    from safe_marl_amd.learner import RolloutGraph
    from safe_marl_amd.util import audit_graph_body
    monkeypatch.delenv("FLEX_MLP_BURST", raising=False)
    tr = _trainer("ippo", 64)
    rg = RolloutGraph(tr.behaviour_net, tr.env, tr.replay_buffer)
    assert rg.mlp_burst and rg.fused_burst
    rg.start_episode(tr.env.reset())
    monkeypatch.setenv("FLEX_GRAPH_AUDIT", "1")
    rg.capture(lengths=[40])
    monkeypatch.delenv("FLEX_GRAPH_AUDIT")
    assert sorted(k for k, _ in rg.bursts) == [40] and all(fused for _, fused in rg.bursts)
    assert rg.burst_chunks(40) == [40] and rg.burst_chunks(1) == [1]
    cursor0 = rg.buf.cursor.clone()
    audit = audit_graph_body(lambda: rg.body(burst=40))
    rg.buf.cursor.copy_(cursor0)
    assert len([k for k in audit if "summed_mlp" in k and "flex_rollout_burst_kernel" in k]) == 1, audit
    assert not any(s in k for k in audit for s in ("sum_explore", "flex_step_kernel", "gauss_head", "actor_r16", "actor_mlp",
                                                   "rollout_pack")), audit
    rg.start_episode(tr.env.reset())
    assert rg.buf.k == 0
    calls = tr.env.calls
    acts = []
    for _ in range(2):
        rg.run(40)
        torch.cuda.synchronize()
        acts.append(rg.act_buf.clone())
    slabs = rg.buf.slabs
    assert rg.buf.k == 80
    assert rg.buf.cursor.tolist() == [80 % slabs, 79 % slabs]
    assert not torch.equal(acts[0], acts[1])
    assert all(float(x.abs().max().item()) <= 1.0 for x in acts)
    for t in (rg.act_buf, rg.hid_buf, rg.acc, rg.means_buf, rg.env_act_buf, rg.buf.small_ring, rg.buf.hid_ring,
              rg.buf.row_ring, tr.env.reward, tr.env.info):
        assert torch.isfinite(t).all()
    assert tr.env.calls == calls
    rg.step()                                                     # the one-step graph: the same launch with one step
    torch.cuda.synchronize()
    assert rg.buf.k == 81 and rg.buf.cursor.tolist() == [81 % slabs, 80 % slabs]


def test_entry_refuses_what_it_cannot_run(monkeypatch):
    """flexenv_rollout_burst_summed_mlp's argument checks on a live handle: a burst as long as the ring, the plain burst's sink
    (aux_counter set), an env without the sink — FLEX_EINVAL, nothing launched, the cursor cells untouched; then a burst runs."""
    from safe_marl_amd import _lib
    from safe_marl_amd.learner import RolloutGraph
    monkeypatch.delenv("FLEX_MLP_BURST", raising=False)
    tr = _trainer("ippo", 64)
    env = tr.env
    rg = RolloutGraph(tr.behaviour_net, env, tr.replay_buffer)
    assert rg.mlp_burst
    rg.start_episode(env.reset())
    rg.body(burst=5)
    for _ in range(5):
        rg.buf.stepped()
    torch.cuda.synchronize()
    cursor, calls, buf = rg.buf.cursor.clone(), env.calls, rg.buf
    refuse = pytest.raises(_lib.FlexLibraryError, match="rollout_burst_summed_mlp failed with code -22")
    with refuse:
        rg.body(burst=buf.slabs)                                  # steps >= slabs
    env.set_replay_sink(rg.act_buf, rg.hid_buf, buf.small_ring, buf.hid_ring, rg.acc, cursor_out=buf.cursor[0:1],
                        aux_counter=rg.rng_state[1:2])            # the plain burst's sink: the in-kernel noise stream's counter
    with refuse:
        rg.body(burst=4)
    env.set_replay_sink(None, None, None, None, None)             # sink off
    with refuse:
        rg.body(burst=4)
    env.calls = calls
    rg._configure_env()                                           # the sink back on: the next burst runs
    torch.cuda.synchronize()
    assert torch.equal(rg.buf.cursor, cursor) and int(rg.rng_state[1].item()) == 0
    rg.body(burst=6)
    for _ in range(6):
        rg.buf.stepped()
    torch.cuda.synchronize()
    assert rg.buf.k == 11 and rg.buf.cursor.tolist() == [11 % buf.slabs, 10 % buf.slabs]


@pytest.mark.parametrize("alg", ["ippo", "matd3"])
def test_training_rolls_out_through_the_burst(alg, monkeypatch):
    """Two train_process calls at 64 envs.  By default: no "capture failed" warning, the trainer keeps its graph rollout, the
    rollout notes no actor_forward fall-back, losses and gradient norms are finite and the policy's weights move.  With
    FLEX_MLP_BURST=0: the warning and the eager loop, as before the burst existed."""
    from safe_marl_amd.util import FALLBACKS
    for flag in ("1", "0"):
        monkeypatch.setenv("FLEX_MLP_BURST", flag)
        tr = _trainer(alg, 64, behaviour_update_freq=7, target_update_freq=11, replay_warmup=0, batch_size=4,
                      value_update_epochs=2, policy_update_epochs=1)
        m = tr.behaviour_net
        w0 = {k: v.detach().clone() for k, v in m.policy_dicts.state_dict().items()}
        before = dict(FALLBACKS)
        stat = {}
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            for _ in range(2):
                m.train_process(stat, tr)
        torch.cuda.synchronize()
        failed = any("rollout graph capture failed" in str(x.message) for x in w)
        assert tr.steps == 190
        assert all(torch.isfinite(p).all() for p in m.parameters())
        if flag == "1":
            assert not failed, [str(x.message) for x in w]
            assert tr.graph_rollout
            rg = m._rollout_graph
            assert rg.mlp_burst and rg.fused_burst and rg.sink_active
            assert rg.bursts and all(fused for _, fused in rg.bursts) and rg.buf.k == 190
            assert FALLBACKS.get("actor_forward", 0) == before.get("actor_forward", 0), (dict(FALLBACKS), before)
            seen = {k: float(v) for k, v in stat.items() if "loss" in k or "grad_norm" in k}
            assert any("loss" in k for k in seen) and any("grad_norm" in k for k in seen), sorted(stat)
            assert all(np.isfinite(v) for v in seen.values()), seen
            assert all(not torch.equal(v, w0[k]) for k, v in m.policy_dicts.state_dict().items())
        else:
            assert failed and tr.graph_rollout is False and not tr.replay_buffer.slab_mode


def test_gaussian_form_is_opt_in(monkeypatch):
    from safe_marl_amd.learner import RolloutGraph
    monkeypatch.delenv("FLEX_GAUSS_BURST", raising=False)
    monkeypatch.delenv("FLEX_MLP_BURST", raising=False)
    tr = _trainer("ippo", 64, gaussian=True)
    rg = RolloutGraph(tr.behaviour_net, tr.env, tr.replay_buffer)
    assert rg.summed and rg.gaussian
    assert not rg.mlp_burst and not rg.sink_active and not rg.fused_burst and not rg.ring_active
