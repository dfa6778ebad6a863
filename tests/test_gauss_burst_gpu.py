"""flexenv_rollout_burst_summed_gauss: the rollout of the agent-summed algorithms with a shared Gaussian actor (gaussian_policy:
True, FLEX_GAUSS_BURST=1) as ONE persistent launch per run of steps — policy with the mean and the log-std head, per-sample
agent-summed selection, environment step with the replay sink.  k steps against k one-step launches bit for bit; the mean /
GRU path against the constant-std burst; the log-std head against fp64; the selection against flexnet_gauss_sum_explore; the
environment against a twin stepped launch by launch; replayed graphs; refusals; training; and the switch's default."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAPE_STEPS = 123
BURSTS = (40, 23, 60)                         # (every episode ends at step 96: the restarts fall inside the third burst)


def _env(n_envs, buildings=None, device="cuda:0"):
    from safe_marl_amd.flex_env import VecFlexProvisionEnv
    from safe_marl_amd.network import create_network
    from safe_marl_amd.series import make_synthetic_series
    env_args = {} if buildings is None else {"buildings": buildings, "pv_nodes": buildings, "ess_nodes": buildings}
    net = create_network(env_args)
    series = make_synthetic_series(net, n_days=30)
    return VecFlexProvisionEnv(env_args, n_envs, device=device, net=net, series=series, seed=9, warm_start=True)


def _trainer(alg, n_envs, buildings=None, device="cuda:0", **over):
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    from train_maddpg import DEFAULT_ALG_ARGS, PPO_ALG_ARGS
    from safe_marl_amd import learner
    from safe_marl_amd.trainer import PGTrainer
    from safe_marl_amd.util import convert
    env = _env(n_envs, buildings, device)
    a = dict(DEFAULT_ALG_ARGS)
    if alg == "ippo":
        a.update(PPO_ALG_ARGS)
    a.update(alg=alg, agent_num=env.n_agents, obs_size=env.obs_size, state_size=env.state_size, action_dim=4,
             behaviour_update_freq=30, batch_size=4, gaussian_policy=True)
    a.update(over)
    torch.manual_seed(3)
    np.random.seed(3)
    cls = {"matd3": learner.MATD3, "iddpg": learner.IDDPG, "ippo": learner.IPPO}[alg]
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


def _rollout(alg, n_envs, buildings, monkeypatch, tape=None):
    """A Gaussian trainer with the switch on, the policy's parameters times ten (both heads matter), reset to _spec."""
    import torch.distributions.normal as tdn
    from safe_marl_amd.learner import RolloutGraph
    monkeypatch.setenv("FLEX_GAUSS_BURST", "1")
    if tape is not None:
        monkeypatch.setattr(tdn, "_standard_normal", tape)
    tr = _trainer(alg, n_envs, buildings)
    m = tr.behaviour_net
    with torch.no_grad():
        for p in m.policy_dicts.parameters():
            p.mul_(10.0)
    rg = RolloutGraph(m, tr.env, tr.replay_buffer)
    assert rg.summed and rg.gaussian and rg.gauss_burst and not rg.summed_sink and not rg.summed_burst and not rg.fast
    assert rg.sink_active and rg.ring_active and rg.fused_burst and rg.buf.row_mode
    rg.start_episode(tr.env.reset(spec=_spec(n_envs, tr.env.n_agents)))
    if tape is not None:
        tape.pos = tape.calls = 0
    return rg, tr


@pytest.mark.parametrize("alg,n_envs,buildings", [("ippo", 531, [3, 17, 28]), ("ippo", 77, [5]), ("ippo", 203, [3, 9, 17, 28]),
                                                  ("ippo", 4100, None), ("matd3", 531, [3, 17, 28])])
def test_k_steps_equal_k_one_step_launches_bit_for_bit(alg, n_envs, buildings, monkeypatch):
    """Eager body(burst=k) for k = 40, 23, 60 against 123 body() calls of a second trainer — the same launch with one step — on
    one noise tape: a batch that is not a multiple of a block's sixteen environments (tail block, empty second group), more
    blocks than CUs (4100 -> 257), one / three / four / five agents (partly filled policy tiles), the episodes' restart inside
    the last burst.  Every ring, cursor, statistic and the environments' own state: identical bits."""
    tape = _Tape(n_envs)
    runs = []
    for bursts in (BURSTS, (0,) * TAPE_STEPS):
        rg, tr = _rollout(alg, n_envs, buildings, monkeypatch, tape)
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
    for name in ("acc", "act_buf", "hid_buf", "means_buf", "log_stds_buf", "env_act_buf"):
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    for name in ("reward", "done", "info", "failed"):
        assert torch.equal(getattr(ta.env, name), getattr(tb.env, name)), name
    assert torch.equal(ta.env.obs_view().clone(), tb.env.obs_view().clone())
    assert float(a.acc[:, 7].abs().sum().item()) > 0
    assert float(a.log_stds_buf.std().item()) > 0.01
    assert torch.isfinite(a.buf.small_ring).all() and torch.isfinite(a.hid_buf).all()
    # the ONE action of an environment in every agent's row
    act = a.act_buf.view(n_envs, na, 4)
    assert torch.equal(act, act[:, :1].expand(n_envs, na, 4))


def _one_step(n_envs, buildings, monkeypatch):
    tape = _Tape(n_envs)
    rg, tr = _rollout("ippo", n_envs, buildings, monkeypatch, tape)
    rg.body(burst=1)
    rg.buf.stepped()
    torch.cuda.synchronize()
    return rg, tr, tape


@pytest.fixture(scope="module")
def one_step():
    """One one-step burst from the reset state at 531 x 3, shared (read-only) by the head and the selection tests."""
    mp = pytest.MonkeyPatch()                     # (the switch and the tape are read while the step runs: undone right after)
    try:
        return _one_step(531, [3, 17, 28], mp)
    finally:
        mp.undo()


def test_mean_and_gru_path_is_the_constant_std_forms(one_step, monkeypatch):
    """From the same reset state and the same parameters: one step of flexenv_rollout_burst_summed on the very actor (its `mean`
    head as fc2, a constant std in place of the log-std head) leaves the same means and the same new hidden state, bit for
    bit — the added columns of the fc2 image touch no other column's accumulator."""
    from safe_marl_amd.nets import fused_actor_forward
    rg, tr, tape = one_step
    n_envs = tr.env.n_envs
    rh, th_ = _rollout("ippo", n_envs, [3, 17, 28], monkeypatch)
    for p, q in zip(rh.model.policy_dicts.parameters(), rg.model.policy_dicts.parameters()):
        assert torch.equal(p, q)
    m, buf, N = rh.model, rh.buf, n_envs
    eps = tape.tape[0:1].contiguous()
    std = torch.ones(4, device="cuda")

    def launch(args):
        args.action, args.env_action = rh.act_buf.data_ptr(), rh.env_act_buf.data_ptr()
        th_.env.rollout_burst_summed(args, 1, buf.row_ring, eps, std, m.args.action_low, m.args.action_high)

    with torch.no_grad():
        out = fused_actor_forward(m.policy_dicts[0], rh._obs, buf.hid_ring[0].view(N, m.n_, m.hid_dim), m.n_, m.args.agent_id,
                                  ring_cursor=buf.cursor, obs_slab_stride=0, obs_source=rh.obs_src,
                                  hid_slab_stride=buf.hid_ring.stride(0), cursor_out=buf.cursor[1:],
                                  out=dict(hidden_out=rh.hid_buf, means=rh.means_buf), ring_slabs=buf.slabs, launch=launch)
    assert out is not None
    torch.cuda.synchronize()
    assert float(rg.means_buf.abs().max().item()) > 0 and float(rg.hid_buf.abs().max().item()) > 0
    assert torch.equal(rg.means_buf, rh.means_buf)
    assert torch.equal(rg.hid_buf, rh.hid_buf)
    assert rh.buf.cursor.tolist() == rg.buf.cursor.tolist() == [1, 0]


def test_log_std_head_against_fp64(one_step):
    """log_stds of the launch against the head evaluated in fp64 on the fp32 hidden state the launch wrote, within the bound
    of tests/test_gauss_head_gpu.py for this computation: max|kernel - fp64| <= 4 max|torch fp32 - fp64| + 4 * 2^-24 max|fp64|."""
    from safe_marl_amd.nets import gauss_log_std_torch
    rg, tr, _ = one_step
    agent = rg.model.policy_dicts[0]
    lo, hi = agent.args.LOG_STD_MIN, agent.args.LOG_STD_MAX
    h = rg.hid_buf.detach()
    w, b = agent.log_std.weight.detach(), agent.log_std.bias.detach()
    f32 = gauss_log_std_torch(h, w, b, lo, hi).double()
    f64 = gauss_log_std_torch(h.double(), w.double(), b.double(), lo, hi)
    got = rg.log_stds_buf.double()
    assert got.shape == f64.shape == (tr.env.n_envs * tr.env.n_agents, 4)
    err, own = (got - f64).abs().max().item(), (f32 - f64).abs().max().item()
    bound = 4.0 * own + 4.0 * 2.0 ** -24 * f64.abs().max().item()
    print(f"log_stds: kernel error {err:.3e}, fp32 composition error {own:.3e}, bound {bound:.3e}")
    assert float(rg.log_stds_buf.std().item()) > 0.01
    assert float(rg.log_stds_buf.min().item()) >= lo and float(rg.log_stds_buf.max().item()) <= hi
    assert err <= bound, (err, own, bound)


def test_selection_is_gauss_sum_explore(one_step):
    """flexnet_gauss_sum_explore on the launch's own means, log-stds and that step's draws: the action the sink filed, the
    action buffer and the environment's action agree with it bit for bit, and every agent of an environment got the one action."""
    from safe_marl_amd import _lib
    rg, tr, tape = one_step
    N, n = tr.env.n_envs, tr.env.n_agents
    m = rg.model
    eps = tape.tape[0].contiguous()
    action, env_action = torch.empty(N, n, 4, device="cuda"), torch.empty(N, n, 4, device="cuda")
    k = _lib.FlexGaussSumArgs()
    k.n_envs, k.n_agents, k.act_dim = N, n, 4
    k.act_low, k.act_high = float(m.args.action_low), float(m.args.action_high)
    k.means, k.log_stds, k.eps = rg.means_buf.data_ptr(), rg.log_stds_buf.data_ptr(), eps.data_ptr()
    k.action, k.env_action = action.data_ptr(), env_action.data_ptr()
    _lib.launch("flexnet_gauss_sum_explore", k)
    torch.cuda.synchronize()
    assert torch.equal(rg.act_buf.view(N, n, 4), action)
    assert torch.equal(rg.env_act_buf.view(N, n, 4), env_action)
    assert torch.equal(rg.buf.small_ring[0, :, :4 * n].reshape(N, n, 4), action)
    assert torch.equal(action, action[:, :1].expand(N, n, 4))
    assert float(action.std().item()) > 0.01 and float(action.abs().max().item()) <= 1.0


@pytest.mark.parametrize("n_envs,buildings", [(77, [5]), (531, [3, 17, 28])])
def test_environment_matches_a_twin_stepped_launch_by_launch(n_envs, buildings, monkeypatch):
    """A twin env reset with the same spec and stepped one flexenv_step launch at a time on translate_action of the actions the
    burst filed in small_ring reproduces the burst's row records, rewards and dones bit for bit over 30 steps."""
    from safe_marl_amd.util import scale_action
    steps = 30
    rg, tr = _rollout("ippo", n_envs, buildings, monkeypatch, _Tape(n_envs))
    rg.body(burst=steps)
    for _ in range(steps):
        rg.buf.stepped()
    torch.cuda.synchronize()
    n, buf, m = tr.env.n_agents, rg.buf, rg.model
    twin = _env(n_envs, buildings)
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


def test_gauss_burst_as_replayed_graphs(monkeypatch):
    """capture(lengths=[40]) records one graph of one burst launch; its body launches the burst kernel and neither the
    stand-alone head, selection nor step; two replays walk ring and cursor cells by 80 steps with fresh draws each."""
    from safe_marl_amd.learner import RolloutGraph
    from safe_marl_amd.util import audit_graph_body
    monkeypatch.setenv("FLEX_GAUSS_BURST", "1")
    tr = _trainer("ippo", 64)
    rg = RolloutGraph(tr.behaviour_net, tr.env, tr.replay_buffer)
    assert rg.gauss_burst and rg.fused_burst
    rg.start_episode(tr.env.reset())
    monkeypatch.setenv("FLEX_GRAPH_AUDIT", "1")
    rg.capture(lengths=[40])
    monkeypatch.delenv("FLEX_GRAPH_AUDIT")
    assert sorted(k for k, _ in rg.bursts) == [40] and all(fused for _, fused in rg.bursts)
    assert rg.burst_chunks(40) == [40] and rg.burst_chunks(1) == [1]
    cursor0 = rg.buf.cursor.clone()
    audit = audit_graph_body(lambda: rg.body(burst=40))
    rg.buf.cursor.copy_(cursor0)
    assert len([k for k in audit if "summed_gauss" in k and "flex_rollout_burst_kernel" in k]) == 1, audit
    assert not any(s in k for k in audit for s in ("sum_explore", "flex_step_kernel", "gauss_head", "actor_r16", "rollout_pack")), audit
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
    for t in (rg.act_buf, rg.hid_buf, rg.acc, rg.means_buf, rg.log_stds_buf, rg.env_act_buf, rg.buf.small_ring, rg.buf.hid_ring,
              rg.buf.row_ring, tr.env.reward, tr.env.info):
        assert torch.isfinite(t).all()
    assert tr.env.calls == calls
    rg.step()                                                     # the one-step graph: the same launch with one step
    torch.cuda.synchronize()
    assert rg.buf.k == 81 and rg.buf.cursor.tolist() == [81 % slabs, 80 % slabs]


def test_entry_refuses_what_it_cannot_run(monkeypatch):
    """flexenv_rollout_burst_summed_gauss's argument checks on a live handle: a burst as long as the ring, the plain burst's sink
    (aux_counter set), an env without the sink — FLEX_EINVAL, nothing launched, the cursor cells untouched; then a burst runs."""
    from safe_marl_amd import _lib
    from safe_marl_amd.learner import RolloutGraph
    monkeypatch.setenv("FLEX_GAUSS_BURST", "1")
    tr = _trainer("ippo", 64)
    env = tr.env
    rg = RolloutGraph(tr.behaviour_net, env, tr.replay_buffer)
    assert rg.gauss_burst
    rg.start_episode(env.reset())
    rg.body(burst=5)
    for _ in range(5):
        rg.buf.stepped()
    torch.cuda.synchronize()
    cursor, calls, buf = rg.buf.cursor.clone(), env.calls, rg.buf
    refuse = pytest.raises(_lib.FlexLibraryError, match="flexenv_rollout_burst_summed_gauss failed with code -22")
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
def test_training_with_the_switch_on(alg, monkeypatch):
    """Two train_process calls with the switch on and off, update events every 7 steps and target updates every 11: the
    same events at the same steps; with the switch on the rollout is the burst, losses and gradient norms are finite, the
    log-std head's weights move and nothing fell back."""
    from safe_marl_amd.util import FALLBACKS
    res = []
    for flag in ("1", "0"):
        monkeypatch.setenv("FLEX_GAUSS_BURST", flag)
        tr = _trainer(alg, 64, behaviour_update_freq=7, target_update_freq=11, replay_warmup=0, batch_size=4,
                      value_update_epochs=2, policy_update_epochs=1)
        m = tr.behaviour_net
        w0 = m.policy_dicts[0].log_std.weight.detach().clone()
        before = dict(FALLBACKS)
        stat, events = {}, []
        update = type(m).transition_update
        monkeypatch.setattr(type(m), "transition_update",
                            lambda self, trainer, trans, st: (events.append(trainer.steps), update(self, trainer, trans, st))[1])
        for _ in range(2):
            m.train_process(stat, tr)
        monkeypatch.setattr(type(m), "transition_update", update)
        torch.cuda.synchronize()
        rg = m._rollout_graph
        assert rg.gauss_burst == rg.fused_burst == rg.sink_active == (flag == "1")
        assert rg.bursts and all(fused == (flag == "1") for _, fused in rg.bursts)
        if flag == "1":
            assert dict(FALLBACKS) == before, (dict(FALLBACKS), before)
            seen = {k: float(v) for k, v in stat.items() if "loss" in k or "grad_norm" in k}
            assert any("loss" in k for k in seen) and any("grad_norm" in k for k in seen), sorted(stat)
            assert all(np.isfinite(v) for v in seen.values()), seen
            assert not torch.equal(m.policy_dicts[0].log_std.weight.detach(), w0)
        assert all(torch.isfinite(p).all() for p in m.parameters())
        res.append((tr.steps, tr.episodes, rg.buf.k, events))        # (the ring's size differs between the forms: no cursor)
    assert res[0] == res[1] and res[0][0] == 190 and len(res[0][3]) > 0


def test_switch_is_off_by_default(monkeypatch):
    from safe_marl_amd.learner import RolloutGraph
    monkeypatch.delenv("FLEX_GAUSS_BURST", raising=False)
    tr = _trainer("ippo", 64)
    rg = RolloutGraph(tr.behaviour_net, tr.env, tr.replay_buffer)
    assert rg.summed and rg.gaussian
    assert not rg.gauss_burst and not rg.sink_active and not rg.fused_burst and not rg.ring_active
