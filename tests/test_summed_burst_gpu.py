"""flexenv_rollout_burst_summed: the rollout of the agent-summed algorithms (MATD3, IDDPG, IPPO, ...) as ONE persistent launch
per run of steps — policy, agent-summed action selection, environment step with the replay sink — against the three launches
per step it replaces (FLEX_SUMMED_BURST=0), bit for bit on the same draws; as replayed graphs; its refusals; and inside the
training loop."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAPE_STEPS = 123
BURSTS = (40, 23, 60)                         # (every episode ends at step 96: the restarts fall inside the third burst)


def _trainer(alg, n_envs, buildings=None, device="cuda:0", **over):
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    from train_maddpg import DEFAULT_ALG_ARGS, PPO_ALG_ARGS
    from safe_marl_amd import learner
    from safe_marl_amd.flex_env import VecFlexProvisionEnv
    from safe_marl_amd.network import create_network
    from safe_marl_amd.series import make_synthetic_series
    from safe_marl_amd.trainer import PGTrainer
    from safe_marl_amd.util import convert
    env_args = {} if buildings is None else {"buildings": buildings, "pv_nodes": buildings, "ess_nodes": buildings}
    net = create_network(env_args)
    series = make_synthetic_series(net, n_days=30)
    env = VecFlexProvisionEnv(env_args, n_envs, device=device, net=net, series=series, seed=9, warm_start=True)
    a = dict(DEFAULT_ALG_ARGS)
    if alg == "ippo":
        a.update(PPO_ALG_ARGS)
    a.update(alg=alg, agent_num=env.n_agents, obs_size=env.obs_size, state_size=env.state_size, action_dim=4,
             behaviour_update_freq=30, batch_size=4)
    a.update(over)
    torch.manual_seed(3)
    np.random.seed(3)
    cls = {"matd3": learner.MATD3, "iddpg": learner.IDDPG, "ippo": learner.IPPO}[alg]
    return PGTrainer(convert(a), cls, env, None, replay_capacity=n_envs * 96 * 2)


class _Tape:
    """torch.distributions.normal._standard_normal served from a fixed tape [123, N, 1, 4]: a burst's one draw of k steps
    (shape (k, N, 1, 4)) gets rows pos .. pos + k - 1, a single step's draw (shape (N, 1, 4)) row pos; either way pos advances.
    Every other shape goes to the real function."""

    def __init__(self, n_envs):
        import torch.distributions.normal as tdn
        self.real = tdn._standard_normal
        g = torch.Generator(device="cuda").manual_seed(11)
        self.tape = torch.randn(TAPE_STEPS, n_envs, 1, 4, device="cuda", generator=g)
        self.n_envs, self.pos = n_envs, 0

    def __call__(self, shape, dtype, device):
        shape = tuple(shape)
        if shape == (self.n_envs, 1, 4):
            out = self.tape[self.pos]
            self.pos += 1
            return out
        if len(shape) == 4 and shape[1:] == (self.n_envs, 1, 4):
            out = self.tape[self.pos:self.pos + shape[0]]
            assert out.shape[0] == shape[0]
            self.pos += shape[0]
            return out
        return self.real(shape, dtype, device)


@pytest.mark.parametrize("alg,n_envs,buildings", [("matd3", 4100, None), ("matd3", 531, [3, 17, 28]), ("matd3", 77, [5]),
                                                  ("matd3", 203, [3, 9, 17, 28]), ("iddpg", 531, [3, 17, 28]),
                                                  ("ippo", 531, [3, 17, 28])])
def test_summed_burst_equals_three_launches_per_step_bit_for_bit(alg, n_envs, buildings, monkeypatch):
    """Eager body(burst=k) for k = 40, 23, 60 against 123 eager three-launch bodies of the same trainer under
    FLEX_SUMMED_BURST=0, both fed from one noise tape: a batch that is not a multiple of a block's sixteen environments (tail
    block, empty second group), more blocks than CUs (4100 -> 257), one / three / four agents (partly filled policy tiles), the
    episodes' restart inside the last burst.  Every ring, cursor, statistic and the environments' own state: identical bits."""
    import torch.distributions.normal as tdn
    from safe_marl_amd import nets
    from safe_marl_amd.learner import RolloutGraph
    # the three-launch side on the 16-row-tile policy kernel whatever the batch (the 32-row kernel groups its LayerNorm sums
    # differently: equal to 2e-6, not to the bit)
    monkeypatch.setattr(nets, "ACTOR_VARIANT", 2)
    tape = _Tape(n_envs)
    monkeypatch.setattr(tdn, "_standard_normal", tape)
    runs = []
    for flag in ("1", "0"):
        monkeypatch.setenv("FLEX_SUMMED_BURST", flag)
        tr = _trainer(alg, n_envs, buildings)
        m = tr.behaviour_net
        with torch.no_grad():
            for p in m.policy_dicts.parameters():
                p.mul_(10.0)
        rg = RolloutGraph(m, tr.env, tr.replay_buffer)
        assert rg.summed and rg.summed_sink and rg.sink_active and not rg.fast
        assert rg.summed_burst == rg.fused_burst == (flag == "1")
        assert max(BURSTS) < rg.buf.slabs
        rng = np.random.default_rng(4)
        na = tr.env.n_agents
        spec = dict(day=rng.integers(0, 20, n_envs).astype(np.int32), hour=rng.integers(0, 24, n_envs).astype(np.int32),
                    interval=rng.integers(0, 4, n_envs).astype(np.int32), e0=0.0125 + 0.001 * rng.random((n_envs, na)),
                    a0=0.5 + 0.5 * rng.random((n_envs, 4 * na)))
        rg.start_episode(tr.env.reset(spec=spec))
        tape.pos = 0
        if flag == "1":
            for k in BURSTS:
                rg.body(burst=k)
                for _ in range(k):
                    rg.buf.stepped()
        else:
            for _ in range(sum(BURSTS)):
                rg.body()
                rg.buf.stepped()
        torch.cuda.synchronize()
        assert tape.pos == TAPE_STEPS == sum(BURSTS)
        runs.append((rg, tr))
    (a, ta), (b, tb) = runs
    assert a.buf.k == b.buf.k == TAPE_STEPS
    assert torch.equal(a.buf.cursor, b.buf.cursor)
    assert a.buf.row_mode and b.buf.row_mode
    for ring in ("row_ring", "hid_ring", "small_ring"):
        assert torch.equal(getattr(a.buf, ring), getattr(b.buf, ring)), ring
    for name in ("acc", "act_buf", "hid_buf"):
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    for name in ("reward", "done", "info", "failed"):
        assert torch.equal(getattr(ta.env, name), getattr(tb.env, name)), name
    assert torch.equal(ta.env.obs_view().clone(), tb.env.obs_view().clone())
    assert float(a.acc[:, 7].abs().sum().item()) > 0
    # the ONE action of an environment in every agent's row
    act = a.act_buf.view(n_envs, na, 4)
    assert torch.equal(act, act[:, :1].expand(n_envs, na, 4))


def test_summed_burst_as_replayed_graphs(monkeypatch):
    """capture(lengths=[40]) records one graph of one burst launch; its body launches the burst kernel and neither the
    stand-alone action selection nor the stand-alone step; two replays walk ring and cursor cells by 80 steps with fresh draws
    each (the generator advances inside the graph)."""
    from safe_marl_amd.learner import RolloutGraph
    from safe_marl_amd.util import audit_graph_body
    monkeypatch.setenv("FLEX_SUMMED_BURST", "1")
    tr = _trainer("matd3", 64)
    rg = RolloutGraph(tr.behaviour_net, tr.env, tr.replay_buffer)
    assert rg.fused_burst and rg.summed_burst
    rg.start_episode(tr.env.reset())
    monkeypatch.setenv("FLEX_GRAPH_AUDIT", "1")
    rg.capture(lengths=[40])
    monkeypatch.delenv("FLEX_GRAPH_AUDIT")
    assert sorted(k for k, _ in rg.bursts) == [40] and all(fused for _, fused in rg.bursts)
    cursor0 = rg.buf.cursor.clone()
    audit = audit_graph_body(lambda: rg.body(burst=40))
    rg.buf.cursor.copy_(cursor0)
    assert any("flex_rollout_burst_kernel" in k for k in audit), audit
    assert not any("agent_sum_explore" in k for k in audit) and not any("flex_step_kernel" in k for k in audit), audit
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
    for t in (rg.act_buf, rg.hid_buf, rg.acc, rg.means_buf, rg.env_act_buf, rg.buf.small_ring, rg.buf.hid_ring, rg.buf.row_ring,
              tr.env.reward, tr.env.info):
        assert torch.isfinite(t).all()
    assert tr.env.calls == calls


def test_summed_burst_entry_refuses_what_it_cannot_run(monkeypatch):
    """flexenv_rollout_burst_summed's argument checks on a live handle (include/flexenv.h): missing draws, missing std, a burst
    as long as the ring, an env without the replay sink, the plain burst's sink (aux_counter set) — FLEX_EINVAL, nothing
    launched, the cursor cells untouched; then a valid burst runs."""
    from safe_marl_amd import _lib
    from safe_marl_amd.learner import RolloutGraph
    monkeypatch.setenv("FLEX_SUMMED_BURST", "1")
    tr = _trainer("matd3", 64)
    env = tr.env
    rg = RolloutGraph(tr.behaviour_net, env, tr.replay_buffer)
    assert rg.fused_burst and rg.summed_burst
    rg.start_episode(env.reset())
    rg.capture()
    rg.run(5)
    torch.cuda.synchronize()
    cursor, calls = rg.buf.cursor.clone(), env.calls
    real = env.rollout_burst_summed
    refuse = pytest.raises(_lib.FlexLibraryError, match="flexenv_rollout_burst_summed failed with code -22")      # FLEX_EINVAL
    with monkeypatch.context() as mp:
        mp.setattr(env, "rollout_burst_summed", lambda args, steps, ring, eps, std, lo, hi: real(args, steps, ring, None, std, lo, hi))
        with refuse:
            rg.body(burst=4)                                      # eps NULL
        mp.setattr(env, "rollout_burst_summed", lambda args, steps, ring, eps, std, lo, hi: real(args, steps, ring, eps, None, lo, hi))
        with refuse:
            rg.body(burst=4)                                      # std NULL
    with refuse:
        rg.body(burst=rg.buf.slabs)                               # steps >= slabs
    env.set_replay_sink(None, None, None, None, None)             # sink off
    with refuse:
        rg.body(burst=4)
    buf = rg.buf
    env.set_replay_sink(rg.act_buf, rg.hid_buf, buf.small_ring, buf.hid_ring, rg.acc, cursor_out=buf.cursor[0:1],
                        aux_counter=rg.rng_state[1:2])            # the plain burst's sink: the in-kernel noise stream's counter
    with refuse:
        rg.body(burst=4)
    env.calls = calls
    rg._configure_env()                                           # the summed sink back on: the next burst runs
    torch.cuda.synchronize()
    assert torch.equal(rg.buf.cursor, cursor)
    before = rg.buf.k
    rg.run(6)
    torch.cuda.synchronize()
    assert rg.buf.k == before + 6
    assert rg.buf.cursor.tolist() == [(before + 6) % buf.slabs, (before + 5) % buf.slabs]


def test_env_on_a_device_without_an_index_runs_the_burst(monkeypatch):
    """An env built with device="cuda" (no index: the constructor takes it as cuda:0) holds tensors on cuda:0, which never
    compare equal to torch.device("cuda"): the burst's tensor checks must take them, as the three-launch form does."""
    from safe_marl_amd.learner import RolloutGraph
    monkeypatch.setenv("FLEX_SUMMED_BURST", "1")
    tr = _trainer("matd3", 64, device="cuda")
    assert tr.env.device.index is None
    rg = RolloutGraph(tr.behaviour_net, tr.env, tr.replay_buffer)
    assert rg.fused_burst and rg.summed_burst
    rg.start_episode(tr.env.reset())
    rg.capture(lengths=[6])
    rg.start_episode(tr.env.reset())
    rg.run(6)
    torch.cuda.synchronize()
    assert rg.buf.k == 6 and rg.buf.cursor.tolist() == [6, 5]
    assert torch.isfinite(rg.act_buf).all() and float(rg.act_buf.abs().max().item()) <= 1.0


def test_training_loop_schedule_is_unchanged_by_summed_bursts(monkeypatch):
    """IDDPG's train_process with the one-launch bursts against three launches per step (FLEX_SUMMED_BURST=0), update events
    every 7 steps and target updates every 11: the same events at the same steps — step and episode counters, ring position —
    with graphs of the form the switch asks for only.  (The draws of a burst come from one call instead of k: the numbers
    differ for one seed, so parameters are not compared bit for bit.)"""
    from safe_marl_amd.learner import RolloutGraph
    res = []
    for flag in ("1", "0"):
        monkeypatch.setenv("FLEX_SUMMED_BURST", flag)
        tr = _trainer("iddpg", 256, behaviour_update_freq=7, target_update_freq=11, replay_warmup=0, batch_size=4,
                      value_update_epochs=2, policy_update_epochs=1)
        init = [p.detach().clone() for p in tr.behaviour_net.parameters()]
        for _ in range(2):
            tr.behaviour_net.train_process({}, tr)
        torch.cuda.synchronize()
        rg = tr.behaviour_net._rollout_graph
        assert rg.summed_sink and rg.fused_burst == (flag == "1")
        assert rg.bursts and all(fused == (flag == "1") for _, fused in rg.bursts)
        if flag == "0":
            assert set(k for k, _ in rg.bursts) <= set(RolloutGraph.BURSTS)
        params = [p.detach().clone() for p in tr.behaviour_net.parameters()]
        assert all(torch.isfinite(p).all() for p in params)
        assert any(not torch.equal(p, q) for p, q in zip(params, init))
        res.append((tr.steps, tr.episodes, rg.buf.k, rg.buf.cursor.tolist()))
    assert res[0] == res[1] and res[0][0] == 190
