"""IPPO / MAPPO (madrl/models/ippo.py, mappo.py with madrl/learning_algorithms/ppo.py) on CPU: golden vectors captured by
importing the reference's own modules (tests/golden/make_ppo_golden.py); the need split; GAE along chains against a float64
evaluation of the reference's literal loop; the on-policy cadence (buffer clear, pooled step-aligned windows, capacity);
the old values filed at the start of an update event against the per-step route; ppo_consistent_ratio; the C ABI; one update event on two gloo ranks."""
import ctypes as C
import os

import numpy as np
import pytest
import torch as th

import safe_marl_amd.learner as L

from .golden_io import StubEnv, _free_port, golden_args, golden_batch, golden_model, golden_tensors, golden_vectors

FIELDS = ("action", "done", "last_step")          # what the reference's PPO runs stored in the batch
CASES = [("ippo", "IPPO"), ("mappo", "MAPPO"), ("ippo3", "IPPO"), ("mappo3", "MAPPO")]


def test_batch_takes_every_branch_of_the_gae_mask():
    gold = golden_vectors("ippo")
    done, last = gold["batch.done"], gold["batch.last_step"]
    assert ((last == 1) & (done == 0)).any() and ((last == 1) & (done == 1)).any() and ((last == 0) & (done == 0)).any()
    b = golden_batch("ippo", gold=gold, fields=FIELDS)
    assert b.value.abs().max() > 0 and b.next_value.abs().max() > 0
    assert all(th.equal(b.action[:, i], b.action[:, 0]) for i in range(5))


@pytest.mark.parametrize("prefix,name", CASES)
def test_golden_parity(prefix, name):
    from safe_marl_amd.trainer import PGTrainer
    gold = golden_vectors(prefix)
    args = golden_args(prefix)
    model = golden_model(name, args, f"{prefix}_state_dict.npz")
    assert "batchnorm.running_mean" in model.state_dict() and not any(k.startswith("rl.") for k in model.state_dict())
    batch = golden_batch(prefix, gold=gold, fields=FIELDS)
    pl, vl, (means, log_stds) = model.get_loss(batch)
    # the tolerances of test_learner_cpu.py / test_sqddpg_cpu.py for the same kinds of quantity
    assert abs(pl.item() - float(gold["policy_loss"])) < 2e-6
    assert abs(vl.item() - float(gold["value_loss"])) < 1e-5 * max(1.0, abs(float(gold["value_loss"])))
    assert np.allclose(means.detach().numpy(), gold["means"], atol=2e-6)
    t = model.last_terms
    assert np.allclose(t["reward_norm"].numpy(), gold["reward_norm"], atol=2e-5)
    for k in ("advantages", "advantages_norm", "returns"):
        assert np.allclose(t[k].numpy(), gold[k], atol=1e-5), k
    assert np.allclose(t["ratios"].numpy(), gold["ratios"], atol=1e-6)
    for name_, bn in (("reward_bn", model.batchnorm), ("adv_bn", model.rl.batchnorm)):
        assert th.allclose(bn.running_mean, th.from_numpy(gold[name_ + ".running_mean"]), atol=1e-6), name_
        assert th.allclose(bn.running_var, th.from_numpy(gold[name_ + ".running_var"]), atol=1e-6, rtol=1e-5), name_
        assert int(bn.num_batches_tracked) == int(gold[name_ + ".num_batches_tracked"]) == 1
    grads = th.autograd.grad(vl, list(model.value_dicts.parameters()), retain_graph=True)
    for (k, _), g in zip(model.value_dicts.named_parameters(), grads):
        ref = gold["vgrad." + k]
        assert np.allclose(g.numpy(), ref, atol=2e-6 + 1e-4 * np.abs(ref).max()), k
    grads = th.autograd.grad(pl, list(model.policy_dicts.parameters()))
    for (k, _), g in zip(model.policy_dicts.named_parameters(), grads):
        ref = gold["pgrad." + k]
        assert np.allclose(g.numpy(), ref, atol=2e-7 + 1e-4 * np.abs(ref).max()), k

    # one value step, then one policy step through PGTrainer; update_target
    th.manual_seed(2468)
    trainer = PGTrainer(args, getattr(L, name), StubEnv(args.agent_num), None)
    net = trainer.behaviour_net
    sd0 = golden_tensors(f"{prefix}_state_dict.npz")
    net.load_state_dict(sd0)
    net.target_net.load_state_dict({k[len("target_net."):]: v for k, v in sd0.items() if k.startswith("target_net.")})
    stat = {}
    trainer.value_transition_process(stat, batch)
    trainer.policy_transition_process(stat, batch)
    keys = {k[5:] for k in gold if k.startswith("stat.")}
    assert keys == set(stat) == {"mean_train_value_loss", "mean_train_value_grad_norm", "mean_train_policy_loss",
                                 "mean_train_policy_grad_norm", "mean_train_entropy"}
    for k in keys:
        assert abs(float(stat[k]) - gold["stat." + k]) < 1e-4 * max(1.0, abs(gold["stat." + k])), k
    after = golden_tensors(f"{prefix}_state_dict_after_step.npz")
    mine = net.state_dict()
    assert sorted(mine) == sorted(after)
    for k, ref in after.items():
        assert th.allclose(mine[k].float(), ref.float(), atol=3e-6, rtol=1e-5), k
    for name_, bn in (("reward_bn", net.batchnorm), ("adv_bn", net.rl.batchnorm)):
        assert th.allclose(bn.running_var, th.from_numpy(gold[f"after_step.{name_}.running_var"]), atol=1e-6, rtol=1e-5)
    net.update_target()
    tgt = golden_tensors(f"{prefix}_target_after_update.npz")
    mine_t = net.target_net.state_dict()
    for k, ref in tgt.items():
        assert th.allclose(mine_t[k].float(), ref.float(), atol=3e-6, rtol=1e-5), k


def test_class_wiring_and_value_shapes():
    import safe_marl_amd
    from safe_marl_amd.learner import IDDPG, IPPO, MADDPG, MAPPO
    assert safe_marl_amd.IPPO is IPPO and safe_marl_amd.MAPPO is MAPPO
    assert IPPO.on_policy and MAPPO.on_policy and not MADDPG.on_policy and not IDDPG.on_policy
    assert IPPO.get_actions is IDDPG.get_actions and IPPO.graph_safe_updates is False
    for prefix, name in CASES[:2]:
        args = golden_args(prefix)
        m = getattr(L, name)(args)
        n, o = args.agent_num, args.obs_size
        assert m.value_dicts[0].fc1.in_features == (o + n if name == "IPPO" else o * n + n)
        noid = getattr(L, name)(golden_args(prefix, agent_id=False))
        assert noid.value_dicts[0].fc1.in_features == (o if name == "IPPO" else o * n)
        obs = th.randn(7, n, o)
        v = m.value(obs, None)
        assert v.shape == (7, n, 1) and th.equal(v, m.value(obs, th.randn(7, n, 4)))
        # log-prob on request, none when nobody asks (the one-launch exploration then applies on the GPU)
        out = m.get_actions(obs, status="train", exploration=True, actions_avail=th.ones(7, n, 4), last_hid=th.zeros(7, n, 64))
        assert out[2] is not None and out[2].shape == (7, 1, 4) and out[1].shape == (7, n, 4)
    with pytest.raises(NotImplementedError):
        IPPO(golden_args("ippo", continuous=False))


def test_mappo_value_is_the_reference_composition():
    """The first layer formed once per sample plus the id column equals the reference's materialised rows."""
    args = golden_args("mappo")
    m = golden_model("MAPPO", args, "mappo_state_dict.npz")
    n, o = args.agent_num, args.obs_size
    obs = th.randn(9, n, o)
    inp = th.cat((obs.reshape(9, 1, n * o).expand(9, n, n * o), th.eye(n).expand(9, n, n)), dim=-1)
    ref, _ = m.value_dicts[0](inp.reshape(9 * n, -1), None)
    assert th.allclose(m.value(obs, None).reshape(-1), ref.reshape(-1), atol=1e-6)


@pytest.mark.parametrize("prefix,name", CASES[:2])
def test_need_split(prefix, name):
    gold = golden_vectors(prefix)
    batch = golden_batch(prefix, gold=gold, fields=FIELDS)
    both = golden_model(name, golden_args(prefix), f"{prefix}_state_dict.npz")
    pl, vl, _ = both.get_loss(batch)
    for need in ("value", "policy"):
        m = golden_model(name, golden_args(prefix), f"{prefix}_state_dict.npz")
        p, v, out = m.get_loss(batch, need=need)
        if need == "value":
            assert p is None and out is None and v.item() == vl.item()
            assert all(g is None for g in th.autograd.grad(v, list(m.policy_dicts.parameters()), allow_unused=True))
        else:
            assert v is None and p.item() == pl.item()
            assert all(g is None for g in th.autograd.grad(p, list(m.value_dicts.parameters()), allow_unused=True))
        for bn, ref in ((m.batchnorm, both.batchnorm), (m.rl.batchnorm, both.rl.batchnorm)):
            assert int(bn.num_batches_tracked) == 1 and th.equal(bn.running_mean, ref.running_mean)
            assert th.equal(bn.running_var, ref.running_var)
        m.get_loss(batch, need=need)
        assert int(m.batchnorm.num_batches_tracked) == 2 and int(m.rl.batchnorm.num_batches_tracked) == 2


# ---- GAE ----------------------------------------------------------------------------------------------------------
def _literal_loop(r, v, nv, done, last, gamma, lam, dtype):
    """ppo.py:44-52 verbatim on one chain."""
    r, v, nv, done, last = (x.to(dtype) for x in (r, v, nv, done, last))
    adv = th.zeros_like(r)
    last_adv = 0
    for i in reversed(range(r.size(0))):
        mask = 1.0 - done[i] if last[i] else 1.0
        deltas = r[i] + gamma * nv[i] * mask - v[i]
        last_adv = deltas + gamma * lam * last_adv * mask
        adv[i] = last_adv
    return adv


def _gae_inputs(rows, n, stride, seed=0):
    g = th.Generator().manual_seed(seed)
    r, v, nv = (th.randn(rows, n, generator=g) for _ in range(3))
    last = (th.rand(rows, generator=g) < 0.1).float()
    done = ((th.rand(rows, generator=g) < 0.5).float() * last)
    return r, v, nv, done, last


# Largest relative error (max |x - x64| / max |x64|) of the reference's own fp32 loop against its float64 evaluation on
# these inputs, measured: 2.9e-7 (stride 1, 256 rows), 1.9e-7 (stride 8), 5.3e-8 (stride 32, three steps).  The bound on
# the composition is four times the measurement the test takes itself; GAE_MEASURED records the largest one seen when the
# test was written and only guards the measurement.
GAE_MEASURED = 2.9e-7


@pytest.mark.parametrize("rows,n,stride", [(256, 5, 1), (256, 3, 8), (96, 5, 32)])
def test_gae_chains_against_the_literal_loop_in_float64(rows, n, stride):
    from safe_marl_amd.nets import ppo_gae_torch
    gamma, lam = 0.99, 0.95
    r, v, nv, done, last = _gae_inputs(rows, n, stride)
    ref64 = th.empty(rows, n, dtype=th.float64)
    ref32 = th.empty(rows, n)
    for e in range(stride):                       # stride N: N separate loops over rows e, e + N, ...
        sl = slice(e, rows, stride)
        ref64[sl] = _literal_loop(r[sl], v[sl], nv[sl], done[sl], last[sl], gamma, lam, th.float64)
        ref32[sl] = _literal_loop(r[sl], v[sl], nv[sl], done[sl], last[sl], gamma, lam, th.float32)
    scale = ref64.abs().max().item()
    measured = (ref32.double() - ref64).abs().max().item() / scale
    print(f"fp32 literal loop vs float64: {measured:.3e}")
    assert 0 < measured < 4 * GAE_MEASURED
    got = ppo_gae_torch(r, v, nv, done, last, gamma, lam, stride)
    err = (got.double() - ref64).abs().max().item() / scale
    print(f"composition vs float64: {err:.3e}")
    assert err <= 4 * measured
    with pytest.raises(ValueError):
        ppo_gae_torch(r[:-1], v[:-1], nv[:-1], done[:-1], last[:-1], gamma, lam, 7)


def test_gae_restarts_after_termination_and_bootstraps_after_truncation():
    from safe_marl_amd.nets import ppo_gae_torch
    gamma, lam = 0.99, 0.95
    r, v, nv = th.randn(12, 2), th.randn(12, 2), th.randn(12, 2)
    done, last = th.zeros(12), th.zeros(12)
    last[3], done[3] = 1.0, 1.0             # terminated
    last[7] = 1.0                           # truncated
    adv = ppo_gae_torch(r, v, nv, done, last, gamma, lam, 1)
    # row 3: nothing of rows 4.. and no bootstrap; exactly the delta without the next value
    assert th.equal(adv[3], r[3] - v[3])
    # changing anything after row 3 leaves rows 0..3 untouched: the chain restarted exactly there
    r2 = r.clone()
    r2[4:] += 5.0
    assert th.equal(ppo_gae_torch(r2, v, nv, done, last, gamma, lam, 1)[:4], adv[:4])
    # row 7 (last_step, not done) keeps its bootstrap and CONTINUES into row 8, as ppo.py:45-50 does
    want7 = (r[7] + gamma * nv[7] - v[7]) + gamma * lam * adv[8]
    assert th.allclose(adv[7], want7, atol=1e-6)
    assert not th.equal(ppo_gae_torch(r2, v, nv, done, last, gamma, lam, 1)[7], adv[7])


# ---- cadence ----------------------------------------------------------------------------------------------------------
class FakeVecEnv:
    """What Model._train_process_vec touches of VecFlexProvisionEnv, on CPU."""
    handle = object()
    episode_limit = 10 ** 6

    def __init__(self, n_envs, n, o, seed=0):
        self.n_envs, self.n, self.o = n_envs, n, o
        self.g = th.Generator().manual_seed(seed)
        self.obs = th.zeros(n_envs, n, o)
        from safe_marl_amd._lib import INFO_KEYS
        self.info = th.zeros(n_envs, len(INFO_KEYS))
        self.failed = th.zeros(n_envs)
        self.t = 0

    def reset(self):
        self.obs = th.randn(self.n_envs, self.n, self.o, generator=self.g) * 0.3
        return self.obs

    def step(self, action, fuse_obs=True, auto_reset=True):
        self.t += 1
        self.obs = (0.9 * self.obs + 0.1 * action.mean(dim=(1, 2), keepdim=True)
                    + 0.05 * th.randn(self.n_envs, self.n, self.o, generator=self.g))
        reward = -self.obs.pow(2).mean(dim=(1, 2)).double()
        done = (th.rand(self.n_envs, generator=self.g) < 0.02)
        return reward, done, self.info


def _vec_trainer(name, n_envs, **over):
    from safe_marl_amd.trainer import PGTrainer
    prefix = name.lower() + "3"
    args = golden_args(prefix, **over)
    env = FakeVecEnv(n_envs, args.agent_num, args.obs_size)
    return PGTrainer(args, getattr(L, name), env, None, graph_rollout=False), args


@pytest.mark.parametrize("name", ["IPPO", "MAPPO"])
def test_event_consumes_aligned_windows_and_clears_the_buffer(name, monkeypatch):
    n_envs = 4
    trainer, args = _vec_trainer(name, n_envs, behaviour_update_freq=40, max_steps=40, batch_size=8, target_update_freq=80)
    assert trainer.batch_scale == n_envs and trainer.effective_batch_size() == 8 * n_envs
    assert trainer.behaviour_net.gae_chain_stride == n_envs
    buf = trainer.replay_buffer
    starts = []
    orig = buf.aligned_window
    monkeypatch.setattr(buf, "aligned_window", lambda step, bs, N: (starts.append((step, bs, N)), orig(step, bs, N))[1])
    stat = {}
    trainer.behaviour_net.train_process(stat, trainer)            # steps 0..39: no event yet (steps > 0 is required)
    assert len(buf.buffer) == 40 * n_envs and not starts
    trainer.behaviour_net.train_process(stat, trainer)            # the event falls on step 40
    assert len(starts) == args.value_update_epochs + args.policy_update_epochs == 20
    assert all(bs == 8 * n_envs and N == n_envs and 0 <= s <= 41 - 8 for s, bs, N in starts)
    assert len(buf.buffer) == 39 * n_envs                         # cleared at the event, 39 steps collected since
    for k in ("mean_train_value_loss", "mean_train_policy_loss", "mean_train_policy_grad_norm"):
        assert np.isfinite(float(stat[k])), k
    assert float(stat["mean_train_policy_grad_norm"]) > 0


def test_reference_cadence_ten_and_ten_windows_at_240_steps(monkeypatch):
    trainer, args = _vec_trainer("IPPO", 2)                       # ippo.yaml: behaviour_update_freq 240, max_steps 240
    assert args.behaviour_update_freq == 240 and args.max_steps == 240 and args.batch_size == 32
    kinds = []
    monkeypatch.setattr(trainer, "_sub_update", lambda which, stat, batch, **k: kinds.append((which, batch.state.shape[0])))
    stat = {}
    trainer.behaviour_net.train_process(stat, trainer)
    trainer.behaviour_net.train_process(stat, trainer)
    assert kinds == [("value", 64)] * 10 + [("policy", 64)] * 10


def test_maddpg_keeps_its_buffer():
    from safe_marl_amd.learner import MADDPG
    from safe_marl_amd.trainer import PGTrainer
    args = golden_args("ippo3", alg="maddpg", behaviour_update_freq=20, max_steps=30, value_update_epochs=1,
                       policy_update_epochs=1, normalize_advantages=False)
    env = FakeVecEnv(4, args.agent_num, args.obs_size)
    trainer = PGTrainer(args, MADDPG, env, None, graph_rollout=False, graph_updates=False)
    assert trainer.batch_scale == 1 and not trainer.on_policy
    trainer.behaviour_net.train_process({}, trainer)
    assert len(trainer.replay_buffer.buffer) == 30 * 4


def test_default_capacity_and_misaligned_batches():
    from safe_marl_amd.replay_buffer import TransReplayBuffer
    from safe_marl_amd.trainer import PGTrainer
    args = golden_args("ippo3")
    env = FakeVecEnv(64, args.agent_num, args.obs_size)
    trainer = PGTrainer(args, getattr(L, "IPPO"), env, None)
    assert trainer.replay_buffer.size >= (240 + 2) * 64
    assert PGTrainer(args, getattr(L, "IPPO"), FakeVecEnv(4096, 3, 144), None).replay_buffer.size >= 242 * 4096
    with pytest.raises(ValueError):
        PGTrainer(args, getattr(L, "IPPO"), env, None, batch_scale=33)              # 32 * 33 is not a multiple of 64
    buf = TransReplayBuffer(1000, device="cpu")
    buf.add_batch(state=th.zeros(12, 3, 2), reward=th.zeros(12, 3))
    with pytest.raises(ValueError):
        buf.sample_aligned(10, 4)
    with pytest.raises(ValueError):
        buf.sample_aligned(16, 4)                                             # three steps held, four asked for
    assert buf.sample_aligned(8, 4) in (0, 1)
    buf.add_batch(state=th.zeros(3, 3, 2), reward=th.zeros(3, 3))
    with pytest.raises(ValueError):
        buf.sample_aligned(8, 4)                                              # 15 transitions: not whole steps


def test_windows_never_cross_a_gap_of_the_slab_ring():
    from safe_marl_amd.replay_buffer import TransReplayBuffer
    N, n = 4, 3
    buf = TransReplayBuffer(40 * N, device="cpu")
    buf.alloc_slabs(N, n, 6, 4, 8)
    buf.begin_stream(th.zeros(N, n, 6))
    for _ in range(5):
        buf.stepped()
    buf.begin_stream(th.zeros(N, n, 6))                 # a hard reset: slab 5 is a gap
    for _ in range(6):
        buf.stepped()
    assert buf.contiguous_runs() == [(0, 5 * N), (5 * N, 6 * N)]
    np.random.seed(0)
    assert {buf.sample_aligned(4 * N, N) for _ in range(200)} == {0, 1, 5, 6, 7}
    with pytest.raises(ValueError):
        buf.aligned_window(3, 4 * N, N)                 # steps 3..6 would span the gap
    buf.enable_filed_columns()
    buf.file_columns(5 * N, 2 * N, value=th.full((2 * N, n, 1), 7.0), next_value=th.full((2 * N, n, 1), 9.0))
    w = buf.aligned_window(5, 4 * N, N)
    assert w.value.shape == (4 * N, n, 1) and th.equal(w.value[:2 * N], th.full((2 * N, n, 1), 7.0))
    assert w.value[2 * N:].abs().max() == 0 and th.equal(w.next_value[:2 * N], th.full((2 * N, n, 1), 9.0))
    buf.clear()
    assert len(buf.buffer) == 0 and buf.contiguous_runs() == []


# ---- old values ------------------------------------------------------------------------------------------------------
# fp32 rounding of the same matrix product at another batch size: the per-step route values one sample per call, the
# event-start pass all of them at once.  The bar is the per-step route's own error against a float64 evaluation of the same
# net on the same inputs, max |a - b| / max |b|: measured 1.8e-7 (both classes); the two routes may differ by four times it.
OLD_VALUES_MEASURED = 1.8e-7


@pytest.mark.parametrize("name", ["IPPO", "MAPPO"])
def test_event_start_pass_files_what_the_per_step_route_stores(name):
    from safe_marl_amd.replay_buffer import TransReplayBuffer
    prefix = name.lower() + "3"
    args = golden_args(prefix)
    model = golden_model(name, args, f"{prefix}_state_dict.npz")
    n, o = args.agent_num, args.obs_size
    th.manual_seed(3)
    steps = 24
    states = th.randn(steps + 1, n, o) * 0.3
    # the per-step route (model.py:218,226): one sample per call
    with th.no_grad():
        per_step_v = th.cat([model.value(states[t:t + 1], None) for t in range(steps)])
        per_step_nv = th.cat([model.value(states[t + 1:t + 2], None) for t in range(steps)])
        v64 = model.double().value(states[:steps].double(), None)
        model.float()
    measured = (per_step_v.double() - v64).abs().max().item() / v64.abs().max().item()
    print(f"per-step fp32 vs float64: {measured:.3e}")
    assert 0 < measured < 4 * OLD_VALUES_MEASURED
    # the event-start pass over a two-env vector replay holding the same trajectory twice
    N = 2
    buf = TransReplayBuffer(1000, device="cpu")
    for t in range(steps):
        buf.add_batch(state=states[t].expand(N, n, o), next_state=states[t + 1].expand(N, n, o),
                      action=th.zeros(N, n, 4), last_hid=th.zeros(N, n, 64), hid=th.zeros(N, n, 64), reward=th.zeros(N, n),
                      done=th.zeros(N), last_step=th.zeros(N), action_avail=1.0, **model._unfiled_columns(N))

    class T:
        replay_buffer = buf
        env = type("E", (), {"n_envs": N})()
    model.begin_update_event(T)
    w = buf.window(0, steps * N)
    scale = per_step_v.abs().max().item()
    for env in range(N):
        assert (w.value[env::N] - per_step_v).abs().max().item() / scale <= 4 * measured
        assert (w.next_value[env::N] - per_step_nv).abs().max().item() / scale <= 4 * measured
    # next_value[t] = value[t + 1] inside an episode
    assert th.equal(w.next_value[:-N], w.value[N:])


def test_consistent_ratio_is_one_before_the_first_policy_step():
    from safe_marl_amd.trainer import PGTrainer
    trainer, args = _vec_trainer("IPPO", 4, behaviour_update_freq=20, max_steps=21, batch_size=8, target_update_freq=80,
                                 ppo_consistent_ratio=True, value_update_epochs=1, policy_update_epochs=2)
    net = trainer.behaviour_net
    assert net.consistent_ratio
    seen = []
    orig = trainer._sub_update

    def spy(which, stat, batch, **k):
        orig(which, stat, batch, **k)
        if which == "policy":
            seen.append(net.last_terms["ratios"].clone())
    trainer._sub_update = spy
    net.train_process({}, trainer)
    assert len(seen) == 2
    assert th.equal(seen[0], th.ones_like(seen[0]))               # exactly 1.0: the same expression on the same parameters
    assert not th.equal(seen[1], th.ones_like(seen[1]))           # the policy has moved
    # off by default: the reference's ratio (old log-prob := the action, model.py:313)
    plain, _ = _vec_trainer("IPPO", 4)
    assert plain.behaviour_net.consistent_ratio is False


# ---- C ABI -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from safe_marl_amd import build, _lib
    build.build()
    return _lib.load()


def test_abi_symbols_layouts_and_argument_checks(lib):
    from safe_marl_amd import _lib
    for name in ("flexnet_ppo_gae", "flexnet_ppo_policy_loss", "flexnet_ppo_value_loss"):
        assert hasattr(lib, name) and name in _lib.SYMBOLS
    assert C.sizeof(_lib.FlexPpoBatchNorm) == 4 * 4 + 5 * 8
    assert C.sizeof(_lib.FlexPpoGaeArgs) == 2 * 8 + 4 * 4 + 5 * 8 + 2 * (4 * 4 + 5 * 8) + 4 * 8 + 8
    assert C.sizeof(_lib.FlexPpoPolicyArgs) == 8 + 4 * 4 + 9 * 8 + 8
    assert C.sizeof(_lib.FlexPpoValueArgs) == 8 + 4 * 4 + 9 * 8 + 8
    assert _lib.FlexPpoGaeArgs.reward_bn.offset == 72 and _lib.FlexPpoGaeArgs.workspace_floats.offset == 216
    assert _lib.FLEXNET_PPO_WS_FLOATS == 2 * _lib.FLEXNET_TD_WS_FLOATS + 2 * 256
    header = open(os.path.join(os.path.dirname(os.path.dirname(__file__)), "include", "flexnet.h")).read()
    assert "#define FLEXNET_PPO_WS_FLOATS (2 * FLEXNET_TD_WS_FLOATS + 2 * FLEXNET_PPO_BLOCKS)" in header
    # rejected before any HIP call
    assert lib.flexnet_ppo_gae(None, None) == -1 and lib.flexnet_ppo_policy_loss(None, None) == -1
    assert lib.flexnet_ppo_value_loss(None, None) == -1
    a = _lib.FlexPpoGaeArgs()
    a.rows, a.chain_stride, a.n_agents = 32, 1, 5
    assert lib.flexnet_ppo_gae(C.byref(a), None) == -1                                  # null tensors
    p = _lib.FlexPpoPolicyArgs()
    p.rows, p.n_agents, p.act_dim = 32, 5, 4
    assert lib.flexnet_ppo_policy_loss(C.byref(p), None) == -1
    v = _lib.FlexPpoValueArgs()
    v.rows, v.n_agents = 32, 5
    assert lib.flexnet_ppo_value_loss(C.byref(v), None) == -1
    ws = (C.c_double * (_lib.FLEXNET_PPO_WS_FLOATS // 2))()
    dummy = (C.c_float * 64)()
    addr = C.addressof(dummy)
    for k in ("values", "old_values", "next_values", "reward_norm", "done", "loss", "d_values"):
        setattr(v, k, addr)
    v.workspace, v.workspace_floats = C.addressof(ws), _lib.FLEXNET_PPO_WS_FLOATS
    v.n_agents = 9
    assert lib.flexnet_ppo_value_loss(C.byref(v), None) == _lib.FLEXNET_EUNSUPPORTED    # more than 8 agents
    v.n_agents, v.workspace_floats = 5, 16
    assert lib.flexnet_ppo_value_loss(C.byref(v), None) == -1                           # short workspace


def test_kernels_use_no_scratch():
    from safe_marl_amd import build
    build.build()
    res = build.kernel_resources("ppo_")
    names = {v["name"] for v in res.values()}
    assert {"ppo_gae_lane_kernel", "ppo_gae_wave_kernel", "ppo_gae_finish_kernel", "ppo_policy_kernel", "ppo_policy_rows_kernel",
            "ppo_value_kernel", "ppo_loss_finish_kernel"} <= names
    assert all(v["scratch_bytes_per_lane"] == 0 for v in res.values())


# ---- two ranks on gloo -----------------------------------------------------------------------------------------------
def _flat(tensors):
    return th.cat([t.detach().reshape(-1).double() for t in tensors]).numpy()


def _gloo_worker(rank, world, port, name, out):
    import torch.distributed as dist
    from safe_marl_amd.trainer import PGTrainer
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    n_envs = 4
    args = golden_args(name.lower() + "3", behaviour_update_freq=20, max_steps=21, batch_size=8, target_update_freq=20,
                       value_update_epochs=3, policy_update_epochs=3)
    th.manual_seed(300 + rank)                    # different initial weights, noise and data per rank: rank 0's weights win
    np.random.seed(40 + rank)                     # ... and different windows of each rank's own replay
    env = FakeVecEnv(n_envs, args.agent_num, args.obs_size, seed=7 + rank)
    trainer = PGTrainer(args, getattr(L, name), env, None, graph_rollout=False, sync_reward_bn=True)
    net = trainer.behaviour_net
    assert trainer.world == 2 and trainer.sync_reward_bn
    assert net.batchnorm.flex_sync_ranks and net.rl.batchnorm.flex_sync_ranks
    w0 = _flat(net.parameters())
    stat = {}
    net.train_process(stat, trainer)              # 21 vector steps: the event (3 value + 3 policy sub-updates) falls on step 20
    out[rank] = dict(w0=w0, w1=_flat(net.parameters()), tgt=_flat(net.target_net.parameters()),
                     reward_bn=_flat([net.batchnorm.running_mean, net.batchnorm.running_var]),
                     adv_bn=_flat([net.rl.batchnorm.running_mean, net.rl.batchnorm.running_var]),
                     tracked=(int(net.batchnorm.num_batches_tracked), int(net.rl.batchnorm.num_batches_tracked)),
                     left=len(trainer.replay_buffer.buffer), obs=env.obs.sum().item(),
                     vg=float(stat["mean_train_value_grad_norm"]), pg=float(stat["mean_train_policy_grad_norm"]),
                     vl=float(stat["mean_train_value_loss"]))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("name", ["IPPO", "MAPPO"])
def test_two_gloo_ranks_stay_identical_after_one_event(name):
    """Each rank rolls out its own environments and samples its own step-aligned windows; the gradients travel as one
    bucket, both BatchNorms take their statistics over both ranks' rows: replicas and running statistics stay bit-equal."""
    import torch.multiprocessing as mp
    mgr = mp.Manager()
    out = mgr.dict()
    mp.spawn(_gloo_worker, args=(2, _free_port(), name, out), nprocs=2, join=True)
    a, b = out[0], out[1]
    assert a["obs"] != b["obs"] and a["vl"] != b["vl"]            # the ranks saw different data
    assert np.array_equal(a["w0"], b["w0"])                      # rank 0's initial weights everywhere
    assert np.array_equal(a["w1"], b["w1"]) and not np.array_equal(a["w0"], a["w1"])
    assert np.array_equal(a["tgt"], b["tgt"])                    # update_target fell on the same step
    assert np.array_equal(a["reward_bn"], b["reward_bn"]) and np.array_equal(a["adv_bn"], b["adv_bn"])
    assert a["tracked"] == b["tracked"] == (6, 6)                # once per get_loss, six sub-updates
    assert a["left"] == b["left"] == 0                           # the event was the last step: cleared, nothing collected since
    assert a["vg"] == b["vg"] and a["pg"] == b["pg"] and a["pg"] > 0     # the all-reduced gradient norms
