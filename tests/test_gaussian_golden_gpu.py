"""GPU: gaussian_policy through the PRODUCT paths against the golden vectors of tests/golden/make_gaussian_golden.py
(the reference's MADDPG / IPPO / COMA with the actors of madrl/agents/rnn_agent_gaussian.py), then the rollout graph and a
short training run.

The golden batch has 32 samples; tile 64 makes it 2 048 samples = 10 240 actor rows, where the update pass is the fused one
(csrc/actor.hip forward with the ``mean`` head in the fc2 slot, csrc/gauss.hip on its hidden state, csrc/gru.hip taking the
log-std head's d_h at the new hidden state).  Every loss is a mean over samples and the BatchNorms use biased batch
statistics, so losses and gradients are invariant under tiling; IPPO's batch is tiled row by row with
``gae_chain_stride`` = tile, which makes every copy its own GAE chain.

Tolerances: policy() and the losses as tests/test_learner_golden_gpu.py / test_ppo_gpu.py compare device with reference
(5e-6, 1e-5).  Policy gradients — the new ground — within 2e-4 of each golden tensor's largest entry with NO absolute term
(the log-std head's gradient is ~2e-5 for MADDPG): 1e-4 is what the CPU test allows the same code with the reference's own
summation order, and the kernels re-order fp32 sums over up to 10 240 rows and use the device's tanhf / expf.  Value
gradients run code this feature does not touch and keep that code's own tolerance, 2e-6 + 1e-4 max|g|."""
import os
import sys

import numpy as np
import pytest
import torch as th

from .golden_io import StubEnv, _np, golden_args, golden_batch, golden_model, golden_tensors, golden_vectors
from .test_gaussian_cpu import BATCH_FIELDS, FAMILIES, gauss_state_dict, recorded, trainer_policy_loss

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tiled_batch(prefix, gold, tile):
    """(batch, chain stride): tile copies of the golden batch; IPPO's row by row, every copy a GAE chain of its own."""
    if prefix != "gauss_ippo":
        b = golden_batch(prefix, "cuda", tile, gold=gold, fields=BATCH_FIELDS[prefix])
    else:
        b = golden_batch(prefix, "cuda", 1, gold=gold, fields=BATCH_FIELDS[prefix])
        b = b._replace(**{k: getattr(b, k).repeat_interleave(tile, dim=0).contiguous() for k in b._fields})
    avail = b.action_avail.clone()
    avail._flex_const = 1.0                   # every action is available: flagged as the replay's constant mask is
    return b._replace(action_avail=avail)


def _first_copy(x, prefix, tile):
    return x[::tile][:32] if prefix == "gauss_ippo" else x[:32]


def _draws(prefix, draws, tile):
    d = th.from_numpy(np.asarray(draws))
    return recorded(d.repeat(1, tile, 1, 1).numpy())


@pytest.mark.parametrize("tile", [1, 64])
@pytest.mark.parametrize("prefix,cls", FAMILIES)
def test_golden_on_the_device(prefix, cls, tile):
    import safe_marl_amd.learner as L
    from safe_marl_amd.trainer import PGTrainer
    from safe_marl_amd.util import FALLBACKS
    gold = golden_vectors(prefix)
    args = golden_args(prefix, cuda=True)
    declined = dict(FALLBACKS)                # counts, not keys: other tests of the process decline on purpose
    batch = _tiled_batch(prefix, gold, tile)
    n = args.agent_num

    def fresh():
        m = golden_model(cls, args, gauss_state_dict(prefix, device="cuda"), "cuda")
        if prefix == "gauss_ippo":
            m.gae_chain_stride = tile
        return m
    model = fresh()
    with th.no_grad():                                   # fused inference: csrc/actor.hip, then the head on its hidden state
        means, log_stds, hid = model.policy(batch.state, last_hid=batch.last_hid)
    assert not hasattr(log_stds, "_flex_entropy") and log_stds.shape == means.shape
    for got, key in ((means, "policy_means"), (log_stds, "policy_log_stds"), (hid, "policy_hiddens")):
        assert np.allclose(_first_copy(_np(got), prefix, tile), gold[key], atol=5e-6), (key, tile)
    means_g, log_stds_g, hid_g = model.policy(batch.state, last_hid=batch.last_hid)      # update pass, graph recorded
    assert log_stds_g.requires_grad and not hasattr(log_stds_g, "_flex_entropy")
    for got, key in ((means_g, "policy_means"), (log_stds_g, "policy_log_stds"), (hid_g, "policy_hiddens")):
        assert np.allclose(_first_copy(_np(got), prefix, tile), gold[key], atol=5e-6), (key, tile)
    assert float(log_stds_g.detach().min()) >= args.LOG_STD_MIN and float(log_stds_g.detach().max()) <= args.LOG_STD_MAX

    model = fresh()
    if cls == "COMA":
        model.sample_source = _draws(prefix, gold["sampled"], tile)
    loss, pl, vl, means, log_stds = trainer_policy_loss(model, batch, args.entr)
    print(f"{prefix} x{tile}: policy loss {pl.item():.8f} (golden {float(gold['policy_loss']):.8f}), "
          f"value loss {vl.item():.8f} (golden {float(gold['value_loss']):.8f})")
    assert abs(pl.item() - float(gold["policy_loss"])) < 1e-5 * max(1.0, abs(float(gold["policy_loss"])))
    assert abs(vl.item() - float(gold["value_loss"])) < 1e-5 * max(1.0, abs(float(gold["value_loss"])))
    assert np.allclose(_first_copy(_np(log_stds), prefix, tile), gold["log_stds"], atol=5e-6)
    names = [k for k, _ in model.value_dicts.named_parameters()]
    grads = th.autograd.grad(vl, list(model.value_dicts.parameters()), retain_graph=True)
    for k, g in zip(names, grads):
        ref = gold["vgrad." + k]
        assert np.allclose(_np(g), ref, atol=2e-6 + 1e-4 * np.abs(ref).max()), (tile, k, np.abs(_np(g) - ref).max())
    names = [k for k, _ in model.policy_dicts.named_parameters()]
    grads = th.autograd.grad(loss, list(model.policy_dicts.parameters()))
    for k, g in zip(names, grads):
        ref = gold["pgrad." + k]
        err, bound = np.abs(_np(g) - ref).max(), 2e-4 * np.abs(ref).max()
        print(f"{prefix} x{tile} pgrad.{k}: error {err:.3e}, bound {bound:.3e}, max|golden| {np.abs(ref).max():.3e}")
        assert err <= bound, (tile, k, err, bound)

    # one value step, then one policy step through PGTrainer: the trainer's own entropy term, csrc/optim.hip
    th.manual_seed(0)
    trainer = PGTrainer(args, getattr(L, cls), StubEnv(n), None)
    net = trainer.behaviour_net
    net.load_state_dict(gauss_state_dict(prefix, device="cuda"))
    if prefix == "gauss_ippo":
        net.gae_chain_stride = tile
    if cls == "COMA":
        net.sample_source = _draws(prefix, gold["step.sampled_policy"], tile)
    stat = {}
    trainer.value_transition_process(stat, batch)
    trainer.policy_transition_process(stat, batch)
    for k in ("mean_train_value_loss", "mean_train_value_grad_norm", "mean_train_policy_loss", "mean_train_policy_grad_norm",
              "mean_train_entropy"):
        ref = float(gold["stat." + k])
        assert abs(float(stat[k]) - ref) < 2e-4 * max(1.0, abs(ref)), (tile, k, float(stat[k]), ref)
    after = gauss_state_dict(prefix, "state_dict_after_step")
    init = golden_tensors(f"{prefix}_state_dict.npz")
    cur = net.state_dict()
    for k, v in after.items():
        if "batchnorm" in k:                  # (running_var sees the unbiased n / (n - 1) factor of a tiled batch)
            continue
        assert np.allclose(_np(cur[k]), v.float().numpy(), atol=5e-5), (tile, k, (cur[k].cpu() - v).abs().max())
    assert not th.equal(cur["policy_dicts.0.log_std.weight"].cpu(), init["policy_dicts.0.log_std.weight"])
    assert dict(FALLBACKS) == declined, (FALLBACKS, declined)       # the fused configuration: nothing declined


def _rollout_setup(alg, n_envs):
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    from train_maddpg import DEFAULT_ALG_ARGS, PPO_ALG_ARGS
    from safe_marl_amd import learner
    from safe_marl_amd.flex_env import VecFlexProvisionEnv
    from safe_marl_amd.network import create_network
    from safe_marl_amd.series import make_synthetic_series
    from safe_marl_amd.util import convert
    net = create_network()
    series = make_synthetic_series(net, n_days=30)
    a = dict(DEFAULT_ALG_ARGS)
    if alg == "ippo":
        a.update(PPO_ALG_ARGS)
    a.update(alg=alg, agent_num=5, obs_size=144, state_size=110, action_dim=4, gaussian_policy=True)
    cls = {"maddpg": learner.MADDPG, "ippo": learner.IPPO}[alg]
    return a, cls, [VecFlexProvisionEnv({}, n_envs, net=net, series=series, seed=4, warm_start=True)]


@pytest.mark.parametrize("alg", ["maddpg", "ippo"])
def test_rollout_graph_general_body_follows_get_actions(alg):
    """Under gaussian_policy the kernels that carry one constant std are off, and a step of the general body is the eager
    loop's get_actions + env_action for the same torch seed.

    MADDPG: the plain body and MADDPG.get_actions are the same tensor expression on the same draws — the action and the
    action handed to the environment are EQUAL, bit for bit.
    IPPO: the body's flexnet_gauss_sum_explore against select_action's tensor ops on the same eps; with 2^-24 the unit in the
    last place of y in [0.5, 1): x = m + eps exp(ls) differs by at most 3 * 2^-23 |x| (two expf within an ulp of the true value
    each, one rounding of the product), tanh maps that to at most 3 * 2^-23 max_x |x| (1 - tanh^2 x) = 3 * 0.448 * 2^-23 =
    2.7 * 2^-24, and two tanhf within two ulps of the true value each differ by at most 4 * 2^-24: 7 * 2^-24 on the action.
    The env's action 0.5 (clamp(y, 0, 1) + 1) halves that and can round c + 1 in [1, 2) the other way (2^-23, halved):
    (3.5 + 1) -> 5 * 2^-24."""
    from safe_marl_amd import learner
    from safe_marl_amd.replay_buffer import TransReplayBuffer
    from safe_marl_amd.util import convert
    N = 64
    a, cls, envs = _rollout_setup(alg, N)
    th.manual_seed(8)
    m = cls(convert(a)).cuda()
    with th.no_grad():
        for p in m.policy_dicts.parameters():
            p.mul_(10.0)                       # the default init is tiny: make both heads matter
    rg = learner.RolloutGraph(m, envs[0], TransReplayBuffer(N * 8, device="cuda"))
    assert rg.gaussian
    assert not (rg._fast or rg.ring_io or rg.sink or rg.summed_sink or rg.burst_launch)
    assert not rg.fast and not rg.sink_active and not rg.ring_active and not rg.fused_burst
    assert rg.plain == (alg == "maddpg") and rg.summed == (alg == "ippo")
    env = envs[0]
    handed, env_step = [], env.step

    def recording_step(action, **kw):          # what the body hands to the environment
        handed.append(action.detach().clone())
        return env_step(action, **kw)
    env.step = recording_step
    rg.start_episode(env.reset())
    avail = th.ones(N, 5, 4, device="cuda")
    for step in range(3):
        obs, hid = rg.obs.clone(), rg.hid.clone()                  # what this step's policy evaluation reads
        th.manual_seed(500 + step)
        rg.step()
        th.manual_seed(500 + step)
        with th.no_grad():
            action, action_pol, _, (_, log_stds), new_hid = m.get_actions(obs, status="train", exploration=True,
                                                                          actions_avail=avail, target=False, last_hid=hid)
            env_action = m.env_action(action)
        th.cuda.synchronize()
        assert log_stds.std() > 0.01                               # per-row standard deviations really differ
        t = rg.last_transition()
        assert th.equal(t.state, obs) and th.equal(t.last_hid, hid)
        want = action_pol.expand(N, 5, 4)
        diff = (t.action - want).abs().max().item()
        env_diff = (handed[-1].reshape(N, 5, 4) - env_action.reshape(N, 5, 4)).abs().max().item()
        print(f"{alg} step {step}: max |action - get_actions| {diff:.3e}, max |env action - env_action| {env_diff:.3e}")
        assert len(handed) == step + 1
        if alg == "maddpg":
            assert th.equal(t.action, want) and th.equal(handed[-1].reshape(N, 5, 4), env_action.reshape(N, 5, 4))
        else:
            assert diff <= 7 * 2.0 ** -24 and env_diff <= 5 * 2.0 ** -24
        assert th.equal(t.hid, new_hid * (1.0 - env.done.float()).view(N, 1, 1))
        assert th.equal(t.next_state, env.obs) and th.equal(rg.obs, env.obs)
    del env.step                               # (the instance attribute: the class's method again)
    rg.capture()
    rg.start_episode(env.reset())
    before = rg.obs.clone()
    for _ in range(4):
        rg.step()
    th.cuda.synchronize()
    t = rg.last_transition()
    assert not th.equal(before, rg.obs) and all(th.isfinite(getattr(t, k)).all() for k in ("state", "action", "reward", "hid"))
    assert float(t.action.abs().max()) <= 1.0


@pytest.mark.parametrize("alg", ["maddpg", "ippo"])
def test_one_update_event_of_training(alg):
    from safe_marl_amd.trainer import PGTrainer
    from safe_marl_amd.util import FALLBACKS, convert
    N = 64
    a, cls, envs = _rollout_setup(alg, N)
    a.update(behaviour_update_freq=60, target_update_freq=120)      # 512 (MADDPG) / 2 048 (IPPO) samples: the fused update pass
    if alg == "ippo":
        a.update(value_update_epochs=2, policy_update_epochs=2)
    declined = dict(FALLBACKS)
    th.manual_seed(3)
    np.random.seed(3)
    tr = PGTrainer(convert(a), cls, envs[0], None, replay_capacity=None if alg == "ippo" else N * 96 * 2)
    net = tr.behaviour_net
    w0 = net.policy_dicts[0].log_std.weight.detach().clone()
    stat = {}
    net.train_process(stat, tr)                                    # 95 vector steps: one update event, at step 60
    th.cuda.synchronize()
    for k in ("mean_train_value_loss", "mean_train_policy_loss", "mean_train_policy_grad_norm", "mean_train_entropy",
              "mean_train_reward"):
        assert np.isfinite(float(stat[k])), (k, stat)
    assert float(stat["mean_train_policy_grad_norm"]) > 0
    assert not th.equal(w0, net.policy_dicts[0].log_std.weight.detach())
    with th.no_grad():
        _, log_stds, _ = net.policy(envs[0].obs.clone(), last_hid=th.zeros(N, 5, 64, device="cuda"))
    assert th.isfinite(log_stds).all()
    assert float(log_stds.min()) >= a["LOG_STD_MIN"] and float(log_stds.max()) <= a["LOG_STD_MAX"]
    assert dict(FALLBACKS) == declined, (FALLBACKS, declined)
