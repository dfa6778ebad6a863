"""FACMADDPG on the GPU (csrc/qmix.hip for the mixer) against the reference's own modules (tests/golden/facmaddpg*_*,
make_facmaddpg_golden.py), and a short vectorised training run with the mixer's sub-updates."""
import os

import numpy as np
import pytest
import torch as th

from .golden_io import (G, StubEnv, _grads, _np, facmaddpg_state_dict, golden_args, golden_batch, golden_model,
                        golden_vectors)

pytestmark = pytest.mark.gpu

PREFIXES = ["facmaddpg", "facmaddpg3"]


@pytest.mark.parametrize("prefix,tile", [("facmaddpg", 1), ("facmaddpg", 64), ("facmaddpg3", 64)])
def test_losses_and_grads_match_the_reference(prefix, tile):
    from safe_marl_amd.learner import FACMADDPG
    args = golden_args(prefix, cuda=True)
    gold = golden_vectors(prefix)
    mgold = dict(np.load(os.path.join(G, prefix + "_golden_mixer_grads.npz")))
    model = golden_model(FACMADDPG, args, facmaddpg_state_dict(prefix, device="cuda", target_mixer=True), "cuda")
    b = golden_batch(prefix, "cuda", tile)
    n, o = args.agent_num, args.obs_size
    assert model.mixer.fused_supported(b.reward, b.state.reshape(-1, n * o))         # the HIP path is the one under test
    with th.no_grad():
        v = model.value(b.state, b.action)
        assert np.allclose(_np(v)[:32], gold["value"], atol=2e-5)
        q = model.mixer(v.view(-1, n), b.state.reshape(-1, n * o)).view(-1, 1)
        assert np.allclose(_np(q)[:32], gold["q_tot"], atol=1e-4, rtol=1e-4)
    pl, vl, _ = model.get_loss(b)
    assert abs(pl.item() - float(gold["policy_loss"])) < 1e-5
    assert abs(vl.item() - float(gold["value_loss"])) < 1e-4 * max(1.0, abs(float(gold["value_loss"])))
    _, vl, _ = model.get_loss(b, need="value")
    names = [k for k, _ in model.value_dicts.named_parameters()]
    for k, g in zip(names, _grads(vl, model.value_dicts.parameters())):
        r = gold["vgrad." + k]
        assert np.allclose(g, r, atol=2e-6 + 2e-4 * np.abs(r).max()), (tile, k, np.abs(g - r).max())
    _, ml, _ = model.get_loss(b, need="mixer")
    names = [k for k, _ in model.mixer.named_parameters()]
    for k, g in zip(names, _grads(ml, model.mixer.parameters())):
        r = mgold["mgrad." + k]
        assert np.allclose(g, r, atol=2e-6 + 2e-4 * np.abs(r).max()), (tile, k, np.abs(g - r).max())
    pl, _, _ = model.get_loss(b, need="policy")
    names = [k for k, _ in model.policy_dicts.named_parameters()]
    for k, g in zip(names, _grads(pl, model.policy_dicts.parameters())):
        r = gold["pgrad." + k]
        assert np.allclose(g, r, atol=2e-7 + 1e-4 * np.abs(r).max()), (tile, k, np.abs(g - r).max())


@pytest.mark.parametrize("prefix", PREFIXES)
def test_trainer_steps_and_target_update_match_the_reference(prefix):
    from safe_marl_amd.learner import FACMADDPG
    from safe_marl_amd.trainer import PGTrainer
    args = golden_args(prefix, cuda=True)
    gold = golden_vectors(prefix)
    tr = PGTrainer(args, FACMADDPG, StubEnv(args.agent_num), None)
    sd = facmaddpg_state_dict(prefix, device="cuda", target_mixer=True)
    tr.behaviour_net.load_state_dict(sd)
    tr.behaviour_net.target_net.load_state_dict({k[len("target_net."):]: v for k, v in sd.items() if k.startswith("target_net.")})
    b = golden_batch(prefix, "cuda")
    stat = {}
    tr.value_transition_process(stat, b)
    tr.policy_transition_process(stat, b)
    tr.mixer_transition_process(stat, b)
    for k in ("mean_train_value_loss", "mean_train_mixer_loss", "mean_train_value_grad_norm", "mean_train_mixer_grad_norm"):
        ref = gold["stat." + k]
        assert abs(float(stat[k]) - ref) < 2e-4 * max(1.0, abs(ref)), k
    after = facmaddpg_state_dict(prefix, "state_dict_after_step", "cuda")
    cur = tr.behaviour_net.state_dict()
    for k, v in after.items():
        assert np.allclose(_np(cur[k]), _np(v), atol=5e-5), (k, np.abs(_np(cur[k]) - _np(v)).max())
    tr.behaviour_net.update_target()
    tgt = facmaddpg_state_dict(prefix, "target_after_update", "cuda")
    cur = tr.behaviour_net.target_net.state_dict()
    for k, v in tgt.items():
        assert np.allclose(_np(cur[k]), _np(v), atol=5e-5), k


def test_short_training_run_moves_the_mixer():
    from safe_marl_amd import learner
    from safe_marl_amd.flex_env import VecFlexProvisionEnv
    from safe_marl_amd.network import create_network
    from safe_marl_amd.series import make_synthetic_series
    from safe_marl_amd.trainer import PGTrainer
    blds = [5, 10, 15, 20, 25]
    env_args = {"buildings": blds, "pv_nodes": blds, "ess_nodes": blds}
    net = create_network(env_args)
    env = VecFlexProvisionEnv(env_args, 256, net=net, series=make_synthetic_series(net, n_days=60), seed=3, warm_start=True)
    args = golden_args("facmaddpg", cuda=True, agent_num=env.n_agents, obs_size=env.obs_size, state_size=env.state_size,
                       v_min=0.9, v_max=1.1, target_update_freq=60)
    th.manual_seed(0)
    np.random.seed(0)
    tr = PGTrainer(args, learner.FACMADDPG, env, None, batch_scale=64, replay_capacity=256 * 96 * 2)
    net_ = tr.behaviour_net
    m0 = [p.detach().clone() for p in net_.mixer.parameters()]
    stat = {}
    for _ in range(2):                                        # 190 vector steps: three update events
        net_.train_process(stat, tr)
    th.cuda.synchronize()
    for k in ("mean_train_value_loss", "mean_train_policy_loss", "mean_train_mixer_loss", "mean_train_mixer_grad_norm"):
        assert k in stat and np.isfinite(float(stat[k])), k
    moved = [not th.equal(a, p) for a, p in zip(m0, net_.mixer.parameters())]
    assert all(moved)
    # the target mixer moves by the soft updates only (target_lr 0.01 at steps 60, 120, 180): away from its start, not onto
    # the behaviour mixer, and one more update_target is exactly t <- (1 - tau) t + tau p
    tau = args.target_lr
    before = [t.detach().clone() for t in net_.target_net.mixer.parameters()]
    for p0, p, t in zip(m0, net_.mixer.parameters(), before):
        assert not th.equal(t, p0) and not th.equal(t, p.detach())
    net_.update_target()
    for p, t, t1 in zip(net_.mixer.parameters(), before, net_.target_net.mixer.parameters()):
        assert th.allclose(t1.detach(), (1 - tau) * t + tau * p.detach(), atol=1e-7, rtol=1e-6)
    assert net_._rollout_graph.summed                          # IDDPG's fused agent-summed action selection
