"""GPU: ``shared_params: False`` with MLP agents and with Gaussian agents through the PRODUCT paths against the golden vectors of
tests/golden/make_unshared_agents_golden.py (the reference's MADDPG / IPPO with one agent module and one critic per agent, three
agents), then short training runs with examples/train_maddpg.py's machinery under ``--unshared`` with ``--agent-type mlp``,
``--gaussian-policy`` and both.

The golden batch has 32 samples; tile 64 makes it 2 048 samples = 6 144 actor rows, so tile 1 takes the loop with gradients and
tile 64 the nodes (nets._ActorMlpUnsharedTrainFn / nets._ActorUnsharedTrainHidFn, and nets._GaussHeadUnsharedFn for the Gaussian
agents); the no_grad pass takes the launches at either size.  Tiling and tolerances are tests/test_unshared_golden_gpu.py's (its
helpers imported; the bounds restated): policy() 5e-6, losses 1e-5 relative, policy gradients within 2e-4 of each golden tensor's
largest entry with no absolute term, value gradients 2e-6 + 1e-4 max|g|, ``stat`` 2e-4, the weights after one value and one
policy step 5e-5."""
import os
import sys

import numpy as np
import pytest
import torch as th

from .golden_io import StubEnv, _np, golden_args, golden_model, golden_tensors, golden_vectors
from .test_gaussian_cpu import gauss_state_dict
from .test_mlp_agent_cpu import mlp_policy_loss
from .test_unshared_agents_cpu import DIR, FAMILIES
from .test_unshared_golden_gpu import _first_copy, _tiled_batch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BATCH_OF = {"MADDPG": "unshared_maddpg", "IPPO": "unshared_ippo"}        # which fields _tiled_batch takes from the golden file
NOTES = ("actor_unshared", "actor_mlp_unshared", "gauss_head", "gaussian_policy", "actor_forward")


def _spy(monkeypatch):
    """Counts of the nodes' applications and of every library launch by name."""
    from safe_marl_amd import _lib, nets
    seen = {}
    real = _lib.try_launch

    def launch(name, *a, **k):
        seen[name] = seen.get(name, 0) + 1
        return real(name, *a, **k)
    monkeypatch.setattr(_lib, "try_launch", launch)
    for fn in ("actor_mlp_unshared_train", "actor_unshared_train", "gauss_log_std_unshared"):
        def wrap(*a, _real=getattr(nets, fn), _fn=fn, **k):
            seen[_fn] = seen.get(_fn, 0) + 1
            return _real(*a, **k)
        monkeypatch.setattr(nets, fn, wrap)
        import safe_marl_amd.learner as L
        if hasattr(L, fn):
            monkeypatch.setattr(L, fn, wrap)
    return seen


@pytest.mark.parametrize("tile", [1, 64])
@pytest.mark.parametrize("family,cls,agent_type,gauss", FAMILIES)
def test_golden_on_the_device(family, cls, agent_type, gauss, tile, monkeypatch):
    import safe_marl_amd.learner as L
    from safe_marl_amd.trainer import PGTrainer
    from safe_marl_amd.util import FALLBACKS
    prefix = DIR + family
    gold = golden_vectors(prefix)
    args = golden_args(prefix, cuda=True)
    noted = {k: FALLBACKS.get(k, 0) for k in NOTES}
    batch = _tiled_batch(BATCH_OF[cls], cls, gold, tile)
    n = args.agent_num
    seen = _spy(monkeypatch)
    mlp = agent_type == "mlp"
    fwd = "flexnet_actor_mlp_unshared_forward" if mlp else "flexnet_actor_unshared_forward"
    bwd = "flexnet_actor_mlp_unshared_backward" if mlp else "flexnet_actor_unshared_backward_hn"
    node = "actor_mlp_unshared_train" if mlp else "actor_unshared_train"

    def fresh():
        m = golden_model(cls, args, gauss_state_dict(prefix, device="cuda"), "cuda")
        if cls == "IPPO":
            m.gae_chain_stride = tile
        return m
    model = fresh()
    assert model.graph_safe_updates is False
    with th.no_grad():                                   # rollout, evaluation, bootstrap targets: the inference launch
        means, log_stds, hid = model.policy(batch.state, last_hid=batch.last_hid)
    assert log_stds.shape == means.shape and seen.get(fwd, 0) == 1 and node not in seen
    assert seen.get("flexnet_gauss_head_unshared_forward", 0) == (1 if gauss else 0)
    for got, key in ((means, "policy_means"), (log_stds, "policy_log_stds"), (hid, "policy_hiddens")):
        err = np.abs(_first_copy(_np(got), cls, tile) - gold[key]).max()
        print(f"{family} x{tile} no-grad {key}: error {err:.3e}")
        assert err <= 5e-6, (key, tile, err)
    means_g, log_stds_g, hid_g = model.policy(batch.state, last_hid=batch.last_hid)      # update pass, graph recorded
    assert means_g.requires_grad and log_stds_g.requires_grad == gauss
    assert seen.get(node, 0) == (1 if tile == 64 else 0)                                  # the node from 2 048 actor rows
    assert seen.get("gauss_log_std_unshared", 0) == (1 if gauss else 0) + (1 if gauss and tile == 64 else 0)
    for got, key in ((means_g, "policy_means"), (log_stds_g, "policy_log_stds"), (hid_g, "policy_hiddens")):
        assert np.allclose(_first_copy(_np(got), cls, tile), gold[key], atol=5e-6), (key, tile)

    model = fresh()
    loss, pl, vl, means, log_stds = mlp_policy_loss(model, batch, args.entr)
    print(f"{family} x{tile}: policy loss {pl.item():.8f} (golden {float(gold['policy_loss']):.8f}), "
          f"value loss {vl.item():.8f} (golden {float(gold['value_loss']):.8f})")
    assert abs(pl.item() - float(gold["policy_loss"])) < 1e-5 * max(1.0, abs(float(gold["policy_loss"])))
    assert abs(vl.item() - float(gold["value_loss"])) < 1e-5 * max(1.0, abs(float(gold["value_loss"])))
    assert np.allclose(_first_copy(_np(log_stds), cls, tile), gold["log_stds"], atol=5e-6)
    names = [k for k, _ in model.value_dicts.named_parameters()]
    grads = th.autograd.grad(vl, list(model.value_dicts.parameters()), retain_graph=True)
    for k, g in zip(names, grads):
        ref = gold["vgrad." + k]
        assert np.allclose(_np(g), ref, atol=2e-6 + 1e-4 * np.abs(ref).max()), (tile, k, np.abs(_np(g) - ref).max())
    names = [k for k, _ in model.policy_dicts.named_parameters()]
    before_bwd = seen.get(bwd, 0)
    grads = th.autograd.grad(loss, list(model.policy_dicts.parameters()))
    ran = seen.get(bwd, 0) - before_bwd                                                   # the fused backward actually ran
    assert ran >= 1 if tile == 64 else ran == 0, seen
    if gauss:
        ran = seen.get("flexnet_gauss_head_unshared_backward", 0)
        assert ran >= 1 if tile == 64 else ran == 0, seen
    for k, g in zip(names, grads):
        ref = gold["pgrad." + k]
        err, bound = np.abs(_np(g) - ref).max(), 2e-4 * np.abs(ref).max()
        print(f"{family} x{tile} pgrad.{k}: error {err:.3e}, bound {bound:.3e}, max|golden| {np.abs(ref).max():.3e}")
        assert err <= bound, (tile, k, err, bound)

    # one value step, then one policy step through PGTrainer: the trainer's own entropy term, csrc/optim.hip
    th.manual_seed(0)
    trainer = PGTrainer(args, getattr(L, cls), StubEnv(n), None)
    net = trainer.behaviour_net
    net.load_state_dict(gauss_state_dict(prefix, device="cuda"))
    if cls == "IPPO":
        net.gae_chain_stride = tile
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
    for a in range(n):
        assert not th.equal(cur[f"policy_dicts.{a}.fc1.weight"].cpu(), init[f"policy_dicts.{a}.fc1.weight"])
    assert {k: FALLBACKS.get(k, 0) for k in NOTES} == noted


@pytest.mark.parametrize("agent_type,gauss", [("mlp", False), ("rnn", True), ("mlp", True)])
def test_two_update_events_of_unshared_training(agent_type, gauss, monkeypatch):
    """examples/train_maddpg.py's machinery with --unshared --alg ippo and --agent-type mlp / --gaussian-policy / both at 64
    environments and 5 agents: two episodes, an update event in each."""
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    from train_maddpg import DEFAULT_ALG_ARGS, PPO_ALG_ARGS
    from safe_marl_amd import learner
    from safe_marl_amd.flex_env import VecFlexProvisionEnv
    from safe_marl_amd.network import create_network
    from safe_marl_amd.series import make_synthetic_series
    from safe_marl_amd.trainer import PGTrainer
    from safe_marl_amd.util import FALLBACKS, convert
    N = 64
    net_ = create_network()
    env = VecFlexProvisionEnv({}, N, net=net_, series=make_synthetic_series(net_, n_days=30), seed=4, warm_start=True)
    a = dict(DEFAULT_ALG_ARGS)
    a.update(PPO_ALG_ARGS)
    a.update(value_update_epochs=2, policy_update_epochs=2)
    a.update(alg="ippo", agent_num=5, obs_size=144, state_size=110, action_dim=4, shared_params=False, agent_type=agent_type,
             gaussian_policy=gauss, behaviour_update_freq=60, target_update_freq=120)     # 2 048 samples per update
    noted = {k: FALLBACKS.get(k, 0) for k in NOTES}
    seen = _spy(monkeypatch)
    allowed, real_body = [], learner.RolloutGraph.body

    def body(self, *args, **kw):                                   # what the rollout body's policy() call will be told
        from safe_marl_amd.nets import mlp_actor_allowed
        allowed.append(mlp_actor_allowed())
        return real_body(self, *args, **kw)
    monkeypatch.setattr(learner.RolloutGraph, "body", body)
    th.manual_seed(3)
    np.random.seed(3)
    tr = PGTrainer(convert(a), learner.IPPO, env, None, replay_capacity=None)
    net = tr.behaviour_net
    assert len(net.policy_dicts) == 5 and net.graph_safe_updates is False
    w0 = {k: v.detach().clone() for k, v in net.policy_dicts.state_dict().items()}
    for _ in range(2):
        stat = {}
        net.train_process(stat, tr)                                # 95 vector steps: one update event, at step 60
        th.cuda.synchronize()
        for k in ("mean_train_value_loss", "mean_train_policy_loss", "mean_train_policy_grad_norm", "mean_train_entropy",
                  "mean_train_reward"):
            assert np.isfinite(float(stat[k])), (k, stat)
        assert float(stat["mean_train_policy_grad_norm"]) > 0
    for k, v in net.policy_dicts.state_dict().items():             # every agent's weights moved
        assert th.isfinite(v).all() and not th.equal(v, w0[k]), k
    # the rollout graph: its three warm-up steps run the body the capture runs — the per-agent paths stand aside in both, so the
    # module loop's library GEMMs are first called eagerly, never inside a capture
    assert tr.graph_rollout and len(allowed) >= 4 and not any(allowed), allowed
    node = "actor_mlp_unshared_train" if agent_type == "mlp" else "actor_unshared_train"
    assert seen.get(node, 0) >= 2 and (not gauss or seen.get("flexnet_gauss_head_unshared_backward", 0) >= 2), seen
    assert {k: FALLBACKS.get(k, 0) for k in NOTES} == noted
