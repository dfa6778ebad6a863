"""GPU: ``shared_params: False`` through the PRODUCT paths against the golden vectors of tests/golden/make_unshared_golden.py
(the reference's MADDPG / IPPO with one RNNAgent and one critic per agent, three agents), then a short training run with
examples/train_maddpg.py's machinery under ``--unshared``.

The actors run in csrc/actor_unshared.hip: the inference launch under no_grad, and from 2 048 actor rows the autograd node.  The
golden batch has 32 samples; tile 64 makes it 2 048 samples = 6 144 actor rows, so tile 1 takes the loop with grad and tile 64
the node.  The per-agent critics keep the composition.  Every loss is a mean over samples and the BatchNorms use biased batch
statistics, so losses and gradients are invariant under tiling; IPPO's batch is tiled row by row with ``gae_chain_stride`` =
tile, which makes every copy its own GAE chain.

Tolerances are those listed in tests/test_mlp_golden_gpu.py: policy() 5e-6, losses 1e-5 relative, policy gradients within 2e-4
of each golden tensor's largest entry with no absolute term, value gradients 2e-6 + 1e-4 max|g|, ``stat`` 2e-4, the weights
after one value and one policy step 5e-5."""
import os
import sys

import numpy as np
import pytest
import torch as th

from .golden_io import StubEnv, _np, golden_args, golden_model, golden_tensors, golden_vectors
from .test_gaussian_cpu import gauss_state_dict
from .test_mlp_agent_cpu import mlp_policy_loss
from .test_unshared_cpu import FAMILIES, unshared_batch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tiled_batch(prefix, cls, gold, tile):
    """tile copies of the golden batch; IPPO's row by row, every copy a GAE chain of its own."""
    if cls != "IPPO":
        b = unshared_batch(prefix, "cuda", tile, gold=gold)
    else:
        b = unshared_batch(prefix, "cuda", 1, gold=gold)
        b = b._replace(**{k: getattr(b, k).repeat_interleave(tile, dim=0).contiguous() for k in b._fields})
    avail = b.action_avail.clone()
    avail._flex_const = 1.0                   # every action is available: flagged as the replay's constant mask is
    return b._replace(action_avail=avail)


def _first_copy(x, cls, tile):
    return x[::tile][:32] if cls == "IPPO" else x[:32]


def _node_of(t):
    fn, seen = t.grad_fn, 0
    while fn is not None and "ActorUnsharedTrainFn" not in type(fn).__name__ and fn.next_functions and seen < 16:
        fn, seen = fn.next_functions[0][0], seen + 1
    return fn if fn is not None and "ActorUnsharedTrainFn" in type(fn).__name__ else None


@pytest.mark.parametrize("tile", [1, 64])
@pytest.mark.parametrize("prefix,cls", FAMILIES)
def test_golden_on_the_device(prefix, cls, tile):
    import safe_marl_amd.learner as L
    from safe_marl_amd.trainer import PGTrainer
    from safe_marl_amd.util import FALLBACKS
    gold = golden_vectors(prefix)
    args = golden_args(prefix, cuda=True)
    declined = FALLBACKS.get("actor_unshared", 0)
    batch = _tiled_batch(prefix, cls, gold, tile)
    n = args.agent_num

    def fresh():
        m = golden_model(cls, args, gauss_state_dict(prefix, device="cuda"), "cuda")
        if cls == "IPPO":
            m.gae_chain_stride = tile
        return m
    model = fresh()
    assert model.graph_safe_updates is False
    with th.no_grad():                                   # rollout, evaluation, bootstrap targets: the inference launch
        means, log_stds, hid = model.policy(batch.state, last_hid=batch.last_hid)
    assert log_stds.shape == means.shape
    for got, key in ((means, "policy_means"), (log_stds, "policy_log_stds"), (hid, "policy_hiddens")):
        err = np.abs(_first_copy(_np(got), cls, tile) - gold[key]).max()
        print(f"{prefix} x{tile} no-grad {key}: error {err:.3e}")
        assert err <= 5e-6, (key, tile, err)
    means_g, log_stds_g, hid_g = model.policy(batch.state, last_hid=batch.last_hid)      # update pass, graph recorded
    assert means_g.requires_grad and (_node_of(means_g) is not None) == (tile == 64)
    for got, key in ((means_g, "policy_means"), (log_stds_g, "policy_log_stds"), (hid_g, "policy_hiddens")):
        assert np.allclose(_first_copy(_np(got), cls, tile), gold[key], atol=5e-6), (key, tile)

    model = fresh()
    loss, pl, vl, means, log_stds = mlp_policy_loss(model, batch, args.entr)
    print(f"{prefix} x{tile}: policy loss {pl.item():.8f} (golden {float(gold['policy_loss']):.8f}), "
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
    assert FALLBACKS.get("actor_unshared", 0) == declined


@pytest.mark.parametrize("alg", ["maddpg", "ippo"])
def test_two_update_events_of_unshared_training(alg):
    """examples/train_maddpg.py's machinery with --unshared at 64 environments: two episodes, an update event in each."""
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
    if alg == "ippo":
        a.update(PPO_ALG_ARGS)
        a.update(value_update_epochs=2, policy_update_epochs=2)
    a.update(alg=alg, agent_num=5, obs_size=144, state_size=110, action_dim=4, shared_params=False,
             behaviour_update_freq=60, target_update_freq=120)          # 512 (MADDPG) / 2 048 (IPPO) samples per update
    cls = {"maddpg": learner.MADDPG, "ippo": learner.IPPO}[alg]
    declined = FALLBACKS.get("actor_unshared", 0)
    th.manual_seed(3)
    np.random.seed(3)
    tr = PGTrainer(convert(a), cls, env, None, replay_capacity=None if alg == "ippo" else N * 96 * 2)
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
    assert FALLBACKS.get("actor_unshared", 0) == declined
