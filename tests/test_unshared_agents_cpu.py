"""shared_params: False with MLP agents and with Gaussian agents, on CPU: golden vectors captured by importing the reference's
MADDPG / IPPO with one agent module and one critic per agent (tests/golden/make_unshared_agents_golden.py, three agents; the files
live in tests/golden/per_agent/) — strict state_dict loads, ``policy()``, both losses, every gradient, ``stat`` and the weights
after one value and one policy step, as tests/test_unshared_cpu.py does for the RNN agents with the fixed std."""
import os

import numpy as np
import pytest
import torch as th

from .golden_io import StubEnv, golden_args, golden_batch, golden_model, golden_tensors, golden_vectors
from .test_gaussian_cpu import assert_grads, gauss_state_dict
from .test_mlp_agent_cpu import mlp_policy_loss

DIR = "per_agent/"
# family, algorithm class, agent_type, gaussian_policy
FAMILIES = [("unshared_mlp_maddpg", "MADDPG", "mlp", False), ("unshared_mlp_ippo", "IPPO", "mlp", False),
            ("unshared_gauss_ippo", "IPPO", "rnn", True), ("unshared_mlp_gauss_ippo", "IPPO", "mlp", True)]
BATCH_FIELDS = {"MADDPG": (), "IPPO": ("action", "done", "last_step")}
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def agents_batch(cls, device="cpu", tile=1, gold=None):
    """The three-agent batch (learner3_batch.npz) with the fields the family's reference run replaced."""
    return golden_batch("learner3", device, tile, gold=gold, fields=BATCH_FIELDS[cls])


def agent_class(agent_type, gauss):
    from safe_marl_amd import nets
    return {("mlp", False): nets.MLPAgent, ("mlp", True): nets.MLPAgentGaussian, ("rnn", True): nets.RNNAgentGaussian}[agent_type, gauss]


@pytest.mark.parametrize("family,cls,agent_type,gauss", FAMILIES)
def test_golden_parity(family, cls, agent_type, gauss):
    import safe_marl_amd.learner as L
    from safe_marl_amd.trainer import PGTrainer
    from safe_marl_amd.util import FALLBACKS
    prefix = DIR + family
    noted = dict(FALLBACKS)
    gold = golden_vectors(prefix)
    args = golden_args(prefix)
    n = args.agent_num
    assert args.agent_type == agent_type and bool(args.gaussian_policy) == gauss
    assert not args.shared_params and args.agent_id and n == 3
    model = golden_model(cls, args, gauss_state_dict(prefix))            # strict: the reference's names and shapes
    assert len(model.policy_dicts) == len(model.value_dicts) == n
    kind = agent_class(agent_type, gauss)
    assert all(type(a) is kind and a.fc1.weight.shape == (64, args.obs_size + n) for a in model.policy_dicts)
    if gauss:
        assert (args.LOG_STD_MIN, args.LOG_STD_MAX) == (0.0, 0.5)
        assert {"0.mean.weight", "0.log_std.weight"} <= set(model.policy_dicts.state_dict())
    batch = agents_batch(cls, gold=gold)

    with th.no_grad():
        means, log_stds, hiddens = model.policy(batch.state, last_hid=batch.last_hid)
    assert log_stds.shape == means.shape == (32, n, 4)
    assert np.allclose(means.numpy(), gold["policy_means"], atol=2e-6)
    assert np.allclose(log_stds.numpy(), gold["policy_log_stds"], atol=2e-6)
    assert np.allclose(hiddens.numpy(), gold["policy_hiddens"], atol=2e-6)

    loss, pl, vl, means, log_stds = mlp_policy_loss(model, batch, args.entr)
    assert abs(pl.item() - float(gold["policy_loss"])) < 2e-6 * max(1.0, abs(float(gold["policy_loss"])))
    assert abs(vl.item() - float(gold["value_loss"])) < 1e-5 * max(1.0, abs(float(gold["value_loss"])))
    assert np.allclose(means.detach().numpy(), gold["means"], atol=2e-6)
    assert np.allclose(log_stds.detach().numpy(), gold["log_stds"], atol=2e-6)
    grads = th.autograd.grad(vl, list(model.value_dicts.parameters()), retain_graph=True)
    assert_grads(model.value_dicts.named_parameters(), grads, gold, "vgrad.")
    grads = th.autograd.grad(loss, list(model.policy_dicts.parameters()))
    assert_grads(model.policy_dicts.named_parameters(), grads, gold, "pgrad.")
    assert len(grads) == len([k for k in gold if k.startswith("pgrad.")])
    # the one-hot input: agent a's id block takes a gradient in its own column only, the bias gradient
    for a in range(n):
        ids = gold[f"pgrad.{a}.fc1.weight"][:, args.obs_size:]
        assert np.all(np.delete(ids, a, axis=1) == 0.0)
        assert np.allclose(ids[:, a], gold[f"pgrad.{a}.fc1.bias"], atol=1e-8, rtol=1e-6)
        if gauss:
            assert np.abs(gold[f"pgrad.{a}.log_std.weight"]).max() > 0

    # one value step, then one policy step through PGTrainer
    th.manual_seed(0)
    trainer = PGTrainer(args, getattr(L, cls), StubEnv(n), None)
    net = trainer.behaviour_net
    net.load_state_dict(gauss_state_dict(prefix))
    stat = {}
    trainer.value_transition_process(stat, batch)
    trainer.policy_transition_process(stat, batch)
    keys = {k[5:] for k in gold if k.startswith("stat.")}
    assert keys == set(stat) == {"mean_train_value_loss", "mean_train_value_grad_norm", "mean_train_policy_loss",
                                 "mean_train_policy_grad_norm", "mean_train_entropy"}
    for k in keys:
        assert abs(float(stat[k]) - gold["stat." + k]) < 1e-4 * max(1.0, abs(gold["stat." + k])), k
    after = gauss_state_dict(prefix, "state_dict_after_step")
    mine = net.state_dict()
    assert sorted(mine) == sorted(after)
    for k, ref in after.items():
        assert th.allclose(mine[k].float(), ref.float(), atol=3e-6, rtol=1e-5), k
    init = golden_tensors(f"{prefix}_state_dict.npz")
    head = "mean" if gauss else ("fc3" if agent_type == "mlp" else "fc2")
    for a in range(n):
        assert (mine[f"policy_dicts.{a}.{head}.weight"] - init[f"policy_dicts.{a}.{head}.weight"]).abs().max() > 0
    assert dict(FALLBACKS) == noted                                      # the CPU takes the loop and notes nothing


def test_fixture_files_are_within_the_committed_size_limit():
    g = os.path.join(ROOT, "tests", "golden", "per_agent")
    files = sorted(os.listdir(g))
    assert len(files) == 16 and {f.rsplit("_", 1)[0] for f in files if f.endswith("_args.json")} == {f[0] for f in FAMILIES}
    assert all(os.path.getsize(os.path.join(g, f)) < (1 << 20) for f in files)
