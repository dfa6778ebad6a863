"""agent_type mlp on CPU: golden vectors captured by importing the reference's MADDPG / IPPO with the actors of
madrl/agents/mlp_agent.py and mlp_agent_gaussian.py (tests/golden/make_mlp_golden.py) — strict state_dict loads, ``policy()``,
both losses, every gradient, ``stat`` and the weights after one value and one policy step, with the tolerances
tests/test_gaussian_cpu.py uses for the same quantities.  The agent runs as the tensor composition; the fixtures pin the host
classes, MLPAgentGaussian as a subclass of MLPAgent included."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch as th

from .golden_io import StubEnv, golden_args, golden_batch, golden_model, golden_tensors, golden_vectors
from .test_gaussian_cpu import assert_grads, gauss_state_dict

FAMILIES = [("mlp_maddpg", "MADDPG"), ("mlp_ippo", "IPPO"), ("mlp_gauss_ippo", "IPPO")]
BATCH_FIELDS = {"mlp_maddpg": (), "mlp_ippo": ("action", "done", "last_step"), "mlp_gauss_ippo": ("action", "done", "last_step")}
HEADS = {False: ["fc3.weight", "fc3.bias"], True: ["mean.weight", "mean.bias", "log_std.weight", "log_std.bias"]}


def mlp_policy_loss(model, batch, entr):
    """The loss a policy sub-update steps on (trainer.py:47-57) and what get_loss returned."""
    from safe_marl_amd.util import normal_entropy
    pl, vl, (means, log_stds) = model.get_loss(batch)
    assert log_stds.requires_grad == bool(model.args.gaussian_policy)
    return pl - entr * normal_entropy(means, log_stds.exp()), pl, vl, means, log_stds


@pytest.mark.parametrize("prefix,cls", FAMILIES)
def test_golden_parity(prefix, cls):
    import safe_marl_amd.learner as L
    from safe_marl_amd.nets import MLPAgent, MLPAgentGaussian
    from safe_marl_amd.trainer import PGTrainer
    gold = golden_vectors(prefix)
    args = golden_args(prefix)
    gauss = prefix == "mlp_gauss_ippo"
    assert args.agent_type == "mlp" and bool(args.gaussian_policy) == gauss and args.shared_params
    model = golden_model(cls, args, gauss_state_dict(prefix))            # strict: the reference's names and shapes
    agent = model.policy_dicts[0]
    assert type(agent) is (MLPAgentGaussian if gauss else MLPAgent) and isinstance(agent, MLPAgent)
    assert [k for k, _ in agent.named_parameters()] == ["fc1.weight", "fc1.bias", "layernorm.weight", "layernorm.bias",
                                                        "fc2.weight", "fc2.bias"] + HEADS[gauss]
    assert list(agent.state_dict()) == [k for k, _ in agent.named_parameters()]
    assert agent.fc3 is (agent.mean if gauss else agent.fc3)             # the mean head sits in the fc3 slot
    batch = golden_batch(prefix, gold=gold, fields=BATCH_FIELDS[prefix])
    n = args.agent_num

    with th.no_grad():
        means, log_stds, hiddens = model.policy(batch.state, last_hid=batch.last_hid)
    assert log_stds.shape == means.shape == (32, n, 4) and hasattr(log_stds, "_flex_entropy") != gauss
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
    assert (mine["policy_dicts.0.fc2.weight"] - init["policy_dicts.0.fc2.weight"]).abs().max() > 0


def test_gaussian_fixture_of_the_mlp_agent_still_loads():
    """MLPAgentGaussian as a subclass keeps exactly the keys fc1, layernorm, fc2, mean, log_std."""
    from safe_marl_amd.nets import MLPAgent, MLPAgentGaussian
    args = golden_args("gauss_maddpg_mlp")
    model = golden_model("MADDPG", args, gauss_state_dict("gauss_maddpg_mlp"))
    agent = model.policy_dicts[0]
    assert isinstance(agent, MLPAgentGaussian) and isinstance(agent, MLPAgent)
    assert not any(k.startswith("fc3") for k in agent.state_dict())
    assert sorted({k.split(".")[0] for k in agent.state_dict()}) == ["fc1", "fc2", "layernorm", "log_std", "mean"]


def test_example_takes_the_agent_type():
    """examples/train_maddpg.py --agent-type {rnn,mlp}, default rnn (the parser runs before anything touches a GPU)."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, os.path.join(root, "examples", "train_maddpg.py"), "--help"], capture_output=True,
                         text=True, timeout=60)
    assert out.returncode == 0 and "--agent-type {rnn,mlp}" in out.stdout, out.stdout + out.stderr
    bad = subprocess.run([sys.executable, os.path.join(root, "examples", "train_maddpg.py"), "--agent-type", "gru"],
                         capture_output=True, text=True, timeout=60)
    assert bad.returncode == 2 and "invalid choice" in bad.stderr
