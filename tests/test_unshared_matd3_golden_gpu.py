"""GPU: MATD3 under ``shared_params: False`` through the PRODUCT path against the golden vectors of
tests/golden/make_unshared_matd3_golden.py (the reference's MATD3 with one RNNAgent and one twin-flag critic per agent, three
agents): the checks of tests/test_unshared_matd3_cpu.py on the device, batch tiled x1 and x64, then a cross-check against the
five-agent shared fixture and a short vectorised training run.

The golden batch has 32 samples; tile 64 makes it 2 048 samples = 6 144 critic rows, so the value loss and the first head's
policy pass come from the autograd node of csrc/critic_unshared_twin.hip (nets._CriticUnsharedTwinFn); at tile 1 they take the
per-agent loop, and the targets come from the no-grad launch at both.  Every loss is a mean over samples, so losses and
gradients are invariant under tiling; the recorded target-smoothing draws are tiled like the batch.

Tolerances on the device are the CPU test's own (tests/test_unshared_cpu.py's for the unshared_maddpg family), unchanged.  One
comparison is left out at tile 64 only, for a reason that is arithmetic and not precision: the BatchNorm's running_var takes the
unbiased n / (n - 1) factor of its batch, 2 048 samples there against the recorded run's 32."""
import copy
import os
import sys

import numpy as np
import pytest
import torch as th

from .golden_io import golden_args, golden_batch, golden_model
from .test_unshared_matd3_cpu import CPU_TOL, check_golden_parity

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("tile", [1, 64])
def test_golden_on_the_device(tile, monkeypatch):
    from safe_marl_amd import learner
    from safe_marl_amd.util import FALLBACKS
    declined = FALLBACKS.get("critic_unshared_twin", 0)
    nodes, launches = [], []
    real_train, real_forward = learner.critic_unshared_twin_train, learner.fused_critic_forward_unshared_twin

    def train(critics, obs, act, heads, **k):
        q = real_train(critics, obs, act, heads, **k)
        nodes.append((heads, k.get("param_grads", True), tuple(q.shape)))
        return q

    def forward(*a, **k):
        q = real_forward(*a, **k)
        launches.append(q is not None)
        return q
    monkeypatch.setattr(learner, "critic_unshared_twin_train", train)
    monkeypatch.setattr(learner, "fused_critic_forward_unshared_twin", forward)
    model = check_golden_parity(monkeypatch, "cuda", tile, CPU_TOL if tile == 1 else dict(CPU_TOL, batchnorm=False))
    assert model.graph_safe_updates is False
    assert launches and all(launches)                        # value() under no_grad and every bootstrap target
    b = 32 * tile
    if tile == 1:
        assert not nodes                                     # 96 critic rows with a graph: the loop, silently
    else:
        # get_loss: the value loss (both heads); need="value": the same; need="policy": the first head, frozen; the trainer's
        # value step and its policy step
        print("nodes", nodes)
        assert set(nodes) == {(2, True, (2, b, 3)), (1, False, (1, b, 3))}
        assert nodes.count((2, True, (2, b, 3))) >= 3 and nodes.count((1, False, (1, b, 3))) >= 2
    assert FALLBACKS.get("critic_unshared_twin", 0) == declined


def test_copies_of_the_shared_critic_agree_with_the_shared_model():
    """The five-agent shared fixture's one critic in all five per-agent critics of an unshared MATD3: the same values."""
    from safe_marl_amd.learner import MATD3
    shared = golden_model(MATD3, golden_args(cuda=True), "matd3_state_dict.npz", "cuda")
    args = golden_args(cuda=True, shared_params=False)
    th.manual_seed(5)
    model = MATD3(args, MATD3(args).cuda()).cuda()
    assert len(model.value_dicts) == 5 and len(shared.value_dicts) == 1
    for c in model.value_dicts:
        c.load_state_dict(copy.deepcopy(shared.value_dicts[0].state_dict()))
    batch = golden_batch("learner", "cuda")
    with th.no_grad():
        want = shared.value(batch.state, batch.action)
        got = model.value(batch.state, batch.action)
        model.fused_inference = False
        loop = model.value(batch.state, batch.action)
    bound = 2e-5 * max(1.0, want.abs().max().item())
    print(f"unshared copies against the shared model: launch {(got - want).abs().max().item():.3e}, "
          f"loop {(loop - want).abs().max().item():.3e}, bound {bound:.3e}")
    assert got.shape == want.shape == (64, 5, 1)
    assert (got - want).abs().max().item() <= bound and (loop - want).abs().max().item() <= bound
    assert (got[:32] - got[32:]).abs().max().item() > 0          # the flag column matters


def test_two_update_events_of_unshared_twin_training(monkeypatch):
    """examples/train_maddpg.py's machinery with --alg matd3 --unshared-twins: 64 environments x 3 agents, two episodes with an
    update event in each, on batches of 1 024 samples = 3 072 critic rows — the node's branch."""
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    from train_maddpg import DEFAULT_ALG_ARGS
    from safe_marl_amd import learner
    from safe_marl_amd.flex_env import VecFlexProvisionEnv
    from safe_marl_amd.network import create_network
    from safe_marl_amd.series import make_synthetic_series
    from safe_marl_amd.trainer import PGTrainer
    from safe_marl_amd.util import FALLBACKS, convert
    N, blds = 64, [5, 15, 25]
    env_args = {"buildings": blds, "pv_nodes": blds, "ess_nodes": blds}
    net_ = create_network(env_args)
    env = VecFlexProvisionEnv(env_args, N, net=net_, series=make_synthetic_series(net_, n_days=30), seed=4, warm_start=True)
    a = dict(DEFAULT_ALG_ARGS)
    a.update(alg="matd3", agent_num=env.n_agents, obs_size=env.obs_size, state_size=env.state_size, action_dim=4,
             shared_params=False, behaviour_update_freq=60, target_update_freq=120, batch_size=64)
    noted = {k: v for k, v in FALLBACKS.items() if "unshared" in k}
    nodes = []
    real = learner.critic_unshared_twin_train

    def train(critics, obs, act, heads, **k):
        nodes.append((heads, k.get("param_grads", True), obs.shape[0] * obs.shape[1]))
        return real(critics, obs, act, heads, **k)
    monkeypatch.setattr(learner, "critic_unshared_twin_train", train)
    th.manual_seed(3)
    np.random.seed(3)
    tr = PGTrainer(convert(a), learner.MATD3, env, None, replay_capacity=N * 96 * 2)
    net = tr.behaviour_net
    assert env.n_agents == 3 and len(net.policy_dicts) == len(net.value_dicts) == 3 and net.graph_safe_updates is False
    assert all(c.fc1.in_features == 3 * (env.obs_size + 4) + 3 + 1 for c in net.value_dicts)
    w0 = {k: v.detach().clone() for k, v in net.state_dict().items() if k.startswith(("policy_dicts.", "value_dicts."))}
    for _ in range(2):
        stat = {}
        net.train_process(stat, tr)                                # 95 vector steps: one update event, at step 60
        th.cuda.synchronize()
        for k in ("mean_train_value_loss", "mean_train_policy_loss", "mean_train_policy_grad_norm", "mean_train_value_grad_norm",
                  "mean_train_entropy", "mean_train_reward"):
            assert np.isfinite(float(stat[k])), (k, stat)
        assert float(stat["mean_train_policy_grad_norm"]) > 0 and float(stat["mean_train_value_grad_norm"]) > 0
    cur = net.state_dict()
    for k, v in w0.items():                                        # every agent's actor and critic moved
        assert th.isfinite(cur[k]).all() and not th.equal(cur[k], v), k
    assert nodes and all(rows == 3072 for _, _, rows in nodes)
    assert {(h, pg) for h, pg, _ in nodes} == {(2, True), (1, False)}
    assert {k: v for k, v in FALLBACKS.items() if "unshared" in k} == noted
