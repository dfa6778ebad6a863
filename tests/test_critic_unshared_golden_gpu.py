"""GPU: the per-agent critics of ``shared_params: False`` through the PRODUCT path against the golden vectors of
tests/golden/make_unshared_golden.py (the reference's MADDPG / IPPO with one RNNAgent and one MLPCritic per agent, three agents).

The golden batch has 32 samples; tile 64 makes it 2 048 samples = 6 144 critic rows, so every value tensor that carries a graph
comes from the autograd node of csrc/critic_unshared.hip (nets._CriticUnsharedFn) and the bootstrap targets from its no-grad
launch.  Every loss is a mean over samples, so losses and gradients are invariant under tiling (tests/test_unshared_golden_gpu.py).
Bounds are the existing golden ones: value gradients 2e-6 + 1e-4 max|golden|, the value loss 2e-4 relative, policy gradients —
MADDPG's reach the actors through the node's own-action gradient — within 2e-4 of each golden tensor's largest entry."""
import numpy as np
import pytest
import torch as th

from .golden_io import _np, golden_args, golden_model, golden_vectors
from .test_gaussian_cpu import gauss_state_dict
from .test_mlp_agent_cpu import mlp_policy_loss
from .test_unshared_cpu import FAMILIES
from .test_unshared_golden_gpu import _tiled_batch

pytestmark = pytest.mark.gpu
TILE = 64


@pytest.mark.parametrize("prefix,cls", FAMILIES)
def test_golden_losses_and_gradients_through_the_node(prefix, cls, monkeypatch):
    from safe_marl_amd import learner
    from safe_marl_amd.util import FALLBACKS
    gold = golden_vectors(prefix)
    args = golden_args(prefix, cuda=True)
    declined = FALLBACKS.get("critic_unshared", 0)
    batch = _tiled_batch(prefix, cls, gold, TILE)
    model = golden_model(cls, args, gauss_state_dict(prefix, device="cuda"), "cuda")
    if cls == "IPPO":
        model.gae_chain_stride = TILE
    nodes, launches = [], []
    real_train, real_forward = learner.critic_unshared_train, learner.fused_critic_forward_unshared

    def train(*a, **k):
        q = real_train(*a, **k)
        nodes.append(q)
        return q

    def forward(*a, **k):
        q = real_forward(*a, **k)
        launches.append(q is not None)
        return q
    monkeypatch.setattr(learner, "critic_unshared_train", train)
    monkeypatch.setattr(learner, "fused_critic_forward_unshared", forward)
    loss, pl, vl, means, log_stds = mlp_policy_loss(model, batch, args.entr)
    # the value tensors: MADDPG's policy loss and value loss, IPPO's value loss from the node; the targets from the launch
    assert len(nodes) == (2 if cls == "MADDPG" else 1) and launches and all(launches)
    assert all("CriticUnsharedFn" in type(q.grad_fn).__name__ and q.shape == (32 * TILE, args.agent_num) for q in nodes)
    ref = float(gold["value_loss"])
    print(f"{prefix} x{TILE}: value loss {vl.item():.8f} (golden {ref:.8f}), policy loss {pl.item():.8f} "
          f"(golden {float(gold['policy_loss']):.8f})")
    assert abs(vl.item() - ref) <= 2e-4 * max(1.0, abs(ref))
    names = [k for k, _ in model.value_dicts.named_parameters()]
    grads = th.autograd.grad(vl, list(model.value_dicts.parameters()), retain_graph=True)
    assert len(names) == 8 * args.agent_num
    for k, g in zip(names, grads):
        want = gold["vgrad." + k]
        err, bound = np.abs(_np(g) - want).max(), 2e-6 + 1e-4 * np.abs(want).max()
        print(f"{prefix} x{TILE} vgrad.{k}: error {err:.3e}, bound {bound:.3e}")
        assert err <= bound, (k, err, bound)
    if cls == "MADDPG":                                    # the policy loss differentiates the critics w.r.t. the own actions
        assert abs(pl.item() - float(gold["policy_loss"])) <= 1e-5 * max(1.0, abs(float(gold["policy_loss"])))
        names = [k for k, _ in model.policy_dicts.named_parameters()]
        grads = th.autograd.grad(loss, list(model.policy_dicts.parameters()))
        for k, g in zip(names, grads):
            want = gold["pgrad." + k]
            err, bound = np.abs(_np(g) - want).max(), 2e-4 * np.abs(want).max()
            print(f"{prefix} x{TILE} pgrad.{k}: error {err:.3e}, bound {bound:.3e}")
            assert err <= bound, (k, err, bound)
    assert FALLBACKS.get("critic_unshared", 0) == declined
