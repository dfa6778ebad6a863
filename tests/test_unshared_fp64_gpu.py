"""The per-agent actors of shared_params False (csrc/actor_unshared.hip: nets.fused_actor_forward_unshared and the training
node nets.actor_unshared_train) against the fp64 copies of the per-agent modules, on tests/fp64_budget.py's error budget and
input families; the saturated family runs through the kernel's own sigmoid, 1 / (1 + expf(-x)).  The figures of a run are
filed in profiles/fp64_error_budget.txt."""
import functools

import pytest
import torch as th

from . import fp64_budget as fb

pytestmark = pytest.mark.gpu

SHAPES = [(13, 5, 144, 4), (417, 5, 144, 4), (1025, 2, 30, 2)]      # 65 rows; 2 085 and 2 050: what the training node accepts
FAMILIES = ("plain", "reset", "saturated", "mixed", "offset", "constant", "dead")


def _per_agent(agents, obs, hid, dtype):
    """The per-agent loop of model.py:124-138 on obs [b, n, o] / hid [b, n, 64]: (means, hidden, pre-activation) as [b * n, .]."""
    n = len(agents)
    outs = [fb.actor_plain(ag, obs[:, i].to(dtype), hid[:, i].to(dtype), n, agent_index=i) for i, ag in enumerate(agents)]
    return tuple(th.stack([o[k] for o in outs], 1).reshape(obs.shape[0] * n, -1) for k in range(3))


def _named(agents):
    return {f"{i}.{k}": p for i, ag in enumerate(agents) for k, p in ag.named_parameters()}


@pytest.fixture(scope="module", autouse=True)
def _release_cases():
    """The cached cases hold GPU tensors: let them go with this file."""
    yield
    _case.cache_clear()
    th.cuda.empty_cache()


@functools.lru_cache(maxsize=None)
def _case(b, n, obs_dim, act, family):
    rows = b * n
    g = th.Generator(device="cuda").manual_seed(rows + act)
    fam = fb.families(rows, n, obs_dim, g)[family]
    agents = fb.apply_params([fb.make_agent(obs_dim, n, act, device="cuda", seed=10 + i) for i in range(n)], fam)
    a64 = fb.ref64(agents)
    obs, hid = fam.inputs[0].view(b, n, obs_dim), fam.inputs[1].view(b, n, 64)
    up = [th.randn(rows, act, device="cuda", generator=g) / rows, None]
    share = fb.clear_ties(lambda o, h: [_per_agent(a64, o, h, th.float64)[2]], (obs, hid), up[:1])
    t32 = fb.run_with_grads(lambda: _per_agent(agents, obs, hid, th.float32)[:2], _named(agents), up)
    r64 = fb.run_with_grads(lambda: _per_agent(a64, obs, hid, th.float64)[:2], _named(a64), [up[0].double(), None])
    return agents, fam, obs, hid, up, share, t32, r64


@pytest.mark.parametrize("b,n,obs_dim,act", SHAPES)
@pytest.mark.parametrize("family", FAMILIES)
def test_inference_launch_within_budget(family, b, n, obs_dim, act):
    from safe_marl_amd.nets import fused_actor_forward_unshared
    agents, fam, obs, hid, _, _, t32, r64 = _case(b, n, obs_dim, act, family)
    out = fused_actor_forward_unshared(agents, obs, hid)
    assert out is not None
    tag = f"actor_unshared_forward {family} {b}x{n}x{obs_dim}x{act}"
    groups = [("", slice(None))]
    if fam.groups is not None:
        groups += [(f"[{nm} rows]", fam.groups == j) for j, nm in enumerate(fb.MIXED_OF["actor"])]
    for sub, rows in groups:
        for k, nm in enumerate(("means", "hidden")):
            assert th.isfinite(out[k][rows]).all(), (tag, nm)
            fb.within_budget(out[k][rows], t32[0][k][rows], r64[0][k][rows], name=f"{tag} {nm}{sub}")


@pytest.mark.parametrize("b,n,obs_dim,act", SHAPES[1:])
@pytest.mark.parametrize("family", FAMILIES)
def test_training_node_within_budget(family, b, n, obs_dim, act):
    from safe_marl_amd import nets
    agents, fam, obs, hid, up, share, t32, r64 = _case(b, n, obs_dim, act, family)
    assert share <= fb.TIE_CAP
    assert nets.actor_unshared_supported(agents, obs, True)

    def fused():
        means, h = nets.actor_unshared_train(agents, obs, hid)
        assert "ActorUnsharedTrainFn" in type(means.grad_fn).__name__          # the HIP node, not a composition
        return means, h

    kern = fb.run_with_grads(fused, _named(agents), up)
    tag = f"actor_unshared_train {family} {b}x{n}x{obs_dim}x{act}"
    for k, nm in enumerate(("means", "hidden")):
        fb.within_budget(kern[0][k], t32[0][k], r64[0][k], name=f"{tag} {nm}")
    for nm, g64 in r64[1].items():
        assert th.isfinite(kern[1][nm]).all(), (tag, nm)
        fb.within_budget(kern[1][nm], t32[1][nm], g64, name=f"{tag} d_{nm}")
