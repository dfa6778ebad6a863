"""The MLP actors (csrc/actor_mlp.hip: nets.fused_actor_forward_mlp and the training node nets.actor_mlp_train;
csrc/actor_mlp.hip's per-agent form: nets.fused_actor_forward_mlp_unshared and nets.actor_mlp_unshared_train) against the fp64 copies
of the modules, on tests/fp64_budget.py's error budget and its families for a module with its own first layer: ``constant``
is fc1.weight = 0 with one inexact bias value, so that every row's 64 LayerNorm inputs are equal bit for bit.  The figures of a
run are filed in profiles/fp64_error_budget.txt."""
import functools

import pytest
import torch as th

from . import fp64_budget as fb

pytestmark = pytest.mark.gpu

INFERENCE = [(13, 5, 144, 4), (7, 3, 72, 2)]       # 65 rows: two full 32-row tiles and one row; 21 rows: one part-filled tile
# the training nodes take whatever the inference launches take (nets.actor_mlp_declines / actor_mlp_unshared_declines: rows a
# multiple of n, from one sample on; the row threshold of the weight-gradient kernels is the dispatch's, not the nodes'): one
# sample, a tile that holds a single row per agent module
TRAINING = INFERENCE + [(1, 2, 6, 2)]
FAMILIES = ("plain", "reset", "offset", "constant", "dead", "mixed")
KINDS = ("shared", "unshared")


def case_inputs(kind, b, n, obs_dim, act, family, device):
    """(agents: one module or n, family, obs [b, n, o], upstream of the means) on ``device``, drawn from the CPU generator: the
    same numbers wherever the case runs, so that tests/test_fp64_budget_cpu.py holds the tie share of these very inputs."""
    rows = b * n
    g = th.Generator().manual_seed(rows + act + 5)
    fam = fb.families(rows, n, obs_dim, g, kind="mlp")[family]
    fam = fam._replace(inputs=tuple(t.to(device) for t in fam.inputs), groups=None if fam.groups is None else fam.groups.to(device))
    if kind == "shared":
        agents = fb.make_mlp_agent(obs_dim, n, act, device=device, seed=3)
    else:
        agents = [fb.make_mlp_agent(obs_dim, n, act, device=device, seed=10 + i) for i in range(n)]
    fb.apply_params(agents, fam)
    up = (th.randn(rows, act, generator=g) / rows).to(device)
    return agents, fam, fam.inputs[0].view(b, n, obs_dim), up


def plain(agents, obs, dtype):
    """The composition on obs [b, n, o]: (means, h, first pre-activation, second) as [b * n, .], rows sample-major."""
    b, n, o = obs.shape
    if not isinstance(agents, list):
        return fb.mlp_actor_plain(agents, obs.reshape(b * n, o).to(dtype), n)
    outs = [fb.mlp_actor_plain(ag, obs[:, i].to(dtype), n, agent_index=i) for i, ag in enumerate(agents)]
    return tuple(th.stack([o_[k] for o_ in outs], 1).reshape(b * n, -1) for k in range(4))


def named(agents):
    if not isinstance(agents, list):
        return dict(agents.named_parameters())
    return {f"{i}.{k}": p for i, ag in enumerate(agents) for k, p in ag.named_parameters()}


@pytest.fixture(scope="module", autouse=True)
def _release_cases():
    """The cached cases hold GPU tensors: let them go with this file."""
    yield
    _case.cache_clear()
    th.cuda.empty_cache()


@functools.lru_cache(maxsize=None)
def _case(kind, b, n, obs_dim, act, family):
    agents, fam, obs, up = case_inputs(kind, b, n, obs_dim, act, family, "cuda")
    a64 = fb.ref64(agents)
    share = fb.clear_ties(lambda o: plain(a64, o, th.float64)[2:], (obs,), [up])
    t32 = fb.run_with_grads(lambda: plain(agents, obs, th.float32)[:2], named(agents), [up, None])
    r64 = fb.run_with_grads(lambda: plain(a64, obs, th.float64)[:2], named(a64), [up.double(), None])
    return agents, fam, obs, up, share, t32, r64


@pytest.mark.parametrize("b,n,obs_dim,act", INFERENCE)
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("kind", KINDS)
def test_inference_launch_within_budget(kind, family, b, n, obs_dim, act):
    from safe_marl_amd import nets
    agents, fam, obs, _, _, t32, r64 = _case(kind, b, n, obs_dim, act, family)
    out = nets.fused_actor_forward_mlp(agents, obs, n, True) if kind == "shared" else nets.fused_actor_forward_mlp_unshared(agents, obs)
    assert out is not None
    tag = f"actor_mlp_{kind}_forward {family} {b}x{n}x{obs_dim}x{act}"
    groups = [("", slice(None))]
    if fam.groups is not None:
        groups += [(f"[{nm} rows]", fam.groups == j) for j, nm in enumerate(fb.MIXED_OF["mlp"])]
    for sub, rows in groups:
        for k, nm in enumerate(("means", "h")):
            assert th.isfinite(out[k][rows]).all(), (tag, nm)
            fb.within_budget(out[k][rows], t32[0][k][rows], r64[0][k][rows], name=f"{tag} {nm}{sub}")


@pytest.mark.parametrize("b,n,obs_dim,act", TRAINING)
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("kind", KINDS)
def test_training_node_within_budget(kind, family, b, n, obs_dim, act):
    from safe_marl_amd import nets
    agents, fam, obs, up, share, t32, r64 = _case(kind, b, n, obs_dim, act, family)
    assert share <= fb.TIE_CAP
    if kind == "shared":
        assert nets.actor_mlp_declines(agents, obs, n, True) is None
    else:
        assert nets.actor_mlp_unshared_declines(agents, obs, True) is None

    def fused():
        means, h = nets.actor_mlp_train(agents, obs, n, True) if kind == "shared" else nets.actor_mlp_unshared_train(agents, obs)
        assert "TrainFn" in type(means.grad_fn).__name__                        # the HIP node, not a composition
        return means, h

    kern = fb.run_with_grads(fused, named(agents), [up, None])
    tag = f"actor_mlp_{kind}_train {family} {b}x{n}x{obs_dim}x{act}"
    groups = [("", slice(None))]
    if fam.groups is not None:
        groups += [(f"[{nm} rows]", fam.groups == j) for j, nm in enumerate(fb.MIXED_OF["mlp"])]
    for sub, rows in groups:
        for k, nm in enumerate(("means", "h")):
            assert th.isfinite(kern[0][k][rows]).all(), (tag, nm)
            fb.within_budget(kern[0][k][rows], t32[0][k][rows], r64[0][k][rows], name=f"{tag} {nm}{sub}")
    for nm, g64 in r64[1].items():
        assert th.isfinite(kern[1][nm]).all(), (tag, nm)
        fb.within_budget(kern[1][nm], t32[1][nm], g64, name=f"{tag} d_{nm}")
