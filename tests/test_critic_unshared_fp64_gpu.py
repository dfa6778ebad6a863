"""The per-agent critics of shared_params False (csrc/critic_unshared.hip: nets.fused_critic_forward_unshared and the training
node nets.critic_unshared_train, with and without parameter gradients) against the fp64 copies of the modules on their
materialised input rows, on tests/fp64_budget.py's error budget and its families for a module with its own first layer.  The
node hands out no dz1; fc1's gradients and the own-action gradient carry it.  The vector-sum gradients (biases, LayerNorm's
pair, fc3.weight) are sums over an agent's b rows of terms that cancel: their floor is fb.row_sum_rounding's, derived there.
The figures of a run are filed in profiles/fp64_error_budget.txt."""
import functools

import pytest
import torch as th

from . import fp64_budget as fb

pytestmark = pytest.mark.gpu

# 33: a full 32-row tile and one that holds a single row; 64: two full tiles, the widest first layer of the workload (745
# columns in MADDPG's form); 257: a third work-group per agent whose only tile holds one row
SHAPES = [(33, 3, 30, 2), (64, 5, 144, 4), (257, 3, 6, 4)]
FORMS = ("maddpg", "ippo")
FAMILIES = ("plain", "reset", "offset", "constant", "dead")


def case_inputs(form, b, n, obs_dim, act_dim, family, device):
    """(critics, family, obs [b, n, o], act [b, n, a] or None, upstream of q [b, n]) on ``device``, drawn from the CPU generator:
    the same numbers wherever the case runs, so that tests/test_fp64_budget_cpu.py holds the tie share of these very inputs."""
    shared, has_act = fb.CRITIC_FORMS[form]
    g = th.Generator().manual_seed(b * n + act_dim + len(form))
    fam = fb.families(b * n, n, obs_dim, g, kind="mlp")[family]
    fam = fam._replace(inputs=tuple(t.to(device) for t in fam.inputs))
    width = obs_dim * (n if shared else 1) + n + (act_dim * (n if shared else 1) if has_act else 0)
    critics = [fb.make_critic(True, device, seed=40 + i, in_features=width) for i in range(n)]
    fb.apply_params(critics, fam)
    act = None
    if has_act:
        act = (0.5 * th.randn(b, n, act_dim, generator=g)).to(device)
        if family == "reset":
            act.zero_()
    up = (th.randn(b, n, generator=g) / (b * n)).to(device)
    return critics, fam, fam.inputs[0].view(b, n, obs_dim), act, up


def plain(critics, obs, act, form, dtype):
    """The per-agent loop on materialised rows: (q [b, n], first pre-activation, second: [b n, 64] each, rows sample-major)."""
    b, n, _ = obs.shape
    outs = [fb.critic_plain(c, fb.critic_rows(obs.to(dtype), None if act is None else act.to(dtype), i, form))
            for i, c in enumerate(critics)]
    return (th.stack([o[0][:, 0] for o in outs], 1),) + tuple(th.stack([o[k] for o in outs], 1).reshape(b * n, -1) for k in (1, 2))


def named(critics, act):
    out = {f"{i}.{k}": p for i, c in enumerate(critics) for k, p in c.named_parameters()}
    if act is not None:
        out["act"] = act
    return out


def reference(critics, obs, act, form, up, dtype):
    """((q detached,), {name: gradient}, {name: fb.row_sum_rounding floor of a vector-sum gradient} — the fp64 run's alone) of
    the composition in ``dtype``; the actions' gradient under "act".  An agent's sums run over its own b rows."""
    a = None if act is None else act.detach().to(dtype).requires_grad_(True)
    outs = [fb.critic_plain(c, fb.critic_rows(obs.to(dtype), a, i, form)) for i, c in enumerate(critics)]
    q = th.stack([o[0][:, 0] for o in outs], 1)
    loss = (q * up.to(dtype)).sum()
    floors = {}
    if dtype == th.float64:
        for i, (c, (q_i, pre1, pre2)) in enumerate(zip(critics, outs)):
            g_q, g1, g2 = th.autograd.grad(loss, [q_i, pre1, pre2], retain_graph=True)
            floors.update({f"{i}.{k}": v for k, v in fb.tail_sum_floors(g_q, g1, g2, pre1, pre2, c.layernorm).items()})
    params = named(critics, a)
    grads = th.autograd.grad(loss, list(params.values()), allow_unused=True)
    return (q.detach(),), dict(zip(params, grads)), floors


@pytest.fixture(scope="module", autouse=True)
def _release_cases():
    """The cached cases hold GPU tensors: let them go with this file."""
    yield
    _case.cache_clear()
    th.cuda.empty_cache()


@functools.lru_cache(maxsize=None)
def _case(form, b, n, obs_dim, act_dim, family):
    critics, fam, obs, act, up = case_inputs(form, b, n, obs_dim, act_dim, family, "cuda")
    c64 = fb.ref64(critics)
    share = fb.clear_ties(lambda o, a: plain(c64, o, a, form, th.float64)[1:], (obs, act), [up])
    t32 = reference(critics, obs, act, form, up, th.float32)
    r64 = reference(c64, obs, act, form, up, th.float64)
    return critics, obs, act, up, share, t32, r64


@pytest.mark.parametrize("b,n,obs_dim,act_dim", SHAPES)
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("form", FORMS)
def test_inference_launch_within_budget(form, family, b, n, obs_dim, act_dim):
    from safe_marl_amd.nets import fused_critic_forward_unshared
    critics, obs, act, _, _, t32, r64 = _case(form, b, n, obs_dim, act_dim, family)
    q = fused_critic_forward_unshared(critics, obs, act, fb.CRITIC_FORMS[form][0])
    assert q is not None and th.isfinite(q).all()
    fb.within_budget(q, t32[0][0], r64[0][0], name=f"critic_unshared_forward {form} {family} {b}x{n}x{obs_dim}x{act_dim} q")


@pytest.mark.parametrize("b,n,obs_dim,act_dim", SHAPES)
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("form", FORMS)
def test_training_node_within_budget(form, family, b, n, obs_dim, act_dim):
    from safe_marl_amd.nets import critic_unshared_train
    critics, obs, act, up, share, t32, r64 = _case(form, b, n, obs_dim, act_dim, family)
    assert share <= fb.TIE_CAP
    shared = fb.CRITIC_FORMS[form][0]
    tag = f"critic_unshared_train {form} {family} {b}x{n}x{obs_dim}x{act_dim}"

    def run(param_grads):
        a = None if act is None else act.detach().clone().requires_grad_(True)

        def fused():
            q = critic_unshared_train(critics, obs, a, shared, param_grads=param_grads)
            assert "CriticUnsharedFn" in type(q.grad_fn).__name__                # the HIP node, not a composition
            return (q,)
        return fb.run_with_grads(fused, named(critics, a), [up])

    kern = run(True)
    assert th.isfinite(kern[0][0]).all()
    fb.within_budget(kern[0][0], t32[0][0], r64[0][0], name=f"{tag} q")
    for nm, g64 in r64[1].items():
        assert th.isfinite(kern[1][nm]).all(), (tag, nm)
        fb.within_budget(kern[1][nm], t32[1][nm], g64, floor_ulps=fb.floor_ulps(r64[2].get(nm), g64), name=f"{tag} d_{nm}")
    if act is not None:                                    # frozen critics (the policy sub-update): the actions' gradient alone
        frozen = run(False)
        assert all(g is None for nm, g in frozen[1].items() if nm != "act")
        assert th.isfinite(frozen[1]["act"]).all()
        fb.within_budget(frozen[0][0], t32[0][0], r64[0][0], name=f"{tag} frozen q")
        fb.within_budget(frozen[1]["act"], t32[1]["act"], r64[1]["act"], name=f"{tag} frozen d_act")
