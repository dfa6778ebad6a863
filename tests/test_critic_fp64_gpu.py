"""The centralised critic's kernels (csrc/critic.hip) against the fp64 evaluation of nets.MLPCritic's tail, on
tests/fp64_budget.py's error budget and input families: the stored and the composed first-layer input, the VALU and the
matrix-core kernels, the dz1-only backward and the backward with parameter gradients on 16-row and 32-row tiles, and the
value loss with the critic's whole backward in one pass (flexnet_critic_td_backward).  The figures of a run are filed in
profiles/fp64_error_budget.txt."""
import copy
import functools

import pytest
import torch as th
import torch.nn as nn

from . import fp64_budget as fb

pytestmark = pytest.mark.gpu

FAMILIES = ("plain", "offset", "constant", "dead", "mixed")
MFMA_ROWS = 65536 + 37                     # csrc/critic.hip CRITIC_MFMA_MIN_ROWS = 65 536: above it the matrix-core kernels
# (rows, CRITIC_VARIANT, backward): "dz1" the critic frozen, "pgrad16" / "pgrad32" parameter gradients with CRITIC_PGRAD32 0 / 1
TAIL_CASES = [(rows, v, mode) for rows in (1, 37, 4099) for v in (0, 1) for mode in ("dz1", "pgrad16")] + \
             [(MFMA_ROWS, 0, "dz1"), (MFMA_ROWS, 0, "pgrad16"), (MFMA_ROWS, 0, "pgrad32"), (MFMA_ROWS, 1, "dz1"), (MFMA_ROWS, 1, "pgrad16")]
COMPOSED_CASES = [(0, "pgrad16"), (0, "pgrad32"), (1, "pgrad16")]


def _tail_params(c):
    return {k: p for k, p in c.named_parameters() if not k.startswith("fc1")}


@pytest.fixture(scope="module", autouse=True)
def _release_cases():
    """The cached cases hold GPU tensors (65 573 x 64 in fp32 and fp64 per family): let them go with this file."""
    yield
    _tail_case.cache_clear()
    _composed_case.cache_clear()
    th.cuda.empty_cache()


@functools.lru_cache(maxsize=None)
def _tail_case(family, rows):
    """Critic, input, upstream gradient (ties cleared over both ReLU layers) and the two references of one stored-input case."""
    g = th.Generator(device="cuda").manual_seed(rows)
    fam = fb.families(rows, 1, None, g)[family]
    critic = fb.apply_params(fb.make_critic(device="cuda"), fam)
    z = fam.inputs[0]
    up = th.randn(rows, 1, device="cuda", generator=g)
    c64 = fb.ref64(critic)
    share = fb.clear_ties(c64, (z.double(),), up)

    def run(c, dtype):
        zz = z.clone().to(dtype).requires_grad_(True)
        return fb.run_with_grads(lambda: (fb.critic_tail_plain(c, zz)[0],), dict(z=zz, **_tail_params(c)), [up.to(dtype)])

    return critic, z, up, share, run(critic, th.float32), run(c64, th.float64)


@pytest.mark.parametrize("rows,variant,mode", TAIL_CASES)
@pytest.mark.parametrize("family", FAMILIES)
def test_tail_on_a_stored_input_within_budget(family, rows, variant, mode, monkeypatch):
    """MLPCritic.forward_from_hidden (need_hidden=False) = CriticTail.apply: q, dz1 and the six tail gradients."""
    from safe_marl_amd import nets
    critic, z, up, share, t32, r64 = _tail_case(family, rows)
    assert share <= fb.TIE_CAP
    monkeypatch.setattr(nets, "CRITIC_VARIANT", variant)
    monkeypatch.setattr(nets, "CRITIC_PGRAD32", 1 if mode == "pgrad32" else 0)
    if mode == "dz1":                                   # a frozen copy: the cached critic is shared and stays as it is
        critic = copy.deepcopy(critic).requires_grad_(False)
    params = _tail_params(critic) if mode != "dz1" else {}
    zz = z.clone().requires_grad_(True)

    def fused():
        q, none = critic.forward_from_hidden(zz, need_hidden=False)
        assert none is None and "CriticTailFn" in type(q.grad_fn).__name__
        return (q,)

    kern = fb.run_with_grads(fused, dict(z=zz, **params), [up])
    tag = f"critic_tail[v{variant} {mode}] {family} {rows}"
    fb.within_budget(kern[0][0], t32[0][0], r64[0][0], name=f"{tag} q")
    if family == "dead":
        assert not r64[1]["z"].any() and not kern[1]["z"].any()          # every first-layer unit off: dz1 rows exactly zero
    for nm, g in kern[1].items():
        assert th.isfinite(g).all(), (tag, nm)
        fb.within_budget(g, t32[1][nm], r64[1][nm], name=f"{tag} d_{nm}")


@functools.lru_cache(maxsize=None)
def _composed_case(family, b, n):
    g = th.Generator(device="cuda").manual_seed(b + n)
    fam = fb.families(b, 1, None, g)[family]
    critic = fb.apply_params(fb.make_critic(device="cuda"), fam)
    shared = fam.inputs[0]
    ids = 0.3 * th.randn(n, 64, device="cuda", generator=g)
    if family == "constant":                    # an agent's id column equal in every unit: the composed rows stay constant
        ids = ids[:, :1].expand(n, 64).contiguous()
    up = th.randn(b * n, 1, device="cuda", generator=g)
    c64 = fb.ref64(critic)
    compose = lambda s, i: (s.unsqueeze(1) + i.unsqueeze(0)).reshape(b * n, 64)
    share = fb.clear_ties(lambda s, i: fb.critic_tail_plain(c64, compose(s, i))[1:], (shared.double(), ids.double()), up)

    def run(c, dtype):
        s, i = shared.clone().to(dtype).requires_grad_(True), ids.clone().to(dtype).requires_grad_(True)
        return fb.run_with_grads(lambda: (fb.critic_tail_plain(c, compose(s, i))[0],), dict(shared=s, ids=i, **_tail_params(c)),
                                 [up.to(dtype)])

    return critic, shared, ids, up, share, run(critic, th.float32), run(c64, th.float64)


@pytest.mark.parametrize("variant,mode", COMPOSED_CASES)
@pytest.mark.parametrize("b,n", [(13108, 5), (21846, 3)])
@pytest.mark.parametrize("family", FAMILIES)
def test_tail_on_the_composed_input_within_budget(family, b, n, variant, mode, monkeypatch):
    """CriticTail.apply_composed, z1[b, i] = shared[b] + id_cols[i] formed in the kernels: q, d_shared, d_ids and the six tail
    gradients; 65 540 and 65 538 rows, so variant 0 is the matrix-core kernels with a ragged last tile."""
    from safe_marl_amd import nets
    critic, shared, ids, up, share, t32, r64 = _composed_case(family, b, n)
    assert share <= fb.TIE_CAP
    monkeypatch.setattr(nets, "CRITIC_VARIANT", variant)
    monkeypatch.setattr(nets, "CRITIC_PGRAD32", 1 if mode == "pgrad32" else 0)
    s, i = shared.clone().requires_grad_(True), ids.clone().requires_grad_(True)
    kern = fb.run_with_grads(lambda: (nets.CriticTail.apply_composed(s, i, critic),), dict(shared=s, ids=i, **_tail_params(critic)), [up])
    tag = f"critic_composed[v{variant} {mode}] {family} {b}x{n}"
    fb.within_budget(kern[0][0], t32[0][0], r64[0][0], name=f"{tag} q")
    if family == "dead":
        assert not kern[1]["shared"].any() and not kern[1]["ids"].any()
    for nm, g in kern[1].items():
        assert th.isfinite(g).all(), (tag, nm)
        fb.within_budget(g, t32[1][nm], r64[1][nm], name=f"{tag} d_{nm}")


@pytest.mark.parametrize("norm", [True, False], ids=["batchnorm", "raw-reward"])
def test_value_loss_with_the_critic_backward_in_one_pass_within_budget(norm):
    """MADDPG._critic_td_loss (nets._CriticTdLossFn, flexnet_critic_td_backward) at 5 x 13 108 = 65 540 critic rows: the loss
    and every critic parameter gradient against the fp64 evaluation of td_loss(value(...)).  The upstream gradient is the
    loss's own, so samples with a ReLU tie are not cleared but replaced by an untied sample."""
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))
    from train_maddpg import DEFAULT_ALG_ARGS
    from safe_marl_amd import learner, nets
    from safe_marl_amd.util import convert, unit_seed
    b, n = 13108, 5
    alg = dict(DEFAULT_ALG_ARGS)
    alg.update(alg="maddpg", agent_num=n, obs_size=144, state_size=110, action_dim=4)
    th.manual_seed(4)
    m = learner.MADDPG(convert(alg)).cuda()
    with th.no_grad():
        for p in m.value_dicts.parameters():
            p.copy_(th.randn_like(p) * 0.1)
    net = m.value_dicts[0]
    g = th.Generator(device="cuda").manual_seed(b)
    obs = th.randn(b, n, 144, device="cuda", generator=g)
    act = th.randn(b, n, 4, device="cuda", generator=g)
    nq = th.randn(b, n, device="cuda", generator=g)
    rew = th.randn(b, n, device="cuda", generator=g) * 3.0 + 1.0
    done = (th.rand(b, 1, device="cuda", generator=g) < 0.05).float()
    n64 = fb.ref64(net)

    def value(c, dtype):
        z = fb.critic_first_layer_plain(c, obs.reshape(b, -1).to(dtype), act.reshape(b, -1).to(dtype), n)
        return fb.critic_tail_plain(c, z)

    with th.no_grad():
        tie = fb.tie_rows(value(n64, th.float64)[1:]).view(b, n)
        assert float(tie.double().mean()) <= fb.TIE_CAP           # the share of critic rows, as everywhere
        tie = tie.any(1)
        keep = int((~tie).nonzero()[0])
        obs[tie], act[tie] = obs[keep].clone(), act[keep].clone()
        assert not fb.tie_rows(value(n64, th.float64)[1:]).any()

    def plain(c, dtype):
        bn = nn.BatchNorm1d(n).cuda().to(dtype) if norm else None
        loss = fb.td_loss_plain(value(c, dtype)[0].view(b, n), nq.to(dtype), rew.to(dtype), done.to(dtype), m.args.gamma, bn)
        return loss, dict(zip(dict(c.named_parameters()), th.autograd.grad(loss, list(c.parameters()))))

    bn = nn.BatchNorm1d(n).cuda().train() if norm else None
    assert nets.critic_td_loss_supported(net, obs.reshape(b, -1), act.reshape(b, -1), n, nq, rew, done, bn)
    loss = m._critic_td_loss(obs, act, nq, rew, done, bn)
    assert type(loss.grad_fn).__name__ == "_CriticTdLossFnBackward"
    grads = dict(zip(dict(net.named_parameters()), th.autograd.grad(loss, list(net.parameters()), grad_outputs=unit_seed("cuda"))))
    l32, g32 = plain(net, th.float32)
    l64, g64 = plain(n64, th.float64)
    tag = f"critic_td_loss[{'batchnorm' if norm else 'raw reward'}] {b}x{n}"
    fb.within_budget(loss.view(1), l32.view(1), l64.view(1), name=f"{tag} loss")
    for nm, ref in g64.items():
        assert th.isfinite(grads[nm]).all(), (tag, nm)
        fb.within_budget(grads[nm], g32[nm], ref, name=f"{tag} d_{nm}")
