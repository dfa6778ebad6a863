"""GPU: every agent's own log-std head in one launch per direction (csrc/gauss.hip: flexnet_gauss_head_unshared_*;
nets._GaussHeadUnsharedFn) against the fp64 composition, and the per-agent RNN actors' node with the gradient the heads send to the
new hidden state (flexnet_actor_unshared_backward_hn; nets._ActorUnsharedTrainHidFn) against the fp64 per-agent module loop.

Bounds are tests/test_actor_mlp_gpu.py's ``_Bounds``: values 2e-5 max(1, max|ref|), gradients 2e-6 + 3e-4 max|ref|, or four times
the error of the fp32 composition on the device against the same fp64 reference where that is larger; every check prints which
applied."""
import copy
import itertools
import json
import os

import pytest
import torch as th
import torch.nn.functional as F

from .test_actor_mlp_gpu import SENTINEL, _Bounds, _guarded, _guards_untouched

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(__file__), "golden")
LO, HI = -1.5, 0.75


def _head_args(h, ws, bs, n, act_dim):
    from safe_marl_amd import _lib
    a = _lib.FlexGaussHeadUnsharedArgs()
    a.rows, a.n_agents, a.act_dim, a.hid = h.shape[0], n, act_dim, 64
    a.log_std_min, a.log_std_max = LO, HI
    for i in range(n):
        a.w[i], a.b[i] = ws[i].data_ptr(), bs[i].data_ptr()
    return a


def _composition(h, ws, bs, proj):
    """Row r = s n + i through head i, in the dtype of ``h`` [b, n, 64]: log_std, t, d_u, d_h of (log_std proj).sum()."""
    b, n, _ = h.shape
    h = h.detach().clone().requires_grad_()
    u = th.stack([h[:, i] @ ws[i].t() + bs[i] for i in range(n)], 1)
    u.retain_grad()
    t = th.tanh(u)
    log_std = LO + 0.5 * (HI - LO) * (t + 1)
    (log_std * proj).sum().backward()
    return dict(log_std=log_std.detach(), t=t.detach(), d_u=u.grad, d_h=h.grad)


CASES = [(b, n, act_dim, k % 2 == 0, (k // 2) % 2 == 0)
         for k, (b, n, act_dim) in enumerate(itertools.product([1, 33, 257], [1, 3, 8], [1, 4, 8]))]


def test_the_cases_cover_every_value():
    assert len(CASES) == 27 and {c[3] for c in CASES} == {c[4] for c in CASES} == {True, False}
    for n in (1, 3, 8):
        assert {(c[3], c[4]) for c in CASES if c[1] == n} == {(True, True), (True, False), (False, True), (False, False)}


@pytest.mark.parametrize("b,n,act_dim,want_t,want_dh", CASES)
def test_entry_points_against_the_composition(b, n, act_dim, want_t, want_dh):
    from safe_marl_amd import _lib
    g = th.Generator(device="cuda").manual_seed(1000 * b + 10 * n + act_dim)
    rows = b * n
    h = th.randn(b, n, 64, device="cuda", generator=g)
    ws = [0.3 * th.randn(act_dim, 64, device="cuda", generator=g) for _ in range(n)]
    bs = [0.3 * th.randn(act_dim, device="cuda", generator=g) for _ in range(n)]
    proj = th.randn(b, n, act_dim, device="cuda", generator=g)
    ref32 = _composition(h, ws, bs, proj)
    ref = _composition(h.double(), [w.double() for w in ws], [x.double() for x in bs], proj.double())
    bounds = _Bounds(f"b {b} n {n} a {act_dim} t {want_t} d_h {want_dh}")
    flat = lambda r, k: r[k].reshape(rows, -1)

    bufs = {"log_std": _guarded(rows, act_dim), "t": _guarded(rows, act_dim)}
    a = _head_args(h.view(rows, 64), ws, bs, n, act_dim)
    a.h, a.log_std = h.data_ptr(), bufs["log_std"][1].data_ptr()
    if want_t:
        a.t = bufs["t"][1].data_ptr()
    _lib.launch("flexnet_gauss_head_unshared_forward", a)
    th.cuda.synchronize()
    assert _guards_untouched(bufs["log_std"][0]) and _guards_untouched(bufs["t"][0])
    bounds.check("log_std", bufs["log_std"][1], flat(ref, "log_std"), flat(ref32, "log_std"), value=True)
    if want_t:
        bounds.check("t", bufs["t"][1], flat(ref, "t"), flat(ref32, "t"), value=True)
    else:
        assert bool((bufs["t"][0] == SENTINEL).all())

    outs = {"d_u": _guarded(rows, act_dim), "d_h": _guarded(rows, 64)}
    t_in = bufs["t"][1] if want_t else ref32["t"].reshape(rows, act_dim).contiguous()
    d_ls = proj.reshape(rows, act_dim)
    gb = _head_args(h.view(rows, 64), ws, bs, n, act_dim)
    gb.t, gb.d_log_std, gb.d_u = t_in.data_ptr(), d_ls.data_ptr(), outs["d_u"][1].data_ptr()
    if want_dh:
        gb.d_h = outs["d_h"][1].data_ptr()
    _lib.launch("flexnet_gauss_head_unshared_backward", gb)
    th.cuda.synchronize()
    assert _guards_untouched(outs["d_u"][0]) and _guards_untouched(outs["d_h"][0])
    bounds.check("d_u", outs["d_u"][1], flat(ref, "d_u"), flat(ref32, "d_u"))
    if want_dh:
        bounds.check("d_h", outs["d_h"][1], flat(ref, "d_h"), flat(ref32, "d_h"))
    else:
        assert bool((outs["d_h"][0] == SENTINEL).all())
    first = {k: buf.clone() for k, (buf, _) in outs.items()}
    _lib.launch("flexnet_gauss_head_unshared_backward", gb)
    th.cuda.synchronize()
    assert all(th.equal(first[k], outs[k][0]) for k in outs)


# a single row; a ragged last 32-sample tile; more than one work-group per agent; the agent maximum
@pytest.mark.parametrize("b,n,act_dim", [(1, 1, 1), (33, 3, 4), (129, 5, 8), (31, 8, 4)])
def test_copies_of_one_head_agree_with_the_shared_kernel_both_ways(b, n, act_dim):
    """The per-agent entry points on n copies of ONE head are the shared entry points on the same rows, bit for bit: the two
    forms are instantiations of one body (csrc/gauss.hip) and differ in the row map alone."""
    from safe_marl_amd import _lib
    g = th.Generator(device="cuda").manual_seed(1000 * b + 10 * n + act_dim)
    rows = b * n
    h = th.randn(rows, 64, device="cuda", generator=g)
    w = 0.3 * th.randn(act_dim, 64, device="cuda", generator=g)
    bias = 0.3 * th.randn(act_dim, device="cuda", generator=g)
    d_ls = th.randn(rows, act_dim, device="cuda", generator=g)
    shared = _lib.FlexGaussHeadArgs()
    shared.rows, shared.act_dim, shared.hid, shared.log_std_min, shared.log_std_max = rows, act_dim, 64, LO, HI
    shared.w, shared.b = w.data_ptr(), bias.data_ptr()
    out = {}
    for form, a in (("shared", shared), ("unshared", _head_args(h, [w] * n, [bias] * n, n, act_dim))):
        o = out[form] = {k: th.full((rows, width), SENTINEL, device="cuda")
                         for k, width in (("log_std", act_dim), ("t", act_dim), ("d_u", act_dim), ("d_h", 64))}
        a.h, a.log_std, a.t = h.data_ptr(), o["log_std"].data_ptr(), o["t"].data_ptr()
        _lib.launch(f"flexnet_gauss_head{'_unshared' if form == 'unshared' else ''}_forward", a)
        a.d_log_std, a.d_u, a.d_h = d_ls.data_ptr(), o["d_u"].data_ptr(), o["d_h"].data_ptr()
        _lib.launch(f"flexnet_gauss_head{'_unshared' if form == 'unshared' else ''}_backward", a)
    th.cuda.synchronize()
    for k, got in out["unshared"].items():
        assert not bool((got == SENTINEL).any()), k
        assert th.equal(got, out["shared"][k]), k


def _rnn_agents(n, obs_dim, act_dim, seed):
    """n RNNAgentGaussian modules with distinct seeded weights, scaled up."""
    from safe_marl_amd.nets import RNNAgentGaussian
    from safe_marl_amd.util import convert
    d = json.load(open(os.path.join(G, "learner_args.json")))
    d.update(agent_num=n, action_dim=act_dim, layernorm=True, agent_id=True, shared_params=False, obs_size=obs_dim,
             gaussian_policy=True)
    args = convert(d)
    th.manual_seed(seed)
    out = []
    for _ in range(n):
        ag = RNNAgentGaussian(obs_dim + n, args).cuda()
        with th.no_grad():
            for p in ag.parameters():
                p.mul_(3.0).add_(0.05 * th.randn_like(p))
        out.append(ag)
    return out


def _loop(agents, obs, hid, proj):
    """Model.policy's per-agent loop on [obs | onehot(i)] in the dtype of ``obs``; loss (means proj).sum() + log_stds.sum()."""
    from safe_marl_amd.nets import RNNAgent, gauss_log_std_torch
    b, n, _ = obs.shape
    for ag in agents:
        ag.zero_grad()
    outs = []
    for i, ag in enumerate(agents):
        inp = th.cat([obs[:, i], F.one_hot(th.full((b,), i, device=obs.device), n).to(obs.dtype)], 1)
        mean, _, h = RNNAgent.forward(ag, inp, hid[:, i])         # (the head as tensor operations: fp64 has no kernel to decline)
        a = ag.args
        outs.append((mean, gauss_log_std_torch(h, ag.log_std.weight, ag.log_std.bias, a.LOG_STD_MIN, a.LOG_STD_MAX), h))
    means, log_stds, hn = (th.stack([o[k] for o in outs], 1) for k in range(3))
    ((means * proj).sum() + log_stds.sum()).backward()
    return dict(means=means.detach(), log_stds=log_stds.detach(), hidden=hn.detach(),
                grads={f"{i}.{k}": p.grad.clone() for i, ag in enumerate(agents) for k, p in ag.named_parameters()})


def test_the_head_node_and_permutation():
    from safe_marl_amd.nets import gauss_log_std_unshared
    n, b = 3, 33
    agents = _rnn_agents(n, 30, 4, seed=5)
    h = th.randn(b, n, 64, device="cuda")
    with th.no_grad():
        l0 = gauss_log_std_unshared(agents, h.view(-1, 64)).view(b, n, -1)
        perm = [2, 0, 1]
        l1 = gauss_log_std_unshared([agents[p] for p in perm], h[:, perm].reshape(-1, 64)).view(b, n, -1)
        assert th.equal(l1, l0[:, perm])
        l2 = gauss_log_std_unshared([agents[p] for p in perm], h.view(-1, 64)).view(b, n, -1)   # other weights on the same rows
        assert (l2 - l0).abs().max().item() > 1e-3
        for i, ag in enumerate(agents):                           # row r uses head r % n: the shared-weight kernel's bits
            assert th.equal(l0[:, i], ag.log_std_of(h[:, i].contiguous()))
    hg = h.view(-1, 64).clone().requires_grad_()
    ls = gauss_log_std_unshared(agents, hg)
    assert "GaussHeadUnsharedFn" in type(ls.grad_fn).__name__
    ls.sum().backward()
    a = agents[0].args
    h64 = h.double().requires_grad_()
    ref = th.stack([a.LOG_STD_MIN + 0.5 * (a.LOG_STD_MAX - a.LOG_STD_MIN)
                    * (th.tanh(F.linear(h64[:, i], ag.log_std.weight.double(), ag.log_std.bias.double())) + 1)
                    for i, ag in enumerate(agents)], 1)
    params64 = [p for ag in agents for p in (ag.log_std.weight, ag.log_std.bias)]
    g64 = th.autograd.grad(ref.sum(), [h64])[0]
    err, bound = (hg.grad.view(b, n, 64).double() - g64).abs().max().item(), 2e-6 + 3e-4 * g64.abs().max().item()
    print(f"head node d_h: error {err:.3e}, project bound {bound:.3e}")
    assert err <= bound and all(p.grad is not None and p.grad.abs().max() > 0 for p in params64)


# 417: a part-filled last tile; 16 417 samples: the backward's wavefronts walk more than one tile
@pytest.mark.parametrize("b,n", [(417, 5), (16417, 2)])
def test_rnn_node_with_the_heads_against_the_loop(b, n):
    from safe_marl_amd.nets import actor_unshared_train, gauss_log_std_unshared
    o, act = 30, 4
    agents = _rnn_agents(n, o, act, seed=b)
    g = th.Generator(device="cuda").manual_seed(b)
    obs = 0.5 * th.randn(b, n, o, device="cuda", generator=g)
    hid = 0.5 * th.randn(b, n, 64, device="cuda", generator=g)
    proj = th.randn(b, n, act, device="cuda", generator=g) / (b * n) * 100.0
    ref32 = _loop(agents, obs, hid, proj)
    ref = _loop([copy.deepcopy(ag).double() for ag in agents], obs.double(), hid.double(), proj.double())

    def run():
        for ag in agents:
            ag.zero_grad()
        means, hn = actor_unshared_train(agents, obs, hid)
        assert "ActorUnsharedTrainHidFn" in type(means.grad_fn).__name__ and hn.requires_grad
        log_stds = gauss_log_std_unshared(agents, hn)
        ((means.view(b, n, act) * proj).sum() + log_stds.sum()).backward()
        return (means.detach().view(b, n, act), log_stds.detach().view(b, n, act), hn.detach().view(b, n, 64),
                {f"{i}.{k}": p.grad.clone() for i, ag in enumerate(agents) for k, p in ag.named_parameters()})

    means, log_stds, hn, g1 = run()
    _, _, _, g2 = run()
    bounds = _Bounds(f"rnn gaussian node b {b} n {n}")
    bounds.check("means", means, ref["means"], ref32["means"], value=True)
    bounds.check("log_stds", log_stds, ref["log_stds"], ref32["log_stds"], value=True)
    bounds.check("hidden", hn, ref["hidden"], ref32["hidden"], value=True)
    assert len(g1) == 12 * n                                     # fc1, LayerNorm, the GRU's four, mean, log_std
    for k, got in g1.items():
        assert th.equal(got, g2[k]), k                           # fixed-order sums everywhere: the same bits
        bounds.check(k, got, ref["grads"][k], ref32["grads"][k])


def test_rnn_node_without_d_hn_is_the_direct_backward_call():
    """The fixed-std RNN agents' node (no gradient at the new hidden state) gives the bits of flexnet_actor_unshared_backward
    called directly on the node's own saves, as tests/test_unshared_gpu.py calls it."""
    from safe_marl_amd import _lib, nets
    from .test_unshared_gpu import _agents, _tables
    b, n, o, act = 417, 5, 30, 4
    agents = _agents(n, o, act, True, True, seed=9)
    rows = b * n
    obs = 0.5 * th.randn(b, n, o, device="cuda")
    hid = 0.5 * th.randn(b, n, 64, device="cuda")
    proj = th.randn(rows, act, device="cuda") / rows
    means, hn = nets.actor_unshared_train(agents, obs, hid)
    node = means.grad_fn
    assert type(node).__name__.startswith("_ActorUnsharedTrainFn") and not hn.requires_grad
    saved = node.saved_tensors[3]                                  # z1 | x | r | z | n | hn
    (means * proj).sum().backward()
    outs = {k: th.empty(rows, w, device="cuda") for k, w in (("d_gi", 192), ("d_gh", 192), ("dz", 64))}
    small = {k: th.empty(n, 64, device="cuda") for k in ("d_ln_w", "d_ln_b", "d_fc1_b")}
    ws = th.empty(_lib.FLEXNET_ACTOR_UNSHARED_WS_FLOATS, dtype=th.float32, device="cuda")
    gb = _lib.FlexActorUnsharedBwdArgs()
    gb.rows, gb.n_agents, gb.obs_dim, gb.act_dim = rows, n, o, act
    gb.agent_id, gb.layernorm, gb.ln_eps = 1, 1, float(agents[0].layernorm.eps)
    gb.d_means, gb.h_prev = proj.data_ptr(), hid.data_ptr()
    for j, k in enumerate(("z1", "x", "r", "z", "n", "hn")):
        setattr(gb, k, saved[j].data_ptr())
    _tables(gb, agents, {f[0] for f in gb._fields_})
    for k, t in list(outs.items()) + list(small.items()):
        setattr(gb, k, t.data_ptr())
    gb.workspace, gb.workspace_floats = ws.data_ptr(), ws.numel()
    _lib.launch("flexnet_actor_unshared_backward", gb)
    th.cuda.synchronize()
    for i, ag in enumerate(agents):
        assert th.equal(ag.fc1.bias.grad, small["d_fc1_b"][i]) and th.equal(ag.layernorm.weight.grad, small["d_ln_w"][i])
        assert th.equal(ag.layernorm.bias.grad, small["d_ln_b"][i])
        assert th.equal(ag.fc1.weight.grad[:, o + i], small["d_fc1_b"][i])
