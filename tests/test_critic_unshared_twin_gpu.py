"""GPU: MATD3's per-agent twin critics of ``shared_params: False`` in one launch per direction
(csrc/critic_unshared_twin.hip; nets.fused_critic_forward_unshared_twin, nets._CriticUnsharedTwinFn) against the per-agent
module composition in fp64 — the loop of matd3.py:74-82 on the rows of matd3.py:33-66, [obs of all | onehot(i) | actions of
all, the others' detached | flag], with the flag at 0 (head 0) and at 1 (head 1).

Bounds by the rule of tests/test_critic_unshared_gpu.py: values 2e-5 max(1, max|ref|), gradients 2e-6 + 3e-4 max|ref|, or four
times the error of the fp32 composition on the device against the same fp64 reference where that is larger; both are printed."""
import copy
import itertools

import pytest
import torch as th
import torch.nn.functional as F

from .test_critic_unshared_gpu import SENTINEL, _Bounds, _args, _guarded, _guards_untouched

pytestmark = pytest.mark.gpu


def _critics(n, obs_dim, act_dim, layernorm, agent_id, seed=3):
    """n MLPCritics of (o + a) n + n_id + 1 columns with seeded weights made distinct per agent."""
    from safe_marl_amd.nets import MLPCritic
    args = _args(agent_num=n, action_dim=act_dim, layernorm=layernorm, agent_id=agent_id, shared_params=False, obs_size=obs_dim)
    th.manual_seed(seed)
    out = []
    for _ in range(n):
        c = MLPCritic((obs_dim + act_dim) * n + (n if agent_id else 0) + 1, 1, args).cuda()
        with th.no_grad():
            for p in c.parameters():
                p.mul_(3.0).add_(0.05 * th.randn_like(p))
        out.append(c)
    return out


def _composition(critics, obs, act, agent_id, proj):
    """mlp_critic.py:28-35 per agent and head on its materialised input row, in the dtype of ``obs``; ``proj`` [heads, b, n]
    weighs the outputs.  q [heads, b, n], z1 [b, n, 64] (head 0's), x / dz1 / dz2 [heads, b, n, 64], every parameter gradient
    of the weighted sum over the heads, and the gradient of the actions through head 0 alone."""
    heads = proj.shape[0]
    b, n, o = obs.shape
    a = act.shape[2]
    out = {k: [] for k in ("q", "z1", "x", "dz1", "dz2", "grads", "d_act")}
    for i, c in enumerate(critics):
        c.zero_grad()
        parts = [obs.reshape(b, n * o)]
        if agent_id:
            parts.append(F.one_hot(th.full((b,), i, device=obs.device), n).to(obs.dtype))
        parts.append(act.reshape(b, n * a))
        per = {k: [] for k in ("q", "z1", "x", "z2")}
        for hd in range(heads):
            rows = th.cat(parts + [th.full((b, 1), float(hd), dtype=obs.dtype, device=obs.device)], 1)
            z1 = c.fc1(rows)
            z1.retain_grad()
            x = F.relu(c.layernorm(z1) if c.args.layernorm else z1)
            z2 = c.fc2(x)
            z2.retain_grad()
            q = c.fc3(F.relu(z2))[:, 0]
            with th.no_grad():
                assert (c(rows, None)[0][:, 0] - q).abs().max().item() <= 1e-6 * max(1.0, q.abs().max().item())
            per["q"].append(q); per["z1"].append(z1); per["x"].append(x.detach()); per["z2"].append(z2)
        sum((per["q"][hd] * proj[hd, :, i]).sum() for hd in range(heads)).backward()
        # matd3.py:46-53 detaches the other agents' actions: agent i's own block takes the gradient, here head 0's alone
        own = c.fc1.weight.shape[1] - 1 - n * a + i * a
        out["d_act"].append(per["z1"][0].grad @ c.fc1.weight.detach()[:, own:own + a])
        out["q"].append(th.stack([q.detach() for q in per["q"]]))
        out["z1"].append(per["z1"][0].detach())
        out["x"].append(th.stack(per["x"]))
        out["dz1"].append(th.stack([z.grad for z in per["z1"]]))
        out["dz2"].append(th.stack([z.grad for z in per["z2"]]))
        out["grads"].append({k: p.grad.clone() for k, p in c.named_parameters()})
    res = {"q": th.stack(out["q"], 2), "z1": th.stack(out["z1"], 1)}                  # [heads, b, n], [b, n, 64]
    res.update({k: th.stack(out[k], 2) for k in ("x", "dz1", "dz2")})                 # [heads, b, n, 64]
    res["grads"], res["d_act"] = out["grads"], th.stack(out["d_act"], 1)           # [b, n, a]
    return res


# every b with every n (the part-filled tiles; 257: a third work-group per agent whose only tile holds one row); obs_dim,
# act_dim, layernorm and agent_id cycle so that every value occurs several times.  Every case runs one and two heads, with and
# without the parameter gradients.  The last b = 33 case is the widest first layer there is (1 152 + 8 + 64 + 1 columns).
_BN = list(itertools.product([1, 31, 33, 64, 257], [1, 3, 5, 8]))
CASES = [(b, n, [6, 144][(k + k // 4) % 2], [2, 4, 8][k % 3], (k // 2) % 2 == 0, k % 5 < 3) for k, (b, n) in enumerate(_BN)]
CASES[_BN.index((33, 8))] = (33, 8, 144, 8, True, True)


def test_the_cases_cover_every_value():
    assert len(CASES) == 20
    for col, values in ((0, {1, 31, 33, 64, 257}), (1, {1, 3, 5, 8}), (2, {6, 144}), (3, {2, 4, 8}), (4, {True, False}),
                        (5, {True, False})):
        assert {c[col] for c in CASES} == values
    assert {(c[0], c[1]) for c in CASES} == set(_BN)
    assert {(c[4], c[5]) for c in CASES} == {(True, True), (True, False), (False, True), (False, False)}
    assert max((c[2] + c[3]) * c[1] + (c[1] if c[5] else 0) + 1 for c in CASES) == 1225


@pytest.mark.parametrize("b,n,obs_dim,act_dim,layernorm,agent_id", CASES)
def test_entry_points_and_node_against_the_composition(b, n, obs_dim, act_dim, layernorm, agent_id):
    _check_case(b, n, obs_dim, act_dim, layernorm, agent_id)


@pytest.mark.parametrize("b,n,layernorm", [(16417, 1, True), (16385, 2, False)])
def test_a_wavefront_that_walks_several_tiles(b, n, layernorm):
    """Past 128 work-groups per agent (16 384 samples) the backward's grid is capped and a wavefront walks a second tile — a
    path no smaller batch reaches.  16 417 samples: 514 tiles, the last one with one row; the narrowest rows keep it quick."""
    from safe_marl_amd.nets import _lib
    assert (b + 31) // 32 > 4 * 128 and _lib.FLEXNET_CRITIC_UNSHARED_TWIN_WS_FLOATS == 8 * 128 * 448
    _check_case(b, n, 6, 2, layernorm, True)


def _check_case(b, n, obs_dim, act_dim, layernorm, agent_id):
    from safe_marl_amd import _lib
    from safe_marl_amd.nets import _CRITIC_UNSHARED_TABLES, _critic_unshared_params, critic_unshared_twin_train
    critics = _critics(n, obs_dim, act_dim, layernorm, agent_id, seed=b + n)
    g = th.Generator(device="cuda").manual_seed(100 * b + n)
    obs = 0.5 * th.randn(b, n, obs_dim, device="cuda", generator=g)
    act = 0.5 * th.randn(b, n, act_dim, device="cuda", generator=g)
    proj = th.randn(2, b, n, device="cuda", generator=g) / (b * n)
    doubles = [copy.deepcopy(c).double() for c in critics]
    ref32 = {hd: _composition(critics, obs, act, agent_id, proj[:hd]) for hd in (1, 2)}
    ref = {hd: _composition(doubles, obs.double(), act.double(), agent_id, proj[:hd].double()) for hd in (1, 2)}
    case = f"b {b} n {n} o {obs_dim} a {act_dim} ln {layernorm} id {agent_id}"
    rows, eps = b * n, float(critics[0].layernorm.eps) if layernorm else 1e-5
    w1, w2 = n * obs_dim, n * act_dim
    ld = w1 + (n if agent_id else 0) + w2 + 1

    def tables(a):
        names = {f[0] for f in a._fields_}
        for i, c in enumerate(critics):
            for k, name in enumerate(_CRITIC_UNSHARED_TABLES):
                p = _critic_unshared_params(c)[k]
                if name in names and p is not None:
                    getattr(a, name)[i] = p.data_ptr()

    def head(a, heads):
        a.rows, a.n_agents, a.w1, a.w2, a.heads = rows, n, w1, w2, heads
        a.agent_id, a.layernorm, a.ln_eps = int(agent_id), int(layernorm), eps
        tables(a)

    def forward(heads):
        """With the saves, every output between guard rows; then without them: the same bits."""
        bufs = {"q": _guarded(heads * b, n), "save_z1": _guarded(rows, 64), "save_x": _guarded(heads * rows, 64)}
        a = _lib.FlexCriticUnsharedTwinArgs()
        head(a, heads)
        a.x1, a.x1_pitch, a.x1_agent_off = obs.data_ptr(), n * obs_dim, 0
        a.x2, a.x2_pitch, a.x2_agent_off = act.data_ptr(), n * act_dim, 0
        for k, (_, view) in bufs.items():
            setattr(a, k, view.data_ptr())
        _lib.launch("flexnet_critic_unshared_twin_forward", a)
        th.cuda.synchronize()
        for k, (buf, _) in bufs.items():
            assert _guards_untouched(buf), k
        bounds = _Bounds(f"{case} heads {heads}")
        bounds.check("q", bufs["q"][1].view(heads, b, n), ref[heads]["q"], ref32[heads]["q"], value=True)
        bounds.check("z1", bufs["save_z1"][1].view(b, n, 64), ref[heads]["z1"], ref32[heads]["z1"], value=True)
        bounds.check("x", bufs["save_x"][1].view(heads, b, n, 64), ref[heads]["x"], ref32[heads]["x"], value=True)
        q2 = _guarded(heads * b, n)
        a.q, a.save_z1, a.save_x = q2[1].data_ptr(), None, None
        _lib.launch("flexnet_critic_unshared_twin_forward", a)
        th.cuda.synchronize()
        assert th.equal(q2[0], bufs["q"][0])
        return bufs

    fwd = {hd: forward(hd) for hd in (1, 2)}
    # head 0 of a two-head launch is a one-head launch, bit for bit
    assert th.equal(fwd[1]["q"][1], fwd[2]["q"][1][:b])
    assert th.equal(fwd[1]["save_z1"][1], fwd[2]["save_z1"][1]) and th.equal(fwd[1]["save_x"][1], fwd[2]["save_x"][1][:rows])

    def backward(heads, param_grads):
        """From the kernel's own saves; run twice: fixed-order sums, the same bits."""
        outs = {"dz1_sum": _guarded(rows, 64), "dz2": _guarded(heads * rows, 64)}
        small = {k: _guarded(n, 64) for k in ("d_ln_w", "d_ln_b", "d_fc1_b", "d_fc2_b", "d_fc3_w", "d_flag")}
        small["d_fc3_b"] = _guarded(n, 1)
        own = _guarded(rows, act_dim)
        ws = th.full((_lib.FLEXNET_CRITIC_UNSHARED_TWIN_WS_FLOATS,), SENTINEL, dtype=th.float32, device="cuda")
        dq = proj[:heads].contiguous()
        gb = _lib.FlexCriticUnsharedTwinBwdArgs()
        head(gb, heads)
        gb.param_grads = int(param_grads)
        gb.dq, gb.z1, gb.x = dq.data_ptr(), fwd[heads]["save_z1"][1].data_ptr(), fwd[heads]["save_x"][1].data_ptr()
        for k, (_, view) in list(outs.items()) + list(small.items()):
            setattr(gb, k, view.data_ptr())
        gb.d_x2_own, gb.own_first, gb.own_step, gb.own_w = own[1].data_ptr(), 0, act_dim, act_dim
        gb.workspace, gb.workspace_floats = ws.data_ptr(), ws.numel()
        _lib.launch("flexnet_critic_unshared_twin_backward", gb)
        th.cuda.synchronize()
        everything = dict(outs, **small, own=own)
        for k, (buf, _) in everything.items():
            assert _guards_untouched(buf), k
        again = {k: buf.clone() for k, (buf, _) in everything.items()}
        _lib.launch("flexnet_critic_unshared_twin_backward", gb)
        th.cuda.synchronize()
        for k, (buf, _) in everything.items():
            assert th.equal(again[k], buf), k
        return everything, ws

    kernel = {}
    for heads in (1, 2):
        bounds = _Bounds(f"{case} heads {heads}")
        r, r32 = ref[heads], ref32[heads]
        out, _ = backward(heads, True)
        kernel[heads] = out
        bounds.check("dz1_sum", out["dz1_sum"][1].view(b, n, 64), r["dz1"].sum(0), r32["dz1"].sum(0))
        bounds.check("dz2", out["dz2"][1].view(heads, b, n, 64), r["dz2"], r32["dz2"])
        sums = {"d_fc1_b": "fc1.bias", "d_fc2_b": "fc2.bias", "d_fc3_b": "fc3.bias", "d_ln_w": "layernorm.weight",
                "d_ln_b": "layernorm.bias"}
        for k, name in sums.items():
            if name.startswith("layernorm") and not layernorm:    # not written without layernorm
                assert bool((out[k][0] == SENTINEL).all())
                continue
            bounds.check(k, out[k][1].view(n, -1), th.stack([g_[name] for g_ in r["grads"]]).view(n, -1),
                         th.stack([g_[name] for g_ in r32["grads"]]).view(n, -1))
        bounds.check("d_fc3_w", out["d_fc3_w"][1], th.stack([g_["fc3.weight"][0] for g_ in r["grads"]]),
                     th.stack([g_["fc3.weight"][0] for g_ in r32["grads"]]))
        bounds.check("d_flag", out["d_flag"][1], th.stack([g_["fc1.weight"][:, -1] for g_ in r["grads"]]),
                     th.stack([g_["fc1.weight"][:, -1] for g_ in r32["grads"]]))
        if heads == 1:
            assert bool((out["d_flag"][1] == 0).all())            # the flag input is 0 on the first head
        bounds.check("d_x2_own", out["own"][1].view(b, n, act_dim), r["d_act"], r32["d_act"])   # head 0's alone
        frozen, ws = backward(heads, False)                       # parameter gradients off: no gradient buffer is touched
        assert th.equal(frozen["dz1_sum"][0], out["dz1_sum"][0]) and th.equal(frozen["own"][0], out["own"][0])
        for k in ("dz2", "d_ln_w", "d_ln_b", "d_fc1_b", "d_fc2_b", "d_fc3_w", "d_fc3_b", "d_flag"):
            assert bool((frozen[k][0] == SENTINEL).all()), k
        assert bool((ws == SENTINEL).all())
    assert th.equal(kernel[1]["own"][1], kernel[2]["own"][1])     # the own-action gradient is the first head's in both

    # the node: every parameter gradient of every agent, the id and flag columns, the actions' gradient
    def node(heads, param_grads=True, act_grad=False):
        for c in critics:
            c.zero_grad()
        act_g = act.clone().requires_grad_() if act_grad else act
        q = critic_unshared_twin_train(critics, obs, act_g, heads, param_grads=param_grads)
        assert "CriticUnsharedTwinFn" in type(q.grad_fn).__name__ and q.shape == (heads, b, n)
        (q * proj[:heads]).sum().backward()
        return q.detach(), [{k: (None if p.grad is None else p.grad.clone()) for k, p in c.named_parameters()} for c in critics], \
            act_g.grad if act_grad else None

    for heads in (2, 1):
        bounds = _Bounds(f"{case} node heads {heads}")
        q1, g1, da1 = node(heads, act_grad=heads == 1)
        q1b, g1b, da1b = node(heads, act_grad=heads == 1)
        assert th.equal(q1, fwd[heads]["q"][1].view(heads, b, n)) and th.equal(q1, q1b)
        for i in range(n):
            assert len(g1[i]) == (8 if layernorm else 6)
            for k, got in g1[i].items():
                assert th.equal(got, g1b[i][k]), (i, k)
                bounds.check(f"agent {i} {k}", got, ref[heads]["grads"][i][k], ref32[heads]["grads"][i][k])
            gw = g1[i]["fc1.weight"]
            assert gw.shape == (64, ld) and th.equal(gw[:, -1], kernel[heads]["d_flag"][1][i])      # the flag column
            if agent_id:                                           # the one-hot input: only the agent's own id column
                ids = gw[:, w1:w1 + n]
                off = th.cat([ids[:, :i], ids[:, i + 1:]], 1)
                assert bool((off == 0).all()) and th.equal(ids[:, i], g1[i]["fc1.bias"])
        if heads == 1:
            assert th.equal(da1, da1b) and th.equal(da1, kernel[1]["own"][1].view(b, n, act_dim))
            _, g0, da0 = node(1, param_grads=False, act_grad=True)       # the policy pass: the actions' gradient alone
            assert th.equal(da0, da1) and all(v is None for gi in g0 for v in gi.values())
    with pytest.raises(RuntimeError, match="first head"):
        critic_unshared_twin_train(critics, obs, act.clone().requires_grad_(), 2)


def test_permuting_the_modules_permutes_the_outputs():
    from safe_marl_amd.nets import fused_critic_forward_unshared_twin
    n, b = 3, 33
    critics = _critics(n, 6, 4, True, False)
    obs = 0.5 * th.randn(b, n, 6, device="cuda")
    act = 0.5 * th.randn(b, n, 4, device="cuda")
    q0 = fused_critic_forward_unshared_twin(critics, obs, act, 2)
    perm = [2, 0, 1]
    q1 = fused_critic_forward_unshared_twin([critics[p] for p in perm], obs, act, 2)
    assert q0.shape == (2, b, n) and th.equal(q1, q0[:, :, perm])     # (shared blocks, no id columns: a critic sees one row)
    assert (q0[0] - q0[1]).abs().max().item() > 1e-3                   # the flag column matters


def _model(n=3, **over):
    import safe_marl_amd.learner as L
    args = _args(cuda=True, shared_params=False, agent_num=n, state_size=3 * 33 + 2 * n + 1, **over)
    th.manual_seed(11)
    m = L.MATD3(args).cuda()
    with th.no_grad():
        for p in m.value_dicts.parameters():
            p.mul_(3.0).add_(0.05 * th.randn_like(p))
    return m


def _is_node(t):
    fn, seen = t.grad_fn, 0
    while fn is not None and "CriticUnsharedTwinFn" not in type(fn).__name__ and fn.next_functions and seen < 8:
        fn, seen = fn.next_functions[0][0], seen + 1
    return fn is not None and "CriticUnsharedTwinFn" in type(fn).__name__


def test_value_dispatch(monkeypatch):
    from safe_marl_amd import learner, util
    m = _model()
    n, o, a = m.n_, m.obs_dim, m.act_dim
    big = (2048 + n - 1) // n                                           # b n >= 2 048
    obs = 0.5 * th.randn(big, n, o, device="cuda")
    act = 0.5 * th.randn(big, n, a, device="cuda")
    before = util.FALLBACKS.get("critic_unshared_twin", 0)
    calls = []
    real = learner.fused_critic_forward_unshared_twin

    def spy(*args):
        out = real(*args)
        calls.append(out is not None)
        return out
    monkeypatch.setattr(learner, "fused_critic_forward_unshared_twin", spy)
    with th.no_grad():
        v_small = m.value(obs[:32], act[:32])                           # no graph at b = 32: the forward launch
    assert calls == [True] and v_small.shape == (64, n, 1)
    v = m.value(obs, act)                                               # with a graph from 2 048 rows: the node
    assert calls == [True] and _is_node(v) and v.shape == (2 * big, n, 1)
    v_loop = m.value(obs[:64], act[:64])                                # below it: the loop, not a decline
    assert calls == [True] and not _is_node(v_loop) and v_loop.requires_grad and v_loop.shape == (128, n, 1)
    act_g = act.clone().requires_grad_()
    v_both = m.value(obs, act_g)                                        # both heads of a live action: the loop
    assert not _is_node(v_both) and v_both.shape == (2 * big, n, 1)
    assert util.FALLBACKS.get("critic_unshared_twin", 0) == before
    m.fused_inference = False
    with th.no_grad():
        v0 = m.value(obs, act)
    assert calls == [True]
    assert (v.detach() - v0).abs().max().item() <= 2e-5 * max(1.0, v0.abs().max().item())
    assert (v_both.detach() - v0).abs().max().item() <= 2e-5 * max(1.0, v0.abs().max().item())
    assert th.equal(v_small[:32], v.detach()[:32]) and th.equal(v_small[32:], v.detach()[big:big + 32])
    # first_head_only with critic_frozen: the policy pass — the actions' gradient, no parameter gradient
    m.fused_inference = True
    m.zero_grad()
    vf = m.value(obs, act_g, critic_frozen=True, first_head_only=True)
    assert _is_node(vf) and vf.shape == (big, n, 1) and th.equal(vf.detach(), v.detach()[:big])
    vf.sum().backward()
    assert act_g.grad is not None and all(p.grad is None for p in m.value_dicts.parameters())
    m.fused_inference = False
    act_l = act.clone().requires_grad_()
    m.value(obs, act_l, critic_frozen=True, first_head_only=True).sum().backward()
    assert (act_g.grad - act_l.grad).abs().max().item() <= 2e-6 + 3e-4 * act_l.grad.abs().max().item()


def test_hid_32_declines_with_a_note():
    from safe_marl_amd import util
    m = _model(hid_size=32)
    n = m.n_
    obs = 0.5 * th.randn(64, n, m.obs_dim, device="cuda")
    act = 0.5 * th.randn(64, n, m.act_dim, device="cuda")
    util.FALLBACKS.pop("critic_unshared_twin", None)
    with th.no_grad():
        with pytest.warns(RuntimeWarning, match="critic_unshared_twin"):
            v1 = m.value(obs, act)
        assert util.FALLBACKS["critic_unshared_twin"] == 1
        m.fused_inference = False
        v0 = m.value(obs, act)
    assert util.FALLBACKS["critic_unshared_twin"] == 1 and th.equal(v1, v0)
