"""GPU: the per-agent MLP actors of ``shared_params: False`` in one launch per direction (csrc/actor_mlp.hip's per-agent form;
nets.fused_actor_forward_mlp_unshared, nets._ActorMlpUnsharedTrainFn) against the per-agent module loop (mlp_agent.py:20-32 on
agent i's rows [obs | onehot(i)]) in fp64, and ``Model.policy``'s dispatch with its capture rule.  Nothing here captures a HIP
graph: the rule is tested by patching what it asks.

Bounds are tests/test_actor_mlp_gpu.py's (its ``_Bounds``, imported): values 2e-5 max(1, max|ref|), gradients 2e-6 + 3e-4
max|ref|, or four times the error of the fp32 loop on the device against the same fp64 reference where that is larger; every
check prints which applied."""
import copy
import itertools
import warnings

import pytest
import torch as th
import torch.nn.functional as F

from .golden_io import golden_args
from .test_actor_mlp_gpu import SENTINEL, _agent, _Bounds, _guarded, _guards_untouched, _record_launches
from .test_unshared_agents_cpu import DIR

pytestmark = pytest.mark.gpu
NEW = ("flexnet_actor_mlp_unshared_forward", "flexnet_actor_mlp_unshared_backward")
TABLES = ("fc1_w", "fc1_b", "ln_w", "ln_b", "fc2_w", "fc2_b", "fc3_w", "fc3_b")


def _agents(n, obs_dim, act_dim, layernorm, agent_id, seed, gaussian=False):
    """n MLP agents with distinct seeded weights, scaled up as tests/test_actor_mlp_gpu.py's ``_agent``."""
    return [_agent(n, obs_dim, act_dim, layernorm, agent_id, seed=1000 * seed + i, gaussian=gaussian) for i in range(n)]


def _loop(agents, obs, agent_id, proj, proj_h=None, log_std_sum=False):
    """The per-agent module loop (model.py:124-138) in the dtype of ``obs`` [b, n, o], layer by layer: per agent, stacked along
    the agent axis, means, h, z1, x, dz1, dz2 [b, n, .] and every parameter gradient of (means proj).sum() (+ (h proj_h).sum())
    (+ log_stds.sum()) as ``grads["i.name"]``."""
    b, n, o = obs.shape
    res = {k: [] for k in ("means", "h", "z1", "x", "dz1", "dz2", "log_stds")}
    grads = {}
    proj, proj_h = proj.view(b, n, -1), None if proj_h is None else proj_h.view(b, n, 64)
    for i, agent in enumerate(agents):
        rows = obs[:, i]
        if agent_id:
            rows = th.cat((rows, F.one_hot(th.tensor(i, device=obs.device), n).to(obs.dtype).expand(b, n)), 1)
        agent.zero_grad()
        z1 = agent.fc1(rows)
        z1.retain_grad()
        x = F.relu(agent.layernorm(z1) if agent.args.layernorm else z1)
        z2 = agent.fc2(x)
        z2.retain_grad()
        h = F.relu(z2)
        means = agent.fc3(h)
        with th.no_grad():                                              # the module itself
            out = agent(rows, None)
            assert (out[0] - means).abs().max().item() <= 1e-6 * max(1.0, means.abs().max().item())
        loss = (means * proj[:, i]).sum()
        if proj_h is not None:
            loss = loss + (h * proj_h[:, i]).sum()
        if log_std_sum:
            a = agent.args
            ls = a.LOG_STD_MIN + 0.5 * (a.LOG_STD_MAX - a.LOG_STD_MIN) * (th.tanh(agent.log_std(h)) + 1)
            loss = loss + ls.sum()
            res["log_stds"].append(ls.detach())
        loss.backward()
        for k, v in (("means", means.detach()), ("h", h.detach()), ("z1", z1.detach()), ("x", x.detach()), ("dz1", z1.grad),
                     ("dz2", z2.grad)):
            res[k].append(v)
        grads.update({f"{i}.{k}": p.grad.clone() for k, p in agent.named_parameters()})
    out = {k: th.stack(v, 1) for k, v in res.items() if v}
    out["grads"] = grads
    return out


def _both(agents, obs, agent_id, proj, proj_h=None, log_std_sum=False):
    ref32 = _loop(agents, obs, agent_id, proj, proj_h, log_std_sum)
    ref = _loop([copy.deepcopy(g).double() for g in agents], obs.double(), agent_id, proj.double(),
                None if proj_h is None else proj_h.double(), log_std_sum)
    return ref, ref32


# every b with every n (the part-filled tiles); 257: a third work-group per agent whose only tile holds one row.  obs_dim,
# act_dim, layernorm and agent_id cycle at different periods so that the last two occur on and off with every obs_dim.
_BN = list(itertools.product([1, 31, 33, 64], [1, 2, 3, 5, 8])) + [(257, 3), (257, 8)]
CASES = [(b, n, [6, 30, 144][k % 3], [1, 2, 4, 8][(k // 3) % 4], (k // 3) % 2 == 0, (k // 6) % 2 == 0) for k, (b, n) in enumerate(_BN)]


def test_the_cases_cover_every_value():
    for col, values in ((2, {6, 30, 144}), (3, {1, 2, 4, 8}), (4, {True, False}), (5, {True, False})):
        assert {c[col] for c in CASES} == values
    assert {(c[0], c[1]) for c in CASES} == set(_BN) and len(CASES) == 22
    for o in (6, 30, 144):
        assert {c[4] for c in CASES if c[2] == o} == {True, False} and {c[5] for c in CASES if c[2] == o} == {True, False}


def _fill(a, agents, names):
    from safe_marl_amd.nets import _actor_mlp_params
    for i, g in enumerate(agents):
        for name, p in zip(TABLES, _actor_mlp_params(g)):
            if name in names and p is not None:
                getattr(a, name)[i] = p.data_ptr()


def _forward_args(agents, obs, agent_id, bufs):
    from safe_marl_amd import _lib
    n, first = len(agents), agents[0]
    a = _lib.FlexActorMlpUnsharedArgs()
    a.rows, a.n_agents, a.obs_dim, a.act_dim, a.hid = obs.shape[0] * n, n, obs.shape[-1], first.args.action_dim, 64
    a.agent_id, a.layernorm = int(agent_id), int(first.args.layernorm)
    a.ln_eps = float(first.layernorm.eps) if first.args.layernorm else 1e-5
    _fill(a, agents, TABLES)
    a.obs = obs.data_ptr()
    for k, (_, view) in bufs.items():
        setattr(a, k, view.data_ptr())
    return a


def _check_id_columns(grads, n, obs_dim):
    for i in range(n):                                         # the one-hot input: only the agent's own id column
        ids = grads[f"{i}.fc1.weight"][:, obs_dim:]
        off = th.cat([ids[:, :i], ids[:, i + 1:]], 1)
        assert bool((off == 0).all()) and th.equal(ids[:, i], grads[f"{i}.fc1.bias"]), i


@pytest.mark.parametrize("b,n,obs_dim,act_dim,layernorm,agent_id", CASES)
def test_entry_points_and_node_against_the_loop(b, n, obs_dim, act_dim, layernorm, agent_id):
    from safe_marl_amd import _lib
    from safe_marl_amd.nets import _ActorMlpUnsharedTrainFn, _actor_mlp_params, fused_actor_forward_mlp_unshared
    agents = _agents(n, obs_dim, act_dim, layernorm, agent_id, seed=b + n)
    g = th.Generator(device="cuda").manual_seed(100 * b + n)
    rows = b * n
    obs = 0.5 * th.randn(b, n, obs_dim, device="cuda", generator=g)
    proj = th.randn(rows, act_dim, device="cuda", generator=g) / rows
    with_dh = (b + n) % 2 == 0                                 # every other case: a gradient arrives at h as well
    proj_h = th.randn(rows, 64, device="cuda", generator=g) / rows if with_dh else None
    ref, ref32 = _both(agents, obs, agent_id, proj, proj_h)
    bounds = _Bounds(f"b {b} n {n} o {obs_dim} a {act_dim} ln {layernorm} id {agent_id} d_h {with_dh}")
    eps = float(agents[0].layernorm.eps) if layernorm else 1e-5
    flat = lambda r, k: r[k].reshape(rows, -1)

    # forward with the two saves, every output between guard rows
    bufs = {"means": _guarded(rows, act_dim), "h": _guarded(rows, 64), "save_z1": _guarded(rows, 64), "save_x": _guarded(rows, 64)}
    a = _forward_args(agents, obs, agent_id, bufs)
    _lib.launch("flexnet_actor_mlp_unshared_forward", a)
    th.cuda.synchronize()
    for k, (buf, _) in bufs.items():
        assert _guards_untouched(buf), k
    for k, name in (("means", "means"), ("h", "h"), ("save_z1", "z1"), ("save_x", "x")):
        bounds.check(name, bufs[k][1], flat(ref, name), flat(ref32, name), value=True)
    again = {"means": _guarded(rows, act_dim), "h": _guarded(rows, 64)}      # the same launch without the saves: the same bits
    _lib.launch("flexnet_actor_mlp_unshared_forward", _forward_args(agents, obs, agent_id, again))
    th.cuda.synchronize()
    assert th.equal(again["means"][0], bufs["means"][0]) and th.equal(again["h"][0], bufs["h"][0])

    # backward from the kernel's own saves
    outs = {"dz1": _guarded(rows, 64), "dz2": _guarded(rows, 64), "d_ln_w": _guarded(n, 64), "d_ln_b": _guarded(n, 64),
            "d_fc1_b": _guarded(n, 64), "d_fc2_b": _guarded(n, 64), "d_fc3_b": _guarded(n, act_dim)}
    ws = th.full((_lib.FLEXNET_ACTOR_MLP_UNSHARED_WS_FLOATS,), SENTINEL, dtype=th.float32, device="cuda")
    gb = _lib.FlexActorMlpUnsharedBwdArgs()
    gb.rows, gb.n_agents, gb.obs_dim, gb.act_dim, gb.hid = rows, n, obs_dim, act_dim, 64
    gb.agent_id, gb.layernorm, gb.ln_eps = int(agent_id), int(layernorm), eps
    gb.d_means = proj.data_ptr()
    if with_dh:
        gb.d_h = proj_h.data_ptr()
    gb.z1, gb.x, gb.h = bufs["save_z1"][1].data_ptr(), bufs["save_x"][1].data_ptr(), bufs["h"][1].data_ptr()
    _fill(gb, agents, ("ln_w", "fc2_w", "fc3_w"))
    for k, (_, view) in outs.items():
        setattr(gb, k, view.data_ptr())
    gb.workspace, gb.workspace_floats = ws.data_ptr(), ws.numel()
    _lib.launch("flexnet_actor_mlp_unshared_backward", gb)
    th.cuda.synchronize()
    for k, (buf, _) in outs.items():
        assert _guards_untouched(buf), k
    first = {k: buf.clone() for k, (buf, _) in outs.items()}
    _lib.launch("flexnet_actor_mlp_unshared_backward", gb)     # fixed-order sums: the same bits
    th.cuda.synchronize()
    for k, (buf, _) in outs.items():
        assert th.equal(first[k], buf), k
    bounds.check("dz1", outs["dz1"][1], flat(ref, "dz1"), flat(ref32, "dz1"))
    bounds.check("dz2", outs["dz2"][1], flat(ref, "dz2"), flat(ref32, "dz2"))
    sums = {"d_fc1_b": "fc1.bias", "d_fc2_b": "fc2.bias", "d_fc3_b": "fc3.bias", "d_ln_w": "layernorm.weight",
            "d_ln_b": "layernorm.bias"}
    per_agent = lambda r, name: th.stack([r["grads"][f"{i}.{name}"] for i in range(n)], 0)
    for k, name in sums.items():
        if name.startswith("layernorm") and not layernorm:    # not written without layernorm
            assert bool((outs[k][0] == SENTINEL).all())
            continue
        bounds.check(k, outs[k][1], per_agent(ref, name), per_agent(ref32, name))

    # the node: the forward's bits, every parameter gradient of every agent, twice
    def node():
        for ag in agents:
            ag.zero_grad()
        flat_params = [p for ag in agents for p in _actor_mlp_params(ag)]
        means, h = _ActorMlpUnsharedTrainFn.apply(obs.reshape(rows, obs_dim), n, agent_id, eps, with_dh, *flat_params)
        assert "ActorMlpUnsharedTrainFn" in type(means.grad_fn).__name__ and h.requires_grad == with_dh
        loss = (means * proj).sum()
        if with_dh:
            loss = loss + (h * proj_h).sum()
        loss.backward()
        return means.detach(), h.detach(), {f"{i}.{k}": p.grad.clone() for i, ag in enumerate(agents) for k, p in ag.named_parameters()}

    m1, h1, g1 = node()
    m2, h2, g2 = node()
    assert th.equal(m1, bufs["means"][1]) and th.equal(h1, bufs["h"][1]) and th.equal(m1, m2) and th.equal(h1, h2)
    inf = fused_actor_forward_mlp_unshared(agents, obs)        # the inference launch: the same bits
    assert th.equal(inf[0], m1) and th.equal(inf[1], h1)
    assert len(g1) == (8 if layernorm else 6) * n
    for k, got in g1.items():
        assert th.equal(got, g2[k]), k
        bounds.check(k, got, ref["grads"][k], ref32["grads"][k])
    if agent_id:
        _check_id_columns(g1, n, obs_dim)
        assert th.equal(th.stack([g1[f"{i}.fc1.bias"] for i in range(n)], 0), outs["d_fc1_b"][1])


def _walk_to_node(t):
    fn, seen = t.grad_fn, 0
    while fn is not None and "ActorMlpUnsharedTrainFn" not in type(fn).__name__ and fn.next_functions and seen < 8:
        fn, seen = fn.next_functions[0][0], seen + 1
    return fn is not None and "ActorMlpUnsharedTrainFn" in type(fn).__name__


# 417: a part-filled last tile; 16 417 samples: past the 128 work-groups of 4 wavefronts per agent a wavefront walks a second tile
@pytest.mark.parametrize("b,n", [(417, 5), (16417, 2)])
def test_the_node_at_update_sizes(b, n):
    from safe_marl_amd.nets import WGRAD_MIN_ROWS, actor_mlp_unshared_train
    o, act = 30, 4
    assert b * n >= WGRAD_MIN_ROWS
    agents = _agents(n, o, act, True, True, seed=b)
    g = th.Generator(device="cuda").manual_seed(b)
    obs = 0.5 * th.randn(b, n, o, device="cuda", generator=g)
    proj = th.randn(b * n, act, device="cuda", generator=g) / (b * n)
    ref, ref32 = _both(agents, obs, True, proj)

    def run():
        for ag in agents:
            ag.zero_grad()
        means, h = actor_mlp_unshared_train(agents, obs)
        assert _walk_to_node(means) and not h.requires_grad
        (means * proj).sum().backward()
        return means.detach(), h, {f"{i}.{k}": p.grad.clone() for i, ag in enumerate(agents) for k, p in ag.named_parameters()}

    means, h, g1 = run()
    _, _, g2 = run()
    bounds = _Bounds(f"node b {b} n {n}")
    bounds.check("means", means, ref["means"].reshape(b * n, -1), ref32["means"].reshape(b * n, -1), value=True)
    bounds.check("h", h, ref["h"].reshape(b * n, -1), ref32["h"].reshape(b * n, -1), value=True)
    assert len(g1) == 8 * n
    for k, got in g1.items():
        assert th.equal(got, g2[k]), k                          # fixed-order sums everywhere: the same bits
        bounds.check(k, got, ref["grads"][k], ref32["grads"][k])
    _check_id_columns(g1, n, o)


@pytest.mark.parametrize("b,n", [(683, 3), (33, 5)])
def test_gaussian_agents(b, n):
    """MLPAgentGaussian per agent: the mean heads in the fc3 slot, the per-agent log-std heads on the node's h, their gradient
    back into the node at h."""
    from safe_marl_amd.nets import actor_mlp_unshared_train, gauss_log_std_unshared
    o, act = 30, 4
    agents = _agents(n, o, act, True, True, seed=b, gaussian=True)
    obs = 0.5 * th.randn(b, n, o, device="cuda")
    ones = th.ones(b * n, act, device="cuda")
    ref, ref32 = _both(agents, obs, True, ones, log_std_sum=True)
    for ag in agents:
        ag.zero_grad()
    means, h = actor_mlp_unshared_train(agents, obs)
    log_stds = gauss_log_std_unshared(agents, h)
    assert _walk_to_node(means) and h.requires_grad and "GaussHeadUnsharedFn" in type(log_stds.grad_fn).__name__
    (means.sum() + log_stds.sum()).backward()
    bounds = _Bounds(f"gaussian b {b} n {n}")
    bounds.check("means", means.detach(), ref["means"].reshape(b * n, -1), ref32["means"].reshape(b * n, -1), value=True)
    bounds.check("log_stds", log_stds.detach(), ref["log_stds"].reshape(b * n, -1), ref32["log_stds"].reshape(b * n, -1), value=True)
    for i, ag in enumerate(agents):
        for k, p in ag.named_parameters():
            bounds.check(f"{i}.{k}", p.grad, ref["grads"][f"{i}.{k}"], ref32["grads"][f"{i}.{k}"])


def test_permuting_the_modules_permutes_the_outputs():
    from safe_marl_amd.nets import fused_actor_forward_mlp_unshared
    n, b = 3, 33
    agents = _agents(n, 30, 4, True, False, seed=7)             # (no id columns: those follow the position, not the module)
    obs = 0.5 * th.randn(b, n, 30, device="cuda")
    m0, h0 = fused_actor_forward_mlp_unshared(agents, obs)
    perm = [2, 0, 1]
    moved = [agents[p] for p in perm]
    m1, h1 = fused_actor_forward_mlp_unshared(moved, obs[:, perm].contiguous())
    assert th.equal(m1.view(b, n, -1), m0.view(b, n, -1)[:, perm]) and th.equal(h1.view(b, n, -1), h0.view(b, n, -1)[:, perm])
    m2, _ = fused_actor_forward_mlp_unshared(moved, obs)                          # other weights on the same rows
    assert (m2 - m0).abs().max().item() > 1e-3


@pytest.mark.parametrize("n,b", [(5, 64), (3, 257)])
def test_identical_copies_agree_with_the_shared_kernel(n, b):
    """The two forms are two instantiations of ONE kernel body per direction (csrc/actor_mlp.hip): on n copies of one agent
    they give the same bits — means and h forward; dz1, dz2 backward (on the forward's own saves, a gradient at h present), and
    the per-agent form's d_fc1_b[a] is the shared form's row a of d_dz1_agent: the same rows, folded and reduced in the same
    order."""
    from safe_marl_amd import _lib
    from safe_marl_amd.nets import _actor_mlp_params, fused_actor_forward_mlp, fused_actor_forward_mlp_unshared
    obs_dim, act_dim, rows = 144, 4, b * n
    agent = _agent(n, obs_dim, act_dim, True, True, seed=3)
    copies = [copy.deepcopy(agent) for _ in range(n)]
    obs = 0.5 * th.randn(b, n, obs_dim, device="cuda")
    ms, hs = fused_actor_forward_mlp(agent, obs, n, True)
    mu, hu = fused_actor_forward_mlp_unshared(copies, obs)
    for what, got, ref in (("means", mu, ms), ("h", hu, hs)):
        print(f"n {n} b {b} {what}: against the shared-weight kernel {(got - ref).abs().max().item():.3e}")
        assert th.equal(got, ref), what

    # the backward entry points, each on its own form's forward with the saves (arguments as in
    # test_entry_points_and_node_against_the_loop)
    new = lambda *shape: th.full(shape, SENTINEL, dtype=th.float32, device="cuda")      # noqa: E731
    d_means, d_h = th.randn(rows, act_dim, device="cuda") / rows, th.randn(rows, 64, device="cuda") / rows
    bufs_u = {k: (None, new(rows, w)) for k, w in (("means", act_dim), ("h", 64), ("save_z1", 64), ("save_x", 64))}
    _lib.launch("flexnet_actor_mlp_unshared_forward", _forward_args(copies, obs, True, bufs_u))
    bufs_s = {k: new(rows, w) for k, w in (("means", act_dim), ("h", 64), ("save_z1", 64), ("save_x", 64))}
    a = _lib.FlexActorMlpArgs()
    a.rows, a.n_agents, a.obs_dim, a.act_dim, a.hid = rows, n, obs_dim, act_dim, 64
    a.agent_id, a.layernorm, a.ln_eps = 1, 1, float(agent.layernorm.eps)
    for name, p in zip(TABLES, _actor_mlp_params(agent)):
        setattr(a, name, p.data_ptr())
    a.obs = obs.data_ptr()
    for k, t in bufs_s.items():
        setattr(a, k, t.data_ptr())
    _lib.launch("flexnet_actor_mlp_forward", a)
    for k, t in bufs_s.items():
        assert th.equal(bufs_u[k][1], t), k
    assert th.equal(bufs_s["means"], ms) and th.equal(bufs_s["h"], hs)

    out_u = {"dz1": new(rows, 64), "dz2": new(rows, 64), "d_ln_w": new(n, 64), "d_ln_b": new(n, 64), "d_fc1_b": new(n, 64),
             "d_fc2_b": new(n, 64), "d_fc3_b": new(n, act_dim)}
    out_s = {"dz1": new(rows, 64), "dz2": new(rows, 64), "d_ln_w": new(64), "d_ln_b": new(64), "d_fc1_b": new(64),
             "d_fc2_b": new(64), "d_fc3_b": new(act_dim), "d_dz1_agent": new(n, 64)}
    for cls, entry, outs, saves, floats in (
            (_lib.FlexActorMlpUnsharedBwdArgs, "flexnet_actor_mlp_unshared_backward", out_u, {k: v[1] for k, v in bufs_u.items()},
             _lib.FLEXNET_ACTOR_MLP_UNSHARED_WS_FLOATS),
            (_lib.FlexActorMlpBwdArgs, "flexnet_actor_mlp_backward", out_s, bufs_s, _lib.FLEXNET_ACTOR_MLP_WS_FLOATS)):
        ws = new(floats)
        g = cls()
        g.rows, g.n_agents, g.obs_dim, g.act_dim, g.hid = rows, n, obs_dim, act_dim, 64
        g.agent_id, g.layernorm, g.ln_eps = 1, 1, float(agent.layernorm.eps)
        g.d_means, g.d_h = d_means.data_ptr(), d_h.data_ptr()
        g.z1, g.x, g.h = saves["save_z1"].data_ptr(), saves["save_x"].data_ptr(), saves["h"].data_ptr()
        if outs is out_u:
            _fill(g, copies, ("ln_w", "fc2_w", "fc3_w"))
        else:
            g.ln_w, g.fc2_w, g.fc3_w = agent.layernorm.weight.data_ptr(), agent.fc2.weight.data_ptr(), agent.fc3.weight.data_ptr()
        for k, t in outs.items():
            setattr(g, k, t.data_ptr())
        g.workspace, g.workspace_floats = ws.data_ptr(), ws.numel()
        _lib.launch(entry, g)
    th.cuda.synchronize()
    for k in ("dz1", "dz2"):
        print(f"n {n} b {b} {k}: against the shared-weight kernel {(out_u[k] - out_s[k]).abs().max().item():.3e}")
        assert th.equal(out_u[k], out_s[k]), k
    assert bool((out_u["dz1"] != SENTINEL).all()) and bool((out_s["d_dz1_agent"] != SENTINEL).all())
    for i in range(n):
        assert th.equal(out_u["d_fc1_b"][i], out_s["d_dz1_agent"][i]), i


def _model(n=5, cls="MADDPG", **over):
    import safe_marl_amd.learner as L
    args = golden_args(DIR + "unshared_mlp_maddpg", cuda=True, agent_num=n, state_size=3 * 33 + 2 * n + 1, **over)
    assert args.agent_type == "mlp" and not args.shared_params
    th.manual_seed(11)
    m = getattr(L, cls)(args).cuda()
    with th.no_grad():
        for p in m.policy_dicts.parameters():
            p.mul_(3.0).add_(0.05 * th.randn_like(p))
    return m


def test_policy_dispatch(monkeypatch):
    from safe_marl_amd import util
    from safe_marl_amd.nets import fused_actor_forward_mlp_unshared
    m = _model(5)
    b, n, o = 416, 5, m.args.obs_size
    obs = 0.5 * th.randn(b, n, o, device="cuda")
    hid = th.zeros(b, n, 64, device="cuda")
    names = _record_launches(monkeypatch)
    before = dict(util.FALLBACKS)
    with th.no_grad():
        means, log_stds, hiddens = m.policy(obs[:33], last_hid=hid[:33])  # the launch under no_grad
        direct = fused_actor_forward_mlp_unshared(list(m.policy_dicts), obs[:33])
    assert names.count(NEW[0]) == 2 and means.shape == log_stds.shape == (33, n, m.act_dim) and hiddens.shape == (33, n, 64)
    assert th.equal(means.reshape(direct[0].shape), direct[0]) and th.equal(hiddens.reshape(direct[1].shape), direct[1])
    with_node = m.policy(obs, last_hid=hid)[0]                            # 2 080 rows with gradients: the node
    assert _walk_to_node(with_node) and names.count(NEW[0]) == 3
    below = m.policy(obs[:64], last_hid=hid[:64])[0]                      # below the threshold: the loop, not a decline
    assert below.requires_grad and not _walk_to_node(below) and names.count(NEW[0]) == 3
    assert dict(util.FALLBACKS) == before
    with monkeypatch.context() as mp:                                     # standing aside for a capture (none anywhere here)
        from safe_marl_amd import learner
        mp.setattr(learner, "mlp_actor_allowed", lambda: False)
        with th.no_grad():
            aside = m.policy(obs, last_hid=hid)
        aside_grad = m.policy(obs, last_hid=hid)[0]
    assert names.count(NEW[0]) == 3 and not _walk_to_node(aside_grad) and dict(util.FALLBACKS) == before
    m.fused_inference = False                                             # the switch: the loop
    with th.no_grad():
        means0, _, hiddens0 = m.policy(obs, last_hid=hid)
    assert th.equal(aside[0], means0) and th.equal(aside[2], hiddens0) and names.count(NEW[0]) == 3
    for got, ref in ((means, means0[:33]), (hiddens, hiddens0[:33]), (with_node.detach(), means0)):
        err, bound = (got - ref).abs().max().item(), 2e-5 * max(1.0, ref.abs().max().item())
        print(f"policy() against the loop {err:.3e}, bound {bound:.3e}")
        assert err <= bound
    m.fused_inference = True
    m.policy_dicts[2].fused_training = False                              # one agent's switch: the whole list takes the loop
    assert not _walk_to_node(m.policy(obs, last_hid=hid)[0]) and dict(util.FALLBACKS) == before


def test_hid_32_declines_once_with_a_warning():
    from safe_marl_amd import util
    m = _model(3, hid_size=32)
    obs = 0.5 * th.randn(64, 3, m.args.obs_size, device="cuda")
    hid = th.zeros(64, 3, 32, device="cuda")
    util.FALLBACKS.pop("actor_mlp_unshared", None)
    with th.no_grad():
        with pytest.warns(RuntimeWarning, match="actor_mlp_unshared.*hid 32"):
            out1 = m.policy(obs, last_hid=hid)
        with warnings.catch_warnings():
            warnings.filterwarnings("error", message=".*actor_mlp_unshared.*")   # reported once per reason
            m.policy(obs, last_hid=hid)
        assert util.FALLBACKS["actor_mlp_unshared"] == 2
        m.fused_inference = False
        out0 = m.policy(obs, last_hid=hid)
    assert util.FALLBACKS["actor_mlp_unshared"] == 2
    assert th.equal(out1[0], out0[0]) and th.equal(out1[2], out0[2])
