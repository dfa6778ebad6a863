"""GPU: the MLP actor of ``agent_type: mlp`` in one launch per direction (csrc/actor_mlp.hip; nets.fused_actor_forward_mlp,
nets._ActorMlpTrainFn) against the module's composition (mlp_agent.py:20-32 on the rows [obs | onehot(r % n)]) in fp64, and
``Model.policy``'s dispatch with its capture rule.  Nothing here captures a HIP graph: the rule is tested by patching what it
asks.

Bounds are tests/test_critic_unshared_gpu.py's, restated: values 2e-5 max(1, max|ref|), gradients 2e-6 + 3e-4 max|ref|, or
four times the error of the fp32 composition on the device against the same fp64 reference where that is larger; every check
prints which applied."""
import copy
import itertools
import json
import os
import warnings

import pytest
import torch as th
import torch.nn.functional as F

from .golden_io import golden_args

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(__file__), "golden")
SENTINEL = -12345.0
GUARD = 3                       # guard rows on either side of every output
NEW = ("flexnet_actor_mlp_forward", "flexnet_actor_mlp_backward")


def _agent(n, obs_dim, act_dim, layernorm, agent_id, seed, gaussian=False):
    """An MLP agent with seeded weights scaled up (the default init is tiny: make every term matter)."""
    from safe_marl_amd.nets import MLPAgent, MLPAgentGaussian
    from safe_marl_amd.util import convert
    d = json.load(open(os.path.join(G, "learner_args.json")))
    d.update(agent_num=n, action_dim=act_dim, layernorm=layernorm, agent_id=agent_id, obs_size=obs_dim, agent_type="mlp",
             gaussian_policy=gaussian)
    th.manual_seed(seed)
    agent = (MLPAgentGaussian if gaussian else MLPAgent)(obs_dim + (n if agent_id else 0), convert(d)).cuda()
    with th.no_grad():
        for p in agent.parameters():
            p.mul_(3.0).add_(0.05 * th.randn_like(p))
    return agent


def _guarded(rows, width):
    """[rows, width] between GUARD sentinel rows: (the whole buffer, the interior view)."""
    buf = th.full((rows + 2 * GUARD, width), SENTINEL, dtype=th.float32, device="cuda")
    return buf, buf[GUARD:GUARD + rows]


def _guards_untouched(buf):
    return bool((buf[:GUARD] == SENTINEL).all() and (buf[-GUARD:] == SENTINEL).all())


def _composition(agent, obs, n, agent_id, proj, proj_h=None, log_std_sum=False):
    """The module's layers on its materialised input rows, in the dtype of ``obs``: means, h, z1, x, dz1, dz2 and every
    parameter gradient of (means proj).sum() (+ (h proj_h).sum()) (+ log_stds.sum())."""
    b, _, o = obs.shape
    rows = obs.reshape(b * n, o)
    if agent_id:
        rows = th.cat((rows, th.eye(n, dtype=obs.dtype, device=obs.device).repeat(b, 1)), 1)
    agent.zero_grad()
    z1 = agent.fc1(rows)
    z1.retain_grad()
    x = F.relu(agent.layernorm(z1) if agent.args.layernorm else z1)
    z2 = agent.fc2(x)
    z2.retain_grad()
    h = F.relu(z2)
    means = agent.fc3(h)
    with th.no_grad():                                                  # the module itself
        out = agent(rows, None)
        assert (out[0] - means).abs().max().item() <= 1e-6 * max(1.0, means.abs().max().item())
        assert (out[2] - h).abs().max().item() <= 1e-6 * max(1.0, h.abs().max().item())
    loss = (means * proj).sum()
    res = {}
    if proj_h is not None:
        loss = loss + (h * proj_h).sum()
    if log_std_sum:
        a = agent.args
        res["log_stds"] = a.LOG_STD_MIN + 0.5 * (a.LOG_STD_MAX - a.LOG_STD_MIN) * (th.tanh(agent.log_std(h)) + 1)
        with th.no_grad():
            assert (out[1] - res["log_stds"]).abs().max().item() <= 1e-6
        loss = loss + res["log_stds"].sum()
        res["log_stds"] = res["log_stds"].detach()
    loss.backward()
    res.update(means=means.detach(), h=h.detach(), z1=z1.detach(), x=x.detach(), dz1=z1.grad, dz2=z2.grad,
               grads={k: p.grad.clone() for k, p in agent.named_parameters()})
    return res


class _Bounds:
    """The larger of the project's bound and 4 x the fp32 device composition's own error against the fp64 reference."""

    def __init__(self, case):
        self.case = case

    def check(self, what, got, ref64, ref32, value=False):
        ref_max = ref64.abs().max().item()
        project = 2e-5 * max(1.0, ref_max) if value else 2e-6 + 3e-4 * ref_max
        comp = 4.0 * (ref32.double() - ref64).abs().max().item()
        err = (got.double() - ref64).abs().max().item()
        bound = max(project, comp)
        print(f"{self.case} {what}: error {err:.3e}, project bound {project:.3e}, 4 x fp32 composition {comp:.3e} -> "
              f"{'project' if project >= comp else 'composition'} bound applies")
        assert err <= bound, (self.case, what, err, bound)


# every b with every n (the part-filled tiles); 257: a third work-group per agent whose only tile holds one row.  obs_dim,
# act_dim, layernorm and agent_id cycle at different periods so that the last two occur on and off with every obs_dim.
_BN = list(itertools.product([1, 31, 33, 64], [1, 2, 3, 5, 8])) + [(257, 3), (257, 8)]
CASES = [(b, n, [6, 30, 144][k % 3], [2, 4, 8][(k // 3) % 3], (k // 3) % 2 == 0, (k // 6) % 2 == 0) for k, (b, n) in enumerate(_BN)]


def test_the_cases_cover_every_value():
    for col, values in ((2, {6, 30, 144}), (3, {2, 4, 8}), (4, {True, False}), (5, {True, False})):
        assert {c[col] for c in CASES} == values
    assert {(c[0], c[1]) for c in CASES} == set(_BN)
    for o in (6, 30, 144):
        assert {c[4] for c in CASES if c[2] == o} == {True, False} and {c[5] for c in CASES if c[2] == o} == {True, False}


def _forward_args(agent, obs, n, agent_id, bufs):
    from safe_marl_amd import _lib
    from safe_marl_amd.nets import _actor_mlp_params
    a = _lib.FlexActorMlpArgs()
    a.rows, a.n_agents, a.obs_dim, a.act_dim, a.hid = obs.shape[0] * n, n, obs.shape[-1], agent.args.action_dim, 64
    a.agent_id, a.layernorm = int(agent_id), int(agent.args.layernorm)
    a.ln_eps = float(agent.layernorm.eps) if agent.args.layernorm else 1e-5
    for name, p in zip(("fc1_w", "fc1_b", "ln_w", "ln_b", "fc2_w", "fc2_b", "fc3_w", "fc3_b"), _actor_mlp_params(agent)):
        if p is not None:
            setattr(a, name, p.data_ptr())
    a.obs = obs.data_ptr()
    for k, (_, view) in bufs.items():
        setattr(a, k, view.data_ptr())
    return a


@pytest.mark.parametrize("b,n,obs_dim,act_dim,layernorm,agent_id", CASES)
def test_entry_points_and_node_against_the_composition(b, n, obs_dim, act_dim, layernorm, agent_id):
    from safe_marl_amd import _lib
    from safe_marl_amd.nets import _ActorMlpTrainFn, _actor_mlp_params, fused_actor_forward_mlp
    agent = _agent(n, obs_dim, act_dim, layernorm, agent_id, seed=b + n)
    g = th.Generator(device="cuda").manual_seed(100 * b + n)
    rows = b * n
    obs = 0.5 * th.randn(b, n, obs_dim, device="cuda", generator=g)
    proj = th.randn(rows, act_dim, device="cuda", generator=g) / rows
    with_dh = (b + n) % 2 == 0                                 # every other case: a gradient arrives at h as well
    proj_h = th.randn(rows, 64, device="cuda", generator=g) / rows if with_dh else None
    ref32 = _composition(agent, obs, n, agent_id, proj, proj_h)
    ref = _composition(copy.deepcopy(agent).double(), obs.double(), n, agent_id, proj.double(),
                       None if proj_h is None else proj_h.double())
    bounds = _Bounds(f"b {b} n {n} o {obs_dim} a {act_dim} ln {layernorm} id {agent_id} d_h {with_dh}")
    eps = float(agent.layernorm.eps) if layernorm else 1e-5

    # forward with the two saves, every output between guard rows
    bufs = {"means": _guarded(rows, act_dim), "h": _guarded(rows, 64), "save_z1": _guarded(rows, 64), "save_x": _guarded(rows, 64)}
    a = _forward_args(agent, obs, n, agent_id, bufs)
    _lib.launch("flexnet_actor_mlp_forward", a)
    th.cuda.synchronize()
    for k, (buf, _) in bufs.items():
        assert _guards_untouched(buf), k
    for k, name in (("means", "means"), ("h", "h"), ("save_z1", "z1"), ("save_x", "x")):
        bounds.check(name, bufs[k][1], ref[name], ref32[name], value=True)
    again = {"means": _guarded(rows, act_dim), "h": _guarded(rows, 64)}      # the same launch without the saves: the same bits
    a2 = _forward_args(agent, obs, n, agent_id, again)
    _lib.launch("flexnet_actor_mlp_forward", a2)
    th.cuda.synchronize()
    assert th.equal(again["means"][0], bufs["means"][0]) and th.equal(again["h"][0], bufs["h"][0])

    # backward from the kernel's own saves
    outs = {"dz1": _guarded(rows, 64), "dz2": _guarded(rows, 64), "d_ln_w": _guarded(1, 64), "d_ln_b": _guarded(1, 64),
            "d_fc1_b": _guarded(1, 64), "d_fc2_b": _guarded(1, 64), "d_fc3_b": _guarded(1, act_dim), "d_dz1_agent": _guarded(n, 64)}
    ws = th.full((_lib.FLEXNET_ACTOR_MLP_WS_FLOATS,), SENTINEL, dtype=th.float32, device="cuda")
    gb = _lib.FlexActorMlpBwdArgs()
    gb.rows, gb.n_agents, gb.obs_dim, gb.act_dim, gb.hid = rows, n, obs_dim, act_dim, 64
    gb.agent_id, gb.layernorm, gb.ln_eps = int(agent_id), int(layernorm), eps
    gb.d_means = proj.data_ptr()
    if with_dh:
        gb.d_h = proj_h.data_ptr()
    gb.z1, gb.x, gb.h = bufs["save_z1"][1].data_ptr(), bufs["save_x"][1].data_ptr(), bufs["h"][1].data_ptr()
    params = _actor_mlp_params(agent)
    gb.fc2_w, gb.fc3_w = params[4].data_ptr(), params[6].data_ptr()
    if layernorm:
        gb.ln_w = params[2].data_ptr()
    for k, (_, view) in outs.items():
        setattr(gb, k, view.data_ptr())
    gb.workspace, gb.workspace_floats = ws.data_ptr(), ws.numel()
    _lib.launch("flexnet_actor_mlp_backward", gb)
    th.cuda.synchronize()
    for k, (buf, _) in outs.items():
        assert _guards_untouched(buf), k
    first = {k: buf.clone() for k, (buf, _) in outs.items()}
    _lib.launch("flexnet_actor_mlp_backward", gb)              # fixed-order sums: the same bits
    th.cuda.synchronize()
    for k, (buf, _) in outs.items():
        assert th.equal(first[k], buf), k
    bounds.check("dz1", outs["dz1"][1], ref["dz1"], ref32["dz1"])
    bounds.check("dz2", outs["dz2"][1], ref["dz2"], ref32["dz2"])
    sums = {"d_fc1_b": "fc1.bias", "d_fc2_b": "fc2.bias", "d_fc3_b": "fc3.bias", "d_ln_w": "layernorm.weight",
            "d_ln_b": "layernorm.bias"}
    for k, name in sums.items():
        if name.startswith("layernorm") and not layernorm:    # not written without layernorm
            assert bool((outs[k][0] == SENTINEL).all())
            continue
        bounds.check(k, outs[k][1][0], ref["grads"][name], ref32["grads"][name])
    per_agent = lambda r: r["dz1"].view(b, n, 64).sum(0)
    bounds.check("d_dz1_agent", outs["d_dz1_agent"][1], per_agent(ref), per_agent(ref32))

    # the node: the forward's bits, every parameter gradient, twice
    def node():
        agent.zero_grad()
        means, h = _ActorMlpTrainFn.apply(obs.reshape(rows, obs_dim), n, agent_id, eps, with_dh, *_actor_mlp_params(agent))
        assert "ActorMlpTrainFn" in type(means.grad_fn).__name__ and h.requires_grad == with_dh
        loss = (means * proj).sum()
        if with_dh:
            loss = loss + (h * proj_h).sum()
        loss.backward()
        return means.detach(), h.detach(), {k: p.grad.clone() for k, p in agent.named_parameters()}

    m1, h1, g1 = node()
    m2, h2, g2 = node()
    assert th.equal(m1, bufs["means"][1]) and th.equal(h1, bufs["h"][1]) and th.equal(m1, m2) and th.equal(h1, h2)
    inf = fused_actor_forward_mlp(agent, obs, n, agent_id)     # the inference launch: the same bits
    assert th.equal(inf[0], m1) and th.equal(inf[1], h1)
    assert len(g1) == (8 if layernorm else 6)
    for k, got in g1.items():
        assert th.equal(got, g2[k]), k
        bounds.check(k, got, ref["grads"][k], ref32["grads"][k])
    if agent_id:                                               # the id columns: the per-agent sums of dz1
        assert th.equal(g1["fc1.weight"][:, obs_dim:], outs["d_dz1_agent"][1].t())


def _walk_to_node(t):
    fn, seen = t.grad_fn, 0
    while fn is not None and "ActorMlpTrainFn" not in type(fn).__name__ and fn.next_functions and seen < 8:
        fn, seen = fn.next_functions[0][0], seen + 1
    return fn is not None and "ActorMlpTrainFn" in type(fn).__name__


def test_the_node_at_an_update_size():
    """2 049 rows (>= WGRAD_MIN_ROWS): three tiles short of a multiple, every parameter gradient through flexnet_wgrad_batched."""
    from safe_marl_amd.nets import WGRAD_MIN_ROWS, actor_mlp_train
    b, n, o, act = 683, 3, 30, 4
    assert b * n >= WGRAD_MIN_ROWS
    agent = _agent(n, o, act, True, True, seed=5)
    obs = 0.5 * th.randn(b, n, o, device="cuda")
    proj = th.randn(b * n, act, device="cuda") / (b * n)
    ref32 = _composition(agent, obs, n, True, proj)
    ref = _composition(copy.deepcopy(agent).double(), obs.double(), n, True, proj.double())
    agent.zero_grad()
    means, h = actor_mlp_train(agent, obs, n, True)
    assert _walk_to_node(means) and not h.requires_grad
    (means * proj).sum().backward()
    bounds = _Bounds("node b 683 n 3")
    bounds.check("means", means.detach(), ref["means"], ref32["means"], value=True)
    bounds.check("h", h, ref["h"], ref32["h"], value=True)
    for k, p in agent.named_parameters():
        bounds.check(k, p.grad, ref["grads"][k], ref32["grads"][k])


@pytest.mark.parametrize("b,n", [(683, 3), (33, 5)])
def test_gaussian_agent(b, n):
    """MLPAgentGaussian: the mean head in the fc3 slot, the log-std head through csrc/gauss.hip on the node's h, its gradient
    back into the node at h."""
    from safe_marl_amd.nets import actor_mlp_train
    o, act = 30, 4
    agent = _agent(n, o, act, True, True, seed=b, gaussian=True)
    assert not any("fc3." in k for k in agent.state_dict()) and {"mean.weight", "log_std.weight"} <= set(agent.state_dict())
    obs = 0.5 * th.randn(b, n, o, device="cuda")
    ones = th.ones(b * n, act, device="cuda")
    ref32 = _composition(agent, obs, n, True, ones, log_std_sum=True)
    ref = _composition(copy.deepcopy(agent).double(), obs.double(), n, True, ones.double(), log_std_sum=True)
    agent.zero_grad()
    means, h = actor_mlp_train(agent, obs, n, True)
    log_stds = agent.log_std_of(h)
    assert _walk_to_node(means) and h.requires_grad and "GaussHeadFn" in type(log_stds.grad_fn).__name__
    (means.sum() + log_stds.sum()).backward()
    bounds = _Bounds(f"gaussian b {b} n {n}")
    bounds.check("means", means.detach(), ref["means"], ref32["means"], value=True)
    bounds.check("log_stds", log_stds.detach(), ref["log_stds"], ref32["log_stds"], value=True)
    for k, p in agent.named_parameters():
        bounds.check(k, p.grad, ref["grads"][k], ref32["grads"][k])


def _model(prefix, cls, **over):
    import safe_marl_amd.learner as L
    args = golden_args(prefix, cuda=True, **over)
    assert args.agent_type == "mlp" and args.shared_params
    th.manual_seed(11)
    m = getattr(L, cls)(args).cuda()
    with th.no_grad():
        for p in m.policy_dicts.parameters():
            p.mul_(3.0).add_(0.05 * th.randn_like(p))
    return m


def _record_launches(monkeypatch):
    from safe_marl_amd import _lib
    names, real = [], _lib.try_launch

    def spy(name, *args, **kw):
        names.append(name)
        return real(name, *args, **kw)
    monkeypatch.setattr(_lib, "try_launch", spy)
    return names


MODELS = [("mlp_maddpg", "MADDPG"), ("mlp_ippo", "IPPO")]


@pytest.mark.parametrize("prefix,cls", MODELS)
def test_policy_dispatch(prefix, cls):
    from safe_marl_amd import util
    from safe_marl_amd.nets import WGRAD_MIN_ROWS
    m = _model(prefix, cls)
    n, o = m.n_, m.obs_dim
    big = (WGRAD_MIN_ROWS + n - 1) // n
    obs = 0.5 * th.randn(big, n, o, device="cuda")
    before = dict(util.FALLBACKS)
    with th.no_grad():
        means, _, hiddens = m.policy(obs[:33])
        from safe_marl_amd.nets import fused_actor_forward_mlp
        direct = fused_actor_forward_mlp(m.policy_dicts[0], obs[:33], n, m.args.agent_id)
    assert util.FALLBACKS.get("actor_forward", 0) == before.get("actor_forward", 0)
    assert means.shape == (33, n, m.act_dim) and hiddens.shape == (33, n, 64)
    assert th.equal(means.reshape(direct[0].shape), direct[0]) and th.equal(hiddens.reshape(direct[1].shape), direct[1])
    with_node = m.policy(obs)[0]                                        # gradients at >= WGRAD_MIN_ROWS rows: the node
    assert _walk_to_node(with_node)
    below = m.policy(obs[:64])[0]                                       # below: the composition, not a decline
    assert below.requires_grad and not _walk_to_node(below)
    assert dict(util.FALLBACKS) == before
    m.fused_inference = False                                           # the switch: the composition
    with th.no_grad():
        means0, _, hiddens0 = m.policy(obs)
    for got, ref in ((means, means0[:33]), (hiddens, hiddens0[:33]), (with_node.detach(), means0)):
        err, bound = (got - ref).abs().max().item(), 2e-5 * max(1.0, ref.abs().max().item())
        print(f"{cls}: policy() against the composition {err:.3e}, bound {bound:.3e}")
        assert err <= bound


@pytest.mark.parametrize("prefix,cls", MODELS)
def test_capture_rule_without_any_capture(prefix, cls, monkeypatch):
    """While the current stream is capturing — here: while torch is made to say so — and inside util.audit_graph_body, policy()
    launches neither new entry point, notes nothing and returns the composition's numbers."""
    from safe_marl_amd import util
    from safe_marl_amd.nets import WGRAD_MIN_ROWS, mlp_actor_allowed
    m = _model(prefix, cls)
    n, o = m.n_, m.obs_dim
    obs = 0.5 * th.randn((WGRAD_MIN_ROWS + n - 1) // n, n, o, device="cuda")
    m.fused_inference = False
    with th.no_grad():
        comp = m.policy(obs)
    m.fused_inference = True
    names = _record_launches(monkeypatch)
    before = dict(util.FALLBACKS)

    def both_modes():
        with th.no_grad():
            a = m.policy(obs)
        b = m.policy(obs)
        assert b[0].requires_grad and not _walk_to_node(b[0])
        return a, b

    assert mlp_actor_allowed()
    with monkeypatch.context() as mp:
        mp.setattr(th.cuda, "is_current_stream_capturing", lambda: True)
        assert not mlp_actor_allowed()
        for out in both_modes():
            assert th.equal(out[0], comp[0]) and th.equal(out[2], comp[2])
    assert mlp_actor_allowed()
    seen = {}
    util.audit_graph_body(lambda: seen.update(out=both_modes(), allowed=mlp_actor_allowed()))
    assert seen["allowed"] is False and mlp_actor_allowed()
    for out in seen["out"]:
        assert th.equal(out[0], comp[0]) and th.equal(out[2], comp[2])
    assert not [k for k in names if k in NEW], names
    assert dict(util.FALLBACKS) == before
    with th.no_grad():                                                  # the patch removed: the entry points again
        m.policy(obs)
    assert names.count(NEW[0]) == 1 and NEW[1] not in names
    m.policy(obs)[0].sum().backward()
    assert names.count(NEW[0]) == 2 and names.count(NEW[1]) == 1


@pytest.mark.parametrize("over,what", [(dict(hid_size=32), "hid 32"), (dict(hid_activation="tanh"), "act tanh")])
def test_declines_once_with_a_warning(over, what):
    from safe_marl_amd import util
    m = _model("mlp_maddpg", "MADDPG", **over)
    obs = 0.5 * th.randn(64, m.n_, m.obs_dim, device="cuda")
    util.FALLBACKS.pop("actor_forward", None)
    with th.no_grad():
        with pytest.warns(RuntimeWarning, match="actor_forward.*" + what):
            out1 = m.policy(obs)
        with warnings.catch_warnings():
            warnings.filterwarnings("error", message=".*actor_forward.*")     # reported once per reason
            m.policy(obs)
        assert util.FALLBACKS["actor_forward"] == 2
        m.fused_inference = False
        out0 = m.policy(obs)
    assert util.FALLBACKS["actor_forward"] == 2
    assert th.equal(out1[0], out0[0]) and th.equal(out1[2], out0[2])
