"""GPU: csrc/attn_critic.hip (MAAC's attention critic, forward and both backward modes) against the fp64 evaluation of
nets.AttentionCritic's plain forward, with the fp32 composition as the yardstick (tests/fp64_budget.py: MARGIN 3, FLOOR_ULPS 8).

Every parameter is 0.2 randn; the inputs are drawn on a CPU generator (0.5 randn observations, tanh(randn) actions).  Shapes:
samples {1, 31, 33, 97} x agents {2, 3, 5, 8} — a lone row, both sides of the 32-sample tile, more than one work-group's worth of
wavefronts, the smallest and largest agent counts — and 2 049 x 5 through the node at an update size.  Families:

    plain      as drawn.
    zero       inputs exactly zero, the workload's own first step: every sample is the same function of the biases alone.
    saturated  K and Q scaled by 8, the logits by 64: the softmax is one-hot to fp32 and exp() of the scaled logits
               themselves would overflow — the subtracted maximum is what keeps it finite.
    mixed      samples cycle plain / zero / inputs scaled by 8 (LeakyReLU is homogeneous up to the biases, so the logits grow by
               about 64 as with K and Q scaled — a parameter change holds for a whole batch and cannot be interleaved), so one
               32-sample tile holds all three.

Gradient comparisons clear the SAMPLES with a LeakyReLU pre-activation within 1e-5 of zero in fp64 — a tie in one agent's encoder
reaches every agent of the sample through the attention.  Below 100 samples one tie is already past TIE_CAP, so the seeds of the
small shapes (SEEDS: for each shape the FIRST seed, counting from zero, without one in any family — found on the CPU in fp64, not by
looking at any kernel) have none, and zero cleared samples is asserted there.

The forward folds every eight terms of a dot product into an fp64 sum and keeps the logits' distance to the largest in fp64
(DESIGN.md §4.6j): a near-tie of the two largest saturated logits carries 64 times the logits' rounding into the attention
weights, and with one fp32 chain per layer, whose error is the composition's own, one or two such samples decided both errors
(six of the 64 small cases were then past MARGIN 3, ratios 3.3-11.6).  Measured on one MI355X with the folded sums: every case is
within the budget; over the 4 100 tensors compared the ratio err_k / err_t has median 0.59, 90th percentile 1.29, 99th 2.59."""
import math
import types
import warnings

import pytest
import torch as th

from .fp64_budget import TIE_CAP, clear_ties, ref64, within_budget

pytestmark = pytest.mark.gpu

O, A = 144, 4
SHAPES = [(b, n) for b in (1, 31, 33, 97) for n in (2, 3, 5, 8)]
FAMILIES = ("plain", "zero", "saturated", "mixed")
# (samples, agents) -> a seed whose parameters and inputs put no LeakyReLU pre-activation within 1e-5 of zero, any family
SEEDS = {(1, 2): 0, (1, 3): 0, (1, 5): 0, (1, 8): 0, (31, 2): 0, (31, 3): 0, (31, 5): 0, (31, 8): 1,
         (33, 2): 0, (33, 3): 0, (33, 5): 1, (33, 8): 1, (97, 2): 3, (97, 3): 2, (97, 5): 5, (97, 8): 9}
GUARD, SENTINEL = 256, 12345.0
NEW = ("flexnet_attn_critic_forward", "flexnet_attn_critic_backward")


def make_critic(n, seed, family="plain", obs_dim=O, act_dim=A, **over):
    from safe_marl_amd.nets import AttentionCritic
    args = types.SimpleNamespace(hid_size=64, attend_heads=1, agent_num=n, obs_size=obs_dim, action_dim=act_dim, continuous=True,
                                 norm_in=False)
    for k, v in over.items():
        setattr(args, k, v)
    g = th.Generator().manual_seed(1000 + seed)
    critic = AttentionCritic(args)
    with th.no_grad():
        for p in critic.parameters():
            p.copy_(0.2 * th.randn(p.shape, generator=g))
        if family == "saturated":
            for m in list(critic.key_extractors) + list(critic.selector_extractors):
                m.weight.mul_(8.0)
    return critic


def make_inputs(b, n, family, seed, obs_dim=O, act_dim=A):
    """(obs [b, n, o], act [b, n, a], dq [b, n]) on the CPU."""
    g = th.Generator().manual_seed(seed)
    obs = 0.5 * th.randn(b, n, obs_dim, generator=g)
    act = th.tanh(th.randn(b, n, act_dim, generator=g))
    dq = th.randn(b, n, generator=g)
    if family == "zero":
        obs, act = th.zeros_like(obs), th.zeros_like(act)
    if family == "mixed":
        kind = th.arange(b) % 3
        obs[kind == 1], act[kind == 1] = 0.0, 0.0
        obs[kind == 2] *= 8.0
        act[kind == 2] *= 8.0
    return obs, act, dq


def preacts(critic64):
    """The callable ``clear_ties`` wants: every LeakyReLU pre-activation, one row per SAMPLE."""
    def run(obs, act):
        pre = []
        critic64(obs, act, pre=pre)
        return [t.reshape(t.shape[0], -1) for t in pre]
    return run


def tie_share(b, n, family, seed):
    critic = make_critic(n, seed, family).double()
    obs, act, dq = make_inputs(b, n, family, seed)
    return clear_ties(preacts(critic), (obs.double(), act.double()), dq)


class Guarded:
    """Device tensors with GUARD sentinel floats on either side."""

    def __init__(self):
        self.all = []

    def new(self, *shape):
        numel = max(1, math.prod(shape))
        pad = (-numel) % 4                                     # the tensor itself stays 16-byte aligned
        flat = th.full((numel + pad + 2 * GUARD,), SENTINEL, dtype=th.float32, device="cuda")
        self.all.append((flat, numel))
        return flat[GUARD:GUARD + numel].view(*shape)

    def check(self):
        for flat, numel in self.all:
            assert bool((flat[:GUARD] == SENTINEL).all()) and bool((flat[GUARD + numel:] == SENTINEL).all())


def direct(critic, obs, act, dq=None, saves=True):
    """The entry points on buffers of the test's own, every output between guard rows: the forward, and with ``dq`` both
    backward modes.  Returns a dict of the outputs."""
    from safe_marl_amd import _lib
    from safe_marl_amd.nets import _attn_critic_params, _attn_critic_tables
    b, n, o = obs.shape
    a = act.shape[2]
    rows = b * n
    flat = _attn_critic_params(critic)
    g = Guarded()
    out = {k: g.new(rows, 64) for k in ("sa", "key", "val")}
    out.update(q=g.new(b, n), reg=g.new(n), ws=g.new(((b + 31) // 32) * n))
    k = _lib.FlexAttnCriticArgs()
    k.batch, k.n_agents, k.obs_dim, k.act_dim = b, n, o, a
    k.obs, k.act = obs.data_ptr(), act.data_ptr()
    _attn_critic_tables(k, flat, n)
    k.sa, k.key, k.val, k.q, k.reg = (out[x].data_ptr() for x in ("sa", "key", "val", "q", "reg"))
    k.workspace, k.workspace_floats = out["ws"].data_ptr(), out["ws"].numel()
    if saves:
        out.update({x: g.new(rows, 64) for x in ("s", "sel", "other", "hc", "hb")}, w=g.new(b, n, n))
        k.save_s, k.save_sel, k.save_other, k.save_hc, k.save_hb, k.save_w = (out[x].data_ptr() for x in
                                                                              ("s", "sel", "other", "hc", "hb", "w"))
    _lib.launch("flexnet_attn_critic_forward", k)
    if dq is not None:
        for pg in (1, 0):
            kb = _lib.FlexAttnCriticBwdArgs()
            kb.batch, kb.n_agents, kb.obs_dim, kb.act_dim, kb.param_grads = b, n, o, a, pg
            kb.dq = dq.data_ptr()
            for x in ("sa", "key", "val", "s", "sel", "hc", "hb", "w"):
                setattr(kb, x, out[x].data_ptr())
            _attn_critic_tables(kb, flat, n)
            scratch = [g.new(rows, 64), g.new(rows, 64), g.new(b, n, n)]
            kb.g_direct, kb.g_other, kb.g_dl = (t.data_ptr() for t in scratch)
            if pg:
                for x in ("dz_c", "dz_b", "dz_s", "d_sel", "d_key", "dz_v", "dz_sa"):
                    out[x] = g.new(rows, 64)
                    setattr(kb, x, out[x].data_ptr())
                out.update(d_c2_b=g.new(n), d_b2_b=g.new(n), ws_b=g.new(2 * ((b + 31) // 32) * n))
                kb.d_c2_b, kb.d_b2_b = out["d_c2_b"].data_ptr(), out["d_b2_b"].data_ptr()
                kb.workspace, kb.workspace_floats = out["ws_b"].data_ptr(), out["ws_b"].numel()
            else:
                out["d_act"] = g.new(b, n, a)
                kb.d_act = out["d_act"].data_ptr()
            _lib.launch("flexnet_attn_critic_backward", kb)
    th.cuda.synchronize()
    g.check()
    return out


def test_the_seeds_have_no_tie():
    """A condition on the inputs, checked in fp64 on the CPU (no kernel involved)."""
    assert set(SEEDS) == set(SHAPES)
    for (b, n), seed in SEEDS.items():
        for family in FAMILIES:
            assert tie_share(b, n, family, seed) == 0.0, (b, n, family, seed)


def _grads(forward, act, params, up, want_act=True, want_params=True):
    act = act.detach().clone().requires_grad_(want_act)
    q, reg = forward(act)
    wrt = ([act] if want_act else []) + (params if want_params else [])
    got = th.autograd.grad((q * up).sum(), wrt, allow_unused=True)
    return q.detach(), reg.detach(), list(got)


def _compare(critic, obs, act, up, label, kernel_forward):
    """q - b, the regulariser, d_act and every parameter gradient of the node against fp64, the composition as yardstick."""
    ref = ref64(critic)
    params = list(critic.parameters())
    names = [k for k, _ in critic.named_parameters()]
    q_t, reg_t, g_t = _grads(lambda a: critic(obs, a), act, params, up)
    q_r, reg_r, g_r = _grads(lambda a: ref(obs.double(), a), act.double(), list(ref.parameters()), up.double())
    q_k, reg_k, g_p = _grads(lambda a: kernel_forward(a, True), act, params, up, want_act=False)
    q_a, reg_a, g_a = _grads(lambda a: kernel_forward(a, False), act, params, up, want_params=False)
    assert th.equal(q_k, q_a) and th.equal(reg_k, reg_a)
    within_budget(q_k, q_t, q_r, name=f"{label} q-b")
    within_budget(reg_k, reg_t, reg_r, name=f"{label} reg")
    within_budget(g_a[0], g_t[0], g_r[0], name=f"{label} d_act")
    for k, gk, gt, gr in zip(names, g_p, g_t[1:], g_r[1:]):
        assert gk is not None, k
        within_budget(gk, gt, gr, name=f"{label} d {k}")
    return q_k, reg_k, g_a[0], g_p


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("b,n", SHAPES)
def test_kernels_within_the_fp64_budget(b, n, family):
    from safe_marl_amd.nets import attn_critic_declines, attn_critic_train, fused_attn_critic_forward
    seed = SEEDS[(b, n)]
    critic = make_critic(n, seed, family).cuda()
    obs, act, dq = (t.cuda() for t in make_inputs(b, n, family, seed))
    assert attn_critic_declines(critic, obs, act) is None
    up = dq.clone()
    share = clear_ties(preacts(ref64(critic)), (obs.double(), act.double()), up)
    assert share == 0.0                                        # (test_the_seeds_have_no_tie: known before any launch)
    label = f"attn_critic {b}x{n} {family}"
    q, reg, d_act, g_p = _compare(critic, obs, act, up, label, lambda a, pg: attn_critic_train(critic, obs, a, param_grads=pg))
    assert bool(th.isfinite(q).all()) and bool(th.isfinite(reg).all()) and float(reg.min()) >= 0.0
    # the entry points themselves, outputs between guard rows: the same bits with and without the saves, and as the node's
    plain = direct(critic, obs, act, saves=False)
    full = direct(critic, obs, act, dq=up)
    with th.no_grad():
        q0, reg0 = fused_attn_critic_forward(critic, obs, act)
    for got in (plain, full):
        assert th.equal(got["q"], q) and th.equal(got["reg"], reg)
        assert th.equal(got["sa"], full["sa"]) and th.equal(got["key"], full["key"]) and th.equal(got["val"], full["val"])
    assert th.equal(q0, q) and th.equal(reg0, reg) and th.equal(full["d_act"], d_act)
    w = full["w"]
    assert bool((w.diagonal(dim1=1, dim2=2) == 0).all()) and float((w.sum(-1) - 1).abs().max()) < 1e-5
    if family == "zero":
        assert bool((w == w[:1]).all()) and bool((q == q[:1]).all())                            # every sample is the same sample
    if family == "saturated":
        assert float(w.max(-1).values.median()) > 0.99                                          # one-hot, but for near-ties
    # two runs give the same bits
    q2, reg2, d_act2, g_p2 = _rerun(critic, obs, act, up)
    assert th.equal(q2, q) and th.equal(reg2, reg) and th.equal(d_act2, d_act)
    assert all(th.equal(x, y) for x, y in zip(g_p2, g_p))


def _rerun(critic, obs, act, up):
    from safe_marl_amd.nets import attn_critic_train
    params = list(critic.parameters())
    q, reg, g_p = _grads(lambda a: attn_critic_train(critic, obs, a, param_grads=True), act, params, up, want_act=False)
    _, _, g_a = _grads(lambda a: attn_critic_train(critic, obs, a, param_grads=False), act, params, up, want_params=False)
    return q, reg, g_a[0], g_p


@pytest.mark.parametrize("obs_dim,act_dim", [(8, 1), (140, 8), (12, 3)])
def test_other_widths(obs_dim, act_dim):
    """Observation widths that are no multiple of the eight-column MFMA group, one action and eight."""
    from safe_marl_amd.nets import attn_critic_train
    b, n, seed = 33, 3, 0                                       # (no tie at any of the three widths: found on the CPU)
    critic = make_critic(n, seed, obs_dim=obs_dim, act_dim=act_dim).cuda()
    obs, act, dq = (t.cuda() for t in make_inputs(b, n, "plain", seed, obs_dim, act_dim))
    up = dq.clone()
    share = clear_ties(preacts(ref64(critic)), (obs.double(), act.double()), up)
    assert share == 0.0
    _compare(critic, obs, act, up, f"attn_critic widths {obs_dim}+{act_dim}",
             lambda a, pg: attn_critic_train(critic, obs, a, param_grads=pg))
    direct(critic, obs, act, dq=up)


def test_the_node_at_an_update_size():
    """2 049 samples x 5 agents through ``nets.attn_critic``: the node, both modes; ties cleared per sample under the cap."""
    from safe_marl_amd import util
    from safe_marl_amd.nets import WGRAD_MIN_ROWS, _AttnCriticFn, attn_critic
    b, n, seed = 2049, 5, 3
    assert b * n >= WGRAD_MIN_ROWS
    critic = make_critic(n, seed).cuda()
    obs, act, dq = (t.cuda() for t in make_inputs(b, n, "mixed", seed))
    up = dq.clone()
    share = clear_ties(preacts(ref64(critic)), (obs.double(), act.double()), up)
    print(f"attn_critic 2049x5 mixed: {share:.4f} of the samples cleared")
    assert share <= TIE_CAP
    before = dict(util.FALLBACKS)
    seen = []

    def forward(a, pg):
        q, reg = attn_critic(critic, obs, a, critic_frozen=not pg)
        seen.append(type(q.grad_fn).__name__)
        assert not reg.requires_grad
        return q, reg

    _compare(critic, obs, act, up, "attn_critic 2049x5 mixed (node)", forward)
    assert seen and all(name == _AttnCriticFn.__name__ + "Backward" for name in seen), seen
    assert dict(util.FALLBACKS) == before


def _record_launches(monkeypatch):
    from safe_marl_amd import _lib
    names, real = [], _lib.try_launch

    def spy(name, *args, **kw):
        names.append(name)
        return real(name, *args, **kw)
    monkeypatch.setattr(_lib, "try_launch", spy)
    return names


def test_dispatch(monkeypatch):
    from safe_marl_amd import util
    from safe_marl_amd.nets import WGRAD_MIN_ROWS, attn_critic
    n = 5
    big = (WGRAD_MIN_ROWS + n - 1) // n
    critic = make_critic(n, 2).cuda()
    obs, act, _ = (t.cuda() for t in make_inputs(big, n, "plain", 2))
    names = _record_launches(monkeypatch)
    before = dict(util.FALLBACKS)
    with th.no_grad():
        q, reg = attn_critic(critic, obs[:7], act[:7])                    # no_grad: the launch at any batch size
        q_c, reg_c = critic(obs[:7], act[:7])
    assert names == [NEW[0]] and not q.requires_grad
    assert float((q - q_c).abs().max()) <= 2e-5 * max(1.0, float(q_c.abs().max())) and th.allclose(reg, reg_c, rtol=1e-4)
    below = attn_critic(critic, obs[:64], act[:64])[0]                    # gradients below the threshold: the composition,
    assert below.requires_grad and names == [NEW[0]]                      # ... silently
    node = attn_critic(critic, obs, act)[0]
    assert node.requires_grad and names == [NEW[0]] * 2
    node.sum().backward()
    assert names.count(NEW[1]) == 1 and all(p.grad is not None for p in critic.parameters())
    a = act.clone().requires_grad_()
    frozen = attn_critic(critic, obs, a, critic_frozen=True)[0]
    for p in critic.parameters():
        p.grad = None
    frozen.sum().backward()
    assert names.count(NEW[1]) == 2 and a.grad is not None and all(p.grad is None for p in critic.parameters())
    assert dict(util.FALLBACKS) == before
    import safe_marl_amd.nets as nets
    monkeypatch.setitem(nets.ATTN_CRITIC_FUSED, "no_grad", False)
    with th.no_grad():
        assert th.equal(attn_critic(critic, obs[:7], act[:7])[0], q_c)   # a gated call class: the composition
    assert names.count(NEW[0]) == 3                                       # (the launch, the node's forward twice: no more)


def test_capture_rule_without_any_capture(monkeypatch):
    """While the current stream is capturing — here: while torch is made to say so — and inside util.audit_graph_body,
    nets.attn_critic launches neither entry point, notes nothing and returns the composition's numbers; the launch helper
    itself refuses."""
    from safe_marl_amd import util
    from safe_marl_amd.nets import WGRAD_MIN_ROWS, _attn_critic_launch_forward, _attn_critic_params, attn_critic, mlp_actor_allowed
    n = 3
    critic = make_critic(n, 4).cuda()
    obs, act, _ = (t.cuda() for t in make_inputs((WGRAD_MIN_ROWS + n - 1) // n, n, "plain", 4))
    with th.no_grad():
        comp = critic(obs, act)
    names = _record_launches(monkeypatch)
    before = dict(util.FALLBACKS)

    def both_modes():
        with th.no_grad():
            a = attn_critic(critic, obs, act)
        b = attn_critic(critic, obs, act)
        assert b[0].requires_grad and "AttnCritic" not in type(b[0].grad_fn).__name__
        return a, b

    assert mlp_actor_allowed()
    with monkeypatch.context() as mp:
        mp.setattr(th.cuda, "is_current_stream_capturing", lambda: True)
        assert not mlp_actor_allowed()
        for out in both_modes():
            assert th.equal(out[0], comp[0]) and th.equal(out[1], comp[1])
        with pytest.raises(RuntimeError, match="eagerly only"):
            _attn_critic_launch_forward(_attn_critic_params(critic), obs, act)
    seen = {}
    util.audit_graph_body(lambda: seen.update(out=both_modes(), allowed=mlp_actor_allowed()),
                          allow=("reduce_kernel", "LpNorm", "batch_norm"))
    assert seen["allowed"] is False and mlp_actor_allowed()
    for out in seen["out"]:
        assert th.equal(out[0], comp[0]) and th.equal(out[1], comp[1])
    assert not [k for k in names if k in NEW], names
    assert dict(util.FALLBACKS) == before
    with th.no_grad():                                                    # the patch removed: the entry point again
        attn_critic(critic, obs, act)
    assert names.count(NEW[0]) == 1


@pytest.mark.parametrize("over,what", [(dict(attend_heads=2), "attend_heads 2"), (dict(norm_in=True), "norm_in True")])
def test_declines_once_with_a_warning(over, what):
    from safe_marl_amd import util
    from safe_marl_amd.nets import attn_critic
    critic = make_critic(3, 5, **over).cuda()
    obs, act, _ = (t.cuda() for t in make_inputs(40, 3, "plain", 5))
    util.FALLBACKS.pop("maac", None)
    with th.no_grad():
        with pytest.warns(RuntimeWarning, match="maac.*" + what):
            out1 = attn_critic(critic, obs, act)
        with warnings.catch_warnings():
            warnings.filterwarnings("error", message=".*'maac'.*")        # reported once per reason
            attn_critic(critic, obs, act)
        assert util.FALLBACKS["maac"] == 2
        out0 = critic(obs, act)
    assert util.FALLBACKS["maac"] == 2
    assert th.equal(out1[0], out0[0]) and th.equal(out1[1], out0[1])
