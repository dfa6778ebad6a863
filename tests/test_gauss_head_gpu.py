"""GPU: csrc/gauss.hip entry by entry against the torch composition evaluated in fp64 on the same fp32 inputs.

Bound, for every output: max|kernel - fp64| <= 4 max|torch fp32 - fp64| + 4 * 2^-24 * max|fp64| — the fp32 composition's own
error (another, equally valid summation order and the device's tanhf / expf are worth a small multiple of it) plus two
units in the last place of the largest entry.  Inputs: h ~ 0.5 N(0, 1), weights ~ 0.1 N(0, 1)."""
import numpy as np
import pytest
import torch as th

pytestmark = pytest.mark.gpu

ROWS = [1, 31, 32, 33, 65, 2053]
RANGES = [(0.0, 0.5), (-5.0, 2.0)]
LOW, HIGH = 0.0, 1.0


def _within(name, kernel, f32, f64):
    f64 = f64.detach().double()
    err = (kernel.detach().double() - f64).abs().max().item()
    ref = (f32.detach().double() - f64).abs().max().item()
    bound = 4.0 * ref + 4.0 * 2.0 ** -24 * f64.abs().max().item()
    print(f"{name}: kernel error {err:.3e}, fp32 composition error {ref:.3e}, bound {bound:.3e}")
    assert err <= bound, (name, err, ref, bound)


def _inputs(rows, a, seed):
    g = th.Generator(device="cuda").manual_seed(seed)
    rnd = lambda *s: th.randn(*s, device="cuda", generator=g)
    return dict(h=0.5 * rnd(rows, 64), w=0.1 * rnd(a, 64), b=0.1 * rnd(a), means=rnd(rows, a), noise=rnd(rows, a),
                d_ls=rnd(rows, a))


def _compose(x, lo, hi, dtype):
    """The composition of rnn_agent_gaussian.py:37-39, maddpg.py:88 under util.py:56-64 and util.py:125-128, with autograd."""
    from safe_marl_amd.nets import gauss_log_std_torch
    h, w, b = (x[k].detach().to(dtype).clone().requires_grad_() for k in ("h", "w", "b"))
    ls = gauss_log_std_torch(h, w, b, lo, hi)
    t = th.tanh(th.nn.functional.linear(h, w, b))
    action = th.tanh(x["means"].to(dtype) + ls.exp() * x["noise"].to(dtype))
    env = 0.5 * (th.clamp(action, min=LOW, max=HIGH) + 1.0) * (HIGH - LOW) + LOW
    d_h, d_w, d_b = th.autograd.grad(ls, (h, w, b), x["d_ls"].to(dtype))
    return dict(log_std=ls, t=t, action=action, env_action=env, d_h=d_h, d_w=d_w, d_b=d_b)


@pytest.mark.parametrize("a", [1, 4, 8])
@pytest.mark.parametrize("rows", ROWS)
def test_head_forward_epilogue_and_backward(rows, a):
    from safe_marl_amd.nets import _GaussHeadFn, gauss_head_forward
    for lo, hi in RANGES:
        x = _inputs(rows, a, 100 * rows + a)
        f32, f64 = _compose(x, lo, hi, th.float32), _compose(x, lo, hi, th.float64)
        out = gauss_head_forward(x["h"], x["w"], x["b"], lo, hi, means=x["means"], noise=x["noise"], low=LOW, high=HIGH)
        assert out is not None
        for name, got in zip(("log_std", "t", "action", "env_action"), out):
            assert got.shape == (rows, a)
            _within(f"{name} rows {rows} a {a} [{lo}, {hi}]", got, f32[name], f64[name])
        assert float(out[0].min()) >= lo and float(out[0].max()) <= hi
        plain = gauss_head_forward(x["h"], x["w"], x["b"], lo, hi, want_t=False)       # no epilogue, no saved tanh
        assert plain[1] is None and th.equal(plain[0], out[0])
        nobias = gauss_head_forward(x["h"], x["w"], None, lo, hi)
        assert th.equal(nobias[0], gauss_head_forward(x["h"], x["w"], th.zeros_like(x["b"]), lo, hi)[0])
        # the autograd node: forward again, backward through csrc/gauss.hip and csrc/wgrad.hip
        h, w, b = (x[k].clone().requires_grad_() for k in ("h", "w", "b"))
        ls = _GaussHeadFn.apply(h, w, b, lo, hi)
        assert th.equal(ls, out[0])
        d_h, d_w, d_b = th.autograd.grad(ls, (h, w, b), x["d_ls"])
        for name, got in (("d_h", d_h), ("d_w", d_w), ("d_b", d_b)):
            _within(f"{name} rows {rows} a {a} [{lo}, {hi}]", got, f32[name], f64[name])
        again = th.autograd.grad(_GaussHeadFn.apply(h, w, b, lo, hi), (h, w, b), x["d_ls"])
        assert all(th.equal(p, q) for p, q in zip(again, (d_h, d_w, d_b)))           # no atomics: the same bits


@pytest.mark.parametrize("n,a", [(1, 4), (3, 1), (3, 4), (5, 4), (5, 8), (8, 8)])
@pytest.mark.parametrize("envs", [1, 33, 2053])
def test_sum_explore(envs, n, a):
    import torch.distributions.normal as tdn
    from safe_marl_amd.learner import _summed_exploration_rows
    from safe_marl_amd.util import convert
    g = th.Generator(device="cuda").manual_seed(7 * envs + n + a)
    means = th.randn(envs, n, a, device="cuda", generator=g)
    log_stds = 0.5 * th.randn(envs, n, a, device="cuda", generator=g) - 0.3
    model = type("M", (), {"args": convert(dict(action_low=LOW, action_high=HIGH))})()
    env_action = th.empty(envs, n, a, device="cuda")
    th.manual_seed(11)
    out = _summed_exploration_rows(model, means, log_stds, env_action, None)
    th.manual_seed(11)
    eps = tdn._standard_normal((envs, 1, a), th.float32, means.device)
    ref = {}
    for dtype in (th.float32, th.float64):
        y = th.tanh(means.to(dtype).sum(1, keepdim=True) + log_stds.to(dtype).sum(1, keepdim=True).exp() * eps.to(dtype))
        ref[dtype] = (y.expand(envs, n, a), (0.5 * (th.clamp(y, min=LOW, max=HIGH) + 1.0) * (HIGH - LOW) + LOW).expand(envs, n, a))
    _within(f"action envs {envs} n {n} a {a}", out, ref[th.float32][0], ref[th.float64][0])
    _within(f"env_action envs {envs} n {n} a {a}", env_action, ref[th.float32][1], ref[th.float64][1])
    assert all(th.equal(out[:, i], out[:, 0]) for i in range(n))                     # the ONE action, to every agent


def _ppo_inputs(rows, n, a, seed, with_old, wide=False):
    """PPO's operating regime: ratios of order one, some inside and some outside the clip range.  ratio = exp(log p - old)
    turns the ABSOLUTE fp32 error of its argument into a relative one, so where the argument is of order ten (ratios in the
    hundreds) the largest error of ratio, d_means and d_log_stds alike is the half-ulp luck of the single largest element, in
    the kernel and in the fp32 composition alike — a comparison of two such maxima says nothing about either.  With
    ``old`` = None the reference's own choice applies, old = the sum of the action's components (model.py:313): the actions
    are centred so that this sum is near the log-density (about -0.9 per component).
    ``wide``: uncentred means and a wider action spread instead — arguments of order ten, ratios up to the hundreds
    (test_ppo_policy_loss_rows_with_large_ratios)."""
    g = th.Generator(device="cuda").manual_seed(seed)
    rnd = lambda *s: th.randn(*s, device="cuda", generator=g)
    if wide:
        means, log_stds = 0.3 * rnd(rows, n, a), 0.15 * rnd(rows, n, a) - 0.05
        one = means.sum(1, keepdim=True) + 0.7 * rnd(rows, 1, a)
    else:
        means, log_stds = -0.9 / n + 0.1 / n ** 0.5 * rnd(rows, n, a), 0.15 / n ** 0.5 * rnd(rows, n, a) - 0.05 / n
        one = means.sum(1, keepdim=True) + 0.25 * rnd(rows, 1, a)                     # ippo.py:72-73: one action for every agent
    actions = one.expand(rows, n, a).contiguous()
    adv = rnd(rows, n)
    old = None
    if with_old:                                                                     # a stored log-density, [rows, n, a]
        old = (-0.5 * ((actions - means.sum(1, keepdim=True)) ** 2) - 0.9 + 0.1 * rnd(rows, n, a)).contiguous()
    return means, log_stds, actions, old, adv


@pytest.mark.parametrize("rows,n,a,with_old", [(1, 3, 4, False), (33, 1, 4, True), (65, 3, 8, False), (65, 5, 4, True),
                                               (2053, 5, 4, False), (2053, 8, 8, True), (100000, 5, 4, False)])
def test_ppo_policy_loss_rows(rows, n, a, with_old):
    from safe_marl_amd.nets import ppo_policy_loss, ppo_policy_loss_torch
    from safe_marl_amd.util import FALLBACKS
    eps_clip = 0.2
    means, log_stds, actions, old, adv = _ppo_inputs(rows, n, a, rows + 10 * n + a, with_old)
    ref = {}
    for dtype in (th.float32, th.float64):
        m, ls = (x.detach().to(dtype).clone().requires_grad_() for x in (means, log_stds))
        o = (actions if old is None else old).to(dtype)
        loss, ratio = ppo_policy_loss_torch(m, ls, actions.to(dtype), o, adv.to(dtype), eps_clip)
        ref[dtype] = (loss, ratio) + th.autograd.grad(loss, (m, ls))
    before = FALLBACKS.get("ppo_policy_loss", 0)
    m, ls = means.detach().clone().requires_grad_(), log_stds.detach().clone().requires_grad_()
    loss, ratio = ppo_policy_loss(m, ls, actions, old, adv, eps_clip)
    assert FALLBACKS.get("ppo_policy_loss", 0) == before                             # the kernel ran
    d_m, d_ls = th.autograd.grad(loss, (m, ls))
    for name, got, i in (("loss", loss, 0), ("ratio", ratio, 1), ("d_means", d_m, 2), ("d_log_stds", d_ls, 3)):
        _within(f"{name} rows {rows} n {n} a {a} old {with_old}", got, ref[th.float32][i], ref[th.float64][i])
    assert float(d_ls.abs().max()) > 0 and all(th.equal(d_ls[:, i], d_ls[:, 0]) for i in range(n))
    loss2, _ = ppo_policy_loss(m, ls, actions, old, adv, eps_clip)
    assert th.equal(loss2, loss)                                                     # fixed-order sums: the same bits


def test_ppo_policy_loss_rows_with_large_ratios():
    """The same kernel where log p - old is of order ten and the ratios reach the hundreds (old = None on uncentred
    actions).  There the LARGEST error of an output is that of its one largest element — half a unit in the last place of an
    order-ten exponent, either way, for the kernel and the fp32 composition alike — so the bound keeps its form and its
    factors and takes the root mean square over the 500 000 / 2 000 000 elements in place of the maximum:
    rms(kernel - fp64) <= 4 rms(torch fp32 - fp64) + 4 * 2^-24 rms(fp64).  An arithmetic that lost accuracy at large
    arguments (a sloppier exponent, a cancelling rearrangement) would raise every large element's error, hence the rms."""
    from safe_marl_amd.nets import ppo_policy_loss, ppo_policy_loss_torch
    rows, n, a, eps_clip = 100000, 5, 4, 0.2
    means, log_stds, actions, _, adv = _ppo_inputs(rows, n, a, 77, False, wide=True)
    ref = {}
    for dtype in (th.float32, th.float64):
        m, ls = (x.detach().to(dtype).clone().requires_grad_() for x in (means, log_stds))
        loss, ratio = ppo_policy_loss_torch(m, ls, actions.to(dtype), actions.to(dtype), adv.to(dtype), eps_clip)
        ref[dtype] = (loss, ratio) + th.autograd.grad(loss, (m, ls))
    assert ref[th.float64][1].max().item() > 50.0                                    # the regime this case is about
    m, ls = means.detach().clone().requires_grad_(), log_stds.detach().clone().requires_grad_()
    loss, ratio = ppo_policy_loss(m, ls, actions, None, adv, eps_clip)
    d_m, d_ls = th.autograd.grad(loss, (m, ls))
    rms = lambda x: x.double().pow(2).mean().sqrt().item()
    for name, got, i in (("loss", loss, 0), ("ratio", ratio, 1), ("d_means", d_m, 2), ("d_log_stds", d_ls, 3)):
        f32, f64 = ref[th.float32][i].detach().double(), ref[th.float64][i].detach()
        err, own = rms(got.detach().double() - f64), rms(f32 - f64)
        bound = 4.0 * own + 4.0 * 2.0 ** -24 * rms(f64)
        print(f"{name} (large ratios): kernel rms error {err:.3e}, fp32 composition rms error {own:.3e}, bound {bound:.3e}")
        assert err <= bound, (name, err, own, bound)


def test_limits_are_refused():
    from safe_marl_amd import _lib
    from safe_marl_amd.nets import _ppo_policy_loss_fused, gauss_head_forward, gauss_log_std, gauss_log_std_torch
    from safe_marl_amd.util import FALLBACKS
    _lib.load()
    h32, w32 = th.randn(8, 32, device="cuda"), th.randn(4, 32, device="cuda")
    assert gauss_head_forward(h32, w32, None, 0.0, 0.5) is None                      # hid != 64
    h, w9 = th.randn(8, 64, device="cuda"), th.randn(9, 64, device="cuda")
    assert gauss_head_forward(h, w9, None, 0.0, 0.5) is None                         # act_dim > FLEXNET_MAX_ACT
    before = FALLBACKS.get("gauss_head", 0)
    for hh, ww in ((h32, w32), (h, w9)):                                             # the caller runs the composition, visibly
        assert th.equal(gauss_log_std(hh, ww, None, 0.0, 0.5), gauss_log_std_torch(hh, ww, None, 0.0, 0.5))
    assert FALLBACKS.get("gauss_head", 0) == before + 2
    s = _lib.FlexGaussSumArgs()
    buf = th.zeros(9 * 9 * 4, device="cuda")
    s.n_envs, s.n_agents, s.act_dim, s.act_high = 4, 9, 4, 1.0
    s.means = s.log_stds = s.eps = s.action = buf.data_ptr()
    assert not _lib.try_launch("flexnet_gauss_sum_explore", s)                       # n_agents > FLEXNET_MAX_AGENTS
    s.n_agents, s.act_dim = 5, 9
    assert not _lib.try_launch("flexnet_gauss_sum_explore", s)
    means, log_stds, actions, _, adv = _ppo_inputs(4, 9, 4, 3, False)
    assert _ppo_policy_loss_fused(means, log_stds.requires_grad_(), actions, None, adv, 0.2, per_row=True) is None
    th.cuda.synchronize()
