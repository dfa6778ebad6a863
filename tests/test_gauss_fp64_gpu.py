"""csrc/gauss.hip's log-std head on the fp64 error budget of tests/fp64_budget.py — the shared head (nets.gauss_head_forward
with the exploration epilogue, nets._GaussHeadFn) and every agent's own (flexnet_gauss_head_unshared_*, nets._GaussHeadUnsharedFn)
against ``fb.gauss_head_plain`` in fp64 on the same fp32 numbers, on the families of ``fb.gauss_families``: a hidden state of
zero, a saturated head (t = +-1, gradients exactly zero), a range of zero width, noise that saturates the action onto both
clamp ends, and rows of each kind inside one 32-row tile.  d_w and d_b are sums over the rows, of at most 129 here: every one
met the plain budget, none takes fb.row_sum_rounding.  The one derived floor is log_std's (``_log_std_floor``: ulps of the
range's ends, not of a single small result).  Then what needs no tolerance: a launch's first rows
are the launch on them alone, and a NaN stays where it is — in its row of the head, in its environment of the two agent-summed
exploration kernels (flexnet_gauss_sum_explore, flexnet_agent_sum_explore), whose env_action an environment would be stepped
with: th.clamp hands a NaN on, and so must they.  The figures of a run are filed in profiles/fp64_error_budget.txt."""
import pytest
import torch as th

from . import fp64_budget as fb

pytestmark = pytest.mark.gpu

ROWS = (1, 31, 32, 33, 129)
ACTS = (1, 3, 8)
UNSHARED = [(1, 1, 1), (33, 3, 4), (31, 8, 8), (129, 5, 3)]           # (b, n, a)
BOUNDS = [(0.0, 1.0), (-1.0, 1.0)]                                    # [LOW, HIGH] of translate_action
FORWARD = ("log_std", "t", "action", "env_action")


def head_case(rows, a, family, n=None):
    """The family's inputs on the CPU (seeded by the shape) and the log-std ranges it runs at."""
    fam = fb.gauss_families(rows, a, th.Generator().manual_seed(1000 * rows + 10 * a + (n or 0)), n=n)[family]
    return fam, ([fam.params["range"]] if "range" in fam.params else list(fb.LOG_STD_RANGES))


def _log_std_floor(lo, hi, ref):
    """log_std = lo + 0.5 (hi - lo) (t + 1) is a sum of two numbers as large as max(|lo|, |hi|), each fp32 rounding 2^-24 of
    THEM, whatever the result: FLOOR_ULPS ulps of that magnitude where it is the larger (one row whose log_std of 0.3 is
    -5 + 5.3; a tensor that reaches an end of its range has the magnitude as its own scale and keeps 8 ulps of it)."""
    return fb.FLOOR_ULPS * max(1.0, max(abs(lo), abs(hi)) / max(float(ref.abs().max()), fb.TINY))


def _expectations(family, lo, hi, got):
    if family == "saturated":
        assert bool((got["t"].abs() == 1).all()) and bool(((got["log_std"] == lo) | (got["log_std"] == hi)).all())
    if family == "flat":
        assert bool((got["log_std"] == lo).all())
    if family in ("saturated", "flat"):
        for name in ("d_h", "d_w", "d_b"):
            assert not got[name].any(), name


@pytest.mark.parametrize("family", fb.GAUSS_FAMILIES)
@pytest.mark.parametrize("a", ACTS)
@pytest.mark.parametrize("rows", ROWS)
def test_shared_head(rows, a, family):
    from safe_marl_amd.nets import _GaussHeadFn, gauss_head_forward
    fam, ranges = head_case(rows, a, family)
    h, w, b, means, noise, d_ls = (t.cuda() for t in fam.inputs)
    for lo, hi in ranges:
        for low, high in (BOUNDS if family == "wide_noise" else BOUNDS[:1]):
            ref = fb.gauss_head_plain(fam.inputs, lo, hi, th.float64, low, high)
            t32 = fb.gauss_head_plain(fam.inputs, lo, hi, th.float32, low, high)
            tag = f"gauss-head {family}[{lo},{hi}]->[{low},{high}] {rows}x{a}"
            out = gauss_head_forward(h, w, b, lo, hi, means=means, noise=noise, low=low, high=high)
            assert out is not None
            got = dict(zip(FORWARD, out))
            for name in FORWARD:
                fb.within_budget(got[name].cpu(), t32[name], ref[name], name=f"{tag} {name}",
                                 floor_ulps=_log_std_floor(lo, hi, ref[name]) if name == "log_std" else fb.FLOOR_ULPS)
            hh, ww, bb = (t.clone().requires_grad_(True) for t in (h, w, b))
            ls = _GaussHeadFn.apply(hh, ww, bb, lo, hi)
            assert th.equal(ls, got["log_std"])
            got["d_h"], got["d_w"], got["d_b"] = th.autograd.grad(ls, (hh, ww, bb), d_ls)
            for name in ("d_h", "d_w", "d_b"):
                fb.within_budget(got[name].cpu(), t32[name], ref[name], name=f"{tag} {name}")
            _expectations(family, lo, hi, got)
            assert float(got["log_std"].min()) >= lo and float(got["log_std"].max()) <= hi


@pytest.mark.parametrize("family", fb.GAUSS_FAMILIES)
@pytest.mark.parametrize("b,n,a", UNSHARED)
def test_per_agent_heads(b, n, a, family):
    from safe_marl_amd import _lib
    from safe_marl_amd.nets import _GaussHeadUnsharedFn, _gauss_head_unshared_args
    rows = b * n
    fam, ranges = head_case(rows, a, family, n=n)
    h, w, bias, _, _, d_ls = (t.cuda() for t in fam.inputs)
    for lo, hi in ranges:
        ref = fb.gauss_head_plain(fam.inputs, lo, hi, th.float64)
        t32 = fb.gauss_head_plain(fam.inputs, lo, hi, th.float32)
        tag = f"gauss-heads {family}[{lo},{hi}] {b}x{n}x{a}"
        ws, bs = [w[i].contiguous() for i in range(n)], [bias[i].contiguous() for i in range(n)]
        got = {"log_std": th.full((rows, a), float("nan"), device="cuda"), "t": th.full((rows, a), float("nan"), device="cuda")}
        k = _gauss_head_unshared_args(rows, n, ws, lo, hi)
        for i in range(n):
            k.b[i] = bs[i].data_ptr()
        k.h, k.log_std, k.t = h.data_ptr(), got["log_std"].data_ptr(), got["t"].data_ptr()
        _lib.launch("flexnet_gauss_head_unshared_forward", k)
        for name in ("log_std", "t"):
            fb.within_budget(got[name].cpu(), t32[name], ref[name], name=f"{tag} {name}",
                             floor_ulps=_log_std_floor(lo, hi, ref[name]) if name == "log_std" else fb.FLOOR_ULPS)
        hh = h.clone().requires_grad_(True)
        flat = [t.clone().requires_grad_(True) for i in range(n) for t in (ws[i], bs[i])]
        ls = _GaussHeadUnsharedFn.apply(hh, n, lo, hi, *flat)
        assert th.equal(ls, got["log_std"])
        grads = th.autograd.grad(ls, [hh] + flat, d_ls)
        got["d_h"], got["d_w"], got["d_b"] = grads[0], th.stack(grads[1::2]), th.stack(grads[2::2])
        for name in ("d_h", "d_w", "d_b"):
            fb.within_budget(got[name].cpu(), t32[name], ref[name], name=f"{tag} {name}")
        _expectations(family, lo, hi, got)


# ---- without tolerance ------------------------------------------------------------------------------------------------------
def test_the_first_rows_of_a_launch_are_the_launch_on_them_alone():
    from safe_marl_amd.nets import gauss_head_backward, gauss_head_forward
    lo, hi = fb.LOG_STD_RANGES[1]
    fam, _ = head_case(129, 8, "mixed")
    h, w, b, means, noise, d_ls = (t.cuda() for t in fam.inputs)
    whole = gauss_head_forward(h, w, b, lo, hi, means=means, noise=noise)
    whole_back = gauss_head_backward(d_ls, whole[1], w, lo, hi)
    for p in (1, 31, 32, 33):
        part = gauss_head_forward(h[:p].contiguous(), w, b, lo, hi, means=means[:p].contiguous(), noise=noise[:p].contiguous())
        for name, x, y in zip(FORWARD, part, whole):
            assert th.equal(x, y[:p]), (p, name)
        back = gauss_head_backward(d_ls[:p].contiguous(), part[1], w, lo, hi)
        assert th.equal(back[0], whole_back[0][:p]) and th.equal(back[1], whole_back[1][:p]), p


@pytest.mark.parametrize("low,high", BOUNDS)
@pytest.mark.parametrize("bad", [0, 31, 32])
def test_a_nan_row_of_h_stays_in_its_row(bad, low, high):
    """That row's log_std, t, action and env_action are NaN (th.clamp hands a NaN on: so does translate_action's clamp); every
    other row has the bits of the clean launch."""
    from safe_marl_amd.nets import gauss_head_forward
    lo, hi = fb.LOG_STD_RANGES[1]
    fam, _ = head_case(65, 3, "plain")
    h, w, b, means, noise, _ = (t.cuda() for t in fam.inputs)
    clean = gauss_head_forward(h, w, b, lo, hi, means=means, noise=noise, low=low, high=high)
    h2 = h.clone()
    h2[bad, 5] = float("nan")
    got = gauss_head_forward(h2, w, b, lo, hi, means=means, noise=noise, low=low, high=high)
    others = th.arange(65, device="cuda") != bad
    for name, x, y in zip(FORWARD, got, clean):
        assert bool(th.isfinite(y).all()), name
        assert bool(th.isnan(x[bad]).all()), f"{name}: the NaN row came out as {x[bad].tolist()}"
        assert th.equal(x[others], y[others]), name


def _sum_explore(kind, means, spread, eps, low, high):
    """(action, env_action) [envs, n, a] of flexnet_gauss_sum_explore (``spread``: log_stds [envs, n, a]) or
    flexnet_agent_sum_explore (``spread``: std [a]): the kernels alone, no environment."""
    from safe_marl_amd import _lib
    envs, n, a = means.shape
    action, env_action = th.full_like(means, 7.0), th.full_like(means, 7.0)
    k = _lib.FlexGaussSumArgs() if kind == "gauss" else _lib.FlexAgentSumArgs()
    k.n_envs, k.n_agents, k.act_dim, k.act_low, k.act_high = envs, n, a, low, high
    k.means, k.eps, k.action, k.env_action = means.data_ptr(), eps.data_ptr(), action.data_ptr(), env_action.data_ptr()
    setattr(k, "log_stds" if kind == "gauss" else "std", spread.data_ptr())
    _lib.launch(f"flexnet_{kind}_sum_explore", k)
    th.cuda.synchronize()
    return action, env_action


@pytest.mark.parametrize("low,high", BOUNDS)
@pytest.mark.parametrize("kind", ["gauss", "agent"])
def test_sum_explore_hands_a_nan_mean_to_its_environment_alone(kind, low, high):
    """One agent's NaN means in one environment: that environment's action AND env_action are NaN for every agent (the
    composition's th.clamp hands it on; a diverged policy must not go on acting), the others keep their bits."""
    envs, n, a, bad = 300, 5, 4, 257
    g = th.Generator().manual_seed(5)
    means = th.randn(envs, n, a, generator=g).cuda()
    eps = th.randn(envs, 1, a, generator=g).cuda()
    spread = (0.5 * th.randn(envs, n, a, generator=g) - 0.3).cuda() if kind == "gauss" else (0.5 + th.rand(a, generator=g)).cuda()
    clean = _sum_explore(kind, means, spread, eps, low, high)
    m2 = means.clone()
    m2[bad, 1] = float("nan")
    got = _sum_explore(kind, m2, spread, eps, low, high)
    others = th.arange(envs, device="cuda") != bad
    for name, x, y in zip(("action", "env_action"), got, clean):
        assert bool(th.isfinite(y).all()), name
        assert bool(th.isnan(x[bad]).all()), f"{name}: the NaN environment came out as {x[bad, 0].tolist()}"
        assert th.equal(x[others], y[others]), name
