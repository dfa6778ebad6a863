"""GPU parity of flexenv_step_many with its launch constants read from the host-prepared block (ManyConsts) and its bases
formed once per wavefront (ManyWave; FLEX_MANY_CONSTS in csrc/flexenv.hip): one launch against the same steps issued as
single ``step(obs_rows=True)`` launches from the same reset.

Bar: equal BIT PATTERNS (integer views: -0.0 and NaN payloads count) of every step's reward / done / info / failed row, of
every peek, of ``obs_view`` and of ``get_state``.  The shapes are the smallest at which a hoisted base or a merged constant
can still be wrong: batches of 1, 2, 3 and 5 environments (an odd batch leaves a spare lane group, 1 leaves only it), launches
of 1, 2 and 9 steps, action periods 1 and 3 (the slab index wraps inside the launch), three agents instead of five (another
stride in every agent-indexed base), the 45-bus feeder (one environment per wavefront), absent outputs, an episode end, a
failed solve, the carry switched off and two launches back to back."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests.test_step_many_waits_gpu import FAIL_CFG, FIRST_FAILURE, N_ENVS, N_STEPS, PEEKS, _failing_input


def _bits(t):
    import torch
    if t.dtype == torch.float64:
        return t.contiguous().view(torch.int64)
    if t.dtype == torch.float32:
        return t.contiguous().view(torch.int32)
    return t


def _same_bits(x, y, tag):
    import torch
    assert x.shape == y.shape and x.dtype == y.dtype, tag
    assert torch.equal(_bits(x), _bits(y)), tag


def _same_state(a, b, tag):
    for k in PEEKS:
        _same_bits(a.peek(k), b.peek(k), (tag, k))
    _same_bits(a.obs_view(), b.obs_view(), (tag, "obs"))
    _same_bits(a.get_state(), b.get_state(), (tag, "state"))


def _pair(net, series, n, cfg=None, seed=7, spec=None):
    from safe_marl_amd.flex_env import VecFlexProvisionEnv
    a = VecFlexProvisionEnv(cfg or {}, n, series=series, net=net, seed=seed)
    b = VecFlexProvisionEnv(cfg or {}, n, series=series, net=net, seed=seed)
    a.reset(spec=spec)
    b.reset(spec=spec)
    return a, b


def _singles(a, acts, steps, auto):
    import torch
    period = acts.shape[0]
    rew, don, inf, fail = [], [], [], []
    for k in range(steps):
        r, d, i = a.step(acts[k % period], obs_rows=True, auto_reset=auto)
        rew.append(r.clone()); don.append(d.clone()); inf.append(i.clone()); fail.append(a.failed.clone())
    return torch.stack(rew), torch.stack(don), torch.stack(inf), torch.stack(fail)


def _run_both(a, b, acts, steps, auto, carry=True, want=("info", "failed"), tag=""):
    """`steps` single launches on `a`, one launch on `b`; `want`: which of the optional outputs the launch is given."""
    import torch
    n = a.n_envs
    r1, d1, i1, f1 = _singles(a, acts, steps, auto)
    out = (torch.empty(steps, n, dtype=torch.float64, device="cuda"), torch.empty(steps, n, dtype=torch.uint8, device="cuda"),
           torch.empty(steps, n, 7, dtype=torch.float64, device="cuda") if "info" in want else None,
           torch.empty(steps, n, dtype=torch.uint8, device="cuda") if "failed" in want else None)
    r2, d2, i2, f2 = b.step_many(acts, steps=steps, auto_reset=auto, out=out, carry=carry)
    torch.cuda.synchronize()
    _same_bits(r1, r2, (tag, "reward"))
    _same_bits(d1, d2, (tag, "done"))
    if "info" in want:
        _same_bits(i1, i2, (tag, "info"))
    else:
        assert i2 is None
    if "failed" in want:
        _same_bits(f1, f2, (tag, "failed"))
    else:
        assert f2 is None
    return d1, f1


def _actions(rng, period, n, na, dtype, lo=0.5):
    import torch
    acts = torch.from_numpy(rng.uniform(lo, 1.0, (period, n, na, 4))).cuda()
    return acts.float() if dtype == "f32" else acts.double()


@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("n", [1, 2, 3, 5])
def test_small_batches_launch_lengths_and_action_periods(net, series_small, n, dtype):
    """33-bus feeder, five agents; every launch goes on from the state the launch before left in both environments."""
    rng = np.random.default_rng(101 + n)
    a, b = _pair(net, series_small, n)
    for period in (1, 3):
        acts = _actions(rng, period, n, 5, dtype)
        for steps in (1, 2, 9):
            tag = f"n={n} {dtype} period={period} steps={steps}"
            _run_both(a, b, acts, steps, True, tag=tag)
            _same_state(a, b, tag)


def test_three_agents():
    """buildings [5, 15, 25]: n_agents = 3 is the stride of the agent record, of the action slab and of the mirror ring."""
    from safe_marl_amd.network import create_network
    from safe_marl_amd.series import make_synthetic_series
    blds = [5, 15, 25]
    cfg = {"buildings": blds, "pv_nodes": blds, "ess_nodes": blds}
    net3 = create_network(cfg)
    a, b = _pair(net3, make_synthetic_series(net3, n_days=10), 4, cfg)
    for dtype in ("f32", "f64"):
        acts = _actions(np.random.default_rng(103), 4, 4, 3, dtype)
        _run_both(a, b, acts, 6, True, tag=f"3 agents {dtype}")
        _same_state(a, b, f"3 agents {dtype}")


def test_one_environment_per_wavefront_on_the_45_bus_feeder():
    from tests.test_pf_gpu import _random_feeder
    from safe_marl_amd.series import make_synthetic_series
    blds = [7, 19, 33, 41]
    netx = _random_feeder(45, 11, blds)
    sx = make_synthetic_series(netx, n_days=6)
    cfg = {"buildings": blds, "pv_nodes": blds, "ess_nodes": blds, "episode_limit": 4}
    a, b = _pair(netx, sx, 3, cfg, seed=5)
    acts = _actions(np.random.default_rng(107), 6, 3, 4, "f64")
    d, _ = _run_both(a, b, acts, 6, True, tag="45-bus")
    assert int(d.sum().item()) >= 3                          # (an episode ended inside the launch)
    _same_state(a, b, "45-bus")


@pytest.mark.parametrize("want", [("failed",), ("info",), ()])
def test_absent_outputs(net, series_small, want):
    """info = None and failed = None, separately and together: an absent row must stay absent in every step of the launch."""
    a, b = _pair(net, series_small, 5)
    acts = _actions(np.random.default_rng(109), 3, 5, 5, "f32")
    _run_both(a, b, acts, 7, True, want=want, tag=f"outputs {want}")
    _same_state(a, b, f"outputs {want}")


@pytest.mark.parametrize("auto", [True, False])
def test_an_episode_end_inside_the_launch(net, series_small, auto):
    """episode_limit 6: every environment ends its episode in step 4 (a reset leaves steps = 1).  With the restart inside the
    launch the next step loads what the restart stored; without it the environments step on past the end."""
    a, b = _pair(net, series_small, 5, {"episode_limit": 6})
    acts = _actions(np.random.default_rng(113), 9, 5, 5, "f32")
    d, _ = _run_both(a, b, acts, 9, auto, tag=f"episode end auto={auto}")
    # (a failed solve ends an episode before step 4; the restarted episode then ends later)
    assert d[:5].any(0).all() and (auto or d[4:].all())
    _same_state(a, b, f"episode end auto={auto}")


@pytest.mark.parametrize("auto", [True, False])
def test_a_failed_solve_inside_the_launch(net, series_small, auto):
    """The poisoned input of tests/test_step_many_waits_gpu.py: environments 1 and 4 fail in steps 4 and 6; the roll-back reads
    the state through the memory path."""
    import torch
    spec, acts = _failing_input()
    a, b = _pair(net, series_small, N_ENVS, FAIL_CFG, spec=spec)
    _, f = _run_both(a, b, torch.from_numpy(acts).cuda(), N_STEPS, auto, tag=f"failed solve auto={auto}")
    f = f.cpu().numpy()
    for env, k in FIRST_FAILURE.items():
        assert not f[:k, env].any() and f[k, env] == 1, (env, f[:, env])
    _same_state(a, b, f"failed solve auto={auto}")


def test_without_the_carry(net, series_small):
    a, b = _pair(net, series_small, 5, {"episode_limit": 6})
    acts = _actions(np.random.default_rng(127), 3, 5, 5, "f32")
    _run_both(a, b, acts, 9, True, carry=False, tag="no carry")
    _same_state(a, b, "no carry")


def test_two_launches_back_to_back_with_a_step_counter(net, series_small):
    """8 then 5 steps against 13 single steps: state, slab index (each launch starts at slab 0) and the counter cell across the
    launch boundary."""
    import torch
    a, b = _pair(net, series_small, 5)
    ca = torch.zeros(1, dtype=torch.int64, device="cuda")
    cb = torch.zeros(1, dtype=torch.int64, device="cuda")
    a.set_step_counter(ca, modulo=7)
    b.set_step_counter(cb, modulo=7)
    acts = _actions(np.random.default_rng(131), 13, 5, 5, "f32")
    _run_both(a, b, acts[:8], 8, True, tag="first launch")
    assert ca.item() == cb.item() == 8 % 7
    _same_state(a, b, "first launch")
    _run_both(a, b, acts[8:], 5, True, tag="second launch")
    assert ca.item() == cb.item() == 13 % 7
    _same_state(a, b, "second launch")
