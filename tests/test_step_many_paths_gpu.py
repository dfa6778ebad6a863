"""GPU parity of flexenv_step_many on the paths its loop branches on: what a step waits for depends on whether the step
before left its state in registers, whether an environment restarted, whether a solve failed and whether a step follows.

Bar: bit-exact against the same number of ``step(obs_rows=True)`` launches, as in tests/test_step_many_gpu.py — the launch
changes when loads are issued and what the loop waits for, never what a step computes or stores."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests.test_step_many_gpu import _pair, _same_state


def _run_both(a, b, acts, steps, auto, carry=True):
    import torch
    period = acts.shape[0]
    rew, don, inf, fail = [], [], [], []
    for k in range(steps):
        r, d, i = a.step(acts[k % period], obs_rows=True, auto_reset=auto)
        rew.append(r.clone()); don.append(d.clone()); inf.append(i.clone()); fail.append(a.failed.clone())
    r2, d2, i2, f2 = b.step_many(acts, steps=steps, auto_reset=auto, carry=carry)
    torch.cuda.synchronize()
    assert torch.equal(torch.stack(rew), r2)
    assert torch.equal(torch.stack(don), d2)
    assert torch.equal(torch.stack(inf), i2)
    assert torch.equal(torch.stack(fail), f2)
    return d2, f2


@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("n,cfg,steps,period,back", [
    (33, {}, 24, 1, None),                    # one slab, read by every step (the slab after the current one is itself)
    (64, {}, 23, 5, None),                    # a period that does not divide the step count
    (17, {}, 1, 3, None),                     # a launch of one step: no step follows the first
    # episode_limit 6: a reset leaves steps = 1 (env:76), so an environment whose solves all succeed ends its episodes in the
    # launch's steps 4, 9, 14, ... (counted from 0); some of these seeded actions fail a solve, which ends an episode early
    (40, {"episode_limit": 6}, 10, 4, 0),     # the launch ENDS on a step in which environments restart
    (40, {"episode_limit": 6}, 11, 11, 1),    # a restart on the step before the last
    (40, {"episode_limit": 6}, 12, 5, 2),     # ... and two steps before it
])
def test_action_periods_launch_lengths_and_restarts_at_the_end(net, series_small, n, cfg, steps, period, back, dtype):
    import torch
    a, b = _pair(net, series_small, n, cfg)
    rng = np.random.default_rng(23)
    acts = torch.from_numpy(rng.uniform(0.5, 1.0, (period, n, 5, 4))).cuda()
    acts = acts.float() if dtype == "f32" else acts.double()
    d2, f2 = _run_both(a, b, acts, steps, True)
    if back is not None:
        per_step = d2.sum(1).tolist()
        print("restarts per step:", per_step, "failed solves:", int(f2.sum().item()))
        assert per_step[steps - 1 - back] > 0             # (the case is the one its comment names)
        assert per_step[4] > 0 and sum(per_step) >= per_step[4] + per_step[9]
    _same_state(a, b, "after the launch")
    # a second launch starts where the first ended (its first step has no carry), and so does a single step
    _run_both(a, b, acts, min(steps, 3), True)
    _same_state(a, b, "after a second launch")


@pytest.mark.parametrize("auto", [True, False])
@pytest.mark.parametrize("carry", [True, False])
def test_steps_whose_solve_fails(auto, carry):
    """The 45-bus feeder and (0, 1) actions of tests/test_step_many_gpu.py: some steps leave the power flow unsolved or E_next
    outside its domain and take the failure path of env:314-337, which re-reads what the step before stored.  Without the
    in-launch restart a failed environment goes on stepping from the state the failure left."""
    import torch
    from tests.test_pf_gpu import _random_feeder
    from safe_marl_amd.series import make_synthetic_series
    from safe_marl_amd.flex_env import VecFlexProvisionEnv
    blds = [7, 19, 33, 41]
    netx = _random_feeder(45, 11, blds)
    sx = make_synthetic_series(netx, n_days=6)
    n, steps = 9, 30
    cfg = {"buildings": blds, "pv_nodes": blds, "ess_nodes": blds, "episode_limit": 9}
    a = VecFlexProvisionEnv(cfg, n, series=sx, net=netx, seed=5)
    b = VecFlexProvisionEnv(cfg, n, series=sx, net=netx, seed=5)
    a.reset(); b.reset()
    rng = np.random.default_rng(17)
    acts = torch.from_numpy(rng.uniform(0, 1, (steps, n, 4, 4))).cuda().float()
    _, f2 = _run_both(a, b, acts, steps, auto, carry)
    print("failed steps:", int(f2.sum().item()), "of", n * steps)
    assert int(f2.sum().item()) > 0
    _same_state(a, b, "45-bus, failures")
