"""GPU parity of flexenv_step_many on the paths of its loop that load from memory what the carried path keeps in registers:
the roll-back of a failed solve, the step behind a restart, the carry switched off, a launch's first step — and the solve's
table constants, which the launch reads once (NetHdrRegs) where every other kernel reads them per solve.

Bar: bit-exact against the same number of ``step(obs_rows=True)`` launches — every step's reward, done, info and failed rows,
then ``get_state``, ``obs_view`` and every peek.  The shapes are the smallest that reach each path: 5 environments are three
wavefronts of two, the last with a spare lane group; 3 environments of the 45-bus feeder are three wavefronts of one."""
import numpy as np
import pytest

PEEKS = ("V", "E", "E_INIT", "PRED", "CH", "DIS", "QPV", "PCT", "CUMREW", "STEPS", "ROW", "START", "PF_ITERS", "EPISODE",
         "PF_SWEEPS")

# The failing input.  e_min = -0.02 lets _clip_power_charging_discharging (env:628-661, which tests E - dis / eta without dt)
# pass a full discharge however little is stored; raw actions (alg safemaddpg, env:268-274) hand [reduction, charge,
# discharge, q] over unscaled.  Environments 1 and 4 discharge p_dis_max from 0.006 / 0.009 of stored energy: dt * p_dis_max
# / eta_dis = 0.00139 per step, so E_next (pf.py:96-98) is negative in step 4 resp. step 6 (counted from 0) — pf.py:45 declares
# it non-negative, the step takes the failure path of env:314-337.  Environment 1 shares its wavefront with environment 0,
# environment 4 with the spare lane group; 0, 2 and 3 charge a little and never fail.
N_ENVS, N_STEPS = 5, 12
FAIL_CFG = {"alg": "safemaddpg", "e_min": -0.02}
FIRST_FAILURE = {1: 4, 4: 6}


def _failing_input():
    rng = np.random.default_rng(31)
    spec = dict(day=np.array([1, 2, 3, 4, 5], np.int32), hour=np.array([3, 9, 12, 15, 20], np.int32),
                interval=np.array([0, 1, 2, 3, 0], np.int32),
                e0=np.repeat(np.array([0.0125, 0.006, 0.0125, 0.0125, 0.009])[:, None], 5, 1), a0=np.zeros((N_ENVS, 20)))
    acts = np.zeros((N_STEPS, N_ENVS, 5, 4))
    acts[..., 0] = rng.uniform(0.0, 0.5, acts.shape[:-1])          # power reduction
    acts[..., 1] = rng.uniform(0.0, 0.002, acts.shape[:-1])        # charge
    acts[..., 3] = rng.uniform(-0.01, 0.01, acts.shape[:-1])       # reactive power
    for env in FIRST_FAILURE:
        acts[:, env, :, 1] = 0.0
        acts[:, env, :, 2] = 0.005                                 # discharge at p_dis_max
    return spec, acts.astype(np.float32)


def _oracle_failures(net, series, spec, acts):
    """failed [steps, N] of oracle/flexenv_oracle.c on the same input (no restarts: a failed environment steps on)."""
    from oracle import c_oracle
    cenv = c_oracle.COracleEnv(net, series.table, N_ENVS, cfg=FAIL_CFG, alg=FAIL_CFG["alg"])
    cenv.reset(spec["interval"] + spec["hour"] * 4 + spec["day"] * 96, spec["e0"], spec["a0"])
    assert not cenv.failed.any()
    out = []
    for k in range(acts.shape[0]):
        cenv.step(acts[k].astype(np.float64))
        out.append(cenv.failed.copy())
    return np.stack(out)


def test_the_failing_input_fails_where_it_is_meant_to(net, series_small):
    """CPU: the C oracle on the input of the failed-solve cases — environment 1 fails first in step 4 and environment 4 in step
    6, both in the middle of the launch, and their wavefront partners (environment 0; 2 and 3 next door) converge throughout."""
    spec, acts = _failing_input()
    failed = _oracle_failures(net, series_small, spec, acts)
    for env in range(N_ENVS):
        if env in FIRST_FAILURE:
            k = FIRST_FAILURE[env]
            assert not failed[:k, env].any() and failed[k:, env].all(), (env, failed[:, env])
            assert 0 < k < N_STEPS - 1
        else:
            assert not failed[:, env].any(), (env, failed[:, env])


def _same_state(a, b, tag):
    import torch
    for k in PEEKS:
        assert torch.equal(a.peek(k), b.peek(k)), (tag, k)
    assert torch.equal(a.obs_view(), b.obs_view()), (tag, "obs")
    assert torch.equal(a.get_state(), b.get_state()), (tag, "state")


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


def _pair(net, series, n, cfg, seed=7, spec=None):
    from safe_marl_amd.flex_env import VecFlexProvisionEnv
    a = VecFlexProvisionEnv(cfg, n, series=series, net=net, seed=seed)
    b = VecFlexProvisionEnv(cfg, n, series=series, net=net, seed=seed)
    a.reset(spec=spec)
    b.reset(spec=spec)
    return a, b


@pytest.mark.gpu
@pytest.mark.parametrize("auto", [True, False])
def test_a_solve_that_fails_in_the_middle_of_a_launch(net, series_small, auto):
    """auto_reset on: the failed environment restarts inside the launch and its wavefront reloads everything in the next step.
    Off: the roll-back alone, with the carry still holding — the environment steps on from the state the failure left and
    fails again in every later step."""
    import torch
    spec, acts = _failing_input()
    oracle = _oracle_failures(net, series_small, spec, acts)
    a, b = _pair(net, series_small, N_ENVS, FAIL_CFG, spec=spec)
    d2, f2 = _run_both(a, b, torch.from_numpy(acts).cuda(), N_STEPS, auto)
    f2 = f2.cpu().numpy()
    print("failed per step:", f2.sum(1).tolist())
    for env, k in FIRST_FAILURE.items():
        assert not f2[:k, env].any() and f2[k, env] == 1, (env, f2[:, env])
    assert not f2[:, [0, 2, 3]].any()
    if not auto:
        assert np.array_equal(f2, oracle)
    _same_state(a, b, "failed solve")


@pytest.mark.gpu
@pytest.mark.parametrize("carry", [True, False])
def test_five_environments_over_an_episode_boundary(net, series_small, carry):
    """episode_limit 6: every environment ends its episode in step 4 (a reset leaves steps = 1, env:76) and restarts inside the
    launch; the new episodes end in step 9, or earlier where a solve fails.  carry off: every step re-loads what the step
    before stored."""
    import torch
    a, b = _pair(net, series_small, N_ENVS, {"episode_limit": 6})
    rng = np.random.default_rng(37)
    acts = torch.from_numpy(rng.uniform(0.5, 1.0, (N_STEPS, N_ENVS, 5, 4))).cuda().float()
    d2, f2 = _run_both(a, b, acts, N_STEPS, True, carry)
    print("restarts per step:", d2.sum(1).tolist(), "failed solves:", int(f2.sum().item()))
    assert d2[4].all() and int(d2[5:].sum().item()) >= N_ENVS
    _same_state(a, b, "episode boundary")
    _run_both(a, b, acts, 3, True, carry)                   # (a second launch starts where the first ended)
    _same_state(a, b, "after a second launch")


@pytest.fixture(scope="module")
def feeder45():
    from tests.test_pf_gpu import _random_feeder
    from safe_marl_amd.series import make_synthetic_series
    blds = [7, 19, 33, 41]
    netx = _random_feeder(45, 11, blds)
    return netx, make_synthetic_series(netx, n_days=6), {"buildings": blds, "pv_nodes": blds, "ess_nodes": blds, "episode_limit": 4}


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_one_environment_per_wavefront(feeder45, dtype):
    """The <1, ...> instantiations on the 45-bus feeder (more than 32 PQ buses; its sweeps take the pointer-jumping path sums,
    whose round count is one of the header constants): 3 environments, 6 steps, a restart inside the launch."""
    import torch
    netx, sx, cfg = feeder45
    a, b = _pair(netx, sx, 3, cfg, seed=5)
    rng = np.random.default_rng(41)
    acts = torch.from_numpy(rng.uniform(0.5, 1.0, (6, 3, 4, 4))).cuda()
    acts = acts.float() if dtype == "f32" else acts.double()
    d2, _ = _run_both(a, b, acts, 6, True)
    assert int(d2.sum().item()) >= 3
    _same_state(a, b, "45-bus")


@pytest.mark.gpu
@pytest.mark.parametrize("steps", [1, 2])
def test_launches_whose_first_step_is_also_the_last(net, series_small, steps):
    import torch
    a, b = _pair(net, series_small, N_ENVS, {})
    rng = np.random.default_rng(43)
    acts = torch.from_numpy(rng.uniform(0.5, 1.0, (steps, N_ENVS, 5, 4))).cuda().float()
    for _ in range(3):                                      # (each launch's first step loads what the launch before stored)
        _run_both(a, b, acts, steps, True)
    _same_state(a, b, f"{steps}-step launches")
