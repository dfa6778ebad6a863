"""GPU: test-mode episodes of a shared MLP agent as one launch (include/flexenv.h: flexenv_test_episodes_mlp; opt-in through
FLEX_MLP_TEST_LAUNCH=1) — k steps against k one-step calls bit for bit, the policy against fp64 on the project's error budget at
every step, the policy phase against the training burst's bit for bit, environment, safety projection and agent-summed selection
against a twin stepped call by call, a whole episode against the CPU oracle, the launch against the loop form, the Gaussian MLP
agent, the training state through an evaluation, refusals on a live handle and the example in a fresh process.  Shapes sit at
the launch's edges: a block is 16 environments, a wavefront 2, a policy tile 16 rows."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from . import fp64_budget as fb
from .test_test_episodes_gpu import G, TRACE, _bits, _resimulate, _setup, _spec, _sums_of_trace, _world

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SWITCH = "FLEX_MLP_TEST_LAUNCH"
SHAPES = [(35, None), (19, [3, 17, 28]), (17, [5])]     # 35 x 5: two blocks and a tail of three, a half-filled wavefront
TANH_TOL = 2e-5                                          # fast_tanh against torch.tanh (tests/test_mlp_plain_burst_gpu.py)
RECORD = ("actions", "v", "agent", "row", "reward", "info", "flags")


def _predictor(n=5):
    """tests/test_test_episodes_gpu.py's: the safety layer intervenes."""
    return (torch.full((n,), -0.08, dtype=torch.float64), torch.full((n,), -0.05, dtype=torch.float64),
            torch.full((n,), 0.915, dtype=torch.float64))


def _mlp_setup(alg, n_envs, buildings=None, **over):
    """A seeded model of ``alg`` with the MLP agent, its policy's weights times ten, and a vectorised env."""
    from safe_marl_amd.nets import MLPAgent, MLPAgentGaussian
    pred = _predictor() if alg == "safemaddpg" else None
    model, env, net, series = _setup(alg, n_envs, buildings, predictor=pred, agent_type="mlp", **over)
    assert type(model.policy_dicts[0]) in (MLPAgent, MLPAgentGaussian)
    return model, env, net, series


class _Launch:
    """flexenv_test_episodes_mlp at the VecFlexProvisionEnv level on a model's shared MLP agent: the test-form arguments of
    nets.mlp_test_actor_args over this object's own output tensors (NaN before every call: whatever is read afterwards was
    written by the launch), the mode the model's algorithm asks for."""

    def __init__(self, model, env):
        from safe_marl_amd import nets
        from safe_marl_amd.learner import IDDPG, MATD3, SAFEMADDPG
        self.model, self.env = model, env
        N, n = env.n_envs, env.n_agents
        self.hid = torch.empty(N * n, 64, device="cuda")
        self.means, self.action, self.env_action = (torch.empty(N * n, 4, device="cuda") for _ in range(3))
        a = model.args
        self.args, self.mlp = nets.mlp_test_actor_args(model.policy_dicts[0], N, n, model.obs_dim, a.agent_id, self.hid, self.means,
                                                       self.action, self.env_action, a.action_low, a.action_high)
        assert not self.args.hidden_in and not self.args.w_ih and not self.args.w_hh and not self.args.b_ih and not self.args.b_hh
        own = type(model).get_actions
        self.summed = own is MATD3.get_actions or own is IDDPG.get_actions
        self.safety = None
        if own is SAFEMADDPG.get_actions:
            s_p, s_q, beta = (torch.as_tensor(x, dtype=torch.float64, device="cuda").contiguous() for x in model.predictor)
            self.safety = dict(s_p=s_p, s_q=s_q, beta=beta, v_min=model.V_min, v_max=model.V_max,
                               adjusted=torch.empty(N, 4 * n, dtype=torch.float64, device="cuda"),
                               env_action=torch.empty(N, 4 * n, dtype=torch.float32, device="cuda"),
                               act_low=a.action_low, act_high=a.action_high)

    def outputs(self):
        out = [self.hid, self.means, self.action, self.env_action]
        if self.safety is not None:
            out += [self.safety["adjusted"], self.safety["env_action"]]
        return out

    def run(self, steps, trace=True):
        for t in self.outputs():
            t.fill_(float("nan"))
        out = self.env.test_out(steps, trace)
        got = self.env.test_episodes(self.args, steps, summed=self.summed, safety=self.safety, out=out, mlp=self.mlp)
        torch.cuda.synchronize()
        assert got is out
        return out


def _check_k_steps_equal_one_step_calls(model, env, spec, k=7):
    """From one reset state: the k-step call, then — reset to the same state — k one-step calls.  The policy carries no state,
    so the environment carries everything from call to call.  Returns the one-step records."""
    lau = _Launch(model, env)
    env.reset(spec=spec)
    whole = lau.run(k)
    last = [t.clone() for t in lau.outputs()]
    env.reset(spec=spec)
    ones, running = [], torch.zeros(env.n_envs, 10, dtype=torch.float64, device="cuda")
    for t in range(k):
        one = lau.run(1)
        assert (one["length"] == 1).all()
        for name in RECORD:
            assert torch.equal(whole[name][t], one[name][0]), (name, t)
        running = running + one["sums"]                                # fp64, in step order: the launch's own additions
        ones.append(one)
    assert torch.equal(whole["sums"], running) and float(running[:, 7].abs().min()) > 0
    assert (whole["length"] == k).all() and (whole["flags"] == 4).all()
    for a, b in zip(last, lau.outputs()):                              # what the last step of either form left
        assert torch.isfinite(a).all() and torch.equal(a, b)
    assert float(whole["actions"].std()) > 1e-3 and float(lau.hid.abs().max()) > 0
    return ones


def _references(model, obs):
    """(means, h) of the shared agent on ``obs`` [N, n, o] fp32: the fp64 reference — a deep copy of the module in fp64 on the
    fp32 observations with the id columns — and the fp32 yardstick, tests/fp64_budget.py's plain composition."""
    agent, n, agent_id = model.policy_dicts[0], model.n_, bool(model.args.agent_id)
    rows = obs.reshape(-1, obs.shape[-1]).contiguous()
    with torch.no_grad():
        inputs = fb.with_ids(rows, n) if agent_id else rows
        out64 = fb.ref64(agent)(inputs.double(), None)
        out32 = fb.mlp_actor_plain(agent, rows, n, agent_id)
    return (out64[0], out64[2]), (out32[0], out32[1])


def _check_policy_against_fp64(model, env, spec, steps, name):
    from safe_marl_amd.util import scale_action
    lau = _Launch(model, env)
    env.reset(spec=spec)
    for t in range(steps):
        obs = env.obs_view().clone()                                   # what the policy phase is about to read in place
        lau.run(1, trace=False)
        (m64, h64), (m32, h32) = _references(model, obs)
        assert float(h64.abs().max()) > 0 and float(m64.abs().max()) > 0
        fb.within_budget(lau.hid, h32, h64, name=f"{name} step {t} h")
        fb.within_budget(lau.means, m32, m64, name=f"{name} step {t} means")
        if not lau.summed:                                             # (agent-summed: the selection rewrites both, test 4)
            err = float((lau.action - torch.tanh(lau.means)).abs().max())
            print(f"{name} step {t}: max |action - tanh(means)| = {err:.3e}")
            assert err < TANH_TOL
            assert torch.equal(lau.env_action, scale_action(model.args, lau.action).to(torch.float32))


@pytest.mark.parametrize("alg,n_envs,buildings", [("maddpg",) + s for s in SHAPES] + [("safemaddpg", 35, None), ("matd3", 35, None)])
def test_k_steps_equal_k_one_step_calls_bit_for_bit(alg, n_envs, buildings, monkeypatch):
    """1. Every trace array of the 7-step call equals the one-step calls' rows, ``sums`` their fp64 running sum in step order,
    ``length`` is 7 — identical bits."""
    monkeypatch.setenv(SWITCH, "1")
    model, env, _, _ = _mlp_setup(alg, n_envs, buildings)
    _check_k_steps_equal_one_step_calls(model, env, _spec(n_envs, env.n_agents))


@pytest.mark.parametrize("n_envs,buildings,steps,over", [s + (7, {}) for s in SHAPES] + [(35, None, 1, {"layernorm": False}),
                                                                                        (35, None, 1, {"agent_id": False})])
def test_policy_against_fp64_every_step(n_envs, buildings, steps, over, monkeypatch):
    """2. ``means`` and ``hidden_out`` of every one-step call inside tests/fp64_budget.py's budget at its defaults, no element
    excluded; action = tanh(means) within the project's bound for fast_tanh; env_action = scale_action of the stored action."""
    monkeypatch.setenv(SWITCH, "1")
    model, env, _, _ = _mlp_setup("maddpg", n_envs, buildings, **over)
    assert bool(model.args.layernorm) == over.get("layernorm", True) and bool(model.args.agent_id) == over.get("agent_id", True)
    _check_policy_against_fp64(model, env, _spec(n_envs, env.n_agents), steps, f"mlp-test {n_envs}x{env.n_agents} {over or ''}")


def test_policy_phase_is_the_training_bursts(monkeypatch):
    """3. The same weights on the same reset state: means and h of one step of flexenv_rollout_burst_mlp equal those of a
    one-step test launch, bit for bit — one policy phase, whatever the epilogue behind it."""
    from .test_mlp_plain_burst_gpu import SHAPES as BURST_SHAPES, _env, _mlp_rollout, _spec as _burst_spec, _steps
    monkeypatch.setenv(SWITCH, "1")
    n_envs = 77
    rg, _ = _mlp_rollout("maddpg", n_envs, monkeypatch)
    env = _env(n_envs, BURST_SHAPES[n_envs])
    env.reset(spec=_burst_spec(n_envs, env.n_agents))
    assert torch.equal(rg.obs.clone().reshape(-1), env.obs_view().clone().reshape(-1))
    _steps(rg, (1,))
    lau = _Launch(rg.model, env)
    lau.run(1, trace=False)
    assert float(lau.means.abs().max()) > 0 and float(lau.hid.abs().max()) > 0
    assert torch.equal(lau.means, rg.means_buf)
    assert torch.equal(lau.hid, rg.hid_buf)


@pytest.mark.parametrize("alg,scale", [("maddpg", 10.0), ("safemaddpg", 10.0), ("matd3", 10.0), ("matd3", 1.0)])
def test_environment_safety_and_selection_match_a_twin_stepped_call_by_call(alg, scale, monkeypatch):
    """4. Six one-step launches next to a twin env reset with the same spec.  SAFEMADDPG: the stand-alone safety_project of the
    twin (in the state the launch's projection saw) on the stored action gives the traced actions and ``adjusted``, bit for bit,
    and the layer intervenes.  MATD3: one action for every agent, translate_action(tanh(((m0 + m1) + m2) + ...)) of the stored
    means with the fp32 sum formed left to right on the host.  The twin stepped on the traced actions has the launch's reward,
    done, v, agent records and row, bit for bit.  (MATD3 a second time with the weights as initialised: at times ten the sum
    of five agents' means saturates the tanh, and the order of the sum shows only in its sign.)"""
    from safe_marl_amd.flex_env import VecFlexProvisionEnv
    from safe_marl_amd.util import scale_action
    monkeypatch.setenv(SWITCH, "1")
    N, steps = 35, 6
    model, env, _, _ = _mlp_setup(alg, N, scale=scale)
    n = env.n_agents
    env_args, net, series = _world(None, alg)
    twin = VecFlexProvisionEnv(env_args, N, net=net, series=series, seed=9, warm_start=True)
    spec = _spec(N, n)
    env.reset(spec=spec)
    twin.reset(spec=spec)
    lau = _Launch(model, env)
    assert lau.summed == (alg == "matd3") and (lau.safety is not None) == (alg == "safemaddpg")
    hits = 0
    for t in range(steps):
        out = lau.run(1)
        fed = out["actions"][0]                                        # [N, n, 4] as the step read it
        if alg == "safemaddpg":
            adj, hit, env_action = twin.safety_project(lau.action.view(N, n, 4), *model.predictor, model.V_min, model.V_max,
                                                       env_action_range=(model.args.action_low, model.args.action_high))
            assert torch.equal(lau.safety["adjusted"], adj), t
            assert torch.equal(lau.safety["env_action"], env_action), t
            assert torch.equal(fed.reshape(N, 4 * n), env_action), t
            hits += int(hit.sum().item())
        elif alg == "matd3":
            m = lau.means.view(N, n, 4)
            total = m[:, 0].clone()
            for j in range(1, n):
                total = total + m[:, j]                                # fp32, left to right
            want = torch.tanh(total)
            assert torch.equal(lau.action.view(N, n, 4), lau.action.view(N, n, 4)[:, :1].expand(N, n, 4)), t
            err = float((lau.action.view(N, n, 4)[:, 0] - want).abs().max())
            print(f"matd3 step {t}: max |action - tanh(sum of means)| = {err:.3e}")
            assert err < TANH_TOL and (scale > 1.0 or float(want.abs().max()) < 0.99)
            assert torch.equal(lau.env_action, scale_action(model.args, lau.action).to(torch.float32)), t
            assert torch.equal(fed.reshape(N * n, 4), lau.env_action), t
        else:
            assert torch.equal(fed.reshape(N * n, 4), lau.env_action), t
        twin.step(fed.contiguous(), obs_rows=True)
        torch.cuda.synchronize()
        assert torch.equal(out["reward"][0], twin.reward) and torch.equal(out["info"][0], twin.info), t
        assert torch.equal(out["flags"][0], 4 + (twin.done != 0).to(torch.uint8) + 2 * (twin.failed != 0).to(torch.uint8)), t
        assert torch.equal(out["v"][0], twin.peek("V")) and torch.equal(out["row"][0], twin.peek("ROW")), t
        agent = torch.stack([twin.peek(f) for f in ("E", "PRED", "CH", "DIS", "QPV")], dim=-1)
        assert torch.equal(out["agent"][0], agent), t
    assert alg != "safemaddpg" or hits > 0
    assert torch.equal(env.get_state(), twin.get_state())
    assert torch.equal(env.obs_view().clone(), twin.obs_view().clone())


def test_a_whole_episode(monkeypatch):
    """5. Model.test_episodes(one_launch=True, trace=True) at 35 x 5: the launch ran, every length is 95, ``sums`` is the fp64
    sum of the trace rows in step order to the bit, environments 0, 17 and 34 re-simulated on the CPU oracle agree within
    1e-10; with steps=100 rows 95.. are not alive and all zero and ``sums`` has the 95-step call's bits."""
    monkeypatch.setenv(SWITCH, "1")
    N = 35
    model, env, net, series = _mlp_setup("maddpg", N)
    spec = _spec(N, 5)
    res = model.test_episodes(env, spec, trace=True, one_launch=True)
    assert res.launch and (res.length == 95).all() and set(res.trace) == set(TRACE)
    assert (res.trace["flags"] == 5 * (np.arange(95) == 94)[:, None] + 4 * (np.arange(95) < 94)[:, None]).all()
    assert np.abs(res.sums[:, 7]).min() > 0 and res.trace["actions"].std() > 1e-3
    assert np.array_equal(_bits(res.sums), _bits(_sums_of_trace(res.trace)))
    _resimulate(res, (0, 17, 34), spec, net, series)
    long = model.test_episodes(env, spec, trace=True, one_launch=True, steps=100)
    assert long.launch and (long.length == 95).all() and np.array_equal(_bits(long.sums), _bits(res.sums))
    assert (long.trace["flags"][95:] == 0).all() and (long.trace["flags"][:95] & 4).all() and (long.trace["flags"][94] & 1).all()
    for k in ("actions", "v", "agent", "row", "reward", "info"):
        assert not long.trace[k][95:].any(), k
        assert np.array_equal(_bits(long.trace[k][:95]), _bits(res.trace[k])), k


@pytest.mark.parametrize("alg", ["maddpg", "ippo"])
def test_launch_against_loop(alg, monkeypatch):
    """6. The loop runs csrc/actor_mlp.hip, another kernel: no bit equality.  Same lengths, same stat() keys, first-step
    actions within the fast_tanh bound, the continuous stat() entries within 1e-5 max(1e-3, |x|) — tests/
    test_test_episodes_gpu.py's bound for the same comparison.  (The two count-derived entries are proved exact by test 4.)"""
    monkeypatch.setenv(SWITCH, "1")
    N = 35
    model, env, _, _ = _mlp_setup(alg, N)
    spec = _spec(N, 5)
    a = model.test_episodes(env, spec, trace=True, one_launch=True)
    b = model.test_episodes(env, spec, trace=True, one_launch=False)
    assert a.launch and not b.launch and np.array_equal(a.length, b.length) and (a.length == 95).all()
    err = np.abs(a.trace["actions"][0] - b.trace["actions"][0]).max()
    print(f"{alg}: first-step actions, launch against loop: max |difference| = {err:.3e}")
    assert err < TANH_TOL and a.trace["actions"].std() > 1e-3
    sa, sb = a.stat(), b.stat()
    assert sa.keys() == sb.keys()
    for k in sa:
        print(f"{alg} {k}: launch {sa[k]!r} loop {sb[k]!r}")
    for k in sa:
        if k not in ("mean_test_violation_rate", "mean_test_solver_failed"):
            assert abs(sa[k] - sb[k]) <= 1e-5 * max(1e-3, abs(sb[k])), (k, sa[k], sb[k])


def test_gaussian_mlp_agent_takes_the_launch(monkeypatch):
    """7. gaussian_policy with agent_type mlp: the ``mean`` head sits in the fc2 slot, test mode never reads the log-std; tests 1
    and 2 hold on it."""
    from safe_marl_amd.flex_env import VecFlexProvisionEnv
    from safe_marl_amd.learner import MADDPG
    from safe_marl_amd.nets import MLPAgentGaussian
    from safe_marl_amd.util import convert
    monkeypatch.setenv(SWITCH, "1")
    d = json.load(open(os.path.join(G, "gauss_maddpg_mlp_args.json")))
    d.update(cuda=True)
    N = 35
    _, net, series = _world()
    env = VecFlexProvisionEnv({}, N, net=net, series=series, seed=9, warm_start=True)
    torch.manual_seed(21)
    model = MADDPG(convert(d), MADDPG(convert(d))).cuda()
    with torch.no_grad():
        for p in model.policy_dicts.parameters():
            p.mul_(10.0)
    agent = model.policy_dicts[0]
    assert type(agent) is MLPAgentGaussian
    lau = _Launch(model, env)
    assert lau.args.fc2_w == agent.mean.weight.data_ptr() and lau.args.fc2_b == agent.mean.bias.data_ptr()
    assert lau.mlp.fc2_w == agent.fc2.weight.data_ptr()
    spec = _spec(N, 5)
    res = model.test_episodes(env, spec, trace=True, one_launch=True, steps=9)
    assert res.launch and (res.length == 9).all() and res.trace["actions"].std() > 1e-3
    _check_k_steps_equal_one_step_calls(model, env, spec)
    _check_policy_against_fp64(model, env, spec, 7, "mlp-test gaussian 35x5")


def test_training_state_is_left_alone(monkeypatch):
    """8. A trainer at 64 environments with the MLP agent, one train_process through mlp_plain_burst behind it: an evaluation
    with one_launch_eval takes the launch and leaves every replay ring, both cursor cells, the noise position and the running
    sums bit-identical; the next train_process runs and spends one gap slab."""
    from test_policy import alg_args
    from safe_marl_amd.flex_env import VecFlexProvisionEnv
    from safe_marl_amd.learner import MADDPG
    from safe_marl_amd.trainer import PGTrainer
    monkeypatch.setenv(SWITCH, "1")
    for k in ("FLEX_MLP_BURST", "FLEX_ROLLOUT_BURST"):
        monkeypatch.delenv(k, raising=False)
    n = 64
    _, net, series = _world()
    env = VecFlexProvisionEnv({}, n, net=net, series=series, seed=11, warm_start=True)
    torch.manual_seed(0)
    np.random.seed(0)
    tr = PGTrainer(alg_args("maddpg", env, behaviour_update_freq=60, target_update_freq=120, agent_type="mlp"), MADDPG, env, None,
                   replay_capacity=n * 96 * 3)
    model, buf = tr.behaviour_net, tr.replay_buffer
    model.train_process({}, tr)
    rg = model._rollout_graph
    assert rg is not None and rg.graph is not None and rg.mlp_plain_burst and buf.slab_mode
    torch.cuda.synchronize()
    keep = {k: getattr(buf, k).clone() for k in ("row_ring", "hid_ring", "small_ring", "cursor")}
    keep.update(rng_state=rg.rng_state.clone(), acc=rg.acc.clone())
    k0 = buf.k
    taken = []
    inner = VecFlexProvisionEnv.test_episodes

    def spy(self, *args, **kw):
        taken.append(kw.get("mlp") is not None)
        return inner(self, *args, **kw)
    monkeypatch.setattr(VecFlexProvisionEnv, "test_episodes", spy)
    model.one_launch_eval = True
    stat = {}
    model.evaluation(stat, tr)
    torch.cuda.synchronize()
    assert taken == [True]
    assert np.isfinite(stat["mean_test_reward"]) and "mean_test_violation_rate" in stat
    for k in ("row_ring", "hid_ring", "small_ring", "cursor"):
        assert torch.equal(getattr(buf, k), keep[k]), k
    assert torch.equal(rg.rng_state, keep["rng_state"]) and torch.equal(rg.acc, keep["acc"]) and buf.k == k0
    st = {}
    model.train_process(st, tr)
    assert np.isfinite(st["mean_train_reward"]) and buf.k - k0 - 95 == 1                   # a hard reset: one gap slab
    assert buf.cursor.tolist() == [buf.k % buf.slabs, (buf.k - 1) % buf.slabs]


def test_refusals_on_a_live_handle(monkeypatch):
    """9. The argument checks with an environment behind them: FLEX_EINVAL, nothing launched; and the eligibility decision
    with the switch on keeps its other reasons."""
    from safe_marl_amd import _lib
    from safe_marl_amd.flex_env import VecFlexProvisionEnv
    monkeypatch.setenv(SWITCH, "1")
    model, env, _, _ = _mlp_setup("maddpg", 16)
    blds = [5, 8, 10, 15, 20, 25, 30]
    env_args, net, series = _world(blds)
    env7 = VecFlexProvisionEnv(env_args, 16, net=net, series=series, seed=9)
    dummy = torch.zeros(16 * 7 * 64, device="cuda")
    out = _lib.FlexTestOut()
    out.sums, out.length = dummy.data_ptr(), dummy.data_ptr()
    mlp = _lib.FlexBurstMlp()
    mlp.fc2_w, mlp.fc2_b = dummy.data_ptr(), dummy.data_ptr()

    def call(e, n_agents=5, act_dim=4, steps=95, summed=0, safety=None, rec=out, second=mlp):
        a = _lib.FlexActorArgs()
        a.rows, a.n_agents, a.obs_dim, a.act_dim = 16 * n_agents, n_agents, 144, act_dim
        for k in ("hidden_out", "means", "action", "env_action", "fc1_w", "fc1_b", "fc2_w", "fc2_b"):
            setattr(a, k, dummy.data_ptr())
        a.action_high = 1.0
        return e.lib.flexenv_test_episodes_mlp(e.handle, C.byref(a), steps, summed, C.byref(second) if second is not None else None,
                                               C.byref(safety) if safety is not None else None,
                                               C.byref(rec) if rec is not None else None, None)

    sf = _lib.FlexBurstSafety()
    for k in ("s_p", "s_q", "beta", "adjusted", "env_action"):
        setattr(sf, k, dummy.data_ptr())
    sf.act_high = 1.0
    calls = env.calls
    assert call(env7, n_agents=7) == -22                               # n_agents > 5
    assert call(env, n_agents=3) == -22                                # a policy of another shape than the environment's
    assert call(env, summed=1, safety=sf) == -22                       # summed together with safety
    assert call(env, act_dim=3, safety=sf) == -22                      # safety with another action width
    assert call(env, steps=0) == -22 and call(env, summed=2) == -22 and call(env, rec=None) == -22
    assert call(env, second=None) == -22 and call(env, second=_lib.FlexBurstMlp()) == -22
    unshared, env_u, _, _ = _mlp_setup("maddpg", 16, shared_params=False)
    calls_u = env_u.calls
    with pytest.raises(ValueError, match="shared_params is False"):
        unshared.test_episodes(env_u, one_launch=True)
    torch.cuda.synchronize()
    assert env.calls == calls and env_u.calls == calls_u and not dummy.any()


def test_parameters_the_kernel_cannot_read_take_the_loop(monkeypatch):
    """An admitted model whose first layer's weight is not contiguous (the same numbers): the launch reads parameters through
    raw pointers, so the default call falls to the loop as the RNN form does, one_launch=True says that the launch declined,
    and the public builder refuses with mlp_burst_declines' reason."""
    from safe_marl_amd import nets
    from safe_marl_amd.learner import one_launch_declines
    monkeypatch.setenv(SWITCH, "1")
    model, env, _, _ = _mlp_setup("maddpg", 17)
    spec = _spec(17, 5)
    good = model.test_episodes(env, spec, steps=3)
    agent = model.policy_dicts[0]
    w = agent.fc1.weight.data
    agent.fc1.weight.data = w.t().contiguous().t()
    assert not agent.fc1.weight.is_contiguous() and torch.equal(agent.fc1.weight.data, w)
    assert one_launch_declines(model) is None
    assert nets.mlp_burst_declines(agent, 5, model.obs_dim, True) == nets.NOT_FP32_DEVICE
    res = model.test_episodes(env, spec, steps=3)
    assert good.launch and not res.launch and (res.length == 3).all()
    assert np.abs(res.sums - good.sums).max() <= 1e-5 * np.abs(good.sums).max()
    with pytest.raises(ValueError, match="declined"):
        model.test_episodes(env, spec, steps=3, one_launch=True)
    with pytest.raises(RuntimeError, match="does not cover this agent"):
        _Launch(model, env)


def test_example_in_a_fresh_process():
    """10. examples/evaluate_policy.py with the MLP agent: --mlp-launch takes the launch and says which entry; without it the loop,
    with the reason."""
    base = [sys.executable, os.path.join(ROOT, "examples", "evaluate_policy.py"), "--alg", "maddpg", "--agent-type", "mlp", "--days", "0:1"]
    env = {k: v for k, v in os.environ.items() if k != SWITCH}
    got = []
    for extra in (["--mlp-launch"], []):
        out = subprocess.run(base + extra, env=env, capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stderr[-2000:]
        got.append(next(json.loads(ln) for ln in reversed(out.stdout.splitlines()) if ln.startswith("{")))
    on, off = got
    assert on["launch_form"] == "one launch (flexenv_test_episodes_mlp)" and on["loop_reason"] is None and on["agent_type"] == "mlp"
    assert off["launch_form"] == "loop" and "agent_type mlp" in off["loop_reason"]
    assert on["episodes"] == off["episodes"] == 96 and on["episode_length"] == off["episode_length"] == {"min": 95, "max": 95}
    assert not on["fallbacks"]
