"""flexenv_rollout_burst_mlp (the one-launch rollout burst of MADDPG / SAFEMADDPG with a shared MLP actor) without a GPU: the
entry point's export, declaration and ctypes binding, the structs and prototypes it must leave alone, the refusals that need no
handle, the compiler's resource report of the four new kernels, RolloutGraph's flag and what body() hands to the launch."""
import ctypes as C
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLEX_EINVAL = -22
NAME = "flexenv_rollout_burst_mlp"


@pytest.fixture(scope="module")
def lib():
    from safe_marl_amd import build, _lib
    build.build()
    return _lib.load()


def _header():
    return open(os.path.join(ROOT, "include", "flexenv.h")).read()


def _proto_args(name):
    proto = re.search(r"int\s+" + name + r"\s*\(([^;]*)\)\s*;", _header()).group(1)
    return re.sub(r"/\*.*?\*/", "", proto, flags=re.S).split(",")


def test_entry_point_is_declared_exported_and_bound(lib):
    from safe_marl_amd import _lib
    assert re.search(r"int\s+" + NAME + r"\s*\(", _header())
    args = [" ".join(a.split()) for a in _proto_args(NAME)]
    assert len(args) == 11
    assert args[8] == "const FlexBurstMlp* mlp" and args[9] == "const FlexBurstSafety* safety" and args[10] == "void* stream"
    assert NAME in _lib.SYMBOLS
    fn = getattr(lib, NAME)                                     # (AttributeError: the library does not export it)
    assert fn.restype is C.c_int and len(fn.argtypes) == 11
    assert fn.argtypes[1] == C.POINTER(_lib.FlexActorArgs) and fn.argtypes[8] == C.POINTER(_lib.FlexBurstMlp)
    assert fn.argtypes[9] == C.POINTER(_lib.FlexBurstSafety)
    from safe_marl_amd.flex_env import VecFlexProvisionEnv
    assert callable(VecFlexProvisionEnv.rollout_burst_mlp)


# the structs and prototypes of the existing burst entry points as the parent commit's header declares them, comments and
# whitespace aside
OLDER = {
    "FlexBurstSafety": "typedef struct { const double* s_p; const double* s_q; const double* beta; double v_min, v_max, penalty; "
                       "double* adjusted; float* env_action; float act_low, act_high; } FlexBurstSafety;",
    "FlexBurstMlp": "typedef struct { const float* fc2_w; const float* fc2_b; } FlexBurstMlp;",
    "flexenv_rollout_burst": "int flexenv_rollout_burst(FlexEnv* env, const FlexActorArgs* actor, double* reward, uint8_t* done, "
                             "double* info, uint8_t* failed, float* obs_ring, int32_t steps, const FlexBurstSafety* safety , "
                             "void* stream);",
    "flexenv_rollout_burst_summed_mlp": "int flexenv_rollout_burst_summed_mlp(FlexEnv* env, const FlexActorArgs* actor, "
                                        "double* reward, uint8_t* done, double* info, uint8_t* failed, float* obs_ring, "
                                        "int32_t steps, const FlexBurstMlp* mlp, const FlexBurstSummed* summed, "
                                        "const FlexBurstSummedGauss* gauss, void* stream);",
}


@pytest.mark.parametrize("name", sorted(OLDER))
def test_older_structs_and_prototypes_are_unchanged(name):
    hdr = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    if name.startswith("Flex"):
        found = re.search(r"typedef struct \{[^}]*\} " + name + ";", hdr).group(0)
    else:
        found = re.search(r"int\s+" + name + r"\s*\([^;]*\)\s*;", hdr).group(0)
    assert " ".join(found.split()) == " ".join(OLDER[name].split())


def test_struct_layouts_are_unchanged():
    from safe_marl_amd import _lib
    assert C.sizeof(_lib.FlexBurstMlp) == 2 * 8 and (_lib.FlexBurstMlp.fc2_w.offset, _lib.FlexBurstMlp.fc2_b.offset) == (0, 8)
    assert C.sizeof(_lib.FlexBurstSafety) == 8 * 8 + 2 * 4
    assert [f[0] for f in _lib.FlexBurstSafety._fields_] == ["s_p", "s_q", "beta", "v_min", "v_max", "penalty", "adjusted",
                                                             "env_action", "act_low", "act_high"]


CASES = ["mlp", "fc2_w", "fc2_b", "n_agents", "steps", "steps_zero", "actor"]


@pytest.mark.parametrize("case,safe", [(c, s) for s in (False, True) for c in CASES] + [("act_dim", True)])
def test_refusals_come_before_any_hip_call(lib, case, safe):
    """On a machine without a device: FLEX_EINVAL, nothing launched.  Each case has ONE thing wrong: every other pointer, the
    handle included, is a non-NULL dummy that none of these refusals follows, so a case fails — or crashes — when its own check
    is removed or moved behind a dereference of the handle or a HIP call.  The GRU pointers and hidden_in are NULL throughout.
    act_dim != 4 is a refusal of the safety phase.  The refusals that read a live handle — a sink without the aux counter among
    them: tests/test_mlp_plain_burst_gpu.py."""
    from safe_marl_amd import _lib
    a = _lib.FlexActorArgs()
    a.rows, a.n_agents, a.obs_dim, a.act_dim, a.ring_slabs = 10, 5, 144, 4, 97
    a.rng_state = 8
    mlp = _lib.FlexBurstMlp()
    mlp.fc2_w, mlp.fc2_b = 8, 8
    sf = _lib.FlexBurstSafety()
    sf.s_p, sf.s_q, sf.beta, sf.adjusted, sf.env_action, sf.act_low, sf.act_high = 8, 8, 8, 8, 8, 0.0, 1.0
    steps = 4
    if case in ("fc2_w", "fc2_b"):
        setattr(mlp, case, None)
    elif case == "act_dim":
        a.act_dim = 3
    elif case == "n_agents":
        a.rows, a.n_agents = 12, 6
    elif case == "steps":
        steps = 97                                              # (a burst as long as the ring)
    elif case == "steps_zero":
        steps = 0
    rc = getattr(lib, NAME)(8, None if case == "actor" else C.byref(a), 8, 8, 8, 8, 8, steps,
                            None if case == "mlp" else C.byref(mlp), C.byref(sf) if safe else None, None)
    assert rc == FLEX_EINVAL


def test_null_handle_is_refused(lib):
    from safe_marl_amd import _lib
    a = _lib.FlexActorArgs()
    a.rows, a.n_agents, a.obs_dim, a.act_dim, a.ring_slabs = 10, 5, 144, 4, 97
    mlp = _lib.FlexBurstMlp()
    mlp.fc2_w, mlp.fc2_b = 8, 8
    assert getattr(lib, NAME)(None, C.byref(a), 8, 8, 8, 8, 8, 4, C.byref(mlp), None, None) == FLEX_EINVAL


NEW = "plain_mlp"
OLD = ("flex_rollout_burst_kernel<", "summed::flex_rollout_burst_kernel<", "summed_gauss::flex_rollout_burst_kernel<",
       "summed_mlp::flex_rollout_burst_kernel<", "summed_gauss_mlp::flex_rollout_burst_kernel<")


def test_resources_of_the_new_kernels():
    """The new form is four instantiations under a namespace of its own (the sets under flex_rollout_burst_kernel< and the
    summed:: families are pinned by other tests and the new names start with none of their prefixes); the burst's LDS image and
    occupancy, no AGPRs, at most 256 VGPRs, and no more scratch than the largest of the twelve existing burst kernels — that
    figure read from this build."""
    from safe_marl_amd import build
    build.build()
    new = build.kernel_resources(f"{NEW}::flex_rollout_burst_kernel<")
    assert sorted(v["name"] for v in new.values()) == sorted(f"{NEW}::flex_rollout_burst_kernel<{c}, {s}>"
                                                             for c in (5, 8) for s in ("false", "true"))
    assert not NEW.startswith("summed") and not f"{NEW}::flex_rollout_burst_kernel<".startswith(OLD[0])
    old = {}
    for prefix in OLD:
        old.update(build.kernel_resources(prefix))
    assert len(old) == 12 and len(new) == 4 and not set(old) & set(new)
    assert len(build.kernel_resources(OLD[0])) == 4
    most = max(v["scratch_bytes_per_lane"] for v in old.values())
    for v in list(new.values()) + list(old.values()):
        print(f"{v['name']}: {v['vgprs']} VGPRs + {v['agprs']} AGPRs, {v['sgprs']} SGPRs, LDS {v['lds_bytes_per_block']} B, "
              f"{v['waves_per_simd']} waves/SIMD, scratch {v['scratch_bytes_per_lane']} B/lane")
    for v in new.values():
        assert v["lds_bytes_per_block"] == 153648 and v["waves_per_simd"] == 2 and v["agprs"] == 0, v
        assert v["vgprs"] <= 256 and v["scratch_bytes_per_lane"] <= most, (v, most)
    for v in old.values():                                      # the existing forms keep the image
        assert v["lds_bytes_per_block"] == 153648 and v["waves_per_simd"] == 2


# ---- RolloutGraph.mlp_plain_burst without a device ------------------------------------------------------------------------------
class _StubVec:
    """What RolloutGraph.__init__ asks of an env while it decides: shapes, CPU buffers and the names of the device-side hooks."""
    history, n_bus = 24, 33

    def __init__(self, n_envs, n_agents, with_method=True):
        import torch
        self.n_envs, self.n_agents = n_envs, n_agents
        self.obs = torch.zeros(n_envs, n_agents, 144)
        self.info = torch.zeros(n_envs, 7, dtype=torch.float64)
        self.rollout_burst = lambda *a, **k: None
        self.rollout_burst_summed_mlp = lambda *a, **k: None
        self.rollout_burst_summed = lambda *a, **k: None
        if with_method:
            self.rollout_burst_mlp = lambda *a, **k: None


def _model(alg="maddpg", agents=5, **over):
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    from train_maddpg import DEFAULT_ALG_ARGS, PPO_ALG_ARGS
    from safe_marl_amd import learner
    from safe_marl_amd.util import convert
    a = dict(DEFAULT_ALG_ARGS)
    if alg == "ippo":
        a.update(PPO_ALG_ARGS)
    a.update(alg=alg, agent_num=agents, obs_size=144, state_size=110, action_dim=4, agent_type="mlp", cuda=False,
             v_min=0.9, v_max=1.1)
    a.update(over)
    if alg == "safemaddpg":                                     # (a predictor triple handed in: nothing is fitted on an env)
        import torch
        return learner.SAFEMADDPG(convert(a), None, predictor=tuple(torch.full((agents,), v, dtype=torch.float64)
                                                                     for v in (0.1, 0.05, 0.01)))
    return {"ippo": learner.IPPO, "maddpg": learner.MADDPG}[alg](convert(a))


def _decide(monkeypatch, model, env, **environ):
    """RolloutGraph's decision for ``model`` on ``env`` with everything that needs a device taken as given: the CPU tensors are
    presented as device tensors to __init__'s own tests, and no buffer is allocated on a device (the model's device is the CPU)."""
    import torch
    from safe_marl_amd import learner
    from safe_marl_amd.replay_buffer import TransReplayBuffer
    for k in ("FLEX_MLP_BURST", "FLEX_GAUSS_BURST", "FLEX_SUMMED_BURST", "FLEX_SUMMED_SINK", "FLEX_ROLLOUT_BURST"):
        monkeypatch.delenv(k, raising=False)
    for k, v in environ.items():
        monkeypatch.setenv(k, v)
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True))
    monkeypatch.setattr(learner.RolloutGraph, "_configure_env", lambda self: None)
    for hook in ("obs_source", "set_obs_ring", "set_step_counter", "set_replay_sink"):
        setattr(env, hook, lambda *a, **k: None)
    return learner.RolloutGraph(model, env, TransReplayBuffer(env.n_envs * 96 * 2))


def test_cpu_model_has_no_mlp_plain_burst():
    from safe_marl_amd.learner import RolloutGraph
    from safe_marl_amd.replay_buffer import TransReplayBuffer
    rg = RolloutGraph(_model(), _StubVec(4, 5), TransReplayBuffer(4 * 96 * 2))
    assert rg.mlp_plain_burst is False and not rg.fused_burst and not rg.sink_active and not rg.ring_active


@pytest.mark.parametrize("alg", ["maddpg", "safemaddpg"])
def test_flag_and_its_reasons(alg, monkeypatch):
    """On for MADDPG and SAFEMADDPG with a shared MLPAgent — with it sink, ring, the fused burst and one chunk per run, and
    neither `fast` nor the summed family; off for each reason the flag names."""
    rg = _decide(monkeypatch, _model(alg), _StubVec(4, 5))
    assert rg.mlp_plain_burst and rg.fused_burst and rg.sink_active and rg.ring_active
    assert not rg.fast and not rg.mlp_burst and not rg.summed and not rg.sink and not rg.burst_launch
    assert rg.safe == (alg == "safemaddpg") and hasattr(rg, "burst_safe_env_act") == rg.safe
    assert rg.burst_chunks(40) == [40] and rg.burst_chunks(1) == [1]
    for name in ("act_buf", "hid_buf", "acc", "means_buf", "burst_env_act"):
        assert hasattr(rg, name), name
    # the RNN agent: `fast` and its burst as before, the new flag off
    rg = _decide(monkeypatch, _model(alg, agent_type="rnn"), _StubVec(4, 5))
    assert not rg.mlp_plain_burst and rg.fast and rg.sink and rg.burst_launch and rg.fused_burst
    for env in ({"FLEX_MLP_BURST": "0"}, {"FLEX_ROLLOUT_BURST": "0"}):
        rg = _decide(monkeypatch, _model(alg), _StubVec(4, 5), **env)
        assert not rg.mlp_plain_burst and not rg.fast and not rg.fused_burst and not rg.sink_active and not rg.ring_active, env
    rg = _decide(monkeypatch, _model(alg, agents=6), _StubVec(4, 6))
    assert not rg.mlp_plain_burst
    rg = _decide(monkeypatch, _model(alg, hid_activation="tanh"), _StubVec(4, 5))
    assert not rg.mlp_plain_burst
    rg = _decide(monkeypatch, _model(alg, gaussian_policy=True), _StubVec(4, 5))
    assert rg.gaussian and not rg.mlp_plain_burst and not rg.sink_active
    rg = _decide(monkeypatch, _model(alg, action_enforcebound=False), _StubVec(4, 5))
    assert not rg.mlp_plain_burst
    rg = _decide(monkeypatch, _model(alg, shared_params=False), _StubVec(4, 5))
    assert not rg.mlp_plain_burst
    rg = _decide(monkeypatch, _model(alg), _StubVec(4, 5, with_method=False))
    assert not rg.mlp_plain_burst and not rg.fused_burst
    if alg == "safemaddpg":
        m = _model(alg)
        m.intended_actions = True
        rg = _decide(monkeypatch, m, _StubVec(4, 5))
        assert not rg.mlp_plain_burst and not rg.fused_burst


def test_ippo_keeps_its_own_flag(monkeypatch):
    rg = _decide(monkeypatch, _model("ippo"), _StubVec(4, 5))
    assert rg.mlp_burst and rg.summed and not rg.mlp_plain_burst


def _body_setup(monkeypatch, alg):
    import torch
    from safe_marl_amd import _lib
    m = _model(alg)
    env = _StubVec(4, 5)
    rg = _decide(monkeypatch, m, env)
    monkeypatch.undo()                                          # (tensors are CPU tensors again: the helper's checks below are real)
    rg.obs_src = _lib.FlexObsSource()
    rg.buf.cursor = torch.zeros(2, dtype=torch.int64)
    rg.buf.row_ring = torch.zeros(1)
    rg.buf.slabs = 97
    return rg, m, env


@pytest.mark.parametrize("alg", ["maddpg", "safemaddpg"])
def test_body_hands_everything_to_the_one_launch(alg, monkeypatch):
    """body() and body(burst=40) of the new form: one call of the env's method each with the MLP's second layer, the output head
    as fc2, no GRU pointers, the noise stream's cell, std and the action range — and neither Model.policy, fused_actor_forward
    nor a draw from torch's generator."""
    import torch
    import torch.distributions.normal as tdn
    from safe_marl_amd import learner, nets
    rg, m, env = _body_setup(monkeypatch, alg)
    seen = []
    env.rollout_burst_mlp = lambda *a, **k: seen.append((a, k))
    monkeypatch.setattr(tdn, "_standard_normal", lambda *a, **k: pytest.fail("tdn._standard_normal called"))
    monkeypatch.setattr(type(m), "policy", lambda *a, **k: pytest.fail("Model.policy called"))
    monkeypatch.setattr(learner, "fused_actor_forward", lambda *a, **k: pytest.fail("fused_actor_forward called"))
    monkeypatch.setattr(nets, "_params_decline", lambda params: None)      # (CPU parameters here)
    state = torch.get_rng_state()
    for k in (0, 40):
        rg.body(burst=k)
    assert torch.equal(torch.get_rng_state(), state)            # torch's generator was not touched
    assert len(seen) == 2
    agent = m.policy_dicts[0]
    for (a, kw), k in zip(seen, (1, 40)):
        args, mlp, steps, ring = a
        assert steps == k and ring is rg.buf.row_ring and set(kw) == {"safety"}
        assert args.fc2_w == agent.fc3.weight.data_ptr() and args.fc2_b == agent.fc3.bias.data_ptr()
        assert mlp.fc2_w == agent.fc2.weight.data_ptr() and mlp.fc2_b == agent.fc2.bias.data_ptr()
        assert not args.hidden_in and not args.w_ih and not args.w_hh and not args.b_ih and not args.b_hh and not args.noise
        assert args.rows == 20 and args.ring_slabs == 97 and args.act_dim == 4 and args.obs_dim == 144
        assert args.rng_state == rg.rng_state.data_ptr()
        assert args.std == pytest.approx(float(m.args.fixed_policy_std)) and args.std > 0
        assert (args.action_low, args.action_high) == (pytest.approx(m.args.action_low), pytest.approx(m.args.action_high))
        assert args.action_high > args.action_low
        assert args.hidden_out == rg.hid_buf.data_ptr() and args.means == rg.means_buf.data_ptr()
        assert args.action == rg.act_buf.data_ptr() and args.env_action == rg.burst_env_act.data_ptr()
        if alg == "safemaddpg":
            sf = kw["safety"]
            assert sf["adjusted"] is rg.burst_adjusted and sf["env_action"] is rg.burst_safe_env_act
            assert (sf["act_low"], sf["act_high"]) == (m.args.action_low, m.args.action_high)
            assert all(sf[k].dtype == torch.float64 and sf[k].numel() == 5 for k in ("s_p", "s_q", "beta"))
        else:
            assert kw["safety"] is None


def test_there_is_no_second_form(monkeypatch):
    """torch_noise and fast have nothing to switch to: their setters raise (and switching them off, which changes nothing,
    passes); body() raises when intended_actions was switched on after construction."""
    rg, m, env = _body_setup(monkeypatch, "safemaddpg")
    with pytest.raises(RuntimeError, match="torch_noise"):
        rg.torch_noise = True
    with pytest.raises(RuntimeError, match="fast"):
        rg.fast = True
    assert not rg.torch_noise and not rg.fast and rg.fused_burst
    env.rollout_burst_mlp = lambda *a, **k: pytest.fail("launched")
    m.intended_actions = True
    with pytest.raises(RuntimeError, match="intended_actions"):
        rg.body()
    with pytest.raises(RuntimeError, match="intended_actions"):
        rg.body(burst=4)


def test_existing_callers_of_the_args_helper_are_unaffected(monkeypatch):
    """nets.mlp_burst_actor_args without the new arguments: no noise cell, zero std and range, as the agent-summed forms pass it."""
    import torch
    from safe_marl_amd import _lib, nets
    m = _model()
    monkeypatch.setattr(nets, "_params_decline", lambda params: None)
    cur = torch.zeros(2, dtype=torch.int64)
    hid, means = torch.zeros(20, 64), torch.zeros(20, 4)
    args, mlp = nets.mlp_burst_actor_args(m.policy_dicts[0], 4, 5, 144, m.args.agent_id, ring_cursor=cur, cursor_out=cur[1:],
                                          obs_source=_lib.FlexObsSource(), ring_slabs=97, hidden_out=hid, means=means)
    assert not args.rng_state and args.std == 0.0 and args.action_low == 0.0 and args.action_high == 0.0
    with pytest.raises(ValueError):
        nets.mlp_burst_actor_args(m.policy_dicts[0], 4, 5, 144, m.args.agent_id, ring_cursor=cur, cursor_out=cur[1:],
                                  obs_source=_lib.FlexObsSource(), ring_slabs=97, hidden_out=hid, means=means,
                                  rng_state=torch.zeros(2, dtype=torch.int64))
