"""flexenv_rollout_burst_summed_mlp (the one-launch rollout burst of the agent-summed algorithms with a shared MLP actor) without
a GPU: the entry point's export, declaration and ctypes binding, its struct's layout, the older structs and prototypes it must
leave alone, the refusals that need no handle, the compiler's resource report of the four new kernels, and RolloutGraph's flag."""
import ctypes as C
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLEX_EINVAL = -22
NAME = "flexenv_rollout_burst_summed_mlp"


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


def _struct_fields(name):
    body = re.search(r"typedef struct \{([^}]*)\} " + name + ";", _header()).group(1)
    return re.findall(r"(\w+)\s*[;,]", re.sub(r"/\*.*?\*/", "", body, flags=re.S))


def test_entry_point_is_declared_exported_and_bound(lib):
    from safe_marl_amd import _lib
    assert re.search(r"int\s+" + NAME + r"\s*\(", _header())
    assert len(_proto_args(NAME)) == 12
    assert NAME in _lib.SYMBOLS
    fn = getattr(lib, NAME)                                     # (AttributeError: the library does not export it)
    assert fn.restype is C.c_int and len(fn.argtypes) == 12
    assert fn.argtypes[1] == C.POINTER(_lib.FlexActorArgs) and fn.argtypes[8] == C.POINTER(_lib.FlexBurstMlp)
    assert fn.argtypes[9] == C.POINTER(_lib.FlexBurstSummed) and fn.argtypes[10] == C.POINTER(_lib.FlexBurstSummedGauss)


def test_struct_layout():
    from safe_marl_amd import _lib
    S = _lib.FlexBurstMlp
    assert C.sizeof(S) == 2 * 8
    assert [f[0] for f in S._fields_] == ["fc2_w", "fc2_b"] == _struct_fields("FlexBurstMlp")
    assert (S.fc2_w.offset, S.fc2_b.offset) == (0, 8)


# the three older structs and prototypes as the parent commit's header declares them, comments and whitespace aside
OLDER = {
    "FlexBurstSafety": "typedef struct { const double* s_p; const double* s_q; const double* beta; double v_min, v_max, penalty; "
                       "double* adjusted; float* env_action; float act_low, act_high; } FlexBurstSafety;",
    "FlexBurstSummed": "typedef struct { const float* eps; const float* std; float act_low, act_high; } FlexBurstSummed;",
    "FlexBurstSummedGauss": "typedef struct { const float* eps; const float* log_std_w; const float* log_std_b; float* log_stds; "
                            "float log_std_min, log_std_max; float act_low, act_high; } FlexBurstSummedGauss;",
    "flexenv_rollout_burst": "int flexenv_rollout_burst(FlexEnv* env, const FlexActorArgs* actor, double* reward, uint8_t* done, "
                             "double* info, uint8_t* failed, float* obs_ring, int32_t steps, const FlexBurstSafety* safety , "
                             "void* stream);",
    "flexenv_rollout_burst_summed": "int flexenv_rollout_burst_summed(FlexEnv* env, const FlexActorArgs* actor, double* reward, "
                                    "uint8_t* done, double* info, uint8_t* failed, float* obs_ring, int32_t steps, "
                                    "const FlexBurstSummed* summed, void* stream);",
    "flexenv_rollout_burst_summed_gauss": "int flexenv_rollout_burst_summed_gauss(FlexEnv* env, const FlexActorArgs* actor, "
                                          "double* reward, uint8_t* done, double* info, uint8_t* failed, float* obs_ring, "
                                          "int32_t steps, const FlexBurstSummedGauss* gauss, void* stream);",
}


@pytest.mark.parametrize("name", sorted(OLDER))
def test_older_structs_and_prototypes_are_unchanged(name):
    hdr = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    if name.startswith("Flex"):
        found = re.search(r"typedef struct \{[^}]*\} " + name + ";", hdr).group(0)
    else:
        found = re.search(r"int\s+" + name + r"\s*\([^;]*\)\s*;", hdr).group(0)
    assert " ".join(found.split()) == " ".join(OLDER[name].split())


def test_older_bindings_are_unchanged(lib):
    from safe_marl_amd import _lib
    for name, struct in (("flexenv_rollout_burst", _lib.FlexBurstSafety), ("flexenv_rollout_burst_summed", _lib.FlexBurstSummed),
                         ("flexenv_rollout_burst_summed_gauss", _lib.FlexBurstSummedGauss)):
        fn = getattr(lib, name)
        assert len(fn.argtypes) == 10 and fn.argtypes[8] == C.POINTER(struct)
    assert C.sizeof(_lib.FlexBurstSafety) == 8 * 8 + 2 * 4
    assert C.sizeof(_lib.FlexBurstSummed) == 2 * 8 + 2 * 4
    assert C.sizeof(_lib.FlexBurstSummedGauss) == 4 * 8 + 4 * 4


@pytest.mark.parametrize("form", ["summed", "gauss"])
@pytest.mark.parametrize("case", ["mlp", "fc2_w", "fc2_b", "both", "neither", "act_dim", "n_agents", "steps", "steps_zero",
                                  "actor", "eps"])
def test_refusals_come_before_any_hip_call(lib, case, form):
    """On a machine without a device: FLEX_EINVAL, nothing launched.  Each case has ONE thing wrong: every other pointer, the
    handle included, is a non-NULL dummy that none of these refusals follows, so a case fails — or crashes — when its own check
    is removed or moved behind a dereference of the handle or a HIP call.  The GRU pointers and hidden_in are NULL throughout.
    The refusals that read a live handle: tests/test_mlp_burst_gpu.py."""
    from safe_marl_amd import _lib
    a = _lib.FlexActorArgs()
    a.rows, a.n_agents, a.obs_dim, a.act_dim, a.ring_slabs = 10, 5, 144, 4, 97
    mlp = _lib.FlexBurstMlp()
    mlp.fc2_w, mlp.fc2_b = 8, 8
    sm = _lib.FlexBurstSummed()
    sm.eps, sm.std, sm.act_low, sm.act_high = 8, 8, 0.0, 1.0
    sg = _lib.FlexBurstSummedGauss()
    sg.eps, sg.log_std_w, sg.log_std_b, sg.log_stds = 8, 8, 8, 8
    sg.log_std_min, sg.log_std_max, sg.act_low, sg.act_high = 0.0, 0.5, 0.0, 1.0
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
    elif case == "eps":
        sm.eps = sg.eps = None
    p_sm = C.byref(sm) if (form == "summed" or case == "both") and case != "neither" else None
    p_sg = C.byref(sg) if (form == "gauss" or case == "both") and case != "neither" else None
    rc = getattr(lib, NAME)(8, None if case == "actor" else C.byref(a), 8, 8, 8, 8, 8, steps,
                            None if case == "mlp" else C.byref(mlp), p_sm, p_sg, None)
    assert rc == FLEX_EINVAL


NEW = ("summed_mlp", "summed_gauss_mlp")
OLD = ("flex_rollout_burst_kernel<", "summed::flex_rollout_burst_kernel<", "summed_gauss::flex_rollout_burst_kernel<")


def test_resources_of_the_new_kernels():
    """The two new forms are two instantiations each under names of their own (the sets under flex_rollout_burst_kernel< and
    summed::flex_rollout_burst_kernel< are pinned by other tests and the new names start with neither); the burst's LDS image
    and occupancy, no AGPRs, at most 256 VGPRs, and no more scratch than the largest of the eight existing burst kernels — that
    figure read from this build."""
    from safe_marl_amd import build
    build.build()
    new = {}
    for ns in NEW:
        got = build.kernel_resources(f"{ns}::flex_rollout_burst_kernel<")
        assert sorted(v["name"] for v in got.values()) == [f"{ns}::flex_rollout_burst_kernel<{c}>" for c in (5, 8)]
        assert not any(ns.startswith(p.split("::")[0] + "::") for p in OLD[1:]) and not f"{ns}::".startswith(OLD[0])
        new.update(got)
    old = {}
    for prefix in OLD:
        old.update(build.kernel_resources(prefix))
    assert len(old) == 8 and len(new) == 4 and not set(old) & set(new)
    most = max(v["scratch_bytes_per_lane"] for v in old.values())
    for v in list(new.values()) + list(old.values()):
        print(f"{v['name']}: {v['vgprs']} VGPRs + {v['agprs']} AGPRs, {v['sgprs']} SGPRs, LDS {v['lds_bytes_per_block']} B, "
              f"{v['waves_per_simd']} waves/SIMD, scratch {v['scratch_bytes_per_lane']} B/lane")
    for v in new.values():
        assert v["lds_bytes_per_block"] == 153648 and v["waves_per_simd"] == 2 and v["agprs"] == 0, v
        assert v["vgprs"] <= 256 and v["scratch_bytes_per_lane"] <= most, (v, most)
    for v in old.values():                                      # the existing forms keep the image
        assert v["lds_bytes_per_block"] == 153648 and v["waves_per_simd"] == 2


# ---- RolloutGraph.mlp_burst without a device ------------------------------------------------------------------------------------
class _StubVec:
    """What RolloutGraph.__init__ asks of an env while it decides: shapes, CPU buffers and the names of the device-side hooks."""
    history, n_bus = 24, 33

    def __init__(self, n_envs, n_agents, with_method=True):
        import torch
        self.n_envs, self.n_agents = n_envs, n_agents
        self.obs = torch.zeros(n_envs, n_agents, 144)
        self.info = torch.zeros(n_envs, 7, dtype=torch.float64)
        if with_method:
            self.rollout_burst_summed_mlp = lambda *a, **k: None
            self.rollout_burst_summed = lambda *a, **k: None


def _model(alg="ippo", agents=5, **over):
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    from train_maddpg import DEFAULT_ALG_ARGS, PPO_ALG_ARGS
    from safe_marl_amd import learner
    from safe_marl_amd.util import convert
    a = dict(DEFAULT_ALG_ARGS)
    if alg == "ippo":
        a.update(PPO_ALG_ARGS)
    a.update(alg=alg, agent_num=agents, obs_size=144, state_size=110, action_dim=4, agent_type="mlp", cuda=False)
    a.update(over)
    return {"ippo": learner.IPPO, "matd3": learner.MATD3, "maddpg": learner.MADDPG}[alg](convert(a))


def test_cpu_model_has_no_mlp_burst():
    """A model on the CPU: the observation is no device tensor, nothing of the summed family is admitted, mlp_burst included."""
    from safe_marl_amd.learner import RolloutGraph
    from safe_marl_amd.replay_buffer import TransReplayBuffer
    m = _model()
    rg = RolloutGraph(m, _StubVec(4, 5), TransReplayBuffer(4 * 96 * 2))
    assert rg.mlp_burst is False and not rg.summed and not rg.summed_sink and not rg.fused_burst and not rg.sink_active


def _decide(monkeypatch, model, env, **environ):
    """RolloutGraph's decision for ``model`` on ``env`` with everything that needs a device taken as given: `summed` and the
    sink's shape conditions are forced true by presenting the CPU tensors as device tensors to __init__'s own tests, and no
    buffer is allocated on a device (the model's device is the CPU)."""
    import torch
    from safe_marl_amd import learner
    from safe_marl_amd.replay_buffer import TransReplayBuffer
    for k in ("FLEX_MLP_BURST", "FLEX_GAUSS_BURST", "FLEX_SUMMED_BURST", "FLEX_SUMMED_SINK"):
        monkeypatch.delenv(k, raising=False)
    for k, v in environ.items():
        monkeypatch.setenv(k, v)
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True))
    monkeypatch.setattr(learner.RolloutGraph, "_configure_env", lambda self: None)
    for hook in ("obs_source", "set_obs_ring", "set_step_counter", "set_replay_sink"):
        setattr(env, hook, lambda *a, **k: None)
    return learner.RolloutGraph(model, env, TransReplayBuffer(env.n_envs * 96 * 2))


def test_flag_and_its_reasons(monkeypatch):
    """The flag on whatever can be built without a device: on for a shared MLPAgent under an agent-summed algorithm; off for the
    RNN agent, with FLEX_MLP_BURST=0 (then the object is what it was: summed_sink and summed_burst set), for six agents, for
    tanh, for an env without the method, for MADDPG, and for the Gaussian MLP agent unless FLEX_GAUSS_BURST=1."""
    rg = _decide(monkeypatch, _model(), _StubVec(4, 5))
    assert rg.summed and rg.mlp_burst and rg.fused_burst and rg.sink_active and rg.ring_active
    assert not rg.summed_sink and not rg.summed_burst and not rg.gauss_burst
    assert rg.burst_chunks(40) == [40]
    rg = _decide(monkeypatch, _model("matd3"), _StubVec(4, 5))
    assert rg.mlp_burst and rg.fused_burst
    rg = _decide(monkeypatch, _model(agent_type="rnn"), _StubVec(4, 5))
    assert not rg.mlp_burst and rg.summed_sink and rg.summed_burst
    rg = _decide(monkeypatch, _model(), _StubVec(4, 5), FLEX_MLP_BURST="0")
    assert not rg.mlp_burst and rg.summed_sink and rg.summed_burst          # (as before: body() then declines and the trainer falls back)
    rg = _decide(monkeypatch, _model(), _StubVec(4, 5), FLEX_SUMMED_BURST="0")
    assert not rg.mlp_burst
    rg = _decide(monkeypatch, _model(agents=6), _StubVec(4, 6))
    assert not rg.mlp_burst and not rg.summed_burst
    rg = _decide(monkeypatch, _model(hid_activation="tanh"), _StubVec(4, 5))
    assert not rg.mlp_burst
    rg = _decide(monkeypatch, _model(), _StubVec(4, 5, with_method=False))
    assert not rg.mlp_burst
    rg = _decide(monkeypatch, _model("maddpg"), _StubVec(4, 5))
    assert not rg.mlp_burst and not rg.summed
    rg = _decide(monkeypatch, _model(gaussian_policy=True), _StubVec(4, 5))
    assert rg.gaussian and not rg.mlp_burst and not rg.sink_active and not rg.fused_burst
    rg = _decide(monkeypatch, _model(gaussian_policy=True), _StubVec(4, 5), FLEX_GAUSS_BURST="1")
    assert rg.gaussian and rg.mlp_burst and rg.fused_burst and not rg.gauss_burst and hasattr(rg, "log_stds_buf")
    rg = _decide(monkeypatch, _model(gaussian_policy=True), _StubVec(4, 5), FLEX_GAUSS_BURST="1", FLEX_MLP_BURST="0")
    assert not rg.mlp_burst and not rg.gauss_burst


def test_body_never_calls_model_policy_or_the_rnn_wrapper(monkeypatch):
    """body() and body(burst=k) of the new form: one draw of (k, N, 1, 4), one call of the env's method with the MLP's second layer
    and the output head as fc2 — and neither Model.policy nor fused_actor_forward."""
    import torch
    import torch.distributions.normal as tdn
    from safe_marl_amd import _lib, learner, nets
    m = _model()
    env = _StubVec(4, 5)
    rg = _decide(monkeypatch, m, env)
    monkeypatch.undo()                                          # (tensors are CPU tensors again: the helper's checks below are real)
    seen, draws = [], []
    env.rollout_burst_summed_mlp = lambda *a, **k: seen.append((a, k))
    real = tdn._standard_normal
    monkeypatch.setattr(tdn, "_standard_normal", lambda shape, *a: (draws.append(tuple(shape)), real(shape, *a))[1])
    monkeypatch.setattr(type(m), "policy", lambda *a, **k: pytest.fail("Model.policy called"))
    monkeypatch.setattr(learner, "fused_actor_forward", lambda *a, **k: pytest.fail("fused_actor_forward called"))
    monkeypatch.setattr(nets, "_params_decline", lambda params: None)      # (CPU parameters here)
    src = _lib.FlexObsSource()
    rg.obs_src = src
    rg.buf.cursor = torch.zeros(2, dtype=torch.int64)
    rg.buf.row_ring = torch.zeros(1)
    rg.buf.slabs = 97
    for k in (0, 40):
        rg.body(burst=k)
    assert draws == [(1, 4, 1, 4), (40, 4, 1, 4)] and len(seen) == 2
    agent = m.policy_dicts[0]
    for (a, kw), k in zip(seen, (1, 40)):
        args, mlp, steps = a[0], a[1], a[2]
        assert steps == k and set(kw) == {"std"}
        assert args.fc2_w == agent.fc3.weight.data_ptr() and args.fc2_b == agent.fc3.bias.data_ptr()
        assert mlp.fc2_w == agent.fc2.weight.data_ptr() and mlp.fc2_b == agent.fc2.bias.data_ptr()
        assert not args.hidden_in and not args.w_ih and not args.w_hh and not args.b_ih and not args.b_hh
        assert args.rows == 20 and args.ring_slabs == 97 and args.act_dim == 4 and args.obs_dim == 144
        assert args.hidden_out == rg.hid_buf.data_ptr() and args.means == rg.means_buf.data_ptr()
        assert args.action == rg.act_buf.data_ptr() and args.env_action == rg.env_act_buf.data_ptr()
