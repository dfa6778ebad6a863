"""CPU: the surface of the one-launch test-mode episodes of a shared MLP agent (include/flexenv.h: flexenv_test_episodes_mlp) —
declaration, export and binding, the argument checks that come before any HIP call, the compiler's resource report of the
three new kernels next to the three they are modelled on, the opt-in eligibility decision (FLEX_MLP_TEST_LAUNCH, read at call
time) and the example's command line.  Nothing here touches a GPU."""
import ctypes as C
import hashlib
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "examples"))
FLEX_EINVAL = -22
SWITCH = "FLEX_MLP_TEST_LAUNCH"

# the declarations this pull request must leave as they are, as the parent commit has them
FLEX_TEST_OUT = """typedef struct {
    double*  sums;     /* [N,10]: info[0..6], reward, steps with voltage_penalty > 0, solver_failed — each summed
                          over the episode's own steps IN STEP ORDER (fp64, one accumulator per env: no atomics) */
    int32_t* length;   /* [N]: steps the episode ran (ends on done — episode_limit or solver failure — or at `steps`) */
    /* optional per-step trace, every pointer may be NULL; row t of an env is written only while its episode is alive */
    float*   actions;  /* [steps,N,n_agents,4]  what the env step read */
    double*  v;        /* [steps,N,n_bus] */
    double*  agent;    /* [steps,N,n_agents,5]  E, PRED, CH, DIS, QPV after the step (the FLEX_PEEK_* fields) */
    int32_t* row;      /* [steps,N]  data row after the step (FLEX_PEEK ROW) */
    double*  reward;   /* [steps,N] */
    double*  info;     /* [steps,N,7] */
    uint8_t* flags;    /* [steps,N]  bit0 done, bit1 solver_failed, bit2 alive (row valid); the one array written for
                          EVERY step: 0 behind the episode's end */
} FlexTestOut;
int flexenv_test_episodes(FlexEnv* env, const FlexActorArgs* actor, int32_t steps, int32_t summed,
                          const FlexBurstSafety* safety /* or NULL */, const FlexTestOut* out, void* stream);
"""
FLEX_BURST_MLP = """typedef struct {
    const float* fc2_w;   /* dev [64, 64]: the second layer's weight */
    const float* fc2_b;   /* dev [64]: its bias */
} FlexBurstMlp;
"""
FLEX_ACTOR_ARGS_SHA256 = "6a48cce283f640cc041c8e2c14ffd87db0948398fa109ca2c5b7fdb601e6cb5b"     # include/flexnet.h: 4 642 characters
PROTOTYPE = """int flexenv_test_episodes_mlp(FlexEnv* env, const FlexActorArgs* actor, int32_t steps, int32_t summed,
                              const FlexBurstMlp* mlp, const FlexBurstSafety* safety /* or NULL */,
                              const FlexTestOut* out, void* stream);
"""


@pytest.fixture(scope="module")
def lib():
    from safe_marl_amd import build, _lib
    build.build()
    return _lib.load()


def _header(name):
    return open(os.path.join(ROOT, "include", name)).read()


def _actor_args_decl(text):
    m = re.search(r"typedef struct \{(?:(?!typedef struct).)*?\} FlexActorArgs;", text, flags=re.S)
    assert m, "FlexActorArgs is not declared"
    return m.group(0)


def test_entry_point_is_declared_exported_and_bound(lib):
    from safe_marl_amd import _lib
    hdr = _header("flexenv.h")
    assert "#define FLEX_ABI_VERSION 2" in hdr                       # an addition: no existing argument changes meaning
    assert PROTOTYPE in hdr
    assert "flexenv_test_episodes_mlp" in _lib.SYMBOLS and hasattr(lib, "flexenv_test_episodes_mlp")
    vp = C.c_void_p
    assert list(lib.flexenv_test_episodes_mlp.argtypes) == [vp, C.POINTER(_lib.FlexActorArgs), C.c_int32, C.c_int32,
                                                            C.POINTER(_lib.FlexBurstMlp), C.POINTER(_lib.FlexBurstSafety),
                                                            C.POINTER(_lib.FlexTestOut), vp]
    assert lib.flexenv_test_episodes_mlp.restype is C.c_int
    # what stays: the record, the second layer's struct, the RNN entry and the actor's struct, textually
    assert FLEX_TEST_OUT in hdr and FLEX_BURST_MLP in hdr
    decl = _actor_args_decl(_header("flexnet.h"))
    assert hashlib.sha256(decl.encode()).hexdigest() == FLEX_ACTOR_ARGS_SHA256
    assert [f[0] for f in _lib.FlexBurstMlp._fields_] == ["fc2_w", "fc2_b"] and C.sizeof(_lib.FlexBurstMlp) == 16
    assert C.sizeof(_lib.FlexTestOut) == 9 * 8
    for f, _ in _lib.FlexActorArgs._fields_:                           # every bound field is a declared one
        assert re.search(r"\b%s\b" % f, decl), f
    assert list(lib.flexenv_test_episodes.argtypes) == [vp, C.POINTER(_lib.FlexActorArgs), C.c_int32, C.c_int32,
                                                        C.POINTER(_lib.FlexBurstSafety), C.POINTER(_lib.FlexTestOut), vp]
    # the header says what is and is not read
    comment = hdr[:hdr.index(PROTOTYPE)].rsplit("/*", 1)[1]
    for word in ("hidden_in", "w_ih", "b_hh", "may be NULL", "hidden_out", "fc2_w", "FLEX_EINVAL"):
        assert word in comment, word


CASES = ["mlp", "fc2_w", "fc2_b", "actor", "out", "sums", "length", "steps", "summed", "summed+safety", "safety act_dim", "agents"]


def _call(lib, case, handle):
    """A call with ONE thing wrong (``case``; None: nothing): every other pointer a non-NULL dummy that no check follows,
    hidden_in and the GRU pointers NULL throughout."""
    from safe_marl_amd import _lib
    d = 4096                                                           # a dummy address: not followed
    a = _lib.FlexActorArgs()
    a.rows, a.n_agents, a.obs_dim, a.act_dim = 80, 5, 144, 4
    for k in ("hidden_out", "means", "action", "env_action", "fc1_w", "fc1_b", "fc2_w", "fc2_b", "ln_w", "ln_b"):
        setattr(a, k, d)
    a.layernorm, a.action_low, a.action_high = 1, 0.0, 1.0
    assert not a.hidden_in and not a.w_ih and not a.w_hh and not a.b_ih and not a.b_hh
    out = _lib.FlexTestOut()
    out.sums, out.length = d, d
    mlp = _lib.FlexBurstMlp()
    mlp.fc2_w, mlp.fc2_b = d, d
    sf = None
    steps, summed = 95, 0

    def safety():
        s = _lib.FlexBurstSafety()
        for k in ("s_p", "s_q", "beta", "adjusted", "env_action"):
            setattr(s, k, d)
        s.act_high = 1.0
        return s
    if case == "fc2_w":
        mlp.fc2_w = None
    elif case == "fc2_b":
        mlp.fc2_b = None
    elif case == "sums":
        out.sums = None
    elif case == "length":
        out.length = None
    elif case == "steps":
        steps = 0
    elif case == "summed":
        summed = 2
    elif case == "summed+safety":
        summed, sf = 1, safety()
    elif case == "safety act_dim":
        a.act_dim, sf = 3, safety()
    elif case == "agents":
        a.n_agents, a.rows = 6, 96
    return lib.flexenv_test_episodes_mlp(handle, None if case == "actor" else C.byref(a), steps, summed,
                                         None if case == "mlp" else C.byref(mlp), C.byref(sf) if sf is not None else None,
                                         None if case == "out" else C.byref(out), None)


@pytest.fixture(scope="module")
def blank_handle():
    """Zeroed memory where a handle would be (no handle can exist on a machine without a device: flexenv_create needs one).
    The refusals below come before the handle is followed; a call with nothing wrong follows it, finds a feeder the
    tiles do not hold (epw 0) and answers FLEXNET_EUNSUPPORTED, still before any HIP call — which is what shows that each
    refusal is owed to the one thing wrong in its case, not to the handle."""
    buf = (C.c_char * (64 << 20))()
    return buf, C.cast(buf, C.c_void_p)


@pytest.mark.parametrize("case", CASES)
def test_refusals_come_before_any_hip_call(lib, blank_handle, case):
    from safe_marl_amd import _lib
    assert _call(lib, None, blank_handle[1]) == _lib.FLEXNET_EUNSUPPORTED
    assert _call(lib, case, blank_handle[1]) == FLEX_EINVAL
    assert _call(lib, case, None) == FLEX_EINVAL


def test_null_handle_is_refused(lib):
    assert _call(lib, None, None) == FLEX_EINVAL


def test_new_kernels_resource_usage_and_the_existing_ones():
    """Three new instantiations under a namespace of their own; the three of flexenv_test_episodes keep their prefix to
    themselves.  The new ones stay inside the footprint that gives two wavefronts per SIMD, with no more scratch than the
    largest of the old three as this very build reports them."""
    from safe_marl_amd import build
    build.build()
    new = build.kernel_resources("test_mlp::flex_test_episodes_kernel<")
    old = build.kernel_resources("flex_test_episodes_kernel")
    assert sorted(v["name"] for v in new.values()) == [f"test_mlp::flex_test_episodes_kernel<{m}>" for m in range(3)]
    assert sorted(v["name"] for v in old.values()) == [f"flex_test_episodes_kernel<{m}>" for m in range(3)]
    for v in list(new.values()) + list(old.values()):
        print(f"{v['name']}: {v['vgprs']} VGPRs + {v['agprs']} AGPRs, {v['sgprs']} SGPRs, LDS {v['lds_bytes_per_block']} B, "
              f"{v['waves_per_simd']} waves/SIMD, scratch {v['scratch_bytes_per_lane']} B/lane")
    cap = max(v["scratch_bytes_per_lane"] for v in old.values())
    for v in new.values():
        assert v["vgprs"] <= 256 and v["agprs"] == 0 and v["lds_bytes_per_block"] == 153648 and v["waves_per_simd"] == 2, v
        assert v["scratch_bytes_per_lane"] <= cap, (v, cap)


def _model(alg="maddpg", n=5, **over):
    import torch
    from train_maddpg import DEFAULT_ALG_ARGS, PPO_ALG_ARGS
    from safe_marl_amd import learner
    from safe_marl_amd.util import convert
    d = dict(DEFAULT_ALG_ARGS)
    if alg == "ippo":
        d.update(PPO_ALG_ARGS)
    d.update(alg=alg, agent_num=n, obs_size=144, state_size=110, action_dim=4, cuda=False, v_min=0.9, v_max=1.1, agent_type="mlp")
    d.update(over)
    torch.manual_seed(0)
    cls = {"maddpg": learner.MADDPG, "matd3": learner.MATD3, "ippo": learner.IPPO, "safemaddpg": learner.SAFEMADDPG}[alg]
    if alg == "safemaddpg":
        z = torch.zeros(n, dtype=torch.float64)
        return cls(convert(d), None, predictor=(z, z, z))
    return cls(convert(d))


class _NoEnv:
    """Stands where an environment would: the refusal comes before anything of it but these attributes is read."""
    episode_limit = 96

    class obs:
        is_cuda = False


def test_eligibility_with_the_switch_on(monkeypatch):
    from safe_marl_amd.learner import one_launch_declines
    from safe_marl_amd.nets import MLPAgent, MLPAgentGaussian
    monkeypatch.setenv(SWITCH, "1")
    for alg in ("maddpg", "matd3", "ippo", "safemaddpg"):
        m = _model(alg)
        assert type(m.policy_dicts[0]) is MLPAgent
        assert one_launch_declines(m) is None, alg
    g = _model(gaussian_policy=True)
    assert type(g.policy_dicts[0]) is MLPAgentGaussian and one_launch_declines(g) is None
    # every other condition is what it is for the RNN agent
    assert "shared_params" in one_launch_declines(_model(shared_params=False))
    assert "7 agents" in one_launch_declines(_model(n=7))
    assert "action_enforcebound" in one_launch_declines(_model(action_enforcebound=False))
    safe = _model("safemaddpg")
    safe.intended_actions = True
    assert "intended_actions" in one_launch_declines(safe)
    assert "hid_size 32" in one_launch_declines(_model(hid_size=32))
    assert "hid_activation tanh" in one_launch_declines(_model(hid_activation="tanh"))
    # admitted, the call gets past the eligibility decision: what stops it here is the machine, not the agent type
    with pytest.raises(ValueError, match="not on a GPU"):
        _model().test_episodes(_NoEnv(), one_launch=True)
    assert one_launch_declines(_model(agent_type="rnn")) is None


@pytest.mark.parametrize("value", [None, "0"])
def test_eligibility_with_the_switch_off(value, monkeypatch):
    """Unset or 0: today's answer.  The switch is read at every call, not at import: the same model changes its answer."""
    from safe_marl_amd.learner import one_launch_declines
    if value is None:
        monkeypatch.delenv(SWITCH, raising=False)
    else:
        monkeypatch.setenv(SWITCH, value)
    m = _model()
    why = one_launch_declines(m)
    assert "agent_type mlp" in why and why.startswith("agent_type mlp: the launch holds the RNN actor's tiles")
    with pytest.raises(ValueError, match="agent_type mlp"):
        m.test_episodes(_NoEnv(), one_launch=True)
    assert "agent_type mlp" in one_launch_declines(_model(gaussian_policy=True))
    assert one_launch_declines(_model(agent_type="rnn")) is None
    monkeypatch.setenv(SWITCH, "1")
    assert one_launch_declines(m) is None
    monkeypatch.setenv(SWITCH, "0")
    assert "agent_type mlp" in one_launch_declines(m)


def test_builder_refuses_an_agent_outside_the_launch_before_it_reads_a_tensor():
    """nets.mlp_test_actor_args asks mlp_burst_declines first: an RNN agent, and an MLP agent whose parameters are not on a
    device, are refused with that function's reason although no tensor was handed in."""
    from safe_marl_amd import nets
    for agent, reason in ((_model(agent_type="rnn").policy_dicts[0], "a RNNAgent"), (_model().policy_dicts[0], nets.NOT_FP32_DEVICE)):
        assert nets.mlp_burst_declines(agent, 5, 144, True) == reason
        with pytest.raises(RuntimeError, match="does not cover this agent: " + reason):
            nets.mlp_test_actor_args(agent, 16, 5, 144, True, None, None, None, None, 0.0, 1.0)


def test_example_and_tools_parse_their_arguments():
    for script, words in ((os.path.join("examples", "evaluate_policy.py"), ("--agent-type", "--mlp-launch", "--alg", "--days")),
                          (os.path.join("tools", "learning_curve.py"), ("--one-launch", SWITCH)),
                          (os.path.join("tools", "mlp_test_episodes_bench.py"), ("--envs", "--runs", "--out"))):
        out = subprocess.run([sys.executable, os.path.join(ROOT, script), "--help"], capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stderr
        for w in words:
            assert w in out.stdout, (script, w)
