"""The MLP actor's fused pair (csrc/actor_mlp.hip) on the host side, no GPU: the binding against include/flexnet.h, the
argument checks that run before any device work, the kernels' resources as compiled, and the CPU dispatch."""
import ctypes as C
import os

import torch as th

from .golden_io import golden_args, golden_batch, golden_model
from .test_gaussian_cpu import gauss_state_dict

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1                                                           # include/flexnet.h: FLEXNET_EINVAL


def _aligned_scratch():
    buf = (C.c_float * 256)()
    p = C.cast(buf, C.c_void_p).value
    return buf, p + (-p) % 16


def test_binding_of_the_actor_mlp_entry_points():
    from safe_marl_amd import _lib, build
    build.build()
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "flexnet.h")).read()
    assert "#define FLEXNET_ACTOR_MLP_WS_FLOATS (FLEXNET_MAX_AGENTS * 128 * 320)" in hdr
    assert _lib.FLEXNET_ACTOR_MLP_WS_FLOATS == 8 * 128 * 320
    # the header's fields: 6 int32 + float + int32, then the pointers (and the workspace length)
    assert C.sizeof(_lib.FlexActorMlpArgs) == 8 * 4 + 9 * 8 + 4 * 8
    assert C.sizeof(_lib.FlexActorMlpBwdArgs) == 8 * 4 + 8 * 8 + 9 * 8 + 8
    for name in ("flexnet_actor_mlp_forward", "flexnet_actor_mlp_backward"):
        assert name in _lib.SYMBOLS and len(getattr(lib, name).argtypes) == 2


def _forward_args(p, rows=9, n=3, obs_dim=30, act_dim=4):
    from safe_marl_amd import _lib
    a = _lib.FlexActorMlpArgs()
    a.rows, a.n_agents, a.obs_dim, a.act_dim, a.hid = rows, n, obs_dim, act_dim, 64
    for k in ("obs", "fc1_w", "fc1_b", "fc2_w", "fc2_b", "fc3_w", "fc3_b", "means", "h"):
        setattr(a, k, p)
    return a


def _backward_args(p, rows=9, n=3, obs_dim=30, act_dim=4):
    from safe_marl_amd import _lib
    g = _lib.FlexActorMlpBwdArgs()
    g.rows, g.n_agents, g.obs_dim, g.act_dim, g.hid = rows, n, obs_dim, act_dim, 64
    for k in ("d_means", "z1", "x", "h", "fc2_w", "fc3_w", "dz1", "dz2", "d_fc1_b", "d_fc2_b", "d_fc3_b", "d_dz1_agent", "workspace"):
        setattr(g, k, p)
    g.workspace_floats = _lib.FLEXNET_ACTOR_MLP_WS_FLOATS
    return g


def test_argument_checks_run_before_any_device_work():
    """Every call here is refused by the checks: nothing is launched (this machine may have no device at all)."""
    from safe_marl_amd import _lib, build
    build.build()
    lib = _lib.load()
    fwd = lambda a: lib.flexnet_actor_mlp_forward(C.byref(a), None)
    bwd = lambda g: lib.flexnet_actor_mlp_backward(C.byref(g), None)
    assert lib.flexnet_actor_mlp_forward(None, None) == EINVAL
    assert lib.flexnet_actor_mlp_backward(None, None) == EINVAL
    keep, p = _aligned_scratch()
    a = _forward_args(None)
    assert fwd(a) == EINVAL                                           # null tensors
    g = _backward_args(None)
    assert bwd(g) == EINVAL
    a = _forward_args(p, rows=10)
    assert fwd(a) == EINVAL                                           # rows % n_agents != 0
    g = _backward_args(p, rows=10)
    assert bwd(g) == EINVAL
    a = _forward_args(p)
    a.save_x = p
    assert fwd(a) == EINVAL                                           # one save without the other
    a.save_x, a.save_z1 = None, p
    assert fwd(a) == EINVAL
    a = _forward_args(p)
    a.layernorm, a.ln_w = 1, p
    assert fwd(a) == EINVAL                                           # LayerNorm without its pair
    g = _backward_args(p)
    g.layernorm, g.ln_w, g.d_ln_w = 1, p, p
    assert bwd(g) == EINVAL
    g = _backward_args(p)
    g.workspace_floats = 3 * 320 - 1                                  # 9 rows of 3 agents: one work-group per agent
    assert bwd(g) == EINVAL                                           # a short workspace
    for over in (dict(obs_dim=145), dict(rows=9, n=9), dict(act_dim=9)):
        assert fwd(_forward_args(p, **over)) == _lib.FLEXNET_EUNSUPPORTED, over
        assert bwd(_backward_args(p, **over)) == _lib.FLEXNET_EUNSUPPORTED, over
    a = _forward_args(p)
    a.hid = 32
    assert fwd(a) == _lib.FLEXNET_EUNSUPPORTED
    a = _forward_args(p)
    a.h = p + 4
    assert fwd(a) == _lib.FLEXNET_EUNSUPPORTED                        # a misaligned [rows, 64] tensor
    g = _backward_args(p)
    g.dz2 = p + 4
    assert bwd(g) == _lib.FLEXNET_EUNSUPPORTED
    del keep


def test_the_new_kernels_do_not_spill():
    from safe_marl_amd import build
    build.build()
    res = build.kernel_resources("actor_mlp")
    names = sorted(v["name"] for v in res.values())
    assert names == ["actor_mlp_backward_kernel", "actor_mlp_forward_kernel", "actor_mlp_reduce_kernel"], names
    for v in res.values():
        print(f"{v['name']}: {v['vgprs']} VGPRs + {v['agprs']} AGPRs, {v['sgprs']} SGPRs, LDS {v['lds_bytes_per_block']} B, "
              f"{v['waves_per_simd']} waves/SIMD, scratch {v['scratch_bytes_per_lane']} B/lane")
        assert v["scratch_bytes_per_lane"] == 0 and v["vgpr_spills"] == 0 and v["sgpr_spills"] == 0, v


def test_cpu_models_keep_the_composition(monkeypatch):
    """The launches are for GPU tensors: on the CPU nothing is launched, nothing declines and nothing is counted."""
    from safe_marl_amd import _lib
    from safe_marl_amd.nets import MLPAgent, actor_mlp_supported
    from safe_marl_amd.util import FALLBACKS
    launched = []
    monkeypatch.setattr(_lib, "try_launch", lambda name, *a, **k: launched.append(name) or True)
    before = dict(FALLBACKS)
    model = golden_model("MADDPG", golden_args("mlp_maddpg"), gauss_state_dict("mlp_maddpg"))
    assert type(model.policy_dicts[0]) is MLPAgent
    batch = golden_batch("mlp_maddpg")
    assert not actor_mlp_supported(model.policy_dicts[0], batch.state, model.n_, model.args.agent_id)
    with th.no_grad():
        means, _, hid = model.policy(batch.state, last_hid=batch.last_hid)
        ref = model.policy_dicts[0](model.with_ids(batch.state).reshape(means.shape[0] * model.n_, -1), None)
    assert th.equal(means.reshape(ref[0].shape), ref[0]) and th.equal(hid.reshape(ref[2].shape), ref[2])
    assert model.policy(batch.state, last_hid=batch.last_hid)[0].requires_grad
    assert not [k for k in launched if "actor_mlp" in k] and dict(FALLBACKS) == before
