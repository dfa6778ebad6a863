"""The per-agent MLP actors (csrc/actor_mlp.hip's per-agent form), the per-agent log-std heads (csrc/gauss.hip) and the per-agent RNN
backward's d_hn variant (csrc/actor_unshared.hip) on the host side, no GPU: the binding against include/flexnet.h, the argument
checks that run before any device work, the kernels' resources as compiled, and the CPU dispatch."""
import ctypes as C
import os

import pytest
import torch as th

from .golden_io import golden_args, golden_model, golden_vectors
from .test_gaussian_cpu import gauss_state_dict
from .test_unshared_agents_cpu import DIR, FAMILIES, agents_batch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1                                                           # include/flexnet.h: FLEXNET_EINVAL
NEW = ("flexnet_actor_mlp_unshared_forward", "flexnet_actor_mlp_unshared_backward", "flexnet_gauss_head_unshared_forward",
       "flexnet_gauss_head_unshared_backward")


def _aligned_scratch():
    buf = (C.c_float * 256)()
    p = C.cast(buf, C.c_void_p).value
    return buf, p + (-p) % 16


def test_binding_of_the_new_entry_points():
    from safe_marl_amd import _lib, build
    build.build()
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "flexnet.h")).read()
    assert "#define FLEXNET_ACTOR_MLP_UNSHARED_WS_FLOATS (FLEXNET_MAX_AGENTS * 128 * 320)" in hdr
    assert _lib.FLEXNET_ACTOR_MLP_UNSHARED_WS_FLOATS == 8 * 128 * 320
    for name in NEW:
        assert name in _lib.SYMBOLS and hasattr(lib, name) and len(getattr(lib, name).argtypes) == 2
        assert f"int {name}(const " in hdr
    assert "flexnet_actor_unshared_backward_hn" in _lib.SYMBOLS and len(lib.flexnet_actor_unshared_backward_hn.argtypes) == 3
    # the header's fields: 6 int32 + float + int32, a pointer, eight tables of FLEXNET_MAX_AGENTS pointers, four pointers
    assert C.sizeof(_lib.FlexActorMlpUnsharedArgs) == 8 * 4 + 8 + 8 * 8 * 8 + 4 * 8
    # ... five pointers, three tables, eight pointers and the workspace length
    assert C.sizeof(_lib.FlexActorMlpUnsharedBwdArgs) == 8 * 4 + 5 * 8 + 3 * 8 * 8 + 8 * 8 + 8
    # int64 + 4 int32 + 2 float, a pointer, two tables, five pointers
    assert C.sizeof(_lib.FlexGaussHeadUnsharedArgs) == 8 + 4 * 4 + 2 * 4 + 8 + 2 * 8 * 8 + 5 * 8
    for st, fields in ((_lib.FlexActorMlpUnsharedArgs, ("fc1_w", "fc1_b", "ln_w", "ln_b", "fc2_w", "fc2_b", "fc3_w", "fc3_b")),
                       (_lib.FlexActorMlpUnsharedBwdArgs, ("ln_w", "fc2_w", "fc3_w")), (_lib.FlexGaussHeadUnsharedArgs, ("w", "b"))):
        for f in fields:
            assert len(getattr(st(), f)) == _lib.FLEXNET_MAX_AGENTS
            assert f"{f}[FLEXNET_MAX_AGENTS];" in hdr.split("} " + st.__name__ + ";")[0].rsplit("typedef struct {", 1)[1]


def _forward_args(p, rows=9, n=3, obs_dim=30, act_dim=4):
    from safe_marl_amd import _lib
    a = _lib.FlexActorMlpUnsharedArgs()
    a.rows, a.n_agents, a.obs_dim, a.act_dim, a.hid = rows, n, obs_dim, act_dim, 64
    for k in ("obs", "means", "h"):
        setattr(a, k, p)
    for k in ("fc1_w", "fc1_b", "fc2_w", "fc2_b", "fc3_w", "fc3_b"):
        for i in range(min(n, 8)):
            getattr(a, k)[i] = p
    return a


def _backward_args(p, rows=9, n=3, obs_dim=30, act_dim=4):
    from safe_marl_amd import _lib
    g = _lib.FlexActorMlpUnsharedBwdArgs()
    g.rows, g.n_agents, g.obs_dim, g.act_dim, g.hid = rows, n, obs_dim, act_dim, 64
    for k in ("d_means", "z1", "x", "h", "dz1", "dz2", "d_fc1_b", "d_fc2_b", "d_fc3_b", "workspace"):
        setattr(g, k, p)
    for k in ("fc2_w", "fc3_w"):
        for i in range(min(n, 8)):
            getattr(g, k)[i] = p
    g.workspace_floats = _lib.FLEXNET_ACTOR_MLP_UNSHARED_WS_FLOATS
    return g


def _head_args(p, rows=9, n=3, act_dim=4):
    from safe_marl_amd import _lib
    a = _lib.FlexGaussHeadUnsharedArgs()
    a.rows, a.n_agents, a.act_dim, a.hid = rows, n, act_dim, 64
    a.log_std_min, a.log_std_max = 0.0, 0.5
    for k in ("h", "log_std", "t", "d_log_std", "d_u", "d_h"):
        setattr(a, k, p)
    for i in range(min(n, 8)):
        a.w[i], a.b[i] = p, p
    return a


def test_actor_argument_checks_run_before_any_device_work():
    """Every call here is refused by the checks: nothing is launched (this machine may have no device at all)."""
    from safe_marl_amd import _lib, build
    build.build()
    lib = _lib.load()
    fwd = lambda a: lib.flexnet_actor_mlp_unshared_forward(C.byref(a), None)
    bwd = lambda g: lib.flexnet_actor_mlp_unshared_backward(C.byref(g), None)
    assert lib.flexnet_actor_mlp_unshared_forward(None, None) == EINVAL
    assert lib.flexnet_actor_mlp_unshared_backward(None, None) == EINVAL
    keep, p = _aligned_scratch()
    assert fwd(_forward_args(None)) == EINVAL                         # null tensors
    assert bwd(_backward_args(None)) == EINVAL
    a = _forward_args(p)
    a.fc2_w[2] = None
    assert fwd(a) == EINVAL                                           # a hole in a parameter table
    g = _backward_args(p)
    g.fc3_w[1] = None
    assert bwd(g) == EINVAL
    assert fwd(_forward_args(p, rows=10)) == EINVAL                   # rows % n_agents != 0
    assert bwd(_backward_args(p, rows=10)) == EINVAL
    a = _forward_args(p)
    a.save_x = p
    assert fwd(a) == EINVAL                                           # one save without the other
    a.save_x, a.save_z1 = None, p
    assert fwd(a) == EINVAL
    a = _forward_args(p)
    a.layernorm = 1
    for i in range(3):
        a.ln_w[i] = p
    assert fwd(a) == EINVAL                                           # LayerNorm without its pair
    g = _backward_args(p)
    g.layernorm, g.d_ln_w = 1, p
    for i in range(3):
        g.ln_w[i] = p
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
    g = _backward_args(p)
    g.hid = 32
    assert bwd(g) == _lib.FLEXNET_EUNSUPPORTED
    a = _forward_args(p)
    a.h = p + 4
    assert fwd(a) == _lib.FLEXNET_EUNSUPPORTED                        # a misaligned [rows, 64] tensor
    g = _backward_args(p)
    g.dz2 = p + 4
    assert bwd(g) == _lib.FLEXNET_EUNSUPPORTED
    g = _backward_args(p)
    g.d_h = p + 4
    assert bwd(g) == _lib.FLEXNET_EUNSUPPORTED
    del keep


def test_head_and_hn_argument_checks_run_before_any_device_work():
    from safe_marl_amd import _lib, build
    build.build()
    lib = _lib.load()
    fwd = lambda a: lib.flexnet_gauss_head_unshared_forward(C.byref(a), None)
    bwd = lambda a: lib.flexnet_gauss_head_unshared_backward(C.byref(a), None)
    assert lib.flexnet_gauss_head_unshared_forward(None, None) == EINVAL
    assert lib.flexnet_gauss_head_unshared_backward(None, None) == EINVAL
    keep, p = _aligned_scratch()
    assert fwd(_head_args(None)) == EINVAL and bwd(_head_args(None)) == EINVAL
    assert fwd(_head_args(p, rows=10)) == EINVAL and bwd(_head_args(p, rows=10)) == EINVAL      # rows % n_agents != 0
    a = _head_args(p)
    a.w[1] = None
    assert fwd(a) == EINVAL and bwd(a) == EINVAL                      # a hole in the weight table
    a = _head_args(p)
    a.b[1] = None
    assert fwd(a) == EINVAL                                           # biases: all or none
    a = _head_args(p)
    a.d_u = a.d_h = None
    assert bwd(a) == EINVAL                                           # nothing to write
    for over in (dict(rows=9, n=9), dict(act_dim=9), dict(rows=(1 << 30) + 2, n=2)):
        assert fwd(_head_args(p, **over)) == _lib.FLEXNET_EUNSUPPORTED, over
        assert bwd(_head_args(p, **over)) == _lib.FLEXNET_EUNSUPPORTED, over
    a = _head_args(p)
    a.hid = 32
    assert fwd(a) == _lib.FLEXNET_EUNSUPPORTED and bwd(a) == _lib.FLEXNET_EUNSUPPORTED
    a = _head_args(p)
    a.h = p + 4
    assert fwd(a) == _lib.FLEXNET_EUNSUPPORTED
    a = _head_args(p)
    a.d_h = p + 4
    assert bwd(a) == _lib.FLEXNET_EUNSUPPORTED
    # the RNN backward's variant: the same checks as flexnet_actor_unshared_backward, and d_hn itself
    g = _lib.FlexActorUnsharedBwdArgs()
    g.rows, g.n_agents, g.obs_dim, g.act_dim = 9, 3, 30, 4
    hn = lambda d: lib.flexnet_actor_unshared_backward_hn(C.byref(g), d, None)
    assert lib.flexnet_actor_unshared_backward_hn(None, p, None) == EINVAL
    assert hn(None) == EINVAL and hn(p) == EINVAL                     # no d_hn; null tensors
    for k in ("d_means", "r", "z", "n", "hn", "h_prev", "z1", "x", "d_gi", "d_gh", "dz", "d_fc1_b", "workspace"):
        setattr(g, k, p)
    for k in ("fc1_w", "fc1_b", "w_ih", "fc2_w"):
        for i in range(3):
            getattr(g, k)[i] = p
    g.workspace_floats = _lib.FLEXNET_ACTOR_UNSHARED_WS_FLOATS
    assert hn(p + 4) == _lib.FLEXNET_EUNSUPPORTED                     # a misaligned d_hn
    g.workspace_floats = 3 * 192 - 1
    assert hn(p) == EINVAL                                            # a short workspace
    del keep


def test_the_new_kernels_do_not_spill():
    from safe_marl_amd import build
    build.build()
    res = {}
    for prefix in ("mlp_unshared_actor", "gauss_head_unshared", "actor_hn_unshared"):
        res.update(build.kernel_resources(prefix))
    names = sorted(v["name"] for v in res.values())
    assert names == ["actor_hn_unshared_backward_kernel", "gauss_head_unshared_backward_kernel", "gauss_head_unshared_forward_kernel",
                     "mlp_unshared_actor_backward_kernel", "mlp_unshared_actor_forward_kernel", "mlp_unshared_actor_reduce_kernel"], names
    for v in res.values():
        print(f"{v['name']}: {v['vgprs']} VGPRs + {v['agprs']} AGPRs, {v['sgprs']} SGPRs, LDS {v['lds_bytes_per_block']} B, "
              f"{v['waves_per_simd']} waves/SIMD, scratch {v['scratch_bytes_per_lane']} B/lane")
        assert v["scratch_bytes_per_lane"] == 0 and v["vgpr_spills"] == 0 and v["sgpr_spills"] == 0, v
    # the d_hn variant is the old kernel's body: the same LDS, and the old kernel under its old name
    old = list(build.kernel_resources("actor_unshared_backward_kernel").values())
    hn = [v for v in res.values() if v["name"] == "actor_hn_unshared_backward_kernel"]
    assert len(old) == 1 and len(hn) == 1 and old[0]["lds_bytes_per_block"] == hn[0]["lds_bytes_per_block"]


@pytest.mark.parametrize("family,cls,agent_type,gauss", FAMILIES)
def test_cpu_models_keep_the_loop(monkeypatch, family, cls, agent_type, gauss):
    """The launches are for GPU tensors: on the CPU nothing is launched, nothing declines and nothing is counted."""
    from safe_marl_amd import _lib
    from safe_marl_amd.nets import actor_mlp_unshared_supported, gauss_head_unshared_supported
    from safe_marl_amd.util import FALLBACKS
    launched = []
    monkeypatch.setattr(_lib, "try_launch", lambda name, *a, **k: launched.append(name) or True)
    before = dict(FALLBACKS)
    model = golden_model(cls, golden_args(DIR + family), gauss_state_dict(DIR + family))
    batch = agents_batch(cls, gold=golden_vectors(DIR + family))
    agents = list(model.policy_dicts)
    assert not actor_mlp_unshared_supported(agents, batch.state, model.args.agent_id)
    with th.no_grad():
        means, log_stds, hid = model.policy(batch.state, last_hid=batch.last_hid)
        obs = model.with_ids(batch.state)
        ref = [g(obs[:, i], batch.last_hid[:, i]) for i, g in enumerate(agents)]
    assert th.equal(means, th.stack([r[0] for r in ref], 1)) and th.equal(hid, th.stack([r[2] for r in ref], 1))
    if gauss:
        assert th.equal(log_stds, th.stack([r[1] for r in ref], 1))
        assert not gauss_head_unshared_supported(agents, hid.reshape(-1, 64))
    out = model.policy(batch.state, last_hid=batch.last_hid)
    assert out[0].requires_grad and out[1].requires_grad == gauss
    assert not launched and dict(FALLBACKS) == before
