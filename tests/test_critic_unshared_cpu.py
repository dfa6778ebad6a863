"""The per-agent critics of ``shared_params: False`` (csrc/critic_unshared.hip) and the batched weight gradient
(flexnet_wgrad_batched, csrc/wgrad.hip) without a GPU: the binding, the argument checks that run before any device work, the
kernels' resources, and what stays as it was — CPU models take the per-agent loop, unshared models do not declare graph-safe
updates."""
import ctypes as C
import os

import torch as th

from .golden_io import golden_args, golden_model, golden_vectors
from .test_gaussian_cpu import gauss_state_dict
from .test_unshared_cpu import unshared_batch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1                                                           # include/flexnet.h: FLEXNET_EINVAL


def _aligned_pointer(buf):
    p = C.cast(buf, C.c_void_p).value
    return p + (-p) % 16


def test_binding_of_the_critic_entry_points():
    from safe_marl_amd import _lib, build
    build.build()
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "flexnet.h")).read()
    assert "#define FLEXNET_CRITIC_UNSHARED_WS_FLOATS (FLEXNET_MAX_AGENTS * 128 * 384)" in hdr
    assert "#define FLEXNET_WGRAD_MAX_BATCH (4 * FLEXNET_MAX_AGENTS)" in hdr
    assert _lib.FLEXNET_CRITIC_UNSHARED_WS_FLOATS == 8 * 128 * 384
    assert _lib.FLEXNET_WGRAD_MAX_BATCH == 32 >= 4 * _lib.FLEXNET_MAX_AGENTS
    assert (_lib.FLEXNET_MAX_AGENTS, _lib.FLEXNET_MAX_OBS, _lib.FLEXNET_MAX_ACT) == (8, 144, 8)
    assert C.sizeof(_lib.FlexCriticUnsharedArgs) == 8 * 4 + 2 * 8 + 4 * 8 + 8 * 8 * 8 + 3 * 8
    assert C.sizeof(_lib.FlexCriticUnsharedBwdArgs) == 8 * 4 + 3 * 8 + 5 * 8 * 8 + 9 * 8 + 4 * 4 + 2 * 8
    for name in ("flexnet_critic_unshared_forward", "flexnet_critic_unshared_backward"):
        assert name in _lib.SYMBOLS and len(getattr(lib, name).argtypes) == 2
    assert "flexnet_wgrad_batched" in _lib.SYMBOLS and len(lib.flexnet_wgrad_batched.argtypes) == 3

    # forward: argument checks that run before any device work
    assert lib.flexnet_critic_unshared_forward(None, None) == EINVAL
    buf = (C.c_float * 64)()
    p = _aligned_pointer(buf)
    a = _lib.FlexCriticUnsharedArgs()
    a.rows, a.n_agents, a.w1, a.w2 = 9, 3, 30, 4
    assert lib.flexnet_critic_unshared_forward(C.byref(a), None) == EINVAL          # null tensors
    a.x1 = a.q = p
    assert lib.flexnet_critic_unshared_forward(C.byref(a), None) == EINVAL          # a second block without its tensor
    a.x2 = p
    assert lib.flexnet_critic_unshared_forward(C.byref(a), None) == EINVAL          # empty parameter tables
    for name in ("fc1_w", "fc1_b", "fc2_w", "fc2_b", "fc3_w", "fc3_b"):
        for i in range(3):
            getattr(a, name)[i] = p
    a.rows = 10
    assert lib.flexnet_critic_unshared_forward(C.byref(a), None) == EINVAL          # rows % n_agents != 0
    a.rows, a.w1 = 9, 0
    assert lib.flexnet_critic_unshared_forward(C.byref(a), None) == EINVAL          # no first block
    a.w1 = 8 * 144 + 1
    assert lib.flexnet_critic_unshared_forward(C.byref(a), None) == _lib.FLEXNET_EUNSUPPORTED
    a.w1, a.w2 = 30, 8 * 8 + 1
    assert lib.flexnet_critic_unshared_forward(C.byref(a), None) == _lib.FLEXNET_EUNSUPPORTED
    a.w2, a.n_agents = 4, 9
    assert lib.flexnet_critic_unshared_forward(C.byref(a), None) == _lib.FLEXNET_EUNSUPPORTED
    a.n_agents, a.save_x = 3, p
    assert lib.flexnet_critic_unshared_forward(C.byref(a), None) == EINVAL          # the saves: both or none
    a.save_x, a.layernorm = None, 1
    assert lib.flexnet_critic_unshared_forward(C.byref(a), None) == EINVAL          # LayerNorm without its pair
    a.layernorm = 0
    for i in range(3):
        a.fc2_w[i] = p + 4
    assert lib.flexnet_critic_unshared_forward(C.byref(a), None) == _lib.FLEXNET_EUNSUPPORTED   # fc2_w not 16-byte aligned
    a.rows = 0
    for i in range(3):
        a.fc2_w[i] = p
    assert lib.flexnet_critic_unshared_forward(C.byref(a), None) == 0               # an empty batch: nothing to launch

    # backward
    assert lib.flexnet_critic_unshared_backward(None, None) == EINVAL
    g = _lib.FlexCriticUnsharedBwdArgs()
    g.rows, g.n_agents, g.w1, g.w2 = 9, 3, 30, 4
    assert lib.flexnet_critic_unshared_backward(C.byref(g), None) == EINVAL         # null tensors
    g.dq = g.z1 = g.x = g.dz1 = p
    g.param_grads = 1
    assert lib.flexnet_critic_unshared_backward(C.byref(g), None) == EINVAL         # parameter gradients without their buffers
    g.param_grads = 0
    assert lib.flexnet_critic_unshared_backward(C.byref(g), None) == EINVAL         # empty parameter tables
    for name in ("fc1_w", "fc2_w", "fc2_b", "fc3_w"):
        for i in range(3):
            getattr(g, name)[i] = p
    g.d_x2_own, g.own_first, g.own_step, g.own_w = p, 0, 2, 2
    assert lib.flexnet_critic_unshared_backward(C.byref(g), None) == EINVAL         # the own block of agent 2 ends past x2
    g.own_step, g.own_w, g.w2 = 0, 9, 12
    assert lib.flexnet_critic_unshared_backward(C.byref(g), None) == _lib.FLEXNET_EUNSUPPORTED
    g.own_w, g.n_agents = 4, 9
    assert lib.flexnet_critic_unshared_backward(C.byref(g), None) == _lib.FLEXNET_EUNSUPPORTED
    g.n_agents, g.rows = 3, 0
    assert lib.flexnet_critic_unshared_backward(C.byref(g), None) == 0


def test_argument_checks_of_the_batched_weight_gradient():
    from safe_marl_amd import _lib, build
    build.build()
    lib = _lib.load()
    assert C.sizeof(_lib.FlexWgradArgs) == 4 * 8 + 4 * 4 + 7 * 8 + 8 + 2 * 4 + 8
    buf = (C.c_float * 64)()
    p = _aligned_pointer(buf)
    slice_floats = _lib.FLEXNET_WGRAD_CS_FLOATS + 2 * 2 * 1024
    table = (_lib.FlexWgradArgs * 3)()
    for i, a in enumerate(table):
        a.k, a.m, a.n, a.lda, a.ldb = 100, 64, 64, 64, 64
        a.a = a.b = a.c = p
        a.workspace, a.workspace_floats = p + 4 * slice_floats * i, slice_floats       # (never dereferenced: every call is refused)
    assert lib.flexnet_wgrad_batched(None, 1, None) == EINVAL
    assert lib.flexnet_wgrad_batched(table, 0, None) == EINVAL
    assert lib.flexnet_wgrad_batched(table, _lib.FLEXNET_WGRAD_MAX_BATCH + 1, None) == EINVAL
    table[2].workspace = table[0].workspace + 4 * (slice_floats - 1)
    assert lib.flexnet_wgrad_batched(table, 3, None) == EINVAL                         # overlapping workspace slices
    table[2].workspace = table[0].workspace + 4 * 2 * slice_floats
    table[1].b2, table[1].c2, table[1].n2, table[1].ldb2 = p, p, 8, 8
    assert lib.flexnet_wgrad_batched(table, 3, None) == _lib.FLEXNET_EUNSUPPORTED      # no second input block here
    table[1].b2, table[1].c2, table[1].n2, table[1].ldb2 = None, None, 0, 0
    table[1].b_row_cell = p
    assert lib.flexnet_wgrad_batched(table, 3, None) == _lib.FLEXNET_EUNSUPPORTED      # no row cell here
    table[1].b_row_cell = None
    table[1].m, table[1].lda = 193, 193
    assert lib.flexnet_wgrad_batched(table, 3, None) == _lib.FLEXNET_EUNSUPPORTED      # flexnet_wgrad's own limit
    table[1].m, table[1].lda = 64, 32
    assert lib.flexnet_wgrad_batched(table, 3, None) == EINVAL                         # a pitch below the width
    table[1].lda = 64
    table[1].workspace_floats = _lib.FLEXNET_WGRAD_CS_FLOATS + 100
    assert lib.flexnet_wgrad_batched(table, 3, None) == EINVAL                         # a slice below one register image


def test_the_new_kernels_do_not_spill():
    from safe_marl_amd import build
    build.build()
    res = build.kernel_resources("critic_unshared")
    names = sorted(v["name"] for v in res.values())
    assert names == ["critic_unshared_backward_kernel<false>", "critic_unshared_backward_kernel<true>",
                     "critic_unshared_forward_kernel", "critic_unshared_reduce_kernel"], names
    batched = build.kernel_resources("wgrad_batched")
    assert len(batched) == 16, sorted(v["name"] for v in batched.values())            # eight shape classes, two stages
    for v in list(res.values()) + list(batched.values()):
        print(f"{v['name']}: {v['vgprs']} VGPRs + {v['agprs']} AGPRs, {v['sgprs']} SGPRs, LDS {v['lds_bytes_per_block']} B, "
              f"{v['waves_per_simd']} waves/SIMD, scratch {v['scratch_bytes_per_lane']} B/lane")
        assert v["scratch_bytes_per_lane"] == 0 and v["vgpr_spills"] == 0 and v["sgpr_spills"] == 0, v


def test_cpu_models_keep_the_loop():
    """The launches are for GPU tensors: on the CPU nothing declines and nothing is counted."""
    from safe_marl_amd.util import FALLBACKS
    before = FALLBACKS.get("critic_unshared", 0)
    for prefix, cls in (("unshared_maddpg", "MADDPG"), ("unshared_ippo", "IPPO")):
        model = golden_model(cls, golden_args(prefix), gauss_state_dict(prefix))
        assert model.unshared_critic_kernel and not model.args.shared_params
        batch = unshared_batch(prefix, gold=golden_vectors(prefix))
        b, n = batch.state.shape[0], model.n_
        act = th.zeros(b, n, model.act_dim)
        assert model.unshared_values(batch.state, act, cls == "MADDPG") is None
        with th.no_grad():
            v0 = model.value(batch.state, act)
        v1 = model.value(batch.state, act.requires_grad_())
        assert v0.shape == v1.shape == (b, n, 1) and th.equal(v0, v1.detach()) and v1.requires_grad
    assert FALLBACKS.get("critic_unshared", 0) == before


def test_which_algorithms_take_the_kernel():
    import safe_marl_amd.learner as L
    assert all(getattr(L, c).unshared_critic_kernel for c in ("MADDPG", "SAFEMADDPG", "IDDPG", "IPPO", "MAPPO"))
    assert not any(getattr(L, c).unshared_critic_kernel for c in ("FACMADDPG", "SQDDPG", "COMA", "MATD3"))


def test_unshared_models_still_do_not_declare_graph_safe_updates():
    """Nothing of the new path is captured into a HIP graph: the per-agent models' sub-updates stay eager."""
    import safe_marl_amd.learner as L
    shared = golden_args("learner3")
    for cls in (L.MADDPG, L.IDDPG):
        assert cls(shared).graph_safe_updates is True
        assert cls(shared._replace(shared_params=False)).graph_safe_updates is False
    assert L.IPPO(golden_args("unshared_ippo")).graph_safe_updates is False
