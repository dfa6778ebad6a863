"""shared_params: False on CPU: golden vectors captured by importing the reference's MADDPG / IPPO with one RNNAgent and one
critic per agent (tests/golden/make_unshared_golden.py, three agents) — strict state_dict loads, ``policy()``, both losses,
every gradient, ``stat`` and the weights after one value and one policy step, with tests/test_mlp_agent_cpu.py's tolerances.
Then what the feature adds on the host side: the graph rule, the binding, the kernels' resources, the example's flag."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch as th

from .golden_io import StubEnv, golden_args, golden_batch, golden_model, golden_tensors, golden_vectors
from .test_gaussian_cpu import assert_grads, gauss_state_dict
from .test_mlp_agent_cpu import mlp_policy_loss

FAMILIES = [("unshared_maddpg", "MADDPG"), ("unshared_ippo", "IPPO")]
BATCH_FIELDS = {"unshared_maddpg": (), "unshared_ippo": ("action", "done", "last_step")}
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def unshared_batch(prefix, device="cpu", tile=1, gold=None):
    """The three-agent batch (learner3_batch.npz) with the fields the family's reference run replaced."""
    return golden_batch("learner3", device, tile, gold=gold, fields=BATCH_FIELDS[prefix])


@pytest.mark.parametrize("prefix,cls", FAMILIES)
def test_golden_parity(prefix, cls):
    import safe_marl_amd.learner as L
    from safe_marl_amd.nets import RNNAgent
    from safe_marl_amd.trainer import PGTrainer
    gold = golden_vectors(prefix)
    args = golden_args(prefix)
    n = args.agent_num
    assert args.agent_type == "rnn" and not args.shared_params and args.agent_id and n == 3 and not args.gaussian_policy
    model = golden_model(cls, args, gauss_state_dict(prefix))            # strict: the reference's names and shapes
    assert len(model.policy_dicts) == len(model.value_dicts) == n
    assert all(type(a) is RNNAgent and a.fc1.weight.shape == (64, args.obs_size + n) for a in model.policy_dicts)
    batch = unshared_batch(prefix, gold=gold)

    with th.no_grad():
        means, log_stds, hiddens = model.policy(batch.state, last_hid=batch.last_hid)
    assert log_stds.shape == means.shape == (32, n, 4)
    assert np.allclose(means.numpy(), gold["policy_means"], atol=2e-6)
    assert np.allclose(log_stds.numpy(), gold["policy_log_stds"], atol=2e-6)
    assert np.allclose(hiddens.numpy(), gold["policy_hiddens"], atol=2e-6)

    loss, pl, vl, means, log_stds = mlp_policy_loss(model, batch, args.entr)
    assert abs(pl.item() - float(gold["policy_loss"])) < 2e-6 * max(1.0, abs(float(gold["policy_loss"])))
    assert abs(vl.item() - float(gold["value_loss"])) < 1e-5 * max(1.0, abs(float(gold["value_loss"])))
    assert np.allclose(means.detach().numpy(), gold["means"], atol=2e-6)
    assert np.allclose(log_stds.detach().numpy(), gold["log_stds"], atol=2e-6)
    grads = th.autograd.grad(vl, list(model.value_dicts.parameters()), retain_graph=True)
    assert_grads(model.value_dicts.named_parameters(), grads, gold, "vgrad.")
    grads = th.autograd.grad(loss, list(model.policy_dicts.parameters()))
    assert_grads(model.policy_dicts.named_parameters(), grads, gold, "pgrad.")
    # the one-hot input: agent a's id block takes a gradient in its own column only, the bias gradient
    for a in range(n):
        ids = gold[f"pgrad.{a}.fc1.weight"][:, args.obs_size:]
        assert np.all(np.delete(ids, a, axis=1) == 0.0)
        assert np.allclose(ids[:, a], gold[f"pgrad.{a}.fc1.bias"], atol=1e-8, rtol=1e-6)

    # one value step, then one policy step through PGTrainer
    th.manual_seed(0)
    trainer = PGTrainer(args, getattr(L, cls), StubEnv(n), None)
    net = trainer.behaviour_net
    net.load_state_dict(gauss_state_dict(prefix))
    stat = {}
    trainer.value_transition_process(stat, batch)
    trainer.policy_transition_process(stat, batch)
    keys = {k[5:] for k in gold if k.startswith("stat.")}
    assert keys == set(stat) == {"mean_train_value_loss", "mean_train_value_grad_norm", "mean_train_policy_loss",
                                 "mean_train_policy_grad_norm", "mean_train_entropy"}
    for k in keys:
        assert abs(float(stat[k]) - gold["stat." + k]) < 1e-4 * max(1.0, abs(gold["stat." + k])), k
    after = gauss_state_dict(prefix, "state_dict_after_step")
    mine = net.state_dict()
    assert sorted(mine) == sorted(after)
    for k, ref in after.items():
        assert th.allclose(mine[k].float(), ref.float(), atol=3e-6, rtol=1e-5), k
    init = golden_tensors(f"{prefix}_state_dict.npz")
    for a in range(n):
        assert (mine[f"policy_dicts.{a}.fc2.weight"] - init[f"policy_dicts.{a}.fc2.weight"]).abs().max() > 0


def test_fixture_files_stay_below_the_largest_committed_one():
    g = os.path.join(ROOT, "tests", "golden")
    files = [f for f in os.listdir(g) if f.startswith("unshared_")]
    assert len(files) == 8
    assert all(os.path.getsize(os.path.join(g, f)) < os.path.getsize(os.path.join(g, "loop_golden.npz")) for f in files)


def test_unshared_models_do_not_declare_graph_safe_updates():
    """The per-agent critics' gradient path holds ATen reductions (util.GRAPH_DENYLIST): their sub-updates run eagerly."""
    import safe_marl_amd.learner as L
    assert L.MADDPG.graph_safe_updates is True and L.IDDPG.graph_safe_updates is True and L.MATD3.graph_safe_updates is True
    assert L.IPPO.graph_safe_updates is False
    shared = golden_args("learner3")
    assert shared.shared_params
    for cls in (L.MADDPG, L.IDDPG):
        assert cls(shared).graph_safe_updates is True
        assert cls(shared._replace(shared_params=False)).graph_safe_updates is False
    assert L.MATD3(shared).graph_safe_updates is True
    assert L.IPPO(golden_args("unshared_ippo")).graph_safe_updates is False


def test_binding_of_the_unshared_entry_points():
    from safe_marl_amd import _lib, build
    build.build()
    lib = _lib.load()
    EINVAL = -1                                                       # include/flexnet.h: FLEXNET_EINVAL
    hdr = open(os.path.join(ROOT, "include", "flexnet.h")).read()
    assert "#define FLEXNET_ACTOR_UNSHARED_WS_FLOATS (FLEXNET_MAX_AGENTS * 128 * 192)" in hdr
    assert _lib.FLEXNET_ACTOR_UNSHARED_WS_FLOATS == 8 * 128 * 192
    assert C.sizeof(_lib.FlexActorUnsharedArgs) == 8 * 4 + 2 * 8 + 10 * 8 * 8 + 8 * 8
    assert C.sizeof(_lib.FlexActorUnsharedBwdArgs) == 8 * 4 + 8 * 8 + 5 * 8 * 8 + 7 * 8 + 8
    for name in ("flexnet_actor_unshared_forward", "flexnet_actor_unshared_backward"):
        assert name in _lib.SYMBOLS and len(getattr(lib, name).argtypes) == 2
    # argument checks that run before any device work
    assert lib.flexnet_actor_unshared_forward(None, None) == EINVAL
    assert lib.flexnet_actor_unshared_backward(None, None) == EINVAL
    a = _lib.FlexActorUnsharedArgs()
    a.rows, a.n_agents, a.obs_dim, a.act_dim = 9, 3, 30, 4
    assert lib.flexnet_actor_unshared_forward(C.byref(a), None) == EINVAL            # null tensors
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p).value
    p -= p % 16
    a.obs = a.hidden_in = a.means = a.hidden_out = p
    assert lib.flexnet_actor_unshared_forward(C.byref(a), None) == EINVAL            # empty parameter tables
    for name in ("fc1_w", "fc1_b", "w_ih", "w_hh", "b_ih", "b_hh", "fc2_w", "fc2_b"):
        for i in range(3):
            getattr(a, name)[i] = p
    a.rows = 10
    assert lib.flexnet_actor_unshared_forward(C.byref(a), None) == EINVAL            # rows % n_agents != 0
    a.rows, a.obs_dim = 9, 145
    assert lib.flexnet_actor_unshared_forward(C.byref(a), None) == _lib.FLEXNET_EUNSUPPORTED
    a.obs_dim, a.n_agents = 30, 9
    assert lib.flexnet_actor_unshared_forward(C.byref(a), None) == _lib.FLEXNET_EUNSUPPORTED
    a.n_agents, a.act_dim = 3, 9
    assert lib.flexnet_actor_unshared_forward(C.byref(a), None) == _lib.FLEXNET_EUNSUPPORTED
    a.act_dim, a.save_x = 4, p
    assert lib.flexnet_actor_unshared_forward(C.byref(a), None) == EINVAL            # the saves: all six or none
    a.save_x, a.layernorm = None, 1
    assert lib.flexnet_actor_unshared_forward(C.byref(a), None) == EINVAL            # LayerNorm without its pair
    g = _lib.FlexActorUnsharedBwdArgs()
    g.rows, g.n_agents, g.obs_dim, g.act_dim = 9, 3, 30, 4
    assert lib.flexnet_actor_unshared_backward(C.byref(g), None) == EINVAL


def test_the_new_kernels_do_not_spill():
    from safe_marl_amd import build
    build.build()
    res = build.kernel_resources("actor_unshared")
    names = sorted(v["name"] for v in res.values())
    assert names == ["actor_unshared_backward_kernel", "actor_unshared_forward_kernel", "actor_unshared_reduce_kernel"], names
    for v in res.values():
        print(f"{v['name']}: {v['vgprs']} VGPRs + {v['agprs']} AGPRs, {v['sgprs']} SGPRs, LDS {v['lds_bytes_per_block']} B, "
              f"{v['waves_per_simd']} waves/SIMD, scratch {v['scratch_bytes_per_lane']} B/lane")
        assert v["scratch_bytes_per_lane"] == 0 and v["vgpr_spills"] == 0 and v["sgpr_spills"] == 0, v


def test_example_takes_unshared():
    """examples/train_maddpg.py --unshared (the parser runs before anything touches a GPU); MATD3 is built for shared_params."""
    script = os.path.join(ROOT, "examples", "train_maddpg.py")
    out = subprocess.run([sys.executable, script, "--help"], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and "--unshared" in out.stdout, out.stdout + out.stderr
    bad = subprocess.run([sys.executable, script, "--unshared", "--alg", "matd3"], capture_output=True, text=True, timeout=60)
    assert bad.returncode == 2 and "shared_params" in bad.stderr, bad.stderr


def test_cpu_models_keep_the_loop():
    """The launch is for GPU tensors: on the CPU nothing declines and nothing is counted."""
    from safe_marl_amd.util import FALLBACKS
    before = FALLBACKS.get("actor_unshared", 0)
    model = golden_model("MADDPG", golden_args("unshared_maddpg"), gauss_state_dict("unshared_maddpg"))
    batch = unshared_batch("unshared_maddpg")
    with th.no_grad():
        model.policy(batch.state, last_hid=batch.last_hid)
    model.policy(batch.state, last_hid=batch.last_hid)
    assert FALLBACKS.get("actor_unshared", 0) == before
