"""MATD3 under ``shared_params: False`` on CPU: golden vectors captured by importing the reference's MATD3 with one RNNAgent
and one twin-flag critic per agent (tests/golden/make_unshared_matd3_golden.py, three agents, the learner3 batch) — a strict
state_dict load, ``value()``, both losses, every gradient, ``need="value"`` / ``"policy"``, ``stat`` and the weights after one
value and one policy step, with the tolerances tests/test_unshared_cpu.py applies to the unshared_maddpg family.  The
target-smoothing noise of the recorded run is handed to ``torch.distributions.normal._standard_normal``.  Then the host side
of csrc/critic_unshared_twin.hip that needs no device: the example's flag, the binding and its argument checks, the kernels'
resources.

(The fixture family is named matd3_unshared: tests/test_unshared_cpu.py counts the files whose names begin with unshared_.)"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import torch as th

from .golden_io import StubEnv, golden_args, golden_batch, golden_model, golden_tensors, golden_vectors
from .test_gaussian_cpu import gauss_state_dict
from .test_mlp_agent_cpu import mlp_policy_loss

PREFIX = "matd3_unshared"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1                                                           # include/flexnet.h: FLEXNET_EINVAL


def recorded_noise(monkeypatch, draws, tile=1):
    """``Normal.rsample`` draws through ``_standard_normal``: the recorded draws, in order, tiled like the batch."""
    import torch.distributions.normal as tdn
    queue = [th.from_numpy(np.asarray(d)) for d in draws]

    def fake(shape, dtype, device):
        d = queue.pop(0)
        assert tuple(shape) == (tile * d.shape[0],) + tuple(d.shape[1:]), (tuple(shape), tuple(d.shape))
        return d.repeat((tile,) + (1,) * (d.dim() - 1)).to(device=device, dtype=dtype)

    monkeypatch.setattr(tdn, "_standard_normal", fake)
    return queue


# tests/test_unshared_cpu.py::test_golden_parity's tolerances for the unshared_maddpg family: losses relative, means absolute,
# gradients (absolute term, share of the golden tensor's largest entry), stat relative, the weights after a step (atol, rtol)
CPU_TOL = dict(pl=2e-6, vl=1e-5, means=2e-6, vgrad=(0.0, 1e-4), pgrad=(0.0, 1e-4), stat=1e-4, after=(3e-6, 1e-5), batchnorm=True)


def _assert_grads(named, grads, gold, key, tol, tag):
    for (k, _), g in zip(named, grads):
        ref = gold[key + k]
        bound = tol[0] + tol[1] * np.abs(ref).max()
        assert g is not None, k
        err = np.abs(g.detach().cpu().numpy() - ref).max()
        print(f"{tag} {key}{k}: error {err:.3e}, bound {bound:.3e}")
        assert err <= bound, (k, err, bound)


def check_golden_parity(monkeypatch, device="cpu", tile=1, tol=CPU_TOL):
    """The checks of tests/test_unshared_cpu.py::test_golden_parity for the MATD3 family, on ``device`` with the batch (and the
    draws) repeated ``tile`` times: every compared quantity is a mean over the batch or a per-sample value."""
    tag = f"{device} x{tile}"
    import safe_marl_amd.learner as L
    from safe_marl_amd.nets import RNNAgent
    from safe_marl_amd.trainer import PGTrainer
    gold = golden_vectors(PREFIX)
    args = golden_args(PREFIX, cuda=device != "cpu")
    n, o, a = args.agent_num, args.obs_size, args.action_dim
    assert args.agent_type == "rnn" and not args.shared_params and args.agent_id and n == 3 and not args.gaussian_policy
    model = golden_model("MATD3", args, gauss_state_dict(PREFIX, device=device), device)      # strict: names and shapes
    assert len(model.policy_dicts) == len(model.value_dicts) == n
    assert all(type(p) is RNNAgent for p in model.policy_dicts)
    assert all(c.fc1.in_features == n * (o + a) + n + 1 == 3 * 148 + 3 + 1 for c in model.value_dicts)
    batch = golden_batch("learner3", device, tile)
    b = 32 * tile

    with th.no_grad():
        v = model.value(batch.state, batch.action)
    assert v.shape == (2 * b, n, 1)
    got = v.cpu().numpy().reshape(2, tile, 32, n, 1)
    ref = gold["value"].reshape(2, 1, 32, n, 1)
    print("value: max error", np.abs(got - ref).max())
    assert np.abs(got - ref).max() <= 2e-5 * max(1.0, np.abs(ref).max())

    queue = recorded_noise(monkeypatch, [gold["sampled"]], tile)
    loss, pl, vl, means, log_stds = mlp_policy_loss(model, batch, args.entr)
    assert not queue                                                     # the one draw of a get_loss call was taken
    print("losses", pl.item(), float(gold["policy_loss"]), vl.item(), float(gold["value_loss"]))
    assert abs(pl.item() - float(gold["policy_loss"])) < tol["pl"] * max(1.0, abs(float(gold["policy_loss"])))
    assert abs(vl.item() - float(gold["value_loss"])) < tol["vl"] * max(1.0, abs(float(gold["value_loss"])))
    assert np.allclose(means.detach().cpu().numpy()[:32], gold["means"], atol=tol["means"])
    assert np.allclose(log_stds.detach().cpu().numpy()[:32], gold["log_stds"], atol=tol["means"])
    grads = th.autograd.grad(vl, list(model.value_dicts.parameters()), retain_graph=True)
    _assert_grads(model.value_dicts.named_parameters(), grads, gold, "vgrad.", tol["vgrad"], tag)
    w1 = n * o
    for i in range(n):                       # the one-hot input and the twin flag of agent i's critic
        gw = grads[[k for k, _ in model.value_dicts.named_parameters()].index(f"{i}.fc1.weight")].cpu().numpy()
        assert np.all(np.delete(gw[:, w1:w1 + n], i, axis=1) == 0.0) and np.abs(gw[:, -1]).max() > 0
    grads = th.autograd.grad(loss, list(model.policy_dicts.parameters()))
    _assert_grads(model.policy_dicts.named_parameters(), grads, gold, "pgrad.", tol["pgrad"], tag)

    # what a sub-update asks for
    recorded_noise(monkeypatch, [gold["sampled"]], tile)
    pl1, vl1, _ = model.get_loss(batch, need="value")
    assert pl1 is None and abs(vl1.item() - float(gold["value_loss"])) < tol["vl"] * max(1.0, abs(float(gold["value_loss"])))
    grads = th.autograd.grad(vl1, list(model.value_dicts.parameters()))
    _assert_grads(model.value_dicts.named_parameters(), grads, gold, "vgrad.", tol["vgrad"], tag + " need=value")
    recorded_noise(monkeypatch, [gold["sampled"]], tile)
    pl2, vl2, (means, log_stds) = model.get_loss(batch, need="policy")
    assert vl2 is None and abs(pl2.item() - float(gold["policy_loss"])) < tol["pl"] * max(1.0, abs(float(gold["policy_loss"])))
    from safe_marl_amd.util import normal_entropy
    grads = th.autograd.grad(pl2 - args.entr * normal_entropy(means, log_stds.exp()), list(model.policy_dicts.parameters()))
    _assert_grads(model.policy_dicts.named_parameters(), grads, gold, "pgrad.", tol["pgrad"], tag + " need=policy")

    # one value step, then one policy step through PGTrainer
    th.manual_seed(0)
    trainer = PGTrainer(args, L.MATD3, StubEnv(n), None)
    net = trainer.behaviour_net
    net.load_state_dict(gauss_state_dict(PREFIX, device=device))
    stat = {}
    recorded_noise(monkeypatch, [gold["step.sampled_value"], gold["step.sampled_policy"]], tile)
    trainer.value_transition_process(stat, batch)
    trainer.policy_transition_process(stat, batch)
    keys = {k[5:] for k in gold if k.startswith("stat.")}
    assert keys == set(stat) == {"mean_train_value_loss", "mean_train_value_grad_norm", "mean_train_policy_loss",
                                 "mean_train_policy_grad_norm", "mean_train_entropy"}
    for k in keys:
        print(k, float(stat[k]), gold["stat." + k])
        assert abs(float(stat[k]) - gold["stat." + k]) < tol["stat"] * max(1.0, abs(gold["stat." + k])), k
    after = gauss_state_dict(PREFIX, "state_dict_after_step")
    mine = net.state_dict()
    assert sorted(mine) == sorted(after)
    for k, ref in after.items():
        if "batchnorm" in k and not tol["batchnorm"]:    # (running_var sees the unbiased n / (n - 1) factor of a tiled batch)
            continue
        err = (mine[k].float().cpu() - ref.float()).abs().max().item()
        assert th.allclose(mine[k].float().cpu(), ref.float(), atol=tol["after"][0], rtol=tol["after"][1]), (k, err)
    init = golden_tensors(f"{PREFIX}_state_dict.npz")
    for i in range(n):
        assert (mine[f"policy_dicts.{i}.fc2.weight"].cpu() - init[f"policy_dicts.{i}.fc2.weight"]).abs().max() > 0
        assert (mine[f"value_dicts.{i}.fc1.weight"].cpu() - init[f"value_dicts.{i}.fc1.weight"])[:, -1].abs().max() > 0
    return model


def test_golden_parity(monkeypatch):
    from safe_marl_amd.util import FALLBACKS
    noted = dict(FALLBACKS)
    model = check_golden_parity(monkeypatch)
    assert model.unshared_twin_kernel and not model.unshared_critic_kernel
    assert dict(FALLBACKS) == noted                                      # the CPU takes the loop and notes nothing


def test_first_head_and_the_own_action_gradient():
    """``first_head_only`` is the first half of ``value()``; an action that takes a gradient carries agent i's own block only."""
    gold = golden_vectors(PREFIX)
    model = golden_model("MATD3", golden_args(PREFIX), gauss_state_dict(PREFIX))
    batch = golden_batch("learner3")
    b, n = 32, 3
    with th.no_grad():
        both = model.value(batch.state, batch.action)
        first = model.value(batch.state, batch.action, first_head_only=True)
    assert first.shape == (b, n, 1) and th.equal(first, both[:b])
    assert np.abs(first.numpy() - gold["value"][:b]).max() <= 2e-5 * max(1.0, np.abs(gold["value"]).max())
    act = batch.action.clone().requires_grad_()
    q = model.value(batch.state, act, critic_frozen=True, first_head_only=True)
    (g,) = th.autograd.grad(q[:, 1].sum(), act)
    assert g[:, 1].abs().max() > 0 and g[:, 0].abs().max() == 0 and g[:, 2].abs().max() == 0
    W = model.value_dicts[1].fc1.weight
    assert W.shape[1] == 3 * 148 + 3 + 1


def test_fixture_files_stay_below_the_largest_committed_one():
    g = os.path.join(ROOT, "tests", "golden")
    files = sorted(f for f in os.listdir(g) if f.startswith(PREFIX + "_"))
    assert files == [f"{PREFIX}_{k}" for k in ("args.json", "golden.npz", "state_dict.npz", "state_dict_after_step.npz")]
    assert all(os.path.getsize(os.path.join(g, f)) < min(os.path.getsize(os.path.join(g, "loop_golden.npz")), 1 << 20)
               for f in files)
    gold = golden_vectors(PREFIX)
    assert gold["sampled"].shape == gold["step.sampled_value"].shape == gold["step.sampled_policy"].shape == (32, 1, 4)
    assert gold["value"].shape == (64, 3, 1)


def test_example_takes_unshared_twins():
    """examples/train_maddpg.py --unshared-twins (the parser runs before anything touches a GPU)."""
    script = os.path.join(ROOT, "examples", "train_maddpg.py")
    out = subprocess.run([sys.executable, script, "--help"], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and "--unshared-twins" in out.stdout, out.stdout + out.stderr
    bad = subprocess.run([sys.executable, script, "--unshared-twins"], capture_output=True, text=True, timeout=60)
    assert bad.returncode == 2 and "--unshared-twins: needs --alg matd3" in bad.stderr, bad.stderr
    bad = subprocess.run([sys.executable, script, "--unshared-twins", "--alg", "iddpg"], capture_output=True, text=True, timeout=60)
    assert bad.returncode == 2 and "--alg matd3" in bad.stderr, bad.stderr
    old = subprocess.run([sys.executable, script, "--unshared", "--alg", "matd3"], capture_output=True, text=True, timeout=60)
    assert old.returncode == 2 and "--unshared: MATD3 is built for shared_params" in old.stderr, old.stderr
    assert "--unshared-twins" in old.stderr


def _aligned_pointer(buf):
    p = C.cast(buf, C.c_void_p).value
    return p + (-p) % 16


def test_binding_of_the_twin_entry_points():
    from safe_marl_amd import _lib, build
    build.build()
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "flexnet.h")).read()
    assert "#define FLEXNET_CRITIC_UNSHARED_TWIN_WS_FLOATS (FLEXNET_MAX_AGENTS * 128 * 448)" in hdr
    assert _lib.FLEXNET_CRITIC_UNSHARED_TWIN_WS_FLOATS == 8 * 128 * 7 * 64
    # the existing structs keep their sizes; the new forward struct has the old one's (`heads` sits in its padding word)
    assert C.sizeof(_lib.FlexCriticUnsharedArgs) == 8 * 4 + 2 * 8 + 4 * 8 + 8 * 8 * 8 + 3 * 8
    assert C.sizeof(_lib.FlexCriticUnsharedBwdArgs) == 8 * 4 + 3 * 8 + 5 * 8 * 8 + 9 * 8 + 4 * 4 + 2 * 8
    assert C.sizeof(_lib.FlexCriticUnsharedTwinArgs) == C.sizeof(_lib.FlexCriticUnsharedArgs)
    assert C.sizeof(_lib.FlexCriticUnsharedTwinBwdArgs) == 10 * 4 + 3 * 8 + 5 * 8 * 8 + 10 * 8 + 4 * 4 + 2 * 8
    for name in ("flexnet_critic_unshared_twin_forward", "flexnet_critic_unshared_twin_backward"):
        assert name in _lib.SYMBOLS and len(getattr(lib, name).argtypes) == 2 and name + "(" in hdr

    # forward: argument checks that run before any device work
    fwd = lib.flexnet_critic_unshared_twin_forward
    assert fwd(None, None) == EINVAL
    buf = (C.c_float * 64)()
    p = _aligned_pointer(buf)
    a = _lib.FlexCriticUnsharedTwinArgs()
    a.rows, a.n_agents, a.w1, a.w2, a.heads = 9, 3, 30, 4, 2
    assert fwd(C.byref(a), None) == EINVAL                       # null tensors
    a.x1 = a.q = p
    assert fwd(C.byref(a), None) == EINVAL                       # a second block without its tensor
    a.x2 = p
    assert fwd(C.byref(a), None) == EINVAL                       # empty parameter tables
    for name in ("fc1_w", "fc1_b", "fc2_w", "fc2_b", "fc3_w", "fc3_b"):
        for i in range(3):
            getattr(a, name)[i] = p
    a.rows = 10
    assert fwd(C.byref(a), None) == EINVAL                       # rows % n_agents != 0
    a.rows = 9
    for heads in (0, 3, -1):
        a.heads = heads
        assert fwd(C.byref(a), None) == EINVAL                   # heads outside {1, 2}
    a.heads, a.w1 = 2, 8 * 144 + 1
    assert fwd(C.byref(a), None) == _lib.FLEXNET_EUNSUPPORTED
    a.w1, a.w2 = 30, 8 * 8 + 1
    assert fwd(C.byref(a), None) == _lib.FLEXNET_EUNSUPPORTED
    a.w2, a.n_agents = 4, 9
    assert fwd(C.byref(a), None) == _lib.FLEXNET_EUNSUPPORTED
    a.n_agents, a.save_x = 3, p
    assert fwd(C.byref(a), None) == EINVAL                       # the saves: both or none
    a.save_x, a.layernorm = None, 1
    assert fwd(C.byref(a), None) == EINVAL                       # LayerNorm without its pair
    a.layernorm = 0
    for i in range(3):
        a.fc2_w[i] = p + 4
    assert fwd(C.byref(a), None) == _lib.FLEXNET_EUNSUPPORTED    # fc2_w not 16-byte aligned
    a.rows = 0
    for i in range(3):
        a.fc2_w[i] = p
    for heads in (1, 2):
        a.heads = heads
        assert fwd(C.byref(a), None) == 0                        # an empty batch: nothing to launch

    # backward
    bwd = lib.flexnet_critic_unshared_twin_backward
    assert bwd(None, None) == EINVAL
    g = _lib.FlexCriticUnsharedTwinBwdArgs()
    g.rows, g.n_agents, g.w1, g.w2, g.heads = 9, 3, 30, 4, 2
    assert bwd(C.byref(g), None) == EINVAL                       # null tensors
    g.dq = g.z1 = g.x = g.dz1_sum = p
    g.param_grads = 1
    assert bwd(C.byref(g), None) == EINVAL                       # parameter gradients without their buffers
    g.dz2 = g.d_fc1_b = g.d_fc2_b = g.d_fc3_w = g.d_fc3_b = g.workspace = p
    assert bwd(C.byref(g), None) == EINVAL                       # ... without d_flag
    g.param_grads = 0
    assert bwd(C.byref(g), None) == EINVAL                       # empty parameter tables
    for name in ("fc1_w", "fc2_w", "fc2_b", "fc3_w"):
        for i in range(3):
            getattr(g, name)[i] = p
    g.heads = 3
    assert bwd(C.byref(g), None) == EINVAL                       # heads outside {1, 2}
    g.heads = 1
    g.d_x2_own, g.own_first, g.own_step, g.own_w = p, 0, 2, 2
    assert bwd(C.byref(g), None) == EINVAL                       # the own block of agent 2 ends past x2
    g.own_step, g.own_w, g.w2 = 0, 9, 12
    assert bwd(C.byref(g), None) == _lib.FLEXNET_EUNSUPPORTED
    g.own_w, g.n_agents = 4, 9
    assert bwd(C.byref(g), None) == _lib.FLEXNET_EUNSUPPORTED
    g.n_agents, g.param_grads, g.d_flag, g.workspace_floats = 3, 1, p, 7 * 64 * 3 - 1
    assert bwd(C.byref(g), None) == EINVAL                       # a short workspace (one work-group per agent)
    g.rows = 0
    assert bwd(C.byref(g), None) == 0


def test_the_twin_kernels_do_not_spill():
    from safe_marl_amd import build
    build.build()
    res = build.kernel_resources("twin_critic_unshared")
    names = sorted(v["name"] for v in res.values())
    assert names == ["twin_critic_unshared_backward_kernel<false>", "twin_critic_unshared_backward_kernel<true>",
                     "twin_critic_unshared_forward_kernel<1>", "twin_critic_unshared_forward_kernel<2>",
                     "twin_critic_unshared_reduce_kernel"], names
    for v in res.values():
        print(f"{v['name']}: {v['vgprs']} VGPRs + {v['agprs']} AGPRs, {v['sgprs']} SGPRs, LDS {v['lds_bytes_per_block']} B, "
              f"{v['waves_per_simd']} waves/SIMD, scratch {v['scratch_bytes_per_lane']} B/lane")
        assert v["scratch_bytes_per_lane"] == 0 and v["vgpr_spills"] == 0 and v["sgpr_spills"] == 0, v
    # critic_unshared.hip's kernels keep their names and its forward its registers (the two files share the backward's stages,
    # csrc/critic_unshared_stages.h): the figures DESIGN.md §4.6h records
    old = {v["name"]: v for v in build.kernel_resources("critic_unshared").values()}
    assert len(old) == 4 and old["critic_unshared_forward_kernel"]["vgprs"] == 155


def test_which_class_takes_the_twin_kernel():
    import safe_marl_amd.learner as L
    assert L.MATD3.unshared_twin_kernel is True and L.MATD3.unshared_critic_kernel is False
    assert not any(hasattr(getattr(L, c), "unshared_twin_kernel") for c in ("MADDPG", "IDDPG", "FACMADDPG", "SQDDPG", "COMA"))
    shared = golden_args("learner3")
    assert L.MATD3(shared).graph_safe_updates is True
    assert L.MATD3(shared._replace(shared_params=False)).graph_safe_updates is False
