"""gaussian_policy on CPU: golden vectors captured by importing the reference's MADDPG / IPPO / COMA with the actors of
madrl/agents/{rnn,mlp}_agent_gaussian.py (tests/golden/make_gaussian_golden.py) — strict state_dict loads, ``policy()``,
both losses, every gradient (the policy ones of the loss the trainer steps on: the entropy bonus is the DDPG family's only
log-std gradient), ``stat`` and the weights after one value and one policy step; the fixed-std path is untouched; the C
ABI's limits; the cross-compiled kernels' resources."""
import ctypes as C

import numpy as np
import pytest
import torch as th

from .golden_io import StubEnv, golden_args, golden_batch, golden_model, golden_tensors, golden_vectors

FAMILIES = [("gauss_maddpg", "MADDPG"), ("gauss_ippo", "IPPO"), ("gauss_coma", "COMA")]
BATCH_FIELDS = {"gauss_maddpg": (), "gauss_ippo": ("action", "done", "last_step"), "gauss_coma": ("action",)}


def gauss_state_dict(prefix, name="state_dict", device="cpu"):
    """The fixture's own entries plus the ``target_net.*`` ones, which the generator asserted equal to the INITIAL own
    entries (the target is a copy at construction; no update_target runs in the recorded step)."""
    sd = golden_tensors(f"{prefix}_{name}.npz", device)
    init = golden_tensors(f"{prefix}_state_dict.npz", device)
    sd.update({"target_net." + k: v.clone() for k, v in init.items()})
    return sd


def recorded(draws):
    draws = th.from_numpy(np.asarray(draws))

    def source(means, std, s):
        assert draws.shape == (s,) + tuple(means.shape)
        return draws.to(means.device)
    return source


def trainer_policy_loss(model, batch, entr):
    """The loss a policy sub-update steps on (trainer.py:47-57) and what get_loss returned."""
    from safe_marl_amd.util import normal_entropy
    pl, vl, (means, log_stds) = model.get_loss(batch)
    assert getattr(log_stds, "_flex_entropy", None) is None and log_stds.requires_grad
    return pl - entr * normal_entropy(means, log_stds.exp()), pl, vl, means, log_stds


def assert_grads(named, grads, gold, key):
    """Within 1e-4 of each golden tensor's largest entry, no absolute term (the log-std head's gradient is ~2e-5)."""
    for (k, _), g in zip(named, grads):
        ref = gold[key + k]
        bound = 1e-4 * np.abs(ref).max()
        assert g is not None, k
        err = np.abs(g.detach().cpu().numpy() - ref).max()
        assert err <= bound, (k, err, bound)


@pytest.mark.parametrize("prefix,cls", FAMILIES)
def test_golden_parity(prefix, cls):
    import safe_marl_amd.learner as L
    from safe_marl_amd.nets import RNNAgentGaussian
    from safe_marl_amd.trainer import PGTrainer
    gold = golden_vectors(prefix)
    args = golden_args(prefix)
    assert args.gaussian_policy and args.agent_type == "rnn" and (args.LOG_STD_MIN, args.LOG_STD_MAX) == (0.0, 0.5)
    model = golden_model(cls, args, gauss_state_dict(prefix))            # strict: the reference's names and shapes
    agent = model.policy_dicts[0]
    assert isinstance(agent, RNNAgentGaussian) and "fc2.weight" not in agent.state_dict()
    assert [k for k, _ in agent.named_parameters()][-4:] == ["mean.weight", "mean.bias", "log_std.weight", "log_std.bias"]
    batch = golden_batch(prefix, gold=gold, fields=BATCH_FIELDS[prefix])
    n = args.agent_num

    with th.no_grad():
        means, log_stds, hiddens = model.policy(batch.state, last_hid=batch.last_hid)
    assert log_stds.shape == means.shape == (32, n, 4) and not hasattr(log_stds, "_flex_entropy")
    assert np.allclose(means.numpy(), gold["policy_means"], atol=2e-6)
    assert np.allclose(log_stds.numpy(), gold["policy_log_stds"], atol=2e-6)
    assert np.allclose(hiddens.numpy(), gold["policy_hiddens"], atol=2e-6)
    assert float(log_stds.min()) >= args.LOG_STD_MIN and float(log_stds.max()) <= args.LOG_STD_MAX

    if cls == "COMA":
        model.sample_source = recorded(gold["sampled"])
    loss, pl, vl, means, log_stds = trainer_policy_loss(model, batch, args.entr)
    assert abs(pl.item() - float(gold["policy_loss"])) < 2e-6 * max(1.0, abs(float(gold["policy_loss"])))
    assert abs(vl.item() - float(gold["value_loss"])) < 1e-5 * max(1.0, abs(float(gold["value_loss"])))
    assert np.allclose(means.detach().numpy(), gold["means"], atol=2e-6)
    assert np.allclose(log_stds.detach().numpy(), gold["log_stds"], atol=2e-6)
    assert np.abs(gold["pgrad.0.log_std.weight"]).max() > 0              # the entropy bonus has a gradient now
    grads = th.autograd.grad(vl, list(model.value_dicts.parameters()), retain_graph=True)
    assert_grads(model.value_dicts.named_parameters(), grads, gold, "vgrad.")
    grads = th.autograd.grad(loss, list(model.policy_dicts.parameters()))
    assert_grads(model.policy_dicts.named_parameters(), grads, gold, "pgrad.")

    # one value step, then one policy step through PGTrainer
    th.manual_seed(0)
    trainer = PGTrainer(args, getattr(L, cls), StubEnv(n), None)
    net = trainer.behaviour_net
    net.load_state_dict(gauss_state_dict(prefix))
    if cls == "COMA":
        net.sample_source = recorded(gold["step.sampled_policy"])          # the value step draws nothing here
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
    moved = (mine["policy_dicts.0.log_std.weight"] - init["policy_dicts.0.log_std.weight"]).abs().max()
    assert moved > 0


def test_mlp_agent_policy():
    from safe_marl_amd.nets import MLPAgentGaussian
    prefix = "gauss_maddpg_mlp"
    gold, args = golden_vectors(prefix), golden_args(prefix)
    assert args.agent_type == "mlp" and args.gaussian_policy
    model = golden_model("MADDPG", args, gauss_state_dict(prefix))
    assert isinstance(model.policy_dicts[0], MLPAgentGaussian)
    assert sorted(k.split(".")[0] for k in model.policy_dicts[0].state_dict()) == sorted(
        2 * ["fc1", "fc2", "layernorm", "log_std", "mean"])
    batch = golden_batch(prefix)
    with th.no_grad():
        means, log_stds, hiddens = model.policy(batch.state, last_hid=batch.last_hid)
    assert np.allclose(means.numpy(), gold["policy_means"], atol=2e-6)
    assert np.allclose(log_stds.numpy(), gold["policy_log_stds"], atol=2e-6)
    assert np.allclose(hiddens.numpy(), gold["policy_hiddens"], atol=2e-6)


def test_unshared_agents_and_action_selection():
    """shared_params: False stacks the per-agent heads; every get_actions works on tensor log-stds."""
    import safe_marl_amd.learner as L
    g = th.Generator().manual_seed(5)
    for cls in ("MADDPG", "MATD3", "IDDPG", "FACMADDPG", "SQDDPG", "IPPO", "MAPPO", "COMA"):
        prefix = {"IPPO": "ippo", "MAPPO": "mappo", "COMA": "coma", "FACMADDPG": "facmaddpg", "SQDDPG": "sqddpg"}.get(cls, "learner")
        for shared in (True, False):
            if not shared and cls == "MATD3":
                continue                                             # (MATD3 is built for shared_params)
            args = golden_args(prefix, gaussian_policy=True, shared_params=shared, LOG_STD_MIN=-5.0, LOG_STD_MAX=2.0)
            th.manual_seed(3)
            m = getattr(L, cls)(args, getattr(L, cls)(args))
            n = args.agent_num
            obs, hid = th.randn(6, n, args.obs_size, generator=g), 0.1 * th.randn(6, n, 64, generator=g)
            avail = th.ones(6, n, 4)
            avail[0, 1, 2] = 0.0
            with th.no_grad():
                means, log_stds, _ = m.policy(obs, last_hid=hid)
                assert log_stds.shape == (6, n, 4) and log_stds.min() >= -5.0 and log_stds.max() <= 2.0
                assert log_stds.std() > 0
                th.manual_seed(9)
                actions, restored, logp, (_, ls), _ = m.get_actions(obs, status="train", exploration=True, actions_avail=avail,
                                                                    target=False, last_hid=hid)
                masked = log_stds.masked_fill(avail == 0, 0.0) if cls == "MATD3" else log_stds      # matd3.py:91-93
                assert th.equal(ls, masked) and restored.shape == (6, n, 4) and th.isfinite(logp).all()
                assert restored[0, 1, 2] == 0.0 and actions.abs().max() <= 1.0
                if cls != "MADDPG":                                  # the agent-summed selection: one action, per-sample std
                    lsum, msum = log_stds, means
                    if cls == "MATD3":
                        lsum, msum = log_stds.masked_fill(avail == 0, 0.0), means.masked_fill(avail == 0, 0.0)
                    th.manual_seed(9)
                    eps = th.randn(6, 1, 4)
                    want = th.tanh(msum.sum(1, keepdim=True) + lsum.sum(1, keepdim=True).exp() * eps)
                    assert th.allclose(actions, want, atol=1e-6)


def test_fixed_std_path_is_untouched():
    from safe_marl_amd.nets import RNNAgent, RNNAgentGaussian
    args = golden_args("learner")
    assert not args.gaussian_policy
    model = golden_model("MADDPG", args, "learner_state_dict.npz")
    assert type(model.policy_dicts[0]) is RNNAgent and not isinstance(model.policy_dicts[0], RNNAgentGaussian)
    batch = golden_batch("learner")
    means, log_stds, _ = model.policy(batch.state, last_hid=batch.last_hid)
    assert log_stds._flex_entropy is not None and log_stds.stride() == (0, 0, 0)      # the cached element, expanded
    assert float(log_stds.max()) == float(np.log(args.fixed_policy_std)) and not log_stds.requires_grad
    again = model.policy(batch.state, last_hid=batch.last_hid)[1]
    assert again.data_ptr() == log_stds.data_ptr()


def test_head_matches_the_reference_formula_in_float64():
    from safe_marl_amd.nets import gauss_log_std, gauss_log_std_torch
    g = th.Generator().manual_seed(2)
    h = (0.5 * th.randn(33, 64, generator=g, dtype=th.float64)).requires_grad_()
    w, b = 0.1 * th.randn(4, 64, generator=g, dtype=th.float64), 0.1 * th.randn(4, generator=g, dtype=th.float64)
    out = gauss_log_std(h, w, b, -5.0, 2.0)                              # CPU: the tensor composition
    u = th.tanh(h @ w.t() + b)
    assert th.equal(out, -5.0 + 0.5 * 7.0 * (u + 1)) and th.equal(out, gauss_log_std_torch(h, w, b, -5.0, 2.0))
    (gh,) = th.autograd.grad(out.sum(), h)
    assert th.allclose(gh, ((1 - u * u) * 3.5) @ w, atol=1e-12)


@pytest.fixture(scope="module")
def lib():
    from safe_marl_amd import build, _lib
    build.build()
    return _lib.load()


def test_abi_limits_are_refused_before_any_device_work(lib):
    from safe_marl_amd import _lib
    assert C.sizeof(_lib.FlexGaussHeadArgs) == 8 + 2 * 4 + 4 * 4 + 12 * 8
    assert C.sizeof(_lib.FlexGaussSumArgs) == 4 * 4 + 2 * 4 + 5 * 8
    assert C.sizeof(_lib.FlexPpoPolicyRowsArgs) == 8 + 4 * 4 + 10 * 8 + 8
    buf = (C.c_float * 1024)()
    p = C.addressof(buf)
    for fn in (lib.flexnet_gauss_head_forward, lib.flexnet_gauss_head_backward):
        assert fn(None, None) == -1                                          # FLEXNET_EINVAL
        a = _lib.FlexGaussHeadArgs()
        a.rows, a.act_dim, a.hid = 4, 4, 64
        assert fn(C.byref(a), None) == -1                                    # null tensors
        a.w = a.h = a.log_std = a.t = a.d_log_std = a.d_u = p
        for act_dim, hid in ((9, 64), (4, 32), (4, 128)):
            a.act_dim, a.hid = act_dim, hid
            assert fn(C.byref(a), None) == _lib.FLEXNET_EUNSUPPORTED, (act_dim, hid)
        a.act_dim, a.hid, a.rows = 4, 64, (1 << 30) + 1
        assert fn(C.byref(a), None) == _lib.FLEXNET_EUNSUPPORTED
    a = _lib.FlexGaussHeadArgs()
    a.rows, a.act_dim, a.hid = 4, 4, 64
    a.w = a.h = a.log_std = a.means = p                                      # an epilogue needs means, noise AND action
    assert lib.flexnet_gauss_head_forward(C.byref(a), None) == -1
    s = _lib.FlexGaussSumArgs()
    s.n_envs, s.n_agents, s.act_dim, s.act_high = 4, 5, 4, 1.0
    assert lib.flexnet_gauss_sum_explore(C.byref(s), None) == -1
    s.means = s.log_stds = s.eps = s.action = p
    for n, a_ in ((9, 4), (5, 9)):
        s.n_agents, s.act_dim = n, a_
        assert lib.flexnet_gauss_sum_explore(C.byref(s), None) == _lib.FLEXNET_EUNSUPPORTED
    r = _lib.FlexPpoPolicyRowsArgs()
    r.rows, r.n_agents, r.act_dim = 8, 5, 4
    assert lib.flexnet_ppo_policy_loss_rows(C.byref(r), None) == -1
    r.means = r.log_stds = r.actions = r.advantages = r.loss = r.d_means = r.workspace = p
    r.workspace_floats = _lib.FLEXNET_PPO_WS_FLOATS
    for n, a_, rows in ((9, 4, 8), (5, 9, 8), (5, 4, 1 << 28)):
        r.n_agents, r.act_dim, r.rows = n, a_, rows
        assert lib.flexnet_ppo_policy_loss_rows(C.byref(r), None) == _lib.FLEXNET_EUNSUPPORTED
    r.n_agents, r.act_dim, r.rows, r.workspace_floats = 5, 4, 8, 16
    assert lib.flexnet_ppo_policy_loss_rows(C.byref(r), None) == -1          # a short workspace


def test_new_kernels_use_no_scratch(lib):
    from safe_marl_amd import build
    names = {}
    for prefix in ("gauss_", "ppo_policy_rows_kernel"):
        names.update({v["name"]: v for v in build.kernel_resources(prefix).values()})
    assert {"gauss_head_forward_kernel", "gauss_head_backward_kernel", "gauss_sum_explore_kernel",
            "ppo_policy_rows_kernel"} <= set(names)
    for k, v in names.items():
        assert v["scratch_bytes_per_lane"] == 0 and v["vgpr_spills"] == 0 and v["sgpr_spills"] == 0, (k, v)
    assert names["gauss_head_forward_kernel"]["lds_bytes_per_block"] == 0
    assert names["gauss_head_backward_kernel"]["lds_bytes_per_block"] == 0
