"""COMA (madrl/models/coma.py) on CPU: golden vectors captured by importing the reference's own modules
(tests/golden/make_coma_golden.py) with the recorded draws of the counterfactual baseline handed in through
``sample_source``; the rank-act_dim identity the HIP kernel rests on; the need split; the baseline takes no gradient; the
on-policy cadence on a vectorised CPU run; the C ABI; the cross-compiled kernels' resources."""
import ctypes as C
import os

import numpy as np
import pytest
import torch as th

from .golden_io import StubEnv, golden_args, golden_batch, golden_model, golden_tensors, golden_vectors

CASES = ["coma", "coma3"]


def _recorded(draws):
    draws = th.from_numpy(np.asarray(draws))

    def source(means, std, s):
        assert draws.shape == (s,) + tuple(means.shape)
        return draws
    return source


@pytest.mark.parametrize("prefix", CASES)
def test_golden_parity(prefix):
    from safe_marl_amd.learner import COMA
    from safe_marl_amd.trainer import PGTrainer
    gold = golden_vectors(prefix)
    args = golden_args(prefix)
    model = golden_model("COMA", args, f"{prefix}_state_dict.npz")
    n = args.agent_num
    assert args.sample_size == 10 and not args.normalize_advantages
    assert "batchnorm.running_mean" in model.state_dict()
    assert model.value_dicts[0].fc1.in_features == (n + 1) * 144 + n * 4 + n
    batch = golden_batch(prefix, gold=gold, fields=("action",))
    assert all(th.equal(batch.action[:, i], batch.action[:, 0]) for i in range(n))
    model.sample_source = _recorded(gold["sampled"])
    pl, vl, (means, log_stds) = model.get_loss(batch)
    # the tolerances of test_ppo_cpu.py / test_sqddpg_cpu.py for the same kinds of quantity
    assert abs(pl.item() - float(gold["policy_loss"])) < 2e-6
    assert abs(vl.item() - float(gold["value_loss"])) < 1e-5 * max(1.0, abs(float(gold["value_loss"])))
    assert np.allclose(means.detach().numpy(), gold["means"], atol=2e-6)
    t = model.last_terms
    for k in ("baselines", "values", "next_values"):
        assert np.allclose(t[k].numpy(), gold[k], atol=1e-5), k
    assert np.allclose(t["returns"].numpy(), gold["returns"], atol=2e-5)
    assert np.allclose(t["log_prob_a"].numpy(), gold["log_prob_a"], atol=1e-5)
    bn = model.batchnorm
    assert th.allclose(bn.running_mean, th.from_numpy(gold["reward_bn.running_mean"]), atol=1e-6)
    assert th.allclose(bn.running_var, th.from_numpy(gold["reward_bn.running_var"]), atol=1e-6, rtol=1e-5)
    assert int(bn.num_batches_tracked) == int(gold["reward_bn.num_batches_tracked"]) == 1
    grads = th.autograd.grad(vl, list(model.value_dicts.parameters()), retain_graph=True)
    for (k, _), g in zip(model.value_dicts.named_parameters(), grads):
        ref = gold["vgrad." + k]
        assert np.allclose(g.numpy(), ref, atol=2e-6 + 1e-4 * np.abs(ref).max()), k
    grads = th.autograd.grad(pl, list(model.policy_dicts.parameters()))
    for (k, _), g in zip(model.policy_dicts.named_parameters(), grads):
        ref = gold["pgrad." + k]
        assert np.allclose(g.numpy(), ref, atol=2e-6 + 1e-4 * np.abs(ref).max()), k

    # one value step, then one policy step through PGTrainer; update_target
    th.manual_seed(2468)
    trainer = PGTrainer(args, COMA, StubEnv(n), None)
    net = trainer.behaviour_net
    sd0 = golden_tensors(f"{prefix}_state_dict.npz")
    net.load_state_dict(sd0)
    net.target_net.load_state_dict({k[len("target_net."):]: v for k, v in sd0.items() if k.startswith("target_net.")})
    net.sample_source = _recorded(gold["step.sampled_policy"])       # the value step draws nothing here
    stat = {}
    trainer.value_transition_process(stat, batch)
    trainer.policy_transition_process(stat, batch)
    keys = {k[5:] for k in gold if k.startswith("stat.")}
    assert keys == set(stat) == {"mean_train_value_loss", "mean_train_value_grad_norm", "mean_train_policy_loss",
                                 "mean_train_policy_grad_norm", "mean_train_entropy"}
    for k in keys:
        assert abs(float(stat[k]) - gold["stat." + k]) < 1e-4 * max(1.0, abs(gold["stat." + k])), k
    after = golden_tensors(f"{prefix}_state_dict_after_step.npz")
    mine = net.state_dict()
    assert sorted(mine) == sorted(after)
    for k, ref in after.items():
        assert th.allclose(mine[k].float(), ref.float(), atol=3e-6, rtol=1e-5), k
    assert th.allclose(net.batchnorm.running_var, th.from_numpy(gold["after_step.reward_bn.running_var"]), atol=1e-6, rtol=1e-5)
    net.update_target()
    tgt = golden_tensors(f"{prefix}_target_after_update.npz")
    mine_t = net.target_net.state_dict()
    for k, ref in tgt.items():
        assert th.allclose(mine_t[k].float(), ref.float(), atol=3e-6, rtol=1e-5), k


def test_class_wiring():
    import safe_marl_amd
    from safe_marl_amd.learner import COMA, IDDPG, Model
    assert safe_marl_amd.COMA is COMA
    assert COMA.on_policy and COMA.graph_safe_updates is False and COMA.get_actions is IDDPG.get_actions
    assert COMA.sample_source is None and COMA._unfiled_columns is Model._unfiled_columns
    args = golden_args("coma")
    m = COMA(args)
    m.begin_update_event(None)                                     # a no-op
    n, o = args.agent_num, args.obs_size
    assert COMA(golden_args("coma", agent_id=False)).value_dicts[0].fc1.in_features == (n + 1) * o + n * 4
    assert len(COMA(golden_args("coma", shared_params=False)).value_dicts) == n
    obs, act = th.randn(7, n, o), th.randn(7, n, 4)
    assert m.value(obs, act).shape == (7, n, 1)
    with pytest.raises(NotImplementedError):
        COMA(golden_args("coma", continuous=False))


@pytest.mark.parametrize("prefix", CASES)
@pytest.mark.parametrize("layernorm", [True, False])
def test_rank_update_identity_in_float64(prefix, layernorm):
    """The critic on the materialised rows of coma.py:139-149 equals the tail of z1 + W_act,i (draw - action)."""
    from safe_marl_amd.nets import coma_baseline, coma_baseline_torch
    if layernorm:
        args = golden_args(prefix)
        model = golden_model("COMA", args, f"{prefix}_state_dict.npz")
    else:
        from safe_marl_amd.learner import COMA
        args = golden_args(prefix, layernorm=False)
        th.manual_seed(3)
        model = COMA(args)
    model = model.double()
    n, o, a, b, s = args.agent_num, args.obs_size, 4, 13, 10
    g = th.Generator().manual_seed(11)
    obs = th.randn(b, n, o, generator=g, dtype=th.float64)
    act = th.randn(b, n, a, generator=g, dtype=th.float64)
    sampled = th.randn(s, b, n, a, generator=g, dtype=th.float64)
    net = model.value_dicts[0]
    with th.no_grad():
        ref_base, ref_q = coma_baseline_torch(net, obs, act, sampled)
        z1 = model.first_layer(obs, act)
        base, q, values = coma_baseline(net, z1, act, sampled, want_q=True, want_values=True)
        plain = model.value(obs, act).view(b, n)
    assert ref_q.shape == q.shape == (s, b, n) and ref_q.abs().max() > 1e-3
    assert (q - ref_q).abs().max().item() < 1e-12
    assert (base - ref_base).abs().max().item() < 1e-12
    assert (values - plain).abs().max().item() < 1e-12
    # a chunked composition is the same composition (another GEMM shape: fp64 rounding only)
    with th.no_grad():
        assert (coma_baseline_torch(net, obs, act, sampled, s_chunk=3)[1] - ref_q).abs().max().item() < 1e-12


def test_need_value_draws_nothing_and_matches_both():
    gold = golden_vectors("coma")
    batch = golden_batch("coma", gold=gold, fields=("action",))
    both = golden_model("COMA", golden_args("coma"), "coma_state_dict.npz")
    both.sample_source = _recorded(gold["sampled"])
    pl, vl, _ = both.get_loss(batch)

    def never(*a):
        raise AssertionError("the value loss needs no draws")

    m = golden_model("COMA", golden_args("coma"), "coma_state_dict.npz")
    m.sample_source = never
    p, v, out = m.get_loss(batch, need="value")
    assert p is None and out is None and v.item() == vl.item()
    assert "baselines" not in m.last_terms and "sampled" not in m.last_terms
    ga = th.autograd.grad(v, list(m.value_dicts.parameters()))
    gb = th.autograd.grad(vl, list(both.value_dicts.parameters()), retain_graph=True)
    assert all(th.equal(x, y) for x, y in zip(ga, gb))
    m2 = golden_model("COMA", golden_args("coma"), "coma_state_dict.npz")
    m2.sample_source = _recorded(gold["sampled"])
    p2, v2, _ = m2.get_loss(batch, need="policy")
    assert v2 is None and p2.item() == pl.item()
    assert int(m.batchnorm.num_batches_tracked) == int(m2.batchnorm.num_batches_tracked) == 1


def test_the_baseline_takes_no_gradient():
    gold = golden_vectors("coma")
    batch = golden_batch("coma", gold=gold, fields=("action",))
    m = golden_model("COMA", golden_args("coma"), "coma_state_dict.npz")
    m.sample_source = _recorded(gold["sampled"])
    pl, vl, _ = m.get_loss(batch)
    for g in th.autograd.grad(pl, list(m.value_dicts.parameters()), allow_unused=True, retain_graph=True):
        assert g is None or float(g.abs().max()) == 0.0
    for g in th.autograd.grad(vl, list(m.policy_dicts.parameters()), allow_unused=True, retain_graph=True):
        assert g is None or float(g.abs().max()) == 0.0
    assert any(float(g.abs().max()) > 0 for g in th.autograd.grad(pl, list(m.policy_dicts.parameters())))
    # other draws move the policy loss and leave the value loss alone
    m2 = golden_model("COMA", golden_args("coma"), "coma_state_dict.npz")
    m2.sample_source = _recorded(gold["sampled"] + 0.5)
    pl2, vl2, _ = m2.get_loss(batch)
    assert vl2.item() == vl.item() and pl2.item() != pl.item()


def test_default_draws_are_torch_normal_in_the_reference_order():
    args = golden_args("coma")
    m = golden_model("COMA", args, "coma_state_dict.npz")
    means, std = th.randn(6, args.agent_num, 4), th.full((6, args.agent_num, 4), 0.7)
    th.manual_seed(5)
    mine = m.draw_samples(means, std)
    th.manual_seed(5)
    ref = th.normal(means.unsqueeze(0).repeat(10, 1, 1, 1), std.unsqueeze(0).repeat(10, 1, 1, 1))       # coma.py:139-141
    assert th.equal(mine, ref)


def test_policy_loss_composition_masks_and_sums():
    from safe_marl_amd.nets import coma_policy_loss, coma_policy_loss_torch
    g = th.Generator().manual_seed(2)
    means = th.randn(9, 3, 4, generator=g, requires_grad=True)
    log_stds = (0.2 * th.randn(9, 3, 4, generator=g)).requires_grad_()
    actions, q, base = th.randn(9, 3, 4, generator=g), th.randn(9, 3, generator=g), th.randn(9, 3, generator=g)
    avail = (th.rand(9, 3, 4, generator=g) > 0.3).float()
    loss, logp = coma_policy_loss(means, log_stds, actions, avail, q, base)
    from torch.distributions.normal import Normal
    want = (avail * Normal(means, log_stds.exp()).log_prob(actions)).sum(-1)
    assert th.allclose(logp, want.detach(), atol=1e-6)
    assert th.allclose(loss, -((q - base) * want).mean(), atol=1e-6)
    loss2, _ = coma_policy_loss_torch(means, log_stds, actions, avail, q - base)
    assert th.equal(loss, loss2)


# ---- cadence ----------------------------------------------------------------------------------------------------------
class FakeVecEnv:
    """What Model._train_process_vec touches of VecFlexProvisionEnv, on CPU."""
    handle = object()
    episode_limit = 10 ** 6

    def __init__(self, n_envs, n, o, seed=0):
        self.n_envs, self.n, self.o = n_envs, n, o
        self.g = th.Generator().manual_seed(seed)
        self.obs = th.zeros(n_envs, n, o)
        from safe_marl_amd._lib import INFO_KEYS
        self.info = th.zeros(n_envs, len(INFO_KEYS))
        self.failed = th.zeros(n_envs)

    def reset(self):
        self.obs = th.randn(self.n_envs, self.n, self.o, generator=self.g) * 0.3
        return self.obs

    def step(self, action, fuse_obs=True, auto_reset=True):
        self.obs = (0.9 * self.obs + 0.1 * action.mean(dim=(1, 2), keepdim=True)
                    + 0.05 * th.randn(self.n_envs, self.n, self.o, generator=self.g))
        reward = -self.obs.pow(2).mean(dim=(1, 2)).double()
        done = (th.rand(self.n_envs, generator=self.g) < 0.02)
        return reward, done, self.info


def test_vectorised_training_smoke_two_update_events():
    from safe_marl_amd.learner import COMA
    from safe_marl_amd.trainer import PGTrainer
    n_envs = 4
    args = golden_args("coma3", behaviour_update_freq=20, max_steps=20, batch_size=8, target_update_freq=40)
    env = FakeVecEnv(n_envs, args.agent_num, args.obs_size)
    th.manual_seed(0)
    trainer = PGTrainer(args, COMA, env, None, graph_rollout=False)
    assert trainer.on_policy and trainer.batch_scale == n_envs and trainer.effective_batch_size() == 8 * n_envs
    kinds = []
    orig = trainer._sub_update
    trainer._sub_update = lambda which, stat, batch, **k: (kinds.append((which, batch.state.shape[0])), orig(which, stat, batch, **k))[1]
    buf, stat = trainer.replay_buffer, {}
    before = [p.detach().clone() for p in trainer.behaviour_net.parameters()]
    trainer.behaviour_net.train_process(stat, trainer)            # steps 0..19: no event yet (steps > 0 is required)
    assert len(buf.buffer) == 20 * n_envs and not kinds
    trainer.behaviour_net.train_process(stat, trainer)            # the event falls on step 20
    assert kinds == [("value", 8 * n_envs)] * 10 + [("policy", 8 * n_envs)]
    assert len(buf.buffer) == 19 * n_envs                         # emptied at the event, 19 steps collected since
    trainer.behaviour_net.train_process(stat, trainer)            # the second event, on step 40
    assert len(kinds) == 22 and len(buf.buffer) == 19 * n_envs
    for k in ("mean_train_value_loss", "mean_train_policy_loss", "mean_train_policy_grad_norm", "mean_train_value_grad_norm"):
        assert np.isfinite(float(stat[k])), k
    after = list(trainer.behaviour_net.parameters())
    assert all(th.isfinite(p).all() for p in after)
    assert any(not th.equal(x, y) for x, y in zip(before, after))


# ---- ABI and build ------------------------------------------------------------------------------------------------------
def test_abi_structs_match_the_header_and_arguments_are_checked():
    from safe_marl_amd import _lib
    assert C.sizeof(_lib.FlexComaBaselineArgs) == 8 + 6 * 4 + 13 * 8
    assert C.sizeof(_lib.FlexComaPolicyArgs) == 8 + 4 * 4 + 12 * 8 + 8
    assert {"flexnet_coma_baseline", "flexnet_coma_policy_loss"} <= set(_lib.SYMBOLS)
    hdr = open(os.path.join(os.path.dirname(__file__), "..", "include", "flexnet.h")).read()
    body = hdr[hdr.index("int64_t batch;             /* b */\n    int32_t n_agents;\n    int32_t act_dim;\n    int32_t sample_size;       /* s */"):]
    body = body[:body.index("} FlexComaBaselineArgs;")]
    names = [ln.split(";")[0].split()[-1].lstrip("*") for ln in body.splitlines() if ";" in ln]
    assert names == [f[0] for f in _lib.FlexComaBaselineArgs._fields_]
    body = hdr[hdr.index("int64_t rows;              /* b */"):]
    body = body[:body.index("} FlexComaPolicyArgs;")]
    names = []
    for ln in body.splitlines():
        if ";" in ln:
            decl = ln.split(";")[0]
            names += [x.strip().split()[-1].lstrip("*") for x in decl.split(",")]
    assert names == [f[0] for f in _lib.FlexComaPolicyArgs._fields_]
    lib = _lib.load()
    a = _lib.FlexComaBaselineArgs()
    assert lib.flexnet_coma_baseline(C.byref(a), None) == -1                  # missing tensors, before any HIP call
    for k in ("z1", "w_act", "act", "sampled", "fc2_w", "fc2_b", "fc3_w", "fc3_b", "baseline"):
        setattr(a, k, 64)
    a.batch, a.n_agents, a.act_dim, a.sample_size = 4, 5, 4, 10
    a.layernorm = 1
    assert lib.flexnet_coma_baseline(C.byref(a), None) == -1                  # LayerNorm without its parameters
    a.layernorm = 0
    a.n_agents = 9
    assert lib.flexnet_coma_baseline(C.byref(a), None) == _lib.FLEXNET_EUNSUPPORTED
    a.n_agents, a.act_dim = 8, 5                                               # n a > 32
    assert lib.flexnet_coma_baseline(C.byref(a), None) == _lib.FLEXNET_EUNSUPPORTED
    a.n_agents, a.act_dim, a.z1 = 5, 4, 68                                     # misaligned z1
    assert lib.flexnet_coma_baseline(C.byref(a), None) == _lib.FLEXNET_EUNSUPPORTED
    a.z1, a.batch = 64, 0
    assert lib.flexnet_coma_baseline(C.byref(a), None) == 0                    # nothing to do, nothing launched
    p = _lib.FlexComaPolicyArgs()
    assert lib.flexnet_coma_policy_loss(C.byref(p), None) == -1


def test_coma_kernels_have_no_scratch():
    from safe_marl_amd import build
    build.build()
    ks = build.kernel_resources("coma")
    names = {v["name"] for v in ks.values()}
    assert {"coma_baseline_kernel", "coma_policy_kernel", "coma_loss_finish_kernel"} <= names
    for v in ks.values():
        assert v.get("scratch_bytes_per_lane", 0) == 0 and v.get("vgpr_spills", 0) == 0
