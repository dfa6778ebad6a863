"""COMA on the GPU: csrc/coma.hip (the counterfactual baseline from the first-layer pre-activation, the policy loss) against
the reference's own modules (tests/golden/coma*_*, make_coma_golden.py) and against the materialising composition, its
determinism, the fallback, the first layer assembled from column blocks, and a short training run."""
import warnings

import numpy as np
import pytest
import torch as th

from .golden_io import StubEnv, _np, golden_args, golden_batch, golden_model, golden_tensors, golden_vectors

pytestmark = pytest.mark.gpu


def _random_model(n, layernorm, seed=0):
    from safe_marl_amd.learner import COMA
    args = golden_args("coma" if n == 5 else "coma3", cuda=True, layernorm=layernorm)
    th.manual_seed(seed)
    return COMA(args).cuda(), args


def _recorded(draws):
    draws = th.from_numpy(np.asarray(draws)).cuda()

    def source(means, std, s):
        assert draws.shape == (s,) + tuple(means.shape)
        return draws
    return source


@pytest.mark.parametrize("prefix", ["coma", "coma3"])
def test_fused_baseline_matches_the_reference(prefix):
    """The kernel on the golden batch, draws and weights: q_sampled, baseline and the values of the unmodified rows."""
    from safe_marl_amd.nets import coma_baseline
    args, gold = golden_args(prefix, cuda=True), golden_vectors(prefix)
    m = golden_model("COMA", args, prefix + "_state_dict.npz", "cuda")
    b = golden_batch(prefix, "cuda", gold=gold, fields=("action",))
    sampled = th.from_numpy(gold["sampled"]).cuda()
    with th.no_grad():
        z1 = m.first_layer(b.state, b.action)
    base, qs, q = coma_baseline(m.value_dicts[0], z1, b.action, sampled, want_q=True, want_values=True)
    for got, key in ((qs, "values_sampled"), (base, "baselines"), (q, "values")):
        print(key, np.abs(_np(got) - gold[key]).max())
        assert np.allclose(_np(got), gold[key], atol=2e-5, rtol=1e-4), key


@pytest.mark.parametrize("n", [5, 3])
@pytest.mark.parametrize("layernorm", [True, False])
@pytest.mark.parametrize("b,s", [(1000, 10), (77, 1), (4096, 10), (32, 3)])
def test_fused_baseline_against_the_materialising_composition(n, layernorm, b, s):
    from safe_marl_amd import util
    from safe_marl_amd.nets import coma_baseline, coma_baseline_torch, coma_rows
    util.FALLBACKS.pop("coma", None)
    m, args = _random_model(n, layernorm, seed=b + s)
    g = th.Generator(device="cuda").manual_seed(b * 7 + s)
    obs = 0.5 * th.randn(b, n, args.obs_size, device="cuda", generator=g)
    act = th.rand(b, n, 4, device="cuda", generator=g)
    sampled = act.unsqueeze(0) + th.randn(s, b, n, 4, device="cuda", generator=g)
    net = m.value_dicts[0]
    with th.no_grad():
        ref_base, ref_q = coma_baseline_torch(net, obs, act, sampled)
        ref_v = net(coma_rows(obs, act).reshape(b * n, -1), None)[0].view(b, n)
        z1 = m.first_layer(obs, act)
    base, qs, q = coma_baseline(net, z1, act, sampled, want_q=True, want_values=True)
    assert "coma" not in util.FALLBACKS
    assert qs.shape == (s, b, n) and base.shape == q.shape == (b, n)
    for got, ref, name in ((qs, ref_q, "q_sampled"), (base, ref_base, "baseline"), (q, ref_v, "values")):
        print(name, float((got - ref).abs().max()))
        assert th.allclose(got, ref, atol=2e-5, rtol=1e-4), name
    # the optional outputs are optional: the baseline alone is the same baseline
    only, none_q, none_v = coma_baseline(net, z1, act, sampled)
    assert none_q is None and none_v is None and th.equal(only, base)


def test_two_runs_are_bit_identical():
    from safe_marl_amd.nets import coma_baseline
    outs = []
    for _ in range(2):
        m, args = _random_model(5, True, seed=3)
        g = th.Generator(device="cuda").manual_seed(9)
        obs = th.randn(4099, 5, args.obs_size, device="cuda", generator=g)
        act = th.rand(4099, 5, 4, device="cuda", generator=g)
        sampled = th.randn(10, 4099, 5, 4, device="cuda", generator=g)
        with th.no_grad():
            z1 = m.first_layer(obs, act)
        outs.append(coma_baseline(m.value_dicts[0], z1, act, sampled, want_q=True, want_values=True))
    assert all(th.equal(x, y) for x, y in zip(*outs))


@pytest.mark.parametrize("rows,n", [(4096, 5), (777, 3)])
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("uniform", [True, False])
def test_policy_loss_kernel_and_gradients(rows, n, masked, uniform):
    from safe_marl_amd import util
    from safe_marl_amd.nets import coma_policy_loss, coma_policy_loss_torch
    util.FALLBACKS.pop("coma_policy_loss", None)
    m, args = _random_model(n, True)
    g = th.Generator(device="cuda").manual_seed(rows + n)
    means = th.randn(rows, n, 4, device="cuda", generator=g).requires_grad_()
    actions = th.randn(rows, n, 4, device="cuda", generator=g)
    q, base = th.randn(rows, n, device="cuda", generator=g), th.randn(rows, n, device="cuda", generator=g)
    avail = (th.rand(rows, n, 4, device="cuda", generator=g) > 0.3).float() if masked else None
    if uniform:
        log_stds = m._log_stds_like(means)
        leaves = [means]
    else:
        log_stds = (0.3 * th.randn(rows, n, 4, device="cuda", generator=g)).requires_grad_()
        leaves = [means, log_stds]
    loss, logp = coma_policy_loss(means, log_stds, actions, avail, q, base)
    assert "coma_policy_loss" not in util.FALLBACKS
    ref_loss, ref_logp = coma_policy_loss_torch(means.double(), log_stds.double(), actions.double(),
                                                None if avail is None else avail.double(), (q - base).double())
    assert th.allclose(logp.double(), ref_logp, atol=1e-5, rtol=1e-5)
    assert abs(loss.item() - ref_loss.item()) < 2e-6 * max(1.0, abs(ref_loss.item()))
    got = th.autograd.grad(loss, leaves)
    ref = th.autograd.grad(ref_loss, leaves)
    for a, r in zip(got, ref):
        assert th.allclose(a, r, atol=2e-6 + 2e-4 * float(r.abs().max())), float((a - r).abs().max())
    # the advantages handed in (the normalised ones) instead of q - baseline; a scaled seed scales the gradients
    loss2, _ = coma_policy_loss(means, log_stds, actions, avail, advantages=q - base)
    assert th.equal(loss2.detach(), loss.detach())
    got3 = th.autograd.grad(3.0 * loss2, leaves)
    for a, r in zip(got3, got):
        assert th.allclose(a, 3.0 * r, rtol=1e-6, atol=0)
    # determinism
    again, _ = coma_policy_loss(means, log_stds, actions, avail, q, base)
    assert th.equal(again.detach(), loss.detach()) and all(th.equal(x, y) for x, y in zip(th.autograd.grad(again, leaves), got))


@pytest.mark.parametrize("prefix", ["coma", "coma3"])
def test_golden_losses_and_steps_on_the_device(prefix):
    from safe_marl_amd import util
    from safe_marl_amd.learner import COMA
    from safe_marl_amd.trainer import PGTrainer
    util.FALLBACKS.pop("coma", None)
    util.FALLBACKS.pop("coma_policy_loss", None)
    args, gold = golden_args(prefix, cuda=True), golden_vectors(prefix)
    m = golden_model("COMA", args, prefix + "_state_dict.npz", "cuda")
    batch = golden_batch(prefix, "cuda", gold=gold, fields=("action",))
    assert m._fused(batch.state)                                       # the HIP path is the one under test
    m.sample_source = _recorded(gold["sampled"])
    pl, vl, (means, _) = m.get_loss(batch)
    assert abs(pl.item() - float(gold["policy_loss"])) < 2e-6
    assert abs(vl.item() - float(gold["value_loss"])) < 1e-5 * max(1.0, abs(float(gold["value_loss"])))
    t = m.last_terms
    for k in ("baselines", "values", "next_values", "returns", "log_prob_a"):
        assert np.allclose(_np(t[k]), gold[k], atol=2e-5, rtol=1e-4), (k, np.abs(_np(t[k]) - gold[k]).max())
    grads = th.autograd.grad(vl, list(m.value_dicts.parameters()), retain_graph=True)
    for (k, _), g in zip(m.value_dicts.named_parameters(), grads):
        r = gold["vgrad." + k]
        assert np.allclose(_np(g), r, atol=2e-6 + 2e-4 * np.abs(r).max()), (k, np.abs(_np(g) - r).max())
    assert all(g is None for g in th.autograd.grad(pl, list(m.value_dicts.parameters()), allow_unused=True, retain_graph=True))
    grads = th.autograd.grad(pl, list(m.policy_dicts.parameters()))
    for (k, _), g in zip(m.policy_dicts.named_parameters(), grads):
        r = gold["pgrad." + k]
        assert np.allclose(_np(g), r, atol=2e-6 + 2e-4 * np.abs(r).max()), (k, np.abs(_np(g) - r).max())
    # the split forms the trainer uses: the same losses
    m2 = golden_model("COMA", args, prefix + "_state_dict.npz", "cuda")
    m2.sample_source = _recorded(gold["sampled"])
    p2, _, _ = m2.get_loss(batch, need="policy")
    _, v2, _ = golden_model("COMA", args, prefix + "_state_dict.npz", "cuda").get_loss(batch, need="value")
    assert abs(p2.item() - pl.item()) < 1e-6 and abs(v2.item() - vl.item()) < 1e-6 * max(1.0, abs(vl.item()))
    # one value and one policy step through the trainer, then the target update
    trainer = PGTrainer(args, COMA, StubEnv(args.agent_num), None)
    net = trainer.behaviour_net
    sd0 = golden_tensors(f"{prefix}_state_dict.npz", "cuda")
    net.load_state_dict(sd0)
    net.target_net.load_state_dict({k[len("target_net."):]: v for k, v in sd0.items() if k.startswith("target_net.")})
    net.sample_source = _recorded(gold["step.sampled_policy"])
    stat = {}
    trainer.value_transition_process(stat, batch)
    trainer.policy_transition_process(stat, batch)
    after = golden_tensors(f"{prefix}_state_dict_after_step.npz", "cuda")
    cur = net.state_dict()
    for k, v in after.items():
        assert np.allclose(_np(cur[k]), _np(v), atol=5e-5), (k, np.abs(_np(cur[k]) - _np(v)).max())
    net.update_target()
    cur = net.target_net.state_dict()
    for k, v in golden_tensors(f"{prefix}_target_after_update.npz", "cuda").items():
        assert np.allclose(_np(cur[k]), _np(v), atol=5e-5), k
    assert "coma" not in util.FALLBACKS and "coma_policy_loss" not in util.FALLBACKS, util.FALLBACKS


def test_unshared_critics_fall_back_and_are_counted():
    from safe_marl_amd import util
    from safe_marl_amd.learner import COMA
    util.FALLBACKS.pop("coma", None)
    args = golden_args("coma", cuda=True, shared_params=False)
    gold = golden_vectors("coma")
    th.manual_seed(0)
    m = COMA(args, COMA(args).cuda()).cuda()
    batch = golden_batch("coma", "cuda", gold=gold, fields=("action",))
    m.sample_source = _recorded(gold["sampled"])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        assert not m._fused(batch.state)
        pl, vl, _ = m.get_loss(batch)
    assert util.FALLBACKS.get("coma", 0) >= 1
    mc = COMA(args._replace(cuda=False), COMA(args._replace(cuda=False)))
    mc.load_state_dict({k: v.cpu() for k, v in m.state_dict().items()})
    mc.sample_source = lambda means, std, s: th.from_numpy(gold["sampled"])
    from safe_marl_amd.replay_buffer import Transition
    plc, vlc, _ = mc.get_loss(Transition(*[f.cpu() for f in batch]))
    assert abs(pl.item() - plc.item()) < 2e-5 and abs(vl.item() - vlc.item()) < 2e-5 * max(1.0, abs(vlc.item()))
    assert np.allclose(_np(m.last_terms["baselines"]), _np(mc.last_terms["baselines"]), atol=2e-5, rtol=1e-4)


@pytest.mark.parametrize("n", [5, 3])
def test_value_from_column_blocks_matches_the_plain_critic(n):
    """value() at update sizes (first layer from fc1's column blocks, the fused tail) against the critic on materialised rows:
    values and parameter gradients."""
    from safe_marl_amd.nets import coma_merged_actions, coma_rows
    m, args = _random_model(n, True, seed=1)
    b = 4096
    obs = 0.3 * th.randn(b, n, args.obs_size, device="cuda")
    act = th.rand(b, n, 4, device="cuda")
    v = m.value(obs, act)
    ref = m.value_dicts[0](coma_rows(obs, act).reshape(b * n, -1), None)[0].view(b, n, 1)
    assert v.shape == (b, n, 1) and th.allclose(v, ref, atol=2e-5, rtol=1e-4), float((v - ref).abs().max())
    params = list(m.value_dicts.parameters())
    g = th.autograd.grad(v.pow(2).mean(), params)
    gr = th.autograd.grad(ref.pow(2).mean(), params)
    for a, r in zip(g, gr):
        assert th.allclose(a, r, atol=2e-6 + 2e-4 * r.abs().max().item()), float((a - r).abs().max())
    with th.no_grad():                                                   # the no-gradient form (bootstrap targets)
        assert th.allclose(m.value(obs, act), ref, atol=2e-5, rtol=1e-4)
        # the baseline's own form of value(): row-specific actions
        merged = coma_merged_actions(act[:64], act[:64].unsqueeze(0).repeat(2, 1, 1, 1))
        assert th.allclose(m.value(obs[:64], merged).view(2, 64, n), ref[:64].view(1, 64, n).expand(2, 64, n), atol=2e-5, rtol=1e-4)


def test_short_training_run_ends_with_finite_weights_and_an_emptied_replay():
    from safe_marl_amd import learner, util
    from safe_marl_amd.flex_env import VecFlexProvisionEnv
    from safe_marl_amd.network import create_network
    from safe_marl_amd.series import make_synthetic_series
    from safe_marl_amd.trainer import PGTrainer
    util.FALLBACKS.pop("coma", None)
    util.FALLBACKS.pop("coma_policy_loss", None)
    blds = [5, 10, 15, 20, 25]
    env_args = {"buildings": blds, "pv_nodes": blds, "ess_nodes": blds}
    net = create_network(env_args)
    n_envs = 64
    env = VecFlexProvisionEnv(env_args, n_envs, net=net, series=make_synthetic_series(net, n_days=60), seed=3, warm_start=True)
    args = golden_args("coma", cuda=True, agent_num=env.n_agents, obs_size=env.obs_size, state_size=env.state_size,
                       v_min=0.9, v_max=1.1)
    assert args.behaviour_update_freq == 60 and args.value_update_epochs == 10 and args.policy_update_epochs == 1
    th.manual_seed(0)
    np.random.seed(0)
    tr = PGTrainer(args, learner.COMA, env, None)
    assert tr.on_policy and tr.effective_batch_size() == 32 * n_envs
    net_ = tr.behaviour_net
    c0 = [p.detach().clone() for p in net_.value_dicts.parameters()]
    p0 = [p.detach().clone() for p in net_.policy_dicts.parameters()]
    buf = tr.replay_buffer
    cleared = []
    orig = buf.clear
    buf.clear = lambda: (cleared.append(len(buf.buffer)), orig())[1]
    stat = {}
    for _ in range(2):                                            # two episodes of 95 vector steps: update events on steps
        net_.train_process(stat, tr)                              # 60, 120 and 180
    th.cuda.synchronize()
    assert len(cleared) == 3 and all(c > 0 for c in cleared)
    assert len(buf.buffer) == 9 * n_envs                          # emptied at the last event, nine steps collected since
    for k in ("mean_train_value_loss", "mean_train_policy_loss", "mean_train_value_grad_norm", "mean_train_policy_grad_norm"):
        assert k in stat and np.isfinite(float(stat[k])), k
    assert all(th.isfinite(p).all() for p in net_.parameters())
    assert all(not th.equal(a, p) for a, p in zip(c0, net_.value_dicts.parameters()))
    assert any(not th.equal(a, p) for a, p in zip(p0, net_.policy_dicts.parameters()))
    assert net_._rollout_graph.summed                             # IDDPG's fused agent-summed action selection
    assert "coma" not in util.FALLBACKS and "coma_policy_loss" not in util.FALLBACKS, util.FALLBACKS
