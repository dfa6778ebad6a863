"""SQDDPG on the GPU: csrc/sqddpg.hip (coalition draw, forward, backward) against the reference's own modules
(tests/golden/sqddpg*_*, make_sqddpg_golden.py) and against autograd of the PyTorch composition, its determinism, the
uniformity of the device draw, its memory at the update batch, the fallback, and a short training run."""
import warnings

import numpy as np
import pytest
import torch as th

from .golden_io import StubEnv, _np, golden_args, golden_batch, golden_model, golden_tensors, golden_vectors

pytestmark = pytest.mark.gpu

ROLES = ("policy", "value", "target")


def _tiled_pos(gold, key, args, tile):
    p = th.from_numpy(gold[key]).cuda()
    n, ns = args.agent_num, args.sample_size
    return p.view(-1, ns, n).repeat(tile, 1, 1).view(-1, n)


@pytest.mark.parametrize("prefix,tile", [("sqddpg", 1), ("sqddpg", 64), ("sqddpg3", 1), ("sqddpg3", 64)])
def test_fused_path_matches_the_reference(prefix, tile):
    from safe_marl_amd import util
    util.FALLBACKS.pop("sqddpg", None)
    args = golden_args(prefix, cuda=True)
    gold = golden_vectors(prefix)
    m = golden_model("SQDDPG", args, prefix + "_state_dict.npz", "cuda")
    b = golden_batch(prefix, "cuda", tile)
    assert m._fused(b.action)                                           # the HIP path is the one under test
    src = {}
    m.coalition_source = lambda role, groups: src[role]
    src["value"] = _tiled_pos(gold, "pos.call.value", args, tile)
    with th.no_grad():
        v = m.value(b.state, b.action)
        assert np.allclose(_np(v)[:32], gold["value"], atol=2e-5), np.abs(_np(v)[:32] - gold["value"]).max()
        phi = v.mean(1).view(-1, args.agent_num)
        assert np.allclose(_np(phi)[:32], gold["phi"], atol=2e-5)
    src.update({r: _tiled_pos(gold, f"pos.loss.{r}", args, tile) for r in ROLES})
    pl, vl, _ = m.get_loss(b)
    assert abs(pl.item() - float(gold["policy_loss"])) < 1e-5
    assert abs(vl.item() - float(gold["value_loss"])) < 1e-4 * max(1.0, abs(float(gold["value_loss"])))
    for k, g in zip([k for k, _ in m.value_dicts.named_parameters()],
                    th.autograd.grad(vl, list(m.value_dicts.parameters()), retain_graph=True)):
        r = gold["vgrad." + k]
        assert np.allclose(_np(g), r, atol=2e-6 + 2e-4 * np.abs(r).max()), (tile, k, np.abs(_np(g) - r).max())
    for k, g in zip([k for k, _ in m.policy_dicts.named_parameters()], th.autograd.grad(pl, list(m.policy_dicts.parameters()))):
        r = gold["pgrad." + k]
        assert np.allclose(_np(g), r, atol=2e-7 + 2e-4 * np.abs(r).max()), (tile, k, np.abs(_np(g) - r).max())
    # the split forms the trainer uses: the same losses and gradients
    _, vl2, _ = m.get_loss(b, need="value")
    assert abs(vl2.item() - vl.item()) < 1e-5 * max(1.0, abs(vl.item()))
    pl2, _, _ = m.get_loss(b, need="policy")
    assert abs(pl2.item() - pl.item()) < 1e-6
    assert "sqddpg" not in util.FALLBACKS


@pytest.mark.parametrize("prefix", ["sqddpg", "sqddpg3"])
def test_trainer_steps_and_target_update_match_the_reference(prefix):
    from safe_marl_amd.learner import SQDDPG
    from safe_marl_amd.trainer import PGTrainer
    args = golden_args(prefix, cuda=True)
    gold = golden_vectors(prefix)
    tr = PGTrainer(args, SQDDPG, StubEnv(args.agent_num), None)
    sd = golden_tensors(prefix + "_state_dict.npz", "cuda")
    tr.behaviour_net.load_state_dict(sd)
    tr.behaviour_net.target_net.load_state_dict({k[len("target_net."):]: v for k, v in sd.items() if k.startswith("target_net.")})
    b = golden_batch(prefix, "cuda")
    src = {}
    tr.behaviour_net.coalition_source = lambda role, groups: src[role]
    stat = {}
    src.update({r: th.from_numpy(gold[f"pos.vstep.{r}"]).cuda() for r in ROLES})
    tr.value_transition_process(stat, b)
    src.update({r: th.from_numpy(gold[f"pos.pstep.{r}"]).cuda() for r in ROLES})
    tr.policy_transition_process(stat, b)
    for k in ("mean_train_value_loss", "mean_train_policy_loss", "mean_train_value_grad_norm", "mean_train_policy_grad_norm"):
        ref = gold["stat." + k]
        assert abs(float(stat[k]) - ref) < 2e-4 * max(1.0, abs(ref)), k
    after = golden_tensors(prefix + "_state_dict_after_step.npz", "cuda")
    cur = tr.behaviour_net.state_dict()
    for k, v in after.items():
        assert np.allclose(_np(cur[k]), _np(v), atol=5e-5), (k, np.abs(_np(cur[k]) - _np(v)).max())
    tr.behaviour_net.update_target()
    cur = tr.behaviour_net.target_net.state_dict()
    for k, v in golden_tensors(prefix + "_target_after_update.npz", "cuda").items():
        assert np.allclose(_np(cur[k]), _np(v), atol=5e-5), k


def _random_model(n, layernorm, seed=0):
    from safe_marl_amd.learner import SQDDPG
    args = golden_args("sqddpg" if n == 5 else "sqddpg3", cuda=True, layernorm=layernorm)
    th.manual_seed(seed)
    m = SQDDPG(args).cuda()
    with th.no_grad():
        for p in m.value_dicts.parameters():
            p.add_(0.05 * th.randn_like(p))
    return m


def _clear_ties(m, obs, act, pos, w):
    """Zero the loss weight of samples with a ReLU pre-activation within 1e-5 of 0 in any of their rows (both fp32 forms may
    take different sides of the kink there): tests/fp64_budget.py's ``clear_ties`` on the fp64 pre-activations of a sample's
    rows side by side."""
    import copy
    from . import fp64_budget as fb
    net = copy.deepcopy(m.value_dicts[0]).double()
    b = obs.size(0)
    w = w.clone()
    fb.clear_ties(lambda: [p.reshape(b, -1) for p in fb.sqddpg_plain(net, obs.double(), act.double(), pos, m.sample_size)[2:]],
                  (), [w])
    return w


@pytest.mark.parametrize("layernorm", [True, False])
def test_kernel_matches_autograd_of_the_composition(layernorm):
    n, B = 5, 2048
    m = _random_model(n, layernorm)
    g = th.Generator(device="cuda").manual_seed(5)
    obs = 0.5 * th.randn(B, n, m.obs_dim, device="cuda", generator=g)
    act = th.rand(B, n, m.act_dim, device="cuda", generator=g)
    pos = th.argsort(th.rand(B * m.sample_size, n, device="cuda", generator=g), dim=1).argsort(dim=1)
    w = _clear_ties(m, obs, act, pos, th.randn(B, n, device="cuda", generator=g) / B)
    params = list(m.value_dicts.parameters())
    keep = (w.abs().sum(-1) > 0).float()

    def run(fused, dtype=th.float32):
        mm = m if dtype == th.float32 else __import__("copy").deepcopy(m).double()
        a = act.to(dtype).clone().requires_grad_(True)
        o = obs.to(dtype)
        if fused:
            phi, q = mm.shapley_values(o, a, pos, want_q=True)
        else:
            q = mm.marginal_contribution_torch(o, a, pos)
            phi = q.mean(1).view(-1, n)
        loss = (phi * w.to(dtype)).sum() + 0.1 * ((phi.sum(-1) ** 2) * keep.to(dtype)).mean()
        gr = th.autograd.grad(loss, [a] + list(mm.value_dicts.parameters()))
        return phi.detach(), q.detach(), gr

    phi, q, gk = run(True)
    phi0, q0, gt = run(False)
    _, _, g64 = run(False, th.float64)
    assert th.allclose(phi, phi0, atol=2e-5, rtol=1e-4), (phi - phi0).abs().max()
    assert th.allclose(q.view_as(q0), q0, atol=2e-5, rtol=1e-4)
    assert th.allclose(phi.sum(-1), phi0.sum(-1), atol=1e-4, rtol=1e-4)
    names = ["d_act_own"] + [k for k, _ in m.value_dicts.named_parameters()]
    for name, a, b_, c in zip(names, gk, gt, g64):
        scale = max(1e-6, float(c.abs().max()))
        err_k = float((a.double() - c).abs().max())
        err_t = float((b_.double() - c).abs().max())
        assert err_k <= 3.0 * err_t + 2e-4 * scale, (name, err_k, err_t, scale)
    # policy form (critic frozen): d act_own alone, the same numbers
    a = act.clone().requires_grad_(True)
    phi_f, _ = m.shapley_values(obs, a, pos, frozen=True)
    (da,) = th.autograd.grad((phi_f * w).sum() + 0.1 * ((phi_f.sum(-1) ** 2) * keep).mean(), [a])
    assert th.equal(da, gk[0])
    assert len(params) == len(gk) - 1


def test_two_runs_with_the_same_seed_are_bit_identical():
    outs = []
    for _ in range(2):
        m = _random_model(5, True, seed=3)
        g = th.Generator(device="cuda").manual_seed(9)
        obs = th.randn(4096, 5, m.obs_dim, device="cuda", generator=g)
        act = th.rand(4096, 5, m.act_dim, device="cuda", generator=g).requires_grad_(True)
        th.manual_seed(11)
        pos = m.draw_coalitions("value", 4096, obs.device)
        phi, _ = m.shapley_values(obs, act, pos)
        gr = th.autograd.grad((phi * phi).sum(), [act] + list(m.value_dicts.parameters()))
        outs.append((pos.clone(), phi.detach(), gr))
    assert th.equal(outs[0][0], outs[1][0]) and th.equal(outs[0][1], outs[1][1])
    assert all(th.equal(a, b) for a, b in zip(outs[0][2], outs[1][2]))


def test_device_draw_is_uniform_and_seeded():
    from safe_marl_amd.nets import sqddpg_draw
    groups = 200000
    rng = th.tensor([12345, 0], dtype=th.int64, device="cuda")
    pos = sqddpg_draw(groups, 5, rng).long().cpu()
    assert int(rng[1]) == 1
    assert th.equal(pos.sort(1).values, th.arange(5).expand(groups, 5))          # permutations
    for i in range(5):
        cnt = th.bincount(pos[:, i], minlength=5).double()
        chi2 = float(((cnt - groups / 5) ** 2 / (groups / 5)).sum())
        assert chi2 < 30.0, (i, chi2)                                            # 4 dof: p ~ 5e-6
    pos3 = sqddpg_draw(groups, 3, rng).long().cpu()
    code = (pos3 * th.tensor([9, 3, 1])).sum(1)
    cnt = th.bincount(code, minlength=27).double()
    perms = cnt[cnt > 0]
    assert perms.numel() == 6 and float(perms.sum()) == groups
    chi2 = float(((perms - groups / 6) ** 2 / (groups / 6)).sum())
    assert chi2 < 32.0, chi2                                                     # 5 dof
    again = sqddpg_draw(groups, 3, rng).long().cpu()
    assert not th.equal(again, pos3)                                             # the step advanced
    other = sqddpg_draw(groups, 5, th.tensor([54321, 0], dtype=th.int64, device="cuda")).long().cpu()
    same = sqddpg_draw(groups, 5, th.tensor([12345, 0], dtype=th.int64, device="cuda")).long().cpu()
    assert th.equal(same, pos) and not th.equal(other, pos)


def test_value_sub_update_memory_at_the_update_batch():
    from safe_marl_amd.learner import SQDDPG
    args = golden_args("sqddpg", cuda=True)
    th.manual_seed(0)
    m = SQDDPG(args, SQDDPG(args).cuda()).cuda()
    B = 32768
    b = golden_batch("sqddpg", "cuda", B // 32)
    _, vl, _ = m.get_loss(b, need="value")                                      # warm-up (workspaces)
    th.autograd.grad(vl, list(m.value_dicts.parameters()))
    del vl
    th.cuda.synchronize()
    th.cuda.reset_peak_memory_stats()
    base = th.cuda.memory_allocated()
    _, vl, _ = m.get_loss(b, need="value")
    gr = th.autograd.grad(vl, list(m.value_dicts.parameters()))
    th.cuda.synchronize()
    assert all(th.isfinite(g).all() for g in gr)
    assert th.cuda.max_memory_allocated() - base <= 256 * 2 ** 20, (th.cuda.max_memory_allocated() - base) / 2 ** 20


def test_unshared_critics_fall_back_to_the_composition():
    from safe_marl_amd import util
    from safe_marl_amd.learner import SQDDPG
    args = golden_args("sqddpg", cuda=True, shared_params=False)
    th.manual_seed(0)
    m = SQDDPG(args).cuda()
    b = golden_batch("sqddpg", "cuda")
    pos = th.from_numpy(golden_vectors("sqddpg")["pos.call.value"]).cuda()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        assert not m._fused(b.action)
        phi, _ = m.shapley_values(b.state, b.action, pos)
    assert util.FALLBACKS.get("sqddpg", 0) >= 1
    mc = SQDDPG(args._replace(cuda=False))
    mc.load_state_dict({k: v.cpu() for k, v in m.state_dict().items()})
    phi_c, _ = mc.shapley_values(b.state.cpu(), b.action.cpu(), pos.cpu())
    assert np.allclose(_np(phi), phi_c.detach().numpy(), atol=2e-5)


def test_short_training_run_moves_critic_and_policy():
    from safe_marl_amd import learner
    from safe_marl_amd.flex_env import VecFlexProvisionEnv
    from safe_marl_amd.network import create_network
    from safe_marl_amd.series import make_synthetic_series
    from safe_marl_amd.trainer import PGTrainer
    blds = [5, 10, 15, 20, 25]
    env_args = {"buildings": blds, "pv_nodes": blds, "ess_nodes": blds}
    net = create_network(env_args)
    env = VecFlexProvisionEnv(env_args, 256, net=net, series=make_synthetic_series(net, n_days=60), seed=3, warm_start=True)
    args = golden_args("sqddpg", cuda=True, agent_num=env.n_agents, obs_size=env.obs_size, state_size=env.state_size,
                       v_min=0.9, v_max=1.1, target_update_freq=60, value_update_epochs=2)
    th.manual_seed(0)
    np.random.seed(0)
    tr = PGTrainer(args, learner.SQDDPG, env, None, batch_scale=64, replay_capacity=256 * 96 * 2)
    net_ = tr.behaviour_net
    c0 = [p.detach().clone() for p in net_.value_dicts.parameters()]
    p0 = [p.detach().clone() for p in net_.policy_dicts.parameters()]
    stat = {}
    for _ in range(2):
        net_.train_process(stat, tr)
    th.cuda.synchronize()
    for k in ("mean_train_value_loss", "mean_train_policy_loss", "mean_train_value_grad_norm"):
        assert k in stat and np.isfinite(float(stat[k])), k
    assert all(not th.equal(a, p) for a, p in zip(c0, net_.value_dicts.parameters()))
    assert any(not th.equal(a, p) for a, p in zip(p0, net_.policy_dicts.parameters()))
    assert net_._rollout_graph.summed                          # IDDPG's fused agent-summed action selection
