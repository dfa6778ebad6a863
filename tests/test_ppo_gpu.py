"""csrc/ppo.hip on the MI355X: the three kernels against the tensor composition of the same formulas evaluated in float64
(values, gradients, ties and clip boundaries), bit identity of repeated runs, the CPU golden vectors reproduced on the
device, and a short training run of both classes.

Tolerances are measured, not chosen: for every compared quantity the bar is the error of the fp32 PyTorch composition itself
against the float64 evaluation on the same inputs (max |x - x64| / max |x64|), and the kernel may be four times that.  An fp32
output cannot be closer to the float64 value than its own rounding, so the measured error enters as max(measured, 2^-24).
Seen when the tests were written (rows 131 072, 5 agents): see MEASURED below."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch as th
import torch.nn as nn

from .golden_io import StubEnv, golden_args, golden_batch, golden_model, golden_tensors, golden_vectors

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GAMMA, LAM, EPS, COEF = 0.99, 0.95, 0.6, 2.0
SIZES = [(32, 3, 1), (32, 5, 8), (4096 * 8, 5, 4096), (4096 * 8, 3, 1), (4096 * 32, 5, 4096), (4096 * 32, 5, 1),
         (4096 * 32, 3, 4096),
         # chains whose length is no multiple of 64: the wavefront scan's partial last tile (identity maps past the start)
         (1000, 5, 1), (900, 3, 3)]
# name: (fp32 composition vs float64, kernel vs float64), the largest over SIZES as these tests printed them on one MI355X
MEASURED = {"reward_norm": (5.3e-7, 1.2e-7), "advantages": (5.8e-7, 3.1e-7), "advantages_norm": (5.7e-7, 2.5e-7),
            "running_mean": (2.9e-7, 5.1e-8), "running_var": (3.9e-7, 2.1e-7), "policy_loss": (7.0e-7, 5.7e-7),
            "d_means": (1.4e-6, 1.2e-6), "ratio": (1.2e-6, 1.0e-6), "value_loss": (9.7e-8, 2.8e-8),
            "d_values": (1.2e-7, 1.2e-7), "returns": (7.2e-8, 7.2e-8)}


def _rel(x, ref):
    ref = ref.double().cpu()
    return (x.double().cpu() - ref).abs().max().item() / max(ref.abs().max().item(), 1e-30)


def _check(name, got, fp32, ref64):
    measured = max(_rel(fp32, ref64), 2.0 ** -24)
    err = _rel(got, ref64)
    print(f"{name}: fp32 composition {measured:.3e}, kernel {err:.3e}")
    assert err <= 4 * measured, (name, err, measured)


def _bn(n, dtype=th.float32, device="cpu", seed=0):
    g = th.Generator().manual_seed(seed)
    bn = nn.BatchNorm1d(n)
    with th.no_grad():
        bn.weight.copy_(1 + 0.1 * th.randn(n, generator=g))
        bn.bias.copy_(0.1 * th.randn(n, generator=g))
        bn.running_mean.copy_(th.randn(n, generator=g))
        bn.running_var.copy_(1 + th.rand(n, generator=g))
    return bn.to(dtype).to(device)


def _gae_inputs(rows, n, seed=0):
    g = th.Generator().manual_seed(seed)
    r = 0.05 * th.randn(rows, n, generator=g) - 0.03
    v, nv = th.randn(rows, n, generator=g), th.randn(rows, n, generator=g)
    last = (th.rand(rows, generator=g) < 0.08).float()
    done = (th.rand(rows, generator=g) < 0.5).float() * last
    return r, v, nv, done, last


@pytest.mark.parametrize("rows,n,stride", SIZES)
def test_gae_kernel(rows, n, stride):
    from safe_marl_amd.nets import ppo_gae
    r, v, nv, done, last = _gae_inputs(rows, n)
    out = {}
    for key, dtype, dev, fused in (("ref", th.float64, "cpu", False), ("fp32", th.float32, "cpu", False),
                                   ("hip", th.float32, "cuda", True)):
        rbn, abn = _bn(n, dtype, dev, 1), _bn(n, dtype, dev, 2)
        args = [x.to(dtype).to(dev) for x in (r, v, nv, done, last)]
        out[key] = ppo_gae(*args, GAMMA, LAM, stride, rbn, abn, fused=fused) + (rbn, abn)
    for i, name in enumerate(("reward_norm", "advantages", "advantages_norm")):
        _check(name, out["hip"][i], out["fp32"][i], out["ref"][i])
    for j in (3, 4):
        for stat in ("running_mean", "running_var"):
            _check(stat, getattr(out["hip"][j], stat), getattr(out["fp32"][j], stat), getattr(out["ref"][j], stat))
        assert int(out["hip"][j].num_batches_tracked) == 1
    # without either normalisation: the reward passes through, advantages_norm is advantages
    args = [x.cuda() for x in (r, v, nv, done, last)]
    rn, adv, advn = ppo_gae(*args, GAMMA, LAM, stride, None, None)
    assert th.equal(rn, args[0]) and advn is adv
    ref = ppo_gae(*[x.double() for x in (r, v, nv, done, last)], GAMMA, LAM, stride, None, None, fused=False)[1]
    fp32 = ppo_gae(r, v, nv, done, last, GAMMA, LAM, stride, None, None, fused=False)[1]
    _check("advantages (raw reward)", adv, fp32, ref)


def _policy_inputs(rows, n, a=4, seed=0):
    g = th.Generator().manual_seed(seed)
    means = 0.3 * th.randn(rows, n, a, generator=g)
    act = th.tanh(means.sum(1, keepdim=True) + th.randn(rows, 1, a, generator=g)).expand(rows, n, a).contiguous()
    adv = th.randn(rows, n, generator=g)
    # ties: rows whose advantage is exactly zero (surr1 == surr2 == 0 whatever the ratio)
    adv[::7] = 0.0
    return means, act, adv


def _log_stds(means, std=1.0):
    ls = th.full((1,), float(np.log(std)), dtype=means.dtype, device=means.device).expand_as(means)
    ls._flex_entropy = th.zeros((), device=means.device)
    return ls


@pytest.mark.parametrize("rows,n,stride", SIZES)
@pytest.mark.parametrize("consistent", [False, True])
def test_policy_loss_kernel_and_gradient(rows, n, stride, consistent):
    from safe_marl_amd.nets import ppo_policy_loss, ppo_policy_loss_torch
    means, act, adv = _policy_inputs(rows, n)
    std = 1.0 if not consistent else 0.9
    old = None
    if consistent:
        # an old log-probability near the new one: ratios on both sides of the clip range, and INSIDE it, where
        # surr1 == surr2 exactly and th.min hands half of the gradient to each argument
        g = th.Generator().manual_seed(5)
        from torch.distributions.normal import Normal
        lp = Normal(means.sum(1, keepdim=True), th.tensor(std ** n)).log_prob(act)
        old = lp + 0.4 * th.randn(rows, n, 1, generator=g).expand(rows, n, 4) / 4
    res = {}
    for key, dtype, dev in (("ref", th.float64, "cpu"), ("fp32", th.float32, "cpu")):
        m = means.to(dtype).requires_grad_(True)
        o = act.to(dtype) if old is None else old.to(dtype)
        loss, ratio = ppo_policy_loss_torch(m, _log_stds(m, std), act.to(dtype), o, adv.to(dtype), EPS)
        (gm,) = th.autograd.grad(loss, [m])
        res[key] = (loss.detach(), gm, ratio.detach())
    m = means.cuda().requires_grad_(True)
    loss, ratio = ppo_policy_loss(m, _log_stds(m, std), act.cuda(), None if old is None else old.cuda(), adv.cuda(), EPS)
    (gm,) = th.autograd.grad(loss, [m])
    from safe_marl_amd.util import FALLBACKS
    assert "ppo_policy_loss" not in FALLBACKS
    if consistent:
        r = res["ref"][2]
        assert ((r < 1 - EPS).any() and (r > 1 + EPS).any() and ((r > 1 - EPS) & (r < 1 + EPS)).any()) or rows == 32
    _check("policy_loss", loss.detach(), res["fp32"][0], res["ref"][0])
    _check("d_means", gm, res["fp32"][1], res["ref"][1])
    _check("ratio", ratio, res["fp32"][2], res["ref"][2])


def test_policy_branch_weights_with_the_ratio_exactly_at_the_clip_boundaries():
    """The ratio comes out of expf, so it cannot be placed on 1 +- eps for eps > 0; with eps_clip = 0 both boundaries are 1,
    and log p - old is exactly 0 where old is the log-density itself on inputs whose terms are exact in fp32 (unit std,
    act - mu in {0, +-0.5, +-1}).  There surr1 == surr2 (th.min: half of the gradient each) AND the ratio sits on both ends
    of clamp's closed range (gradient passes): d loss / d log p is the whole -A/(rows n).  Rows with old off by +-0.25 are
    outside the (empty) range: the clipped branch has no gradient, the unclipped one only where it is the smaller.  The
    reference here is autograd through the fp32 composition: in float64 the upcast old no longer equals log p."""
    from torch.distributions.normal import Normal
    from safe_marl_amd.nets import ppo_policy_loss, ppo_policy_loss_torch
    rows, n, a = 4096, 5, 2          # two action dimensions: the sum over them is the same in any order
    g = th.Generator().manual_seed(11)
    means = th.randint(-2, 3, (rows, n, a), generator=g).float() * 0.25
    d = th.randint(-2, 3, (rows, 1, a), generator=g).float() * 0.5
    act = (means.sum(1, keepdim=True) + d).expand(rows, n, a).contiguous()
    adv = th.randn(rows, n, generator=g)
    lp = Normal(means.sum(1, keepdim=True), th.ones(())).log_prob(act)
    off = th.zeros(rows, 1, 1)
    off[1::3], off[2::3] = 0.25, -0.25
    old = lp + off.expand(rows, n, a) / a * 1.0
    m = means.clone().requires_grad_(True)
    loss, ratio = ppo_policy_loss_torch(m, _log_stds(m), act, old, adv, 0.0)
    (gref,) = th.autograd.grad(loss, [m])
    assert th.equal(ratio[0::3], th.ones_like(ratio[0::3])) and not (ratio[1::3] == 1).any()
    mc = means.cuda().requires_grad_(True)
    loss_k, ratio_k = ppo_policy_loss(mc, _log_stds(mc), act.cuda(), old.cuda(), adv.cuda(), 0.0)
    (gk,) = th.autograd.grad(loss_k, [mc])
    assert th.equal(ratio_k[0::3].cpu(), th.ones_like(ratio[0::3]))             # exactly on both boundaries
    scale = gref.abs().max().item()
    # same branches on every row; off the boundary the two expf (each good to an ulp or two: 2^-22 of the ratio between them)
    # and the order of the sum over five agents differ: four times that
    assert (gk.cpu() - gref).abs().max().item() <= 4 * 2.0 ** -22 * scale
    # the boundary rows carry the FULL gradient: d loss / d mu_k = -A/(rows n) * (act_k - mu_k), summed over the agents
    want = (-(adv[0::3] / (rows * n)).sum(1, keepdim=True) * d[0::3, 0]).unsqueeze(1).expand(-1, n, -1)
    assert th.allclose(gk.cpu()[0::3], want, atol=1e-9, rtol=1e-5)
    assert abs(loss_k.item() - loss.item()) <= 4 * 2.0 ** -22 * abs(loss.item())


def test_gae_entry_point_with_a_stride_beyond_the_rows():
    """include/flexnet.h: any rows / chain_stride >= 1.  A stride larger than the batch makes every row a chain of its own
    (the Python wrapper asks for whole steps and never sends this): the advantage is the row's delta."""
    import ctypes as C
    from safe_marl_amd import _lib
    rows, n = 5, 3
    r, v, nv, done, last = (x.cuda() for x in _gae_inputs(rows, n))
    rn, adv = th.empty_like(r), th.full_like(r, float("nan"))
    ws = th.empty(_lib.FLEXNET_PPO_WS_FLOATS // 2, dtype=th.float64, device="cuda")
    a = _lib.FlexPpoGaeArgs()
    a.rows, a.chain_stride, a.n_agents, a.gamma, a.lambda_ = rows, 8, n, GAMMA, LAM
    a.reward, a.old_values, a.old_next_values, a.done, a.last_step = (x.data_ptr() for x in (r, v, nv, done, last))
    a.reward_norm, a.advantages, a.workspace, a.workspace_floats = rn.data_ptr(), adv.data_ptr(), ws.data_ptr(), 2 * ws.numel()
    _lib.check(_lib.load().flexnet_ppo_gae(C.byref(a), C.c_void_p(th.cuda.current_stream().cuda_stream)), "flexnet_ppo_gae")
    m = th.where(last != 0, 1 - done, th.ones_like(done)).view(-1, 1)
    assert th.equal(rn, r) and th.allclose(adv, r + GAMMA * nv * m - v, atol=1e-6)


def test_nan_inputs_are_not_hidden():
    """th.min / th.max / th.clamp propagate a NaN; so do the kernels (a diverged run must not report a finite loss)."""
    from safe_marl_amd.nets import ppo_policy_loss, ppo_value_loss
    means, act, adv = (x.cuda() for x in _policy_inputs(64, 3))
    means[5, 1, 2] = float("nan")
    m = means.requires_grad_(True)
    assert th.isnan(ppo_policy_loss(m, _log_stds(m), act, None, adv, EPS)[0])
    values, old, nv, rn, done, eps = _value_inputs(64, 3)
    values[7, 2] = float("nan")
    assert th.isnan(ppo_value_loss(values.cuda().requires_grad_(True), old.cuda(), nv.cuda(), rn.cuda(), done.cuda(), GAMMA, eps,
                                   COEF)[0])


def _value_inputs(rows, n, seed=0):
    g = th.Generator().manual_seed(seed)
    old = th.randn(rows, n, generator=g)
    values = old + 0.5 * th.randn(rows, n, generator=g)
    nv, rn = th.randn(rows, n, generator=g), th.randn(rows, n, generator=g)
    done = (th.rand(rows, generator=g) < 0.05).float()
    eps = 0.5
    # rows exactly at the clip boundaries (V - old = +-eps, representable: old in quarters) ...
    old[0::16] = (old[0::16] * 4).round() / 4
    values[0::16] = old[0::16] + eps
    old[1::16] = (old[1::16] * 4).round() / 4
    values[1::16] = old[1::16] - eps
    # ... and ties surr1 == surr2 outside the range: returns midway between V and the clipped value (no bootstrap: done)
    old[2::16] = (old[2::16] * 4).round() / 4
    values[2::16] = old[2::16] + 1.5
    done2 = done.clone()
    done2[2::16] = 1.0
    rn[2::16] = old[2::16] + 1.0          # V - ret = 0.5, vc - ret = old + 0.5 - ret = -0.5
    return values, old, nv, rn, done2, eps


@pytest.mark.parametrize("rows,n,stride", SIZES)
def test_value_loss_kernel_and_gradient(rows, n, stride):
    from safe_marl_amd.nets import ppo_value_loss, ppo_value_loss_torch
    values, old, nv, rn, done, eps = _value_inputs(rows, n)
    res = {}
    for key, dtype in (("ref", th.float64), ("fp32", th.float32)):
        v = values.to(dtype).requires_grad_(True)
        loss, ret = ppo_value_loss_torch(v, old.to(dtype), nv.to(dtype), rn.to(dtype), done.to(dtype), GAMMA, eps, COEF)
        (gv,) = th.autograd.grad(loss, [v])
        res[key] = (loss.detach(), gv, ret.detach())
    v = values.cuda().requires_grad_(True)
    loss, ret = ppo_value_loss(v, old.cuda(), nv.cuda(), rn.cuda(), done.cuda(), GAMMA, eps, COEF)
    (gv,) = th.autograd.grad(loss, [v])
    from safe_marl_amd.util import FALLBACKS
    assert "ppo_value_loss" not in FALLBACKS
    _check("value_loss", loss.detach(), res["fp32"][0], res["ref"][0])
    _check("d_values", gv, res["fp32"][1], res["ref"][1])
    _check("returns", ret, res["fp32"][2], res["ref"][2])
    # the tie rule on the constructed rows, against autograd through the composition in float64:
    ref_g = res["ref"][1] * rows * n / (2 * COEF)
    got_g = gv.double().cpu() * rows * n / (2 * COEF)
    at_hi, at_lo, tie = slice(0, None, 16), slice(1, None, 16), slice(2, None, 16)
    # the clipped branch keeps its gradient AT the boundary (clamp's range includes its ends) ...
    assert th.allclose(got_g[at_hi], ref_g[at_hi], atol=1e-6) and th.allclose(got_g[at_lo], ref_g[at_lo], atol=1e-6)
    # ... and a tie outside the range hands half of the gradient to the unclipped branch only: 0.5 * (V - ret) = 0.25
    assert th.allclose(ref_g[tie], th.full_like(ref_g[tie], 0.25)) and th.allclose(got_g[tie], ref_g[tie], atol=1e-6)


@pytest.mark.parametrize("rows,n,stride", [(4096 * 32, 5, 4096), (4096 * 8, 5, 1), (32, 3, 1)])
def test_bit_identity(rows, n, stride):
    from safe_marl_amd.nets import ppo_gae, ppo_policy_loss, ppo_value_loss
    r, v, nv, done, last = (x.cuda() for x in _gae_inputs(rows, n))
    means, act, adv = (x.cuda() for x in _policy_inputs(rows, n))
    values, old, nv2, rn, done2, eps = _value_inputs(rows, n)
    runs = []
    for _ in range(2):
        rbn, abn = _bn(n, device="cuda", seed=1), _bn(n, device="cuda", seed=2)
        out = list(ppo_gae(r, v, nv, done, last, GAMMA, LAM, stride, rbn, abn))
        out += [rbn.running_mean, rbn.running_var, abn.running_mean, abn.running_var]
        m = means.clone().requires_grad_(True)
        loss, ratio = ppo_policy_loss(m, _log_stds(m), act, None, out[2], EPS)
        out += [loss.detach(), ratio, th.autograd.grad(loss, [m])[0]]
        vv = values.cuda().requires_grad_(True)
        loss, ret = ppo_value_loss(vv, old.cuda(), nv2.cuda(), out[0], done2.cuda(), GAMMA, eps, COEF)
        out += [loss.detach(), ret, th.autograd.grad(loss, [vv])[0]]
        runs.append([x.clone() for x in out])
    for a, b in zip(*runs):
        assert th.equal(a, b)


def test_configurations_outside_the_kernels_take_the_composition():
    from safe_marl_amd.nets import ppo_gae, ppo_policy_loss
    from safe_marl_amd.util import FALLBACKS
    rows, n = 64, 9
    r, v, nv, done, last = (x.cuda() for x in _gae_inputs(rows, n))
    before = dict(FALLBACKS)
    with pytest.warns(RuntimeWarning) if "ppo_gae" not in before else _nullcontext():
        rn, adv, advn = ppo_gae(r, v, nv, done, last, GAMMA, LAM, 1, _bn(n, device="cuda"), None)
    assert FALLBACKS.get("ppo_gae", 0) == before.get("ppo_gae", 0) + 1
    ref = ppo_gae(r.cpu(), v.cpu(), nv.cpu(), done.cpu(), last.cpu(), GAMMA, LAM, 1, _bn(n), None, fused=False)[1]
    assert th.allclose(adv.cpu(), ref, atol=1e-5)
    means, act, advp = (x.cuda() for x in _policy_inputs(64, 3))
    avail = th.ones(64, 3, 4, device="cuda")
    avail[:, 0, 0] = 0
    m = means.requires_grad_(True)
    ppo_policy_loss(m, _log_stds(m), act, None, advp, EPS, actions_avail=avail)
    assert FALLBACKS.get("ppo_policy_loss", 0) == before.get("ppo_policy_loss", 0) + 1


class _nullcontext:
    def __enter__(self):
        return None

    def __exit__(self, *a):
        return False


# ---- golden on the device --------------------------------------------------------------------------------------------
def _golden_setup(prefix, name):
    import safe_marl_amd.learner as L
    gold = golden_vectors(prefix)
    batch = golden_batch(prefix, "cuda", gold=gold, fields=("action", "done", "last_step"))
    return getattr(L, name), golden_args(prefix, cuda=True), gold, batch, golden_tensors(prefix + "_state_dict.npz")


@pytest.mark.parametrize("prefix,name", [("ippo", "IPPO"), ("mappo", "MAPPO"), ("ippo3", "IPPO"), ("mappo3", "MAPPO")])
def test_golden_losses_and_steps_on_the_device(prefix, name):
    from safe_marl_amd.trainer import PGTrainer
    from safe_marl_amd.util import FALLBACKS
    cls, args, gold, batch, sd = _golden_setup(prefix, name)
    model = golden_model(cls, args, sd, "cuda")
    # every action is available: flagged as the replay's constant mask is, the policy loss takes the kernel (a mask tensor
    # without the flag takes the composition — the steps through PGTrainer below run that way, as stored)
    before = {k: v for k, v in FALLBACKS.items() if k.startswith("ppo_")}
    avail = batch.action_avail.clone()
    avail._flex_const = 1.0
    pl, vl, (means, _) = model.get_loss(batch._replace(action_avail=avail))
    assert {k: v for k, v in FALLBACKS.items() if k.startswith("ppo_")} == before
    # the tolerances test_learner_golden_gpu.py / test_facmaddpg_golden_gpu.py apply to device-versus-reference comparisons
    assert abs(pl.item() - float(gold["policy_loss"])) < 1e-5
    assert abs(vl.item() - float(gold["value_loss"])) < 1e-5 * max(1.0, abs(float(gold["value_loss"])))
    assert np.allclose(means.detach().cpu().numpy(), gold["means"], atol=5e-6)
    t = model.last_terms
    for k in ("reward_norm", "advantages", "advantages_norm", "returns"):
        assert np.allclose(t[k].cpu().numpy(), gold[k], atol=2e-5), k
    assert np.allclose(t["ratios"].cpu().numpy(), gold["ratios"], atol=5e-6)
    for key, bn in (("reward_bn", model.batchnorm), ("adv_bn", model.rl.batchnorm)):
        assert th.allclose(bn.running_mean.cpu(), th.from_numpy(gold[key + ".running_mean"]), atol=1e-6)
        assert th.allclose(bn.running_var.cpu(), th.from_numpy(gold[key + ".running_var"]), atol=1e-6, rtol=1e-5)
        assert int(bn.num_batches_tracked) == 1

    after = golden_tensors(prefix + "_state_dict_after_step.npz")
    tgt = golden_tensors(prefix + "_target_after_update.npz")
    # the steps through PGTrainer twice: with the mask flagged (ppo_policy_kernel's d_means goes through the optimiser step)
    # and as stored (a mask tensor without the flag: the policy loss takes the composition, a recorded fallback)
    for label, b in (("kernel", batch._replace(action_avail=avail)), ("as stored", batch)):
        th.manual_seed(2468)
        trainer = PGTrainer(args, cls, StubEnv(args.agent_num), None)
        net = trainer.behaviour_net
        net.load_state_dict(sd)
        net.target_net.load_state_dict({k[len("target_net."):]: v for k, v in sd.items() if k.startswith("target_net.")})
        before = FALLBACKS.get("ppo_policy_loss", 0)
        stat = {}
        trainer.value_transition_process(stat, b)
        trainer.policy_transition_process(stat, b)
        assert FALLBACKS.get("ppo_policy_loss", 0) == before + (0 if label == "kernel" else 1), label
        for k in ("mean_train_value_loss", "mean_train_value_grad_norm", "mean_train_policy_loss", "mean_train_policy_grad_norm",
                  "mean_train_entropy"):
            ref = float(gold["stat." + k])
            assert abs(float(stat[k]) - ref) < 2e-4 * max(1.0, abs(ref)), (label, k)
        cur = net.state_dict()
        for k, v in after.items():
            assert np.allclose(cur[k].float().cpu().numpy(), v.float().numpy(), atol=5e-5), (label, k, (cur[k].cpu() - v).abs().max())
        net.update_target()
        mine_t = net.target_net.state_dict()
        for k, ref in tgt.items():
            assert th.allclose(mine_t[k].float().cpu(), ref.float(), atol=3e-6, rtol=1e-5), (label, k)


@pytest.mark.parametrize("name", ["MAPPO", "IPPO"])
def test_values_at_update_sizes_match_the_composition(name):
    """The tall passes (first layer once per sample + the id column; csrc/wgrad.hip behind IPPO's rows) against the plain
    module, values and parameter gradients."""
    cls, args, gold, batch, sd = _golden_setup(name.lower(), name)
    model = cls(args).cuda()
    obs = 0.3 * th.randn(4096, args.agent_num, args.obs_size, device="cuda")
    v = model.value(obs, None)
    model.fused_inference = False
    ref = model.value(obs, None)
    model.fused_inference = True
    assert th.allclose(v, ref, atol=2e-5)
    params = list(model.value_dicts.parameters())
    g = th.autograd.grad(v.pow(2).mean(), params)
    gr = th.autograd.grad(ref.pow(2).mean(), params)
    for a, b in zip(g, gr):
        assert th.allclose(a, b, atol=2e-6 + 2e-4 * b.abs().max().item())


# ---- training --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("alg", ["mappo", "ippo"])
def test_short_training_run(alg):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "train_maddpg.py"), "--alg", alg, "--envs", "256",
                          "--episodes", "6"], capture_output=True, text=True, timeout=420, cwd=ROOT)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    res = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])
    # the trainer's real vector path (slab windows, the constant action mask, filed columns) ran the kernels every time
    assert not [k for k in res["fallbacks"] if k.startswith("ppo_")], res["fallbacks"]
    assert res["grad_steps"] > 0
    stat = res["stat"]
    for k in ("mean_train_value_loss", "mean_train_policy_loss", "mean_train_policy_grad_norm", "mean_train_reward"):
        assert np.isfinite(stat[k]), (k, stat)
    assert stat["mean_train_policy_grad_norm"] > 0
