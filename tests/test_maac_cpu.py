"""MAAC (madrl/models/maac.py, madrl/critics/maac_critic.py) on CPU: golden vectors captured by importing the reference's own
modules (tests/golden/make_maac_golden.py) with the recorded exploration draws handed in through ``noise_source``; the
state_dict keys; the configurations the HIP kernel declines (two heads, input BatchNorm) against a direct fp64 evaluation; the
need split; the C ABI; the cross-compiled kernels' resources; the example's command line."""
import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch as th
import torch.nn.functional as F

from .golden_io import StubEnv, golden_args, golden_batch, golden_model, golden_tensors, golden_vectors

CASES = ["maac", "maac3"]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _state_dict(prefix):
    sd = golden_tensors(f"{prefix}_state_dict.npz")
    sd.update({"target_net." + k: v for k, v in golden_tensors(f"{prefix}_target_state_dict.npz").items()})
    return sd


def _recorded(gold, keys):
    """``noise_source`` that hands out gold[keys[role]] and counts the calls."""
    calls = []

    def source(role, shape):
        draw = th.from_numpy(np.asarray(gold[keys[role]]))
        assert tuple(draw.shape) == tuple(shape), (role, draw.shape, shape)
        calls.append(role)
        return draw
    source.calls = calls
    return source


@pytest.mark.parametrize("prefix", CASES)
def test_golden_parity(prefix):
    from safe_marl_amd.learner import MAAC
    from safe_marl_amd.trainer import PGTrainer
    gold = golden_vectors(prefix)
    args = golden_args(prefix)
    model = golden_model("MAAC", args, _state_dict(prefix))
    n = args.agent_num
    assert args.soft and args.reward_scale == 100 and args.gaussian_policy and not args.normalize_advantages
    assert len(model.value_dicts) == 1 and sum(p.numel() for p in model.value_dicts.parameters()) == \
        n * (64 * 149 + 64 * 145 + 64 * 129 + 65 + 64 * 65 + 65) + 3 * 64 * 64 + 64
    tgt, own = model.target_net.state_dict(), model.state_dict()
    assert any(not th.equal(tgt[k], own[k]) for k in tgt if k.startswith("policy_dicts."))      # a target of its own
    batch = golden_batch(prefix)
    with th.no_grad():
        value = model.value(batch.state, batch.action)
    assert value.shape == (33, n)
    # the tolerances of test_coma_cpu.py for the same kinds of quantity
    assert np.allclose(value[:-1].numpy(), gold["value"][:-1], atol=1e-5)
    assert np.allclose(value[-1].numpy(), gold["value"][-1], atol=1e-9, rtol=1e-5)               # the regulariser row, ~1e-4
    model.noise_source = _recorded(gold, {"behaviour": "draws.behaviour", "target": "draws.target"})
    pl, vl, (means, log_stds) = model.get_loss(batch)
    assert model.noise_source.calls == ["behaviour", "target"]
    assert abs(pl.item() - float(gold["policy_loss"])) < 2e-6
    assert abs(vl.item() - float(gold["value_loss"])) < 1e-5 * max(1.0, abs(float(gold["value_loss"])))
    assert np.allclose(means.detach().numpy(), gold["means"], atol=2e-6)
    assert np.allclose(log_stds.detach().numpy(), gold["log_stds"], atol=2e-6)
    assert model.last_terms["log_prob_a"].shape == (32, n)
    assert np.allclose(model.last_terms["log_prob_a"].numpy(), gold["log_prob_a"], atol=1e-5)
    vgold = dict(np.load(os.path.join(ROOT, "tests", "golden", f"{prefix}_golden_vgrads.npz")))
    grads = th.autograd.grad(vl, list(model.value_dicts.parameters()), retain_graph=True)
    assert len(grads) == len(vgold)
    for (k, _), g in zip(model.value_dicts.named_parameters(), grads):
        ref = vgold["vgrad." + k]
        assert np.allclose(g.numpy(), ref, atol=2e-6 + 1e-4 * np.abs(ref).max()), k
    grads = th.autograd.grad(pl, list(model.policy_dicts.parameters()))
    for (k, _), g in zip(model.policy_dicts.named_parameters(), grads):
        ref = gold["pgrad." + k]
        assert np.abs(ref).max() > 0 and np.allclose(g.numpy(), ref, atol=2e-6 + 1e-4 * np.abs(ref).max()), k

    # one value step, then one policy step through PGTrainer; update_target
    th.manual_seed(8642)
    trainer = PGTrainer(args, MAAC, StubEnv(n), None)
    net = trainer.behaviour_net
    net.load_state_dict(_state_dict(prefix))
    stat = {}
    net.noise_source = _recorded(gold, {"behaviour": "step.draws.value.behaviour", "target": "step.draws.value.target"})
    trainer.value_transition_process(stat, batch)
    assert net.noise_source.calls == ["behaviour", "target"]
    net.noise_source = _recorded(gold, {"behaviour": "step.draws.policy.behaviour"})           # no TD target, no target draw
    trainer.policy_transition_process(stat, batch)
    assert net.noise_source.calls == ["behaviour"]
    keys = {k[5:] for k in gold if k.startswith("stat.")}
    assert keys == set(stat) == {"mean_train_value_loss", "mean_train_value_grad_norm", "mean_train_policy_loss",
                                 "mean_train_policy_grad_norm", "mean_train_entropy"}
    for k in keys:
        assert abs(float(stat[k]) - gold["stat." + k]) < 1e-4 * max(1.0, abs(gold["stat." + k])), k
    after = golden_tensors(f"{prefix}_state_dict_after_step.npz")
    mine = {k: v for k, v in net.state_dict().items() if not k.startswith("target_net.")}
    assert sorted(mine) == sorted(after)
    for k, ref in after.items():
        assert th.allclose(mine[k].float(), ref.float(), atol=3e-6, rtol=1e-5), k
    before = golden_tensors(f"{prefix}_target_state_dict.npz")
    net.update_target()
    tgt = golden_tensors(f"{prefix}_target_after_update.npz")
    mine_t = net.target_net.state_dict()
    moved = 0
    for k, ref in tgt.items():
        assert th.allclose(mine_t[k].float(), ref.float(), atol=3e-6, rtol=1e-5), k
        moved += int(not th.equal(ref, before[k]))
    assert moved >= len(list(net.policy_dicts.parameters())) + len(list(net.value_dicts.parameters()))


def test_state_dict_keys_are_the_references():
    args = golden_args("maac")
    from safe_marl_amd.nets import AttentionCritic
    keys = set(AttentionCritic(args).state_dict())
    want = {"key_extractors.0.weight", "selector_extractors.0.weight", "value_extractors.0.0.weight", "value_extractors.0.0.bias"}
    for i in range(5):
        for stem in (f"critic_encoders.{i}.enc_fc1", f"critics.{i}.critic_fc1", f"critics.{i}.critic_fc2", f"biases.{i}.bias_fc1",
                     f"biases.{i}.bias_fc2", f"state_encoders.{i}.s_enc_fc1"):
            want |= {stem + ".weight", stem + ".bias"}
    assert keys == want
    assert {"value_dicts.0." + k for k in want} == {k for k in golden_tensors("maac_state_dict.npz") if k.startswith("value_dicts.")}
    normed = set(AttentionCritic(golden_args("maac", norm_in=True, attend_heads=2)).state_dict())
    extra = {f"{stem}.{i}.{bn}.{buf}" for i in range(5) for stem, bn in (("critic_encoders", "enc_bn"), ("state_encoders", "s_enc_bn"))
             for buf in ("running_mean", "running_var", "num_batches_tracked")}
    heads = {"key_extractors.1.weight", "selector_extractors.1.weight", "value_extractors.1.0.weight", "value_extractors.1.0.bias"}
    assert normed == want | extra | heads


def test_class_wiring():
    import safe_marl_amd
    from safe_marl_amd.learner import MAAC, MADDPG
    assert safe_marl_amd.MAAC is MAAC
    assert MAAC.graph_safe_updates is False and not MAAC.on_policy and MAAC.noise_source is None
    assert MAAC.get_actions is not MADDPG.get_actions
    args = golden_args("maac")
    assert len(MAAC(golden_args("maac", shared_params=False)).value_dicts) == 1          # ONE critic whatever shared_params says
    assert len(MAAC(golden_args("maac", shared_params=False)).policy_dicts) == 5
    forced = MAAC(golden_args("maac", gaussian_policy=False))
    assert forced.args.gaussian_policy and type(forced.policy_dicts[0]).__name__ == "RNNAgentGaussian"
    assert type(MAAC(golden_args("maac", agent_type="mlp")).policy_dicts[0]).__name__ == "MLPAgentGaussian"
    m = MAAC(args, MAAC(args))
    obs, act = th.randn(7, 5, 144), th.randn(7, 5, 4)
    assert m.value(obs, act).shape == (8, 5)
    avail = th.ones(7, 5, 4)
    avail[:, 2, 1] = 0
    a, ra, lp, (means, log_stds), hid = m.get_actions(obs, "train", True, avail, last_hid=th.zeros(7, 5, 64))
    assert a.shape == (7, 1, 4) and ra.shape == (7, 5, 4) and lp.shape == (7, 5) and hid.shape == (7, 5, 64)
    assert float(ra[:, 2, 1].detach().abs().max()) == 0.0 and th.equal(ra[:, 0], a[:, 0])
    assert not th.allclose(lp[:, 2], lp[:, 0]) and th.equal(lp[:, 1], lp[:, 0])         # the masked action leaves the sum
    with pytest.raises(NotImplementedError):
        MAAC(golden_args("maac", continuous=False))


def _direct_fp64(critic, obs, act):
    """maac_critic.py:86-159 written out agent by agent and head by head, in the module's dtype."""
    n, hid, heads = critic.nagents, critic.hidden_dim, critic.attend_heads
    d = hid // heads
    lre = lambda x: th.where(x > 0, x, 0.01 * x)          # noqa: E731

    def norm(x):
        return (x - x.mean(0, keepdim=True)) / th.sqrt(x.var(0, unbiased=False, keepdim=True) + 1e-5)

    sa_in = th.cat((obs, act), -1)
    sa, s = [], []
    for j in range(n):
        x, y = sa_in[:, j], obs[:, j]
        if critic.norm_in:
            x, y = norm(x), norm(y)
        e, se = critic.critic_encoders[j].enc_fc1, critic.state_encoders[j].s_enc_fc1
        sa.append(lre(x @ e.weight.t() + e.bias))
        s.append(lre(y @ se.weight.t() + se.bias))
    qs, regs = [], []
    for i in range(n):
        others, reg = [], 0.0
        for hd in range(heads):
            K, Q, V = critic.key_extractors[hd], critic.selector_extractors[hd], critic.value_extractors[hd][0]
            sel = s[i] @ Q.weight.t()
            logits = th.stack([(sel * (sa[j] @ K.weight.t())).sum(-1) for j in range(n) if j != i], dim=1)
            vals = th.stack([lre(sa[j] @ V.weight.t() + V.bias) for j in range(n) if j != i], dim=1)
            w = th.softmax(logits / math.sqrt(d), dim=1)
            others.append((w.unsqueeze(-1) * vals).sum(1))
            reg = reg + 1e-3 * (logits ** 2).mean()
        c, bm = critic.critics[i], critic.biases[i]
        x = th.cat([sa[i]] + others, dim=1)
        q = lre(x @ c.critic_fc1.weight.t() + c.critic_fc1.bias) @ c.critic_fc2.weight.t() + c.critic_fc2.bias
        b = lre(s[i] @ bm.bias_fc1.weight.t() + bm.bias_fc1.bias) @ bm.bias_fc2.weight.t() + bm.bias_fc2.bias
        qs.append(q - b)
        regs.append(reg)
    return th.cat(qs, dim=1), th.stack(regs)


@pytest.mark.parametrize("over", [dict(), dict(attend_heads=2), dict(norm_in=True), dict(attend_heads=4, norm_in=True)],
                         ids=["default", "heads2", "norm_in", "heads4_norm_in"])
def test_composition_against_a_direct_fp64_evaluation(over):
    from safe_marl_amd.nets import AttentionCritic, attn_critic, attn_critic_declines
    from safe_marl_amd.util import FALLBACKS
    args = golden_args("maac3", **over)
    th.manual_seed(4)
    critic = AttentionCritic(args).double()
    with th.no_grad():
        for p in critic.parameters():
            p.copy_(0.2 * th.randn_like(p))
    g = th.Generator().manual_seed(9)
    obs = 0.5 * th.randn(19, 3, 144, generator=g, dtype=th.float64)
    act = th.tanh(th.randn(19, 3, 4, generator=g, dtype=th.float64)).requires_grad_()
    before = dict(FALLBACKS)
    q, reg = attn_critic(critic, obs, act)                       # train mode: the BatchNorm normalises with batch statistics
    assert dict(FALLBACKS) == before                            # on the CPU nothing declines and nothing is counted
    rq, rreg = _direct_fp64(critic, obs, act)
    assert q.shape == (19, 3) and reg.shape == (3,)
    assert (q - rq).abs().max().item() < 1e-12 and (reg - rreg).abs().max().item() < 1e-14
    up = th.randn(19, 3, generator=g, dtype=th.float64)
    params = list(critic.parameters())
    mine = th.autograd.grad((q * up).sum() + reg.sum(), [act] + params)
    ref = th.autograd.grad((rq * up).sum() + rreg.sum(), [act] + params)
    for a, b in zip(mine, ref):
        assert (a - b).abs().max().item() < 1e-11
    why = attn_critic_declines(critic, obs, act)
    assert why is not None                                        # (CPU tensors, fp64: outside the kernel's domain anyway)
    pre = []
    critic(obs, act.detach(), pre=pre)
    assert len(pre) == 4 + args.attend_heads and all(t.shape[:2] == (19, 3) for t in pre)


def test_declines_name_the_reason():
    from safe_marl_amd.nets import AttentionCritic, attn_critic_declines

    class OnDevice(th.Tensor):
        """A CPU tensor that says it lives on the GPU: the checks past the device test, without a device."""
        is_cuda = True

    obs, act = th.zeros(4, 5, 144).as_subclass(OnDevice), th.zeros(4, 5, 4).as_subclass(OnDevice)
    assert "attend_heads 2" in attn_critic_declines(AttentionCritic(golden_args("maac", attend_heads=2)), obs, act)
    assert "norm_in True" in attn_critic_declines(AttentionCritic(golden_args("maac", norm_in=True)), obs, act)
    assert "hid 32" in attn_critic_declines(AttentionCritic(golden_args("maac", hid_size=32)), obs, act)
    assert "agents 9" in attn_critic_declines(AttentionCritic(golden_args("maac", agent_num=9)), th.zeros(4, 9, 144).as_subclass(OnDevice),
                                              th.zeros(4, 9, 4).as_subclass(OnDevice))
    assert "obs 142" in attn_critic_declines(AttentionCritic(golden_args("maac", obs_size=142)), th.zeros(4, 5, 142).as_subclass(OnDevice), act)
    assert "float64" in attn_critic_declines(AttentionCritic(golden_args("maac")), obs.double().as_subclass(OnDevice), act)
    # everything about the call is inside the domain: what is left is where the parameters live
    assert "parameter" in attn_critic_declines(AttentionCritic(golden_args("maac")), obs, act)


def test_need_split_matches_the_single_call():
    gold = golden_vectors("maac")
    batch = golden_batch("maac")
    keys = {"behaviour": "draws.behaviour", "target": "draws.target"}

    def fresh():
        m = golden_model("MAAC", golden_args("maac"), _state_dict("maac"))
        m.noise_source = _recorded(gold, keys)
        return m

    both = fresh()
    pl, vl, _ = both.get_loss(batch)
    m = fresh()
    p, v, out = m.get_loss(batch, need="value")
    assert p is None and out is None and abs(v.item() - vl.item()) < 1e-6
    ga = th.autograd.grad(v, list(m.value_dicts.parameters()))
    gb = th.autograd.grad(vl, list(both.value_dicts.parameters()), retain_graph=True)
    assert all(th.allclose(x, y, atol=1e-7, rtol=1e-5) for x, y in zip(ga, gb))
    for g in th.autograd.grad(v, list(m.policy_dicts.parameters()), allow_unused=True):
        assert g is None                                         # the draw's log-density enters the target without a graph
    m2 = fresh()
    p2, v2, out2 = m2.get_loss(batch, need="policy")
    assert v2 is None and out2 is not None and abs(p2.item() - pl.item()) < 1e-6 and m2.noise_source.calls == ["behaviour"]
    ga = th.autograd.grad(p2, list(m2.policy_dicts.parameters()))
    gb = th.autograd.grad(pl, list(both.policy_dicts.parameters()), retain_graph=True)
    assert all(th.allclose(x, y, atol=1e-7, rtol=1e-5) for x, y in zip(ga, gb))
    assert int(m.batchnorm.num_batches_tracked) == int(m2.batchnorm.num_batches_tracked) == 1
    # the reference's single call sends the regulariser's gradient to the critic and the value loss's to the policy
    assert any(float(g.abs().max()) > 0 for g in th.autograd.grad(pl, list(both.value_dicts.parameters()), retain_graph=True))
    assert any(float(g.abs().max()) > 0 for g in th.autograd.grad(vl, list(both.policy_dicts.parameters()), allow_unused=True)
               if g is not None)
    # other draws move both losses: the behaviour draw's log-density is in the TD target
    m3 = fresh()
    m3.noise_source = lambda role, shape: th.from_numpy(gold[keys[role]]) + 0.5
    pl3, vl3, _ = m3.get_loss(batch)
    assert pl3.item() != pl.item() and vl3.item() != vl.item()


def test_default_draws_are_rsamples_own():
    args = golden_args("maac")
    batch = golden_batch("maac")
    a, b = (golden_model("MAAC", args, _state_dict("maac")) for _ in range(2))
    th.manual_seed(5)
    pa, va, _ = a.get_loss(batch)
    th.manual_seed(5)
    import torch.distributions.normal as tdn
    b.noise_source = lambda role, shape: tdn._standard_normal(shape, dtype=th.float32, device=th.device("cpu"))
    pb, vb, _ = b.get_loss(batch)
    assert abs(pa.item() - pb.item()) < 1e-6 and abs(va.item() - vb.item()) < 1e-6


# ---- ABI and build ------------------------------------------------------------------------------------------------------
def _header_fields(hdr, struct):
    body = hdr[:hdr.index("} " + struct + ";")]
    body = body[body.rindex("typedef struct {"):]
    names = []
    for ln in body.splitlines():
        if ";" in ln:
            decl = ln.split(";")[0]
            names += [x.strip().split()[-1].lstrip("*").split("[")[0] for x in decl.split(",")]
    return names


def test_abi_structs_match_the_header_and_arguments_are_checked():
    from safe_marl_amd import _lib
    assert C.sizeof(_lib.FlexAttnCriticArgs) == 8 + 4 * 4 + 2 * 8 + 12 * 8 * 8 + 16 * 8 + 8
    assert C.sizeof(_lib.FlexAttnCriticBwdArgs) == 8 + 4 * 4 + 9 * 8 + 5 * 8 * 8 + 17 * 8 + 8
    assert {"flexnet_attn_critic_forward", "flexnet_attn_critic_backward"} <= set(_lib.SYMBOLS)
    hdr = open(os.path.join(ROOT, "include", "flexnet.h")).read()
    assert _header_fields(hdr, "FlexAttnCriticArgs") == [f[0] for f in _lib.FlexAttnCriticArgs._fields_]
    assert _header_fields(hdr, "FlexAttnCriticBwdArgs") == [f[0] for f in _lib.FlexAttnCriticBwdArgs._fields_]
    lib = _lib.load()
    assert lib.flexnet_attn_critic_forward(None, None) == -1
    a = _lib.FlexAttnCriticArgs()
    assert lib.flexnet_attn_critic_forward(C.byref(a), None) == -1                   # missing tensors, before any HIP call
    shared = ("obs", "act", "key_w", "sel_w", "val_w", "val_b", "sa", "key", "val", "q", "reg", "workspace")
    for k in shared:
        setattr(a, k, 64)
    a.batch, a.n_agents, a.obs_dim, a.act_dim, a.workspace_floats = 40, 5, 144, 4, 10
    assert lib.flexnet_attn_critic_forward(C.byref(a), None) == -1                   # a missing per-agent table entry
    for name in ("enc_w", "enc_b", "senc_w", "senc_b", "c1_w", "c1_b", "c2_w", "c2_b", "b1_w", "b1_b", "b2_w", "b2_b"):
        for i in range(8):
            getattr(a, name)[i] = 64
    a.workspace_floats = 9
    assert lib.flexnet_attn_critic_forward(C.byref(a), None) == -1                   # a short workspace (two tiles of five)
    a.workspace_floats = 10
    a.save_s = 64
    assert lib.flexnet_attn_critic_forward(C.byref(a), None) == -1                   # one save without the others
    a.save_s = None
    for bad in (dict(n_agents=1), dict(n_agents=9), dict(obs_dim=148), dict(obs_dim=142), dict(act_dim=9),
                dict(batch=_lib.FLEXNET_ATTN_CRITIC_MAX_BATCH + 1, workspace_floats=1 << 40), dict(sa=68), dict(key_w=72)):
        keep = {k: getattr(a, k) for k in bad}
        for k, v in bad.items():
            setattr(a, k, v)
        assert lib.flexnet_attn_critic_forward(C.byref(a), None) == _lib.FLEXNET_EUNSUPPORTED, bad
        for k, v in keep.items():
            setattr(a, k, v)
    a.batch = 0
    assert lib.flexnet_attn_critic_forward(C.byref(a), None) == 0                    # nothing to do, nothing launched
    g = _lib.FlexAttnCriticBwdArgs()
    assert lib.flexnet_attn_critic_backward(None, None) == -1 and lib.flexnet_attn_critic_backward(C.byref(g), None) == -1
    for k in ("dq", "sa", "key", "val", "sel", "hc", "w", "key_w", "val_w", "g_direct", "g_other", "g_dl"):
        setattr(g, k, 64)
    for name in ("enc_w", "c1_w", "c2_w", "b1_w", "b2_w"):
        for i in range(8):
            getattr(g, name)[i] = 64
    g.batch, g.n_agents, g.obs_dim, g.act_dim = 0, 5, 144, 4
    assert lib.flexnet_attn_critic_backward(C.byref(g), None) == -1                  # actions mode without d_act
    g.d_act = 64
    assert lib.flexnet_attn_critic_backward(C.byref(g), None) == 0
    g.param_grads = 1
    assert lib.flexnet_attn_critic_backward(C.byref(g), None) == -1                  # parameters mode without its outputs
    for k in ("s", "hb", "sel_w", "dz_c", "dz_b", "dz_s", "d_sel", "d_key", "dz_v", "dz_sa", "d_c2_b", "d_b2_b", "workspace"):
        setattr(g, k, 64)
    assert lib.flexnet_attn_critic_backward(C.byref(g), None) == 0
    g.batch = 33
    g.workspace_floats = 19
    assert lib.flexnet_attn_critic_backward(C.byref(g), None) == -1                  # a short workspace (two tiles of five doubles)
    g.workspace_floats, g.workspace = 20, 68
    assert lib.flexnet_attn_critic_backward(C.byref(g), None) == _lib.FLEXNET_EUNSUPPORTED      # ... of doubles
    g.batch, g.workspace = 0, 64
    g.dz_v = 68
    assert lib.flexnet_attn_critic_backward(C.byref(g), None) == _lib.FLEXNET_EUNSUPPORTED
    g.dz_v, g.n_agents = 64, 9
    assert lib.flexnet_attn_critic_backward(C.byref(g), None) == _lib.FLEXNET_EUNSUPPORTED


def test_attn_critic_kernels_have_no_scratch():
    from safe_marl_amd import build
    build.build()
    ks = build.kernel_resources("attn_critic")
    names = {v["name"] for v in ks.values()}
    assert names == {"attn_critic_forward_kernel", "attn_critic_reg_kernel", "attn_critic_backward_kernel<true>",
                     "attn_critic_backward_kernel<false>", "attn_critic_dq_sum_kernel"}
    for v in ks.values():
        print("attn_critic resources", v["name"], {k: v.get(k) for k in ("vgprs", "agprs", "sgprs", "waves_per_simd",
                                                                          "lds_bytes_per_block", "scratch_bytes_per_lane",
                                                                          "vgpr_spills", "sgpr_spills")})
        assert v.get("scratch_bytes_per_lane", 0) == 0 and v.get("vgpr_spills", 0) == 0 and v.get("sgpr_spills", 0) == 0


def test_the_example_takes_alg_maac():
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    try:
        import train_maddpg
    finally:
        sys.path.pop(0)
    assert train_maddpg.MAAC_ALG_ARGS == dict(policy_lrate=1.0e-4, value_lrate=1.0e-4, attend_heads=1, norm_in=False, soft=True,
                                              reward_scale=100, gaussian_policy=True, action_enforcebound=True)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "train_maddpg.py"), "--alg", "maac", "--unshared",
                          "--alg", "matd3"], capture_output=True, text=True)
    assert out.returncode == 2 and "MATD3 is built for shared_params" in out.stderr       # (the refusal, before any import)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "train_maddpg.py"), "--alg", "maacx"],
                         capture_output=True, text=True)
    assert out.returncode == 2 and "'maac'" in out.stderr                                   # maac is among the choices
    from safe_marl_amd.learner import MAAC
    from safe_marl_amd.util import convert
    alg = dict(train_maddpg.DEFAULT_ALG_ARGS)
    alg.update(train_maddpg.MAAC_ALG_ARGS)
    alg.update(alg="maac", agent_num=3, obs_size=144, state_size=106, action_dim=4, cuda=False)
    assert MAAC(convert(alg)).value(th.zeros(2, 3, 144), th.zeros(2, 3, 4)).shape == (3, 3)


def test_the_gpu_tests_small_shapes_have_no_tie():
    """tests/test_attn_critic_gpu.py asserts zero cleared samples below 100 samples: its seeds, checked here without a GPU."""
    from . import test_attn_critic_gpu as gpu_tests
    gpu_tests.test_the_seeds_have_no_tie()
