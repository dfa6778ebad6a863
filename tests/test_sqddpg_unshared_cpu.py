"""SQDDPG and FACMADDPG with ``shared_params: False`` without a GPU: the C ABI of flexnet_sqddpg_unshared_* (exports, struct
size, argument checks before any device work), the kernels' resources (the new ones under their own prefix, the existing ones as
the parent commit's build gave them), the CPU composition against the reference's own modules run with one network per agent
(tests/golden/make_sqddpg_unshared_golden.py, make_facmaddpg_unshared_golden.py), the host node that forms z_shared, and the
rules of the FLEX_UNSHARED_CRITICS switch."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch as th

from .golden_io import G, StubEnv, facmaddpg_state_dict, golden_args, golden_batch, golden_model, golden_tensors, golden_vectors

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SQ, FAC = "sqddpg_unshared3", "facmaddpg_unshared3"
ROLES = ("policy", "value", "target")
SWITCH = "FLEX_UNSHARED_CRITICS"
EINVAL = -1                      # include/flexnet.h: FLEXNET_EINVAL


def sq_state_dict(name="state_dict", device="cpu"):
    """The behaviour net's keys and the target replica's (``<name>_target.npz``) as one state_dict."""
    sd = golden_tensors(f"{SQ}_{name}.npz", device)
    if os.path.exists(os.path.join(G, f"{SQ}_{name}_target.npz")):
        sd.update(golden_tensors(f"{SQ}_{name}_target.npz", device))
    return sd


def fac_state_dict(name="state_dict", device="cpu", target_mixer=False):
    sd = facmaddpg_state_dict(FAC, name, device, target_mixer=target_mixer)
    if os.path.exists(os.path.join(G, f"{FAC}_{name}_target.npz")):
        sd.update(golden_tensors(f"{FAC}_{name}_target.npz", device))
    return sd


def replay(model, gold, label, roles=ROLES, device="cpu"):
    src = {r: th.from_numpy(gold[f"pos.{label}.{r}"]).to(device) for r in roles}
    model.coalition_source = lambda role, groups: src[role]


# ---- the C ABI ----------------------------------------------------------------------------------------------------------------
def _lib():
    from safe_marl_amd import build, _lib
    build.build()
    return _lib.load(), _lib


def _valid_args(L):
    """Every tensor and table entry a fake 16-byte aligned address: the checks never read them."""
    a = L.FlexSqddpgUnsharedArgs()
    a.batch, a.n_agents, a.act_dim, a.sample_size, a.layernorm, a.ld_fc1 = 64, 5, 4, 10, 1, 745
    for k in ("z_shared", "act", "pos") + L.SQDDPG_UNSHARED_PTRS:
        setattr(a, k, 1 << 20)
    for k in L.SQDDPG_UNSHARED_TABLES:
        for i in range(5):
            getattr(a, k)[i] = 1 << 20
    a.want_param_grads = 1
    return a


def test_entry_points_are_exported_and_the_struct_matches_the_header():
    lib, L = _lib()
    for name in ("flexnet_sqddpg_unshared_forward", "flexnet_sqddpg_unshared_backward"):
        assert hasattr(lib, name) and name in L.SYMBOLS
    # int64 batch, 6 x 4 bytes, int64 ld_fc1, 3 pointers, 8 tables of FLEXNET_MAX_AGENTS pointers, 15 pointers
    assert C.sizeof(L.FlexSqddpgUnsharedArgs) == 8 + 6 * 4 + 8 + 3 * 8 + 8 * 8 * 8 + 15 * 8
    hdr = open(os.path.join(ROOT, "include", "flexnet.h")).read()
    assert f"#define FLEXNET_SQDDPG_UNSHARED_WS_ROW {L.FLEXNET_SQDDPG_UNSHARED_WS_ROW}\n" in hdr
    assert f"#define FLEXNET_SQDDPG_UNSHARED_BWD_GRID {L.FLEXNET_SQDDPG_UNSHARED_BWD_GRID}\n" in hdr
    body = hdr[hdr.index("typedef struct {", hdr.index("FLEXNET_SQDDPG_UNSHARED_BWD_GRID 256")):hdr.index("} FlexSqddpgUnsharedArgs;")]
    fields = [ln.split(";")[0].split()[-1].lstrip("*").split("[")[0] for ln in body.splitlines() if ";" in ln]
    assert fields == [f[0] for f in L.FlexSqddpgUnsharedArgs._fields_]


def test_bad_arguments_are_rejected_before_any_device_work():
    """A NULL stream and no device: every answer below comes from the checks alone."""
    lib, L = _lib()
    fwd, bwd = lib.flexnet_sqddpg_unshared_forward, lib.flexnet_sqddpg_unshared_backward
    assert fwd(None, None) == EINVAL and bwd(None, None) == EINVAL
    a = L.FlexSqddpgUnsharedArgs()
    a.batch, a.n_agents, a.act_dim, a.sample_size, a.layernorm, a.ld_fc1 = 64, 5, 4, 10, 1, 745
    assert fwd(C.byref(a), None) == EINVAL                           # null tensors
    a = _valid_args(L)

    def both(mutate, want):
        b = L.FlexSqddpgUnsharedArgs.from_buffer_copy(a)
        mutate(b)
        assert fwd(C.byref(b), None) == want and bwd(C.byref(b), None) == want

    for table in L.SQDDPG_UNSHARED_TABLES:                                     # a NULL table entry of an agent that exists
        both(lambda b, t=table: getattr(b, t).__setitem__(4, None), EINVAL)
    both(lambda b: setattr(b, "batch", -1), EINVAL)
    both(lambda b: setattr(b, "z_shared", None), EINVAL)
    both(lambda b: setattr(b, "ld_fc1", 19), EINVAL)                 # narrower than the action columns
    for field, bad in (("n_agents", 9), ("n_agents", 0), ("act_dim", 9), ("act_dim", 0), ("act_dim", 7), ("sample_size", 0),
                       ("sample_size", 1000)):
        both(lambda b, f=field, v=bad: setattr(b, f, v), L.FLEXNET_EUNSUPPORTED)

    def n_a_33(b):                                                             # n a = 33
        b.n_agents, b.act_dim = 3, 11
    both(n_a_33, L.FLEXNET_EUNSUPPORTED)
    both(lambda b: b.fc2_w.__setitem__(2, (1 << 20) + 4), L.FLEXNET_EUNSUPPORTED)      # a misaligned fc2_w
    both(lambda b: setattr(b, "z_shared", (1 << 20) + 8), L.FLEXNET_EUNSUPPORTED)
    # a table entry past n_agents may be NULL; without LayerNorm so may its tables
    b = _valid_args(L)
    b.n_agents, b.layernorm, b.batch = 4, 0, 0
    for t in L.SQDDPG_UNSHARED_TABLES:
        getattr(b, t)[4] = None
    b.ln_w[0] = b.ln_b[1] = None
    assert fwd(C.byref(b), None) == 0 and bwd(C.byref(b), None) == 0     # (batch 0: nothing launched)
    # the forward wants an output, the backward its upstream gradient and somewhere for the parameter gradients to go
    b = _valid_args(L)
    b.q = b.phi = None
    assert fwd(C.byref(b), None) == EINVAL
    for k in ("d_phi", "workspace", "d_w_act", "d_fc3_b"):
        b = _valid_args(L)
        setattr(b, k, None)
        assert bwd(C.byref(b), None) == EINVAL, k


# ---- resources ------------------------------------------------------------------------------------------------------------------
FIELDS = ("vgprs", "agprs", "sgprs", "sgpr_spills", "vgpr_spills", "scratch_bytes_per_lane", "lds_bytes_per_block", "waves_per_simd")
# a build of the parent commit with the compiler that built this tree (profiles/sqddpg_unshared.txt has both builds)
PARENT = {
    "critic_unshared_backward_kernel<false>": (148, 48, 50, 0, 0, 0, 36608, 2),
    "critic_unshared_backward_kernel<true>": (256, 151, 62, 0, 0, 0, 36608, 1),
    "critic_unshared_forward_kernel": (155, 32, 32, 0, 0, 0, 0, 2),
    "critic_unshared_reduce_kernel": (20, 0, 35, 0, 0, 0, 4096, 8),
    "sqddpg_backward_kernel": (256, 200, 106, 21, 0, 0, 31616, 1),
    "sqddpg_draw_kernel": (10, 0, 27, 0, 0, 0, 0, 8),
    "sqddpg_forward_kernel": (110, 32, 78, 0, 0, 0, 384, 3),
    "sqddpg_reduce_kernel": (22, 0, 30, 0, 0, 0, 4096, 8),
}


def test_the_new_kernels_have_their_own_prefix_and_do_not_spill():
    from safe_marl_amd import build
    build.build()
    ks = {v["name"]: v for v in build.kernel_resources("agent_sqddpg").values()}
    assert set(ks) == {"agent_sqddpg_forward_kernel", "agent_sqddpg_backward_kernel<true>", "agent_sqddpg_backward_kernel<false>",
                       "agent_sqddpg_reduce_kernel"}
    for name, v in ks.items():
        print(name, {f: v[f] for f in FIELDS})
        assert v["scratch_bytes_per_lane"] == 0 and v["vgpr_spills"] == 0 and v["sgpr_spills"] == 0, (name, v)
    assert ks["agent_sqddpg_backward_kernel<true>"]["lds_bytes_per_block"] * 4 <= 160 * 1024      # four work-groups per CU
    # build.kernel_resources("sqddpg") keeps naming the shared critic's four kernels only
    assert {v["name"] for v in build.kernel_resources("sqddpg").values()} == \
        {"sqddpg_draw_kernel", "sqddpg_forward_kernel", "sqddpg_backward_kernel", "sqddpg_reduce_kernel"}


def test_the_existing_kernels_are_what_the_parent_commit_built():
    from safe_marl_amd import build
    build.build()
    got = {}
    for prefix in ("sqddpg_", "critic_unshared"):
        got.update({v["name"]: tuple(v[f] for f in FIELDS) for v in build.kernel_resources(prefix).values()})
    assert got == PARENT


# ---- the CPU composition against the reference with one network per agent ----------------------------------------------------------
def test_sqddpg_state_dict_keys_are_the_reference_s():
    from safe_marl_amd.learner import SQDDPG
    args = golden_args(SQ)
    assert args.shared_params is False and args.agent_num == 3
    ref = sq_state_dict()
    sd = SQDDPG(args, SQDDPG(args)).state_dict()
    assert sorted(sd) == sorted(ref) and all(tuple(sd[k].shape) == tuple(v.shape) for k, v in ref.items())
    assert sum(k.startswith("value_dicts.") and k.endswith("fc1.weight") for k in sd) == 3
    for f in os.listdir(G):                                                   # no new fixture above the tree's largest one
        if f.startswith((SQ, FAC)):
            assert os.path.getsize(os.path.join(G, f)) <= 1482460, f


def test_sqddpg_value_phi_losses_and_grads_match_the_reference():
    args = golden_args(SQ)
    gold = golden_vectors(SQ)
    model = golden_model("SQDDPG", args, sq_state_dict())
    batch = golden_batch(SQ)
    n = args.agent_num
    replay(model, gold, "call", ("value", "target"))
    with th.no_grad():
        v = model.value(batch.state, batch.action)
        assert np.allclose(v.numpy(), gold["value"], atol=1e-6)
        phi = v.mean(1).view(-1, n)
        assert np.allclose(phi.numpy(), gold["phi"], atol=1e-6)
        assert np.allclose(phi.sum(-1).numpy(), gold["S"], atol=1e-5)
        _, na, _, _, _ = model.get_actions(batch.next_state, status="train", exploration=False,
                                           actions_avail=batch.action_avail, target=False, last_hid=batch.hid)
        nphi, _ = model.target_net.shapley_values(batch.next_state, na, model.draw_coalitions("target", 32, na.device))
        assert np.allclose(nphi.sum(-1).numpy(), gold["S_next"], atol=1e-5)
    replay(model, gold, "loss")
    pl, vl, _ = model.get_loss(batch)
    assert abs(vl.item() - float(gold["value_loss"])) < 1e-5 * max(1.0, abs(float(gold["value_loss"])))
    assert abs(pl.item() - float(gold["policy_loss"])) < 1e-6
    names = [k for k, _ in model.value_dicts.named_parameters()]
    assert len(names) == 8 * n
    for k, g in zip(names, th.autograd.grad(vl, list(model.value_dicts.parameters()), retain_graph=True)):
        assert np.allclose(g.numpy(), gold["vgrad." + k], atol=1e-5, rtol=1e-4), k
    for (k, _), g in zip(model.policy_dicts.named_parameters(), th.autograd.grad(pl, list(model.policy_dicts.parameters()))):
        assert np.allclose(g.numpy(), gold["pgrad." + k], atol=1e-6, rtol=1e-4), k
    # critic i's id columns k != i never meet a 1: exactly zero
    no = n * args.obs_size + n * args.action_dim
    for i in range(n):
        gid = gold[f"vgrad.{i}.fc1.weight"][:, no:]
        assert all(np.count_nonzero(gid[:, k]) == 0 for k in range(n) if k != i) and np.count_nonzero(gid[:, i]) > 0


def test_sqddpg_trainer_steps_and_target_update_match_the_reference():
    from safe_marl_amd.learner import SQDDPG
    from safe_marl_amd.trainer import PGTrainer
    args = golden_args(SQ)
    gold = golden_vectors(SQ)
    trainer = PGTrainer(args, SQDDPG, StubEnv(args.agent_num), None)
    sd = sq_state_dict()
    trainer.behaviour_net.load_state_dict(sd)
    trainer.behaviour_net.target_net.load_state_dict({k[len("target_net."):]: v for k, v in sd.items() if k.startswith("target_net.")})
    batch = golden_batch(SQ)
    stat = {}
    replay(trainer.behaviour_net, gold, "vstep")
    trainer.value_transition_process(stat, batch)
    replay(trainer.behaviour_net, gold, "pstep")
    trainer.policy_transition_process(stat, batch)
    for k in ("mean_train_value_loss", "mean_train_policy_loss", "mean_train_value_grad_norm", "mean_train_policy_grad_norm"):
        ref = gold["stat." + k]
        assert abs(float(stat[k]) - ref) < 1e-4 * max(1.0, abs(ref)), k
    cur = trainer.behaviour_net.state_dict()
    for k, v in sq_state_dict("state_dict_after_step").items():
        assert np.allclose(cur[k].numpy(), v.numpy(), atol=2e-5), k
    trainer.behaviour_net.update_target()
    tsd = trainer.behaviour_net.target_net.state_dict()
    for k, v in golden_tensors(f"{SQ}_target_after_update.npz").items():
        assert np.allclose(tsd[k].numpy(), v.numpy(), atol=2e-5), k


def test_facmaddpg_values_losses_and_grads_match_the_reference():
    args = golden_args(FAC)
    assert args.shared_params is False
    gold = golden_vectors(FAC)
    mgold = dict(np.load(os.path.join(G, FAC + "_golden_mixer_grads.npz")))
    model = golden_model("FACMADDPG", args, fac_state_dict(target_mixer=True))
    batch = golden_batch(FAC)
    n, o = args.agent_num, args.obs_size
    with th.no_grad():
        v = model.value(batch.state, batch.action)
        assert np.allclose(v.numpy(), gold["value"], atol=1e-5)
        b = batch.state.shape[0]
        q_tot = model.mixer(v.view(-1, n), batch.state.reshape(b, n * o)).view(-1, 1)
        assert np.allclose(q_tot.numpy(), gold["q_tot"], atol=1e-4, rtol=1e-5)
        _, na, _, _, _ = model.get_actions(batch.next_state, status="train", exploration=False,
                                           actions_avail=batch.action_avail, target=False, last_hid=batch.hid)
        nv = model.target_net.value(batch.next_state, na).view(-1, n)
        nq = model.target_net.mixer(nv, batch.next_state.reshape(b, n * o)).view(-1, 1)
        assert np.allclose(nq.numpy(), gold["next_q_tot"], atol=1e-4, rtol=1e-5)
    pl, vl, _ = model.get_loss(batch)
    assert abs(vl.item() - float(gold["value_loss"])) < 1e-4 * max(1.0, abs(float(gold["value_loss"])))
    assert abs(pl.item() - float(gold["policy_loss"])) < 1e-5
    crit, mix = list(model.value_dicts.parameters()), list(model.mixer.parameters())
    gr = th.autograd.grad(vl, crit + mix, retain_graph=True)
    for (k, _), g in zip(model.value_dicts.named_parameters(), gr[:len(crit)]):
        assert np.allclose(g.numpy(), gold["vgrad." + k], atol=1e-4, rtol=1e-4), k
    for (k, _), g in zip(model.mixer.named_parameters(), gr[len(crit):]):
        assert np.allclose(g.numpy(), mgold["mgrad." + k], atol=1e-4, rtol=1e-4), k
    for (k, _), g in zip(model.policy_dicts.named_parameters(), th.autograd.grad(pl, list(model.policy_dicts.parameters()))):
        assert np.allclose(g.numpy(), gold["pgrad." + k], atol=1e-5, rtol=1e-4), k


def test_facmaddpg_trainer_steps_and_target_update_match_the_reference():
    from safe_marl_amd.learner import FACMADDPG
    from safe_marl_amd.trainer import PGTrainer
    args = golden_args(FAC)
    gold = golden_vectors(FAC)
    trainer = PGTrainer(args, FACMADDPG, StubEnv(args.agent_num), None)
    sd = fac_state_dict(target_mixer=True)
    trainer.behaviour_net.load_state_dict(sd)
    trainer.behaviour_net.target_net.load_state_dict({k[len("target_net."):]: v for k, v in sd.items() if k.startswith("target_net.")})
    batch = golden_batch(FAC)
    stat = {}
    trainer.value_transition_process(stat, batch)
    trainer.policy_transition_process(stat, batch)
    trainer.mixer_transition_process(stat, batch)
    for k in ("mean_train_value_loss", "mean_train_policy_loss", "mean_train_mixer_loss", "mean_train_value_grad_norm",
              "mean_train_policy_grad_norm", "mean_train_mixer_grad_norm"):
        ref = gold["stat." + k]
        assert abs(float(stat[k]) - ref) < 1e-4 * max(1.0, abs(ref)), k
    cur = trainer.behaviour_net.state_dict()
    for k, v in fac_state_dict("state_dict_after_step").items():
        assert np.allclose(cur[k].numpy(), v.numpy(), atol=2e-5), k
    trainer.behaviour_net.update_target()
    tsd = trainer.behaviour_net.target_net.state_dict()
    tgt = facmaddpg_state_dict(FAC, "target_after_update")
    for k, v in tgt.items():
        assert np.allclose(tsd[k].numpy(), v.numpy(), atol=2e-5), k
    assert any(k.startswith("mixer.") for k in tgt)


# ---- the host node that forms z_shared ------------------------------------------------------------------------------------------
def test_z_shared_node_is_the_per_agent_first_layer_on_the_observation_columns():
    """nets._SqddpgZSharedFn on the CPU (its library-GEMM branch): z_shared[:, i] = obs2d @ W_i[:, :no].T + b_i, and the
    gradients of every fc1.weight (full width, zero outside the observation columns), every fc1.bias and obs2d."""
    from safe_marl_amd.nets import _SqddpgZSharedFn
    th.manual_seed(3)
    b, n, no, ld = 9, 3, 10, 17
    obs = th.randn(b, no, dtype=th.float64, requires_grad=True)
    ws = [th.randn(64, ld, dtype=th.float64, requires_grad=True) for _ in range(n)]
    bs = [th.randn(64, dtype=th.float64, requires_grad=True) for _ in range(n)]
    up = th.randn(b, n, 64, dtype=th.float64)
    z = _SqddpgZSharedFn.apply(obs, no, *[t for pair in zip(ws, bs) for t in pair])
    want = th.stack([obs @ w[:, :no].t() + c for w, c in zip(ws, bs)], 1)
    assert z.shape == (b, n, 64) and th.allclose(z, want, atol=1e-12)
    got = th.autograd.grad((z * up).sum(), [obs] + ws + bs)
    ref = th.autograd.grad((want * up).sum(), [obs] + ws + bs)
    for g, r in zip(got, ref):
        assert g.shape == r.shape and th.allclose(g, r, atol=1e-11)
    assert all(th.count_nonzero(g[:, no:]) == 0 for g in got[1:1 + n])


def test_ordered_floor_is_fp64_budget_s_ordered_sum_rounding():
    """tests/sqddpg_unshared_floor.py's ``ordered_floor`` (cumulative sums) against fb.ordered_sum_rounding's loop over the
    runs it stands for: one run per sample, the sample's ns rows."""
    from . import fp64_budget as fb
    from .sqddpg_unshared_floor import ordered_floor
    g = th.Generator().manual_seed(4)
    for b, ns, shape in ((7, 1, (64,)), (9, 3, (64,)), (5, 10, (1,)), (6, 4, (2, 3))):
        x = th.randn(b * ns, *shape, generator=g, dtype=th.float64) + 0.3
        runs = x.view(b, ns, *shape)
        want = fb.ordered_sum_rounding([(ns, runs[j].mean(0), runs[j].var(0, unbiased=False)) for j in range(b)])
        assert th.allclose(ordered_floor(x, ns), want, rtol=1e-12, atol=0)
    # a sum that cancels, of rows that repeat within a sample (a shared d_phi): partial sums, and the floor, above the
    # exchangeable form's
    d = th.randn(64, 1, generator=g, dtype=th.float64)
    d = (d - d.mean()).repeat_interleave(10, 0)
    assert float(ordered_floor(d, 10)) > float(fb.row_sum_rounding(d))


# ---- the switch -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("value", [None, "1"])
def test_the_switch_leaves_the_pinned_defaults_alone(value, monkeypatch):
    """Set or unset: the class flags other tests pin stay as they are, and SQDDPG._fused keeps its meaning."""
    import safe_marl_amd.learner as L
    from safe_marl_amd import nets
    if value is None:
        monkeypatch.delenv(SWITCH, raising=False)
    else:
        monkeypatch.setenv(SWITCH, value)
    assert nets.unshared_critics_switch() is (value == "1")                   # read at every call
    assert all(getattr(L, c).unshared_critic_kernel for c in ("MADDPG", "SAFEMADDPG", "IDDPG", "IPPO", "MAPPO"))
    assert not any(getattr(L, c).unshared_critic_kernel for c in ("FACMADDPG", "SQDDPG", "COMA", "MATD3"))
    assert not any(hasattr(getattr(L, c), "unshared_twin_kernel") for c in ("MADDPG", "IDDPG", "FACMADDPG", "SQDDPG", "COMA"))
    assert L.FACMADDPG.graph_safe_updates is False and L.SQDDPG.graph_safe_updates is False
    assert [c for c in ("MADDPG", "IDDPG", "FACMADDPG", "SQDDPG", "COMA", "MATD3", "IPPO", "MAPPO")
            if getattr(L, c).unshared_critic_opt_in] == ["FACMADDPG"]
    m = L.SQDDPG(golden_args(SQ))
    assert not m._fused(th.zeros(2, 3, 4))                                    # CPU tensors: never fused, no note
    # on the CPU the switch changes nothing: the composition, and FACMADDPG's per-agent loop
    gold = golden_vectors(SQ)
    model = golden_model("SQDDPG", golden_args(SQ), sq_state_dict())
    batch = golden_batch(SQ)
    replay(model, gold, "call", ("value",))
    with th.no_grad():
        assert np.allclose(model.value(batch.state, batch.action).numpy(), gold["value"], atol=1e-6)
    fac = golden_model("FACMADDPG", golden_args(FAC), fac_state_dict(target_mixer=True))
    assert fac.unshared_values(batch.state, batch.action, False) is None


def test_switch_values_other_than_1_do_not_switch(monkeypatch):
    from safe_marl_amd import nets
    for v in ("", "0", "true", "2"):
        monkeypatch.setenv(SWITCH, v)
        assert not nets.unshared_critics_switch()


@pytest.mark.parametrize("extra", [[], ["--unshared", "--alg", "maddpg"], ["--alg", "sqddpg"], ["--unshared", "--alg", "coma"]])
def test_unshared_critics_flag_needs_unshared_and_one_of_the_two_algorithms(extra):
    """An ap.error (exit status 2, before anything is imported or built) unless --unshared and --alg sqddpg | facmaddpg."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "train_maddpg.py"), "--unshared-critics"] + extra,
                       capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 2 and "--unshared-critics" in r.stderr, r.stderr[-400:]
