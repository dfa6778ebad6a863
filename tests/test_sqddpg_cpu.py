"""SQDDPG (madrl/models/sqddpg.py) on CPU against golden vectors captured by importing the reference's own modules
(tests/golden/make_sqddpg_golden.py), with the reference's coalition draws replayed by role; the coalition mapping on
hand-picked permutations; the C ABI's argument checks of flexnet_sqddpg_*; the kernels' resources; two ranks on gloo."""
import ctypes as C
import os

import numpy as np
import pytest
import torch as th

from .golden_io import StubEnv, _free_port, golden_args, golden_batch, golden_model, golden_tensors, golden_vectors

PREFIXES = ["sqddpg", "sqddpg3"]
ROLES = ("policy", "value", "target")


def _replay(model, gold, label, roles=ROLES):
    src = {r: th.from_numpy(gold[f"pos.{label}.{r}"]) for r in roles}
    model.coalition_source = lambda role, groups: src[role]


def test_state_dict_keys_and_class_wiring():
    from safe_marl_amd.learner import IDDPG, MADDPG, SQDDPG
    for prefix in PREFIXES:
        args = golden_args(prefix)
        ref = golden_tensors(f"{prefix}_state_dict.npz")
        sd = SQDDPG(args, SQDDPG(args)).state_dict()
        assert sorted(sd) == sorted(ref)
        assert all(tuple(sd[k].shape) == tuple(v.shape) for k, v in ref.items())
        assert sorted(SQDDPG(args).state_dict()) == sorted(MADDPG(args).state_dict())
    assert SQDDPG.get_actions is IDDPG.get_actions
    assert SQDDPG.bootstrap_cacheable is False and SQDDPG.graph_safe_updates is False
    m = SQDDPG(golden_args("sqddpg"))
    assert m.reads_state_in_place(32768) is False and m.reads_next_state_in_place(32768) is False
    import safe_marl_amd
    assert safe_marl_amd.SQDDPG is SQDDPG


def test_coalition_mapping_on_hand_picked_permutations():
    """pos[g, i] is agent i's position; the agent at position p is gc[g, p]; row i holds the actions of positions
    0..pos[g, i] in coalition order, agent i's own in block pos[g, i]."""
    from safe_marl_amd.learner import SQDDPG
    args = golden_args("sqddpg3")._replace(sample_size=2)
    m = SQDDPG(args)
    pos = th.tensor([[2, 0, 1], [0, 1, 2]])                                   # one sample, two coalitions
    sub, grand, ind = m.coalition_maps(pos, 1)
    assert grand[0, 0, 0].tolist() == [1, 2, 0] and grand[0, 1, 0].tolist() == [0, 1, 2]
    assert all(th.equal(grand[0, s, i], grand[0, s, 0]) for s in range(2) for i in range(3))
    assert sub[0, 0].tolist() == [[1, 1, 1], [1, 0, 0], [1, 1, 0]]
    assert sub[0, 1].tolist() == [[1, 0, 0], [1, 1, 0], [1, 1, 1]]
    assert ind[0, 0].tolist() == [[0, 0, 1], [1, 0, 0], [0, 1, 0]]
    # the composed rows: fc1 of row (s, i) equals z_shared + W_id[:, i] + sum_{j: pos_j <= pos_i} W_act[:, block pos_j] act_j
    th.manual_seed(0)
    n, o, a = 3, m.obs_dim, m.act_dim
    obs, act = th.randn(1, n, o), th.randn(1, n, a)
    net = m.value_dicts[0]
    seen = []
    net.fc1.register_forward_hook(lambda mod, inp, out: seen.append(out.detach()))
    m.marginal_contribution_torch(obs, act, pos)
    z1 = seen[-1].view(2, n, -1)
    W, bias = net.fc1.weight.detach(), net.fc1.bias.detach()
    W_obs, W_act, W_id = W[:, :n * o], W[:, n * o:n * o + n * a], W[:, n * o + n * a:]
    for s in range(2):
        for i in range(n):
            want = W_obs @ obs.reshape(-1) + bias + W_id[:, i]
            for j in range(n):
                if pos[s, j] <= pos[s, i]:
                    p = int(pos[s, j])
                    want = want + W_act[:, p * a:(p + 1) * a] @ act[0, j]
            assert th.allclose(z1[s, i], want, atol=1e-5), (s, i)
    # only agent i's own action reaches row i's gradient
    act_g = act.clone().requires_grad_(True)
    v = m.marginal_contribution_torch(obs, act_g, pos)
    (g,) = th.autograd.grad(v[0, :, 1].sum(), [act_g])
    assert th.count_nonzero(g[0, 0]) == 0 and th.count_nonzero(g[0, 2]) == 0 and th.count_nonzero(g[0, 1]) > 0


@pytest.mark.parametrize("prefix", PREFIXES)
def test_value_phi_losses_and_grads_match_the_reference(prefix):
    args = golden_args(prefix)
    gold = golden_vectors(prefix)
    model = golden_model("SQDDPG", args, f"{prefix}_state_dict.npz")
    batch = golden_batch(prefix)
    n = args.agent_num
    _replay(model, gold, "call", ("value", "target"))
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
    _replay(model, gold, "loss")
    pl, vl, _ = model.get_loss(batch)
    assert abs(vl.item() - float(gold["value_loss"])) < 1e-5 * max(1.0, abs(float(gold["value_loss"])))
    assert abs(pl.item() - float(gold["policy_loss"])) < 1e-6
    grads = th.autograd.grad(vl, list(model.value_dicts.parameters()), retain_graph=True)
    for (k, _), g in zip(model.value_dicts.named_parameters(), grads):
        assert np.allclose(g.numpy(), gold["vgrad." + k], atol=1e-5, rtol=1e-4), k
    grads = th.autograd.grad(pl, list(model.policy_dicts.parameters()))
    for (k, _), g in zip(model.policy_dicts.named_parameters(), grads):
        assert np.allclose(g.numpy(), gold["pgrad." + k], atol=1e-6, rtol=1e-4), k
    # the split forms draw by role: the same losses
    _, vl2, _ = model.get_loss(batch, need="value")
    pl2, _, _ = model.get_loss(batch, need="policy")
    assert abs(vl2.item() - vl.item()) < 1e-6 * max(1.0, abs(vl.item())) and abs(pl2.item() - pl.item()) < 1e-7


@pytest.mark.parametrize("prefix", PREFIXES)
def test_trainer_steps_and_target_update_match_the_reference(prefix):
    from safe_marl_amd.learner import SQDDPG
    from safe_marl_amd.trainer import PGTrainer
    args = golden_args(prefix)
    gold = golden_vectors(prefix)
    trainer = PGTrainer(args, SQDDPG, StubEnv(args.agent_num), None)
    sd = golden_tensors(f"{prefix}_state_dict.npz")
    trainer.behaviour_net.load_state_dict(sd)
    trainer.behaviour_net.target_net.load_state_dict({k[len("target_net."):]: v for k, v in sd.items()
                                                       if k.startswith("target_net.")})
    batch = golden_batch(prefix)
    stat = {}
    _replay(trainer.behaviour_net, gold, "vstep")
    trainer.value_transition_process(stat, batch)
    _replay(trainer.behaviour_net, gold, "pstep")
    trainer.policy_transition_process(stat, batch)
    for k in ("mean_train_value_loss", "mean_train_policy_loss", "mean_train_value_grad_norm",
              "mean_train_policy_grad_norm"):
        ref = gold["stat." + k]
        assert abs(float(stat[k]) - ref) < 1e-4 * max(1.0, abs(ref)), k
    cur = trainer.behaviour_net.state_dict()
    for k, v in golden_tensors(f"{prefix}_state_dict_after_step.npz").items():
        assert np.allclose(cur[k].numpy(), v.numpy(), atol=2e-5), k
    trainer.behaviour_net.update_target()
    tsd = trainer.behaviour_net.target_net.state_dict()
    for k, v in golden_tensors(f"{prefix}_target_after_update.npz").items():
        assert np.allclose(tsd[k].numpy(), v.numpy(), atol=2e-5), k


def test_sqddpg_abi_rejects_bad_arguments_before_any_device_work():
    from safe_marl_amd import build, _lib
    build.build()
    lib = _lib.load()
    assert lib.flexnet_sqddpg_forward(None, None) == -1
    assert lib.flexnet_sqddpg_backward(None, None) == -1
    assert lib.flexnet_sqddpg_draw(None, None) == -1
    assert C.sizeof(_lib.FlexSqddpgArgs) == 8 + 6 * 4 + 27 * 8
    assert C.sizeof(_lib.FlexSqddpgDrawArgs) == 8 + 2 * 4 + 2 * 8
    d = _lib.FlexSqddpgDrawArgs()
    d.groups, d.n_agents = 10, 5
    assert lib.flexnet_sqddpg_draw(C.byref(d), None) == -1                   # null tensors
    d.rng_state, d.pos, d.n_agents = 1 << 20, 1 << 20, 9
    assert lib.flexnet_sqddpg_draw(C.byref(d), None) == _lib.FLEXNET_EUNSUPPORTED
    a = _lib.FlexSqddpgArgs()
    a.batch, a.n_agents, a.act_dim, a.sample_size, a.layernorm = 64, 5, 4, 10, 1
    assert lib.flexnet_sqddpg_forward(C.byref(a), None) == -1                # null tensors
    for k in _lib.SQDDPG_PTRS:                                               # 16-byte aligned fake addresses: never read
        setattr(a, k, 1 << 20)
    a.want_param_grads = 1
    for field, bad in (("n_agents", 9), ("n_agents", 0), ("act_dim", 9), ("act_dim", 7), ("sample_size", 0),
                       ("sample_size", 1000)):
        b = _lib.FlexSqddpgArgs.from_buffer_copy(a)
        setattr(b, field, bad)
        assert lib.flexnet_sqddpg_forward(C.byref(b), None) == _lib.FLEXNET_EUNSUPPORTED, (field, bad)
        assert lib.flexnet_sqddpg_backward(C.byref(b), None) == _lib.FLEXNET_EUNSUPPORTED, (field, bad)
    b = _lib.FlexSqddpgArgs.from_buffer_copy(a)
    b.z_shared = (1 << 20) + 4                                               # misaligned rows
    assert lib.flexnet_sqddpg_forward(C.byref(b), None) == _lib.FLEXNET_EUNSUPPORTED
    b = _lib.FlexSqddpgArgs.from_buffer_copy(a)
    b.workspace = None                                                       # parameter gradients asked for, nowhere to go
    assert lib.flexnet_sqddpg_backward(C.byref(b), None) == -1
    b = _lib.FlexSqddpgArgs.from_buffer_copy(a)
    b.d_phi = None
    assert lib.flexnet_sqddpg_backward(C.byref(b), None) == -1
    b.batch = -1
    assert lib.flexnet_sqddpg_forward(C.byref(b), None) == -1


def test_sqddpg_kernels_have_no_scratch():
    from safe_marl_amd import build
    build.build()
    ks = build.kernel_resources("sqddpg")
    names = {v["name"] for v in ks.values()}
    assert {"sqddpg_draw_kernel", "sqddpg_forward_kernel", "sqddpg_backward_kernel", "sqddpg_reduce_kernel"} <= names
    for v in ks.values():
        assert v.get("scratch_bytes_per_lane", 0) == 0 and v.get("vgpr_spills", 0) == 0


def _worker(rank, world, port, out):
    import torch.distributed as dist
    import safe_marl_amd  # noqa: F401
    from safe_marl_amd.learner import SQDDPG
    from safe_marl_amd.trainer import PGTrainer
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    args = golden_args("sqddpg")
    th.manual_seed(200 + rank)                    # different initial weights and coalitions per rank: rank 0's weights win
    trainer = PGTrainer(args, SQDDPG, StubEnv(5), None)
    w0 = th.cat([p.detach().reshape(-1) for p in trainer.behaviour_net.parameters()])
    full = golden_batch("sqddpg")
    lo, hi = (0, 16) if rank == 0 else (16, 32)
    batch = type(full)(*[f[lo:hi] for f in full])
    stat = {}
    trainer.value_transition_process(stat, batch)
    trainer.policy_transition_process(stat, batch)
    w1 = th.cat([p.detach().reshape(-1) for p in trainer.behaviour_net.parameters()])
    out[rank] = dict(w0=w0.numpy(), w1=w1.numpy(), g=float(stat["mean_train_value_grad_norm"]))
    dist.barrier()
    dist.destroy_process_group()


def test_two_gloo_ranks_stay_identical_after_a_step():
    import torch.multiprocessing as mp
    port = _free_port()
    mgr = mp.Manager()
    out = mgr.dict()
    mp.spawn(_worker, args=(2, port, out), nprocs=2, join=True)
    a, b = out[0], out[1]
    assert np.array_equal(a["w0"], b["w0"])
    assert np.array_equal(a["w1"], b["w1"])
    assert not np.array_equal(a["w0"], a["w1"])
    assert a["g"] == b["g"]                                      # the all-reduced value gradient norm
