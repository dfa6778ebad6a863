"""FACMADDPG (madrl/models/facmaddpg.py + madrl/critics/qmix.py) on CPU against golden vectors captured by importing the
reference's own modules (tests/golden/make_facmaddpg_golden.py), the update cadence with the mixer, the C ABI's argument
checks of flexnet_qmix_*, the kernels' resources and the two-rank path on gloo."""
import ctypes as C
import os

import numpy as np
import pytest
import torch as th

from .golden_io import (G, StubEnv, _free_port, facmaddpg_state_dict, golden_args, golden_batch, golden_model, golden_tensors,
                        golden_vectors)


PREFIXES = ["facmaddpg", "facmaddpg3"]


def test_mixer_state_dict_keys_match_the_reference():
    from safe_marl_amd.nets import QMIX_PARAMS
    for prefix in PREFIXES:
        args = golden_args(prefix)
        from safe_marl_amd.nets import QMixer
        mixer = QMixer(args)
        ref = golden_tensors(f"{prefix}_state_dict_mixer.npz")
        assert sorted("mixer." + k for k in mixer.state_dict()) == sorted(ref)
        assert sorted(QMIX_PARAMS) == sorted(mixer.state_dict())
        for k, v in mixer.state_dict().items():
            assert tuple(v.shape) == tuple(ref["mixer." + k].shape)
    n = sum(p.numel() for p in QMixer(golden_args("facmaddpg")).parameters())
    assert n == 209601                                               # 5 agents, S = 720


def test_init_weights_reach_the_mixer():
    from safe_marl_amd.learner import FACMADDPG
    args = golden_args("facmaddpg")
    th.manual_seed(0)
    m = FACMADDPG(args)
    w = m.mixer.hyper_w_1[0].weight.detach()
    assert abs(float(w.std()) - args.init_std) < 0.01 and abs(float(w.mean())) < 0.01


@pytest.mark.parametrize("prefix", PREFIXES)
def test_value_qtot_losses_and_grads(prefix):
    args = golden_args(prefix)
    gold = golden_vectors(prefix)
    mgold = dict(np.load(os.path.join(G, prefix + "_golden_mixer_grads.npz")))
    model = golden_model("FACMADDPG", args, facmaddpg_state_dict(prefix, target_mixer=True))
    batch = golden_batch(prefix)
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
    model = golden_model("FACMADDPG", args, facmaddpg_state_dict(prefix, target_mixer=True))
    pl, vl, _ = model.get_loss(batch)
    assert abs(vl.item() - float(gold["value_loss"])) < 1e-4 * max(1.0, abs(float(gold["value_loss"])))
    assert abs(pl.item() - float(gold["policy_loss"])) < 1e-5
    model.zero_grad()
    vl.backward()
    for k, p in model.value_dicts.named_parameters():
        assert np.allclose(p.grad.numpy(), gold["vgrad." + k], atol=1e-4, rtol=1e-4), k
    for k, p in model.mixer.named_parameters():
        assert np.allclose(p.grad.numpy(), mgold["mgrad." + k], atol=1e-4, rtol=1e-4), k
    pl2, _, _ = model.get_loss(batch)
    model.zero_grad()
    pl2.backward()
    for k, p in model.policy_dicts.named_parameters():
        assert np.allclose(p.grad.numpy(), gold["pgrad." + k], atol=1e-5, rtol=1e-4), k


@pytest.mark.parametrize("prefix", PREFIXES)
def test_split_losses_give_each_optimiser_the_reference_gradients(prefix):
    """need="value" differentiates the critic only, need="mixer" the mixer only: same loss, same gradients."""
    args = golden_args(prefix)
    mgold = dict(np.load(os.path.join(G, prefix + "_golden_mixer_grads.npz")))
    gold = golden_vectors(prefix)
    model = golden_model("FACMADDPG", args, facmaddpg_state_dict(prefix, target_mixer=True))
    batch = golden_batch(prefix)
    _, vl, _ = model.get_loss(batch, need="value")
    crit = list(model.value_dicts.parameters())
    mix = list(model.mixer.parameters())
    gr = th.autograd.grad(vl, crit + mix, allow_unused=True)
    assert all(g is None for g in gr[len(crit):])                  # the mixer takes nothing from a value step
    for (k, _), g in zip(model.value_dicts.named_parameters(), gr[:len(crit)]):
        assert np.allclose(g.numpy(), gold["vgrad." + k], atol=1e-4, rtol=1e-4), k
    _, ml, _ = model.get_loss(batch, need="mixer")
    assert abs(ml.item() - vl.item()) < 1e-5 * max(1.0, abs(vl.item()))
    gr = th.autograd.grad(ml, mix)
    for (k, _), g in zip(model.mixer.named_parameters(), gr):
        assert np.allclose(g.numpy(), mgold["mgrad." + k], atol=1e-4, rtol=1e-4), k


@pytest.mark.parametrize("prefix", PREFIXES)
def test_trainer_steps_value_policy_mixer_and_target_update(prefix):
    from safe_marl_amd.learner import FACMADDPG
    from safe_marl_amd.trainer import PGTrainer
    args = golden_args(prefix)
    gold = golden_vectors(prefix)
    trainer = PGTrainer(args, FACMADDPG, StubEnv(args.agent_num), None)
    sd = facmaddpg_state_dict(prefix, target_mixer=True)
    trainer.behaviour_net.load_state_dict(sd)
    trainer.behaviour_net.target_net.load_state_dict({k[len("target_net."):]: v for k, v in sd.items()
                                                       if k.startswith("target_net.")})
    assert trainer.mixer_optimizer.param_groups[0]["lr"] == args.mixer_lrate
    assert {id(p) for p in trainer.mixer_optimizer.param_groups[0]["params"]} == \
        {id(p) for p in trainer.behaviour_net.mixer.parameters()}
    batch = golden_batch(prefix)
    stat = {}
    trainer.value_transition_process(stat, batch)
    trainer.policy_transition_process(stat, batch)
    trainer.mixer_transition_process(stat, batch)
    for k in ("mean_train_value_loss", "mean_train_policy_loss", "mean_train_mixer_loss", "mean_train_value_grad_norm",
              "mean_train_policy_grad_norm", "mean_train_mixer_grad_norm"):
        ref = gold["stat." + k]
        assert abs(float(stat[k]) - ref) < 1e-4 * max(1.0, abs(ref)), k
    after = facmaddpg_state_dict(prefix, "state_dict_after_step")
    sd = trainer.behaviour_net.state_dict()
    for k, v in after.items():
        assert np.allclose(sd[k].numpy(), v.numpy(), atol=2e-5), k
    trainer.behaviour_net.update_target()
    tgt = facmaddpg_state_dict(prefix, "target_after_update")
    tsd = trainer.behaviour_net.target_net.state_dict()
    for k, v in tgt.items():
        assert np.allclose(tsd[k].numpy(), v.numpy(), atol=2e-5), k
    assert any(k.startswith("mixer.") for k in tgt)                # the soft update covers the mixer


def test_update_event_order_is_value_policy_mixer():
    from safe_marl_amd.learner import FACMADDPG
    args = golden_args("facmaddpg")._replace(value_update_epochs=2, policy_update_epochs=1, mixer_update_epochs=3,
                                             replay_warmup=0, behaviour_update_freq=1, target_update_freq=10 ** 9)
    model = FACMADDPG(args)

    class Buf:
        buffer = [0] * 1000

        def add_experience(self, t):
            pass

    class T:
        steps = 5
        replay_buffer = Buf()
        log = []

        def effective_batch_size(self):
            return 32

        def value_replay_process(self, stat):
            self.log.append("value")

        def policy_replay_process(self, stat):
            self.log.append("policy")

        def mixer_replay_process(self, stat):
            self.log.append("mixer")

    t = T()
    model.transition_update(t, None, {})
    assert t.log == ["value", "value", "policy", "mixer", "mixer", "mixer"]
    # models without a mixer keep their cadence
    from safe_marl_amd.learner import IDDPG
    t.log = []
    IDDPG(args._replace(mixer=False)).transition_update(t, None, {})
    assert t.log == ["value", "value", "policy"]


def test_qmix_abi_rejects_bad_arguments_before_any_device_work():
    from safe_marl_amd import build, _lib
    build.build()
    lib = _lib.load()
    assert lib.flexnet_qmix_forward(None, None) == -1
    assert lib.flexnet_qmix_backward(None, None) == -1
    assert C.sizeof(_lib.FlexQmixArgs) == 2 * 8 + 4 * 4 + 23 * 8
    a = _lib.FlexQmixArgs()
    a.batch, a.n_agents, a.state_dim, a.ld_state = 64, 5, 720, 720
    assert lib.flexnet_qmix_forward(C.byref(a), None) == -1             # null tensors
    assert lib.flexnet_qmix_backward(C.byref(a), None) == -1
    for k in _lib.QMIX_PTRS:                                             # 16-byte aligned fake addresses: never read
        setattr(a, k, 1 << 20)
    a.want_param_grads = 1
    for field, bad in (("n_agents", 9), ("n_agents", 0), ("state_dim", 728), ("state_dim", 1040), ("ld_state", 718)):
        b = _lib.FlexQmixArgs.from_buffer_copy(a)
        setattr(b, field, bad)
        assert lib.flexnet_qmix_forward(C.byref(b), None) == _lib.FLEXNET_EUNSUPPORTED, (field, bad)
    b = _lib.FlexQmixArgs.from_buffer_copy(a)
    b.state = (1 << 20) + 4                                              # misaligned rows
    assert lib.flexnet_qmix_forward(C.byref(b), None) == _lib.FLEXNET_EUNSUPPORTED
    b = _lib.FlexQmixArgs.from_buffer_copy(a)
    b.d_pre1 = None                                                      # parameter gradients asked for, nowhere to go
    assert lib.flexnet_qmix_backward(C.byref(b), None) == -1
    b.batch = -1
    assert lib.flexnet_qmix_forward(C.byref(b), None) == -1


def test_qmix_kernels_have_no_scratch():
    from safe_marl_amd import build
    build.build()
    ks = build.kernel_resources("qmix")
    names = {v["name"] for v in ks.values()} if isinstance(ks, dict) else {k["name"] for k in ks}
    assert {"qmix_forward_kernel", "qmix_backward_kernel"} <= names
    for v in (ks.values() if isinstance(ks, dict) else ks):
        assert v.get("scratch_bytes_per_lane", 0) == 0 and v.get("vgpr_spills", 0) == 0


def _worker(rank, world, port, out):
    import torch.distributed as dist
    import safe_marl_amd  # noqa: F401
    from safe_marl_amd.learner import FACMADDPG
    from safe_marl_amd.trainer import PGTrainer
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    args = golden_args("facmaddpg")
    th.manual_seed(200 + rank)                    # different initial weights per rank: rank 0's are broadcast
    trainer = PGTrainer(args, FACMADDPG, StubEnv(5), None)
    w0 = th.cat([p.detach().reshape(-1) for p in trainer.behaviour_net.parameters()])
    full = golden_batch("facmaddpg")
    lo, hi = (0, 16) if rank == 0 else (16, 32)
    batch = type(full)(*[f[lo:hi] for f in full])
    stat = {}
    trainer.value_transition_process(stat, batch)
    trainer.policy_transition_process(stat, batch)
    trainer.mixer_transition_process(stat, batch)
    w1 = th.cat([p.detach().reshape(-1) for p in trainer.behaviour_net.parameters()])
    out[rank] = dict(w0=w0.numpy(), w1=w1.numpy(), m0=float(stat["mean_train_mixer_grad_norm"]),
                     mix=th.cat([p.detach().reshape(-1) for p in trainer.behaviour_net.mixer.parameters()]).numpy())
    dist.barrier()
    dist.destroy_process_group()


def test_two_gloo_ranks_stay_identical_after_a_mixer_step():
    import torch.multiprocessing as mp
    port = _free_port()
    mgr = mp.Manager()
    out = mgr.dict()
    mp.spawn(_worker, args=(2, port, out), nprocs=2, join=True)
    a, b = out[0], out[1]
    assert np.array_equal(a["w0"], b["w0"])
    assert np.array_equal(a["w1"], b["w1"])
    assert not np.array_equal(a["w0"], a["w1"])
    assert a["m0"] == b["m0"]                                    # the all-reduced mixer gradient norm
