"""episodic: True (default.yaml:9) on CPU: the trainer constructs; episode_update fires on the reference's schedule and never
moves the target; EpisodeReplayBuffer draws and concatenates as the reference's does under the same NumPy seed; one value and
one policy sub-update through PGTrainer and the episodic buffer against the reference's (tests/golden/make_episodic_golden.py,
three agents, the bounds of tests/test_learner_cpu.py and tests/test_unshared_cpu.py); the vectorised ring's composition
equals ``slab_window`` row by row; the example's flag; flexnet_gather_episodes' argument checks, which need no GPU."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch as th

from .golden_io import G, StubEnv, golden_args, golden_model, golden_tensors

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 20251                                       # make_episodic_golden.py
FAMILIES = {"maddpg": ("learner3", "MADDPG"), "ippo": ("ippo3", "IPPO")}


def episodic_args(alg, cuda=False, **over):
    prefix, _ = FAMILIES[alg]
    gold = dict(np.load(os.path.join(G, f"episodic_{alg}_golden.npz")))
    bs, size, freq = (int(x) for x in gold["settings"])
    kw = dict(episodic=True, replay=True, batch_size=bs, replay_buffer_size=size, behaviour_update_freq=freq)
    kw.update(over)
    return golden_args(prefix, cuda=cuda, **kw), gold


def episodic_episodes(gold, tile=1):
    """learner3_batch.npz with the fields the reference run replaced, cut into the fixture's episodes: lists of per-step
    Transitions with numpy fields (model.py:230-242).  ``tile``: every episode ``tile`` times (ids e, e + 7, ...)."""
    from safe_marl_amd.replay_buffer import Transition
    b = dict(np.load(os.path.join(G, "learner3_batch.npz")))
    for k in gold:
        if k.startswith("batch."):
            b[k[6:]] = gold[k]
    out, t0 = [], 0
    for length in gold["episode_lengths"]:
        ep = []
        for t in range(t0, t0 + int(length)):
            ep.append(Transition(b["state"][t], b["action"][t][None], b["log_prob_a"][t][None], b["value"][t][None],
                                 b["next_value"][t][None], b["reward"][t], b["next_state"][t], bool(b["done"][t]),
                                 bool(b["last_step"][t]), b["action_avail"][t][None], b["last_hid"][t][None], b["hid"][t][None]))
        out.append(ep)
        t0 += int(length)
    return out * tile


def episodic_state_dict(alg, device="cpu"):
    """The initial weights (the learner3 / ippo3 fixtures) and the reference's after one value and one policy sub-update: the
    latter file holds the model's own entries, its target is the initial one — the target never moves in episodic mode."""
    prefix, _ = FAMILIES[alg]
    init = golden_tensors(prefix + "_state_dict.npz", device)
    after = golden_tensors(f"episodic_{alg}_state_dict_after_step.npz", device)
    after.update({k: v for k, v in init.items() if k.startswith("target_net.")})
    return init, after


def assert_after_step(net, stat, gold, after):
    keys = {k[5:] for k in gold if k.startswith("stat.")}
    assert keys <= set(stat)
    for k in keys:
        assert abs(float(stat[k]) - float(gold["stat." + k])) < 1e-4 * max(1.0, abs(float(gold["stat." + k]))), k
    mine = net.state_dict()
    assert sorted(mine) == sorted(after)
    for k, ref in after.items():
        if k.startswith("target_net."):
            assert th.equal(mine[k], ref), k                               # bit-equal: update_target is never called
        elif ref.is_floating_point():
            assert th.allclose(mine[k].float(), ref.float(), atol=3e-6, rtol=1e-5), k


@pytest.mark.parametrize("alg", sorted(FAMILIES))
def test_trainer_constructs_in_episodic_mode(alg):
    import safe_marl_amd.learner as L
    from safe_marl_amd.replay_buffer import EpisodeReplayBuffer
    from safe_marl_amd.trainer import PGTrainer
    args, _ = episodic_args(alg)
    trainer = PGTrainer(args, getattr(L, FAMILIES[alg][1]), StubEnv(3), None)
    assert trainer.episodic is True and type(trainer.replay_buffer) is EpisodeReplayBuffer
    assert len(trainer.replay_buffer.buffer) == 0 and trainer.replay_buffer.capacity == int(args.replay_buffer_size)
    assert getattr(trainer.behaviour_net, "gae_chain_stride", 1) == 1
    with pytest.raises(NotImplementedError):
        PGTrainer(args._replace(replay=False), getattr(L, FAMILIES[alg][1]), StubEnv(3), None)


@pytest.mark.parametrize("setting", ["a", "b"])
def test_firing_schedule_equals_the_references(setting):
    import safe_marl_amd.learner as L
    from safe_marl_amd.trainer import PGTrainer
    sched = dict(np.load(os.path.join(G, "episodic_schedule.npz")))
    bs, size, freq, warmup = (int(x) for x in sched[f"schedule.{setting}.settings"])
    args, gold = episodic_args("maddpg", batch_size=bs, replay_buffer_size=size, behaviour_update_freq=freq, replay_warmup=warmup)
    assert [args.value_update_epochs, args.policy_update_epochs] == list(sched[f"schedule.{setting}.epochs"])
    trainer = PGTrainer(args, L.MADDPG, StubEnv(3), None)
    net = trainer.behaviour_net
    target0 = {k: v.clone() for k, v in net.target_net.state_dict().items()}
    calls, targets = [], []
    trainer._sub_update = lambda which, stat, batch, **kw: calls.append((which, int(batch.reward.shape[0])))
    net.update_target = lambda: targets.append(1)
    episodes = episodic_episodes(gold)
    value, policy, length = [], [], []
    for ep in range(40):
        trainer.episodes += 1
        del calls[:]
        net.episode_update(trainer, {}, episodes[ep % len(episodes)])
        value.append(sum(1 for c in calls if c[0] == "value"))
        policy.append(sum(1 for c in calls if c[0] == "policy"))
        length.append(len(trainer.replay_buffer.buffer))
        # value sub-updates first, then the policy's, each on a fresh batch of `bs` whole episodes
        assert [c[0] for c in calls] == ["value"] * value[-1] + ["policy"] * policy[-1]
        assert all(bs <= c[1] <= 7 * bs for c in calls)
    assert value == list(sched[f"schedule.{setting}.value_sub_updates"])
    assert policy == list(sched[f"schedule.{setting}.policy_sub_updates"])
    assert length == list(sched[f"schedule.{setting}.buffer_length"]) and max(length) == size
    assert int(sched[f"schedule.{setting}.update_target_calls"]) == 0 and not targets
    assert sum(value) > 0 and (setting == "a" or value[:8] == [0] * 8)
    for k, v in net.target_net.state_dict().items():
        assert th.equal(v, target0[k]), k


def test_buffer_draws_and_concatenates_as_the_reference():
    from safe_marl_amd.replay_buffer import EpisodeReplayBuffer, Transition
    sched = dict(np.load(os.path.join(G, "episodic_schedule.npz")))
    lengths = [int(x) for x in np.load(os.path.join(G, "episodic_maddpg_golden.npz"))["episode_lengths"]]
    buf = EpisodeReplayBuffer(4, device="cpu")
    z = np.zeros((1, 3, 4), np.float32)
    for ep, length in enumerate(lengths):
        # (episode, step) travels in the reward and the done column is the step's parity: any field would do
        buf.add_experience([Transition(np.zeros((3, 6), np.float32), z, z, z[:, :, :1], z[:, :, :1],
                                       np.array([ep, t, 0], np.float32), np.zeros((3, 6), np.float32), bool(t % 2), t == length - 1,
                                       z + 1, z, z) for t in range(length)])
        assert len(buf.buffer) == min(ep + 1, 4)
    held = [int(buf.episodes[i]["reward"][0, 0]) for i in range(4)]
    assert held == list(sched["buffer.held"]) == [3, 4, 5, 6]                       # FIFO by episode at capacity
    np.random.seed(SEED)
    for call in range(3):
        w = buf.get_batch_tensors(2)
        assert [held[i] for i in buf.last_draw] == list(sched[f"buffer.draw{call}.ids"])
        assert np.array_equal(w.reward[:, :2].numpy().astype(np.int64), sched[f"buffer.draw{call}.order"])
        assert w.state.shape == (w.reward.shape[0], 3, 6) and w.done.shape == (w.reward.shape[0],)
        assert np.array_equal(w.done.numpy(), sched[f"buffer.draw{call}.order"][:, 1] % 2)
    single = buf.get_single(1)
    assert np.array_equal(np.array([[int(t.reward[0]), int(t.reward[1])] for t in single]), sched["buffer.single1"])
    np.random.seed(SEED)
    rows = buf.get_batch(2)
    assert np.array_equal(np.array([[int(t.reward[0]), int(t.reward[1])] for t in rows]), sched["buffer.draw0.order"])
    with pytest.raises(ValueError):
        buf.get_batch_tensors(5)                                                   # more episodes than the buffer holds


@pytest.mark.parametrize("alg", sorted(FAMILIES))
def test_sub_updates_match_the_reference(alg):
    import safe_marl_amd.learner as L
    from safe_marl_amd.trainer import PGTrainer
    args, gold = episodic_args(alg)
    cls = getattr(L, FAMILIES[alg][1])
    init, after = episodic_state_dict(alg)
    th.manual_seed(0)
    trainer = PGTrainer(args, cls, StubEnv(3), None)
    net = trainer.behaviour_net
    net.load_state_dict(init)
    for ep in episodic_episodes(gold):
        trainer.replay_buffer.add_experience(ep)
    first = int(gold["held"][0])
    assert len(trainer.replay_buffer.buffer) == len(gold["held"])

    # one get_loss on the first drawn batch, on a model of its own
    np.random.seed(SEED)
    batch = trainer._sample_batch()
    assert [first + i for i in trainer.replay_buffer.last_draw] == list(gold["draw.value"])
    assert batch.reward.shape[0] == int(gold["rows_first_batch"])
    ends = np.cumsum([int(gold["episode_lengths"][e]) for e in gold["draw.value"]]) - 1
    assert np.array_equal(np.flatnonzero(batch.last_step.numpy()), ends)          # every episode ends with last_step = 1
    model = golden_model(cls, args, init)
    policy_loss, value_loss, (means, log_stds) = model.get_loss(batch)
    print(alg, "policy loss", policy_loss.item(), float(gold["policy_loss"]), "value loss", value_loss.item(), float(gold["value_loss"]))
    assert abs(policy_loss.item() - float(gold["policy_loss"])) < 2e-6
    assert abs(value_loss.item() - float(gold["value_loss"])) < 1e-5 * max(1.0, abs(float(gold["value_loss"])))
    grads = th.autograd.grad(value_loss, list(model.value_dicts.parameters()), retain_graph=True)
    for (k, _), g in zip(model.value_dicts.named_parameters(), grads):
        ref = gold["vgrad." + k]
        assert np.allclose(g.numpy(), ref, atol=2e-6 + 1e-4 * np.abs(ref).max()), k
    from safe_marl_amd.util import normal_entropy
    loss = policy_loss - args.entr * normal_entropy(means, log_stds.exp())        # trainer.py:47-57
    grads = th.autograd.grad(loss, list(model.policy_dicts.parameters()))
    for (k, _), g in zip(model.policy_dicts.named_parameters(), grads):
        ref = gold["pgrad." + k]
        assert np.allclose(g.numpy(), ref, atol=2e-7 + 1e-4 * np.abs(ref).max()), k

    # one value and one policy sub-update, each on a fresh batch of whole episodes
    np.random.seed(SEED)
    stat = {}
    trainer.value_replay_process(stat)
    assert [first + i for i in trainer.replay_buffer.last_draw] == list(gold["draw.value"])
    trainer.policy_replay_process(stat)
    assert [first + i for i in trainer.replay_buffer.last_draw] == list(gold["draw.policy"])
    assert_after_step(net, stat, gold, after)
    assert not trainer._update_graphs and not trainer._event_graphs               # eager, always


def _hand_filled_ring(device, N, n, history, transitions, act_dim=4, hid_dim=8, first_stream=False, filed=False, seed=5):
    """An episodic slab ring of ``transitions`` (+ history - 1) slabs for N environments, filled by hand past its seam: random
    rings, ``older`` counting up from each environment's last restart, last_step at the restarts and on the final step."""
    from safe_marl_amd.replay_buffer import EpisodeReplayBuffer
    g = th.Generator().manual_seed(seed)
    block = transitions - 3                                                   # (one block, its gap slab, two steps in flight)
    buf = EpisodeReplayBuffer(1, device=device)
    buf.configure_blocks(N, block)
    obs_dim = 6 * history if history else 10
    buf.alloc_slabs(N, n, obs_dim, act_dim, hid_dim, history=history)
    assert buf.slabs == transitions + (history - 1 if history else 0)
    steps = block if first_stream else buf.slabs + 5                          # (otherwise the cursor has passed the seam)
    for ring in (buf.row_ring if history else buf.obs_ring, buf.hid_ring, buf.small_ring, buf.nv_ring):
        ring.copy_(th.randn(ring.shape, generator=g).to(device))
    if filed:
        buf.enable_filed_columns(log_prob=True)
        buf.v_ring.copy_(th.randn(buf.v_ring.shape, generator=g).to(device))
        buf.lp_ring.copy_(th.randn(buf.lp_ring.shape, generator=g).to(device))
    na = n * act_dim
    restart = th.rand(steps + 1, N, generator=g) < 0.3                        # environment e restarts AFTER step c
    restart[steps - 1] = True                                                 # the block's last step
    restart[steps - block - 1] = True                                         # ... and the one before the block
    restart[steps - block, 0] = True                                          # an episode of length 1 at the block's start
    restart[steps - block + 2, 1] = restart[steps - block + 3, 1] = True      # ... and one in its middle
    age = th.zeros(N)
    buf.begin_stream(th.randn(N, n, obs_dim, generator=g).to(device))
    for c in range(steps + 1):
        p = c % buf.slabs
        if history:
            rec = buf.row_ring[p].view(N, n, 8)
            rec[:, :, 6] = age.to(device)[:, None]
            rec[:, :, 7] = 0.0
        if c < steps:
            buf.small_ring[p, :, na + n] = (restart[c] & (th.arange(N) % 2 == 0)).float().to(device)      # done
            buf.small_ring[p, :, na + n + 1] = restart[c].float().to(device)                              # last_step
            age = th.where(restart[c], th.zeros(N), age + 1)
            buf.stepped()
    buf.end_block(block)
    return buf, block


def assert_equals_slab_windows(buf, batch, ids):
    """Row by row: what ``slab_window`` hands out for the one transition at that row's slot."""
    from safe_marl_amd.replay_buffer import FIELDS
    row = 0
    for i in ids:
        c0, e, length = buf.episodes[i]
        for j in range(length):
            w = buf.slab_window((c0 + j) * buf.n_envs + e, 1)
            for k in FIELDS:
                got, want = getattr(batch, k)[row], getattr(w, k)[0]
                assert got.shape == want.shape and th.equal(got, want), (k, i, j)
            row += 1
    assert row == batch.reward.shape[0]


def test_ring_composition_equals_slab_window_rows():
    buf, block = _hand_filled_ring("cpu", N=5, n=3, history=4, transitions=9)
    assert buf.slabs == 12 and buf.k > buf.slabs and block == 6
    eps = buf.episodes
    assert len(eps) >= 5 + 3 and eps == sorted(eps) and all(c0 >= buf.first for c0, _, _ in eps)
    assert sorted({e for _, e, _ in eps}) == list(range(5))
    for e in range(5):                                                         # each environment's rows split into whole episodes
        mine = [(c0, length) for c0, env, length in eps if env == e]
        assert mine[0][0] == buf.k - block and sum(length for _, length in mine) == block
        assert all(a[0] + a[1] == b[0] for a, b in zip(mine, mine[1:]))
    assert any(length == 1 for _, _, length in eps)
    np.random.seed(3)
    batch = buf.get_batch_tensors(6)
    assert len(set(buf.last_draw)) == 6
    assert_equals_slab_windows(buf, batch, buf.last_draw)
    ends = np.cumsum([eps[i][2] for i in buf.last_draw]) - 1
    assert np.array_equal(np.flatnonzero(batch.last_step.numpy()), ends)
    assert batch.action_avail.shape == (batch.reward.shape[0], 3, 4) and float(batch.action_avail.min()) == 1.0
    # the next block retires the episodes of this one (capacity: one block)
    for _ in range(block):
        buf.small_ring[buf.k % buf.slabs, :, -1] = 0.0
        buf.small_ring[buf.k % buf.slabs, :, 3 * 4 + 3 + 1] = 0.0
        buf.stepped()
    buf.small_ring[(buf.k - 1) % buf.slabs, :, 3 * 4 + 3 + 1] = 1.0
    buf.end_block(block)
    assert buf.episodes == [(buf.k - block, e, block) for e in range(5)]


def test_field_store_episodes_of_a_vectorised_block():
    """The eager vectorised rollout files vector steps with add_batch: episodes are strided rows of the time-major store."""
    from safe_marl_amd.replay_buffer import EpisodeReplayBuffer
    N, n, T = 4, 3, 6
    buf = EpisodeReplayBuffer(2, device="cpu")
    buf.configure_blocks(N, T)
    marks = {}
    for blk in range(3):
        for t in range(T):
            last = th.zeros(N)
            if t == T - 1:
                last[:] = 1.0
            if t == 2:
                last[blk % N] = 1.0                                           # one early termination per block
            c = blk * T + t
            marks[c] = last.clone()
            tag = (c * N + th.arange(N)).float()
            buf.add_batch(state=tag.view(N, 1, 1).expand(N, n, 2).contiguous(), action=th.zeros(N, n, 4), log_prob_a=0.0,
                          value=0.0, next_value=0.0, reward=tag.view(N, 1).expand(N, n).contiguous(),
                          next_state=(tag + N).view(N, 1, 1).expand(N, n, 2).contiguous(), done=th.zeros(N), last_step=last,
                          action_avail=1.0, last_hid=th.zeros(N, n, 8), hid=th.zeros(N, n, 8))
        buf.end_block(T)
        assert len(buf.buffer) == min(blk + 1, 2) * (N + 1)
    assert min(c0 for c0, _, _ in buf.episodes) == T                           # the first block left: capacity counts blocks
    np.random.seed(1)
    w = buf.get_batch_tensors(5)
    want = np.concatenate([(np.arange(c0, c0 + length) * N + e) for c0, e, length in (buf.episodes[i] for i in buf.last_draw)])
    assert np.array_equal(w.reward[:, 0].numpy(), want.astype(np.float32))
    assert np.array_equal(w.next_state[:, 0, 0].numpy(), want.astype(np.float32) + N)
    ends = np.cumsum([buf.episodes[i][2] for i in buf.last_draw]) - 1
    assert np.array_equal(np.flatnonzero(w.last_step.numpy()), ends)
    assert w.action_avail.shape[0] == len(want) and float(w.action_avail.min()) == 1.0


def test_example_lists_the_episodic_flag():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "train_maddpg.py"), "--help"], capture_output=True,
                         text=True, check=True).stdout
    assert "--episodic" in out


def test_gather_episodes_rejects_bad_arguments_without_a_gpu():
    from safe_marl_amd import _lib, build
    build.build()
    lib = _lib.load()
    EINVAL = -1                                                       # include/flexnet.h: FLEXNET_EINVAL
    assert "flexnet_gather_episodes" in _lib.SYMBOLS and len(lib.flexnet_gather_episodes.argtypes) == 2
    hdr = open(os.path.join(ROOT, "include", "flexnet.h")).read()
    assert f"#define FLEXNET_EPISODE_ROWS {_lib.FLEXNET_EPISODE_ROWS}" in hdr
    assert C.sizeof(_lib.FlexEpisodeGatherArgs) == 20 * 8 + 8 + 10 * 4
    assert lib.flexnet_gather_episodes(None, None) == EINVAL
    store = (C.c_float * 64)()
    p = C.cast(store, C.c_void_p).value
    p -= p % 16
    table = np.array([[0, 1, 3, 0], [4, 0, 2, 3]], dtype=np.int64)
    tensors = ("hid_ring", "small_ring", "episodes", "state", "next_state", "last_hid", "hid", "action", "reward", "done", "last_step")

    def args(**over):
        a = _lib.FlexEpisodeGatherArgs()
        for k in tensors + ("row_ring",):
            setattr(a, k, p)
        a.episodes_host = table.ctypes.data
        a.rows, a.n_episodes, a.n_envs, a.n_agents, a.history, a.obs_dim = 5, 2, 2, 3, 4, 24
        a.hid_dim, a.act_dim, a.small_w, a.slabs = 8, 4, 20, 12
        for k, v in over.items():
            setattr(a, k, v)
        return a

    def rc(**over):
        return lib.flexnet_gather_episodes(C.byref(args(**over)), None)

    for k in tensors + ("row_ring", "episodes_host"):                             # a missing tensor (row_ring: no observation ring)
        assert rc(**{k: None}) == EINVAL, k
    assert rc(obs_ring=p) == EINVAL                                               # both observation rings
    assert rc(v_ring=p) == EINVAL and rc(value=p) == EINVAL                       # a filed ring without its output, and the reverse
    assert rc(nv_ring=p) == EINVAL and rc(lp_ring=p) == EINVAL and rc(log_prob_a=p) == EINVAL
    assert rc(history=3) == EINVAL and rc(history=0) == EINVAL                    # history not matching the ring
    assert rc(row_ring=None, obs_ring=p, history=4) == EINVAL                     # ... a history on the stacked ring
    assert rc(small_w=3 * 4 + 3 + 1) == EINVAL and rc(n_episodes=0) == EINVAL and rc(rows=0) == EINVAL
    assert rc(rows=6) == EINVAL and rc(rows=4) == EINVAL                          # the table's total is not the batch
    for row, col, bad in ((0, 2, 0), (1, 2, -1),                                   # a length < 1
                          (1, 3, 5), (1, 3, 7), (1, 3, 2), (0, 3, 1),              # an output offset outside the batch / the tiling
                          (0, 1, 2), (0, 1, -1), (1, 0, -1),                       # an environment outside the ring, a negative counter
                          (0, 2, 9)):                                              # an episode longer than the ring holds
        keep = table[row, col]
        table[row, col] = bad
        assert rc() == EINVAL, (row, col, bad)
        table[row, col] = keep
