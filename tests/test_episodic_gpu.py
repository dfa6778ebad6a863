"""GPU: ``episodic: True`` through the product paths.  The vectorised trainer at 8 environments and three agents, with the
graph rollout on (slab ring, flexnet_gather_episodes) and off (field-by-field store), for MADDPG and for IPPO with the
on-policy triple, over three blocks: the update fires by the rule of model.py:76-78, every batch handed to get_loss is the
concatenation of the drawn episodes rebuilt on the host from the episode table, every episode ends with last_step = 1, losses
are finite, parameters move on the firing blocks only, the target stays bit-equal.  Then the reference's golden sub-updates
(tests/golden/make_episodic_golden.py) through PGTrainer and the episodic buffer on the device, tiled as
tests/test_unshared_golden_gpu.py tiles its batch, within that file's bounds (losses 1e-5 relative, ``stat`` 2e-4, the weights
after one value and one policy sub-update 5e-5)."""
import numpy as np
import pytest
import torch as th

from .golden_io import StubEnv, _np
from .test_episodic_cpu import FAMILIES, SEED, episodic_args, episodic_episodes, episodic_state_dict

pytestmark = pytest.mark.gpu

BLOCK = 24                                         # vector steps per block (max_steps)


def _trainer(alg, graph_rollout):
    from safe_marl_amd import learner
    from safe_marl_amd.flex_env import VecFlexProvisionEnv
    from safe_marl_amd.network import create_network
    from safe_marl_amd.series import make_synthetic_series
    from safe_marl_amd.trainer import PGTrainer
    blds = [5, 15, 25]
    env_args = {"buildings": blds, "pv_nodes": blds, "ess_nodes": blds}
    net = create_network(env_args)
    env = VecFlexProvisionEnv(env_args, 8, net=net, series=make_synthetic_series(net, n_days=30), seed=4, warm_start=True)
    over = dict(max_steps=BLOCK, value_update_epochs=2, policy_update_epochs=2)
    if alg == "ippo":
        over.update(batch_size=2, replay_buffer_size=2, behaviour_update_freq=2)             # default.yaml:1
    else:
        over.update(batch_size=4, replay_buffer_size=2, behaviour_update_freq=2)
    args, _ = episodic_args(alg, cuda=True, **over)
    assert args.agent_num == env.n_agents == 3 and args.obs_size == env.obs_size
    th.manual_seed(3)
    np.random.seed(3)
    return PGTrainer(args, getattr(learner, FAMILIES[alg][1]), env, None, graph_rollout=graph_rollout), args


def _host_batch(buf, ids):
    """The drawn episodes' transitions one behind the other, rebuilt from the episode table one transition at a time."""
    from safe_marl_amd.replay_buffer import DeviceReplayBuffer, FIELDS
    rows = []
    for i in ids:
        c0, e, length = buf.episodes[i]
        for j in range(length):
            slot = (c0 + j) * buf.block_envs + e
            if buf.slab_mode:
                rows.append(buf.slab_window(slot, 1))
            else:                                                              # the time-major field store: row = slot mod size
                p = slot % buf.size
                rows.append({k: v[p:p + 1] for k, v in buf.store.items()})
    if buf.slab_mode:
        return {k: th.cat([getattr(r, k) for r in rows]) for k in FIELDS}
    return {k: th.cat([r[k] for r in rows]) for k in buf.store}


@pytest.mark.parametrize("graph_rollout", [True, False])
@pytest.mark.parametrize("alg", ["maddpg", "ippo"])
def test_three_blocks_of_vectorised_episodic_training(alg, graph_rollout):
    from safe_marl_amd.replay_buffer import EpisodeReplayBuffer
    from safe_marl_amd.util import FALLBACKS
    declined = FALLBACKS.get("gather_episodes", 0)
    trainer, args = _trainer(alg, graph_rollout)
    net, buf = trainer.behaviour_net, trainer.replay_buffer
    assert type(buf) is EpisodeReplayBuffer and buf.block_steps == BLOCK and trainer.effective_batch_size() == args.batch_size
    target0 = {k: v.clone() for k, v in net.target_net.state_dict().items()}
    seen = []
    get_loss = trainer.get_loss

    def checking_get_loss(batch, need="both"):
        ids = list(buf.last_draw)
        want = _host_batch(buf, ids)
        for k, v in want.items():
            got = getattr(batch, k)
            assert got.shape == v.shape and th.equal(got, v), (k, ids)
        ends = np.cumsum([buf.episodes[i][2] for i in ids]) - 1
        last = _np(batch.last_step)
        assert np.all(last[ends] == 1.0) and batch.reward.shape[0] == ends[-1] + 1
        assert len(ids) == len(set(ids)) == trainer.effective_batch_size()
        out = get_loss(batch, need=need)
        seen.append((need, float(out[1 if need == "value" else 0].detach())))
        return out

    trainer.get_loss = checking_get_loss
    fired = []
    for block in range(1, 4):
        before = {k: v.clone() for k, v in net.state_dict().items() if not k.startswith("target_net.")}
        del seen[:]
        stat = {}
        net.train_process(stat, trainer)
        th.cuda.synchronize()
        assert trainer.episodes == block and trainer.steps == block * BLOCK
        assert buf.slab_mode == graph_rollout
        assert len(buf.buffer) >= 8 * min(block, 2) and all(length >= 1 for _, _, length in buf.episodes)
        assert len(buf.block_starts) == min(block, 2) and min(c0 for c0, _, _ in buf.episodes) == buf.block_starts[0]   # two blocks
        due = block > args.replay_warmup and block % args.behaviour_update_freq == 0        # model.py:76-78
        fired.append(bool(seen))
        assert bool(seen) == due, (block, seen)
        moved = any(not th.equal(v, before[k]) for k, v in net.state_dict().items()
                    if k in before and "batchnorm" not in k and v.is_floating_point())
        assert moved == due, block
        if due:
            assert [s[0] for s in seen] == ["value"] * 2 + ["policy"] * 2
            assert all(np.isfinite(s[1]) for s in seen), seen
            assert np.isfinite(float(stat["mean_train_value_loss"])) and np.isfinite(float(stat["mean_train_policy_loss"]))
        assert np.isfinite(float(stat["mean_train_reward"]))
    assert fired == [False, True, False]
    for k, v in net.target_net.state_dict().items():
        assert th.equal(v, target0[k]), k
    assert not trainer._update_graphs and not trainer._event_graphs             # episodic sub-updates are never captured
    assert FALLBACKS.get("gather_episodes", 0) == declined


def _tiled(batch, cls, tile):
    """tile copies of a batch of whole episodes; IPPO's row by row (every copy a GAE chain of its own, stride = tile)."""
    if tile == 1:
        return batch
    if cls != "IPPO":
        return batch._replace(**{k: getattr(batch, k).repeat((tile,) + (1,) * (getattr(batch, k).dim() - 1)).contiguous()
                                 for k in batch._fields})
    return batch._replace(**{k: getattr(batch, k).repeat_interleave(tile, dim=0).contiguous() for k in batch._fields})


@pytest.mark.parametrize("tile", [1, 64])
@pytest.mark.parametrize("alg", sorted(FAMILIES))
def test_golden_sub_updates_on_the_device(alg, tile):
    import safe_marl_amd.learner as L
    from safe_marl_amd.trainer import PGTrainer
    cls = FAMILIES[alg][1]
    args, gold = episodic_args(alg, cuda=True)
    init, after = episodic_state_dict(alg, "cuda")
    th.manual_seed(0)
    trainer = PGTrainer(args, getattr(L, cls), StubEnv(3), None)
    net = trainer.behaviour_net
    net.load_state_dict(init)
    if cls == "IPPO":
        net.gae_chain_stride = tile
    for ep in episodic_episodes(gold):
        trainer.replay_buffer.add_experience(ep)
    first = int(gold["held"][0])
    draws = []
    sample = trainer._sample_batch

    def tiled_sample():
        b = sample()
        assert b.reward.is_cuda
        draws.append([first + i for i in trainer.replay_buffer.last_draw])
        return _tiled(b, cls, tile)

    trainer._sample_batch = tiled_sample
    np.random.seed(SEED)
    stat = {}
    trainer.value_replay_process(stat)
    trainer.policy_replay_process(stat)
    assert draws == [list(gold["draw.value"]), list(gold["draw.policy"])]
    for k in ("mean_train_value_loss", "mean_train_value_grad_norm", "mean_train_policy_loss", "mean_train_policy_grad_norm",
              "mean_train_entropy"):
        ref = float(gold["stat." + k])
        print(f"episodic {alg} x{tile} {k}: {float(stat[k]):.8f} (golden {ref:.8f})")
        assert abs(float(stat[k]) - ref) < 2e-4 * max(1.0, abs(ref)), (tile, k, float(stat[k]), ref)
    cur = net.state_dict()
    for k, v in after.items():
        if k.startswith("target_net."):
            assert th.equal(cur[k], v), k                                        # the target never moves
        elif "batchnorm" not in k:            # (running_var sees the unbiased n / (n - 1) factor of a tiled batch)
            assert np.allclose(_np(cur[k]), _np(v), atol=5e-5), (tile, k, float((cur[k].float() - v.float()).abs().max()))
    assert any(not th.equal(cur[k], init[k]) for k in init if k.startswith("policy_dicts."))
