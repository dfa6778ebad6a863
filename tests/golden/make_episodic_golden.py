#!/usr/bin/env python3
"""Generates tests/golden/episodic_* by IMPORTING the reference's EpisodeReplayBuffer (utils/replay_buffer.py:33-56),
Model.episode_update (madrl/models/model.py:73-86), MADDPG / IPPO and PGTrainer (utils/trainer.py) on CPU with
``episodic: True`` (default.yaml:9).  Run on a CPU machine that holds a checkout of the reference, named by --reference (or
REFERENCE_DIR):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_episodic_golden.py --reference <reference checkout>

Three agents.  The arguments and the initial weights are those of the learner3 (MADDPG) and ippo3 (IPPO) fixtures — loaded,
not stored again; the episodes are cut from learner3_batch.npz at unequal lengths (EPISODE_LENGTHS), every episode ending
with last_step = 1, two of them with done = 1 (IPPO also stores agent 0's action for every agent, ippo.py:72-73); the fields
replaced are recorded as ``batch.*``.  Written:

  episodic_schedule.npz   (1) the firing schedule of episode_update over 40 episodes with a stub trainer, at two settings
                          (``a``: no warm-up; ``b``: replay_warmup 7): per episode the number of value / policy sub-updates
                          and the buffer's length, and the number of update_target calls (zero);
                          (2) EpisodeReplayBuffer: fill, overflow and three get_batch calls under np.random.seed — the
                          drawn episode ids and the concatenated (episode, step) order.
  episodic_{maddpg,ippo}_golden.npz, episodic_{maddpg,ippo}_state_dict_after_step.npz
                          (3) through the reference's PGTrainer and its episodic buffer, after np.random.seed: the gradients
                          of one get_loss on the first drawn batch, then one value_replay_process and one
                          policy_replay_process — the drawn episodes, both losses, ``stat`` and the model's own state_dict
                          entries (its ``target_net.*`` entries equal the initial ones: asserted here, the target never moves).

The fixtures are data; no reference source travels.  Running it twice writes the same bytes.
"""
import json
import os
import sys

import numpy as np
import torch as th

REF = os.environ.get("REFERENCE_DIR")
if "--reference" in sys.argv:
    REF = sys.argv[sys.argv.index("--reference") + 1]
if not REF or not os.path.isdir(os.path.join(REF, "madrl")):
    sys.exit("make_episodic_golden.py: name the reference checkout with --reference DIR (or REFERENCE_DIR)")
REF = os.path.abspath(REF)
OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REF)
os.chdir(REF)

from utils.util import convert, normal_entropy  # noqa: E402
from utils.trainer import PGTrainer  # noqa: E402
from utils.replay_buffer import EpisodeReplayBuffer  # noqa: E402
from madrl.models.maddpg import MADDPG  # noqa: E402
from madrl.models.ippo import IPPO  # noqa: E402

N_AGENTS = 3
OUT_DIR = os.environ.get("GOLDEN_OUT", OUT)
EPISODE_LENGTHS = (5, 3, 7, 1, 6, 4, 6)            # 32 rows of learner3_batch.npz
DONE_EPISODES = (1, 4)                             # ... whose last row is a termination (done = 1)
SEED = 20251
SETTINGS = {"a": dict(batch_size=2, replay_buffer_size=4, behaviour_update_freq=2, replay_warmup=0),
            "b": dict(batch_size=3, replay_buffer_size=5, behaviour_update_freq=3, replay_warmup=7)}
FAMILIES = {"maddpg": ("learner3", MADDPG, dict(batch_size=2, replay_buffer_size=4, behaviour_update_freq=2)),
            "ippo": ("ippo3", IPPO, dict(batch_size=3, replay_buffer_size=3, behaviour_update_freq=3))}     # the on-policy triple


class StubEnv:
    def get_num_of_agents(self):
        return N_AGENTS


def load_args(prefix, **over):
    d = json.load(open(os.path.join(OUT, prefix + "_args.json")))
    d.update(cuda=False, episodic=True, replay=True, **over)
    return convert(d)


def batch_arrays(alg):
    b = dict(np.load(os.path.join(OUT, "learner3_batch.npz")))
    rows = b["state"].shape[0]
    assert sum(EPISODE_LENGTHS) == rows
    ends = np.cumsum(EPISODE_LENGTHS) - 1
    done, last = np.zeros(rows), np.zeros(rows)
    last[ends] = 1.0
    done[ends[list(DONE_EPISODES)]] = 1.0
    b["done"], b["last_step"] = done, last
    replaced = dict(done=done, last_step=last)
    if alg == "ippo":
        b["action"] = replaced["action"] = np.repeat(b["action"][:, :1], N_AGENTS, axis=1)
    return b, replaced


def episodes_of(model, b):
    """The batch as episodes: lists of the per-step Transitions model.py:230-242 stores."""
    out, t0 = [], 0
    for length in EPISODE_LENGTHS:
        ep = []
        for t in range(t0, t0 + length):
            ep.append(model.Transition(
                list(b["state"][t]), b["action"][t][None].astype(np.float32), b["log_prob_a"][t][None].astype(np.float32),
                b["value"][t][None].astype(np.float32), b["next_value"][t][None].astype(np.float32), b["reward"][t],
                list(b["next_state"][t]), bool(b["done"][t]), bool(b["last_step"][t]), b["action_avail"][t][None],
                b["last_hid"][t][None].astype(np.float32), b["hid"][t][None].astype(np.float32)))
        out.append(ep)
        t0 += length
    return out


class CountingTrainer:
    """What episode_update touches of a trainer (model.py:73-86), counting instead of training."""

    def __init__(self, size):
        self.replay_buffer = EpisodeReplayBuffer(size)
        self.episodes = self.steps = 0
        self.calls = dict(value=0, policy=0, mixer=0)

    def value_replay_process(self, stat):
        self.calls["value"] += 1

    def policy_replay_process(self, stat):
        self.calls["policy"] += 1

    def mixer_replay_process(self, stat):
        self.calls["mixer"] += 1


def schedule(g):
    for name, over in SETTINGS.items():
        args = load_args("learner3", **over)
        model = MADDPG(args, MADDPG(args))
        targets = []
        model.update_target = lambda: targets.append(1)
        trainer = CountingTrainer(int(args.replay_buffer_size))
        value, policy, length = [], [], []
        for ep in range(40):
            trainer.episodes += 1                                         # model.py:247
            before = dict(trainer.calls)
            model.episode_update(trainer, [("episode", ep)], {})
            value.append(trainer.calls["value"] - before["value"])
            policy.append(trainer.calls["policy"] - before["policy"])
            length.append(len(trainer.replay_buffer.buffer))
        assert trainer.calls["mixer"] == 0
        g[f"schedule.{name}.settings"] = np.array([over[k] for k in ("batch_size", "replay_buffer_size", "behaviour_update_freq",
                                                                      "replay_warmup")], dtype=np.int64)
        g[f"schedule.{name}.epochs"] = np.array([args.value_update_epochs, args.policy_update_epochs], dtype=np.int64)
        g[f"schedule.{name}.value_sub_updates"] = np.array(value, dtype=np.int64)
        g[f"schedule.{name}.policy_sub_updates"] = np.array(policy, dtype=np.int64)
        g[f"schedule.{name}.buffer_length"] = np.array(length, dtype=np.int64)
        g[f"schedule.{name}.update_target_calls"] = np.int64(len(targets))


def buffer_sequence(g):
    buf = EpisodeReplayBuffer(4)
    for ep, length in enumerate(EPISODE_LENGTHS):
        buf.add_experience([(ep, t) for t in range(length)])
    g["buffer.held"] = np.array([e[0][0] for e in buf.buffer], dtype=np.int64)
    np.random.seed(SEED)
    for call in range(3):
        batch = buf.get_batch(2)
        order = np.array(batch, dtype=np.int64)                           # [rows, 2]: (episode, step)
        ids = [int(order[0, 0])] + [int(order[i, 0]) for i in range(1, len(order)) if order[i, 0] != order[i - 1, 0]]
        g[f"buffer.draw{call}.ids"], g[f"buffer.draw{call}.order"] = np.array(ids, dtype=np.int64), order
    g["buffer.single1"] = np.array(buf.get_single(1), dtype=np.int64)


def family(alg):
    prefix, cls, over = FAMILIES[alg]
    args = load_args(prefix, **over)
    sd0 = {k: th.from_numpy(v) for k, v in np.load(os.path.join(OUT, prefix + "_state_dict.npz")).items()}
    b, replaced = batch_arrays(alg)
    g = {"batch." + k: v for k, v in replaced.items()}
    g["episode_lengths"] = np.array(EPISODE_LENGTHS, dtype=np.int64)
    g["settings"] = np.array([over[k] for k in ("batch_size", "replay_buffer_size", "behaviour_update_freq")], dtype=np.int64)

    th.manual_seed(SEED)
    trainer = PGTrainer(args, cls, StubEnv(), None)
    net = trainer.behaviour_net
    net.load_state_dict(sd0)
    assert type(trainer.replay_buffer) is EpisodeReplayBuffer and trainer.episodic
    for ep in episodes_of(net, b):
        trainer.replay_buffer.add_experience(ep)
    first = len(EPISODE_LENGTHS) - int(args.replay_buffer_size)         # id of the oldest episode still held
    assert len(trainer.replay_buffer.buffer) == int(args.replay_buffer_size)
    g["held"] = np.arange(first, len(EPISODE_LENGTHS), dtype=np.int64)

    draws = []
    choice = np.random.choice

    def recording_choice(*a, **k):
        out = choice(*a, **k)
        draws.append(np.asarray(out).copy() + first)
        return out

    np.random.choice = recording_choice
    try:
        # the gradients of one get_loss on the first drawn batch, on a model of its own
        np.random.seed(SEED)
        batch = net.Transition(*zip(*trainer.replay_buffer.get_batch(args.batch_size)))
        g["rows_first_batch"] = np.int64(len(batch.reward))
        model = cls(args, cls(args))
        model.load_state_dict(sd0)
        model.zero_grad()
        policy_loss, value_loss, (means, log_stds) = model.get_loss(batch)
        g["policy_loss"], g["value_loss"] = policy_loss.item(), value_loss.item()
        value_loss.backward(retain_graph=True)
        for k, p in model.value_dicts.named_parameters():
            g["vgrad." + k] = p.grad.numpy().copy()
        model.zero_grad()
        entropy = normal_entropy(means, log_stds.exp())
        (policy_loss - args.entr * entropy).backward()                   # trainer.py:47-57
        for k, p in model.policy_dicts.named_parameters():
            g["pgrad." + k] = p.grad.numpy().copy()
        # one value and one policy sub-update through the trainer, each on a fresh batch of whole episodes
        np.random.seed(SEED)
        stat = {}
        trainer.value_replay_process(stat)
        trainer.policy_replay_process(stat)
    finally:
        np.random.choice = choice
    assert len(draws) == 3 and np.array_equal(draws[0], draws[1])
    g["draw.value"], g["draw.policy"] = draws[1].astype(np.int64), draws[2].astype(np.int64)
    for k, v in stat.items():
        g["stat." + k] = float(v)
    own = {}
    for k, v in net.state_dict().items():
        if k.startswith("target_net."):
            assert np.array_equal(v.numpy(), sd0[k].numpy()), k        # update_target is never called in episodic mode
        else:
            own[k] = v.detach().cpu().numpy().copy()
    np.savez_compressed(os.path.join(OUT_DIR, f"episodic_{alg}_state_dict_after_step.npz"), **own)
    np.savez_compressed(os.path.join(OUT_DIR, f"episodic_{alg}_golden.npz"), **g)


if __name__ == "__main__":
    g = {}
    schedule(g)
    buffer_sequence(g)
    np.savez_compressed(os.path.join(OUT_DIR, "episodic_schedule.npz"), **g)
    for alg in FAMILIES:
        family(alg)
    print("wrote", sorted(f for f in os.listdir(OUT_DIR) if f.startswith("episodic_")))
