#!/usr/bin/env python3
"""Generates tests/golden/{ippo,mappo}*_*.npz by IMPORTING the reference's IPPO / MAPPO (madrl/models/ippo.py, mappo.py)
and PGTrainer (utils/trainer.py) on CPU, with alg_args/ippo.yaml or mappo.yaml merged over default.yaml and seeded
weights.  Run on a CPU machine that holds a checkout of the reference, named by --reference (or REFERENCE_DIR):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_ppo_golden.py --reference <reference checkout>
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_ppo_golden.py --reference <reference checkout> --agents 3

Both algorithms are written per call.  The batch is learner_batch.npz (learner3_batch.npz with three agents) with three
fields replaced and recorded in the fixture: the action of agent 0 for every agent (what ippo.py:72-73 stores), and a
done / last_step pattern that takes every branch of the GAE mask (ppo.py:45-48).  The intermediates of get_loss are taken
by wrapping the functions it calls (th.clamp, BatchNorm1d.forward).  The fixtures are data; no reference source travels.
"""
import json
import os
import sys

import numpy as np
import torch as th
import torch.nn as nn
import yaml

REF = os.environ.get("REFERENCE_DIR")
if "--reference" in sys.argv:
    REF = sys.argv[sys.argv.index("--reference") + 1]
if not REF or not os.path.isdir(os.path.join(REF, "madrl")):
    sys.exit("make_ppo_golden.py: name the reference checkout with --reference DIR (or REFERENCE_DIR)")
REF = os.path.abspath(REF)
OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REF)
os.chdir(REF)

from utils.util import convert  # noqa: E402
from utils.trainer import PGTrainer  # noqa: E402
from madrl.models.ippo import IPPO  # noqa: E402
from madrl.models.mappo import MAPPO  # noqa: E402

N_AGENTS = 5
if "--agents" in sys.argv:
    N_AGENTS = int(sys.argv[sys.argv.index("--agents") + 1])
OUT_DIR = os.environ.get("GOLDEN_OUT", OUT)
BATCH = "learner_batch.npz" if N_AGENTS == 5 else f"learner{N_AGENTS}_batch.npz"

CLAMPS, NORMS = [], []
_clamp, _bn_forward = th.clamp, nn.BatchNorm1d.forward


def _recording_clamp(x, *a, **k):
    CLAMPS.append(x.detach().clone())
    return _clamp(x, *a, **k)


def _recording_bn(self, x):
    out = _bn_forward(self, x)
    NORMS.append((x.detach().clone(), out.detach().clone()))
    return out


th.clamp = _recording_clamp
nn.BatchNorm1d.forward = _recording_bn


def load_args(alg):
    with open("madrl/args/default.yaml") as f:
        d = yaml.safe_load(f)
    with open(f"madrl/args/alg_args/{alg}.yaml") as f:
        a = yaml.safe_load(f)["alg_args"]
    with open("madrl/args/env_args/flex_provision.yaml") as f:
        e = yaml.safe_load(f)["env_args"]
    for k, v in (("action_low", 0.0), ("action_high", 1.0), ("action_bias", 0.0), ("action_scale", 1.0)):
        a[k] = e.get(k, v)
    a["alg"] = alg
    d = {**d, **a}
    d.update(agent_num=N_AGENTS, obs_size=144, state_size=3 * 33 + 2 * N_AGENTS + 1, action_dim=4, cuda=False)
    return d


class StubEnv:
    def get_num_of_agents(self):
        return N_AGENTS


def ppo_batch():
    b = dict(np.load(os.path.join(OUT, BATCH)))
    rows = b["state"].shape[0]
    b["action"] = np.repeat(b["action"][:, :1], N_AGENTS, axis=1)         # ippo.py:72-73: one action, every agent
    done, last = np.zeros(rows), np.zeros(rows)
    last[[6, 13, 20, rows - 1]] = 1.0          # truncated: the chain restarts, the bootstrap stays
    done[[13]] = 1.0                           # terminated: the chain restarts, no bootstrap
    last[[25]], done[[25]] = 1.0, 1.0
    b["done"], b["last_step"] = done, last
    assert np.abs(b["value"]).max() > 0 and np.abs(b["next_value"]).max() > 0
    return b


def transitions(model, b):
    """The packed batch back into the per-sample fields model.py:230-242 stores."""
    out = []
    for t in range(b["state"].shape[0]):
        out.append(model.Transition(
            list(b["state"][t]), b["action"][t][None].astype(np.float32), b["log_prob_a"][t][None].astype(np.float32),
            b["value"][t][None].astype(np.float32), b["next_value"][t][None].astype(np.float32), b["reward"][t],
            list(b["next_state"][t]), bool(b["done"][t]), bool(b["last_step"][t]), b["action_avail"][t][None],
            b["last_hid"][t][None].astype(np.float32), b["hid"][t][None].astype(np.float32)))
    return model.Transition(*zip(*out))


def main(alg, cls):
    prefix = alg if N_AGENTS == 5 else f"{alg}{N_AGENTS}"

    def save_sd(name, sd):
        np.savez_compressed(os.path.join(OUT_DIR, f"{prefix}_{name}.npz"),
                            **{k: v.detach().cpu().numpy().copy() for k, v in sd.items()})

    argd = load_args(alg)
    args = convert(argd)
    json.dump(argd, open(os.path.join(OUT_DIR, prefix + "_args.json"), "w"), indent=1, sort_keys=True)
    th.manual_seed(2468)
    target = cls(args)
    model = cls(args, target)
    sd0 = {k: v.detach().clone() for k, v in model.state_dict().items()}
    tgt0 = {k: v.detach().clone() for k, v in target.state_dict().items()}
    save_sd("state_dict", sd0)
    b = ppo_batch()
    g = {"batch.action": b["action"], "batch.done": b["done"], "batch.last_step": b["last_step"]}
    batch = transitions(model, b)

    # (1) one get_loss call (ppo.py:14-69) with its intermediates
    CLAMPS.clear(), NORMS.clear()
    policy_loss, value_loss, (means, _) = model.get_loss(batch)
    assert len(CLAMPS) == 2 and len(NORMS) == 2, (len(CLAMPS), len(NORMS))
    g["policy_loss"], g["value_loss"], g["means"] = policy_loss.item(), value_loss.item(), means.detach().numpy()
    g["reward_norm"], g["advantages"], g["advantages_norm"] = NORMS[0][1].numpy(), NORMS[1][0].numpy(), NORMS[1][1].numpy()
    g["ratios"] = CLAMPS[0].numpy()
    with th.no_grad():
        up = model.unpack_data(batch)              # (moves the reward BatchNorm once more: statistics recorded first)
    NORMS.clear()
    for name, bn in (("reward_bn", model.batchnorm), ("adv_bn", model.rl.batchnorm)):
        g[name + ".num_batches_tracked"] = int(bn.num_batches_tracked)
    model2 = cls(args, cls(args))
    model2.load_state_dict(sd0)
    policy_loss2, _, _ = model2.get_loss(batch)
    assert policy_loss2.item() == policy_loss.item()
    for name, bn in (("reward_bn", model2.batchnorm), ("adv_bn", model2.rl.batchnorm)):
        g[name + ".running_mean"], g[name + ".running_var"] = bn.running_mean.numpy().copy(), bn.running_var.numpy().copy()
        g[name + ".num_batches_tracked"] = int(bn.num_batches_tracked)
    with th.no_grad():
        next_values = model2.value(up[6], None).contiguous().view(-1, N_AGENTS)
        g["returns"] = (th.from_numpy(g["reward_norm"]) + args.gamma * (1 - up[7]) * next_values).numpy()      # ppo.py:53
        g["value"] = model2.value(up[0], None).numpy()
    model2.zero_grad()
    pl, vl, _ = model2.get_loss(batch)
    vl.backward(retain_graph=True)
    for k, p in model2.value_dicts.named_parameters():
        g["vgrad." + k] = p.grad.numpy().copy()
    model2.zero_grad()
    pl.backward()
    for k, p in model2.policy_dicts.named_parameters():
        g["pgrad." + k] = p.grad.numpy().copy()
    g["policy_loss_second_call"], g["value_loss_second_call"] = pl.item(), vl.item()

    # (2) one value and one policy step through PGTrainer (trainer.py:81-108): each evaluates get_loss once
    th.manual_seed(2468)
    trainer = PGTrainer(args, cls, StubEnv(), None)
    trainer.behaviour_net.load_state_dict(sd0)
    trainer.behaviour_net.target_net.load_state_dict(tgt0)
    stat = {}
    trainer.value_transition_process(stat, batch)
    trainer.policy_transition_process(stat, batch)
    for k, v in stat.items():
        g["stat." + k] = float(v)
    save_sd("state_dict_after_step", trainer.behaviour_net.state_dict())
    for name, bn in (("reward_bn", trainer.behaviour_net.batchnorm), ("adv_bn", trainer.behaviour_net.rl.batchnorm)):
        g["after_step." + name + ".running_mean"] = bn.running_mean.numpy().copy()
        g["after_step." + name + ".running_var"] = bn.running_var.numpy().copy()

    # (3) update_target on the post-step weights (model.py:28-38)
    trainer.behaviour_net.update_target()
    save_sd("target_after_update", trainer.behaviour_net.target_net.state_dict())

    np.savez_compressed(os.path.join(OUT_DIR, prefix + "_golden.npz"), **g)
    print("wrote", sorted(f for f in os.listdir(OUT_DIR) if f.startswith(prefix + "_")))


if __name__ == "__main__":
    main("ippo", IPPO)
    main("mappo", MAPPO)
