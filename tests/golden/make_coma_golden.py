#!/usr/bin/env python3
"""Generates tests/golden/coma*_*.npz by IMPORTING the reference's COMA (madrl/models/coma.py) and PGTrainer
(utils/trainer.py) on CPU, with alg_args/coma.yaml merged over default.yaml and seeded weights.  Run on a CPU machine that
holds a checkout of the reference, named by --reference (or REFERENCE_DIR):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_coma_golden.py --reference <reference checkout>
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_coma_golden.py --reference <reference checkout> --agents 3

The batch is learner_batch.npz (learner3_batch.npz with three agents) with the action of agent 0 repeated for every agent
(what coma.py:104-124 stores).  The draws of the counterfactual baseline (coma.py:141) are recorded by wrapping th.normal,
the critic's values by wrapping the model's own ``value``.  The fixtures are data; no reference source travels.
"""
import json
import os
import sys

import numpy as np
import torch as th
import yaml

REF = os.environ.get("REFERENCE_DIR")
if "--reference" in sys.argv:
    REF = sys.argv[sys.argv.index("--reference") + 1]
if not REF or not os.path.isdir(os.path.join(REF, "madrl")):
    sys.exit("make_coma_golden.py: name the reference checkout with --reference DIR (or REFERENCE_DIR)")
REF = os.path.abspath(REF)
OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REF)
os.chdir(REF)

from utils.util import convert, normal_log_density  # noqa: E402
from utils.trainer import PGTrainer  # noqa: E402
from madrl.models.coma import COMA  # noqa: E402

N_AGENTS = 5
if "--agents" in sys.argv:
    N_AGENTS = int(sys.argv[sys.argv.index("--agents") + 1])
OUT_DIR = os.environ.get("GOLDEN_OUT", OUT)
BATCH = "learner_batch.npz" if N_AGENTS == 5 else f"learner{N_AGENTS}_batch.npz"

DRAWS = []
_normal = th.normal


def _recording_normal(*a, **k):
    out = _normal(*a, **k)
    DRAWS.append(out.detach().clone())
    return out


th.normal = _recording_normal


def load_args():
    with open("madrl/args/default.yaml") as f:
        d = yaml.safe_load(f)
    with open("madrl/args/alg_args/coma.yaml") as f:
        a = yaml.safe_load(f)["alg_args"]
    with open("madrl/args/env_args/flex_provision.yaml") as f:
        e = yaml.safe_load(f)["env_args"]
    for k, v in (("action_low", 0.0), ("action_high", 1.0), ("action_bias", 0.0), ("action_scale", 1.0)):
        a[k] = e.get(k, v)
    a["alg"] = "coma"
    d = {**d, **a}
    d.update(agent_num=N_AGENTS, obs_size=144, state_size=3 * 33 + 2 * N_AGENTS + 1, action_dim=4, cuda=False)
    return d


class StubEnv:
    def get_num_of_agents(self):
        return N_AGENTS


def coma_batch():
    b = dict(np.load(os.path.join(OUT, BATCH)))
    b["action"] = np.repeat(b["action"][:, :1], N_AGENTS, axis=1)         # one action, every agent
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


def record_values(net, sink):
    inner = net.value

    def value(obs, act):
        out = inner(obs, act)
        sink.append(out.detach().clone())
        return out
    net.value = value


def main():
    prefix = "coma" if N_AGENTS == 5 else f"coma{N_AGENTS}"

    def save_sd(name, sd):
        np.savez_compressed(os.path.join(OUT_DIR, f"{prefix}_{name}.npz"),
                            **{k: v.detach().cpu().numpy().copy() for k, v in sd.items()})

    argd = load_args()
    args = convert(argd)
    json.dump(argd, open(os.path.join(OUT_DIR, prefix + "_args.json"), "w"), indent=1, sort_keys=True)
    th.manual_seed(2468)
    target = COMA(args)
    model = COMA(args, target)
    sd0 = {k: v.detach().clone() for k, v in model.state_dict().items()}
    tgt0 = {k: v.detach().clone() for k, v in target.state_dict().items()}
    save_sd("state_dict", sd0)
    b = coma_batch()
    g = {"batch.action": b["action"]}
    batch = transitions(model, b)

    # (1) one get_loss call (coma.py:126-189) with its intermediates
    own, tgt = [], []
    record_values(model, own)
    record_values(target, tgt)
    DRAWS.clear()
    model.zero_grad()
    policy_loss, value_loss, (means, log_stds) = model.get_loss(batch)
    assert len(DRAWS) == 1 and len(own) == 2 and len(tgt) == 1, (len(DRAWS), len(own), len(tgt))
    s, rows = args.sample_size, b["state"].shape[0]
    g["sampled"] = DRAWS[0].numpy()                                        # [s, b, n, a]
    g["values_sampled"] = own[0].view(s, rows, N_AGENTS).numpy()
    g["baselines"] = own[0].view(s, rows, N_AGENTS).mean(dim=0).numpy()
    g["values"] = own[1].view(rows, N_AGENTS).numpy()
    g["next_values"] = tgt[0].view(rows, N_AGENTS).numpy()
    g["policy_loss"], g["value_loss"], g["means"] = policy_loss.item(), value_loss.item(), means.detach().numpy()
    for name in ("running_mean", "running_var"):
        g["reward_bn." + name] = getattr(model.batchnorm, name).numpy().copy()
    g["reward_bn.num_batches_tracked"] = int(model.batchnorm.num_batches_tracked)
    value_loss.backward(retain_graph=True)
    for k, p in model.value_dicts.named_parameters():
        g["vgrad." + k] = p.grad.numpy().copy()
    assert all(p.grad is None or float(p.grad.abs().sum()) == 0.0 for p in model.policy_dicts.parameters())
    model.zero_grad()
    policy_loss.backward()
    for k, p in model.policy_dicts.named_parameters():
        g["pgrad." + k] = p.grad.numpy().copy()
    with th.no_grad():
        up = model.unpack_data(batch)              # (moves the reward BatchNorm once more: statistics recorded above)
        own.clear(), tgt.clear()
        mask = 1.0 - (up[9] == 0).float()
        g["log_prob_a"] = (mask * normal_log_density(up[1], means, log_stds)).sum(dim=-1).numpy()      # coma.py:183-185
        # coma.py:175 on the first call's reward normalisation: a fresh module sees the same batch statistics
        fresh = COMA(args, COMA(args))
        fresh.load_state_dict(sd0)
        g["reward_norm"] = fresh.unpack_data(batch)[5].numpy()
        g["returns"] = (th.from_numpy(g["reward_norm"]) + args.gamma * (1 - up[7]) * th.from_numpy(g["next_values"])).numpy()

    # (2) one value and one policy step through PGTrainer (trainer.py:81-108): each evaluates get_loss once
    th.manual_seed(2468)
    trainer = PGTrainer(args, COMA, StubEnv(), None)
    trainer.behaviour_net.load_state_dict(sd0)
    trainer.behaviour_net.target_net.load_state_dict(tgt0)
    stat = {}
    DRAWS.clear()
    trainer.value_transition_process(stat, batch)
    trainer.policy_transition_process(stat, batch)
    assert len(DRAWS) == 2
    g["step.sampled_value"], g["step.sampled_policy"] = DRAWS[0].numpy(), DRAWS[1].numpy()
    for k, v in stat.items():
        g["stat." + k] = float(v)
    save_sd("state_dict_after_step", trainer.behaviour_net.state_dict())
    g["after_step.reward_bn.running_mean"] = trainer.behaviour_net.batchnorm.running_mean.numpy().copy()
    g["after_step.reward_bn.running_var"] = trainer.behaviour_net.batchnorm.running_var.numpy().copy()

    # (3) update_target on the post-step weights (model.py:28-38)
    trainer.behaviour_net.update_target()
    save_sd("target_after_update", trainer.behaviour_net.target_net.state_dict())

    np.savez_compressed(os.path.join(OUT_DIR, prefix + "_golden.npz"), **g)
    print("wrote", sorted(f for f in os.listdir(OUT_DIR) if f.startswith(prefix + "_")))


if __name__ == "__main__":
    main()
