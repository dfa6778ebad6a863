#!/usr/bin/env python3
"""Generates tests/golden/sqddpg*_*.npz by IMPORTING the reference's SQDDPG (madrl/models/sqddpg.py) and PGTrainer
(utils/trainer.py) on CPU, with alg_args/sqddpg.yaml merged over default.yaml, seeded weights and the replay batch of
learner_batch.npz (learner3_batch.npz with three agents).  Run on a CPU machine that holds a checkout of the reference,
named by --reference (or the REFERENCE_DIR environment variable):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_sqddpg_golden.py --reference <reference checkout>
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_sqddpg_golden.py --reference <reference checkout> --agents 3

Every coalition draw (th.multinomial in sample_grandcoalitions) is recorded and labelled by its role: get_loss evaluates
the policy term, the value term and the target term in that order, value() draws once.  The tests replay them through
SQDDPG.coalition_source.  The fixtures are data (inputs + expected outputs); no reference source travels.
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
    sys.exit("make_sqddpg_golden.py: name the reference checkout with --reference DIR (or REFERENCE_DIR)")
REF = os.path.abspath(REF)
OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REF)
os.chdir(REF)

from utils.util import convert  # noqa: E402
from utils.trainer import PGTrainer  # noqa: E402
from madrl.models.sqddpg import SQDDPG  # noqa: E402

N_AGENTS = 5
if "--agents" in sys.argv:
    N_AGENTS = int(sys.argv[sys.argv.index("--agents") + 1])
OUT_DIR = os.environ.get("GOLDEN_OUT", OUT)
PREFIX = "sqddpg" if N_AGENTS == 5 else f"sqddpg{N_AGENTS}"
BATCH = "learner_batch.npz" if N_AGENTS == 5 else f"learner{N_AGENTS}_batch.npz"
ROLES = ("policy", "value", "target")              # the order of get_loss's three marginal_contribution calls

DRAWS = []
_multinomial = th.multinomial


def _recording_multinomial(*a, **k):
    out = _multinomial(*a, **k)
    DRAWS.append(out.clone())
    return out


th.multinomial = _recording_multinomial


def load_args():
    with open("madrl/args/default.yaml") as f:
        d = yaml.safe_load(f)
    with open("madrl/args/alg_args/sqddpg.yaml") as f:
        a = yaml.safe_load(f)["alg_args"]
    with open("madrl/args/env_args/flex_provision.yaml") as f:
        e = yaml.safe_load(f)["env_args"]
    for k, v in (("action_low", 0.0), ("action_high", 1.0), ("action_bias", 0.0), ("action_scale", 1.0)):
        a[k] = e.get(k, v)
    a["alg"] = "sqddpg"
    d = {**d, **a}
    d.update(agent_num=N_AGENTS, obs_size=144, state_size=3 * 33 + 2 * N_AGENTS + 1, action_dim=4, cuda=False)
    return d


class StubEnv:
    def get_num_of_agents(self):
        return N_AGENTS


def save_sd(name, sd):
    np.savez_compressed(os.path.join(OUT_DIR, f"{PREFIX}_{name}.npz"),
                        **{k: v.detach().cpu().numpy().copy() for k, v in sd.items()})


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


def take_draws(label, g, roles):
    assert len(DRAWS) == len(roles), (label, len(DRAWS))
    for role, d in zip(roles, DRAWS):
        g[f"pos.{label}.{role}"] = d.numpy().astype(np.int64)
    DRAWS.clear()


def main():
    argd = load_args()
    args = convert(argd)
    json.dump(argd, open(os.path.join(OUT_DIR, PREFIX + "_args.json"), "w"), indent=1, sort_keys=True)
    g = {}
    th.manual_seed(1357)
    target = SQDDPG(args)
    model = SQDDPG(args, target)
    sd0 = {k: v.detach().clone() for k, v in model.state_dict().items()}
    tgt0 = {k: v.detach().clone() for k, v in target.state_dict().items()}
    save_sd("state_dict", sd0)
    batch = transitions(model, dict(np.load(os.path.join(OUT, BATCH))))
    n = N_AGENTS
    DRAWS.clear()

    # (1) value() = marginal_contribution [b, ns, n, 1], phi, S, and S' of the target critic (sqddpg.py:63-107, 136-147)
    with th.no_grad():
        up = model.unpack_data(batch)
        state, actions, next_state, hids = up[0], up[1], up[6], up[11]
        values = model.value(state, actions)
        take_draws("call", g, ("value",))
        g["value"] = values.numpy()
        phi = values.mean(dim=1).contiguous().view(-1, n)
        g["phi"] = phi.numpy()
        g["S"] = phi.sum(dim=-1).numpy()
        _, next_actions, _, _, _ = model.get_actions(next_state, status="train", exploration=False,
                                                     actions_avail=up[9], target=False, last_hid=hids)
        nphi = model.target_net.marginal_contribution(next_state, next_actions).mean(dim=1).contiguous().view(-1, n)
        take_draws("call", g, ("target",))
        g["S_next"] = nphi.sum(dim=-1).numpy()

    # (2) both losses and their gradients from ONE get_loss call (sqddpg.py:131-158)
    model.load_state_dict(sd0)
    policy_loss, value_loss, _ = model.get_loss(batch)
    take_draws("loss", g, ROLES)
    g["policy_loss"], g["value_loss"] = policy_loss.item(), value_loss.item()
    model.zero_grad()
    value_loss.backward(retain_graph=True)
    for k, p in model.value_dicts.named_parameters():
        g["vgrad." + k] = p.grad.numpy().copy()
    model.zero_grad()
    policy_loss.backward()
    for k, p in model.policy_dicts.named_parameters():
        g["pgrad." + k] = p.grad.numpy().copy()

    # (3) one value and one policy step through PGTrainer (trainer.py:81-108): each evaluates get_loss once
    th.manual_seed(1357)
    trainer = PGTrainer(args, SQDDPG, StubEnv(), None)
    trainer.behaviour_net.load_state_dict(sd0)
    trainer.behaviour_net.target_net.load_state_dict(tgt0)
    DRAWS.clear()
    stat = {}
    trainer.value_transition_process(stat, batch)
    take_draws("vstep", g, ROLES)
    trainer.policy_transition_process(stat, batch)
    take_draws("pstep", g, ROLES)
    for k, v in stat.items():
        g["stat." + k] = float(v)
    save_sd("state_dict_after_step", trainer.behaviour_net.state_dict())

    # (4) update_target on the post-step weights (model.py:28-38)
    trainer.behaviour_net.update_target()
    save_sd("target_after_update", trainer.behaviour_net.target_net.state_dict())

    np.savez_compressed(os.path.join(OUT_DIR, PREFIX + "_golden.npz"), **g)
    print("wrote", sorted(f for f in os.listdir(OUT_DIR) if f.startswith(PREFIX + "_")))


if __name__ == "__main__":
    main()
