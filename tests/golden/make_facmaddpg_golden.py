#!/usr/bin/env python3
"""Generates tests/golden/facmaddpg*_*.npz by IMPORTING the reference's FACMADDPG (madrl/models/facmaddpg.py), QMixer
(madrl/critics/qmix.py) and PGTrainer (utils/trainer.py) on CPU, with alg_args/facmaddpg.yaml merged over default.yaml,
seeded weights and the replay batch of learner_batch.npz (learner3_batch.npz with three agents).  Run on a CPU machine
that holds a checkout of the reference, named by --reference (or the REFERENCE_DIR environment variable):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_facmaddpg_golden.py --reference <reference checkout>
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_facmaddpg_golden.py --reference <reference checkout> --agents 3

Every state_dict is split into its mixer part (``*_mixer.npz``) and the rest, so that no fixture exceeds 1 MiB.  The fixtures are data (inputs + expected outputs); no reference source travels.
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
    sys.exit("make_facmaddpg_golden.py: name the reference checkout with --reference DIR (or REFERENCE_DIR)")
REF = os.path.abspath(REF)
OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REF)
os.chdir(REF)

from utils.util import convert  # noqa: E402
from utils.trainer import PGTrainer  # noqa: E402
from madrl.models.facmaddpg import FACMADDPG  # noqa: E402

N_AGENTS = 5
if "--agents" in sys.argv:
    N_AGENTS = int(sys.argv[sys.argv.index("--agents") + 1])
OUT_DIR = os.environ.get("GOLDEN_OUT", OUT)
PREFIX = "facmaddpg" if N_AGENTS == 5 else f"facmaddpg{N_AGENTS}"
BATCH = "learner_batch.npz" if N_AGENTS == 5 else f"learner{N_AGENTS}_batch.npz"


def load_args():
    with open("madrl/args/default.yaml") as f:
        d = yaml.safe_load(f)
    with open("madrl/args/alg_args/facmaddpg.yaml") as f:
        a = yaml.safe_load(f)["alg_args"]
    with open("madrl/args/env_args/flex_provision.yaml") as f:
        e = yaml.safe_load(f)["env_args"]
    for k, v in (("action_low", 0.0), ("action_high", 1.0), ("action_bias", 0.0), ("action_scale", 1.0)):
        a[k] = e.get(k, v)
    a["alg"] = "facmaddpg"
    d = {**d, **a}
    d.update(agent_num=N_AGENTS, obs_size=144, state_size=3 * 33 + 2 * N_AGENTS + 1, action_dim=4, cuda=False)
    return d


class StubEnv:
    def get_num_of_agents(self):
        return N_AGENTS


def save_sd(name, sd):
    """state_dict -> <PREFIX>_<name>.npz (everything but the mixers) and <PREFIX>_<name>_mixer.npz (``mixer.*``).  The target
    replica's mixer (``target_net.mixer.*``) is left out: in the behaviour net's state_dict it is the initial mixer
    (reload_params_to_target, and no step moves it)."""
    sd = {k: v.detach().cpu().numpy().copy() for k, v in sd.items()}
    np.savez_compressed(os.path.join(OUT_DIR, f"{PREFIX}_{name}.npz"), **{k: v for k, v in sd.items() if "mixer." not in k})
    np.savez_compressed(os.path.join(OUT_DIR, f"{PREFIX}_{name}_mixer.npz"), **{k: v for k, v in sd.items() if k.startswith("mixer.")})


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


def main():
    argd = load_args()
    args = convert(argd)
    json.dump(argd, open(os.path.join(OUT_DIR, PREFIX + "_args.json"), "w"), indent=1, sort_keys=True)
    g, gm = {}, {}
    th.manual_seed(1357)
    target = FACMADDPG(args)
    model = FACMADDPG(args, target)
    sd0 = {k: v.detach().clone() for k, v in model.state_dict().items()}
    assert all(th.equal(v, sd0["target_net." + k]) for k, v in sd0.items() if k.startswith("mixer."))
    tgt0 = {k: v.detach().clone() for k, v in target.state_dict().items()}
    save_sd("state_dict", sd0)
    batch = transitions(model, dict(np.load(os.path.join(OUT, BATCH))))
    n, o = N_AGENTS, 144

    # (1) value(), q_tot, next_q_tot on the batch (facmaddpg.py:36-61, 85-102)
    with th.no_grad():
        up = model.unpack_data(batch)
        state, actions, next_state, hids = up[0], up[1], up[6], up[11]
        b = state.size(0)
        values = model.value(state, actions)
        g["value"] = values.numpy()
        g["q_tot"] = model.mixer(values.view(-1, n), state.reshape(b, n * o)).view(-1, 1).numpy()
        _, next_actions, _, _, _ = model.get_actions(next_state, status="train", exploration=False,
                                                     actions_avail=up[9], target=False, last_hid=hids)
        nv = model.target_net.value(next_state, next_actions).view(-1, n)
        g["next_q_tot"] = model.target_net.mixer(nv, next_state.reshape(b, n * o)).view(-1, 1).numpy()

    # (2) both losses and their gradients (facmaddpg.py:85-114)
    model.load_state_dict(sd0)
    policy_loss, value_loss, _ = model.get_loss(batch)
    g["policy_loss"], g["value_loss"] = policy_loss.item(), value_loss.item()
    model.zero_grad()
    value_loss.backward()
    for k, p in model.value_dicts.named_parameters():
        g["vgrad." + k] = p.grad.numpy().copy()
    for k, p in model.mixer.named_parameters():
        gm["mgrad." + k] = p.grad.numpy().copy()
    policy_loss2, _, _ = model.get_loss(batch)
    model.zero_grad()
    policy_loss2.backward()
    for k, p in model.policy_dicts.named_parameters():
        g["pgrad." + k] = p.grad.numpy().copy()

    # (3) one value, one policy and one mixer step through PGTrainer (trainer.py:81-119)
    th.manual_seed(1357)
    trainer = PGTrainer(args, FACMADDPG, StubEnv(), None)
    trainer.behaviour_net.load_state_dict(sd0)
    trainer.behaviour_net.target_net.load_state_dict(tgt0)
    stat = {}
    trainer.value_transition_process(stat, batch)
    trainer.policy_transition_process(stat, batch)
    trainer.mixer_transition_process(stat, batch)
    for k, v in stat.items():
        g["stat." + k] = float(v)
    save_sd("state_dict_after_step", trainer.behaviour_net.state_dict())

    # (4) update_target on the post-step weights (model.py:28-38, mixer included)
    trainer.behaviour_net.update_target()
    save_sd("target_after_update", trainer.behaviour_net.target_net.state_dict())

    np.savez_compressed(os.path.join(OUT_DIR, PREFIX + "_golden.npz"), **g)
    np.savez_compressed(os.path.join(OUT_DIR, PREFIX + "_golden_mixer_grads.npz"), **gm)
    print("wrote", sorted(f for f in os.listdir(OUT_DIR) if f.startswith(PREFIX + "_")))


if __name__ == "__main__":
    main()
