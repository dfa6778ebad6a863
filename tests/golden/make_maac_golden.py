#!/usr/bin/env python3
"""Generates tests/golden/maac*_*.npz by IMPORTING the reference's MAAC (madrl/models/maac.py), its AttentionCritic
(madrl/critics/maac_critic.py) and PGTrainer (utils/trainer.py) on CPU, with alg_args/maac.yaml merged over default.yaml and
seeded weights.  Run on a CPU machine that holds a checkout of the reference, named by --reference (or REFERENCE_DIR):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_maac_golden.py --reference <reference checkout>
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_maac_golden.py --reference <reference checkout> --agents 3

Two directories go on sys.path: the reference root, as for every other algorithm, and <root>/madrl beside it.  maac.py:24-29
imports its actor as ``from agents.rnn_agent_gaussian import RNNAgent`` — a path that only resolves from inside madrl/ — and
that import is the one thing that keeps the reference's MAAC from running from the root.  With madrl/ on the path it
resolves to the reference's own file and MAAC executes unmodified.

The batch is learner_batch.npz (learner3_batch.npz with three agents).  The target's weights are moved away from the
behaviour net's after construction, so that the next actions' coming from the TARGET policy (maac.py:96) shows in the
numbers.  The exploration draws of get_loss — two ``Normal.rsample`` calls, maac.py:95-96 — are recorded by wrapping
torch.distributions.normal._standard_normal, the function rsample draws from (th.normal is wrapped as well: nothing of MAAC
calls it).  The fixtures are data; no reference source travels.
"""
import json
import os
import sys

import numpy as np
import torch as th
import torch.distributions.normal as tdn
import yaml

REF = os.environ.get("REFERENCE_DIR")
if "--reference" in sys.argv:
    REF = sys.argv[sys.argv.index("--reference") + 1]
if not REF or not os.path.isdir(os.path.join(REF, "madrl")):
    sys.exit("make_maac_golden.py: name the reference checkout with --reference DIR (or REFERENCE_DIR)")
REF = os.path.abspath(REF)
OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(REF, "madrl"))
sys.path.insert(0, REF)
os.chdir(REF)

from utils.util import convert  # noqa: E402
from utils.trainer import PGTrainer  # noqa: E402
from madrl.models.maac import MAAC  # noqa: E402

N_AGENTS = 5
if "--agents" in sys.argv:
    N_AGENTS = int(sys.argv[sys.argv.index("--agents") + 1])
OUT_DIR = os.environ.get("GOLDEN_OUT", OUT)
BATCH = "learner_batch.npz" if N_AGENTS == 5 else f"learner{N_AGENTS}_batch.npz"

DRAWS = []
_normal, _standard_normal = th.normal, tdn._standard_normal


def _recording_normal(*a, **k):
    out = _normal(*a, **k)
    DRAWS.append(out.detach().clone())
    return out


def _recording_standard_normal(*a, **k):
    out = _standard_normal(*a, **k)
    DRAWS.append(out.detach().clone())
    return out


th.normal = _recording_normal
tdn._standard_normal = _recording_standard_normal


def load_args():
    with open("madrl/args/default.yaml") as f:
        d = yaml.safe_load(f)
    with open("madrl/args/alg_args/maac.yaml") as f:
        a = yaml.safe_load(f)["alg_args"]
    with open("madrl/args/env_args/flex_provision.yaml") as f:
        e = yaml.safe_load(f)["env_args"]
    for k, v in (("action_low", 0.0), ("action_high", 1.0), ("action_bias", 0.0), ("action_scale", 1.0)):
        a[k] = e.get(k, v)
    a["alg"] = "maac"
    d = {**d, **a}
    d.update(agent_num=N_AGENTS, obs_size=144, state_size=3 * 33 + 2 * N_AGENTS + 1, action_dim=4, cuda=False)
    return d


class StubEnv:
    def get_num_of_agents(self):
        return N_AGENTS


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


def own_entries(sd):
    return {k: v.detach().clone() for k, v in sd.items() if not k.startswith("target_net.")}


def main():
    prefix = "maac" if N_AGENTS == 5 else f"maac{N_AGENTS}"

    def save(name, sd):
        np.savez_compressed(os.path.join(OUT_DIR, f"{prefix}_{name}.npz"),
                            **{k: v.detach().cpu().numpy().copy() for k, v in sd.items()})

    argd = load_args()
    args = convert(argd)
    assert args.gaussian_policy and args.soft and args.attend_heads == 1 and not args.norm_in
    json.dump(argd, open(os.path.join(OUT_DIR, prefix + "_args.json"), "w"), indent=1, sort_keys=True)
    th.manual_seed(8642)
    target = MAAC(args)
    model = MAAC(args, target)
    with th.no_grad():                                  # a target that is not the behaviour net
        for p in list(target.policy_dicts.parameters()) + list(target.value_dicts.parameters()):
            p.add_(0.03 * th.randn_like(p))
    assert len(model.value_dicts) == 1
    sd0, tgt0 = own_entries(model.state_dict()), own_entries(target.state_dict())
    save("state_dict", sd0)
    save("target_state_dict", tgt0)
    b = dict(np.load(os.path.join(OUT, BATCH)))
    rows = b["state"].shape[0]
    g = {}
    batch = transitions(model, b)

    # (1) value(state, actions): [b + 1, n], the last row the attention regulariser
    with th.no_grad():
        state = th.tensor(b["state"]).float()
        action = th.tensor(b["action"]).float()
        g["value"] = model.value(state, action).numpy()
    assert g["value"].shape == (rows + 1, N_AGENTS)

    # (2) one get_loss call (maac.py:92-119) with its two draws
    DRAWS.clear()
    model.zero_grad()
    policy_loss, value_loss, (means, log_stds) = model.get_loss(batch)
    assert len(DRAWS) == 2, len(DRAWS)
    g["draws.behaviour"], g["draws.target"] = DRAWS[0].numpy(), DRAWS[1].numpy()      # [b, 1, a] each
    g["policy_loss"], g["value_loss"] = policy_loss.item(), value_loss.item()
    g["means"], g["log_stds"] = means.detach().numpy(), log_stds.detach().numpy()
    value_loss.backward(retain_graph=True)
    for k, p in model.value_dicts.named_parameters():
        g["vgrad." + k] = p.grad.numpy().copy()
    model.zero_grad()
    policy_loss.backward()
    for k, p in model.policy_dicts.named_parameters():
        g["pgrad." + k] = p.grad.numpy().copy()
    with th.no_grad():                                  # log_prob_a [b, n] of maac.py:77-80 on the recorded draw
        fresh = MAAC(args, MAAC(args))
        fresh.load_state_dict(model.state_dict())
        up = fresh.unpack_data(batch)
        tdn._standard_normal = lambda *a, **k: DRAWS[0].clone()
        g["log_prob_a"] = fresh.get_actions(up[0], status="train", exploration=True, actions_avail=up[9], target=False,
                                            last_hid=up[10])[2].numpy()
        tdn._standard_normal = _recording_standard_normal
    assert g["log_prob_a"].shape == (rows, N_AGENTS)
    vgrads = {k: g.pop(k) for k in list(g) if k.startswith("vgrad.")}
    np.savez_compressed(os.path.join(OUT_DIR, prefix + "_golden_vgrads.npz"), **vgrads)

    # (3) one value and one policy step through PGTrainer (trainer.py:81-108): each evaluates get_loss once
    th.manual_seed(8642)
    trainer = PGTrainer(args, MAAC, StubEnv(), None)
    net = trainer.behaviour_net
    net.load_state_dict({**sd0, **{"target_net." + k: v for k, v in tgt0.items()}})
    stat = {}
    DRAWS.clear()
    trainer.value_transition_process(stat, batch)
    trainer.policy_transition_process(stat, batch)
    assert len(DRAWS) == 4
    for i, k in enumerate(("value.behaviour", "value.target", "policy.behaviour", "policy.target")):
        g["step.draws." + k] = DRAWS[i].numpy()
    for k, v in stat.items():
        g["stat." + k] = float(v)
    for k, v in own_entries(net.target_net.state_dict()).items():       # the steps leave the target's nets alone
        assert k.startswith("batchnorm.") or th.equal(v, tgt0[k]), k
    save("state_dict_after_step", own_entries(net.state_dict()))

    # (4) update_target on the post-step weights (model.py:28-38)
    net.update_target()
    save("target_after_update", own_entries(net.target_net.state_dict()))

    np.savez_compressed(os.path.join(OUT_DIR, prefix + "_golden.npz"), **g)
    print("wrote", sorted((f, os.path.getsize(os.path.join(OUT_DIR, f))) for f in os.listdir(OUT_DIR) if f.startswith(prefix + "_")))


if __name__ == "__main__":
    main()
