#!/usr/bin/env python3
"""Generates tests/golden/per_agent/unshared_{mlp_maddpg,mlp_ippo,gauss_ippo,mlp_gauss_ippo}_* by IMPORTING the reference's
MADDPG / IPPO and PGTrainer (utils/trainer.py) on CPU with ``shared_params: False`` (default.yaml:26; one agent module and one
critic per agent, madrl/models/model.py:124-138) for the agent classes make_unshared_golden.py leaves out: ``agent_type:
"mlp"`` (madrl/agents/mlp_agent.py) and ``gaussian_policy: True`` (madrl/agents/{rnn,mlp}_agent_gaussian.py), under ``agent_id:
True``, merged over default.yaml and the algorithm's yaml, with seeded weights.  Run on a CPU machine that holds a checkout of
the reference, named by --reference (or REFERENCE_DIR):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_unshared_agents_golden.py --reference <reference checkout>

Three agents and the batch of learner3_batch.npz with the fields the on-policy algorithm's own fixtures replace (recorded as
``batch.*``), as make_unshared_golden.py.  Four families, one per way a gradient reaches the per-agent actors:

    unshared_mlp_maddpg       MLP agents; through the critic
    unshared_mlp_ippo         MLP agents; PPO's loss at the means
    unshared_gauss_ippo       RNN agents with log-std heads; at the means and, through the head, at the new hidden state
    unshared_mlp_gauss_ippo   MLP agents with log-std heads; at the means and, through the head, at h

The Gaussian families take make_gaussian_golden.py's override (``gaussian_policy=True``; LOG_STD_MIN / LOG_STD_MAX of
default.yaml).  Per family the content is make_unshared_golden.py's: the arguments, the initial state_dict, ``policy()`` on the
batch, both losses, every value gradient of the value loss and every policy gradient of the loss the trainer steps on, then
``stat`` and the state_dict after one value and one policy step through PGTrainer.  The files live in their own directory
(``per_agent/``): tests/test_unshared_cpu.py counts the ``unshared_*`` files next to this script.  The fixtures are data; no
reference source travels.  Running it twice writes the same bytes (numpy's zip entries carry a fixed date).
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
    sys.exit("make_unshared_agents_golden.py: name the reference checkout with --reference DIR (or REFERENCE_DIR)")
REF = os.path.abspath(REF)
OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REF)
os.chdir(REF)

from utils.util import convert, normal_entropy  # noqa: E402
from utils.trainer import PGTrainer  # noqa: E402
from madrl.models.maddpg import MADDPG  # noqa: E402
from madrl.models.ippo import IPPO  # noqa: E402

N_AGENTS = 3
OUT_DIR = os.environ.get("GOLDEN_OUT", os.path.join(OUT, "per_agent"))

DRAWS = []
_normal = th.normal


def _recording_normal(*a, **k):
    out = _normal(*a, **k)
    DRAWS.append(out.detach().clone())
    return out


th.normal = _recording_normal


def load_args(alg, **over):
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
    d.update(agent_num=N_AGENTS, obs_size=144, state_size=3 * 33 + 2 * N_AGENTS + 1, action_dim=4, cuda=False,
             shared_params=False, agent_id=True, **over)
    return d


class StubEnv:
    def get_num_of_agents(self):
        return N_AGENTS


def batch_arrays(alg):
    b = dict(np.load(os.path.join(OUT, "learner3_batch.npz")))
    replaced = {}
    if alg == "ippo":                              # ippo.py:72-73 stores one action for every agent
        b["action"] = replaced["action"] = np.repeat(b["action"][:, :1], N_AGENTS, axis=1)
        rows = b["state"].shape[0]                 # every branch of the GAE mask (ppo.py:45-48), as make_ppo_golden.py
        done, last = np.zeros(rows), np.zeros(rows)
        last[[6, 13, 20, rows - 1]] = 1.0
        done[[13]] = 1.0
        last[[25]], done[[25]] = 1.0, 1.0
        b["done"], b["last_step"] = done, last
        replaced.update(done=done, last_step=last)
    return b, replaced


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


def main(alg, cls, seed, prefix, **over):
    def save_sd(name, sd, target_of):
        """Without the ``target_net.*`` entries, which must equal ``target_of``'s own (the initial weights: the target is a
        copy at construction and no update_target runs here) — the tests put them back before the strict load."""
        own = {k: v.detach().cpu().numpy().copy() for k, v in sd.items() if not k.startswith("target_net.")}
        for k, v in sd.items():
            if k.startswith("target_net."):
                assert np.array_equal(v.detach().cpu().numpy(), target_of[k[len("target_net."):]].detach().cpu().numpy()), k
        np.savez_compressed(os.path.join(OUT_DIR, f"{prefix}_{name}.npz"), **own)

    os.makedirs(OUT_DIR, exist_ok=True)
    argd = load_args(alg, **over)
    args = convert(argd)
    assert not args.shared_params and args.agent_id and args.entr > 0
    json.dump(argd, open(os.path.join(OUT_DIR, prefix + "_args.json"), "w"), indent=1, sort_keys=True)
    th.manual_seed(seed)
    target = cls(args)
    model = cls(args, target)
    sd0 = {k: v.detach().clone() for k, v in model.state_dict().items()}
    tgt0 = {k: v.detach().clone() for k, v in target.state_dict().items()}
    save_sd("state_dict", sd0, sd0)
    b, replaced = batch_arrays(alg)
    g = {"batch." + k: v for k, v in replaced.items()}
    batch = transitions(model, b)

    # (1) policy() on the batch (model.py:102-140)
    with th.no_grad():
        up = cls(args, cls(args)).unpack_data(batch)                 # (a throw-away module: its BatchNorm moves, not the model's)
        means, log_stds, hiddens = model.policy(up[0], last_hid=up[10])
    g["policy_means"], g["policy_log_stds"], g["policy_hiddens"] = means.numpy(), log_stds.numpy(), hiddens.numpy()

    # (2) one get_loss call: the losses, the value gradients of the value loss, the policy gradients of the trainer's loss
    DRAWS.clear()
    model.zero_grad()
    policy_loss, value_loss, (means, log_stds) = model.get_loss(batch)
    if DRAWS:
        g["sampled"] = DRAWS[0].numpy()
    g["policy_loss"], g["value_loss"] = policy_loss.item(), value_loss.item()
    g["means"], g["log_stds"] = means.detach().numpy(), log_stds.detach().numpy()
    value_loss.backward(retain_graph=True)
    for k, p in model.value_dicts.named_parameters():
        g["vgrad." + k] = p.grad.numpy().copy()
    model.zero_grad()
    entropy = normal_entropy(means, log_stds.exp())
    g["entropy"] = entropy.item()
    (policy_loss - args.entr * entropy).backward()                    # trainer.py:47-57
    for k, p in model.policy_dicts.named_parameters():
        g["pgrad." + k] = p.grad.numpy().copy()
    assert all(np.abs(v).max() > 0 for k, v in g.items() if k.startswith("pgrad.")), "a policy gradient is identically zero"
    assert len(model.policy_dicts) == len(model.value_dicts) == N_AGENTS
    if args.gaussian_policy:
        assert f"pgrad.{N_AGENTS - 1}.log_std.weight" in g
    o = args.obs_size
    for a in range(N_AGENTS):      # the one-hot input: agent a's id block is zero off its own column, which is its bias gradient
        ids = g[f"pgrad.{a}.fc1.weight"][:, o:]
        assert np.all(np.delete(ids, a, axis=1) == 0.0) and np.allclose(ids[:, a], g[f"pgrad.{a}.fc1.bias"], atol=1e-8, rtol=1e-6)

    # (3) one value and one policy step through PGTrainer (trainer.py:81-108): each evaluates get_loss once
    th.manual_seed(seed)
    trainer = PGTrainer(args, cls, StubEnv(), None)
    trainer.behaviour_net.load_state_dict(sd0)
    trainer.behaviour_net.target_net.load_state_dict(tgt0)
    stat = {}
    DRAWS.clear()
    trainer.value_transition_process(stat, batch)
    trainer.policy_transition_process(stat, batch)
    if DRAWS:
        assert len(DRAWS) == 2
        g["step.sampled_value"], g["step.sampled_policy"] = DRAWS[0].numpy(), DRAWS[1].numpy()
    for k, v in stat.items():
        g["stat." + k] = float(v)
    save_sd("state_dict_after_step", trainer.behaviour_net.state_dict(), sd0)

    np.savez_compressed(os.path.join(OUT_DIR, prefix + "_golden.npz"), **g)
    print("wrote", sorted(f for f in os.listdir(OUT_DIR) if f.startswith(prefix + "_")))


if __name__ == "__main__":
    main("maddpg", MADDPG, 6925, "unshared_mlp_maddpg", agent_type="mlp", gaussian_policy=False)
    main("ippo", IPPO, 7036, "unshared_mlp_ippo", agent_type="mlp", gaussian_policy=False)
    main("ippo", IPPO, 8147, "unshared_gauss_ippo", agent_type="rnn", gaussian_policy=True)
    main("ippo", IPPO, 9258, "unshared_mlp_gauss_ippo", agent_type="mlp", gaussian_policy=True)
