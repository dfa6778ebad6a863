#!/usr/bin/env python3
"""Generates tests/golden/matd3_unshared_*.{json,npz} by IMPORTING the reference's MATD3 and PGTrainer (utils/trainer.py) on
CPU with ``shared_params: False`` (default.yaml:26) — one RNNAgent and one twin-flag critic per agent, matd3.py:24-27 and
matd3.py:74-82 — under ``agent_type: "rnn"`` and ``agent_id: True``, merged over default.yaml and matd3.yaml, with seeded
weights.  The recipe of make_unshared_golden.py: three agents, the batch of learner3_batch.npz.  Run on a CPU machine that
holds a checkout of the reference, named by --reference (or REFERENCE_DIR):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_unshared_matd3_golden.py --reference <reference checkout>

What differs from make_unshared_golden.py: MATD3's target-smoothing noise comes from ``Normal.rsample``, which draws through
``torch.distributions.normal._standard_normal`` and never through ``th.normal`` — that function is hooked here and the draws
are stored: ``sampled`` for the one draw of a get_loss call, ``step.sampled_value`` and ``step.sampled_policy`` for the two
draws of the PGTrainer steps (each step evaluates get_loss once).  ``value`` is ``model.value(state, action)``, [2b, n, 1]:
cat([Q1, Q2], 0).  The state_dict files hold the model's own entries; its ``target_net.*`` entries equal the initial own ones
in both (asserted here).  The fixtures are data; no reference source travels.  Each file stays below the largest fixture the
repository already keeps (asserted).  Running it twice writes the same bytes.
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
    sys.exit("make_unshared_matd3_golden.py: name the reference checkout with --reference DIR (or REFERENCE_DIR)")
REF = os.path.abspath(REF)
OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REF)
os.chdir(REF)

from utils.util import convert, normal_entropy  # noqa: E402
from utils.trainer import PGTrainer  # noqa: E402
from madrl.models.matd3 import MATD3  # noqa: E402

N_AGENTS = 3
SEED = 6925
PREFIX = "matd3_unshared"
OUT_DIR = os.environ.get("GOLDEN_OUT", OUT)

DRAWS = []
_standard_normal = tdn._standard_normal


def _recording_standard_normal(*a, **k):
    out = _standard_normal(*a, **k)
    DRAWS.append(out.detach().clone())
    return out


tdn._standard_normal = _recording_standard_normal


def load_args(**over):
    with open("madrl/args/default.yaml") as f:
        d = yaml.safe_load(f)
    with open("madrl/args/alg_args/matd3.yaml") as f:
        a = yaml.safe_load(f)["alg_args"]
    with open("madrl/args/env_args/flex_provision.yaml") as f:
        e = yaml.safe_load(f)["env_args"]
    for k, v in (("action_low", 0.0), ("action_high", 1.0), ("action_bias", 0.0), ("action_scale", 1.0)):
        a[k] = e.get(k, v)
    a["alg"] = "matd3"
    d = {**d, **a}
    d.update(agent_num=N_AGENTS, obs_size=144, state_size=3 * 33 + 2 * N_AGENTS + 1, action_dim=4, cuda=False,
             agent_type="rnn", shared_params=False, agent_id=True, **over)
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


def main():
    def save_sd(name, sd, target_of):
        own = {k: v.detach().cpu().numpy().copy() for k, v in sd.items() if not k.startswith("target_net.")}
        for k, v in sd.items():
            if k.startswith("target_net."):
                assert np.array_equal(v.detach().cpu().numpy(), target_of[k[len("target_net."):]].detach().cpu().numpy()), k
        np.savez_compressed(os.path.join(OUT_DIR, f"{PREFIX}_{name}.npz"), **own)

    argd = load_args(gaussian_policy=False)
    args = convert(argd)
    assert args.agent_type == "rnn" and not args.shared_params and args.agent_id and args.entr > 0
    json.dump(argd, open(os.path.join(OUT_DIR, PREFIX + "_args.json"), "w"), indent=1, sort_keys=True)
    th.manual_seed(SEED)
    target = MATD3(args)
    model = MATD3(args, target)
    o, a = args.obs_size, args.action_dim
    assert len(model.value_dicts) == N_AGENTS
    assert all(c.fc1.weight.shape[1] == (o + a) * N_AGENTS + N_AGENTS + 1 for c in model.value_dicts)
    sd0 = {k: v.detach().clone() for k, v in model.state_dict().items()}
    tgt0 = {k: v.detach().clone() for k, v in target.state_dict().items()}
    save_sd("state_dict", sd0, sd0)
    b = dict(np.load(os.path.join(OUT, "learner3_batch.npz")))
    g = {}
    batch = transitions(model, b)

    # (1) policy() and value() on the batch
    with th.no_grad():
        up = MATD3(args, MATD3(args)).unpack_data(batch)             # (a throw-away module: its BatchNorm moves, not the model's)
        means, log_stds, hiddens = model.policy(up[0], last_hid=up[10])
        g["value"] = model.value(up[0], up[1]).numpy()
    assert g["value"].shape == (2 * b["state"].shape[0], N_AGENTS, 1)
    g["policy_means"], g["policy_log_stds"], g["policy_hiddens"] = means.numpy(), log_stds.numpy(), hiddens.numpy()

    # (2) one get_loss call: the losses, the value gradients of the value loss, the policy gradients of the trainer's loss
    DRAWS.clear()
    model.zero_grad()
    policy_loss, value_loss, (means, log_stds) = model.get_loss(batch)
    assert len(DRAWS) == 1, len(DRAWS)
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
    w1 = o * N_AGENTS
    for i in range(N_AGENTS):      # the one-hot input and the twin flag of agent i's critic
        w = g[f"vgrad.{i}.fc1.weight"]
        ids = w[:, w1:w1 + N_AGENTS]
        assert np.all(np.delete(ids, i, axis=1) == 0.0) and np.allclose(ids[:, i], g[f"vgrad.{i}.fc1.bias"], atol=1e-8, rtol=1e-5)
        assert np.abs(w[:, -1]).max() > 0

    # (3) one value and one policy step through PGTrainer (trainer.py:81-108): each evaluates get_loss once
    th.manual_seed(SEED)
    trainer = PGTrainer(args, MATD3, StubEnv(), None)
    trainer.behaviour_net.load_state_dict(sd0)
    trainer.behaviour_net.target_net.load_state_dict(tgt0)
    stat = {}
    DRAWS.clear()
    trainer.value_transition_process(stat, batch)
    trainer.policy_transition_process(stat, batch)
    assert len(DRAWS) == 2, len(DRAWS)
    g["step.sampled_value"], g["step.sampled_policy"] = DRAWS[0].numpy(), DRAWS[1].numpy()
    for k, v in stat.items():
        g["stat." + k] = float(v)
    save_sd("state_dict_after_step", trainer.behaviour_net.state_dict(), sd0)

    np.savez_compressed(os.path.join(OUT_DIR, PREFIX + "_golden.npz"), **g)
    written = sorted(f for f in os.listdir(OUT_DIR) if f.startswith(PREFIX + "_"))
    largest = max(os.path.getsize(os.path.join(OUT, f)) for f in os.listdir(OUT) if not f.startswith(PREFIX + "_")
                  and not f.endswith(".py"))
    for f in written:
        assert os.path.getsize(os.path.join(OUT_DIR, f)) < largest, (f, os.path.getsize(os.path.join(OUT_DIR, f)), largest)
    print("wrote", written)


if __name__ == "__main__":
    main()
