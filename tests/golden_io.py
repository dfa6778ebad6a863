"""The loaders of tests/golden that the learner-class tests share: plain functions, one copy each.  ``prefix`` names a
fixture family (learner, learner3, facmaddpg, sqddpg3, ippo, coma3, ...); a prefix ending in 3 is the three-agent one."""
import json
import os
import socket

import numpy as np
import torch as th

G = os.path.join(os.path.dirname(__file__), "golden")


def golden_args(prefix="learner", cuda=False, **over):
    from safe_marl_amd.util import convert
    d = json.load(open(os.path.join(G, prefix + "_args.json")))
    d.update(dict(cuda=True) if cuda else {}, **over)
    return convert(d)


def golden_tensors(name, device="cpu"):
    z = np.load(os.path.join(G, name))
    return {k: th.from_numpy(z[k]).to(device) for k in z.files}


def golden_vectors(prefix):
    return dict(np.load(os.path.join(G, prefix + "_golden.npz")))


def golden_batch(prefix="learner", device="cpu", tile=1, gold=None, fields=()):
    """learner_batch.npz (learner3_batch.npz for a three-agent prefix) as a Transition, repeated ``tile`` times along the
    batch axis, with ``fields`` taken from ``gold`` (what the on-policy algorithms' reference runs stored instead)."""
    from safe_marl_amd.replay_buffer import Transition
    z = dict(np.load(os.path.join(G, "learner3_batch.npz" if prefix.endswith("3") else "learner_batch.npz")))
    for f in fields:
        z[f] = gold["batch." + f]
    out = {}
    for k in Transition._fields:
        t = th.from_numpy(z[k]).float().to(device)
        out[k] = t.repeat((tile,) + (1,) * (t.dim() - 1)).contiguous()
    return Transition(**out)


def golden_model(cls, args, sd, device="cpu"):
    """``cls`` (or its name in learner.py) with its target, holding the state_dict ``sd`` (or the fixture of that name): the
    reference's keys and shapes, none missing, none extra."""
    import safe_marl_amd.learner as L
    cls = getattr(L, cls) if isinstance(cls, str) else cls
    sd = golden_tensors(sd, device) if isinstance(sd, str) else sd
    model = cls(args, cls(args).to(device)).to(device)
    res = model.load_state_dict(sd, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    return model


def facmaddpg_state_dict(prefix, name="state_dict", device="cpu", target_mixer=False):
    """FACMADDPG's nets and mixer as one state_dict; ``target_mixer``: and the target's mixer, which is the initial one."""
    sd = golden_tensors(f"{prefix}_{name}.npz", device)
    sd.update(golden_tensors(f"{prefix}_{name}_mixer.npz", device))
    if target_mixer:
        sd.update({"target_net." + k: v for k, v in sd.items() if k.startswith("mixer.")})
    return sd


class StubEnv:
    n_envs = 1

    def __init__(self, n=5):
        self.n = n

    def get_num_of_agents(self):
        return self.n


def _np(t):
    return t.detach().float().cpu().numpy()


def _grads(loss, params):
    return [_np(g) for g in th.autograd.grad(loss, list(params))]      # what trainer._sub_update hands the optimiser


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]
