#!/usr/bin/env python3
"""Generates tests/golden/facmaddpg_unshared3_*: make_facmaddpg_golden.py's run of the reference's FACMADDPG with
``shared_params: False`` (one actor and one critic per agent), three agents and learner3_batch.npz.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_facmaddpg_unshared_golden.py --reference <reference checkout>

Every state_dict is split three ways, so that no fixture exceeds the largest one in the tree: the behaviour net without its
mixer (``<name>.npz``), its mixer (``<name>_mixer.npz``) and the target replica without its mixer (``target_net.*``:
``<name>_target.npz``; the replica's mixer is the initial mixer, as in make_facmaddpg_golden.py).  The fixtures are data
(inputs + expected outputs); no reference source travels.
"""
import os
import sys

import numpy as np

sys.argv += ["--agents", "3"]
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_facmaddpg_golden as base  # noqa: E402  (names the reference and chdirs into it)

base.PREFIX = "facmaddpg_unshared3"
_shared_args = base.load_args


def load_args():
    d = _shared_args()
    d["shared_params"] = False
    return d


def save_sd(name, sd):
    sd = {k: v.detach().cpu().numpy().copy() for k, v in sd.items()}
    parts = {"": {k: v for k, v in sd.items() if "mixer." not in k and not k.startswith("target_net.")},
             "_mixer": {k: v for k, v in sd.items() if k.startswith("mixer.")},
             "_target": {k: v for k, v in sd.items() if "mixer." not in k and k.startswith("target_net.")}}
    for suffix, part in parts.items():
        if part:
            np.savez_compressed(os.path.join(base.OUT_DIR, f"{base.PREFIX}_{name}{suffix}.npz"), **part)


base.load_args, base.save_sd = load_args, save_sd

if __name__ == "__main__":
    base.main()
