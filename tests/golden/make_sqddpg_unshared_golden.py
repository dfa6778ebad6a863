#!/usr/bin/env python3
"""Generates tests/golden/sqddpg_unshared3_*: make_sqddpg_golden.py's run of the reference's SQDDPG with ``shared_params:
False`` (one actor and one critic per agent, madrl/models/sqddpg.py:94-100), three agents and learner3_batch.npz.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_sqddpg_unshared_golden.py --reference <reference checkout>

A state_dict of six networks and their target replicas is larger than the largest fixture in the tree, so the behaviour net's
keys (``<name>.npz``) and the target replica's (``target_net.*``: ``<name>_target.npz``) are written as separate files.  The
fixtures are data (inputs + expected outputs); no reference source travels.
"""
import os
import sys

import numpy as np

sys.argv += ["--agents", "3"]
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_sqddpg_golden as base  # noqa: E402  (names the reference, chdirs into it and records the coalition draws)

base.PREFIX = "sqddpg_unshared3"
_shared_args = base.load_args


def load_args():
    d = _shared_args()
    d["shared_params"] = False
    return d


def save_sd(name, sd):
    sd = {k: v.detach().cpu().numpy().copy() for k, v in sd.items()}
    own = {k: v for k, v in sd.items() if not k.startswith("target_net.")}
    tgt = {k: v for k, v in sd.items() if k.startswith("target_net.")}
    np.savez_compressed(os.path.join(base.OUT_DIR, f"{base.PREFIX}_{name}.npz"), **own)
    if tgt:
        np.savez_compressed(os.path.join(base.OUT_DIR, f"{base.PREFIX}_{name}_target.npz"), **tgt)


base.load_args, base.save_sd = load_args, save_sd

if __name__ == "__main__":
    base.main()
