#!/usr/bin/env python3
"""Test a policy over every start time of a range of days — the vectorised test_agent.py.

The reference's test_agent.py:60-96 loads a checkpoint and runs ONE test-mode episode from a (day, hour, quarter) the user
names.  Here one environment per (day, hour, interval) start of ``--days A:B`` is evaluated in a single call of
``Model.test_episodes`` — one launch where the model is eligible (a shared RNN actor; ``safe_marl_amd.learner.
one_launch_declines``), the stepping loop otherwise — and the answer is per episode: the return and the number of steps with a
voltage violation of every start time, not only their means.

    python examples/test_policy.py --alg maddpg --days 0:30
    python examples/test_policy.py --alg matd3 --load model.pt --days 100:107 --trace-out traces/

Prints one JSON line: the reference's ``mean_test_*`` keys (model.py:285-306), the 5 / 50 / 95 % quantiles of the per-episode
return and of the per-episode violation-step count, the launch form used, and ``fallbacks``.  Every number is on the stand-in
IEEE-33 feeder and the synthetic series unless the caller's checkpoint says otherwise."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

ALGS = ("maddpg", "safemaddpg", "matd3", "iddpg", "facmaddpg", "sqddpg", "ippo", "mappo", "coma")


def alg_args(alg, env, **over):
    """default.yaml merged with the algorithm's own file, as examples/train_maddpg.py builds them."""
    import train_maddpg as t
    from safe_marl_amd.util import convert
    d = dict(t.DEFAULT_ALG_ARGS)
    d.update({"facmaddpg": t.FACMADDPG_ALG_ARGS, "sqddpg": t.SQDDPG_ALG_ARGS, "ippo": t.PPO_ALG_ARGS, "mappo": t.PPO_ALG_ARGS,
              "coma": t.COMA_ALG_ARGS}.get(alg, {}))
    d.update(alg=alg, agent_num=env.n_agents, obs_size=env.obs_size, state_size=env.state_size, action_dim=4, v_min=0.9, v_max=1.1)
    d.update(over)
    return convert(d)


def build_model(alg, args, env):
    from safe_marl_amd import learner
    cls = {"maddpg": learner.MADDPG, "safemaddpg": learner.SAFEMADDPG, "matd3": learner.MATD3, "iddpg": learner.IDDPG,
           "facmaddpg": learner.FACMADDPG, "sqddpg": learner.SQDDPG, "ippo": learner.IPPO, "mappo": learner.MAPPO,
           "coma": learner.COMA}[alg]
    ctor = (args, env) if alg == "safemaddpg" else (args,)
    if args.target:                                                    # the checkpoint of train_agent.py:144-147 holds target_net.* too
        return cls(*ctor, cls(*ctor)).cuda()
    return cls(*ctor).cuda()


def start_times(days, per_hour=4):
    """One (day, hour, interval) per environment: every start of the days A .. B - 1."""
    import numpy as np
    a, b = days
    day, hour, interval = np.meshgrid(np.arange(a, b), np.arange(24), np.arange(per_hour), indexing="ij")
    return dict(day=day.reshape(-1).astype(np.int32), hour=hour.reshape(-1).astype(np.int32),
                interval=interval.reshape(-1).astype(np.int32))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--alg", choices=ALGS, default="maddpg")
    ap.add_argument("--agents", type=int, default=5, choices=[3, 5])
    ap.add_argument("--load", metavar="PATH", default=None,
                    help='a {"model_state_dict": ...} file as train_agent.py:144-147 writes; default: the seeded initial weights')
    ap.add_argument("--days", default="0:30", metavar="A:B", help="start days A .. B - 1 of the series (96 start times each)")
    ap.add_argument("--trace-out", metavar="DIR", default=None, help="write the per-step trace there, one .npy per array")
    ap.add_argument("--loop", action="store_true", help="the stepping loop even where the launch is eligible")
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    try:
        d0, d1 = (int(x) for x in a.days.split(":"))
    except ValueError:
        ap.error("--days takes A:B")
    if not 0 <= d0 < d1:
        ap.error("--days A:B needs 0 <= A < B")

    import numpy as np
    import torch
    import safe_marl_amd  # noqa: F401
    from safe_marl_amd.flex_env import VecFlexProvisionEnv
    from safe_marl_amd.learner import one_launch_declines
    from safe_marl_amd.network import create_network
    from safe_marl_amd.series import make_synthetic_series
    from safe_marl_amd.util import FALLBACKS

    blds = [5, 10, 15, 20, 25] if a.agents == 5 else [5, 15, 25]
    env_args = {"buildings": blds, "pv_nodes": blds, "ess_nodes": blds}
    if a.alg == "safemaddpg":
        env_args["alg"] = "safemaddpg"
    net = create_network(env_args)
    series = make_synthetic_series(net, n_days=365)
    if d1 > series.n_start_days(96):
        ap.error(f"--days: the series has {series.n_start_days(96)} start days")
    spec = start_times((d0, d1))
    n = len(spec["day"])
    env = VecFlexProvisionEnv(env_args, n, net=net, series=series, seed=1234, warm_start=True)
    torch.manual_seed(a.seed)
    model = build_model(a.alg, alg_args(a.alg, env), env)
    if a.load:
        model.load_state_dict(torch.load(a.load, map_location="cuda")["model_state_dict"])
    why = one_launch_declines(model)
    res = model.test_episodes(env, spec=spec, trace=a.trace_out is not None, one_launch=False if a.loop else None)
    ret, viol = res.sums[:, 7], res.sums[:, 8]
    q = (5, 50, 95)
    out = dict(res.stat())
    out.update(alg=a.alg, n_agents=env.n_agents, episodes=n, days=[d0, d1], checkpoint=a.load,
               launch_form="one launch (flexenv_test_episodes)" if res.launch else "loop",
               loop_reason=None if res.launch else ("--loop" if a.loop and why is None else why),
               episode_length={"min": int(res.length.min()), "max": int(res.length.max())},
               episode_return_quantiles={f"p{p}": float(np.percentile(ret, p)) for p in q},
               episode_violation_steps_quantiles={f"p{p}": float(np.percentile(viol, p)) for p in q},
               fallbacks=dict(FALLBACKS))
    if a.trace_out:
        os.makedirs(a.trace_out, exist_ok=True)
        for k, v in dict(res.trace, sums=res.sums, length=res.length, **spec).items():
            np.save(os.path.join(a.trace_out, k + ".npy"), v)
        out["trace_out"] = a.trace_out
    print(json.dumps(out))


if __name__ == "__main__":
    main()
