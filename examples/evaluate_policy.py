#!/usr/bin/env python3
"""Test a policy of either agent type over every start time of a range of days — examples/test_policy.py with the choice of the
policy network.

test_policy.py evaluates the recurrent agent of default.yaml.  This script takes ``--agent-type {rnn,mlp}`` and, for the MLP
agent, ``--mlp-launch``: it sets FLEX_MLP_TEST_LAUNCH=1 for the process before the model is built, which admits a shared MLP
actor to the one launch (``safe_marl_amd.learner.one_launch_declines`` reads the switch at every call; include/flexenv.h:
flexenv_test_episodes_mlp).  Without it an MLP model takes the stepping loop, and the output names the reason.

    python examples/evaluate_policy.py --alg maddpg --agent-type mlp --mlp-launch --days 0:30
    python examples/evaluate_policy.py --alg matd3 --agent-type mlp --load model.pt --days 100:107 --trace-out traces/

``--intended-actions`` (with ``--alg safemaddpg``) evaluates SAFEMADDPG.intended_actions, and ``--intended-launch`` sets
FLEX_INTENDED_LAUNCH=1 the same way, which admits that routing to the one launch (flexenv_test_episodes_routed).

Prints one JSON line: test_policy.py's keys, ``agent_type``, and in ``launch_form`` the entry point that was used."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def main():
    from test_policy import ALGS, alg_args, build_model, start_times
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--alg", choices=ALGS, default="maddpg")
    ap.add_argument("--agent-type", choices=["rnn", "mlp"], default="rnn", help="the policy network (default.yaml: rnn)")
    ap.add_argument("--mlp-launch", action="store_true",
                    help="admit a shared MLP agent to the one launch (sets FLEX_MLP_TEST_LAUNCH=1 for this process)")
    ap.add_argument("--intended-actions", action="store_true",
                    help="with --alg safemaddpg: SAFEMADDPG.intended_actions (not the reference's routing; the form that learns)")
    ap.add_argument("--intended-launch", action="store_true",
                    help="with --intended-actions: admit that routing to the one launch (sets FLEX_INTENDED_LAUNCH=1 for this "
                         "process; flexenv_test_episodes_routed)")
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
    if a.intended_actions and a.alg != "safemaddpg":
        ap.error("--intended-actions: needs --alg safemaddpg")
    if a.intended_launch:
        if not a.intended_actions:
            ap.error("--intended-launch: needs --intended-actions")
        os.environ["FLEX_INTENDED_LAUNCH"] = "1"                        # (read at call time by one_launch_declines)
    if a.mlp_launch:                                                    # (before the model is built; read at call time)
        os.environ["FLEX_MLP_TEST_LAUNCH"] = "1"

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
    model = build_model(a.alg, alg_args(a.alg, env, agent_type=a.agent_type), env)
    if a.load:
        model.load_state_dict(torch.load(a.load, map_location="cuda")["model_state_dict"])
    if a.intended_actions:
        model.intended_actions = True
    why = one_launch_declines(model)
    res = model.test_episodes(env, spec=spec, trace=a.trace_out is not None, one_launch=False if a.loop else None)
    ret, viol = res.sums[:, 7], res.sums[:, 8]
    q = (5, 50, 95)
    entry = "flexenv_test_episodes_mlp" if a.agent_type == "mlp" else "flexenv_test_episodes"
    if a.intended_actions:
        entry = "flexenv_test_episodes_routed"
    out = dict(res.stat())
    if a.intended_actions:
        out["intended_actions"] = True
    out.update(alg=a.alg, agent_type=a.agent_type, n_agents=env.n_agents, episodes=n, days=[d0, d1], checkpoint=a.load,
               launch_form=f"one launch ({entry})" if res.launch else "loop",
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
