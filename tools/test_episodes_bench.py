#!/usr/bin/env python3
"""Test-mode episodes, loop against launch: one process, after warm-up, the median of ``--runs`` (>= 10) runs each.

    python tools/test_episodes_bench.py [--envs 4096] [--tester-envs 512] [--runs 10] [--out profiles/test_episodes_bench.txt]

Timed at ``--envs`` environments x 5 agents for 95 steps, host wall clock around a call that ends with its results on the host
(so a run holds the reset, the launches, the device-to-host copies of the record and, for the loop forms, the host's own time):
  evaluate_on                       today's evaluation: means over env-steps, a Python loop
  test_episodes loop                the loop form of Model.test_episodes (per-episode record)
  test_episodes launch              flexenv_test_episodes, no trace
  test_episodes launch + trace      the same with the per-step trace (about 620 B per env-step of stores, and their copy out)
  PGTester.run loop / one_launch    the tester's record at ``--tester-envs`` environments
and, as the yardstick of the launch without trace, the training burst (flexenv_rollout_burst: noise and replay on top of the
same policy and step) per vector step, device events around graph-replayed runs of 95 steps in the same session.  The launch's
own device time per vector step (events around the launch alone, reset and copies outside) is printed next to it."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "examples"))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--tester-envs", type=int, default=512)
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.runs < 10:
        ap.error("--runs: at least ten")

    import numpy as np
    import torch
    import safe_marl_amd  # noqa: F401
    from learning_curve import eval_spec
    from test_policy import alg_args
    from safe_marl_amd.flex_env import VecFlexProvisionEnv
    from safe_marl_amd.learner import MADDPG, RolloutGraph
    from safe_marl_amd.network import create_network
    from safe_marl_amd.series import make_synthetic_series
    from safe_marl_amd.tester import PGTester
    from safe_marl_amd.trainer import PGTrainer

    lines = []

    def say(line):
        print(line, flush=True)
        lines.append(line)

    def wall(fn):
        fn()
        fn()                                                            # warm-up: allocations, first launches
        torch.cuda.synchronize()
        ts = []
        for _ in range(a.runs):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        return statistics.median(ts), min(ts), max(ts)

    net = create_network({})
    series = make_synthetic_series(net, n_days=365)
    N, steps = a.envs, 95
    env = VecFlexProvisionEnv({}, N, net=net, series=series, seed=9, warm_start=True)
    torch.manual_seed(3)
    np.random.seed(3)
    tr = PGTrainer(alg_args("maddpg", env, behaviour_update_freq=30, batch_size=4), MADDPG, env, None, replay_capacity=N * 96 * 2)
    model = tr.behaviour_net
    ev = VecFlexProvisionEnv({}, N, net=net, series=series, seed=77, warm_start=True)
    spec = eval_spec(series, N, ev.n_agents)
    say(f"# test_episodes_bench: {N} envs x {ev.n_agents} agents x {steps} steps, median [min .. max] of {a.runs} runs, same process")

    # the yardstick: the training burst per vector step
    rg = RolloutGraph(model, env, tr.replay_buffer)
    rg.start_episode(env.reset())
    rg.capture()
    rg.run(steps)
    torch.cuda.synchronize()
    per = []
    for _ in range(a.runs):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        rg.run(steps)
        e1.record()
        torch.cuda.synchronize()
        per.append(e0.elapsed_time(e1) * 1e3 / steps)
    burst = statistics.median(per)
    say(f"training burst (flexenv_rollout_burst, fused={rg.fused_burst}): {burst:.2f} us per vector step [{min(per):.2f} .. {max(per):.2f}] (device events)")
    rg.release()

    # the launch alone, device time: reset and copies outside the events
    from safe_marl_amd.nets import fused_actor_forward
    launch = {}
    for trace in (False, True):
        out = ev.test_out(steps, trace)
        per = []
        for i in range(a.runs + 2):
            ev.reset(spec=spec)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fused_actor_forward(model.policy_dicts[0], ev.obs.view(N, ev.n_agents, -1), torch.zeros(N * ev.n_agents, 64, device="cuda"),
                                ev.n_agents, model.args.agent_id, noise=torch.zeros(N, ev.n_agents, 4, device="cuda"), std=0.0,
                                low=model.args.action_low, high=model.args.action_high,
                                launch=lambda args: ev.test_episodes(args, steps, out=out))
            e1.record()
            torch.cuda.synchronize()
            if i >= 2:
                per.append(e0.elapsed_time(e1) * 1e3 / steps)
        launch[trace] = statistics.median(per)
        say(f"test launch (flexenv_test_episodes, {'with' if trace else 'no'} trace): {launch[trace]:.2f} us per vector step "
            f"[{min(per):.2f} .. {max(per):.2f}] (device events; {launch[trace] / burst:.3f} x the training burst)")
        del out
    row_bytes = 4 * 4 * ev.n_agents + 8 * ev.n_bus + 8 * 5 * ev.n_agents + 4 + 8 + 8 * 7 + 1      # FlexTestOut, one env-step
    say(f"trace stores: {launch[True] - launch[False]:+.2f} us per vector step on the device ({row_bytes} B per env-step)")

    for name, fn in (("evaluate_on", lambda: model.evaluate_on(ev, spec)),
                     ("test_episodes loop", lambda: model.test_episodes(ev, spec, one_launch=False)),
                     ("test_episodes launch", lambda: model.test_episodes(ev, spec, one_launch=True)),
                     ("test_episodes launch + trace", lambda: model.test_episodes(ev, spec, trace=True, one_launch=True))):
        med, lo, hi = wall(fn)
        say(f"{name}: {med:.2f} ms per call [{lo:.2f} .. {hi:.2f}] = {med * 1e3 / steps:.1f} us per vector step (wall, results on the host)")

    n = a.tester_envs
    tv = VecFlexProvisionEnv({}, n, net=net, series=series, seed=5, warm_start=True)
    sp = eval_spec(series, n, tv.n_agents, seed=7)
    tester = PGTester(model.args, model, tv)
    for name, one in (("PGTester.run loop", False), ("PGTester.run one_launch", True)):
        med, lo, hi = wall(lambda: tester.run(sp["day"], sp["hour"], sp["interval"], one_launch=one, e0=sp["e0"], a0=sp["a0"]))
        say(f"{name} ({n} envs): {med:.2f} ms per call [{lo:.2f} .. {hi:.2f}] (wall)")
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
