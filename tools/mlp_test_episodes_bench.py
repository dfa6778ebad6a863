#!/usr/bin/env python3
"""Test-mode episodes of a shared MLP agent, loop against launch: tools/test_episodes_bench.py for ``agent_type: mlp``, with
FLEX_MLP_TEST_LAUNCH=1 set for the process.  One process, every form alternating within a round so that each sees the same
neighbours, two warm-up rounds, then the median [min .. max] of ``--runs`` (>= 10) rounds.

    python tools/mlp_test_episodes_bench.py [--envs 4096] [--runs 10] [--out profiles/mlp_test_episodes_bench.txt]

At ``--envs`` environments x 5 agents for 95 steps:
  device events per vector step (the launch alone: reset and copies outside the events; the burst graph-replayed)
    flexenv_test_episodes_mlp without and with the per-step trace, the RNN agent's flexenv_test_episodes, and the MLP agent's
    training burst (flexenv_rollout_burst_mlp: noise and replay on top of the same policy and step)
  wall time per call that ends with its results on the host
    evaluate_on, Model.test_episodes in its loop form, its launch form, and the launch with the trace
The bar: the launch's slowest call beats the loop's fastest (exit status 1 otherwise).  The compiler's resource report of the
six test kernels closes the output."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "examples"))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def run(a):
    os.environ["FLEX_MLP_TEST_LAUNCH"] = "1"                             # (read at call time by one_launch_declines)
    import numpy as np
    import torch
    import safe_marl_amd  # noqa: F401
    from learning_curve import eval_spec
    from test_policy import alg_args
    from safe_marl_amd import build
    from safe_marl_amd.flex_env import VecFlexProvisionEnv
    from safe_marl_amd.learner import MADDPG, RolloutGraph
    from safe_marl_amd.nets import fused_actor_forward, mlp_test_actor_args
    from safe_marl_amd.network import create_network
    from safe_marl_amd.series import make_synthetic_series
    from safe_marl_amd.trainer import PGTrainer

    lines = []

    def say(line):
        print(line, flush=True)
        lines.append(line)

    def fmt(ts):
        return f"{statistics.median(ts):.2f} [{min(ts):.2f} .. {max(ts):.2f}]"

    net = create_network({})
    series = make_synthetic_series(net, n_days=365)
    N, steps = a.envs, 95
    env = VecFlexProvisionEnv({}, N, net=net, series=series, seed=9, warm_start=True)
    torch.manual_seed(3)
    np.random.seed(3)
    tr = PGTrainer(alg_args("maddpg", env, behaviour_update_freq=30, batch_size=4, agent_type="mlp"), MADDPG, env, None,
                   replay_capacity=N * 96 * 2)
    model = tr.behaviour_net
    rnn = MADDPG(alg_args("maddpg", env)).cuda()
    ev = VecFlexProvisionEnv({}, N, net=net, series=series, seed=77, warm_start=True)
    n = ev.n_agents
    spec = eval_spec(series, N, n)
    say(f"# mlp_test_episodes_bench: {N} envs x {n} agents x {steps} steps, median [min .. max] of {a.runs} runs, "
        f"forms alternating in one process; {torch.cuda.get_device_name(0)}; library digest {str(build.built_digest())[:16]}")
    rg = RolloutGraph(model, env, tr.replay_buffer)
    rg.start_episode(env.reset())
    rg.capture()
    say(f"training burst: {type(model.policy_dicts[0]).__name__}, mlp_plain_burst={rg.mlp_plain_burst}, fused_burst={rg.fused_burst}")

    hid, hid2 = (torch.zeros(N * n, 64, device="cuda") for _ in range(2))
    means, action, env_action = (torch.zeros(N * n, 4, device="cuda") for _ in range(3))
    margs, mlp = mlp_test_actor_args(model.policy_dicts[0], N, n, model.obs_dim, model.args.agent_id, hid, means, action, env_action,
                                     model.args.action_low, model.args.action_high)
    outs = {trace: ev.test_out(steps, trace) for trace in (False, True)}

    def mlp_launch(trace):
        assert ev.test_episodes(margs, steps, out=outs[trace], mlp=mlp) is not None

    def rnn_launch():
        fused_actor_forward(rnn.policy_dicts[0], ev.obs.view(N, n, -1), hid2, n, rnn.args.agent_id,
                            noise=torch.zeros(N, n, 4, device="cuda"), std=0.0, low=rnn.args.action_low, high=rnn.args.action_high,
                            launch=lambda args: ev.test_episodes(args, steps, out=outs[False]))

    # device events per vector step: the launch alone (reset and copies outside the events), the burst graph-replayed
    forms = (("MLP test launch (flexenv_test_episodes_mlp, no trace)", lambda: mlp_launch(False), True),
             ("MLP test launch (flexenv_test_episodes_mlp, with trace)", lambda: mlp_launch(True), True),
             ("RNN test launch (flexenv_test_episodes, no trace)", rnn_launch, True),
             ("MLP training burst (flexenv_rollout_burst_mlp)", lambda: rg.run(steps), False))
    per = {name: [] for name, _, _ in forms}
    for i in range(a.runs + 2):                                         # (two warm-up rounds)
        for name, fn, reset in forms:
            if reset:
                ev.reset(spec=spec)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            if i >= 2:
                per[name].append(e0.elapsed_time(e1) * 1e3 / steps)
    for name, _, _ in forms:
        say(f"{name}: {fmt(per[name])} us per vector step (device events)")
    m0, m1, r0, b0 = (statistics.median(per[name]) for name, _, _ in forms)
    say(f"the MLP test launch runs at {m0 / b0:.3f} x the MLP training burst and {m0 / r0:.3f} x the RNN test launch; "
        f"trace stores: {m1 - m0:+.2f} us per vector step")
    rg.release()

    # wall time per call, results on the host
    calls = (("evaluate_on", lambda: model.evaluate_on(ev, spec)),
             ("test_episodes loop", lambda: model.test_episodes(ev, spec, one_launch=False)),
             ("test_episodes launch", lambda: model.test_episodes(ev, spec, one_launch=True)),
             ("test_episodes launch + trace", lambda: model.test_episodes(ev, spec, trace=True, one_launch=True)))
    wall = {name: [] for name, _ in calls}
    for i in range(a.runs + 2):
        for name, fn in calls:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = fn()
            torch.cuda.synchronize()
            if i >= 2:
                wall[name].append((time.perf_counter() - t0) * 1e3)
            if name.startswith("test_episodes"):
                assert res.launch == ("launch" in name), name
    for name, _ in calls:
        med = statistics.median(wall[name])
        say(f"{name}: {fmt(wall[name])} ms per call = {med * 1e3 / steps:.1f} us per vector step (wall, results on the host)")
    slowest, fastest = max(wall["test_episodes launch"]), min(wall["test_episodes loop"])
    ok = slowest < fastest
    say(f"the launch's slowest run {slowest:.2f} ms {'is below' if ok else 'IS NOT BELOW'} the loop's fastest, {fastest:.2f} ms "
        f"({statistics.median(wall['test_episodes loop']) / statistics.median(wall['test_episodes launch']):.1f} x between the medians)")
    say("# compiler resource report of this build (build.kernel_resources)")
    for prefix in ("test_mlp::flex_test_episodes_kernel<", "flex_test_episodes_kernel"):
        for v in sorted(build.kernel_resources(prefix).values(), key=lambda v: v["name"]):
            say(f"{v['name']}: {v['vgprs']} VGPRs + {v['agprs']} AGPRs, {v['sgprs']} SGPRs, scratch {v['scratch_bytes_per_lane']} B/lane, "
                f"LDS {v['lds_bytes_per_block']} B, {v['waves_per_simd']} waves/SIMD")
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    if not ok:
        raise SystemExit("the speed bar was not met (see above)")


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.runs < 10:
        ap.error("--runs: at least ten")
    run(a)


if __name__ == "__main__":
    main()
