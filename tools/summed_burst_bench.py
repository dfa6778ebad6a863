"""Rollout step time of an agent-summed algorithm (MATD3), graph-replayed, with and without the one-launch burst
(flexenv_rollout_burst_summed; FLEX_SUMMED_BURST=1 / 0): us per vector step of run(m) from device events, both forms in ONE
process and alternating, every length warmed, medians of `--reps` samples with min .. max; then the training rate of
examples/train_maddpg.py for matd3 / iddpg / ippo under both settings (fresh child processes), and the compiler's resource
report of the burst kernels of the build that was timed.
usage: python tools/summed_burst_bench.py [--envs 4096] [--reps 11] [--runs 5] [--no-train] [--out profiles/summed_burst_bench.txt]"""
import argparse
import gc
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "examples"))
LENGTHS = (60, 36, 16, 96)


def _rollout(flag, n_envs):
    import numpy as np
    import torch
    from train_maddpg import DEFAULT_ALG_ARGS
    from safe_marl_amd.flex_env import VecFlexProvisionEnv
    from safe_marl_amd.learner import MATD3, RolloutGraph
    from safe_marl_amd.network import create_network
    from safe_marl_amd.series import make_synthetic_series
    from safe_marl_amd.trainer import PGTrainer
    from safe_marl_amd.util import convert
    os.environ["FLEX_SUMMED_BURST"] = flag                  # (read when the RolloutGraph is built)
    net = create_network({})
    env = VecFlexProvisionEnv({}, n_envs, net=net, series=make_synthetic_series(net, n_days=30), seed=9, warm_start=True)
    alg = dict(DEFAULT_ALG_ARGS)
    alg.update(alg="matd3", agent_num=env.n_agents, obs_size=env.obs_size, state_size=env.state_size, action_dim=4)
    torch.manual_seed(3)
    np.random.seed(3)
    tr = PGTrainer(convert(alg), MATD3, env, None, replay_capacity=n_envs * 96 * 2)
    rg = RolloutGraph(tr.behaviour_net, env, tr.replay_buffer)
    rg.start_episode(env.reset())
    rg.capture(lengths=LENGTHS)
    return rg, tr


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=11, help="samples per form and length (the median is reported)")
    ap.add_argument("--runs", type=int, default=5, help="run(m) calls per sample")
    ap.add_argument("--no-train", action="store_true", help="skip the training-rate runs")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "summed_burst_bench.txt"))
    a = ap.parse_args()
    if a.reps < 10:
        ap.error("--reps: medians of at least ten samples")

    import torch
    from safe_marl_amd import build
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"# tools/summed_burst_bench.py --envs {a.envs} --reps {a.reps} --runs {a.runs}; {torch.cuda.get_device_name(0)}; "
        f"library digest {str(build.built_digest())[:16]}")
    forms = {flag: _rollout(flag, a.envs) for flag in ("0", "1")}
    for flag, (rg, _) in forms.items():
        say(f"FLEX_SUMMED_BURST={flag}: MATD3, {a.envs} envs x {rg.model.n_} agents, summed_sink={rg.summed_sink}, "
            f"fused_burst={rg.fused_burst}, graphs {sorted(k for k, _ in rg.bursts)}")
    assert forms["1"][0].fused_burst and not forms["0"][0].fused_burst
    for m in LENGTHS:
        for rg, _ in forms.values():                        # every length warmed, both forms
            rg.run(m)
            rg.run(m)
        torch.cuda.synchronize()
        per = {"0": [], "1": []}
        for _ in range(a.reps):
            for flag in ("0", "1"):                         # alternating: both forms see the same neighbours
                rg = forms[flag][0]
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.runs):
                    rg.run(m)
                e1.record()
                torch.cuda.synchronize()
                per[flag].append(e0.elapsed_time(e1) * 1e3 / (a.runs * m))
        med = {f: statistics.median(v) for f, v in per.items()}
        say(f"m {m:3d}: three launches per step {med['0']:.2f} us per vector step [{min(per['0']):.2f} .. {max(per['0']):.2f}]  |  "
            f"one-launch burst {med['1']:.2f} us per vector step [{min(per['1']):.2f} .. {max(per['1']):.2f}]  "
            f"(medians of {a.reps}, device events, {a.runs} x run({m}) per sample)")
    del forms, rg
    gc.collect()
    torch.cuda.empty_cache()

    if not a.no_train:
        for alg in ("matd3", "iddpg", "ippo"):
            rate = {}
            for flag in ("0", "1"):
                env = dict(os.environ, FLEX_SUMMED_BURST=flag)
                out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "train_maddpg.py"), "--alg", alg, "--envs",
                                      str(a.envs), "--episodes", "4"], env=env, capture_output=True, text=True, timeout=900)
                if out.returncode != 0:
                    say(f"train {alg} FLEX_SUMMED_BURST={flag}: exit {out.returncode}\n{out.stderr[-2000:]}")
                    raise SystemExit(1)
                res = next(json.loads(ln) for ln in reversed(out.stdout.splitlines()) if ln.startswith("{"))
                rate[flag] = res["value"]
            say(f"train {alg} --envs {a.envs} --episodes 4: {rate['0']:.0f} env-steps/s (FLEX_SUMMED_BURST=0)  |  "
                f"{rate['1']:.0f} env-steps/s (FLEX_SUMMED_BURST=1)")

    say("# compiler resource report of this build (build.kernel_resources)")
    for prefix in ("flex_rollout_burst", "summed::flex_rollout_burst", "flex_test_episodes", "agent_sum_explore"):
        for v in sorted(build.kernel_resources(prefix).values(), key=lambda v: v["name"]):
            say(f"{v['name']}: {v['vgprs']} VGPRs + {v['agprs']} AGPRs, {v['sgprs']} SGPRs, spills {v.get('sgpr_spills', 0)} s / "
                f"{v.get('vgpr_spills', 0)} v, scratch {v['scratch_bytes_per_lane']} B/lane, LDS {v['lds_bytes_per_block']} B, "
                f"{v['waves_per_simd']} waves/SIMD")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
