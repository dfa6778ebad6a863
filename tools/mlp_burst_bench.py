"""Rollout step time of IPPO with agent_type mlp, graph-replayed: the one-launch MLP burst (flexenv_rollout_burst_summed_mlp, the
default) against the RNN agent's summed burst (flexenv_rollout_burst_summed) as the yardstick and, opt-in (FLEX_GAUSS_BURST=1), the
Gaussian MLP burst: us per vector step of run(m) from device events, all forms in ONE process and alternating, every length
warmed, medians of `--reps` samples with min .. max.  The bar per length: the MLP burst's median no more than the RNN burst's
median plus that burst's own spread (max - min).  Then the training rate of examples/train_maddpg.py --agent-type mlp for ippo
and matd3 in fresh child processes, alternating between this tree, this tree with FLEX_MLP_BURST=0 (the eager loop behind the
declined capture, as before the burst existed) and — with --parent PATH, a checkout of the parent commit built from its own
tree — that tree; and the compiler's resource report of the burst kernels of the build that was timed.
usage: python tools/mlp_burst_bench.py [--envs 4096] [--reps 11] [--runs 5] [--no-train] [--parent PATH] [--rounds 2]
                                       [--out profiles/mlp_burst_bench.txt]"""
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
LENGTHS = (16, 36, 60, 96)
FORMS = ("mlp", "rnn", "mlp-gauss")


def _rollout(form, n_envs):
    import numpy as np
    import torch
    from train_maddpg import DEFAULT_ALG_ARGS, PPO_ALG_ARGS
    from safe_marl_amd.flex_env import VecFlexProvisionEnv
    from safe_marl_amd.learner import IPPO, RolloutGraph
    from safe_marl_amd.network import create_network
    from safe_marl_amd.series import make_synthetic_series
    from safe_marl_amd.trainer import PGTrainer
    from safe_marl_amd.util import convert
    os.environ["FLEX_GAUSS_BURST"] = "1" if form == "mlp-gauss" else "0"      # (read when the RolloutGraph is built)
    os.environ.pop("FLEX_MLP_BURST", None)
    net = create_network({})
    env = VecFlexProvisionEnv({}, n_envs, net=net, series=make_synthetic_series(net, n_days=30), seed=9, warm_start=True)
    alg = dict(DEFAULT_ALG_ARGS)
    alg.update(PPO_ALG_ARGS)
    alg.update(alg="ippo", agent_num=env.n_agents, obs_size=env.obs_size, state_size=env.state_size, action_dim=4,
               agent_type="rnn" if form == "rnn" else "mlp", gaussian_policy=form == "mlp-gauss")
    torch.manual_seed(3)
    np.random.seed(3)
    tr = PGTrainer(convert(alg), IPPO, env, None, replay_capacity=n_envs * 96 * 2)
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
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit: its examples/train_maddpg.py alternates "
                                                   "with this tree's")
    ap.add_argument("--rounds", type=int, default=2, help="training-rate runs per side and algorithm")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mlp_burst_bench.txt"))
    a = ap.parse_args()
    if a.reps < 10:
        ap.error("--reps: medians of at least ten samples")

    import torch
    from safe_marl_amd import build
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"# tools/mlp_burst_bench.py --envs {a.envs} --reps {a.reps} --runs {a.runs}; {torch.cuda.get_device_name(0)}; "
        f"library digest {str(build.built_digest())[:16]}")
    forms = {form: _rollout(form, a.envs) for form in FORMS}
    for form, (rg, _) in forms.items():
        say(f"{form}: IPPO, {a.envs} envs x {rg.model.n_} agents, {type(rg.model.policy_dicts[0]).__name__}, mlp_burst={rg.mlp_burst}, "
            f"summed_burst={rg.summed_burst}, fused_burst={rg.fused_burst}, graphs {sorted(k for k, _ in rg.bursts)}")
    assert forms["mlp"][0].mlp_burst and forms["mlp"][0].fused_burst and not forms["mlp"][0].gaussian
    assert forms["mlp-gauss"][0].mlp_burst and forms["mlp-gauss"][0].gaussian
    assert forms["rnn"][0].summed_burst and not forms["rnn"][0].mlp_burst
    verdict = []
    for m in LENGTHS:
        for rg, _ in forms.values():                        # every length warmed, every form
            rg.run(m)
            rg.run(m)
        torch.cuda.synchronize()
        per = {form: [] for form in FORMS}
        for _ in range(a.reps):
            for form in FORMS:                              # alternating: every form sees the same neighbours
                rg = forms[form][0]
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.runs):
                    rg.run(m)
                e1.record()
                torch.cuda.synchronize()
                per[form].append(e0.elapsed_time(e1) * 1e3 / (a.runs * m))
        txt = "  |  ".join(f"{form} {statistics.median(per[form]):.2f} [{min(per[form]):.2f} .. {max(per[form]):.2f}]" for form in FORMS)
        say(f"m {m:3d}: us per vector step: {txt}  (medians of {a.reps}, device events, {a.runs} x run({m}) per sample)")
        bar = statistics.median(per["rnn"]) + (max(per["rnn"]) - min(per["rnn"]))
        verdict.append((m, statistics.median(per["mlp"]), bar))
    for m, med, bar in verdict:
        say(f"m {m:3d}: the MLP burst's median {med:.2f} {'is within' if med <= bar else 'EXCEEDS'} the RNN burst's median plus its "
            f"spread, {bar:.2f}")
    del forms, rg
    gc.collect()
    torch.cuda.empty_cache()

    if not a.no_train:
        sides = [("tree", ROOT, {}), ("tree FLEX_MLP_BURST=0", ROOT, {"FLEX_MLP_BURST": "0"})]
        if a.parent:
            sides.append(("parent", os.path.abspath(a.parent), {}))
        for alg in ("ippo", "matd3"):
            rate = {name: [] for name, _, _ in sides}
            for _ in range(a.rounds):
                for name, root, extra in sides:             # alternating, a fresh process each
                    cmd = [sys.executable, os.path.join(root, "examples", "train_maddpg.py"), "--alg", alg, "--agent-type", "mlp",
                           "--envs", str(a.envs), "--episodes", "4"]
                    env = {k: v for k, v in os.environ.items() if k not in ("FLEX_GAUSS_BURST", "FLEX_MLP_BURST", "PYTHONPATH")}
                    env.update(extra)
                    out = subprocess.run(cmd, env=env, cwd=root, capture_output=True, text=True, timeout=900)
                    if out.returncode != 0:
                        say(f"train {alg} --agent-type mlp ({name}): exit {out.returncode}\n{out.stderr[-2000:]}")
                        raise SystemExit(1)
                    res = next(json.loads(ln) for ln in reversed(out.stdout.splitlines()) if ln.startswith("{"))
                    rate[name].append(res["value"])
                    if res.get("fallbacks"):
                        say(f"train {alg} --agent-type mlp ({name}): fallbacks {res['fallbacks']}")
            say(f"train {alg} --agent-type mlp --envs {a.envs} --episodes 4, env-steps/s: " +
                "  |  ".join(f"{name} " + " ".join(f"{v:.0f}" for v in vs) for name, vs in rate.items()))

    say("# compiler resource report of this build (build.kernel_resources)")
    for prefix in ("summed_mlp::flex_rollout_burst", "summed_gauss_mlp::flex_rollout_burst", "summed::flex_rollout_burst",
                   "summed_gauss::flex_rollout_burst", "flex_rollout_burst"):
        for v in sorted(build.kernel_resources(prefix).values(), key=lambda v: v["name"]):
            say(f"{v['name']}: {v['vgprs']} VGPRs + {v['agprs']} AGPRs, {v['sgprs']} SGPRs, spills {v.get('sgpr_spills', 0)} s / "
                f"{v.get('vgpr_spills', 0)} v, scratch {v['scratch_bytes_per_lane']} B/lane, LDS {v['lds_bytes_per_block']} B, "
                f"{v['waves_per_simd']} waves/SIMD")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
