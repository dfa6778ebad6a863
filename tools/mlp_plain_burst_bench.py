"""Rollout step time of MADDPG with agent_type mlp, graph-replayed: the one-launch MLP burst (flexenv_rollout_burst_mlp, the
default) against the RNN agent's plain burst (flexenv_rollout_burst) as the yardstick and the general body this configuration ran
before (FLEX_MLP_BURST=0: Model.policy as a tensor composition, select_action, env.step, flexnet_rollout_pack): us per vector step
of run(m) from device events, all forms in ONE process and alternating, every length warmed, medians of `--reps` samples with
min .. max.  The bar per length: the new form's slowest sample faster than the general body's fastest.  Then the training rate of
examples/train_maddpg.py --agent-type mlp for maddpg (--envs) and safemaddpg (twice --envs) in fresh child processes, alternating
between this tree, this tree with FLEX_MLP_BURST=0 and — with --parent PATH, a checkout of the parent commit built from its own
tree — that tree; and the compiler's resource report of the burst kernels of the build that was timed.
usage: python tools/mlp_plain_burst_bench.py [--envs 4096] [--reps 11] [--runs 5] [--no-train] [--parent PATH]
                                             [--parent-failed ALG] [--rounds 2] [--out profiles/mlp_plain_burst_bench.txt]"""
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
FORMS = ("mlp", "rnn", "general")


def _rollout(form, n_envs):
    import numpy as np
    import torch
    from train_maddpg import DEFAULT_ALG_ARGS
    from safe_marl_amd.flex_env import VecFlexProvisionEnv
    from safe_marl_amd.learner import MADDPG, RolloutGraph
    from safe_marl_amd.network import create_network
    from safe_marl_amd.series import make_synthetic_series
    from safe_marl_amd.trainer import PGTrainer
    from safe_marl_amd.util import convert
    os.environ["FLEX_MLP_BURST"] = "0" if form == "general" else "1"          # (read when the RolloutGraph is built)
    net = create_network({})
    env = VecFlexProvisionEnv({}, n_envs, net=net, series=make_synthetic_series(net, n_days=30), seed=9, warm_start=True)
    alg = dict(DEFAULT_ALG_ARGS)
    alg.update(alg="maddpg", agent_num=env.n_agents, obs_size=env.obs_size, state_size=env.state_size, action_dim=4,
               agent_type="rnn" if form == "rnn" else "mlp")
    torch.manual_seed(3)
    np.random.seed(3)
    tr = PGTrainer(convert(alg), MADDPG, env, None, replay_capacity=n_envs * 96 * 2)
    rg = RolloutGraph(tr.behaviour_net, env, tr.replay_buffer)
    rg.start_episode(env.reset())
    rg.capture(lengths=LENGTHS)
    os.environ.pop("FLEX_MLP_BURST", None)
    return rg, tr


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=11, help="samples per form and length (the median is reported)")
    ap.add_argument("--runs", type=int, default=5, help="run(m) calls per sample")
    ap.add_argument("--no-train", action="store_true", help="skip the training-rate runs")
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit: its examples/train_maddpg.py alternates "
                                                   "with this tree's")
    ap.add_argument("--parent-failed", action="append", default=[], metavar="ALG",
                    help="the parent's run of this --alg ended with an error in an earlier session of this tool: reported as "
                         "failed, not started again")
    ap.add_argument("--rounds", type=int, default=2, help="training-rate runs per side and algorithm")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mlp_plain_burst_bench.txt"))
    a = ap.parse_args()
    if a.reps < 10:
        ap.error("--reps: medians of at least ten samples")

    import torch
    from safe_marl_amd import build
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"# tools/mlp_plain_burst_bench.py --envs {a.envs} --reps {a.reps} --runs {a.runs}; {torch.cuda.get_device_name(0)}; "
        f"library digest {str(build.built_digest())[:16]}")
    forms = {form: _rollout(form, a.envs) for form in FORMS}
    for form, (rg, _) in forms.items():
        say(f"{form}: MADDPG, {a.envs} envs x {rg.model.n_} agents, {type(rg.model.policy_dicts[0]).__name__}, "
            f"mlp_plain_burst={rg.mlp_plain_burst}, fast={rg.fast}, fused_burst={rg.fused_burst}, "
            f"graphs {sorted(k for k, _ in rg.bursts)}")
    assert forms["mlp"][0].mlp_plain_burst and forms["mlp"][0].fused_burst
    assert forms["rnn"][0].fast and forms["rnn"][0].fused_burst and not forms["rnn"][0].mlp_plain_burst
    assert not forms["general"][0].mlp_plain_burst and not forms["general"][0].fused_burst and not forms["general"][0].fast
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
        verdict.append((m, max(per["mlp"]), min(per["general"]), statistics.median(per["mlp"]), statistics.median(per["rnn"])))
    ok = True
    for m, slowest, fastest, med, rnn in verdict:
        ok = ok and slowest < fastest
        say(f"m {m:3d}: the MLP burst's slowest sample {slowest:.2f} {'is below' if slowest < fastest else 'IS NOT BELOW'} the general "
            f"body's fastest, {fastest:.2f}; its median {med:.2f} {'is below' if med < rnn else 'is not below'} the RNN burst's, {rnn:.2f}")
    del forms, rg
    gc.collect()
    torch.cuda.empty_cache()

    if not a.no_train:
        sides = [("tree", ROOT, {}), ("tree FLEX_MLP_BURST=0", ROOT, {"FLEX_MLP_BURST": "0"})]
        if a.parent:
            sides.append(("parent", os.path.abspath(a.parent), {}))
        for alg, envs in (("maddpg", a.envs), ("safemaddpg", 2 * a.envs)):
            rate = {name: [] for name, _, _ in sides}
            for _ in range(a.rounds):
                for name, root, extra in sides:             # alternating, a fresh process each
                    if name == "parent" and (alg in a.parent_failed or None in rate[name]):
                        rate[name].append(None)              # (it ended with an error before: once is the finding)
                        continue
                    cmd = [sys.executable, os.path.join(root, "examples", "train_maddpg.py"), "--alg", alg, "--agent-type", "mlp",
                           "--envs", str(envs), "--episodes", "4"]
                    env = {k: v for k, v in os.environ.items() if k not in ("FLEX_GAUSS_BURST", "FLEX_MLP_BURST", "PYTHONPATH")}
                    env.update(extra)
                    out = subprocess.run(cmd, env=env, cwd=root, capture_output=True, text=True, timeout=900)
                    if out.returncode != 0:
                        tail = (out.stderr.strip().splitlines() or [""])[-1]
                        say(f"train {alg} --agent-type mlp ({name}): exit {out.returncode}: {tail[:60]} ... {tail[-40:]}")
                        if name != "parent":
                            raise SystemExit(1)
                        rate[name].append(None)              # (the parent's own failure is a result: reported, not timed)
                        continue
                    res = next(json.loads(ln) for ln in reversed(out.stdout.splitlines()) if ln.startswith("{"))
                    rate[name].append(res["value"])
                    if name == "tree" and res.get("rollout") != "flexenv_rollout_burst_mlp":
                        say(f"train {alg} --agent-type mlp ({name}): rollout {res.get('rollout')}")
                        ok = False
                    if res.get("fallbacks"):
                        say(f"train {alg} --agent-type mlp ({name}): fallbacks {res['fallbacks']}")
            say(f"train {alg} --agent-type mlp --envs {envs} --episodes 4, env-steps/s: " +
                "  |  ".join(f"{name} " + " ".join("failed" if v is None else f"{v:.0f}" for v in vs) for name, vs in rate.items()))
            if a.parent and None in rate["parent"]:
                faster = all(t > p for t, p in zip(rate["tree"], rate["tree FLEX_MLP_BURST=0"]))
                ok = ok and faster
                say(f"train {alg}: the parent's tree does not finish this run; against FLEX_MLP_BURST=0 this tree "
                    f"{'is' if faster else 'IS NOT'} faster in every round")
            elif a.parent:
                faster = all(t > p for t, p in zip(rate["tree"], rate["parent"]))
                ok = ok and faster
                say(f"train {alg}: this tree {'is' if faster else 'IS NOT'} faster than the parent in every round")

    say("# compiler resource report of this build (build.kernel_resources)")
    for prefix in ("plain_mlp::flex_rollout_burst", "summed_mlp::flex_rollout_burst", "flex_rollout_burst"):
        for v in sorted(build.kernel_resources(prefix).values(), key=lambda v: v["name"]):
            say(f"{v['name']}: {v['vgprs']} VGPRs + {v['agprs']} AGPRs, {v['sgprs']} SGPRs, spills {v.get('sgpr_spills', 0)} s / "
                f"{v.get('vgpr_spills', 0)} v, scratch {v['scratch_bytes_per_lane']} B/lane, LDS {v['lds_bytes_per_block']} B, "
                f"{v['waves_per_simd']} waves/SIMD")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    if not ok:
        raise SystemExit("the speed bars were not all met (see above)")


if __name__ == "__main__":
    main()
