"""SAFEMADDPG.intended_actions inside the one-launch paths (FLEX_INTENDED_LAUNCH=1: flexenv_rollout_burst_routed,
flexenv_test_episodes_routed) against forms that exist without the switch, for the RNN and the MLP agent, all forms in ONE process
and alternating, medians of `--reps` samples with min .. max, device events.
Rollout, us per vector step of graph-replayed run(m), m in 16 / 36 / 60 / 96: the routed burst (routing 1), the reference-routing
burst (intended_actions off: flexenv_rollout_burst / flexenv_rollout_burst_mlp) and today's intended body (the switch unset: policy
launch, flexenv_safety_project, the transpose in torch and the env launch per step for the RNN agent, the general Model.policy body
for the MLP agent).  Bars: (1) at every m and for both agents the routed burst's slowest sample is below today's body's fastest;
(2) at m = 96 the routed burst's median lies within the reference-routing burst's [min .. max] widened by 3 %.
Test mode, us per vector step of Model.test_episodes as a call (95 steps): the launch with routing 1, the launch with the reference
routing, the loop with intended_actions.
Then examples/train_maddpg.py --alg safemaddpg --intended-actions with and without --intended-launch in fresh child processes,
alternating (context, not a bar), and the compiler's resource report of the kernels that were timed.
usage: python tools/intended_launch_bench.py [--envs 4096] [--reps 11] [--runs 5] [--no-train] [--train-envs 8192] [--rounds 2]
                                             [--out profiles/intended_launch_bench.txt]"""
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
FORMS = ("routed", "reference", "body")
AGENTS = ("rnn", "mlp")
SWITCH = "FLEX_INTENDED_LAUNCH"


def _world():
    from safe_marl_amd.network import create_network
    from safe_marl_amd.series import make_synthetic_series
    env_args = {"alg": "safemaddpg"}
    net = create_network(env_args)
    return env_args, net, make_synthetic_series(net, n_days=30)


def _model(agent_type, env, form):
    import numpy as np
    import torch
    from train_maddpg import DEFAULT_ALG_ARGS
    from safe_marl_amd.learner import SAFEMADDPG
    from safe_marl_amd.util import convert
    alg = dict(DEFAULT_ALG_ARGS)
    alg.update(alg="safemaddpg", agent_num=env.n_agents, obs_size=env.obs_size, state_size=env.state_size, action_dim=4,
               v_min=0.9, v_max=1.1, agent_type=agent_type)
    torch.manual_seed(3)
    np.random.seed(3)
    m = SAFEMADDPG(convert(alg), env).cuda()
    m.intended_actions = form != "reference"
    return m


def _rollout(agent_type, form, n_envs, world):
    from safe_marl_amd.flex_env import VecFlexProvisionEnv
    from safe_marl_amd.learner import RolloutGraph
    from safe_marl_amd.replay_buffer import TransReplayBuffer
    env_args, net, series = world
    os.environ[SWITCH] = "1" if form == "routed" else "0"                # (read when the RolloutGraph is built)
    env = VecFlexProvisionEnv(env_args, n_envs, net=net, series=series, seed=9, warm_start=True)
    m = _model(agent_type, env, form)
    rg = RolloutGraph(m, env, TransReplayBuffer(n_envs * 96 * 2, device="cuda"))
    rg.start_episode(env.reset())
    try:
        rg.capture(lengths=LENGTHS)
    except Exception as exc:                  # (a body the graph cannot hold is timed as eager steps, and the output says so)
        if form != "body":
            raise
        rg.bench_note = f"capture failed ({type(exc).__name__}: {str(exc).splitlines()[0][:100]}): timed as eager steps"
        rg.graph, rg.bursts = None, {}
    os.environ.pop(SWITCH, None)
    return rg


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=11, help="samples per form and length (the median is reported)")
    ap.add_argument("--runs", type=int, default=5, help="run(m) calls per sample")
    ap.add_argument("--no-train", action="store_true", help="skip the training-rate runs")
    ap.add_argument("--train-envs", type=int, default=8192)
    ap.add_argument("--rounds", type=int, default=2, help="training-rate runs per side")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "intended_launch_bench.txt"))
    a = ap.parse_args()
    if a.reps < 10:
        ap.error("--reps: medians of at least ten samples")

    import numpy as np
    import torch
    from safe_marl_amd import build
    from safe_marl_amd.flex_env import VecFlexProvisionEnv
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"# tools/intended_launch_bench.py --envs {a.envs} --reps {a.reps} --runs {a.runs}; {torch.cuda.get_device_name(0)}; "
        f"library digest {str(build.built_digest())[:16]}")
    world = _world()
    ok = True
    for agent in AGENTS:
        forms = {form: _rollout(agent, form, a.envs, world) for form in FORMS}
        for form, rg in forms.items():
            say(f"{agent} {form}: SAFEMADDPG, {a.envs} envs x {rg.model.n_} agents, {type(rg.model.policy_dicts[0]).__name__}, "
                f"intended_actions={rg.model.intended_actions}, intended_launch={rg.intended_launch}, fast={rg.fast}, "
                f"mlp_plain_burst={rg.mlp_plain_burst}, fused_burst={rg.fused_burst}, graphs {sorted(k for k, _ in rg.bursts)}" +
                (f"; {rg.bench_note}" if hasattr(rg, "bench_note") else ""))
        assert forms["routed"].fused_burst and forms["routed"].intended_launch and forms["routed"]._burst_form == "intended"
        assert forms["reference"].fused_burst and not forms["reference"].intended_launch
        assert not forms["body"].fused_burst and not forms["body"].mlp_plain_burst
        for m in LENGTHS:
            for rg in forms.values():                           # every length warmed, every form
                rg.run(m)
                rg.run(m)
            torch.cuda.synchronize()
            per = {form: [] for form in FORMS}
            for _ in range(a.reps):
                for form in FORMS:                              # alternating: every form sees the same neighbours
                    rg = forms[form]
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(a.runs):
                        rg.run(m)
                    e1.record()
                    torch.cuda.synchronize()
                    per[form].append(e0.elapsed_time(e1) * 1e3 / (a.runs * m))
            txt = "  |  ".join(f"{form} {statistics.median(per[form]):.2f} [{min(per[form]):.2f} .. {max(per[form]):.2f}]" for form in FORMS)
            say(f"{agent} m {m:3d}: us per vector step: {txt}  (medians of {a.reps}, device events, {a.runs} x run({m}) per sample)")
            slowest, fastest = max(per["routed"]), min(per["body"])
            ok = ok and slowest < fastest
            say(f"{agent} m {m:3d}: bar 1: the routed burst's slowest sample {slowest:.2f} {'is below' if slowest < fastest else 'IS NOT BELOW'} "
                f"today's intended body's fastest, {fastest:.2f}")
            if m == 96:
                med, lo, hi = statistics.median(per["routed"]), min(per["reference"]) / 1.03, max(per["reference"]) * 1.03
                inside = lo <= med <= hi
                ok = ok and inside
                say(f"{agent} m  96: bar 2: the routed burst's median {med:.2f} {'lies within' if inside else 'LIES OUTSIDE'} the reference-"
                    f"routing burst's spread widened by 3 %, [{lo:.2f} .. {hi:.2f}]; ratio of medians "
                    f"{med / statistics.median(per['reference']):.4f}")
        # what the environment phase had to do under each routing: the two routings feed the step different actions, so the
        # trajectories — and with them the data-dependent work of a step's power-flow solve — are not the same
        work = {form: [] for form in FORMS}
        for _ in range(8):
            for form in FORMS:
                vec = getattr(forms[form].env, "vec", forms[form].env)
                forms[form].run(12)
                work[form].append((float(vec.peek("PF_SWEEPS").double().mean()), float(vec.peek("PF_ITERS").double().mean()),
                                   float((vec.done != 0).double().mean()), float((vec.failed != 0).double().mean()),
                                   # (the stand-alone projection of the last stored action on the state the step left: one step
                                   #  late, which as a share over 4096 environments is neither here nor there)
                                   float(vec.safety_project(forms[form].act_buf.view(a.envs, -1, 4), *forms[form].predictor,
                                                            forms[form].model.V_min, forms[form].model.V_max)[1].double().mean())
                                   if hasattr(forms[form], "act_buf") else float("nan")))
        say(f"{agent}: work of a step, mean over envs and 8 samples 12 steps apart (power-flow sweeps, Newton iterations, share of "
            f"envs restarted in the step, share whose solve failed, share where the projection intervenes): " +
            "  |  ".join(f"{form} " + ", ".join(f"{statistics.mean(w[j] for w in work[form]):.4f}" for j in range(5)) for form in FORMS))
        del forms, rg
        gc.collect()
        torch.cuda.empty_cache()

    # test mode: Model.test_episodes as a call
    os.environ["FLEX_MLP_TEST_LAUNCH"] = "1"                             # (read at call time by one_launch_declines)
    env_args, net, series = world
    rng = np.random.default_rng(4)
    spec = dict(day=rng.integers(0, 20, a.envs).astype(np.int32), hour=rng.integers(0, 24, a.envs).astype(np.int32),
                interval=rng.integers(0, 4, a.envs).astype(np.int32))
    tests = ("launch routing 1", "launch reference", "loop intended")
    for agent in AGENTS:
        env = VecFlexProvisionEnv(env_args, a.envs, net=net, series=series, seed=9, warm_start=True)
        models = {"launch routing 1": _model(agent, env, "routed"), "launch reference": _model(agent, env, "reference"),
                  "loop intended": _model(agent, env, "body")}

        def call(name):
            os.environ[SWITCH] = "1" if name == "launch routing 1" else "0"
            res = models[name].test_episodes(env, spec, one_launch=name != "loop intended")
            assert res.launch == (name != "loop intended") and (res.length == 95).all()

        for name in tests:
            call(name)
            call(name)
        torch.cuda.synchronize()
        per = {name: [] for name in tests}
        for _ in range(a.reps):
            for name in tests:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                call(name)
                e1.record()
                torch.cuda.synchronize()
                per[name].append(e0.elapsed_time(e1) * 1e3 / 95)
        txt = "  |  ".join(f"{name} {statistics.median(per[name]):.2f} [{min(per[name]):.2f} .. {max(per[name]):.2f}]" for name in tests)
        say(f"{agent} test_episodes, {a.envs} envs, 95 steps: us per vector step as a call: {txt}  (medians of {a.reps}, device events)")
        del models, env
        gc.collect()
        torch.cuda.empty_cache()
    os.environ.pop(SWITCH, None)
    os.environ.pop("FLEX_MLP_TEST_LAUNCH", None)

    if not a.no_train:
        sides = [("--intended-launch", ["--intended-launch"]), ("switch unset", [])]
        rate = {name: [] for name, _ in sides}
        for _ in range(a.rounds):
            for name, extra in sides:                           # alternating, a fresh process each
                cmd = [sys.executable, os.path.join(ROOT, "examples", "train_maddpg.py"), "--alg", "safemaddpg", "--envs",
                       str(a.train_envs), "--intended-actions"] + extra
                env = {k: v for k, v in os.environ.items() if k not in (SWITCH, "FLEX_MLP_BURST", "FLEX_ROLLOUT_BURST", "PYTHONPATH")}
                out = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=900)
                if out.returncode != 0:
                    tail = (out.stderr.strip().splitlines() or [""])[-1]
                    say(f"train safemaddpg --intended-actions ({name}): exit {out.returncode}: {tail[:200]}")
                    raise SystemExit(1)
                res = next(json.loads(ln) for ln in reversed(out.stdout.splitlines()) if ln.startswith("{"))
                rate[name].append(res["value"])
                say(f"train safemaddpg --intended-actions ({name}): {res['value']:.0f} env-steps/s, {res['ms_per_vector_step']:.3f} ms "
                    f"per vector step, rollout_burst_launch {res.get('rollout_burst_launch')}, fallbacks {res.get('fallbacks')}")
                if bool(res.get("rollout_burst_launch")) != bool(extra):
                    ok = False
        say(f"train safemaddpg --envs {a.train_envs} --intended-actions, env-steps/s (context, not a bar): " +
            "  |  ".join(f"{name} " + " ".join(f"{v:.0f}" for v in vs) for name, vs in rate.items()))

    say("# compiler resource report of this build (build.kernel_resources)")
    for prefix in ("intended::", "flex_rollout_burst_kernel<", "plain_mlp::flex_rollout_burst", "flex_test_episodes_kernel<",
                   "test_mlp::flex_test_episodes"):
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
