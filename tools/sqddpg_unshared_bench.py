"""SQDDPG with shared_params False: csrc/sqddpg_unshared.hip (FLEX_UNSHARED_CRITICS=1) against the tensor composition that runs
without the switch, at 5 agents, obs 144, act 4, sample_size 10 and 4 096 / 32 768 samples.  The two paths alternate in one
process; every figure is the median of ten single calls between device events, with min .. max.  Three calls: shapley_values
under no_grad; the value term forward + backward with every critic parameter's gradient; the policy term (critic frozen, the
own-action gradient).  The shared critic's kernel (csrc/sqddpg.hip) on the same rows is timed in the same process as context:
five sets of weights cost something.  Bar: at both sizes and for all three calls the kernel path's slowest sample is below the
composition's fastest.

With --train it then runs examples/train_maddpg.py --unshared --envs 4096 --episodes 3 in fresh processes, alternating without
and with --unshared-critics, two runs a side, for --alg sqddpg (bar 2: the switched runs' slower run beats the unswitched
runs' faster one) and for --alg facmaddpg (reported without a bar: its loop is cheap).

    python tools/sqddpg_unshared_bench.py [--train] [out.txt]          (default: profiles/sqddpg_unshared_bench.txt)
"""
import json
import os
import statistics
import subprocess
import sys
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import safe_marl_amd  # noqa: E402,F401
from safe_marl_amd import build, util  # noqa: E402
from safe_marl_amd.learner import SQDDPG  # noqa: E402
from safe_marl_amd.util import convert  # noqa: E402

SWITCH = "FLEX_UNSHARED_CRITICS"
REPS = 10
G = os.path.join(ROOT, "tests", "golden")
base = json.load(open(os.path.join(G, "sqddpg_args.json")))


def model(shared):
    torch.manual_seed(0)
    return SQDDPG(convert({**base, "cuda": True, "shared_params": shared})).cuda()


def one_call(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3                       # microseconds


def calls(m, obs, act, pos, w):
    n = act.shape[1]
    params = list(m.value_dicts.parameters())

    def forward():
        with torch.no_grad():
            m.shapley_values(obs, act, pos)

    def value_term():
        phi, _ = m.shapley_values(obs, act, pos)
        torch.autograd.grad(((phi.sum(-1) - w[:, 0]) ** 2).mean(), params)

    def policy_term():
        a = act.detach().requires_grad_(True)
        phi, _ = m.shapley_values(obs, a, pos, frozen=True)
        torch.autograd.grad(-phi.mean(), [a])
    assert n == 5
    return {"shapley_values (no_grad)": forward, "value term (forward + backward, parameter gradients)": value_term,
            "policy term (frozen critic)": policy_term}


def train_pairs(lines):
    """Bar 2 and FACMADDPG's pair: env-steps/s of fresh processes, off / on / off / on."""
    lines += ["examples/train_maddpg.py --unshared --envs 4096 --episodes 3, fresh processes alternating without / with",
              "--unshared-critics (training env-steps/s: rollout + replay + updates; the fallback counts are the run's own):"]
    bar = None
    for alg in ("sqddpg", "facmaddpg"):
        rate = {False: [], True: []}
        for run in range(2):
            for on in (False, True):
                cmd = [sys.executable, os.path.join(ROOT, "examples", "train_maddpg.py"), "--unshared", "--alg", alg, "--envs", "4096",
                       "--episodes", "3"] + (["--unshared-critics"] if on else [])
                env = {k: v for k, v in os.environ.items() if k != SWITCH}
                r = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=300, check=True)
                res = json.loads(r.stdout.strip().splitlines()[-1])
                rate[on].append(res["value"])
                lines.append(f"  {alg:10s} run {run + 1} {'with   ' if on else 'without'} {res['value'] / 1e6:7.3f} M env-steps/s, "
                             f"{res['ms_per_vector_step']:.3f} ms per vector step, fallbacks {res['fallbacks']}")
        ok = min(rate[True]) > max(rate[False])
        lines.append(f"  {alg}: slower switched run {min(rate[True]) / 1e6:.3f} M against faster unswitched run "
                     f"{max(rate[False]) / 1e6:.3f} M ({min(rate[True]) / max(rate[False]):.2f}x)"
                     + (f"; bar 2: {'met' if ok else 'NOT met'}" if alg == "sqddpg" else " (no bar)"))
        if alg == "sqddpg":
            bar = ok
    lines.append("")
    return bar


def main():
    argv = [a for a in sys.argv[1:] if a != "--train"]
    out = argv[0] if argv else os.path.join(ROOT, "profiles", "sqddpg_unshared_bench.txt")
    lines = [f"tools/sqddpg_unshared_bench.py on {torch.cuda.get_device_name(0)}, library source digest {build.source_digest()[:16]}",
             f"5 agents, obs 144, act 4, sample_size 10; microseconds per call, median of {REPS} [min .. max], device events;",
             "the kernel path (FLEX_UNSHARED_CRITICS=1) and the composition (unset) alternate call by call in one process.", ""]
    unshared, shared = model(False), model(True)
    bar = True
    warnings.simplefilter("ignore")
    for B in (4096, 32768):
        g = torch.Generator(device="cuda").manual_seed(B)
        obs = 0.5 * torch.randn(B, 5, 144, device="cuda", generator=g)
        act = torch.rand(B, 5, 4, device="cuda", generator=g)
        w = torch.randn(B, 5, device="cuda", generator=g)
        pos = torch.argsort(torch.rand(B * 10, 5, device="cuda", generator=g), dim=1).argsort(dim=1).to(torch.int32)
        lines.append(f"{B} samples ({B * 50} critic rows of 745 columns: {B * 50 * 745 * 4 / 1e9:.2f} GB if formed)")
        un, sh = calls(unshared, obs, act, pos, w), calls(shared, obs, act, pos, w)
        for name in un:
            t = {"kernel": [], "composition": [], "shared": []}
            for rep in range(-2, REPS):                    # two warm-up rounds of all three
                for path in t:
                    if path == "kernel":
                        os.environ[SWITCH] = "1"
                    else:
                        os.environ.pop(SWITCH, None)
                    us = one_call(sh[name] if path == "shared" else un[name])
                    if rep >= 0:
                        t[path].append(us)
            ok = max(t["kernel"]) < min(t["composition"])
            bar = bar and ok
            lines.append(f"  {name}")
            for path, label in (("kernel", "per-agent kernels"), ("composition", "composition"), ("shared", "shared kernel (context)")):
                lines.append(f"    {label:26s} {statistics.median(t[path]):10.1f} [{min(t[path]):10.1f} .. {max(t[path]):10.1f}]")
            lines.append(f"    composition / kernel (medians) {statistics.median(t['composition']) / statistics.median(t['kernel']):.1f}x; "
                         f"slowest kernel sample below the fastest composition sample: {ok}")
        lines.append("")
        torch.cuda.empty_cache()
    assert util.FALLBACKS.get("sqddpg_unshared", 0) == 0, "the kernel path declined"
    lines += [f"bar 1 (all six comparisons): {'met' if bar else 'NOT met'}", ""]
    if "--train" in sys.argv[1:]:
        del unshared, shared, obs, act, w, pos, un, sh
        torch.cuda.empty_cache()
        train_pairs(lines)
    else:
        lines.append("not measured in this run: the training pairs of bar 2 (--train)")
    text = "\n".join(lines) + "\n"
    print(text)
    with open(out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
