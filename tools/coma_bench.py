"""COMA's counterfactual baseline (csrc/coma.hip) against the materialising composition (nets.coma_baseline_torch, which
restates coma.py:139-149), the fused policy loss, and whole value / policy sub-updates through the trainer, at the trainer's
pooled on-policy batch (32 steps x 4096 envs = 131 072 samples x 5 agents x 10 draws = 6.55 M critic rows) and at a
quarter of it.  Every figure is the median (and min..max) of single calls timed with HIP events after warm-up, the two
baseline forms alternated call by call.  The composition runs ``--chunk`` draws at a time (all ten at once are 23 GB at the
full batch).  ``--train`` adds the env-steps/s of ``examples/train_maddpg.py --alg coma --envs 4096`` (a child process).
Prints one JSON line and writes it to the file named last on the command line, if any.

    python tools/coma_bench.py [--batches 131072,32768] [--chunk 1] [--reps 15] [--train] [out.json]
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import safe_marl_amd  # noqa: F401
from safe_marl_amd.learner import COMA
from safe_marl_amd.nets import coma_baseline, coma_baseline_torch, coma_policy_loss
from safe_marl_amd.replay_buffer import Transition
from safe_marl_amd.trainer import PGTrainer
from safe_marl_amd.util import convert

ap = argparse.ArgumentParser()
ap.add_argument("--batches", default="131072,32768")
ap.add_argument("--chunk", type=int, default=1, help="draws per pass of the composition")
ap.add_argument("--reps", type=int, default=15)
ap.add_argument("--train", action="store_true")
ap.add_argument("out", nargs="?")
cli = ap.parse_args()

G = os.path.join(ROOT, "tests", "golden")
args = convert({**json.load(open(os.path.join(G, "coma_args.json"))), "cuda": True})
N, O, A, NS = args.agent_num, args.obs_size, args.action_dim, args.sample_size
PEAK_FP32_MATRIX = 157.3e12
torch.manual_seed(0)


class StubEnv:
    n_envs = 1

    def get_num_of_agents(self):
        return N


def once(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3


def stats(xs):
    return {"median_us": round(float(np.median(xs)), 2), "min_us": round(min(xs), 2), "max_us": round(max(xs), 2), "calls": len(xs)}


def timed(fn, reps, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    return stats([once(fn) for _ in range(reps)])


tr = PGTrainer(args, COMA, StubEnv(), None)
m = tr.behaviour_net
net = m.value_dicts[0]
z = dict(np.load(os.path.join(G, "learner_batch.npz")))
z["action"] = np.repeat(z["action"][:, :1], N, axis=1)
res = {"n_agents": N, "sample_size": NS, "composition_chunk_draws": cli.chunk, "sizes": {}}

for B in [int(x) for x in cli.batches.split(",")]:
    r = {"critic_rows": B * N * NS}
    obs = 0.5 * torch.randn(B, N, O, device="cuda")
    act = torch.rand(B, N, A, device="cuda")
    sampled = act.unsqueeze(0) + torch.randn(NS, B, N, A, device="cuda")
    with torch.no_grad():
        z1 = m.first_layer(obs, act)
    fused = lambda: coma_baseline(net, z1, act, sampled, want_values=True)                        # noqa: E731
    comp = lambda: coma_baseline_torch(net, obs, act, sampled, s_chunk=cli.chunk)                 # noqa: E731
    with torch.no_grad():
        for _ in range(3):
            fused()
        comp()
        torch.cuda.synchronize()
        tf, tc = [], []
        for _ in range(cli.reps):                                # alternated: both see the same machine
            tf.append(once(fused))
            tc.append(once(comp))
        base, _, _ = fused()
        ref, _ = comp()
    r["baseline_hip"], r["baseline_composition"] = stats(tf), stats(tc)
    r["baseline_max_abs_difference"] = float((base - ref).abs().max())
    r["faster_beyond_spread"] = bool(max(tf) < min(tc))
    r["speedup_median"] = round(r["baseline_composition"]["median_us"] / r["baseline_hip"]["median_us"], 2)
    flop = 2.0 * 64 * 64 * B * N * (NS + 1)                       # fc2 of every row walked (the draws and the row itself)
    r["fc2_gflop"] = round(flop / 1e9, 2)
    r["baseline_hip_fp32_matrix_peak_fraction"] = round(flop / (r["baseline_hip"]["median_us"] * 1e-6) / PEAK_FP32_MATRIX, 4)
    del sampled, ref
    torch.cuda.empty_cache()
    # policy loss with its gradients: forward launch + backward through the node
    means = torch.randn(B, N, A, device="cuda", requires_grad=True)
    log_stds = m._log_stds_like(means)
    q, bl = torch.randn(B, N, device="cuda"), torch.randn(B, N, device="cuda")

    def ploss(fused_):
        loss, _ = coma_policy_loss(means, log_stds, act, None, q, bl, fused=fused_)
        torch.autograd.grad(loss, [means])
    r["policy_loss_hip"] = timed(lambda: ploss(True), cli.reps)
    r["policy_loss_composition"] = timed(lambda: ploss(False), cli.reps)
    # whole sub-updates through the trainer (loss, backward, clip, RMSprop)
    batch = Transition(**{k: torch.from_numpy(z[k]).float().cuda().repeat((B // 32,) + (1,) * (z[k].ndim - 1)).contiguous()
                          for k in Transition._fields})
    stat = {}
    r["value_sub_update"] = timed(lambda: tr._sub_update("value", stat, batch), max(5, cli.reps // 2))
    r["policy_sub_update"] = timed(lambda: tr._sub_update("policy", stat, batch), max(5, cli.reps // 2))
    res["sizes"][str(B)] = r
    del batch, obs, act, z1, means, q, bl
    torch.cuda.empty_cache()

if cli.train:
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "train_maddpg.py"), "--alg", "coma", "--envs", "4096",
                          "--episodes", "3"], capture_output=True, text=True, cwd=ROOT)
    if out.returncode != 0:
        sys.exit("train_maddpg.py --alg coma failed:\n" + out.stderr[-3000:])
    t = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("{")][-1])
    res["train"] = {k: t[k] for k in ("value", "unit", "envs_per_gpu", "vector_steps", "ms_per_vector_step", "batch", "grad_steps",
                                      "fallbacks")}

line = json.dumps(res)
print(line)
if cli.out:
    with open(cli.out, "w") as f:
        f.write(line + "\n")
