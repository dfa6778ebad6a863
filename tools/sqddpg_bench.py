"""SQDDPG's Shapley-value critic: csrc/sqddpg.hip (forward; backward with parameter gradients) and whole value / policy
sub-updates through the trainer, against the PyTorch composition (SQDDPG.marginal_contribution_torch), at the trainer's
batch (4096 envs: 32 768 samples, 5 agents, sample_size 10 -> 1 638 400 critic rows per call).  HIP-event timed after
warm-up.  The composition materialises the [rows, 745] critic input (4.9 GB) and its activations; where it does not fit
in memory it is reported as such.  Prints one JSON line; FLOP counts from the multiply-adds of the critic rows."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import safe_marl_amd  # noqa: F401
from safe_marl_amd.learner import SQDDPG
from safe_marl_amd.replay_buffer import Transition
from safe_marl_amd.trainer import PGTrainer
from safe_marl_amd.util import convert

B = int(os.environ.get("SQDDPG_BENCH_B", "32768"))
G = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden")
args = convert({**json.load(open(os.path.join(G, "sqddpg_args.json"))), "cuda": True})
N, O, A, NS = args.agent_num, args.obs_size, args.action_dim, args.sample_size
ROWS = B * NS * N
torch.manual_seed(0)


class StubEnv:
    n_envs = 1

    def get_num_of_agents(self):
        return N


tr = PGTrainer(args, SQDDPG, StubEnv(), None)
m = tr.behaviour_net
obs = 0.5 * torch.randn(B, N, O, device="cuda")
act = torch.rand(B, N, A, device="cuda", requires_grad=True)
w = torch.randn(B, N, device="cuda") / B
pos = m.draw_coalitions("value", B, obs.device)
z = np.load(os.path.join(G, "learner_batch.npz"))
batch = Transition(**{k: torch.from_numpy(z[k]).float().cuda().repeat((B // 32,) + (1,) * (z[k].ndim - 1)).contiguous()
                      for k in Transition._fields})


def timed(fn, n=20, warm=3):
    for _ in range(warm):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e3


def fwd(fused):
    with torch.no_grad():
        if fused:
            m.shapley_values(obs, act, pos)
        else:
            m.marginal_contribution_torch(obs, act, pos).mean(1)


def fwd_bwd(fused):
    if fused:
        phi, _ = m.shapley_values(obs, act, pos)
    else:
        phi = m.marginal_contribution_torch(obs, act, pos).mean(1).view(B, N)
    return torch.autograd.grad((phi * w).sum(), [act] + list(m.value_dicts.parameters()))


res = {}
res["hip_forward_us"] = timed(lambda: fwd(True))
res["hip_forward_backward_us"] = timed(lambda: fwd_bwd(True))
res["hip_backward_us"] = res["hip_forward_backward_us"] - res["hip_forward_us"]
stat = {}
res["value_sub_update_us"] = timed(lambda: tr._sub_update("value", stat, batch), n=10)
res["policy_sub_update_us"] = timed(lambda: tr._sub_update("policy", stat, batch), n=10)
for name, fn in (("torch_forward_us", lambda: fwd(False)), ("torch_forward_backward_us", lambda: fwd_bwd(False))):
    try:
        res[name] = timed(fn, n=3, warm=1)
    except torch.cuda.OutOfMemoryError as e:
        res[name] = None
        res[name.replace("_us", "_error")] = "out of memory: " + str(e).split("\n")[0][:160]
    torch.cuda.empty_cache()
macs_row = 64 * (N * A) + 64 * 64 + 64                  # the composed row: action block, fc2, fc3 (z_shared once per sample)
macs_fwd = ROWS * macs_row + B * 64 * N * O
macs_bwd = ROWS * (macs_row + 2 * 64 * 64 + 64 * N * A) + 2 * B * 64 * N * O    # recomputed forward + dW2, da1, dW_act
peak = 157.3e12
res.update(batch=B, n_agents=N, sample_size=NS, critic_rows=ROWS, forward_gflop=2 * macs_fwd / 1e9,
           backward_gflop=2 * macs_bwd / 1e9,
           hip_forward_peak_fraction=2 * macs_fwd / (res["hip_forward_us"] * 1e-6) / peak,
           hip_backward_peak_fraction=2 * macs_bwd / (res["hip_backward_us"] * 1e-6) / peak)
if res.get("torch_forward_us"):
    res["speedup_forward"] = res["torch_forward_us"] / res["hip_forward_us"]
if res.get("torch_forward_backward_us"):
    res["speedup_forward_backward"] = res["torch_forward_backward_us"] / res["hip_forward_backward_us"]
out = json.dumps({k: (round(v, 4) if isinstance(v, float) else v) for k, v in res.items()})
print(out)
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f:
        f.write(out + "\n")
