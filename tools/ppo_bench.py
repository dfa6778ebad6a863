"""PPO around the networks (csrc/ppo.hip) at the trainer's pooled batch — 4096 envs x 32 steps x 5 agents = 131 072 rows,
chain stride 4096 — against the PyTorch composition of the same formulas (nets.ppo_gae_torch with its time-step loop,
ppo_policy_loss_torch, ppo_value_loss_torch) run in the same process on the same tensors, alternating; then whole
``get_loss`` value and policy paths of IPPO and MAPPO (fused_ppo on / off), each with its backward; optionally (--train) the
training rate of examples/train_maddpg.py --alg ippo / mappo.  HIP-event timed after warm-up, median and min..max of
repeated windows.  Prints one JSON line."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import torch.nn as nn
import safe_marl_amd  # noqa: F401
from safe_marl_amd import nets
from safe_marl_amd.learner import IPPO, MAPPO
from safe_marl_amd.replay_buffer import Transition
from safe_marl_amd.util import convert

ENVS, STEPS = int(os.environ.get("PPO_BENCH_ENVS", "4096")), 32
G = os.path.join(ROOT, "tests", "golden")
ARGS = {**json.load(open(os.path.join(G, "ippo_args.json"))), "cuda": True}
N, O, A = ARGS["agent_num"], ARGS["obs_size"], ARGS["action_dim"]
ROWS = ENVS * STEPS
dev = "cuda"
torch.manual_seed(0)


def timed(fn, n=20, warm=3, windows=5):
    for _ in range(warm):
        fn()
    out = []
    for _ in range(windows):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / n * 1e3)
    return out


def pair(fused, plain, **k):
    """Both forms in alternating windows: {fused_us, torch_us: [median, min, max], speedup (of the medians)}."""
    f, p = [], []
    for _ in range(3):
        f += timed(fused, windows=2, **k)
        p += timed(plain, windows=2, **k)
    s = lambda x: [round(float(np.median(x)), 1), round(min(x), 1), round(max(x), 1)]
    return {"fused_us": s(f), "torch_us": s(p), "speedup": round(float(np.median(p) / np.median(f)), 2)}


def bn():
    return nn.BatchNorm1d(N).to(dev)


reward = 0.05 * torch.randn(ROWS, N, device=dev) - 0.03
old_v, old_nv = torch.randn(ROWS, N, device=dev), torch.randn(ROWS, N, device=dev)
last = (torch.rand(ROWS, device=dev) < 0.05).float()
done = (torch.rand(ROWS, device=dev) < 0.5).float() * last
rbn, abn = bn(), bn()
res = {"rows": ROWS, "agents": N, "chain_stride": ENVS, "steps_per_chain": STEPS}
gae = lambda fused: nets.ppo_gae(reward, old_v, old_nv, done, last, 0.99, 0.95, ENVS, rbn, abn, fused=fused)
res["gae"] = pair(lambda: gae(True), lambda: gae(False))
rn, adv, advn = gae(True)

means = (0.3 * torch.randn(ROWS, N, A, device=dev)).requires_grad_(True)
act = torch.tanh(torch.randn(ROWS, 1, A, device=dev)).expand(ROWS, N, A).contiguous()
ls = torch.zeros(1, device=dev).expand_as(means)
ls._flex_entropy = torch.zeros((), device=dev)
avail = torch.ones(1, 1, 1, device=dev).expand(ROWS, N, A)
avail._flex_const = 1.0


def pol(fused):
    loss, _ = nets.ppo_policy_loss(means, ls, act, None, advn, 0.6, avail, fused=fused)
    torch.autograd.grad(loss, [means])


res["policy_loss_fwd_bwd"] = pair(lambda: pol(True), lambda: pol(False))
values = torch.randn(ROWS, N, device=dev, requires_grad=True)
nv = torch.randn(ROWS, N, device=dev)


def val(fused):
    loss, _ = nets.ppo_value_loss(values, old_v, nv, rn, done, 0.99, 0.6, 2.0, fused=fused)
    torch.autograd.grad(loss, [values])


res["value_loss_fwd_bwd"] = pair(lambda: val(True), lambda: val(False))

# whole get_loss + backward of the parameters the sub-update steps on
z = np.load(os.path.join(G, "learner_batch.npz"))
batch = {k: torch.from_numpy(z[k]).float().to(dev).repeat((ROWS // 32,) + (1,) * (z[k].ndim - 1)).contiguous()
         for k in Transition._fields}
batch["action"] = batch["action"][:, :1].expand(ROWS, N, A).contiguous()
batch["action_avail"] = avail
batch["last_step"], batch["done"] = last, done
batch = Transition(**batch)
for name, cls in (("ippo", IPPO), ("mappo", MAPPO)):
    model = cls(convert(ARGS)).to(dev)
    model.gae_chain_stride = ENVS
    for need, params in (("value", list(model.value_dicts.parameters())), ("policy", list(model.policy_dicts.parameters()))):
        def step(fused):
            model.fused_ppo = fused
            p, v, _ = model.get_loss(batch, need=need)
            torch.autograd.grad(v if need == "value" else p, params)
        res[f"{name}_get_loss_{need}"] = pair(lambda: step(True), lambda: step(False), n=5, warm=2)
    del model

if "--train" in sys.argv:
    for alg in ("ippo", "mappo"):
        out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "train_maddpg.py"), "--alg", alg, "--envs",
                              str(ENVS), "--episodes", "10"], capture_output=True, text=True, timeout=900, cwd=ROOT)
        line = [l for l in out.stdout.splitlines() if l.startswith("{")]
        res[f"train_{alg}_env_steps_per_s"] = round(json.loads(line[-1])["value"]) if line else out.stderr[-400:]
print(json.dumps(res))
