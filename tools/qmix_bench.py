"""QMIX mixer of FACMADDPG: csrc/qmix.hip (forward, and backward with the flexnet_wgrad reductions) against the PyTorch
composition of the same module (QMixer.forward_torch), at the trainer's batch (4096 envs: 32 768 samples, 5 agents).
HIP-event timed, 50 calls each after warm-up.  Prints one JSON line; FLOP counts from the multiply-adds of qmix.py:53-81."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import safe_marl_amd  # noqa: F401
from safe_marl_amd.nets import QMixer
from safe_marl_amd.util import convert

B = int(os.environ.get("QMIX_BENCH_B", "32768"))
N, O = 5, 144
S = N * O
args = convert(dict(agent_num=N, obs_size=O, mixing_embed_dim=64, hypernet_layers=2, hypernet_embed=64,
                    hyper_initialization_nonzeros=0, gated=False, skip_connections=False))
torch.manual_seed(0)
m = QMixer(args).cuda()
q = torch.randn(B, N, device="cuda", requires_grad=True)
x = 0.3 * torch.randn(B, S, device="cuda")
w = torch.randn(B, device="cuda") / B


def timed(fn, n=50):
    for _ in range(10):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e3


def fwd(f):
    with torch.no_grad():
        f(q, x)


def fwd_bwd(f):
    y = f(q, x)
    grads = torch.autograd.grad((y.view(-1) * w).sum(), [q] + list(m.parameters()))
    return grads


res = {}
res["hip_forward_us"] = timed(lambda: fwd(m))
res["torch_forward_us"] = timed(lambda: fwd(m.forward_torch))
res["hip_forward_backward_us"] = timed(lambda: fwd_bwd(m))
res["torch_forward_backward_us"] = timed(lambda: fwd_bwd(m.forward_torch))
res["hip_backward_us"] = res["hip_forward_backward_us"] - res["hip_forward_us"]
res["torch_backward_us"] = res["torch_forward_backward_us"] - res["torch_forward_us"]
macs_fwd = B * (S * 256 + 64 * 64 * N + 64 * 64 + 64 + 64 * N + 64)
macs_bwd = B * (S * 256 + 2 * (64 * 64 * N + 64 * 64 + 64))            # weight gradients + input gradients of the second layers
peak = 157.3e12
res.update(batch=B, n_agents=N, state_dim=S, forward_gflop=2 * macs_fwd / 1e9, backward_gflop=2 * macs_bwd / 1e9,
           hip_forward_peak_fraction=2 * macs_fwd / (res["hip_forward_us"] * 1e-6) / peak,
           hip_backward_peak_fraction=2 * macs_bwd / (res["hip_backward_us"] * 1e-6) / peak,
           speedup_forward=res["torch_forward_us"] / res["hip_forward_us"],
           speedup_forward_backward=res["torch_forward_backward_us"] / res["hip_forward_backward_us"])
print(json.dumps({k: (round(v, 4) if isinstance(v, float) else v) for k, v in res.items()}))
