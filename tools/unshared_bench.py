"""The per-agent actors of ``shared_params: False`` (csrc/actor_unshared.hip) against the module composition they replace —
Model.policy's loop over ``policy_dicts`` with ``model.fused_inference = False`` — in ONE process on one GPU, on the same
tensors, in alternating windows: 20 480 rows (the rollout: 4 096 environments x 5 agents) and 163 840 rows (the update),
inference (no_grad) and training forward + backward (every agent's ten parameter gradients).  As a yardstick, the shared
kernel (csrc/actor.hip and its node) on ONE agent's weights at the same row counts: what n identical copies would cost with
``shared_params: True``.  HIP-event timed after warm-up, median and min..max of repeated windows.  Prints one JSON line."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "examples"))
import numpy as np
import torch
import safe_marl_amd  # noqa: F401
from safe_marl_amd import build, nets
from safe_marl_amd.learner import MADDPG
from safe_marl_amd.util import FALLBACKS, convert
from train_maddpg import DEFAULT_ALG_ARGS

N, OBS, A = 5, 144, 4
SIZES = [int(s) for s in os.environ.get("UNSHARED_BENCH_ROWS", "20480,163840").split(",")]
dev = "cuda"


def timed(fn, n=10, warm=3, windows=2):
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


def stat(x):
    return [round(float(np.median(x)), 1), round(min(x), 1), round(max(x), 1)]


def pair(fused, plain):
    """Both forms in alternating windows: {fused_us, torch_us: [median, min, max], speedup (of the medians)}."""
    f, p = [], []
    for _ in range(3):
        f += timed(fused)
        p += timed(plain)
    return {"fused_us": stat(f), "torch_us": stat(p), "speedup": round(float(np.median(p) / np.median(f)), 2)}


def model_of(shared):
    a = dict(DEFAULT_ALG_ARGS)
    a.update(alg="maddpg", agent_num=N, obs_size=OBS, state_size=3 * 33 + 2 * N + 1, action_dim=A, shared_params=shared)
    torch.manual_seed(0)
    m = MADDPG(convert(a)).cuda()
    with torch.no_grad():
        for p in m.policy_dicts.parameters():
            p.mul_(3.0).add_(0.05 * torch.randn_like(p))
    return m


res = {"n_agents": N, "obs_dim": OBS, "act_dim": A, "device": torch.cuda.get_device_name(0), "library": build.built_digest()[:16]}
unshared, shared = model_of(False), model_of(True)
for rows in SIZES:
    b = rows // N
    obs = 0.5 * torch.randn(b, N, OBS, device=dev)
    hid = 0.5 * torch.randn(b, N, 64, device=dev)
    proj = torch.randn(b, N, A, device=dev) / rows

    def infer(model, fused):
        model.fused_inference = fused
        with torch.no_grad():
            return model.policy(obs, last_hid=hid)

    def train(model, fused):
        model.fused_inference = fused
        means, _, _ = model.policy(obs, last_hid=hid)
        return torch.autograd.grad((means * proj).sum(), list(model.policy_dicts.parameters()))

    r = {"inference": pair(lambda: infer(unshared, True), lambda: infer(unshared, False)),
         "train_forward_backward": pair(lambda: train(unshared, True), lambda: train(unshared, False)),
         "shared_kernel_inference_us": stat(timed(lambda: infer(shared, True), windows=6)),
         "shared_kernel_train_forward_backward_us": stat(timed(lambda: train(shared, True), windows=6))}
    unshared.fused_inference = True
    # the device side of the node alone: forward launch, backward launch, the 4 n weight-gradient launches
    means, _, _ = unshared.policy(obs, last_hid=hid)
    params = list(unshared.policy_dicts.parameters())
    loss = (means * proj).sum()
    r["node_backward_only_us"] = stat(timed(lambda: torch.autograd.grad(loss, params, retain_graph=True), windows=6))
    with torch.no_grad():
        r["inference_launch_only_us"] = stat(timed(lambda: nets.fused_actor_forward_unshared(unshared.policy_dicts, obs, hid),
                                                   n=50, windows=6))
    res[f"rows_{rows}"] = r
res["fallbacks"] = dict(FALLBACKS)
print(json.dumps(res))
