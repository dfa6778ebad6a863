"""MATD3's per-agent twin critics of ``shared_params: False`` (csrc/critic_unshared_twin.hip, flexnet_wgrad_batched) against the
composition they replace — the per-agent loop of MATD3.unshared_twin_values with ``model.fused_inference = False`` — in ONE
process on one GPU, on the same tensors, eager, in alternating windows: 5 agents, obs 144, act 4 (rows of 746 columns) at 20 480
and 163 840 critic rows.  Three branches, the ones MATD3.value dispatches: ``value()`` under no_grad (two heads, the bootstrap
target), the value loss forward + backward with every parameter gradient (two heads), and the policy pass (first head, critics
frozen, the gradient of the actions).  Device-event timed after warm-up; per form the median and min .. max of twelve windows of
ten calls.  Prints one JSON line; ``dispatch`` says per branch whether the fused median is at or below the composition's at
BOTH sizes — the bar a dispatch branch of MATD3.value has to clear to stay on."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "examples"))
import numpy as np
import torch
import safe_marl_amd  # noqa: F401
from safe_marl_amd import build, learner
from safe_marl_amd.util import FALLBACKS, convert
from train_maddpg import DEFAULT_ALG_ARGS

N, OBS, A = 5, 144, 4
SIZES = [int(s) for s in os.environ.get("UNSHARED_BENCH_ROWS", "20480,163840").split(",")]
dev = "cuda"


def timed(fn, n=10, warm=3, windows=4):
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
    """Both forms in alternating windows: {fused_us, torch_us: [median, min, max] of twelve windows, speedup (of the medians)}."""
    f, p = [], []
    for _ in range(3):
        f += timed(fused)
        p += timed(plain)
    return {"fused_us": stat(f), "torch_us": stat(p), "windows": len(f), "speedup": round(float(np.median(p) / np.median(f)), 2)}


a = dict(DEFAULT_ALG_ARGS)
a.update(alg="matd3", agent_num=N, obs_size=OBS, state_size=3 * 33 + 2 * N + 1, action_dim=A, shared_params=False)
torch.manual_seed(0)
model = learner.MATD3(convert(a)).cuda()
with torch.no_grad():
    for p in list(model.policy_dicts.parameters()) + list(model.value_dicts.parameters()):
        p.mul_(3.0).add_(0.05 * torch.randn_like(p))
params = list(model.value_dicts.parameters())
assert all(c.fc1.in_features == 746 for c in model.value_dicts)

res = {"n_agents": N, "obs_dim": OBS, "act_dim": A, "fc1_columns": 746, "device": torch.cuda.get_device_name(0),
       "library": build.built_digest()[:16]}
for rows in SIZES:
    b = rows // N
    obs = 0.5 * torch.randn(b, N, OBS, device=dev)
    act = 0.5 * torch.randn(b, N, A, device=dev)
    target = torch.randn(2 * b, N, 1, device=dev)
    proj = torch.randn(b, N, 1, device=dev) / rows

    def value(fused):
        model.fused_inference = fused
        with torch.no_grad():
            return model.value(obs, act)

    def loss(fused):
        model.fused_inference = fused
        v = model.value(obs, act)
        return torch.autograd.grad((v - target).pow(2).mean(), params)

    def policy(fused):
        model.fused_inference = fused
        act_g = act.detach().requires_grad_()
        v = model.value(obs, act_g, critic_frozen=True, first_head_only=True)
        return torch.autograd.grad((v * proj).sum(), act_g)

    v1, v0 = value(True), value(False)
    g1, g0 = loss(True), loss(False)
    d1, d0 = policy(True)[0], policy(False)[0]
    res[f"rows_{rows}"] = {
        "value_no_grad": pair(lambda: value(True), lambda: value(False)),
        "value_loss_forward_backward": pair(lambda: loss(True), lambda: loss(False)),
        "policy_pass_forward_backward": pair(lambda: policy(True), lambda: policy(False)),
        "max_abs_difference_of_the_values": float((v1 - v0).abs().max()),
        "max_rel_difference_of_the_value_gradients": max(float((x - y).abs().max() / y.abs().max().clamp_min(1e-30))
                                                         for x, y in zip(g1, g0)),
        # (a sample with a unit within rounding of ReLU's edge takes another mask in another summation order: counted, not
        # averaged away — the fp64 composition disagrees with both forms on such samples alike)
        "samples_whose_action_gradient_differs_by_1e-4_of_the_largest_entry":
            int(((d1 - d0).abs().amax(dim=(1, 2)) > 1e-4 * d0.abs().max()).sum()),
        "median_rel_difference_of_the_action_gradient": float(((d1 - d0).abs().amax(dim=(1, 2)) / d0.abs().max()).median()),
    }
    model.fused_inference = True
res["dispatch"] = {k: all(res[f"rows_{rows}"][k]["fused_us"][0] <= res[f"rows_{rows}"][k]["torch_us"][0] for rows in SIZES)
                   for k in ("value_no_grad", "value_loss_forward_backward", "policy_pass_forward_backward")}
res["fallbacks"] = dict(FALLBACKS)
print(json.dumps(res))
