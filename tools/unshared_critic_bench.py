"""The per-agent critics of ``shared_params: False`` (csrc/critic_unshared.hip, flexnet_wgrad_batched) against the module
composition they replace — the per-agent loops of MADDPG.value and Model.row_values with ``model.fused_inference = False`` — in
ONE process on one GPU, on the same tensors, in alternating windows: 5 agents at 20 480 and 163 840 critic rows, for the MADDPG
input form ([o_1 .. o_n | onehot(i) | a_1 .. a_n], 745 columns) and the IPPO form ([o_i | onehot(i)], 149 columns): ``value()``
under no_grad, and a value loss forward + backward with every parameter gradient.  Then the actor node of
tools/unshared_bench.py again (forward + backward, its 4 n weight gradients now one flexnet_wgrad_batched call).  HIP-event
timed after warm-up, median and min..max of repeated windows.  Prints one JSON line."""
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
from train_maddpg import DEFAULT_ALG_ARGS, PPO_ALG_ARGS

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


def model_of(alg):
    a = dict(DEFAULT_ALG_ARGS)
    if alg == "ippo":
        a.update(PPO_ALG_ARGS)
    a.update(alg=alg, agent_num=N, obs_size=OBS, state_size=3 * 33 + 2 * N + 1, action_dim=A, shared_params=False)
    torch.manual_seed(0)
    m = {"maddpg": learner.MADDPG, "ippo": learner.IPPO}[alg](convert(a)).cuda()
    with torch.no_grad():
        for p in list(m.policy_dicts.parameters()) + list(m.value_dicts.parameters()):
            p.mul_(3.0).add_(0.05 * torch.randn_like(p))
    return m


res = {"n_agents": N, "obs_dim": OBS, "act_dim": A, "device": torch.cuda.get_device_name(0), "library": build.built_digest()[:16]}
models = {alg: model_of(alg) for alg in ("maddpg", "ippo")}
for rows in SIZES:
    b = rows // N
    obs = 0.5 * torch.randn(b, N, OBS, device=dev)
    act = 0.5 * torch.randn(b, N, A, device=dev)
    hid = 0.5 * torch.randn(b, N, 64, device=dev)
    target = torch.randn(b, N, 1, device=dev)
    proj = torch.randn(b, N, A, device=dev) / rows
    r = {}
    for alg, model in models.items():
        params = list(model.value_dicts.parameters())

        def value(fused, model=model):
            model.fused_inference = fused
            with torch.no_grad():
                return model.value(obs, act)

        def loss(fused, model=model, params=params):
            model.fused_inference = fused
            v = model.value(obs, act)
            return torch.autograd.grad((v - target).pow(2).mean(), params)

        with torch.no_grad():
            model.fused_inference = True
            v1 = model.value(obs, act)
            model.fused_inference = False
            v0 = model.value(obs, act)
        r[alg] = {"value_no_grad": pair(lambda: value(True), lambda: value(False)),
                  "value_loss_forward_backward": pair(lambda: loss(True), lambda: loss(False)),
                  "max_abs_difference_of_the_values": float((v1 - v0).abs().max())}
        model.fused_inference = True
    actor = models["maddpg"]
    aparams = list(actor.policy_dicts.parameters())

    def actor_train(fused):
        actor.fused_inference = fused
        means, _, _ = actor.policy(obs, last_hid=hid)
        return torch.autograd.grad((means * proj).sum(), aparams)

    r["actor_train_forward_backward"] = pair(lambda: actor_train(True), lambda: actor_train(False))
    actor.fused_inference = True
    means, _, _ = actor.policy(obs, last_hid=hid)
    aloss = (means * proj).sum()
    r["actor_node_backward_only_us"] = stat(timed(lambda: torch.autograd.grad(aloss, aparams, retain_graph=True), windows=6))
    res[f"rows_{rows}"] = r
res["fallbacks"] = dict(FALLBACKS)
print(json.dumps(res))
