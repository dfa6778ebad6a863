"""The per-agent MLP and Gaussian actors of ``shared_params: False`` (csrc/actor_mlp.hip's per-agent form, csrc/gauss.hip's per-agent heads,
csrc/actor_unshared.hip's d_hn variant) against the per-agent module loop they replace — ``Model.policy`` with
``model.fused_inference = False`` — in ONE process on one GPU, on the same tensors, alternating: 5 agents, obs_dim 144, act_dim 4
at 20 480 and 163 840 actor rows, for the MLP, the MLP-Gaussian and the RNN-Gaussian agents: ``policy()`` under no_grad, and
forward + backward with every parameter gradient.  Every call is timed by its own pair of HIP events after warm-up; median, min
and max over the timed calls.  A call class (inference or training, at a size) passes the default rule of DESIGN.md §4.6f when
the fused median beats the loop's by more than the loop's own spread (max - min).  All eager: nothing here captures a HIP graph.
Prints one JSON line."""
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
SIZES = [int(s) for s in os.environ.get("UNSHARED_AGENTS_BENCH_ROWS", "20480,163840").split(",")]
CALLS = int(os.environ.get("UNSHARED_AGENTS_BENCH_CALLS", "24"))
AGENTS = {"mlp": ("mlp", False), "mlp_gaussian": ("mlp", True), "rnn_gaussian": ("rnn", True)}
dev = "cuda"


def timed(fn, calls):
    """Microseconds of ``calls`` calls, each between its own events (the queue is empty before each)."""
    out = []
    for _ in range(calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) * 1e3)
    return out


def stat(x):
    return {"median": round(float(np.median(x)), 1), "min": round(min(x), 1), "max": round(max(x), 1), "calls": len(x)}


def pair(fused, plain):
    """Both forms after warm-up, in alternating halves."""
    for _ in range(5):
        fused()
        plain()
    f, p = [], []
    for _ in range(2):
        f += timed(fused, CALLS // 2)
        p += timed(plain, CALLS // 2)
    sf, sp = stat(f), stat(p)
    spread = sp["max"] - sp["min"]
    return {"fused_us": sf, "loop_us": sp, "speedup_of_medians": round(sp["median"] / sf["median"], 2),
            "loop_spread_us": round(spread, 1), "fused_wins_by_more_than_the_spread": sp["median"] - sf["median"] > spread}


def model_of(agent_type, gaussian):
    a = dict(DEFAULT_ALG_ARGS)
    a.update(PPO_ALG_ARGS)
    a.update(alg="ippo", agent_num=N, obs_size=OBS, state_size=3 * 33 + 2 * N + 1, action_dim=A, agent_type=agent_type,
             gaussian_policy=gaussian, shared_params=False)
    torch.manual_seed(0)
    m = learner.IPPO(convert(a)).cuda()
    with torch.no_grad():
        for p in m.policy_dicts.parameters():
            p.mul_(3.0).add_(0.05 * torch.randn_like(p))
    return m


if __name__ == "__main__":
    kernels = {}
    for prefix in ("mlp_unshared_actor", "gauss_head_unshared", "actor_hn_unshared", "actor_unshared"):
        kernels.update({v["name"]: {k: v[k] for k in ("vgprs", "agprs", "lds_bytes_per_block", "waves_per_simd")}
                        for v in build.kernel_resources(prefix).values()})
    res = {"n_agents": N, "obs_dim": OBS, "act_dim": A, "device": torch.cuda.get_device_name(0), "library": build.built_digest()[:16],
           "kernels": kernels}
    models = {name: model_of(*spec) for name, spec in AGENTS.items()}
    for rows in SIZES:
        b = rows // N
        obs = 0.5 * torch.randn(b, N, OBS, device=dev)
        hid = 0.5 * torch.randn(b, N, 64, device=dev)
        proj = torch.randn(b, N, A, device=dev) / rows
        r = {}
        for name, model in models.items():
            params = list(model.policy_dicts.parameters())
            gaussian = AGENTS[name][1]

            def infer(fused, model=model):
                model.fused_inference = fused
                with torch.no_grad():
                    return model.policy(obs, last_hid=hid)

            def train(fused, model=model, params=params, gaussian=gaussian):
                model.fused_inference = fused
                means, log_stds, _ = model.policy(obs, last_hid=hid)
                loss = (means * proj).sum()
                if gaussian:
                    loss = loss + (log_stds * proj).sum()
                return torch.autograd.grad(loss, params)

            m1, m0 = infer(True)[0], infer(False)[0]
            g1, g0 = train(True), train(False)
            r[name] = {"policy_no_grad": pair(lambda: infer(True), lambda: infer(False)),
                       "forward_backward": pair(lambda: train(True), lambda: train(False)),
                       "max_abs_difference_of_the_means": float((m1 - m0).abs().max()),
                       "max_rel_difference_of_the_gradients": max(float((x - y).abs().max() / y.abs().max().clamp_min(1e-30))
                                                                  for x, y in zip(g1, g0))}
            model.fused_inference = True
        res[f"rows_{rows}"] = r
    res["fallbacks"] = dict(FALLBACKS)
    print(json.dumps(res))
