"""MAAC's attention critic fused in HIP (csrc/attn_critic.hip: nets.fused_attn_critic_forward, nets._AttnCriticFn) against the
tensor composition it replaces (nets.AttentionCritic's own forward) in ONE process on one GPU, on the same tensors, alternating:
5 agents, obs_dim 144, act_dim 4 at 32 768 and 131 072 samples.  Three call classes, as ``learner.MAAC.get_loss`` makes them:
``value()`` under no_grad (the TD target's critic), the value loss forward + backward with every critic parameter gradient, the
policy loss forward + backward with the action gradient alone (critic frozen).  Every call is timed by its own pair of HIP
events after warm-up; median, min and max over the timed calls.  A call class passes when the fused median beats the
composition's by more than the composition's own spread (max - min) — DESIGN.md §4.6f's rule.  All eager: nothing here captures a
HIP graph.  Prints one JSON line."""
import json
import os
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import safe_marl_amd  # noqa: F401
from safe_marl_amd import build, nets
from safe_marl_amd.util import FALLBACKS

N, OBS, A = 5, 144, 4
SIZES = [int(s) for s in os.environ.get("MAAC_BENCH_SAMPLES", "32768,131072").split(",")]
CALLS = int(os.environ.get("MAAC_BENCH_CALLS", "16"))
# per sample: 2 n encoders (2 * 64 * (148 + 144)), K, Q, V per agent (3 * 2 * 64 * 64), critic fc1 (2 * 64 * 128) and bias fc1
# (2 * 64 * 64) per agent: 0.43 Mflop at n = 5 -> 14 GFLOP at 32 768 samples, 90 us at the 157 TFLOP/s fp32 matrix peak
FLOP_PER_SAMPLE = N * (2 * 64 * (OBS + A) + 2 * 64 * OBS + 3 * 2 * 64 * 64 + 2 * 64 * 128 + 2 * 64 * 64)
PEAK_FP32_MATRIX = 157.3e12
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
    for _ in range(3):
        fused()
        plain()
    f, p = [], []
    for _ in range(2):
        f += timed(fused, CALLS // 2)
        p += timed(plain, CALLS // 2)
    sf, sp = stat(f), stat(p)
    spread = sp["max"] - sp["min"]
    return {"fused_us": sf, "composition_us": sp, "speedup_of_medians": round(sp["median"] / sf["median"], 2),
            "composition_spread_us": round(spread, 1), "fused_wins_by_more_than_the_spread": sp["median"] - sf["median"] > spread}


if __name__ == "__main__":
    args = types.SimpleNamespace(hid_size=64, attend_heads=1, agent_num=N, obs_size=OBS, action_dim=A, continuous=True, norm_in=False)
    torch.manual_seed(0)
    critic = nets.AttentionCritic(args).cuda()
    with torch.no_grad():
        for p in critic.parameters():
            p.copy_(0.2 * torch.randn_like(p))
    params = list(critic.parameters())
    res = {"n_agents": N, "obs_dim": OBS, "act_dim": A, "device": torch.cuda.get_device_name(0), "library": build.built_digest()[:16],
           "kernels": {v["name"]: {k: v[k] for k in ("vgprs", "agprs", "lds_bytes_per_block", "waves_per_simd")}
                       for v in build.kernel_resources("attn_critic").values()}}
    for b in SIZES:
        obs = 0.5 * torch.randn(b, N, OBS, device=dev)
        act = torch.tanh(torch.randn(b, N, A, device=dev))
        up = torch.randn(b, N, device=dev) / b

        def value(fused):
            with torch.no_grad():
                return nets.fused_attn_critic_forward(critic, obs, act) if fused else critic(obs, act)

        def value_loss(fused):
            q, _ = nets.attn_critic_train(critic, obs, act, param_grads=True) if fused else critic(obs, act)
            return torch.autograd.grad((q * up).sum(), params)

        def policy_loss(fused):
            a = act.detach().requires_grad_()
            q, _ = nets.attn_critic_train(critic, obs, a, param_grads=False) if fused else critic(obs, a)
            return torch.autograd.grad((q * up).sum(), a)

        q1, q0 = value(True), value(False)
        g1, g0 = value_loss(True), value_loss(False)
        a1, a0 = policy_loss(True), policy_loss(False)
        r = {"value_no_grad": pair(lambda: value(True), lambda: value(False)),
             "value_loss_forward_backward": pair(lambda: value_loss(True), lambda: value_loss(False)),
             "policy_loss_forward_backward": pair(lambda: policy_loss(True), lambda: policy_loss(False)),
             "max_abs_difference_of_q": float((q1[0] - q0[0]).abs().max()),
             "max_rel_difference_of_the_regulariser": float(((q1[1] - q0[1]).abs() / q0[1].abs()).max()),
             "max_rel_difference_of_the_parameter_gradients": max(float((x - y).abs().max() / y.abs().max().clamp_min(1e-30))
                                                                  for x, y in zip(g1, g0)),
             "max_rel_difference_of_d_act": float((a1[0] - a0[0]).abs().max() / a0[0].abs().max())}
        floor = FLOP_PER_SAMPLE * b / PEAK_FP32_MATRIX * 1e6
        r["derived_floor_us"] = round(floor, 1)
        r["value_no_grad_over_floor"] = round(r["value_no_grad"]["fused_us"]["median"] / floor, 2)
        res[f"samples_{b}"] = r
    res["fallbacks"] = dict(FALLBACKS)
    print(json.dumps(res))
