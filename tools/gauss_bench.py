"""The log-std head of the Gaussian actors (csrc/gauss.hip) at update size — 163 840 rows x 64 hidden units, act_dim 4 —
and PPO's per-row policy loss at 32 768 samples x 5 agents, each against the eager fp32 PyTorch composition it replaces,
run in the same process on the same tensors in alternating windows: head forward, head forward + backward (with the
weight / bias gradients of csrc/wgrad.hip), loss forward + backward.  HIP-event timed after warm-up, median and min..max of
repeated windows; the head's HBM traffic over its time is quoted against the bytes the algorithm needs.  Then the pieces of
the head's forward + backward each on its own (`pieces_us`), and the same forward + backward replayed as a captured HIP
graph (`head_forward_backward_graph_us`: what is left of the eager call without its host side).  Optionally
(--train) the training rate of examples/train_maddpg.py --alg ippo --gaussian-policy next to the fixed-std one.  Prints one
JSON line."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import safe_marl_amd  # noqa: F401
from safe_marl_amd import nets

ROWS = int(os.environ.get("GAUSS_BENCH_ROWS", "163840"))
N, A, HID = 5, 4, 64
LO, HI = 0.0, 0.5
ENVS = int(os.environ.get("GAUSS_BENCH_ENVS", "4096"))
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


h = (0.5 * torch.randn(ROWS, HID, device=dev)).requires_grad_()
w = (0.1 * torch.randn(A, HID, device=dev)).requires_grad_()
b = (0.1 * torch.randn(A, device=dev)).requires_grad_()
d_ls = torch.randn(ROWS, A, device=dev)
res = {"rows": ROWS, "act_dim": A, "hid": HID}


def head(fused, backward):
    ls = nets._GaussHeadFn.apply(h, w, b, LO, HI) if fused else nets.gauss_log_std_torch(h, w, b, LO, HI)
    if backward:
        return torch.autograd.grad(ls, (h, w, b), d_ls)


# the forward as the update pass runs it, t = tanh(u) saved for the backward (without a graph the node skips that store)
with torch.no_grad():
    res["head_forward"] = pair(lambda: nets.gauss_head_forward(h, w, b, LO, HI), lambda: head(False, False))
res["head_forward_backward"] = pair(lambda: head(True, True), lambda: head(False, True))
# what the algorithm moves: forward reads h, writes log_std and t; backward reads d_log_std and t, writes d_u and d_h, and
# the weight gradient reads d_u and h again
fwd_bytes = 4 * ROWS * (HID + 2 * A)
bwd_bytes = 4 * ROWS * (2 * A + A + HID) + 4 * ROWS * (A + HID)
res["head_forward_MB"], res["head_forward_backward_MB"] = round(fwd_bytes / 1e6, 1), round((fwd_bytes + bwd_bytes) / 1e6, 1)
res["head_forward_GBps"] = round(fwd_bytes / res["head_forward"]["fused_us"][0] / 1e3, 1)
res["head_forward_backward_GBps"] = round((fwd_bytes + bwd_bytes) / res["head_forward_backward"]["fused_us"][0] / 1e3, 1)

# the pieces, each alone: [median, min, max] us
with torch.no_grad():
    hd, wd = h.detach(), w.detach()
    _, t_saved = nets.gauss_head_forward(hd, wd, b, LO, HI)
    d_u, _ = nets.gauss_head_backward(d_ls, t_saved, wd, LO, HI)
    db = torch.empty(A, device=dev)
    mu, noise = torch.randn(ROWS, A, device=dev), torch.randn(ROWS, A, device=dev)
    stat = lambda x: [round(float(np.median(x)), 1), round(min(x), 1), round(max(x), 1)]
    res["pieces_us"] = {
        "head_forward_kernel": stat(timed(lambda: nets.gauss_head_forward(hd, wd, b, LO, HI), n=50, windows=7)),
        "head_forward_kernel_with_epilogue": stat(timed(lambda: nets.gauss_head_forward(hd, wd, b, LO, HI, means=mu, noise=noise),
                                                        n=50, windows=7)),
        "head_backward_kernel": stat(timed(lambda: nets.gauss_head_backward(d_ls, t_saved, wd, LO, HI), n=50, windows=7)),
        "tall_wgrad_du_h": stat(timed(lambda: nets.tall_wgrad(d_u, hd, colsum=db), n=50, windows=7)),
        "torch_dW_gemm": stat(timed(lambda: d_u.t() @ hd, n=50, windows=7))}

B = ROWS // N
means = (0.3 * torch.randn(B, N, A, device=dev)).requires_grad_()
log_stds = (0.05 * torch.randn(B, N, A, device=dev) + 0.05).requires_grad_()
act = torch.tanh(torch.randn(B, 1, A, device=dev)).expand(B, N, A).contiguous()
adv = torch.randn(B, N, device=dev)
avail = torch.ones(1, 1, 1, device=dev).expand(B, N, A)
avail._flex_const = 1.0


def pol(fused):
    loss, _ = nets.ppo_policy_loss(means, log_stds, act, None, adv, 0.6, avail, fused=fused)
    torch.autograd.grad(loss, [means, log_stds])


res["ppo_policy_loss_rows_fwd_bwd"] = pair(lambda: pol(True), lambda: pol(False))
res["ppo_samples"] = B

# the fused forward + backward as a captured graph: the device side of the eager call
try:
    from safe_marl_amd.util import graph_capture
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            head(True, True)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with graph_capture(graph):
        kept = head(True, True)
    res["head_forward_backward_graph_us"] = stat(timed(graph.replay, n=50, windows=7))
    res["head_forward_backward_graph_GBps"] = round((fwd_bytes + bwd_bytes) / res["head_forward_backward_graph_us"][0] / 1e3, 1)
except Exception as exc:                          # reported, not hidden: the figure is then absent from the result
    res["head_forward_backward_graph_us"] = f"capture failed: {exc!r}"

if "--train" in sys.argv:
    for label, extra in (("gaussian", ["--gaussian-policy"]), ("fixed_std", [])):
        out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "train_maddpg.py"), "--alg", "ippo", "--envs",
                              str(ENVS), "--episodes", "10"] + extra, capture_output=True, text=True, timeout=900, cwd=ROOT)
        line = [l for l in out.stdout.splitlines() if l.startswith("{")]
        if line:
            r = json.loads(line[-1])
            res[f"train_ippo_{label}_env_steps_per_s"] = round(r["value"])
            res[f"train_ippo_{label}_fallbacks"] = r["fallbacks"]
        else:
            res[f"train_ippo_{label}_env_steps_per_s"] = out.stderr[-400:]
print(json.dumps(res))
