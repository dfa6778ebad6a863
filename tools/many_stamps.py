"""Where a step of flex_step_many_kernel's loop spends its cycles, from a DIAGNOSTIC build (-DFLEX_MANY_STAMPS): s_memtime
stamps that do NOT drain the vector-memory counter (tools/stamps.py's do: made for the one-step kernel, they would serialise
the overlaps the loop is built for).  Four segments per step — loop top -> solve start, the solve, solve end -> last
instruction of the epilogue, the fence — for step 0 of a launch and summed over the steps behind it, per wavefront.

Build:  mkdir -p tools/variants      (git-ignored; the diagnostic library is never committed)
        hipcc -O3 --offload-arch=gfx950 -std=c++17 -shared -fPIC -DFLEX_MANY_STAMPS [-DFLEX_MANY_PREFETCH_ACT=0 ...] \\
            -Iinclude -Isafe-marl_amd/csrc -o tools/variants/libflexenv_hip_stamps_many.so safe-marl_amd/csrc/*.hip
Run:    FLEX_STAMPS_LIB=tools/variants/libflexenv_hip_stamps_many.so python tools/many_stamps.py [--steps 20] [--envs 4096]
Read the SHARES, never the run time of this build (each stamp waits for the scalar-memory counter)."""
import argparse
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warm", type=int, default=3, help="launches before the recorded one")
    a = ap.parse_args()
    import numpy as np
    import torch
    import safe_marl_amd  # noqa: F401
    from safe_marl_amd import _lib
    _lib.LIB_PATH = os.path.abspath(os.environ.get("FLEX_STAMPS_LIB", "tools/variants/libflexenv_hip_stamps_many.so"))
    from safe_marl_amd.network import create_network
    from safe_marl_amd.series import make_synthetic_series
    from safe_marl_amd.flex_env import VecFlexProvisionEnv

    net = create_network()
    series = make_synthetic_series(net)
    gen = torch.Generator(device="cuda").manual_seed(99)
    pool = (0.5 + 0.5 * torch.rand(16, a.envs, 5, 4, device="cuda", generator=gen)).float()
    env = VecFlexProvisionEnv({}, a.envs, device="cuda:0", net=net, series=series, seed=1234, warm_start=True)
    env.reset()
    lib = _lib.load()
    for _ in range(a.warm):
        env.step_many(pool, steps=a.steps, auto_reset=True)
    stamps = torch.zeros(a.envs, 16, dtype=torch.int64, device="cuda")
    lib.flexenv_debug_set_stamps.argtypes = [C.c_void_p]
    lib.flexenv_debug_set_stamps(C.c_void_p(stamps.data_ptr()))
    env.step_many(pool, steps=a.steps, auto_reset=True)
    torch.cuda.synchronize()
    lib.flexenv_debug_set_stamps(None)
    st = stamps.cpu().numpy().astype(np.float64)
    st = st[st[:, 8] != 0]              # lane 0 of a wavefront writes the row of its first environment (one or two envs each)
    assert len(st) and (st[:, 8] == a.steps).all(), "not a -DFLEX_MANY_STAMPS build"
    names = ["top->solve", "solve", "epilogue", "fence"]
    rest = max(1, a.steps - 1)
    print(f"{a.envs} envs, one launch of {a.steps} steps; cycles per wavefront (mean / median / max over {len(st)} wavefronts)")
    print("step 0:")
    for i, nm in enumerate(names):
        print(f"  {nm:11s} {st[:, i].mean():9.1f} {np.median(st[:, i]):9.1f} {st[:, i].max():9.1f}")
    print(f"steps 1..{a.steps - 1}, per step:")
    for i, nm in enumerate(names):
        d = st[:, 4 + i] / rest
        print(f"  {nm:11s} {d.mean():9.1f} {np.median(d):9.1f} {d.max():9.1f}")
    tot = st[:, 9]
    print(f"whole loop: {tot.mean():.0f} cycles per wavefront = {tot.mean() / a.steps:.0f} per step; "
          f"outside the solve {(st[:, 4] + st[:, 6] + st[:, 7]).mean() / rest:.0f} per step behind the first")


if __name__ == "__main__":
    main()
