#!/usr/bin/env python3
"""Episodic batch gather, kernel against tensor composition: one process, after warm-up, the median of ``--runs`` (>= 10)
runs each, device events.

    python tools/episodic_bench.py [--envs 4096] [--episodes 344] [--runs 10] [--out profiles/episodic_bench.txt]

One block of ``--envs`` environments x 5 agents x 95 steps in a row-mode slab ring (history 24, hand-filled: the gather does
not care what the numbers are), every environment one episode of 95 steps, and a batch of ``--episodes`` episodes drawn
without replacement (344 x 95 = 32 680 rows, the default transition batch's size).  Timed, on the same table of episodes:
  flexnet_gather_episodes        EpisodeReplayBuffer._gather_slabs: the table's upload and ONE launch into allocated tensors,
                                 and the launch alone with the table already on the device
  tensor composition             EpisodeReplayBuffer._compose_slabs: index tensors, index_select on the rings and the
                                 stacked-observation im2col (what runs where the kernel declines)
  get_batch product path         episodes_batch with and without the kernel (allocation of the outputs included)
and the kernel's share of the HBM peak (8.0 TB/s) on the bytes it must read plus the bytes it writes.  The two results are
compared bit for bit before anything is timed."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--episodes", type=int, default=344)
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.runs < 10:
        ap.error("--runs: at least ten")

    import numpy as np
    import torch
    import safe_marl_amd  # noqa: F401
    from safe_marl_amd.replay_buffer import EpisodeReplayBuffer

    lines = []

    def say(line):
        print(line, flush=True)
        lines.append(line)

    def timed(fn):
        fn()
        fn()                                                            # warm-up: allocations, first launches
        torch.cuda.synchronize()
        ts = []
        for _ in range(a.runs):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1) * 1e3)
        return statistics.median(ts), min(ts), max(ts)

    N, n, H, steps, act, hid = a.envs, 5, 24, 95, 4, 64
    buf = EpisodeReplayBuffer(1, device="cuda")
    buf.configure_blocks(N, steps)
    buf.alloc_slabs(N, n, 6 * H, act, hid, history=H)
    g = torch.Generator(device="cuda").manual_seed(1)
    for ring in (buf.row_ring, buf.hid_ring, buf.small_ring):
        ring.copy_(torch.randn(ring.shape, generator=g, device="cuda"))
    col = n * act + n
    buf.begin_stream(torch.randn(N, n, 6 * H, generator=g, device="cuda"))
    for c in range(steps + 1):
        p = c % buf.slabs
        buf.row_ring[p].view(N, n, 8)[:, :, 6] = float(c)               # `older`: steps since the episode began
        if c < steps:
            buf.small_ring[p, :, col] = 0.0
            buf.small_ring[p, :, col + 1] = 1.0 if c == steps - 1 else 0.0
            buf.stepped()
    buf.end_block(steps)
    assert len(buf.buffer) == N and all(length == steps for _, _, length in buf.episodes)
    np.random.seed(5)
    ids = buf.draw(a.episodes)
    table = buf.episode_table(ids)
    rows = int(table[:, 2].sum())
    say(f"# episodic_bench: one block of {N} envs x {n} agents x {steps} steps (history {H}), a batch of {a.episodes} episodes = "
        f"{rows} rows, median [min .. max] of {a.runs} runs, device events, same process")

    kernel, comp = buf._gather_slabs(table), buf._compose_slabs(table)
    assert kernel is not None, "flexnet_gather_episodes declined this shape"
    for k in kernel._fields:
        assert torch.equal(getattr(kernel, k), getattr(comp, k)), k
    say("kernel and composition: bit-equal in every field")
    out = {k: getattr(kernel, k) for k in ("state", "next_state", "last_hid", "hid", "action", "reward", "done", "last_step")}

    k_med, k_lo, k_hi = timed(lambda: buf._gather_slabs(table, out=out))
    dev_table = torch.from_numpy(table).cuda()
    l_med, l_lo, l_hi = timed(lambda: buf._gather_slabs(table, out=out, dev_table=dev_table))
    c_med, c_lo, c_hi = timed(lambda: buf._compose_slabs(table))
    written = rows * 4 * (2 * n * 6 * H + 2 * n * hid + n * act + n + 2)
    read = a.episodes * 4 * ((steps + H) * n * 8 + (steps + 1) * n * hid + steps * buf.small_w)
    say(f"flexnet_gather_episodes: {k_med:.1f} us [{k_lo:.1f} .. {k_hi:.1f}]  (table upload + one launch)")
    say(f"  the launch alone:      {l_med:.1f} us [{l_lo:.1f} .. {l_hi:.1f}]  (table already on the device)")
    say(f"tensor composition:      {c_med:.1f} us [{c_lo:.1f} .. {c_hi:.1f}]  (index tensors, index_select, im2col)")
    say(f"kernel / composition: {k_med / c_med:.3f}  (kernel's slowest run {k_hi:.1f} us against the composition's fastest {c_lo:.1f} us)")
    say(f"bytes: {written / 1e6:.1f} MB written + {read / 1e6:.1f} MB that must be read = {(written + read) / 1e6:.1f} MB; "
        f"the launch alone moves them at {(written + read) / (l_med * 1e-6) / 1e12:.2f} TB/s = "
        f"{100 * (written + read) / (l_med * 1e-6) / HBM_PEAK:.1f} % of the {HBM_PEAK / 1e12:.1f} TB/s HBM peak")
    for use in (True, False):
        buf.use_kernel = use
        med, lo, hi = timed(lambda: buf.episodes_batch(ids))
        say(f"episodes_batch, {'kernel' if use else 'composition'}: {med:.1f} us [{lo:.1f} .. {hi:.1f}]  (outputs allocated per call)")
    buf.use_kernel = True
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
