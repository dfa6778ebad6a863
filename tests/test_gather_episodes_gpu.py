"""GPU: flexnet_gather_episodes (csrc/episodes.hip) on hand-filled rings, bit-equal to the composition of ``slab_window`` rows
it replaces, at the smallest shapes at which it can go wrong: (N 5, n 3, history 4, ring of 9 + 3 slabs: rows of 72 floats)
and (N 4, n 5, history 24, ring of 30 + 23 slabs: the reference's history), the stacked-observation ring without a history, with and without the filed columns; episodes of length 1, an episode whose first step is the stream's
first slab (all padding), histories that reach across the ring's seam, episodes that end on the last written slab (next_state
and hid from the slab at the cursor), two episodes of one environment back to back, a batch of a single episode, batches whose
rows are no multiple of 32 or of the rows a block owns; guard values around every output tensor stay untouched."""
import functools

import numpy as np
import pytest
import torch as th

from .test_episodic_cpu import _hand_filled_ring

pytestmark = pytest.mark.gpu

SHAPES = {"h4": dict(N=5, n=3, history=4, transitions=9), "h24": dict(N=4, n=5, history=24, transitions=30),
          "stacked": dict(N=5, n=3, history=None, transitions=9)}
GUARD = 64                                         # floats on either side of every output tensor
SENTINEL = -12345.5


@functools.lru_cache(maxsize=None)
def ring(shape, filed, first_stream=False):
    """(buffer, {(step counter, environment): the Transition slab_window hands out for that one transition}) — the reference
    is computed once per ring and shared."""
    buf, block = _hand_filled_ring("cuda", filed=filed, first_stream=first_stream, **SHAPES[shape])
    ref = {}
    for c in range(buf.k - block, buf.k):
        for e in range(buf.n_envs):
            ref[(c, e)] = buf.slab_window(c * buf.n_envs + e, 1)
    return buf, ref


def gather_guarded(buf, ids):
    """The kernel's batch for the episodes ``ids``, written between guard bands; returns (Transition, rows)."""
    table = buf.episode_table(ids)
    rows = int(table[:, 2].sum())
    n = buf.n_agents
    shapes = {"state": (n, buf.obs_dim), "next_state": (n, buf.obs_dim), "last_hid": (n, buf.hid_dim), "hid": (n, buf.hid_dim),
              "action": (n, buf.act_dim), "reward": (n,), "done": (), "last_step": ()}
    for k in buf.filed:
        shapes[k] = tuple(buf.const_shapes[k])
    padded, out = {}, {}
    for k, s in shapes.items():
        count = rows * int(np.prod(s)) if s else rows
        padded[k] = th.full((count + 2 * GUARD,), SENTINEL, device="cuda")
        out[k] = padded[k][GUARD:GUARD + count].view((rows,) + s)
    batch = buf._gather_slabs(table, out=out)
    assert batch is not None
    th.cuda.synchronize()
    for k, p in padded.items():
        assert bool((p[:GUARD] == SENTINEL).all()) and bool((p[-GUARD:] == SENTINEL).all()), k
        assert not bool((p[GUARD:-GUARD] == SENTINEL).any()), k               # ... and every element inside was written
    return batch, rows


def assert_rows(buf, ref, batch, ids):
    from safe_marl_amd.replay_buffer import FIELDS
    row = 0
    for i in ids:
        c0, e, length = buf.episodes[i]
        for j in range(length):
            w = ref[(c0 + j, e)]
            for k in FIELDS:
                got, want = getattr(batch, k)[row], getattr(w, k)[0]
                assert got.shape == want.shape and th.equal(got, want), (k, i, j, row)
            row += 1
    assert row == batch.reward.shape[0]


def _cases(buf):
    eps = buf.episodes
    by_env = {}
    for i, (c0, e, length) in enumerate(eps):
        by_env.setdefault(e, []).append(i)
    rng = np.random.RandomState(1)
    everything = [int(i) for i in rng.permutation(len(eps))]
    longest = max(range(len(eps)), key=lambda i: eps[i][2])
    ones = [i for i, ep in enumerate(eps) if ep[2] == 1]
    pair = next(v[:2] for v in by_env.values() if len(v) >= 2)
    assert eps[pair[0]][0] + eps[pair[0]][2] == eps[pair[1]][0]               # back to back
    odd = list(everything)
    while sum(eps[i][2] for i in odd) % 4 == 0 or sum(eps[i][2] for i in odd) % 32 == 0:
        odd.pop()
    at_cursor = [i for i, ep in enumerate(eps) if ep[0] + ep[2] == buf.k]
    assert ones and len(at_cursor) == buf.n_envs
    return {"everything": everything, "single": [longest], "length one": ones, "back to back": pair, "reversed pair": pair[::-1],
            "odd rows": odd, "ends at the cursor": at_cursor}


@pytest.mark.parametrize("filed", [False, True])
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_bit_equal_to_the_slab_window_composition(shape, filed):
    from safe_marl_amd.util import FALLBACKS
    declined = FALLBACKS.get("gather_episodes", 0)
    buf, ref = ring(shape, filed)
    assert buf.k > buf.slabs                                                    # the block lies across the ring's seam
    assert (buf.history or 0) == (SHAPES[shape]["history"] or 0) and bool(buf.filed) == filed
    for name, ids in _cases(buf).items():
        batch, rows = gather_guarded(buf, ids)
        assert rows == sum(buf.episodes[i][2] for i in ids), name
        assert_rows(buf, ref, batch, ids)
        comp = buf._compose_slabs(buf.episode_table(ids))                        # the fallback: the same bits
        for k in batch._fields:
            assert th.equal(getattr(batch, k), getattr(comp, k)), (name, k)
        assert set(buf.filed) <= set(batch._fields) and all(not hasattr(getattr(batch, k), "_flex_const") for k in buf.filed)
    # the product path: a draw, one launch, the drawn order
    np.random.seed(7)
    batch = buf.get_batch_tensors(5)
    assert_rows(buf, ref, batch, buf.last_draw)
    assert batch.action_avail.shape == (batch.reward.shape[0], buf.n_agents, buf.act_dim)
    assert getattr(batch.action_avail, "_flex_const", None) == 1.0
    assert FALLBACKS.get("gather_episodes", 0) == declined


@pytest.mark.parametrize("shape", ["h4", "h24"])
def test_an_episode_from_the_streams_first_slab_is_all_padding(shape):
    buf, ref = ring(shape, False, True)
    assert buf.k < buf.slabs
    first = [i for i, ep in enumerate(buf.episodes) if ep[0] == 0]
    assert len(first) == buf.n_envs
    batch, _ = gather_guarded(buf, first)
    assert_rows(buf, ref, batch, first)
    row = 0
    for i in first:                                                             # step 0: only the newest feature row is there
        s = batch.state[row].view(buf.n_agents, buf.history, 6)
        assert bool((s[:, :-1] == 0).all()) and bool((s[:, -1] != 0).any())
        row += buf.episodes[i][2]


def test_unaligned_outputs_take_the_narrow_stores():
    """state / next_state that are 8- but not 16-byte aligned: the kernel's 8-byte form; hidden-state outputs off their 16-byte
    alignment: the field-by-field copies instead of the loads issued up front.  Same bits."""
    buf, ref = ring("h4", False)
    ids = _cases(buf)["everything"]
    table = buf.episode_table(ids)
    rows = int(table[:, 2].sum())
    n = buf.n_agents
    base = {k: th.full((rows * n * buf.obs_dim + 2,), SENTINEL, device="cuda") for k in ("state", "next_state")}
    out = {k: v[2:].view(rows, n, buf.obs_dim) for k, v in base.items()}
    assert out["state"].data_ptr() % 16 == 8
    hbase = {k: th.full((rows * n * buf.hid_dim + 1,), SENTINEL, device="cuda") for k in ("last_hid", "hid")}
    out.update({k: v[1:].view(rows, n, buf.hid_dim) for k, v in hbase.items()})
    assert out["hid"].data_ptr() % 16 == 4
    out.update(action=th.empty(rows, n, buf.act_dim, device="cuda"), reward=th.empty(rows, n, device="cuda"),
               done=th.empty(rows, device="cuda"), last_step=th.empty(rows, device="cuda"))
    batch = buf._gather_slabs(table, out=out)
    assert_rows(buf, ref, batch, ids)
    assert all(float(v[0]) == SENTINEL and float(v[1]) == SENTINEL for v in base.values())
    assert all(float(v[0]) == SENTINEL for v in hbase.values())
