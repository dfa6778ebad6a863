"""Device-resident replay memory with the reference's TransReplayBuffer surface
(utils/replay_buffer.py:3-30: ``add_experience``, ``get_batch``, ``clear``, ``.buffer`` whose only
use is ``len()``; trainer.py:31,67 and model.py:42,44,57 are the call sites).

Storage is a ring of pre-allocated tensors, one per Transition field (model.py:19), living where the
learner runs (HBM on the GPU box).  Semantics kept from the reference:
  * FIFO with capacity ``size``: the oldest transition is dropped first (replay_buffer.py:23-27);
  * a batch is ``batch_size`` CONSECUTIVE transitions starting at
    ``np.random.choice(len - batch_size + 1, 1, replace=False)[0]`` (replay_buffer.py:17-21),
    drawn from the global NumPy RNG so that ``np.random.seed`` reproduces the reference's index sequence.
Added for the vectorised path: ``add_batch`` appends one transition per environment in a single
indexed copy, and ``get_batch_tensors`` returns the window as device tensors (no host round trip,
no per-sample Python objects).  With N envs the ring is time-major — consecutive slots are the N envs
of one vector step — so a window is a contiguous, coalesced slab.
``EpisodeReplayBuffer`` (below) is the memory of ``episodic: True`` (utils/replay_buffer.py:33-56): whole episodes, drawn
without replacement and concatenated.
"""
from __future__ import annotations

from collections import namedtuple

import numpy as np
import torch as th

Transition = namedtuple("Transition", ("state", "action", "log_prob_a", "value", "next_value", "reward",
                                       "next_state", "done", "last_step", "action_avail", "last_hid", "hid"))

FIELDS = Transition._fields


def _transition_row(trans):
    """The Transition of model.py:230-242 (numpy fields) as one row [1, ...] per field."""
    return {
        "state": np.asarray(trans.state, np.float32)[None],
        "action": np.asarray(trans.action, np.float32).reshape(1, *np.shape(trans.action)[-2:]),
        "log_prob_a": np.asarray(trans.log_prob_a, np.float32).reshape(1, *np.shape(trans.log_prob_a)[-2:]),
        "value": np.asarray(trans.value, np.float32).reshape(1, *np.shape(trans.value)[-2:]),
        "next_value": np.asarray(trans.next_value, np.float32).reshape(1, *np.shape(trans.next_value)[-2:]),
        "reward": np.asarray(trans.reward, np.float32)[None],
        "next_state": np.asarray(trans.next_state, np.float32)[None],
        "done": np.asarray([float(trans.done)], np.float32),
        "last_step": np.asarray([float(trans.last_step)], np.float32),
        "action_avail": np.asarray(trans.action_avail, np.float32).reshape(1, *np.shape(trans.action_avail)[-2:]),
        "last_hid": np.asarray(trans.last_hid, np.float32).reshape(1, *np.shape(trans.last_hid)[-2:]),
        "hid": np.asarray(trans.hid, np.float32).reshape(1, *np.shape(trans.hid)[-2:]),
    }


class _LenView:
    """What ``.buffer`` exposes: the reference only ever calls len() on it."""

    def __init__(self, owner):
        self._owner = owner

    def __len__(self):
        return self._owner.length


class DeviceReplayBuffer:
    EXACT_STREAM_MAX = 16384       # the reference's buffer holds 5000 transitions (default.yaml:23)

    def __init__(self, size, device="cpu"):
        self.size = int(size)
        self.device = th.device(device)
        self.store = None          # dict field -> tensor [size, ...]
        self.head = 0              # physical slot of the oldest transition
        self.length = 0
        self.buffer = _LenView(self)
        self.consts = {}           # field -> python float, for fields that are never stored
        self.const_shapes = {}     # field -> trailing shape of the broadcast view
        self.v_ring = self.nv_ring = self.lp_ring = None       # slab mode: value / next_value / log_prob_a columns
        self.filed = ()            # ... of them, the ones an on-policy learner files (enable_filed_columns)

    # -- allocation on first use (shapes come from the first transition) ---------------------
    def _alloc(self, shapes):
        self.store = {k: th.zeros((self.size,) + tuple(s), dtype=th.float32, device=self.device)
                      for k, s in shapes.items()}

    # -- slab mode: the vectorised, graph-captured rollout ------------------------------------------------------------
    ROW_W = 8                      # floats per row record: [Pd, Qd, Ppv, V, price, E, older, 0] (include/flexenv.h)
    HID_TAIL_SLABS = 40            # mirrored tail of the hidden-state ring: windows of up to 39 slabs (+ next) are read in place

    def alloc_slabs(self, n_envs, n_agents, obs_dim, act_dim, hid_dim, history=None):
        """Slab-structured ring for N environments stepping in lockstep (include/flexnet.h: flexnet_rollout_pack writes it
        at a device-side cursor).  Slab k = vector step k: the observation acted on, ``hid_ring[k]`` the hidden state going
        in, ``small_ring[k]`` = [action | reward | done | last_step].  Every observation is stored once: next_state of slab
        k is the observation of slab k + 1, model.py:241's ``hid`` is ``hid_ring[k + 1]``.

        ``history`` = H (row mode; the flexibility-provision env's observation is its last H feature rows, env:387-401): the
        ring keeps every feature ROW once — ``row_ring[k]`` = one 32-byte record per (env, agent), written by the env's
        step kernel (FLEX_STEP_OBS_RING) — 1/18 of the bytes of a stacked observation per slab; a window's stacked
        observations are formed when it is gathered (flexnet_gather_window: the gather is the im2col).  The H - 1 slabs
        behind the oldest transition stay in the ring for that (H - 1 physical slabs on top of ``size // n_envs``).
        ``history`` None: ``obs_ring[k]`` holds the stacked observation itself (general rollout bodies, hand-filled rings).

        Host-side bookkeeping mirrors the device cursor: slab counter ``k`` (monotone), the slab being filled is
        ``k % slabs``; transitions are the COMPLETE slabs still in the ring.  A slab left without an action (the rollout
        was restarted from a hard reset instead of continuing) is a *gap*; sampled windows never span one."""
        self.n_envs, self.n_agents, self.obs_dim, self.act_dim, self.hid_dim = n_envs, n_agents, obs_dim, act_dim, hid_dim
        self.history = int(history) if history else None
        if self.history is not None and (obs_dim % self.history != 0 or obs_dim // self.history != 6):
            raise ValueError("row mode stores 6-feature rows: obs_dim must be 6 * history")
        self.keep_back = self.history - 1 if self.history else 0      # slabs behind a transition its observation reaches into
        self.slabs = self.size // n_envs + self.keep_back
        if self.slabs - self.keep_back < 4:
            raise ValueError("slab replay needs room for at least 4 vector steps")
        no, nh = n_agents * obs_dim, n_agents * hid_dim
        self.small_w = ((n_agents * act_dim + n_agents + 2 + 3) // 4) * 4       # 16-byte rows
        dev = self.device
        if self.history is None:
            self.obs_ring = th.zeros(self.slabs, n_envs, no, dtype=th.float32, device=dev)
            self.row_ring = None
        else:
            self.obs_ring = None
            self.row_ring = th.zeros(self.slabs, n_envs, n_agents * self.ROW_W, dtype=th.float32, device=dev)
        # (the hidden-state ring has room for a mirrored tail behind its last slab — enable_stacked_ring uses it; everybody else
        #  sees the ring proper)
        self.hid_tail_slabs = min(self.slabs, self.HID_TAIL_SLABS) if self.history is not None else 0
        self.hid_store = th.zeros(self.slabs + self.hid_tail_slabs, n_envs, nh, dtype=th.float32, device=dev)
        self.hid_ring = self.hid_store[:self.slabs]
        self.small_ring = th.zeros(self.slabs, n_envs, self.small_w, dtype=th.float32, device=dev)
        # bootstrap values r + gamma (1 - done) Q'(s', pi(s')) needs, per transition, filed by the trainer for the windows of
        # ONE update event (trainer.replay_event: the networks behind them do not change between its value sub-updates)
        self.nv_ring = th.zeros(self.slabs, n_envs, n_agents, dtype=th.float32, device=dev)
        # physical slab indices on the device (include/flexnet.h): [0] the slab the policy reads, [1] the slab being filled
        self.cursor = th.zeros(2, dtype=th.int64, device=dev)
        self.k = 0                   # host mirror of cursor[0]
        self.first = 0               # oldest slab counter whose transition may still be in the ring
        self.gaps = []               # slab counters without a transition (half-written by the step before a hard reset)
        self.consts = {"log_prob_a": 0.0, "value": 0.0, "next_value": 0.0, "action_avail": 1.0}
        self.const_shapes = {"log_prob_a": (n_agents, act_dim), "value": (n_agents, 1), "next_value": (n_agents, 1),
                             "action_avail": (n_agents, act_dim)}
        self.store = None
        self.head = 0
        self.length = 0
        self.v_ring = self.lp_ring = None      # enable_filed_columns
        self.filed = ()

    @property
    def slab_mode(self):
        return getattr(self, "hid_ring", None) is not None

    @property
    def row_mode(self):
        return getattr(self, "row_ring", None) is not None

    def release_slabs(self):
        """Back to the field-by-field mode (the graph rollout could not be captured): the rings and their bookkeeping go,
        ``add_batch`` allocates its own store on the next call.  Transitions the ring held are dropped."""
        self.obs_ring = self.row_ring = self.hid_ring = self.hid_store = self.small_ring = self.nv_ring = self.cursor = None
        self.stack_ring = None
        self.v_ring = self.lp_ring = None
        self.filed = ()
        self.k = self.first = 0
        self.gaps = []
        self.consts, self.const_shapes = {}, {}
        self.store = None
        self.head = self.length = 0

    def begin_stream(self, first_obs):
        """A rollout starts from a hard reset: ``first_obs`` [N, n, obs] becomes the observation of the slab at the
        cursor, its hidden state is zero.  If a previous stream left the slab at the cursor half-written (observation
        without an action), that slab becomes a gap and the stream starts one slab later."""
        if self.k > 0:
            self.gaps.append(self.k)
            self.k += 1
        p = self.k % self.slabs
        if self.row_mode:
            # the first observation of an episode: its newest feature row, no older ones (zero left-padding)
            rec = self.row_ring[p].view(self.n_envs, self.n_agents, self.ROW_W)
            rec.zero_()
            rec[:, :, :6].copy_(first_obs.reshape(self.n_envs, self.n_agents, self.obs_dim)[:, :, -6:])
        else:
            self.obs_ring[p].copy_(first_obs.reshape(self.n_envs, -1))
        self.hid_ring[p].zero_()
        self.cursor.fill_(p)
        self._retire()

    def stepped(self):
        """Host mirror of one flexnet_rollout_pack launch (or graph replay): slab k is complete, the cursor moved on.
        Returns the physical index of the slab just completed."""
        done_slab = self.k % self.slabs
        self.k += 1
        self._retire()
        return done_slab

    def _retire(self):
        # the slab at the cursor (and its half-written successor after the next step) overwrite the oldest ones; in row mode
        # the oldest transition's observation also reaches keep_back slabs further back
        self.first = max(self.first, self.k + 2 - self.slabs + self.keep_back)
        self.gaps = [g for g in self.gaps if g >= self.first]
        self.length = self.n_envs * (self.k - self.first - len(self.gaps))

    def _runs(self):
        """Maximal runs [a, b) of slab counters holding consecutive complete transitions."""
        runs, a = [], self.first
        for g in self.gaps:
            if g > a:
                runs.append((a, g))
            a = g + 1
        if self.k > a:
            runs.append((a, self.k))
        return runs

    def sample_slot(self, batch_size):
        """utils/replay_buffer.py:17-21 on the slab ring: a uniformly random start among the windows of ``batch_size``
        consecutive transitions (slots; time-major, so consecutive slots are the N environments of one vector step, then
        the next step).  Returns the start as a global slot number (slab counter * N + env)."""
        N = self.n_envs
        spans = [(a * N, (b - a) * N - batch_size + 1) for a, b in self._runs() if (b - a) * N >= batch_size]
        total = sum(c for _, c in spans)
        if total < 1:
            raise ValueError("not enough transitions for a batch")
        r = int(np.random.randint(total))
        for base, c in spans:
            if r < c:
                return base + r
            r -= c
        raise AssertionError

    def warmup_slot(self, rows):
        """Start of a window of ``rows`` consecutive complete slots for a capture's warm-up steps: the first run of the
        ring that is long enough (the oldest run otherwise — its tail may then be slabs no transition was filed in, which
        the warm-up, whose steps are undone, only needs to be finite).  Deterministic: sample_slot would move the global
        NumPy stream that utils/replay_buffer.py:17-21 draws the real windows from."""
        N = self.n_envs
        for a, b in self._runs():
            if (b - a) * N >= rows:
                return a * N
        return self._logical_to_slot(0)

    def segments(self, slot, rows):
        """Physical pieces of the global slot range [slot, slot + rows): [(physical_slot, count)] (two at the ring's seam)."""
        cap = self.slabs * self.n_envs
        p = slot % cap
        first = min(rows, cap - p)
        return [(p, first)] + ([(0, rows - first)] if first < rows else [])

    def slab_window(self, slot, batch_size):
        """Transition of device tensors for the window starting at global slot ``slot`` (eager consumers)."""
        N, n = self.n_envs, self.n_agents

        def take(ring, start, rows):
            flat = ring.view(self.slabs * N, -1)
            parts = [flat[p:p + c] for p, c in self.segments(start, rows)]
            return parts[0] if len(parts) == 1 else th.cat(parts)

        na = n * self.act_dim
        small = take(self.small_ring, slot, batch_size)
        if self.row_mode:
            state, next_state = self.stacked_obs(slot, batch_size), self.stacked_obs(slot + N, batch_size)
        else:
            state, next_state = take(self.obs_ring, slot, batch_size), take(self.obs_ring, slot + N, batch_size)
        out = {"state": state.view(batch_size, n, self.obs_dim),
               "next_state": next_state.view(batch_size, n, self.obs_dim),
               "last_hid": take(self.hid_ring, slot, batch_size).view(batch_size, n, self.hid_dim),
               "hid": take(self.hid_ring, slot + N, batch_size).view(batch_size, n, self.hid_dim),
               "action": small[:, :na].reshape(batch_size, n, self.act_dim),
               "reward": small[:, na:na + n], "done": small[:, na + n], "last_step": small[:, na + n + 1]}
        for k, c in self.consts.items():
            shape = self.const_shapes.get(k, ())
            out[k] = th.full((1,) + tuple(1 for _ in shape), float(c), device=self.device).expand((batch_size,) + tuple(shape))
            out[k]._flex_const = float(c)
        for k, ring in self._filed_rings().items():           # columns an on-policy learner filed (enable_filed_columns)
            out[k] = take(ring, slot, batch_size).view((batch_size,) + tuple(self.const_shapes[k]))
        return Transition(**out)

    # -- columns filed after the fact (on-policy learners: learner.IPPO.begin_update_event) -------------------------------
    def enable_filed_columns(self, log_prob=False):
        """Slab mode: ``value`` / ``next_value`` (and ``log_prob_a``) become real columns — rings beside ``small_ring``
        that ``file_columns`` writes and ``slab_window`` hands out — instead of the constants the DDPG losses never read."""
        dev, n = self.device, self.n_agents
        if self.v_ring is None:
            self.v_ring = th.zeros(self.slabs, self.n_envs, n, dtype=th.float32, device=dev)
        if log_prob and self.lp_ring is None:
            self.lp_ring = th.zeros(self.slabs, self.n_envs, n * self.act_dim, dtype=th.float32, device=dev)
        self.filed = ("value", "next_value") + (("log_prob_a",) if log_prob else ())
        for k in self.filed:
            self.consts.pop(k, None)

    def _filed_rings(self):
        rings = {"value": self.v_ring, "next_value": self.nv_ring, "log_prob_a": self.lp_ring}
        return {k: rings[k] for k in self.filed}

    def contiguous_runs(self):
        """[(first logical transition, count)] of the runs of consecutive transitions (slab mode: between the gaps)."""
        if not self.slab_mode:
            return [(0, self.length)] if self.length else []
        out, at = [], 0
        for a, b in self._runs():
            out.append((at, (b - a) * self.n_envs))
            at += (b - a) * self.n_envs
        return out

    def field_rows(self, name):
        """Rows per transition of a stored field (the reference's single-env rollout stores [1, a] log-probabilities)."""
        if self.slab_mode:
            return self.const_shapes[name][0]
        return self.store[name].shape[1]

    def file_columns(self, start, rows, **cols):
        """Writes ``cols`` (field -> [rows, ...]) over the logical transitions [start, start + rows)."""
        if self.slab_mode:
            slot = self._logical_to_slot(start)
            rings = self._filed_rings()
            for k, v in cols.items():
                flat, v, off = rings[k].view(self.slabs * self.n_envs, -1), v.reshape(rows, -1), 0
                for p, c in self.segments(slot, rows):
                    flat[p:p + c].copy_(v[off:off + c])
                    off += c
            return
        p0 = (self.head + start) % self.size
        for k, v in cols.items():
            dst = self.store[k]
            if p0 + rows <= self.size:
                dst[p0:p0 + rows].copy_(v.reshape((rows,) + dst.shape[1:]))
            else:
                idx = (p0 + th.arange(rows, device=self.device)) % self.size
                dst.index_copy_(0, idx, v.reshape((rows,) + dst.shape[1:]).to(dst.dtype))

    def aligned_window(self, step, batch_size, n_envs):
        """The window of ``batch_size`` transitions that starts at vector step ``step`` (0 = the oldest) of a time-major
        replay of ``n_envs`` environments: whole vector steps, row = t * n_envs + env.  ValueError where the batch is not a
        whole number of steps, the replay is not step-aligned, or the window would cross a gap of the ring."""
        self._check_aligned(batch_size, n_envs)
        return self.window(step * n_envs, batch_size)

    def _check_aligned(self, batch_size, n_envs):
        if batch_size % n_envs != 0 or batch_size < n_envs:
            raise ValueError(f"a pooled window of {batch_size} transitions is not a whole number of steps of {n_envs} environments")
        if self.slab_mode:
            if n_envs != self.n_envs:
                raise ValueError("the slab ring was allocated for another number of environments")
        elif self.length % n_envs != 0 or self.head % n_envs != 0:
            raise ValueError("the replay does not hold whole vector steps")

    def sample_aligned(self, batch_size, n_envs):
        """utils/replay_buffer.py:17-21 over step-aligned windows: a uniformly random start among the windows of
        ``batch_size // n_envs`` consecutive whole vector steps (none spans a gap).  Returns the start's vector step."""
        self._check_aligned(batch_size, n_envs)
        w = batch_size // n_envs
        spans, at = [], 0
        for _, count in self.contiguous_runs():
            steps = count // n_envs
            if steps >= w:
                spans.append((at, steps - w + 1))
            at += steps
        total = sum(c for _, c in spans)
        if total < 1:
            raise ValueError("not enough transitions for a batch")
        r = int(np.random.randint(total))
        for base, c in spans:
            if r < c:
                return base + r
            r -= c
        raise AssertionError

    def get_window_aligned(self, batch_size, n_envs):
        return self.aligned_window(self.sample_aligned(batch_size, n_envs), batch_size, n_envs)

    def stacked_obs(self, slot, rows, out=None):
        """Row mode: the stacked observations [rows, n_agents * obs_dim] of the global slot range [slot, slot + rows), formed
        from the row ring by ONE launch of flexnet_gather_window (include/flexnet.h); the ring's seam is the kernel's business."""
        from . import _lib
        if self.device.type != "cuda":                    # (no kernel off the GPU: the same rows as a tensor composition)
            g = th.arange(int(slot), int(slot) + rows, dtype=th.int64)
            res = self.stacked_rows(g // self.n_envs, g % self.n_envs).reshape(rows, -1)
            return res if out is None else out.copy_(res)
        if out is None:
            out = th.empty(rows, self.n_agents * self.obs_dim, dtype=th.float32, device=self.device)
        a = _lib.FlexWindowArgs()
        a.row_ring, a.dst, a.rows, a.first_slot = self.row_ring.data_ptr(), out.data_ptr(), rows, int(slot)
        a.n_envs, a.n_agents, a.history, a.slabs = self.n_envs, self.n_agents, self.history, self.slabs
        _lib.launch("flexnet_gather_window", a)
        return out

    def stacked_rows(self, counters, envs):
        """Row mode: the stacked observations [R, n_agents, obs_dim] of the (slab counter, environment) pairs given as two
        int64 tensors — flexnet_gather_window's rule (include/flexnet.h) as index tensors, an im2col and a select; plain
        copies, so bit-equal to the kernel's rows."""
        H, n, N = self.history, self.n_agents, self.n_envs
        dev = self.device
        c, e = counters.to(dev), envs.to(dev)
        rec = self.row_ring.view(self.slabs, N, n, self.ROW_W)
        back = th.arange(H - 1, -1, -1, device=dev)                                   # slot h reaches H - 1 - h slabs back
        rows = rec[(c[:, None] - back[None, :]) % self.slabs, e[:, None]]            # [R, H, n, 8]
        older = rec[c % self.slabs, e][:, :, 6]                                       # [R, n]
        live = back.to(th.float32)[None, :, None] <= older[:, None, :]               # [R, H, n]
        out = th.where(live[..., None], rows[..., :6], th.zeros((), device=dev))
        return out.permute(0, 2, 1, 3).reshape(c.shape[0], n, 6 * H)

    # -- stacked-observation ring (row mode, round 5): every slab's stacked observations formed ONCE ------------------------
    def enable_stacked_ring(self, max_window_rows):
        """Keep, next to the row ring, the stacked observations [n_agents * obs_dim] of every slab — ``stack_ring`` [slabs * N
        + tail, n * obs] — so that a sampled window is a contiguous run of its rows and captured sub-updates read it IN PLACE
        (nets.RING_VIEWS) instead of gathering it into a static batch first.  A slab is expanded once, when it has entered the
        replay (``expand_stacked``: flexnet_gather_window into the ring); at the reference's sample reuse the per-window gather
        expanded each observation ~6 times.  The first ``tail`` rows are mirrored behind the ring's end, so a window of up to
        ``max_window_rows`` rows that starts anywhere in the ring never wraps.  2 880 B per transition: 2.5 GB for the bench's
        ring of 192 + 23 slabs of 4 096 environments."""
        if not self.row_mode:
            raise RuntimeError("the stacked-observation ring lives next to the ROW ring (row mode)")
        N = self.n_envs
        tail = -(-int(max_window_rows) // N) * N
        if getattr(self, "stack_ring", None) is not None and self.stack_tail >= tail:
            return
        if tail > self.slabs * N:
            raise ValueError("window longer than the ring")
        # (a longer tail than the existing ring's: a NEW ring — graphs captured against the old one have its address baked in
        #  and are recaptured when next used, trainer._ensure_graph compares ``stack_gen``)
        self.stack_gen = getattr(self, "stack_gen", 0) + 1
        old = getattr(self, "stack_ring", None)
        if old is not None:
            from . import nets
            old_ptr = old.untyped_storage().data_ptr()
            for key in list(nets.RING_VIEWS):
                ring, _cell, ref = nets.RING_VIEWS[key]
                if ref() is None or ring.untyped_storage().data_ptr() == old_ptr:
                    del nets.RING_VIEWS[key]
            del old
        self.stack_rows = self.slabs * N
        self.stack_tail = tail
        self.stack_ring = th.zeros(self.stack_rows + tail, self.n_agents * self.obs_dim, dtype=th.float32, device=self.device)
        self.stacked_next = None         # slab counter the next expansion starts at (None: the oldest transition's)
        # every possible first row, as int64: a window's cell is set by ONE 8-byte row copy inside the gather launch that
        # refreshes the batch's other fields (no launch of its own: a fill kernel per cell was 4.5 us of a 360-us sub-update)
        self.slot_table = th.arange(self.stack_rows, dtype=th.int64, device=self.device)

    def expand_stacked(self):
        """Bring the stacked ring up to date: the slabs filed since the last call (the slab at the cursor included — it holds
        the newest observation, the next_state of the last complete transition)."""
        if getattr(self, "stack_ring", None) is None:
            return
        N = self.n_envs
        lo = self.first if self.stacked_next is None else max(self.stacked_next, self.first)
        hi = self.k
        if hi - lo + 1 > self.slabs:
            lo = hi - self.slabs + 1
        tail_slabs = self.stack_tail // N
        c = lo
        while c <= hi:
            p = c % self.slabs
            run = min(hi - c + 1, self.slabs - p)
            self.stacked_obs(c * N, run * N, out=self.stack_ring[p * N:(p + run) * N])
            if p < tail_slabs:                            # the ring's head, mirrored behind its end
                q = min(run, tail_slabs - p)
                self.stack_ring[self.stack_rows + p * N:self.stack_rows + (p + q) * N].copy_(self.stack_ring[p * N:(p + q) * N])
            if p < self.hid_tail_slabs:                   # ... and the hidden states of the same slabs (read in place as well)
                q = min(run, self.hid_tail_slabs - p)
                self.hid_store[self.slabs + p:self.slabs + p + q].copy_(self.hid_store[p:p + q])
            c += run
        self.stacked_next = hi + 1

    @property
    def obs_source_ring(self):
        """Name of the ring observations are gathered from: "row_ring" (row mode) or "obs_ring"."""
        return "row_ring" if self.row_mode else "obs_ring"

    # what a field of the Transition is in the ring: (ring name, first column, width or None = whole row, slab offset)
    def field_source(self, name):
        n, na = self.n_agents, self.n_agents * self.act_dim
        obs = self.obs_source_ring
        return {"state": (obs, 0, None, 0), "next_state": (obs, 0, None, 1),
                "last_hid": ("hid_ring", 0, None, 0), "hid": ("hid_ring", 0, None, 1),
                "action": ("small_ring", 0, na, 0), "reward": ("small_ring", na, n, 0),
                "done": ("small_ring", na + n, 1, 0), "last_step": ("small_ring", na + n + 1, 1, 0),
                "next_value": ("nv_ring", 0, None, 0)}[name]

    def field_shape(self, name):
        n = self.n_agents
        return {"state": (n, self.obs_dim), "next_state": (n, self.obs_dim), "last_hid": (n, self.hid_dim),
                "hid": (n, self.hid_dim), "action": (n, self.act_dim), "reward": (n,), "done": (), "last_step": (),
                "next_value": (n, 1)}[name]

    STORED = ("state", "action", "reward", "next_state", "done", "last_step", "last_hid", "hid")

    def gather(self, plan, slot, td=None):
        """Refresh static batch tensors from the window starting at global slot ``slot``: ONE launch of
        flexnet_gather_rows (include/flexnet.h).  ``plan`` = [(ring name, first column, width, row offset, rows, dst)],
        dst a contiguous [rows, width] fp32 tensor.  ``td`` = (reward tensor of the plan, FlexTdLossArgs): the value loss's
        reward-statistics pass rides in the same launch (flexnet_gather_rows_td; nets.offer_td_stats)."""
        from . import _lib
        jobs = []
        td_first = td_count = None
        for ring_name, col0, width, row_off, rows, dst in plan:
            if td is not None and dst is td[0]:
                td_first = len(jobs)
            if ring_name == "stack_ring":                # read in place (enable_stacked_ring): only the window's first row moves
                cell = dst[0]
                self.expand_stacked()
                if rows + row_off > self.stack_tail:
                    raise ValueError("window longer than the stacked ring's mirrored tail")
                p = slot % self.stack_rows               # (views further into the window shift the ring's BASE, not the cell)
                jobs.append((self.slot_table.data_ptr() + 8 * p, cell.data_ptr(), 1, 2, 2))
                continue
            if ring_name == "row_ring":                  # stacked observations out of the row ring: a launch of its own kind
                self.stacked_obs(slot + row_off, rows, out=dst)
                continue
            ring = getattr(self, ring_name)
            stride = ring.shape[2]
            width = stride if width is None else width
            base, out, done_rows = ring.data_ptr(), dst.data_ptr(), 0
            for p, c in self.segments(slot + row_off, rows):
                jobs.append((base + 4 * (p * stride + col0), out + 4 * done_rows * width, c, width, stride))
                done_rows += c
            if td is not None and dst is td[0]:
                td_count = len(jobs) - td_first
        # a window that wraps the ring's seam splits every field in two: up to 2 x 8 stored fields = 16 jobs against the
        # launch's FLEXNET_GATHER_MAX_JOBS (12) — the rest goes out as a second launch instead of an intermittent error
        for lo in range(0, len(jobs), _lib.FLEXNET_GATHER_MAX_JOBS):
            a = _lib.FlexGatherArgs()
            chunk = jobs[lo:lo + _lib.FLEXNET_GATHER_MAX_JOBS]
            for j, (src, dst_p, c, width, stride) in enumerate(chunk):
                a.src[j], a.dst[j] = src, dst_p
                a.rows[j], a.width[j], a.src_stride[j], a.dst_stride[j] = c, width, stride, width
            a.n_jobs = len(chunk)
            if td_count and lo <= td_first and td_first + td_count <= lo + len(chunk):
                _lib.launch("flexnet_gather_rows_td", a, td_first - lo, td_count, td[1])
                td_count = 0
            else:
                _lib.launch("flexnet_gather_rows", a)
        if td is not None and td_count != 0:
            # (the reward's copies fell across two launches, or the plan does not gather the tensor: the pass on its own)
            _lib.launch("flexnet_td_stats", td[1])

    def window_refresh_args(self, plan, start_cell, td=None):
        """``plan`` as FlexWindowRefreshArgs with the window's first slot read from the device cell ``start_cell`` (int64, a
        global slot number as sample_slot returns it) — the refresh a HIP graph can hold (trainer: one graph per update
        event).  Returns (args, FlexTdLossArgs or None), or None when the plan holds something this form does not cover (a
        window expanded out of the row ring, rings of different lengths, more jobs than the launch takes)."""
        from . import _lib
        a = _lib.FlexWindowRefreshArgs()
        a.start, a.ring_rows = start_cell.data_ptr(), self.slabs * self.n_envs
        nj = nc = 0
        td_args = None
        for ring_name, col0, width, row_off, rows, dst in plan:
            if ring_name == "stack_ring":
                if nc >= _lib.FLEXNET_WINDOW_MAX_CELLS or rows + row_off > self.stack_tail or self.stack_rows != a.ring_rows:
                    return None
                a.cell[nc], a.cell_mod[nc] = dst[0].data_ptr(), self.stack_rows
                nc += 1
                continue
            if ring_name == "row_ring" or nj >= _lib.FLEXNET_WINDOW_MAX_JOBS:
                return None
            ring = getattr(self, ring_name)
            if ring.shape[0] * ring.shape[1] != a.ring_rows:
                return None
            stride = ring.shape[2]
            width = stride if width is None else width
            a.base[nj], a.dst[nj] = ring.data_ptr() + 4 * col0, dst.data_ptr()
            a.rows[nj], a.row_off[nj], a.width[nj], a.src_stride[nj] = rows, row_off, width, stride
            if td is not None and dst is td[0]:
                a.reward_job, td_args = nj, td[1]
            nj += 1
        if td is not None and td_args is None:
            return None
        a.n_jobs, a.n_cells = nj, nc
        return a, td_args

    def window_refresh(self, args):
        """Launch a refresh prepared by window_refresh_args on the current stream (capturable)."""
        from . import _lib
        _lib.launch("flexnet_window_refresh", *args)

    def scatter(self, ring_name, src, slot, rows):
        """The reverse of one gather job: rows of the contiguous [rows, width] tensor ``src`` into the ring's slots of the
        global slot range [slot, slot + rows) (two pieces at the seam): one launch of flexnet_gather_rows."""
        from . import _lib
        ring = getattr(self, ring_name)
        stride = ring.shape[2]
        if not (src.is_contiguous() and src.dtype == th.float32 and src.numel() == rows * stride):
            raise ValueError("scatter: src must be a contiguous fp32 [rows, row width of the ring] tensor")
        a = _lib.FlexGatherArgs()
        done_rows = 0
        for j, (p, c) in enumerate(self.segments(slot, rows)):
            a.src[j], a.dst[j] = src.data_ptr() + 4 * done_rows * stride, ring.data_ptr() + 4 * p * stride
            a.rows[j], a.width[j], a.src_stride[j], a.dst_stride[j] = c, stride, stride, stride
            done_rows += c
            a.n_jobs = j + 1
        _lib.launch("flexnet_gather_rows", a)

    def _logical_to_slot(self, index):
        """Global slot of logical transition ``index`` (0 = oldest), skipping gaps."""
        N = self.n_envs
        for a, b in self._runs():
            cnt = (b - a) * N
            if index < cnt:
                return a * N + index
            index -= cnt
        raise IndexError("transition index out of range")

    def _slots(self, count):
        """Physical slots for ``count`` new transitions, dropping the oldest when full."""
        if count > self.size:
            raise ValueError("more transitions than capacity in one add")
        start = (self.head + self.length) % self.size
        overflow = max(0, self.length + count - self.size)
        self.head = (self.head + overflow) % self.size
        self.length = self.length + count - overflow
        return start

    def add_batch(self, **fields):
        """One transition per row: every field is a tensor [B, ...] already on the device.  Fields given as a
        python float are constants (e.g. action_avail = 1.0, the unused value/next_value = 0.0): nothing is stored
        for them, ``window`` hands out a broadcast view with the shape given in ``const_shapes``."""
        consts = {k: v for k, v in fields.items() if not isinstance(v, th.Tensor)}
        fields = {k: v for k, v in fields.items() if isinstance(v, th.Tensor)}
        b = next(iter(fields.values())).shape[0]
        if self.slab_mode:
            raise RuntimeError("this replay buffer is in slab mode (written by flexnet_rollout_pack); add_batch is the "
                               "field-by-field mode of the eager rollout")
        if self.store is None:
            self._alloc({k: v.shape[1:] for k, v in fields.items()})
            self.consts = dict(consts)
        start = self._slots(b)
        first = min(b, self.size - start)
        for k, v in fields.items():
            dst = self.store[k]
            v = v.to(dst.dtype)
            dst[start:start + first].copy_(v[:first])
            if first < b:
                dst[:b - first].copy_(v[first:])

    def add_experience(self, trans):
        """replay_buffer.py:23-27 with the Transition of model.py:230-242 (numpy fields)."""
        row = _transition_row(trans)
        self.add_batch(**{k: th.from_numpy(v).to(self.device) for k, v in row.items()})

    def clear(self):
        self.head = 0
        self.length = 0
        if self.slab_mode:
            self.first, self.gaps = self.k, []

    # -- sampling ------------------------------------------------------------------------------
    def sample_start(self, batch_size):
        sample_range = self.length - batch_size + 1
        if sample_range < 1:
            raise ValueError("not enough transitions for a batch")
        if sample_range <= self.EXACT_STREAM_MAX:
            # replay_buffer.py:18-19 verbatim, so that np.random.seed reproduces the reference's index sequence;
            # NumPy draws it as the head of a full permutation of `sample_range` elements
            return int(np.random.choice(sample_range, 1, replace=False)[0])
        # vectorised buffers hold 10^5..10^7 slots: the same uniform start without an O(n) permutation per sample
        return int(np.random.randint(sample_range))

    def window(self, start, batch_size):
        """Device tensors of logical transitions [start, start+batch_size)."""
        if self.slab_mode:
            slot = self._logical_to_slot(start)
            if self._logical_to_slot(start + batch_size - 1) != slot + batch_size - 1:
                raise ValueError("window spans a gap of the slab ring")
            return self.slab_window(slot, batch_size)
        p0 = (self.head + start) % self.size
        out = {}
        for k, c in self.consts.items():
            shape = self.const_shapes.get(k, ())
            out[k] = th.full((1,) + tuple(1 for _ in shape), float(c), device=self.device).expand((batch_size,) + tuple(shape))
            out[k]._flex_const = float(c)          # readers may skip work that a known constant makes the identity
        if p0 + batch_size <= self.size:
            out.update({k: v[p0:p0 + batch_size] for k, v in self.store.items()})
        else:
            idx = (p0 + th.arange(batch_size, device=self.device)) % self.size
            out.update({k: v.index_select(0, idx) for k, v in self.store.items()})
        return Transition(**out)

    def get_batch_tensors(self, batch_size):
        if self.slab_mode:
            return self.slab_window(self.sample_slot(batch_size), batch_size)
        return self.window(self.sample_start(batch_size), batch_size)

    def get_single(self, index):
        w = self.window(index, 1)
        return Transition(*[f[0] for f in w])

    def get_batch(self, batch_size):
        """replay_buffer.py:14-21: a list of ``batch_size`` per-transition tuples (device tensors inside).
        Kept for callers written against the reference (trainer.py:67-68 zips it back into columns)."""
        w = self.get_batch_tensors(batch_size)
        return [Transition(*[f[i] for f in w]) for i in range(batch_size)]


class TransReplayBuffer(DeviceReplayBuffer):
    """Name and constructor of utils/replay_buffer.py:3-6 (``TransReplayBuffer(int size)``)."""

    def __init__(self, size, device=None):
        if device is None:
            device = "cuda" if th.cuda.is_available() else "cpu"
        super().__init__(size, device)


class _EpisodeCount:
    """``.buffer`` of the episodic memory: len() is the number of EPISODES (model.py:77)."""

    def __init__(self, owner):
        self._owner = owner

    def __len__(self):
        return len(self._owner.episodes)


class EpisodeReplayBuffer(DeviceReplayBuffer):
    """utils/replay_buffer.py:33-56 (``episodic: True``, default.yaml:9), device-resident: ``add_experience(episode)``,
    ``get_batch``, ``get_single`` and ``.buffer`` whose len() counts episodes.  Kept from the reference:
      * the capacity ``size`` counts EPISODES and the oldest episode is dropped first (replay_buffer.py:52-56);
      * a batch is the transitions of ``np.random.choice(len, batch_size, replace=False)`` episodes — that very call on the
        global NumPy stream, so ``np.random.seed`` reproduces the reference's draws — CONCATENATED in the drawn order
        (replay_buffer.py:44-50);
      * there is no ``clear`` in the reference; the on-policy classes' data is NOT dropped after an update — their episodic
        mode is ``batch_size = replay_buffer_size = behaviour_update_freq`` (default.yaml:1).

    Three stores, one surface (``get_batch_tensors`` is what the trainer uses: a Transition of device tensors, rows
    episode-major in the drawn order; ``last_draw`` keeps the drawn ids):
      * one environment (``add_experience``): a list of episodes, each a tensor per field — the reference's semantics
        exactly;
      * N environments in lockstep (``configure_blocks`` by the trainer, then the rollouts' own ``add_batch`` / slab ring and
        ``end_block``): the transitions live in the parent's time-major ring, field by field (eager rollout) or in slabs
        (graph rollout), and this class keeps an episode TABLE of (step counter of the first step, environment, length).

    The N > 1 mapping.  One ``train_process`` call is a *block*: N environments for ``horizon`` vector
    steps.  Each environment's rows of a block split at ``last_step`` into complete episodes (an early termination restarts
    in place; the block's last step carries last_step = 1), so a block adds at least N episodes.  Capacity: ``size`` counts
    BLOCKS — the table holds the episodes of the last ``size`` blocks, and the ring is sized to keep their slabs:
    ``size * (horizon + 1)`` vector steps (one slab per block may be a gap, left behind by a hard reset) + the two in flight
    + the slabs an observation reaches back into; should the ring retire the slab of an episode's first step all the same,
    that episode leaves too.  "Oldest first" is therefore by block: the episodes of the oldest block leave together, whichever
    environment they belong to; within the table the order is (first step, environment).  Cadence:
    ``trainer.episodes`` counts blocks, as a vector step is one "step" of the transition modes.  An episode of environment e
    is the strided rows (c0 + j) * N + e of the ring; a batch is gathered by ONE launch of flexnet_gather_episodes
    (include/flexnet.h) from the slab rings, by index tensors from the field-by-field store."""

    def __init__(self, size, device=None):
        if device is None:
            device = "cuda" if th.cuda.is_available() else "cpu"
        super().__init__(size, device)
        self.capacity = int(size)         # episodes (blocks, once configure_blocks was called)
        self.episodes = []                # list store: {field: tensor [L, ...]}; ring stores: (first step, env, length)
        self.buffer = _EpisodeCount(self)
        self.block_steps = None           # ring stores: vector steps per block
        self.block_envs = 1
        self.block_starts = []            # ring stores: step counter of the first step of every block in the table
        self.k_field = 0                  # field-by-field ring: vector steps added so far (the slab ring's ``k``)
        self.last_draw = None             # ids of the last batch's episodes, in the drawn order
        self.use_kernel = True            # (tests and tools compare with the tensor composition)

    # -- configuration of the vectorised form ----------------------------------------------------------------------------
    def configure_blocks(self, n_envs, horizon):
        """N environments for ``horizon`` vector steps per block: the parent's ring is sized for ``capacity`` blocks, a gap slab
        per block, plus the two vector steps the slab ring keeps back for the step in flight."""
        if self.episodes or self.store is not None or self.slab_mode:
            raise RuntimeError("configure_blocks comes before the first transition")
        self.block_envs, self.block_steps = int(n_envs), int(horizon)
        self.size = (self.capacity * (self.block_steps + 1) + 2) * self.block_envs

    @property
    def ring_store(self):
        return self.block_steps is not None

    def _step_counter(self):
        return self.k if self.slab_mode else self.k_field

    def add_batch(self, **fields):
        super().add_batch(**fields)
        if self.ring_store:
            b = next(v for v in fields.values() if isinstance(v, th.Tensor)).shape[0]
            if b != self.block_envs:
                raise ValueError("the episodic ring takes one vector step of all its environments per add_batch")
            self.k_field += 1

    def release_slabs(self):
        super().release_slabs()
        self.episodes, self.block_starts, self.k_field = [], [], 0

    def clear(self):
        """Not part of the reference's EpisodeReplayBuffer; drops every episode (and, with them, the ring's transitions)."""
        super().clear()
        self.episodes, self.block_starts = [], []
        if self.ring_store and not self.slab_mode:
            self.store, self.k_field = None, 0

    # -- filling ----------------------------------------------------------------------------------------------------------
    def add_experience(self, episode):
        """replay_buffer.py:52-56: ``episode`` is the list of an episode's Transitions (model.py:230-242, numpy fields)."""
        if self.ring_store:
            raise RuntimeError("this episodic memory was configured for a vectorised rollout (end_block files its episodes)")
        if len(episode) < 1:
            raise ValueError("an episode holds at least one transition")
        rows = [_transition_row(t) for t in episode]
        if 1 + len(self.episodes) > self.capacity:
            self.episodes.pop(0)
        self.episodes.append({k: th.from_numpy(np.concatenate([r[k] for r in rows])).to(self.device) for k in FIELDS})

    def end_block(self, steps):
        """The last ``steps`` vector steps of the ring are a block: every environment's rows split at ``last_step`` into
        episodes, which join the table; rows behind an environment's last mark belong to no episode.  One device read."""
        if not self.ring_store:
            raise RuntimeError("end_block belongs to the vectorised form (configure_blocks)")
        N, k = self.block_envs, self._step_counter()
        steps = int(steps)
        if steps < 1 or steps > k:
            raise ValueError("a block is at least one and at most every vector step filed so far")
        cs = th.arange(k - steps, k, device=self.device)
        if self.slab_mode:
            col = self.n_agents * self.act_dim + self.n_agents + 1
            last = self.small_ring[cs % self.slabs, :, col]
        else:
            rows = (cs[:, None] * N + th.arange(N, device=self.device)[None, :]) % self.size
            last = self.store["last_step"].reshape(self.size)[rows]
        last = last.cpu().numpy() != 0
        new = []
        for e in range(N):
            start = 0
            for t in np.flatnonzero(last[:, e]):
                new.append((k - steps + start, e, int(t) - start + 1))
                start = int(t) + 1
        self.episodes.extend(sorted(new))
        self.block_starts.append(k - steps)
        del self.block_starts[:-self.capacity]
        self._retire_episodes()

    def _retire_episodes(self):
        if not self.ring_store or not self.episodes:
            return
        k = self._step_counter()
        lo = max(self.block_starts[0], self.first if self.slab_mode else k - self.size // self.block_envs)
        if self.episodes[0][0] < lo:
            self.episodes = [ep for ep in self.episodes if ep[0] >= lo]

    # -- batches ----------------------------------------------------------------------------------------------------------
    def draw(self, batch_size):
        """replay_buffer.py:45-46, verbatim."""
        self._retire_episodes()
        length = len(self.episodes)
        indices = np.random.choice(length, batch_size, replace=False)
        self.last_draw = [int(i) for i in indices]
        return self.last_draw

    def get_batch_tensors(self, batch_size):
        return self.episodes_batch(self.draw(batch_size))

    def episode_table(self, ids):
        """[len(ids), 4] int64 (first step, environment, length, first output row) of the episodes ``ids``, in that order."""
        table = np.zeros((len(ids), 4), dtype=np.int64)
        at = 0
        for i, j in enumerate(ids):
            c0, e, length = self.episodes[j]
            table[i] = (c0, e, length, at)
            at += length
        return table

    def episodes_batch(self, ids):
        """The transitions of the episodes ``ids`` one behind the other, as a Transition of device tensors."""
        if not self.ring_store:
            eps = [self.episodes[i] for i in ids]
            return Transition(**{k: th.cat([ep[k] for ep in eps]) for k in FIELDS})
        table = self.episode_table(ids)
        if not self.slab_mode:
            return self._compose_fields(table)
        if self.use_kernel and self.device.type == "cuda":
            out = self._gather_slabs(table)
            if out is not None:
                return out
            from .util import note_fallback
            note_fallback("gather_episodes", f"rows {int(table[:, 2].sum())}, agents {self.n_agents}, obs_dim {self.obs_dim}")
        return self._compose_slabs(table)

    def _table_rows(self, table):
        """(step counter, environment) of every output row, as int64 device tensors."""
        c = np.concatenate([np.arange(c0, c0 + length) for c0, _, length, _ in table])
        e = np.concatenate([np.full(length, env) for _, env, length, _ in table])
        return th.from_numpy(c).to(self.device), th.from_numpy(e).to(self.device)

    def _const_fields(self, rows):
        out = {}
        for k, c in self.consts.items():
            shape = self.const_shapes.get(k, ())
            out[k] = th.full((1,) + tuple(1 for _ in shape), float(c), device=self.device).expand((rows,) + tuple(shape))
            out[k]._flex_const = float(c)
        return out

    def _compose_fields(self, table):
        c, e = self._table_rows(table)
        idx = (c * self.block_envs + e) % self.size
        out = self._const_fields(idx.shape[0])
        out.update({k: v.index_select(0, idx) for k, v in self.store.items()})
        return Transition(**out)

    def _compose_slabs(self, table):
        """What flexnet_gather_episodes writes, as index tensors, ``index_select`` on the rings and the stacked-observation
        im2col: row i equals ``slab_window`` of one transition at that row's slot."""
        N, n = self.n_envs, self.n_agents
        c, e = self._table_rows(table)
        rows = c.shape[0]
        p0, p1 = (c % self.slabs) * N + e, ((c + 1) % self.slabs) * N + e

        def take(ring, p):
            return ring.view(self.slabs * N, -1).index_select(0, p)

        if self.row_mode:
            state, next_state = self.stacked_rows(c, e), self.stacked_rows(c + 1, e)
        else:
            state, next_state = take(self.obs_ring, p0), take(self.obs_ring, p1)
        na = n * self.act_dim
        small = take(self.small_ring, p0)
        out = self._const_fields(rows)
        out.update({"state": state.reshape(rows, n, self.obs_dim), "next_state": next_state.reshape(rows, n, self.obs_dim),
                    "last_hid": take(self.hid_ring, p0).view(rows, n, self.hid_dim),
                    "hid": take(self.hid_ring, p1).view(rows, n, self.hid_dim),
                    "action": small[:, :na].reshape(rows, n, self.act_dim), "reward": small[:, na:na + n].contiguous(),
                    "done": small[:, na + n].contiguous(), "last_step": small[:, na + n + 1].contiguous()})
        for k, ring in self._filed_rings().items():
            out[k] = take(ring, p0).view((rows,) + tuple(self.const_shapes[k]))
        return Transition(**out)

    def _gather_slabs(self, table, out=None, dev_table=None):
        """ONE launch of flexnet_gather_episodes; None where the library answers FLEXNET_EUNSUPPORTED.  ``out``: tensors to
        write into (tools and tests), field -> contiguous fp32 tensor; ``dev_table``: the table already on the device."""
        from . import _lib
        n, rows = self.n_agents, int(table[:, 2].sum())
        dev = self.device
        table = np.ascontiguousarray(table, dtype=np.int64)
        shapes = {"state": (n, self.obs_dim), "next_state": (n, self.obs_dim), "last_hid": (n, self.hid_dim),
                  "hid": (n, self.hid_dim), "action": (n, self.act_dim), "reward": (n,), "done": (), "last_step": ()}
        filed = self._filed_rings()
        for k in filed:
            shapes[k] = tuple(self.const_shapes[k])
        if out is None:
            out = {k: th.empty((rows,) + s, dtype=th.float32, device=dev) for k, s in shapes.items()}
        if dev_table is None:
            dev_table = th.from_numpy(table).to(dev)
        a = _lib.FlexEpisodeGatherArgs()
        a.row_ring = self.row_ring.data_ptr() if self.row_mode else None
        a.obs_ring = None if self.row_mode else self.obs_ring.data_ptr()
        a.hid_ring, a.small_ring = self.hid_ring.data_ptr(), self.small_ring.data_ptr()
        a.v_ring = self.v_ring.data_ptr() if "value" in filed else None
        a.nv_ring = self.nv_ring.data_ptr() if "next_value" in filed else None
        a.lp_ring = self.lp_ring.data_ptr() if "log_prob_a" in filed else None
        a.episodes, a.episodes_host = dev_table.data_ptr(), table.ctypes.data
        for k in shapes:
            setattr(a, k, out[k].data_ptr())
        a.rows, a.n_episodes, a.n_envs, a.n_agents = rows, table.shape[0], self.n_envs, n
        a.history, a.obs_dim, a.hid_dim, a.act_dim = self.history or 0, self.obs_dim, self.hid_dim, self.act_dim
        a.small_w, a.slabs = self.small_w, self.slabs
        if not _lib.try_launch("flexnet_gather_episodes", a):
            return None
        res = self._const_fields(rows)
        res.update(out)
        return Transition(**res)

    def get_single(self, index):
        """replay_buffer.py:38-39: episode ``index`` (0 = the oldest) as its list of per-transition tuples."""
        w = self.episodes_batch([index])
        return [Transition(*[f[i] for f in w]) for i in range(w.reward.shape[0])]

    def get_batch(self, batch_size):
        """replay_buffer.py:44-50: the drawn episodes' per-transition tuples, one list (device tensors inside)."""
        w = self.get_batch_tensors(batch_size)
        return [Transition(*[f[i] for f in w]) for i in range(w.reward.shape[0])]

    # -- the list store as logical transitions (columns an on-policy learner files after the fact) ---------------------------
    def contiguous_runs(self):
        if self.ring_store:
            return super().contiguous_runs()
        out, at = [], 0
        for ep in self.episodes:
            out.append((at, ep["reward"].shape[0]))
            at += ep["reward"].shape[0]
        return out

    def _locate(self, start, rows):
        for (at, count), ep in zip(self.contiguous_runs(), self.episodes):
            if at <= start and start + rows <= at + count:
                return ep, start - at
        raise ValueError("window spans two episodes")

    def window(self, start, batch_size):
        if self.ring_store:
            return super().window(start, batch_size)
        ep, off = self._locate(start, batch_size)
        return Transition(**{k: ep[k][off:off + batch_size] for k in FIELDS})

    def file_columns(self, start, rows, **cols):
        if self.ring_store:
            return super().file_columns(start, rows, **cols)
        ep, off = self._locate(start, rows)
        for k, v in cols.items():
            ep[k][off:off + rows].copy_(v.reshape((rows,) + ep[k].shape[1:]))

    def field_rows(self, name):
        if self.ring_store:
            return super().field_rows(name)
        return self.episodes[0][name].shape[1]
