"""Evaluation rollouts with the reference's record format (utils/tester.py:6-70).

``PGTester(args, behaviour_net, env).run(day, hour, quarter)`` returns the dict ``test_agent.py:84-96`` pickles:
keys pv_active, pv_reactive, bus_active, bus_reactive, bus_voltage, ess_energy, power_reduction, ess_charging,
ess_discharging, price — one entry after the manual reset and one per step.  With the N=1 drop-in env the
entries are the 1-D arrays the reference stores; with a ``VecFlexProvisionEnv`` every entry gains a leading
environment axis and ``day/hour/quarter`` may be arrays (one start time per environment)."""
from __future__ import annotations

import numpy as np
import torch as th

from .util import prep_obs, translate_action

RECORD_KEYS = ("pv_active", "pv_reactive", "bus_active", "bus_reactive", "bus_voltage", "ess_energy",
               "power_reduction", "ess_charging", "ess_discharging", "price")


def record_from_trace(trace, series_rows):
    """The record of ``PGTester.run`` on a vectorised env from the trace of ``Model.test_episodes(trace=True)``: ``RECORD_KEYS``
    plus ``actions``, the reset entry plus one entry per step (``actions``: one per step), every entry with the leading
    environment axis ``_run_vec`` gives it.  ``series_rows`` [steps + 1, N, cols]: the series table's rows at ``row0`` and at
    every traced ``row`` ([Pd(n_bus) | Qd(n_bus) | Ppv(n_agents) | price]).  Entries behind an environment's episode end hold
    what the trace holds there: zeros."""
    v = np.concatenate([trace["v0"][None], trace["v"]], axis=0)                    # [steps + 1, N, n_bus]
    agent = np.concatenate([trace["agent0"][None], trace["agent"]], axis=0)        # [steps + 1, N, n_agents, 5]: E, PRED, CH, DIS, QPV
    series_rows = np.asarray(series_rows)
    nb, na = v.shape[2], agent.shape[2]
    if series_rows.shape != (v.shape[0], v.shape[1], 2 * nb + na + 1):
        raise ValueError(f"series_rows must be [steps + 1, N, {2 * nb + na + 1}], got {series_rows.shape}")
    whole = {"bus_active": series_rows[:, :, :nb], "bus_reactive": series_rows[:, :, nb:2 * nb],
             "pv_active": series_rows[:, :, 2 * nb:2 * nb + na], "price": series_rows[:, :, 2 * nb + na:],
             "bus_voltage": v, "ess_energy": agent[..., 0], "power_reduction": agent[..., 1], "ess_charging": agent[..., 2],
             "ess_discharging": agent[..., 3], "pv_reactive": agent[..., 4]}
    record = {k: [np.ascontiguousarray(x) for x in whole[k]] for k in RECORD_KEYS}
    record["actions"] = [np.ascontiguousarray(x) for x in trace["actions"]]
    return record


class PGTester(object):
    def __init__(self, args, behaviour_net, env):
        self.args, self.env = args, env
        self.device = th.device("cuda" if th.cuda.is_available() and args.cuda else "cpu")
        self.behaviour_net = behaviour_net.to(self.device).eval()
        self.n_, self.obs_dim, self.act_dim = args.agent_num, args.obs_size, args.action_dim

    # -- N = 1, the reference's loop (tester.py:16-70) --------------------------------------------------------
    def _snapshot_single(self, record):
        e = self.env
        for key, fn in zip(RECORD_KEYS, (e._get_pv_active, e._get_pv_reactive, e._get_bus_active, e._get_bus_reactive,
                                         e._get_bus_v, e._get_ess_energy, e._get_power_reduction, e._get_ess_charging,
                                         e._get_ess_discharging, e._get_price)):
            record[key].append(fn())

    def _run_single(self, day, hour, quarter):
        state, _ = self.env.manual_reset(day, hour, quarter)
        last_hid = self.behaviour_net.policy_dicts[0].init_hidden()
        record = {k: [] for k in RECORD_KEYS}
        self._snapshot_single(record)
        avail = th.tensor(self.env.get_avail_actions())
        for t in range(self.args.max_steps):
            state_ = prep_obs(state).contiguous().view(1, self.n_, self.obs_dim).to(self.device)
            with th.no_grad():
                action, _, _, _, hid = self.behaviour_net.get_actions(state_, status="test", exploration=False,
                                                                      actions_avail=avail, target=False, last_hid=last_hid)
            _, actual = translate_action(self.args, action, self.env)
            _, done, _ = self.env.step(actual)
            self._snapshot_single(record)
            state, last_hid = self.env.get_obs(), hid
            if done or t == self.args.max_steps - 1:
                break
        return record

    # -- N envs at once -------------------------------------------------------------------------------------------
    def _snapshot_vec(self, record):
        v = self.env
        nb, na = v.n_bus, v.n_agents
        rows = v.series_dev.index_select(0, v.peek("ROW").long())                     # current data row per env
        record["bus_active"].append(rows[:, :nb].cpu().numpy())
        record["bus_reactive"].append(rows[:, nb:2 * nb].cpu().numpy())
        record["pv_active"].append(rows[:, 2 * nb:2 * nb + na].cpu().numpy())
        record["price"].append(rows[:, 2 * nb + na:].cpu().numpy())
        for key, field in (("pv_reactive", "QPV"), ("bus_voltage", "V"), ("ess_energy", "E"),
                           ("power_reduction", "PRED"), ("ess_charging", "CH"), ("ess_discharging", "DIS")):
            record[key].append(v.peek(field).cpu().numpy())

    def _run_vec(self, day, hour, quarter, e0=None, a0=None):
        v = self.env
        N = v.n_envs
        spec = dict(day=np.broadcast_to(np.asarray(day, np.int32), (N,)).copy(),
                    hour=np.broadcast_to(np.asarray(hour, np.int32), (N,)).copy(),
                    interval=np.broadcast_to(np.asarray(quarter, np.int32), (N,)).copy(), e0=e0, a0=a0)
        obs = v.reset(spec=spec).clone()
        if int(v.failed.sum().item()):
            raise RuntimeError("The power flow for the current initialization cannot be solved.")
        last_hid = th.zeros(N, self.n_, self.args.hid_size, device=self.device)
        avail = th.ones(N, self.n_, self.act_dim, device=self.device)
        record = {k: [] for k in RECORD_KEYS}
        record["actions"] = []                 # extra: what the env received, so a record can be re-simulated
        self._snapshot_vec(record)
        horizon = min(self.args.max_steps, v.episode_limit - 1)
        for t in range(horizon):
            with th.no_grad():
                action, _, _, _, hid = self.behaviour_net.get_actions(obs, status="test", exploration=False,
                                                                      actions_avail=avail, target=False, last_hid=last_hid)
                actual = self.behaviour_net.env_action(action)
            v.step(actual, fuse_obs=True)
            record["actions"].append(actual.cpu().numpy())
            self._snapshot_vec(record)
            obs, last_hid = v.obs.clone(), hid
        return record

    def _run_vec_traced(self, day, hour, quarter, e0=None, a0=None):
        """``_run_vec`` from the trace of ``Model.test_episodes``: one launch where the model is eligible, no host copy per
        step either way, and ONE gather of the series table by the traced rows at the end."""
        v = self.env
        N = v.n_envs
        spec = dict(day=np.broadcast_to(np.asarray(day, np.int32), (N,)).copy(),
                    hour=np.broadcast_to(np.asarray(hour, np.int32), (N,)).copy(),
                    interval=np.broadcast_to(np.asarray(quarter, np.int32), (N,)).copy(), e0=e0, a0=a0)
        res = self.behaviour_net.test_episodes(v, spec=spec, trace=True)
        tr = res.trace
        rows = np.concatenate([tr["row0"][None], tr["row"]], axis=0)              # [steps + 1, N]
        idx = th.as_tensor(rows.reshape(-1), device=v.series_dev.device).long()
        series_rows = v.series_dev.index_select(0, idx).cpu().numpy().reshape(rows.shape + (-1,))
        return record_from_trace(tr, series_rows)

    def run(self, day, hour, quarter, one_launch=False, **spec):
        """``one_launch`` (vectorised env only): the record from ``Model.test_episodes``' trace instead of the stepping loop."""
        if hasattr(self.env, "handle"):
            if one_launch:
                return self._run_vec_traced(day, hour, quarter, **spec)
            return self._run_vec(day, hour, quarter, **spec)
        return self._run_single(day, hour, quarter)
