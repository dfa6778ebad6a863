"""CPU: the surface of the one-launch test-mode episodes (include/flexenv.h: flexenv_test_episodes) — declaration, binding,
argument checks that come before any HIP call, the per-episode statistics, the tester's record from a trace, the eligibility
decision and the example's command line.  Nothing here touches a GPU."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "examples"))
FLEX_EINVAL = -22


@pytest.fixture(scope="module")
def lib():
    from safe_marl_amd import build, _lib
    build.build()
    return _lib.load()


def test_entry_point_is_declared_exported_and_bound(lib):
    from safe_marl_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "flexenv.h")).read()
    assert "#define FLEX_ABI_VERSION 2" in hdr                       # an addition: no existing flag or ring changes meaning
    m = re.search(r"\bint\s+flexenv_test_episodes\s*\(([^;]*?)\)\s*;", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S), flags=re.S)
    assert m, "flexenv_test_episodes is not declared"
    n_params = len([p for p in m.group(1).split(",") if p.strip()])
    assert n_params == 7
    assert "flexenv_test_episodes" in _lib.SYMBOLS and hasattr(lib, "flexenv_test_episodes")
    assert len(lib.flexenv_test_episodes.argtypes) == n_params
    assert C.sizeof(_lib.FlexTestOut) == 2 * 8 + 7 * 8
    assert [f[0] for f in _lib.FlexTestOut._fields_] == ["sums", "length", "actions", "v", "agent", "row", "reward", "info", "flags"]


def _valid_call():
    """Arguments that pass every check that does not need a live handle (pointers are never followed before the checks end)."""
    from safe_marl_amd import _lib
    a = _lib.FlexActorArgs()
    a.rows, a.n_agents, a.obs_dim, a.act_dim = 10, 5, 144, 4
    out = _lib.FlexTestOut()
    out.sums, out.length = 8, 8
    return a, out


@pytest.mark.parametrize("case", ["env", "actor", "out", "sums", "length", "steps", "summed", "agents", "summed+safety", "safety act_dim"])
def test_refusals_come_before_any_hip_call(lib, case):
    """Every refusal of include/flexenv.h, on a machine without a device: FLEX_EINVAL, nothing launched.  (No handle can exist
    here: flexenv_create needs a device.  The same refusals on a live handle: tests/test_test_episodes_gpu.py.)"""
    from safe_marl_amd import _lib
    a, out = _valid_call()
    sf = None
    steps, summed = 95, 0
    if case == "sums":
        out.sums = None
    elif case == "length":
        out.length = None
    elif case == "steps":
        steps = 0
    elif case == "summed":
        summed = 2
    elif case == "agents":
        a.n_agents = 6
    elif case == "summed+safety":
        summed, sf = 1, _lib.FlexBurstSafety()
    elif case == "safety act_dim":
        a.act_dim, sf = 6, _lib.FlexBurstSafety()
    rc = lib.flexenv_test_episodes(None, None if case == "actor" else C.byref(a), steps, summed,
                                   C.byref(sf) if sf is not None else None, None if case == "out" else C.byref(out), None)
    assert rc == FLEX_EINVAL


def test_episode_stats_restates_the_reference_loop():
    """model.py:285-306 on a hand-made case with unequal lengths, one episode of a single step among them: per episode the
    sums over its own steps divided by its own length t + 1, then the mean over episodes."""
    from safe_marl_amd._lib import INFO_KEYS
    from safe_marl_amd.learner import episode_stats
    rng = np.random.default_rng(0)
    lengths = [95, 1, 7, 40]
    steps = [[(dict(zip(INFO_KEYS, rng.normal(size=7))), float(rng.normal())) for _ in range(n)] for n in lengths]
    # the loop of model.py:272-306, literally (info and reward per step instead of an env)
    stat_test = {}
    for epi in steps:
        stat_test_epi = {"mean_test_reward": 0}
        for t, (info, reward) in enumerate(epi):
            for k, v in info.items():
                if "mean_test_" + k not in stat_test_epi.keys():
                    stat_test_epi["mean_test_" + k] = v
                else:
                    stat_test_epi["mean_test_" + k] += v
            stat_test_epi["mean_test_reward"] += reward
        for k, v in stat_test_epi.items():
            stat_test_epi[k] = v / float(t + 1)
        for k, v in stat_test_epi.items():
            if k not in stat_test.keys():
                stat_test[k] = v
            else:
                stat_test[k] += v
    for k, v in stat_test.items():
        stat_test[k] = v / float(len(steps))
    sums = np.zeros((len(lengths), 10))
    for i, epi in enumerate(steps):
        for info, reward in epi:                                       # step order, one accumulator per figure
            sums[i, :7] += [info[k] for k in INFO_KEYS]
            sums[i, 7] += reward
            sums[i, 8] += 1.0 if info["voltage_penalty"] > 0 else 0.0
    got = episode_stats(sums, np.array(lengths, np.int32))
    assert set(stat_test) <= set(got) and set(got) - set(stat_test) == {"mean_test_violation_rate", "mean_test_solver_failed"}
    for k, v in stat_test.items():
        # the same additions; mean_test_reward's two series are summed apart here and interleaved there: fp64 reassociation
        # of 2 * 95 terms of size ~1, far below 1e-12 relative to their absolute sum
        assert abs(got[k] - v) <= 1e-12 * max(1.0, abs(v)), (k, got[k], v)
    viol = np.mean([sums[i, 8] / lengths[i] for i in range(4)])
    assert abs(got["mean_test_violation_rate"] - viol) < 1e-15 and got["mean_test_solver_failed"] == 0.0
    # not the mean over env-steps: the single-step episode weighs as much as the 95-step one
    assert abs(got["mean_test_revenue"] - sums[:, 1].sum() / sum(lengths)) > 1e-3
    with pytest.raises(ValueError):
        episode_stats(sums, np.array([95, 0, 7, 40]))


def test_record_from_trace_keys_counts_and_shapes():
    from safe_marl_amd.tester import RECORD_KEYS, record_from_trace
    steps, n, nb, na = 6, 3, 33, 5
    rng = np.random.default_rng(1)
    trace = dict(v0=rng.random((n, nb)), agent0=rng.random((n, na, 5)), row0=np.arange(n, dtype=np.int32),
                 v=rng.random((steps, n, nb)), agent=rng.random((steps, n, na, 5)),
                 row=rng.integers(0, 50, (steps, n)).astype(np.int32), actions=rng.random((steps, n, na, 4)).astype(np.float32),
                 reward=rng.random((steps, n)), info=rng.random((steps, n, 7)), flags=np.full((steps, n), 4, np.uint8))
    series_rows = rng.random((steps + 1, n, 2 * nb + na + 1))
    rec = record_from_trace(trace, series_rows)
    assert set(rec) == set(RECORD_KEYS) | {"actions"}
    for k in RECORD_KEYS:
        assert len(rec[k]) == steps + 1, k
    assert len(rec["actions"]) == steps and rec["actions"][0].shape == (n, na, 4)
    shapes = dict(pv_active=(n, na), pv_reactive=(n, na), bus_active=(n, nb), bus_reactive=(n, nb), bus_voltage=(n, nb),
                  ess_energy=(n, na), power_reduction=(n, na), ess_charging=(n, na), ess_discharging=(n, na), price=(n, 1))
    for k, shp in shapes.items():
        assert all(x.shape == shp for x in rec[k]), k
    assert np.array_equal(rec["bus_voltage"][0], trace["v0"]) and np.array_equal(rec["bus_voltage"][3], trace["v"][2])
    assert np.array_equal(rec["ess_energy"][4], trace["agent"][3][..., 0])
    assert np.array_equal(rec["power_reduction"][1], trace["agent"][0][..., 1])
    assert np.array_equal(rec["ess_charging"][1], trace["agent"][0][..., 2])
    assert np.array_equal(rec["ess_discharging"][1], trace["agent"][0][..., 3])
    assert np.array_equal(rec["pv_reactive"][0], trace["agent0"][..., 4])
    assert np.array_equal(rec["bus_reactive"][2], series_rows[2][:, nb:2 * nb])
    assert np.array_equal(rec["pv_active"][2], series_rows[2][:, 2 * nb:2 * nb + na])
    assert np.array_equal(rec["price"][5], series_rows[5][:, -1:])
    with pytest.raises(ValueError):
        record_from_trace(trace, series_rows[:-1])


def _model(alg="maddpg", n=5, **over):
    import torch
    from train_maddpg import DEFAULT_ALG_ARGS, PPO_ALG_ARGS
    from safe_marl_amd import learner
    from safe_marl_amd.util import convert
    d = dict(DEFAULT_ALG_ARGS)
    if alg == "ippo":
        d.update(PPO_ALG_ARGS)
    d.update(alg=alg, agent_num=n, obs_size=144, state_size=110, action_dim=4, cuda=False, v_min=0.9, v_max=1.1)
    d.update(over)
    torch.manual_seed(0)
    cls = {"maddpg": learner.MADDPG, "matd3": learner.MATD3, "ippo": learner.IPPO, "safemaddpg": learner.SAFEMADDPG}[alg]
    if alg == "safemaddpg":
        z = torch.zeros(n, dtype=torch.float64)
        return cls(convert(d), None, predictor=(z, z, z))
    return cls(convert(d))


def test_eligibility_gives_a_reason_or_none():
    from safe_marl_amd.learner import one_launch_declines
    for alg in ("maddpg", "matd3", "ippo", "safemaddpg"):
        assert one_launch_declines(_model(alg)) is None, alg
    assert one_launch_declines(_model(gaussian_policy=True)) is None              # the mean head sits in the fc2 slot
    assert "agent_type mlp" in one_launch_declines(_model(agent_type="mlp"))
    assert "shared_params" in one_launch_declines(_model(shared_params=False))
    assert "7 agents" in one_launch_declines(_model(n=7))
    assert "action_enforcebound" in one_launch_declines(_model(action_enforcebound=False))
    safe = _model("safemaddpg")
    safe.intended_actions = True
    assert "intended_actions" in one_launch_declines(safe)
    with pytest.raises(ValueError, match="agent_type mlp"):
        _model(agent_type="mlp").test_episodes(_NoEnv(), one_launch=True)


class _NoEnv:
    """Stands where an environment would: the refusal comes before anything of it but these attributes is read."""
    episode_limit = 96

    class obs:
        is_cuda = False


def test_example_and_tools_parse_their_arguments():
    for script, words in ((os.path.join("examples", "test_policy.py"), ("--alg", "--agents", "--load", "--days", "--trace-out")),
                          (os.path.join("tools", "learning_curve.py"), ("--one-launch",)),
                          (os.path.join("tools", "test_episodes_bench.py"), ("--envs",))):
        out = subprocess.run([sys.executable, os.path.join(ROOT, script), "--help"], capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stderr
        for w in words:
            assert w in out.stdout, (script, w)


def test_new_kernels_resource_usage_and_the_existing_ones():
    """The launch is three new instantiations; the compiler's report for them (DESIGN.md §4 quotes it) and for the burst they are
    modelled on, whose own figures this pull request must not move."""
    from safe_marl_amd import build
    build.build()
    new = build.kernel_resources("flex_test_episodes_kernel")
    assert sorted(v["name"] for v in new.values()) == [f"flex_test_episodes_kernel<{m}>" for m in range(3)]
    burst = build.kernel_resources("flex_rollout_burst_kernel")
    assert len(burst) == 4
    for v in list(new.values()) + list(burst.values()):
        print(f"{v['name']}: {v['vgprs']} VGPRs + {v['agprs']} AGPRs, {v['sgprs']} SGPRs, LDS {v['lds_bytes_per_block']} B, "
              f"{v['waves_per_simd']} waves/SIMD, scratch {v['scratch_bytes_per_lane']} B/lane")
    for v in burst.values():                                           # as at the parent commit
        safe = v["name"].endswith("true>")
        assert (v["vgprs"], v["agprs"], v["lds_bytes_per_block"], v["scratch_bytes_per_lane"], v["waves_per_simd"]) == \
               (256, 0, 153648, 20 if safe else 16, 2), v
    for v in new.values():                                             # the burst's footprint: no more scratch than its SAFE form
        assert v["vgprs"] <= 256 and v["agprs"] == 0 and v["lds_bytes_per_block"] == 153648 and v["waves_per_simd"] == 2
        assert v["scratch_bytes_per_lane"] <= 20, v
