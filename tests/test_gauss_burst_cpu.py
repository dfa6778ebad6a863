"""flexenv_rollout_burst_summed_gauss (the one-launch rollout burst of the agent-summed algorithms with a shared Gaussian actor)
without a GPU: the entry point's export, declaration and ctypes binding, its struct's layout, the refusals that need no handle,
the prototypes and structs it must leave alone, the compiler's resource report of the new kernel, and the example's flag."""
import ctypes as C
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLEX_EINVAL = -22
FIELDS = ["eps", "log_std_w", "log_std_b", "log_stds", "log_std_min", "log_std_max", "act_low", "act_high"]


@pytest.fixture(scope="module")
def lib():
    from safe_marl_amd import build, _lib
    build.build()
    return _lib.load()


def _header():
    return open(os.path.join(ROOT, "include", "flexenv.h")).read()


def _proto_args(name):
    proto = re.search(r"int\s+" + name + r"\s*\(([^;]*)\)\s*;", _header()).group(1)
    return re.sub(r"/\*.*?\*/", "", proto, flags=re.S).split(",")


def test_entry_point_is_declared_exported_and_bound(lib):
    from safe_marl_amd import _lib
    assert re.search(r"int\s+flexenv_rollout_burst_summed_gauss\s*\(", _header())
    assert len(_proto_args("flexenv_rollout_burst_summed_gauss")) == 10
    assert "flexenv_rollout_burst_summed_gauss" in _lib.SYMBOLS
    fn = lib.flexenv_rollout_burst_summed_gauss                 # (AttributeError: the library does not export it)
    assert fn.restype is C.c_int and len(fn.argtypes) == 10
    assert fn.argtypes[1] == C.POINTER(_lib.FlexActorArgs) and fn.argtypes[8] == C.POINTER(_lib.FlexBurstSummedGauss)


def test_struct_layout():
    from safe_marl_amd import _lib
    S = _lib.FlexBurstSummedGauss
    assert C.sizeof(S) == 4 * 8 + 4 * 4
    assert [f[0] for f in S._fields_] == FIELDS
    assert [getattr(S, f).offset for f in FIELDS] == [0, 8, 16, 24, 32, 36, 40, 44]
    body = re.search(r"typedef struct \{([^}]*)\} FlexBurstSummedGauss;", _header()).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert re.findall(r"(\w+)\s*[;,]", body) == FIELDS
    # pointers are declared as pointers, the ranges as floats
    assert len(re.findall(r"\*\s*\w+\s*;", body)) == 4 and len(re.findall(r"float\s+\w+\s*,\s*\w+\s*;", body)) == 2


@pytest.mark.parametrize("case", ["env", "actor", "gauss", "eps", "log_std_w", "log_std_b", "log_stds", "log_std_range",
                                  "log_std_nan", "act_range", "act_dim", "n_agents", "steps"])
def test_refusals_come_before_any_hip_call(lib, case):
    """On a machine without a device: FLEX_EINVAL, nothing launched.  Each case has ONE thing wrong: every other pointer, the
    handle included, is a non-NULL dummy that none of these refusals follows (the handle is first read behind all of them), so
    a case fails — or crashes — when its own check is removed or moved behind a dereference or a HIP call.  The refusals that
    read a live handle: tests/test_gauss_burst_gpu.py."""
    from safe_marl_amd import _lib
    a = _lib.FlexActorArgs()
    a.rows, a.n_agents, a.obs_dim, a.act_dim = 10, 5, 144, 4
    sg = _lib.FlexBurstSummedGauss()
    sg.eps, sg.log_std_w, sg.log_std_b, sg.log_stds = 8, 8, 8, 8
    sg.log_std_min, sg.log_std_max, sg.act_low, sg.act_high = 0.0, 0.5, 0.0, 1.0
    if case in ("eps", "log_std_w", "log_std_b", "log_stds"):
        setattr(sg, case, None)
    elif case == "log_std_range":
        sg.log_std_min, sg.log_std_max = 0.5, 0.0
    elif case == "log_std_nan":
        sg.log_std_max = float("nan")
    elif case == "act_range":
        sg.act_low, sg.act_high = 1.0, 0.0
    elif case == "act_dim":
        a.act_dim = 3
    elif case == "n_agents":
        a.rows, a.n_agents = 12, 6
    rc = lib.flexenv_rollout_burst_summed_gauss(None if case == "env" else 8, None if case == "actor" else C.byref(a), 8, 8, 8,
                                                8, 8, 0 if case == "steps" else 4, None if case == "gauss" else C.byref(sg),
                                                None)
    assert rc == FLEX_EINVAL


def test_plain_and_summed_bursts_keep_their_prototypes_and_structs(lib):
    from safe_marl_amd import _lib
    for name, struct in (("flexenv_rollout_burst", _lib.FlexBurstSafety), ("flexenv_rollout_burst_summed", _lib.FlexBurstSummed)):
        assert len(_proto_args(name)) == 10
        fn = getattr(lib, name)
        assert len(fn.argtypes) == 10 and fn.argtypes[8] == C.POINTER(struct)
    assert C.sizeof(_lib.FlexBurstSafety) == 8 * 8 + 2 * 4
    assert C.sizeof(_lib.FlexBurstSummed) == 2 * 8 + 2 * 4
    assert [f[0] for f in _lib.FlexBurstSummed._fields_] == ["eps", "std", "act_low", "act_high"]
    body = re.search(r"typedef struct \{([^}]*)\} FlexBurstSummed;", _header()).group(1)
    assert re.findall(r"(\w+)\s*[;,]", re.sub(r"/\*.*?\*/", "", body, flags=re.S)) == ["eps", "std", "act_low", "act_high"]


def test_resources_of_the_new_kernel():
    """The new form is two instantiations under a name of its own (the set under flex_rollout_burst_kernel< is pinned by other
    tests); the burst's LDS image and occupancy, no AGPRs, and no more scratch than the largest of the existing burst forms —
    that figure read from this build."""
    from safe_marl_amd import build
    build.build()
    new = build.kernel_resources("summed_gauss::flex_rollout_burst_kernel<")
    assert sorted(v["name"] for v in new.values()) == [f"summed_gauss::flex_rollout_burst_kernel<{c}>" for c in (5, 8)]
    old = {**build.kernel_resources("flex_rollout_burst_kernel<"), **build.kernel_resources("summed::flex_rollout_burst_kernel<")}
    assert len(old) == 6
    most = max(v["scratch_bytes_per_lane"] for v in old.values())
    for v in list(new.values()) + list(old.values()):
        print(f"{v['name']}: {v['vgprs']} VGPRs + {v['agprs']} AGPRs, {v['sgprs']} SGPRs, LDS {v['lds_bytes_per_block']} B, "
              f"{v['waves_per_simd']} waves/SIMD, scratch {v['scratch_bytes_per_lane']} B/lane")
    for v in new.values():
        assert v["lds_bytes_per_block"] == 153648 and v["waves_per_simd"] == 2 and v["agprs"] == 0, v
        assert v["vgprs"] <= 256 and v["scratch_bytes_per_lane"] <= most, (v, most)
    for v in old.values():                                      # the existing forms keep the image
        assert v["lds_bytes_per_block"] == 153648 and v["waves_per_simd"] == 2


@pytest.mark.parametrize("argv", [["--alg", "ippo", "--gauss-burst"], ["--alg", "maddpg", "--gaussian-policy", "--gauss-burst"],
                                  ["--alg", "maac", "--gauss-burst"]])
def test_example_refuses_the_flag_outside_its_configuration(argv):
    """--gauss-burst without --gaussian-policy, or with an algorithm that is not agent-summed: argparse's error, status 2, before
    anything touches a device."""
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "train_maddpg.py")] + argv, capture_output=True,
                         text=True, timeout=120)
    assert out.returncode == 2, out.stderr[-500:]
    assert "--gauss-burst" in out.stderr and "--gaussian-policy" in out.stderr
