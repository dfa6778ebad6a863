"""flexenv_rollout_burst_summed (the one-launch rollout burst of the agent-summed algorithms) without a GPU: the entry point's
export, declaration and ctypes binding, its struct's layout, the refusals that need no handle, and the plain burst's prototype,
which the new entry point must leave alone."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLEX_EINVAL = -22


@pytest.fixture(scope="module")
def lib():
    from safe_marl_amd import build, _lib
    build.build()
    return _lib.load()


def test_entry_point_is_declared_exported_and_bound(lib):
    from safe_marl_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "flexenv.h")).read()
    assert re.search(r"int\s+flexenv_rollout_burst_summed\s*\(", hdr)
    assert "flexenv_rollout_burst_summed" in _lib.SYMBOLS
    fn = lib.flexenv_rollout_burst_summed                       # (AttributeError: the library does not export it)
    assert fn.restype is C.c_int and len(fn.argtypes) == 10
    assert fn.argtypes[1] == C.POINTER(_lib.FlexActorArgs) and fn.argtypes[8] == C.POINTER(_lib.FlexBurstSummed)


def test_struct_layout():
    from safe_marl_amd import _lib
    assert C.sizeof(_lib.FlexBurstSummed) == 2 * 8 + 2 * 4
    assert [f[0] for f in _lib.FlexBurstSummed._fields_] == ["eps", "std", "act_low", "act_high"]
    assert (_lib.FlexBurstSummed.eps.offset, _lib.FlexBurstSummed.std.offset, _lib.FlexBurstSummed.act_low.offset,
            _lib.FlexBurstSummed.act_high.offset) == (0, 8, 16, 20)
    hdr = open(os.path.join(ROOT, "include", "flexenv.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\} FlexBurstSummed;", hdr).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert re.findall(r"(\w+)\s*[;,]", body) == ["eps", "std", "act_low", "act_high"]


@pytest.mark.parametrize("case", ["env", "actor", "summed", "eps", "std", "steps"])
def test_refusals_come_before_any_hip_call(lib, case):
    """On a machine without a device: FLEX_EINVAL, nothing launched.  Each case has ONE thing wrong: every other pointer, the
    handle included, is a non-NULL dummy that none of these refusals follows (the handle is first read behind all of them), so
    a case fails — or crashes — when its own check is removed or moved behind a dereference or a HIP call.  The refusals that
    read a live handle: tests/test_summed_burst_gpu.py."""
    from safe_marl_amd import _lib
    a = _lib.FlexActorArgs()
    a.rows, a.n_agents, a.obs_dim, a.act_dim = 10, 5, 144, 4
    sm = _lib.FlexBurstSummed()
    sm.eps, sm.std, sm.act_low, sm.act_high = 8, 8, 0.0, 1.0
    if case == "eps":
        sm.eps = None
    elif case == "std":
        sm.std = None
    rc = lib.flexenv_rollout_burst_summed(None if case == "env" else 8, None if case == "actor" else C.byref(a), 8, 8, 8, 8, 8,
                                          0 if case == "steps" else 4, None if case == "summed" else C.byref(sm), None)
    assert rc == FLEX_EINVAL


def test_plain_burst_keeps_its_prototype(lib):
    from safe_marl_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "flexenv.h")).read()
    proto = re.search(r"int\s+flexenv_rollout_burst\s*\(([^;]*)\)\s*;", hdr).group(1)
    proto = re.sub(r"/\*.*?\*/", "", proto, flags=re.S)
    assert len(proto.split(",")) == 10
    fn = lib.flexenv_rollout_burst
    assert len(fn.argtypes) == 10 and fn.argtypes[8] == C.POINTER(_lib.FlexBurstSafety)
    assert C.sizeof(_lib.FlexBurstSafety) == 8 * 8 + 2 * 4
