"""Register budget of the step kernels after a cross-build (no GPU): flex_step_many_kernel carries the next step's actions
across the solve, which the kernel had avoided; it must still fit two wavefronts per SIMD without scratch, and the kernels
that share flex_step_body must not pay for it."""
import os
import subprocess

import pytest

# safe-marl_amd/kernel_resources.json of commit 63bd014 (the parent of the change that added the action prefetch)
PARENT = "63bd014"
# per instantiation: (VGPRs + AGPRs, SGPRs, SGPR spills, VGPR spills, scratch bytes per lane, waves per SIMD)
PARENT_KERNELS = {
    "flex_rollout_burst_kernel<5, false>": (256, 106, 161, 3, 16, 2),
    "flex_rollout_burst_kernel<5, true>": (256, 106, 171, 4, 20, 2),
    "flex_rollout_burst_kernel<8, false>": (256, 106, 161, 3, 16, 2),
    "flex_rollout_burst_kernel<8, true>": (256, 106, 171, 4, 20, 2),
    "flex_step_kernel<1, double, double, 5, false, false>": (193, 106, 17, 0, 0, 2),
    "flex_step_kernel<1, double, double, 8, false, false>": (193, 106, 17, 0, 0, 2),
    "flex_step_kernel<1, double, float, 5, false, false>": (193, 106, 17, 0, 0, 2),
    "flex_step_kernel<1, double, float, 8, false, false>": (193, 106, 17, 0, 0, 2),
    "flex_step_kernel<1, float, double, 5, false, false>": (195, 106, 17, 0, 0, 2),
    "flex_step_kernel<1, float, double, 5, false, true>": (192, 106, 19, 0, 0, 2),
    "flex_step_kernel<1, float, double, 8, false, false>": (195, 106, 19, 0, 0, 2),
    "flex_step_kernel<1, float, float, 5, false, false>": (195, 106, 17, 0, 0, 2),
    "flex_step_kernel<1, float, float, 5, false, true>": (192, 106, 19, 0, 0, 2),
    "flex_step_kernel<1, float, float, 8, false, false>": (195, 106, 19, 0, 0, 2),
    "flex_step_kernel<2, double, double, 5, false, false>": (199, 106, 11, 0, 0, 2),
    "flex_step_kernel<2, double, double, 8, false, false>": (212, 106, 11, 0, 0, 2),
    "flex_step_kernel<2, double, float, 5, false, false>": (199, 106, 11, 0, 0, 2),
    "flex_step_kernel<2, double, float, 8, false, false>": (212, 106, 11, 0, 0, 2),
    "flex_step_kernel<2, float, double, 5, false, false>": (201, 106, 11, 0, 0, 2),
    "flex_step_kernel<2, float, double, 5, false, true>": (198, 106, 15, 0, 0, 2),
    "flex_step_kernel<2, float, double, 8, false, false>": (214, 106, 11, 0, 0, 2),
    "flex_step_kernel<2, float, float, 5, false, false>": (201, 106, 11, 0, 0, 2),
    "flex_step_kernel<2, float, float, 5, false, true>": (198, 106, 15, 0, 0, 2),
    "flex_step_kernel<2, float, float, 5, true, true>": (199, 106, 16, 0, 0, 2),
    "flex_step_kernel<2, float, float, 8, false, false>": (214, 106, 11, 0, 0, 2),
}


def _resources(prefix):
    from safe_marl_amd import build
    build.build()
    ks = build.kernel_resources(prefix)
    assert ks, prefix
    return {v["name"]: v for v in ks.values()}


def test_step_many_kernels_fit_two_wavefronts_per_simd_without_scratch():
    ks = _resources("flex_step_many_kernel<")
    assert set(ks) == {"flex_step_many_kernel<1, float>", "flex_step_many_kernel<1, double>",
                       "flex_step_many_kernel<2, float>", "flex_step_many_kernel<2, double>"}
    for name, v in ks.items():
        print(name, v["vgprs"], v["sgprs"], v.get("sgpr_spills"), v["waves_per_simd"])
        assert v["scratch_bytes_per_lane"] == 0 and v.get("vgpr_spills", 0) == 0, name
        assert v["vgprs"] + v.get("agprs", 0) <= 256, name
        assert v["waves_per_simd"] >= 2, name


def test_kernels_sharing_the_step_body_are_no_worse_than_the_parent():
    ks = {**_resources("flex_step_kernel<"), **_resources("flex_rollout_burst_kernel<")}
    assert set(ks) == set(PARENT_KERNELS), (PARENT, sorted(set(ks) ^ set(PARENT_KERNELS)))
    for name, (regs, sgprs, sspills, vspills, scratch, waves) in PARENT_KERNELS.items():
        v = ks[name]
        print(name, v["vgprs"], v.get("agprs", 0), v["sgprs"], v.get("sgpr_spills", 0), v.get("vgpr_spills", 0),
              v["scratch_bytes_per_lane"], v["waves_per_simd"])
        assert v["vgprs"] + v.get("agprs", 0) <= regs and v["sgprs"] <= sgprs, (PARENT, name, v)
        assert v.get("sgpr_spills", 0) <= sspills and v.get("vgpr_spills", 0) <= vspills, (PARENT, name, v)
        assert v["scratch_bytes_per_lane"] <= scratch and v["waves_per_simd"] >= waves, (PARENT, name, v)


@pytest.mark.parametrize("off", ["FLEX_MANY_PREFETCH_ACT", "FLEX_MANY_EARLY_HEAD", "all"])
def test_env_kernels_compile_with_each_loop_item_built_out(tmp_path, off):
    from safe_marl_amd import build
    macros = ["FLEX_MANY_PREFETCH_ACT", "FLEX_MANY_EARLY_HEAD"]
    defs = [f"-D{m}=0" for m in (macros if off == "all" else [off])]
    src = os.path.join(build.CSRC, "flexenv.hip")
    cmd = [build.HIPCC] + build.CFLAGS + defs + ["-c", src, "-o", str(tmp_path / "flexenv.o")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
