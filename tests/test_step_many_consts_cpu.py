"""Cross-build checks (no GPU) of flex_step_many_kernel's constants block (FLEX_MANY_CONSTS, csrc/flexenv.hip): the switch
builds out, alone and with every other FLEX_MANY_* item, and the default build's four instantiations need no more registers
than they did before the block — the loop runs at exactly two wavefronts per SIMD with three vector registers to spare."""
import os
import subprocess

import pytest

# VGPRs of the four instantiations before the constants block ("The solve's table constants")
PARENT_VGPRS = {
    "flex_step_many_kernel<2, float>": 249,
    "flex_step_many_kernel<2, double>": 253,
    "flex_step_many_kernel<1, float>": 244,
    "flex_step_many_kernel<1, double>": 248,
}
SWITCHES = ["FLEX_MANY_CONSTS", "FLEX_MANY_PREFETCH_ACT", "FLEX_MANY_EARLY_HEAD", "FLEX_MANY_HDR_REGS"]


@pytest.mark.parametrize("off", ["FLEX_MANY_CONSTS", "all"])
def test_the_env_kernels_compile_with_the_block_built_out(tmp_path, off):
    from safe_marl_amd import build
    defs = [f"-D{m}=0" for m in (SWITCHES if off == "all" else [off])]
    src = os.path.join(build.CSRC, "flexenv.hip")
    cmd = [build.HIPCC] + build.CFLAGS + defs + ["-c", src, "-o", str(tmp_path / "flexenv.o")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]


def test_the_four_instantiations_need_no_more_registers_than_before():
    from safe_marl_amd import build
    build.build()
    ks = {v["name"]: v for v in build.kernel_resources("flex_step_many_kernel<").values()}
    assert set(ks) == set(PARENT_VGPRS)
    for name, vgprs in PARENT_VGPRS.items():
        v = ks[name]
        print(name, v["vgprs"], v.get("agprs", 0), v["sgprs"], v.get("sgpr_spills"), v["waves_per_simd"])
        assert v["vgprs"] + v.get("agprs", 0) <= vgprs, (name, v)
        assert v["scratch_bytes_per_lane"] == 0 and v.get("vgpr_spills", 0) == 0, (name, v)
        assert v["waves_per_simd"] >= 2, (name, v)
