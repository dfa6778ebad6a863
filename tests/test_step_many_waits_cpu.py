"""Cross-build (no GPU): flexenv.hip compiles with the step-many loop's header-scalar item built out — the -DFLEX_MANY_HDR_REGS=0
form the A/B measurements of DESIGN §4.2a are taken with — and with every loop item off."""
import os
import subprocess

import pytest

MACROS = ["FLEX_MANY_HDR_REGS", "FLEX_MANY_PREFETCH_ACT", "FLEX_MANY_EARLY_HEAD"]


@pytest.mark.parametrize("off", ["FLEX_MANY_HDR_REGS", "all"])
def test_env_kernels_compile_with_the_header_item_built_out(tmp_path, off):
    from safe_marl_amd import build
    defs = [f"-D{m}=0" for m in (MACROS if off == "all" else [off])]
    src = os.path.join(build.CSRC, "flexenv.hip")
    cmd = [build.HIPCC] + build.CFLAGS + defs + ["-c", src, "-o", str(tmp_path / "flexenv.o")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
