"""The mixture-of-experts kernels (csrc/moe.hip) keep their operand fragments, top-k lists and
accumulators in registers: like the kernels of test_sampler_resources_cpu.py every one of them must
compile for gfx950 without scratch.  CPU-only (hipcc)."""
import re
import shutil
import subprocess
from pathlib import Path

import pytest

CSRC = Path(__file__).resolve().parents[1] / "lumen_amd" / "csrc"
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


@pytest.mark.skipif(not Path(HIPCC).exists(), reason="hipcc not available")
def test_moe_kernels_do_not_spill():
    out = subprocess.run([HIPCC, "-x", "hip", "--offload-arch=gfx950", "-O3", "-std=c++17", "-c",
                          str(CSRC / "moe.hip"), "-o", "/dev/null", "-Rpass-analysis=kernel-resource-usage"],
                         capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    names = re.findall(r"Function Name: (\S+)", out.stderr)
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", out.stderr)]
    assert names and len(names) == len(scratch), "moe.hip: no kernels reported"
    for kernel in ("moe_gemm_kernel", "moe_topk_kernel", "moe_group_kernel", "moe_combine_kernel"):
        assert any(kernel in n for n in names), f"{kernel} not reported"
    assert sum("moe_gemm_kernel" in n for n in names) == 6, "router / gate|up / down x 16- and 64-row tiles"
    bad = [(n, s) for n, s in zip(names, scratch) if s > 0]
    assert not bad, f"kernels with scratch: {bad}"
