"""The fp8 and 4-bit instantiations of the grouped expert GEMM (csrc/moe_wq.hip) keep their operand
fragments and accumulators in registers: every one of them must compile for gfx950 without scratch,
and there are exactly as many as the dispatcher launches.  CPU-only (hipcc)."""
import re
import shutil
import subprocess
from pathlib import Path

import pytest

CSRC = Path(__file__).resolve().parents[1] / "lumen_amd" / "csrc"
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


@pytest.mark.skipif(not Path(HIPCC).exists(), reason="hipcc not available")
def test_quantised_moe_kernels_do_not_spill():
    out = subprocess.run([HIPCC, "-x", "hip", "--offload-arch=gfx950", "-O3", "-std=c++17", "-c",
                          str(CSRC / "moe_wq.hip"), "-o", "/dev/null", "-Rpass-analysis=kernel-resource-usage"],
                         capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    names = re.findall(r"Function Name: (\S+)", out.stderr)
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", out.stderr)]
    assert names and len(names) == len(scratch), "moe_wq.hip: no kernels reported"
    # {gate|up, down} x {16, 64 rows} x {fp8, 4-bit G = 128, 4-bit G = 32}
    assert sum("moe_gemm_kernel" in n for n in names) == 12, names
    bad = [(n, s) for n, s in zip(names, scratch) if s > 0]
    assert not bad, f"kernels with scratch: {bad}"
