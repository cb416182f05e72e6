"""The device sampler's kernels keep row_topk's 64-deep register lists: like the hot kernels of
test_kernel_resources.py they must compile for gfx950 without scratch spills.  CPU-only (hipcc)."""
import re
import shutil
import subprocess
from pathlib import Path

import pytest

CSRC = Path(__file__).resolve().parents[1] / "lumen_amd" / "csrc"
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


@pytest.mark.skipif(not Path(HIPCC).exists(), reason="hipcc not available")
def test_sampler_kernels_do_not_spill():
    out = subprocess.run([HIPCC, "-x", "hip", "--offload-arch=gfx950", "-O3", "-std=c++17", "-c",
                          str(CSRC / "sampler.hip"), "-o", "/dev/null", "-Rpass-analysis=kernel-resource-usage"],
                         capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    names = re.findall(r"Function Name: (\S+)", out.stderr)
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", out.stderr)]
    assert names and len(names) == len(scratch), "sampler.hip: no kernels reported"
    assert any("sample_rows_kernel" in n for n in names)
    bad = [(n, s) for n, s in zip(names, scratch) if s > 0]
    assert not bad, f"kernels with scratch spills: {bad}"
