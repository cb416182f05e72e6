"""The paged-verify kernel carries up to four column tiles of running softmax state next to a whole
block's K and V fragments: like the hot kernels of test_kernel_resources.py every instantiation
must compile for gfx950 without scratch spills.  CPU-only (hipcc)."""
import re
import shutil
import subprocess
from pathlib import Path

import pytest

from lumen_amd.ops.llm import PAGED_VERIFY_MAX_COLS

CSRC = Path(__file__).resolve().parents[1] / "lumen_amd" / "csrc"
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


@pytest.mark.skipif(not Path(HIPCC).exists(), reason="hipcc not available")
def test_paged_verify_kernels_do_not_spill():
    out = subprocess.run([HIPCC, "-x", "hip", "--offload-arch=gfx950", "-O3", "-std=c++17", "-c",
                          str(CSRC / "llm.hip"), "-o", "/dev/null", "-Rpass-analysis=kernel-resource-usage"],
                         capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    names = re.findall(r"Function Name: (\S+)", out.stderr)
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", out.stderr)]
    assert names and len(names) == len(scratch), "llm.hip: no kernels reported"
    verify = [(n, s) for n, s in zip(names, scratch) if "paged_verify_kernel" in n]
    # head dims 32 / 64 / 128 x bf16 / fp8 cache x 1 / 2 / 4 column tiles
    assert len(verify) == 18 and PAGED_VERIFY_MAX_COLS == 64
    bad = [(n, s) for n, s in verify if s > 0]
    assert not bad, f"kernels with scratch spills: {bad}"
