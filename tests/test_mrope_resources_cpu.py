"""The RoPE + KV-write kernels hold a thread's 8 or 16 rotation pairs (and, under the q / k norm, its
raw values and gammas) in registers; the multimodal form adds three table rows and the axis codes.
Like the kernels of test_paged_verify_resources_cpu.py every instantiation, the plain ones and the
MROPE ones, must compile for gfx950 without scratch spills.  CPU-only (hipcc)."""
import re
import shutil
import subprocess
from pathlib import Path

import pytest

CSRC = Path(__file__).resolve().parents[1] / "lumen_amd" / "csrc"
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


@pytest.mark.skipif(not Path(HIPCC).exists(), reason="hipcc not available")
def test_rope_kv_kernels_do_not_spill():
    out = subprocess.run([HIPCC, "-x", "hip", "--offload-arch=gfx950", "-O3", "-std=c++17", "-c",
                          str(CSRC / "llm.hip"), "-o", "/dev/null", "-Rpass-analysis=kernel-resource-usage"],
                         capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    names = re.findall(r"Function Name: (\S+)", out.stderr)
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", out.stderr)]
    assert names and len(names) == len(scratch), "llm.hip: no kernels reported"
    rope = {n: s for n, s in zip(names, scratch) if "rope_kv" in n}
    # mangled names: rope_kv_kernel<NORM, MROPE> is ...ILb?ELb?EE..., rope_kv_tile_kernel<D, NORM, MROPE>
    # ...ILi<D>ELb?ELb?EE...
    elem = sorted(re.search(r"rope_kv_kernelILb(\d)ELb(\d)EE", n).groups() for n in rope if "rope_kv_kernel" in n)
    tile = sorted(re.search(r"rope_kv_tile_kernelILi(\d+)ELb(\d)ELb(\d)EE", n).groups()
                  for n in rope if "rope_kv_tile_kernel" in n)
    flags = [(a, b) for a in "01" for b in "01"]
    assert elem == flags                                            # norm x mrope
    assert tile == [(d, a, b) for d in ("128", "64") for a, b in flags]    # head dims 64 / 128 x norm x mrope
    assert len(rope) == 12
    bad = {n: s for n, s in rope.items() if s > 0}
    assert not bad, f"kernels with scratch spills: {bad}"
