"""The block manager's prefix index under AddressSanitizer + UBSan and ThreadSanitizer: a
stand-alone driver (tests/native/kv_prefix_stress.cpp, its own ``main``) hammers publish, match,
reserve and release from 4 threads against a pool small enough to evict constantly, and runs the
manager's self-check (no referenced block on the free list, reference sums consistent)."""
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
HOST = ROOT / "lumen_amd" / "csrc" / "host"
DRIVER = Path(__file__).parent / "native" / "kv_prefix_stress.cpp"
CXX = shutil.which("g++")


@pytest.mark.skipif(CXX is None, reason="g++ not available")
@pytest.mark.parametrize("san", ["address,undefined", "thread"])
def test_kv_prefix_index_under_sanitizer(tmp_path, san):
    exe = tmp_path / f"kv_prefix_{san.split(',')[0]}"
    cmd = [CXX, "-std=c++17", "-O1", "-g", f"-fsanitize={san}", "-fno-omit-frame-pointer", "-pthread",
           str(DRIVER), str(HOST / "kv_blocks.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    env = {"ASAN_OPTIONS": "detect_leaks=1", "TSAN_OPTIONS": "halt_on_error=1"}
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300, env=env)
    setarch = shutil.which("setarch")
    if run.returncode != 0 and "unexpected memory mapping" in run.stderr and setarch:
        # the sanitizer runtime gave up before main(): its shadow layout does not fit this kernel's
        # address-space randomisation.  Same executable, randomisation off for this one process.
        run = subprocess.run([setarch, "-R", str(exe)], capture_output=True, text=True, timeout=300, env=env)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.startswith("ok hits=")
