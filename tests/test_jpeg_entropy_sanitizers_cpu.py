"""Host sanitizer + fuzz build of the GPU entropy decoder's host-side code: the scan front end
(csrc/jpeg.cpp rdp_jpeg_scan) and the per-lane decode core the HIP kernels run (csrc/jpeg_sync.h) through
its CPU emulation, on bytes a client controls.

tests/native/jpeg_sync_fuzz_main.cpp -- a stand-alone program -- is compiled with AddressSanitizer +
UndefinedBehaviorSanitizer and fed a marker-less baseline JPEG plus 1,500 deterministic mutants, with the
scan and coefficient buffers sized exactly from the headers; it also checks the emulation's verdict and
coefficients against the serial decoder on every mutant the front end takes.
"""
import io
import os
import shutil
import subprocess

import numpy as np
import pytest
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = [os.path.join(ROOT, "csrc", "jpeg.cpp"), os.path.join(ROOT, "tests", "native", "jpeg_sync_fuzz_main.cpp")]


def _frame(h, w, seed=0):
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    base = np.stack([(x * 255 // max(w - 1, 1)), (y * 255 // max(h - 1, 1)), ((x + y) * 3) % 256], -1)
    return np.clip(base + rng.integers(-40, 40, (h, w, 3)), 0, 255).astype(np.uint8)


@pytest.mark.skipif(shutil.which("g++") is None, reason="no host C++ compiler")
def test_scan_and_sync_core_address_undefined_fuzz(tmp_path):
    seed = tmp_path / "seed.jpg"
    buf = io.BytesIO()
    Image.fromarray(_frame(48, 80, 1), "RGB").save(buf, format="JPEG", quality=90, subsampling=2)
    seed.write_bytes(buf.getvalue())
    exe = str(tmp_path / "jpeg_sync_fuzz")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-fno-omit-frame-pointer", *SRC, "-lpthread", "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    if b.returncode != 0 and "asan" in (b.stderr or "").lower():
        pytest.skip("sanitizer runtime not installed: " + b.stderr[-200:])
    assert b.returncode == 0, b.stderr
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1", RDP_HOST_THREADS="2")
    r = subprocess.run([exe, str(seed), "1500"], capture_output=True, text=True, timeout=900, env=env)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert " 0 failures" in r.stdout, r.stdout
    # the mutants reach the entropy stage, with both verdicts
    took, equal, corrupt = (int(r.stdout.split(k)[1].split()[0].rstrip(";,)")) for k in
                            ("front end took ", "serial decode: ", "corrupt for both: "))
    assert took > 700 and equal > 100 and corrupt > 100, r.stdout
