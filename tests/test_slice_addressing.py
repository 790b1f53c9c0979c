"""The addressing every strided reduction shares (slice_row_bases / slice_row_base / slice_elem_off in rten_amd/csrc/slice.h), host side: the same functions compiled by
hipcc for the host and compared with a naive unravel-and-dot-product over 0 to 6 levels, extents 1, 2, 3, 7 and 16, zero and non-monotone strides, both
stride lists of a two-list description, and a row count above 2^31 (the 64-bit branch).  No GPU, no memory touched."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_row_base_and_elem_off_agree_with_unravel_and_dot():
    src = os.path.join(ROOT, "tests", "cpp", "test_slice.hip")
    out = os.path.join(ROOT, "tests", "cpp", "_build", "test_slice")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O2", "-std=c++17", "-w", src, "-o", out])
    r = subprocess.run([out], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and " 0 mismatches" in r.stdout, r.stdout + r.stderr
