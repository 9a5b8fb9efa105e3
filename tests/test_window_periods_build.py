"""What the window period trend compiles to, without a GPU: the planning header under host
sanitizers, and the kernel's compile-time resources for gfx950."""

import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
LDS_BYTES_PER_CU = 160 * 1024


def test_plan_header_under_sanitizers(tmp_path):
    """tools/periods_plan_check.cpp - a host-only program over the planning header the kernel
    compiles - built with AddressSanitizer and UBSan and run here."""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/lib/llvm/bin/clang++"
    exe = tmp_path / "periods_plan_check"
    build = subprocess.run(
        [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
         f"-I{ROOT}/csrc", os.path.join(ROOT, "tools", "periods_plan_check.cpp"), "-o", str(exe)],
        capture_output=True, text=True, timeout=600)
    assert build.returncode == 0, build.stderr[-3000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0 and "ok" in run.stdout, (run.stdout[-2000:], run.stderr[-2000:])


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_periods_kernel_has_no_scratch_and_fits_lds(tmp_path):
    """The check of test_kernel_resources.py for window_periods.hip: both epilogues of the kernel
    without scratch and within the LDS of a CU."""
    res = subprocess.run(
        [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", f"-I{ROOT}/csrc", "--cuda-device-only", "-c",
         os.path.join(ROOT, "csrc", "window_periods.hip"), "-o", str(tmp_path / "k.o"),
         "-Rpass-analysis=kernel-resource-usage"],
        capture_output=True, text=True, timeout=600,
    )
    assert res.returncode == 0, res.stderr[-3000:]
    kernels = {}
    name = None
    for line in res.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            kernels[name] = {}
            continue
        m = re.search(r"(ScratchSize \[bytes/lane\]|LDS Size \[bytes/block\]|VGPRs): (\d+)", line)
        if m and name is not None:
            kernels[name][m.group(1)] = int(m.group(2))
    assert len(kernels) == 2 and all("periods_ring_kernel" in k for k in kernels), res.stderr[-2000:]
    for k, r in kernels.items():
        assert r.get("ScratchSize [bytes/lane]", 0) == 0, (k, r)
        assert 0 < r.get("LDS Size [bytes/block]", 0) <= LDS_BYTES_PER_CU, (k, r)
