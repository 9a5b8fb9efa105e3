"""The window period trend's planning header under host sanitizers, without a GPU. The kernel's
compile-time resources are checked with the other lag kernels' in test_window_lag_build.py."""

import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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
