"""What the three lag kernels (window autocorrelation, cross-correlation, period trend) compile
to for gfx950, without a GPU: no scratch, and the two facts their launch rules rest on - at most
256 VGPRs, so two waves share a SIMD, and LDS for two workgroups per CU."""

import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
LDS_BYTES_PER_CU = 160 * 1024
MAX_VGPRS_TWO_WAVES = 256

# source in csrc/ (without .hip) -> the kernels it must hold (substrings of the mangled names)
LAG_KERNELS = {
    "window_autocorr": ["autocorr_ring_kernel"],
    "window_xcorr": ["xcorr_ring_kernel"],
    "window_periods": ["periods_ring_kernelILb1EE", "periods_ring_kernelILb0EE"],
}


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
@pytest.mark.parametrize("source", sorted(LAG_KERNELS))
def test_lag_kernels_have_no_scratch_and_fit_two_per_cu(source, tmp_path):
    """The check of test_kernel_resources.py for the lag sources: every kernel (both epilogues of
    the period trend's) without scratch and within the LDS of a CU, and beyond it the occupancy
    the design states: VGPRs <= 256 and twice the LDS <= 160 KiB."""
    res = subprocess.run(
        [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", f"-I{ROOT}/csrc", "--cuda-device-only", "-c",
         os.path.join(ROOT, "csrc", source + ".hip"), "-o", str(tmp_path / "k.o"),
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
    want = LAG_KERNELS[source]
    assert len(kernels) == len(want) and all(any(w in k for k in kernels) for w in want), res.stderr[-2000:]
    for k, r in kernels.items():
        assert r.get("ScratchSize [bytes/lane]", 0) == 0, (k, r)
        assert 0 < r.get("LDS Size [bytes/block]", 0) <= LDS_BYTES_PER_CU, (k, r)
        assert 0 < r.get("VGPRs", 0) <= MAX_VGPRS_TWO_WAVES, (k, r)
        assert 2 * r["LDS Size [bytes/block]"] <= LDS_BYTES_PER_CU, (k, r)
