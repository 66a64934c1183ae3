"""The source-compatible C++ layer (vision::Tensor, va_cv::) in libvacv.so.

CPU: the library exports the reference's API (cv.h:85-239, tensor.h:27-84),
host Tensor semantics hold, and every operator fails loudly without a GPU.
GPU: tests/cpp/vacv_api_test -- the reference harness's cases
(src/test/src/test_main.cpp) on the reference's own test images, each scored
with ImageUtil::compare_image_data (cosine >= 1 - 5e-4, cv_profile.cpp:10)
AND the build's exact bar against the oracle.
"""
from __future__ import annotations

import json
import subprocess
from pathlib import Path

import numpy as np
import pytest

from conftest import GOLDEN, PKG, REPO

API_LIB = PKG / "lib" / "libvacv.so"
HARNESS = REPO / "tests" / "cpp" / "build" / "vacv_api_test"

# demangled prefixes every caller of the reference API links against
EXPORTS = [
    "va_cv::resize(vision::Tensor const&, vision::Tensor&, va_cv::VSize, double, double, int)",
    "va_cv::cvt_color(vision::Tensor const&, vision::Tensor&, int)",
    "va_cv::normalize(vision::Tensor const&, vision::Tensor&, vision::Tensor const&, vision::Tensor const&)",
    "va_cv::warp_affine(vision::Tensor const&, vision::Tensor&, vision::Tensor const&, va_cv::VSize, int, int, "
    "va_cv::VScalar const&)",
    "va_cv::warp_affine(vision::Tensor const&, vision::Tensor&, float, float, va_cv::VSize, va_cv::VScalar const&, "
    "int, int, va_cv::VScalar const&)",
    "va_cv::resize_normalize(vision::Tensor const&, vision::Tensor&, va_cv::VSize, double, double, int, "
    "vision::Tensor const&, vision::Tensor const&)",
    "va_cv::warp_affine_normalize(vision::Tensor const&, vision::Tensor&, vision::Tensor const&, va_cv::VSize, int, "
    "int, va_cv::VScalar const&, vision::Tensor const&, vision::Tensor const&)",
    "va_cv::warp_affine_normalize(vision::Tensor const&, vision::Tensor&, float, float, va_cv::VSize, "
    "va_cv::VScalar const&, int, int, va_cv::VScalar const&, vision::Tensor const&, vision::Tensor const&)",
    "va_cv::crop(vision::Tensor const&, vision::Tensor&, vision::VRect const&)",
    "va_cv::match_template(vision::Tensor const&, vision::Tensor const&, vision::Tensor&, int)",
    "va_cv::minMaxIdx(vision::Tensor const&, double*, double*, int*, int*, vision::Tensor const&)",
    "vision::Tensor::change_layout(vision::DLayout)",
    "vision::Tensor::change_dtype(vision::DType)",
    "vision::Tensor::clone() const",
    "vision::Tensor::create(int, int, int, vision::DType, vision::DLayout)",
    "vision::Tensor::create(int, int, int, vision::DLayout, vision::DType)",
    "vision::Tensor::Tensor(int, int, int, void*, vision::DType, vision::DLayout)",
    "vision::Tensor::release()",
    "vision::Tensor::get_ref_count() const",
    "vision::Tensor::to_device(int) const",
    "ImageUtil::bgr2nv21(unsigned char*, unsigned char*, int, int)",
    "AutoPerf::AutoPerf(double&)",
]


def _need(path: Path):
    if not path.exists():
        pytest.skip(f"{path} not built (run __graft_entry__.build())")


def test_api_exports():
    _need(API_LIB)
    out = subprocess.run(["nm", "-DC", "--defined-only", str(API_LIB)], capture_output=True, text=True,
                         check=True).stdout
    missing = [e for e in EXPORTS if e not in out]
    assert not missing, f"libvacv.so lacks {missing}"


def test_api_links_only_the_hip_library():
    """The C++ layer sits on the C ABI; it must not pull in the oracle."""
    _need(API_LIB)
    out = subprocess.run(["ldd", str(API_LIB)], capture_output=True, text=True).stdout
    assert "libvacv_hip.so" in out
    assert "oracle" not in out and "vacv_ref" not in out


def test_host_semantics_and_loud_failure():
    _need(HARNESS)
    try:
        import torch
        if torch.cuda.is_available():
            pytest.skip("GPU present: test_no_device_fails_loudly only applies to GPU-less hosts")
    except ImportError:
        pass
    r = subprocess.run([str(HARNESS), "--host-only", "--times", "1"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert json.loads(r.stdout.strip().splitlines()[-1])["failed"] == 0


def _write_res(tmp: Path) -> Path:
    """Decode the reference's test JPEGs once (PIL) into raw BGR / grey frames."""
    from PIL import Image
    for p in sorted((GOLDEN / "res").iterdir()):
        stem = p.stem
        im = Image.open(p)
        rgb = np.asarray(im.convert("RGB"), dtype=np.uint8)
        np.ascontiguousarray(rgb[:, :, ::-1]).tofile(tmp / f"{stem}.bgr")
        np.ascontiguousarray(np.asarray(im.convert("L"), dtype=np.uint8)).tofile(tmp / f"{stem}.gray")
    return tmp


@pytest.mark.gpu
def test_reference_harness_cases(hip_device, tmp_path):
    _need(HARNESS)
    res = _write_res(tmp_path)
    r = subprocess.run([str(HARNESS), "--res", str(res), "--times", "2"], capture_output=True, text=True,
                       timeout=300)
    print(r.stdout)
    summary = json.loads(r.stdout.strip().splitlines()[-1])
    assert r.returncode == 0 and summary["failed"] == 0, r.stdout + r.stderr
    assert summary["cases"] >= 40
