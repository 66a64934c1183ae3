"""The ROI crop + resize entry points without a GPU: argument validation
(before any HIP call, with fake pointers, as test_warp_rois_abi does), the
exported surface, the host-side byte count of the roofline and the box ->
rect truncation on CPU tensors."""
from __future__ import annotations

import ctypes

import numpy as np
import pytest

OK, INVALID, UNSUPPORTED = 0, -1, -2
FP32, INT8 = 0, 2
NCHW, NHWC = 0, 1
INTER_NEAREST, INTER_LINEAR, INTER_CUBIC, INTER_AREA = 0, 1, 2, 3
REFERENCE, NEON, OPENCV = 0, 1, 2
NAMES = ("vacv_crop_resize_rois", "vacv_crop_resize_rois_normalize")


@pytest.fixture(scope="module")
def lib():
    import vacv_amd
    if not vacv_amd._lib.HIP_LIB.exists():
        vacv_amd._lib.build()
    return vacv_amd._lib.load()


def img(ptr, n, w, h, c, dtype=INT8, layout=NHWC):
    from vacv_amd._lib import VacvImage
    return VacvImage(ptr, n, w, h, c, dtype, layout, 0, 0, 0)


def test_crop_resize_rois_argument_validation_without_device(lib):
    """Descriptor, interpolation and mode checks happen before any HIP call
    and before the device arrays could be touched: rects and src_index are
    fake pointers."""
    RECTS, IDX = 0x3000, 0x4000  # never dereferenced on the host
    by = ctypes.byref
    mean = (ctypes.c_float * 4)(1, 2, 3, 4)
    std = (ctypes.c_float * 4)(4, 5, 6, 7)

    def r(src, dst, rects=RECTS, idx=IDX, interp=INTER_LINEAR, mode=REFERENCE):
        return lib.vacv_crop_resize_rois(by(src) if src else None, by(dst) if dst else None, rects, idx, interp, mode,
                                         None)

    def n(src, dst, rects=RECTS, idx=IDX, interp=INTER_LINEAR, mode=REFERENCE, mean=mean, std=std):
        return lib.vacv_crop_resize_rois_normalize(by(src) if src else None, by(dst) if dst else None, rects, idx,
                                                   interp, mode, mean, std, None)

    src1, src2, src3 = img(0x1000, 1, 8, 8, 3), img(0x1000, 2, 8, 8, 3), img(0x1000, 3, 8, 8, 3)
    srcf = img(0x1000, 1, 8, 8, 3, FP32)
    dst3, dstf = img(0x2000, 3, 4, 4, 3), img(0x2000, 3, 4, 4, 3, FP32)
    dstp = img(0x2000, 3, 4, 4, 3, FP32, NCHW)

    # NULL rects
    assert r(src1, dst3, rects=None) == INVALID and r(src1, dst3, rects=None, idx=None) == INVALID
    assert n(src1, dstf, rects=None) == INVALID
    # src_index NULL: one frame for all, or one frame per ROI, nothing else
    assert r(src2, dst3, idx=None) == INVALID and n(src2, dstf, idx=None) == INVALID
    # null descriptors / data
    assert r(None, dst3) == INVALID and r(src1, None) == INVALID
    assert n(None, dstf) == INVALID and n(src1, None) == INVALID
    assert r(img(None, 1, 8, 8, 3), dst3) == INVALID and r(src1, img(None, 3, 4, 4, 3)) == INVALID
    # NCHW frames
    chw = img(0x1000, 1, 8, 8, 3, INT8, NCHW)
    assert r(chw, img(0x2000, 3, 4, 4, 3, INT8, NCHW)) == UNSUPPORTED
    assert n(chw, dstf) == UNSUPPORTED and n(chw, dstp) == UNSUPPORTED
    # five channels
    assert r(img(0x1000, 1, 8, 8, 5), img(0x2000, 3, 4, 4, 5)) == UNSUPPORTED
    # channel counts differ
    assert r(src1, img(0x2000, 3, 4, 4, 4)) == INVALID
    assert n(src1, img(0x2000, 3, 4, 4, 4, FP32)) == INVALID
    # _rois keeps the source's dtype and layout
    assert r(src1, dstf) == INVALID and r(srcf, dst3) == INVALID
    assert r(src1, img(0x2000, 3, 4, 4, 3, INT8, NCHW)) == INVALID
    assert r(srcf, dstp) == INVALID
    # _rois_normalize writes FP32
    assert n(src1, dst3) == INVALID and n(srcf, dst3) == INVALID
    # planar output exists for 3 channels and for 1
    for c in (2, 4):
        assert n(img(0x1000, 1, 8, 8, c), img(0x2000, 3, 4, 4, c, FP32, NCHW)) == UNSUPPORTED, c
    # interpolation: INTER_LINEAR only
    for interp in (INTER_NEAREST, INTER_CUBIC, INTER_AREA, 4, 7, -1, INTER_LINEAR | 16):
        assert r(src1, dst3, interp=interp) == UNSUPPORTED, interp
        assert n(src1, dstf, interp=interp) == UNSUPPORTED, interp
    # mode: the three VACV_LINEAR_* values
    for mode in (-1, 3, 99):
        assert r(src1, dst3, mode=mode) == INVALID, mode
        assert n(src1, dstf, mode=mode) == INVALID, mode
    # statistics: per-image (NULL/NULL) is not built for ROIs; exactly one NULL is a caller error
    assert n(src1, dstf, mean=None, std=None) == UNSUPPORTED
    assert n(src1, dstf, std=None) == INVALID
    assert n(src1, dstf, mean=None) == INVALID
    # a source the bilinear sampler cannot tap
    assert r(img(0x1000, 1, 1, 8, 3), dst3) == INVALID and r(img(0x1000, 1, 8, 1, 3), dst3) == INVALID
    assert n(img(0x1000, 1, 1, 8, 3), dstf) == INVALID
    # beyond the kernel's indices: a destination row of more than 2^20 pixels
    assert r(src1, img(0x2000, 3, (1 << 20) + 1, 1, 3)) == UNSUPPORTED


def test_crop_resize_rois_binding_matches_header(lib):
    import subprocess

    import vacv_amd
    assert vacv_amd._lib.ABI_VERSION == 5 and lib.vacv_abi_version() == 5  # added exports do not bump it
    header = vacv_amd._lib.HEADER.read_text()
    exported = subprocess.run(["nm", "-D", "--defined-only", str(vacv_amd._lib.HIP_LIB)], capture_output=True,
                              text=True, check=True).stdout
    for name in NAMES:
        assert name in vacv_amd._lib.SIGNATURES and f"int {name}(" in header and f" T {name}\n" in exported, name
    from vacv_amd import crop_resize_rois, crop_resize_rois_normalize, ops, rects_from_boxes
    assert crop_resize_rois is ops.crop_resize_rois
    assert crop_resize_rois_normalize is ops.crop_resize_rois_normalize
    assert rects_from_boxes is ops.rects_from_boxes


def test_crop_resize_rois_byte_counting():
    """roofline.crop_resize_rois_bytes: output bytes + w*h*c*esize of each valid rect, by hand."""
    from vacv_amd import roofline
    rects = [[0, 0, 64, 48],     # the whole of a 64 x 48 frame
             [10, 5, 7, 3],
             [3, 3, 1, 9]]       # one pixel wide: no two taps, reads nothing
    # u8 in, u8 out, 3 channels, 16 x 8 crops
    assert roofline.crop_resize_rois_bytes(3, 1, 16, 8, rects, 1) == 3 * 16 * 8 * 3 + (64 * 48 + 7 * 3) * 3
    # u8 in, fp32 out
    assert roofline.crop_resize_rois_bytes(3, 1, 16, 8, rects, 4) == 3 * 16 * 8 * 3 * 4 + (64 * 48 + 7 * 3) * 3
    # fp32 in and out, one channel; a negative origin and a zero height are invalid too
    more = rects + [[-1, 0, 8, 8], [0, 0, 8, 0]]
    assert roofline.crop_resize_rois_bytes(1, 4, 5, 5, more, 4) == 5 * 5 * 5 * 4 + (64 * 48 + 7 * 3) * 4
    # with the frame's size, a rect past its edge is invalid as well
    assert roofline.crop_resize_rois_bytes(3, 1, 16, 8, rects, 1, w_in=63, h_in=48) == 3 * 16 * 8 * 3 + 7 * 3 * 3
    assert roofline.crop_resize_rois_bytes(3, 1, 16, 8, rects, 1, w_in=64, h_in=48) == \
        roofline.crop_resize_rois_bytes(3, 1, 16, 8, rects, 1)
    assert roofline.crop_resize_rois_bytes(3, 1, 16, 8, np.zeros((0, 4), np.int32), 1) == 0


def test_rects_from_boxes_truncates_as_crop_naive():
    """On CPU tensors, against int() of the same float32 values: int(left),
    int(top), int(right - left), int(bottom - top), float32 subtraction."""
    import torch
    from vacv_amd import ops
    boxes = np.array([[10.0, 20.0, 110.0, 70.0],
                      [10.9, 20.9, 110.1, 70.1],          # width int(99.2), not int(110.1) - int(10.9)
                      [0.5, 0.99, 3.49, 2.0],
                      [-0.9, -1.5, 5.25, 4.75],           # toward zero: left 0, top -1
                      [-7.75, -3.0, -2.5, -1.25],
                      [5.0, 6.0, 4.25, 2.5],              # negative sizes stay negative
                      [16777216.0, 3.0, 16777218.0, 3.5],
                      [0.1, 0.2, 0.3, 1000000.7]], np.float32)
    want = np.array([[int(l), int(t), int(np.float32(r) - np.float32(l)), int(np.float32(b) - np.float32(t))]
                     for l, t, r, b in boxes], np.int32)
    got = ops.rects_from_boxes(torch.from_numpy(boxes))
    assert got.dtype == torch.int32 and tuple(got.shape) == (8, 4) and got.is_contiguous()
    assert np.array_equal(got.numpy(), want)
    assert want[1].tolist() == [10, 20, 99, 49] and want[3].tolist() == [0, -1, 6, 6]
    with pytest.raises(ValueError):
        ops.rects_from_boxes(torch.from_numpy(boxes.astype(np.float64)))
    with pytest.raises(ValueError):
        ops.rects_from_boxes(torch.from_numpy(boxes.reshape(4, 8)))
