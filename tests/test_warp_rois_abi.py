"""The ROI warp entry points without a GPU: argument validation (before any
HIP call, with fake pointers, as test_abi does for the other entry points)
and the host-side byte count of the roofline."""
from __future__ import annotations

import ctypes

import numpy as np
import pytest

OK, INVALID, UNSUPPORTED = 0, -1, -2
FP32, INT8 = 0, 2
NCHW, NHWC = 0, 1
INTER_NEAREST, INTER_LINEAR, WARP_INVERSE_MAP = 0, 1, 16
BORDER_CONSTANT, BORDER_TRANSPARENT = 0, 5


@pytest.fixture(scope="module")
def lib():
    import vacv_amd
    if not vacv_amd._lib.HIP_LIB.exists():
        vacv_amd._lib.build()
    return vacv_amd._lib.load()


def img(ptr, n, w, h, c, dtype=INT8, layout=NHWC):
    from vacv_amd._lib import VacvImage
    return VacvImage(ptr, n, w, h, c, dtype, layout, 0, 0, 0)


def test_rois_argument_validation_without_device(lib):
    """Descriptor and flag checks happen before any HIP call and before the
    device arrays could be touched: m and src_index are fake pointers."""
    R, N = lib.vacv_warp_affine_rois, lib.vacv_warp_affine_rois_normalize
    M, IDX = 0x3000, 0x4000  # never dereferenced on the host
    by = ctypes.byref
    src1, src2 = img(0x1000, 1, 8, 8, 3), img(0x1000, 2, 8, 8, 3)
    dst3 = img(0x2000, 3, 4, 4, 3)
    dstf = img(0x2000, 3, 4, 4, 3, FP32)
    mean = (ctypes.c_float * 3)(1, 2, 3)
    std = (ctypes.c_float * 3)(4, 5, 6)

    assert R(by(src1), by(dst3), None, None, INTER_LINEAR, BORDER_CONSTANT, None, None) == INVALID   # NULL m
    assert R(by(src1), by(dst3), None, IDX, INTER_LINEAR, BORDER_CONSTANT, None, None) == INVALID
    assert N(by(src1), by(dstf), None, None, INTER_LINEAR, BORDER_CONSTANT, None, mean, std, None) == INVALID
    # src_index NULL: one frame for all, or one frame per ROI, nothing else
    assert R(by(src2), by(dst3), M, None, INTER_LINEAR, BORDER_CONSTANT, None, None) == INVALID
    assert N(by(src2), by(dstf), M, None, INTER_LINEAR, BORDER_CONSTANT, None, mean, std, None) == INVALID
    # channel counts differ
    dst4 = img(0x2000, 3, 4, 4, 4)
    assert R(by(src1), by(dst4), M, IDX, INTER_LINEAR, BORDER_CONSTANT, None, None) == INVALID
    assert N(by(src1), by(img(0x2000, 3, 4, 4, 4, FP32)), M, IDX, INTER_LINEAR, BORDER_CONSTANT, None, mean, std,
             None) == INVALID
    # _rois keeps the source's dtype and layout
    assert R(by(src1), by(dstf), M, IDX, INTER_LINEAR, BORDER_CONSTANT, None, None) == INVALID
    assert R(by(img(0x1000, 1, 8, 8, 3, FP32)), by(dst3), M, IDX, INTER_LINEAR, BORDER_CONSTANT, None, None) == INVALID
    # _rois_normalize writes FP32
    assert N(by(src1), by(dst3), M, IDX, INTER_LINEAR, BORDER_CONSTANT, None, mean, std, None) == INVALID
    # null descriptors / data
    assert R(None, by(dst3), M, IDX, INTER_LINEAR, BORDER_CONSTANT, None, None) == INVALID
    assert R(by(img(None, 1, 8, 8, 3)), by(dst3), M, IDX, INTER_LINEAR, BORDER_CONSTANT, None, None) == INVALID
    # a source the bilinear sampler cannot tap
    assert R(by(img(0x1000, 1, 1, 8, 3)), by(dst3), M, IDX, INTER_LINEAR, BORDER_CONSTANT, None, None) == INVALID

    for flags in (INTER_NEAREST, INTER_NEAREST | WARP_INVERSE_MAP, 2, INTER_LINEAR | 32):
        assert R(by(src1), by(dst3), M, IDX, flags, BORDER_CONSTANT, None, None) == UNSUPPORTED, flags
        assert N(by(src1), by(dstf), M, IDX, flags, BORDER_CONSTANT, None, mean, std, None) == UNSUPPORTED, flags
    for border in (BORDER_TRANSPARENT, 16, -1):
        assert R(by(src1), by(dst3), M, IDX, INTER_LINEAR, border, None, None) == UNSUPPORTED, border
        assert N(by(src1), by(dstf), M, IDX, INTER_LINEAR, border, None, mean, std, None) == UNSUPPORTED, border
    chw = img(0x1000, 1, 8, 8, 3, INT8, NCHW)
    assert R(by(chw), by(img(0x2000, 3, 4, 4, 3, INT8, NCHW)), M, IDX, INTER_LINEAR, BORDER_CONSTANT, None,
             None) == UNSUPPORTED
    assert N(by(chw), by(dstf), M, IDX, INTER_LINEAR, BORDER_CONSTANT, None, mean, std, None) == UNSUPPORTED
    # statistics: per-image (NULL/NULL) is not built for ROIs; exactly one NULL is a caller error
    assert N(by(src1), by(dstf), M, IDX, INTER_LINEAR, BORDER_CONSTANT, None, None, None, None) == UNSUPPORTED
    assert N(by(src1), by(dstf), M, IDX, INTER_LINEAR, BORDER_CONSTANT, None, mean, None, None) == INVALID
    assert N(by(src1), by(dstf), M, IDX, INTER_LINEAR, BORDER_CONSTANT, None, None, std, None) == INVALID
    # planar output exists for 3 channels and for 1
    src2c = img(0x1000, 1, 8, 8, 2)
    assert N(by(src2c), by(img(0x2000, 3, 4, 4, 2, FP32, NCHW)), M, IDX, INTER_LINEAR, BORDER_CONSTANT, None, mean,
             std, None) == UNSUPPORTED

    assert lib.vacv_invert_affine_device(None, 0x5000, 4, None) == INVALID
    assert lib.vacv_invert_affine_device(0x5000, None, 4, None) == INVALID
    assert lib.vacv_invert_affine_device(0x5000, 0x6000, -1, None) == INVALID
    assert lib.vacv_invert_affine_device(0x5000, 0x6000, 0, None) == OK  # nothing to do, nothing queued


def test_rois_byte_counting():
    """roofline.warp_rois_bytes: output bytes + each ROI's source
    parallelogram clipped to the frame, by hand."""
    from vacv_amd import roofline
    ident = [1, 0, 0, 0, 1, 0]
    # identity onto the whole frame: every source pixel once, every output pixel once
    assert roofline.warp_rois_bytes(64, 48, 3, 64, 48, [ident]) == 64 * 48 * 3 + 64 * 48 * 3
    # identity, a 16 x 8 crop of the top-left corner, fp32 planar out: 16*8 source pixels
    assert roofline.warp_rois_bytes(64, 48, 3, 16, 8, [ident], out_esize=4) == 16 * 8 * 3 + 16 * 8 * 3 * 4
    # fully off-frame (the crop looks at x in [1000, 1016]): only the output counts
    off = [1, 0, -1000, 0, 1, 0]
    assert roofline.warp_rois_bytes(64, 48, 3, 16, 8, [off]) == 16 * 8 * 3
    # the dst -> src map given directly: a crop whose left half hangs off the frame
    half = [1, 0, -8, 0, 1, 4]
    assert roofline.warp_rois_bytes(64, 48, 1, 16, 8, [half], inverse_map=True) == 8 * 8 + 16 * 8
    # forward scale by 2: a 16 x 8 output reads an 8 x 4 source box; fp32 in and out
    assert roofline.warp_rois_bytes(64, 48, 2, 16, 8, [[2, 0, 0, 0, 2, 0]], in_esize=4, out_esize=4) == \
        8 * 4 * 2 * 4 + 16 * 8 * 2 * 4
    # several ROIs add up; singular and non-finite maps read nothing
    ms = np.array([ident, off, [0, 0, 0, 0, 0, 0], [np.nan, 0, 0, 0, 1, 0]], np.float32)
    assert roofline.warp_rois_bytes(64, 48, 3, 16, 8, ms) == 4 * 16 * 8 * 3 + 16 * 8 * 3
