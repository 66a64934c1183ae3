"""vacv_cvt_color_warp_affine_rois[_normalize] without a GPU: argument
validation (before any HIP call, with fake pointers, as test_warp_rois_abi
does for the BGR entry points) and the host-side byte count of the roofline."""
from __future__ import annotations

import ctypes

import pytest

OK, INVALID, UNSUPPORTED = 0, -1, -2
FP32, INT8 = 0, 2
NCHW, NHWC = 0, 1
INTER_NEAREST, INTER_LINEAR, WARP_INVERSE_MAP = 0, 1, 16
BORDER_CONSTANT, BORDER_TRANSPARENT = 0, 5
NV21_BGR, NV21_RGB, NV12_BGR, NV12_RGB = 93, 92, 91, 90


@pytest.fixture(scope="module")
def lib():
    import vacv_amd
    if not vacv_amd._lib.HIP_LIB.exists():
        vacv_amd._lib.build()
    return vacv_amd._lib.load()


def img(ptr, n, w, h, c, dtype=INT8, layout=NHWC):
    from vacv_amd._lib import VacvImage
    return VacvImage(ptr, n, w, h, c, dtype, layout, 0, 0, 0)


def test_yuv_rois_argument_validation_without_device(lib):
    """Descriptor, code and flag checks happen before any HIP call and before
    the device arrays could be touched: m and src_index are fake pointers."""
    R, N = lib.vacv_cvt_color_warp_affine_rois, lib.vacv_cvt_color_warp_affine_rois_normalize
    M, IDX = 0x3000, 0x4000  # never dereferenced on the host
    by = ctypes.byref
    src1, src2 = img(0x1000, 1, 8, 12, 1), img(0x1000, 2, 8, 12, 1)  # 8 x 8 frames
    dst3 = img(0x2000, 3, 4, 4, 3)
    dstf = img(0x2000, 3, 4, 4, 3, FP32)
    dstp = img(0x2000, 3, 4, 4, 3, FP32, NCHW)
    mean = (ctypes.c_float * 3)(1, 2, 3)
    std = (ctypes.c_float * 3)(4, 5, 6)

    def r(src, dst, code=NV21_BGR, m=M, idx=IDX, flags=INTER_LINEAR, border=BORDER_CONSTANT):
        return R(by(src) if src is not None else None, by(dst), code, m, idx, flags, border, None, None)

    def n(src, dst, code=NV21_BGR, m=M, idx=IDX, flags=INTER_LINEAR, border=BORDER_CONSTANT, mean=mean, std=std):
        return N(by(src) if src is not None else None, by(dst), code, m, idx, flags, border, None, mean, std, None)

    # NULL m
    assert r(src1, dst3, m=None, idx=None) == INVALID
    assert r(src1, dst3, m=None) == INVALID
    assert n(src1, dstf, m=None, idx=None) == INVALID
    # src_index NULL: one frame for all, or one frame per ROI, nothing else
    assert r(src2, dst3, idx=None) == INVALID
    assert n(src2, dstf, idx=None) == INVALID
    assert n(src2, dstp, idx=None) == INVALID
    # null descriptors / data
    assert r(None, dst3) == INVALID
    assert r(img(None, 1, 8, 12, 1), dst3) == INVALID
    assert n(None, dstf) == INVALID
    # odd w, w < 2, heights that are no h * 3 / 2 of an even h >= 2 (7 and 10 would be h = 5 and 7), a
    # source that is not (w, h*3/2, 1) INT8
    for bad in (img(0x1000, 1, 7, 12, 1), img(0x1000, 1, 8, 7, 1), img(0x1000, 1, 8, 10, 1), img(0x1000, 1, 1, 12, 1),
                img(0x1000, 1, 8, 13, 1),
                img(0x1000, 1, 8, 2, 1), img(0x1000, 1, 8, 12, 3), img(0x1000, 1, 8, 12, 1, FP32)):
        assert r(bad, dst3) == INVALID, (bad.w, bad.h, bad.c, bad.dtype)
        assert n(bad, dstf) == INVALID, (bad.w, bad.h, bad.c, bad.dtype)
    # dst->c != 3
    for c in (1, 2, 4):
        assert r(src1, img(0x2000, 3, 4, 4, c)) == INVALID, c
        assert n(src1, img(0x2000, 3, 4, 4, c, FP32)) == INVALID, c
        assert n(src1, img(0x2000, 3, 4, 4, c, FP32, NCHW)) == INVALID, c
    # _rois writes INT8 NHWC, _rois_normalize FP32
    assert r(src1, dstf) == INVALID
    assert r(src1, img(0x2000, 3, 4, 4, 3, INT8, NCHW)) == INVALID
    assert n(src1, dst3) == INVALID
    assert n(src1, img(0x2000, 3, 4, 4, 3, INT8, NCHW)) == INVALID
    # the codes of OpenCV's arithmetic, and codes that do not exist
    for code in (8, 94, 95, 96, 97, 99, 98, 0, -1):
        assert r(src1, dst3, code=code) == UNSUPPORTED, code
        assert n(src1, dstf, code=code) == UNSUPPORTED, code
    for flags in (INTER_NEAREST, INTER_NEAREST | WARP_INVERSE_MAP, 2, INTER_LINEAR | 32):
        assert r(src1, dst3, flags=flags) == UNSUPPORTED, flags
        assert n(src1, dstf, flags=flags) == UNSUPPORTED, flags
    for border in (BORDER_TRANSPARENT, 16, -1):
        assert r(src1, dst3, border=border) == UNSUPPORTED, border
        assert n(src1, dstf, border=border) == UNSUPPORTED, border
    # statistics: per-image (NULL/NULL) is not built for ROIs; exactly one NULL is a caller error
    assert n(src1, dstf, mean=None, std=None) == UNSUPPORTED
    assert n(src1, dstf, std=None) == INVALID
    assert n(src1, dstf, mean=None) == INVALID


def test_yuv_rois_binding_matches_header(lib):
    import vacv_amd
    assert vacv_amd._lib.ABI_VERSION == 5 and lib.vacv_abi_version() == 5
    for name in ("vacv_cvt_color_warp_affine_rois", "vacv_cvt_color_warp_affine_rois_normalize"):
        assert name in vacv_amd._lib.SIGNATURES and name in vacv_amd._lib.HEADER.read_text()
    from vacv_amd import cvt_color_warp_affine_rois, cvt_color_warp_affine_rois_normalize, ops
    assert cvt_color_warp_affine_rois is ops.cvt_color_warp_affine_rois
    assert cvt_color_warp_affine_rois_normalize is ops.cvt_color_warp_affine_rois_normalize


def test_yuv_rois_byte_counting():
    """roofline.yuv_warp_rois_bytes: 3-channel output bytes + each ROI's source
    parallelogram clipped to the frame at 1.5 bytes per pixel, by hand."""
    from vacv_amd import roofline
    ident = [1, 0, 0, 0, 1, 0]
    # identity onto the whole frame: every Y byte and every chroma byte once, every output byte once
    assert roofline.yuv_warp_rois_bytes(64, 48, 64, 48, [ident]) == 64 * 48 * 3 // 2 + 64 * 48 * 3
    # fully off-frame (the crop looks at x in [1000, 1016]): only the output counts
    off = [1, 0, -1000, 0, 1, 0]
    assert roofline.yuv_warp_rois_bytes(64, 48, 16, 8, [off]) == 16 * 8 * 3
    # a 16 x 8 crop of the top-left corner, fp32 out: 128 Y bytes and 8 x 4 chroma pairs
    assert roofline.yuv_warp_rois_bytes(64, 48, 16, 8, [ident], out_esize=4) == 16 * 8 + 8 * 4 * 2 + 16 * 8 * 3 * 4
    # the dst -> src map given directly: a crop whose left half hangs off the frame
    half = [1, 0, -8, 0, 1, 4]
    assert roofline.yuv_warp_rois_bytes(64, 48, 16, 8, [half], inverse_map=True) == 8 * 8 * 3 // 2 + 16 * 8 * 3
    # several ROIs add up; singular and non-finite maps read nothing
    ms = [ident, off, [0, 0, 0, 0, 0, 0], [float("nan"), 0, 0, 0, 1, 0]]
    assert roofline.yuv_warp_rois_bytes(64, 48, 16, 8, ms) == 4 * 16 * 8 * 3 + 16 * 8 * 3 // 2
