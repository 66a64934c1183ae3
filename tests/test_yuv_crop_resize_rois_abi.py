"""vacv_cvt_color_crop_resize_rois[_normalize] without a GPU: argument
validation (before any HIP call, with fake pointers, as test_yuv_rois_abi does
for the warp entry points) with the ORDER of the checks pinned by rows of two
defects, the binding, the Python wrappers' own checks and the host-side byte
count of the roofline.  Every call here is one the library rejects, so none
reaches a launch."""
from __future__ import annotations

import ctypes

import numpy as np
import pytest

OK, INVALID, UNSUPPORTED = 0, -1, -2
FP32, INT8 = 0, 2
NCHW, NHWC = 0, 1
INTER_NEAREST, INTER_LINEAR, INTER_CUBIC = 0, 1, 2
REFERENCE, NEON, OPENCV = 0, 1, 2
NV21_BGR, NV21_RGB, NV12_BGR, NV12_RGB = 93, 92, 91, 90
BAD_CODES = (8, 94, 95, 96, 97, 99, 98, 0, -1)  # GRAY2BGR, the RGBA / BGRA codes, YV12, codes that do not exist


@pytest.fixture(scope="module")
def lib():
    import vacv_amd
    if not vacv_amd._lib.HIP_LIB.exists():
        vacv_amd._lib.build()
    return vacv_amd._lib.load()


def img(ptr, n, w, h, c, dtype=INT8, layout=NHWC):
    from vacv_amd._lib import VacvImage
    return VacvImage(ptr, n, w, h, c, dtype, layout, 0, 0, 0)


@pytest.fixture(scope="module")
def calls(lib):
    """r(...) and n(...): the two entry points with one good set of arguments
    (8 x 8 decoded frames, three 4 x 4 ROIs, fake device pointers), each
    argument replaceable."""
    R, N = lib.vacv_cvt_color_crop_resize_rois, lib.vacv_cvt_color_crop_resize_rois_normalize
    RECTS, IDX = 0x3000, 0x4000  # never dereferenced on the host
    by = ctypes.byref
    mean = (ctypes.c_float * 3)(1, 2, 3)
    std = (ctypes.c_float * 3)(4, 5, 6)
    src1 = img(0x1000, 1, 8, 12, 1)
    dst3 = img(0x2000, 3, 4, 4, 3)
    dstf = img(0x2000, 3, 4, 4, 3, FP32)

    def ref(d):
        return by(d) if d is not None else None

    def r(src=src1, dst=dst3, code=NV21_BGR, rects=RECTS, idx=IDX, interp=INTER_LINEAR, mode=REFERENCE):
        return R(ref(src), ref(dst), code, rects, idx, interp, mode, None)

    def n(src=src1, dst=dstf, code=NV21_BGR, rects=RECTS, idx=IDX, interp=INTER_LINEAR, mode=REFERENCE, mean=mean,
          std=std):
        return N(ref(src), ref(dst), code, rects, idx, interp, mode, mean, std, None)

    return r, n


BAD_DTYPE = lambda: img(0x1000, 1, 8, 12, 1, FP32)   # noqa: E731
BAD_GEOMETRY = lambda: img(0x1000, 1, 8, 10, 1)      # noqa: E731  (h = 7)
TWO_FRAMES = lambda: img(0x1000, 2, 8, 12, 1)        # noqa: E731  (three ROIs, no index)


def test_every_rejection_in_order(calls):
    """One row per check of the documented order, each with its own defect alone."""
    r, n = calls
    # 1. descriptors
    assert r(src=None) == INVALID and n(src=None) == INVALID
    assert r(dst=None) == INVALID and n(dst=None) == INVALID
    assert r(src=img(None, 1, 8, 12, 1)) == INVALID and n(src=img(None, 1, 8, 12, 1)) == INVALID
    # 2. rects NULL
    assert r(rects=None) == INVALID and n(rects=None) == INVALID
    assert r(rects=None, idx=None) == INVALID
    # 3. the code: the four NV21 / NV12 -> BGR / RGB ones pass (and fail later, on the mode, so that nothing is launched)
    for code in BAD_CODES:
        assert r(code=code) == UNSUPPORTED, code
        assert n(code=code) == UNSUPPORTED, code
    for code in (NV21_BGR, NV21_RGB, NV12_BGR, NV12_RGB):
        assert r(code=code, mode=3) == INVALID, code
        assert n(code=code, mode=3) == INVALID, code
    # 4. a source that is not INT8 / c = 1 / NHWC
    for bad in (img(0x1000, 1, 8, 12, 1, FP32), img(0x1000, 1, 8, 12, 3), img(0x1000, 1, 8, 12, 1, INT8, NCHW)):
        assert r(src=bad) == INVALID, (bad.c, bad.dtype, bad.layout)
        assert n(src=bad) == INVALID, (bad.c, bad.dtype, bad.layout)
    # 5. odd w, w < 2, heights that are no h * 3 / 2 of an even h >= 2 (7 and 10 would be h = 5 and 7)
    for bad in (img(0x1000, 1, 7, 12, 1), img(0x1000, 1, 8, 7, 1), img(0x1000, 1, 8, 10, 1), img(0x1000, 1, 1, 12, 1),
                img(0x1000, 1, 8, 13, 1), img(0x1000, 1, 8, 2, 1)):
        assert r(src=bad) == INVALID, (bad.w, bad.h)
        assert n(src=bad) == INVALID, (bad.w, bad.h)
    # 6. dst->c != 3
    for c in (1, 2, 4):
        assert r(dst=img(0x2000, 3, 4, 4, c)) == INVALID, c
        assert n(dst=img(0x2000, 3, 4, 4, c, FP32)) == INVALID, c
        assert n(dst=img(0x2000, 3, 4, 4, c, FP32, NCHW)) == INVALID, c
    # 7. src_index NULL: one frame for all, or one frame per ROI, nothing else
    assert r(src=TWO_FRAMES(), idx=None) == INVALID
    assert n(src=TWO_FRAMES(), idx=None) == INVALID
    assert n(src=TWO_FRAMES(), dst=img(0x2000, 3, 4, 4, 3, FP32, NCHW), idx=None) == INVALID
    # 8. interpolation
    for interp in (INTER_NEAREST, INTER_CUBIC, 3, 4, 17, -1):
        assert r(interp=interp) == UNSUPPORTED, interp
        assert n(interp=interp) == UNSUPPORTED, interp
    # 9. mode
    for mode in (-1, 3, 100):
        assert r(mode=mode) == INVALID, mode
        assert n(mode=mode) == INVALID, mode
    # 10. the output: _rois writes INT8 NHWC, _rois_normalize FP32
    assert r(dst=img(0x2000, 3, 4, 4, 3, FP32)) == INVALID
    assert r(dst=img(0x2000, 3, 4, 4, 3, INT8, NCHW)) == INVALID
    assert n(dst=img(0x2000, 3, 4, 4, 3)) == INVALID
    assert n(dst=img(0x2000, 3, 4, 4, 3, INT8, NCHW)) == INVALID
    # 11. size limits: a destination wider than 2^20 pixels, a pixel count past an int
    for mode in (REFERENCE, NEON, OPENCV):
        assert r(dst=img(0x2000, 3, (1 << 20) + 1, 1, 3), mode=mode) == UNSUPPORTED
        assert n(dst=img(0x2000, 3, (1 << 20) + 1, 1, 3, FP32), mode=mode) == UNSUPPORTED
        assert n(dst=img(0x2000, 3, (1 << 20) + 1, 1, 3, FP32, NCHW), mode=mode) == UNSUPPORTED
    assert r(dst=img(0x2000, 1, 1 << 20, 1 << 12, 3)) == UNSUPPORTED
    # the statistics come first of all: per-image (NULL/NULL) is not built for ROIs; exactly one NULL is a caller error
    assert n(mean=None, std=None) == UNSUPPORTED
    assert n(std=None) == INVALID
    assert n(mean=None) == INVALID


def test_two_defects_pin_the_order(calls):
    """Each row has the defect of one check and that of a LATER one with the
    other status: the earlier check's status is what comes back."""
    r, n = calls
    f32 = img(0x2000, 3, 4, 4, 3, FP32)
    wide = img(0x2000, 3, (1 << 20) + 1, 1, 3)
    for f, good_dst in ((r, img(0x2000, 3, 4, 4, 3)), (n, f32)):
        # 1 < 3: NULL descriptors and a bad code
        assert f(src=None, code=97) == INVALID
        # 2 < 3: NULL rects and a bad code
        assert f(rects=None, code=97) == INVALID
        assert f(rects=None, interp=INTER_CUBIC) == INVALID
        # 3 < 4, 5, 6, 7, 9: a bad code and ...
        assert f(code=97, src=BAD_DTYPE()) == UNSUPPORTED
        assert f(code=99, src=BAD_GEOMETRY()) == UNSUPPORTED
        # (_normalize has looked at dst's channels with the statistics, before the code)
        assert f(code=8, dst=img(0x2000, 3, 4, 4, 1, good_dst.dtype)) == (UNSUPPORTED if f is r else INVALID)
        assert f(code=0, src=TWO_FRAMES(), idx=None) == UNSUPPORTED
        assert f(code=94, mode=7) == UNSUPPORTED
        # 4, 5, 6, 7 < 8: the source, the geometry, the channels, the index rule and a bad interpolation
        assert f(src=BAD_DTYPE(), interp=INTER_NEAREST) == INVALID
        assert f(src=BAD_GEOMETRY(), interp=INTER_NEAREST) == INVALID
        assert f(dst=img(0x2000, 3, 4, 4, 4, good_dst.dtype), interp=INTER_CUBIC) == INVALID
        assert f(src=TWO_FRAMES(), idx=None, interp=INTER_CUBIC) == INVALID
        # 8 < 9: a bad interpolation and a bad mode
        assert f(interp=INTER_CUBIC, mode=3) == UNSUPPORTED
        assert f(interp=INTER_NEAREST, mode=-1) == UNSUPPORTED
        # 8 < 10: a bad interpolation and the wrong output dtype
        assert f(interp=INTER_CUBIC, dst=img(0x2000, 3, 4, 4, 3, FP32 if f is r else INT8)) == UNSUPPORTED
        # 9 < 11: a bad mode and a destination past the size limit
        assert f(mode=3, dst=img(0x2000, 3, (1 << 20) + 1, 1, 3, good_dst.dtype)) == INVALID
    # 10 < 11: the wrong output dtype and a destination past the size limit
    assert r(dst=img(0x2000, 3, (1 << 20) + 1, 1, 3, FP32)) == INVALID
    assert n(dst=wide) == INVALID
    # the statistics before everything: both NULL with NULL descriptors, with NULL rects, with a 4-channel dst
    assert n(mean=None, std=None, src=None) == UNSUPPORTED
    assert n(mean=None, std=None, src=None, dst=None) == UNSUPPORTED
    assert n(mean=None, std=None, rects=None) == UNSUPPORTED
    assert n(mean=None, std=None, dst=img(0x2000, 3, 4, 4, 4, FP32)) == UNSUPPORTED
    # one NULL with a bad code
    assert n(mean=None, code=97) == INVALID
    # given statistics, then the descriptors, then one value per decoded channel -- before the code
    assert n(dst=img(0x2000, 3, 4, 4, 4, FP32), code=97) == INVALID


def test_binding_matches_header(lib):
    import vacv_amd
    assert vacv_amd._lib.ABI_VERSION == 5 and lib.vacv_abi_version() == 5
    header = vacv_amd._lib.HEADER.read_text()
    for name in ("vacv_cvt_color_crop_resize_rois", "vacv_cvt_color_crop_resize_rois_normalize"):
        assert name in vacv_amd._lib.SIGNATURES and f"int {name}(" in header
        assert getattr(lib, name).restype is ctypes.c_int
    assert len(vacv_amd._lib.SIGNATURES["vacv_cvt_color_crop_resize_rois"][0]) == 8
    assert len(vacv_amd._lib.SIGNATURES["vacv_cvt_color_crop_resize_rois_normalize"][0]) == 10
    from vacv_amd import cvt_color_crop_resize_rois, cvt_color_crop_resize_rois_normalize, ops
    assert cvt_color_crop_resize_rois is ops.cvt_color_crop_resize_rois
    assert cvt_color_crop_resize_rois_normalize is ops.cvt_color_crop_resize_rois_normalize
    assert "cvt_color_crop_resize_rois" in vacv_amd.__all__ and "cvt_color_crop_resize_rois_normalize" in vacv_amd.__all__


def test_python_argument_checks():
    """Every ValueError of the two wrappers that is raised before the library
    is called, on CPU tensors: the texts and their order are those of the six
    existing ROI wrappers (test_rois_status_grid.test_rois_python_argument_checks)."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present: the CPU tensors of this test would be refused for their device first")
    from vacv_amd import ops

    yuv = torch.zeros((2, 12, 8), dtype=torch.uint8)
    mean, std = [1.0, 2.0, 3.0], [4.0, 5.0, 6.0]
    good = np.zeros((3, 4), np.int32)
    misshapen, shape_msg = np.zeros((3, 3), np.int32), "rects must have shape (n, 4), got (3, 3)"
    empty, empty_msg = np.zeros((0, 4), np.int32), "rects holds no rect"
    for fn, normalize in ((ops.cvt_color_crop_resize_rois, False), (ops.cvt_color_crop_resize_rois_normalize, True)):
        stats = (mean, std) if normalize else ()

        def raises(text, s, arr, st=stats, **kw):
            with pytest.raises(ValueError) as e:
                fn(s, arr, 4, 4, *st, **kw)
            assert str(e.value) == text, (fn.__name__, str(e.value))

        raises(shape_msg, yuv, misshapen)
        raises(empty_msg, yuv, empty)
        raises("rects must be torch.int32, not torch.float64", yuv, torch.zeros(good.shape, dtype=torch.float64))
        raises("rects must be contiguous", yuv, torch.zeros((6, 4), dtype=torch.int32)[::2])
        raises("src_index must have shape (3,), got (2,)", yuv, good, src_index=torch.zeros(2, dtype=torch.int32))
        raises("src_index must be torch.int32, not torch.int64", yuv, good, src_index=torch.zeros(3, dtype=torch.int64))
        raises("src_index must be contiguous", yuv, good, src_index=torch.zeros(6, dtype=torch.int32)[::2])
        raises("without src_index, src must hold 1 or 3 images, not 2", yuv, good)
        # two defects: the array's shape is looked at before src_index
        raises(shape_msg, yuv, misshapen, src_index=torch.zeros(3, dtype=torch.int64))
        if normalize:
            need = f"{fn.__name__} needs mean and stddev (no per-image statistics for ROIs)"
            raises(need, yuv[:1], good, st=(None, std))
            raises(need, yuv[:1], good, st=(mean, None))
            raises(need, yuv[:1], good, st=(None, None))
            # ... and the array and the frames before the statistics
            raises(shape_msg, yuv[:1], misshapen, st=(None, None))
            raises("without src_index, src must hold 1 or 3 images, not 2", yuv, good, st=(None, None))
        # frames of too many dimensions are refused before the array is looked at
        for arr in (good, misshapen):
            raises("expected a 2-4 dimensional image tensor, got shape (1, 2, 12, 8, 1, 1)", yuv.unsqueeze(-1), arr)


def test_byte_counting():
    """roofline.yuv_crop_resize_rois_bytes: 3-channel output bytes + each valid
    rect's Y bytes and the chroma pairs that cover it, by hand."""
    from vacv_amd.roofline import yuv_crop_resize_rois_bytes as count
    # 16 x 8 at the origin: 128 Y bytes and 8 x 4 chroma pairs
    assert count(16, 8, [[0, 0, 16, 8]]) == 16 * 8 * 3 + 128 + 2 * 8 * 4
    # 2 x 2 at an odd origin straddles two pairs and two chroma rows
    assert count(16, 8, [[1, 1, 2, 2]]) == 16 * 8 * 3 + 4 + 8
    # ... at an even origin it has one pair
    assert count(16, 8, [[2, 2, 2, 2]]) == 16 * 8 * 3 + 4 + 2
    # the whole 64 x 48 frame: every source byte once
    assert count(37, 29, [[0, 0, 64, 48]], w_in=64, h_in=48) == 37 * 29 * 3 + 64 * 48 * 3 // 2
    # fp32 output
    assert count(16, 8, [[0, 0, 16, 8]], out_esize=4) == 16 * 8 * 3 * 4 + 128 + 2 * 8 * 4
    # invalid rects count their output only: width 1, height 1, negative origin, past w_in / h_in
    out = 16 * 8 * 3
    for bad in ([5, 4, 1, 30], [5, 4, 30, 1], [-1, 4, 10, 10], [5, -1, 10, 10], [60, 4, 5, 10], [5, 40, 10, 9]):
        assert count(16, 8, [bad], w_in=64, h_in=48) == out, bad
    # ... and their valid neighbours (an edge ON the frame's) read
    assert count(16, 8, [[60, 4, 4, 10]], w_in=64, h_in=48) == out + 40 + 2 * 2 * 5
    assert count(16, 8, [[5, 40, 10, 8]], w_in=64, h_in=48) == out + 80 + 2 * 6 * 4
    # without the frame's size an edge cannot be judged
    assert count(16, 8, [[60, 4, 5, 10]]) == out + 50 + 2 * 3 * 5
    # several rects add up
    assert count(16, 8, [[0, 0, 16, 8], [5, 4, 1, 30], [1, 1, 2, 2]], w_in=64, h_in=48) == 3 * out + 128 + 64 + 4 + 8
