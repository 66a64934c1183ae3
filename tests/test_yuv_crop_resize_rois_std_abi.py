"""vacv_cvt_color_crop_resize_rois_standardize without a GPU: argument
validation (before any HIP call, with fake pointers, as
test_yuv_crop_resize_rois_abi does) with the ORDER of the checks pinned by rows
of two defects, the LDS gate at its limit, the exported surface, the Python
wrapper's own checks and the roofline's byte count.

No call here reaches a launch: a case that has to show that a check was PASSED
gives one pointer for mean_out and stddev_out, which the entry point refuses
with INVALID_ARG only after every other check (the order of the checks is part
of its header comment)."""
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
NAME = "vacv_cvt_color_crop_resize_rois_standardize"
RECTS, IDX, STATS, OTHER = 0x3000, 0x4000, 0x5000, 0x6000  # never dereferenced on the host


@pytest.fixture(scope="module")
def lib():
    import vacv_amd
    if not vacv_amd._lib.HIP_LIB.exists():
        vacv_amd._lib.build()
    return vacv_amd._lib.load()


def img(ptr, n, w, h, c, dtype=INT8, layout=NHWC):
    from vacv_amd._lib import VacvImage
    return VacvImage(ptr, n, w, h, c, dtype, layout, 0, 0, 0)


SRC1 = lambda: img(0x1000, 1, 8, 12, 1)                # noqa: E731  one 8 x 8 decoded frame
DSTF = lambda: img(0x2000, 3, 4, 4, 3, FP32)           # noqa: E731  three 4 x 4 ROIs
BAD_DTYPE = lambda: img(0x1000, 1, 8, 12, 1, FP32)     # noqa: E731
BAD_GEOMETRY = lambda: img(0x1000, 1, 8, 10, 1)        # noqa: E731  (h = 7)
TWO_FRAMES = lambda: img(0x1000, 2, 8, 12, 1)          # noqa: E731  (three ROIs, no index)
TOO_TALL = lambda: img(0x2000, 3, 145, 144, 3, FP32)   # noqa: E731  past the LDS limit


@pytest.fixture(scope="module")
def r(lib):
    """The entry point with one good set of arguments, each replaceable.
    mean == std by default: a call that passes every other check ends in
    INVALID_ARG, not in a launch."""
    by = ctypes.byref

    def call(src="good", dst="good", code=NV21_BGR, rects=RECTS, idx=IDX, interp=INTER_LINEAR, mode=REFERENCE,
             mean=STATS, std=STATS):
        src = SRC1() if isinstance(src, str) else src
        dst = DSTF() if isinstance(dst, str) else dst
        return lib.vacv_cvt_color_crop_resize_rois_standardize(by(src) if src is not None else None,
                                                               by(dst) if dst is not None else None, code, rects, idx,
                                                               interp, mode, mean, std, None)
    return call


def lds_need(w, h):
    """The header comment's formula (csrc/k_yuv_crop_resize_rois_std.hip), restated."""
    return 256 + (3 * w * h + 15) // 16 * 16 + max(8 * (w + h), 3072)


def test_every_rejection_in_order(r):
    """One row per check of the documented order, each with its own defect alone."""
    # accepted up to the last check: NHWC and planar, with and without an index, every code and mode
    assert r() == INVALID and r(dst=img(0x2000, 3, 4, 4, 3, FP32, NCHW)) == INVALID and r(idx=None) == INVALID
    for code in (NV21_BGR, NV21_RGB, NV12_BGR, NV12_RGB):
        for mode in (REFERENCE, NEON, OPENCV):
            assert r(code=code, mode=mode) == INVALID, (code, mode)
    # 1. descriptors
    assert r(src=None) == INVALID and r(dst=None) == INVALID
    assert r(src=img(None, 1, 8, 12, 1)) == INVALID and r(dst=img(None, 3, 4, 4, 3, FP32)) == INVALID
    # 2. rects NULL
    assert r(rects=None, mean=None, std=None) == INVALID and r(rects=None, idx=None, mean=STATS, std=OTHER) == INVALID
    # 3. the code
    for code in BAD_CODES:
        assert r(code=code) == UNSUPPORTED, code
    # 4. a source that is not INT8 / c = 1 / NHWC
    for bad in (img(0x1000, 1, 8, 12, 1, FP32), img(0x1000, 1, 8, 12, 3), img(0x1000, 1, 8, 12, 1, INT8, NCHW)):
        assert r(src=bad, mean=None, std=None) == INVALID, (bad.c, bad.dtype, bad.layout)
    # 5. odd w, w < 2, heights that are no h * 3 / 2 of an even h >= 2 (7 and 10 would be h = 5 and 7)
    for bad in (img(0x1000, 1, 7, 12, 1), img(0x1000, 1, 8, 7, 1), img(0x1000, 1, 8, 10, 1), img(0x1000, 1, 1, 12, 1),
                img(0x1000, 1, 8, 13, 1), img(0x1000, 1, 8, 2, 1)):
        assert r(src=bad, mean=None, std=None) == INVALID, (bad.w, bad.h)
    # 6. dst->c != 3
    for c in (1, 2, 4):
        assert r(dst=img(0x2000, 3, 4, 4, c, FP32), mean=None, std=None) == INVALID, c
        assert r(dst=img(0x2000, 3, 4, 4, c, FP32, NCHW), mean=STATS, std=OTHER) == INVALID, c
    # 7. src_index NULL: one frame for all, or one frame per ROI, nothing else
    assert r(src=TWO_FRAMES(), idx=None, mean=None, std=None) == INVALID
    assert r(src=img(0x1000, 3, 8, 12, 1), idx=None) == INVALID  # frame i for ROI i: the last check
    # 8. interpolation
    for interp in (INTER_NEAREST, INTER_CUBIC, 3, 4, 17, -1):
        assert r(interp=interp) == UNSUPPORTED, interp
    # 9. mode
    for mode in (-1, 3, 100):
        assert r(mode=mode, mean=None, std=None) == INVALID, mode
    # 10. the output is FP32
    assert r(dst=img(0x2000, 3, 4, 4, 3), mean=None, std=None) == INVALID
    assert r(dst=img(0x2000, 3, 4, 4, 3, INT8, NCHW), mean=STATS, std=OTHER) == INVALID
    # 11. the work shape's limits: one workgroup's LDS, 1,024 threads per ROI within a 32-bit grid
    assert r(dst=TOO_TALL()) == UNSUPPORTED and r(dst=TOO_TALL(), mean=None, std=None) == UNSUPPORTED
    assert r(dst=img(0x2000, 3, 144, 144, 3, FP32)) == INVALID  # exactly 64 KiB: the last check
    assert r(dst=img(0x2000, 4194304, 2, 2, 3, FP32)) == UNSUPPORTED
    assert r(dst=img(0x2000, 4194303, 2, 2, 3, FP32)) == INVALID
    # 12. one array for both statistics
    assert r(mean=STATS, std=STATS) == INVALID


def test_two_defects_pin_the_order(r):
    """Each row has the defect of one check and that of a LATER one with the
    other status: the earlier check's status is what comes back."""
    # 1 < 3: NULL descriptors and a bad code
    assert r(src=None, code=97) == INVALID
    # 2 < 3, 8: NULL rects and a bad code, a bad interpolation
    assert r(rects=None, code=97) == INVALID
    assert r(rects=None, interp=INTER_CUBIC) == INVALID
    # 3 < 4, 5, 6, 7, 9, 10: a bad code and ...
    assert r(code=97, src=BAD_DTYPE()) == UNSUPPORTED
    assert r(code=99, src=BAD_GEOMETRY()) == UNSUPPORTED
    assert r(code=8, dst=img(0x2000, 3, 4, 4, 1, FP32)) == UNSUPPORTED
    assert r(code=0, src=TWO_FRAMES(), idx=None) == UNSUPPORTED
    assert r(code=94, mode=7) == UNSUPPORTED
    assert r(code=95, dst=img(0x2000, 3, 4, 4, 3)) == UNSUPPORTED
    # 4, 5, 6, 7 < 8: the source, the geometry, the channels, the index rule and a bad interpolation
    assert r(src=BAD_DTYPE(), interp=INTER_NEAREST) == INVALID
    assert r(src=BAD_GEOMETRY(), interp=INTER_NEAREST) == INVALID
    assert r(dst=img(0x2000, 3, 4, 4, 4, FP32), interp=INTER_CUBIC) == INVALID
    assert r(src=TWO_FRAMES(), idx=None, interp=INTER_CUBIC) == INVALID
    # 8 < 9: a bad interpolation and a bad mode
    assert r(interp=INTER_CUBIC, mode=3) == UNSUPPORTED
    assert r(interp=INTER_NEAREST, mode=-1) == UNSUPPORTED
    # 8 < 10: a bad interpolation and an INT8 dst
    assert r(interp=INTER_CUBIC, dst=img(0x2000, 3, 4, 4, 3)) == UNSUPPORTED
    # 9 < 11: a bad mode and a destination past the LDS limit
    assert r(mode=3, dst=TOO_TALL()) == INVALID
    # 10 < 11: an INT8 dst past the LDS limit, past the grid limit
    assert r(dst=img(0x2000, 3, 145, 144, 3)) == INVALID
    assert r(dst=img(0x2000, 4194304, 2, 2, 3)) == INVALID
    # 11 < 12: past the LDS limit with one array for both statistics: UNSUPPORTED, not INVALID_ARG
    assert r(dst=TOO_TALL(), mean=STATS, std=STATS) == UNSUPPORTED
    assert r(dst=img(0x2000, 4194304, 2, 2, 3, FP32), mean=STATS, std=STATS) == UNSUPPORTED


@pytest.mark.parametrize("w", [144, 250, 3, 1500, 2000])
def test_lds_gate(r, w):
    """At a fixed width, the tallest ROI the documented formula admits passes
    the gate and one row more does not."""
    h = max(h for h in range(1, 30000) if lds_need(w, h) <= 65536)
    assert lds_need(w, h) <= 65536 < lds_need(w, h + 1)
    assert r(dst=img(0x2000, 2, w, h, 3, FP32)) == INVALID, (w, h)  # past the gate: refused by the last check only
    assert r(dst=img(0x2000, 2, w, h + 1, 3, FP32)) == UNSUPPORTED, (w, h + 1)
    assert r(dst=img(0x2000, 2, w, h + 1, 3, FP32, NCHW), mean=None, std=None) == UNSUPPORTED, (w, h + 1)


def test_lds_formula_admits_the_model_inputs():
    assert lds_need(112, 112) == 40960 and lds_need(128, 128) == 52480
    assert lds_need(144, 144) == 65536 and lds_need(145, 144) > 65536
    assert lds_need(8000, 1) == 256 + 24000 + 64008  # a row longer than the table: the taps set the need
    # a ROI that fits has fewer than 65,536 / 3 pixels: Sum v^2 of a channel stays below 2^32
    assert (65536 // 3) * 255 * 255 < 2 ** 32


def test_binding_matches_header(lib):
    import subprocess

    import vacv_amd
    assert vacv_amd._lib.ABI_VERSION == 5 and lib.vacv_abi_version() == 5  # an added export does not bump it
    header = vacv_amd._lib.HEADER.read_text()
    assert "#define VACV_ABI_VERSION 5\n" in header
    exported = subprocess.run(["nm", "-D", "--defined-only", str(vacv_amd._lib.HIP_LIB)], capture_output=True,
                              text=True, check=True).stdout
    assert NAME in vacv_amd._lib.SIGNATURES and f"int {NAME}(" in header and f" T {NAME}\n" in exported
    assert len(vacv_amd._lib.SIGNATURES[NAME][0]) == 10 and getattr(lib, NAME).restype is ctypes.c_int
    assert "cvt_color_crop_resize_rois_standardize" in vacv_amd._OPS
    assert "cvt_color_crop_resize_rois_standardize" in vacv_amd.__all__
    from vacv_amd import cvt_color_crop_resize_rois_standardize, ops
    assert cvt_color_crop_resize_rois_standardize is ops.cvt_color_crop_resize_rois_standardize
    # the formula the header states is the one tested above
    assert "256 + 16 ceil(3 w h / 16) + max(8 (w + h), 3072)" in header


def test_python_argument_checks():
    """Every ValueError of the wrapper that is raised before the library is
    called, on CPU tensors: the texts and their order are those of
    cvt_color_crop_resize_rois (test_yuv_crop_resize_rois_abi)."""
    import torch
    from vacv_amd import ops

    fn = ops.cvt_color_crop_resize_rois_standardize
    yuv = torch.zeros((2, 12, 8), dtype=torch.uint8)
    good = np.zeros((3, 4), np.int32)
    misshapen, shape_msg = np.zeros((3, 3), np.int32), "rects must have shape (n, 4), got (3, 3)"

    def raises(text, s, arr, **kw):
        with pytest.raises(ValueError) as e:
            fn(s, arr, 4, 4, **kw)
        assert str(e.value) == text, str(e.value)

    raises(shape_msg, yuv, misshapen)
    raises("rects holds no rect", yuv, np.zeros((0, 4), np.int32))
    raises("rects must be torch.int32, not torch.float64", yuv, torch.zeros(good.shape, dtype=torch.float64))
    raises("rects must be contiguous", yuv, torch.zeros((6, 4), dtype=torch.int32)[::2])
    raises("src_index must have shape (3,), got (2,)", yuv, good, src_index=torch.zeros(2, dtype=torch.int32))
    raises("src_index must be torch.int32, not torch.int64", yuv, good, src_index=torch.zeros(3, dtype=torch.int64))
    raises("src_index must be contiguous", yuv, good, src_index=torch.zeros(6, dtype=torch.int32)[::2])
    raises("without src_index, src must hold 1 or 3 images, not 2", yuv, good)
    raises("without src_index, src must hold 1 or 3 images, not 2", yuv, good, stats=True, layout=NCHW)
    # two defects: the array's shape is looked at before src_index
    raises(shape_msg, yuv, misshapen, src_index=torch.zeros(3, dtype=torch.int64))
    # frames of too many dimensions are refused before the array is looked at
    for arr in (good, misshapen):
        raises("expected a 2-4 dimensional image tensor, got shape (1, 2, 12, 8, 1, 1)", yuv.unsqueeze(-1), arr)


def test_byte_counting():
    """roofline.yuv_crop_resize_rois_standardize_bytes: fp32 3-channel output +
    statistics + each valid rect's Y bytes and the chroma pairs that cover it,
    by hand."""
    from vacv_amd.roofline import yuv_crop_resize_rois_bytes, yuv_crop_resize_rois_standardize_bytes as count
    out = 16 * 8 * 3 * 4
    # 16 x 8 at the origin: 128 Y bytes and 8 x 4 chroma pairs
    assert count(16, 8, [[0, 0, 16, 8]]) == out + 128 + 2 * 8 * 4
    assert count(16, 8, [[0, 0, 16, 8]], stats=True) == out + 128 + 2 * 8 * 4 + 2 * 1 * 3 * 4
    # 2 x 2 at an odd origin straddles two pairs and two chroma rows; at an even one it has one pair
    assert count(16, 8, [[1, 1, 2, 2]]) == out + 4 + 8 and count(16, 8, [[2, 2, 2, 2]]) == out + 4 + 2
    # the whole 64 x 48 frame: every source byte once
    assert count(37, 29, [[0, 0, 64, 48]], w_in=64, h_in=48) == 37 * 29 * 3 * 4 + 64 * 48 * 3 // 2
    # invalid rects count their output (and their statistics) only
    for bad in ([5, 4, 1, 30], [5, 4, 30, 1], [-1, 4, 10, 10], [60, 4, 5, 10], [5, 40, 10, 9]):
        assert count(16, 8, [bad], w_in=64, h_in=48) == out, bad
        assert count(16, 8, [bad], stats=True, w_in=64, h_in=48) == out + 24, bad
    # several rects add up; three ROIs' statistics are 2 * 3 * 3 floats
    rects = [[0, 0, 16, 8], [5, 4, 1, 30], [1, 1, 2, 2]]
    assert count(16, 8, rects, stats=True, w_in=64, h_in=48) == 3 * out + 128 + 64 + 4 + 8 + 72
    # it is the YUV count at 4 bytes per output element
    assert count(16, 8, rects, w_in=64, h_in=48) == yuv_crop_resize_rois_bytes(16, 8, rects, 4, 64, 48)
    assert count(16, 8, np.zeros((0, 4), np.int32), stats=True) == 0
