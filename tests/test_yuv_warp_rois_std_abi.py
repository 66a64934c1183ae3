"""vacv_cvt_color_warp_affine_rois_standardize without a GPU: argument
validation (before any HIP call, with fake pointers, as test_yuv_rois_abi does)
with the ORDER of the checks pinned by rows of two defects, the LDS gate at its
limit, the exported surface, the Python wrapper's own checks and the roofline's
byte count.

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
INTER_NEAREST, INTER_LINEAR, INTER_CUBIC, WARP_INVERSE_MAP = 0, 1, 2, 16
CONSTANT, REPLICATE, REFLECT, WRAP, REFLECT_101, TRANSPARENT = 0, 1, 2, 3, 4, 5
NV21_BGR, NV21_RGB, NV12_BGR, NV12_RGB = 93, 92, 91, 90
BAD_CODES = (8, 94, 95, 96, 97, 99, 98, 0, -1)  # GRAY2BGR, the RGBA / BGRA codes, YV12, codes that do not exist
NAME = "vacv_cvt_color_warp_affine_rois_standardize"
MS, IDX, STATS, OTHER = 0x3000, 0x4000, 0x5000, 0x6000  # never dereferenced on the host


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
    bv = (ctypes.c_double * 4)(7, 99, 200, 33)

    def call(src="good", dst="good", code=NV21_BGR, m=MS, idx=IDX, flags=INTER_LINEAR, border=CONSTANT, mean=STATS,
             std=STATS, border_value=bv):
        src = SRC1() if isinstance(src, str) else src
        dst = DSTF() if isinstance(dst, str) else dst
        return lib.vacv_cvt_color_warp_affine_rois_standardize(by(src) if src is not None else None,
                                                               by(dst) if dst is not None else None, code, m, idx,
                                                               flags, border, border_value, mean, std, None)
    return call


def lds_need(w, h):
    """The header comment's formula (csrc/k_yuv_warp_rois_std.hip), restated."""
    return 256 + (3 * w * h + 15) // 16 * 16 + 3072


def test_every_rejection_in_order(r):
    """One row per check of the documented order, each with its own defect alone."""
    # accepted up to the last check: NHWC and planar, with and without an index, every code, flag and border mode
    assert r() == INVALID and r(dst=img(0x2000, 3, 4, 4, 3, FP32, NCHW)) == INVALID and r(idx=None) == INVALID
    assert r(border_value=None) == INVALID
    for code in (NV21_BGR, NV21_RGB, NV12_BGR, NV12_RGB):
        for border in (CONSTANT, REPLICATE, REFLECT, WRAP, REFLECT_101):
            for flags in (INTER_LINEAR, INTER_LINEAR | WARP_INVERSE_MAP):
                assert r(code=code, border=border, flags=flags) == INVALID, (code, border, flags)
    # 1. descriptors
    assert r(src=None) == INVALID and r(dst=None) == INVALID
    assert r(src=img(None, 1, 8, 12, 1)) == INVALID and r(dst=img(None, 3, 4, 4, 3, FP32)) == INVALID
    # 2. m NULL
    assert r(m=None, mean=None, std=None) == INVALID and r(m=None, idx=None, mean=STATS, std=OTHER) == INVALID
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
    # 8. flags and border mode
    for flags in (INTER_NEAREST, INTER_NEAREST | WARP_INVERSE_MAP, INTER_CUBIC, INTER_LINEAR | 32):
        assert r(flags=flags) == UNSUPPORTED, flags
    for border in (TRANSPARENT, 16, -1):
        assert r(border=border) == UNSUPPORTED, border
    # 9. the output is FP32
    assert r(dst=img(0x2000, 3, 4, 4, 3), mean=None, std=None) == INVALID
    assert r(dst=img(0x2000, 3, 4, 4, 3, INT8, NCHW), mean=STATS, std=OTHER) == INVALID
    # 10. the work shape's limits: one workgroup's LDS, 1,024 threads per ROI within a 32-bit grid
    assert r(dst=TOO_TALL()) == UNSUPPORTED and r(dst=TOO_TALL(), mean=None, std=None) == UNSUPPORTED
    assert r(dst=img(0x2000, 3, 144, 144, 3, FP32)) == INVALID  # exactly 64 KiB: the last check
    assert r(dst=img(0x2000, 4194304, 2, 2, 3, FP32)) == UNSUPPORTED
    assert r(dst=img(0x2000, 4194303, 2, 2, 3, FP32)) == INVALID
    # 11. one array for both statistics
    assert r(mean=STATS, std=STATS) == INVALID


def test_two_defects_pin_the_order(r):
    """Each row has the defect of one check and that of a LATER one with the
    other status: the earlier check's status is what comes back."""
    # 1 < 3: NULL descriptors and a bad code
    assert r(src=None, code=97) == INVALID
    # 2 < 3, 8: NULL m and a bad code, bad flags, TRANSPARENT
    assert r(m=None, code=97) == INVALID
    assert r(m=None, flags=INTER_CUBIC) == INVALID
    assert r(m=None, border=TRANSPARENT) == INVALID
    # 3 < 4, 5, 6, 7, 9: a bad code and ...
    assert r(code=97, src=BAD_DTYPE()) == UNSUPPORTED
    assert r(code=99, src=BAD_GEOMETRY()) == UNSUPPORTED
    assert r(code=8, dst=img(0x2000, 3, 4, 4, 1, FP32)) == UNSUPPORTED
    assert r(code=0, src=TWO_FRAMES(), idx=None) == UNSUPPORTED
    assert r(code=95, dst=img(0x2000, 3, 4, 4, 3)) == UNSUPPORTED
    # 4, 5, 6, 7 < 8: the source, the geometry, the channels, the index rule and bad flags / TRANSPARENT
    assert r(src=BAD_DTYPE(), flags=INTER_NEAREST) == INVALID
    assert r(src=BAD_GEOMETRY(), border=TRANSPARENT) == INVALID
    assert r(dst=img(0x2000, 3, 4, 4, 4, FP32), flags=INTER_CUBIC) == INVALID
    assert r(src=TWO_FRAMES(), idx=None, border=TRANSPARENT) == INVALID
    # 8 < 9: bad flags / TRANSPARENT and an INT8 dst
    assert r(flags=INTER_CUBIC, dst=img(0x2000, 3, 4, 4, 3)) == UNSUPPORTED
    assert r(border=TRANSPARENT, dst=img(0x2000, 3, 4, 4, 3)) == UNSUPPORTED
    # 9 < 10: an INT8 dst past the LDS limit, past the grid limit
    assert r(dst=img(0x2000, 3, 145, 144, 3)) == INVALID
    assert r(dst=img(0x2000, 4194304, 2, 2, 3)) == INVALID
    # 10 < 11: past the LDS limit with one array for both statistics: UNSUPPORTED, not INVALID_ARG
    assert r(dst=TOO_TALL(), mean=STATS, std=STATS) == UNSUPPORTED
    assert r(dst=img(0x2000, 4194304, 2, 2, 3, FP32), mean=STATS, std=STATS) == UNSUPPORTED


@pytest.mark.parametrize("w", [144, 250, 3, 1500, 20000])
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
    assert lds_need(20000, 1) <= 65536 < lds_need(20000, 2)  # no taps are tabled: a long row fits
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
    assert len(vacv_amd._lib.SIGNATURES[NAME][0]) == 11 and getattr(lib, NAME).restype is ctypes.c_int
    assert "cvt_color_warp_affine_rois_standardize" in vacv_amd._OPS
    assert "cvt_color_warp_affine_rois_standardize" in vacv_amd.__all__
    from vacv_amd import cvt_color_warp_affine_rois_standardize, ops
    assert cvt_color_warp_affine_rois_standardize is ops.cvt_color_warp_affine_rois_standardize
    # the formula the header states is the one tested above
    assert "256 + 16 ceil(3 w h / 16) + 3072" in header


def test_python_argument_checks():
    """Every ValueError of the wrapper that is raised before the library is
    called, on CPU tensors: the texts and their order are those of
    cvt_color_warp_affine_rois."""
    import torch
    from vacv_amd import ops

    fn = ops.cvt_color_warp_affine_rois_standardize
    yuv = torch.zeros((2, 12, 8), dtype=torch.uint8)
    good = np.zeros((3, 6), np.float32)
    misshapen, shape_msg = np.zeros((3, 5), np.float32), "ms must have shape (n, 6) or (n, 2, 3), got (3, 5)"

    def raises(text, s, arr, **kw):
        with pytest.raises(ValueError) as e:
            fn(s, arr, 4, 4, **kw)
        assert str(e.value) == text, str(e.value)

    raises(shape_msg, yuv, misshapen)
    raises("ms must have shape (n, 6) or (n, 2, 3), got (3, 3, 2)", yuv, np.zeros((3, 3, 2), np.float32))
    raises("ms holds no matrix", yuv, np.zeros((0, 6), np.float32))
    raises("ms must be torch.float32, not torch.float64", yuv, torch.zeros(good.shape, dtype=torch.float64))
    raises("ms must be contiguous", yuv, torch.zeros((6, 6), dtype=torch.float32)[::2])
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
    """roofline.yuv_warp_rois_standardize_bytes: fp32 3-channel output +
    statistics + each ROI's source parallelogram clipped to the frame at 1.5
    bytes per pixel, by hand."""
    from vacv_amd.roofline import yuv_warp_rois_bytes, yuv_warp_rois_standardize_bytes as count
    ident = [1, 0, 0, 0, 1, 0]
    # identity onto the whole frame: every Y byte and every chroma byte once, every output float once
    assert count(64, 48, 64, 48, [ident]) == 64 * 48 * 3 // 2 + 64 * 48 * 3 * 4
    assert count(64, 48, 64, 48, [ident], stats=True) == 64 * 48 * 3 // 2 + 64 * 48 * 3 * 4 + 2 * 1 * 3 * 4
    # fully off-frame (the crop looks at x in [1000, 1016]): only the output (and its statistics) counts
    off = [1, 0, -1000, 0, 1, 0]
    out = 16 * 8 * 3 * 4
    assert count(64, 48, 16, 8, [off]) == out and count(64, 48, 16, 8, [off], stats=True) == out + 24
    # a 16 x 8 crop of the top-left corner: 128 Y bytes and 8 x 4 chroma pairs
    assert count(64, 48, 16, 8, [ident]) == 16 * 8 + 8 * 4 * 2 + out
    # the dst -> src map given directly: a crop whose left half hangs off the frame
    half = [1, 0, -8, 0, 1, 4]
    assert count(64, 48, 16, 8, [half], inverse_map=True) == 8 * 8 * 3 // 2 + out
    # several ROIs add up; singular and non-finite maps read nothing; four ROIs' statistics are 2 * 4 * 3 floats
    ms = [ident, off, [0, 0, 0, 0, 0, 0], [float("nan"), 0, 0, 0, 1, 0]]
    assert count(64, 48, 16, 8, ms, stats=True) == 4 * out + 16 * 8 * 3 // 2 + 96
    # it is the YUV count at 4 bytes per output element
    assert count(64, 48, 16, 8, ms) == yuv_warp_rois_bytes(64, 48, 16, 8, ms, out_esize=4)
    assert count(64, 48, 16, 8, np.zeros((0, 6), np.float32), stats=True) == 0
