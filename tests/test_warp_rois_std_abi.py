"""vacv_warp_affine_rois_standardize without a GPU: argument validation (before
any HIP call, with fake pointers, as test_crop_resize_rois_std_abi does), the
LDS gate at its limit, the exported surface and the roofline's byte count.

No call here reaches a launch: a case that has to show that a check was PASSED
(the LDS need at its largest) gives one pointer for mean_out and stddev_out,
which the entry point refuses with INVALID_ARG only after every other check
(the order of the checks is part of its header comment)."""
from __future__ import annotations

import ctypes

import numpy as np
import pytest

OK, INVALID, UNSUPPORTED = 0, -1, -2
FP32, INT8 = 0, 2
NCHW, NHWC = 0, 1
INTER_NEAREST, INTER_LINEAR, INTER_CUBIC, INTER_AREA = 0, 1, 2, 3
INVERSE_MAP = 16
CONSTANT, REPLICATE, REFLECT, WRAP, REFLECT_101, TRANSPARENT = 0, 1, 2, 3, 4, 5
NAME = "vacv_warp_affine_rois_standardize"
MAPS, IDX, STATS = 0x3000, 0x4000, 0x5000  # never dereferenced on the host


@pytest.fixture(scope="module")
def lib():
    import vacv_amd
    if not vacv_amd._lib.HIP_LIB.exists():
        vacv_amd._lib.build()
    return vacv_amd._lib.load()


def img(ptr, n, w, h, c, dtype=INT8, layout=NHWC):
    from vacv_amd._lib import VacvImage
    return VacvImage(ptr, n, w, h, c, dtype, layout, 0, 0, 0)


def call(lib, src, dst, m=MAPS, idx=IDX, flags=INTER_LINEAR, border=CONSTANT, bv=(1, 2, 3, 4), mean=STATS,
         std=STATS):
    """mean == std by default: a call that passes every other check ends in INVALID_ARG, not in a launch."""
    by = ctypes.byref
    return lib.vacv_warp_affine_rois_standardize(by(src) if src else None, by(dst) if dst else None, m, idx, flags,
                                                 border, (ctypes.c_double * 4)(*bv) if bv is not None else None,
                                                 mean, std, None)


def lds_need(w, h, c):
    """The header comment's formula (csrc/k_warp_rois_std.hip), restated."""
    return 256 + (w * h * c + 15) // 16 * 16 + 1024 * c


def test_status_grid(lib):
    src1, src2 = img(0x1000, 1, 8, 8, 3), img(0x1000, 2, 8, 8, 3)
    srcf = img(0x1000, 1, 8, 8, 3, FP32)
    dst3, dstf = img(0x2000, 3, 4, 4, 3), img(0x2000, 3, 4, 4, 3, FP32)
    dstp = img(0x2000, 3, 4, 4, 3, FP32, NCHW)

    def r(src, dst, **kw):
        return call(lib, src, dst, **kw)

    # accepted up to the last check: NHWC and planar, with and without an index or a border value
    assert r(src1, dstf) == INVALID and r(src1, dstp) == INVALID and r(src1, dstf, idx=None) == INVALID
    assert r(src1, dstf, bv=None) == INVALID
    # NULL descriptors / data
    assert r(None, dstf) == INVALID and r(src1, None) == INVALID
    assert r(img(None, 1, 8, 8, 3), dstf) == INVALID and r(src1, img(None, 3, 4, 4, 3, FP32)) == INVALID
    # NULL maps
    assert r(src1, dstf, m=None) == INVALID and r(src1, dstf, m=None, idx=None) == INVALID
    # channel counts differ
    assert r(src1, img(0x2000, 3, 4, 4, 4, FP32)) == INVALID
    # src_index NULL: one frame for all, or one frame per ROI, nothing else
    assert r(src2, dstf, idx=None) == INVALID
    src3 = img(0x1000, 3, 8, 8, 3)  # frame i for ROI i: accepted up to the last check
    assert r(src3, dstf, idx=None) == INVALID and r(src3, dstp, idx=None) == INVALID
    # NCHW frames, five channels
    chw = img(0x1000, 1, 8, 8, 3, INT8, NCHW)
    assert r(chw, dstf) == UNSUPPORTED and r(chw, dstp) == UNSUPPORTED
    assert r(img(0x1000, 1, 8, 8, 5), img(0x2000, 3, 4, 4, 5, FP32)) == UNSUPPORTED
    # FP32 frames: their sums are order-dependent
    assert r(srcf, dstf) == UNSUPPORTED and r(srcf, dstp) == UNSUPPORTED
    # flags: INTER_LINEAR, optionally | WARP_INVERSE_MAP
    assert r(src1, dstf, flags=INTER_LINEAR | INVERSE_MAP) == INVALID  # the last check
    for flags in (INTER_NEAREST, INTER_CUBIC, INTER_AREA, 4, 7, INTER_NEAREST | INVERSE_MAP, INTER_LINEAR | 8,
                  INTER_LINEAR | 32):
        assert r(src1, dstf, flags=flags) == UNSUPPORTED, flags
        assert r(src1, dstf, flags=flags, mean=None, std=None) == UNSUPPORTED, flags
    # border modes: every one but TRANSPARENT
    for border in (REPLICATE, REFLECT, WRAP, REFLECT_101):
        assert r(src1, dstf, border=border) == INVALID, border  # the last check
    for border in (TRANSPARENT, -1, 6, 99):
        assert r(src1, dstf, border=border) == UNSUPPORTED, border
        assert r(src1, dstf, border=border, mean=None, std=None) == UNSUPPORTED, border
    # a source the bilinear sampler cannot tap
    assert r(img(0x1000, 1, 1, 8, 3), dstf, mean=None) == INVALID
    assert r(img(0x1000, 1, 8, 1, 3), dstf, std=None) == INVALID
    # a u8 destination
    assert r(src1, dst3) == INVALID and r(src1, img(0x2000, 3, 4, 4, 3, INT8, NCHW)) == INVALID
    assert r(src1, dst3, mean=None, std=None) == INVALID
    # planar output exists for 3 channels and for 1
    for c in (2, 4):
        assert r(img(0x1000, 1, 8, 8, c), img(0x2000, 3, 4, 4, c, FP32, NCHW)) == UNSUPPORTED, c
        assert r(img(0x1000, 1, 8, 8, c), img(0x2000, 3, 4, 4, c, FP32, NCHW), mean=None, std=None) == UNSUPPORTED
        assert r(img(0x1000, 1, 8, 8, c), img(0x2000, 3, 4, 4, c, FP32)) == INVALID, c  # NHWC: the last check
    assert r(img(0x1000, 1, 8, 8, 1), img(0x2000, 3, 4, 4, 1, FP32, NCHW)) == INVALID
    # order: the FP32 source is refused before a bad flag or border mode ...
    assert r(srcf, dstf, flags=INTER_NEAREST) == UNSUPPORTED and r(srcf, dstf, border=TRANSPARENT) == UNSUPPORTED
    # ... before the 2 x 2 rule's INVALID_ARG and before a u8 destination's
    assert r(img(0x1000, 1, 1, 8, 3, FP32), dstf) == UNSUPPORTED and r(srcf, dst3) == UNSUPPORTED
    # ... and the channel mismatch and the index rule before it
    assert r(srcf, img(0x2000, 3, 4, 4, 4, FP32)) == INVALID
    assert r(img(0x1000, 2, 8, 8, 3, FP32), dstf, idx=None) == INVALID
    # the options before the 2 x 2 rule, that before the destination's dtype, that before the planar counts
    assert r(img(0x1000, 1, 1, 8, 3), dstf, flags=INTER_NEAREST) == UNSUPPORTED
    assert r(img(0x1000, 1, 1, 8, 2), img(0x2000, 3, 4, 4, 2, FP32, NCHW)) == INVALID
    assert r(img(0x1000, 1, 8, 8, 2), img(0x2000, 3, 4, 4, 2, INT8, NCHW)) == INVALID


def test_the_old_entry_points_still_refuse_null_statistics(lib):
    by = ctypes.byref
    src, yuv = img(0x1000, 1, 8, 8, 3), img(0x1000, 1, 8, 12, 1)
    dstf = img(0x2000, 3, 4, 4, 3, FP32)
    rects = 0x6000
    bv = (ctypes.c_double * 4)(0, 0, 0, 0)
    assert lib.vacv_warp_affine_rois_normalize(by(src), by(dstf), MAPS, IDX, 1, 0, bv, None, None, None) == UNSUPPORTED
    assert lib.vacv_crop_resize_rois_normalize(by(src), by(dstf), rects, IDX, 1, 0, None, None, None) == UNSUPPORTED
    assert lib.vacv_cvt_color_warp_affine_rois_normalize(by(yuv), by(dstf), 93, MAPS, IDX, 1, 0, bv, None, None,
                                                         None) == UNSUPPORTED
    assert lib.vacv_cvt_color_crop_resize_rois_normalize(by(yuv), by(dstf), 93, rects, IDX, 1, 0, None, None,
                                                         None) == UNSUPPORTED


@pytest.mark.parametrize("c,w", [(1, 250), (3, 144), (4, 127), (1, 3), (3, 1500)])
def test_lds_gate(lib, c, w):
    """At a fixed width, the tallest ROI the documented formula admits passes
    the gate and one row more does not."""
    h = max(h for h in range(1, 70000) if lds_need(w, h, c) <= 65536)
    assert lds_need(w, h, c) <= 65536 < lds_need(w, h + 1, c)
    src = img(0x1000, 1, 64, 64, c)

    def r(hh, **kw):
        return call(lib, src, img(0x2000, 2, w, hh, c, FP32), **kw)

    assert r(h) == INVALID, (w, h)           # past the gate: refused by the last check only
    assert r(h + 1) == UNSUPPORTED and r(h + 1, mean=None, std=None) == UNSUPPORTED, (w, h + 1)
    assert r(h + 1, border=REFLECT_101, flags=INTER_LINEAR | INVERSE_MAP) == UNSUPPORTED
    assert r(1) == INVALID


def test_lds_arithmetic():
    assert lds_need(112, 112, 3) == 40960 and lds_need(128, 128, 3) == 52480
    assert lds_need(144, 144, 3) == 65536 and lds_need(145, 144, 3) > 65536
    assert 250 * 257 == 64250 and lds_need(250, 257, 1) == 256 + 64256 + 1024 <= 65536 < lds_need(250, 258, 1)
    # a ROI that fits has at most 65,536 - 256 - 1,024 = 64,256 pixels, so the
    # per-thread uint32 partial sums cannot overflow: Sum v^2 <= 64,256 * 255^2 < 2^32
    assert lds_need(64256, 1, 1) == 65536 < lds_need(64257, 1, 1)
    assert 64256 * 255 * 255 == 4178246400 < 2 ** 32


def test_other_limits(lib):
    src = img(0x1000, 1, 8, 8, 3)
    # a workgroup of 1,024 threads per ROI: the grid's threads fit 32 bits
    assert (2 ** 32 - 1) // 1024 == 4194303
    assert call(lib, src, img(0x2000, 4194303, 2, 2, 3, FP32)) == INVALID
    assert call(lib, src, img(0x2000, 4194304, 2, 2, 3, FP32)) == UNSUPPORTED
    assert call(lib, src, img(0x2000, 4194304, 2, 2, 3, FP32), mean=None, std=None) == UNSUPPORTED
    # one array for both statistics; distinct or NULL arrays pass (and would launch: not called here)
    assert call(lib, src, img(0x2000, 3, 4, 4, 3, FP32), mean=STATS, std=STATS) == INVALID


def test_binding_matches_header(lib):
    import subprocess

    import vacv_amd
    assert vacv_amd._lib.ABI_VERSION == 5 and lib.vacv_abi_version() == 5  # an added export does not bump it
    header = vacv_amd._lib.HEADER.read_text()
    assert "#define VACV_ABI_VERSION 5\n" in header
    exported = subprocess.run(["nm", "-D", "--defined-only", str(vacv_amd._lib.HIP_LIB)], capture_output=True,
                              text=True, check=True).stdout
    assert NAME in vacv_amd._lib.SIGNATURES and f"int {NAME}(" in header and f" T {NAME}\n" in exported
    assert len(vacv_amd._lib.SIGNATURES[NAME][0]) == 10
    assert "warp_affine_rois_standardize" in vacv_amd._OPS
    # the formula the header states is the one tested above
    assert "256 + 16 ceil(w h c / 16) + 1024 c bytes" in header


def test_byte_counting():
    """roofline.warp_affine_rois_standardize_bytes: fp32 output + statistics + each map's clipped source
    parallelogram, by hand, on a 64 x 48 frame and 16 x 8 outputs."""
    from vacv_amd import roofline
    ms = [[1, 0, 0, 0, 1, 0],        # identity: the source is the output's own 16 x 8 rectangle
          [0.5, 0, 10, 0, 0.5, 5],   # dst = src / 2 + (10, 5): the source is 32 x 16 at (-20, -10), 12 x 6 of it in
          [1, 0, 1000, 0, 1, 1000]]  # the source rectangle lies wholly off the frame: reads nothing
    out = 3 * 16 * 8 * 3 * 4
    src = (16 * 8 + 12 * 6) * 3
    f = roofline.warp_affine_rois_standardize_bytes
    assert f(64, 48, 3, 16, 8, ms) == out + src
    assert f(64, 48, 3, 16, 8, ms, stats=True) == out + 2 * 3 * 3 * 4 + src
    assert f(64, 48, 3, 16, 8, ms[2:]) == out // 3
    # the same maps given as dst -> src maps: [2] then reads the frame at (1000, 1000): still nothing;
    # [1] reads the 8 x 4 rectangle at (10, 5)
    assert f(64, 48, 3, 16, 8, ms, inverse_map=True) == out + (16 * 8 + 8 * 4) * 3
    assert f(64, 48, 3, 16, 8, np.zeros((0, 6), np.float32)) == 0
