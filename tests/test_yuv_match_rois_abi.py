"""vacv_cvt_color_match_template_rois without a GPU: argument validation
(before any HIP call, with fake pointers, as test_match_rois_abi does), the
exported surface, the order of the checks and the roofline's byte count.

No call here reaches a launch: a case that has to show that a check was PASSED
gives vals without idx, which the entry point refuses with INVALID_ARG only
after every UNSUPPORTED limit (the order of the checks is part of its header
comment): descriptors and origin; code / method / dtype / layout; shapes;
limits; the vals / idx and src_index rules."""
from __future__ import annotations

import ctypes

import pytest

from test_match_rois_abi import lds_need

OK, INVALID, UNSUPPORTED = 0, -1, -2
FP32, FP16, INT8 = 0, 1, 2
NCHW, NHWC = 0, 1
CCOEFF_NORMED = 5
NV12_RGB, NV12_BGR, NV21_RGB, NV21_BGR = 90, 91, 92, 93
NAME = "vacv_cvt_color_match_template_rois"
SRC, TPL, RES, ORIGIN, IDX, VALS, PEAKS = 0x1000, 0x2000, 0x3000, 0x4000, 0x5000, 0x6000, 0x7000  # never dereferenced


@pytest.fixture(scope="module")
def lib():
    import vacv_amd
    if not vacv_amd._lib.HIP_LIB.exists():
        vacv_amd._lib.build()
    return vacv_amd._lib.load()


def img(ptr, n, w, h, c, dtype=INT8, layout=NHWC):
    from vacv_amd._lib import VacvImage
    return VacvImage(ptr, n, w, h, c, dtype, layout, 0, 0, 0)


def call(lib, src, tpl, res, code=NV21_BGR, origin=ORIGIN, idx=IDX, method=CCOEFF_NORMED, vals=VALS, peaks=PEAKS):
    by = ctypes.byref
    return lib.vacv_cvt_color_match_template_rois(by(src) if src else None, by(tpl) if tpl else None,
                                                  by(res) if res else None, code, origin, idx, method, vals, peaks,
                                                  None)


def test_yuv_match_rois_argument_validation_without_device(lib):
    """Every refusal below is answered before any HIP call; each case breaks one rule."""
    import vacv_amd
    src1, src2 = img(SRC, 1, 64, 72, 1), img(SRC, 2, 64, 72, 1)  # 64 x 48 decoded
    tpl1, tpl3 = img(TPL, 1, 5, 4, 3), img(TPL, 3, 5, 4, 3)
    res3 = img(RES, 3, 8, 6, 1, FP32)

    def r(src=src1, tpl=tpl1, res=res3, **kw):
        return call(lib, src, tpl, res, **kw)

    # the base case passes every check but the last
    assert r(vals=None) == INVALID and r(tpl=tpl3, vals=None) == INVALID
    # null descriptors / data
    assert r(src=None) == INVALID and r(tpl=None) == INVALID and r(res=None) == INVALID
    assert r(src=img(None, 1, 64, 72, 1)) == INVALID and r(res=img(None, 3, 8, 6, 1, FP32)) == INVALID
    # NULL origin
    assert r(origin=None) == INVALID and r(origin=None, idx=None) == INVALID
    # vals and idx: both or neither
    assert r(vals=None) == INVALID and r(peaks=None) == INVALID
    # src_index NULL: one frame for all, or one frame per ROI, nothing else
    assert r(src=src2, idx=None) == INVALID
    assert r(src=img(SRC, 3, 64, 72, 1), idx=None, vals=None) == INVALID  # accepted: the last check refuses
    # templates: one, or one per ROI
    for n in (2, 4):
        assert r(tpl=img(TPL, n, 5, 4, 3)) == INVALID, n
    # the four codes of the naive decode and nothing else: the OpenCV-arithmetic ones are UNSUPPORTED
    L = vacv_amd._lib
    for code in (L.COLOR_YUV2RGBA_NV12, L.COLOR_YUV2BGRA_NV12, L.COLOR_YUV2RGBA_NV21, L.COLOR_YUV2BGRA_NV21,
                 L.COLOR_YUV2BGR_YV12, L.COLOR_GRAY2BGR, -1, 0, 12345):
        assert r(code=code) == UNSUPPORTED, code
    assert (L.COLOR_YUV2RGB_NV12, L.COLOR_YUV2BGR_NV12, L.COLOR_YUV2RGB_NV21, L.COLOR_YUV2BGR_NV21) == \
        (NV12_RGB, NV12_BGR, NV21_RGB, NV21_BGR)
    for code in (NV12_RGB, NV12_BGR, NV21_RGB, NV21_BGR):
        assert r(code=code, vals=None) == INVALID, code  # accepted: refused only by the last check
    # the six VACV_TM_* and nothing else
    for method in (-1, 6, 99):
        assert r(method=method) == UNSUPPORTED, method
    for method in range(6):
        assert r(method=method, vals=None) == INVALID, method
    # the source is (w, h * 3 / 2, 1) INT8 NHWC with w and h even, as the sibling YUV calls take it
    assert r(src=img(SRC, 1, 64, 72, 1, FP32)) == INVALID and r(src=img(SRC, 1, 64, 72, 1, FP16)) == INVALID
    assert r(src=img(SRC, 1, 64, 72, 3)) == INVALID
    assert r(src=img(SRC, 1, 63, 72, 1)) == INVALID   # odd w
    for rows in (73, 74, 70, 1, 2):                   # not h * 3 / 2 of an even h >= 2 (an odd h: 49 + 24.5 rows)
        assert r(src=img(SRC, 1, 64, rows, 1)) == INVALID, rows
    over = dict(tpl=img(TPL, 1, 2, 10, 3), res=img(RES, 3, 51, 57, 1, FP32))  # reaches the limits: the shapes passed
    assert r(src=img(SRC, 1, 64, 75, 1), **over) == UNSUPPORTED and r(src=img(SRC, 1, 2, 3, 1), **over) == UNSUPPORTED
    # the template is (tw, th, 3) INT8 NHWC
    assert r(tpl=img(TPL, 1, 5, 4, 1)) == INVALID and r(tpl=img(TPL, 1, 5, 4, 4)) == INVALID
    assert r(tpl=img(TPL, 1, 5, 4, 3, FP32)) == INVALID
    assert r(tpl=img(TPL, 1, 5, 4, 3, INT8, NCHW)) == UNSUPPORTED
    # the result is one FP32 channel
    assert r(res=img(RES, 3, 8, 6, 1, INT8)) == INVALID and r(res=img(RES, 3, 8, 6, 3, FP32)) == INVALID


def test_yuv_match_rois_host_limits(lib):
    """The c = 3 LDS formula at exactly 64 KiB is accepted and 8 bytes more are
    not; tw * th = 66,001; result->n past a workgroup per ROI."""
    src = img(SRC, 1, 4096, 6144, 1)

    def r(tw, th, rw, rh, n=1, **kw):
        return call(lib, src, img(TPL, 1, tw, th, 3), img(RES, n, rw, rh, 1, FP32), **kw)

    assert lds_need(2, 9, 3, 51, 58) == 65536 and lds_need(2, 10, 3, 51, 57) == 65544
    assert r(2, 9, 51, 58, vals=None) == INVALID  # past the limits, refused by the last check
    assert r(2, 10, 51, 57) == UNSUPPORTED and r(2, 10, 51, 57, vals=None) == UNSUPPORTED
    assert lds_need(32, 32, 3, 33, 33) == 50688 and r(32, 32, 33, 33, vals=None) == INVALID  # the tracker shape fits
    assert 66001 == 13 * 5077 and r(5077, 13, 1, 1) == UNSUPPORTED and r(13, 5077, 1, 1) == UNSUPPORTED
    assert r(3, 3, 4, 4, n=(2 ** 32 - 1) // 256, vals=None) == INVALID
    assert r(3, 3, 4, 4, n=(2 ** 32 - 1) // 256 + 1) == UNSUPPORTED


def test_yuv_match_rois_check_order(lib):
    """Pairs of defects: the earlier group of the header's order answers."""
    src, tpl, res = img(SRC, 1, 64, 72, 1), img(TPL, 1, 5, 4, 3), img(RES, 3, 8, 6, 1, FP32)
    bad_code, bad_method = 12345, 99
    over = (img(TPL, 1, 2, 10, 3), img(RES, 3, 51, 57, 1, FP32))  # 8 bytes over the LDS limit
    # 1 before 2: a NULL origin (INVALID) with a bad code or method (UNSUPPORTED)
    assert call(lib, src, tpl, res, origin=None, code=bad_code) == INVALID
    assert call(lib, src, tpl, res, origin=None, method=bad_method) == INVALID
    assert call(lib, None, tpl, res, code=bad_code) == INVALID
    # 2 before 3: a bad code, method or template layout (UNSUPPORTED) with contradicting shapes (INVALID)
    assert call(lib, src, img(TPL, 2, 5, 4, 3), res, code=bad_code) == UNSUPPORTED
    assert call(lib, src, img(TPL, 1, 5, 4, 1), res, method=bad_method) == UNSUPPORTED
    assert call(lib, img(SRC, 1, 63, 72, 1), tpl, res, code=bad_code) == UNSUPPORTED
    assert call(lib, src, img(TPL, 2, 5, 4, 3, INT8, NCHW), res) == UNSUPPORTED
    # 3 before 4: contradicting shapes (INVALID) with a ROI over the LDS limit (UNSUPPORTED)
    assert call(lib, src, over[0], over[1]) == UNSUPPORTED
    assert call(lib, src, img(TPL, 2, 2, 10, 3), over[1]) == INVALID
    assert call(lib, img(SRC, 1, 63, 72, 1), over[0], over[1]) == INVALID
    assert call(lib, src, over[0], img(RES, 3, 51, 57, 1, INT8)) == INVALID
    # 4 before 5: over the limit (UNSUPPORTED) with vals without idx or a missing index (INVALID)
    assert call(lib, src, over[0], over[1], vals=None) == UNSUPPORTED
    assert call(lib, img(SRC, 2, 64, 72, 1), over[0], over[1], idx=None) == UNSUPPORTED


def test_yuv_match_rois_binding_matches_header(lib):
    import subprocess

    import vacv_amd
    assert vacv_amd._lib.ABI_VERSION == 5 and lib.vacv_abi_version() == 5  # an added export does not bump it
    header = vacv_amd._lib.HEADER.read_text()
    assert "#define VACV_ABI_VERSION 5" in header
    exported = subprocess.run(["nm", "-D", "--defined-only", str(vacv_amd._lib.HIP_LIB)], capture_output=True,
                              text=True, check=True).stdout
    assert NAME in vacv_amd._lib.SIGNATURES and f"int {NAME}(" in header and f" T {NAME}\n" in exported
    args, res = vacv_amd._lib.SIGNATURES[NAME]
    proto = header[header.index(f"int {NAME}("):]
    proto = proto[:proto.index(";")]
    assert len(args) == proto.count(",") + 1 == 10 and res is ctypes.c_int
    # descriptor pointers, the int code, two device arrays, the int method, two device arrays, the stream
    params = [p.strip() for p in proto[proto.index("(") + 1:proto.rindex(")")].split(",")]
    P, I, IMG = ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(vacv_amd._lib.VacvImage)
    kinds = [IMG if p.startswith("const vacv_image*") else I if p.startswith("int ") else P for p in params]
    assert kinds == [IMG, IMG, IMG, I, P, P, I, P, P, P] and list(args) == kinds
    from vacv_amd import cvt_color_match_template_rois, ops
    assert cvt_color_match_template_rois is ops.cvt_color_match_template_rois


def test_yuv_match_rois_byte_counting():
    """roofline.cvt_color_match_template_rois_bytes by hand: maps, peaks, Y, chroma pairs, templates."""
    from vacv_amd import roofline
    fn = roofline.cvt_color_match_template_rois_bytes
    # one 5 x 4 window, a 2 x 3 template: the map is 4 x 2 floats
    out = 4 * 2 * 4 + 32
    # even origin (2, 6): Y 20; chroma columns 2..6 -> pairs 1..3 (3), rows 6..9 -> chroma rows 3..4 (2): 3 * 2 pairs
    assert fn(5, 4, 2, 3, [[2, 6]]) == out + 20 + 2 * 3 * 2 + 2 * 3 * 3
    # odd origin (1, 1): columns 1..5 -> pairs 0..2 (3), rows 1..4 -> chroma rows 0..2 (3)
    assert fn(5, 4, 2, 3, [[1, 1]]) == out + 20 + 2 * 3 * 3 + 18
    assert fn(5, 4, 2, 3, [[1, 1]], peaks=False) == out - 32 + 20 + 18 + 18
    # invalid windows count their outputs only; with the frame's size an edge past it is invalid too
    assert fn(5, 4, 2, 3, [[-1, 0], [0, -2]]) == 2 * out
    assert fn(5, 4, 2, 3, [[2, 6]], w_in=6, h_in=10) == out and fn(5, 4, 2, 3, [[2, 6]], w_in=7, h_in=9) == out
    assert fn(5, 4, 2, 3, [[2, 6]], w_in=7, h_in=10) == out + 20 + 12 + 18
    # the tracker shape at an even origin: 64 x 64 of Y, 32 x 32 pairs, a 32 x 32 x 3 template
    assert fn(64, 64, 32, 32, [[10, 20]], n_templ=1) == 33 * 33 * 4 + 32 + 4096 + 2048 + 3072
    assert fn(64, 64, 32, 32, [[11, 21]]) == 33 * 33 * 4 + 32 + 4096 + 2 * 33 * 33 + 3072
    with pytest.raises(ValueError):
        fn(5, 4, 2, 3, [[0, 0], [1, 1], [2, 2]], n_templ=2)
