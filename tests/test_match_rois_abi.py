"""vacv_match_template_rois without a GPU: argument validation (before any HIP
call, with fake pointers, as test_crop_resize_rois_abi does), the exported
surface, the LDS formula at its limit, the host-side byte count of the roofline
and search_origins on CPU tensors.

No call here reaches a launch: a case that has to show that a check was PASSED
(the LDS need at exactly 64 KiB) gives vals without idx, which the entry point
refuses with INVALID_ARG only after every UNSUPPORTED limit (the order of the
checks is part of its header comment)."""
from __future__ import annotations

import ctypes

import numpy as np
import pytest

OK, INVALID, UNSUPPORTED = 0, -1, -2
FP32, FP16, INT8 = 0, 1, 2
NCHW, NHWC = 0, 1
CCOEFF_NORMED = 5
NAME = "vacv_match_template_rois"
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


def lds_need(tw, th, cn, rw, rh):
    """The header comment's formula (csrc/k_match_rois.hip match_rois_lds_bytes), restated."""
    k4 = (tw * cn + 3) // 4
    g = (rw + 3) // 4
    w, h = rw + tw - 1, rh + th - 1
    ws4 = max((w * cn + 3) // 4, (g - 1) * cn + k4 + (3 * cn) // 4 + 2) | 1
    return 256 + 4 * (th * k4 + h * ws4 + h * rw * (cn + 1))


def call(lib, src, tpl, res, origin=ORIGIN, idx=IDX, method=CCOEFF_NORMED, vals=VALS, peaks=PEAKS):
    by = ctypes.byref
    return lib.vacv_match_template_rois(by(src) if src else None, by(tpl) if tpl else None, by(res) if res else None,
                                        origin, idx, method, vals, peaks, None)


def test_match_rois_argument_validation_without_device(lib):
    """Every refusal below is answered before any HIP call; each case breaks one rule."""
    src1, src2 = img(SRC, 1, 64, 48, 3), img(SRC, 2, 64, 48, 3)
    tpl1, tpl3 = img(TPL, 1, 5, 4, 3), img(TPL, 3, 5, 4, 3)
    res3 = img(RES, 3, 8, 6, 1, FP32)

    def r(src=src1, tpl=tpl1, res=res3, **kw):
        return call(lib, src, tpl, res, **kw)

    # null descriptors / data
    assert r(src=None) == INVALID and r(tpl=None) == INVALID and r(res=None) == INVALID
    assert r(src=img(None, 1, 64, 48, 3)) == INVALID and r(res=img(None, 3, 8, 6, 1, FP32)) == INVALID
    # NULL origin
    assert r(origin=None) == INVALID and r(origin=None, idx=None) == INVALID
    # vals and idx: both or neither
    assert r(vals=None) == INVALID and r(peaks=None) == INVALID
    # src_index NULL: one frame for all, or one frame per ROI, nothing else
    assert r(src=src2, idx=None) == INVALID
    # templates: one, or one per ROI
    for n in (2, 4):
        assert r(tpl=img(TPL, n, 5, 4, 3)) == INVALID, n
    assert r(tpl=tpl3, vals=None) == INVALID  # n templates pass that check and reach the last one
    # the template's dtype and channels are the frame's
    assert r(tpl=img(TPL, 1, 5, 4, 1)) == INVALID
    assert r(tpl=img(TPL, 1, 5, 4, 3, FP32)) == INVALID
    # the result is one FP32 channel
    assert r(res=img(RES, 3, 8, 6, 1, INT8)) == INVALID and r(res=img(RES, 3, 8, 6, 3, FP32)) == INVALID
    # FP32 (and every other dtype) is not built; nor are NCHW frames or five channels
    assert r(src=img(SRC, 1, 64, 48, 3, FP32), tpl=img(TPL, 1, 5, 4, 3, FP32)) == UNSUPPORTED
    assert r(src=img(SRC, 1, 64, 48, 3, FP16), tpl=img(TPL, 1, 5, 4, 3, FP16)) == UNSUPPORTED
    assert r(src=img(SRC, 1, 64, 48, 3, INT8, NCHW)) == UNSUPPORTED
    assert r(tpl=img(TPL, 1, 5, 4, 3, INT8, NCHW)) == UNSUPPORTED
    assert r(src=img(SRC, 1, 64, 48, 5), tpl=img(TPL, 1, 5, 4, 5)) == UNSUPPORTED
    # the six VACV_TM_* and nothing else, as vacv_match_template answers
    for method in (-1, 6, 99):
        assert r(method=method) == UNSUPPORTED, method
    for method in range(6):
        assert r(method=method, vals=None) == INVALID, method  # accepted: refused only by the last check


def test_match_rois_host_limits(lib):
    """The LDS formula at exactly 64 KiB is accepted and 4 bytes more -- its
    smallest step -- are not; tw * th = 66,001; result->n past a workgroup per ROI."""
    src = img(SRC, 1, 4096, 4096, 1)

    def r(tw, th, rw, rh, n=1, **kw):
        return call(lib, src, img(TPL, 1, tw, th, 1), img(RES, n, rw, rh, 1, FP32), **kw)

    assert lds_need(3, 29, 1, 79, 62) == 65532 and lds_need(3, 30, 1, 79, 61) == 65536
    assert lds_need(3, 31, 1, 79, 60) == 65540
    for tw, th, rw, rh in ((3, 29, 79, 62), (3, 30, 79, 61)):
        assert r(tw, th, rw, rh, vals=None) == INVALID, (tw, th, rw, rh)  # past the limits, refused by the last check
    assert r(3, 31, 79, 60) == UNSUPPORTED and r(3, 31, 79, 60, vals=None) == UNSUPPORTED
    assert lds_need(32, 32, 3, 33, 33) == 50688  # the tracker shape of the README fits
    # the uint32 window sums' bound: 66,000 template pixels
    assert 251 * 263 == 66013 and 250 * 264 == 66000
    assert r(251, 263, 1, 1) == UNSUPPORTED
    assert lds_need(250, 264, 1, 1, 1) > 65536 and r(250, 264, 1, 1) == UNSUPPORTED  # (its LDS need refuses it too)
    assert 66001 == 13 * 5077 and r(5077, 13, 1, 1) == UNSUPPORTED and r(13, 5077, 1, 1) == UNSUPPORTED
    # a workgroup of 256 threads per ROI: the grid's threads fit 32 bits
    assert r(3, 3, 4, 4, n=(2 ** 32 - 1) // 256, vals=None) == INVALID
    assert r(3, 3, 4, 4, n=(2 ** 32 - 1) // 256 + 1) == UNSUPPORTED


def test_match_rois_binding_matches_header(lib):
    import subprocess

    import vacv_amd
    assert vacv_amd._lib.ABI_VERSION == 5 and lib.vacv_abi_version() == 5  # an added export does not bump it
    header = vacv_amd._lib.HEADER.read_text()
    exported = subprocess.run(["nm", "-D", "--defined-only", str(vacv_amd._lib.HIP_LIB)], capture_output=True,
                              text=True, check=True).stdout
    assert NAME in vacv_amd._lib.SIGNATURES and f"int {NAME}(" in header and f" T {NAME}\n" in exported
    args, res = vacv_amd._lib.SIGNATURES[NAME]
    proto = header[header.index(f"int {NAME}("):]
    proto = proto[:proto.index(";")]
    assert len(args) == proto.count(",") + 1 == 9 and res is ctypes.c_int
    from vacv_amd import match_template_rois, ops, search_origins
    assert match_template_rois is ops.match_template_rois and search_origins is ops.search_origins


def test_match_rois_byte_counting():
    """roofline.match_template_rois_bytes by hand: maps, peaks, windows and templates."""
    from vacv_amd import roofline
    origins = [[0, 0], [10, 5], [-1, 0], [0, -3]]
    maps, peaks = 4 * 33 * 33 * 4, 4 * (16 + 16)
    read = 2 * (64 * 64 + 32 * 32) * 3  # the two valid windows and their templates
    assert roofline.match_template_rois_bytes(3, 64, 64, 32, 32, origins) == maps + peaks + read
    assert roofline.match_template_rois_bytes(3, 64, 64, 32, 32, origins, n_templ=4) == maps + peaks + read
    assert roofline.match_template_rois_bytes(3, 64, 64, 32, 32, origins, peaks=False) == maps + read
    # with the frame's size a window past its edge is invalid as well
    assert roofline.match_template_rois_bytes(3, 64, 64, 32, 32, origins, w_in=73, h_in=69) == \
        maps + peaks + (64 * 64 + 32 * 32) * 3
    assert roofline.match_template_rois_bytes(3, 64, 64, 32, 32, origins, w_in=74, h_in=69) == maps + peaks + read
    assert roofline.match_template_rois_bytes(1, 9, 8, 9, 8, [[2, 3]]) == 4 + 32 + 2 * 72
    assert roofline.match_template_rois_bytes(3, 64, 64, 32, 32, np.zeros((0, 2), np.int32)) == 0
    with pytest.raises(ValueError):
        roofline.match_template_rois_bytes(3, 64, 64, 32, 32, origins, n_templ=2)


def test_search_origins_truncates_and_clamps():
    """On CPU tensors: (int(cx) - w // 2, int(cy) - h // 2), toward zero, clamped into the frame."""
    import torch
    from vacv_amd import ops
    centers = np.array([[100.0, 50.0],
                        [100.9, 50.9],          # toward zero: as 100, 50
                        [31.99, 32.0],          # 31 - 32 < 0: clamped to 0; 32 - 32 = 0
                        [-5.5, -0.9],           # toward zero, then clamped
                        [1919.0, 1079.0],       # the far corner: clamped to frame - window
                        [1887.5, 1047.99],      # the last position that needs no clamp
                        [1e9, -1e9]], np.float32)
    got = ops.search_origins(torch.from_numpy(centers), 64, 64, 1920, 1080)
    assert got.dtype == torch.int32 and tuple(got.shape) == (7, 2) and got.is_contiguous()
    want = np.array([[68, 18], [68, 18], [0, 0], [0, 0], [1856, 1016], [1855, 1015], [1856, 0]], np.int32)
    assert np.array_equal(got.numpy(), want)
    # odd sizes: w // 2
    got = ops.search_origins(torch.tensor([[10, 10], [3, 2]], dtype=torch.int32), 9, 5, 20, 20)
    assert np.array_equal(got.numpy(), np.array([[6, 8], [0, 0]], np.int32))
    # a window of the frame's size has one position
    assert ops.search_origins(torch.tensor([[7.0, 3.0]]), 20, 20, 20, 20).tolist() == [[0, 0]]
    with pytest.raises(ValueError):
        ops.search_origins(torch.from_numpy(centers.astype(np.float64)), 64, 64, 1920, 1080)
    with pytest.raises(ValueError):
        ops.search_origins(torch.from_numpy(centers.reshape(2, 7)), 64, 64, 1920, 1080)
    with pytest.raises(ValueError):
        ops.search_origins(torch.from_numpy(centers), 64, 1081, 1920, 1080)
