"""vacv_cvt_color_match_template_rois on the GPU: many templates matched in
per-object search windows straight from NV21 / NV12 frames in one launch, with
each result's peaks (csrc/k_yuv_match_rois.hip).

No assertion is a tolerance.  Every case is compared, bit for bit (the map's
float bits, the vals doubles, idx), with two references:
  A  the contract: the product's chain, ops.cvt_color of all frames, then
     ops.match_template_rois on the decoded frames;
  B  independent: the oracle's yuv420sp_to_bgr of the indexed frame (`decode`
     of tests/test_yuv_rois_gpu.py), then ref_window_sums / ref_formula /
     ref_min_max_idx of tests/test_gpu_match.py on the numpy crop.
Frames are 130 x 98 decoded: rows of 130 bytes start at 2 modulo 4 and a dense
frame is 130 x 147 bytes.  The shapes are the smallest at which the staging can
go wrong: every residue of W modulo the four pixels of a staging item, odd and
even origins (taps straddling chroma pairs and chroma rows), the last Y byte
and the last chroma pair of a buffer, more staging items than a workgroup has
threads, more ROIs than CUs.
"""
from __future__ import annotations

import ctypes
import subprocess
from pathlib import Path

import numpy as np
import pytest

from test_gpu_match import ref_min_max_idx
from test_gpu_plumbing import SENTINEL, assert_bits, assert_rim_intact, assert_untouched, blank, host, place, unsupported
from test_match_rois_gpu import assert_same, lds_need, rand_u8, to_dev, want_numpy
from test_yuv_rois_gpu import CODE_IDS, CODES, all_pairs_frame, decode, make_yuv  # noqa: F401 (a fixture)

gpu = pytest.mark.gpu
SQDIFF, SQDIFF_NORMED, CCORR, CCORR_NORMED, CCOEFF, CCOEFF_NORMED = range(6)  # include/vacv_hip.h VACV_TM_*
ALL = tuple(range(6))
TWO = (SQDIFF_NORMED, CCOEFF_NORMED)
NV12_RGB, NV12_BGR, NV21_RGB, NV21_BGR = 90, 91, 92, 93
INT32_MAX = 2 ** 31 - 1
W, H = 130, 98  # decoded frames
IDX = [2, 0, 2, 1, 1, 0]  # mixed and repeated


@pytest.fixture(scope="module")
def ops(hip_device):
    from vacv_amd import ops
    return ops


@pytest.fixture(scope="module")
def dev(hip_device):
    return hip_device


@pytest.fixture(scope="module")
def frames3(oracle):
    """Three 130 x 98 frames and reference B's decode of them under every code, computed once."""
    yuv = make_yuv(3, W, H, 20261021)
    return yuv, {code: decode(oracle, yuv, code) for code in CODES}


def check(ops, dev, yuv, bgr, tpls, origins, idx, w, h, methods, code, what, d_yuv=None, chain=True):
    """One fused call per method against both references.  bgr: decode(oracle, yuv, code)."""
    d_yuv = to_dev(yuv, dev) if d_yuv is None else d_yuv
    d_tpls = to_dev(tpls, dev)
    d_tpl = d_tpls if len(tpls) > 1 else d_tpls[0]
    d_origins = to_dev(np.asarray(origins, np.int32), dev)
    d_idx = to_dev(np.asarray(idx, np.int32), dev) if idx is not None else None
    d_bgr = ops.cvt_color(d_yuv, code) if chain else None
    for method in methods:
        got = ops.cvt_color_match_template_rois(d_yuv, d_tpl, d_origins, w, h, method, code=code, src_index=d_idx)
        assert_same(got, want_numpy(bgr, tpls, origins, idx, w, h, method),
                    f"{what} {CODE_IDS[code]} method {method} vs the oracle's decode + numpy")
        if chain:
            want = ops.match_template_rois(d_bgr, d_tpl, d_origins, w, h, method, src_index=d_idx)
            assert_same(got, [host(x) for x in want], f"{what} {CODE_IDS[code]} method {method} vs the chain")


# ---------------------------------------------------------------------------
# 1. the shapes, the six methods, the four codes

#         tw th   W   H
SHAPES = [(1, 1, 1, 1),        # a 1 x 1 template and result: even and odd origins below
          (5, 4, 5, 4),        # the window is the template
          (5, 3, 9, 8),        # W * 3 = 27 bytes: the last staging item is partial, the zero padding matters
          (5, 3, 10, 8),       # ... and the other three residues of W modulo 4
          (5, 3, 11, 8),
          (5, 3, 12, 8),
          (3, 2, 67, 3),       # a result row of 65
          (2, 3, 4, 90),       # more than 256 four-pixel staging items in a single column of items
          (7, 5, 130, 5)]      # the whole frame width: rw = 124


def shape_origins(w, h):
    """Six windows: two corners, odd / even mixes, clamped into the frame."""
    pts = [(0, 0), (W - w, H - h), (5, 3), (2, 1), (4, 7), (7, 4)]
    return [[min(l, W - w), min(t, H - h)] for l, t in pts]


@gpu
@pytest.mark.parametrize("code", list(CODES), ids=lambda c: CODE_IDS[c])
@pytest.mark.parametrize("tw,th,w,h", SHAPES)
def test_shapes_methods_codes(ops, dev, frames3, tw, th, w, h, code):
    yuv, bgr = frames3
    tpls = rand_u8((6, th, tw, 3), 2000 + 13 * w + h)
    methods = ALL if code == NV21_BGR else TWO
    check(ops, dev, yuv, bgr[code], tpls, shape_origins(w, h), IDX, w, h, methods, code, f"{tw}x{th} in {w}x{h}")


# ---------------------------------------------------------------------------
# 2. origins: the corners, odd left and top (taps straddle chroma pairs and rows), the mixes

@gpu
@pytest.mark.parametrize("w,h", [(10, 8), (9, 7), (12, 9)])
def test_origins(ops, dev, frames3, w, h):
    yuv, bgr = frames3
    origins = [[0, 0], [W - w, H - h], [1, 1], [W - w - 1, H - h - 1], [4, 7], [7, 4],
               [W - w - (W - w) % 2, H - h - 1 + (H - h) % 2],     # even left, odd top, at the far edge
               [W - w - 1 + (W - w) % 2, H - h - (H - h) % 2]]     # odd left, even top
    if (w, h) == (10, 8):
        assert origins[3] == [119, 89] and origins[6] == [120, 89] and origins[7] == [119, 90]
    idx = [0, 2, 1, 2, 0, 1, 2, 0]
    tpls = rand_u8((8, 3, 5, 3), 300 + w)
    check(ops, dev, yuv, bgr[NV21_BGR], tpls, origins, idx, w, h, ALL, NV21_BGR, f"origins {w}x{h}")
    check(ops, dev, yuv, bgr[NV12_RGB], tpls[:1], origins, idx, w, h, TWO, NV12_RGB, f"origins {w}x{h} shared")


# ---------------------------------------------------------------------------
# 3. the frame as the last bytes of its buffer

@gpu
@pytest.mark.parametrize("off", [0, 1, 2, 3])
def test_frame_end(ops, dev, oracle, off):
    """The 130 x 98 frame as the last bytes of its buffer, at every base
    alignment, the windows in its bottom-right corner: a load reaching past
    the last chroma pair has nothing behind it."""
    import torch
    yuv = make_yuv(1, W, H, 700 + off)
    buf = torch.full((off + yuv.size,), SENTINEL, dtype=torch.uint8, device=dev)
    buf[off:] = to_dev(yuv.reshape(-1), dev)
    d_yuv = buf[off:].view(1, H * 3 // 2, W)
    assert d_yuv.data_ptr() + yuv.size == buf.data_ptr() + buf.numel()
    for code in (NV21_BGR, NV12_RGB):
        bgr = decode(oracle, yuv, code)
        for tw, th, w, h in [(1, 1, 1, 1), (5, 3, 9, 8), (5, 3, 12, 8), (3, 2, 67, 3)]:
            origins = [[W - w, H - h], [W - w - 1, H - h - 1], [W - w, H - h - 1]]
            check(ops, dev, yuv, bgr, rand_u8((3, th, tw, 3), 710 + w), origins, None, w, h, TWO, code,
                  f"off {off} {w}x{h}", d_yuv=d_yuv)
    assert_bits(host(buf)[:off], np.full(off, SENTINEL, np.uint8), "bytes before the frame")
    assert_bits(host(buf)[off:], yuv.reshape(-1), "the frame")


# ---------------------------------------------------------------------------
# 4. every chroma pair

def test_every_chroma_pair_lds_need():
    """What test_every_chroma_pair asks of a workgroup: about 20 KB (no GPU needed to know)."""
    # one template dword; window rows of 24 data dwords, 27 with the sliding window's reach; 32 x 32 x (3 + 1) sums
    assert lds_need(1, 1, 3, 32, 32) == 256 + 4 * (1 + 32 * 27 + 32 * 32 * 4) == 20100


@gpu
@pytest.mark.parametrize("code", [NV21_BGR, NV12_RGB], ids=lambda c: CODE_IDS[c])
def test_every_chroma_pair(ops, dev, oracle, all_pairs_frame, code):  # noqa: F811
    """256 windows of 32 x 32 tile the 512 x 512 frame of all 65,536 chroma
    pairs; under TM_CCORR a 1 x 1 template (1, 0, 0) makes the map channel 0 of
    the decoded window as exact floats, and so on."""
    yuv = all_pairs_frame
    bgr = decode(oracle, yuv, code)[0]
    d_yuv = to_dev(yuv, dev)
    origins = np.array([[32 * x, 32 * y] for y in range(16) for x in range(16)], np.int32)
    d_origins = to_dev(origins, dev)
    for ch in range(3):
        tpl = np.zeros((1, 1, 3), np.uint8)
        tpl[0, 0, ch] = 1
        res, vals, peaks = ops.cvt_color_match_template_rois(d_yuv, to_dev(tpl, dev), d_origins, 32, 32, CCORR, code=code)
        want = bgr[:, :, ch].astype(np.float32).reshape(16, 32, 16, 32).transpose(0, 2, 1, 3).reshape(256, 32, 32)
        assert_bits(host(res), want, f"{CODE_IDS[code]} channel {ch}")
        ref = [ref_min_max_idx(m) for m in want]
        assert_bits(host(vals), np.array([[r[0], r[1]] for r in ref], np.float64), f"channel {ch}: vals")
        assert_bits(host(peaks), np.array([[*r[2], *r[3]] for r in ref], np.int32), f"channel {ch}: idx")


# ---------------------------------------------------------------------------
# 5. placement: odd byte bases, pitched rows and batches, a pitched result

@gpu
def test_operand_placement(ops, dev, frames3):
    yuv, bgr = frames3
    w, h, tw, th, n = 14, 9, 5, 3, 4
    tpls = rand_u8((n, th, tw, 3), 33)
    origins = np.array([[0, 0], [W - w, H - h], [3, 2], [101, 77]], np.int32)
    idx = np.array([1, 0, 2, 0], np.int32)
    d_origins, d_idx = to_dev(origins, dev), to_dev(idx, dev)
    rw, rh = w - tw + 1, h - th + 1
    for off, row_pad, batch_pad in ((1, 0, 0), (2, 3, 0), (3, 5, 7), (0, 1, 2)):
        _, d_yuv4 = place(yuv[..., None], dev, off=off, row_pad=row_pad, batch_pad=batch_pad)
        d_yuv = d_yuv4[..., 0]
        _, d_tpls = place(tpls, dev, off=(off + 1) % 4, row_pad=batch_pad, batch_pad=row_pad)
        buf, out = place(blank((n, rh, rw, 1), np.float32), dev, off=4 * off, row_pad=row_pad, batch_pad=batch_pad)
        for code, method in ((NV21_BGR, SQDIFF_NORMED), (NV12_RGB, CCOEFF_NORMED)):
            what = f"off={off} pads {row_pad}, {batch_pad} {CODE_IDS[code]} method {method}"
            res, vals, peaks = ops.cvt_color_match_template_rois(d_yuv, d_tpls, d_origins, w, h, method, code=code,
                                                                 src_index=d_idx, out=out[..., 0])
            assert res.data_ptr() == out.data_ptr()
            assert_same((res, vals, peaks), want_numpy(bgr[code], tpls, origins, idx, w, h, method), what)
            chain = ops.match_template_rois(ops.cvt_color(d_yuv, code), d_tpls, d_origins, w, h, method, src_index=d_idx)
            assert_same((res, vals, peaks), [host(x) for x in chain], what + " vs the chain")
            assert_rim_intact(buf, out, what)  # the rim and the gaps between rows and ROIs


# ---------------------------------------------------------------------------
# 6. device-supplied garbage, judged against the decoded size

@gpu
def test_invalid_windows_and_indices(ops, dev, oracle):
    w, h, n_src, fw, fh = 10, 8, 2, 30, 20
    yuv, tpls = make_yuv(n_src, fw, fh, 61), rand_u8((1, 3, 4, 3), 62)
    bgr = decode(oracle, yuv, NV21_BGR)
    #           left        top          frame
    rois = [(4, 5, 0),
            (-1, 0, 0),                  # left = -1
            (fw - w, fh - h, 1),         # the last valid position
            (0, fh - h + 1, 1),          # top + H = h + 1: inside the YUV buffer's rows, outside the decoded frame
            (INT32_MAX, 0, 0),           # left + W overflows an int
            (3, 3, -1),                  # src_index = -1
            (3, 3, n_src),               # src_index = src->n
            (fw - w + 1, 0, 0),          # left + W = w + 1
            (0, -INT32_MAX - 1, 1),
            (0, INT32_MAX, 1),
            (7, 2, INT32_MAX),
            (20, 12, 1),
            (0, fh * 3 // 2 - h, 0)]     # the window's rows are the chroma rows
    valid = [0, 2, 11]
    origins = np.array([r[:2] for r in rois], np.int32)
    idx = np.array([r[2] for r in rois], np.int32)
    d_yuv, d_tpl = to_dev(yuv, dev), to_dev(tpls[0], dev)
    for method in (SQDIFF, CCOEFF_NORMED):
        res, vals, peaks = ops.cvt_color_match_template_rois(d_yuv, d_tpl, to_dev(origins, dev), w, h, method,
                                                             src_index=to_dev(idx, dev))  # returns: the call answered OK
        res, vals, peaks = host(res), host(vals), host(peaks)
        want = want_numpy(bgr, tpls, origins[valid], idx[valid], w, h, method)
        assert_same((res[valid], vals[valid], peaks[valid]), want, f"the valid neighbours, method {method}")
        bad = [i for i in range(len(rois)) if i not in valid]
        assert_bits(res[bad], np.zeros((len(bad), h - 2, w - 3), np.float32), "invalid ROIs are zeros")
        assert_bits(vals[bad], np.zeros((len(bad), 2), np.float64), "their vals")
        assert_bits(peaks[bad], np.full((len(bad), 4), -1, np.int32), "their idx")
    # a window larger than the decoded frame: every ROI is invalid
    for ww, hh in ((fw + 1, h), (w, fh + 1)):
        res, vals, peaks = ops.cvt_color_match_template_rois(d_yuv[0], d_tpl, to_dev(origins[:1] * 0, dev), ww, hh, SQDIFF)
        assert not host(res).any() and host(peaks).tolist() == [[-1] * 4] and host(vals).tolist() == [[0.0, 0.0]]


# ---------------------------------------------------------------------------
# 7. more ROIs than CUs

@gpu
@pytest.mark.parametrize("shared", [False, True], ids=["per_roi", "shared"])
def test_more_rois_than_cus(ops, dev, oracle, shared):
    """300 ROIs of a tiny 12 x 12 window on 4 frames: overlapping, identical and corner windows."""
    n, w, h, fw, fh = 300, 12, 12, 50, 40
    rng = np.random.default_rng(5)
    yuv = make_yuv(4, fw, fh, 21)
    bgr = decode(oracle, yuv, NV21_BGR)
    tpls = rand_u8((1 if shared else n, 4, 5, 3), 22)
    origins = np.stack([rng.integers(0, fw - w + 1, n), rng.integers(0, fh - h + 1, n)], 1).astype(np.int32)
    origins[10:14] = origins[9]                # identical windows
    origins[20] = [min(origins[19][0] + 1, fw - w), origins[19][1]]  # overlapping
    origins[0], origins[299] = [0, 0], [fw - w, fh - h]
    idx = rng.integers(0, 4, n).astype(np.int32)
    idx[10:12] = idx[9]                        # ... two of them in the same frame as well
    check(ops, dev, yuv, bgr, tpls, origins, idx, w, h, (CCOEFF_NORMED, SQDIFF), NV21_BGR, f"n=300 shared={shared}")


# ---------------------------------------------------------------------------
# 8. the LDS limit, peaks=False, statuses, the Python checks

@gpu
def test_lds_limit(ops, dev, oracle):
    """A ROI of exactly 64 KiB of LDS is computed (the decode adds none); 8
    bytes more are refused with nothing written."""
    assert lds_need(2, 9, 3, 51, 58) == 65536 and lds_need(2, 10, 3, 51, 57) == 65544
    w, h = 52, 66
    yuv = make_yuv(1, w + 4, h + 2, 71)
    check(ops, dev, yuv, decode(oracle, yuv, NV21_BGR), rand_u8((2, 9, 2, 3), 72), [[3, 1], [0, 0]], None, w, h, TWO,
          NV21_BGR, "64 KiB of LDS")
    buf, out = place(blank((2, 57, 51, 1), np.float32), dev)
    d_origins = to_dev(np.array([[3, 1], [0, 0]], np.int32), dev)
    unsupported(lambda: ops.cvt_color_match_template_rois(to_dev(yuv, dev), to_dev(rand_u8((2, 10, 2, 3), 73), dev),
                                                          d_origins, w, h, CCOEFF_NORMED, out=out[..., 0]))
    assert_untouched(buf, "past the LDS limit")


@gpu
def test_peaks_off_writes_the_same_maps(ops, dev, frames3):
    """peaks=False: only the maps, the same bytes; and through the C ABI with
    NULL vals / idx, sentinel-filled buffers standing where they would be."""
    import torch
    from vacv_amd import _lib
    yuv, _ = frames3
    tpls = rand_u8((3, 5, 7, 3), 82)
    origins, idx = np.array([[0, 0], [9, 5], [107, 80]], np.int32), np.array([1, 1, 0], np.int32)
    d = [to_dev(a, dev) for a in (yuv, tpls, origins, idx)]
    for method in (SQDIFF, CCOEFF_NORMED):
        res, _, _ = ops.cvt_color_match_template_rois(d[0], d[1], d[2], 23, 18, method, src_index=d[3])
        only = ops.cvt_color_match_template_rois(d[0], d[1], d[2], 23, 18, method, src_index=d[3], peaks=False)
        assert isinstance(only, torch.Tensor)
        assert_bits(host(only), host(res), f"peaks=False, method {method}")
    vals = torch.full((3 * 16,), SENTINEL, dtype=torch.uint8, device=dev)
    peaks = torch.full((3 * 16,), SENTINEL, dtype=torch.uint8, device=dev)
    out = torch.full((3, 14, 17), float("nan"), dtype=torch.float32, device=dev)
    by = ctypes.byref
    st = _lib.load().vacv_cvt_color_match_template_rois(
        by(ops.describe(d[0].unsqueeze(-1))), by(ops.describe(d[1])), by(ops.describe(out.unsqueeze(-1))), NV21_BGR,
        d[2].data_ptr(), d[3].data_ptr(), CCOEFF_NORMED, None, None, torch.cuda.current_stream().cuda_stream)
    assert st == 0
    assert_bits(host(out), host(res), "NULL vals / idx")
    assert_untouched(vals, "vals")
    assert_untouched(peaks, "idx")


@gpu
def test_statuses(ops, dev, frames3):
    """With real operands: what the entry point refuses, and that it writes nothing then."""
    import torch
    import vacv_amd as V
    L = V._lib
    yuv, _ = frames3
    d_yuv, d_tpl = to_dev(yuv, dev), to_dev(rand_u8((3, 5, 3), 91), dev)
    d_origins = to_dev(np.array([[0, 0], [3, 5]], np.int32), dev)
    buf, out = place(blank((2, 6, 6, 1), np.float32), dev)

    def status(fn):
        with pytest.raises(V.VacvError) as e:
            fn()
        return e.value.status

    def call(y=d_yuv[:1], t=d_tpl, **kw):
        return ops.cvt_color_match_template_rois(y, t, d_origins, 10, 8, CCORR, out=out[..., 0], **kw)

    for code in (L.COLOR_YUV2RGBA_NV12, L.COLOR_YUV2BGRA_NV12, L.COLOR_YUV2RGBA_NV21, L.COLOR_YUV2BGRA_NV21,
                 L.COLOR_YUV2BGR_YV12, L.COLOR_GRAY2BGR):
        assert status(lambda: call(code=code)) == L.ERR_UNSUPPORTED, code
    # odd w, and rows that are no h * 3 / 2 of an even h: as the sibling YUV calls answer
    for bad in (d_yuv[:1, :, :129].contiguous(), d_yuv[:1, :146].contiguous()):
        want = status(lambda: ops.cvt_color_crop_resize_rois(bad, to_dev(np.array([[0, 0, 4, 4]] * 2, np.int32), dev), 4, 4))
        assert status(lambda: call(y=bad)) == want == L.ERR_INVALID_ARG
    # templates of another channel count or dtype, FP32 frames: through the C ABI (the wrapper checks the former itself)
    by, lib = ctypes.byref, L.load()
    stream = torch.cuda.current_stream().cuda_stream

    def abi(y, t):
        return lib.vacv_cvt_color_match_template_rois(by(ops.describe(y.unsqueeze(-1))), by(ops.describe(t.unsqueeze(0))),
                                                      by(ops.describe(out)), NV21_BGR, d_origins.data_ptr(), None, CCORR,
                                                      None, None, stream)

    assert abi(d_yuv[:1], d_tpl) == 0
    buf2, out = place(blank((2, 6, 6, 1), np.float32), dev)
    for c in (1, 2, 4):
        assert abi(d_yuv[:1], to_dev(rand_u8((3, 5, c), 92), dev)) == L.ERR_INVALID_ARG, c
    assert abi(d_yuv[:1], d_tpl.float()) == L.ERR_INVALID_ARG
    assert abi(d_yuv[:1].float(), d_tpl) == L.ERR_INVALID_ARG
    assert abi(d_yuv[:1].float(), d_tpl.float()) == L.ERR_INVALID_ARG
    assert_untouched(buf2, "a refused call")


@gpu
def test_python_argument_checks(ops, dev, frames3):
    import torch
    yuv, bgr = frames3
    d_yuv = to_dev(yuv[:1], dev)
    tpl = to_dev(rand_u8((3, 4, 3), 92), dev)
    origins = torch.tensor([[0, 0], [3, 5]], dtype=torch.int32, device=dev)

    def fn(o, t=tpl, y=d_yuv, **kw):
        return ops.cvt_color_match_template_rois(y, t, o, 8, 8, CCORR, **kw)

    with pytest.raises(ValueError):
        fn(origins.cpu())                                  # a host tensor: the wrong device
    with pytest.raises(ValueError):
        fn(origins, t=tpl.cpu())
    with pytest.raises(ValueError):
        fn(origins.long())
    with pytest.raises(ValueError):
        fn(origins.reshape(1, 4))                          # shape
    with pytest.raises(ValueError):
        fn(origins, src_index=torch.zeros(2, dtype=torch.int64, device=dev))
    with pytest.raises(ValueError):
        fn(origins, src_index=torch.zeros(3, dtype=torch.int32, device=dev))
    with pytest.raises(ValueError):
        fn(origins, t=tpl[..., :1])                        # a one-channel template
    with pytest.raises(ValueError):
        fn(origins, t=tpl[0])                              # not (th, tw, 3)
    with pytest.raises(ValueError):
        fn(origins, y=to_dev(yuv, dev))                    # 3 frames, 2 windows, no index
    with pytest.raises(ValueError):
        ops.cvt_color_match_template_rois(d_yuv, tpl, origins, 3, 8, CCORR)   # the template is wider than the window
    with pytest.raises(ValueError):
        fn(origins, out=torch.empty((2, 5, 5), dtype=torch.float32, device=dev))
    # lists are moved for convenience; search_origins on the device, with the decoded size
    res, vals, peaks = fn([[0, 0], [3, 5]], src_index=[0, 0])
    assert tuple(res.shape) == (2, 6, 5) and tuple(vals.shape) == (2, 2) and tuple(peaks.shape) == (2, 4)
    o = ops.search_origins(torch.tensor([[7.9, 9.0], [1000.0, 97.0]], device=dev), 8, 8, W, H)
    assert o.device.type == "cuda" and host(o).tolist() == [[3, 5], [W - 8, H - 8]]
    got = fn(o)
    assert_bits(host(got[0])[0], host(res)[1], "origins from centres")
    assert_same(got, want_numpy(bgr[NV21_BGR][:1], host(tpl)[None], host(o), None, 8, 8, CCORR), "the clamped corner")
    # one (h * 3 / 2, w) frame without a batch dimension
    assert_same(fn(o, y=d_yuv[0]), [host(x) for x in got], "a 2-D frame")


# ---------------------------------------------------------------------------
# 9. the C++ layer

@gpu
def test_cpp_yuv_match_rois(hip_device, tmp_path):
    repo = Path(__file__).resolve().parent.parent
    pkg = repo / "arm-neon-opencv_amd"
    lib = pkg / "lib"
    exe = tmp_path / "vacv_yuv_match_rois_test"
    r = subprocess.run(["g++", "-std=c++14", "-O1", str(repo / "tests" / "cpp" / "vacv_yuv_match_rois_test.cpp"), "-o",
                        str(exe), "-I", str(pkg / "src"), "-L", str(lib), "-lvacv", "-lvacv_hip",
                        f"-Wl,-rpath,{lib}"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run(["timeout", "-k", "10", "120", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "failed 0" in r.stdout, r.stdout[-3000:]
