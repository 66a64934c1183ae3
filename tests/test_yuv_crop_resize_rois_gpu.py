"""vacv_cvt_color_crop_resize_rois[_normalize] on the GPU: many upright crop +
resize ROIs straight from NV21 / NV12 frames in one launch
(csrc/k_yuv_crop_resize_rois.hip).

Every comparison is bit-exact, and the expected ROI is computed two ways that
both have to equal the result:
 (a) on the host: the oracle's yuv420sp_to_bgr of the indexed frame, then its
     crop and resize_linear (+ u8_to_f32, normalize, hwc_to_chw);
 (b) on the GPU: ops.cvt_color of all frames, then ops.crop_resize_rois
     [_normalize] on the decoded frames -- the chain the call replaces.
Frames are 130 x 98: even rows of 130 bytes start at 2 modulo 4, a dense frame
is 130 x 147 bytes.  The rects reach both corners of the frame (the last Y
bytes and the last chroma pair), odd origins (the two taps straddle two chroma
pairs and two chroma rows), every edge, up- and down-scales and the output's
own size; the output sizes reach every path of the kernel (two 1024-pixel
tiles split mid-row, one pixel, one row, one column, wider than a tile).
"""
from __future__ import annotations

import subprocess
from pathlib import Path

import numpy as np
import pytest

from test_crop_resize_rois_gpu import oracle_normalized, oracle_roi, oracle_rois, to_dev, to_planar, view_in_buffer
from test_gpu_plumbing import SENTINEL, assert_bits, assert_rim_intact, host, place
from test_yuv_rois_gpu import CODE_IDS, CODES, DST_CASES, all_pairs_frame, decode, make_yuv  # noqa: F401 (a fixture)

gpu = pytest.mark.gpu
NHWC, NCHW = 1, 0
REFERENCE, NEON, OPENCV = 0, 1, 2
MODES = (REFERENCE, NEON, OPENCV)
NV12_RGB, NV12_BGR, NV21_RGB, NV21_BGR = 90, 91, 92, 93
W, H = 130, 98   # decoded frames
WO, HO = 37, 29  # 1,073 pixels: two tiles, the boundary falls mid-row
INT32_MAX = 2 ** 31 - 1
MEAN3 = np.array([104.5, 117.25, 123.0], np.float32)
STD3 = np.array([57.375, 57.12, 58.395], np.float32)

# (left, top, width, height) in the decoded 130 x 98 frame
RECTS = np.array([
    [0, 0, W, H],             # the whole frame
    [0, 0, 2, 2],             # the smallest rect at both corners:
    [W - 2, H - 2, 2, 2],     # ... the last Y bytes and the last chroma pair
    [1, 1, 2, 2],             # odd origin: the taps straddle two chroma pairs and two chroma rows,
    [W - 3, H - 3, 3, 3],     # ... at the frame's end too
    [40, 10, 90, 20],         # the right edge
    [10, 30, 30, 68],         # the bottom edge
    [21, 11, 5, 3],           # up-scale, odd left
    [3, 2, 120, 90],          # down-scale by more than 2
    [13, 7, WO, HO],          # the output's own size at an odd
    [12, 8, WO, HO],          # ... and at an even origin: the decoded crop
    [31, 2, 3, 95],           # extreme aspect
    [4, 22, 121, 2],
    [17, 9, 31, 23],          # primes
], np.int32)
IDX = np.array([2, 0, 0, 1, 2, 2, 1, 0, 1, 2, 0, 1, 1, 0], np.int32)  # mixed and repeated
assert (RECTS[:, 0] + RECTS[:, 2] <= W).all() and (RECTS[:, 1] + RECTS[:, 3] <= H).all() and len(IDX) == len(RECTS)


@pytest.fixture(scope="module")
def ops(hip_device):
    from vacv_amd import ops
    return ops


@pytest.fixture(scope="module")
def dev(hip_device):
    return hip_device


def normalized(oracle, rois, layout):
    """(a): u8 ROIs [n, ho, wo, 3] -> fp32, normalized, NHWC or NCHW."""
    f = oracle_normalized(oracle, rois, MEAN3, STD3)
    return f if layout == NHWC else to_planar(oracle, f)


def check_both(ops, oracle, got, yuv, d_yuv, code, idx, rects, d_rects, d_idx, wo, ho, mode, what, layout=None):
    """got == (a) the host chain == (b) the GPU chain on the decoded frames."""
    want = oracle_rois(oracle, decode(oracle, yuv if yuv.ndim == 3 else yuv[None], code), idx, rects, wo, ho, mode)
    bgr = ops.cvt_color(d_yuv, code)
    if layout is None:
        chain = ops.crop_resize_rois(bgr, d_rects, wo, ho, src_index=d_idx, mode=mode)
    else:
        want = normalized(oracle, want, layout)
        chain = ops.crop_resize_rois_normalize(bgr, d_rects, wo, ho, MEAN3, STD3, src_index=d_idx, mode=mode,
                                               layout=layout)
    got = host(got)
    for i in range(len(rects)):
        assert_bits(got[i], want[i], f"{what} roi {i} rect {np.asarray(rects[i]).tolist()} vs oracle")
    assert_bits(got, host(chain), what + " vs cvt_color + crop_resize_rois")
    return want


# ---------------------------------------------------------------------------
# 1. parity: every code, every mode

@gpu
@pytest.mark.parametrize("mode", MODES, ids=["reference", "neon", "opencv"])
@pytest.mark.parametrize("code", list(CODES), ids=lambda c: CODE_IDS[c])
def test_parity(ops, dev, oracle, code, mode):
    import torch
    yuv = make_yuv(3, W, H, 500 + code)
    d_yuv, d_rects, d_idx = to_dev(yuv, dev), to_dev(RECTS, dev), to_dev(IDX, dev)
    bgr = decode(oracle, yuv, code)
    assert_bits(host(ops.cvt_color(d_yuv, code)), bgr, "cvt_color vs oracle")
    # 1025 columns: wider than a tile, the column taps are computed per pixel
    for wo, ho in [(WO, HO), (112, 112), (1, 1), (1, 7), (9, 1), (1025, 3)]:
        what = f"{CODE_IDS[code]} mode {mode} {wo}x{ho}"
        got = ops.cvt_color_crop_resize_rois(d_yuv, d_rects, wo, ho, code=code, src_index=d_idx, mode=mode)
        assert tuple(got.shape) == (len(RECTS), ho, wo, 3) and got.dtype == torch.uint8
        check_both(ops, oracle, got, yuv, d_yuv, code, IDX, RECTS, d_rects, d_idx, wo, ho, mode, what)
        if (wo, ho) == (WO, HO):  # a rect of the output's own size is the decoded crop itself
            for i in (9, 10):
                l, t, w, h = RECTS[i]
                assert_bits(host(got)[i], bgr[IDX[i], t:t + h, l:l + w], f"{what}: identity size, rect {RECTS[i].tolist()}")


# ---------------------------------------------------------------------------
# 2. fused normalize, NHWC and NCHW

@gpu
@pytest.mark.parametrize("layout", [NHWC, NCHW], ids=["nhwc", "nchw"])
@pytest.mark.parametrize("code", [NV21_BGR, NV12_RGB], ids=lambda c: CODE_IDS[c])
def test_normalize(ops, dev, oracle, code, layout):
    import torch
    yuv = make_yuv(3, W, H, 600 + code)
    d_yuv, d_rects, d_idx = to_dev(yuv, dev), to_dev(RECTS, dev), to_dev(IDX, dev)
    for wo, ho in [(WO, HO), (5, 3)]:
        for mode in MODES:
            got = ops.cvt_color_crop_resize_rois_normalize(d_yuv, d_rects, wo, ho, MEAN3, STD3, code=code, src_index=d_idx,
                                                           mode=mode, layout=layout)
            assert got.dtype == torch.float32
            assert tuple(got.shape) == ((len(RECTS), ho, wo, 3) if layout == NHWC else (len(RECTS), 3, ho, wo))
            check_both(ops, oracle, got, yuv, d_yuv, code, IDX, RECTS, d_rects, d_idx, wo, ho, mode,
                       f"{CODE_IDS[code]} layout {layout} {wo}x{ho} mode {mode}", layout=layout)


# ---------------------------------------------------------------------------
# 3. taps clamp at the rect's edge, not the frame's

@gpu
@pytest.mark.parametrize("code", [NV21_BGR, NV12_RGB], ids=lambda c: CODE_IDS[c])
def test_taps_clamp_at_the_rect_edge(ops, dev, oracle, code):
    """The frame decodes to one colour inside the rect and to another outside
    it (even origin, even size: no chroma pair straddles the edge), up-scaled
    x 4: one tap past the rect's edge would show as another colour."""
    l, t, w, h = 10, 6, 8, 4
    yuv = np.zeros((1, 30, 32), np.uint8)  # 32 x 20 decoded
    yuv[0, :20] = 200
    yuv[0, 20:, 0::2], yuv[0, 20:, 1::2] = 30, 220
    yuv[0, t:t + h, l:l + w] = 90
    yuv[0, 20 + t // 2:20 + (t + h) // 2, l:l + w:2] = 100
    yuv[0, 20 + t // 2:20 + (t + h) // 2, l + 1:l + w:2] = 160
    bgr = decode(oracle, yuv, code)[0]
    inside = bgr[t, l].copy()
    assert (bgr[t:t + h, l:l + w] == inside).all(), "one colour inside"
    outside = bgr[0, 0].copy()
    mask = np.ones((20, 32), bool)
    mask[t:t + h, l:l + w] = False
    assert (bgr[mask] == outside).all() and (outside != inside).all(), "another one outside, in every channel"
    d_yuv, d_rect = to_dev(yuv, dev), to_dev(np.array([[l, t, w, h]], np.int32), dev)
    want = np.broadcast_to(inside, (1, 4 * h, 4 * w, 3))
    for mode in MODES:
        got = ops.cvt_color_crop_resize_rois(d_yuv, d_rect, 4 * w, 4 * h, code=code, mode=mode)
        assert_bits(host(got), want, f"mode {mode}")
        check_both(ops, oracle, got, yuv, d_yuv, code, [0], [[l, t, w, h]], d_rect, None, 4 * w, 4 * h, mode, f"mode {mode}")
        gotn = ops.cvt_color_crop_resize_rois_normalize(d_yuv, d_rect, 4 * w, 4 * h, MEAN3, STD3, code=code, mode=mode,
                                                        layout=NCHW)
        assert_bits(host(gotn), normalized(oracle, want, NCHW), f"normalized, mode {mode}")


# ---------------------------------------------------------------------------
# 4. every chroma pair

@gpu
@pytest.mark.parametrize("code", list(CODES), ids=lambda c: CODE_IDS[c])
def test_every_chroma_pair(ops, dev, oracle, all_pairs_frame, code):  # noqa: F811
    yuv = all_pairs_frame
    d_yuv = to_dev(yuv, dev)
    decoded = ops.cvt_color(d_yuv, code)
    assert_bits(host(decoded), decode(oracle, yuv, code), "cvt_color vs oracle")
    whole = np.array([[0, 0, 512, 512]], np.int32)
    d_whole = to_dev(whole, dev)
    # the whole frame at its own size is the decoded frame itself
    got = ops.cvt_color_crop_resize_rois(d_yuv, d_whole, 512, 512, code=code)
    assert_bits(host(got), host(decoded), f"{CODE_IDS[code]}: identity")
    # x 1.25: every neighbouring tap pair and row pair blended
    got = ops.cvt_color_crop_resize_rois(d_yuv, d_whole, 640, 640, code=code)
    check_both(ops, oracle, got, yuv, d_yuv, code, [0], whole, d_whole, None, 640, 640, REFERENCE,
               f"{CODE_IDS[code]}: 512 -> 640")


# ---------------------------------------------------------------------------
# 5. the frame's end and tiny frames

END_RECTS = np.array([[W - 2, H - 2, 2, 2], [W - 3, H - 3, 3, 3], [100, 80, 30, 18]], np.int32)


@gpu
@pytest.mark.parametrize("off", [0, 1, 2, 3])
def test_frame_end(ops, dev, oracle, off):
    """The 130 x 98 frame as the last bytes of its buffer, at every base
    alignment: a load reaching past the last chroma pair has nothing behind it."""
    import torch
    yuv = make_yuv(1, W, H, 700 + off)
    buf = torch.full((off + yuv.size,), SENTINEL, dtype=torch.uint8, device=dev)
    buf[off:] = to_dev(yuv.reshape(-1), dev)
    d_yuv = buf[off:].view(1, H * 3 // 2, W)
    assert d_yuv.data_ptr() + yuv.size == buf.data_ptr() + buf.numel()
    d_rects = to_dev(END_RECTS, dev)
    idx = [0] * len(END_RECTS)
    for wo, ho in [(WO, HO), (5, 3)]:
        for code in (NV21_BGR, NV12_RGB):
            for mode in (REFERENCE, NEON):
                what = f"off {off} {CODE_IDS[code]} {wo}x{ho} mode {mode}"
                got = ops.cvt_color_crop_resize_rois(d_yuv, d_rects, wo, ho, code=code, mode=mode)
                check_both(ops, oracle, got, yuv, d_yuv, code, idx, END_RECTS, d_rects, None, wo, ho, mode, what)
                gotn = ops.cvt_color_crop_resize_rois_normalize(d_yuv, d_rects, wo, ho, MEAN3, STD3, code=code, mode=mode,
                                                                layout=NCHW)
                check_both(ops, oracle, gotn, yuv, d_yuv, code, idx, END_RECTS, d_rects, None, wo, ho, mode,
                           what + " normalized", layout=NCHW)
    assert_bits(host(buf)[:off], np.full(off, SENTINEL, np.uint8), "bytes before the frame")
    assert_bits(host(buf)[off:], yuv.reshape(-1), "the frame")


def all_valid_rects(w, h):
    return [[l, t, cw, ch] for cw in range(2, w + 1) for ch in range(2, h + 1)
            for l in range(w - cw + 1) for t in range(h - ch + 1)]


@gpu
@pytest.mark.parametrize("w,h", [(2, 2), (4, 2), (6, 4)])
def test_tiny_frames(ops, dev, oracle, w, h):
    yuv = make_yuv(2, w, h, 800 + w)
    d_yuv = to_dev(yuv, dev)
    rects = all_valid_rects(w, h)
    assert len(rects) == {2: 1, 4: 6, 6: 90}[w]
    if w == 6:  # a handful: the frame, its corners at odd and even origins, odd sizes
        rects = [[0, 0, 6, 4], [4, 2, 2, 2], [3, 1, 3, 3], [1, 1, 2, 2], [0, 0, 5, 3], [1, 0, 5, 4], [2, 2, 4, 2]]
    rects = np.array(rects, np.int32)
    idx = np.array([i % 2 for i in range(len(rects))], np.int32)
    d_rects, d_idx = to_dev(rects, dev), to_dev(idx, dev)
    for wo, ho in [(8, 8), (5, 3)]:
        for code in (NV21_BGR, NV12_RGB):
            for mode in MODES:
                got = ops.cvt_color_crop_resize_rois(d_yuv, d_rects, wo, ho, code=code, src_index=d_idx, mode=mode)
                check_both(ops, oracle, got, yuv, d_yuv, code, idx, rects, d_rects, d_idx, wo, ho, mode,
                           f"{w}x{h} frame {CODE_IDS[code]} {wo}x{ho} mode {mode}")


# ---------------------------------------------------------------------------
# 6. pitched, misaligned

SIZES6 = [(WO, HO), (140, 9), (5, 3)]


@pytest.fixture(scope="module")
def pitched_reference(oracle):
    """Frames and (a) for the pitched cases, computed once."""
    yuv = make_yuv(3, W, H, 900)
    bgr = decode(oracle, yuv, NV21_BGR)
    return yuv, {(wo, ho): oracle_rois(oracle, bgr, IDX, RECTS, wo, ho, REFERENCE) for wo, ho in SIZES6}


@gpu
@pytest.mark.parametrize("row_pad", [0, 5, 14], ids=lambda p: f"pitch{130 + p}")
@pytest.mark.parametrize("soff", [0, 1, 2, 3])
def test_pitched_misaligned(ops, dev, oracle, pitched_reference, soff, row_pad):
    assert len(DST_CASES) == 8  # 5 u8, 2 fp32 NCHW, 1 fp32 NHWC
    yuv, ref = pitched_reference
    n = len(RECTS)
    sbuf, sview = place(yuv[..., None], dev, NHWC, off=soff, row_pad=row_pad, batch_pad=7)
    d_yuv = sview[..., 0]
    assert d_yuv.stride() == ((H * 3 // 2) * (W + row_pad) + 7, W + row_pad, 1)
    d_rects, d_idx = to_dev(RECTS, dev), to_dev(IDX, dev)
    d_bgr = ops.cvt_color(d_yuv, NV21_BGR)
    for (wo, ho) in SIZES6:
        want_u8 = ref[(wo, ho)]
        for case in DST_CASES:
            _, c, out, _, _, doff, rpad, ppad, bpad = case
            odt = np.uint8 if out == "same" else np.float32
            if out == NCHW:
                rp = wo + rpad
                pl = ho * rp + ppad
                shape, strides = (n, c, ho, wo), (c * pl + bpad, pl, rp, 1)
            else:
                rp = wo * c + rpad
                shape, strides = (n, ho, wo, c), (ho * rp + bpad, rp, c, 1)
            dbuf, dview = view_in_buffer(shape, strides, doff, odt, dev)
            cbuf, cview = view_in_buffer(shape, strides, doff, odt, dev)
            what = f"src off {soff} pitch {W + row_pad}, dst {case[2:]} {wo}x{ho}"
            if out == "same":
                got = ops.cvt_color_crop_resize_rois(d_yuv, d_rects, wo, ho, src_index=d_idx, out=dview)
                ops.crop_resize_rois(d_bgr, d_rects, wo, ho, src_index=d_idx, out=cview)
                want = want_u8
            else:
                got = ops.cvt_color_crop_resize_rois_normalize(d_yuv, d_rects, wo, ho, MEAN3, STD3, src_index=d_idx,
                                                               layout=out, out=dview)
                ops.crop_resize_rois_normalize(d_bgr, d_rects, wo, ho, MEAN3, STD3, src_index=d_idx, layout=out, out=cview)
                want = normalized(oracle, want_u8, out)
            assert got.data_ptr() == dview.data_ptr()
            assert_bits(host(dview), want, what + " vs oracle")
            assert_bits(host(dview), host(cview), what + " vs cvt_color + crop_resize_rois")
            assert_rim_intact(dbuf, dview, what)
    assert_bits(host(sview)[..., 0], yuv, "source")
    assert_rim_intact(sbuf, sview, "source rim")


# ---------------------------------------------------------------------------
# 7. invalid device values: range checks, zeros, nothing read

@gpu
def test_invalid_rects_and_indices_give_zeros(ops, dev, oracle):
    """src = the middle two frames of a four-frame allocation, so nothing here
    could leave the allocation even unguarded: a missing check would show the
    neighbours' pixels instead of zeros.  A rect is judged against the DECODED
    130 x 98 size: the chroma rows below row 98 are no place for one."""
    wo, ho = WO, HO
    big = make_yuv(4, W, H, 17)
    d_big = to_dev(big, dev)
    src = d_big[1:3]
    good = [5, 4, 40, 30]
    cases = [  # (index, rect, valid)
        (0, good, True),
        (-1, good, False),                       # index below the range
        (2, good, False),                        # index n
        (1, [5, 4, 1, 30], False),               # width 1
        (1, good, True),
        (0, [5, 4, 40, 0], False),               # height 0
        (0, [-1, 4, 40, 30], False),             # left -1
        (0, [5, -1, 40, 30], False),
        (1, [W - 39, 4, 40, 30], False),         # left + width = W + 1
        (1, [W - 40, 4, 40, 30], True),          # ... = W: the neighbour that is valid
        (0, [5, H - 29, 40, 30], False),         # top + height = H + 1: inside the Y + chroma rows, outside the frame
        (0, [5, H - 30, 40, 30], True),
        (0, [5, H, 40, 30], False),              # wholly in the chroma rows
        (1, [5, 4, INT32_MAX, 30], False),       # left + width overflows int32
        (1, [5, 4, 40, INT32_MAX], False),
        (0, [INT32_MAX, INT32_MAX, 2, 2], False),
        (0, [0, 0, -5, -5], False),
        (-2 ** 31, good, False),
        (INT32_MAX, good, False),
        (1, [0, 0, W, H], True),
    ]
    idx = np.array([k for k, _, _ in cases], np.int32)
    rects = np.array([r for _, r, _ in cases], np.int32)
    n = len(cases)
    d_rects, d_idx = to_dev(rects, dev), to_dev(idx, dev)
    bgr = decode(oracle, big, NV21_BGR)
    want = []
    for k, r, ok in cases:
        want.append(oracle_roi(oracle, bgr[1 + k], r, wo, ho, REFERENCE) if ok else np.zeros((ho, wo, 3), np.uint8))
        assert not ok or want[-1].any(), "a valid ROI must not look like an invalid one"
    want = np.stack(want)
    dbuf, dview = view_in_buffer((n, ho, wo, 3), (ho * wo * 3 + 7, wo * 3, 3, 1), 4, np.uint8, dev)
    ops.cvt_color_crop_resize_rois(src, d_rects, wo, ho, src_index=d_idx, out=dview)
    got = host(dview)
    for i, (k, r, ok) in enumerate(cases):
        assert_bits(got[i], want[i], f"index {k} rect {r}")
    assert_rim_intact(dbuf, dview, "invalid values")
    for layout in (NHWC, NCHW):
        gotn = host(ops.cvt_color_crop_resize_rois_normalize(src, d_rects, wo, ho, MEAN3, STD3, src_index=d_idx,
                                                             layout=layout))
        wantn = normalized(oracle, want, layout)  # an invalid ROI is the normalized value of 0
        for i, (k, r, ok) in enumerate(cases):
            assert_bits(gotn[i], wantn[i], f"normalize {layout}: index {k} rect {r}")
    assert_bits(host(d_big), big, "source allocation")


# ---------------------------------------------------------------------------
# 8. the index and array contract

@gpu
def test_null_index_broadcast_and_identity(ops, dev, oracle):
    yuv = make_yuv(4, W, H, 11)
    rects = RECTS[[0, 4, 8, 13]]
    d_rects = to_dev(rects, dev)
    for code in (NV21_BGR, NV12_RGB):
        # one frame: every ROI reads it
        d1 = to_dev(yuv[:1], dev)
        got = ops.cvt_color_crop_resize_rois(d1, d_rects, WO, HO, code=code)
        check_both(ops, oracle, got, yuv[:1], d1, code, [0] * 4, rects, d_rects, None, WO, HO, REFERENCE, "broadcast")
        d2 = to_dev(yuv[1], dev)  # (h * 3 / 2, w)
        got = ops.cvt_color_crop_resize_rois(d2, d_rects, WO, HO, code=code)
        check_both(ops, oracle, got, yuv[1], d2, code, [0] * 4, rects, d_rects, None, WO, HO, REFERENCE, "2-d frame")
        # as many frames as ROIs: ROI i reads frame i
        d4 = to_dev(yuv, dev)
        got = ops.cvt_color_crop_resize_rois(d4, d_rects, WO, HO, code=code)
        check_both(ops, oracle, got, yuv, d4, code, [0, 1, 2, 3], rects, d_rects, None, WO, HO, REFERENCE, "identity")
        gotn = ops.cvt_color_crop_resize_rois_normalize(d4, d_rects, WO, HO, MEAN3, STD3, code=code, layout=NCHW)
        check_both(ops, oracle, gotn, yuv, d4, code, [0, 1, 2, 3], rects, d_rects, None, WO, HO, REFERENCE,
                   "identity nchw", layout=NCHW)
    # any other count without an index is refused
    with pytest.raises(ValueError):
        ops.cvt_color_crop_resize_rois(to_dev(yuv[:2], dev), d_rects, WO, HO)
    with pytest.raises(ValueError):
        ops.cvt_color_crop_resize_rois_normalize(to_dev(yuv[:3], dev), d_rects, WO, HO, MEAN3, STD3)


@gpu
def test_many_and_one(ops, dev, oracle):
    yuv = make_yuv(1, 64, 64, 23)
    d_yuv = to_dev(yuv, dev)
    rng = np.random.default_rng(24)
    wh = rng.integers(2, 40, (300, 2))
    lt = (rng.random((300, 2)) * (65 - wh)).astype(np.int64)
    rects = np.concatenate([lt, wh], 1).astype(np.int32)
    assert (rects[:, 0] + rects[:, 2] <= 64).all() and (rects[:, 1] + rects[:, 3] <= 64).all()
    d_rects = to_dev(rects, dev)
    got = ops.cvt_color_crop_resize_rois(d_yuv, d_rects, 8, 8)
    check_both(ops, oracle, got, yuv, d_yuv, NV21_BGR, [0] * 300, rects, d_rects, None, 8, 8, REFERENCE, "300 ROIs")
    gotn = ops.cvt_color_crop_resize_rois_normalize(d_yuv, d_rects, 8, 8, MEAN3, STD3, layout=NCHW)
    check_both(ops, oracle, gotn, yuv, d_yuv, NV21_BGR, [0] * 300, rects, d_rects, None, 8, 8, REFERENCE, "300 planar",
               layout=NCHW)
    one = ops.cvt_color_crop_resize_rois(d_yuv, d_rects[:1], 112, 112)
    check_both(ops, oracle, one, yuv, d_yuv, NV21_BGR, [0], rects[:1], d_rects[:1], None, 112, 112, REFERENCE, "one ROI")


@gpu
def test_arrays_read_at_execution_time(ops, dev, oracle):
    import torch
    yuv = make_yuv(3, W, H, 29)
    d_yuv = to_dev(yuv, dev)
    rects_a, rects_b = RECTS[:7], RECTS[7:14]
    idx_a, idx_b = IDX[:7], IDX[:7][::-1].copy()
    d_rects, d_idx = to_dev(rects_a, dev), to_dev(idx_a, dev)
    d_rects_b, d_idx_b = to_dev(rects_b, dev), to_dev(idx_b, dev)
    out_a = torch.empty((7, HO, WO, 3), dtype=torch.uint8, device=dev)
    out_b = torch.empty_like(out_a)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        ops.cvt_color_crop_resize_rois(d_yuv, d_rects, WO, HO, src_index=d_idx, out=out_a, stream=stream)
        d_rects.copy_(d_rects_b, non_blocking=True)   # overwritten on the stream, between the two calls,
        d_idx.copy_(d_idx_b, non_blocking=True)       # with no host synchronisation
        ops.cvt_color_crop_resize_rois(d_yuv, d_rects, WO, HO, src_index=d_idx, out=out_b, stream=stream)
    stream.synchronize()
    bgr = decode(oracle, yuv, NV21_BGR)
    assert_bits(host(out_a), oracle_rois(oracle, bgr, idx_a, rects_a, WO, HO), "first call")
    assert_bits(host(out_b), oracle_rois(oracle, bgr, idx_b, rects_b, WO, HO), "second call")


@gpu
def test_binding_refuses_silent_copies(ops, dev):
    import torch
    frame = to_dev(make_yuv(1, 16, 16, 1), dev)
    rects = torch.tensor([[0, 0, 4, 4]] * 4, dtype=torch.int32, device=dev)
    for fn in (lambda r, **kw: ops.cvt_color_crop_resize_rois(frame, r, 4, 4, **kw),
               lambda r, **kw: ops.cvt_color_crop_resize_rois_normalize(frame, r, 4, 4, [0, 0, 0], [1, 1, 1], **kw)):
        with pytest.raises(ValueError):
            fn(rects.cpu())                                   # a host tensor: the wrong device
        with pytest.raises(ValueError):
            fn(rects.long())                                  # int64
        with pytest.raises(ValueError):
            fn(rects.float())
        with pytest.raises(ValueError):
            fn(torch.zeros((8, 4), dtype=torch.int32, device=dev)[::2])  # not contiguous
        with pytest.raises(ValueError):
            fn(rects.reshape(2, 8))                           # shape
        with pytest.raises(ValueError):
            fn(rects, src_index=torch.zeros(4, dtype=torch.int64, device=dev))
        with pytest.raises(ValueError):
            fn(rects, src_index=torch.zeros(4, dtype=torch.int32))
    with pytest.raises(ValueError):
        ops.cvt_color_crop_resize_rois_normalize(frame, rects, 4, 4, None, None)   # no per-image statistics for ROIs
    with pytest.raises(ValueError):
        ops.cvt_color_crop_resize_rois_normalize(frame, rects, 4, 4, [0, 0, 0], None)
    # lists and numpy arrays are moved for convenience
    got = ops.cvt_color_crop_resize_rois(frame, [[0, 0, 4, 4], [3, 5, 4, 4]], 4, 4, src_index=[0, 0])
    assert tuple(got.shape) == (2, 4, 4, 3)
    assert_bits(host(got)[1], host(ops.cvt_color(frame))[0, 5:9, 3:7], "identity crop")


# ---------------------------------------------------------------------------
# 9. the C++ layer

@gpu
def test_cpp_yuv_crop_resize(hip_device, tmp_path):
    repo = Path(__file__).resolve().parent.parent
    pkg = repo / "arm-neon-opencv_amd"
    lib = pkg / "lib"
    exe = tmp_path / "vacv_yuv_crop_resize_test"
    r = subprocess.run(["g++", "-std=c++14", "-O1", str(repo / "tests" / "cpp" / "vacv_yuv_crop_resize_test.cpp"), "-o",
                        str(exe), "-I", str(pkg / "src"), "-L", str(lib), "-lvacv", "-lvacv_hip",
                        f"-Wl,-rpath,{lib}"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run(["timeout", "-k", "10", "120", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "failed 0" in r.stdout, r.stdout[-3000:]
