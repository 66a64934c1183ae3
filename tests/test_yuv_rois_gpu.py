"""vacv_cvt_color_warp_affine_rois[_normalize] on the GPU: many crops straight
from NV21 / NV12 frames in one launch (csrc/k_yuv_rois.hip).

Every comparison is bit-exact, and the expected ROI is computed two ways that
both have to equal the result:
 (a) on the host: the oracle's yuv420sp_to_bgr of the indexed frame, then its
     warp_affine (+ u8_to_f32, normalize, hwc_to_chw) under the ROI's map;
 (b) on the GPU: ops.cvt_color of all frames, then ops.warp_affine_rois
     [_normalize] on the decoded frames -- the chain the call replaces.
Frames are 130 x 98: even rows of 130 bytes start at 2 modulo 4, a dense frame
is 130 x 147 bytes, and the ROI sizes reach every path of the kernel (narrower
and wider than a wave, one pixel, two 1024-pixel tiles split mid-row).
"""
from __future__ import annotations

import subprocess
from pathlib import Path

import numpy as np
import pytest

from test_gpu_plumbing import SENTINEL, assert_bits, assert_rim_intact, host, place
from test_warp_rois_gpu import (BORDER_U8, IDX7, MEAN, PITCH_CASES, STD, filled, oracle_normalized, oracle_rois,
                                random_maps, to_dev, view_in_buffer)

gpu = pytest.mark.gpu
NHWC, NCHW = 1, 0
CONSTANT, REPLICATE, REFLECT, WRAP, REFLECT_101 = 0, 1, 2, 3, 4
NV12_RGB, NV12_BGR, NV21_RGB, NV21_BGR = 90, 91, 92, 93
CODES = {NV21_BGR: (True, False), NV21_RGB: (True, True), NV12_BGR: (False, False), NV12_RGB: (False, True)}
CODE_IDS = {NV21_BGR: "nv21-bgr", NV21_RGB: "nv21-rgb", NV12_BGR: "nv12-bgr", NV12_RGB: "nv12-rgb"}
W, H = 130, 98  # decoded frames
MEAN3, STD3, BORDER3 = MEAN[:3], STD[:3], BORDER_U8[:3]


@pytest.fixture(scope="module")
def ops(hip_device):
    from vacv_amd import ops
    return ops


@pytest.fixture(scope="module")
def dev(hip_device):
    return hip_device


def make_yuv(n, w, h, seed):
    """Random Y and chroma bytes: neighbouring taps differ in all three planes."""
    return np.random.default_rng(seed).integers(0, 256, (n, h * 3 // 2, w), dtype=np.uint8)


def decode(oracle, yuv, code):
    """(a): [n, h, w, 3], the oracle's cvt_color of every frame."""
    v_first, rgb = CODES[code]
    return np.stack([oracle.yuv420sp_to_bgr(f, v_first, rgb) for f in yuv])


def normalized(oracle, rois, layout):
    """(a): u8 ROIs [n, ho, wo, 3] -> fp32, normalized, NHWC or NCHW."""
    f = oracle_normalized(oracle, rois, MEAN3, STD3)
    return f if layout == NHWC else np.stack([oracle.hwc_to_chw(r) for r in f])


def check_both(ops, oracle, got, yuv, d_yuv, code, idx, ms, d_ms, d_idx, wo, ho, mode, what, layout=None, **kw):
    """got == (a) the host chain == (b) the GPU chain on the decoded frames."""
    want = oracle_rois(oracle, decode(oracle, yuv, code), idx, ms, wo, ho, BORDER3, mode)
    bgr = ops.cvt_color(d_yuv, code)
    if layout is None:
        chain = ops.warp_affine_rois(bgr, d_ms, wo, ho, src_index=d_idx, border_mode=mode, border_value=BORDER_U8, **kw)
    else:
        want = normalized(oracle, want, layout)
        chain = ops.warp_affine_rois_normalize(bgr, d_ms, wo, ho, MEAN3, STD3, src_index=d_idx, out_layout=layout,
                                               border_mode=mode, border_value=BORDER_U8, **kw)
    got = host(got)
    for i in range(len(ms)):
        assert_bits(got[i], want[i], f"{what} roi {i} m={np.asarray(ms[i]).tolist()} vs oracle")
    assert_bits(got, host(chain), what + " vs cvt_color + warp_affine_rois")


# ---------------------------------------------------------------------------
# 1. parity: every code, every border mode

@gpu
@pytest.mark.parametrize("code", list(CODES), ids=lambda c: CODE_IDS[c])
def test_yuv_rois_parity(ops, dev, oracle, code):
    import torch
    yuv = make_yuv(3, W, H, 500 + code)
    d_yuv, d_idx = to_dev(yuv, dev), to_dev(np.array(IDX7, np.int32), dev)
    bgr = decode(oracle, yuv, code)
    d_bgr = ops.cvt_color(d_yuv, code)
    assert_bits(host(d_bgr), bgr, "cvt_color vs oracle")
    rng = np.random.default_rng(20261020 + code)
    for wo, ho in [(112, 112), (37, 53), (65, 5), (5, 3), (1, 1)]:  # 37 x 53 = 1961 px: two tiles split mid-row
        ms = random_maps(rng, 7, W, H, wo, ho)
        d_ms = to_dev(ms, dev)
        for mode in (CONSTANT, REPLICATE, REFLECT, WRAP, REFLECT_101):
            what = f"{CODE_IDS[code]} {wo}x{ho} border {mode}"
            got = ops.cvt_color_warp_affine_rois(d_yuv, d_ms, wo, ho, code=code, src_index=d_idx, border_mode=mode,
                                                 border_value=BORDER_U8)
            assert tuple(got.shape) == (7, ho, wo, 3) and got.dtype == torch.uint8
            want = oracle_rois(oracle, bgr, IDX7, ms, wo, ho, BORDER3, mode)
            chain = ops.warp_affine_rois(d_bgr, d_ms, wo, ho, src_index=d_idx, border_mode=mode, border_value=BORDER_U8)
            got = host(got)
            for i in range(7):
                assert_bits(got[i], want[i], f"{what} roi {i} m={ms[i].tolist()} vs oracle")
            assert_bits(got, host(chain), what + " vs cvt_color + warp_affine_rois")


# ---------------------------------------------------------------------------
# 2. fused normalize, NHWC and NCHW

@gpu
@pytest.mark.parametrize("layout", [NHWC, NCHW], ids=["nhwc", "nchw"])
@pytest.mark.parametrize("code", [NV21_BGR, NV12_RGB], ids=lambda c: CODE_IDS[c])
def test_yuv_rois_normalize(ops, dev, oracle, code, layout):
    import torch
    yuv = make_yuv(3, W, H, 600 + code)
    d_yuv, d_idx = to_dev(yuv, dev), to_dev(np.array(IDX7, np.int32), dev)
    rng = np.random.default_rng(61 + code)
    for wo, ho in [(112, 112), (37, 53), (5, 3)]:
        ms = random_maps(rng, 7, W, H, wo, ho)
        d_ms = to_dev(ms, dev)
        for mode in (CONSTANT, REFLECT_101):
            got = ops.cvt_color_warp_affine_rois_normalize(d_yuv, d_ms, wo, ho, MEAN3, STD3, code=code, src_index=d_idx,
                                                           layout=layout, border_mode=mode, border_value=BORDER_U8)
            assert got.dtype == torch.float32
            assert tuple(got.shape) == ((7, ho, wo, 3) if layout == NHWC else (7, 3, ho, wo))
            check_both(ops, oracle, got, yuv, d_yuv, code, IDX7, ms, d_ms, d_idx, wo, ho, mode,
                       f"{CODE_IDS[code]} layout {layout} {wo}x{ho} border {mode}", layout=layout)


# ---------------------------------------------------------------------------
# 3. every chroma pair

@pytest.fixture(scope="module")
def all_pairs_frame():
    """One 512 x 512 frame: its 256 x 256 chroma pairs are the 65,536 (byte 0,
    byte 1) values, each once, in a random order; Y is pseudo-random."""
    rng = np.random.default_rng(7)
    yuv = np.zeros((1, 768, 512), np.uint8)
    yuv[0, :512] = rng.integers(0, 256, (512, 512), dtype=np.uint8)
    pairs = rng.permutation(65536).astype(np.uint16).reshape(256, 256)
    yuv[0, 512:, 0::2] = pairs >> 8
    yuv[0, 512:, 1::2] = pairs & 0xFF
    seen = yuv[0, 512:].reshape(-1, 2).astype(np.int64)
    assert np.unique(seen[:, 0] * 256 + seen[:, 1]).size == 65536
    return yuv


@gpu
@pytest.mark.parametrize("code", list(CODES), ids=lambda c: CODE_IDS[c])
def test_yuv_rois_every_chroma_pair(ops, dev, oracle, all_pairs_frame, code):
    yuv = all_pairs_frame
    d_yuv = to_dev(yuv, dev)
    decoded = ops.cvt_color(d_yuv, code)
    assert_bits(host(decoded), decode(oracle, yuv, code), "cvt_color vs oracle")
    # the identity map under REPLICATE is the decoded frame itself, last row and column included
    ident = np.array([[1, 0, 0, 0, 1, 0]], np.float32)
    got = ops.cvt_color_warp_affine_rois(d_yuv, to_dev(ident, dev), 512, 512, code=code, border_mode=REPLICATE)
    assert_bits(host(got), host(decoded), f"{CODE_IDS[code]}: identity")
    # half a pixel off: every tap pair and every row pair blended
    half = np.array([[1, 0, 0.5, 0, 1, 0.5]], np.float32)
    d_half = to_dev(half, dev)
    got = ops.cvt_color_warp_affine_rois(d_yuv, d_half, 512, 512, code=code, border_mode=REPLICATE, border_value=BORDER_U8)
    check_both(ops, oracle, got, yuv, d_yuv, code, [0], half, d_half, None, 512, 512, REPLICATE,
               f"{CODE_IDS[code]}: half-pixel translation")


# ---------------------------------------------------------------------------
# 4. the frame's end and tiny frames

def corner_maps(w, h, wo, ho):
    """Forward maps whose ROIs cover the frame's bottom-right corner: whole-
    and part-pixel translations (the last Y bytes and the last chroma pair
    are tapped), a magnified and a rotated view of the corner."""
    ms = []
    for fx, fy in ((0.0, 0.0), (0.25, 0.5), (1.0, 1.0), (1.5, 0.75)):
        ms.append([1, 0, -(w - np.floor(wo * 0.6) - fx), 0, 1, -(h - np.floor(ho * 0.6) - fy)])
    ms.append([3, 0, -3 * (w - wo / 4.0), 0, 3, -3 * (h - ho / 4.0)])  # the last 2 x 2 pixels fill most of the ROI
    a = np.deg2rad(30.0)
    c, s = np.cos(a), np.sin(a)
    ms.append([c, -s, wo / 2 - (c * (w - 1) - s * (h - 1)), s, c, ho / 2 - (s * (w - 1) + c * (h - 1))])
    return np.array(ms, np.float32)


@gpu
@pytest.mark.parametrize("off", [0, 1, 2, 3])
def test_yuv_rois_frame_end(ops, dev, oracle, off):
    """The 130 x 98 frame as the last bytes of its buffer, at every base
    alignment: a load reaching past the last chroma pair has nothing behind it."""
    import torch
    yuv = make_yuv(1, W, H, 700 + off)
    buf = torch.full((off + yuv.size,), SENTINEL, dtype=torch.uint8, device=dev)
    buf[off:] = to_dev(yuv.reshape(-1), dev)
    d_yuv = buf[off:].view(1, H * 3 // 2, W)
    assert d_yuv.data_ptr() + yuv.size == buf.data_ptr() + buf.numel()
    for wo, ho in [(37, 21), (5, 3)]:
        ms = corner_maps(W, H, wo, ho)
        d_ms = to_dev(ms, dev)
        for code in (NV21_BGR, NV12_RGB):
            for mode in (CONSTANT, REPLICATE):
                what = f"off {off} {CODE_IDS[code]} {wo}x{ho} border {mode}"
                got = ops.cvt_color_warp_affine_rois(d_yuv, d_ms, wo, ho, code=code, border_mode=mode,
                                                     border_value=BORDER_U8)
                check_both(ops, oracle, got, yuv, d_yuv, code, [0] * len(ms), ms, d_ms, None, wo, ho, mode, what)
                gotn = ops.cvt_color_warp_affine_rois_normalize(d_yuv, d_ms, wo, ho, MEAN3, STD3, code=code, layout=NCHW,
                                                                border_mode=mode, border_value=BORDER_U8)
                check_both(ops, oracle, gotn, yuv, d_yuv, code, [0] * len(ms), ms, d_ms, None, wo, ho, mode,
                           what + " normalized", layout=NCHW)
    assert_bits(host(buf)[:off], np.full(off, SENTINEL, np.uint8), "bytes before the frame")


@gpu
@pytest.mark.parametrize("w,h", [(2, 2), (4, 2), (6, 4)])
def test_yuv_rois_tiny_frames(ops, dev, oracle, w, h):
    yuv = make_yuv(2, w, h, 800 + w)
    d_yuv = to_dev(yuv, dev)
    rng = np.random.default_rng(81 + w)
    for wo, ho in [(8, 8), (5, 3)]:
        ms = np.concatenate([[[1, 0, 0, 0, 1, 0], [1, 0, 0.5, 0, 1, 0.5], [4, 0, 0.5, 0, 4, 0.25], [2.5, 0, 1, 0, 2.5, 1]],
                             corner_maps(w, h, wo, ho), random_maps(rng, 4, w, h, wo, ho)]).astype(np.float32)
        idx = [i % 2 for i in range(len(ms))]
        d_ms, d_idx = to_dev(ms, dev), to_dev(np.array(idx, np.int32), dev)
        for code in (NV21_BGR, NV12_RGB):
            for mode in (CONSTANT, REPLICATE):
                got = ops.cvt_color_warp_affine_rois(d_yuv, d_ms, wo, ho, code=code, src_index=d_idx, border_mode=mode,
                                                     border_value=BORDER_U8)
                check_both(ops, oracle, got, yuv, d_yuv, code, idx, ms, d_ms, d_idx, wo, ho, mode,
                           f"{w}x{h} frame {CODE_IDS[code]} {wo}x{ho} border {mode}")


# ---------------------------------------------------------------------------
# 5. pitched, misaligned

DST_CASES = [c for c in PITCH_CASES if c[0] == np.uint8 and c[1] == 3]  # 5 u8, 2 fp32 NCHW, 1 fp32 NHWC
SIZES5 = [(37, 53), (140, 9), (5, 3)]


@pytest.fixture(scope="module")
def pitched_reference(oracle):
    """Frames, maps and (a) for the pitched cases, computed once."""
    yuv = make_yuv(3, W, H, 900)
    bgr = decode(oracle, yuv, NV21_BGR)
    rng = np.random.default_rng(91)
    ref = {}
    for wo, ho in SIZES5:
        ms = random_maps(rng, 7, W, H, wo, ho)
        ref[(wo, ho)] = (ms, oracle_rois(oracle, bgr, IDX7, ms, wo, ho, BORDER3, CONSTANT))
    return yuv, ref


@gpu
@pytest.mark.parametrize("row_pad", [0, 5, 14], ids=lambda p: f"pitch{130 + p}")
@pytest.mark.parametrize("soff", [0, 1, 2, 3])
def test_yuv_rois_pitched_misaligned(ops, dev, oracle, pitched_reference, soff, row_pad):
    assert len(DST_CASES) == 8
    yuv, ref = pitched_reference
    sbuf, sview = place(yuv[..., None], dev, NHWC, off=soff, row_pad=row_pad, batch_pad=7)
    d_yuv = sview[..., 0]
    assert d_yuv.stride() == ((H * 3 // 2) * (W + row_pad) + 7, W + row_pad, 1)
    d_idx = to_dev(np.array(IDX7, np.int32), dev)
    d_bgr = ops.cvt_color(d_yuv, NV21_BGR)
    for (wo, ho) in SIZES5:
        ms, want_u8 = ref[(wo, ho)]
        d_ms = to_dev(ms, dev)
        for case in DST_CASES:
            _, c, out, _, _, doff, rpad, ppad, bpad = case
            odt = np.uint8 if out == "same" else np.float32
            if out == NCHW:
                rp = wo + rpad
                pl = ho * rp + ppad
                dbuf, dview = view_in_buffer((7, c, ho, wo), (c * pl + bpad, pl, rp, 1), doff, odt, dev)
                cbuf, cview = view_in_buffer((7, c, ho, wo), (c * pl + bpad, pl, rp, 1), doff, odt, dev)
            else:
                rp = wo * c + rpad
                dbuf, dview = view_in_buffer((7, ho, wo, c), (ho * rp + bpad, rp, c, 1), doff, odt, dev)
                cbuf, cview = view_in_buffer((7, ho, wo, c), (ho * rp + bpad, rp, c, 1), doff, odt, dev)
            what = f"src off {soff} pitch {W + row_pad}, dst {case[2:]} {wo}x{ho}"
            if out == "same":
                got = ops.cvt_color_warp_affine_rois(d_yuv, d_ms, wo, ho, src_index=d_idx, border_value=BORDER_U8, out=dview)
                ops.warp_affine_rois(d_bgr, d_ms, wo, ho, src_index=d_idx, border_value=BORDER_U8, out=cview)
                want = want_u8
            else:
                got = ops.cvt_color_warp_affine_rois_normalize(d_yuv, d_ms, wo, ho, MEAN3, STD3, src_index=d_idx,
                                                               layout=out, border_value=BORDER_U8, out=dview)
                ops.warp_affine_rois_normalize(d_bgr, d_ms, wo, ho, MEAN3, STD3, src_index=d_idx, out_layout=out,
                                               border_value=BORDER_U8, out=cview)
                want = normalized(oracle, want_u8, out)
            assert got.data_ptr() == dview.data_ptr()
            assert_bits(host(dview), want, what + " vs oracle")
            assert_bits(host(dview), host(cview), what + " vs cvt_color + warp_affine_rois")
            assert_rim_intact(dbuf, dview, what)
    assert_bits(host(sview)[..., 0], yuv, "source")
    assert_rim_intact(sbuf, sview, "source rim")


# ---------------------------------------------------------------------------
# 6. the contract of the device arrays

@gpu
def test_yuv_rois_null_index_broadcast_and_identity(ops, dev, oracle):
    wo, ho = 53, 37
    yuv = make_yuv(4, W, H, 11)
    ms = random_maps(np.random.default_rng(12), 4, W, H, wo, ho)
    d_ms = to_dev(ms, dev)
    for code in (NV21_BGR, NV12_RGB):
        # one frame: every ROI reads it
        d1 = to_dev(yuv[:1], dev)
        got = ops.cvt_color_warp_affine_rois(d1, d_ms, wo, ho, code=code, border_value=BORDER_U8)
        check_both(ops, oracle, got, yuv[:1], d1, code, [0] * 4, ms, d_ms, None, wo, ho, CONSTANT, "broadcast")
        d2 = to_dev(yuv[1], dev)  # (h * 3 / 2, w)
        got = ops.cvt_color_warp_affine_rois(d2, d_ms, wo, ho, code=code, border_value=BORDER_U8)
        assert_bits(host(got), oracle_rois(oracle, decode(oracle, yuv, code), [1] * 4, ms, wo, ho, BORDER3, CONSTANT),
                    "2-d frame")
        # as many frames as ROIs: ROI i reads frame i
        d4 = to_dev(yuv, dev)
        got = ops.cvt_color_warp_affine_rois(d4, d_ms, wo, ho, code=code, border_value=BORDER_U8)
        check_both(ops, oracle, got, yuv, d4, code, [0, 1, 2, 3], ms, d_ms, None, wo, ho, CONSTANT, "identity")
        gotn = ops.cvt_color_warp_affine_rois_normalize(d4, d_ms, wo, ho, MEAN3, STD3, code=code, layout=NCHW,
                                                        border_value=BORDER_U8)
        check_both(ops, oracle, gotn, yuv, d4, code, [0, 1, 2, 3], ms, d_ms, None, wo, ho, CONSTANT, "identity nchw",
                   layout=NCHW)
    # any other count without an index is refused
    with pytest.raises(ValueError):
        ops.cvt_color_warp_affine_rois(to_dev(yuv[:2], dev), d_ms, wo, ho)


@gpu
def test_yuv_rois_inverse_map(ops, dev, oracle):
    from vacv_amd import INTER_LINEAR, WARP_INVERSE_MAP
    wo, ho = 37, 53
    yuv = make_yuv(3, W, H, 7)
    d_yuv, d_idx = to_dev(yuv, dev), to_dev(np.array(IDX7, np.int32), dev)
    ms = random_maps(np.random.default_rng(5), 7, W, H, wo, ho)
    inv = np.stack([ops.invert_affine(m) for m in ms])
    d_ms = to_dev(ms, dev)
    for mode in (CONSTANT, REFLECT_101):
        fwd = ops.cvt_color_warp_affine_rois(d_yuv, d_ms, wo, ho, src_index=d_idx, border_mode=mode, border_value=BORDER_U8)
        back = ops.cvt_color_warp_affine_rois(d_yuv, to_dev(inv, dev).reshape(7, 2, 3), wo, ho, src_index=d_idx,
                                              flags=INTER_LINEAR | WARP_INVERSE_MAP, border_mode=mode,
                                              border_value=BORDER_U8)
        assert_bits(host(back), host(fwd), f"inverse map, border {mode}")
        check_both(ops, oracle, fwd, yuv, d_yuv, NV21_BGR, IDX7, ms, d_ms, d_idx, wo, ho, mode, f"forward, border {mode}")


@gpu
def test_yuv_rois_index_out_of_range_is_all_border(ops, dev, oracle):
    """src = the middle two frames of a four-frame allocation: an index the
    kernel failed to guard would show the neighbours' pixels, never leave the
    allocation."""
    wo, ho, w, h = 37, 21, 46, 32
    big = make_yuv(4, w, h, 17)
    d_big = to_dev(big, dev)
    src = d_big[1:3]
    idx = [-1, 0, 2, 1, 2 ** 30, -2 ** 31, 2 ** 31 - 1]
    # every ROI looks at the same, well-covered part of its frame
    ms = np.repeat(np.array([[1.1, 0.2, 3.0, -0.2, 1.1, 2.0]], np.float32), len(idx), 0)
    d_ms, d_idx = to_dev(ms, dev), to_dev(np.array(idx, np.int32), dev)
    bgr = decode(oracle, big[1:3], NV21_BGR)
    border_roi = filled(1, ho, wo, BORDER3, np.uint8)[0]
    border_n = normalized(oracle, border_roi[None], NCHW)[0]
    for mode in (CONSTANT, REPLICATE, WRAP):
        got = host(ops.cvt_color_warp_affine_rois(src, d_ms, wo, ho, src_index=d_idx, border_mode=mode,
                                                  border_value=BORDER_U8))
        gotn = host(ops.cvt_color_warp_affine_rois_normalize(src, d_ms, wo, ho, MEAN3, STD3, src_index=d_idx, layout=NCHW,
                                                             border_mode=mode, border_value=BORDER_U8))
        for i, k in enumerate(idx):
            if 0 <= k < 2:
                want = oracle_rois(oracle, bgr, [k], ms[i:i + 1], wo, ho, BORDER3, mode)[0]
                assert not np.array_equal(want, border_roi), "the map must hit the frame"
                assert_bits(got[i], want, f"index {k}, border {mode}")
            else:
                assert_bits(got[i], border_roi, f"index {k}, border {mode}")
                assert_bits(gotn[i], border_n, f"normalize: index {k}, border {mode}")
    assert_bits(host(d_big), big, "source allocation")


@gpu
def test_yuv_rois_degenerate_matrices(ops, dev, oracle):
    wo, ho, w, h = 37, 21, 46, 32
    big = make_yuv(4, w, h, 19)
    src = to_dev(big, dev)[1:3]
    inf, nan = np.inf, np.nan
    ms = np.array([[0, 0, 0, 0, 0, 0],                 # zero determinant: the inverse is all zeros
                   [0.5, 1.0, 3.0, 0.25, 0.5, -2.0],   # rank 1
                   [1, nan, 0, 0, 1, 0],
                   [nan] * 6,
                   [inf, 0, 0, 0, 1, 0],
                   [1, 0, -inf, 0, 1, 0],
                   [1, 0, 0, 0, 1, inf],
                   [1.25, 0.1, -4.0, -0.1, 0.9, 2.5]], np.float32)  # an ordinary one among them
    idx = [0, 1, 0, 1, 0, 1, 0, 1]
    got = host(ops.cvt_color_warp_affine_rois(src, to_dev(ms, dev), wo, ho, src_index=to_dev(np.array(idx, np.int32), dev),
                                              border_value=BORDER_U8))
    bgr = decode(oracle, big[1:3], NV21_BGR)
    border_roi = filled(1, ho, wo, BORDER3, np.uint8)[0]
    for i in (0, 1, 7):
        want = oracle_rois(oracle, bgr, [idx[i]], ms[i:i + 1], wo, ho, BORDER3, CONSTANT)[0]
        assert_bits(got[i], want, f"matrix {ms[i].tolist()} vs oracle")
    assert not np.array_equal(got[7], border_roi)
    for i in (2, 3, 4, 5, 6):
        assert_bits(got[i], border_roi, f"matrix {ms[i].tolist()}: all border")


@gpu
def test_yuv_rois_many_and_one(ops, dev, oracle):
    yuv = make_yuv(1, 64, 64, 23)
    d_yuv = to_dev(yuv, dev)
    ms = random_maps(np.random.default_rng(24), 300, 64, 64, 8, 8)
    d_ms = to_dev(ms, dev)
    got = ops.cvt_color_warp_affine_rois(d_yuv, d_ms, 8, 8, border_value=BORDER_U8)
    check_both(ops, oracle, got, yuv, d_yuv, NV21_BGR, [0] * 300, ms, d_ms, None, 8, 8, CONSTANT, "300 ROIs")
    gotn = ops.cvt_color_warp_affine_rois_normalize(d_yuv, d_ms, 8, 8, MEAN3, STD3, layout=NCHW, border_value=BORDER_U8)
    check_both(ops, oracle, gotn, yuv, d_yuv, NV21_BGR, [0] * 300, ms, d_ms, None, 8, 8, CONSTANT, "300 planar", layout=NCHW)
    one = ops.cvt_color_warp_affine_rois(d_yuv, d_ms[:1], 112, 112, border_value=BORDER_U8)
    check_both(ops, oracle, one, yuv, d_yuv, NV21_BGR, [0], ms[:1], d_ms[:1], None, 112, 112, CONSTANT, "one ROI")


@gpu
def test_yuv_rois_arrays_read_at_execution_time(ops, dev, oracle):
    import torch
    wo, ho = 53, 37
    yuv = make_yuv(3, W, H, 29)
    d_yuv = to_dev(yuv, dev)
    rng = np.random.default_rng(30)
    ms_a, ms_b = random_maps(rng, 7, W, H, wo, ho), random_maps(rng, 7, W, H, wo, ho)
    idx_a, idx_b = np.array(IDX7, np.int32), np.array(IDX7[::-1], np.int32)
    d_ms, d_idx = to_dev(ms_a, dev), to_dev(idx_a, dev)
    d_ms_b, d_idx_b = to_dev(ms_b, dev), to_dev(idx_b, dev)
    out_a = torch.empty((7, ho, wo, 3), dtype=torch.uint8, device=dev)
    out_b = torch.empty_like(out_a)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        ops.cvt_color_warp_affine_rois(d_yuv, d_ms, wo, ho, src_index=d_idx, out=out_a, stream=stream)
        d_ms.copy_(d_ms_b, non_blocking=True)      # overwritten on the stream, between the two calls,
        d_idx.copy_(d_idx_b, non_blocking=True)    # with no host synchronisation
        ops.cvt_color_warp_affine_rois(d_yuv, d_ms, wo, ho, src_index=d_idx, out=out_b, stream=stream)
    stream.synchronize()
    bgr = decode(oracle, yuv, NV21_BGR)
    assert_bits(host(out_a), oracle_rois(oracle, bgr, idx_a, ms_a, wo, ho, (0, 0, 0), CONSTANT), "first call")
    assert_bits(host(out_b), oracle_rois(oracle, bgr, idx_b, ms_b, wo, ho, (0, 0, 0), CONSTANT), "second call")


@gpu
def test_yuv_rois_binding_refuses_silent_copies(ops, dev):
    import torch
    frame = to_dev(make_yuv(1, 16, 16, 1), dev)
    ms = torch.zeros((4, 6), dtype=torch.float32, device=dev)
    mean, std = MEAN3, STD3
    with pytest.raises(ValueError):
        ops.cvt_color_warp_affine_rois(frame, ms.double(), 4, 4)                        # dtype
    with pytest.raises(ValueError):
        ops.cvt_color_warp_affine_rois(frame, torch.zeros((6, 4), device=dev).t(), 4, 4)  # not contiguous
    with pytest.raises(ValueError):
        ops.cvt_color_warp_affine_rois(frame, ms.cpu(), 4, 4)                           # a host tensor
    with pytest.raises(ValueError):
        ops.cvt_color_warp_affine_rois(frame, ms, 4, 4, src_index=torch.zeros(4, dtype=torch.int64, device=dev))
    with pytest.raises(ValueError):
        ops.cvt_color_warp_affine_rois_normalize(frame, ms.cpu(), 4, 4, mean, std)
    with pytest.raises(ValueError):
        ops.cvt_color_warp_affine_rois_normalize(frame, ms, 4, 4, mean, None)
    # lists and numpy arrays are moved for convenience
    got = ops.cvt_color_warp_affine_rois(frame, [[1, 0, 0, 0, 1, 0]] * 2, 4, 4, src_index=[0, 0])
    assert tuple(got.shape) == (2, 4, 4, 3)
    assert_bits(host(got)[0], host(ops.cvt_color(frame))[0, :4, :4], "identity crop")


# ---------------------------------------------------------------------------
# 7. the C++ layer

@gpu
def test_cpp_yuv_vector_overloads(hip_device, tmp_path):
    repo = Path(__file__).resolve().parent.parent
    pkg = repo / "arm-neon-opencv_amd"
    lib = pkg / "lib"
    exe = tmp_path / "vacv_yuv_rois_test"
    r = subprocess.run(["g++", "-std=c++14", "-O1", str(repo / "tests" / "cpp" / "vacv_yuv_rois_test.cpp"), "-o", str(exe),
                        "-I", str(pkg / "src"), "-L", str(lib), "-lvacv", "-lvacv_hip", f"-Wl,-rpath,{lib}"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run(["timeout", "-k", "10", "120", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "failed 0" in r.stdout, r.stdout[-3000:]
