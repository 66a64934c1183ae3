"""The colour operators -- vacv_cvt_color, vacv_cvt_color_normalize,
vacv_cvt_color_resize and vacv_cvt_color_resize_normalize (csrc/k_pixel.hip's
color_kernel, csrc/k_color_cv.hip, csrc/k_yuv_resize.hip) -- on every
(Y, U, V) byte triple, and at the misaligned, pitched and tail shapes that
select their kernels and store widths.

The decode is a function of one (Y, U, V) triple and there are 2^24 of them:
one 4096 x 4096 frame holds them all (cube()), so the arithmetic is checked
exhaustively.  The dispatch is a function of byte alignment: as in
test_gpu_plumbing every input and output is a view placed inside a larger
device buffer of SENTINEL bytes, so a case controls each base and pitch and a
stray write shows in the rim.  Every comparison is bit-exact.

The references of the plain conversions are numpy restatements of the two
arithmetics (ref_nv, ref_cv, ref_gray), independent of the library;
test_references_match_oracle checks them against the oracle's C functions on
the CPU, on the whole cube.  The fused resize is compared with the oracle's
chain, step by step.  All GPU tests carry the gpu mark one by one because that
one test must run without a device.
"""
from __future__ import annotations

import functools

import numpy as np
import pytest

from test_gpu_plumbing import (SENTINEL, _torch_dtype, assert_bits, assert_rim_intact, assert_untouched, blank, host,
                               place, ref_mean_std, ref_normalize, ref_sums, unsupported)

gpu = pytest.mark.gpu
NHWC, NCHW = 1, 0
# include/vacv_hip.h; asserted against the package in the ops fixture
RGB_NV12, BGR_NV12, RGB_NV21, BGR_NV21 = 90, 91, 92, 93
RGBA_NV12, BGRA_NV12, RGBA_NV21, BGRA_NV21, BGR_YV12, GRAY2BGR = 94, 95, 96, 97, 99, 8
NV12, NV21, YV12 = 0, 1, 2  # chroma layouts: interleaved UV, interleaved VU, a V plane then a U plane
# code -> (chroma layout, RGB order, output channels)
NV_CODES = {BGR_NV21: (NV21, False, 3), BGR_NV12: (NV12, False, 3), RGB_NV21: (NV21, True, 3), RGB_NV12: (NV12, True, 3)}
CV_CODES = {RGBA_NV12: (NV12, True, 4), BGRA_NV12: (NV12, False, 4), RGBA_NV21: (NV21, True, 4),
            BGRA_NV21: (NV21, False, 4), BGR_YV12: (YV12, False, 3)}
MEAN = np.array([103.94, 116.78, 123.68], np.float32)
STD = np.array([57.375, 57.12, 58.395], np.float32)


@pytest.fixture(scope="module")
def ops(hip_device):
    import vacv_amd as V
    from vacv_amd import ops
    assert (V.NHWC, V.NCHW) == (NHWC, NCHW)
    assert (V.COLOR_YUV2RGB_NV12, V.COLOR_YUV2BGR_NV12, V.COLOR_YUV2RGB_NV21, V.COLOR_YUV2BGR_NV21) == (90, 91, 92, 93)
    assert (V.COLOR_YUV2RGBA_NV12, V.COLOR_YUV2BGRA_NV12, V.COLOR_YUV2RGBA_NV21, V.COLOR_YUV2BGRA_NV21,
            V.COLOR_YUV2BGR_YV12, V.COLOR_GRAY2BGR) == (94, 95, 96, 97, 99, 8)
    return ops


@pytest.fixture(scope="module")
def dev(hip_device):
    return hip_device


# ---------------------------------------------------------------------------
# YUV 4:2:0 frames: (h * 3 / 2, w) bytes, h rows of Y then h / 2 rows of chroma

def pack_yuv(Y, U, V, layout):
    """A frame (..., h * 3 / 2, w) from a Y plane (..., h, w) and half-resolution U and V planes."""
    h, w = Y.shape[-2:]
    lead = Y.shape[:-2]
    if layout == YV12:
        c = np.concatenate([V.reshape(lead + (-1,)), U.reshape(lead + (-1,))], axis=-1).reshape(lead + (h // 2, w))
    else:
        c = np.empty(lead + (h // 2, w), np.uint8)
        c[..., 0::2], c[..., 1::2] = (U, V) if layout == NV12 else (V, U)
    return np.concatenate([Y, c], axis=-2)


def split_yuv(frame, layout):
    """(Y, U, V) of a frame; U and V at half resolution."""
    frame = np.asarray(frame)
    hh, w = frame.shape[-2:]
    h = hh // 3 * 2
    lead = frame.shape[:-2]
    Y, c = frame[..., :h, :], frame[..., h:, :]
    if layout == YV12:  # OpenCV's contiguous planes: (h / 2) x (w / 2) bytes of V, then of U
        planes = c.reshape(lead + (2, h // 2, w // 2))
        return Y, planes[..., 1, :, :], planes[..., 0, :, :]
    pairs = c.reshape(lead + (h // 2, w // 2, 2))
    first, second = pairs[..., 0], pairs[..., 1]
    return (Y, first, second) if layout == NV12 else (Y, second, first)


def rand_frames(n, w, h, layout, seed):
    """n random frames whose first has the saturating extremes in its corner blocks."""
    rng = np.random.default_rng(seed)
    Y = rng.integers(0, 256, (n, h, w), dtype=np.uint8)
    U = rng.integers(0, 256, (n, h // 2, w // 2), dtype=np.uint8)
    V = rng.integers(0, 256, (n, h // 2, w // 2), dtype=np.uint8)
    Y[0, :2, :2], U[0, 0, 0], V[0, 0, 0] = 255, 255, 255
    Y[0, -2:, -2:], U[0, -1, -1], V[0, -1, -1] = ((0, 16), (235, 255)), 0, 0
    return pack_yuv(Y, U, V, layout)


@functools.lru_cache(maxsize=None)
def cube_planes():
    """Y (4096 x 4096), U, V (2048 x 2048) holding every (Y, U, V) byte triple
    once: 2 x 2 block b = by * 2048 + bx has U = (b >> 6) & 255, V = b >> 14
    and the four Y values 4 (b & 63) .. 4 (b & 63) + 3."""
    b = np.arange(2048 * 2048, dtype=np.int64).reshape(2048, 2048)
    uv, q = b >> 6, b & 63
    U, V = (uv & 255).astype(np.uint8), (uv >> 8).astype(np.uint8)
    Y = np.empty((4096, 4096), np.uint8)
    for k, (r, c) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
        Y[r::2, c::2] = 4 * q + k
    for a in (Y, U, V):
        a.setflags(write=False)
    return Y, U, V


@functools.lru_cache(maxsize=None)
def cube(layout):
    frame = pack_yuv(*cube_planes(), layout)
    frame.setflags(write=False)
    return frame


# ---------------------------------------------------------------------------
# numpy references (independent of the library)

def _up(p):
    """A half-resolution plane at full resolution: each sample covers its 2 x 2 block."""
    return np.repeat(np.repeat(p, 2, axis=-2), 2, axis=-1)


def _clip_into(out, k, v):
    out[..., k] = np.clip(v, 0, 255)


def ref_nv(frame, layout, rgb):
    """The reference's own NV21 / NV12 decode: ra = 179 (v - 128) >> 7,
    ga = (44 (u - 128) + 91 (v - 128)) >> 7, ba = 227 (u - 128) >> 7 (arithmetic
    shifts of ints), then clamp Y + ba, Y - ga, Y + ra to a byte; BGR or RGB."""
    Y, U, V = split_yuv(frame, layout)
    u, v = U.astype(np.int32) - 128, V.astype(np.int32) - 128
    ra, ga, ba = (179 * v) >> 7, (44 * u + 91 * v) >> 7, (227 * u) >> 7
    y = Y.astype(np.int32)
    out = np.empty(Y.shape + (3,), np.uint8)
    _clip_into(out, 2 if rgb else 0, y + _up(ba))
    _clip_into(out, 1, y - _up(ga))
    _clip_into(out, 0 if rgb else 2, y + _up(ra))
    return out


def ref_cv(frame, layout, rgb, dcn):
    """OpenCV 2.4's BT.601 in 20-bit fixed point (the header comment of
    csrc/k_color_cv.hip): y' = max(0, Y - 16) * 1220542, R = sat((y' + 2^19 +
    1673527 v) >> 20), G = sat((y' + 2^19 - 852492 v - 409993 u) >> 20), B =
    sat((y' + 2^19 + 2116026 u) >> 20) with u = U - 128, v = V - 128; alpha
    255.  int32 holds every intermediate: |y' + 2^19 + term| < 2^30."""
    Y, U, V = split_yuv(frame, layout)
    u, v = U.astype(np.int32) - 128, V.astype(np.int32) - 128
    ruv, guv, buv = (1 << 19) + 1673527 * v, (1 << 19) - 852492 * v - 409993 * u, (1 << 19) + 2116026 * u
    yy = np.maximum(Y.astype(np.int32) - 16, 0) * 1220542
    out = np.full(Y.shape + (dcn,), 255, np.uint8)
    _clip_into(out, 0 if rgb else 2, (yy + _up(ruv)) >> 20)
    _clip_into(out, 1, (yy + _up(guv)) >> 20)
    _clip_into(out, 2 if rgb else 0, (yy + _up(buv)) >> 20)
    return out


def ref_gray(g):
    """GRAY2BGR: the value in every colour channel."""
    g = np.asarray(g)
    return np.ascontiguousarray(np.broadcast_to(g[..., None], g.shape + (3,)))


def ref_code(frame, code):
    if code in NV_CODES:
        layout, rgb, _ = NV_CODES[code]
        return ref_nv(frame, layout, rgb)
    layout, rgb, dcn = CV_CODES[code]
    return ref_cv(frame, layout, rgb, dcn)


def code_layout(code):
    return (NV_CODES.get(code) or CV_CODES[code])[0]


@functools.lru_cache(maxsize=None)
def cube_ref(code):
    """The reference decode of the cube, computed once per code and shared by the CPU and the GPU tests."""
    out = ref_code(cube(code_layout(code)), code)
    out.setflags(write=False)
    return out


@pytest.fixture(scope="module", autouse=True)
def _release_cube():
    """The cached cube and its nine decodes are half a gigabyte: dropped when this module's tests are done."""
    yield
    for f in (cube_ref, cube, cube_planes):
        f.cache_clear()


def yuv_chain(oracle, yuv, w, h, v_first, rgb, mode, mean=None, std=None, chw=False, u8=False):
    """The reference's own chain, step by step, on the oracle: cvt_color ->
    resize INTER_LINEAR u8 -> change_dtype FP32 -> normalize -> change_layout
    (as _yuv_chain of test_gpu_parity)."""
    r = oracle.resize_linear(oracle.yuv420sp_to_bgr(yuv, v_first=v_first, rgb=rgb), w, h, mode)
    if not u8:
        r = oracle.u8_to_f32(r)
        if mean is not None:
            r = oracle.normalize(r, mean, std)
    return oracle.hwc_to_chw(r) if chw else r


def exact_stats(u8_images):
    """Per-image (n, c) mean / stddev of u8 NHWC images from exact integer sums (stats_kernel's formula)."""
    sums, _, count = ref_sums(u8_images)
    return ref_mean_std(sums, count)


# ---------------------------------------------------------------------------
# 1. the references against the oracle's C functions (CPU, no device)

def test_references_match_oracle(oracle):
    """ref_nv, ref_cv and ref_gray equal oracle.yuv420sp_to_bgr, yuv420_cv and
    gray_to_bgr on the cube -- every (Y, U, V) triple, for every code -- and on
    2 x 2 and 10 x 6 frames (one block; odd block counts).  The cube holds
    2^24 distinct triples by construction.  The oracle's resize_linear at equal
    size is the identity on the decoded cube in all three modes: the premise
    of test_cube_nv_codes' equal-size cvt_color_resize runs."""
    Y, U, V = cube_planes()
    key = (Y.astype(np.int64) << 16) | (_up(U).astype(np.int64) << 8) | _up(V)
    assert np.array_equal(np.bincount(key.reshape(-1), minlength=1 << 24), np.ones(1 << 24, np.int64))
    del key
    for layout in (NV12, NV21, YV12):  # the three layouts hold the same planes
        for got, want in zip(split_yuv(cube(layout), layout), (Y, U, V)):
            assert np.array_equal(got, want)
    for code in list(NV_CODES) + list(CV_CODES):
        layout, rgb, _ = (NV_CODES.get(code) or CV_CODES[code])
        small = [rand_frames(1, w, h, layout, 10 * w + code)[0] for w, h in ((2, 2), (10, 6))]
        for frame, ref in [(cube(layout), cube_ref(code))] + [(f, ref_code(f, code)) for f in small]:
            if code in NV_CODES:
                want = oracle.yuv420sp_to_bgr(frame, v_first=layout == NV21, rgb=rgb)
            else:
                want = oracle.yuv420_cv(frame, code)
            assert_bits(ref, want, f"code {code} {frame.shape}")
    for mode in (0, 1, 2):
        assert_bits(oracle.resize_linear(cube_ref(BGR_NV21), 4096, 4096, mode), cube_ref(BGR_NV21), f"identity mode {mode}")
    # the other three codes decode to the same frame or to its channels reversed, and the resize treats every
    # channel alike: the identity holds for them too
    assert np.array_equal(cube_ref(BGR_NV12), cube_ref(BGR_NV21))
    for code in (RGB_NV21, RGB_NV12):
        assert np.array_equal(cube_ref(code), cube_ref(BGR_NV21)[..., ::-1])
    for g in (cube(NV21), rand_frames(1, 2, 2, NV21, 3)[0], rand_frames(1, 10, 6, NV21, 4)[0]):
        assert_bits(ref_gray(g), oracle.gray_to_bgr(g), "gray u8")
        f = g[:64].astype(np.float32) * np.float32(0.37) - np.float32(11.5)
        assert_bits(ref_gray(f), oracle.gray_to_bgr(f), "gray fp32")


# ---------------------------------------------------------------------------
# helpers: placed YUV sources and destinations

def to_dev(a, dev):
    import torch
    return torch.from_numpy(np.array(a)).to(dev)  # a copy: the cached cube is read-only


def place_yuv(frames, dev, off=0, row_pad=0, batch_pad=0):
    """(n, h * 3 / 2, w) frames as the (n, h * 3 / 2, w, 1) NHWC image of
    `place`: every row (chroma rows too) followed by row_pad bytes, every frame
    by batch_pad bytes.  Returns the (n, h * 3 / 2, w) view the ops take."""
    _, view = place(np.asarray(frames)[..., None], dev, NHWC, off=off, row_pad=row_pad, batch_pad=batch_pad)
    return view[..., 0]


def place_planes(a, dev, off=0, row_pad=0, plane_pad=0, batch_pad=0):
    """`place` for NCHW with plane padding: every row followed by row_pad,
    every plane by plane_pad and every image by batch_pad unused elements."""
    import torch
    a = np.ascontiguousarray(a)
    es = a.itemsize
    assert off % es == 0
    n, c, h, w = a.shape
    rp = w + row_pad
    pl = h * rp + plane_pad
    img = c * pl + batch_pad
    strides = (img, pl, rp, 1)
    flat = np.full(off + n * img * es + 32, SENTINEL, np.uint8)
    typed = flat[off:off + n * img * es].view(a.dtype)
    np.lib.stride_tricks.as_strided(typed, a.shape, [s * es for s in strides])[...] = a
    buffer = torch.from_numpy(flat).to(dev)
    view = buffer[off:off + n * img * es].view(_torch_dtype(a.dtype)).as_strided(a.shape, strides)
    return buffer, view


def check_into(fn, want, dev, what, layout=NHWC, off=0, row_pad=0, plane_pad=0, batch_pad=0):
    """Run fn(out=view) on a SENTINEL destination placed as given: the view equals `want` bit for bit and the
    rim is intact."""
    if layout == NHWC:
        dbuf, dview = place(blank(want.shape, want.dtype), dev, NHWC, off=off, row_pad=row_pad, batch_pad=batch_pad)
    else:
        dbuf, dview = place_planes(blank(want.shape, want.dtype), dev, off, row_pad, plane_pad, batch_pad)
    fn(dview)
    assert_bits(host(dview), want, what)
    assert_rim_intact(dbuf, dview, what)


def invalid_arg(fn):
    import vacv_amd as V
    with pytest.raises(V.VacvError) as e:
        fn()
    assert e.value.status == V._lib.ERR_INVALID_ARG, e.value.status


# ---------------------------------------------------------------------------
# 2. every (Y, U, V) triple

RESIZE_KNOBS = ({}, dict(RESIZE_TILE_W=64), dict(RESIZE_DIRECT=3), dict(RESIZE_DIRECT=2))


@gpu
@pytest.mark.parametrize("code", list(NV_CODES))
def test_cube_nv_codes(ops, dev, code):
    """chroma_terms (color_kernel) and the packed int16 decode_yuv
    (k_yuv_resize.hip) on all 2^24 triples.  cvt_color of the cube equals
    ref_nv.  cvt_color_resize at wo = w, ho = h (every tap weighs one source
    pixel with 2048: the oracle's resize is the identity there,
    test_references_match_oracle) must return the same frame in modes 0, 1, 2
    through each instance of the decode: the default (4096-byte rows at a
    128-byte aligned base, step 1: yuv_cols_cw = 2, POINT), RESIZE_TILE_W = 64
    (CW = 1, POINT), RESIZE_DIRECT = 3 (the blending column kernel, ONE_ROW)
    and RESIZE_DIRECT = 2 (the row-major yuv_resize_kernel, ONE_ROW, dense
    chunked stores)."""
    import torch
    layout, rgb, _ = NV_CODES[code]
    src = to_dev(cube(layout), dev)[None]
    got = ops.cvt_color(src, code)
    assert_bits(host(got)[0], cube_ref(code), f"cvt_color code {code}, all triples")
    for mode in (0, 1, 2):
        for knobs in RESIZE_KNOBS:
            with ops.tuning(**knobs):
                r = ops.cvt_color_resize(src, 4096, 4096, code, mode=mode)
            assert torch.equal(r, got), f"equal-size cvt_color_resize code {code} mode {mode} {knobs}: " \
                                        f"{int((r != got).sum())} values differ"
            del r


@gpu
@pytest.mark.parametrize("code", list(CV_CODES))
def test_cube_cv_codes(ops, dev, code):
    """bt601's saturating 20-bit fixed point on all 2^24 triples, in each of
    its three kernels.  The dense cube at an aligned base takes
    yuv420_cv8x_kernel (w % 8 == 0, every base and pitch 16-byte aligned);
    RESIZE_DIRECT = 2 takes yuv420_cv8_kernel; a destination 4 (BGRA) or 2
    (BGR) bytes into its buffer fails launch_color_cv's 16 / 8-byte condition
    and takes the 2 x 2 yuv420_cv_kernel with byte stores (BGRA: aligned needs
    8) or 2-byte stores (BGR: aligned needs 2)."""
    import torch
    layout, rgb, dcn = CV_CODES[code]
    src = to_dev(cube(layout), dev)[None]
    got = ops.cvt_color(src, code)
    assert_bits(host(got)[0], cube_ref(code), f"cvt_color code {code}, all triples")
    with ops.tuning(RESIZE_DIRECT=2):
        b = ops.cvt_color(src, code)
    assert torch.equal(b, got), f"code {code}: yuv420_cv8_kernel differs on {int((b != got).sum())} values"
    del b
    off = 4 if dcn == 4 else 2
    buf = torch.full((got.numel() + 32,), SENTINEL, dtype=torch.uint8, device=dev)
    view = buf[off:off + got.numel()].view(got.shape)
    ops.cvt_color(src, code, out=view)
    assert torch.equal(view, got), f"code {code}: yuv420_cv_kernel differs on {int((view != got).sum())} values"
    assert bool((buf[:off] == SENTINEL).all()) and bool((buf[off + got.numel():] == SENTINEL).all())


# ---------------------------------------------------------------------------
# 3. misaligned, pitched and tail shapes: color_kernel

COLOR_FRAMES = [(2, 2), (6, 2), (8, 6), (258, 10), (512, 2)]
# (source offset, source row pad, u8 destination offset, u8 destination row pad, fp32 destination offset,
# fp32 destination row pad); offsets in bytes, pads in elements.  A padded side also gets a batch pad.
COLOR_SAMPLE = [(0, 0, 0, 0, 0, 0),    # dword loads; u8 dword stores; fp32 16-byte stores / the LDS exchange
                (1, 3, 1, 1, 4, 1),    # byte loads; u8 byte stores; fp32 rows 4 mod 16 and moving: dword stores
                (2, 4, 2, 4, 8, 3),    # byte loads (base 2 mod 4); fp32 rows 8 mod 16, pitch + 12 bytes
                (4, 16, 4, 0, 16, 4),  # dword loads from a pitched source; everything 16-byte aligned again
                (0, 4, 0, 4, 4, 0),    # fp32 dense at offset 4: never 16-byte aligned
                (4, 0, 4, 1, 0, 1),    # u8 rows change alignment from row to row; fp32 pad 1
                (1, 0, 2, 0, 16, 0),
                (0, 16, 1, 4, 8, 4),
                (2, 3, 0, 1, 0, 3)]


@gpu
@pytest.mark.parametrize("wh", COLOR_FRAMES, ids=lambda t: f"{t[0]}x{t[1]}")
def test_color_kernel_paths(ops, dev, wh):
    """color_kernel for NV21 -> BGR and NV12 -> RGB: cvt_color (u8),
    cvt_color_normalize with host mean / std, and with mean = None (fp32 first
    pass, per-image statistics, normalize in place) into a dense destination
    at byte offsets 0 and 4; batch of 3, against ref_nv.

    Frames: 2 x 2 -- one thread with 2 valid pixels (byte loads, element
    stores); 6 x 2 -- a full thread and a 2-pixel one; 8 x 6 -- three row
    pairs in a four-wave block (the fourth wave leaves at 2 yy >= h); 258 x 10
    -- a whole 256-pixel block (wave_full) and a second block of one 2-pixel
    thread, five row pairs so the second block row is partial; 512 x 2 -- two
    whole blocks.
    Loads: dwords when y0p | y1p | uvp is 4-byte aligned (source offsets 0, 4
    with row pads 0, 4, 16; a batch pad of 5 moves images 1 and 2 off it),
    bytes otherwise (offsets 1, 2, row pad 3).
    Stores: u8 rows go out as dwords when the row start is 4-byte aligned
    (offsets 0, 4 with pads 0, 4 -- at w = 258 / 6 / 2 the 3 w-byte dense rows
    alternate), bytes otherwise.  fp32: 16-byte stores when dp is 16-byte
    aligned, dwords otherwise; a wave_full block whose row start wbase is
    16-byte aligned takes the LDS exchange (w = 512 at offsets 0 / 16: every
    row; w = 258: 3,096-byte dense rows, so every other row), and the cases
    with w >= 256 and offset 4 / 8 or a row pad of 1 / 3 floats are the
    "whole block, misaligned row" fallback to per-lane stores."""
    w, h = wh
    for code in (BGR_NV21, RGB_NV12):
        layout, rgb, _ = NV_CODES[code]
        frames = rand_frames(3, w, h, layout, 1000 * w + h + code)
        want = ref_nv(frames, layout, rgb)
        wantn = ref_normalize(want, MEAN, STD)
        for soff, spad, d8, p8, d32, p32 in COLOR_SAMPLE:
            what = f"code {code} {w}x{h} src off {soff} pad {spad} dst u8 {d8}/{p8} fp32 {d32}/{p32}"
            src = place_yuv(frames, dev, soff, spad, 5 if spad else 0)
            check_into(lambda o: ops.cvt_color(src, code, out=o), want, dev, "cvt_color " + what,
                       off=d8, row_pad=p8, batch_pad=7 if p8 else 0)
            check_into(lambda o: ops.cvt_color_normalize(src, code, MEAN, STD, out=o), wantn, dev,
                       "cvt_color_normalize " + what, off=d32, row_pad=p32, batch_pad=p32)
        m, s = exact_stats(want)
        wanta = ref_normalize(want, m, s)
        for doff, (soff, spad) in ((0, (0, 0)), (4, (1, 3)), (4, (0, 0)), (0, (2, 4))):
            src = place_yuv(frames, dev, soff, spad, 5 if spad else 0)
            check_into(lambda o: ops.cvt_color_normalize(src, code, out=o), wanta, dev,
                       f"cvt_color_normalize, own statistics, code {code} {w}x{h} dst off {doff} src {soff}/{spad}", off=doff)


# ---------------------------------------------------------------------------
# 3. k_color_cv.hip: the YUV codes

CV_FRAMES = [(2, 2), (10, 6), (8, 2), (24, 2), (16, 4), (520, 4)]
# (source offset, source row pad (NV codes only), destination offset, destination row pad in PIXELS, source batch
# pad, destination batch pad); the rest in bytes
CV_SAMPLE = [(0, 0, 0, 0, 0, 0),    # all aligned: w % 8 == 0 -> the 8 x 2 kernels (where the rows are)
             (0, 0, 8, 0, 0, 0),    # destination 8 mod 16: BGRA -> 2 x 2 (needs 16), BGR -> yuv420_cv8_kernel
             (0, 0, 16, 4, 0, 0),   # rows + 16 (BGRA) / + 12 (BGR) bytes
             (0, 8, 0, 2, 0, 0),    # BGRA rows + 8: not 16 -> 2 x 2 with uint2 stores; BGR rows + 6
             (8, 8, 16, 4, 0, 0),   # source 8 mod 16 keeps the 8-byte loads
             (8, 0, 8, 2, 0, 0),
             (1, 3, 1, 1, 0, 0),    # everything odd: 2 x 2, byte loads, byte stores
             (0, 3, 2, 1, 0, 0),    # BGR at 2 mod 8 with odd rows (pad 1 px = 3 bytes): bytes; BGRA 2 mod 8: bytes
             (1, 0, 0, 0, 0, 0),    # only the source misaligned: 2 x 2 with aligned (uint2 / 2-byte) stores
             (8, 3, 2, 4, 0, 0),    # BGR rows + 12 at base 2: the 2-byte stores of the 2 x 2 kernel
             (0, 8, 1, 2, 0, 0),
             (0, 8, 0, 0, 8, 16),   # aligned batch pads keep the 8 x 2 kernels
             (0, 0, 0, 0, 4, 0)]    # src_img & 7 != 0 alone -> 2 x 2


def _cv_case(ops, dev, frames, want, code, soff, spad, doff, dpad_bytes, sbp, dbp, what):
    src = place_yuv(frames, dev, soff, spad, sbp)
    for knobs in ({}, dict(RESIZE_DIRECT=2)):
        with ops.tuning(**knobs):
            check_into(lambda o: ops.cvt_color(src, code, out=o), want, dev, f"{what} {knobs}",
                       off=doff, row_pad=dpad_bytes, batch_pad=dbp)


@gpu
@pytest.mark.parametrize("wh", CV_FRAMES, ids=lambda t: f"{t[0]}x{t[1]}")
def test_color_cv_yuv_paths(ops, dev, wh):
    """launch_color_cv's four YUV kernels for NV12 / NV21 -> RGBA / BGRA and
    YV12 -> BGR, batch of 3, against ref_cv, at the default knobs and under
    RESIZE_DIRECT = 2 (yuv420_cv8_kernel instead of the wave kernel).

    The 8 x 2 kernels need w % 8 == 0, the source base, row and image pitch
    8-byte aligned and the destination's 16 (BGRA) or 8 (BGR); the wave kernel
    yuv420_cv8x_kernel needs the destination's 16 as well; everything else
    takes the 2 x 2 yuv420_cv_kernel, whose stores are uint2 (BGRA) / 2-byte
    (BGR) when the destination base, row and image pitch are 8 / 2-byte
    aligned, bytes otherwise.
    Frames: 2 x 2 and 10 x 6 -- w % 8 != 0: always 2 x 2 (one block; 15
    blocks); 8 x 2 -- one 8 x 2 unit (BGR rows of 24 bytes: 8- but not 16-byte
    aligned, so yuv420_cv8_kernel; one live lane and the odd-lane tail with an
    8-byte row pad); 24 x 2 -- 36-byte frames, src_img & 7 != 0 selects 2 x 2
    although w % 8 == 0; 16 x 4 -- two units, two row pairs, 96-byte frames;
    520 x 4 -- 65 units: the wave kernel's second block has one live lane
    (BGRA: nck = 2 whole chunks; BGR: nck = 1 and the (nl & 1) 8-byte tail).
    A dense BGR row of an odd unit count is 8 mod 16, so the BGR tail needs
    pitched rows: an 8-byte row pad (1,568-byte rows) reaches it.
    Destination offsets 0, 1, 2, 8, 16 and row pads of 0, 1, 2, 4 pixels move
    BGRA rows across the 8- and 16-byte conditions and BGR rows across 2 / 8 /
    16; source offsets 0, 1, 8 and row pads 0, 3, 8 across the source's 8."""
    w, h = wh
    for code, (layout, rgb, dcn) in CV_CODES.items():
        frames = rand_frames(3, w, h, layout, 100 * w + h + code)
        want = ref_cv(frames, layout, rgb, dcn)
        for soff, spad, doff, dpad, sbp, dbp in CV_SAMPLE:
            spad = 0 if layout == YV12 else spad  # planar chroma: dense rows only
            what = f"code {code} {w}x{h} src {soff}/{spad}/{sbp} dst {doff}/{dpad}px/{dbp}"
            _cv_case(ops, dev, frames, want, code, soff, spad, doff, dpad * dcn, sbp, dbp, what)
        if dcn == 3:  # 16-byte aligned BGR rows at an odd unit count (w = 8, 520): the wave kernel's tail store
            for doff in (0, 16):
                _cv_case(ops, dev, frames, want, code, 0, 0, doff, 8, 0, 0, f"code {code} {w}x{h} dst {doff}/8 bytes")


@gpu
def test_color_cv_yv12_source_pitch(ops, dev):
    """YV12's chroma planes are addressed as (w / 2)-byte rows right after the
    Y plane, so a row-pitched source is VACV_ERR_INVALID_ARG (color_cv_impl:
    src.row != src.w) and nothing is written; a batch pad leaves each frame
    contiguous and is accepted (16 x 4 frames of 96 + 5 bytes: src_img & 7 != 0
    -> 2 x 2; 96 + 8: the 8 x 2 kernels)."""
    frames = rand_frames(3, 16, 4, YV12, 5)
    want = ref_cv(frames, YV12, False, 3)
    for spad in (3, 8):
        src = place_yuv(frames, dev, 0, spad, 0)
        dbuf, dview = place(blank(want.shape, np.uint8), dev)
        invalid_arg(lambda: ops.cvt_color(src, BGR_YV12, out=dview))
        assert_untouched(dbuf, f"YV12 with a row pad of {spad}")
    for sbp in (5, 8):
        _cv_case(ops, dev, frames, want, BGR_YV12, 0, 0, 0, 0, sbp, 0, f"YV12 with a batch pad of {sbp}")


# ---------------------------------------------------------------------------
# 3. k_color_cv.hip: GRAY2BGR

GRAY_WIDTHS = {np.uint8: (1, 15, 16, 17, 1040), np.float32: (1, 3, 4, 5, 260)}
# (source offset, destination offset, source row pad, destination row pad); offsets in bytes, pads in elements
GRAY_SAMPLE = {
    np.uint8: [(0, 0, 0, 0), (16, 16, 16, 16), (16, 0, 0, 16), (0, 16, 16, 0), (1, 0, 0, 0), (0, 1, 0, 1), (4, 4, 1, 1),
               (0, 4, 1, 0), (4, 0, 16, 1), (1, 16, 1, 16)],
    np.float32: [(0, 0, 0, 0), (16, 16, 16, 16), (16, 0, 0, 16), (0, 16, 16, 0), (4, 0, 0, 0), (0, 4, 1, 1), (4, 4, 16, 1),
                 (0, 16, 1, 0), (16, 4, 0, 16)]}


@gpu
@pytest.mark.parametrize("dtype", [np.uint8, np.float32])
def test_color_cv_gray_paths(ops, dev, dtype):
    """GRAY2BGR, batch of 3 of height 3, against ref_gray, at the default
    knobs and under RESIZE_DIRECT = 2.  A unit is 16 u8 / 4 fp32 pixels.
    launch_color_cv takes the vector path when every base, row and image pitch
    is 16-byte aligned (offsets 0 / 16, pads 0 / 16, and a width whose dense
    row and image are multiples of 16 bytes: u8 16 and 1040, fp32 4 and 260);
    gray_x_kernel (a wave per 64 units) when also w % unit == 0 and the knob
    allows, gray_kernel otherwise, whose whole units go out as vectors and
    whose partial last unit (widths 1, 15, 17; 1, 3, 5) and every unit of a
    misaligned image (offsets 1, 4; pad 1) element by element.  1040 u8 / 260
    fp32 pixels are 65 units: gray_x_kernel's second block has one live lane."""
    for w in GRAY_WIDTHS[dtype]:
        g = np.random.default_rng(w).integers(0, 256, (3, 3, w)).astype(dtype)
        if dtype == np.float32:
            g = g * np.float32(0.37) - np.float32(11.5)
        want = ref_gray(g)
        for soff, doff, spad, dpad in GRAY_SAMPLE[dtype]:
            _, sview = place(g[..., None], dev, NHWC, off=soff, row_pad=spad)
            src = sview[..., 0]
            for knobs in ({}, dict(RESIZE_DIRECT=2)):
                with ops.tuning(**knobs):
                    check_into(lambda o: ops.cvt_color(src, GRAY2BGR, out=o), want, dev,
                               f"gray {np.dtype(dtype).name} w {w} off {soff}/{doff} pad {spad}/{dpad} {knobs}",
                               off=doff, row_pad=dpad)


# ---------------------------------------------------------------------------
# 3. k_yuv_resize.hip

# ((w, h), (wo, ho), modes)
RESIZE_GEOMS = [((4, 2), (1, 1), (0,)), ((4, 2), (3, 5), (0,)), ((50, 36), (17, 11), (0, 1, 2)),
                ((50, 36), (65, 5), (0,)), ((50, 36), (64, 9), (0,)), ((176, 144), (130, 3), (0,)),
                ((192, 24), (64, 8), (0, 1, 2)), ((384, 24), (128, 8), (0, 1, 2)),
                ((520, 6), (260, 4), (0,)), ((1560, 6), (520, 2), (0,))]
# (source offset, source row pad, source batch pad)
RESIZE_SRC = [(0, 0, 0), (1, 0, 0), (2, 3, 5), (3, 78, 0), (0, 78, 5), (0, 3, 0)]
# output kinds: (name, layout, dtype)
RESIZE_KINDS = [("u8 nhwc", NHWC, np.uint8), ("u8 nchw", NCHW, np.uint8), ("f32 nhwc", NHWC, np.float32),
                ("norm nhwc", NHWC, np.float32), ("norm nchw", NCHW, np.float32)]


def _dst_placements(wo, ho, layout, es):
    """(name, byte offset, row pad, plane pad, batch pad), pads in elements."""
    per = 16 // es  # elements in 16 bytes
    row = wo * (3 if layout == NHWC else 1)
    r16 = per - row % per  # the smallest positive pad that makes the pitch a multiple of 16 bytes
    out = [("dense at 0", 0, 0, 0, 0), ("dense at 16", 16, 0, 0, 0), ("dense, misaligned", 1 if es == 1 else 4, 0, 0, 0),
           # pitched rows with every pitch a multiple of 16 bytes (the plane's rounded up for NCHW)
           ("rows + pad, 16-byte pitches", 0, r16, (-ho * (row + r16)) % per if layout == NCHW else 0, 0),
           ("rows + 1", 0, 1, 0, 0)]
    if layout == NCHW:
        out += [("planes + 4", 0, 0, 4, 0), ("planes + 5", 0, 0, 5, 0)]
    return out


@gpu
@pytest.mark.parametrize("geom", RESIZE_GEOMS, ids=lambda g: f"{g[0][0]}x{g[0][1]}-{g[1][0]}x{g[1][1]}")
def test_yuv_resize_paths(ops, dev, oracle, geom):
    """cvt_color_resize / cvt_color_resize_normalize for NV21 -> BGR and NV12
    -> RGB into u8 NHWC, u8 NCHW, fp32 NHWC, normalised fp32 NHWC and NCHW,
    batch of 3, against the oracle's chain, at the default knobs and under
    RESIZE_DIRECT = 2 for every destination placement.

    launch_layout_t takes the column-stationary yuv_cols_kernel when the
    destination base, row, plane and image pitch are all 16-byte aligned, else
    the row-major yuv_resize_kernel (always under RESIZE_DIRECT = 2).
    Destination placements: dense at byte offset 0 and 16 -- the column kernel
    where the dense rows, planes and images are multiples of 16 bytes (64 x 8,
    128 x 8, 64 x 9); at the other sizes a pitch is off 16 and the row-major
    kernel runs, dense: store_range_from_lds chunked on the images (planes)
    that start aligned with aligned rows, bytes on the others; dense at
    offset 1 (u8) / 4 (fp32) -- row-major,
    unchunked; a row pad that makes every pitch a multiple of 16 -- the column
    kernel with pitched rows (16-byte chunks where a block row's bytes are
    whole chunks, bytes otherwise), and under RESIZE_DIRECT = 2 the row-major
    kernel with chunked pitched stores where the dense row is whole chunks (wo
    = 64, 128; fp32 NCHW wo % 4 == 0), unchunked otherwise; a row pad of 1
    element -- row-major, pitched, unchunked; NCHW plane pads of 4 elements
    (fp32: 16 bytes, alignment kept where the plane had it) and 5 (planes 1
    and 2 misaligned: row-major with a chunked plane 0 and byte planes).
    Geometries: 4 x 2 -> 1 x 1 and 3 x 5 -- the narrowest legal source (the
    chroma dword is the whole row), one pixel, upscaling; 50 x 36 -> 17 x 11 --
    two-tap rows (taps 0); -> 65 x 5 -- a second column block of one column;
    -> 64 x 9 -- one whole column block, one row group of 8 and one row; 176 x
    144 -> 130 x 3 -- three column blocks, the last of two columns; 192 x 24
    -> 64 x 8 -- 3 x point sampling (POINT; RESIZE_DIRECT = 2: ONE_ROW);
    384 x 24 -> 128 x 8 -- 3 x with 384-byte rows, the only shape here where
    yuv_cols_cw returns 2: at source offset 0 with dense rows and no batch pad
    (rows, base and frames whole 128-byte lines); at offset 1, 2, 3, with a row
    pad or the batch pad of 5 it returns 1; 520 x 6 -> 260 x 4 (two-tap) and
    1560 x 6 -> 520 x 2 (3 x) -- outputs at least as wide as a wave's 256
    (two-row) or 512 (ONE_ROW) pixels: yuv_resize_kernel's `wide` branch, where
    a wave spans at most two output rows and selects between their two
    precomputed vertical taps (the second wave of 260 x 4 starts at pixel 256
    of row 0 and runs into row 1, whose weights differ).
    Source placements: byte offsets 0-3 are make_rsrc's delta (the buffer
    resource starts at the 16-byte boundary below); row pads 0, 3 and 78 (128
    byte rows at w = 50); a batch pad of 5.  Every source placement runs into
    the first destination placement; the others take them in turn.
    Modes 0, 1, 2 on the two-tap and the point geometries, mode 0 elsewhere."""
    import torch
    (w, h), (wo, ho), modes = geom
    k = 0
    for code in (BGR_NV21, RGB_NV12):
        layout, rgb, _ = NV_CODES[code]
        frames = rand_frames(3, w, h, layout, 7 * w + wo + code)
        srcs = [place_yuv(frames, dev, *s) for s in RESIZE_SRC]
        for mode in modes:
            for name, lay, dt in RESIZE_KINDS:
                norm = name.startswith("norm")
                want = np.stack([yuv_chain(oracle, f, wo, ho, layout == NV21, rgb, mode, MEAN if norm else None, STD,
                                           chw=lay == NCHW, u8=dt == np.uint8) for f in frames])
                for i, (pname, off, rpad, ppad, bpad) in enumerate(_dst_placements(wo, ho, lay, np.dtype(dt).itemsize)):
                    for knobs in ({}, dict(RESIZE_DIRECT=2)):
                        for si in (range(len(srcs)) if i == 0 else [k % len(srcs)]):
                            k += 1
                            src = srcs[si]
                            if norm:
                                fn = lambda o: ops.cvt_color_resize_normalize(src, wo, ho, MEAN, STD, code, layout=lay,
                                                                              mode=mode, out=o)
                            else:
                                fn = lambda o: ops.cvt_color_resize(src, wo, ho, code, layout=lay, dtype=_torch_dtype(dt),
                                                                    mode=mode, out=o)
                            with ops.tuning(**knobs):
                                check_into(fn, want, dev,
                                           f"code {code} {w}x{h}->{wo}x{ho} mode {mode} {name}, {pname}, src {RESIZE_SRC[si]} {knobs}",
                                           layout=lay, off=off, row_pad=rpad, plane_pad=ppad, batch_pad=bpad)
    if (w, wo) == (384, 128):  # CW = 2 (dense source at a 128-byte aligned base) against CW = 1
        src = to_dev(frames, dev)
        assert src.data_ptr() % 128 == 0
        for lay in (NHWC, NCHW):
            a = ops.cvt_color_resize_normalize(src, wo, ho, MEAN, STD, RGB_NV12, layout=lay)
            with ops.tuning(RESIZE_TILE_W=64):
                b = ops.cvt_color_resize_normalize(src, wo, ho, MEAN, STD, RGB_NV12, layout=lay)
            assert torch.equal(a, b), "128-column blocks differ from 64-column ones"


# ---------------------------------------------------------------------------
# 4. refusals write nothing

@gpu
def test_auto_statistics_refuse_pitched_destination(ops, dev, oracle):
    """mean = stddev = NULL asks for per-image statistics of the fp32 result,
    which are taken over one dense range per image (per_image_stats): a
    destination with a row pad or a batch pad is VACV_ERR_UNSUPPORTED through
    all four fused entry points, and -- as for every refused call -- nothing
    is written (fused_normalize used to run its first pass into the
    destination before the statistics refused it); so is an NHWC destination
    of 5 channels and an NCHW one with a plane pad.  The same calls into a
    dense destination 4 bytes into its buffer succeed and equal the chain of
    the oracle's operator, the exact per-image statistics and normalize."""
    rng = np.random.default_rng(77)
    img = rng.integers(0, 256, (2, 20, 30, 3), dtype=np.uint8)
    frames = rand_frames(2, 30, 20, NV21, 78)
    m = np.array([0.9, 0.2, 1.5, -0.3, 1.1, 2.0], np.float32)
    wo, ho = 17, 11
    simg, syuv = to_dev(img, dev), to_dev(frames, dev)
    bgr = ref_nv(frames, NV21, False)
    calls = [
        ("resize_normalize", lambda o: ops.resize_normalize(simg, wo, ho, out=o),
         np.stack([oracle.resize_linear(x, wo, ho) for x in img])),
        ("warp_affine_normalize", lambda o: ops.warp_affine_normalize(simg, m, wo, ho, out=o),
         np.stack([oracle.warp_affine(x, m, wo, ho) for x in img])),
        ("cvt_color_normalize", lambda o: ops.cvt_color_normalize(syuv, BGR_NV21, out=o), bgr),
        ("cvt_color_resize_normalize", lambda o: ops.cvt_color_resize_normalize(syuv, wo, ho, layout=NHWC, out=o),
         np.stack([oracle.resize_linear(x, wo, ho) for x in bgr]))]
    for name, fn, u8 in calls:
        for rpad, bpad in ((4, 0), (0, 4), (1, 3)):
            dbuf, dview = place(blank(u8.shape, np.float32), dev, row_pad=rpad, batch_pad=bpad)
            unsupported(lambda: fn(dview))
            assert_untouched(dbuf, f"{name} with own statistics, row pad {rpad}, batch pad {bpad}")
        mean, std = exact_stats(u8)
        check_into(fn, ref_normalize(u8, mean, std), dev, f"{name} with own statistics, dense at offset 4", off=4)
    # NHWC with more than 4 channels has no per-image statistics either: refused before the first pass, dense or not
    img5 = to_dev(rng.integers(0, 256, (2, 20, 30, 5), dtype=np.uint8), dev)
    dbuf, dview = place(blank((2, ho, wo, 5), np.float32), dev)
    unsupported(lambda: ops.resize_normalize(img5, wo, ho, out=dview))
    assert_untouched(dbuf, "resize_normalize with own statistics, 5 channels")
    # the planar destination of the fused colour resize: a plane pad is not dense either
    u8 = calls[3][2]
    chw = np.ascontiguousarray(u8.transpose(0, 3, 1, 2))
    fn = lambda o: ops.cvt_color_resize_normalize(syuv, wo, ho, layout=NCHW, out=o)
    dbuf, dview = place_planes(blank(chw.shape, np.float32), dev, plane_pad=4)
    unsupported(lambda: fn(dview))
    assert_untouched(dbuf, "cvt_color_resize_normalize with own statistics, NCHW plane pad")
    mean, std = exact_stats(u8)
    check_into(fn, ref_normalize(chw, mean, std, NCHW), dev, "NCHW, own statistics, dense at offset 4", layout=NCHW, off=4)
