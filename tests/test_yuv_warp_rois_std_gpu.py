"""vacv_cvt_color_warp_affine_rois_standardize on the GPU: many affine crops
straight from NV21 / NV12 frames in one launch, each standardized by its own
per-channel mean and standard deviation (csrc/k_yuv_warp_rois_std.hip).

Every comparison is bit-exact, on the int32 views of the floats, so that -0.0
and +0.0 differ, and the expected value comes from two sources that must both
agree with the result, output and statistics:
 (a) the host oracle: yuv420sp_to_bgr of the indexed frame, warp_affine with
     the border mode, mean_stddev_exact, normalize, hwc_to_chw;
 (b) the GPU chain the call replaces: ops.cvt_color of all frames, then
     ops.warp_affine_rois_standardize on the decoded frames.
Frames are 130 x 98: rows start at 2 modulo 4, a dense frame is 130 x 147
bytes.  The shapes are the smallest that reach every path of the kernel:
outputs of fewer pixels than a workgroup has threads and of more, dense
destinations at every 16-byte phase and pitched ones, maps that sample the
frame's last pixel with the frame's last byte the allocation's last, the
largest ROI the LDS gate admits, more ROIs than the device has CUs.
"""
from __future__ import annotations

import ctypes
import subprocess
from pathlib import Path

import numpy as np
import pytest

from test_crop_resize_rois_std_gpu import oracle_standardized, same_bits
from test_gpu_plumbing import SENTINEL, assert_rim_intact, assert_untouched, host, place, unsupported
from test_warp_rois_gpu import BORDER_U8, IDX7, oracle_rois, random_maps, to_dev, view_in_buffer
from test_yuv_rois_gpu import CODE_IDS, CODES, corner_maps, decode, make_yuv

gpu = pytest.mark.gpu
NHWC, NCHW = 1, 0
INTER_LINEAR, WARP_INVERSE_MAP = 1, 16
CONSTANT, REPLICATE, REFLECT, WRAP, REFLECT_101 = 0, 1, 2, 3, 4
BORDERS = (CONSTANT, REPLICATE, REFLECT, WRAP, REFLECT_101)
NV12_RGB, NV12_BGR, NV21_RGB, NV21_BGR = 90, 91, 92, 93
W, H = 130, 98   # decoded frames
BORDER3 = BORDER_U8[:3]
INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1
SIZES = [(37, 29), (1, 1), (1, 7), (9, 1), (2, 2)]


@pytest.fixture(scope="module")
def ops(hip_device):
    from vacv_amd import ops
    return ops


@pytest.fixture(scope="module")
def dev(hip_device):
    return hip_device


def lds_need(w, h):
    """include/vacv_hip.h's formula (csrc/k_yuv_warp_rois_std.hip), restated."""
    return 256 + (3 * w * h + 15) // 16 * 16 + 3072


def gpu_chain(ops, d_yuv, code, d_ms, wo, ho, d_idx, mode, layout, flags=INTER_LINEAR, border=BORDER_U8):
    """(b): the two calls whose result the one call must reproduce."""
    return ops.warp_affine_rois_standardize(ops.cvt_color(d_yuv, code), d_ms, wo, ho, src_index=d_idx, flags=flags,
                                            border_mode=mode, border_value=border, layout=layout, stats=True)


def check(ops, dev, oracle, yuv, ms, idx, wo, ho, code, layout, modes, what, d_yuv=None, host_oracle=True,
          inverse=False):
    """One call against (a) and (b), output and statistics, for each border
    mode.  inverse: the call and (b) also get the oracle's inverse maps with
    WARP_INVERSE_MAP, which must give the forward call's bits."""
    frames = yuv if yuv.ndim == 3 else yuv[None]
    d_yuv = to_dev(yuv, dev) if d_yuv is None else d_yuv
    ms = np.asarray(ms, np.float32)
    d_ms = to_dev(ms, dev)
    d_idx = to_dev(np.asarray(idx, np.int32), dev) if idx is not None else None
    n = len(ms)
    oidx = idx if idx is not None else ([0] * n if len(frames) == 1 else list(range(n)))
    bgr = decode(oracle, frames, code) if host_oracle else None
    d_inv = to_dev(np.stack([oracle.invert_affine(m) for m in ms]).astype(np.float32), dev) if inverse else None
    for mode in modes:
        w_ = f"{what} {CODE_IDS[code]} layout {layout} {wo}x{ho} border {mode}"
        got, mean, std = ops.cvt_color_warp_affine_rois_standardize(
            d_yuv, d_ms, wo, ho, code=code, src_index=d_idx, border_mode=mode, border_value=BORDER_U8, layout=layout,
            stats=True)
        assert tuple(got.shape) == ((n, ho, wo, 3) if layout == NHWC else (n, 3, ho, wo))
        assert tuple(mean.shape) == tuple(std.shape) == (n, 3)
        c_out, c_mean, c_std = gpu_chain(ops, d_yuv, code, d_ms, wo, ho, d_idx, mode, layout)
        same_bits(got, c_out, w_ + " vs cvt_color + warp_affine_rois_standardize")
        same_bits(mean, c_mean, w_ + ": mean vs the chain")
        same_bits(std, c_std, w_ + ": stddev vs the chain")
        if host_oracle:
            want, wmean, wstd = oracle_standardized(oracle, oracle_rois(oracle, bgr, oidx, ms, wo, ho, BORDER3, mode),
                                                    layout)
            same_bits(got, want, w_ + " vs the oracle chain")
            same_bits(mean, wmean, w_ + ": mean vs oracle")
            same_bits(std, wstd, w_ + ": stddev vs oracle")
        if inverse:
            back = ops.cvt_color_warp_affine_rois_standardize(
                d_yuv, d_inv.reshape(n, 2, 3), wo, ho, code=code, src_index=d_idx,
                flags=INTER_LINEAR | WARP_INVERSE_MAP, border_mode=mode, border_value=BORDER_U8, layout=layout,
                stats=True)
            c_back = gpu_chain(ops, d_yuv, code, d_inv, wo, ho, d_idx, mode, layout, INTER_LINEAR | WARP_INVERSE_MAP)
            for g, c, f, name in zip(back, c_back, (got, mean, std), ("output", "mean", "stddev")):
                same_bits(g, c, w_ + f": WARP_INVERSE_MAP {name} vs the chain")
                same_bits(g, f, w_ + f": WARP_INVERSE_MAP {name} vs the forward call")
        # stats=False writes the same output
        same_bits(ops.cvt_color_warp_affine_rois_standardize(
            d_yuv, d_ms, wo, ho, code=code, src_index=d_idx, border_mode=mode, border_value=BORDER_U8, layout=layout),
            got, w_ + ": stats=False")
    return got, mean, std


# ---------------------------------------------------------------------------
# 1. codes x border modes (with and without WARP_INVERSE_MAP) x layouts x sizes

@gpu
@pytest.mark.parametrize("layout", [NHWC, NCHW], ids=["nhwc", "nchw"])
@pytest.mark.parametrize("code", list(CODES), ids=lambda c: CODE_IDS[c])
def test_matches_both_chains(ops, dev, oracle, code, layout):
    yuv = make_yuv(3, W, H, 1600 + code)
    rng = np.random.default_rng(20261100 + code)
    for wo, ho in SIZES:
        ms = random_maps(rng, 7, W, H, wo, ho)
        got, mean, std = check(ops, dev, oracle, yuv, ms, IDX7, wo, ho, code, layout, BORDERS, "grid", inverse=True)
        if (wo, ho) == (1, 1):  # one pixel: the deviation 0, the output +0.0
            assert not host(std).any() and not host(got).view(np.int32).any() and host(mean).any()


@gpu
def test_model_input_size(ops, dev, oracle):
    yuv = make_yuv(3, W, H, 1611)
    ms = random_maps(np.random.default_rng(1612), 4, W, H, 112, 112)
    check(ops, dev, oracle, yuv, ms, IDX7[:4], 112, 112, NV21_BGR, NCHW, (CONSTANT, REFLECT), "112")


# ---------------------------------------------------------------------------
# 2. the frame's end

@gpu
@pytest.mark.parametrize("off", [0, 1, 2, 3])
def test_frame_end(ops, dev, oracle, off):
    """The dense 130 x 98 frame as the last bytes of its buffer, at every base
    alignment, under maps that sample its last pixel: the last chroma pair is
    read byte by byte, and a load reaching past it has nothing behind it."""
    import torch
    yuv = make_yuv(1, W, H, 1620 + off)
    buf = torch.full((off + yuv.size,), SENTINEL, dtype=torch.uint8, device=dev)
    buf[off:] = to_dev(yuv.reshape(-1), dev)
    d_yuv = buf[off:].view(1, H * 3 // 2, W)
    assert d_yuv.data_ptr() + yuv.size == buf.data_ptr() + buf.numel()
    for wo, ho in [(37, 21), (5, 3)]:
        ms = corner_maps(W, H, wo, ho)
        for code, layout in ((NV21_BGR, NCHW), (NV12_RGB, NHWC)):
            check(ops, dev, oracle, yuv, ms, None, wo, ho, code, layout, (CONSTANT, REPLICATE, WRAP), f"off {off}",
                  d_yuv=d_yuv)
    assert (host(buf)[:off] == SENTINEL).all() and np.array_equal(host(buf)[off:], yuv.reshape(-1))


# ---------------------------------------------------------------------------
# 3. the LDS limit

@gpu
def test_largest_roi_constant_frame(ops, dev):
    """144 x 144 is exactly 64 KiB of LDS.  A constant Y / VU frame decodes to
    one colour, which REPLICATE continues over the whole ROI: stddev 0 and
    every output +0.0.  One row more is refused with nothing written."""
    wo, ho = 144, 144
    assert lds_need(wo, ho) == 65536 < lds_need(wo, ho + 1)
    yuv = np.empty((1, H * 3 // 2, W), np.uint8)
    yuv[0, :H] = 180
    yuv[0, H:, 0::2], yuv[0, H:, 1::2] = 90, 170
    d_yuv = to_dev(yuv, dev)
    d_ms = to_dev(np.array([[1, 0, 0, 0, 1, 0], [1.25, 0.1, 3.5, -0.1, 0.9, 2.25]], np.float32), dev)
    got, mean, std = ops.cvt_color_warp_affine_rois_standardize(d_yuv, d_ms, wo, ho, border_mode=REPLICATE,
                                                                border_value=BORDER_U8, stats=True)
    same_bits(got, np.zeros((2, ho, wo, 3), np.float32), "constant frame")
    assert not host(std).view(np.int32).any() and (host(mean)[0] == host(mean)[1]).all() and host(mean).all()
    c_out, c_mean, c_std = gpu_chain(ops, d_yuv, NV21_BGR, d_ms, wo, ho, None, REPLICATE, NHWC)
    same_bits(got, c_out, "vs the chain")
    same_bits(mean, c_mean, "mean")
    same_bits(std, c_std, "stddev")
    buf, out = place(np.zeros((2, ho + 1, wo, 3), np.float32), dev)
    buf.fill_(SENTINEL)
    unsupported(lambda: ops.cvt_color_warp_affine_rois_standardize(d_yuv, d_ms, wo, ho + 1, border_mode=REPLICATE,
                                                                   out=out))
    assert_untouched(buf, "past the LDS limit")


@gpu
def test_largest_roi_random_frame(ops, dev, oracle):
    yuv = make_yuv(3, W, H, 1631)
    ms = random_maps(np.random.default_rng(1632), 2, W, H, 144, 144)
    check(ops, dev, oracle, yuv, ms, [2, 0], 144, 144, NV21_BGR, NCHW, (CONSTANT, WRAP), "64 KiB", host_oracle=False)


# ---------------------------------------------------------------------------
# 4. pitched, misaligned shapes

PITCH_CASES = [  # layout, dst off (bytes), pitched dst (row + 5, plane + 9, batch + 11 floats)
    (NHWC, 4, True), (NCHW, 8, True), (NCHW, 12, True), (NHWC, 12, True), (NCHW, 4, True), (NHWC, 8, True),
] + [(NHWC, off, False) for off in (0, 4, 8, 12)] + [(NCHW, off, False) for off in (0, 4, 8, 12)]
PITCH_SIZES = [((33, 9), REFLECT), ((5, 3), CONSTANT)]


@pytest.fixture(scope="module")
def pitched_reference(oracle):
    """Frames, maps and (a) for the pitched cases, computed once."""
    yuv = make_yuv(3, W, H, 1640)
    bgr = decode(oracle, yuv, NV21_BGR)
    rng = np.random.default_rng(1641)
    ref = {}
    for (wo, ho), mode in PITCH_SIZES:
        ms = random_maps(rng, 7, W, H, wo, ho)
        u8 = oracle_rois(oracle, bgr, IDX7, ms, wo, ho, BORDER3, mode)
        ref[(wo, ho)] = (ms, {layout: oracle_standardized(oracle, u8, layout) for layout in (NHWC, NCHW)})
    return yuv, ref


@gpu
@pytest.mark.parametrize("case", PITCH_CASES,
                         ids=lambda t: f"{'nchw' if t[0] == NCHW else 'nhwc'}-d{t[1]}-{'pitched' if t[2] else 'dense'}")
def test_pitched_misaligned(ops, dev, pitched_reference, case):
    """src: base off by 3 bytes, rows 5 and frames 7 bytes further apart.  dst:
    dense at every 4-byte alignment class modulo 16, or pitched (row + 5, plane
    + 9, batch + 11 floats); the padding keeps its sentinel."""
    layout, doff, pitched = case
    yuv, ref = pitched_reference
    sbuf, sview = place(yuv[..., None], dev, NHWC, off=3, row_pad=5, batch_pad=7)
    d_yuv = sview[..., 0]
    assert d_yuv.stride() == ((H * 3 // 2) * (W + 5) + 7, W + 5, 1)
    d_idx = to_dev(np.array(IDX7, np.int32), dev)
    n = 7
    rpad, ppad, bpad = (5, 9, 11) if pitched else (0, 0, 0)
    for (wo, ho), mode in PITCH_SIZES:
        ms, want_by_layout = ref[(wo, ho)]
        d_ms = to_dev(ms, dev)
        if layout == NCHW:
            rp = wo + rpad
            pl = ho * rp + ppad
            dbuf, dview = view_in_buffer((n, 3, ho, wo), (3 * pl + bpad, pl, rp, 1), doff, np.float32, dev)
        else:
            rp = wo * 3 + rpad
            dbuf, dview = view_in_buffer((n, ho, wo, 3), (ho * rp + bpad, rp, 3, 1), doff, np.float32, dev)
        what = f"{case} {wo}x{ho}"
        got, mean, std = ops.cvt_color_warp_affine_rois_standardize(
            d_yuv, d_ms, wo, ho, src_index=d_idx, border_mode=mode, border_value=BORDER_U8, layout=layout, out=dview,
            stats=True)
        assert got.data_ptr() == dview.data_ptr()
        want, wmean, wstd = want_by_layout[layout]
        c_out, c_mean, c_std = gpu_chain(ops, d_yuv, NV21_BGR, d_ms, wo, ho, d_idx, mode, layout)
        same_bits(host(dview), want, what)
        same_bits(host(dview), c_out, what + " vs the chain")
        same_bits(mean, wmean, what + ": mean")
        same_bits(mean, c_mean, what + ": mean vs the chain")
        same_bits(std, wstd, what + ": stddev")
        same_bits(std, c_std, what + ": stddev vs the chain")
        assert_rim_intact(dbuf, dview, what)
    assert np.array_equal(host(sview)[..., 0], yuv), "source"
    assert_rim_intact(sbuf, sview, "source rim")


# ---------------------------------------------------------------------------
# 5. invalid device values: all border, nothing read; degenerate maps

@gpu
@pytest.mark.parametrize("layout", [NHWC, NCHW])
def test_index_out_of_range_is_all_border(ops, dev, oracle, layout):
    """src = the middle two frames of a four-frame allocation, so nothing here
    could leave the allocation even unguarded: a missing check would show the
    neighbours' pixels instead of the border value."""
    wo, ho, w, h = 37, 21, 46, 32
    big = make_yuv(4, w, h, 1650)
    d_big = to_dev(big, dev)
    src = d_big[1:3]
    idx = [-1, 0, 2, 1, 2 ** 30, INT32_MIN, INT32_MAX]
    # every ROI looks at the same, well-covered part of its frame
    ms = np.repeat(np.array([[1.1, 0.2, 3.0, -0.2, 1.1, 2.0]], np.float32), len(idx), 0)
    d_ms, d_idx = to_dev(ms, dev), to_dev(np.array(idx, np.int32), dev)
    n = len(idx)
    shape, strides = (((n, ho, wo, 3), (ho * wo * 3 + 7, wo * 3, 3, 1)) if layout == NHWC else
                      ((n, 3, ho, wo), (3 * ho * wo + 7, ho * wo, wo, 1)))
    bgr = decode(oracle, big[1:3], NV21_BGR)
    for mode in (CONSTANT, REPLICATE, WRAP):
        dbuf, dview = view_in_buffer(shape, strides, 4, np.float32, dev)
        got, mean, std = ops.cvt_color_warp_affine_rois_standardize(
            src, d_ms, wo, ho, src_index=d_idx, border_mode=mode, border_value=BORDER_U8, layout=layout, out=dview,
            stats=True)
        c_out, c_mean, c_std = gpu_chain(ops, src, NV21_BGR, d_ms, wo, ho, d_idx, mode, layout)
        same_bits(host(got), c_out, f"border {mode} vs the chain")
        same_bits(mean, c_mean, f"border {mode}: mean vs the chain")
        same_bits(std, c_std, f"border {mode}: stddev vs the chain")
        got, mean, std = host(got), host(mean), host(std)
        for i, k in enumerate(idx):
            what = f"layout {layout}: index {k}, border {mode}"
            if 0 <= k < 2:
                want, wmean, wstd = oracle_standardized(
                    oracle, oracle_rois(oracle, bgr, [k], ms[i:i + 1], wo, ho, BORDER3, mode), layout)
                assert wstd.all(), "a valid ROI must not look like an invalid one"
                same_bits(got[i], want[0], what)
                same_bits(mean[i], wmean[0], what + ": mean")
                same_bits(std[i], wstd[0], what + ": stddev")
            else:
                assert not got[i].view(np.int32).any(), what + ": +0.0 everywhere"
                assert mean[i].tolist() == [float(b) for b in BORDER3], what + ": the mean is the border value"
                assert not std[i].view(np.int32).any(), what + ": stddev 0"
        assert_rim_intact(dbuf, dview, f"border {mode}")
    assert np.array_equal(host(d_big), big), "source allocation"  # and the device reads back normally


@gpu
def test_degenerate_matrices(ops, dev, oracle):
    wo, ho, w, h = 37, 21, 46, 32
    big = make_yuv(4, w, h, 1660)
    d_big = to_dev(big, dev)
    src = d_big[1:3]
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
    d_ms, d_idx = to_dev(ms, dev), to_dev(np.array(idx, np.int32), dev)
    bgr = decode(oracle, big[1:3], NV21_BGR)
    for layout in (NHWC, NCHW):
        got, mean, std = ops.cvt_color_warp_affine_rois_standardize(src, d_ms, wo, ho, src_index=d_idx,
                                                                    border_value=BORDER_U8, layout=layout, stats=True)
        c_out, c_mean, c_std = gpu_chain(ops, src, NV21_BGR, d_ms, wo, ho, d_idx, CONSTANT, layout)
        same_bits(got, c_out, "vs the chain")
        same_bits(mean, c_mean, "mean vs the chain")
        same_bits(std, c_std, "stddev vs the chain")
        got, mean, std = host(got), host(mean), host(std)
        for i in (0, 1, 7):
            want, wmean, wstd = oracle_standardized(
                oracle, oracle_rois(oracle, bgr, [idx[i]], ms[i:i + 1], wo, ho, BORDER3, CONSTANT), layout)
            same_bits(got[i], want[0], f"matrix {ms[i].tolist()} vs oracle")
            same_bits(mean[i], wmean[0], f"matrix {ms[i].tolist()}: mean")
            same_bits(std[i], wstd[0], f"matrix {ms[i].tolist()}: stddev")
        assert std[7].all()
        for i in (2, 3, 4, 5, 6):  # all border under CONSTANT
            what = f"matrix {ms[i].tolist()}"
            assert not got[i].view(np.int32).any(), what + ": +0.0 everywhere"
            assert mean[i].tolist() == [float(b) for b in BORDER3] and not std[i].view(np.int32).any(), what
    assert np.array_equal(host(d_big), big), "source allocation"


# ---------------------------------------------------------------------------
# 6. / 7. more ROIs than CUs, the index contract

@gpu
def test_more_rois_than_cus(ops, dev, oracle):
    yuv = make_yuv(1, 64, 64, 1670)
    ms = random_maps(np.random.default_rng(1671), 300, 64, 64, 8, 8)
    check(ops, dev, oracle, yuv, ms, None, 8, 8, NV21_BGR, NCHW, (CONSTANT,), "300 ROIs")


@gpu
def test_null_index_broadcast_and_identity(ops, dev, oracle):
    wo, ho = 9, 6
    yuv = make_yuv(4, W, H, 1680)
    ms = random_maps(np.random.default_rng(1681), 4, W, H, wo, ho)
    check(ops, dev, oracle, yuv[:1], ms, None, wo, ho, NV12_RGB, NCHW, (CONSTANT,), "broadcast")
    check(ops, dev, oracle, yuv, ms, None, wo, ho, NV21_BGR, NHWC, (REPLICATE,), "frame i for ROI i")
    check(ops, dev, oracle, yuv[1], ms, None, wo, ho, NV21_BGR, NHWC, (CONSTANT,), "2-d frame")
    for k in (2, 3):  # any other count without an index is refused
        with pytest.raises(ValueError, match="without src_index, src must hold 1 or 4 images"):
            ops.cvt_color_warp_affine_rois_standardize(to_dev(yuv[:k], dev), to_dev(ms, dev), wo, ho)


# ---------------------------------------------------------------------------
# 8. mean_out / stddev_out NULL in turn, through the C ABI

@gpu
def test_null_statistics_arrays(ops, dev, oracle):
    import torch
    from vacv_amd import _lib
    wo, ho, n = 11, 7, 7
    yuv = make_yuv(3, W, H, 1690)
    ms = random_maps(np.random.default_rng(1691), n, W, H, wo, ho)
    d_yuv, d_ms, d_idx = to_dev(yuv, dev), to_dev(ms, dev), to_dev(np.array(IDX7, np.int32), dev)
    want, wmean, wstd = oracle_standardized(
        oracle, oracle_rois(oracle, decode(oracle, yuv, NV12_BGR), IDX7, ms, wo, ho, BORDER3, WRAP), NHWC)
    lib = _lib.load()
    stream = torch.cuda.current_stream().cuda_stream
    bv = (ctypes.c_double * 4)(*BORDER_U8)
    for give_mean, give_std in [(True, False), (False, True), (False, False), (True, True)]:
        out = torch.full((n, ho, wo, 3), -7.0, dtype=torch.float32, device=dev)
        # two neighbouring [n][3] arrays in one sentinel buffer: the one not passed keeps its bytes
        buf = torch.full((2 * n * 3 * 4,), SENTINEL, dtype=torch.uint8, device=dev)
        first, second = buf[:n * 3 * 4], buf[n * 3 * 4:]
        st = lib.vacv_cvt_color_warp_affine_rois_standardize(
            ctypes.byref(ops.describe(d_yuv.unsqueeze(-1))), ctypes.byref(ops.describe(out)), NV12_BGR,
            d_ms.data_ptr(), d_idx.data_ptr(), INTER_LINEAR, WRAP, bv, first.data_ptr() if give_mean else None,
            second.data_ptr() if give_std else None, stream)
        assert st == 0, (give_mean, give_std, st)
        what = f"mean {give_mean} stddev {give_std}"
        same_bits(out, want, what)
        if give_mean:
            same_bits(host(first).view(np.float32).reshape(n, 3), wmean, what + ": mean")
        else:
            assert (host(first) == SENTINEL).all(), what + ": the array not passed was written"
        if give_std:
            same_bits(host(second).view(np.float32).reshape(n, 3), wstd, what + ": stddev")
        else:
            assert (host(second) == SENTINEL).all(), what + ": the array not passed was written"


# ---------------------------------------------------------------------------
# 9. the arrays are read when the kernel runs

@gpu
def test_arrays_read_at_execution_time(ops, dev, oracle):
    import torch
    wo, ho = 21, 10
    yuv = make_yuv(3, W, H, 1700)
    d_yuv = to_dev(yuv, dev)
    rng = np.random.default_rng(1701)
    ms_a, ms_b = random_maps(rng, 7, W, H, wo, ho), random_maps(rng, 7, W, H, wo, ho)
    idx_a, idx_b = np.array(IDX7, np.int32), np.array(IDX7[::-1], np.int32)
    d_ms, d_idx = to_dev(ms_a, dev), to_dev(idx_a, dev)
    d_ms_b, d_idx_b = to_dev(ms_b, dev), to_dev(idx_b, dev)
    out_a = torch.empty((7, 3, ho, wo), dtype=torch.float32, device=dev)
    out_b = torch.empty_like(out_a)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        ops.cvt_color_warp_affine_rois_standardize(d_yuv, d_ms, wo, ho, src_index=d_idx, border_value=BORDER_U8,
                                                   layout=NCHW, out=out_a, stream=stream)
        d_ms.copy_(d_ms_b, non_blocking=True)      # overwritten on the stream, between the two calls,
        d_idx.copy_(d_idx_b, non_blocking=True)    # with no host synchronisation
        ops.cvt_color_warp_affine_rois_standardize(d_yuv, d_ms, wo, ho, src_index=d_idx, border_value=BORDER_U8,
                                                   layout=NCHW, out=out_b, stream=stream)
    stream.synchronize()
    bgr = decode(oracle, yuv, NV21_BGR)
    for out, ms, idx, name in ((out_a, ms_a, idx_a, "first"), (out_b, ms_b, idx_b, "second")):
        same_bits(out, oracle_standardized(oracle, oracle_rois(oracle, bgr, idx, ms, wo, ho, BORDER3, CONSTANT),
                                           NCHW)[0], name)


# ---------------------------------------------------------------------------
# 10. the Python wrapper's checks

@gpu
def test_binding_checks(ops, dev):
    import torch
    import vacv_amd as V
    frame = to_dev(make_yuv(1, 16, 16, 1), dev)
    ms = torch.tensor([[1, 0, 0, 0, 1, 0]] * 4, dtype=torch.float32, device=dev)

    def fn(m, **kw):
        return ops.cvt_color_warp_affine_rois_standardize(frame, m, 4, 4, **kw)

    with pytest.raises(ValueError, match="must live on"):
        fn(ms.cpu())                                      # a host tensor: the wrong device
    with pytest.raises(ValueError, match="ms must be torch.float32"):
        fn(ms.double())
    with pytest.raises(ValueError, match="ms must be contiguous"):
        fn(torch.zeros((8, 6), dtype=torch.float32, device=dev)[::2])
    with pytest.raises(ValueError, match=r"ms must have shape \(n, 6\) or \(n, 2, 3\)"):
        fn(ms.reshape(2, 12))
    with pytest.raises(ValueError, match="src_index must be torch.int32"):
        fn(ms, src_index=torch.zeros(4, dtype=torch.int64, device=dev))
    with pytest.raises(ValueError, match="src_index must live on"):
        fn(ms, src_index=torch.zeros(4, dtype=torch.int32))
    # an FP32 "yuv" and a multi-channel one are no YUV420sp frames
    with pytest.raises(V.VacvError) as e:
        ops.cvt_color_warp_affine_rois_standardize(frame.float(), ms, 4, 4)
    assert e.value.status == V._lib.ERR_INVALID_ARG
    with pytest.raises(ValueError, match="expected a 2-4 dimensional image tensor"):
        ops.cvt_color_warp_affine_rois_standardize(torch.zeros((1, 24, 16, 3), dtype=torch.uint8, device=dev), ms, 4, 4)
    with pytest.raises(V.VacvError) as e:  # a u8 destination
        fn(ms, out=torch.empty((4, 4, 4, 3), dtype=torch.uint8, device=dev))
    assert e.value.status == V._lib.ERR_INVALID_ARG
    unsupported(lambda: fn(ms, border_mode=5))  # TRANSPARENT
    # lists and numpy arrays are moved for convenience; (n, 2, 3) is a shape of ms too
    got, mean, std = ops.cvt_color_warp_affine_rois_standardize(frame, [[1, 0, 0, 0, 1, 0], [1, 0, -3, 0, 1, -5]], 4, 4,
                                                                src_index=[0, 0], stats=True)
    assert tuple(got.shape) == (2, 4, 4, 3) and tuple(mean.shape) == tuple(std.shape) == (2, 3)
    assert got.dtype == mean.dtype == std.dtype == torch.float32
    again = ops.cvt_color_warp_affine_rois_standardize(
        frame, np.array([[[1, 0, 0], [0, 1, 0]], [[1, 0, -3], [0, 1, -5]]], np.float32), 4, 4,
        src_index=np.zeros(2, np.int32))
    same_bits(again, got, "numpy (n, 2, 3) maps")
    from vacv_amd import cvt_color_warp_affine_rois_standardize
    assert cvt_color_warp_affine_rois_standardize is ops.cvt_color_warp_affine_rois_standardize


# ---------------------------------------------------------------------------
# 11. the C++ layer

@gpu
def test_cpp_cvt_color_warp_affine_standardize(hip_device, tmp_path):
    repo = Path(__file__).resolve().parent.parent
    pkg = repo / "arm-neon-opencv_amd"
    lib = pkg / "lib"
    exe = tmp_path / "vacv_yuv_warp_std_test"
    r = subprocess.run(["g++", "-std=c++14", "-O1", str(repo / "tests" / "cpp" / "vacv_yuv_warp_std_test.cpp"),
                        "-o", str(exe), "-I", str(pkg / "src"), "-L", str(lib), "-lvacv", "-lvacv_hip",
                        f"-Wl,-rpath,{lib}"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run(["timeout", "-k", "10", "120", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "failed 0" in r.stdout, r.stdout[-3000:]
