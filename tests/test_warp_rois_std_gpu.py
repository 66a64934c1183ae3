"""vacv_warp_affine_rois_standardize on the GPU: many affine crops in one launch,
each standardized by its own per-channel mean and standard deviation
(csrc/k_warp_rois_std.hip).

Every comparison is bit-exact, on the int32 views of the floats, so that -0.0
and +0.0 differ.  The expected value comes from two sources that must both
agree with the result:
  * the library's own chain on the GPU -- ops.warp_affine_rois (u8),
    ops.mean_stddev, ops.normalize(None, None), ops.change_layout;
  * the oracle's chain on the CPU -- warp_affine with the border mode,
    mean_stddev_exact, normalize, hwc_to_chw.
The shapes are the smallest that reach every path of the kernel: outputs of
fewer pixels than a workgroup has threads and of more, rows longer than a
workgroup, dense destinations at every 16-byte phase and pitched ones, the
largest ROIs the LDS gate admits, more ROIs than the device has CUs.
"""
from __future__ import annotations

import ctypes
import subprocess
from pathlib import Path

import numpy as np
import pytest

from test_crop_resize_rois_std_gpu import oracle_standardized, same_bits
from test_gpu_plumbing import SENTINEL, assert_rim_intact, assert_untouched, host, place, unsupported
from test_warp_rois_gpu import (BORDER_U8, IDX7, border4, make_frames, oracle_rois, random_maps, to_dev,
                                view_in_buffer)

gpu = pytest.mark.gpu
NHWC, NCHW = 1, 0
INTER_LINEAR, WARP_INVERSE_MAP = 1, 16
CONSTANT, REPLICATE, REFLECT, WRAP, REFLECT_101 = 0, 1, 2, 3, 4
BORDERS = (CONSTANT, REPLICATE, REFLECT, WRAP, REFLECT_101)
H, W = 40, 48   # frames
INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1


@pytest.fixture(scope="module")
def ops(hip_device):
    from vacv_amd import ops
    return ops


@pytest.fixture(scope="module")
def dev(hip_device):
    return hip_device


def lds_need(w, h, c):
    """include/vacv_hip.h's formula (csrc/k_warp_rois_std.hip), restated."""
    return 256 + (w * h * c + 15) // 16 * 16 + 1024 * c


def library_chain(ops, d_frames, d_ms, wo, ho, d_idx, mode, border, layout, flags=INTER_LINEAR):
    """The four existing calls whose result the one call must reproduce."""
    u = ops.warp_affine_rois(d_frames, d_ms, wo, ho, src_index=d_idx, flags=flags, border_mode=mode,
                             border_value=border)
    mean, std = ops.mean_stddev(u)
    f = ops.normalize(u, None, None)
    if layout == NCHW:
        f = ops.change_layout(f, NCHW)
    return f, mean, std


def check(ops, dev, oracle, frames, ms, idx, wo, ho, layout, modes, what, border=BORDER_U8):
    """One call against both chains, output and statistics, for each border mode."""
    c = frames.shape[3]
    d_frames = to_dev(frames, dev)
    d_ms = to_dev(np.asarray(ms, np.float32), dev)
    d_idx = to_dev(np.asarray(idx, np.int32), dev) if idx is not None else None
    n = len(ms)
    oidx = idx if idx is not None else ([0] * n if len(frames) == 1 else list(range(n)))
    for mode in modes:
        w_ = f"{what} c={c} layout {layout} {wo}x{ho} border {mode}"
        got, mean, std = ops.warp_affine_rois_standardize(d_frames, d_ms, wo, ho, src_index=d_idx, border_mode=mode,
                                                          border_value=border, layout=layout, stats=True)
        assert tuple(got.shape) == ((n, ho, wo, c) if layout == NHWC else (n, c, ho, wo))
        assert tuple(mean.shape) == tuple(std.shape) == (n, c)
        lib_out, lib_mean, lib_std = library_chain(ops, d_frames, d_ms, wo, ho, d_idx, mode, border, layout)
        same_bits(got, lib_out, w_ + " vs the library chain")
        same_bits(mean, lib_mean, w_ + ": mean vs ops.mean_stddev")
        same_bits(std, lib_std, w_ + ": stddev vs ops.mean_stddev")
        want, wmean, wstd = oracle_standardized(oracle, oracle_rois(oracle, frames, oidx, ms, wo, ho, border[:c], mode),
                                                layout)
        same_bits(got, want, w_ + " vs the oracle chain")
        same_bits(mean, wmean, w_ + ": mean vs oracle")
        same_bits(std, wstd, w_ + ": stddev vs oracle")
        # stats=False writes the same output
        same_bits(ops.warp_affine_rois_standardize(d_frames, d_ms, wo, ho, src_index=d_idx, border_mode=mode,
                                                   border_value=border, layout=layout), got, w_ + ": stats=False")
    return got, mean, std


# ---------------------------------------------------------------------------
# 1. channels x layouts x border modes, WARP_INVERSE_MAP

@gpu
@pytest.mark.parametrize("c,layout", [(1, NHWC), (1, NCHW), (2, NHWC), (3, NHWC), (3, NCHW), (4, NHWC)])
def test_matches_both_chains(ops, dev, oracle, c, layout):
    frames = make_frames(3, H, W, c, np.uint8, 600 + c)
    rng = np.random.default_rng(20261021 + c)
    for wo, ho in [(5, 3), (33, 9)]:
        check(ops, dev, oracle, frames, random_maps(rng, 7, W, H, wo, ho), IDX7, wo, ho, layout, BORDERS, "grid")


@gpu
@pytest.mark.parametrize("layout", [NHWC, NCHW])
def test_inverse_map(ops, dev, oracle, layout):
    c, wo, ho = 3, 33, 9
    frames = make_frames(3, H, W, c, np.uint8, 611)
    d_frames, d_idx = to_dev(frames, dev), to_dev(np.array(IDX7, np.int32), dev)
    ms = random_maps(np.random.default_rng(612), 7, W, H, wo, ho)
    inv = np.stack([oracle.invert_affine(m) for m in ms]).astype(np.float32)
    for mode in (CONSTANT, REFLECT_101):
        fwd = check(ops, dev, oracle, frames, ms, IDX7, wo, ho, layout, (mode,), "forward")
        back = ops.warp_affine_rois_standardize(d_frames, to_dev(inv, dev).reshape(7, 2, 3), wo, ho, src_index=d_idx,
                                                flags=INTER_LINEAR | WARP_INVERSE_MAP, border_mode=mode,
                                                border_value=BORDER_U8, layout=layout, stats=True)
        for g, f, name in zip(back, fwd, ("output", "mean", "stddev")):
            same_bits(g, f, f"inverse map, border {mode}: {name}")


# ---------------------------------------------------------------------------
# 2. output sizes that split the work differently

@gpu
@pytest.mark.parametrize("wo,ho,c,layout", [(1, 1, 3, NHWC), (1, 1, 3, NCHW), (2, 2, 3, NCHW), (7, 5, 3, NHWC),
                                             (7, 5, 4, NHWC), (1500, 2, 1, NHWC), (2, 1500, 3, NCHW),
                                             (2, 1500, 3, NHWC), (112, 112, 3, NCHW)])
def test_output_sizes(ops, dev, oracle, wo, ho, c, layout):
    h, w = 61, 83
    frames = make_frames(3, h, w, c, np.uint8, 620 + c)
    n = 7 if wo * ho < 2000 else 4
    ms = random_maps(np.random.default_rng(621 + wo), n, w, h, wo, ho)
    got, mean, std = check(ops, dev, oracle, frames, ms, IDX7[:n], wo, ho, layout,
                           (CONSTANT, REFLECT) if wo * ho > 100 else BORDERS, "sizes")
    if (wo, ho) == (1, 1):  # one pixel: the mean is the pixel, the deviation 0, the output +0.0
        assert not host(std).any() and not host(got).view(np.int32).any() and host(mean).any()


@gpu
def test_largest_three_channel_roi(ops, dev, oracle):
    """144 x 144 x 3 is exactly 64 KiB of LDS."""
    assert lds_need(144, 144, 3) == 65536
    h, w = 61, 83
    frames = make_frames(3, h, w, 3, np.uint8, 631)
    ms = random_maps(np.random.default_rng(632), 2, w, h, 144, 144)
    check(ops, dev, oracle, frames, ms, [2, 0], 144, 144, NCHW, (CONSTANT, WRAP), "64 KiB")


@gpu
def test_largest_roi_all_255(ops, dev):
    """250 x 257 x 1 is the tallest 250-wide ROI the LDS gate admits: 64,250
    pixels of 255 sum to 64,250 * 65,025 = 4,177,856,250 squares, past 2^31.
    The statistics are exactly (255, 0) and every output is +0.0."""
    wo, ho = 250, 257
    assert lds_need(wo, ho, 1) <= 65536 < lds_need(wo, ho + 1, 1)
    assert 2 ** 31 < wo * ho * 255 * 255 == 4177856250 < 2 ** 32
    d_frame = to_dev(np.full((1, H, W, 1), 255, np.uint8), dev)
    # identity-like: REPLICATE continues the frame's 255 over the rest of the ROI
    d_ms = to_dev(np.array([[1, 0, 0, 0, 1, 0], [1.25, 0.1, 3.5, -0.1, 0.9, 2.25]], np.float32), dev)
    got, mean, std = ops.warp_affine_rois_standardize(d_frame, d_ms, wo, ho, border_mode=REPLICATE,
                                                      border_value=BORDER_U8, stats=True)
    assert host(mean).tolist() == [[255.0]] * 2 and host(std).tolist() == [[0.0]] * 2
    same_bits(got, np.zeros((2, ho, wo, 1), np.float32), "all-255 frame")
    lib_out, lib_mean, lib_std = library_chain(ops, d_frame, d_ms, wo, ho, None, REPLICATE, BORDER_U8, NHWC)
    same_bits(got, lib_out, "vs the library chain")
    same_bits(mean, lib_mean, "mean")
    same_bits(std, lib_std, "stddev")
    # one row more is refused with nothing written
    buf, out = place(np.zeros((2, ho + 1, wo, 1), np.float32), dev)
    buf.fill_(SENTINEL)
    unsupported(lambda: ops.warp_affine_rois_standardize(d_frame, d_ms, wo, ho + 1, border_mode=REPLICATE, out=out))
    assert_untouched(buf, "past the LDS limit")


# ---------------------------------------------------------------------------
# 3. border pixels are part of the ROI's statistics; deviations of exactly 0

@gpu
@pytest.mark.parametrize("layout", [NHWC, NCHW])
def test_border_counts_in_the_statistics(ops, dev, oracle, layout):
    c, wo, ho = 3, 24, 10
    border = (17, 200, 255, 0)
    frames = make_frames(1, H, W, c, np.uint8, 641)
    half = np.array([[1, 0, 12, 0, 1, -5]], np.float32)  # dst x = src x + 12: the left half of the ROI is off the frame
    roi = oracle_rois(oracle, frames, [0], half, wo, ho, border[:c], CONSTANT)[0]
    assert (roi[:, :11] == np.array(border[:c], np.uint8)).all() and not (roi[:, 12:] == border[:c]).all()
    whole_mean, _ = oracle.mean_stddev_exact(roi)
    inside_mean, _ = oracle.mean_stddev_exact(np.ascontiguousarray(roi[:, 12:]))
    assert (np.asarray(whole_mean) != np.asarray(inside_mean)).all(), "the border must move the mean"
    got, mean, std = check(ops, dev, oracle, frames, half, None, wo, ho, layout, (CONSTANT,), "half off", border)
    same_bits(mean, np.asarray(whole_mean, np.float32).reshape(1, c), "the mean spans the border pixels")
    # wholly off the frame: the ROI is border_value
    off = np.array([[1, 0, 1000, 0, 1, 1000], [0.5, 0.1, -900, 0, 2, 40]], np.float32)
    got, mean, std = check(ops, dev, oracle, frames, off, None, wo, ho, layout, (CONSTANT,), "all off", border)
    assert host(mean).tolist() == [[17.0, 200.0, 255.0]] * 2 and not host(std).view(np.int32).any()
    assert not host(got).view(np.int32).any(), "a ROI of border_value is +0.0 everywhere"


@gpu
@pytest.mark.parametrize("layout", [NHWC, NCHW])
def test_constant_region_in_a_varying_frame(ops, dev, oracle, layout):
    c = 3
    frames = make_frames(1, H, W, c, np.uint8, 651)
    frames[0, 10:24, 12:30] = (17, 200, 255)       # constant per channel
    frames[0, 26:38, 4:20] = (9, 9, 9)
    frames[0, 30, 11] = (200, 9, 255)               # one differing pixel, in two of the channels
    # whole-pixel shifts whose taps stay inside the regions, and a map across both
    ms = np.array([[1, 0, -12, 0, 1, -10], [1, 0, -4, 0, 1, -26], [0.9, 0.2, -3, -0.2, 0.9, 1]], np.float32)
    got, mean, std = check(ops, dev, oracle, frames, ms, None, 15, 11, layout, (CONSTANT, REFLECT_101), "constant")
    assert host(mean)[0].tolist() == [17.0, 200.0, 255.0] and host(std)[0].tolist() == [0.0, 0.0, 0.0]
    assert not host(got)[0].view(np.int32).any(), "a constant ROI is +0.0 everywhere"
    assert host(std)[1, 1] == 0.0 and host(std)[1, 0] > 0 and host(std)[1, 2] > 0
    assert host(std)[2].all()


# ---------------------------------------------------------------------------
# 4. pitched, misaligned shapes

PITCH_CASES = [
    # c, layout, src off, dst off, pitched dst (row + 5, plane + 9, batch + 11 floats)
    (3, NHWC, 1, 4, True), (3, NCHW, 3, 8, True), (3, NCHW, 5, 16, True), (1, NHWC, 1, 12, True),
    (1, NCHW, 3, 4, True), (2, NHWC, 5, 4, True), (4, NHWC, 3, 20, True),
] + [(3, NHWC, 1, off, False) for off in (0, 4, 8, 12)] + [(3, NCHW, 3, off, False) for off in (0, 4, 8, 12)] + [
    (1, NHWC, 5, 4, False), (2, NHWC, 1, 8, False), (4, NHWC, 5, 12, False),
]


@gpu
@pytest.mark.parametrize("case", PITCH_CASES,
                         ids=lambda t: f"c{t[0]}-{'nchw' if t[1] == NCHW else 'nhwc'}-s{t[2]}-d{t[3]}-"
                                       f"{'pitched' if t[4] else 'dense'}")
def test_pitched_misaligned(ops, dev, oracle, case):
    """src: base off by 1, 3, 5 bytes, rows 7 and frames 13 bytes further
    apart.  dst: dense at every 4-byte alignment class modulo 16, or pitched
    (row + 5, plane + 9, batch + 11 floats); the padding keeps its sentinel."""
    c, layout, soff, doff, pitched = case
    frames = make_frames(3, H, W, c, np.uint8, 660 + c)
    sbuf, sview = place(frames, dev, NHWC, off=soff, row_pad=7, batch_pad=13)
    d_idx = to_dev(np.array(IDX7, np.int32), dev)
    n = 7
    rng = np.random.default_rng(661 + soff)
    rpad, ppad, bpad = (5, 9, 11) if pitched else (0, 0, 0)
    for (wo, ho), mode in [((33, 9), REFLECT), ((5, 3), CONSTANT)]:
        ms = random_maps(rng, n, W, H, wo, ho)
        if layout == NCHW:
            rp = wo + rpad
            pl = ho * rp + ppad
            dbuf, dview = view_in_buffer((n, c, ho, wo), (c * pl + bpad, pl, rp, 1), doff, np.float32, dev)
        else:
            rp = wo * c + rpad
            dbuf, dview = view_in_buffer((n, ho, wo, c), (ho * rp + bpad, rp, c, 1), doff, np.float32, dev)
        what = f"{case} {wo}x{ho}"
        got, mean, std = ops.warp_affine_rois_standardize(sview, to_dev(ms, dev), wo, ho, src_index=d_idx,
                                                          border_mode=mode, border_value=BORDER_U8, layout=layout,
                                                          out=dview, stats=True)
        assert got.data_ptr() == dview.data_ptr()
        lib_out, lib_mean, lib_std = library_chain(ops, sview, to_dev(ms, dev), wo, ho, d_idx, mode, BORDER_U8, layout)
        want, wmean, wstd = oracle_standardized(oracle, oracle_rois(oracle, frames, IDX7, ms, wo, ho, BORDER_U8[:c],
                                                                    mode), layout)
        same_bits(host(dview), want, what)
        same_bits(host(dview), lib_out, what + " vs the library chain")
        same_bits(mean, wmean, what + ": mean")
        same_bits(mean, lib_mean, what + ": mean vs the library chain")
        same_bits(std, wstd, what + ": stddev")
        same_bits(std, lib_std, what + ": stddev vs the library chain")
        assert_rim_intact(dbuf, dview, what)
        assert np.array_equal(host(sview), frames), what + ": source"
        assert_rim_intact(sbuf, sview, what + ": source padding")


# ---------------------------------------------------------------------------
# 5. invalid device values: all border, nothing read; degenerate maps

@gpu
@pytest.mark.parametrize("layout", [NHWC, NCHW])
def test_index_out_of_range_is_all_border(ops, dev, oracle, layout):
    """src = the middle two frames of a four-frame allocation, so nothing here
    could leave the allocation even unguarded: a missing check would show the
    neighbours' pixels instead of the border value."""
    c, wo, ho = 3, 37, 21
    big = make_frames(4, 33, 47, c, np.uint8, 17)
    d_big = to_dev(big, dev)
    src = d_big[1:3]
    idx = [-1, 0, 2, 1, INT32_MIN, INT32_MAX]
    # every ROI looks at the same, well-covered part of its frame
    ms = np.repeat(np.array([[1.1, 0.2, 3.0, -0.2, 1.1, 2.0]], np.float32), len(idx), 0)
    d_ms, d_idx = to_dev(ms, dev), to_dev(np.array(idx, np.int32), dev)
    shape, strides = (((6, ho, wo, c), (ho * wo * c + 7, wo * c, c, 1)) if layout == NHWC else
                      ((6, c, ho, wo), (c * ho * wo + 7, ho * wo, wo, 1)))
    for mode in (CONSTANT, REPLICATE, WRAP):
        dbuf, dview = view_in_buffer(shape, strides, 4, np.float32, dev)
        got, mean, std = ops.warp_affine_rois_standardize(src, d_ms, wo, ho, src_index=d_idx, border_mode=mode,
                                                          border_value=BORDER_U8, layout=layout, out=dview, stats=True)
        lib_out, lib_mean, lib_std = library_chain(ops, src, d_ms, wo, ho, d_idx, mode, BORDER_U8, layout)
        same_bits(host(got), lib_out, f"border {mode} vs the library chain")
        same_bits(mean, lib_mean, f"border {mode}: mean vs the library chain")
        same_bits(std, lib_std, f"border {mode}: stddev vs the library chain")
        got, mean, std = host(got), host(mean), host(std)
        for i, k in enumerate(idx):
            what = f"layout {layout}: index {k}, border {mode}"
            if 0 <= k < 2:
                want, wmean, wstd = oracle_standardized(
                    oracle, oracle_rois(oracle, big[1:3], [k], ms[i:i + 1], wo, ho, BORDER_U8[:c], mode), layout)
                assert wstd.all(), "a valid ROI must not look like an invalid one"
                same_bits(got[i], want[0], what)
                same_bits(mean[i], wmean[0], what + ": mean")
                same_bits(std[i], wstd[0], what + ": stddev")
            else:
                assert not got[i].view(np.int32).any(), what + ": +0.0 everywhere"
                assert mean[i].tolist() == [float(b) for b in BORDER_U8[:c]], what + ": the mean is the border value"
                assert not std[i].view(np.int32).any(), what + ": stddev 0"
        assert_rim_intact(dbuf, dview, f"border {mode}")
    assert np.array_equal(host(d_big), big), "source allocation"


@gpu
def test_degenerate_matrices(ops, dev, oracle):
    c, wo, ho = 3, 37, 21
    big = make_frames(4, 33, 47, c, np.uint8, 19)
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
    for layout in (NHWC, NCHW):
        got, mean, std = ops.warp_affine_rois_standardize(src, d_ms, wo, ho, src_index=d_idx, border_value=BORDER_U8,
                                                          layout=layout, stats=True)
        lib_out, lib_mean, lib_std = library_chain(ops, src, d_ms, wo, ho, d_idx, CONSTANT, BORDER_U8, layout)
        same_bits(got, lib_out, "vs the library chain")
        same_bits(mean, lib_mean, "mean vs the library chain")
        same_bits(std, lib_std, "stddev vs the library chain")
        got, mean, std = host(got), host(mean), host(std)
        for i in (0, 1, 7):
            want, wmean, wstd = oracle_standardized(
                oracle, oracle_rois(oracle, big[1:3], [idx[i]], ms[i:i + 1], wo, ho, BORDER_U8[:c], CONSTANT), layout)
            same_bits(got[i], want[0], f"matrix {ms[i].tolist()} vs oracle")
            same_bits(mean[i], wmean[0], f"matrix {ms[i].tolist()}: mean")
            same_bits(std[i], wstd[0], f"matrix {ms[i].tolist()}: stddev")
        assert std[7].all()
        for i in (2, 3, 4, 5, 6):  # all border under CONSTANT
            what = f"matrix {ms[i].tolist()}"
            assert not got[i].view(np.int32).any(), what + ": +0.0 everywhere"
            assert mean[i].tolist() == [float(b) for b in BORDER_U8[:c]] and not std[i].view(np.int32).any(), what
    assert np.array_equal(host(d_big), big), "source allocation"


# ---------------------------------------------------------------------------
# 6. / 7. the index contract, more ROIs than CUs

@gpu
def test_null_index_broadcast_and_identity(ops, dev, oracle):
    c, wo, ho = 3, 9, 6
    frames = make_frames(4, H, W, c, np.uint8, 671)
    ms = random_maps(np.random.default_rng(672), 4, W, H, wo, ho)
    check(ops, dev, oracle, frames[:1], ms, None, wo, ho, NCHW, (CONSTANT,), "broadcast")
    check(ops, dev, oracle, frames, ms, None, wo, ho, NHWC, (REPLICATE,), "frame i for ROI i")
    got = ops.warp_affine_rois_standardize(to_dev(frames[1], dev), to_dev(ms, dev), wo, ho,
                                           border_value=BORDER_U8)  # an (h, w, c) frame
    want, _, _ = oracle_standardized(oracle, oracle_rois(oracle, frames, [1] * 4, ms, wo, ho, BORDER_U8[:c], CONSTANT),
                                     NHWC)
    same_bits(got, want, "3-d frame")
    with pytest.raises(ValueError):  # any other count without an index is refused
        ops.warp_affine_rois_standardize(to_dev(frames[:2], dev), to_dev(ms, dev), wo, ho)


@gpu
def test_more_rois_than_cus(ops, dev, oracle):
    frame = make_frames(1, H, W, 3, np.uint8, 681)
    ms = random_maps(np.random.default_rng(682), 300, W, H, 4, 4)
    check(ops, dev, oracle, frame, ms, None, 4, 4, NCHW, (CONSTANT,), "300 ROIs")


# ---------------------------------------------------------------------------
# 8. mean_out / stddev_out NULL in turn, through the C ABI

@gpu
def test_null_statistics_arrays(ops, dev, oracle):
    import torch
    from vacv_amd import _lib
    c, wo, ho, n = 3, 11, 7, 7
    frames = make_frames(3, H, W, c, np.uint8, 691)
    ms = random_maps(np.random.default_rng(692), n, W, H, wo, ho)
    d_frames, d_ms, d_idx = to_dev(frames, dev), to_dev(ms, dev), to_dev(np.array(IDX7, np.int32), dev)
    want, wmean, wstd = oracle_standardized(oracle, oracle_rois(oracle, frames, IDX7, ms, wo, ho, BORDER_U8[:c], WRAP),
                                            NHWC)
    lib = _lib.load()
    stream = torch.cuda.current_stream().cuda_stream
    bv = (ctypes.c_double * 4)(*BORDER_U8)
    for give_mean, give_std in [(True, False), (False, True), (False, False), (True, True)]:
        out = torch.full((n, ho, wo, c), -7.0, dtype=torch.float32, device=dev)
        # two neighbouring [n][c] arrays in one sentinel buffer: the one not passed keeps its bytes
        buf = torch.full((2 * n * c * 4,), SENTINEL, dtype=torch.uint8, device=dev)
        first, second = buf[:n * c * 4], buf[n * c * 4:]
        st = lib.vacv_warp_affine_rois_standardize(
            ctypes.byref(ops.describe(d_frames)), ctypes.byref(ops.describe(out)), d_ms.data_ptr(),
            d_idx.data_ptr(), INTER_LINEAR, WRAP, bv, first.data_ptr() if give_mean else None,
            second.data_ptr() if give_std else None, stream)
        assert st == 0, (give_mean, give_std, st)
        what = f"mean {give_mean} stddev {give_std}"
        same_bits(out, want, what)
        if give_mean:
            same_bits(host(first).view(np.float32).reshape(n, c), wmean, what + ": mean")
        else:
            assert (host(first) == SENTINEL).all(), what + ": the array not passed was written"
        if give_std:
            same_bits(host(second).view(np.float32).reshape(n, c), wstd, what + ": stddev")
        else:
            assert (host(second) == SENTINEL).all(), what + ": the array not passed was written"


# ---------------------------------------------------------------------------
# 9. the arrays are read when the kernel runs

@gpu
def test_arrays_read_at_execution_time(ops, dev, oracle):
    import torch
    c, wo, ho = 3, 21, 10
    frames = make_frames(3, H, W, c, np.uint8, 701)
    d_frames = to_dev(frames, dev)
    rng = np.random.default_rng(702)
    ms_a, ms_b = random_maps(rng, 7, W, H, wo, ho), random_maps(rng, 7, W, H, wo, ho)
    idx_a, idx_b = np.array(IDX7, np.int32), np.array(IDX7[::-1], np.int32)
    d_ms, d_idx = to_dev(ms_a, dev), to_dev(idx_a, dev)
    d_ms_b, d_idx_b = to_dev(ms_b, dev), to_dev(idx_b, dev)
    out_a = torch.empty((7, c, ho, wo), dtype=torch.float32, device=dev)
    out_b = torch.empty_like(out_a)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        ops.warp_affine_rois_standardize(d_frames, d_ms, wo, ho, src_index=d_idx, border_value=BORDER_U8, layout=NCHW,
                                         out=out_a, stream=stream)
        d_ms.copy_(d_ms_b, non_blocking=True)      # overwritten on the stream, between the two calls,
        d_idx.copy_(d_idx_b, non_blocking=True)    # with no host synchronisation
        ops.warp_affine_rois_standardize(d_frames, d_ms, wo, ho, src_index=d_idx, border_value=BORDER_U8, layout=NCHW,
                                         out=out_b, stream=stream)
    stream.synchronize()
    for out, ms, idx, name in ((out_a, ms_a, idx_a, "first"), (out_b, ms_b, idx_b, "second")):
        same_bits(out, oracle_standardized(oracle, oracle_rois(oracle, frames, idx, ms, wo, ho, BORDER_U8[:c], CONSTANT),
                                           NCHW)[0], name)


# ---------------------------------------------------------------------------
# 10. the Python wrapper's checks

@gpu
def test_binding_checks(ops, dev):
    import torch
    frame = to_dev(make_frames(1, 16, 16, 3, np.uint8, 1), dev)
    ms = torch.tensor([[1, 0, 0, 0, 1, 0]] * 4, dtype=torch.float32, device=dev)

    def fn(m, **kw):
        return ops.warp_affine_rois_standardize(frame, m, 4, 4, **kw)

    with pytest.raises(ValueError, match="must live on"):
        fn(ms.cpu())                                      # a host tensor: the wrong device
    with pytest.raises(ValueError, match="ms must be torch.float32"):
        fn(ms.double())
    with pytest.raises(ValueError, match="ms must be torch.float32"):
        fn(ms.int())
    with pytest.raises(ValueError, match="ms must be contiguous"):
        fn(torch.zeros((8, 6), dtype=torch.float32, device=dev)[::2])
    with pytest.raises(ValueError, match=r"ms must have shape \(n, 6\) or \(n, 2, 3\)"):
        fn(ms.reshape(2, 12))
    with pytest.raises(ValueError, match="ms holds no matrix"):
        fn(ms[:0])
    with pytest.raises(ValueError, match="src_index must be torch.int32"):
        fn(ms, src_index=torch.zeros(4, dtype=torch.int64, device=dev))
    with pytest.raises(ValueError, match="src_index must live on"):
        fn(ms, src_index=torch.zeros(4, dtype=torch.int32))
    with pytest.raises(ValueError, match=r"src_index must have shape \(4,\)"):
        fn(ms, src_index=torch.zeros(3, dtype=torch.int32, device=dev))
    with pytest.raises(ValueError, match="takes uint8 frames"):
        ops.warp_affine_rois_standardize(frame.float(), ms, 4, 4)
    # two or four channels have no planar output; a u8 destination is refused
    for c in (2, 4):
        unsupported(lambda: ops.warp_affine_rois_standardize(to_dev(make_frames(1, 16, 16, c, np.uint8, 2), dev),
                                                             ms, 4, 4, layout=NCHW))
    import vacv_amd as V
    with pytest.raises(V.VacvError) as e:
        fn(ms, out=torch.empty((4, 4, 4, 3), dtype=torch.uint8, device=dev))
    assert e.value.status == V._lib.ERR_INVALID_ARG
    # lists and numpy arrays are moved for convenience; (n, 2, 3) is a shape of ms too
    got, mean, std = ops.warp_affine_rois_standardize(frame, [[1, 0, 0, 0, 1, 0], [1, 0, -3, 0, 1, -5]], 4, 4,
                                                      src_index=[0, 0], stats=True)
    assert tuple(got.shape) == (2, 4, 4, 3) and tuple(mean.shape) == tuple(std.shape) == (2, 3)
    again = ops.warp_affine_rois_standardize(frame, np.array([[[1, 0, 0], [0, 1, 0]], [[1, 0, -3], [0, 1, -5]]],
                                                             np.float32), 4, 4, src_index=np.zeros(2, np.int32))
    same_bits(again, got, "numpy (n, 2, 3) maps")
    from vacv_amd import warp_affine_rois_standardize
    assert warp_affine_rois_standardize is ops.warp_affine_rois_standardize


# ---------------------------------------------------------------------------
# 11. the C++ layer

@gpu
def test_cpp_warp_affine_standardize(hip_device, tmp_path):
    repo = Path(__file__).resolve().parent.parent
    pkg = repo / "arm-neon-opencv_amd"
    lib = pkg / "lib"
    exe = tmp_path / "vacv_warp_std_test"
    r = subprocess.run(["g++", "-std=c++14", "-O1", str(repo / "tests" / "cpp" / "vacv_warp_std_test.cpp"),
                        "-o", str(exe), "-I", str(pkg / "src"), "-L", str(lib), "-lvacv", "-lvacv_hip",
                        f"-Wl,-rpath,{lib}"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run(["timeout", "-k", "10", "120", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "failed 0" in r.stdout, r.stdout[-3000:]
