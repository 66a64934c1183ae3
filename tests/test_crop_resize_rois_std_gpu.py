"""vacv_crop_resize_rois_standardize on the GPU: many upright crops in one
launch, each standardized by its own per-channel mean and standard deviation
(csrc/k_crop_resize_rois_std.hip).

Every comparison is bit-exact, on the int32 views of the floats, so that -0.0
and +0.0 differ.  The expected value comes from two sources that must both
agree with the result:
  * the library's own chain on the GPU -- ops.crop_resize_rois (u8),
    ops.mean_stddev, ops.normalize(None, None), ops.change_layout;
  * the oracle's chain on the CPU -- crop, resize_linear, mean_stddev_exact,
    normalize, hwc_to_chw.
The shapes are the smallest that reach every path of the kernel: outputs of
fewer pixels than a workgroup has threads and of more, rows longer than a
workgroup, dense destinations at every 16-byte phase and pitched ones, the
largest ROI the LDS gate admits, more ROIs than the device has CUs.
"""
from __future__ import annotations

import ctypes
import subprocess
from pathlib import Path

import numpy as np
import pytest

from test_crop_resize_rois_gpu import make_frames, oracle_rois, to_dev, view_in_buffer
from test_gpu_plumbing import SENTINEL, assert_rim_intact, assert_untouched, host, place, unsupported

gpu = pytest.mark.gpu
NHWC, NCHW = 1, 0
REFERENCE, NEON, OPENCV = 0, 1, 2
MODES = (REFERENCE, NEON, OPENCV)
H, W = 40, 48   # frames
INT32_MAX = 2 ** 31 - 1

# (left, top, width, height) in a 48 x 40 frame
RECTS = np.array([
    [0, 0, W, H],            # the whole frame: every edge
    [0, 0, 2, 2],            # the smallest rect, top-left corner
    [W - 2, H - 2, 2, 2],    # ... bottom-right corner
    [30, 9, 18, 20],         # touches the right edge only
    [10, 25, 30, 15],        # touches the bottom edge only
    [0, 11, 7, 9],           # the left edge
    [13, 0, 9, 5],           # the top edge
    [20, 11, 5, 3],          # up-scale (the output's own size for 5 x 3)
    [3, 2, 44, 36],          # down-scale
    [7, 5, 33, 9],           # the output's own size for 33 x 9
    [31, 2, 3, 37],          # extreme aspect
    [17, 9, 31, 23],         # primes
], np.int32)
IDX = np.array([2, 0, 0, 1, 2, 2, 1, 0, 1, 2, 0, 1], np.int32)  # mixed and repeated


@pytest.fixture(scope="module")
def ops(hip_device):
    from vacv_amd import ops
    return ops


@pytest.fixture(scope="module")
def dev(hip_device):
    return hip_device


def lds_need(w, h, c):
    """include/vacv_hip.h's formula (csrc/k_crop_resize_rois_std.hip), restated."""
    return 256 + (w * h * c + 15) // 16 * 16 + max(8 * (w + h), 1024 * c)


def same_bits(got, want, what):
    """torch.equal on the int32 views: -0.0 is not +0.0."""
    import torch
    g = got.detach().cpu().contiguous() if isinstance(got, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(got))
    w = want.detach().cpu().contiguous() if isinstance(want, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(want))
    assert g.shape == w.shape and g.dtype == w.dtype == torch.float32, (what, g.shape, w.shape, g.dtype, w.dtype)
    gi, wi = g.view(torch.int32), w.view(torch.int32)
    assert torch.equal(gi, wi), f"{what}: {int((gi != wi).sum())} of {gi.numel()} floats differ"


def oracle_standardized(oracle, rois, layout):
    """(out, mean, std) of [n, ho, wo, c] u8 ROIs: each by its own exact statistics."""
    outs, means, stds = [], [], []
    for r in rois:
        c = r.shape[2]
        f = r if c > 1 else r[..., 0]
        m, s = oracle.mean_stddev_exact(f)
        o = oracle.normalize(oracle.u8_to_f32(f), m, s).reshape(r.shape)
        outs.append(oracle.hwc_to_chw(o) if layout == NCHW else o)
        means.append(np.asarray(m, np.float32).reshape(c))
        stds.append(np.asarray(s, np.float32).reshape(c))
    return np.stack(outs), np.stack(means), np.stack(stds)


def library_chain(ops, d_frames, d_rects, wo, ho, d_idx, mode, layout):
    """The four existing calls whose result the one call must reproduce."""
    u = ops.crop_resize_rois(d_frames, d_rects, wo, ho, src_index=d_idx, mode=mode)
    mean, std = ops.mean_stddev(u)
    f = ops.normalize(u, None, None)
    if layout == NCHW:
        f = ops.change_layout(f, NCHW)
    return f, mean, std


def check(ops, dev, oracle, frames, rects, idx, wo, ho, c, layout, modes, what, d_frames=None):
    """One call against both chains, output and statistics, for each mode."""
    d_frames = to_dev(frames, dev) if d_frames is None else d_frames
    d_rects = to_dev(np.asarray(rects, np.int32), dev)
    d_idx = to_dev(np.asarray(idx, np.int32), dev) if idx is not None else None
    n = len(rects)
    oidx = idx if idx is not None else ([0] * n if len(frames) == 1 else list(range(n)))
    for mode in modes:
        w_ = f"{what} c={c} layout {layout} {wo}x{ho} mode {mode}"
        got, mean, std = ops.crop_resize_rois_standardize(d_frames, d_rects, wo, ho, src_index=d_idx, mode=mode,
                                                          layout=layout, stats=True)
        assert tuple(got.shape) == ((n, ho, wo, c) if layout == NHWC else (n, c, ho, wo))
        assert tuple(mean.shape) == tuple(std.shape) == (n, c)
        lib_out, lib_mean, lib_std = library_chain(ops, d_frames, d_rects, wo, ho, d_idx, mode, layout)
        same_bits(got, lib_out, w_ + " vs the library chain")
        same_bits(mean, lib_mean, w_ + ": mean vs ops.mean_stddev")
        same_bits(std, lib_std, w_ + ": stddev vs ops.mean_stddev")
        want, wmean, wstd = oracle_standardized(oracle, oracle_rois(oracle, frames, oidx, rects, wo, ho, mode), layout)
        same_bits(got, want, w_ + " vs the oracle chain")
        same_bits(mean, wmean, w_ + ": mean vs oracle")
        same_bits(std, wstd, w_ + ": stddev vs oracle")
        # stats=False writes the same output
        same_bits(ops.crop_resize_rois_standardize(d_frames, d_rects, wo, ho, src_index=d_idx, mode=mode,
                                                   layout=layout), got, w_ + ": stats=False")


# ---------------------------------------------------------------------------
# 1. channels x layouts x modes

@gpu
@pytest.mark.parametrize("c,layout", [(1, NHWC), (1, NCHW), (2, NHWC), (3, NHWC), (3, NCHW), (4, NHWC)])
def test_matches_both_chains(ops, dev, oracle, c, layout):
    frames = make_frames(3, H, W, c, np.uint8, 500 + c)
    for wo, ho in [(5, 3), (33, 9)]:
        check(ops, dev, oracle, frames, RECTS, IDX, wo, ho, c, layout, MODES, "grid")


# ---------------------------------------------------------------------------
# 2. output sizes that stress the split of the work

@gpu
@pytest.mark.parametrize("wo,ho,c,layout", [(1, 1, 3, NHWC), (1, 1, 3, NCHW), (2, 2, 3, NCHW), (7, 5, 3, NHWC),
                                             (7, 5, 4, NHWC), (1500, 2, 1, NHWC), (2, 1500, 3, NCHW),
                                             (2, 1500, 3, NHWC), (112, 112, 3, NCHW)])
def test_output_sizes(ops, dev, oracle, wo, ho, c, layout):
    frames = make_frames(3, H, W, c, np.uint8, 520 + c)
    rects, idx = (RECTS, IDX) if wo * ho < 2000 else (RECTS[[0, 3, 7, 11]], IDX[[0, 3, 7, 11]])
    check(ops, dev, oracle, frames, rects, idx, wo, ho, c, layout, (REFERENCE,) if wo * ho > 100 else MODES, "sizes")
    if (wo, ho) == (1, 1):  # one pixel: the mean is the pixel, the deviation 0, the output +0.0
        got, mean, std = ops.crop_resize_rois_standardize(to_dev(frames, dev), to_dev(RECTS, dev), 1, 1,
                                                          src_index=to_dev(IDX, dev), layout=layout, stats=True)
        assert not host(std).any() and not host(got).view(np.int32).any() and host(mean).any()


# ---------------------------------------------------------------------------
# 3. the largest ROI of one channel: the sums at their bound

@gpu
@pytest.mark.parametrize("value", [255, 0])
def test_largest_roi_constant_frame(ops, dev, value):
    """250 x 245 x 1 is the tallest 250-wide ROI the LDS gate admits: 61,250
    pixels of 255 sum to 61,250 * 65,025 = 3,982,781,250 squares, past 2^31.
    The statistics are exactly (value, 0) and every output is +0.0."""
    wo, ho = 250, 245
    assert lds_need(wo, ho, 1) <= 65536 < lds_need(wo, ho + 1, 1)
    frame = np.full((1, H, W, 1), value, np.uint8)
    d_rects = to_dev(np.array([[0, 0, W, H], [5, 3, 20, 30]], np.int32), dev)
    got, mean, std = ops.crop_resize_rois_standardize(to_dev(frame, dev), d_rects, wo, ho, stats=True)
    assert host(mean).tolist() == [[float(value)]] * 2 and host(std).tolist() == [[0.0]] * 2
    same_bits(got, np.zeros((2, ho, wo, 1), np.float32), f"all-{value} frame")
    lib_out, lib_mean, lib_std = library_chain(ops, to_dev(frame, dev), d_rects, wo, ho, None, REFERENCE, NHWC)
    same_bits(got, lib_out, "vs the library chain")
    same_bits(mean, lib_mean, "mean")
    same_bits(std, lib_std, "stddev")
    # one row more is refused with nothing written
    buf, out = place(np.zeros((2, ho + 1, wo, 1), np.float32), dev)
    buf.fill_(SENTINEL)
    unsupported(lambda: ops.crop_resize_rois_standardize(to_dev(frame, dev), d_rects, wo, ho + 1, out=out))
    assert_untouched(buf, "past the LDS limit")


@gpu
def test_largest_three_channel_roi(ops, dev, oracle):
    """144 x 144 x 3 is exactly 64 KiB of LDS."""
    assert lds_need(144, 144, 3) == 65536
    frames = make_frames(3, H, W, 3, np.uint8, 531)
    check(ops, dev, oracle, frames, RECTS[[0, 8]], IDX[[3, 5]], 144, 144, 3, NCHW, (REFERENCE,), "64 KiB")


# ---------------------------------------------------------------------------
# 4. a deviation of exactly 0 inside a varying frame, and one differing pixel

@gpu
@pytest.mark.parametrize("layout", [NHWC, NCHW])
def test_constant_roi_and_one_pixel(ops, dev, oracle, layout):
    c = 3
    frames = make_frames(1, H, W, c, np.uint8, 541)
    frames[0, 10:24, 12:30] = (17, 200, 255)       # constant per channel
    frames[0, 26:38, 4:20] = (9, 9, 9)
    frames[0, 30, 11] = (200, 9, 255)               # one differing pixel, in two of the channels
    rects = np.array([[12, 10, 18, 14], [4, 26, 16, 12], [11, 9, 20, 16]], np.int32)
    for wo, ho in [(18, 14), (23, 11)]:
        check(ops, dev, oracle, frames, rects, None, wo, ho, c, layout, MODES, "constant")
    got, mean, std = ops.crop_resize_rois_standardize(to_dev(frames, dev), to_dev(rects, dev), 23, 11, layout=layout,
                                                      stats=True)
    assert host(mean)[0].tolist() == [17.0, 200.0, 255.0] and host(std)[0].tolist() == [0.0, 0.0, 0.0]
    assert not host(got)[0].view(np.int32).any(), "a constant ROI is +0.0 everywhere"
    assert host(std)[1, 1] == 0.0 and host(std)[1, 0] > 0 and host(std)[1, 2] > 0


# ---------------------------------------------------------------------------
# 5. pitched, misaligned shapes

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
    frames = make_frames(3, H, W, c, np.uint8, 550 + c)
    sbuf, sview = place(frames, dev, NHWC, off=soff, row_pad=7, batch_pad=13)
    d_rects, d_idx = to_dev(RECTS, dev), to_dev(IDX, dev)
    n = len(RECTS)
    rpad, ppad, bpad = (5, 9, 11) if pitched else (0, 0, 0)
    for wo, ho in [(33, 9), (5, 3)]:
        if layout == NCHW:
            rp = wo + rpad
            pl = ho * rp + ppad
            dbuf, dview = view_in_buffer((n, c, ho, wo), (c * pl + bpad, pl, rp, 1), doff, np.float32, dev)
        else:
            rp = wo * c + rpad
            dbuf, dview = view_in_buffer((n, ho, wo, c), (ho * rp + bpad, rp, c, 1), doff, np.float32, dev)
        what = f"{case} {wo}x{ho}"
        got, mean, std = ops.crop_resize_rois_standardize(sview, d_rects, wo, ho, src_index=d_idx, layout=layout,
                                                          out=dview, stats=True)
        assert got.data_ptr() == dview.data_ptr()
        want, wmean, wstd = oracle_standardized(oracle, oracle_rois(oracle, frames, IDX, RECTS, wo, ho), layout)
        same_bits(host(dview), want, what)
        same_bits(mean, wmean, what + ": mean")
        same_bits(std, wstd, what + ": stddev")
        assert_rim_intact(dbuf, dview, what)
        assert np.array_equal(host(sview), frames), what + ": source"


# ---------------------------------------------------------------------------
# 6. invalid device values: range checks, zeros, nothing read

@gpu
@pytest.mark.parametrize("layout", [NHWC, NCHW])
def test_invalid_rects_and_indices_give_zeros(ops, dev, oracle, layout):
    """src = the middle two frames of a four-frame allocation, so nothing here
    could leave the allocation even unguarded: a missing check would show the
    neighbours' pixels instead of zeros."""
    c, wo, ho = 3, 13, 7
    big = make_frames(4, H, W, c, np.uint8, 17)
    d_big = to_dev(big, dev)
    src = d_big[1:3]
    good = [5, 4, 30, 25]
    cases = [  # (index, rect, valid)
        (0, good, True),
        (-1, good, False),                       # index below the range
        (2, good, False),                        # index n
        (1, [5, 4, 1, 25], False),               # width 1
        (1, good, True),
        (0, [5, 4, 30, 0], False),               # height 0
        (0, [-1, 4, 30, 25], False),             # left -1
        (0, [5, -1, 30, 25], False),
        (1, [W - 29, 4, 30, 25], False),         # left + width = W + 1
        (1, [W - 30, 4, 30, 25], True),          # ... = W: the neighbour that is valid
        (0, [5, H - 24, 30, 25], False),         # top + height = H + 1
        (0, [5, H - 25, 30, 25], True),
        (1, [5, 4, INT32_MAX, 25], False),       # left + width overflows int32
        (1, [5, 4, 30, INT32_MAX], False),
        (0, [INT32_MAX, INT32_MAX, 2, 2], False),
        (0, [0, 0, -5, -5], False),
        (-2 ** 31, good, False),
        (INT32_MAX, good, False),
        (1, [0, 0, W, H], True),
    ]
    idx = np.array([k for k, _, _ in cases], np.int32)
    rects = np.array([r for _, r, _ in cases], np.int32)
    n = len(cases)
    shape, strides = (((n, ho, wo, c), (ho * wo * c + 7, wo * c, c, 1)) if layout == NHWC else
                      ((n, c, ho, wo), (c * ho * wo + 7, ho * wo, wo, 1)))
    dbuf, dview = view_in_buffer(shape, strides, 4, np.float32, dev)
    got, mean, std = ops.crop_resize_rois_standardize(src, to_dev(rects, dev), wo, ho, src_index=to_dev(idx, dev),
                                                      layout=layout, out=dview, stats=True)
    got, mean, std = host(got), host(mean), host(std)
    for i, (k, r, ok) in enumerate(cases):
        what = f"layout {layout}: index {k} rect {r}"
        if ok:
            want, wmean, wstd = oracle_standardized(oracle, oracle_rois(oracle, big[1:3], [k], [r], wo, ho), layout)
            assert wstd.all(), "a valid ROI must not look like an invalid one"
            same_bits(got[i], want[0], what)
            same_bits(mean[i], wmean[0], what + ": mean")
            same_bits(std[i], wstd[0], what + ": stddev")
        else:
            assert not got[i].view(np.int32).any(), what + ": +0.0 everywhere"
            assert not mean[i].view(np.int32).any() and not std[i].view(np.int32).any(), what + ": statistics (0, 0)"
    assert_rim_intact(dbuf, dview, "invalid values")
    assert np.array_equal(host(d_big), big), "source allocation"


# ---------------------------------------------------------------------------
# 7. the index contract, more ROIs than CUs

@gpu
def test_null_index_broadcast_and_identity(ops, dev, oracle):
    c = 3
    frames = make_frames(4, H, W, c, np.uint8, 561)
    rects = RECTS[[0, 3, 8, 11]]
    check(ops, dev, oracle, frames[:1], rects, None, 9, 6, c, NCHW, (REFERENCE,), "broadcast")
    check(ops, dev, oracle, frames, rects, None, 9, 6, c, NHWC, (REFERENCE,), "frame i for ROI i")
    got = ops.crop_resize_rois_standardize(to_dev(frames[1], dev), to_dev(rects, dev), 9, 6)  # an (h, w, c) frame
    want, _, _ = oracle_standardized(oracle, oracle_rois(oracle, frames, [1] * 4, rects, 9, 6), NHWC)
    same_bits(got, want, "3-d frame")
    with pytest.raises(ValueError):  # any other count without an index is refused
        ops.crop_resize_rois_standardize(to_dev(frames[:2], dev), to_dev(rects, dev), 9, 6)


@gpu
def test_more_rois_than_cus(ops, dev, oracle):
    c = 3
    frame = make_frames(1, H, W, c, np.uint8, 563)
    rng = np.random.default_rng(564)
    wh = rng.integers(2, 30, (300, 2))
    lt = (rng.random((300, 2)) * (np.array([W, H]) + 1 - wh)).astype(np.int64)
    rects = np.concatenate([lt, wh], 1).astype(np.int32)
    assert (rects[:, 0] + rects[:, 2] <= W).all() and (rects[:, 1] + rects[:, 3] <= H).all()
    check(ops, dev, oracle, frame, rects, None, 4, 4, c, NCHW, (REFERENCE,), "300 ROIs")


# ---------------------------------------------------------------------------
# 8. mean_out / stddev_out NULL in turn, through the C ABI

@gpu
def test_null_statistics_arrays(ops, dev, oracle):
    import torch
    from vacv_amd import _lib
    c, wo, ho, n = 3, 11, 7, len(RECTS)
    frames = make_frames(3, H, W, c, np.uint8, 571)
    d_frames, d_rects, d_idx = to_dev(frames, dev), to_dev(RECTS, dev), to_dev(IDX, dev)
    want, wmean, wstd = oracle_standardized(oracle, oracle_rois(oracle, frames, IDX, RECTS, wo, ho), NHWC)
    lib = _lib.load()
    stream = torch.cuda.current_stream().cuda_stream
    for give_mean, give_std in [(True, False), (False, True), (False, False), (True, True)]:
        out = torch.full((n, ho, wo, c), -7.0, dtype=torch.float32, device=dev)
        # two neighbouring [n][c] arrays in one sentinel buffer: the one not passed keeps its bytes
        buf = torch.full((2 * n * c * 4,), SENTINEL, dtype=torch.uint8, device=dev)
        first, second = buf[:n * c * 4], buf[n * c * 4:]
        st = lib.vacv_crop_resize_rois_standardize(
            ctypes.byref(ops.describe(d_frames)), ctypes.byref(ops.describe(out)), d_rects.data_ptr(),
            d_idx.data_ptr(), 1, REFERENCE, first.data_ptr() if give_mean else None,
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
    frames = make_frames(3, H, W, c, np.uint8, 581)
    d_frames = to_dev(frames, dev)
    rects_a, rects_b = RECTS[:7], RECTS[5:12]
    idx_a, idx_b = IDX[:7], IDX[:7][::-1].copy()
    d_rects, d_idx = to_dev(rects_a, dev), to_dev(idx_a, dev)
    d_rects_b, d_idx_b = to_dev(rects_b, dev), to_dev(idx_b, dev)
    out_a = torch.empty((7, c, ho, wo), dtype=torch.float32, device=dev)
    out_b = torch.empty_like(out_a)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        ops.crop_resize_rois_standardize(d_frames, d_rects, wo, ho, src_index=d_idx, layout=NCHW, out=out_a,
                                         stream=stream)
        d_rects.copy_(d_rects_b, non_blocking=True)   # overwritten on the stream, between the two calls,
        d_idx.copy_(d_idx_b, non_blocking=True)       # with no host synchronisation
        ops.crop_resize_rois_standardize(d_frames, d_rects, wo, ho, src_index=d_idx, layout=NCHW, out=out_b,
                                         stream=stream)
    stream.synchronize()
    same_bits(out_a, oracle_standardized(oracle, oracle_rois(oracle, frames, idx_a, rects_a, wo, ho), NCHW)[0], "first")
    same_bits(out_b, oracle_standardized(oracle, oracle_rois(oracle, frames, idx_b, rects_b, wo, ho), NCHW)[0], "second")


# ---------------------------------------------------------------------------
# 10. the Python wrapper's checks

@gpu
def test_binding_checks(ops, dev):
    import torch
    frame = to_dev(make_frames(1, 16, 16, 3, np.uint8, 1), dev)
    rects = torch.tensor([[0, 0, 4, 4]] * 4, dtype=torch.int32, device=dev)

    def fn(r, **kw):
        return ops.crop_resize_rois_standardize(frame, r, 4, 4, **kw)

    with pytest.raises(ValueError, match="must live on"):
        fn(rects.cpu())                                   # a host tensor: the wrong device
    with pytest.raises(ValueError, match="rects must be torch.int32"):
        fn(rects.long())
    with pytest.raises(ValueError, match="rects must be torch.int32"):
        fn(rects.float())
    with pytest.raises(ValueError, match="rects must be contiguous"):
        fn(torch.zeros((8, 4), dtype=torch.int32, device=dev)[::2])
    with pytest.raises(ValueError, match=r"rects must have shape \(n, 4\)"):
        fn(rects.reshape(2, 8))
    with pytest.raises(ValueError, match="rects holds no rect"):
        fn(rects[:0])
    with pytest.raises(ValueError, match="src_index must be torch.int32"):
        fn(rects, src_index=torch.zeros(4, dtype=torch.int64, device=dev))
    with pytest.raises(ValueError, match="src_index must live on"):
        fn(rects, src_index=torch.zeros(4, dtype=torch.int32))
    with pytest.raises(ValueError, match=r"src_index must have shape \(4,\)"):
        fn(rects, src_index=torch.zeros(3, dtype=torch.int32, device=dev))
    with pytest.raises(ValueError, match="takes uint8 frames"):
        ops.crop_resize_rois_standardize(frame.float(), rects, 4, 4)
    # two or four channels have no planar output; a u8 destination is refused
    for c in (2, 4):
        unsupported(lambda: ops.crop_resize_rois_standardize(to_dev(make_frames(1, 16, 16, c, np.uint8, 2), dev),
                                                             rects, 4, 4, layout=NCHW))
    import vacv_amd as V
    with pytest.raises(V.VacvError) as e:
        fn(rects, out=torch.empty((4, 4, 4, 3), dtype=torch.uint8, device=dev))
    assert e.value.status == V._lib.ERR_INVALID_ARG
    # lists and numpy arrays are moved for convenience
    got, mean, std = ops.crop_resize_rois_standardize(frame, [[0, 0, 4, 4], [3, 5, 4, 4]], 4, 4, src_index=[0, 0],
                                                      stats=True)
    assert tuple(got.shape) == (2, 4, 4, 3) and tuple(mean.shape) == tuple(std.shape) == (2, 3)
    from vacv_amd import crop_resize_rois_standardize
    assert crop_resize_rois_standardize is ops.crop_resize_rois_standardize


# ---------------------------------------------------------------------------
# 11. the C++ layer

@gpu
def test_cpp_crop_resize_standardize(hip_device, tmp_path):
    repo = Path(__file__).resolve().parent.parent
    pkg = repo / "arm-neon-opencv_amd"
    lib = pkg / "lib"
    exe = tmp_path / "vacv_crop_resize_std_test"
    r = subprocess.run(["g++", "-std=c++14", "-O1", str(repo / "tests" / "cpp" / "vacv_crop_resize_std_test.cpp"),
                        "-o", str(exe), "-I", str(pkg / "src"), "-L", str(lib), "-lvacv", "-lvacv_hip",
                        f"-Wl,-rpath,{lib}"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run(["timeout", "-k", "10", "120", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "failed 0" in r.stdout, r.stdout[-3000:]
