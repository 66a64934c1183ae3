"""vacv_cvt_color_crop_resize_rois_standardize on the GPU: many upright crops
straight from NV21 / NV12 frames in one launch, each standardized by its own
per-channel mean and standard deviation (csrc/k_yuv_crop_resize_rois_std.hip).

Every comparison is bit-exact, on the int32 views of the floats, so that -0.0
and +0.0 differ, and the expected value comes from two sources that must both
agree with the result, output and statistics:
 (a) the host oracle: yuv420sp_to_bgr of the indexed frame, crop, resize_linear,
     mean_stddev_exact, normalize, hwc_to_chw;
 (b) the GPU chain the call replaces: ops.cvt_color of all frames, then
     ops.crop_resize_rois_standardize on the decoded frames.
Frames are 130 x 98: rows start at 2 modulo 4, a dense frame is 130 x 147
bytes.  The shapes are the smallest that reach every path of the kernel:
outputs of fewer pixels than a workgroup has threads and of more, dense
destinations at every 16-byte phase and pitched ones, the frame's last bytes
as the allocation's last, the largest ROI the LDS gate admits, more ROIs than
the device has CUs.
"""
from __future__ import annotations

import ctypes
import subprocess
from pathlib import Path

import numpy as np
import pytest

from test_crop_resize_rois_gpu import oracle_rois, to_dev, view_in_buffer
from test_crop_resize_rois_std_gpu import oracle_standardized, same_bits
from test_gpu_plumbing import SENTINEL, assert_rim_intact, assert_untouched, host, place, unsupported
from test_yuv_crop_resize_rois_gpu import IDX, RECTS
from test_yuv_rois_gpu import CODE_IDS, CODES, decode, make_yuv

gpu = pytest.mark.gpu
NHWC, NCHW = 1, 0
REFERENCE, NEON, OPENCV = 0, 1, 2
MODES = (REFERENCE, NEON, OPENCV)
NV12_RGB, NV12_BGR, NV21_RGB, NV21_BGR = 90, 91, 92, 93
W, H = 130, 98   # decoded frames
INT32_MAX = 2 ** 31 - 1
SIZES = [(37, 29), (1, 1), (1, 7), (9, 1), (2, 2)]
END_RECTS = np.array([[W - 2, H - 2, 2, 2], [W - 3, H - 3, 3, 3], [100, 80, 30, 18]], np.int32)


@pytest.fixture(scope="module")
def ops(hip_device):
    from vacv_amd import ops
    return ops


@pytest.fixture(scope="module")
def dev(hip_device):
    return hip_device


def lds_need(w, h):
    """include/vacv_hip.h's formula (csrc/k_yuv_crop_resize_rois_std.hip), restated."""
    return 256 + (3 * w * h + 15) // 16 * 16 + max(8 * (w + h), 3072)


def gpu_chain(ops, d_yuv, code, d_rects, wo, ho, d_idx, mode, layout):
    """(b): the two calls whose result the one call must reproduce."""
    return ops.crop_resize_rois_standardize(ops.cvt_color(d_yuv, code), d_rects, wo, ho, src_index=d_idx, mode=mode,
                                            layout=layout, stats=True)


def check(ops, dev, oracle, yuv, rects, idx, wo, ho, code, layout, modes, what, d_yuv=None, host_oracle=True):
    """One call against (a) and (b), output and statistics, for each mode."""
    frames = yuv if yuv.ndim == 3 else yuv[None]
    d_yuv = to_dev(yuv, dev) if d_yuv is None else d_yuv
    d_rects = to_dev(np.asarray(rects, np.int32), dev)
    d_idx = to_dev(np.asarray(idx, np.int32), dev) if idx is not None else None
    n = len(rects)
    oidx = idx if idx is not None else ([0] * n if len(frames) == 1 else list(range(n)))
    bgr = decode(oracle, frames, code) if host_oracle else None
    for mode in modes:
        w_ = f"{what} {CODE_IDS[code]} layout {layout} {wo}x{ho} mode {mode}"
        got, mean, std = ops.cvt_color_crop_resize_rois_standardize(d_yuv, d_rects, wo, ho, code=code, src_index=d_idx,
                                                                    mode=mode, layout=layout, stats=True)
        assert tuple(got.shape) == ((n, ho, wo, 3) if layout == NHWC else (n, 3, ho, wo))
        assert tuple(mean.shape) == tuple(std.shape) == (n, 3)
        c_out, c_mean, c_std = gpu_chain(ops, d_yuv, code, d_rects, wo, ho, d_idx, mode, layout)
        same_bits(got, c_out, w_ + " vs cvt_color + crop_resize_rois_standardize")
        same_bits(mean, c_mean, w_ + ": mean vs the chain")
        same_bits(std, c_std, w_ + ": stddev vs the chain")
        if host_oracle:
            want, wmean, wstd = oracle_standardized(oracle, oracle_rois(oracle, bgr, oidx, rects, wo, ho, mode), layout)
            same_bits(got, want, w_ + " vs the oracle chain")
            same_bits(mean, wmean, w_ + ": mean vs oracle")
            same_bits(std, wstd, w_ + ": stddev vs oracle")
        # stats=False writes the same output
        same_bits(ops.cvt_color_crop_resize_rois_standardize(d_yuv, d_rects, wo, ho, code=code, src_index=d_idx,
                                                             mode=mode, layout=layout), got, w_ + ": stats=False")
    return got, mean, std


# ---------------------------------------------------------------------------
# 1. codes x modes x layouts x sizes

@gpu
@pytest.mark.parametrize("layout", [NHWC, NCHW], ids=["nhwc", "nchw"])
@pytest.mark.parametrize("code", list(CODES), ids=lambda c: CODE_IDS[c])
def test_matches_both_chains(ops, dev, oracle, code, layout):
    yuv = make_yuv(3, W, H, 1500 + code)
    for wo, ho in SIZES:
        got, mean, std = check(ops, dev, oracle, yuv, RECTS, IDX, wo, ho, code, layout, MODES, "grid")
        if (wo, ho) == (1, 1):  # one pixel: the mean is the pixel, the deviation 0, the output +0.0
            assert not host(std).any() and not host(got).view(np.int32).any() and host(mean).any()


@gpu
def test_model_input_size(ops, dev, oracle):
    yuv = make_yuv(3, W, H, 1511)
    check(ops, dev, oracle, yuv, RECTS[[0, 4, 8, 13]], IDX[[0, 4, 8, 13]], 112, 112, NV21_BGR, NCHW, (REFERENCE,), "112")


# ---------------------------------------------------------------------------
# 2. the frame's end

@gpu
@pytest.mark.parametrize("off", [0, 1, 2, 3])
def test_frame_end(ops, dev, oracle, off):
    """The dense 130 x 98 frame as the last bytes of its buffer, at every base
    alignment: the last chroma pair is read byte by byte, and a load reaching
    past it has nothing behind it."""
    import torch
    yuv = make_yuv(1, W, H, 1520 + off)
    buf = torch.full((off + yuv.size,), SENTINEL, dtype=torch.uint8, device=dev)
    buf[off:] = to_dev(yuv.reshape(-1), dev)
    d_yuv = buf[off:].view(1, H * 3 // 2, W)
    assert d_yuv.data_ptr() + yuv.size == buf.data_ptr() + buf.numel()
    for wo, ho in [(37, 29), (5, 3)]:
        for code, layout in ((NV21_BGR, NCHW), (NV12_RGB, NHWC)):
            check(ops, dev, oracle, yuv, END_RECTS, None, wo, ho, code, layout, (REFERENCE, NEON), f"off {off}",
                  d_yuv=d_yuv)
    assert (host(buf)[:off] == SENTINEL).all() and np.array_equal(host(buf)[off:], yuv.reshape(-1))


# ---------------------------------------------------------------------------
# 3. the LDS limit

@gpu
def test_largest_roi_constant_frame(ops, dev):
    """144 x 144 is exactly 64 KiB of LDS.  A constant Y / VU frame decodes to
    one colour: stddev 0 and every output +0.0.  One row more is refused with
    nothing written."""
    wo, ho = 144, 144
    assert lds_need(wo, ho) == 65536 < lds_need(wo, ho + 1)
    yuv = np.empty((1, H * 3 // 2, W), np.uint8)
    yuv[0, :H] = 180
    yuv[0, H:, 0::2], yuv[0, H:, 1::2] = 90, 170
    d_yuv = to_dev(yuv, dev)
    d_rects = to_dev(np.array([[0, 0, W, H], [5, 3, 20, 30]], np.int32), dev)
    got, mean, std = ops.cvt_color_crop_resize_rois_standardize(d_yuv, d_rects, wo, ho, stats=True)
    same_bits(got, np.zeros((2, ho, wo, 3), np.float32), "constant frame")
    assert not host(std).view(np.int32).any() and (host(mean)[0] == host(mean)[1]).all() and host(mean).all()
    c_out, c_mean, c_std = gpu_chain(ops, d_yuv, NV21_BGR, d_rects, wo, ho, None, REFERENCE, NHWC)
    same_bits(got, c_out, "vs the chain")
    same_bits(mean, c_mean, "mean")
    same_bits(std, c_std, "stddev")
    buf, out = place(np.zeros((2, ho + 1, wo, 3), np.float32), dev)
    buf.fill_(SENTINEL)
    unsupported(lambda: ops.cvt_color_crop_resize_rois_standardize(d_yuv, d_rects, wo, ho + 1, out=out))
    assert_untouched(buf, "past the LDS limit")


@gpu
def test_largest_roi_random_frame(ops, dev, oracle):
    yuv = make_yuv(3, W, H, 1531)
    check(ops, dev, oracle, yuv, RECTS[[0, 8]], IDX[[3, 5]], 144, 144, NV21_BGR, NCHW, (REFERENCE,), "64 KiB",
          host_oracle=False)


# ---------------------------------------------------------------------------
# 4. pitched, misaligned shapes

PITCH_CASES = [  # layout, dst off (bytes), pitched dst (row + 5, plane + 9, batch + 11 floats)
    (NHWC, 4, True), (NCHW, 8, True), (NCHW, 12, True), (NHWC, 12, True), (NCHW, 4, True), (NHWC, 8, True),
] + [(NHWC, off, False) for off in (0, 4, 8, 12)] + [(NCHW, off, False) for off in (0, 4, 8, 12)]


@pytest.fixture(scope="module")
def pitched_reference(oracle):
    """Frames and (a) for the pitched cases, computed once."""
    yuv = make_yuv(3, W, H, 1540)
    bgr = decode(oracle, yuv, NV21_BGR)
    ref = {(wo, ho, layout): oracle_standardized(oracle, oracle_rois(oracle, bgr, IDX, RECTS, wo, ho), layout)
           for wo, ho in [(33, 9), (5, 3)] for layout in (NHWC, NCHW)}
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
    d_rects, d_idx = to_dev(RECTS, dev), to_dev(IDX, dev)
    n = len(RECTS)
    rpad, ppad, bpad = (5, 9, 11) if pitched else (0, 0, 0)
    for wo, ho in [(33, 9), (5, 3)]:
        if layout == NCHW:
            rp = wo + rpad
            pl = ho * rp + ppad
            dbuf, dview = view_in_buffer((n, 3, ho, wo), (3 * pl + bpad, pl, rp, 1), doff, np.float32, dev)
        else:
            rp = wo * 3 + rpad
            dbuf, dview = view_in_buffer((n, ho, wo, 3), (ho * rp + bpad, rp, 3, 1), doff, np.float32, dev)
        what = f"{case} {wo}x{ho}"
        got, mean, std = ops.cvt_color_crop_resize_rois_standardize(d_yuv, d_rects, wo, ho, src_index=d_idx,
                                                                    layout=layout, out=dview, stats=True)
        assert got.data_ptr() == dview.data_ptr()
        want, wmean, wstd = ref[(wo, ho, layout)]
        c_out, c_mean, c_std = gpu_chain(ops, d_yuv, NV21_BGR, d_rects, wo, ho, d_idx, REFERENCE, layout)
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
# 5. invalid device values: range checks, zeros, nothing read

@gpu
@pytest.mark.parametrize("layout", [NHWC, NCHW])
def test_invalid_rects_and_indices_give_zeros(ops, dev, oracle, layout):
    """src = the middle two frames of a four-frame allocation, so nothing here
    could leave the allocation even unguarded: a missing check would show the
    neighbours' pixels instead of zeros.  A rect is judged against the DECODED
    130 x 98 size: the chroma rows below row 98 are no place for one."""
    wo, ho = 13, 7
    big = make_yuv(4, W, H, 1550)
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
    shape, strides = (((n, ho, wo, 3), (ho * wo * 3 + 7, wo * 3, 3, 1)) if layout == NHWC else
                      ((n, 3, ho, wo), (3 * ho * wo + 7, ho * wo, wo, 1)))
    dbuf, dview = view_in_buffer(shape, strides, 4, np.float32, dev)
    d_rects, d_idx = to_dev(rects, dev), to_dev(idx, dev)
    got, mean, std = ops.cvt_color_crop_resize_rois_standardize(src, d_rects, wo, ho, src_index=d_idx, layout=layout,
                                                                out=dview, stats=True)
    c_out, c_mean, c_std = gpu_chain(ops, src, NV21_BGR, d_rects, wo, ho, d_idx, REFERENCE, layout)
    same_bits(host(got), c_out, "vs the chain")
    same_bits(mean, c_mean, "mean vs the chain")
    same_bits(std, c_std, "stddev vs the chain")
    got, mean, std = host(got), host(mean), host(std)
    bgr = decode(oracle, big[1:3], NV21_BGR)
    for i, (k, r, ok) in enumerate(cases):
        what = f"layout {layout}: index {k} rect {r}"
        if ok:
            want, wmean, wstd = oracle_standardized(oracle, oracle_rois(oracle, bgr, [k], [r], wo, ho), layout)
            assert wstd.all(), "a valid ROI must not look like an invalid one"
            same_bits(got[i], want[0], what)
            same_bits(mean[i], wmean[0], what + ": mean")
            same_bits(std[i], wstd[0], what + ": stddev")
        else:
            assert not got[i].view(np.int32).any(), what + ": +0.0 everywhere"
            assert not mean[i].view(np.int32).any() and not std[i].view(np.int32).any(), what + ": statistics (0, 0)"
    assert_rim_intact(dbuf, dview, "invalid values")
    assert np.array_equal(host(d_big), big), "source allocation"  # and the device reads back normally


# ---------------------------------------------------------------------------
# 6. / 7. more ROIs than CUs, the index contract

@gpu
def test_more_rois_than_cus(ops, dev, oracle):
    yuv = make_yuv(1, 64, 64, 1560)
    rng = np.random.default_rng(1561)
    wh = rng.integers(2, 40, (300, 2))
    lt = (rng.random((300, 2)) * (65 - wh)).astype(np.int64)
    rects = np.concatenate([lt, wh], 1).astype(np.int32)
    assert (rects[:, 0] + rects[:, 2] <= 64).all() and (rects[:, 1] + rects[:, 3] <= 64).all()
    check(ops, dev, oracle, yuv, rects, None, 8, 8, NV21_BGR, NCHW, (REFERENCE,), "300 ROIs")


@gpu
def test_null_index_broadcast_and_identity(ops, dev, oracle):
    yuv = make_yuv(4, W, H, 1570)
    rects = RECTS[[0, 4, 8, 13]]
    check(ops, dev, oracle, yuv[:1], rects, None, 9, 6, NV12_RGB, NCHW, (REFERENCE,), "broadcast")
    check(ops, dev, oracle, yuv, rects, None, 9, 6, NV21_BGR, NHWC, (REFERENCE,), "frame i for ROI i")
    check(ops, dev, oracle, yuv[1], rects, None, 9, 6, NV21_BGR, NHWC, (REFERENCE,), "2-d frame")
    for k in (2, 3):  # any other count without an index is refused
        with pytest.raises(ValueError, match="without src_index, src must hold 1 or 4 images"):
            ops.cvt_color_crop_resize_rois_standardize(to_dev(yuv[:k], dev), to_dev(rects, dev), 9, 6)


# ---------------------------------------------------------------------------
# 8. mean_out / stddev_out NULL in turn, through the C ABI

@gpu
def test_null_statistics_arrays(ops, dev, oracle):
    import torch
    from vacv_amd import _lib
    wo, ho, n = 11, 7, len(RECTS)
    yuv = make_yuv(3, W, H, 1580)
    d_yuv, d_rects, d_idx = to_dev(yuv, dev), to_dev(RECTS, dev), to_dev(IDX, dev)
    want, wmean, wstd = oracle_standardized(
        oracle, oracle_rois(oracle, decode(oracle, yuv, NV12_BGR), IDX, RECTS, wo, ho), NHWC)
    lib = _lib.load()
    stream = torch.cuda.current_stream().cuda_stream
    for give_mean, give_std in [(True, False), (False, True), (False, False), (True, True)]:
        out = torch.full((n, ho, wo, 3), -7.0, dtype=torch.float32, device=dev)
        # two neighbouring [n][3] arrays in one sentinel buffer: the one not passed keeps its bytes
        buf = torch.full((2 * n * 3 * 4,), SENTINEL, dtype=torch.uint8, device=dev)
        first, second = buf[:n * 3 * 4], buf[n * 3 * 4:]
        st = lib.vacv_cvt_color_crop_resize_rois_standardize(
            ctypes.byref(ops.describe(d_yuv.unsqueeze(-1))), ctypes.byref(ops.describe(out)), NV12_BGR,
            d_rects.data_ptr(), d_idx.data_ptr(), 1, REFERENCE, first.data_ptr() if give_mean else None,
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
    yuv = make_yuv(3, W, H, 1590)
    d_yuv = to_dev(yuv, dev)
    rects_a, rects_b = RECTS[:7], RECTS[7:14]
    idx_a, idx_b = IDX[:7], IDX[:7][::-1].copy()
    d_rects, d_idx = to_dev(rects_a, dev), to_dev(idx_a, dev)
    d_rects_b, d_idx_b = to_dev(rects_b, dev), to_dev(idx_b, dev)
    out_a = torch.empty((7, 3, ho, wo), dtype=torch.float32, device=dev)
    out_b = torch.empty_like(out_a)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        ops.cvt_color_crop_resize_rois_standardize(d_yuv, d_rects, wo, ho, src_index=d_idx, layout=NCHW, out=out_a,
                                                   stream=stream)
        d_rects.copy_(d_rects_b, non_blocking=True)   # overwritten on the stream, between the two calls,
        d_idx.copy_(d_idx_b, non_blocking=True)       # with no host synchronisation
        ops.cvt_color_crop_resize_rois_standardize(d_yuv, d_rects, wo, ho, src_index=d_idx, layout=NCHW, out=out_b,
                                                   stream=stream)
    stream.synchronize()
    bgr = decode(oracle, yuv, NV21_BGR)
    same_bits(out_a, oracle_standardized(oracle, oracle_rois(oracle, bgr, idx_a, rects_a, wo, ho), NCHW)[0], "first")
    same_bits(out_b, oracle_standardized(oracle, oracle_rois(oracle, bgr, idx_b, rects_b, wo, ho), NCHW)[0], "second")


# ---------------------------------------------------------------------------
# 10. the Python wrapper's checks

@gpu
def test_binding_checks(ops, dev):
    import torch
    import vacv_amd as V
    frame = to_dev(make_yuv(1, 16, 16, 1), dev)
    rects = torch.tensor([[0, 0, 4, 4]] * 4, dtype=torch.int32, device=dev)

    def fn(r, **kw):
        return ops.cvt_color_crop_resize_rois_standardize(frame, r, 4, 4, **kw)

    with pytest.raises(ValueError, match="must live on"):
        fn(rects.cpu())                                   # a host tensor: the wrong device
    with pytest.raises(ValueError, match="rects must be torch.int32"):
        fn(rects.long())
    with pytest.raises(ValueError, match="rects must be contiguous"):
        fn(torch.zeros((8, 4), dtype=torch.int32, device=dev)[::2])
    with pytest.raises(ValueError, match=r"rects must have shape \(n, 4\)"):
        fn(rects.reshape(2, 8))
    with pytest.raises(ValueError, match="src_index must be torch.int32"):
        fn(rects, src_index=torch.zeros(4, dtype=torch.int64, device=dev))
    with pytest.raises(ValueError, match="src_index must live on"):
        fn(rects, src_index=torch.zeros(4, dtype=torch.int32))
    # an FP32 "yuv" and a multi-channel one are no YUV420sp frames
    with pytest.raises(V.VacvError) as e:
        ops.cvt_color_crop_resize_rois_standardize(frame.float(), rects, 4, 4)
    assert e.value.status == V._lib.ERR_INVALID_ARG
    with pytest.raises(ValueError, match="expected a 2-4 dimensional image tensor"):
        ops.cvt_color_crop_resize_rois_standardize(torch.zeros((1, 24, 16, 3), dtype=torch.uint8, device=dev), rects, 4, 4)
    with pytest.raises(V.VacvError) as e:  # a u8 destination
        fn(rects, out=torch.empty((4, 4, 4, 3), dtype=torch.uint8, device=dev))
    assert e.value.status == V._lib.ERR_INVALID_ARG
    # lists and numpy arrays are moved for convenience
    got, mean, std = ops.cvt_color_crop_resize_rois_standardize(frame, [[0, 0, 4, 4], [3, 5, 4, 4]], 4, 4,
                                                                src_index=[0, 0], stats=True)
    assert tuple(got.shape) == (2, 4, 4, 3) and tuple(mean.shape) == tuple(std.shape) == (2, 3)
    assert got.dtype == mean.dtype == std.dtype == torch.float32
    from vacv_amd import cvt_color_crop_resize_rois_standardize
    assert cvt_color_crop_resize_rois_standardize is ops.cvt_color_crop_resize_rois_standardize


# ---------------------------------------------------------------------------
# 11. the C++ layer

@gpu
def test_cpp_cvt_color_crop_resize_standardize(hip_device, tmp_path):
    repo = Path(__file__).resolve().parent.parent
    pkg = repo / "arm-neon-opencv_amd"
    lib = pkg / "lib"
    exe = tmp_path / "vacv_yuv_crop_resize_std_test"
    r = subprocess.run(["g++", "-std=c++14", "-O1", str(repo / "tests" / "cpp" / "vacv_yuv_crop_resize_std_test.cpp"),
                        "-o", str(exe), "-I", str(pkg / "src"), "-L", str(lib), "-lvacv", "-lvacv_hip",
                        f"-Wl,-rpath,{lib}"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run(["timeout", "-k", "10", "120", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "failed 0" in r.stdout, r.stdout[-3000:]
