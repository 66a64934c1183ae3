"""vacv_warp_affine_rois / _rois_normalize / vacv_invert_affine_device on the
GPU: many crops in one launch, each with its own device-resident matrix and
source index (csrc/k_warp_rois.hip).

Every comparison is bit-exact: the expected ROI is the oracle's warp_affine of
the indexed frame (the single-call path already agrees with it to the bit),
and the single-call entry points are asserted equal too.  The shapes are the
smallest that reach every path of the kernel: ROIs narrower than a wave (5, 8,
37), wider (112, 140), one pixel, more than one 1024-pixel tile per ROI,
dense and pitched destinations at every base alignment, more than 256 ROIs.
"""
from __future__ import annotations

import subprocess
from pathlib import Path

import numpy as np
import pytest

from test_gpu_plumbing import SENTINEL, assert_bits, assert_rim_intact, host, place

gpu = pytest.mark.gpu
NHWC, NCHW = 1, 0
CONSTANT, REPLICATE, REFLECT, WRAP, REFLECT_101 = 0, 1, 2, 3, 4
H, W = 97, 131  # frames
SIZES = [(112, 112), (140, 210), (37, 53), (64, 64), (65, 5), (5, 3), (1, 1)]  # (wo, ho)
IDX7 = [2, 0, 0, 1, 2, 2, 1]
BORDER_U8 = (7, 99, 200, 33)
BORDER_F32 = (7.5, -3.25, 200.0, 0.125)
MEAN = np.array([104.5, 117.25, 123.0, 1.0], np.float32)
STD = np.array([57.375, 57.12, 58.395, 2.0], np.float32)


@pytest.fixture(scope="module")
def ops(hip_device):
    from vacv_amd import ops
    return ops


@pytest.fixture(scope="module")
def dev(hip_device):
    return hip_device


def to_dev(a, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def make_frames(n, h, w, c, dtype, seed):
    """Smooth-ish random frames: neighbouring pixels differ, so a wrong tap shows."""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 256, (n, h, w, c), dtype=np.uint8)
    if np.dtype(dtype) == np.uint8:
        return a
    return a.astype(np.float32) * np.float32(0.75) + np.float32(0.125)


def random_maps(rng, n, w, h, wo, ho):
    """As test_warp_random_matrices: any rotation, anisotropic scale 0.4-2.5,
    shear, the centre jittered by up to half an output; several hang off the frame."""
    ms = np.zeros((n, 6), np.float32)
    for i in range(n):
        a = np.deg2rad(rng.uniform(-180.0, 180.0))
        sx, sy = rng.uniform(0.4, 2.5, 2)
        A = np.array([[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]]) @ np.array([[sx, rng.uniform(-0.6, 0.6)],
                                                                                   [0.0, sy]])
        tv = np.array([wo / 2, ho / 2]) - A @ np.array([w / 2, h / 2]) + rng.uniform(-0.5, 0.5, 2) * (wo, ho)
        ms[i] = np.concatenate([A, tv[:, None]], 1).astype(np.float32).reshape(6)
    return ms


def border_of(dtype, c):
    """The oracle's per-channel border; the library takes border_value[4] (the rest unused)."""
    return (BORDER_U8 if np.dtype(dtype) == np.uint8 else BORDER_F32)[:c]


def border4(dtype):
    return BORDER_U8 if np.dtype(dtype) == np.uint8 else BORDER_F32


def oracle_rois(oracle, frames, idx, ms, wo, ho, border, mode):
    """[n_roi, ho, wo, c]: the oracle's warp_affine of frame idx[i] under ms[i]."""
    c = frames.shape[3]
    out = []
    for i, m in enumerate(ms):
        f = frames[idx[i]]
        want = oracle.warp_affine(f if c > 1 else f[..., 0], m, wo, ho, border=border if c > 1 else border[0],
                                  border_mode=mode)
        out.append(want.reshape(ho, wo, c))
    return np.stack(out)


def filled(n, ho, wo, border, dtype):
    c = len(border)
    return np.broadcast_to(np.asarray(border, dtype), (n, ho, wo, c)).copy()


def view_in_buffer(shape, strides, off, dtype, dev):
    """(buffer, view): a strided view (`strides` in elements, first element
    `off` bytes in) of a SENTINEL-filled flat device buffer, 32 bytes to spare."""
    import torch
    es = np.dtype(dtype).itemsize
    assert off % es == 0
    span = 1 + sum((s - 1) * st for s, st in zip(shape, strides))
    buffer = torch.full((off + span * es + 32,), SENTINEL, dtype=torch.uint8, device=dev)
    tdt = torch.uint8 if es == 1 else torch.float32
    view = buffer[off:off + span * es].view(tdt).as_strided(shape, strides)
    return buffer, view


# ---------------------------------------------------------------------------
# 1. parity with the oracle and with the single-call entry point

@gpu
@pytest.mark.parametrize("dtype", [np.uint8, np.float32], ids=["u8", "f32"])
@pytest.mark.parametrize("c", [1, 2, 3, 4])
def test_rois_match_oracle_and_single_calls(ops, dev, oracle, c, dtype):
    import torch
    frames = make_frames(3, H, W, c, dtype, 100 + c)
    d_frames = to_dev(frames, dev)
    d_idx = to_dev(np.array(IDX7, np.int32), dev)
    border = border_of(dtype, c)
    rng = np.random.default_rng(20261019 + c)
    for wo, ho in SIZES:
        ms = random_maps(rng, 7, W, H, wo, ho)
        d_ms = to_dev(ms, dev)
        for mode in (CONSTANT, REPLICATE, REFLECT, WRAP, REFLECT_101):
            what = f"c={c} {np.dtype(dtype).name} {wo}x{ho} border {mode}"
            got = ops.warp_affine_rois(d_frames, d_ms, wo, ho, src_index=d_idx, border_mode=mode, border_value=border4(dtype))
            assert tuple(got.shape) == (7, ho, wo, c) and got.dtype == d_frames.dtype
            single = torch.stack([ops.warp_affine(d_frames[IDX7[i]], ms[i], wo, ho, border_mode=mode,
                                                  border_value=border4(dtype)) for i in range(7)])
            want = oracle_rois(oracle, frames, IDX7, ms, wo, ho, border, mode)
            got = host(got)
            for i in range(7):
                assert_bits(got[i], want[i], f"{what} roi {i} m={ms[i].tolist()} vs oracle")
            assert_bits(got, host(single), what + " vs vacv_warp_affine per ROI")


# ---------------------------------------------------------------------------
# 2. WARP_INVERSE_MAP

@gpu
@pytest.mark.parametrize("dtype", [np.uint8, np.float32], ids=["u8", "f32"])
def test_rois_inverse_map(ops, dev, oracle, dtype):
    from vacv_amd import INTER_LINEAR, WARP_INVERSE_MAP
    c, wo, ho = 3, 37, 53
    frames = make_frames(3, H, W, c, dtype, 7)
    d_frames, d_idx = to_dev(frames, dev), to_dev(np.array(IDX7, np.int32), dev)
    ms = random_maps(np.random.default_rng(5), 7, W, H, wo, ho)
    inv = np.stack([oracle.invert_affine(m) for m in ms])
    for mode in (CONSTANT, REFLECT_101):
        fwd = ops.warp_affine_rois(d_frames, to_dev(ms, dev), wo, ho, src_index=d_idx, border_mode=mode,
                                   border_value=border4(dtype))
        back = ops.warp_affine_rois(d_frames, to_dev(inv, dev).reshape(7, 2, 3), wo, ho, src_index=d_idx,
                                    flags=INTER_LINEAR | WARP_INVERSE_MAP, border_mode=mode,
                                    border_value=border4(dtype))
        assert_bits(host(back), host(fwd), f"inverse map, border {mode}")
        assert_bits(host(fwd), oracle_rois(oracle, frames, IDX7, ms, wo, ho, border_of(dtype, c), mode), "forward")


# ---------------------------------------------------------------------------
# 3. fused normalize, NHWC and NCHW

def oracle_normalized(oracle, want, mean, std):
    """normalize of [n, ho, wo, c] u8 or fp32 ROIs, as the single-call path does it."""
    out = []
    for r in want:
        f = oracle.u8_to_f32(r) if r.dtype == np.uint8 else r
        c = f.shape[2]
        out.append(oracle.normalize(f if c > 1 else f[..., 0], mean, std).reshape(f.shape))
    return np.stack(out)


@gpu
@pytest.mark.parametrize("dtype", [np.uint8, np.float32], ids=["u8", "f32"])
@pytest.mark.parametrize("c,layout", [(3, NCHW), (1, NCHW), (2, NHWC), (4, NHWC), (3, NHWC), (1, NHWC)])
def test_rois_normalize(ops, dev, oracle, c, layout, dtype):
    import torch
    frames = make_frames(3, H, W, c, dtype, 200 + c)
    d_frames, d_idx = to_dev(frames, dev), to_dev(np.array(IDX7, np.int32), dev)
    mean, std, border = MEAN[:c], STD[:c], border_of(dtype, c)
    rng = np.random.default_rng(31 + c)
    for wo, ho in [(112, 112), (37, 53), (5, 3)]:
        ms = random_maps(rng, 7, W, H, wo, ho)
        for mode in (CONSTANT, REPLICATE):
            what = f"c={c} layout {layout} {np.dtype(dtype).name} {wo}x{ho} border {mode}"
            got = ops.warp_affine_rois_normalize(d_frames, to_dev(ms, dev), wo, ho, mean, std, src_index=d_idx,
                                                 out_layout=layout, border_mode=mode, border_value=border4(dtype))
            assert got.dtype == torch.float32
            assert tuple(got.shape) == ((7, ho, wo, c) if layout == NHWC else (7, c, ho, wo))
            want = oracle_normalized(oracle, oracle_rois(oracle, frames, IDX7, ms, wo, ho, border, mode), mean, std)
            if layout == NCHW:
                want = want.transpose(0, 3, 1, 2)
            assert_bits(host(got), want, what + " vs oracle")
            # vacv_warp_affine_normalize per ROI (+ vacv_change_layout for planar output)
            single = torch.stack([ops.warp_affine_normalize(d_frames[IDX7[i]], ms[i], wo, ho, mean, std,
                                                            border_mode=mode, border_value=border4(dtype)) for i in range(7)])
            if layout == NCHW:
                single = ops.change_layout(single.reshape(7, ho, wo, c), NCHW)
            assert_bits(host(got), host(single).reshape(got.shape), what + " vs single calls")


# ---------------------------------------------------------------------------
# 4. pitched, misaligned, tail shapes

PITCH_CASES = [
    # dtype, c, out ("same" | NHWC | NCHW normalize), src off, src row pad, dst off, dst row pad, plane pad, batch pad
    (np.uint8, 3, "same", 0, 0, 1, 0, 0, 0),      # dense ROIs at an odd base: 16-byte stores after a byte head
    (np.uint8, 3, "same", 1, 5, 3, 0, 0, 0),
    (np.uint8, 3, "same", 3, 2, 16, 0, 0, 5),     # dense rows, ROIs 5 bytes apart
    (np.uint8, 3, "same", 1, 7, 0, 7, 0, 11),     # pitched rows: 16-, 4-byte and byte runs
    (np.uint8, 3, "same", 0, 1, 5, 1, 0, 0),
    (np.uint8, 1, "same", 3, 3, 2, 3, 0, 2),
    (np.uint8, 4, "same", 1, 4, 4, 4, 0, 4),
    (np.uint8, 3, NCHW, 1, 5, 4, 0, 0, 0),        # planar fp32, dense planes
    (np.uint8, 3, NCHW, 3, 0, 8, 3, 5, 7),        # row, plane and batch padding
    (np.uint8, 3, NHWC, 0, 9, 12, 2, 0, 3),
    (np.float32, 3, "same", 4, 3, 4, 0, 0, 0),
    (np.float32, 3, "same", 4, 1, 8, 5, 0, 9),
    (np.float32, 3, NCHW, 4, 2, 12, 1, 3, 2),
    (np.float32, 2, NHWC, 0, 0, 4, 3, 0, 1),
]


@gpu
@pytest.mark.parametrize("case", PITCH_CASES, ids=lambda t: f"{np.dtype(t[0]).name}-c{t[1]}-{t[2]}-s{t[3]}_{t[4]}-d{t[5]}_{t[6]}_{t[7]}_{t[8]}")
def test_rois_pitched_misaligned(ops, dev, oracle, case):
    dtype, c, out, soff, spad, doff, rpad, ppad, bpad = case
    frames = make_frames(3, 61, 83, c, dtype, 300 + c)
    sbuf, sview = place(frames, dev, NHWC, off=soff, row_pad=spad, batch_pad=spad)
    d_idx = to_dev(np.array(IDX7, np.int32), dev)
    border = border_of(dtype, c)
    mean, std = MEAN[:c], STD[:c]
    rng = np.random.default_rng(41)
    for wo, ho in [(37, 53), (140, 9), (5, 3)]:  # 37 * 3 = 111 row bytes; 1961 px = two tiles split mid-row
        ms = random_maps(rng, 7, 83, 61, wo, ho)
        want = oracle_rois(oracle, frames, IDX7, ms, wo, ho, border, CONSTANT)
        odt = dtype if out == "same" else np.float32
        if out == NCHW:
            rp = wo + rpad
            pl = ho * rp + ppad
            dbuf, dview = view_in_buffer((7, c, ho, wo), (c * pl + bpad, pl, rp, 1), doff, odt, dev)
        else:
            rp = wo * c + rpad
            dbuf, dview = view_in_buffer((7, ho, wo, c), (ho * rp + bpad, rp, c, 1), doff, odt, dev)
        what = f"{case} {wo}x{ho}"
        if out == "same":
            got = ops.warp_affine_rois(sview, to_dev(ms, dev), wo, ho, src_index=d_idx, border_value=border4(dtype), out=dview)
        else:
            got = ops.warp_affine_rois_normalize(sview, to_dev(ms, dev), wo, ho, mean, std, src_index=d_idx,
                                                 out_layout=out, border_value=border4(dtype), out=dview)
            want = oracle_normalized(oracle, want, mean, std)
            if out == NCHW:
                want = want.transpose(0, 3, 1, 2)
        assert got.data_ptr() == dview.data_ptr()
        assert_bits(host(dview), want, what)
        assert_rim_intact(dbuf, dview, what)
        assert_bits(host(sview), frames, what + ": source")


# ---------------------------------------------------------------------------
# 5. src_index rules

@gpu
def test_rois_null_index_broadcast_and_identity(ops, dev, oracle):
    c, wo, ho = 3, 53, 37
    frames = make_frames(4, H, W, c, np.uint8, 11)
    ms = random_maps(np.random.default_rng(12), 4, W, H, wo, ho)
    # one frame: every ROI reads it
    got = ops.warp_affine_rois(to_dev(frames[:1], dev), to_dev(ms, dev), wo, ho, border_value=BORDER_U8)
    assert_bits(host(got), oracle_rois(oracle, frames, [0] * 4, ms, wo, ho, BORDER_U8[:c], CONSTANT), "broadcast")
    got = ops.warp_affine_rois(to_dev(frames[1], dev), to_dev(ms, dev), wo, ho, border_value=BORDER_U8)  # (h, w, c)
    assert_bits(host(got), oracle_rois(oracle, frames, [1] * 4, ms, wo, ho, BORDER_U8[:c], CONSTANT), "3-d frame")
    # as many frames as ROIs: ROI i reads frame i
    got = ops.warp_affine_rois(to_dev(frames, dev), to_dev(ms, dev), wo, ho, border_value=BORDER_U8)
    assert_bits(host(got), oracle_rois(oracle, frames, [0, 1, 2, 3], ms, wo, ho, BORDER_U8[:c], CONSTANT), "identity")
    # ... and with every matrix equal that is the existing batched call, byte for byte
    same = np.repeat(ms[2:3], 4, 0)
    for dtype in (np.uint8, np.float32):
        fr = to_dev(make_frames(4, H, W, c, dtype, 13), dev)
        for mode in (CONSTANT, WRAP):
            got = ops.warp_affine_rois(fr, to_dev(same, dev), wo, ho, border_mode=mode, border_value=border4(dtype))
            batched = ops.warp_affine(fr, ms[2], wo, ho, border_mode=mode, border_value=border4(dtype))
            assert_bits(host(got), host(batched), f"batched {np.dtype(dtype).name} border {mode}")
    # any other count without an index is refused
    with pytest.raises(ValueError):
        ops.warp_affine_rois(to_dev(frames[:2], dev), to_dev(ms, dev), wo, ho)


@gpu
@pytest.mark.parametrize("dtype", [np.uint8, np.float32], ids=["u8", "f32"])
def test_rois_index_out_of_range_is_all_border(ops, dev, oracle, dtype):
    """src = the middle two images of a four-image allocation: an index the
    kernel failed to guard would show the neighbours' pixels, never leave the
    allocation."""
    c, wo, ho = 3, 37, 21
    big = make_frames(4, 33, 47, c, dtype, 17)
    d_big = to_dev(big, dev)
    src = d_big[1:3]
    idx = [-1, 0, 2, 1, -2 ** 31, 2 ** 31 - 1]
    # every ROI looks at the same, well-covered part of its frame
    ms = np.repeat(np.array([[1.1, 0.2, 3.0, -0.2, 1.1, 2.0]], np.float32), len(idx), 0)
    border = border_of(dtype, c)
    for mode in (CONSTANT, REPLICATE, WRAP):
        got = host(ops.warp_affine_rois(src, to_dev(ms, dev), wo, ho, src_index=to_dev(np.array(idx, np.int32), dev),
                                        border_mode=mode, border_value=border4(dtype)))
        for i, k in enumerate(idx):
            if 0 <= k < 2:
                want = oracle_rois(oracle, big[1:3], [k], ms[i:i + 1], wo, ho, border, mode)[0]
                assert not np.array_equal(want, filled(1, ho, wo, border, dtype)[0]), "the map must hit the frame"
            else:
                want = filled(1, ho, wo, border, dtype)[0]
            assert_bits(got[i], want, f"index {k}, border {mode}")
        gotn = host(ops.warp_affine_rois_normalize(src, to_dev(ms, dev), wo, ho, MEAN[:c], STD[:c],
                                                   src_index=to_dev(np.array(idx, np.int32), dev), out_layout=NCHW,
                                                   border_mode=mode, border_value=border4(dtype)))
        wantn = oracle_normalized(oracle, filled(1, ho, wo, border, dtype), MEAN[:c], STD[:c])[0].transpose(2, 0, 1)
        for i, k in enumerate(idx):
            if not 0 <= k < 2:
                assert_bits(gotn[i], wantn, f"normalize: index {k}, border {mode}")
    assert_bits(host(d_big), big, "source allocation")


# ---------------------------------------------------------------------------
# 6. degenerate matrices

@gpu
@pytest.mark.parametrize("dtype", [np.uint8, np.float32], ids=["u8", "f32"])
def test_rois_degenerate_matrices(ops, dev, oracle, dtype):
    c, wo, ho = 3, 37, 21
    big = make_frames(4, 33, 47, c, dtype, 19)
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
    border = border_of(dtype, c)
    got = host(ops.warp_affine_rois(src, to_dev(ms, dev), wo, ho, src_index=to_dev(np.array(idx, np.int32), dev),
                                    border_value=border4(dtype)))
    for i in (0, 1, 7):
        want = oracle_rois(oracle, big[1:3], [idx[i]], ms[i:i + 1], wo, ho, border, CONSTANT)[0]
        assert_bits(got[i], want, f"matrix {ms[i].tolist()} vs oracle")
    assert not np.array_equal(got[7], filled(1, ho, wo, border, dtype)[0])
    for i in (2, 3, 4, 5, 6):
        assert_bits(got[i], filled(1, ho, wo, border, dtype)[0], f"matrix {ms[i].tolist()}: all border")


# ---------------------------------------------------------------------------
# 7. many ROIs, one ROI

@gpu
def test_rois_many_and_one(ops, dev, oracle):
    c = 3
    frame = make_frames(1, 64, 64, c, np.uint8, 23)
    d_frame = to_dev(frame, dev)
    ms = random_maps(np.random.default_rng(24), 300, 64, 64, 8, 8)
    got = host(ops.warp_affine_rois(d_frame, to_dev(ms, dev), 8, 8, border_value=BORDER_U8))
    want = oracle_rois(oracle, frame, [0] * 300, ms, 8, 8, BORDER_U8[:c], CONSTANT)
    for i in range(300):
        assert_bits(got[i], want[i], f"roi {i} of 300")
    gotn = host(ops.warp_affine_rois_normalize(d_frame, to_dev(ms, dev), 8, 8, MEAN[:c], STD[:c], out_layout=NCHW,
                                               border_value=BORDER_U8))
    assert_bits(gotn, oracle_normalized(oracle, want, MEAN[:c], STD[:c]).transpose(0, 3, 1, 2), "300 planar")
    one = host(ops.warp_affine_rois(d_frame, to_dev(ms[:1], dev), 112, 112, border_value=BORDER_U8))
    assert_bits(one, oracle_rois(oracle, frame, [0], ms[:1], 112, 112, BORDER_U8[:c], CONSTANT), "n_out = 1")


# ---------------------------------------------------------------------------
# 8. the arrays are read when the kernel runs

@gpu
def test_rois_arrays_read_at_execution_time(ops, dev, oracle):
    import torch
    c, wo, ho = 3, 53, 37
    frames = make_frames(3, H, W, c, np.uint8, 29)
    d_frames = to_dev(frames, dev)
    rng = np.random.default_rng(30)
    ms_a, ms_b = random_maps(rng, 7, W, H, wo, ho), random_maps(rng, 7, W, H, wo, ho)
    idx_a, idx_b = np.array(IDX7, np.int32), np.array(IDX7[::-1], np.int32)
    d_ms, d_idx = to_dev(ms_a, dev), to_dev(idx_a, dev)
    d_ms_b, d_idx_b = to_dev(ms_b, dev), to_dev(idx_b, dev)
    out_a = torch.empty((7, ho, wo, c), dtype=torch.uint8, device=dev)
    out_b = torch.empty_like(out_a)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        ops.warp_affine_rois(d_frames, d_ms, wo, ho, src_index=d_idx, out=out_a, stream=stream)
        d_ms.copy_(d_ms_b, non_blocking=True)      # overwritten on the stream, between the two calls,
        d_idx.copy_(d_idx_b, non_blocking=True)    # with no host synchronisation
        ops.warp_affine_rois(d_frames, d_ms, wo, ho, src_index=d_idx, out=out_b, stream=stream)
    stream.synchronize()
    assert_bits(host(out_a), oracle_rois(oracle, frames, idx_a, ms_a, wo, ho, (0, 0, 0), CONSTANT), "first call")
    assert_bits(host(out_b), oracle_rois(oracle, frames, idx_b, ms_b, wo, ho, (0, 0, 0), CONSTANT), "second call")


@gpu
def test_rois_binding_refuses_silent_copies(ops, dev):
    import torch
    frame = to_dev(make_frames(1, 16, 16, 3, np.uint8, 1), dev)
    ms = torch.zeros((4, 6), dtype=torch.float32, device=dev)
    with pytest.raises(ValueError):
        ops.warp_affine_rois(frame, ms.double(), 4, 4)                        # dtype
    with pytest.raises(ValueError):
        ops.warp_affine_rois(frame, torch.zeros((6, 4), device=dev).t(), 4, 4)  # not contiguous
    with pytest.raises(ValueError):
        ops.warp_affine_rois(frame, ms.cpu(), 4, 4)                           # a host tensor
    with pytest.raises(ValueError):
        ops.warp_affine_rois(frame, ms, 4, 4, src_index=torch.zeros(4, dtype=torch.int64, device=dev))
    with pytest.raises(ValueError):
        ops.warp_affine_rois(frame, ms.reshape(8, 3), 4, 4)                   # shape
    # lists and numpy arrays are moved for convenience
    got = ops.warp_affine_rois(frame, [[1, 0, 0, 0, 1, 0]] * 2, 4, 4, src_index=[0, 0])
    assert tuple(got.shape) == (2, 4, 4, 3)
    assert_bits(host(got)[0, :3, :3], host(frame)[0, :3, :3], "identity crop")


# ---------------------------------------------------------------------------
# 9. invert_affine_device

@gpu
def test_invert_affine_device_matches_host(ops, dev):
    rng = np.random.default_rng(0)
    base = rng.uniform(-3, 3, (1024, 6)).astype(np.float32)
    sing = rng.uniform(-3, 3, (1024, 6)).astype(np.float32)
    sing[:512, 3:5] = sing[:512, 0:2] * np.float32(2.0)   # exact zero determinant (a power-of-two multiple)
    sing[512:, [0, 1, 3, 4]] = 0
    ms = np.concatenate([base, base * np.float32(1e-20), base * np.float32(1e15), sing]).astype(np.float32)
    assert ms.shape == (4096, 6)
    want = np.stack([ops.invert_affine(m) for m in ms])
    assert np.array_equal(want[3072:], np.zeros((1024, 6), np.float32)), "the zero-determinant rows invert to zeros"
    got = host(ops.invert_affine_device(to_dev(ms, dev)))
    assert got.shape == (4096, 6) and got.dtype == np.float32
    fin = np.isfinite(want)
    assert fin.sum() > 3 * 4096
    assert np.array_equal(np.isfinite(got), fin), "non-finite results in other positions"
    assert np.array_equal(got.view(np.uint32)[fin], want.view(np.uint32)[fin])
    # (n, 2, 3) in, the same shape out
    got3 = host(ops.invert_affine_device(to_dev(ms.reshape(4096, 2, 3), dev)))
    assert got3.shape == (4096, 2, 3)
    assert np.array_equal(got3.view(np.uint32).reshape(4096, 6)[fin], want.view(np.uint32)[fin])


# ---------------------------------------------------------------------------
# 10. the C++ layer

@gpu
def test_cpp_vector_overloads(hip_device, tmp_path):
    repo = Path(__file__).resolve().parent.parent
    pkg = repo / "arm-neon-opencv_amd"
    lib = pkg / "lib"
    exe = tmp_path / "vacv_rois_test"
    r = subprocess.run(["g++", "-std=c++14", "-O1", str(repo / "tests" / "cpp" / "vacv_rois_test.cpp"), "-o", str(exe),
                        "-I", str(pkg / "src"), "-L", str(lib), "-lvacv", "-lvacv_hip", f"-Wl,-rpath,{lib}"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run(["timeout", "-k", "10", "120", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "failed 0" in r.stdout, r.stdout[-3000:]
