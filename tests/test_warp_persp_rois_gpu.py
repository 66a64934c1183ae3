"""vacv_warp_perspective_rois / _rois_normalize on the GPU: many projective
crops in one launch, each with its own device-resident homography and source
index (csrc/k_warp_persp_rois.hip).

Every comparison of pixels is by bits.  The definition: pixel
(x, y) of ROI i is the single pixel of a 1 x 1 vacv_warp_affine_rois[_normalize]
ROI of the same frame under the inverse-flag map [1 0 fx; 0 1 fy], with (fx, fy)
the float64 coordinates restated here in numpy.  Each case asserts, from those
coordinates alone, how many of its pixels the sampler accepts, so none passes as
all border.
"""
from __future__ import annotations

import subprocess
from pathlib import Path

import numpy as np
import pytest

from test_gpu_plumbing import assert_bits, assert_rim_intact, host, place
from test_warp_rois_gpu import (BORDER_U8, CONSTANT, H, IDX7, MEAN, NCHW, NHWC, REFLECT, REFLECT_101, REPLICATE, STD,
                                W, WRAP, border4, filled, make_frames, to_dev, view_in_buffer)

gpu = pytest.mark.gpu
MODES = (CONSTANT, REPLICATE, REFLECT, WRAP, REFLECT_101)
SIZES = [(37, 53), (65, 5), (5, 3), (1, 1), (40, 30)]  # (wo, ho); 40 x 30 spans two 1,024-pixel tiles
INTER_LINEAR, WARP_INVERSE_MAP = 1, 16


@pytest.fixture(scope="module")
def ops(hip_device):
    from vacv_amd import ops
    return ops


@pytest.fixture(scope="module")
def dev(hip_device):
    return hip_device


# ---------------------------------------------------------------------------
# the reference: numpy float64 coordinates, then the 1 x 1 affine chain

def coords(N, wo, ho):
    """(fx, fy), float32 [n, ho, wo], of the dst -> src maps N [n, 9] float64:
    three rows in double, one reciprocal, two products rounded to float."""
    N = np.asarray(N, np.float64).reshape(-1, 9, 1, 1)
    xd = np.arange(wo, dtype=np.float64)[None, None, :]
    yd = np.arange(ho, dtype=np.float64)[None, :, None]
    with np.errstate(all="ignore"):
        X = (N[:, 0] * xd + N[:, 1] * yd) + N[:, 2]
        Y = (N[:, 3] * xd + N[:, 4] * yd) + N[:, 5]
        Wd = (N[:, 6] * xd + N[:, 7] * yd) + N[:, 8]
        r = 1.0 / Wd
        return (X * r).astype(np.float32), (Y * r).astype(np.float32)


def share(fx, fy, w=W, h=H):
    """The share of pixels that pass affine_tap both ways."""
    with np.errstate(invalid="ignore"):
        return float(((fx >= 0) & (fx < np.float32(w - 1)) & (fy >= 0) & (fy < np.float32(h - 1))).mean())


def chain(ops, d_frames, idx, fx, fy, mode, border, norm=None, layout=NHWC):
    """Every pixel as its own 1 x 1 vacv_warp_affine_rois[_normalize] ROI under [1 0 fx; 0 1 fy] | WARP_INVERSE_MAP."""
    n, ho, wo = fx.shape
    ms = np.zeros((n * ho * wo, 6), np.float32)
    ms[:, 0] = ms[:, 4] = 1
    ms[:, 2], ms[:, 5] = fx.ravel(), fy.ravel()
    dev = d_frames.device
    sidx = to_dev(np.repeat(np.asarray(idx, np.int32), ho * wo), dev)
    kw = dict(src_index=sidx, flags=INTER_LINEAR | WARP_INVERSE_MAP, border_mode=mode, border_value=border)
    if norm is None:
        out = ops.warp_affine_rois(d_frames, to_dev(ms, dev), 1, 1, **kw)
    else:
        out = ops.warp_affine_rois_normalize(d_frames, to_dev(ms, dev), 1, 1, norm[0], norm[1], **kw)
    out = host(out).reshape(n, ho, wo, -1)
    return out.transpose(0, 3, 1, 2) if layout == NCHW else out


def quads_inside(rng, n, w=W, h=H):
    """Rotated boxes (+-30 degrees) with every corner moved by up to 15 % of the side, inside the frame."""
    out = np.zeros((n, 4, 2))
    for i in range(n):
        side = rng.uniform(0.3, 0.55) * min(w, h)
        a = np.deg2rad(rng.uniform(-30, 30))
        R = np.array([[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]])
        box = np.array([[-1, -1], [1, -1], [1, 1], [-1, 1]]) * (side / 2) * (rng.uniform(0.8, 1.4), 1.0)
        c = rng.uniform(0.4, 0.6, 2) * (w, h)
        q = box @ R.T + c + rng.uniform(-0.15, 0.15, (4, 2)) * side
        out[i] = np.clip(q, 0.25, (w - 1.5, h - 1.5))
    return out


def quads_hanging(rng, n, w=W, h=H):
    """The same boxes centred on the frame's border: about half of each hangs off."""
    out = quads_inside(rng, n, w, h)
    for i in range(n):
        c = out[i].mean(0)
        edge = i % 4  # top, right, bottom, left in turn: the top-left corners alone (a 1 x 1 output) are in and out too
        t =np.array([(c[0], 0.0), (w - 1.0, c[1]), (c[0], h - 1.0), (0.0, c[1])][edge])
        out[i] += t - c
    return out


def maps_of(ops, quads, wo, ho):
    """homographies_from_quads (on the host: elementwise torch) -> [n, 9] float32 dst -> src maps.
    A 1-wide or 1-high output takes the first column / row of the 2-wide map."""
    import torch
    return ops.homographies_from_quads(torch.from_numpy(np.asarray(quads, np.float64)), max(wo, 2), max(ho, 2)).numpy()


def case_maps(ops, kind, seed, n, wo, ho):
    rng = np.random.default_rng(seed)
    hs = maps_of(ops, quads_inside(rng, n) if kind == "inside" else quads_hanging(rng, n), wo, ho)
    fx, fy = coords(hs.astype(np.float64), wo, ho)
    s = share(fx, fy)
    if kind == "inside":
        assert s >= 0.9, (kind, seed, wo, ho, s)
    else:
        assert 0.2 <= s <= 0.8, (kind, seed, wo, ho, s)
    return hs, fx, fy


def seed_of(kind, wo, ho, c=0):
    return 20261021 + 1000 * wo + 10 * ho + c + (500000 if kind == "hanging" else 0)


def test_the_seeds_meet_their_shares():
    """No GPU: every (kind, size, c) the cases below draw has its share of sampled pixels."""
    from vacv_amd import ops
    for kind in ("inside", "hanging"):
        for wo, ho in SIZES + [(16, 12), (21, 9)]:
            for c in range(0, 5):
                case_maps(ops, kind, seed_of(kind, wo, ho, c), 7, wo, ho)


# ---------------------------------------------------------------------------
# 1. parity with the 1 x 1 chain

@gpu
@pytest.mark.parametrize("dtype", [np.uint8, np.float32], ids=["u8", "f32"])
@pytest.mark.parametrize("c", [1, 2, 3, 4])
def test_persp_rois_match_the_chain(ops, dev, c, dtype):
    frames = make_frames(3, H, W, c, dtype, 100 + c)
    d_frames = to_dev(frames, dev)
    d_idx = to_dev(np.array(IDX7, np.int32), dev)
    every_mode = (c == 3 and dtype == np.uint8) or (c == 1 and dtype == np.float32)
    for wo, ho in SIZES:
        for kind in ("inside", "hanging"):
            hs, fx, fy = case_maps(ops, kind, seed_of(kind, wo, ho, c), 7, wo, ho)
            for mode in (MODES if every_mode else (CONSTANT,)):
                what = f"c={c} {np.dtype(dtype).name} {wo}x{ho} {kind} border {mode}"
                got = ops.warp_perspective_rois(d_frames, to_dev(hs, dev), wo, ho, src_index=d_idx,
                                                flags=INTER_LINEAR | WARP_INVERSE_MAP, border_mode=mode,
                                                border_value=border4(dtype))
                assert tuple(got.shape) == (7, ho, wo, c) and got.dtype == d_frames.dtype
                want = chain(ops, d_frames, IDX7, fx, fy, mode, border4(dtype))
                got = host(got)
                for i in range(7):
                    assert_bits(got[i], want[i], f"{what} roi {i} h={hs[i].tolist()}")
                if mode == CONSTANT:
                    assert not np.array_equal(got, filled(7, ho, wo, border4(dtype)[:c], dtype)), what + ": all border"
    # (n, 3, 3) is the same array
    got33 = ops.warp_perspective_rois(d_frames, to_dev(hs.reshape(7, 3, 3), dev), wo, ho, src_index=d_idx,
                                      flags=INTER_LINEAR | WARP_INVERSE_MAP, border_value=border4(dtype))
    assert_bits(host(got33), want if not every_mode else chain(ops, d_frames, IDX7, fx, fy, CONSTANT, border4(dtype)),
                "(n, 3, 3)")


# ---------------------------------------------------------------------------
# 2. the reference's own loops, pixel by pixel

@gpu
@pytest.mark.parametrize("dtype", [np.uint8, np.float32], ids=["u8", "f32"])
def test_persp_rois_match_the_reference_loops(ops, dev, oracle, dtype):
    from oracle import Reference
    c, wo, ho, n = 3, 16, 12, 3
    frames = make_frames(3, H, W, c, dtype, 41)
    border = border4(dtype)[:c]
    if Reference.available():  # warp_affine_naive.cpp itself, compiled
        ref = Reference()

        def one_pixel(img, inv):
            return ref.warp_affine_inv(img, inv, 1, 1, border=border)
    else:  # its C restatement, which inverts the forward map [1 0 -fx; 0 1 -fy] to exactly [1 0 fx; 0 1 fy]
        def one_pixel(img, inv):
            fwd = np.array([1, 0, -inv[2], 0, 1, -inv[5]], np.float32)
            assert np.array_equal(oracle.invert_affine(fwd), inv)
            return oracle.warp_affine(img, fwd, 1, 1, border=border)
    for kind in ("inside", "hanging"):
        hs, fx, fy = case_maps(ops, kind, seed_of(kind, wo, ho), 7, wo, ho)
        hs, fx, fy = hs[:n], fx[:n], fy[:n]
        got = host(ops.warp_perspective_rois(to_dev(frames, dev), to_dev(hs, dev), wo, ho,
                                             src_index=to_dev(np.array(IDX7[:n], np.int32), dev),
                                             flags=INTER_LINEAR | WARP_INVERSE_MAP, border_value=border4(dtype)))
        want = np.zeros_like(got)
        for i in range(n):
            for y in range(ho):
                for x in range(wo):
                    inv = np.array([1, 0, fx[i, y, x], 0, 1, fy[i, y, x]], np.float32)
                    want[i, y, x] = one_pixel(frames[IDX7[i]], inv).reshape(c)
        assert_bits(got, want, f"{kind} {np.dtype(dtype).name} vs warp_affine_naive's loops")


# ---------------------------------------------------------------------------
# 3. forward maps are inverted in float64

@gpu
@pytest.mark.parametrize("dtype", [np.uint8, np.float32], ids=["u8", "f32"])
def test_persp_rois_forward_maps_invert_in_fp64(ops, dev, dtype):
    c, wo, ho = 3, 37, 53
    frames = make_frames(3, H, W, c, dtype, 43)
    d_frames, d_idx = to_dev(frames, dev), to_dev(np.array(IDX7, np.int32), dev)
    for kind in ("inside", "hanging"):
        inv_maps, _, _ = case_maps(ops, kind, seed_of(kind, wo, ho, 3), 7, wo, ho)
        fwd = np.stack([np.linalg.inv(m.reshape(3, 3).astype(np.float64)).reshape(9) for m in inv_maps])
        fwd = (fwd / fwd[:, 8:9]).astype(np.float32)
        N = np.stack([ops.invert_homography(m) for m in fwd])
        assert N.dtype == np.float64
        fx, fy = coords(N, wo, ho)
        s = share(fx, fy)
        assert s >= 0.9 if kind == "inside" else 0.2 <= s <= 0.8, s
        fx32, fy32 = coords(N.astype(np.float32).astype(np.float64), wo, ho)
        differ = ((fx != fx32) | (fy != fy32)).mean()
        assert differ > 0.1, f"the float32 inverse must give other coordinates ({differ:.3f})"
        for mode in (CONSTANT, REFLECT_101):
            got = host(ops.warp_perspective_rois(d_frames, to_dev(fwd, dev), wo, ho, src_index=d_idx,
                                                 flags=INTER_LINEAR, border_mode=mode, border_value=border4(dtype)))
            assert_bits(got, chain(ops, d_frames, IDX7, fx, fy, mode, border4(dtype)), f"forward {kind} border {mode}")
            if dtype == np.float32:  # fp32 pixels move with every ulp of a coordinate; 11-bit u8 weights seldom do
                assert not np.array_equal(got, chain(ops, d_frames, IDX7, fx32, fy32, mode, border4(dtype))), \
                    "a float32 inverse would have passed"


# ---------------------------------------------------------------------------
# 4. fused normalize

@gpu
@pytest.mark.parametrize("dtype", [np.uint8, np.float32], ids=["u8", "f32"])
@pytest.mark.parametrize("c,layout", [(3, NHWC), (3, NCHW), (1, NHWC), (1, NCHW)])
def test_persp_rois_normalize(ops, dev, c, layout, dtype):
    import torch
    frames = make_frames(3, H, W, c, dtype, 200 + c)
    d_frames, d_idx = to_dev(frames, dev), to_dev(np.array(IDX7, np.int32), dev)
    mean, std = MEAN[:c], STD[:c]
    for wo, ho in [(37, 53), (5, 3), (40, 30)]:
        for kind in ("inside", "hanging"):
            hs, fx, fy = case_maps(ops, kind, seed_of(kind, wo, ho, c), 7, wo, ho)
            for mode in (CONSTANT, REPLICATE):
                what = f"c={c} layout {layout} {np.dtype(dtype).name} {wo}x{ho} {kind} border {mode}"
                got = ops.warp_perspective_rois_normalize(d_frames, to_dev(hs, dev), wo, ho, mean, std,
                                                          src_index=d_idx, out_layout=layout,
                                                          flags=INTER_LINEAR | WARP_INVERSE_MAP, border_mode=mode,
                                                          border_value=border4(dtype))
                assert got.dtype == torch.float32
                assert tuple(got.shape) == ((7, ho, wo, c) if layout == NHWC else (7, c, ho, wo))
                want = chain(ops, d_frames, IDX7, fx, fy, mode, border4(dtype), (mean, std), layout)
                assert_bits(host(got), want, what)


# ---------------------------------------------------------------------------
# 5. placement

@gpu
@pytest.mark.parametrize("dtype", [np.uint8, np.float32], ids=["u8", "f32"])
def test_persp_rois_dense_at_every_offset(ops, dev, dtype):
    c, n = 3, 7
    frames = make_frames(3, H, W, c, dtype, 300)
    d_frames, d_idx = to_dev(frames, dev), to_dev(np.array(IDX7, np.int32), dev)
    for wo, ho in [(37, 53), (5, 3)]:  # 1,961 pixels: two tiles, the second starts mid-row
        hs, fx, fy = case_maps(ops, "inside", seed_of("inside", wo, ho, 3), n, wo, ho)
        want = chain(ops, d_frames, IDX7, fx, fy, CONSTANT, border4(dtype))
        wantn = chain(ops, d_frames, IDX7, fx, fy, CONSTANT, border4(dtype), (MEAN[:c], STD[:c]), NCHW)
        for off in (range(16) if dtype == np.uint8 else (0, 4, 8, 12)):
            what = f"{np.dtype(dtype).name} {wo}x{ho} dense at +{off}"
            dbuf, dview = view_in_buffer((n, ho, wo, c), (ho * wo * c, wo * c, c, 1), off, dtype, dev)
            ops.warp_perspective_rois(d_frames, to_dev(hs, dev), wo, ho, src_index=d_idx,
                                      flags=INTER_LINEAR | WARP_INVERSE_MAP, border_value=border4(dtype), out=dview)
            assert_bits(host(dview), want, what)
            assert_rim_intact(dbuf, dview, what)
            if off % 4 == 0:
                dbuf, dview = view_in_buffer((n, c, ho, wo), (c * ho * wo, ho * wo, wo, 1), off, np.float32, dev)
                ops.warp_perspective_rois_normalize(d_frames, to_dev(hs, dev), wo, ho, MEAN[:c], STD[:c],
                                                    src_index=d_idx, out_layout=NCHW,
                                                    flags=INTER_LINEAR | WARP_INVERSE_MAP,
                                                    border_value=border4(dtype), out=dview)
                assert_bits(host(dview), wantn, what + " planar")
                assert_rim_intact(dbuf, dview, what + " planar")


PITCH_CASES = [
    # dtype, c, out ("same" | NHWC | NCHW normalize), src off, src row pad, dst off, dst row pad, plane pad, batch pad
    (np.uint8, 3, "same", 3, 2, 16, 0, 0, 5),     # dense rows, ROIs 5 bytes apart
    (np.uint8, 3, "same", 1, 7, 0, 7, 0, 11),     # pitched rows: 16-, 4-byte and byte runs
    (np.uint8, 1, "same", 3, 3, 2, 3, 0, 2),
    (np.uint8, 4, "same", 1, 4, 4, 4, 0, 4),
    (np.uint8, 3, NCHW, 3, 0, 8, 3, 5, 7),        # row, plane and batch padding
    (np.uint8, 3, NHWC, 0, 9, 12, 2, 0, 3),
    (np.float32, 3, "same", 4, 1, 8, 5, 0, 9),
    (np.float32, 3, NCHW, 4, 2, 12, 1, 3, 2),
    (np.float32, 2, "same", 0, 0, 4, 3, 0, 1),
]


@gpu
@pytest.mark.parametrize("case", PITCH_CASES, ids=lambda t: f"{np.dtype(t[0]).name}-c{t[1]}-{t[2]}-s{t[3]}_{t[4]}-d{t[5]}_{t[6]}_{t[7]}_{t[8]}")
def test_persp_rois_pitched(ops, dev, case):
    dtype, c, out, soff, spad, doff, rpad, ppad, bpad = case
    frames = make_frames(3, H, W, c, dtype, 300 + c)
    sbuf, sview = place(frames, dev, NHWC, off=soff, row_pad=spad, batch_pad=spad)
    d_frames, d_idx = to_dev(frames, dev), to_dev(np.array(IDX7, np.int32), dev)
    mean, std = MEAN[:c], STD[:c]
    for wo, ho in [(37, 53), (5, 3)]:
        hs, fx, fy = case_maps(ops, "hanging", seed_of("hanging", wo, ho, c), 7, wo, ho)
        odt = dtype if out == "same" else np.float32
        if out == NCHW:
            rp = wo + rpad
            pl = ho * rp + ppad
            dbuf, dview = view_in_buffer((7, c, ho, wo), (c * pl + bpad, pl, rp, 1), doff, odt, dev)
        else:
            rp = wo * c + rpad
            dbuf, dview = view_in_buffer((7, ho, wo, c), (ho * rp + bpad, rp, c, 1), doff, odt, dev)
        what = f"{case} {wo}x{ho}"
        kw = dict(src_index=d_idx, flags=INTER_LINEAR | WARP_INVERSE_MAP, border_value=border4(dtype), out=dview)
        if out == "same":
            got = ops.warp_perspective_rois(sview, to_dev(hs, dev), wo, ho, **kw)
            want = chain(ops, d_frames, IDX7, fx, fy, CONSTANT, border4(dtype))
        else:
            got = ops.warp_perspective_rois_normalize(sview, to_dev(hs, dev), wo, ho, mean, std, out_layout=out, **kw)
            want = chain(ops, d_frames, IDX7, fx, fy, CONSTANT, border4(dtype), (mean, std), out)
        assert got.data_ptr() == dview.data_ptr()
        assert_bits(host(dview), want, what)
        assert_rim_intact(dbuf, dview, what)
        assert_bits(host(sview), frames, what + ": source")


@gpu
@pytest.mark.parametrize("c", [1, 3, 4])
def test_persp_rois_frame_at_the_end_of_its_allocation(ops, dev, c):
    """The quad covers the frame up to its last row and column: the taps of the
    last pixel are the last bytes of the allocation, at every base offset."""
    import torch
    h, w, wo, ho = 33, 47, 21, 9
    frame = make_frames(1, h, w, c, np.uint8, 77)
    quad = np.array([[[0.0, 0.0], [w - 1.25, 0.0], [w - 1.25, h - 1.25], [0.0, h - 1.25]]])
    hs = maps_of(ops, quad, wo, ho)
    fx, fy = coords(hs.astype(np.float64), wo, ho)
    assert share(fx, fy, w, h) == 1.0 and int(np.floor(fx.max())) == w - 2 and int(np.floor(fy.max())) == h - 2
    want = chain(ops, to_dev(frame, dev), [0], fx, fy, CONSTANT, BORDER_U8)
    for off in range(4):
        buf = torch.empty(off + frame.size, dtype=torch.uint8, device=dev)  # nothing after the last pixel
        view = buf[off:].view(1, h, w, c)
        view.copy_(to_dev(frame, dev))
        got = ops.warp_perspective_rois(view, to_dev(hs, dev), wo, ho, flags=INTER_LINEAR | WARP_INVERSE_MAP,
                                        border_value=BORDER_U8)
        assert_bits(host(got), want, f"c={c} frame at +{off}")


# ---------------------------------------------------------------------------
# 6. more than 256 ROIs

@gpu
def test_persp_rois_many(ops, dev):
    c, n, wo, ho = 3, 301, 5, 3  # 301 workgroups: not a multiple of the 8 XCDs
    frames = make_frames(3, H, W, c, np.uint8, 23)
    d_frames = to_dev(frames, dev)
    idx = (np.arange(n) % 3).astype(np.int32)
    rng = np.random.default_rng(24)
    hs = maps_of(ops, quads_inside(rng, n), wo, ho)
    fx, fy = coords(hs.astype(np.float64), wo, ho)
    assert share(fx, fy) >= 0.9
    got = host(ops.warp_perspective_rois(d_frames, to_dev(hs, dev), wo, ho, src_index=to_dev(idx, dev),
                                         flags=INTER_LINEAR | WARP_INVERSE_MAP, border_value=BORDER_U8))
    want = chain(ops, d_frames, idx, fx, fy, CONSTANT, BORDER_U8)
    for i in range(n):
        assert_bits(got[i], want[i], f"roi {i} of {n}")
    gotn = host(ops.warp_perspective_rois_normalize(d_frames, to_dev(hs, dev), wo, ho, MEAN[:c], STD[:c],
                                                    src_index=to_dev(idx, dev), out_layout=NCHW,
                                                    flags=INTER_LINEAR | WARP_INVERSE_MAP, border_value=BORDER_U8))
    assert_bits(gotn, chain(ops, d_frames, idx, fx, fy, CONSTANT, BORDER_U8, (MEAN[:c], STD[:c]), NCHW), "planar")


# ---------------------------------------------------------------------------
# 7. device-supplied values cannot fault

@gpu
@pytest.mark.parametrize("dtype", [np.uint8, np.float32], ids=["u8", "f32"])
def test_persp_rois_index_out_of_range_is_all_border(ops, dev, dtype):
    """src = the middle two images of a four-image allocation: an index the
    kernel failed to guard would show the neighbours' pixels, never leave the
    allocation."""
    c, wo, ho = 3, 21, 9
    big = make_frames(4, 33, 47, c, dtype, 17)
    d_big = to_dev(big, dev)
    src = d_big[1:3]
    idx = [-1, 0, 2, 1, -2 ** 31, 2 ** 31 - 1]
    quad = np.repeat(np.array([[[4.0, 3.0], [40.0, 5.0], [38.0, 28.0], [6.0, 25.0]]]), len(idx), 0)
    hs = maps_of(ops, quad, wo, ho)
    fx, fy = coords(hs.astype(np.float64), wo, ho)
    assert share(fx, fy, 47, 33) == 1.0
    border = border4(dtype)[:c]
    for mode in MODES:
        d_idx = to_dev(np.array(idx, np.int32), dev)
        got = host(ops.warp_perspective_rois(src, to_dev(hs, dev), wo, ho, src_index=d_idx,
                                             flags=INTER_LINEAR | WARP_INVERSE_MAP, border_mode=mode,
                                             border_value=border4(dtype)))
        want = chain(ops, src, idx, fx, fy, mode, border4(dtype))
        for i, k in enumerate(idx):
            if not 0 <= k < 2:
                assert_bits(got[i], filled(1, ho, wo, border, dtype)[0], f"index {k}, border {mode}")
            else:
                assert not np.array_equal(got[i], filled(1, ho, wo, border, dtype)[0])
            assert_bits(got[i], want[i], f"index {k}, border {mode} vs the chain")
        gotn = host(ops.warp_perspective_rois_normalize(src, to_dev(hs, dev), wo, ho, MEAN[:c], STD[:c],
                                                        src_index=d_idx, out_layout=NCHW,
                                                        flags=INTER_LINEAR | WARP_INVERSE_MAP, border_mode=mode,
                                                        border_value=border4(dtype)))
        assert_bits(gotn, chain(ops, src, idx, fx, fy, mode, border4(dtype), (MEAN[:c], STD[:c]), NCHW),
                    f"normalize, border {mode}")
    assert_bits(host(d_big), big, "source allocation")


@gpu
@pytest.mark.parametrize("dtype", [np.uint8, np.float32], ids=["u8", "f32"])
def test_persp_rois_degenerate_maps(ops, dev, dtype):
    c, wo, ho = 3, 21, 9
    big = make_frames(4, 33, 47, c, dtype, 19)
    src = to_dev(big, dev)[1:3]
    inf, nan = np.inf, np.nan
    hs = np.array([[0] * 9,                                         # W == 0 everywhere / a zero determinant
                   [nan] * 9,
                   [1, nan, 0, 0, 1, 0, 0, 0, 1],
                   [1, 0, 0, 0, 1, 0, nan, 0, 1],
                   [inf, 0, 0, 0, 1, 0, 0, 0, 1],
                   [1, 0, -inf, 0, 1, 0, 0, 0, 1],
                   [1, 0, 0, 0, 1, 0, 0, inf, 1],
                   [1, 2, 3, 2, 4, 6, 0.5, 0.25, 1],                # singular: inverts to zeros
                   [1.5, 0.1, 2, -0.1, 1.2, 3, -0.125, 0, 1],       # W changes sign inside the ROI, through 0 at x = 8
                   [1.5, 0.1, 2, -0.1, 1.2, 3, 0.02, -0.25, 1.0],   # ... and between two rows
                   [1.4, 0.1, 2.0, -0.1, 1.3, 1.5, 0.004, 0.006, 1]], np.float32)  # an ordinary one among them
    idx = [i % 2 for i in range(len(hs))]
    d_idx = to_dev(np.array(idx, np.int32), dev)
    border = border4(dtype)[:c]
    for inverse in (True, False):
        N = hs.astype(np.float64) if inverse else np.stack([ops.invert_homography(m) for m in hs])
        fx, fy = coords(N, wo, ho)
        if inverse:
            assert np.isinf(fx[8, 0, 8]) and fx[8, 0, 7] > 0 > fx[8, 0, 9]
            assert share(fx[10:], fy[10:], 47, 33) > 0.9
        else:
            assert not N[0].any() and not N[7].any()
        for mode in MODES:
            what = f"{'inverse' if inverse else 'forward'} maps, border {mode}"
            got = host(ops.warp_perspective_rois(src, to_dev(hs, dev), wo, ho, src_index=d_idx,
                                                 flags=INTER_LINEAR | (WARP_INVERSE_MAP if inverse else 0),
                                                 border_mode=mode, border_value=border4(dtype)))
            want = chain(ops, src, idx, fx, fy, mode, border4(dtype))
            for i in range(len(hs)):
                assert_bits(got[i], want[i], f"{what}, map {hs[i].tolist()}")
            if mode == CONSTANT:
                for i in ((0, 1, 2, 3) if inverse else (0, 1, 7)):
                    assert_bits(got[i], filled(1, ho, wo, border, dtype)[0], f"{what}, map {i}: all border")
                if inverse:
                    assert not np.array_equal(got[10], filled(1, ho, wo, border, dtype)[0])


# ---------------------------------------------------------------------------
# 8. homographies_from_quads

@gpu
def test_homographies_from_quads_land_on_the_quads(ops, dev):
    """0.01 px for frames up to 2048: nine float32 coefficients, 2^-24 relative
    each, coordinates <= 2048, a handful of terms (about 5e-4 px), 20x margin."""
    import torch
    rng = np.random.default_rng(8)
    for fw, fh, wo, ho in [(131, 97, 37, 53), (2048, 2048, 112, 112), (1920, 1080, 140, 210), (640, 480, 2, 2)]:
        quads = np.concatenate([quads_inside(rng, 100, fw, fh), quads_hanging(rng, 100, fw, fh)])
        d_quads = to_dev(quads.astype(np.float32), dev)
        hs = ops.homographies_from_quads(d_quads, wo, ho)
        assert hs.device == d_quads.device and hs.dtype == torch.float32 and tuple(hs.shape) == (200, 9)
        hm = host(hs).astype(np.float64).reshape(200, 3, 3)
        corners = np.array([[0, 0, 1], [wo - 1, 0, 1], [wo - 1, ho - 1, 1], [0, ho - 1, 1]], np.float64)
        p = np.einsum("nij,kj->nki", hm, corners)
        err = np.abs(p[..., :2] / p[..., 2:] - quads.astype(np.float32).astype(np.float64)).max()
        print(f"homographies_from_quads {fw}x{fh} -> {wo}x{ho}: worst corner error {err:.3g} px")
        assert err <= 0.01, (fw, fh, wo, ho, err)
    with pytest.raises(ValueError):
        ops.homographies_from_quads(d_quads, 1, 4)
    with pytest.raises(ValueError):
        ops.homographies_from_quads(d_quads.reshape(200, 8), 4, 4)


@gpu
def test_persp_rois_binding_refuses_silent_copies(ops, dev):
    import torch
    frame = to_dev(make_frames(1, 16, 16, 3, np.uint8, 1), dev)
    hs = torch.zeros((4, 9), dtype=torch.float32, device=dev)
    with pytest.raises(ValueError):
        ops.warp_perspective_rois(frame, hs.double(), 4, 4)
    with pytest.raises(ValueError):
        ops.warp_perspective_rois(frame, hs.cpu(), 4, 4)
    with pytest.raises(ValueError):
        ops.warp_perspective_rois(frame, hs.reshape(6, 6), 4, 4)
    with pytest.raises(ValueError):
        ops.warp_perspective_rois(frame, hs.reshape(4, 9), 4, 4, src_index=torch.zeros(3, dtype=torch.int32, device=dev))
    with pytest.raises(ValueError):
        ops.warp_perspective_rois_normalize(frame, hs, 4, 4, None, None)
    got = ops.warp_perspective_rois(frame, [[1, 0, 0, 0, 1, 0, 0, 0, 1]] * 2, 4, 4, src_index=[0, 0])
    assert tuple(got.shape) == (2, 4, 4, 3)
    assert_bits(host(got)[0, :3, :3], host(frame)[0, :3, :3], "identity crop")


# ---------------------------------------------------------------------------
# 9. the C++ layer

@gpu
def test_cpp_warp_perspective(hip_device, tmp_path):
    repo = Path(__file__).resolve().parent.parent
    pkg = repo / "arm-neon-opencv_amd"
    lib = pkg / "lib"
    exe = tmp_path / "vacv_warp_persp_test"
    r = subprocess.run(["g++", "-std=c++14", "-O1", str(repo / "tests" / "cpp" / "vacv_warp_persp_test.cpp"), "-o",
                        str(exe), "-I", str(pkg / "src"), "-I", str(repo / "include"), "-L", str(lib), "-lvacv",
                        "-lvacv_hip", f"-Wl,-rpath,{lib}"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run(["timeout", "-k", "10", "120", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "failed 0" in r.stdout, r.stdout[-3000:]
