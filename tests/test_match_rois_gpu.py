"""vacv_match_template_rois on the GPU: many templates matched in per-object
search windows in one launch, with each result's peaks
(csrc/k_match_rois.hip).

No assertion is a tolerance.  Every case is compared, bit for bit, with two
references:
  A  the contract: the product's own single calls, ops.match_template(ops.crop(
     frame, window), template, method) and ops.min_max_idx of it, per ROI;
  B  independent: ref_window_sums / ref_formula of tests/test_gpu_match.py on
     the numpy crop, and numpy's first-occurrence argmin / argmax.
The shapes are the smallest at which this kernel can go wrong: a 1 x 1 template
and result, a window equal to the template, template rows that are no whole
dwords, a result row of 65 (one past a wave), results of 257 elements and of
257 four-column items (one past a workgroup's single pass), more ROIs than CUs.
"""
from __future__ import annotations

import ctypes
import subprocess
from pathlib import Path

import numpy as np
import pytest

from test_gpu_match import ref_formula, ref_min_max_idx, ref_window_sums
from test_gpu_plumbing import SENTINEL, assert_bits, assert_rim_intact, assert_untouched, blank, host, place, unsupported

gpu = pytest.mark.gpu
SQDIFF, SQDIFF_NORMED, CCORR, CCORR_NORMED, CCOEFF, CCOEFF_NORMED = range(6)  # include/vacv_hip.h VACV_TM_*
ALL = tuple(range(6))
INT32_MAX = 2 ** 31 - 1


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


def rand_u8(shape, seed):
    return np.random.default_rng(seed).integers(0, 256, shape, dtype=np.uint8)


def frame_of(i, idx, n_src):
    return int(idx[i]) if idx is not None else (0 if n_src == 1 else i)


def want_numpy(frames, tpls, origins, idx, w, h, method):
    """Reference B: (maps, vals, peaks) of every ROI from the numpy crops."""
    maps, vals, peaks = [], [], []
    for i, (l, t) in enumerate(np.asarray(origins).tolist()):
        tpl = tpls[i if len(tpls) > 1 else 0]
        crop = frames[frame_of(i, idx, len(frames))][t:t + h, l:l + w]
        m = ref_formula(ref_window_sums(crop, tpl), tpl, method)
        mn, mx, imn, imx = ref_min_max_idx(m)
        maps.append(m)
        vals.append([mn, mx])
        peaks.append([*imn, *imx])
    return np.stack(maps), np.array(vals, np.float64), np.array(peaks, np.int32)


def want_single(ops, d_frames, d_tpls, origins, idx, w, h, method):
    """Reference A: the same from the product's single calls on the device tensors."""
    maps, vals, peaks = [], [], []
    for i, (l, t) in enumerate(np.asarray(origins).tolist()):
        k = frame_of(i, idx, d_frames.shape[0])
        tpl = d_tpls[i if d_tpls.shape[0] > 1 else 0]
        m = ops.match_template(ops.crop(d_frames[k:k + 1], (l, t, l + w, t + h)), tpl, method)[0]
        mn, mx, imn, imx = ops.min_max_idx(m)
        maps.append(host(m))
        vals.append([mn, mx])
        peaks.append([*imn, *imx])
    return np.stack(maps), np.array(vals, np.float64), np.array(peaks, np.int32)


def assert_same(got, want, what):
    for g, w, name in zip(got, want, ("map", "vals", "idx")):
        assert_bits(host(g) if hasattr(g, "cpu") else g, w, f"{what}: {name}")


def check(ops, dev, frames, tpls, origins, idx, w, h, methods, what, single=True):
    """One batched call per method against both references."""
    d_frames, d_tpls = to_dev(frames, dev), to_dev(tpls, dev)
    d_origins = to_dev(np.asarray(origins, np.int32), dev)
    d_idx = to_dev(np.asarray(idx, np.int32), dev) if idx is not None else None
    for method in methods:
        got = ops.match_template_rois(d_frames, d_tpls if len(tpls) > 1 else d_tpls[0], d_origins, w, h, method,
                                      src_index=d_idx)
        assert_same(got, want_numpy(frames, tpls, origins, idx, w, h, method), f"{what} method {method} vs numpy")
        if single:
            assert_same(got, want_single(ops, d_frames, d_tpls, origins, idx, w, h, method),
                        f"{what} method {method} vs the single calls")


# ---------------------------------------------------------------------------
# 1. the shapes, all six methods, per-ROI templates, frames repeated and permuted

#          c  tw th   W    H
SHAPES = [(1, 1, 1, 1, 1),        # a 1 x 1 template and result
          (3, 1, 1, 1, 1),
          (3, 5, 4, 5, 4),        # the window is the template: rw = rh = 1
          (1, 5, 3, 9, 8),        # template rows of 5, 10, 15, 20 bytes: tw c % 4 = 1, 2, 3, 0
          (2, 5, 3, 9, 8),
          (3, 5, 3, 9, 8),
          (4, 5, 3, 9, 8),
          (3, 3, 2, 67, 3),       # a result row of 65: one past a wave
          (1, 2, 2, 258, 2),      # a result of 257 elements
          (2, 2, 3, 4, 259),      # ... and of 257 items of 4 columns (rw = 3): one past a workgroup's pass
          (1, 7, 5, 1031, 5)]     # ... in one row (rw = 1025)


@gpu
@pytest.mark.parametrize("c,tw,th,w,h", SHAPES)
def test_shapes_all_methods(ops, dev, c, tw, th, w, h):
    frames = rand_u8((3, h + 3, w + 5, c), 1000 + 7 * c + tw + w)
    tpls = rand_u8((3, th, tw, c), 2000 + c + w)
    origins = [[0, 0], [5, 3], [2, 1]]  # two corners and an odd byte offset
    check(ops, dev, frames, tpls, origins, [2, 0, 2], w, h, ALL, f"c={c} {tw}x{th} in {w}x{h}")


# ---------------------------------------------------------------------------
# 2. batch sizes, the index rules, shared and per-ROI templates

@gpu
def test_one_roi_and_null_index(ops, dev):
    frames = rand_u8((3, 20, 31, 3), 11)
    tpls = rand_u8((3, 4, 6, 3), 12)
    # n = 1, one frame, no index
    check(ops, dev, frames[:1], tpls[:1], [[7, 3]], None, 13, 11, (SQDIFF, CCOEFF_NORMED), "n=1")
    # no index, frame i for ROI i; per-ROI and shared templates
    origins = [[0, 0], [18, 9], [5, 5]]
    check(ops, dev, frames, tpls, origins, None, 13, 11, (SQDIFF_NORMED, CCORR_NORMED), "frame i, template i")
    check(ops, dev, frames, tpls[:1], origins, None, 13, 11, (CCOEFF,), "frame i, shared template")
    # no index, one frame for all
    check(ops, dev, frames[1:2], tpls, origins, None, 13, 11, (CCORR,), "one frame")


@gpu
@pytest.mark.parametrize("shared", [False, True], ids=["per_roi", "shared"])
def test_more_rois_than_cus(ops, dev, shared):
    """300 ROIs of a tiny 12 x 12 window on 4 frames: overlapping, identical and corner windows."""
    n, w, h = 300, 12, 12
    rng = np.random.default_rng(5)
    frames = rand_u8((4, 40, 50, 3), 21)
    tpls = rand_u8((1 if shared else n, 4, 5, 3), 22)
    origins = np.stack([rng.integers(0, 50 - w + 1, n), rng.integers(0, 40 - h + 1, n)], 1).astype(np.int32)
    origins[10:14] = origins[9]                # identical windows
    origins[20] = [min(origins[19][0] + 1, 50 - w), origins[19][1]]  # overlapping
    origins[0], origins[299] = [0, 0], [50 - w, 40 - h]
    idx = rng.integers(0, 4, n).astype(np.int32)
    idx[10:12] = idx[9]                        # ... two of them in the same frame as well
    check(ops, dev, frames, tpls, origins, idx, w, h, (CCOEFF_NORMED,), f"n=300 shared={shared}")
    check(ops, dev, frames, tpls, origins, idx, w, h, (SQDIFF,), f"n=300 shared={shared}", single=False)


# ---------------------------------------------------------------------------
# 3. placement: odd byte bases, pitched rows and batches, a pitched result

@gpu
@pytest.mark.parametrize("c", [1, 3])
def test_operand_placement(ops, dev, c):
    w, h, tw, th, n = 14, 9, 5, 3, 4
    frames, tpls = rand_u8((2, 17, 23, c), 31 + c), rand_u8((n, th, tw, c), 33 + c)
    origins = np.array([[0, 0], [9, 8], [3, 2], [3, 2]], np.int32)
    idx = np.array([1, 0, 1, 0], np.int32)
    d_origins, d_idx = to_dev(origins, dev), to_dev(idx, dev)
    rw, rh = w - tw + 1, h - th + 1
    for off, row_pad, batch_pad in ((1, 0, 0), (2, 3, 0), (3, 5, 7), (0, 1, 2)):
        _, d_frames = place(frames, dev, off=off, row_pad=row_pad, batch_pad=batch_pad)
        _, d_tpls = place(tpls, dev, off=(off + 1) % 4, row_pad=batch_pad, batch_pad=row_pad)
        buf, out = place(blank((n, rh, rw, 1), np.float32), dev, off=4 * off, row_pad=row_pad, batch_pad=batch_pad)
        for method in (SQDIFF_NORMED, CCOEFF_NORMED):
            what = f"c={c} off={off} pads {row_pad}, {batch_pad} method {method}"
            res, vals, peaks = ops.match_template_rois(d_frames, d_tpls, d_origins, w, h, method, src_index=d_idx,
                                                       out=out[..., 0])
            assert res.data_ptr() == out.data_ptr()
            assert_same((res, vals, peaks), want_numpy(frames, tpls, origins, idx, w, h, method), what)
            assert_same((res, vals, peaks), want_single(ops, d_frames, d_tpls, origins, idx, w, h, method),
                        what + " vs the single calls")
            assert_rim_intact(buf, out, what)  # the rim and the gaps between rows and ROIs


# ---------------------------------------------------------------------------
# 4. degenerate values and known peaks

@gpu
def test_flat_frame_and_flat_template(ops, dev):
    w, h = 11, 9
    flat = np.full((1, 20, 20, 3), 77, np.uint8)
    tpls = rand_u8((1, 3, 4, 3), 41)
    origins = [[0, 0], [6, 7]]
    d_flat, d_origins = to_dev(flat, dev), to_dev(np.array(origins, np.int32), dev)
    for method in ALL:  # every element is equal: both peaks are the first element
        res, vals, peaks = ops.match_template_rois(d_flat, to_dev(tpls[0], dev), d_origins, w, h, method)
        r = host(res)
        assert (r.view(np.uint32) == r.view(np.uint32)[0, 0, 0]).all(), method
        assert host(peaks).tolist() == [[0, 0, 0, 0]] * 2, method
        assert_same((res, vals, peaks), want_numpy(flat, tpls, origins, None, w, h, method), f"flat frame {method}")
    check(ops, dev, flat, tpls, origins, None, w, h, (SQDIFF_NORMED, CCOEFF_NORMED), "flat frame")
    # a flat template under CCOEFF_NORMED: all 1.f
    frames = rand_u8((1, 20, 20, 3), 42)
    ones = np.full((1, 3, 4, 3), 200, np.uint8)
    res, vals, peaks = ops.match_template_rois(to_dev(frames, dev), to_dev(ones[0], dev), d_origins, w, h, CCOEFF_NORMED)
    assert_bits(host(res), np.ones((2, h - 2, w - 3), np.float32), "flat template")
    assert host(vals).tolist() == [[1.0, 1.0]] * 2 and host(peaks).tolist() == [[0, 0, 0, 0]] * 2
    check(ops, dev, frames, ones, origins, None, w, h, ALL, "flat template")
    # all-zero operands
    zeros = np.zeros((1, 20, 20, 3), np.uint8)
    check(ops, dev, zeros, tpls, origins, None, w, h, ALL, "zero frame")
    check(ops, dev, frames, np.zeros((1, 3, 4, 3), np.uint8), origins, None, w, h, ALL, "zero template")


@gpu
def test_planted_template_is_the_peak(ops, dev):
    w, h, tw, th = 24, 20, 6, 5
    frames = rand_u8((2, 40, 48, 3), 51)
    tpls = rand_u8((3, th, tw, 3), 52)
    origins = np.array([[3, 4], [20, 17], [24, 20]], np.int32)
    idx = np.array([0, 1, 0], np.int32)
    planted = [(7, 11), (0, 0), (h - th, w - tw)]  # (row, col) in the result, its corners included
    for i, (r, c) in enumerate(planted):
        l, t = origins[i]
        frames[idx[i], t + r:t + r + th, l + c:l + c + tw] = tpls[i]
    d = [to_dev(a, dev) for a in (frames, tpls, origins, idx)]
    _, vals, peaks = ops.match_template_rois(d[0], d[1], d[2], w, h, SQDIFF, src_index=d[3])
    assert [p[:2] for p in host(peaks).tolist()] == [list(p) for p in planted]
    # (the minimum itself is 0 only up to templSum2's rounding in double: `check` below has its bits)
    _, vals, peaks = ops.match_template_rois(d[0], d[1], d[2], w, h, CCOEFF_NORMED, src_index=d[3])
    assert [p[2:] for p in host(peaks).tolist()] == [list(p) for p in planted]
    check(ops, dev, frames, tpls, origins, idx, w, h, (SQDIFF, CCOEFF_NORMED), "planted")


# ---------------------------------------------------------------------------
# 5. device-supplied garbage

@gpu
def test_invalid_windows_and_indices(ops, dev):
    w, h, n_src, fh, fw = 10, 8, 2, 20, 30
    frames, tpls = rand_u8((n_src, fh, fw, 3), 61), rand_u8((1, 3, 4, 3), 62)
    #           left        top          frame
    rois = [(4, 5, 0),
            (-1, 0, 0),                  # left = -1
            (fw - w, fh - h, 1),         # the last valid position
            (0, fh - h + 1, 1),          # top + H = src->h + 1
            (INT32_MAX, 0, 0),           # left + W overflows an int
            (3, 3, -1),                  # src_index = -1
            (3, 3, n_src),               # src_index = src->n
            (fw - w + 1, 0, 0),          # left + W = src->w + 1
            (0, -INT32_MAX - 1, 1),
            (0, INT32_MAX, 1),
            (7, 2, INT32_MAX),
            (20, 12, 1)]
    valid = [0, 2, 11]
    origins = np.array([r[:2] for r in rois], np.int32)
    idx = np.array([r[2] for r in rois], np.int32)
    d_frames, d_tpl = to_dev(frames, dev), to_dev(tpls[0], dev)
    for method in (SQDIFF, CCOEFF_NORMED):
        res, vals, peaks = ops.match_template_rois(d_frames, d_tpl, to_dev(origins, dev), w, h, method,
                                                   src_index=to_dev(idx, dev))  # returns: the call answered OK
        res, vals, peaks = host(res), host(vals), host(peaks)
        want = want_numpy(frames, tpls, origins[valid], idx[valid], w, h, method)
        assert_same((res[valid], vals[valid], peaks[valid]), want, f"the valid neighbours, method {method}")
        bad = [i for i in range(len(rois)) if i not in valid]
        assert_bits(res[bad], np.zeros((len(bad), h - 2, w - 3), np.float32), "invalid ROIs are zeros")
        assert_bits(vals[bad], np.zeros((len(bad), 2), np.float64), "their vals")
        assert_bits(peaks[bad], np.full((len(bad), 4), -1, np.int32), "their idx")
    # a window larger than the frame: every ROI is invalid
    res, vals, peaks = ops.match_template_rois(d_frames[0], d_tpl, to_dev(origins[:1] * 0, dev), fw + 1, h, SQDIFF)
    assert not host(res).any() and host(peaks).tolist() == [[-1] * 4]


# ---------------------------------------------------------------------------
# 6. the LDS limit, peaks=False, the Python checks

def lds_need(tw, th, cn, rw, rh):
    """include/vacv_hip.h's formula (csrc/k_match_rois.hip match_rois_lds_bytes), restated."""
    k4 = (tw * cn + 3) // 4
    g = (rw + 3) // 4
    w, h = rw + tw - 1, rh + th - 1
    ws4 = max((w * cn + 3) // 4, (g - 1) * cn + k4 + (3 * cn) // 4 + 2) | 1
    return 256 + 4 * (th * k4 + h * ws4 + h * rw * (cn + 1))


@gpu
def test_lds_limit(ops, dev):
    """A ROI of exactly 64 KiB of LDS is computed; 8 bytes more are refused with nothing written."""
    assert lds_need(2, 9, 3, 51, 58) == 65536 and lds_need(2, 10, 3, 51, 57) == 65544
    w, h = 52, 66
    frames = rand_u8((1, h + 2, w + 3, 3), 71)
    check(ops, dev, frames, rand_u8((2, 9, 2, 3), 72), [[3, 2], [0, 0]], None, w, h, (SQDIFF_NORMED, CCOEFF_NORMED),
          "64 KiB of LDS")
    buf, out = place(blank((2, 57, 51, 1), np.float32), dev)
    d_origins = to_dev(np.array([[3, 2], [0, 0]], np.int32), dev)
    unsupported(lambda: ops.match_template_rois(to_dev(frames, dev), to_dev(rand_u8((2, 10, 2, 3), 73), dev), d_origins,
                                                w, h, CCOEFF_NORMED, out=out[..., 0]))
    assert_untouched(buf, "past the LDS limit")


@gpu
def test_peaks_off_writes_the_same_maps(ops, dev):
    """peaks=False: only the maps, the same bytes; and through the C ABI with
    NULL vals / idx, sentinel-filled buffers standing where they would be."""
    import torch
    from vacv_amd import _lib
    frames, tpls = rand_u8((2, 30, 40, 3), 81), rand_u8((3, 5, 7, 3), 82)
    origins, idx = np.array([[0, 0], [9, 4], [17, 12]], np.int32), np.array([1, 1, 0], np.int32)
    d = [to_dev(a, dev) for a in (frames, tpls, origins, idx)]
    for method in (SQDIFF, CCOEFF_NORMED):
        res, _, _ = ops.match_template_rois(d[0], d[1], d[2], 23, 18, method, src_index=d[3])
        only = ops.match_template_rois(d[0], d[1], d[2], 23, 18, method, src_index=d[3], peaks=False)
        assert isinstance(only, torch.Tensor)
        assert_bits(host(only), host(res), f"peaks=False, method {method}")
    vals = torch.full((3 * 16,), SENTINEL, dtype=torch.uint8, device=dev)
    peaks = torch.full((3 * 16,), SENTINEL, dtype=torch.uint8, device=dev)
    out = torch.full((3, 14, 17), float("nan"), dtype=torch.float32, device=dev)
    by = ctypes.byref
    st = _lib.load().vacv_match_template_rois(by(ops.describe(d[0])), by(ops.describe(d[1])),
                                              by(ops.describe(out.unsqueeze(-1))), d[2].data_ptr(), d[3].data_ptr(),
                                              CCOEFF_NORMED, None, None, torch.cuda.current_stream().cuda_stream)
    assert st == 0
    assert_bits(host(out), host(res), "NULL vals / idx")
    assert_untouched(vals, "vals")
    assert_untouched(peaks, "idx")


@gpu
def test_python_argument_checks(ops, dev):
    import torch
    frame = to_dev(rand_u8((1, 16, 16, 3), 91), dev)
    tpl = to_dev(rand_u8((3, 4, 3), 92), dev)
    origins = torch.tensor([[0, 0], [3, 5]], dtype=torch.int32, device=dev)

    def fn(o, **kw):
        return ops.match_template_rois(frame, tpl, o, 8, 8, CCORR, **kw)

    with pytest.raises(ValueError):
        fn(origins.cpu())                                  # a host tensor: the wrong device
    with pytest.raises(ValueError):
        fn(origins.long())
    with pytest.raises(ValueError):
        fn(origins.reshape(1, 4))                          # shape
    with pytest.raises(ValueError):
        fn(origins, src_index=torch.zeros(2, dtype=torch.int64, device=dev))
    with pytest.raises(ValueError):
        ops.match_template_rois(frame, tpl, origins, 3, 8, CCORR)   # the template is wider than the window
    with pytest.raises(ValueError):
        fn(origins, out=torch.empty((2, 5, 5), dtype=torch.float32, device=dev))
    # lists are moved for convenience; search_origins on the device
    res, vals, peaks = fn([[0, 0], [3, 5]], src_index=[0, 0])
    assert tuple(res.shape) == (2, 6, 5) and tuple(vals.shape) == (2, 2) and tuple(peaks.shape) == (2, 4)
    o = ops.search_origins(torch.tensor([[7.9, 9.0], [100.0, -3.0]], device=dev), 8, 8, 16, 16)
    assert o.device.type == "cuda" and host(o).tolist() == [[3, 5], [8, 0]]
    assert_bits(host(fn(o)[0])[0], host(res)[1], "origins from centres")


# ---------------------------------------------------------------------------
# 7. the C++ layer

@gpu
def test_cpp_match_rois(hip_device, tmp_path):
    repo = Path(__file__).resolve().parent.parent
    pkg = repo / "arm-neon-opencv_amd"
    lib = pkg / "lib"
    exe = tmp_path / "vacv_match_rois_test"
    r = subprocess.run(["g++", "-std=c++14", "-O1", str(repo / "tests" / "cpp" / "vacv_match_rois_test.cpp"), "-o",
                        str(exe), "-I", str(pkg / "src"), "-L", str(lib), "-lvacv", "-lvacv_hip",
                        f"-Wl,-rpath,{lib}"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run(["timeout", "-k", "10", "120", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "failed 0" in r.stdout, r.stdout[-3000:]
