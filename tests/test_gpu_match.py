"""match_template and minMaxIdx (csrc/k_match.hip, vacv_match_template /
vacv_min_max_idx in csrc/vacv_abi.cpp, va_cv::match_template / minMaxIdx in
src/cv/cv.cpp) at the tails, pitches, channel counts and route boundaries that
select their code paths: the MFMA correlation's operand pipeline (every
remainder of its 8-step groups, fewer steps than a group, than a prefetch), the
K-block count's steps, result tiles +-1, cn = 2, the three window-statistics
routes and their boundaries for every cn, operands placed at odd bases with
pitched rows, workspaces reused at other sizes, and the host limits.

The references are plain numpy, independent of the library and of the oracle
(test_references_match_oracle checks them against the oracle's C functions on
the CPU).  No assertion here is a tolerance:
  * u8: every sum is an integer, so the result is the exact correlation
    rounded to float followed by templmatch.cpp's double formula;
  * fp32: all data is k / 8 with |k| <= 1024.  Every product is a multiple of
    1 / 64 below 2^14, so every correlation, window sum, integral-image entry
    and template sum is exact in fp64 in ANY order, and the GPU's other
    summation order cannot change a bit.  A difference on such data is an
    index, a tap or a contraction, never rounding.
All GPU tests carry the gpu mark one by one because that one test must run
without a device.
"""
from __future__ import annotations

import contextlib
import math
import struct
import subprocess
from pathlib import Path

import numpy as np
import pytest
from numpy.lib.stride_tricks import sliding_window_view

from test_gpu_plumbing import (SENTINEL, assert_bits, assert_rim_intact, assert_untouched, blank, host, place,
                               unsupported)

gpu = pytest.mark.gpu
SQDIFF, SQDIFF_NORMED, CCORR, CCORR_NORMED, CCOEFF, CCOEFF_NORMED = range(6)  # include/vacv_hip.h VACV_TM_*
ALL = tuple(range(6))
STATS = (0, 1, 3, 4, 5)  # every method that takes window statistics
U8, F32 = np.dtype(np.uint8), np.dtype(np.float32)


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


def data(rng, shape, dtype):
    """u8: any byte.  fp32: k / 8, |k| <= 1024 -- the exact-sum data of the module docstring."""
    if np.dtype(dtype) == U8:
        return rng.integers(0, 256, shape, dtype=np.uint8)
    return (rng.integers(-1024, 1025, shape) / 8).astype(np.float32)


# ---------------------------------------------------------------------------
# numpy references (independent of the library and of the oracle)

def _hwc(a):
    a = np.asarray(a)
    return a[..., None] if a.ndim == 2 else a


def ref_window_sums(img, tpl):
    """(corr, S, Q) of every window: the correlation with the template, the
    per-channel sums S[y, x, c] and the sum of squares over all channels --
    int64 for u8, float64 for fp32 (exact for this module's data)."""
    img, tpl = _hwc(img), _hwc(tpl)
    wide = np.int64 if img.dtype == U8 else np.float64
    im, tp = img.astype(wide), tpl.astype(wide)
    h, w, _ = tp.shape
    win = sliding_window_view(im, (h, w), axis=(0, 1))  # (rh, rw, c, h, w), a view
    corr = np.einsum("yxcij,ijc->yx", win, tp)
    s = np.einsum("yxcij->yxc", win)
    q = np.einsum("yxcij->yx", sliding_window_view(im * im, (h, w), axis=(0, 1)))
    return corr, s.astype(np.float64), q.astype(np.float64)


def ref_formula(sums, tpl, method):
    """templmatch.cpp's normalisation in float64, in the operation order of
    oracle_match_template, of the float-rounded correlation."""
    corr, S, Q = sums
    tpl = _hwc(tpl)
    h, w, cn = tpl.shape
    n = h * w
    t64 = tpl.reshape(n, cn).astype(np.float64)
    tm, td = [0.0] * 4, [0.0] * 4
    for c in range(cn):  # meanStdDev: population
        s, q = math.fsum(t64[:, c]), math.fsum(t64[:, c] * t64[:, c])
        tm[c] = s / n
        var = q / n - tm[c] * tm[c]
        td[c] = math.sqrt(var) if var > 0 else 0.0
    inv_area = 1.0 / (float(h) * w)
    num_type = 0 if method in (CCORR, CCORR_NORMED) else 1 if method in (CCOEFF, CCOEFF_NORMED) else 2
    normed = method in (SQDIFF_NORMED, CCORR_NORMED, CCOEFF_NORMED)
    num = corr.astype(np.float32).astype(np.float64)  # crossCorr's float result, widened back
    if method == CCORR:
        return num.astype(np.float32)
    templ_norm = templ_sum2 = 0.0
    tmean = list(tm)
    if method != CCOEFF:
        templ_norm = td[0] * td[0] + td[1] * td[1] + td[2] * td[2] + td[3] * td[3]
        if templ_norm < 2.220446049250313e-16 and method == CCOEFF_NORMED:
            return np.ones(corr.shape, np.float32)
        templ_sum2 = templ_norm + tm[0] * tm[0] + tm[1] * tm[1] + tm[2] * tm[2] + tm[3] * tm[3]
        if num_type != 1:
            tmean = [0.0] * 4
            templ_norm = templ_sum2
        templ_sum2 /= inv_area
        templ_norm = math.sqrt(templ_norm)
        templ_norm /= math.sqrt(inv_area)
    wnd_mean2 = np.zeros(corr.shape, np.float64)
    wnd_sum2 = np.zeros(corr.shape, np.float64)
    if num_type == 1:
        for c in range(cn):
            t = S[..., c]
            wnd_mean2 = wnd_mean2 + t * t
            num = num - t * tmean[c]
        wnd_mean2 = wnd_mean2 * inv_area
    if normed or num_type == 2:
        wnd_sum2 = Q
        if num_type == 2:
            num = wnd_sum2 - 2 * num + templ_sum2
            num = np.where(num > 0, num, 0.0)
    if normed:
        d = wnd_sum2 - wnd_mean2
        t = np.sqrt(np.where(d > 0, d, 0.0)) * templ_norm
        with np.errstate(divide="ignore", invalid="ignore"):
            quot = num / t
        sign = np.where(num > 0, 1.0, -1.0)
        num = np.where(np.abs(num) < t, quot,
                       np.where(np.abs(num) < t * 1.125, sign, 1.0 if method == SQDIFF_NORMED else 0.0))
    return num.astype(np.float32)


def ref_match_template(img, tpl, method):
    """cv::matchTemplate (OpenCV 2.4 templmatch.cpp) of img[h, w, c] with the
    exact correlation: (H - h + 1, W - w + 1) fp32."""
    return ref_formula(ref_window_sums(img, tpl), tpl, method)


def ref_methods(imgs, tpl, methods):
    """{method: (n, rh, rw)} of a batch against one template; the window sums once per image."""
    sums = [ref_window_sums(im, tpl) for im in imgs]
    return {m: np.stack([ref_formula(s, tpl, m) for s in sums]) for m in methods}


def ref_min_max_idx(a, mask=None):
    """cv::minMaxIdx: the first row-major minimum / maximum among the unmasked,
    non-NaN elements; none -> (0.0, 0.0, (-1, -1), (-1, -1))."""
    a = np.asarray(a)
    v = a.astype(np.float64).ravel()
    ok = ~np.isnan(v)
    if mask is not None:
        ok &= np.asarray(mask).ravel() != 0
    idx = np.flatnonzero(ok)
    if idx.size == 0:
        return 0.0, 0.0, (-1, -1), (-1, -1)
    imn, imx = int(idx[np.argmin(v[idx])]), int(idx[np.argmax(v[idx])])  # argmin / argmax: the first
    w = a.shape[1]
    return float(v[imn]), float(v[imx]), (imn // w, imn % w), (imx // w, imx % w)


def mm_key(r):
    """A minMaxIdx result with its values as bit patterns: -0.0 is not +0.0."""
    mn, mx, imn, imx = r
    return struct.pack("<dd", mn, mx), tuple(int(i) for i in imn), tuple(int(i) for i in imx)


# ---------------------------------------------------------------------------
# the launcher's plan restated (csrc/k_match.hip: match_mfma_plan,
# match_lds_bytes, launch_match_template), so a case can assert the path it is
# meant to reach and a later change of the plan cannot silently move it

def mfma_plan(tw, th, cn):
    """(KB, stride, fits): K blocks per template row, LDS row stride, and
    whether the matrix-core correlation takes the template."""
    K = tw * cn
    KB = (cn * 31 + K + 31) // 32
    stride = (cn * 32 + KB * 32 + 15) // 16 * 16
    return KB, stride, (63 + th) * stride <= 64 * 1024 and K * th <= (1 << 19)


def lds_bytes(tw, th, cn, esize):
    if esize == 1:
        K4 = (tw * cn + 3) // 4
        span4 = 64 * cn + K4 + (3 * cn) // 4 + 2 + 1
        return (th * K4 + 4 * span4) * 4
    return (th * tw * cn + 4 * (256 + tw - 1) * cn) * 4


def stats_route(iw, cn, tw, th, esize):
    """'box' (u8 uint32 box sums), 'wave' (u8 integral rows, a wave per row),
    'thread' (u8 integral rows, a thread per row and channel) or 'f32'."""
    finish_lds = 2 * (iw + 1) * cn * 4 + 2 * 4 * 4 * 4
    if esize != 1:
        return "f32"
    if tw * th <= 66000 and finish_lds <= 64 * 1024:
        return "box"
    return "wave" if iw <= 33000 else "thread"


def widest_box(cn):
    return (64 * 1024 - 2 * 4 * 4 * 4) // (8 * cn) - 1


def width_with_residue(cn, lo, mod, target):
    """The first width >= lo whose row bytes iw * cn leave `target` modulo
    `mod` -- target 0, 1 or mod - 1; for an even cn, whose row bytes are
    multiples of g = gcd(cn, mod), the nearest residues there are: g, mod - g."""
    g = math.gcd(cn, mod)
    want = {0: 0, 1: g % mod, mod - 1: mod - g}[target]
    return next(iw for iw in range(lo, lo + mod + 1) if iw * cn % mod == want)


# ---------------------------------------------------------------------------
# helpers

def same(got, want, what):
    """assert_bits, naming the first differing element."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    if got.shape == want.shape and got.dtype == want.dtype == F32:
        bad = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
        if len(bad):
            i = tuple(int(k) for k in bad[0])
            what = f"{what}: {len(bad)} of {got.size} differ, first at {i}: got {got[i]!r}, want {want[i]!r}"
    assert_bits(got, want, what)


def kernel_knob(ops, k):
    return ops.tuning(MATCH_KERNEL=0) if k == 0 else contextlib.nullcontext()


def kernels_of(dtype):
    """u8: the default dispatch and the v_dot4 kernel; fp32 has one correlation."""
    return ("default", 0) if np.dtype(dtype) == U8 else ("default",)


def check(ops, dev, imgs, tpl, methods, what):
    """imgs (n, h, w, c) against tpl (h, w, c): every method, under every
    correlation kernel of the dtype, equals the numpy reference bit for bit."""
    want = ref_methods(imgs, tpl, methods)
    d_img, d_tpl = to_dev(imgs, dev), to_dev(tpl, dev)
    for k in kernels_of(imgs.dtype):
        with kernel_knob(ops, k):
            for m in methods:
                got = host(ops.match_template(d_img, d_tpl, m))
                same(got, want[m], f"{what}: image {imgs.shape[1:]}, template {tpl.shape}, method {m}, kernel {k}")


# ---------------------------------------------------------------------------
# the references themselves, on the CPU

def minmax_cases():
    """[(name, array, mask or None)] of 1(j), shared by the CPU and the GPU test."""
    rng = np.random.default_rng(2026)
    cases = []
    for h, w in [(63, 65), (64, 64), (17, 241), (1, 5000), (5000, 1), (2049, 2049)]:
        # 4095 / 4096 / 4097 elements: the step of the partition count; 2049^2 > 1024 * 4096: the grid-stride loop
        cases.append((f"f32 {h}x{w}", data(rng, (h, w), F32), None))
        cases.append((f"u8 {h}x{w}", data(rng, (h, w), U8), None))
        cases.append((f"u8 {h}x{w} masked", data(rng, (h, w), U8), (rng.random((h, w)) < 0.3).astype(np.uint8)))
    # the extremes at the last element, equal values in an earlier workgroup's share: the first wins
    a = data(rng, (3, 4096), F32)
    a.flat[-1] = a.flat[5] = a.min() - 1
    a.flat[-2] = a.flat[300] = a.max() + 1
    cases.append(("ties across partitions", a, None))
    u = data(rng, (3, 4096), U8).clip(1, 254)
    u.flat[-1] = u.flat[777] = 0
    u.flat[-2] = u.flat[1500] = 255
    cases.append(("u8 ties across partitions", u, None))
    cases.append(("constant", np.full((9, 31), 2.5, np.float32), None))
    cases.append(("u8 constant", np.full((9, 31), 7, np.uint8), None))
    inf = data(rng, (7, 13), F32)
    inf[2, 3], inf[5, 1], inf[6, 12] = np.inf, -np.inf, np.inf
    cases.append(("infinities", inf, None))
    z = np.zeros((4, 9), np.float32)
    z[0, 0] = -0.0
    cases.append(("-0.0 before +0.0", z, None))
    z2 = np.zeros((4, 9), np.float32)
    z2[0, 1] = -0.0
    cases.append(("+0.0 before -0.0", z2, None))
    nan0 = data(rng, (7, 13), F32)
    nan0[0, 0] = np.nan
    cases.append(("NaN at index 0", nan0, None))
    cases.append(("all NaN", np.full((7, 13), np.nan, np.float32), None))
    one = np.zeros((7, 13), np.uint8)
    one[4, 11] = 1
    cases.append(("mask of one element", data(rng, (7, 13), F32), one))
    cases.append(("u8 mask of one element", data(rng, (7, 13), U8), one))
    cases.append(("mask of none", data(rng, (7, 13), F32), np.zeros((7, 13), np.uint8)))
    return cases


ORACLE_SHAPES = [((40, 70), (7, 9)), ((70, 130), (17, 23)), ((9, 300), (3, 5)), ((20, 20), (20, 20)),
                 ((66, 66), (1, 1))]


def test_references_match_oracle(oracle):
    """ref_match_template equals oracle_match_template bit for bit: cn 1-4, u8
    and the exact-sum fp32 data, six methods, five shapes, and flat / saturated
    / zero images and templates; ref_min_max_idx equals oracle.min_max_idx on
    the minMaxIdx cases."""
    rng = np.random.default_rng(1)
    count = 0
    for dtype in (U8, F32):
        top = 255 if dtype == U8 else 128.0
        for cn in (1, 2, 3, 4):
            pairs = [(data(rng, ih + (cn,), dtype), data(rng, th + (cn,), dtype)) for ih, th in ORACLE_SHAPES]
            img, tpl = pairs[0]
            pairs += [(img, np.full_like(tpl, 9)), (np.zeros_like(img), tpl), (np.full_like(img, top), tpl),
                      (np.full_like(img, top), np.full_like(tpl, top)), (img, np.zeros_like(tpl)),
                      (np.repeat(np.repeat(img[:5, :9], 8, 0), 8, 1), tpl), (img, img[11:18, 30:39])]
            for img, tpl in pairs:
                sums = ref_window_sums(img, tpl)
                for m in ALL:
                    same(ref_formula(sums, tpl, m), oracle.match_template(img, tpl, m),
                         f"{dtype.name} c{cn} image {img.shape} template {tpl.shape} method {m}")
                    count += 1
    assert count >= 288
    for name, a, mask in minmax_cases():
        assert mm_key(ref_min_max_idx(a, mask)) == mm_key(oracle.min_max_idx(a, mask)), name
    assert ref_min_max_idx(np.float32([[3, 1, 1], [7, 7, 0]])) == (0.0, 7.0, (1, 2), (1, 0))


def test_plan_restatement():
    """The numbers the cases below rely on, from the restated formulas."""
    assert [mfma_plan(tw, 1, 1)[0] for tw in (1, 2, 33, 34, 65, 66)] == [1, 2, 2, 3, 3, 4]
    assert mfma_plan(2, 1, 3)[0] == 4 and mfma_plan(2, 1, 2)[0] == 3
    assert mfma_plan(226, 141, 1)[2] and not mfma_plan(226, 142, 1)[2]
    assert lds_bytes(256, 247, 1, 1) <= 64 * 1024 < lds_bytes(256, 248, 1, 1)
    assert [widest_box(c) for c in (1, 2, 3, 4)] == [8175, 4087, 2724, 2043]
    assert stats_route(33000, 1, 3, 2, 1) == "wave" and stats_route(33001, 1, 3, 2, 1) == "thread"


# ---------------------------------------------------------------------------
# a. the MFMA kernel's operand pipeline: nit = th * KB steps in groups of 8

@gpu
@pytest.mark.parametrize("cn,tw,kb,th_max", [(1, 1, 1, 17), (1, 2, 2, 9), (3, 2, 4, 5), (2, 2, 3, 6)])
def test_pipeline_tails(ops, dev, cn, tw, kb, th_max):
    rng = np.random.default_rng(100 + 10 * cn + tw)
    nits = set()
    for th in range(1, th_max + 1):
        KB, _, fits = mfma_plan(tw, th, cn)
        assert fits and KB == kb
        nits.add(th * KB)
        img = data(rng, (1, th + 5, tw + 69, cn), U8)  # result 6 x 70: two column tiles, the second partial
        check(ops, dev, img, data(rng, (th, tw, cn), U8), (CCORR, CCOEFF_NORMED), f"pipeline nit {th * KB}")
    if kb == 1:  # every remainder of 8, fewer steps than a prefetch (4) and than a group (8), 8 and 16 exactly
        assert nits == set(range(1, 18))


# ---------------------------------------------------------------------------
# b. the template widths at which KB (and the LDS stride) steps

def kb_steps(cn):
    """[(tw - 1, tw)] for every tw <= 66 at which KB increments."""
    return [(tw - 1, tw) for tw in range(2, 67) if mfma_plan(tw, 3, cn)[0] > mfma_plan(tw - 1, 3, cn)[0]]


@gpu
@pytest.mark.parametrize("cn", [1, 2, 3, 4])
def test_kb_steps(ops, dev, cn):
    steps = kb_steps(cn)
    assert len(steps) >= 3
    if cn in (1, 3, 4):
        assert steps[:3] == {1: [(1, 2), (33, 34), (65, 66)], 3: [(1, 2), (11, 12), (22, 23)],
                             4: [(1, 2), (9, 10), (17, 18)]}[cn]
    rng = np.random.default_rng(200 + cn)
    for below, at in steps:
        assert mfma_plan(at, 3, cn)[0] == mfma_plan(below, 3, cn)[0] + 1
        for tw in (below, at):
            assert mfma_plan(tw, 3, cn)[2]
            img = data(rng, (1, 7, tw + 69, cn), U8)  # result 5 x 70
            check(ops, dev, img, data(rng, (3, tw, cn), U8), (CCORR, CCORR_NORMED), f"KB {mfma_plan(tw, 3, cn)[0]}")


# ---------------------------------------------------------------------------
# c. result tile edges

TILE = (1, 31, 32, 33, 63, 64, 65)


@gpu
@pytest.mark.parametrize("rh,rw", sorted({(r, 65) for r in TILE} | {(65, r) for r in TILE}))
def test_result_tiles_u8(ops, dev, rh, rw):
    """MFMA: 64 x 64 results per workgroup, 32 x 32 per wave; the dot4 kernel through the knob."""
    rng = np.random.default_rng(300 + rh * 100 + rw)
    assert mfma_plan(2, 3, 3)[2]
    img = data(rng, (1, rh + 2, rw + 1, 3), U8)
    check(ops, dev, img, data(rng, (3, 2, 3), U8), (CCORR, CCOEFF_NORMED), "result tile")


@gpu
@pytest.mark.parametrize("rh", [3, 4, 5])
def test_result_tiles_f32(ops, dev, rh):
    """match_corr_f32_kernel: 256 columns x 4 rows per workgroup."""
    rng = np.random.default_rng(310 + rh)
    for rw in (255, 256, 257):
        img = data(rng, (1, rh + 2, rw + 1, 3), F32)
        check(ops, dev, img, data(rng, (3, 2, 3), F32), (CCORR, CCOEFF_NORMED), "fp32 result tile")


@gpu
@pytest.mark.parametrize("th", [1, 7, 8, 9, 16, 17])
def test_box_sum_rows(ops, dev, th):
    """match_vsum_u8_kernel: 64 result rows per thread, the template's rows in groups of 8."""
    rng = np.random.default_rng(320 + th)
    for rh in (63, 64, 65):
        img = data(rng, (1, rh + th - 1, 8, 3), U8)
        assert stats_route(8, 3, 2, th, 1) == "box"
        check(ops, dev, img, data(rng, (th, 2, 3), U8), STATS, "box sums rows")


@gpu
@pytest.mark.parametrize("iw", [255, 256, 257, 511, 512, 513])
def test_box_sum_columns(ops, dev, iw):
    """match_finish_u8_kernel: ceil(iw / 256) pixels per thread."""
    rng = np.random.default_rng(330 + iw)
    th = 3
    assert stats_route(iw, 3, 2, th, 1) == "box"
    img = data(rng, (1, th + 2, iw, 3), U8)
    check(ops, dev, img, data(rng, (th, 2, 3), U8), STATS, "box sums columns")


# ---------------------------------------------------------------------------
# d. fp32 statistics: the integral images' row and column passes

@gpu
@pytest.mark.parametrize("cn", [1, 2, 3, 4])
def test_f32_statistics(ops, dev, cn):
    """th = 1, so match_integral_cols_kernel (32 rows per step) covers exactly
    ih rows; rw around match_finish_kernel's 256 columns per workgroup."""
    rng = np.random.default_rng(400 + cn)
    for ih in (1, 31, 32, 33, 65):
        for rw in (255, 256, 257):
            img = data(rng, (1, ih, rw + 1, cn), F32)
            check(ops, dev, img, data(rng, (1, 2, cn), F32), ALL, "fp32 statistics")


# ---------------------------------------------------------------------------
# e. operand placement: bases, pitches, a template that is a view of the image

def placement_cases(dtype, count=40):
    """A seeded sample in which every value of every factor occurs."""
    rng = np.random.default_rng(500 + np.dtype(dtype).itemsize)
    factors = dict(cn=[1, 2, 3, 4], method=list(ALL), off=[0, 1, 3, 5, 16] if np.dtype(dtype) == U8 else [0, 4, 8],
                   row_pad=[0, 1, 3, 16], batch_pad=[0, 7], residue=[0, 1, 15], tpl=["dense", "slice", "placed"],
                   out_row_pad=[0, 3], out_batch_pad=[0, 5])
    cols = {}
    for name, values in factors.items():
        col = (values * (count // len(values) + 1))[:count]
        rng.shuffle(col)
        assert set(col) == set(values)
        cols[name] = col
    return [{name: cols[name][i] for name in cols} for i in range(count)]


@gpu
@pytest.mark.parametrize("dtype", [U8, F32], ids=["u8", "f32"])
def test_operand_placement(ops, dev, dtype):
    n, ih, th, tw = 2, 37, 9, 11
    for i, p in enumerate(placement_cases(dtype)):
        rng = np.random.default_rng(510 + i)
        cn = p["cn"]
        # the last 16-byte chunk of the last row straddles the image's end in the MFMA staging
        iw = width_with_residue(cn, 83, 16, p["residue"])
        imgs = data(rng, (n, ih, iw, cn), dtype)
        ibuf, iview = place(imgs, dev, off=p["off"], row_pad=p["row_pad"], batch_pad=p["batch_pad"])
        y, x = int(rng.integers(0, ih - th + 1)), int(rng.integers(0, iw - tw + 1))
        if p["tpl"] == "slice":  # the most natural caller: a pitched view at an odd byte offset
            tpl = np.ascontiguousarray(imgs[0, y:y + th, x:x + tw])
            tview = iview[0, y:y + th, x:x + tw]
        elif p["tpl"] == "placed":
            tpl = data(rng, (th, tw, cn), dtype)
            tview = place(tpl[None], dev, off=3 * dtype.itemsize, row_pad=5)[1][0]
        else:
            tpl = data(rng, (th, tw, cn), dtype)
            tview = to_dev(tpl, dev)
        m = p["method"]
        want = ref_methods(imgs, tpl, (m,))[m]
        rh, rw = ih - th + 1, iw - tw + 1
        for k in kernels_of(dtype):
            obuf, oview = place(blank((n, rh, rw, 1), np.float32), dev, off=4, row_pad=p["out_row_pad"],
                                batch_pad=p["out_batch_pad"])
            what = f"placement {i} {p} iw {iw} kernel {k}"
            with kernel_knob(ops, k):
                got = ops.match_template(iview, tview, m, out=oview[..., 0])
            assert got.data_ptr() == oview.data_ptr()
            same(host(oview)[..., 0], want, what)
            assert_rim_intact(obuf, oview, what)
        assert_bits(host(iview), imgs, f"placement {i}: source")


# ---------------------------------------------------------------------------
# f. the window-statistics routes of u8

@gpu
@pytest.mark.parametrize("cn", [2, 3])
def test_box_integral_boundary(ops, dev, cn):
    """The widest box-sum image and the narrowest integral-image one (cn = 1
    and 4: test_gpu_parity.py): each against the reference, and equal on the
    columns they share."""
    wbox = widest_box(cn)
    assert wbox == {2: 4087, 3: 2724}[cn]
    assert stats_route(wbox, cn, 9, 7, 1) == "box" and stats_route(wbox + 1, cn, 9, 7, 1) == "wave"
    rng = np.random.default_rng(600 + cn)
    edge = data(rng, (1, 9, wbox + 1, cn), U8)
    tpl = np.ascontiguousarray(edge[0, 1:8, 50:59])  # 7 rows x 9 columns
    narrow = np.ascontiguousarray(edge[:, :, :wbox])
    for imgs in (narrow, edge):
        check(ops, dev, imgs, tpl, (SQDIFF_NORMED, CCOEFF_NORMED), "box / integral boundary")
    for m in (SQDIFF_NORMED, CCOEFF_NORMED):
        box = host(ops.match_template(to_dev(narrow, dev), to_dev(tpl, dev), m))
        integ = host(ops.match_template(to_dev(edge, dev), to_dev(tpl, dev), m))
        same(integ[:, :, :box.shape[2]], box, f"box sums vs integral images c{cn} method {m}")


@gpu
@pytest.mark.parametrize("cn", [1, 2, 3, 4])
def test_integral_row_carries(ops, dev, cn):
    """match_integral_rows_u8_kernel: 64 row bytes per step, the first channel
    of a step and each channel's carry lane move with cn; the last step is
    full, one byte or 63 bytes (an even cn: the nearest residues)."""
    rng = np.random.default_rng(610 + cn)
    for target in (0, 1, 63):
        iw = width_with_residue(cn, widest_box(cn) + 1, 64, target)
        assert stats_route(iw, cn, 4, 3, 1) == "wave"
        img = data(rng, (1, 5, iw, cn), U8)
        check(ops, dev, img, data(rng, (3, 4, cn), U8), (SQDIFF_NORMED, CCOEFF_NORMED), f"integral rows % 64 = {target}")


@gpu
@pytest.mark.parametrize("iw,route", [(33000, "wave"), (33001, "thread")])
def test_integral_rows_widest(ops, dev, iw, route):
    """An all-255 row of 33,000 pixels puts 33,000 * 255^2 = 2,145,825,000 <
    2^31 in the wave kernel's int32 square sums; one pixel more takes the
    per-thread kernel."""
    assert stats_route(iw, 1, 3, 2, 1) == route
    rng = np.random.default_rng(620)
    img = data(rng, (1, 4, iw, 1), U8)
    img[0, 1] = 255
    check(ops, dev, img, data(rng, (2, 3, 1), U8), (SQDIFF_NORMED, CCOEFF_NORMED), f"integral rows {route}")


# ---------------------------------------------------------------------------
# g. limits

@gpu
@pytest.mark.parametrize("th,fits", [(141, True), (142, False)])
def test_mfma_lds_boundary(ops, dev, th, fits):
    """226 x 141 is the last template whose image block fits the MFMA kernel's
    64 KiB; one row more goes to the dot4 kernel by dispatch."""
    assert mfma_plan(226, th, 1)[2] == fits
    rng = np.random.default_rng(700 + th)
    img = data(rng, (1, th + 3, 231, 1), U8)
    check(ops, dev, img, data(rng, (th, 226, 1), U8), (CCORR, CCOEFF_NORMED), "MFMA LDS boundary")


@gpu
@pytest.mark.parametrize("dtype,tw", [(U8, 256), (F32, 64)], ids=["u8", "f32"])
def test_largest_template(ops, dev, dtype, tw):
    """The tallest template match_lds_bytes admits; one row more is refused before anything is written."""
    es = dtype.itemsize
    th = max(t for t in range(1, 2000) if lds_bytes(tw, t, 1, es) <= 64 * 1024)
    assert (dtype, th) in ((U8, 247), (F32, 236))
    rng = np.random.default_rng(710 + es)
    img = data(rng, (1, th + 4, tw + 5, 1), dtype)
    check(ops, dev, img[:, :th + 3], data(rng, (th, tw, 1), dtype), (CCORR, CCOEFF_NORMED), "largest template")
    obuf, oview = place(blank((1, 4, 6, 1), np.float32), dev, off=4)
    d_img, d_tpl = to_dev(img, dev), to_dev(data(rng, (th + 1, tw, 1), dtype), dev)
    unsupported(lambda: ops.match_template(d_img, d_tpl, CCORR, out=oview[..., 0]))
    assert_untouched(obuf, "a template past the LDS limit")


# ---------------------------------------------------------------------------
# h. degenerate values

@gpu
@pytest.mark.parametrize("dtype", [U8, F32], ids=["u8", "f32"])
@pytest.mark.parametrize("cn", [1, 3])
def test_degenerate_values(ops, dev, cn, dtype):
    rng = np.random.default_rng(800 + cn + dtype.itemsize)
    top = 255 if dtype == U8 else 128.0
    img = data(rng, (1, 24, 32, cn), dtype)
    tpl = data(rng, (3, 2, cn), dtype)
    blocks = np.repeat(np.repeat(data(rng, (1, 3, 4, cn), dtype), 8, 1), 8, 2)  # 8 x 8 constant blocks: t = 0 inside
    cases = [("flat template", img, np.full_like(tpl, 9)),
             ("constant blocks", blocks, tpl),
             ("zero image", np.zeros_like(img), tpl),
             ("saturated", np.full_like(img, top), np.full_like(tpl, top)),
             ("template cut from the image", img, np.ascontiguousarray(img[0, 5:12, 9:20])),
             ("template of the image's size", img, np.ascontiguousarray(img[0]))]
    for name, im, tp in cases:
        check(ops, dev, im, tp, ALL, name)


# ---------------------------------------------------------------------------
# i. call order: the bfrag and box workspaces reused at other sizes

@gpu
def test_call_order(ops, dev):
    rng = np.random.default_rng(900)
    img_a, tpl_a = data(rng, (60, 60, 3), U8), data(rng, (47, 41, 3), U8)
    img_b, tpl_b = data(rng, (10, 10, 1), U8), data(rng, (3, 2, 1), U8)
    d = [to_dev(a, dev) for a in (img_a, tpl_a, img_b, tpl_b)]
    a1 = ops.match_template(d[0], d[1], CCOEFF_NORMED)
    mm_a1 = ops.min_max_idx(a1)
    b = ops.match_template(d[2], d[3], CCOEFF_NORMED)
    mm_b = ops.min_max_idx(b)
    a2 = ops.match_template(d[0], d[1], CCOEFF_NORMED)
    mm_a2 = ops.min_max_idx(a2)
    want_a, want_b = ref_match_template(img_a, tpl_a, CCOEFF_NORMED), ref_match_template(img_b, tpl_b, CCOEFF_NORMED)
    same(host(a1), want_a, "A, first")
    same(host(b), want_b, "B")
    same(host(a2), want_a, "A, after B")
    assert mm_key(mm_a1) == mm_key(mm_a2) == mm_key(ref_min_max_idx(want_a))
    assert mm_key(mm_b) == mm_key(ref_min_max_idx(want_b))


# ---------------------------------------------------------------------------
# j. minMaxIdx

@gpu
def test_min_max_idx_cases(ops, dev):
    for name, a, mask in minmax_cases():
        got = ops.min_max_idx(to_dev(a, dev), None if mask is None else to_dev(mask, dev))
        assert mm_key(got) == mm_key(ref_min_max_idx(a, mask)), (name, got, ref_min_max_idx(a, mask))


@gpu
@pytest.mark.parametrize("dtype", [U8, F32], ids=["u8", "f32"])
def test_min_max_idx_placed(ops, dev, dtype):
    """Source and mask as pitched views at odd bases (L.row, L.mask_row)."""
    rng = np.random.default_rng(1000 + dtype.itemsize)
    a = data(rng, (37, 83), dtype)
    a[36, 82] = a.min()  # a later tie
    mask = (rng.random((37, 83)) < 0.3).astype(np.uint8)
    abuf, aview = place(a[None, :, :, None], dev, off=3 if dtype == U8 else 4, row_pad=3)
    mbuf, mview = place(mask[None, :, :, None], dev, off=5, row_pad=3)
    assert mm_key(ops.min_max_idx(aview[0, :, :, 0])) == mm_key(ref_min_max_idx(a))
    assert mm_key(ops.min_max_idx(aview[0, :, :, 0], mview[0, :, :, 0])) == mm_key(ref_min_max_idx(a, mask))
    assert_bits(host(aview)[0, :, :, 0], a, "source")


# ---------------------------------------------------------------------------
# k. ops.match_template's swap rule, and result rows past a grid's y limit

@gpu
@pytest.mark.parametrize("dtype", [U8, F32], ids=["u8", "f32"])
def test_swap_rule(ops, dev, dtype):
    """cv::matchTemplate's rule: w >= W and h >= H and one of them larger."""
    rng = np.random.default_rng(1100 + dtype.itemsize)
    img = data(rng, (5, 9, 3), dtype)
    for th, tw in [(8, 9), (5, 12), (8, 12)]:  # taller at equal width, wider at equal height, both
        tpl = data(rng, (th, tw, 3), dtype)
        for m in (SQDIFF, CCOEFF_NORMED):
            got = host(ops.match_template(to_dev(img, dev), to_dev(tpl, dev), m))
            same(got, ref_match_template(tpl, img, m), f"swapped: template {th} x {tw}, method {m}")


@gpu
def test_unfitting_template_raises_before_allocating(ops, dev, monkeypatch):
    rng = np.random.default_rng(1110)
    imgs, tpl = to_dev(data(rng, (2, 5, 9, 3), U8), dev), to_dev(data(rng, (8, 12, 3), U8), dev)
    one, wide = to_dev(data(rng, (5, 9, 3), U8), dev), to_dev(data(rng, (3, 12, 3), U8), dev)

    def no_alloc(*a, **k):
        raise AssertionError("allocated a result for a template that does not fit")
    monkeypatch.setattr(ops.torch, "empty", no_alloc)
    with pytest.raises(ValueError, match=r"12 x 8 .*9 x 5"):  # a batch is never swapped
        ops.match_template(imgs, tpl, CCORR)
    with pytest.raises(ValueError, match=r"12 x 3 .*9 x 5"):  # wider but shorter: neither order fits
        ops.match_template(one, wide, CCORR)


@gpu
@pytest.mark.parametrize("dtype", [U8, F32], ids=["u8", "f32"])
def test_result_rows_past_grid_y(ops, dev, dtype):
    """65,537 result rows: match_finish_kernel (fp32's route) folds the row
    into the grid's x, whose y ends at 65,535."""
    rng = np.random.default_rng(1120)
    img = data(rng, (1, 65538, 3, 1), dtype)
    check(ops, dev, img, data(rng, (2, 2, 1), dtype), (SQDIFF_NORMED, CCOEFF_NORMED), "65,537 result rows")


# ---------------------------------------------------------------------------
# the C++ layer

@gpu
def test_cpp_match_template_and_minmax(hip_device, tmp_path):
    """tests/cpp/vacv_match_test.cpp: va_cv::match_template and va_cv::minMaxIdx
    on host and device tensors against this module's references, by bytes."""
    rng = np.random.default_rng(1200)
    u_img, u_tpl = data(rng, (23, 40, 3), U8), data(rng, (5, 7, 3), U8)
    f_img, f_tpl = data(rng, (19, 33, 1), F32), data(rng, (4, 6, 1), F32)
    tall = data(rng, (27, 40, 3), U8)  # the image's width, taller: swapped
    mm_src = data(rng, (21, 37), F32)
    mm_src[3, 5] = np.nan
    mm_src[20, 36] = mm_src[~np.isnan(mm_src)].min()  # a later tie
    mm_mask = (rng.random((21, 37)) < 0.3).astype(np.uint8)
    d = tmp_path / "data"
    d.mkdir()
    (d / "dims.txt").write_text("23 40 5 7 19 33 4 6 27 21 37\n")
    for name, a in [("u8_img", u_img), ("u8_tpl", u_tpl), ("f32_img", f_img), ("f32_tpl", f_tpl), ("u8_tall", tall),
                    ("mm_src", mm_src), ("mm_mask", mm_mask)]:
        a.tofile(d / f"{name}.bin")
    for m in ALL:
        ref_match_template(u_img, u_tpl, m).tofile(d / f"u8_want_{m}.bin")
        ref_match_template(f_img, f_tpl, m).tofile(d / f"f32_want_{m}.bin")
    ref_match_template(tall, u_img, CCORR_NORMED).tofile(d / "swap_want.bin")
    with open(d / "mm_want.bin", "wb") as f:
        for mask in (None, mm_mask, np.zeros_like(mm_mask)):
            mn, mx, imn, imx = ref_min_max_idx(mm_src, mask)
            f.write(struct.pack("<dd4i", mn, mx, *imn, *imx))

    repo = Path(__file__).resolve().parent.parent
    pkg = repo / "arm-neon-opencv_amd"
    lib = pkg / "lib"
    exe = tmp_path / "vacv_match_test"
    r = subprocess.run(["g++", "-std=c++14", "-O1", str(repo / "tests" / "cpp" / "vacv_match_test.cpp"), "-o", str(exe),
                        "-I", str(pkg / "src"), "-L", str(lib), "-lvacv", "-lvacv_hip", f"-Wl,-rpath,{lib}"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run(["timeout", "-k", "10", "120", str(exe), str(d)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "failed 0" in r.stdout, r.stdout[-3000:]
