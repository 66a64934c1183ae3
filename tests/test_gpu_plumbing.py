"""The pixel-plumbing operators every pipeline runs before and after the
resize / warp / colour kernels -- crop / clone, change_layout, change_dtype,
normalize, channel_sums / mean_stddev and the equal-size shortcut of
vacv_resize (csrc/k_pixel.hip, csrc/vacv_abi.cpp) -- at the misaligned,
pitched and tail shapes that select their code paths.

Every input and output is a view placed inside a larger device buffer that is
filled with a sentinel byte, so a case controls the base alignment and the
pitches exactly and a stray write (a zero included) shows in the rim.  The
references are plain numpy, independent of the library;
test_references_match_oracle checks them against the oracle's C functions on
the CPU.  All GPU tests carry the gpu mark one by one (not through pytestmark)
because that one test must run without a device.
"""
from __future__ import annotations

import itertools
import math

import numpy as np
import pytest

gpu = pytest.mark.gpu

SENTINEL = 0xA5  # as bytes: a non-NaN pattern in fp16 / fp32 / fp64 too
NHWC, NCHW = 1, 0  # include/vacv_hip.h; asserted against the package in the ops fixture


@pytest.fixture(scope="module")
def ops(hip_device):
    import vacv_amd
    from vacv_amd import ops
    assert (vacv_amd.NHWC, vacv_amd.NCHW) == (NHWC, NCHW)
    return ops


@pytest.fixture(scope="module")
def dev(hip_device):
    return hip_device


def host(t):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy()


# ---------------------------------------------------------------------------
# helpers: an image inside a sentinel-filled buffer, and the rim check

def _torch_dtype(npdt):
    import torch
    return {np.dtype(np.uint8): torch.uint8, np.dtype(np.float16): torch.float16,
            np.dtype(np.float32): torch.float32, np.dtype(np.float64): torch.float64}[np.dtype(npdt)]


def place(a, dev, layout=NHWC, off=0, row_pad=0, batch_pad=0):
    """(buffer, view): `a` (n, h, w, c) NHWC or (n, c, h, w) NCHW laid out in a
    flat uint8 device buffer of SENTINEL bytes, its first element `off` bytes
    in, every row followed by `row_pad` and every image by `batch_pad` unused
    elements; 32 sentinel bytes follow the last image."""
    import torch
    a = np.ascontiguousarray(a)
    es = a.itemsize
    assert off % es == 0, "a typed view starts on an element boundary"
    if layout == NHWC:
        n, h, w, c = a.shape
        rp = w * c + row_pad
        img = h * rp + batch_pad
        strides = (img, rp, c, 1)
    else:
        n, c, h, w = a.shape
        rp = w + row_pad
        img = c * h * rp + batch_pad
        strides = (img, h * rp, rp, 1)
    flat = np.full(off + n * img * es + 32, SENTINEL, np.uint8)
    typed = flat[off:off + n * img * es].view(a.dtype)
    np.lib.stride_tricks.as_strided(typed, a.shape, [s * es for s in strides])[...] = a
    buffer = torch.from_numpy(flat).to(dev)
    view = buffer[off:off + n * img * es].view(_torch_dtype(a.dtype)).as_strided(a.shape, strides)
    return buffer, view


def blank(shape, dtype):
    """An array of SENTINEL bytes: a destination's initial content."""
    return np.full(int(np.prod(shape)) * np.dtype(dtype).itemsize, SENTINEL, np.uint8).view(dtype).reshape(shape)


def assert_rim_intact(buffer, view, what=""):
    """Every byte of `buffer` outside `view` still holds SENTINEL."""
    es = view.element_size()
    off = view.data_ptr() - buffer.data_ptr()
    nelem = (buffer.numel() - off) // es
    inside_e = np.zeros(nelem, bool)
    np.lib.stride_tricks.as_strided(inside_e, tuple(view.shape), tuple(view.stride()))[...] = True
    inside = np.zeros(buffer.numel(), bool)
    inside[off:off + nelem * es] = np.repeat(inside_e, es)
    got = host(buffer)
    bad = (got != SENTINEL) & ~inside
    assert not bad.any(), f"{what}: {int(bad.sum())} bytes written outside the view, first at {int(np.argmax(bad))}"


def assert_untouched(buffer, what=""):
    assert (host(buffer) == SENTINEL).all(), f"{what}: a refused call wrote to the destination"


def assert_bits(got, want, what=""):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    bad = got.view(np.uint8) != want.view(np.uint8)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} bytes differ"


def rand(shape, dtype, seed):
    rng = np.random.default_rng(seed)
    if np.dtype(dtype) == np.uint8:
        return rng.integers(0, 256, shape, dtype=np.uint8)
    return (rng.standard_normal(shape) * 64 + 100).astype(dtype)


def unsupported(fn):
    import vacv_amd as V
    with pytest.raises(V.VacvError) as e:
        fn()
    assert e.value.status == V._lib.ERR_UNSUPPORTED, e.value.status


# ---------------------------------------------------------------------------
# numpy references (independent of the library)

# NaN, +-inf, +-0, the smallest denormal, the values around 1 and 256, negative
# values, and the uint32 range's upper half and end (vacv_semantics.hpp:171-177)
SPECIALS = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, 1.401298464324817e-45, 0.99, 1.0, 255.0, 255.99, 256.0,
                     256.7, 511.5, -1.0, -1e30, 2.0 ** 31, 2.0 ** 31 + 2.0 ** 8, 2.0 ** 32 - 2.0 ** 8, 2.0 ** 32,
                     1e30], np.float32)


def ref_f32_to_u8(f):
    """f32_to_u8_neon as written: not > 0 (NaN too) -> 0; >= 2^32 -> 0xFFFFFFFF;
    else truncate to uint32; keep the low 8 bits."""
    f = np.asarray(f, np.float32)
    u = np.zeros(f.shape, np.uint64)
    pos = f > 0
    big = pos & (f >= np.float32(4294967296.0))
    mid = pos & ~big
    u[mid] = np.floor(f[mid].astype(np.float64)).astype(np.uint64)
    u[big] = 0xFFFFFFFF
    return (u & 0xFF).astype(np.uint8)


def ref_normalize(x, mean, std, layout=NHWC):
    """normalize_value (vacv_semantics.hpp:165-168): d = float32(x) - mean in
    fp32, then float32(float64(d) / (float64(std) + 1e-6)); x is 4-D, mean /
    std are (c,) or per-image (n, c)."""
    x = np.asarray(x)
    n = x.shape[0]
    c = x.shape[3] if layout == NHWC else x.shape[1]
    m = np.broadcast_to(np.asarray(mean, np.float32).reshape(-1, c), (n, c))
    s = np.broadcast_to(np.asarray(std, np.float32).reshape(-1, c), (n, c))
    bshape = (n, 1, 1, c) if layout == NHWC else (n, c, 1, 1)
    d = x.astype(np.float32) - m.reshape(bshape)
    assert d.dtype == np.float32
    return (d.astype(np.float64) / (s.reshape(bshape).astype(np.float64) + 1e-6)).astype(np.float32)


def ref_sums(x, layout=NHWC, per_image=True):
    """(groups, c, 2) fp64 (Sum x, Sum x^2): int64 arithmetic for u8 (exact),
    math.fsum of the fp64 values for fp32 (exact, correctly rounded; an fp32
    value's square is exact in fp64).  Also returns (groups, c) Sum |x| and
    Sum x^2 magnitudes and the summand count, for the fp32 bound."""
    x = np.asarray(x)
    if layout == NCHW:
        x = x.transpose(0, 2, 3, 1)
    n, c = x.shape[0], x.shape[3]
    v = x.reshape(n, -1, c) if per_image else x.reshape(1, -1, c)
    g = v.shape[0]
    sums = np.zeros((g, c, 2), np.float64)
    mags = np.zeros((g, c, 2), np.float64)
    for i in range(g):
        for k in range(c):
            if x.dtype == np.uint8:
                col = v[i, :, k].astype(np.int64)
                sums[i, k] = (int(col.sum()), int((col * col).sum()))
                mags[i, k] = sums[i, k]
            else:
                col = v[i, :, k].astype(np.float64)
                sums[i, k] = (math.fsum(col), math.fsum(col * col))
                mags[i, k] = (math.fsum(np.abs(col)), sums[i, k, 1])
    return sums, mags, v.shape[1]


def ref_mean_std(sums, count):
    """stats_kernel: mean = S1 / count, stddev = sqrt(max(S2 / count - mean^2, 0)) in fp64, stored as fp32."""
    m = sums[..., 0] / count
    var = np.maximum(sums[..., 1] / count - m * m, 0.0)
    return m.astype(np.float32), np.sqrt(var).astype(np.float32)


def assert_sums(got, x, layout, per_image, what):
    want, mags, count = ref_sums(x, layout, per_image)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if np.asarray(x).dtype == np.uint8:
        assert np.array_equal(got, want), f"{what}: u8 sums are integers and exact"
        return
    # fp32 input: the kernel adds `count` fp64 terms per output in some fixed
    # order (lanes, waves, blocks, images).  Every term (x, or x*x which is
    # exact in fp64) is an exact fp64 number, so the only error is the fp64
    # rounding of the count - 1 additions: for ANY order of recursive or tree
    # summation |S_computed - S| <= gamma_(count-1) * Sum|t_i| with gamma_k =
    # k u / (1 - k u), u = 2^-53 (Higham, Accuracy and Stability, 4.2), and
    # gamma_(count-1) <= count * u while count^2 * u <= 1 (count < 9e7).  The
    # reference (math.fsum) is the correctly rounded exact sum: half an ulp,
    # <= u * Sum|t_i|, covered by using count + 1.
    bound = (count + 1) * 2.0 ** -53 * mags
    err = np.abs(got - want)
    assert (err <= bound).all(), f"{what}: fp32 sums off by {err.max()} (bound {bound[err == err.max()][0]})"


# ---------------------------------------------------------------------------
# the references against the oracle's C functions (CPU, no device)

def test_references_match_oracle(oracle):
    for dt in (np.uint8, np.float32):
        a = rand((11, 37, 3), dt, 1)
        assert_bits(a[2:10, 5:26], oracle.crop(a, 5, 2, 21, 8), "crop")
        chw = np.ascontiguousarray(a.transpose(2, 0, 1))
        assert_bits(chw[:, 2:10, 5:26], oracle.crop(chw, 5, 2, 21, 8, chw=True), "crop chw")
        assert_bits(chw, oracle.hwc_to_chw(a), "hwc->chw")
        assert_bits(a, oracle.chw_to_hwc(chw), "chw->hwc")
    u = rand((7, 9, 3), np.uint8, 2)
    assert_bits(u.astype(np.float32), oracle.u8_to_f32(u), "u8->f32")
    f = np.concatenate([SPECIALS, (np.random.default_rng(3).standard_normal(300) * 200 + 100).astype(np.float32)])
    assert_bits(ref_f32_to_u8(f), oracle.f32_to_u8(f), "f32->u8")
    want = dict(zip(SPECIALS[[0, 1, 2, 9, 10, 11, 12, 15, 17, 18]].tolist(), [0, 255, 0, 255, 0, 0, 255, 0, 0, 255]))
    for v, w in want.items():  # the semantics spelled out, so that two equal mistakes do not pass
        assert ref_f32_to_u8(np.array([v], np.float32))[0] == w, (v, w)
    for c in (1, 3, 4):
        mean, std = np.arange(c, dtype=np.float32) * 7 + 50.5, np.arange(c, dtype=np.float32) * 3 + 40.25
        for dt in (np.uint8, np.float32):
            x = rand((5, 7, c), dt, 4 + c)
            assert_bits(ref_normalize(x[None], mean, std)[0], oracle.normalize(x.astype(np.float32), mean, std),
                        f"normalize c{c}")
            s, mags, count = ref_sums(x[None])
            o = oracle.channel_sums(x).reshape(c, 2)
            if dt == np.uint8:
                assert np.array_equal(s[0], o)
            else:  # the oracle adds sequentially in fp64: within the bound of assert_sums
                assert (np.abs(s[0] - o) <= (count + 1) * 2.0 ** -53 * mags[0]).all()
            m, sd = ref_mean_std(s[0], count)
            om, osd = oracle.stats_from_sums(s[0].reshape(-1), count)
            assert_bits(m, om, "mean from sums")
            assert_bits(sd, osd, "stddev from sums")


# ---------------------------------------------------------------------------
# crop / clone: row_copy_kernel

# (left, source base offset, destination base offset, source row pad, destination row pad); offsets in
# bytes, pads in elements.  Each row takes the 16-byte path when src | dst is 16-byte aligned, the dword
# path when 4-byte aligned, else the byte path; an odd pad (5) makes consecutive rows take different ones.
CROP_SAMPLE = [(0, 0, 0, 0, 0),     # dense destination, 16-byte path on the rows that line up
               (1, 0, 0, 0, 0),     # left = 1: u8 source rows off a dword -> byte path
               (4, 0, 16, 0, 16),   # everything a multiple of 4 -> dword path (16-byte where the row starts line up)
               (4, 4, 4, 16, 16),   # both bases 4 mod 16
               (5, 0, 0, 5, 5),     # odd pitches on both sides: the path changes from row to row
               (16, 0, 16, 16, 0),  # left = 16 elements
               (16, 4, 4, 5, 16),
               (0, 8, 8, 5, 0),
               (1, 1, 1, 16, 5),    # u8 only (odd base offsets)
               (4, 1, 4, 5, 16),    # u8 only
               (5, 4, 1, 0, 5)]     # u8 only


def _crop_case(ops, dev, a, layout, rect, soff, doff, spad, dpad, what, strided=False, clone=False):
    left, top, cw, ch = rect
    sbuf, sview = place(a, dev, layout, off=soff, row_pad=spad, batch_pad=3 if spad else 0)
    src, ref = (sview[::2], a[::2]) if strided else (sview, a)
    want = ref[:, top:top + ch, left:left + cw] if layout == NHWC else ref[:, :, top:top + ch, left:left + cw]
    dbuf, dview = place(blank(want.shape, a.dtype), dev, layout, off=doff, row_pad=dpad, batch_pad=7 if dpad else 0)
    if clone:  # change_dtype with equal dtypes: the same row copy, source window taken by slicing
        win = src[:, top:top + ch, left:left + cw] if layout == NHWC else src[:, :, top:top + ch, left:left + cw]
        ops.change_dtype(win, win.dtype, layout=layout, out=dview)
    else:
        ops.crop(src, (left, top, left + cw, top + ch), layout=layout, out=dview)
    assert_bits(host(dview), want, what)
    assert_rim_intact(dbuf, dview, what)


@gpu
@pytest.mark.parametrize("dtype", [np.uint8, np.float16, np.float32, np.float64])
def test_crop_clone_row_paths(ops, dev, dtype):
    """row_copy_kernel's three per-row paths and their tails, bit-exact
    against numpy slicing with an intact rim.  Crop width 21 of a 37-pixel
    row: 63 bytes for u8 c = 3 (16-byte path: 3 vectors + 15 tail bytes; dword
    path: 15 dwords + 3 tail bytes), 126 for fp16 c = 3 (dword path + 2 tail
    bytes).  383 of 400 pixels: 1,149 bytes for u8, more than one 64-lane pass
    of 16-byte (1,024 B) and of 4-byte (256 B) accesses, with a tail."""
    es = np.dtype(dtype).itemsize
    u8 = dtype == np.uint8
    full = list(itertools.product((0, 1, 4, 5, 16), (0, 1, 4), (0, 1, 4, 16), (0, 5, 16), (0, 5, 16)))
    seed = 0
    for layout in (NHWC, NCHW):
        for (h, w), cs in (((11, 37), (1, 2, 3, 4)), ((6, 400), (3,))):
            top, cw, ch = (2, 21, h - 3) if w == 37 else (1, 383, 4)
            for c in cs:
                seed += 1
                a = rand((4, h, w, c) if layout == NHWC else (4, c, h, w), dtype, seed)
                # u8, c = 3, NHWC, small: every combination of lefts, base offsets and row pitches
                # (alignment is a matter of bytes, so this is where the whole path logic is enumerated);
                # the other element sizes, channel counts and the NCHW planes take the sample above
                combos = full if (u8 and c == 3 and layout == NHWC and w == 37) else CROP_SAMPLE
                for i, (left, soff, doff, spad, dpad) in enumerate(combos):
                    if soff % es or doff % es:
                        continue  # a typed tensor cannot start inside an element
                    what = (f"crop {np.dtype(dtype).name} layout {layout} {h}x{w}x{c} left {left} off {soff}/{doff} "
                            f"pad {spad}/{dpad}")
                    _crop_case(ops, dev, a[:2], layout, (left, top, cw, ch), soff, doff, spad, dpad, what)
                    if combos is CROP_SAMPLE and i % 3 == 1:
                        _crop_case(ops, dev, a[:2], layout, (left, top, cw, ch), soff, doff, spad, dpad, "clone " + what,
                                   clone=True)
                # a batch-strided source (src[::2]: the image pitch is twice the image) into a pitched out=
                _crop_case(ops, dev, a, layout, (5, top, cw, ch), 0, 0, 5, 16, "batch-strided crop", strided=True)
                _crop_case(ops, dev, a, layout, (4, top, cw, ch), 0, 16, 0, 0, "batch-strided clone", strided=True, clone=True)


# ---------------------------------------------------------------------------
# change_layout: layout_kernel<T> and the u8 c = 3 dword kernels

# (dtype, n, h, w, c, source base offset, destination base offset): which kernel launch_layout picks
LAYOUT_CASES = [
    (np.uint8, 1, 8, 12, 3, 0, 0),    # w*h % 4 == 0, aligned: hwc3_to_chw_u8_kernel / chw_to_hwc3_u8_kernel
    (np.uint8, 1, 8, 12, 3, 16, 16),  # the same with a leading rim
    (np.uint8, 3, 8, 12, 3, 0, 16),   # a batch of 3 through the dword kernels (288-byte images)
    (np.uint8, 1, 7, 9, 3, 0, 0),     # w*h = 63, % 4 != 0: generic layout_kernel<uint8_t> with c = 3
    (np.uint8, 3, 7, 9, 3, 0, 16),    # batch of 3, 189-byte images: generic
    (np.uint8, 1, 8, 12, 3, 1, 0),    # source base 1 mod 4: generic
    (np.uint8, 1, 8, 12, 3, 2, 16),   # source base 2 mod 4: generic
    (np.uint8, 1, 8, 12, 3, 0, 1),    # destination base 1 mod 4: generic
    (np.uint8, 3, 8, 12, 3, 16, 2),   # destination base 2 mod 4, batch of 3: generic
    (np.uint8, 2, 7, 9, 2, 0, 16),    # c = 2
    (np.uint8, 2, 7, 9, 4, 1, 16),    # c = 4
    (np.uint8, 3, 7, 9, 5, 0, 3),     # c = 5 (> 4)
    (np.float16, 3, 7, 9, 3, 2, 16),  # 2-byte elements
    (np.float32, 3, 7, 9, 3, 4, 16),  # 4-byte elements
    (np.float64, 3, 7, 9, 3, 8, 16),  # 8-byte elements
    (np.uint8, 3, 7, 9, 1, 1, 16),    # c = 1: the same bytes in both layouts, row_copy_kernel
    (np.float32, 2, 7, 9, 1, 0, 4),   # c = 1, fp32
]


@gpu
@pytest.mark.parametrize("case", LAYOUT_CASES, ids=lambda t: f"{np.dtype(t[0]).name}-n{t[1]}-{t[2]}x{t[3]}x{t[4]}-off{t[5]}_{t[6]}")
def test_change_layout_paths(ops, dev, case):
    """Both directions, bit-exact against transpose, around a dense destination inside a larger buffer."""
    dtype, n, h, w, c, soff, doff = case
    a = rand((n, h, w, c), dtype, 100 + h * w * c + soff)
    chw = np.ascontiguousarray(a.transpose(0, 3, 1, 2))
    for src, want, lay, to in ((a, chw, NHWC, NCHW), (chw, a, NCHW, NHWC)):
        _, sview = place(src, dev, lay, off=soff)
        dbuf, dview = place(blank(want.shape, dtype), dev, to, off=doff)
        ops.change_layout(sview, to, layout=lay, out=dview)
        assert_bits(host(dview), want, f"layout {lay}->{to} {case}")
        assert_rim_intact(dbuf, dview, f"layout {lay}->{to} {case}")


@gpu
def test_change_layout_refuses_pitched(ops, dev):
    """Across layouts both images must be dense (include/vacv_hip.h): a row- or batch-pitched source or
    destination is VACV_ERR_UNSUPPORTED and nothing is written.  The same layout is a clone and takes pitches."""
    a = rand((2, 7, 9, 3), np.uint8, 7)
    chw = np.ascontiguousarray(a.transpose(0, 3, 1, 2))
    for c1 in (False, True):  # c = 1 is a copy across layouts, under the same rule
        x, xc = (a[..., :1].copy(), chw[:, :1].copy()) if c1 else (a, chw)
        for spad, sbp, dpad, dbp in ((5, 0, 0, 0), (0, 3, 0, 0), (0, 0, 5, 0), (0, 0, 0, 3)):
            _, sview = place(x, dev, NHWC, row_pad=spad, batch_pad=sbp)
            dbuf, dview = place(blank(xc.shape, np.uint8), dev, NCHW, row_pad=dpad, batch_pad=dbp)
            unsupported(lambda: ops.change_layout(sview, NCHW, layout=NHWC, out=dview))
            assert_untouched(dbuf, f"pitched layout change {spad, sbp, dpad, dbp}")
    _, sview = place(a, dev, NHWC, row_pad=5, batch_pad=3)
    dbuf, dview = place(blank(a.shape, np.uint8), dev, NHWC, off=1, row_pad=16, batch_pad=7)
    ops.change_layout(sview, NHWC, layout=NHWC, out=dview)
    assert_bits(host(dview), a, "same-layout clone, pitched")
    assert_rim_intact(dbuf, dview, "same-layout clone, pitched")


# ---------------------------------------------------------------------------
# change_dtype: the flat kernels and the element-wise fallbacks

DTYPE_SHAPES = [(1, 3, 5, 3), (1, 7, 9, 1), (1, 4, 4, 4), (2, 5, 7, 3)]  # counts 45, 63, 64, 210: % 4 = 1, 3, 0, 2


@gpu
@pytest.mark.parametrize("shape", DTYPE_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_change_dtype_paths(ops, dev, shape):
    """launch_dtype: the flat kernels need the u8 side 4-byte and the fp32
    side 16-byte aligned (offsets 0 or 4, and 0 or 16); every other pair of
    the offsets below takes u8_to_f32_kernel / f32_to_u8_kernel, which touch
    one element per access.  fp32 -> u8 runs over the special values of
    f32_to_u8_neon tiled to the count, and over ordinary values."""
    import torch
    count = int(np.prod(shape))
    u = rand(shape, np.uint8, count)
    spec = np.resize(SPECIALS, count).reshape(shape)
    ordinary = (np.random.default_rng(count).standard_normal(shape) * 200 + 100).astype(np.float32)
    ordinary.reshape(-1)[:4] = (255.99, 256.0, 0.99, -0.0)
    for o8, o32 in itertools.product((0, 1, 2, 4), (0, 4, 8, 16)):
        what = f"dtype {shape} u8 offset {o8} fp32 offset {o32}"
        _, sview = place(u, dev, off=o8)
        dbuf, dview = place(blank(shape, np.float32), dev, off=o32)
        ops.change_dtype(sview, torch.float32, out=dview)
        assert_bits(host(dview), u.astype(np.float32), "u8->f32 " + what)
        assert_rim_intact(dbuf, dview, "u8->f32 " + what)
        for f in (spec, ordinary):
            _, sview = place(f, dev, off=o32)
            dbuf, dview = place(blank(shape, np.uint8), dev, off=o8)
            ops.change_dtype(sview, torch.uint8, out=dview)
            assert_bits(host(dview), ref_f32_to_u8(f), "f32->u8 " + what)
            assert_rim_intact(dbuf, dview, "f32->u8 " + what)


@gpu
def test_change_dtype_refuses_pitched(ops, dev):
    """u8 <-> fp32 needs dense images (include/vacv_hip.h): VACV_ERR_UNSUPPORTED, nothing written."""
    import torch
    u = rand((2, 5, 7, 3), np.uint8, 9)
    for spad, sbp, dpad, dbp in ((5, 0, 0, 0), (0, 3, 0, 0), (0, 0, 5, 0), (0, 0, 0, 3)):
        _, sview = place(u, dev, row_pad=spad, batch_pad=sbp)
        dbuf, dview = place(blank(u.shape, np.float32), dev, row_pad=dpad, batch_pad=dbp)
        unsupported(lambda: ops.change_dtype(sview, torch.float32, out=dview))
        assert_untouched(dbuf, "pitched u8->f32")
        _, sview = place(u.astype(np.float32), dev, row_pad=spad, batch_pad=sbp)
        dbuf, dview = place(blank(u.shape, np.uint8), dev, row_pad=dpad, batch_pad=dbp)
        unsupported(lambda: ops.change_dtype(sview, torch.uint8, out=dview))
        assert_untouched(dbuf, "pitched f32->u8")


# ---------------------------------------------------------------------------
# normalize: normalize_kernel's float4 and element-wise stores

NORM_SHAPES = [(5, 7, 3), (4, 8, 4), (6, 9, 1), (3, 10, 3)]  # (w, h, c): w*c % 4 = 3, 0, 2, 1


def _mean_std(c):
    return np.arange(c, dtype=np.float32) * 7 + 50.5, np.arange(c, dtype=np.float32) * 3 + 40.25


@gpu
@pytest.mark.parametrize("dtype", [np.uint8, np.float32])
def test_normalize_store_paths(ops, dev, dtype):
    """A thread owns 4 consecutive elements of a row and stores them as one
    float4 only when all 4 exist and d + e0 is 16-byte aligned: rows of w*c %
    4 = 0..3 elements end in partial chunks, and destination offsets 4 / 8, a
    destination row pad of 1 or 3 floats and a batch pad move the aligned
    chunks around.  Batch of 3, pitched source, bit-exact against
    normalize_value in numpy, intact rim."""
    cases = [(NHWC, w, h, c) for (w, h, c) in NORM_SHAPES] + [(NCHW, 5, 7, 3), (NCHW, 4, 8, 3)]
    for layout, w, h, c in cases:
        x = rand((3, h, w, c) if layout == NHWC else (3, c, h, w), dtype, w * h * c)
        mean, std = _mean_std(c)
        want = ref_normalize(x, mean, std, layout)
        for doff, spad, dpad, dbp in ((0, 0, 0, 0), (4, 0, 0, 0), (8, 5, 0, 0), (16, 0, 1, 0), (0, 3, 3, 5), (4, 5, 1, 2)):
            what = f"normalize {np.dtype(dtype).name} layout {layout} {w}x{h}x{c} dst off {doff} pads {spad}/{dpad}/{dbp}"
            _, sview = place(x, dev, layout, off=0, row_pad=spad, batch_pad=3 if spad else 0)
            dbuf, dview = place(blank(x.shape, np.float32), dev, layout, off=doff, row_pad=dpad, batch_pad=dbp)
            ops.normalize(sview, mean, std, layout=layout, out=dview)
            assert_bits(host(dview), want, what)
            assert_rim_intact(dbuf, dview, what)


@gpu
def test_normalize_statistics_mode_batch(ops, dev):
    """mean = None (NormSpec mode 2, per-image device statistics) on a batch
    of 3 odd-sized images: each image is normalised with ITS statistics.  u8:
    the exact statistics from integer sums; fp32: the library's own
    mean_stddev of the same batch (test_channel_sums_paths bounds those).  The
    source of this mode must be dense; the destination may sit anywhere."""
    for layout, w, h, c in [(NHWC, 5, 7, 3), (NHWC, 3, 11, 4), (NHWC, 7, 9, 1), (NCHW, 5, 7, 3)]:
        for dtype in (np.uint8, np.float32):
            x = rand((3, h, w, c) if layout == NHWC else (3, c, h, w), dtype, 31 * w + c)
            x[1] = x[1] // 2 if dtype == np.uint8 else x[1] * np.float32(0.5)  # images with different statistics
            _, sview = place(x, dev, layout, off=0)
            if dtype == np.uint8:
                sums, _, count = ref_sums(x, layout)
                mean, std = ref_mean_std(sums, count)
            else:
                m, s = ops.mean_stddev(sview, layout=layout)
                mean, std = host(m), host(s)
            want = ref_normalize(x, mean, std, layout)
            for doff, dpad in ((0, 0), (4, 0), (8, 3)):
                dbuf, dview = place(blank(x.shape, np.float32), dev, layout, off=doff, row_pad=dpad, batch_pad=dpad)
                ops.normalize(sview, layout=layout, out=dview)
                what = f"normalize auto {np.dtype(dtype).name} layout {layout} {w}x{h}x{c} off {doff} pad {dpad}"
                assert_bits(host(dview), want, what)
                assert_rim_intact(dbuf, dview, what)
    # a pitched source has no per-image statistics (dense only): refused, nothing written
    x = rand((3, 7, 5, 3), np.uint8, 5)
    _, sview = place(x, dev, row_pad=5)
    dbuf, dview = place(blank(x.shape, np.float32), dev)
    unsupported(lambda: ops.normalize(sview, out=dview))
    assert_untouched(dbuf, "normalize auto, pitched source")


# ---------------------------------------------------------------------------
# channel_sums / mean_stddev: channel_sums_kernel and stats_reduce_kernel

# (dtype, layout, n, h, w, c, base offset)
SUMS_CASES = (
    # image bytes not a multiple of 16 (u8: 35 c; fp32: 2,244 c, except c = 4): images 1 and 2 start off a
    # 16-byte boundary, scalar_only is set and every element goes through the tail loop
    [(np.uint8, NHWC, 3, 5, 7, c, 0) for c in (1, 2, 3, 4)] +
    [(np.float32, NHWC, 3, 17, 33, c, 0) for c in (1, 2, 3, 4)] +  # c = 4: 8,976-byte images, the vector body + tail
    # NCHW: one channel per plane; 35-byte u8 planes and 2,244-byte fp32 planes -> scalar_only
    [(np.uint8, NCHW, 3, 5, 7, 3, 0), (np.float32, NCHW, 3, 17, 33, 3, 0),
     # 64 x 64 x 3: 12,288 elements = 3 workgroups per image, aligned: the vector body of every CC, no tail
     (np.uint8, NHWC, 2, 64, 64, 3, 0), (np.float32, NHWC, 2, 64, 64, 3, 0),
     (np.uint8, NHWC, 2, 64, 64, 4, 0), (np.float32, NHWC, 2, 64, 64, 2, 0),
     (np.uint8, NCHW, 2, 64, 64, 3, 0), (np.float32, NCHW, 2, 64, 64, 3, 0),
     # 65 x 63 x 3 = 12,285 elements: vector body, then a tail split over the 2 workgroups
     (np.uint8, NHWC, 1, 65, 63, 3, 0), (np.float32, NHWC, 1, 65, 63, 3, 0),
     # a dense image at a misaligned base: scalar_only with the tail split over 3 workgroups
     (np.uint8, NHWC, 1, 64, 64, 3, 1), (np.float32, NHWC, 1, 64, 64, 3, 4)])


@gpu
@pytest.mark.parametrize("case", SUMS_CASES, ids=lambda t: f"{np.dtype(t[0]).name}-l{t[1]}-n{t[2]}-{t[3]}x{t[4]}x{t[5]}-off{t[6]}")
def test_channel_sums_paths(ops, dev, case):
    """channel_sums with both per_image values and mean_stddev: u8 equal to
    the integer sums, fp32 within the derived bound (assert_sums);
    mean_stddev bit-equal to stats_kernel's formula applied to the sums the
    library returned (the same kernels in the same fixed order)."""
    dtype, layout, n, h, w, c, off = case
    x = rand((n, h, w, c) if layout == NHWC else (n, c, h, w), dtype, h * w + c)
    if dtype == np.float32:
        x = (x - np.float32(90.0)).astype(np.float32)  # both signs: cancellation in Sum x
    _, view = place(x, dev, layout, off=off)
    per = host(ops.channel_sums(view, per_image=True, layout=layout))
    assert_sums(per, x, layout, True, f"per-image sums {case}")
    assert_sums(host(ops.channel_sums(view, per_image=False, layout=layout)), x, layout, False, f"batch sums {case}")
    m, s = ops.mean_stddev(view, layout=layout)
    wm, ws = ref_mean_std(per, h * w)
    assert_bits(host(m), wm, f"mean {case}")
    assert_bits(host(s), ws, f"stddev {case}")


@gpu
@pytest.mark.parametrize("dtype", [np.uint8, np.float32])
def test_stats_reduce_unrolled(ops, dev, dtype):
    """stats_reduce_kernel's 16-deep unrolled loop runs while t + 15 * 256 <
    terms, i.e. from 4,096 partials; with one workgroup per image that takes
    4,096 images.  4,396 images of 2 x 3 x 3 (79 KB as u8), per_image=False:
    every thread makes one unrolled pass and 1 or 2 single steps."""
    x = rand((4396, 3, 2, 3), dtype, 11)
    if dtype == np.float32:
        x = (x - np.float32(90.0)).astype(np.float32)
    _, view = place(x, dev)
    assert_sums(host(ops.channel_sums(view, per_image=False)), x, NHWC, False, "4,396-image batch sums")


@gpu
def test_stats_refuse_non_dense(ops, dev):
    """channel_sums and mean_stddev read one dense range per image (include/vacv_hip.h): a row-pitched or a
    batch-strided image is VACV_ERR_UNSUPPORTED."""
    for dtype in (np.uint8, np.float32):
        x = rand((4, 7, 5, 3), dtype, 13)
        _, pitched = place(x, dev, row_pad=4)
        _, dense = place(x, dev)
        for v in (pitched, dense[::2]):
            unsupported(lambda: ops.channel_sums(v, per_image=True))
            unsupported(lambda: ops.channel_sums(v, per_image=False))
            unsupported(lambda: ops.mean_stddev(v))
        nchw = np.ascontiguousarray(x.transpose(0, 3, 1, 2))
        _, pitched = place(nchw, dev, NCHW, row_pad=4)
        unsupported(lambda: ops.channel_sums(pitched, layout=NCHW))
        unsupported(lambda: ops.mean_stddev(pitched, layout=NCHW))


# ---------------------------------------------------------------------------
# vacv_resize at equal size

@gpu
def test_resize_equal_size_shortcut(ops, dev):
    """vacv_resize with dst size == src size copies (resize.cpp:58-61):
    INTER_LINEAR u8 -> u8 and fp32 -> fp32, INTER_CUBIC fp32 -> fp32 are row
    copies; INTER_CUBIC u8 -> fp32 widens -- dense through the flat dtype
    kernel, pitched through u8_to_f32_rows_kernel (it used to be refused at
    exactly this output size).  Dense, pitched source, pitched destination:
    the source values bit for bit, status OK, intact rim."""
    from vacv_amd import INTER_CUBIC, INTER_LINEAR
    w, h, c = 9, 13, 3
    for interp, sdt, ddt in ((INTER_LINEAR, np.uint8, np.uint8), (INTER_LINEAR, np.float32, np.float32),
                             (INTER_CUBIC, np.float32, np.float32), (INTER_CUBIC, np.uint8, np.float32)):
        for layout in (NHWC, NCHW):
            x = rand((2, h, w, c) if layout == NHWC else (2, c, h, w), sdt, 17 + interp)
            want = x.astype(ddt)
            for spad, dpad, doff in ((0, 0, 0), (5, 0, 0), (0, 3, 0), (16, 1, 16), (0, 0, 4)):
                what = (f"equal-size resize interp {interp} {np.dtype(sdt).name}->{np.dtype(ddt).name} layout {layout} "
                        f"pads {spad}/{dpad} off {doff}")
                _, sview = place(x, dev, layout, row_pad=spad, batch_pad=3 if spad else 0)
                dbuf, dview = place(blank(x.shape, ddt), dev, layout, off=doff, row_pad=dpad, batch_pad=2 * dpad)
                ops.resize(sview, w, h, interpolation=interp, layout=layout, out=dview)
                assert_bits(host(dview), want, what)
                assert_rim_intact(dbuf, dview, what)
