"""The perspective ROI entry points without a GPU: the status of every refused
call (fake pointers, before any HIP call) equals vacv_warp_affine_rois
[_normalize]'s on the same defect, singly and in pairs; vacv_invert_homography
by bits against a numpy float64 restatement; vacv_perspective_transform on
seeded convex quads."""
from __future__ import annotations

import ctypes
import itertools

import numpy as np
import pytest

OK, INVALID, UNSUPPORTED = 0, -1, -2
FP32, FP16, INT8 = 0, 1, 2
NCHW, NHWC = 0, 1
INTER_NEAREST, INTER_LINEAR, WARP_INVERSE_MAP = 0, 1, 16
BORDER_CONSTANT, BORDER_TRANSPARENT = 0, 5


@pytest.fixture(scope="module")
def lib():
    import vacv_amd
    if not vacv_amd._lib.HIP_LIB.exists():
        vacv_amd._lib.build()
    return vacv_amd._lib.load()


def img(ptr, n, w, h, c, dtype=INT8, layout=NHWC):
    from vacv_amd._lib import VacvImage
    return VacvImage(ptr, n, w, h, c, dtype, layout, 0, 0, 0)


# One defect = edits of the arguments of an otherwise valid call.  Keys: the
# fields of the two descriptors ("s_*", "d_*"; "s_none" / "d_none": a NULL
# descriptor), "m" (the matrices), "idx", "flags", "border", "mean", "std".
BASE = dict(s_ptr=0x1000, s_n=1, s_w=8, s_h=8, s_c=3, s_dtype=INT8, s_layout=NHWC, s_none=False,
            d_ptr=0x2000, d_n=3, d_w=4, d_h=4, d_c=3, d_dtype=None, d_layout=NHWC, d_none=False,
            m=0x3000, idx=0x4000, flags=INTER_LINEAR, border=BORDER_CONSTANT, mean=True, std=True)

DEFECTS = {
    "null src descriptor": (dict(s_none=True), INVALID, INVALID),
    "null dst descriptor": (dict(d_none=True), INVALID, INVALID),
    "null src data": (dict(s_ptr=None), INVALID, INVALID),
    "null dst data": (dict(d_ptr=None), INVALID, INVALID),
    "null matrices": (dict(m=None), INVALID, INVALID),
    "channel counts differ": (dict(d_c=4), INVALID, INVALID),
    "two frames, three ROIs, no index": (dict(s_n=2, idx=None), INVALID, INVALID),
    "FP16 source": (dict(s_dtype=FP16), UNSUPPORTED, UNSUPPORTED),
    "NCHW source": (dict(s_layout=NCHW), UNSUPPORTED, UNSUPPORTED),
    "five channels": (dict(s_c=5, d_c=5), UNSUPPORTED, None),  # _normalize: mean / stddev hold too few values
    "INTER_NEAREST": (dict(flags=INTER_NEAREST | WARP_INVERSE_MAP), UNSUPPORTED, UNSUPPORTED),
    "an unknown flag": (dict(flags=INTER_LINEAR | 32), UNSUPPORTED, UNSUPPORTED),
    "BORDER_TRANSPARENT": (dict(border=BORDER_TRANSPARENT), UNSUPPORTED, UNSUPPORTED),
    "a border mode out of range": (dict(border=-1), UNSUPPORTED, UNSUPPORTED),
    "a source one pixel wide": (dict(s_w=1), INVALID, INVALID),
    "a source one pixel high": (dict(s_h=1), INVALID, INVALID),
    "dst of the other dtype": (dict(d_dtype="other"), INVALID, INVALID),
    "planar dst": (dict(d_layout=NCHW), INVALID, OK),  # fine for _normalize with c = 3: no defect there
    "planar dst, two channels": (dict(s_c=2, d_c=2, d_layout=NCHW), INVALID, UNSUPPORTED),
    "a frame past the 32-bit offsets": (dict(s_w=40000, s_h=40000), UNSUPPORTED, UNSUPPORTED),
    "no statistics": (dict(mean=False, std=False), OK, UNSUPPORTED),
    "mean alone": (dict(std=False), OK, INVALID),
    "stddev alone": (dict(mean=False), OK, INVALID),
}


def call(lib, persp, normalize, edits):
    a = dict(BASE)
    a.update(edits)
    same = FP32 if normalize else a["s_dtype"]
    ddt = same if a["d_dtype"] is None else (INT8 if same == FP32 else FP32)
    src = img(a["s_ptr"], a["s_n"], a["s_w"], a["s_h"], a["s_c"], a["s_dtype"], a["s_layout"])
    dst = img(a["d_ptr"], a["d_n"], a["d_w"], a["d_h"], a["d_c"], ddt, a["d_layout"])
    sp = None if a["s_none"] else ctypes.byref(src)
    dp = None if a["d_none"] else ctypes.byref(dst)
    name = ("vacv_warp_perspective_rois" if persp else "vacv_warp_affine_rois") + ("_normalize" if normalize else "")
    fn = getattr(lib, name)
    if not normalize:
        return fn(sp, dp, a["m"], a["idx"], a["flags"], a["border"], None, None)
    mean = (ctypes.c_float * 4)(1, 2, 3, 4) if a["mean"] else None
    std = (ctypes.c_float * 4)(4, 5, 6, 7) if a["std"] else None
    return fn(sp, dp, a["m"], a["idx"], a["flags"], a["border"], None, mean, std, None)


@pytest.mark.parametrize("normalize", [False, True], ids=["rois", "rois_normalize"])
def test_every_check_singly(lib, normalize):
    """Each defect alone: the documented status, and vacv_warp_affine_rois' on the same call."""
    seen = 0
    for name, (edits, want_r, want_n) in DEFECTS.items():
        want = want_n if normalize else want_r
        if want == OK:  # no defect for this entry point: the call would reach the device
            continue
        got = call(lib, True, normalize, edits)
        assert got == call(lib, False, normalize, edits), name
        assert got != OK, name
        if want is not None:
            assert got == want, name
        seen += 1
    assert seen >= 20


@pytest.mark.parametrize("normalize", [False, True], ids=["rois", "rois_normalize"])
def test_checks_in_pairs_pin_the_order(lib, normalize):
    """Two defects at once: which status wins is the order of the checks, and it is vacv_warp_affine_rois'."""
    pairs = both = 0
    for (na, (ea, ra, nna)), (nb, (eb, rb, nnb)) in itertools.combinations(DEFECTS.items(), 2):
        wa, wb = (nna, nnb) if normalize else (ra, rb)
        if wa == OK and wb == OK:
            continue
        if set(ea) & set(eb):  # edits of the same argument do not combine
            continue
        edits = dict(ea)
        edits.update(eb)
        got = call(lib, True, normalize, edits)
        assert got == call(lib, False, normalize, edits), (na, nb)
        assert got in (INVALID, UNSUPPORTED), (na, nb)
        pairs += 1
        both += wa not in (OK, None) and wb not in (OK, None) and wa != wb
    assert pairs >= 150 and both >= 40  # pairs whose two statuses differ are the ones that show the order


def test_null_h_sits_where_null_m_does(lib):
    """NULL h after the descriptors, before everything else."""
    assert call(lib, True, False, dict(m=None, s_none=True)) == INVALID
    assert call(lib, True, False, dict(m=None, flags=INTER_NEAREST)) == INVALID       # before the options
    assert call(lib, True, False, dict(m=None, s_layout=NCHW)) == INVALID             # before the source's layout
    assert call(lib, True, True, dict(m=None, mean=False, std=False)) == UNSUPPORTED  # the statistics come first
    assert call(lib, True, True, dict(m=None, s_dtype=FP16)) == INVALID


# ---------------------------------------------------------------------------
# vacv_invert_homography

def np_invert_homography(h):
    """DESIGN 3.21 in numpy float64: every operation rounded separately."""
    with np.errstate(all="ignore"):
        a = [np.float64(v) for v in np.asarray(h, np.float32).reshape(9)]
        c = [a[4] * a[8] - a[5] * a[7], a[2] * a[7] - a[1] * a[8], a[1] * a[5] - a[2] * a[4],
             a[5] * a[6] - a[3] * a[8], a[0] * a[8] - a[2] * a[6], a[2] * a[3] - a[0] * a[5],
             a[3] * a[7] - a[4] * a[6], a[1] * a[6] - a[0] * a[7], a[0] * a[4] - a[1] * a[3]]
        det = (a[0] * c[0] + a[1] * c[3]) + a[2] * c[6]
        D = np.float64(1.0) / det if det != 0 else np.float64(0.0)
        return np.array([v * D for v in c], np.float64)


def lib_invert_homography(lib, h):
    h = np.ascontiguousarray(h, np.float32).reshape(9)
    out = np.full(9, 7.0, np.float64)
    st = lib.vacv_invert_homography(h.ctypes.data_as(ctypes.POINTER(ctypes.c_float)),
                                    out.ctypes.data_as(ctypes.POINTER(ctypes.c_double)))
    assert st == OK
    return out


def homography_inputs():
    rng = np.random.default_rng(20261021)
    hs = [rng.uniform(-3, 3, 9) * 10.0 ** rng.integers(-3, 4) for _ in range(1000)]
    for _ in range(50):  # affine maps: last row 0 0 1
        h = rng.uniform(-3, 3, 9)
        h[6:] = (0, 0, 1)
        hs.append(h)
    for _ in range(50):  # the shape of a real one: a small projective row
        h = rng.uniform(-2, 2, 9)
        h[6:8] = rng.uniform(-2e-3, 2e-3, 2)
        h[8] = 1
        hs.append(h)
    return np.asarray(hs, np.float32)


def test_invert_homography_bits(lib):
    hs = homography_inputs()
    for h in hs:
        got, want = lib_invert_homography(lib, h), np_invert_homography(h)
        assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), (h.tolist(), got.tolist(), want.tolist())
        assert np.isfinite(got).all() and got.any()
    # affine: the last row of the adjugate is (0, 0, det2) and the rest is the 2x3 inverse
    h = np.array([2, 0.5, 3, -0.25, 4, 1, 0, 0, 1], np.float32)
    got = lib_invert_homography(lib, h)
    assert got[6] == 0 and got[7] == 0
    assert np.allclose(got.reshape(3, 3) @ h.reshape(3, 3).astype(np.float64), np.eye(3), atol=1e-15)


def test_invert_homography_singular_and_non_finite(lib):
    zeros = np.zeros(9, np.float64)
    for h in ([0] * 9, [1, 2, 3, 2, 4, 6, 0.5, 0.25, 1], [1, 2, 3, 4, 5, 6, 5, 7, 9], [1, 0, 0, 0, 1, 0, 0, 0, 0]):
        got = lib_invert_homography(lib, h)
        assert (got == 0).all(), (h, got)  # cofactor * 0: a zero of either sign
        assert np.array_equal(got.view(np.uint64), np_invert_homography(h).view(np.uint64)), (h, got)
    inf, nan = np.inf, np.nan
    for h in ([nan] * 9, [1, nan, 0, 0, 1, 0, 0, 0, 1], [inf, 0, 0, 0, 1, 0, 0, 0, 1], [1, 0, -inf, 0, 1, 0, 0, 0, 1],
              [1, 0, 0, 0, 1, 0, 0, inf, 1], [1, 0, 0, 0, 1, 0, nan, 0, 1]):
        got, want = lib_invert_homography(lib, h), np_invert_homography(h)
        assert not np.isfinite(want).all()
        assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), (h, got.tolist(), want.tolist())
    assert lib.vacv_invert_homography(None, zeros.ctypes.data_as(ctypes.POINTER(ctypes.c_double))) == INVALID
    h = np.zeros(9, np.float32)
    assert lib.vacv_invert_homography(h.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), None) == INVALID


# ---------------------------------------------------------------------------
# vacv_perspective_transform

def convex_quad(rng, size=2048.0):
    """Four points on a circle inside the frame, one per quadrant (TL, TR, BR, BL): always convex."""
    r = rng.uniform(40.0, size / 2 - 1)
    cx, cy = rng.uniform(r, size - r, 2)
    ang = np.deg2rad(np.array([225.0, 315.0, 45.0, 135.0]) + rng.uniform(-30, 30, 4))
    return np.stack([cx + r * np.cos(ang), cy + r * np.sin(ang)], 1).astype(np.float32)


def lib_perspective_transform(lib, sq, dq):
    sq, dq = np.ascontiguousarray(sq, np.float32).reshape(8), np.ascontiguousarray(dq, np.float32).reshape(8)
    out = np.zeros(9, np.float32)
    fp = ctypes.POINTER(ctypes.c_float)
    return lib.vacv_perspective_transform(sq.ctypes.data_as(fp), dq.ctypes.data_as(fp), out.ctypes.data_as(fp)), out


def apply_h(h, pts):
    h = np.asarray(h, np.float64).reshape(3, 3)
    p = np.concatenate([np.asarray(pts, np.float64), np.ones((len(pts), 1))], 1) @ h.T
    return p[:, :2] / p[:, 2:]


def test_perspective_transform_maps_the_corners(lib):
    """0.01 px: the fp32 rounding of nine coefficients (2^-24 relative each,
    coordinates <= 2048, a handful of terms: about 5e-4 px) with a 20x margin."""
    rng = np.random.default_rng(20261022)
    worst = 0.0
    for _ in range(200):
        sq, dq = convex_quad(rng), convex_quad(rng)
        st, h = lib_perspective_transform(lib, sq, dq)
        assert st == OK and h[8] == 1
        err = np.abs(apply_h(h, sq) - dq.astype(np.float64)).max()
        worst = max(worst, err)
        assert err <= 0.01, (sq.tolist(), dq.tolist(), h.tolist(), err)
    print(f"perspective_transform: worst corner error {worst:.3g} px")
    # a rectangle onto itself is the identity
    rect = np.array([[0, 0], [111, 0], [111, 63], [0, 63]], np.float32)
    st, h = lib_perspective_transform(lib, rect, rect)
    assert st == OK and np.allclose(h, np.eye(3).reshape(9), atol=1e-6)


def test_perspective_transform_refuses_degenerate_quads(lib):
    ok = np.array([[0, 0], [100, 0], [100, 50], [0, 50]], np.float32)
    for bad in ([[10, 10], [20, 20], [30, 30], [0, 50]],         # three collinear points
                [[0, 0], [64, 0], [128, 0], [7, 90]],
                [[5, 5], [5, 5], [90, 80], [3, 70]],            # two equal points
                [[1, 2], [1, 2], [1, 2], [1, 2]]):
        st, _ = lib_perspective_transform(lib, np.array(bad, np.float32), ok)
        assert st == INVALID, bad
    fp = ctypes.POINTER(ctypes.c_float)
    assert lib.vacv_perspective_transform(None, ok.ctypes.data_as(fp), ok.ctypes.data_as(fp)) == INVALID
    nanq = ok.copy()
    nanq[2, 0] = np.nan
    assert lib_perspective_transform(lib, nanq, ok)[0] == INVALID
