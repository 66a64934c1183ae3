#!/usr/bin/env python3
"""Record the status code of a grid of calls into the C ABI, defects in pairs.

    python tests/golden/make_status_grid.py LIBVACV_HIP_SO COMMIT [OUT.npz]

The grid covers the six batched-ROI entry points and the other callers of the
host helpers they share (the YUV420sp geometry check and fused_normalize).
Every call takes descriptors with fake data pointers; the argument checks run
before any HIP call, so on a host without a device a call that passes them
comes back as VACV_ERR_HIP and nothing is launched.  Run it there.

tests/golden/rois_status_grid.npz is this script's output for a build of the
commit named in its metadata, the parent of the change that merged the ROI
host paths.  It pins which check fails first for every row: it is never
regenerated from the code under test (tests/test_rois_status_grid.py replays
the rejected rows; pass OUT.npz to compare a later build on every row).

One int8 array per entry point: the statuses of its grids' rows, one grid
after the other, each in itertools.product order of its axes.
"""
from __future__ import annotations

import ctypes
import itertools
import json
import sys
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
FIXTURE = HERE / "rois_status_grid.npz"
GRID_VERSION = 1

INVALID, UNSUPPORTED, ERR_HIP = -1, -2, -3
FP32, FP16, INT8, NO_DTYPE = 0, 1, 2, 7
NCHW, NHWC = 0, 1
LINEAR, NEAREST, INVERSE = 1, 0, 16
HUGE_ROW = (1 << 20) + 1


class Image(ctypes.Structure):  # vacv_image (include/vacv_hip.h)
    _fields_ = [("data", ctypes.c_void_p), ("n", ctypes.c_int32), ("w", ctypes.c_int32), ("h", ctypes.c_int32),
                ("c", ctypes.c_int32), ("dtype", ctypes.c_int32), ("layout", ctypes.c_int32),
                ("row_pitch", ctypes.c_int64), ("plane_pitch", ctypes.c_int64), ("batch_pitch", ctypes.c_int64)]


# ---- descriptors: a base and what differs from it ---------------------------

def variants(base: dict, factors: dict, most: int, least: int = 0) -> list:
    """`base` with `least`..`most` of its fields replaced, every combination."""
    out = []
    for k in range(least, most + 1):
        for names in itertools.combinations(factors, k):
            for vals in itertools.product(*(factors[f] for f in names)):
                out.append({**base, **dict(zip(names, vals))})
    return out


def desc(ptr, n, wh, c, dtype=INT8, layout=NHWC, pitch=0) -> dict:
    return dict(ptr=ptr, n=n, wh=wh, c=c, dtype=dtype, layout=layout, pitch=pitch)


SRC_PTR, DST_PTR, ARR, IDX = 0x1000, 0x2000, 0x3000, 0x4000  # never dereferenced on the host

BGR = desc(SRC_PTR, 1, (8, 8), 3)
BGR_DEFECTS = dict(ptr=(None,), n=(2, 3), wh=((1, 8), (8, 1), (1, 1)), c=(1, 2, 4, 5), dtype=(FP32, FP16, NO_DTYPE),
                   layout=(NCHW,), pitch=(1,))
YUV = desc(SRC_PTR, 1, (8, 12), 1)  # an 8 x 8 NV21 / NV12 frame
YUV_DEFECTS = dict(ptr=(None,), n=(2, 3), wh=((7, 12), (8, 13), (8, 10), (8, 7), (1, 12), (8, 2), (7, 13)), c=(2, 3),
                   dtype=(FP32, FP16, NO_DTYPE), layout=(NCHW,), pitch=(1,))
GRAY = desc(SRC_PTR, 1, (8, 8), 1)

# the ROI destinations: three crops
ROI_DST = desc(DST_PTR, 3, (4, 4), 3)
DST_DEFECTS = dict(ptr=(None,), wh=((HUGE_ROW, 1),), c=(1, 2, 4, 5), dtype=(FP32, FP16), layout=(NCHW,))
TRIPLES = dict(c=(1, 2, 4, 5), dtype=(FP32, FP16), layout=(NCHW,))
# one image per source image: the other operators
ONE_DST = desc(DST_PTR, 1, (8, 8), 3)
ONE_DEFECTS = dict(DST_DEFECTS, n=(2,), wh=((4, 4), (HUGE_ROW, 1), (HUGE_ROW, 4)))


def with_null(descs: list) -> list:
    return [None] + descs


def dsts(base: dict, defects: dict) -> list:
    return with_null(variants(base, defects, 2) + variants(base, TRIPLES, 3, 3))


ROI_SRCS = with_null(variants(BGR, BGR_DEFECTS, 1)) + [YUV]
ROI_SRC_PAIRS = variants(BGR, BGR_DEFECTS, 2, 2)
YUV_SRCS = with_null(variants(YUV, YUV_DEFECTS, 1)) + [BGR]
YUV_SRC_PAIRS = variants(YUV, YUV_DEFECTS, 2, 2)
ROI_DSTS = dsts(ROI_DST, DST_DEFECTS)
# beside the source pairs: good u8 / fp32 / planar outputs and one defect of each kind
FEW_DSTS = [ROI_DST, {**ROI_DST, "dtype": FP32}, {**ROI_DST, "dtype": FP32, "layout": NCHW}, {**ROI_DST, "c": 4},
            {**ROI_DST, "dtype": FP32, "layout": NCHW, "c": 2}, {**ROI_DST, "wh": (HUGE_ROW, 1)}, None]
ONE_DSTS = dsts(ONE_DST, ONE_DEFECTS)
COLOR_SRCS = YUV_SRCS + variants(GRAY, dict(dtype=(FP32, FP16), layout=(NCHW,), n=(2,)), 1)

PTRS = (ARR, None)       # the device array (matrices / rects), then src_index
# (flags, border mode): good, then one defect, then two
WARP_OPTS = ((LINEAR, 0), (LINEAR | INVERSE, 4), (NEAREST, 0), (LINEAR | 32, 0), (LINEAR, 5), (LINEAR, -1),
             (NEAREST | INVERSE, 5), (2, 16))
FEW_WARP_OPTS = ((LINEAR, 0), (NEAREST, 0), (LINEAR, 5))
# (interpolation, mode)
LINEAR_OPTS = ((LINEAR, 0), (LINEAR, 2), (NEAREST, 0), (2, 0), (LINEAR | 16, 1), (LINEAR, -1), (LINEAR, 3), (3, 99))
FEW_LINEAR_OPTS = ((LINEAR, 0), (2, 0), (LINEAR, 3))
RESIZE_OPTS = tuple((i, m) for i in (0, 1, 2, 3, 4, 5, -1) for m in (0, 2, -1, 3))
ROI_CODES = (93, 90, 94)  # NV21 -> BGR, NV12 -> RGB, a code of OpenCV's arithmetic
FEW_CODES = (93, 99)
CODES = (93, 92, 91, 90, 8, 94, 95, 96, 97, 99, 98, 0, -1)
STATS = ("both", "none", "mean", "std")  # which of mean / stddev are given


# ---- the grids ---------------------------------------------------------------

class Grid:
    """One entry point over the product of `axes` ((name, values) pairs);
    `args(*values)` orders one row's values as the C function takes them."""

    def __init__(self, fn: str, axes: list, args):
        self.fn, self.axes, self.args = fn, axes, args
        self.rows = int(np.prod([len(v) for _, v in axes]))

    def describe(self, row: int) -> str:
        idx = np.unravel_index(row, [len(v) for _, v in self.axes])
        return ", ".join(f"{name}={vals[i]}" for (name, vals), i in zip(self.axes, idx))


def grids() -> list:
    g = []

    def roi(fn, srcs, pairs, opts, few_opts, arr, codes=None, few_codes=None):
        for suffix, stats in (("", None), ("_normalize", STATS)):
            for s, d, o, k in ((srcs, ROI_DSTS, opts, codes), (pairs, FEW_DSTS, few_opts, few_codes)):
                axes = [("src", s), ("dst", d), (arr, PTRS), ("src_index", (IDX, None)), ("opts", o)]
                if k:
                    axes.append(("code", k))
                if stats:
                    axes.append(("stats", stats))
                g.append(Grid(fn + suffix, axes, _roi_args(arr == "m", bool(k), bool(stats))))

    roi("vacv_warp_affine_rois", ROI_SRCS, ROI_SRC_PAIRS, WARP_OPTS, FEW_WARP_OPTS, "m")
    roi("vacv_crop_resize_rois", ROI_SRCS, ROI_SRC_PAIRS, LINEAR_OPTS, FEW_LINEAR_OPTS, "rects")
    roi("vacv_cvt_color_warp_affine_rois", YUV_SRCS, YUV_SRC_PAIRS, WARP_OPTS, FEW_WARP_OPTS, "m", ROI_CODES,
        FEW_CODES)

    # the other callers of the YUV420sp geometry check and of fused_normalize
    sd = [("src", COLOR_SRCS), ("dst", ONE_DSTS)]
    g.append(Grid("vacv_cvt_color", sd + [("code", CODES)], lambda s, d, code: (s, d, code, None)))
    g.append(Grid("vacv_cvt_color_normalize", sd + [("code", CODES), ("stats", STATS)],
                  lambda s, d, code, st: (s, d, code, *st, None)))
    sd = [("src", YUV_SRCS), ("dst", ONE_DSTS)]
    g.append(Grid("vacv_cvt_color_resize", sd + [("code", CODES), ("opts", LINEAR_OPTS)],
                  lambda s, d, code, o: (s, d, code, *o, None)))
    g.append(Grid("vacv_cvt_color_resize_normalize", sd + [("code", ROI_CODES), ("opts", LINEAR_OPTS), ("stats", STATS)],
                  lambda s, d, code, o, st: (s, d, code, *o, *st, None)))
    sd = [("src", ROI_SRCS + ROI_SRC_PAIRS), ("dst", ONE_DSTS)]
    g.append(Grid("vacv_resize_normalize", sd + [("opts", RESIZE_OPTS), ("stats", STATS)],
                  lambda s, d, o, st: (s, d, *o, *st, None)))
    g.append(Grid("vacv_warp_affine_normalize", sd + [("m", ("M", None)), ("opts", WARP_OPTS), ("stats", STATS)],
                  lambda s, d, m, o, st: (s, d, m, *o, None, *st, None)))
    return g


def _roi_args(border: bool, code: bool, stats: bool):
    """(src, dst, [code], array, src_index, opts..., [border_value], [mean, stddev], stream)"""
    bv = (None,) if border else ()

    def args(s, d, a, i, o, *rest):
        k = (rest[0],) if code else ()
        st = rest[-1] if stats else ()
        return (s, d, *k, a, i, *o, *bv, *st, None)
    return args


def entry_points() -> list:
    return sorted({g.fn for g in grids()})


# ---- calling -----------------------------------------------------------------

class Caller:
    """Turns a row's values into ctypes arguments (descriptors and statistics
    are built once and kept alive here) and calls the library."""

    def __init__(self, lib_path):
        self.lib = ctypes.CDLL(str(lib_path))
        self._keep = {}
        mean = (ctypes.c_float * 16)(*range(1, 17))
        std = (ctypes.c_float * 16)(*range(4, 20))
        self._m = (ctypes.c_float * 6)(1, 0, 0, 0, 1, 0)
        self._stats = {"both": (mean, std), "none": (None, None), "mean": (mean, None), "std": (None, std)}

    def _c(self, v):
        if isinstance(v, dict):
            key = tuple(v.items())
            if key not in self._keep:
                w, h = v["wh"]
                im = Image(v["ptr"], v["n"], w, h, v["c"], v["dtype"], v["layout"], v["pitch"], 0, 0)
                self._keep[key] = (im, ctypes.byref(im))
            return self._keep[key][1]
        if isinstance(v, str):
            return self._stats[v] if v in self._stats else self._m
        if isinstance(v, int):
            return ctypes.c_void_p(v)  # ARR / IDX: bare addresses as pointers, not as C ints
        return v

    def statuses(self, grid: Grid, only=None) -> np.ndarray:
        """The status of every row, or of the rows whose index is in `only`
        (the others 0)."""
        fn = getattr(self.lib, grid.fn)
        fn.restype = ctypes.c_int
        axes = [[self._c(v) for v in vals] for _, vals in grid.axes]
        out = np.zeros(grid.rows, np.int8)
        args = grid.args
        for row, vals in enumerate(itertools.product(*axes)):
            if only is None or only[row]:
                out[row] = fn(*args(*vals))
        return out


def record(lib_path) -> dict:
    caller = Caller(lib_path)
    out = {}
    for g in grids():
        out.setdefault(g.fn, []).append(caller.statuses(g))
    return {fn: np.concatenate(parts) for fn, parts in out.items()}


def main(argv) -> int:
    if len(argv) not in (3, 4):
        print(__doc__)
        return 2
    got = record(argv[1])
    rows = 0
    for fn, st in got.items():
        accepted = int(((st != INVALID) & (st != UNSUPPORTED)).sum())
        rows += st.size
        print(f"{fn}: {st.size} rows, {accepted} accepted ({100.0 * accepted / st.size:.3f} %), "
              f"statuses {sorted(set(st.tolist()))}")
    print(f"{rows} rows")
    if len(argv) == 4:
        want = np.load(argv[3])
        bad = [fn for fn in got if not np.array_equal(want[fn], got[fn])]
        print("differs from", argv[3], "in", bad if bad else "no row")
        return 1 if bad else 0
    meta = json.dumps({"commit": argv[2], "grid_version": GRID_VERSION, "rows": {fn: int(st.size) for fn, st in got.items()}})
    np.savez_compressed(FIXTURE, meta=np.frombuffer(meta.encode(), np.uint8), **got)
    print("wrote", FIXTURE, FIXTURE.stat().st_size, "bytes")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
