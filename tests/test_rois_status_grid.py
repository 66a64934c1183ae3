"""The host path of the batched-ROI operators, pinned without a GPU.

tests/golden/rois_status_grid.npz holds the status code that the commit named
in its metadata returned for every row of tests/golden/make_status_grid.py's
grid: the six ROI entry points and the other callers of the host helpers they
share, with defects in pairs, so that the ORDER of the argument checks is
pinned and not only their presence.  The rows that commit rejected are
replayed here; the few it accepted (VACV_ERR_HIP on the device-less host that
recorded them) are stored but never called, so no call here reaches a launch.

The Python wrappers' own argument checks run before the library is called;
their messages are the recorded ones, as literals.
"""
from __future__ import annotations

import importlib.util
import json

import numpy as np
import pytest

from conftest import GOLDEN

INVALID, UNSUPPORTED = -1, -2


def _no_device():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present: the fixture's accepted rows were told apart on a GPU-less host")


@pytest.fixture(scope="module")
def grid():
    spec = importlib.util.spec_from_file_location("make_status_grid", GOLDEN / "make_status_grid.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_rois_status_grid_matches_the_recorded_statuses(grid):
    _no_device()
    import vacv_amd
    if not vacv_amd._lib.HIP_LIB.exists():
        vacv_amd._lib.build()
    want = np.load(grid.FIXTURE)
    meta = json.loads(bytes(want["meta"]).decode())
    assert len(meta["commit"]) == 40 and meta["grid_version"] == grid.GRID_VERSION
    assert sorted(meta["rows"]) == grid.entry_points() == sorted(k for k in want.files if k != "meta")

    caller = grid.Caller(vacv_amd._lib.HIP_LIB)
    at = dict.fromkeys(meta["rows"], 0)
    for g in grid.grids():
        recorded = want[g.fn][at[g.fn]:at[g.fn] + g.rows]
        at[g.fn] += g.rows
        assert recorded.size == g.rows, f"{g.fn}: the grid no longer has the recorded shape"
        rejected = (recorded == INVALID) | (recorded == UNSUPPORTED)
        got = caller.statuses(g, only=rejected)
        bad = np.flatnonzero(rejected & (got != recorded))
        for row in bad[:10]:
            print(f"{g.fn}: recorded {recorded[row]}, got {got[row]} for {g.describe(row)}")
        assert bad.size == 0, f"{g.fn}: {bad.size} of {g.rows} rows changed status (first ones above)"
    for fn, rows in meta["rows"].items():
        assert at[fn] == rows == want[fn].size, fn
        accepted = int(((want[fn] != INVALID) & (want[fn] != UNSUPPORTED)).sum())
        assert accepted <= 0.01 * rows, f"{fn}: {accepted} of {rows} recorded rows are never replayed"


def test_rois_python_argument_checks():
    """Every ValueError of the six ops.*_rois* wrappers that is raised before
    the library is called, on CPU tensors: the text is the recorded one."""
    _no_device()
    import torch
    from vacv_amd import ops

    frames = torch.zeros((2, 8, 8, 3), dtype=torch.uint8)
    yuv = torch.zeros((2, 12, 8), dtype=torch.uint8)
    mean, std = [1.0, 2.0, 3.0], [4.0, 5.0, 6.0]
    ms, rects = np.zeros((3, 6), np.float32), np.zeros((3, 4), np.int32)
    ms_msgs = ("ms", np.zeros((3, 5), np.float32), "ms must have shape (n, 6) or (n, 2, 3), got (3, 5)",
               np.zeros((0, 6), np.float32), "ms holds no matrix")
    rects_msgs = ("rects", np.zeros((3, 3), np.int32), "rects must have shape (n, 4), got (3, 3)",
                  np.zeros((0, 4), np.int32), "rects holds no rect")
    cases = [(ops.warp_affine_rois, frames, ms, ms_msgs, False),
             (ops.warp_affine_rois_normalize, frames, ms, ms_msgs, True),
             (ops.crop_resize_rois, frames, rects, rects_msgs, False),
             (ops.crop_resize_rois_normalize, frames, rects, rects_msgs, True),
             (ops.cvt_color_warp_affine_rois, yuv, ms, ms_msgs, False),
             (ops.cvt_color_warp_affine_rois_normalize, yuv, ms, ms_msgs, True)]
    for fn, src, good, (what, misshapen, shape_msg, empty, empty_msg), normalize in cases:
        stats = (mean, std) if normalize else ()

        def raises(text, s, arr, st=stats, **kw):
            with pytest.raises(ValueError) as e:
                fn(s, arr, 4, 4, *st, **kw)
            assert str(e.value) == text, (fn.__name__, str(e.value))

        raises(shape_msg, src, misshapen)
        raises(empty_msg, src, empty)
        raises(f"{what} must be torch.{'float32' if what == 'ms' else 'int32'}, not torch.float64", src,
               torch.zeros(good.shape, dtype=torch.float64))
        raises("src_index must have shape (3,), got (2,)", src, good, src_index=torch.zeros(2, dtype=torch.int32))
        raises("src_index must be torch.int32, not torch.int64", src, good, src_index=torch.zeros(3, dtype=torch.int64))
        raises("src_index must be contiguous", src, good, src_index=torch.zeros(6, dtype=torch.int32)[::2])
        raises("without src_index, src must hold 1 or 3 images, not 2", src, good)
        # two defects: the array's shape is looked at before src_index
        raises(shape_msg, src, misshapen, src_index=torch.zeros(3, dtype=torch.int64))
        if normalize:
            need = f"{fn.__name__} needs mean and stddev (no per-image statistics for ROIs)"
            raises(need, src[:1], good, st=(None, std))
            raises(need, src[:1], good, st=(mean, None))
            raises(need, src[:1], good, st=(None, None))
            # ... and the array and the frames before the statistics
            raises(shape_msg, src[:1], misshapen, st=(None, None))
            raises("without src_index, src must hold 1 or 3 images, not 2", src, good, st=(None, None))
        if src is yuv:
            # frames of too many dimensions are refused before the array is looked at
            for arr in (good, misshapen):
                raises("expected a 2-4 dimensional image tensor, got shape (1, 2, 12, 8, 1, 1)", src.unsqueeze(-1), arr)
