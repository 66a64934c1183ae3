"""Algorithmic byte counts for the roofline.

B_alg(image) = bytes of every source row that carries a non-zero vertical
weight for some output row (each counted once) + bytes written.  For the
elementwise operators it is simply input + output bytes.  The row weights are
recomputed here with the reference's arithmetic (numpy float32/float64 in the
same order as vacv_semantics.hpp), so the count matches what the resize
kernel actually stages.
"""
from __future__ import annotations

import numpy as np

HBM_PEAK_GBS = 8000.0   # MI355X HBM3E spec peak (MI355X_MICROARCH.md)


def _sat_short_away(x: np.ndarray) -> np.ndarray:
    x = x.astype(np.float32)
    r = x + np.where(x >= 0, np.float32(0.5), np.float32(-0.5)).astype(np.float32)
    return np.clip(np.trunc(r), -32768, 32767).astype(np.int32)


def linear_row_weights(n_in: int, n_out: int, mode: int = 0):
    d = np.arange(n_out, dtype=np.float64)
    if mode == 0:
        s = np.float64(np.float32(n_in) / np.float32(n_out))
    else:
        s = np.float64(n_in) / np.float64(n_out)
    f = ((d + 0.5) * s - 0.5).astype(np.float32)
    i = np.floor(f).astype(np.int64)
    f = (f - i.astype(np.float32)).astype(np.float32)
    lo = i < 0
    i[lo], f[lo] = 0, np.float32(0)
    hi = i >= n_in - 1
    i[hi], f[hi] = n_in - 2, np.float32(1)
    a = ((np.float32(1) - f) * np.float32(2048)).astype(np.float32)
    b = (f * np.float32(2048)).astype(np.float32)
    if mode == 2:
        w0, w1 = np.rint(a).astype(np.int32), np.rint(b).astype(np.int32)
    else:
        w0, w1 = _sat_short_away(a), _sat_short_away(b)
    return i, w0, w1


def weighted_rows_linear(n_in: int, n_out: int, mode: int = 0) -> int:
    i, w0, w1 = linear_row_weights(n_in, n_out, mode)
    rows = set(i[w0 != 0].tolist()) | set((i[w1 != 0] + 1).tolist())
    return len(rows)


def weighted_rows_cubic(n_in: int, n_out: int) -> int:
    A = np.float32(-0.75)
    rows = set()
    s = np.float64(n_in) / np.float64(n_out)
    for d in range(n_out):
        f = np.float32((d + 0.5) * s - 0.5)
        i = int(np.floor(f))
        f = np.float32(f - np.float32(i))
        t0, t1, t2 = np.float32(f + 1), f, np.float32(1 - f)
        c0 = A * t0 * t0 * t0 - np.float32(5) * A * t0 * t0 + np.float32(8) * A * t0 - np.float32(4) * A
        c1 = (A + 2) * t1 * t1 * t1 - (A + 3) * t1 * t1 + np.float32(1)
        c2 = (A + 2) * t2 * t2 * t2 - (A + 3) * t2 * t2 + np.float32(1)
        c3 = np.float32(1) - c0 - c1 - c2
        c = [c0, c1, c2, c3]
        if i <= -1:
            i, c = 1, [1 - c[3], c[3], 0, 0]
        if i == 0:
            i, c = 1, [c[0] + c[1], c[2], c[3], 0]
        if i == n_in - 2:
            i, c = n_in - 3, [0, c[0], c[1], c[2] + c[3]]
        if i >= n_in - 1:
            i, c = n_in - 3, [0, 0, c[0], 1 - c[0]]
        for j in range(4):
            if c[j] != 0:
                rows.add(i - 1 + j)
    return len(rows)


def resize_bytes(w_in: int, h_in: int, c: int, w_out: int, h_out: int, in_esize: int = 1, out_esize: int = 1,
                 cubic: bool = False, mode: int = 0) -> int:
    rows = weighted_rows_cubic(h_in, h_out) if cubic else weighted_rows_linear(h_in, h_out, mode)
    return rows * w_in * c * in_esize + w_out * h_out * c * out_esize


def yuv_resize_bytes(w_in: int, h_in: int, w_out: int, h_out: int, out_esize: int = 4, mode: int = 0) -> int:
    """B_alg of the fused YUV420sp -> BGR -> resize kernel: every weighted Y row,
    every chroma row (one per Y row pair) that a weighted Y row needs, and the
    3-channel output."""
    i, w0, w1 = linear_row_weights(h_in, h_out, mode)
    rows = set(i[w0 != 0].tolist()) | set((i[w1 != 0] + 1).tolist())
    chroma = {r >> 1 for r in rows}
    return (len(rows) + len(chroma)) * w_in + w_out * h_out * 3 * out_esize


def _clip_polygon(poly, w: float, h: float):
    """Sutherland-Hodgman: the convex polygon `poly` cut to [0, w] x [0, h]."""
    def cut(pts, inside, cross):
        out = []
        for i, p in enumerate(pts):
            q = pts[(i + 1) % len(pts)]
            if inside(p):
                out.append(p)
                if not inside(q):
                    out.append(cross(p, q))
            elif inside(q):
                out.append(cross(p, q))
        return out

    def at_x(x0):
        return lambda p, q: (x0, p[1] + (q[1] - p[1]) * (x0 - p[0]) / (q[0] - p[0]))

    def at_y(y0):
        return lambda p, q: (p[0] + (q[0] - p[0]) * (y0 - p[1]) / (q[1] - p[1]), y0)

    for inside, cross in ((lambda p: p[0] >= 0, at_x(0.0)), (lambda p: p[0] <= w, at_x(float(w))),
                          (lambda p: p[1] >= 0, at_y(0.0)), (lambda p: p[1] <= h, at_y(float(h)))):
        if not poly:
            break
        poly = cut(poly, inside, cross)
    return poly


def _roi_source_pixels(w_in: int, h_in: int, w_out: int, h_out: int, ms, inverse_map: bool):
    """Per map: the whole pixels of the ROI's source parallelogram clipped to the frame."""
    for m in np.asarray(ms, dtype=np.float64).reshape(-1, 6):
        if not np.all(np.isfinite(m)):
            continue
        if inverse_map:
            inv = m
        else:
            det = m[0] * m[4] - m[1] * m[3]
            if det == 0:
                continue
            a, b, d, e = m[4] / det, -m[1] / det, -m[3] / det, m[0] / det
            inv = np.array([a, b, -a * m[2] - b * m[5], d, e, -d * m[2] - e * m[5]])
        corners = [(inv[0] * x + inv[1] * y + inv[2], inv[3] * x + inv[4] * y + inv[5])
                   for x, y in ((0, 0), (w_out, 0), (w_out, h_out), (0, h_out))]
        poly = _clip_polygon(corners, w_in, h_in)
        if len(poly) < 3:
            continue
        area = 0.5 * abs(sum(p[0] * q[1] - q[0] * p[1] for p, q in zip(poly, poly[1:] + poly[:1])))
        yield int(round(area))


def yuv_warp_rois_bytes(w_in: int, h_in: int, w_out: int, h_out: int, ms, out_esize: int = 1,
                        inverse_map: bool = False) -> int:
    """B_alg of vacv_cvt_color_warp_affine_rois[_normalize]: the 3-channel
    output of every ROI plus each ROI's clipped source parallelogram (as
    warp_rois_bytes finds it, in the decoded w_in x h_in frame) at 1 byte per
    pixel of Y and the chroma covering it at half a byte per pixel (one VU
    pair per 2 x 2 pixels; an odd pixel count rounds the half byte up)."""
    n = np.asarray(ms, dtype=np.float64).reshape(-1, 6).shape[0]
    total = n * w_out * h_out * 3 * out_esize
    for px in _roi_source_pixels(w_in, h_in, w_out, h_out, ms, inverse_map):
        total += px + (px + 1) // 2
    return int(total)


def yuv_warp_rois_standardize_bytes(w_in: int, h_in: int, w_out: int, h_out: int, ms, stats: bool = False,
                                    inverse_map: bool = False) -> int:
    """B_alg of vacv_cvt_color_warp_affine_rois_standardize: yuv_warp_rois_bytes
    with an fp32 output -- the u8 ROI and its statistics live in LDS and cost
    no memory traffic -- plus, with stats, the two (n, 3) fp32 arrays."""
    n = np.asarray(ms, dtype=np.float64).reshape(-1, 6).shape[0]
    return yuv_warp_rois_bytes(w_in, h_in, w_out, h_out, ms, 4, inverse_map) + (2 * n * 3 * 4 if stats else 0)


def warp_rois_bytes(w_in: int, h_in: int, c: int, w_out: int, h_out: int, ms, in_esize: int = 1,
                    out_esize: int = 1, inverse_map: bool = False) -> int:
    """B_alg of vacv_warp_affine_rois: the output bytes of every ROI plus the
    bytes of each ROI's source parallelogram -- the image of the output
    rectangle [0, w_out] x [0, h_out] under the dst -> src map -- clipped to
    the frame [0, w_in] x [0, h_in] (its area rounded to whole pixels).  From
    shapes and matrices alone, on the host, in float64; a singular or
    non-finite map reads nothing.  Source pixels that two ROIs share are
    counted for both: each ROI is its own launch-independent piece of work."""
    n = np.asarray(ms, dtype=np.float64).reshape(-1, 6).shape[0]
    total = n * w_out * h_out * c * out_esize
    for px in _roi_source_pixels(w_in, h_in, w_out, h_out, ms, inverse_map):
        total += px * c * in_esize
    return int(total)


def warp_affine_rois_standardize_bytes(w_in: int, h_in: int, c: int, w_out: int, h_out: int, ms,
                                       stats: bool = False, inverse_map: bool = False) -> int:
    """B_alg of vacv_warp_affine_rois_standardize: warp_rois_bytes of u8 frames
    and an fp32 output -- the u8 ROI and its statistics live in LDS and cost no
    memory traffic -- plus, with stats, the two (n, c) fp32 arrays."""
    n = np.asarray(ms, dtype=np.float64).reshape(-1, 6).shape[0]
    return warp_rois_bytes(w_in, h_in, c, w_out, h_out, ms, 1, 4, inverse_map) + (2 * n * c * 4 if stats else 0)


def crop_resize_rois_bytes(c: int, in_esize: int, w_out: int, h_out: int, rects, out_esize: int = 1,
                           w_in: int = None, h_in: int = None) -> int:
    """B_alg of vacv_crop_resize_rois[_normalize]: the output bytes of every
    ROI plus each valid rect's w * h * c * in_esize source bytes (a bilinear
    resize reads every pixel of its crop once, up-scale or down-scale by less
    than 2; larger down-scales skip rows and columns, which this does not
    discount).  rects: (n, 4) of (left, top, width, height).  An invalid rect,
    as the kernel judges it (width or height below 2, a negative origin, or --
    where the frame size w_in x h_in is given -- an edge past the frame), reads
    nothing and counts its output only."""
    r = np.asarray(rects, dtype=np.int64).reshape(-1, 4)
    total = r.shape[0] * w_out * h_out * c * out_esize
    for left, top, w, h in r.tolist():
        if w < 2 or h < 2 or left < 0 or top < 0:
            continue
        if (w_in is not None and left + w > w_in) or (h_in is not None and top + h > h_in):
            continue
        total += w * h * c * in_esize
    return int(total)


def crop_resize_rois_standardize_bytes(c: int, w_out: int, h_out: int, rects, stats: bool = False,
                                       w_in: int = None, h_in: int = None) -> int:
    """B_alg of vacv_crop_resize_rois_standardize: crop_resize_rois_bytes of u8
    frames and an fp32 output -- the u8 ROI and its statistics live in LDS and
    cost no memory traffic -- plus, with stats, the two (n, c) fp32 arrays."""
    n = np.asarray(rects, dtype=np.int64).reshape(-1, 4).shape[0]
    return crop_resize_rois_bytes(c, 1, w_out, h_out, rects, 4, w_in, h_in) + (2 * n * c * 4 if stats else 0)


def match_template_rois_bytes(c: int, w: int, h: int, tw: int, th: int, origins, n_templ: int = 1,
                              peaks: bool = True, w_in: int = None, h_in: int = None) -> int:
    """B_alg of vacv_match_template_rois: per ROI the (w - tw + 1) x (h - th + 1)
    fp32 map written and, with peaks, its 2 doubles and 4 int32; each valid
    w x h search window's w * h * c source bytes, read once; and each of the
    n_templ (1 = shared, or one per ROI) templates' tw * th * c bytes, read
    once per ROI that uses it.  origins: (n, 2) of (left, top).  A window with
    a negative origin or -- where the frame size w_in x h_in is given -- an
    edge past the frame reads neither source nor template and counts its
    outputs only."""
    o = np.asarray(origins, dtype=np.int64).reshape(-1, 2)
    if n_templ not in (1, o.shape[0]):
        raise ValueError("n_templ is 1 or the number of ROIs")
    per_roi = (w - tw + 1) * (h - th + 1) * 4 + (2 * 8 + 4 * 4 if peaks else 0)
    total = o.shape[0] * per_roi
    for left, top in o.tolist():
        if left < 0 or top < 0:
            continue
        if (w_in is not None and left + w > w_in) or (h_in is not None and top + h > h_in):
            continue
        total += (w * h + tw * th) * c
    return int(total)


def cvt_color_match_template_rois_bytes(w: int, h: int, tw: int, th: int, origins, n_templ: int = 1,
                                        peaks: bool = True, w_in: int = None, h_in: int = None) -> int:
    """B_alg of vacv_cvt_color_match_template_rois: the maps, the peaks and the
    3-channel templates as match_template_rois_bytes counts them, and per
    valid w x h search window (judged in the decoded w_in x h_in frame) its
    w * h Y bytes and the chroma pairs that cover it -- columns left >> 1 to
    (left + w - 1) >> 1 of chroma rows top >> 1 to (top + h - 1) >> 1, 2 bytes
    each.  An invalid window reads nothing and counts its outputs only."""
    o = np.asarray(origins, dtype=np.int64).reshape(-1, 2)
    if n_templ not in (1, o.shape[0]):
        raise ValueError("n_templ is 1 or the number of ROIs")
    per_roi = (w - tw + 1) * (h - th + 1) * 4 + (2 * 8 + 4 * 4 if peaks else 0)
    total = o.shape[0] * per_roi
    for left, top in o.tolist():
        if left < 0 or top < 0:
            continue
        if (w_in is not None and left + w > w_in) or (h_in is not None and top + h > h_in):
            continue
        total += w * h + tw * th * 3
        total += 2 * (((left + w - 1) >> 1) - (left >> 1) + 1) * (((top + h - 1) >> 1) - (top >> 1) + 1)
    return int(total)


def yuv_crop_resize_rois_bytes(w_out: int, h_out: int, rects, out_esize: int = 1, w_in: int = None,
                               h_in: int = None) -> int:
    """B_alg of vacv_cvt_color_crop_resize_rois[_normalize]: the 3-channel
    output bytes of every ROI plus, per valid rect (judged as
    crop_resize_rois_bytes judges it, in the decoded w_in x h_in frame), its
    w * h Y bytes and the chroma pairs that cover it -- columns left >> 1 to
    (left + w - 1) >> 1 of chroma rows top >> 1 to (top + h - 1) >> 1, 2 bytes
    each.  An invalid rect reads nothing and counts its output only."""
    r = np.asarray(rects, dtype=np.int64).reshape(-1, 4)
    total = r.shape[0] * w_out * h_out * 3 * out_esize
    for left, top, w, h in r.tolist():
        if w < 2 or h < 2 or left < 0 or top < 0:
            continue
        if (w_in is not None and left + w > w_in) or (h_in is not None and top + h > h_in):
            continue
        total += w * h
        total += 2 * (((left + w - 1) >> 1) - (left >> 1) + 1) * (((top + h - 1) >> 1) - (top >> 1) + 1)
    return int(total)


def yuv_crop_resize_rois_standardize_bytes(w_out: int, h_out: int, rects, stats: bool = False, w_in: int = None,
                                           h_in: int = None) -> int:
    """B_alg of vacv_cvt_color_crop_resize_rois_standardize:
    yuv_crop_resize_rois_bytes with an fp32 output -- the u8 ROI and its
    statistics live in LDS and cost no memory traffic -- plus, with stats, the
    two (n, 3) fp32 arrays."""
    n = np.asarray(rects, dtype=np.int64).reshape(-1, 4).shape[0]
    return yuv_crop_resize_rois_bytes(w_out, h_out, rects, 4, w_in, h_in) + (2 * n * 3 * 4 if stats else 0)
