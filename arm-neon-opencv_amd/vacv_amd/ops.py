"""Batched vacv operators on device tensors, through the C ABI.

The names and argument meanings follow the reference's ``va_cv::`` API
(/root/reference/src/cv/cv.h:85-209); every call goes straight to a HIP
kernel in lib/libvacv_hip.so.  PyTorch is only the allocator and the stream
provider here: tensors must live on a HIP device, and nothing is computed on
the CPU.

Image tensors
  NHWC: (n, h, w, c), (h, w, c) or (h, w)          -- the reference's default
  NCHW: (n, c, h, w) or (c, h, w)                   -- pass layout=NCHW
Rows may be pitched (e.g. a slice of a larger image) as long as each row's
pixels are contiguous; the descriptor carries the byte pitches.
"""
from __future__ import annotations

import ctypes
from typing import Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib as L
from ._lib import (BORDER_CONSTANT, FP16, FP32, FP64, INT8, INTER_CUBIC, INTER_LINEAR, LINEAR_REFERENCE, NCHW,
                   NHWC, VacvImage, check)

_DTYPES = {torch.uint8: INT8, torch.float32: FP32, torch.float16: FP16, torch.float64: FP64}
_TORCH = {v: k for k, v in _DTYPES.items()}


def _stream(stream=None) -> int:
    if stream is None:
        stream = torch.cuda.current_stream()
    return int(stream.cuda_stream) if hasattr(stream, "cuda_stream") else int(stream)


def _as4d(t: torch.Tensor, layout: int) -> torch.Tensor:
    if t.dim() == 4:
        return t
    if t.dim() == 3:
        return t.unsqueeze(0)
    if t.dim() == 2:
        return t.unsqueeze(0).unsqueeze(-1 if layout == NHWC else 1)
    raise ValueError(f"expected a 2-4 dimensional image tensor, got shape {tuple(t.shape)}")


def describe(t: torch.Tensor, layout: int = NHWC) -> VacvImage:
    """vacv_image descriptor of a device tensor (no copy)."""
    if not t.is_cuda:
        raise ValueError("vacv operators take device tensors (the C++ API stages host images)")
    if t.dtype not in _DTYPES:
        raise TypeError(f"unsupported dtype {t.dtype}")
    t4 = _as4d(t, layout)
    es = t4.element_size()
    st = t4.stride()
    # strides of size-1 dimensions are meaningless (numpy/torch may report 0):
    # pass 0 there and let the C side use the dense pitch
    if layout == NHWC:
        n, h, w, c = t4.shape
        if (c > 1 and st[3] != 1) or (w > 1 and st[2] != c):
            raise ValueError("NHWC rows must be contiguous (pixel stride == c)")
        row, plane, batch = (st[1] * es if h > 1 else 0), 0, (st[0] * es if n > 1 else 0)
    else:
        n, c, h, w = t4.shape
        if w > 1 and st[3] != 1:
            raise ValueError("NCHW rows must be contiguous")
        row, plane, batch = (st[2] * es if h > 1 else 0), (st[1] * es if c > 1 else 0), (st[0] * es if n > 1 else 0)
    return VacvImage(t4.data_ptr(), n, w, h, c, _DTYPES[t.dtype], layout, row, plane, batch)


def _empty_like_shape(src4: torch.Tensor, layout: int, w: int, h: int, dtype, squeeze: bool, src_dim: int,
                      c: Optional[int] = None):
    n = src4.shape[0]
    c = c if c is not None else (src4.shape[3] if layout == NHWC else src4.shape[1])
    shape = (n, h, w, c) if layout == NHWC else (n, c, h, w)
    out = torch.empty(shape, dtype=dtype, device=src4.device)
    return out


def _shape_back(out4: torch.Tensor, src: torch.Tensor, layout: int) -> torch.Tensor:
    if src.dim() == 4:
        return out4
    if src.dim() == 3:
        return out4[0]
    return out4[0, ..., 0] if layout == NHWC else out4[0, 0]


def _fptr(a) -> Tuple[object, ctypes.POINTER(ctypes.c_float)]:
    arr = np.ascontiguousarray(np.asarray(a, dtype=np.float32).reshape(-1))
    return arr, arr.ctypes.data_as(ctypes.POINTER(ctypes.c_float))


def _dptr(a) -> Tuple[object, ctypes.POINTER(ctypes.c_double)]:
    arr = np.ascontiguousarray(np.asarray(a, dtype=np.float64).reshape(-1))
    return arr, arr.ctypes.data_as(ctypes.POINTER(ctypes.c_double))


def _meanstd(mean, std, c):
    if mean is None and std is None:
        return (None, None), (None, None)
    if mean is None or std is None:
        raise ValueError("give both mean and stddev, or neither (per-image statistics)")
    m, s = _fptr(mean), _fptr(std)
    if m[0].size != c or s[0].size != c:
        raise ValueError(f"mean/stddev need {c} values")
    return m, s


# ---------------------------------------------------------------------------
# geometry / dtype

def crop(src: torch.Tensor, rect: Sequence[float], layout: int = NHWC, out=None, stream=None) -> torch.Tensor:
    """va_cv::crop (cv.h:209): rect = (left, top, right, bottom), truncated
    to int exactly as crop_naive does (crop.cpp:128-131)."""
    left, top = int(rect[0]), int(rect[1])
    cw, ch = int(np.float32(rect[2]) - np.float32(rect[0])), int(np.float32(rect[3]) - np.float32(rect[1]))
    s4 = _as4d(src, layout)
    if out is None:
        out = _empty_like_shape(s4, layout, cw, ch, src.dtype, True, src.dim())
    o4 = _as4d(out, layout)
    check("vacv_crop", L.load().vacv_crop(ctypes.byref(describe(s4, layout)), ctypes.byref(describe(o4, layout)),
                                          left, top, _stream(stream)))
    return _shape_back(o4, src, layout)


def change_layout(src: torch.Tensor, to_layout: int, layout: int = NHWC, out=None, stream=None) -> torch.Tensor:
    """Tensor::change_layout (tensor.cpp:393-457).  Across layouts both images
    must be dense; `out` (optional) is a preallocated 4-D output."""
    s4 = _as4d(src, layout)
    if layout == NHWC:
        n, h, w, c = s4.shape
    else:
        n, c, h, w = s4.shape
    if out is None:
        out = torch.empty((n, h, w, c) if to_layout == NHWC else (n, c, h, w), dtype=src.dtype, device=src.device)
    check("vacv_change_layout", L.load().vacv_change_layout(ctypes.byref(describe(s4, layout)),
                                                            ctypes.byref(describe(out, to_layout)), _stream(stream)))
    return out


def change_dtype(src: torch.Tensor, dtype: torch.dtype, layout: int = NHWC, out=None, stream=None) -> torch.Tensor:
    """Tensor::change_dtype (tensor.cpp:459-502): u8<->fp32 between dense
    images; equal dtypes copy (pitches allowed).  `out` (optional) is a
    preallocated output of the source's shape and dtype `dtype`."""
    s4 = _as4d(src, layout)
    if out is None:
        out = torch.empty(s4.shape, dtype=dtype, device=src.device)
    o4 = _as4d(out, layout)
    check("vacv_change_dtype", L.load().vacv_change_dtype(ctypes.byref(describe(s4, layout)),
                                                          ctypes.byref(describe(o4, layout)), _stream(stream)))
    return _shape_back(o4, src, layout)


def resize(src: torch.Tensor, w: int, h: int, interpolation: int = INTER_LINEAR, mode: int = LINEAR_REFERENCE,
           layout: int = NHWC, out=None, stream=None, fx: float = 0.0, fy: float = 0.0) -> torch.Tensor:
    """va_cv::resize (cv.h:85-87).  INTER_CUBIC on u8 input returns fp32.
    w = h = 0 with fx, fy > 0 (INTER_NEAREST / INTER_AREA / INTER_LANCZOS4): cv::resize's
    dsize = (round(w_in * fx), round(h_in * fy)) and inv_scale = (fx, fy)."""
    s4 = _as4d(src, layout)
    dt = torch.float32 if (interpolation == INTER_CUBIC) else src.dtype
    scaled = w == 0 and h == 0 and fx > 0 and fy > 0
    if scaled:  # saturate_cast<int>(double): round half to even, as Python's round
        w_in, h_in = (s4.shape[2], s4.shape[1]) if layout == NHWC else (s4.shape[3], s4.shape[2])
        w, h = int(round(w_in * fx)), int(round(h_in * fy))
    if out is None:
        out = _empty_like_shape(s4, layout, w, h, dt, True, src.dim())
    if scaled:
        check("vacv_resize_scaled", L.load().vacv_resize_scaled(
            ctypes.byref(describe(s4, layout)), ctypes.byref(describe(out, layout)), interpolation, mode,
            float(fx), float(fy), _stream(stream)))
    else:
        check("vacv_resize", L.load().vacv_resize(ctypes.byref(describe(s4, layout)),
                                                  ctypes.byref(describe(out, layout)), interpolation, mode,
                                                  _stream(stream)))
    return _shape_back(out, src, layout)


def resize_normalize(src: torch.Tensor, w: int, h: int, mean=None, std=None, interpolation: int = INTER_LINEAR,
                     mode: int = LINEAR_REFERENCE, layout: int = NHWC, out=None, stream=None) -> torch.Tensor:
    """va_cv::resize_normalize (cv.h:154-158): resize, fp32, normalize."""
    s4 = _as4d(src, layout)
    c = s4.shape[3] if layout == NHWC else s4.shape[1]
    if out is None:
        out = _empty_like_shape(s4, layout, w, h, torch.float32, True, src.dim())
    (ma, mp), (sa, sp) = _meanstd(mean, std, c)
    check("vacv_resize_normalize",
          L.load().vacv_resize_normalize(ctypes.byref(describe(s4, layout)), ctypes.byref(describe(out, layout)),
                                         interpolation, mode, mp, sp, _stream(stream)))
    return _shape_back(out, src, layout)


def rotation_matrix(scale: float, rot: float, aux: Sequence[float] = (0, 0, 0, 0)) -> np.ndarray:
    """get_rotation_matrix_2D + aux fix (warp_affine.cpp:76-109), host."""
    m = np.zeros(6, np.float32)
    a, ap = _dptr(aux)
    check("vacv_rotation_matrix", L.load().vacv_rotation_matrix(scale, rot, ap,
                                                                m.ctypes.data_as(ctypes.POINTER(ctypes.c_float))))
    return m


def invert_affine(m) -> np.ndarray:
    mm, mp = _fptr(m)
    inv = np.zeros(6, np.float32)
    check("vacv_invert_affine", L.load().vacv_invert_affine(mp, inv.ctypes.data_as(ctypes.POINTER(ctypes.c_float))))
    return inv


def warp_affine(src: torch.Tensor, m, w: int, h: int, flags: int = INTER_LINEAR, border_mode: int = BORDER_CONSTANT,
                border_value=(0, 0, 0, 0), layout: int = NHWC, out=None, stream=None) -> torch.Tensor:
    """va_cv::warp_affine (cv.h:118-122); m is the forward 2x3 map, or the
    inverse one with flags | WARP_INVERSE_MAP; flags INTER_LINEAR (the
    reference's naive sampler) or INTER_NEAREST (OpenCV 2.4's)."""
    s4 = _as4d(src, layout)
    if out is None:
        out = _empty_like_shape(s4, layout, w, h, src.dtype, True, src.dim())
    mm, mp = _fptr(m)
    bv, bp = _dptr(border_value)
    check("vacv_warp_affine", L.load().vacv_warp_affine(ctypes.byref(describe(s4, layout)),
                                                        ctypes.byref(describe(out, layout)), mp, flags, border_mode,
                                                        bp, _stream(stream)))
    return _shape_back(out, src, layout)


def warp_affine_rot(src: torch.Tensor, scale: float, rot: float, w: int, h: int, aux=(0, 0, 0, 0), **kw):
    """va_cv::warp_affine(src, dst, scale, rot, dsize, aux, ...) (cv.h:136-141)."""
    return warp_affine(src, rotation_matrix(scale, rot, aux), w, h, **kw)


def warp_affine_normalize(src: torch.Tensor, m, w: int, h: int, mean=None, std=None, flags: int = INTER_LINEAR,
                          border_mode: int = BORDER_CONSTANT, border_value=(0, 0, 0, 0), layout: int = NHWC,
                          out=None, stream=None) -> torch.Tensor:
    """va_cv::warp_affine_normalize (cv.h:172-201)."""
    s4 = _as4d(src, layout)
    c = s4.shape[3] if layout == NHWC else s4.shape[1]
    if out is None:
        out = _empty_like_shape(s4, layout, w, h, torch.float32, True, src.dim())
    mm, mp = _fptr(m)
    bv, bp = _dptr(border_value)
    (ma, meanp), (sa, stdp) = _meanstd(mean, std, c)
    check("vacv_warp_affine_normalize",
          L.load().vacv_warp_affine_normalize(ctypes.byref(describe(s4, layout)), ctypes.byref(describe(out, layout)),
                                              mp, flags, border_mode, bp, meanp, stdp, _stream(stream)))
    return _shape_back(out, src, layout)


def _device_array(a, dtype: torch.dtype, device, what: str) -> torch.Tensor:
    """A device tensor as it is (dense, of `dtype`, on `device`: anything else
    raises, nothing is copied silently); numpy arrays and lists are moved to
    the device for convenience."""
    if not isinstance(a, torch.Tensor):
        return torch.as_tensor(np.asarray(a), dtype=dtype).contiguous().to(device)
    if a.device != device:
        raise ValueError(f"{what} must live on {device}, not {a.device}")
    if a.dtype != dtype:
        raise ValueError(f"{what} must be {dtype}, not {a.dtype}")
    if not a.is_contiguous():
        raise ValueError(f"{what} must be contiguous")
    return a


def _roi_batch(src4, arr, what, dtype, shape_ok, shape_msg, empty_msg, src_index):
    """A batched-ROI call's per-ROI array (one row per ROI) and src_index, checked against the frames src4."""
    arr = _device_array(arr, dtype, src4.device, what)
    if not shape_ok(arr):
        raise ValueError(f"{what} must have shape {shape_msg}, got {tuple(arr.shape)}")
    n = arr.shape[0]
    if n < 1:
        raise ValueError(empty_msg)
    if src_index is not None:
        src_index = _device_array(src_index, torch.int32, src4.device, "src_index")
        if tuple(src_index.shape) != (n,):
            raise ValueError(f"src_index must have shape ({n},), got {tuple(src_index.shape)}")
    elif src4.shape[0] not in (1, n):
        raise ValueError(f"without src_index, src must hold 1 or {n} images, not {src4.shape[0]}")
    return src4, arr, src_index, n


# _roi_batch's (what, dtype, shape_ok, shape_msg, empty_msg) of the two kinds of per-ROI array
_MS = ("ms", torch.float32,
       lambda a: (a.dim() == 2 and a.shape[1] == 6) or (a.dim() == 3 and tuple(a.shape[1:]) == (2, 3)),
       "(n, 6) or (n, 2, 3)", "ms holds no matrix")
_RECTS = ("rects", torch.int32, lambda a: a.dim() == 2 and a.shape[1] == 4, "(n, 4)", "rects holds no rect")


def _idx_ptr(src_index):
    return src_index.data_ptr() if src_index is not None else None


def _border(border_value):
    return _dptr((list(border_value) + [0, 0, 0, 0])[:4])  # the C side reads four


def warp_affine_rois(src: torch.Tensor, ms, w: int, h: int, src_index=None, flags: int = INTER_LINEAR,
                     border_mode: int = BORDER_CONSTANT, border_value=(0, 0, 0, 0), out=None,
                     stream=None) -> torch.Tensor:
    """Many crops in one launch: out[i] = warp_affine(src[src_index[i]], ms[i], w, h).
    src: NHWC frames (n, h, w, c) or one (h, w, c) / (h, w) frame.  ms: (n, 6)
    or (n, 2, 3) float32 device tensor; src_index: (n,) int32 device tensor, or
    None (one frame for all, or frame i for ROI i).  Both are read by the
    kernel when it runs on `stream`, not by this call.  Returns (n, h, w, c)."""
    s4, ms, src_index, n = _roi_batch(_as4d(src, NHWC), ms, *_MS, src_index)
    if out is None:
        out = torch.empty((n, h, w, s4.shape[3]), dtype=src.dtype, device=src.device)
    bv, bp = _border(border_value)
    check("vacv_warp_affine_rois", L.load().vacv_warp_affine_rois(
        ctypes.byref(describe(s4, NHWC)), ctypes.byref(describe(out, NHWC)), ms.data_ptr(),
        _idx_ptr(src_index), flags, border_mode, bp, _stream(stream)))
    return out


def warp_affine_rois_normalize(src: torch.Tensor, ms, w: int, h: int, mean, std, src_index=None,
                               out_layout: int = NHWC, flags: int = INTER_LINEAR,
                               border_mode: int = BORDER_CONSTANT, border_value=(0, 0, 0, 0), out=None,
                               stream=None) -> torch.Tensor:
    """warp_affine_rois with the fused normalize: fp32 (n, h, w, c), or planar
    (n, c, h, w) with out_layout=NCHW (c = 3 or 1), the model-input layout."""
    s4, ms, src_index, n = _roi_batch(_as4d(src, NHWC), ms, *_MS, src_index)
    c = s4.shape[3]
    if mean is None or std is None:
        raise ValueError("warp_affine_rois_normalize needs mean and stddev (no per-image statistics for ROIs)")
    if out is None:
        out = torch.empty((n, h, w, c) if out_layout == NHWC else (n, c, h, w), dtype=torch.float32,
                          device=src.device)
    bv, bp = _border(border_value)
    (ma, meanp), (sa, stdp) = _meanstd(mean, std, c)
    check("vacv_warp_affine_rois_normalize", L.load().vacv_warp_affine_rois_normalize(
        ctypes.byref(describe(s4, NHWC)), ctypes.byref(describe(out, out_layout)), ms.data_ptr(),
        _idx_ptr(src_index), flags, border_mode, bp, meanp, stdp, _stream(stream)))
    return out


def warp_affine_rois_standardize(src: torch.Tensor, ms, w: int, h: int, src_index=None, flags: int = INTER_LINEAR,
                                 border_mode: int = BORDER_CONSTANT, border_value=(0, 0, 0, 0), layout: int = NHWC,
                                 out=None, stats: bool = False, stream=None):
    """warp_affine_rois with each crop standardized by its OWN per-channel mean
    and standard deviation (the reference's warp_affine_normalize with mean and
    stddev left empty), in one launch: fp32 (n, h, w, c), or planar
    (n, c, h, w) with layout=NCHW (c = 3 or 1).  src: uint8 frames.  Bit for
    bit warp_affine_rois -> mean_stddev -> normalize(None, None) ->
    change_layout: border pixels count in the statistics, and an index outside
    the frames gives zeros with mean = border_value and stddev 0.
    stats=True: returns (out, mean, std), the two (n, c) float32 device tensors
    of every crop's statistics.  A crop must fit one workgroup's LDS (144 x 144
    x 3 does): VacvError(UNSUPPORTED) otherwise."""
    s4, ms, src_index, n = _roi_batch(_as4d(src, NHWC), ms, *_MS, src_index)
    c = s4.shape[3]
    if src.dtype != torch.uint8:
        raise ValueError(f"warp_affine_rois_standardize takes uint8 frames, not {src.dtype}")
    if out is None:
        out = torch.empty((n, h, w, c) if layout == NHWC else (n, c, h, w), dtype=torch.float32, device=src.device)
    mean = std = None
    if stats:
        mean = torch.empty((n, c), dtype=torch.float32, device=src.device)
        std = torch.empty((n, c), dtype=torch.float32, device=src.device)
    bv, bp = _border(border_value)
    check("vacv_warp_affine_rois_standardize", L.load().vacv_warp_affine_rois_standardize(
        ctypes.byref(describe(s4, NHWC)), ctypes.byref(describe(out, layout)), ms.data_ptr(),
        _idx_ptr(src_index), flags, border_mode, bp, mean.data_ptr() if stats else None,
        std.data_ptr() if stats else None, _stream(stream)))
    return (out, mean, std) if stats else out


def invert_affine_device(ms: torch.Tensor, out=None, stream=None) -> torch.Tensor:
    """vacv_invert_affine of every map of a float32 device tensor (n, 6) or
    (n, 2, 3), on the device (bit-identical to the host function)."""
    if not isinstance(ms, torch.Tensor) or not ms.is_cuda:
        raise ValueError("invert_affine_device takes a device tensor (invert_affine is the host function)")
    ms = _device_array(ms, torch.float32, ms.device, "ms")
    if ms.numel() % 6:
        raise ValueError(f"ms must hold 2x3 maps, got shape {tuple(ms.shape)}")
    if out is None:
        out = torch.empty_like(ms)
    else:
        out = _device_array(out, torch.float32, ms.device, "out")
        if out.shape != ms.shape:
            raise ValueError("out must have the shape of ms")
    check("vacv_invert_affine_device", L.load().vacv_invert_affine_device(ms.data_ptr(), out.data_ptr(),
                                                                          ms.numel() // 6, _stream(stream)))
    return out


_HS = ("hs", torch.float32,
       lambda a: (a.dim() == 2 and a.shape[1] == 9) or (a.dim() == 3 and tuple(a.shape[1:]) == (3, 3)),
       "(n, 9) or (n, 3, 3)", "hs holds no matrix")


def warp_perspective_rois(src: torch.Tensor, hs, w: int, h: int, src_index=None, flags: int = INTER_LINEAR,
                          border_mode: int = BORDER_CONSTANT, border_value=(0, 0, 0, 0), out=None,
                          stream=None) -> torch.Tensor:
    """Many projective crops in one launch: out[i] = warp_perspective(src[src_index[i]], hs[i], w, h).
    src and src_index as warp_affine_rois takes them.  hs: (n, 9) or (n, 3, 3)
    float32 device tensor of homographies, forward maps, or dst -> src maps with
    flags | WARP_INVERSE_MAP (homographies_from_quads makes those).  Read by the
    kernel when it runs on `stream`, not by this call.  Returns (n, h, w, c)."""
    s4, hs, src_index, n = _roi_batch(_as4d(src, NHWC), hs, *_HS, src_index)
    if out is None:
        out = torch.empty((n, h, w, s4.shape[3]), dtype=src.dtype, device=src.device)
    bv, bp = _border(border_value)
    check("vacv_warp_perspective_rois", L.load().vacv_warp_perspective_rois(
        ctypes.byref(describe(s4, NHWC)), ctypes.byref(describe(out, NHWC)), hs.data_ptr(),
        _idx_ptr(src_index), flags, border_mode, bp, _stream(stream)))
    return out


def warp_perspective_rois_normalize(src: torch.Tensor, hs, w: int, h: int, mean, std, src_index=None,
                                    out_layout: int = NHWC, flags: int = INTER_LINEAR,
                                    border_mode: int = BORDER_CONSTANT, border_value=(0, 0, 0, 0), out=None,
                                    stream=None) -> torch.Tensor:
    """warp_perspective_rois with the fused normalize: fp32 (n, h, w, c), or
    planar (n, c, h, w) with out_layout=NCHW (c = 3 or 1), the model-input layout."""
    s4, hs, src_index, n = _roi_batch(_as4d(src, NHWC), hs, *_HS, src_index)
    c = s4.shape[3]
    if mean is None or std is None:
        raise ValueError("warp_perspective_rois_normalize needs mean and stddev (no per-image statistics for ROIs)")
    if out is None:
        out = torch.empty((n, h, w, c) if out_layout == NHWC else (n, c, h, w), dtype=torch.float32,
                          device=src.device)
    bv, bp = _border(border_value)
    (ma, meanp), (sa, stdp) = _meanstd(mean, std, c)
    check("vacv_warp_perspective_rois_normalize", L.load().vacv_warp_perspective_rois_normalize(
        ctypes.byref(describe(s4, NHWC)), ctypes.byref(describe(out, out_layout)), hs.data_ptr(),
        _idx_ptr(src_index), flags, border_mode, bp, meanp, stdp, _stream(stream)))
    return out


def invert_homography(h) -> np.ndarray:
    """The float64 inverse (up to scale) of a float32 3x3 homography: what the
    ROI kernel samples through for a forward map.  Host; returns (9,) float64."""
    hh, hp = _fptr(np.asarray(h, np.float32).reshape(9))
    inv = np.zeros(9, np.float64)
    check("vacv_invert_homography",
          L.load().vacv_invert_homography(hp, inv.ctypes.data_as(ctypes.POINTER(ctypes.c_double))))
    return inv


def perspective_transform(src_quad, dst_quad) -> np.ndarray:
    """cv::getPerspectiveTransform: the (9,) float32 homography (h8 = 1) that
    maps the four points src_quad (4, 2) to dst_quad.  Host; a degenerate quad
    raises VacvError(INVALID_ARG)."""
    sq, sp = _fptr(np.asarray(src_quad, np.float32).reshape(8))
    dq, dp = _fptr(np.asarray(dst_quad, np.float32).reshape(8))
    out = np.zeros(9, np.float32)
    check("vacv_perspective_transform",
          L.load().vacv_perspective_transform(sp, dp, out.ctypes.data_as(ctypes.POINTER(ctypes.c_float))))
    return out


def homographies_from_quads(quads: torch.Tensor, w: int, h: int) -> torch.Tensor:
    """(n, 4, 2) quads (TL, TR, BR, BL, in frame pixels) -> (n, 9) float32
    dst -> src maps for warp_perspective_rois(..., flags | WARP_INVERSE_MAP):
    the output corners (0, 0), (w-1, 0), (w-1, h-1), (0, h-1) land on the
    quad's points.  The closed-form square-to-quad map, elementwise in float64
    on the quads' device: no solver, no host round trip."""
    if w < 2 or h < 2:
        raise ValueError(f"homographies_from_quads needs w, h >= 2, got {w} x {h}")
    if quads.dim() != 3 or tuple(quads.shape[1:]) != (4, 2):
        raise ValueError(f"quads must have shape (n, 4, 2), got {tuple(quads.shape)}")
    q = quads.to(torch.float64)
    x0, y0, x1, y1 = q[:, 0, 0], q[:, 0, 1], q[:, 1, 0], q[:, 1, 1]
    x2, y2, x3, y3 = q[:, 2, 0], q[:, 2, 1], q[:, 3, 0], q[:, 3, 1]
    dx1, dy1, dx2, dy2 = x1 - x2, y1 - y2, x3 - x2, y3 - y2
    sx, sy = x0 - x1 + x2 - x3, y0 - y1 + y2 - y3
    den = dx1 * dy2 - dx2 * dy1
    g = (sx * dy2 - dx2 * sy) / den
    k = (dx1 * sy - sx * dy1) / den
    # the unit square's map (u, v, 1) -> (a u + b v + x0, d u + e v + y0, g u + k v + 1), u = x / (w-1), v = y / (h-1)
    su, sv = 1.0 / (w - 1), 1.0 / (h - 1)
    rows = [(x1 - x0 + g * x1) * su, (x3 - x0 + k * x3) * sv, x0,
            (y1 - y0 + g * y1) * su, (y3 - y0 + k * y3) * sv, y0,
            g * su, k * sv, torch.ones_like(g)]
    return torch.stack(rows, dim=1).to(torch.float32).contiguous()


def rects_from_boxes(boxes: torch.Tensor) -> torch.Tensor:
    """(n, 4) float32 boxes (left, top, right, bottom) -> (n, 4) int32 rects
    (left, top, width, height) as crop_naive truncates them (crop.cpp:128-131):
    int(left), int(top), int(right - left), int(bottom - top), the differences
    in float32, every conversion toward zero.  Computed where `boxes` lives, so
    a detector's device output never visits the host."""
    if not isinstance(boxes, torch.Tensor) or boxes.dtype != torch.float32:
        raise ValueError("boxes must be a float32 tensor")
    if boxes.dim() != 2 or boxes.shape[1] != 4:
        raise ValueError(f"boxes must have shape (n, 4), got {tuple(boxes.shape)}")
    lt = boxes[:, :2]
    return torch.cat([lt, boxes[:, 2:] - lt], 1).to(torch.int32).contiguous()


def crop_resize_rois(src: torch.Tensor, rects, w: int, h: int, src_index=None, mode: int = LINEAR_REFERENCE,
                     out=None, stream=None) -> torch.Tensor:
    """Many upright crops in one launch: out[i] = resize(crop(src[src_index[i]],
    rects[i]), w, h), the reference's crop + resize chain byte for byte (taps
    clamped at the rect's edges).  src: NHWC frames (n, h, w, c) or one
    (h, w, c) / (h, w) frame.  rects: (n, 4) int32 device tensor of (left, top,
    width, height) (rects_from_boxes makes them from float boxes); src_index:
    (n,) int32 device tensor, or None (one frame for all, or frame i for ROI i).
    Both are read by the kernel when it runs on `stream`, not by this call; an
    invalid rect or index gives a ROI of zeros.  Returns (n, h, w, c)."""
    s4, rects, src_index, n = _roi_batch(_as4d(src, NHWC), rects, *_RECTS, src_index)
    if out is None:
        out = torch.empty((n, h, w, s4.shape[3]), dtype=src.dtype, device=src.device)
    check("vacv_crop_resize_rois", L.load().vacv_crop_resize_rois(
        ctypes.byref(describe(s4, NHWC)), ctypes.byref(describe(out, NHWC)), rects.data_ptr(),
        _idx_ptr(src_index), INTER_LINEAR, mode, _stream(stream)))
    return out


def crop_resize_rois_normalize(src: torch.Tensor, rects, w: int, h: int, mean, std, src_index=None,
                               mode: int = LINEAR_REFERENCE, layout: int = NHWC, out=None,
                               stream=None) -> torch.Tensor:
    """crop_resize_rois with the fused normalize: fp32 (n, h, w, c), or planar
    (n, c, h, w) with layout=NCHW (c = 3 or 1), the model-input layout."""
    s4, rects, src_index, n = _roi_batch(_as4d(src, NHWC), rects, *_RECTS, src_index)
    c = s4.shape[3]
    if mean is None or std is None:
        raise ValueError("crop_resize_rois_normalize needs mean and stddev (no per-image statistics for ROIs)")
    if out is None:
        out = torch.empty((n, h, w, c) if layout == NHWC else (n, c, h, w), dtype=torch.float32, device=src.device)
    (ma, meanp), (sa, stdp) = _meanstd(mean, std, c)
    check("vacv_crop_resize_rois_normalize", L.load().vacv_crop_resize_rois_normalize(
        ctypes.byref(describe(s4, NHWC)), ctypes.byref(describe(out, layout)), rects.data_ptr(),
        _idx_ptr(src_index), INTER_LINEAR, mode, meanp, stdp, _stream(stream)))
    return out


def crop_resize_rois_standardize(src: torch.Tensor, rects, w: int, h: int, src_index=None,
                                 mode: int = LINEAR_REFERENCE, layout: int = NHWC, out=None, stats: bool = False,
                                 stream=None):
    """crop_resize_rois with each crop standardized by its OWN per-channel mean
    and standard deviation (the reference's resize_normalize of a crop with
    mean and stddev left empty), in one launch: fp32 (n, h, w, c), or planar
    (n, c, h, w) with layout=NCHW (c = 3 or 1).  src: uint8 frames.  Bit for
    bit crop_resize_rois -> mean_stddev -> normalize(None, None) ->
    change_layout; an invalid rect or index gives zeros with mean and stddev 0.
    stats=True: returns (out, mean, std), the two (n, c) float32 device tensors
    of every crop's statistics.  A crop must fit one workgroup's LDS (144 x 144
    x 3 does): VacvError(UNSUPPORTED) otherwise."""
    s4, rects, src_index, n = _roi_batch(_as4d(src, NHWC), rects, *_RECTS, src_index)
    c = s4.shape[3]
    if src.dtype != torch.uint8:
        raise ValueError(f"crop_resize_rois_standardize takes uint8 frames, not {src.dtype}")
    if out is None:
        out = torch.empty((n, h, w, c) if layout == NHWC else (n, c, h, w), dtype=torch.float32, device=src.device)
    mean = std = None
    if stats:
        mean = torch.empty((n, c), dtype=torch.float32, device=src.device)
        std = torch.empty((n, c), dtype=torch.float32, device=src.device)
    check("vacv_crop_resize_rois_standardize", L.load().vacv_crop_resize_rois_standardize(
        ctypes.byref(describe(s4, NHWC)), ctypes.byref(describe(out, layout)), rects.data_ptr(),
        _idx_ptr(src_index), INTER_LINEAR, mode, mean.data_ptr() if stats else None,
        std.data_ptr() if stats else None, _stream(stream)))
    return (out, mean, std) if stats else out


# ---------------------------------------------------------------------------
# colour

def _yuv4(yuv: torch.Tensor) -> torch.Tensor:
    return yuv if yuv.dim() == 3 else yuv.unsqueeze(0)


def _yuv_desc(yuv: torch.Tensor) -> VacvImage:
    return describe(_yuv4(yuv).unsqueeze(-1), NHWC)


_DCN4 = (L.COLOR_YUV2RGBA_NV12, L.COLOR_YUV2BGRA_NV12, L.COLOR_YUV2RGBA_NV21, L.COLOR_YUV2BGRA_NV21)


def cvt_color(yuv: torch.Tensor, code: int = L.COLOR_YUV2BGR_NV21, out=None, stream=None) -> torch.Tensor:
    """va_cv::cvt_color (cv.h:95): (n, h*3/2, w) u8 -> (n, h, w, 3) u8 (4
    channels for the RGBA/BGRA codes; YV12 is Y then the V and U planes).
    COLOR_GRAY2BGR: (n, h, w) u8/fp32 -> (n, h, w, 3) of the same dtype.
    `out` (optional): a preallocated output of that shape."""
    if code == L.COLOR_GRAY2BGR:
        g4 = _yuv4(yuv)
        if out is None:
            out = torch.empty(tuple(g4.shape) + (3,), dtype=g4.dtype, device=yuv.device)
        out = out if out.dim() == 4 else out.unsqueeze(0)
        check("vacv_cvt_color", L.load().vacv_cvt_color(ctypes.byref(describe(g4.unsqueeze(-1), NHWC)),
                                                        ctypes.byref(describe(out, NHWC)), code, _stream(stream)))
        return out if yuv.dim() == 3 else out[0]
    y4 = _yuv4(yuv)
    n, hh, w = y4.shape
    if out is None:
        out = torch.empty((n, hh // 3 * 2, w, 4 if code in _DCN4 else 3), dtype=torch.uint8, device=yuv.device)
    out = out if out.dim() == 4 else out.unsqueeze(0)
    check("vacv_cvt_color", L.load().vacv_cvt_color(ctypes.byref(_yuv_desc(y4)), ctypes.byref(describe(out, NHWC)),
                                                    code, _stream(stream)))
    return out if yuv.dim() == 3 else out[0]


def cvt_color_normalize(yuv: torch.Tensor, code: int = L.COLOR_YUV2BGR_NV21, mean=None, std=None, out=None,
                        stream=None) -> torch.Tensor:
    y4 = _yuv4(yuv)
    n, hh, w = y4.shape
    if out is None:
        out = torch.empty((n, hh // 3 * 2, w, 3), dtype=torch.float32, device=yuv.device)
    (ma, mp), (sa, sp) = _meanstd(mean, std, 3)
    check("vacv_cvt_color_normalize",
          L.load().vacv_cvt_color_normalize(ctypes.byref(_yuv_desc(y4)), ctypes.byref(describe(out, NHWC)), code, mp,
                                            sp, _stream(stream)))
    return out if yuv.dim() == 3 else out[0]


def cvt_color_resize(yuv: torch.Tensor, w: int, h: int, code: int = L.COLOR_YUV2BGR_NV21, layout: int = NHWC,
                     dtype: torch.dtype = torch.uint8, mode: int = LINEAR_REFERENCE, out=None,
                     stream=None) -> torch.Tensor:
    """cvt_color -> resize(INTER_LINEAR) [-> change_dtype(FP32)] [-> change_layout]
    (cvt_color.cpp:39-157, resize_naive.cpp:10-68) in one kernel:
    (n, h_in*3/2, w_in) u8 -> (n, h, w, 3) NHWC or (n, 3, h, w) NCHW."""
    y4 = _yuv4(yuv)
    n = y4.shape[0]
    if out is None:
        shape = (n, h, w, 3) if layout == NHWC else (n, 3, h, w)
        out = torch.empty(shape, dtype=dtype, device=yuv.device)
    check("vacv_cvt_color_resize",
          L.load().vacv_cvt_color_resize(ctypes.byref(_yuv_desc(y4)), ctypes.byref(describe(out, layout)), code,
                                         INTER_LINEAR, mode, _stream(stream)))
    return out if yuv.dim() == 3 else out[0]


def cvt_color_resize_normalize(yuv: torch.Tensor, w: int, h: int, mean=None, std=None,
                               code: int = L.COLOR_YUV2BGR_NV21, layout: int = NCHW, mode: int = LINEAR_REFERENCE,
                               out=None, stream=None) -> torch.Tensor:
    """The camera-frame -> model-input step: cvt_color, resize, convert to
    fp32, normalize((x - mean) / (std + 1e-6)), change_layout -- one kernel.
    Default layout NCHW (planar fp32).  mean/std None = per-image stats of
    the resized image (two passes)."""
    y4 = _yuv4(yuv)
    n = y4.shape[0]
    if out is None:
        shape = (n, h, w, 3) if layout == NHWC else (n, 3, h, w)
        out = torch.empty(shape, dtype=torch.float32, device=yuv.device)
    (ma, mp), (sa, sp) = _meanstd(mean, std, 3)
    check("vacv_cvt_color_resize_normalize",
          L.load().vacv_cvt_color_resize_normalize(ctypes.byref(_yuv_desc(y4)), ctypes.byref(describe(out, layout)),
                                                   code, INTER_LINEAR, mode, mp, sp, _stream(stream)))
    return out if yuv.dim() == 3 else out[0]


def cvt_color_warp_affine_rois(yuv: torch.Tensor, ms, w: int, h: int, code: int = L.COLOR_YUV2BGR_NV21,
                               src_index=None, flags: int = INTER_LINEAR, border_mode: int = BORDER_CONSTANT,
                               border_value=(0, 0, 0, 0), out=None, stream=None) -> torch.Tensor:
    """Many crops straight from NV21 / NV12 frames in one launch: out[i] =
    warp_affine(cvt_color(yuv[src_index[i]], code), ms[i], w, h), byte for byte,
    without the decoded frames.  yuv: (n, h_in*3/2, w_in) u8 frames or one
    (h_in*3/2, w_in) frame; ms / src_index as warp_affine_rois takes them
    (device tensors, read by the kernel when it runs on `stream`);
    border_value in the decoded channel order.  Returns (n, h, w, 3) u8."""
    y4 = _yuv4(yuv)
    _, ms, src_index, n = _roi_batch(_as4d(y4.unsqueeze(-1), NHWC), ms, *_MS, src_index)
    if out is None:
        out = torch.empty((n, h, w, 3), dtype=torch.uint8, device=yuv.device)
    bv, bp = _border(border_value)
    check("vacv_cvt_color_warp_affine_rois", L.load().vacv_cvt_color_warp_affine_rois(
        ctypes.byref(_yuv_desc(y4)), ctypes.byref(describe(out, NHWC)), code, ms.data_ptr(),
        _idx_ptr(src_index), flags, border_mode, bp, _stream(stream)))
    return out


def cvt_color_warp_affine_rois_normalize(yuv: torch.Tensor, ms, w: int, h: int, mean, std,
                                         code: int = L.COLOR_YUV2BGR_NV21, src_index=None, layout: int = NHWC,
                                         flags: int = INTER_LINEAR, border_mode: int = BORDER_CONSTANT,
                                         border_value=(0, 0, 0, 0), out=None, stream=None) -> torch.Tensor:
    """cvt_color_warp_affine_rois with the fused normalize: fp32 (n, h, w, 3),
    or planar (n, 3, h, w) with layout=NCHW, the model-input layout."""
    y4 = _yuv4(yuv)
    _, ms, src_index, n = _roi_batch(_as4d(y4.unsqueeze(-1), NHWC), ms, *_MS, src_index)
    if mean is None or std is None:
        raise ValueError("cvt_color_warp_affine_rois_normalize needs mean and stddev (no per-image statistics for ROIs)")
    if out is None:
        out = torch.empty((n, h, w, 3) if layout == NHWC else (n, 3, h, w), dtype=torch.float32, device=yuv.device)
    bv, bp = _border(border_value)
    (ma, meanp), (sa, stdp) = _meanstd(mean, std, 3)
    check("vacv_cvt_color_warp_affine_rois_normalize", L.load().vacv_cvt_color_warp_affine_rois_normalize(
        ctypes.byref(_yuv_desc(y4)), ctypes.byref(describe(out, layout)), code, ms.data_ptr(),
        _idx_ptr(src_index), flags, border_mode, bp, meanp, stdp, _stream(stream)))
    return out


def cvt_color_crop_resize_rois(yuv: torch.Tensor, rects, w: int, h: int, code: int = L.COLOR_YUV2BGR_NV21,
                               src_index=None, mode: int = LINEAR_REFERENCE, out=None,
                               stream=None) -> torch.Tensor:
    """Many upright crops straight from NV21 / NV12 frames in one launch:
    out[i] = resize(crop(cvt_color(yuv[src_index[i]], code), rects[i]), w, h),
    byte for byte, without the decoded frames or the crops.  yuv:
    (n, h_in*3/2, w_in) u8 frames or one (h_in*3/2, w_in) frame; rects: (n, 4)
    int32 device tensor of (left, top, width, height) in the decoded frame;
    src_index as crop_resize_rois takes it.  Both are read by the kernel when
    it runs on `stream`; an invalid rect or index gives a ROI of zeros.
    Returns (n, h, w, 3) u8."""
    y4 = _yuv4(yuv)
    _, rects, src_index, n = _roi_batch(_as4d(y4.unsqueeze(-1), NHWC), rects, *_RECTS, src_index)
    if out is None:
        out = torch.empty((n, h, w, 3), dtype=torch.uint8, device=yuv.device)
    check("vacv_cvt_color_crop_resize_rois", L.load().vacv_cvt_color_crop_resize_rois(
        ctypes.byref(_yuv_desc(y4)), ctypes.byref(describe(out, NHWC)), code, rects.data_ptr(),
        _idx_ptr(src_index), INTER_LINEAR, mode, _stream(stream)))
    return out


def cvt_color_crop_resize_rois_normalize(yuv: torch.Tensor, rects, w: int, h: int, mean, std,
                                         code: int = L.COLOR_YUV2BGR_NV21, src_index=None,
                                         mode: int = LINEAR_REFERENCE, layout: int = NHWC, out=None,
                                         stream=None) -> torch.Tensor:
    """cvt_color_crop_resize_rois with the fused normalize: fp32 (n, h, w, 3),
    or planar (n, 3, h, w) with layout=NCHW, the model-input layout."""
    y4 = _yuv4(yuv)
    _, rects, src_index, n = _roi_batch(_as4d(y4.unsqueeze(-1), NHWC), rects, *_RECTS, src_index)
    if mean is None or std is None:
        raise ValueError("cvt_color_crop_resize_rois_normalize needs mean and stddev (no per-image statistics for ROIs)")
    if out is None:
        out = torch.empty((n, h, w, 3) if layout == NHWC else (n, 3, h, w), dtype=torch.float32, device=yuv.device)
    (ma, meanp), (sa, stdp) = _meanstd(mean, std, 3)
    check("vacv_cvt_color_crop_resize_rois_normalize", L.load().vacv_cvt_color_crop_resize_rois_normalize(
        ctypes.byref(_yuv_desc(y4)), ctypes.byref(describe(out, layout)), code, rects.data_ptr(),
        _idx_ptr(src_index), INTER_LINEAR, mode, meanp, stdp, _stream(stream)))
    return out


def _own_stats(n: int, stats: bool, device):
    """The (n, 3) mean / std tensors of a standardize-from-YUV call and their pointers (None: not written)."""
    if not stats:
        return None, None, None, None
    mean = torch.empty((n, 3), dtype=torch.float32, device=device)
    std = torch.empty((n, 3), dtype=torch.float32, device=device)
    return mean, std, mean.data_ptr(), std.data_ptr()


def cvt_color_crop_resize_rois_standardize(yuv: torch.Tensor, rects, w: int, h: int,
                                           code: int = L.COLOR_YUV2BGR_NV21, src_index=None,
                                           mode: int = LINEAR_REFERENCE, layout: int = NHWC, out=None,
                                           stats: bool = False, stream=None):
    """cvt_color_crop_resize_rois with each crop standardized by its OWN
    per-channel mean and standard deviation, in one launch: fp32 (n, h, w, 3),
    or planar (n, 3, h, w) with layout=NCHW.  Bit for bit cvt_color ->
    crop_resize_rois_standardize, without the decoded frames; yuv, rects and
    src_index as cvt_color_crop_resize_rois takes them; an invalid rect or
    index gives zeros with mean and stddev 0.  stats=True: returns (out, mean,
    std), the two (n, 3) float32 device tensors of every crop's statistics.  A
    crop must fit one workgroup's LDS (144 x 144 does): VacvError(UNSUPPORTED)
    otherwise."""
    y4 = _yuv4(yuv)
    _, rects, src_index, n = _roi_batch(_as4d(y4.unsqueeze(-1), NHWC), rects, *_RECTS, src_index)
    if out is None:
        out = torch.empty((n, h, w, 3) if layout == NHWC else (n, 3, h, w), dtype=torch.float32, device=yuv.device)
    mean, std, meanp, stdp = _own_stats(n, stats, yuv.device)
    check("vacv_cvt_color_crop_resize_rois_standardize", L.load().vacv_cvt_color_crop_resize_rois_standardize(
        ctypes.byref(_yuv_desc(y4)), ctypes.byref(describe(out, layout)), code, rects.data_ptr(),
        _idx_ptr(src_index), INTER_LINEAR, mode, meanp, stdp, _stream(stream)))
    return (out, mean, std) if stats else out


def cvt_color_warp_affine_rois_standardize(yuv: torch.Tensor, ms, w: int, h: int, code: int = L.COLOR_YUV2BGR_NV21,
                                           src_index=None, flags: int = INTER_LINEAR,
                                           border_mode: int = BORDER_CONSTANT, border_value=(0, 0, 0, 0),
                                           layout: int = NHWC, out=None, stats: bool = False, stream=None):
    """cvt_color_warp_affine_rois with each crop standardized by its OWN
    per-channel mean and standard deviation, in one launch: fp32 (n, h, w, 3),
    or planar (n, 3, h, w) with layout=NCHW.  Bit for bit cvt_color ->
    warp_affine_rois_standardize, without the decoded frames; yuv, ms and
    src_index as cvt_color_warp_affine_rois takes them; border pixels count in
    the statistics, and an index outside the frames gives zeros with mean =
    border_value and stddev 0.  stats=True: returns (out, mean, std), the two
    (n, 3) float32 device tensors of every crop's statistics.  A crop must fit
    one workgroup's LDS (144 x 144 does): VacvError(UNSUPPORTED) otherwise."""
    y4 = _yuv4(yuv)
    _, ms, src_index, n = _roi_batch(_as4d(y4.unsqueeze(-1), NHWC), ms, *_MS, src_index)
    if out is None:
        out = torch.empty((n, h, w, 3) if layout == NHWC else (n, 3, h, w), dtype=torch.float32, device=yuv.device)
    mean, std, meanp, stdp = _own_stats(n, stats, yuv.device)
    bv, bp = _border(border_value)
    check("vacv_cvt_color_warp_affine_rois_standardize", L.load().vacv_cvt_color_warp_affine_rois_standardize(
        ctypes.byref(_yuv_desc(y4)), ctypes.byref(describe(out, layout)), code, ms.data_ptr(),
        _idx_ptr(src_index), flags, border_mode, bp, meanp, stdp, _stream(stream)))
    return (out, mean, std) if stats else out


# ---------------------------------------------------------------------------
# normalize / statistics

def normalize(src: torch.Tensor, mean=None, std=None, layout: int = NHWC, out=None, stream=None) -> torch.Tensor:
    """va_cv::normalize (cv.h:104-106)."""
    s4 = _as4d(src, layout)
    c = s4.shape[3] if layout == NHWC else s4.shape[1]
    if out is None:
        out = torch.empty(s4.shape, dtype=torch.float32, device=src.device)
    (ma, mp), (sa, sp) = _meanstd(mean, std, c)
    check("vacv_normalize", L.load().vacv_normalize(ctypes.byref(describe(s4, layout)), ctypes.byref(describe(out, layout)),
                                                    mp, sp, _stream(stream)))
    return _shape_back(out, src, layout)


def channel_sums(src: torch.Tensor, per_image: bool = True, layout: int = NHWC, stream=None) -> torch.Tensor:
    """(groups, c, 2) fp64 device tensor of (Sum x, Sum x^2)."""
    s4 = _as4d(src, layout)
    n = s4.shape[0]
    c = s4.shape[3] if layout == NHWC else s4.shape[1]
    out = torch.empty((n if per_image else 1, c, 2), dtype=torch.float64, device=src.device)
    check("vacv_channel_sums", L.load().vacv_channel_sums(ctypes.byref(describe(s4, layout)), out.data_ptr(),
                                                          int(per_image), _stream(stream)))
    return out


def resize_channel_sums(src: torch.Tensor, w: int, h: int, interpolation: int = INTER_LINEAR,
                        mode: int = LINEAR_REFERENCE, per_image: bool = True, layout: int = NHWC, out=None,
                        stream=None) -> Tuple[torch.Tensor, torch.Tensor]:
    """resize() and channel_sums() of its output in one pass where the kernel
    fuses them (u8 -> fp32 INTER_CUBIC).  Returns (resized, sums)."""
    s4 = _as4d(src, layout)
    if out is None:
        dt = torch.float32 if (interpolation == INTER_CUBIC or src.dtype == torch.float32) else src.dtype
        out = _empty_like_shape(s4, layout, w, h, dt, False, src.dim())
    o4 = _as4d(out, layout)
    c = o4.shape[3] if layout == NHWC else o4.shape[1]
    sums = torch.empty((o4.shape[0] if per_image else 1, c, 2), dtype=torch.float64, device=src.device)
    check("vacv_resize_channel_sums",
          L.load().vacv_resize_channel_sums(ctypes.byref(describe(s4, layout)), ctypes.byref(describe(o4, layout)),
                                            interpolation, mode, sums.data_ptr(), int(per_image), _stream(stream)))
    return out, sums


def resize_mean_stddev(src: torch.Tensor, w: int, h: int, interpolation: int = INTER_LINEAR,
                       mode: int = LINEAR_REFERENCE, per_image: bool = True, layout: int = NHWC, out=None,
                       stream=None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """resize() and the population mean / stddev of its output (per image, or
    over the whole batch) in one call: the one-GPU form of cfg5 (resize, then
    normalize_naive.cpp:7-48's mean_stddev).  Returns (resized, sums, mean,
    stddev); sums is (groups, c, 2) fp64, mean / stddev (groups, c) fp32."""
    s4 = _as4d(src, layout)
    if out is None:
        dt = torch.float32 if (interpolation == INTER_CUBIC or src.dtype == torch.float32) else src.dtype
        out = _empty_like_shape(s4, layout, w, h, dt, False, src.dim())
    o4 = _as4d(out, layout)
    c = o4.shape[3] if layout == NHWC else o4.shape[1]
    groups = o4.shape[0] if per_image else 1
    sums = torch.empty((groups, c, 2), dtype=torch.float64, device=src.device)
    mean = torch.empty((groups, c), dtype=torch.float32, device=src.device)
    std = torch.empty((groups, c), dtype=torch.float32, device=src.device)
    check("vacv_resize_mean_stddev",
          L.load().vacv_resize_mean_stddev(ctypes.byref(describe(s4, layout)), ctypes.byref(describe(o4, layout)),
                                           interpolation, mode, sums.data_ptr(), mean.data_ptr(), std.data_ptr(),
                                           int(per_image), _stream(stream)))
    return out, sums, mean, std


def stats_from_sums(sums: torch.Tensor, count: float, stream=None) -> Tuple[torch.Tensor, torch.Tensor]:
    sums = sums.contiguous()
    groups, c = sums.shape[0], sums.shape[1]
    mean = torch.empty((groups, c), dtype=torch.float32, device=sums.device)
    std = torch.empty((groups, c), dtype=torch.float32, device=sums.device)
    check("vacv_stats_from_sums", L.load().vacv_stats_from_sums(sums.data_ptr(), groups, c, float(count),
                                                                mean.data_ptr(), std.data_ptr(), _stream(stream)))
    return mean, std


def mean_stddev(src: torch.Tensor, layout: int = NHWC, stream=None) -> Tuple[torch.Tensor, torch.Tensor]:
    """Per-image (n, c) population mean / stddev (normalize_naive.cpp:7-72)."""
    s4 = _as4d(src, layout)
    n = s4.shape[0]
    c = s4.shape[3] if layout == NHWC else s4.shape[1]
    mean = torch.empty((n, c), dtype=torch.float32, device=src.device)
    std = torch.empty((n, c), dtype=torch.float32, device=src.device)
    check("vacv_mean_stddev", L.load().vacv_mean_stddev(ctypes.byref(describe(s4, layout)), mean.data_ptr(),
                                                        std.data_ptr(), _stream(stream)))
    return mean, std


def match_template(img: torch.Tensor, templ: torch.Tensor, method: int, out=None, stream=None) -> torch.Tensor:
    """va_cv::match_template (cv.h:211-219): cv::matchTemplate of every image
    (NHWC, u8 or fp32) against one template -> (n,) H-h+1 x W-w+1 fp32."""
    i4 = _as4d(img, NHWC)
    t4 = _as4d(templ, NHWC)
    n, H, W, _ = i4.shape
    _, h, w, _ = t4.shape
    # vacv_match_template's (cv::matchTemplate's) rule: a template at least as
    # large as the image in both directions, and larger in one, is the image
    if w >= W and h >= H and (w > W or h > H) and n == 1:
        W, H, w, h = w, h, W, H
    if w > W or h > H:
        raise ValueError(f"match_template: a {w} x {h} template does not fit the {W} x {H} image"
                         + (" (a batch is never swapped)" if n > 1 else ""))
    if out is None:
        out = torch.empty((n, H - h + 1, W - w + 1), dtype=torch.float32, device=img.device)
    o4 = out.reshape(n, H - h + 1, W - w + 1, 1)  # one channel, NHWC
    check("vacv_match_template", L.load().vacv_match_template(
        ctypes.byref(describe(i4, NHWC)), ctypes.byref(describe(t4, NHWC)), ctypes.byref(describe(o4, NHWC)),
        int(method), _stream(stream)))
    return out if img.dim() == 4 else out[0]


def min_max_idx(src: torch.Tensor, mask: Optional[torch.Tensor] = None, stream=None):
    """va_cv::minMaxIdx (cv.h:221-231) of a 2-D single-channel tensor:
    (min, max, (row, col) of the min, (row, col) of the max)."""
    if src.dim() != 2:
        raise ValueError("minMaxIdx takes a 2-D single-channel tensor")
    vals = torch.empty(2, dtype=torch.float64, device=src.device)
    idx = torch.empty(4, dtype=torch.int32, device=src.device)
    md = ctypes.byref(describe(mask)) if mask is not None else None
    check("vacv_min_max_idx", L.load().vacv_min_max_idx(ctypes.byref(describe(src)), md, vals.data_ptr(),
                                                        idx.data_ptr(), _stream(stream)))
    v = vals.cpu().tolist()
    i = idx.cpu().tolist()
    return v[0], v[1], (i[0], i[1]), (i[2], i[3])


_ORIGINS = ("origins", torch.int32, lambda a: a.dim() == 2 and a.shape[1] == 2, "(n, 2)", "origins holds no window")


def search_origins(centers: torch.Tensor, w: int, h: int, frame_w: int, frame_h: int) -> torch.Tensor:
    """(n, 2) centres (cx, cy), float32 or an integer dtype -> (n, 2) int32
    origins (left, top) of the w x h search windows around them: (int(cx) -
    w // 2, int(cy) - h // 2), a float centre truncated toward zero as crop
    truncates a box, then clamped so that the window lies inside the frame_w x
    frame_h frame.  Computed where `centers` lives."""
    if not isinstance(centers, torch.Tensor) or centers.dim() != 2 or centers.shape[1] != 2:
        raise ValueError("centers must be an (n, 2) tensor")
    if centers.dtype != torch.float32 and (centers.dtype.is_floating_point or centers.dtype == torch.bool):
        raise ValueError("centers must be float32 or an integer tensor")
    if w < 1 or h < 1 or w > frame_w or h > frame_h:
        raise ValueError(f"a {w} x {h} window does not fit a {frame_w} x {frame_h} frame")
    c = centers.to(torch.int64)  # toward zero
    left = (c[:, 0] - w // 2).clamp(0, frame_w - w)
    top = (c[:, 1] - h // 2).clamp(0, frame_h - h)
    return torch.stack([left, top], 1).to(torch.int32).contiguous()


def match_template_rois(src: torch.Tensor, templ: torch.Tensor, origins, w: int, h: int, method: int,
                        src_index=None, peaks: bool = True, out=None, stream=None):
    """Many matches in one launch: result[i] = match_template(the w x h window
    at origins[i] of src[src_index[i]], templ[i] or the one shared templ), and
    with `peaks` its minMaxIdx.  u8 only.  src: NHWC frames (n, h, w, c) or one
    (h, w, c) / (h, w) frame; templ: (th, tw, c) shared, or (n, th, tw, c) one
    per ROI.  origins: (n, 2) int32 device tensor of (left, top) (search_origins
    makes them from centres); src_index: (n,) int32 device tensor, or None (one
    frame for all, or frame i for ROI i).  Both are read by the kernel when it
    runs on `stream`, not by this call; a window outside its frame or a bad
    index gives a map of zeros, vals (0, 0) and idx of -1s.
    Returns (result, vals, idx): (n, h - th + 1, w - tw + 1) float32, (n, 2)
    float64 (min, max) and (n, 4) int32 (min row, min col, max row, max col),
    all on the device; or just result with peaks=False."""
    s4, origins, src_index, n = _roi_batch(_as4d(src, NHWC), origins, *_ORIGINS, src_index)
    t4 = _as4d(templ, NHWC)
    th, tw = t4.shape[1], t4.shape[2]
    if tw > w or th > h:
        raise ValueError(f"match_template_rois: a {tw} x {th} template does not fit the {w} x {h} window")
    rh, rw = h - th + 1, w - tw + 1
    if out is None:
        out = torch.empty((n, rh, rw), dtype=torch.float32, device=src.device)
    elif tuple(out.shape) != (n, rh, rw):
        raise ValueError(f"out must have shape {(n, rh, rw)}, got {tuple(out.shape)}")
    vals = torch.empty((n, 2), dtype=torch.float64, device=src.device) if peaks else None
    idx = torch.empty((n, 4), dtype=torch.int32, device=src.device) if peaks else None
    check("vacv_match_template_rois", L.load().vacv_match_template_rois(
        ctypes.byref(describe(s4, NHWC)), ctypes.byref(describe(t4, NHWC)),
        ctypes.byref(describe(out.unsqueeze(-1), NHWC)), origins.data_ptr(), _idx_ptr(src_index), int(method),
        vals.data_ptr() if peaks else None, idx.data_ptr() if peaks else None, _stream(stream)))
    return (out, vals, idx) if peaks else out


def cvt_color_match_template_rois(yuv: torch.Tensor, templ: torch.Tensor, origins, w: int, h: int, method: int,
                                  code: int = L.COLOR_YUV2BGR_NV21, src_index=None, peaks: bool = True, out=None,
                                  stream=None):
    """match_template_rois straight from NV21 / NV12 frames in one launch:
    bit for bit match_template_rois(cvt_color(yuv, code), templ, ...), without
    the decoded frames.  yuv: (n, h_in*3/2, w_in) u8 frames or one
    (h_in*3/2, w_in) frame; templ: (th, tw, 3) or (n, th, tw, 3) u8 in the
    decoded channel order of `code`; origins: (left, top) of the w x h windows
    in the DECODED frame (search_origins with the decoded frame_w, frame_h).
    Everything else, and what is returned, as match_template_rois."""
    y4 = _yuv4(yuv)
    _, origins, src_index, n = _roi_batch(_as4d(y4.unsqueeze(-1), NHWC), origins, *_ORIGINS, src_index)
    if not isinstance(templ, torch.Tensor) or templ.device != yuv.device:
        raise ValueError("templ must be a tensor on the frames' device")
    if templ.dim() not in (3, 4) or templ.shape[-1] != 3:
        raise ValueError(f"templ must have shape (th, tw, 3) or (n, th, tw, 3), got {tuple(templ.shape)}")
    t4 = _as4d(templ, NHWC)
    th, tw = t4.shape[1], t4.shape[2]
    if tw > w or th > h:
        raise ValueError(f"cvt_color_match_template_rois: a {tw} x {th} template does not fit the {w} x {h} window")
    rh, rw = h - th + 1, w - tw + 1
    if out is None:
        out = torch.empty((n, rh, rw), dtype=torch.float32, device=yuv.device)
    elif tuple(out.shape) != (n, rh, rw):
        raise ValueError(f"out must have shape {(n, rh, rw)}, got {tuple(out.shape)}")
    vals = torch.empty((n, 2), dtype=torch.float64, device=yuv.device) if peaks else None
    idx = torch.empty((n, 4), dtype=torch.int32, device=yuv.device) if peaks else None
    check("vacv_cvt_color_match_template_rois", L.load().vacv_cvt_color_match_template_rois(
        ctypes.byref(_yuv_desc(y4)), ctypes.byref(describe(t4, NHWC)),
        ctypes.byref(describe(out.unsqueeze(-1), NHWC)), int(code), origins.data_ptr(), _idx_ptr(src_index),
        int(method), vals.data_ptr() if peaks else None, idx.data_ptr() if peaks else None, _stream(stream)))
    return (out, vals, idx) if peaks else out


def set_tuning(name: str, value: int) -> int:
    """Select a kernel variant (VACV_TUNE_<name>, include/vacv_hip.h); value
    < 0 restores the built-in choice.  Returns the previous value."""
    key = L.TUNE[name]
    lib = L.load()
    old = lib.vacv_get_tuning(key)
    check("vacv_set_tuning", lib.vacv_set_tuning(key, int(value)))
    return old


def release_workspace() -> None:
    """vacv_release_workspace: frees the per-stream workspaces and the cached plans and tables; the next call rebuilds them."""
    check("vacv_release_workspace", L.load().vacv_release_workspace())


class tuning:
    """Context manager: `with ops.tuning(WARP_KERNEL=0): ...` runs the block
    with those kernel variants and restores the previous choices after."""

    def __init__(self, **knobs):
        self.knobs = knobs
        self.old = {}

    def __enter__(self):
        for k, v in self.knobs.items():
            self.old[k] = set_tuning(k, v)
        return self

    def __exit__(self, *exc):
        for k, v in self.old.items():
            set_tuning(k, v)
        return False
