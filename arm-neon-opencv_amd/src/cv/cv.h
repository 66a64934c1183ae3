// va_cv:: -- the vacv image-operator API, MI355X build.
//
// Same names, signatures, defaults and enum values as the reference's
// src/cv/cv.h:9-241, so code written against it (including the reference's
// src/test harness) compiles unchanged.  Every operator is one or more HIP
// kernels for gfx950 behind the C ABI in include/vacv_hip.h; nothing here
// computes pixels on the host.
//
// Behaviour relative to the reference:
//   - outputs take the placement of `src` (host tensors are staged through
//     pinned buffers; device tensors stay in HBM), and calls are synchronous;
//   - combinations the reference silently skips or recurses on forever throw
//     std::runtime_error instead;
//   - warp_affine does not modify M and writes borderValue outside the source.
#ifndef VISION_CV_H
#define VISION_CV_H

#include <vector>

#include "../common/tensor.h"
#include "../common/vision_structs.h"

namespace va_cv {

struct VSize {
    int w;
    int h;
    VSize() : w(0), h(0) {}
    VSize(int _w, int _h) : w(_w), h(_h) {}
};

struct VScalar {
    double v0;
    double v1;
    double v2;
    double v3;
    VScalar() : v0(0), v1(0), v2(0), v3(0) {}
};

/// interpolation (cv.h:27-36)
enum VInterMode {
    INTER_NEAREST = 0,
    INTER_LINEAR = 1,
    INTER_CUBIC = 2,
    INTER_AREA = 3,
    INTER_LANCZOS4 = 4,
    INTER_MAX = 7,
    WARP_INVERSE_MAP = 16
};

/// border handling (cv.h:39-49)
enum VBorderMode {
    BORDER_REPLICATE = 1,
    BORDER_CONSTANT = 0,
    BORDER_REFLECT = 2,
    BORDER_WRAP = 3,
    BORDER_REFLECT_101 = 4,
    BORDER_REFLECT101 = 4,
    BORDER_TRANSPARENT = 5,
    BORDER_DEFAULT = 4,
    BORDER_ISOLATED = 16
};

/// template-matching methods (cv.h:52-59)
enum VMatchMode {
    TM_SQDIFF = 0,
    TM_SQDIFF_NORMED = 1,
    TM_CCORR = 2,
    TM_CCORR_NORMED = 3,
    TM_CCOEFF = 4,
    TM_CCOEFF_NORMED = 5
};

/// colour conversion codes (cv.h:62-74)
enum InputImageFormat {
    COLOR_GRAY2RGB = 8,
    COLOR_GRAY2BGR = COLOR_GRAY2RGB,
    COLOR_YUV2RGB_NV12 = 90,
    COLOR_YUV2BGR_NV12 = 91,
    COLOR_YUV2RGB_NV21 = 92,
    COLOR_YUV2BGR_NV21 = 93,
    COLOR_YUV2RGBA_NV12 = 94,
    COLOR_YUV2BGRA_NV12 = 95,
    COLOR_YUV2RGBA_NV21 = 96,
    COLOR_YUV2BGRA_NV21 = 97,
    COLOR_YUV2BGR_YV12 = 99
};

/// Resize to dsize (fx, fy ignored, as in resize.cpp:51-56, except for
/// INTER_NEAREST / INTER_AREA with dsize = 0, which the reference hands to
/// cv::resize: dsize = round(w * fx, h * fy), inv_scale = fx, fy).
/// INTER_LINEAR: INT8 -> INT8 (bit-exact with resize_naive_inter_linear_u8),
/// FP32 -> FP32.  INTER_CUBIC: FP32 -> FP32, and INT8 -> FP32 (a fused widen;
/// the reference recurses forever on INT8 cubic).  NHWC or NCHW.
void resize(const vision::Tensor& src, vision::Tensor& dst,
            VSize dsize, double fx = 0, double fy = 0,
            int interpolation = INTER_LINEAR);

/// YUV420sp (w, h*3/2, 1) INT8 -> (w, h, 3) INT8 NHWC (cvt_color.cpp:137-157).
/// COLOR_YUV2BGR_NV21 is bit-exact with nv_to_bgr_naive; NV12 and the RGB
/// orders are also decoded.  The codes the reference hands to cv::cvtColor
/// (cvt_color.cpp:139-141) follow OpenCV 2.4: COLOR_YUV2RGBA/BGRA_NV12/NV21
/// -> (w, h, 4), COLOR_YUV2BGR_YV12 (planar V, U) -> (w, h, 3), and
/// COLOR_GRAY2BGR (w, h, 1) INT8/FP32 -> (w, h, 3) of the same dtype.
void cvt_color(const vision::Tensor& src, vision::Tensor& dst, int code);

/// dst = (x - mean[k]) / (stddev[k] + 1e-6), FP32, same layout
/// (normalize.cpp:84-121).  mean/stddev: FP32 tensors of c values; both
/// empty = per-image statistics of src.
void normalize(const vision::Tensor& src, vision::Tensor& dst,
               const vision::Tensor& mean = vision::Tensor(),
               const vision::Tensor& stddev = vision::Tensor());

/// Affine warp by the FORWARD 2x3 map M (3x2x1 FP32 tensor), INTER_LINEAR
/// (warp_affine.cpp:111-169).  M is not modified.  BORDER_CONSTANT is the
/// reference's naive path; REPLICATE / REFLECT / WRAP / REFLECT_101 /
/// TRANSPARENT extend it (the reference hands them to OpenCV).
void warp_affine(const vision::Tensor& src, vision::Tensor& dst,
                 const vision::Tensor& M, VSize dsize,
                 int flags = INTER_LINEAR,
                 int borderMode = BORDER_CONSTANT,
                 const VScalar& borderValue = VScalar());

/// Warp by rotation `rot` (degrees) and `scale` about the origin, translated
/// by aux_param (warp_affine.cpp:76-109).
void warp_affine(const vision::Tensor& src, vision::Tensor& dst,
                 float scale, float rot, VSize dsize,
                 const VScalar& aux_param = VScalar(),
                 int flags = INTER_LINEAR,
                 int borderMode = BORDER_CONSTANT,
                 const VScalar& borderValue = VScalar());

/// resize + convert to FP32 + normalize in one kernel (resize_normalize.cpp:
/// 33-107).  Either statistic empty = per-image statistics of the resized
/// image.
void resize_normalize(const vision::Tensor& src, vision::Tensor& dst,
                      VSize dsize, double fx = 0, double fy = 0,
                      int interpolation = INTER_LINEAR,
                      const vision::Tensor& mean = vision::Tensor(),
                      const vision::Tensor& stddev = vision::Tensor());

/// warp_affine + convert to FP32 + normalize in one kernel
/// (warp_affine_normalize.cpp:13-210).
void warp_affine_normalize(const vision::Tensor& src, vision::Tensor& dst,
                           const vision::Tensor& M, VSize dsize,
                           int flags = INTER_LINEAR,
                           int borderMode = BORDER_CONSTANT,
                           const VScalar& borderValue = VScalar(),
                           const vision::Tensor& mean = vision::Tensor(),
                           const vision::Tensor& stddev = vision::Tensor());

void warp_affine_normalize(const vision::Tensor& src, vision::Tensor& dst,
                           float scale, float rot, VSize dsize,
                           const VScalar& aux_param = VScalar(),
                           int flags = INTER_LINEAR,
                           int borderMode = BORDER_CONSTANT,
                           const VScalar& borderValue = VScalar(),
                           const vision::Tensor& mean = vision::Tensor(),
                           const vision::Tensor& stddev = vision::Tensor());

/// ROI copy; the rect is truncated to int (crop.cpp:127-142).
void crop(const vision::Tensor& src, vision::Tensor& dst, const vision::VRect& rect);

/// Template matching (match_template.cpp:13-41 hands it to cv::matchTemplate):
/// OpenCV 2.4's six TM_* methods, INT8 / FP32 NHWC, c <= 4; result =
/// (W-w+1, H-h+1, 1) FP32.  The correlation is computed exactly on the GPU.
void match_template(const vision::Tensor& src, const vision::Tensor& target,
                    vision::Tensor& result, int method);
/// cv::minMaxIdx of a single-channel tensor (match_template.cpp:43-46):
/// first minimum / maximum in row-major order among mask != 0; indices are
/// (row, col).
void minMaxIdx(const vision::Tensor& src, double* minVal, double* maxVal,
               int* minIdx = nullptr, int* maxIdx = nullptr, const vision::Tensor& mask = vision::Tensor());
/// OpenCV-only in the reference (imencode.cpp, a codec): throws.
void imencode(const vision::Tensor& src, std::vector<unsigned char>& buf, const char* format);

// ---- additions (not in the reference) -----------------------------------

/// Per-channel population mean / stddev of one image (the statistics the
/// reference computes inside normalize, normalize_naive.cpp:7-72), exact
/// (integer / fp64 accumulation).  mean, stddev: host FP32 tensors (c).
void mean_stddev(const vision::Tensor& src, vision::Tensor& mean, vision::Tensor& stddev);

/// cvt_color then normalize, one kernel (the BASELINE cfg3 pipeline).
void cvt_color_normalize(const vision::Tensor& src, vision::Tensor& dst, int code,
                         const vision::Tensor& mean = vision::Tensor(),
                         const vision::Tensor& stddev = vision::Tensor());

/// Batched frames: the operator above applied to every
/// frame of `src` into the matching `dst` (resized to src.size()).  Host
/// frames are staged through a ring of HBM buffers on three HIP streams, so
/// the H2D copy of frame i+1, the kernel of frame i and the D2H copy of frame
/// i-1 overlap -- one call per frame serialises them on one stream.  Device
/// frames run back to back.  Returns when every dst is written.
void resize(const std::vector<vision::Tensor>& src, std::vector<vision::Tensor>& dst, VSize dsize,
            double fx = 0, double fy = 0, int interpolation = INTER_LINEAR);
void resize_normalize(const std::vector<vision::Tensor>& src, std::vector<vision::Tensor>& dst, VSize dsize,
                      double fx = 0, double fy = 0, int interpolation = INTER_LINEAR,
                      const vision::Tensor& mean = vision::Tensor(),
                      const vision::Tensor& stddev = vision::Tensor());
void warp_affine(const std::vector<vision::Tensor>& src, std::vector<vision::Tensor>& dst,
                 const vision::Tensor& M, VSize dsize, int flags = INTER_LINEAR,
                 int borderMode = BORDER_CONSTANT, const VScalar& borderValue = VScalar());
/// One frame, M.size() crops, ONE kernel launch (the detection-pipeline shape
/// of the (scale, rot, aux) overload above: one small upright crop per
/// object, each with its own map).  dst[i] = warp_affine(src, M[i], dsize),
/// byte for byte; src NHWC, INTER_LINEAR (optionally | WARP_INVERSE_MAP), every
/// border mode but TRANSPARENT.  A host frame and host matrices are staged
/// once through the pinned pool; device tensors stay where they are.  dst is
/// resized to M.size(), each crop with the placement of src.
void warp_affine(const vision::Tensor& src, std::vector<vision::Tensor>& dst,
                 const std::vector<vision::Tensor>& M, VSize dsize, int flags = INTER_LINEAR,
                 int borderMode = BORDER_CONSTANT, const VScalar& borderValue = VScalar());
/// The same with the fused normalize (FP32 crops); mean and stddev are
/// required (no per-image statistics for crops).
void warp_affine_normalize(const vision::Tensor& src, std::vector<vision::Tensor>& dst,
                           const std::vector<vision::Tensor>& M, VSize dsize, int flags = INTER_LINEAR,
                           int borderMode = BORDER_CONSTANT, const VScalar& borderValue = VScalar(),
                           const vision::Tensor& mean = vision::Tensor(),
                           const vision::Tensor& stddev = vision::Tensor());
/// The same with every crop standardized by ITS OWN per-channel mean and
/// standard deviation, ONE kernel launch: dst[i] is, bit for bit,
/// warp_affine(src, M[i], dsize) then normalize() with mean and stddev left
/// empty (FP32 crops; border pixels count in the statistics;
/// vacv_warp_affine_rois_standardize).  src INT8 (an FP32 frame throws), and
/// a crop must fit one workgroup's LDS -- 144 x 144 x 3 does; a larger dsize
/// throws.  stats, when given, becomes {mean, stddev}: two host FP32 tensors
/// (w = c, h = M.size()), row i the statistics of crop i.
void warp_affine_standardize(const vision::Tensor& src, std::vector<vision::Tensor>& dst,
                             const std::vector<vision::Tensor>& M, VSize dsize, int flags = INTER_LINEAR,
                             int borderMode = BORDER_CONSTANT, const VScalar& borderValue = VScalar(),
                             std::vector<vision::Tensor>* stats = nullptr);
/// The same crops straight from one YUV420sp frame (w, h*3/2, 1) INT8 NHWC,
/// ONE kernel launch and no decoded frame: dst[i] = warp_affine(cvt_color(yuv,
/// code), M[i], dsize), byte for byte, (w, h, 3) crops.  code: the NV21 / NV12
/// -> BGR / RGB codes; borderValue in the decoded channel order.
void cvt_color_warp_affine(const vision::Tensor& yuv, std::vector<vision::Tensor>& dst,
                           const std::vector<vision::Tensor>& M, int code, VSize dsize, int flags = INTER_LINEAR,
                           int borderMode = BORDER_CONSTANT, const VScalar& borderValue = VScalar());
void cvt_color_warp_affine_normalize(const vision::Tensor& yuv, std::vector<vision::Tensor>& dst,
                                     const std::vector<vision::Tensor>& M, int code, VSize dsize,
                                     int flags = INTER_LINEAR, int borderMode = BORDER_CONSTANT,
                                     const VScalar& borderValue = VScalar(),
                                     const vision::Tensor& mean = vision::Tensor(),
                                     const vision::Tensor& stddev = vision::Tensor());
/// ... each standardized by ITS OWN per-channel mean and standard deviation,
/// ONE kernel launch and no decoded frame: dst[i] is, bit for bit, what
/// warp_affine_standardize gives on cvt_color(yuv, code)
/// (vacv_cvt_color_warp_affine_rois_standardize).  dsize up to 144 x 144 (a
/// larger one throws); stats as warp_affine_standardize fills it, c = 3.
void cvt_color_warp_affine_standardize(const vision::Tensor& yuv, std::vector<vision::Tensor>& dst,
                                       const std::vector<vision::Tensor>& M, int code, VSize dsize,
                                       int flags = INTER_LINEAR, int borderMode = BORDER_CONSTANT,
                                       const VScalar& borderValue = VScalar(),
                                       std::vector<vision::Tensor>* stats = nullptr);
/// One frame, M.size() projective crops, ONE kernel launch (the rectified
/// quads of an OCR, plate or document pipeline): dst[i] = OpenCV's
/// warpPerspective shape under the 3x3 homography M[i] (3x3x1 FP32 tensor,
/// row-major; FORWARD maps, or dst -> src maps with flags | WARP_INVERSE_MAP),
/// the coordinates in double with one reciprocal and the pixel the naive
/// warp_affine sampler's (vacv_warp_perspective_rois).  Everything else --
/// src, flags, border modes, staging, placement of dst -- as the warp_affine
/// overload with a vector of matrices above.
void warp_perspective(const vision::Tensor& src, std::vector<vision::Tensor>& dst,
                      const std::vector<vision::Tensor>& M, VSize dsize, int flags = INTER_LINEAR,
                      int borderMode = BORDER_CONSTANT, const VScalar& borderValue = VScalar());
/// The same with the fused normalize (FP32 crops); mean and stddev are required.
void warp_perspective_normalize(const vision::Tensor& src, std::vector<vision::Tensor>& dst,
                                const std::vector<vision::Tensor>& M, VSize dsize, int flags = INTER_LINEAR,
                                int borderMode = BORDER_CONSTANT, const VScalar& borderValue = VScalar(),
                                const vision::Tensor& mean = vision::Tensor(),
                                const vision::Tensor& stddev = vision::Tensor());
/// OpenCV's single-image signature: a batch of one.
void warp_perspective(const vision::Tensor& src, vision::Tensor& dst, const vision::Tensor& M, VSize dsize,
                      int flags = INTER_LINEAR, int borderMode = BORDER_CONSTANT,
                      const VScalar& borderValue = VScalar());
/// cv::getPerspectiveTransform: M (3x3x1 host FP32, M[8] = 1) maps the four
/// points src_quad (x0 y0 .. x3 y3) to dst_quad.  A degenerate quad throws.
void get_perspective_transform(const float src_quad[8], const float dst_quad[8], vision::Tensor& M);
/// One frame, rects.size() upright crops, ONE kernel launch: dst[i] =
/// resize(crop(src, rects[i]), dsize), byte for byte what crop() followed by
/// resize() gives (taps clamped at the rect's edges; vacv_crop_resize_rois).
/// src NHWC, INT8 or FP32, c <= 4; INTER_LINEAR only.  The rects are truncated
/// as crop() truncates them and staged once through the pinned pool with a
/// host frame; a device frame stays where it is.  A rect that does not lie
/// inside the frame, or is smaller than 2 x 2, throws.  dst is resized to
/// rects.size(), each crop with the placement of src.
void crop_resize(const vision::Tensor& src, std::vector<vision::Tensor>& dst,
                 const std::vector<vision::VRect>& rects, VSize dsize, int interpolation = INTER_LINEAR);
/// The same with the fused normalize (FP32 crops); mean and stddev are
/// required (no per-image statistics for crops).
void crop_resize_normalize(const vision::Tensor& src, std::vector<vision::Tensor>& dst,
                           const std::vector<vision::VRect>& rects, VSize dsize, int interpolation = INTER_LINEAR,
                           const vision::Tensor& mean = vision::Tensor(),
                           const vision::Tensor& stddev = vision::Tensor());
/// The same with every crop standardized by ITS OWN per-channel mean and
/// standard deviation, ONE kernel launch: dst[i] is, bit for bit, crop() then
/// resize() then normalize() with mean and stddev left empty (FP32 crops;
/// vacv_crop_resize_rois_standardize).  src INT8 (an FP32 frame throws), and
/// a crop must fit one workgroup's LDS -- 144 x 144 x 3 does; a larger dsize
/// throws.  stats, when given, becomes {mean, stddev}: two host FP32 tensors
/// (w = c, h = rects.size()), row i the statistics of crop i.
void crop_resize_standardize(const vision::Tensor& src, std::vector<vision::Tensor>& dst,
                             const std::vector<vision::VRect>& rects, VSize dsize, int interpolation = INTER_LINEAR,
                             std::vector<vision::Tensor>* stats = nullptr);
/// The same upright crops straight from one YUV420sp frame (w, h*3/2, 1) INT8
/// NHWC, ONE kernel launch and no decoded frame: dst[i] = resize(crop(
/// cvt_color(yuv, code), rects[i]), dsize), byte for byte, (w, h, 3) crops.
/// code: the NV21 / NV12 -> BGR / RGB codes; the rects lie in the decoded frame.
void cvt_color_crop_resize(const vision::Tensor& yuv, std::vector<vision::Tensor>& dst,
                           const std::vector<vision::VRect>& rects, int code, VSize dsize,
                           int interpolation = INTER_LINEAR);
void cvt_color_crop_resize_normalize(const vision::Tensor& yuv, std::vector<vision::Tensor>& dst,
                                     const std::vector<vision::VRect>& rects, int code, VSize dsize,
                                     int interpolation = INTER_LINEAR,
                                     const vision::Tensor& mean = vision::Tensor(),
                                     const vision::Tensor& stddev = vision::Tensor());
/// ... each standardized by ITS OWN per-channel mean and standard deviation,
/// ONE kernel launch and no decoded frame: dst[i] is, bit for bit, what
/// crop_resize_standardize gives on cvt_color(yuv, code)
/// (vacv_cvt_color_crop_resize_rois_standardize).  dsize up to 144 x 144 (a
/// larger one throws); stats as crop_resize_standardize fills it, c = 3.
void cvt_color_crop_resize_standardize(const vision::Tensor& yuv, std::vector<vision::Tensor>& dst,
                                       const std::vector<vision::VRect>& rects, int code, VSize dsize,
                                       int interpolation = INTER_LINEAR,
                                       std::vector<vision::Tensor>* stats = nullptr);
/// A tracker's step: one frame, windows.size() search windows, ONE kernel
/// launch.  results[i] = match_template(crop(src, windows[i]), target i,
/// method) and, with `peaks`, (*peaks)[i] = its minMaxIdx, byte for byte what
/// the three single calls give (vacv_match_template_rois).  src and targets
/// INT8 NHWC, c <= 4.  The windows are truncated as crop() truncates them; all
/// windows have one size and all targets one size; targets.size() is 1 (shared)
/// or windows.size().  Anything else, a window outside the frame, a template
/// larger than the window or a window too large for one workgroup's LDS
/// throws.  A host frame, host templates and the origins are staged once
/// through the pinned pool; device tensors stay where they are.  results and
/// peaks are resized to windows.size(), each result with the placement of src.
struct VMatchPeak { double minVal, maxVal; int minIdx[2], maxIdx[2]; };   // (row, col), as minMaxIdx
void match_template(const vision::Tensor& src, const std::vector<vision::Tensor>& targets,
                    const std::vector<vision::VRect>& windows, std::vector<vision::Tensor>& results,
                    int method, std::vector<VMatchPeak>* peaks = nullptr);
/// The same step straight from one YUV420sp frame (w, h*3/2, 1) INT8 NHWC, ONE
/// kernel launch and no decoded frame: results and peaks are bit for bit those
/// of match_template(cvt_color(yuv, code), targets, windows, ...)
/// (vacv_cvt_color_match_template_rois).  code: the NV21 / NV12 -> BGR / RGB
/// codes; the windows lie in the decoded (w, h) frame and the targets are
/// (tw, th, 3) INT8 NHWC in the decoded channel order.  Truncation, the
/// throwing conditions and the placement of the results are the overload's above.
void cvt_color_match_template(const vision::Tensor& yuv, const std::vector<vision::Tensor>& targets,
                              const std::vector<vision::VRect>& windows, std::vector<vision::Tensor>& results,
                              int code, int method, std::vector<VMatchPeak>* peaks = nullptr);
void cvt_color(const std::vector<vision::Tensor>& src, std::vector<vision::Tensor>& dst, int code);
void cvt_color_normalize(const std::vector<vision::Tensor>& src, std::vector<vision::Tensor>& dst, int code,
                         const vision::Tensor& mean = vision::Tensor(),
                         const vision::Tensor& stddev = vision::Tensor());

}  // namespace va_cv

#endif  // VISION_CV_H
