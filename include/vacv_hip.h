/*
 * vacv_hip.h -- C ABI of the MI355X-native vacv pixel operators.
 *
 * This is the drop-in boundary for the reference's operator API
 * (/root/reference/src/cv/cv.h:85-209, vision::Tensor in
 * src/common/tensor.h:27-84).  The C++ surface in
 * arm-neon-opencv_amd/src/{common,cv,util} keeps the reference's names and
 * signatures and is a thin wrapper over these entry points; any FFI
 * (ctypes, cgo, JNI, N-API) binds this header directly.
 *
 * Conventions
 *  - Every image pointer is DEVICE-accessible memory (hipMalloc, or mapped
 *    hipHostMalloc).  Nothing here copies host<->device; the C++ wrapper
 *    stages host tensors.
 *  - Batched: an image descriptor covers `n` images, `batch_pitch` bytes
 *    apart.  One call = one launch sequence on `stream` (a hipStream_t, or
 *    NULL for the default stream).  Calls are asynchronous and never
 *    synchronise the device; host-side arrays passed in (mean, stddev, M,
 *    border values) are consumed before the call returns.
 *  - Return value: VACV_OK (0) or a negative vacv_status.  No C++ exception
 *    crosses this boundary.
 *  - dtype / layout codes are the reference's vision::DType / DLayout values
 *    (tensor.h:12-24); interpolation, border and colour codes are the
 *    reference's va_cv enums (cv.h:27-74).
 */
#ifndef VACV_HIP_H
#define VACV_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Bumped when a signature, an enum value or the tuning enum changes.  An
 * added export alone does not bump it (vacv_crop_resize_rois[_normalize] and
 * the four _rois_standardize functions came under 5): a caller built against the older header still gets what it asked. */
#define VACV_ABI_VERSION 5
#define VACV_MAX_CHANNELS 16

typedef enum vacv_status {
    VACV_OK = 0,
    VACV_ERR_INVALID_ARG = -1,  /* bad pointer / size / pitch / rect */
    VACV_ERR_UNSUPPORTED = -2,  /* dtype, layout, mode or code not implemented */
    VACV_ERR_HIP = -3,          /* a HIP runtime call failed */
    VACV_ERR_NO_MEMORY = -4     /* device workspace allocation failed */
} vacv_status;

/* vision::DType (tensor.h:12-18) */
enum { VACV_FP32 = 0, VACV_FP16 = 1, VACV_INT8 = 2 /* unsigned bytes */, VACV_FP64 = 3 };
/* vision::DLayout (tensor.h:21-24) */
enum { VACV_NCHW = 0, VACV_NHWC = 1 };
/* va_cv::VInterMode (cv.h:27-35) */
enum { VACV_INTER_NEAREST = 0, VACV_INTER_LINEAR = 1, VACV_INTER_CUBIC = 2, VACV_INTER_AREA = 3, VACV_INTER_LANCZOS4 = 4 };
/* warp flag (cv.h:35): m is already the inverse (dst -> src) map */
enum { VACV_WARP_INVERSE_MAP = 16 };
/* va_cv::VBorderMode (cv.h:38-48) */
enum {
    VACV_BORDER_CONSTANT = 0, VACV_BORDER_REPLICATE = 1, VACV_BORDER_REFLECT = 2, VACV_BORDER_WRAP = 3,
    VACV_BORDER_REFLECT_101 = 4, VACV_BORDER_TRANSPARENT = 5
};
/* va_cv::InputImageFormat (cv.h:62-74) */
enum {
    VACV_COLOR_YUV2RGB_NV12 = 90, VACV_COLOR_YUV2BGR_NV12 = 91,
    VACV_COLOR_YUV2RGB_NV21 = 92, VACV_COLOR_YUV2BGR_NV21 = 93,
    /* the codes the reference hands to cv::cvtColor (cvt_color.cpp:139-141) */
    VACV_COLOR_GRAY2BGR = 8,
    VACV_COLOR_YUV2RGBA_NV12 = 94, VACV_COLOR_YUV2BGRA_NV12 = 95,
    VACV_COLOR_YUV2RGBA_NV21 = 96, VACV_COLOR_YUV2BGRA_NV21 = 97,
    VACV_COLOR_YUV2BGR_YV12 = 99
};
/* Arithmetic of the u8 bilinear sampler.
 *  REFERENCE: the path the reference's public API actually dispatches to,
 *             ResizeNaive::resize_naive_inter_linear_u8 (resize_naive.cpp:10-68).
 *  NEON:      ResizeNeon (resize_neon.cpp:12-188), two-pass fixed point.
 *  OPENCV:    NEON arithmetic with round-half-even coefficients (OpenCV 2.4's
 *             saturate_cast<short>); SURVEY.md App. B. */
enum { VACV_LINEAR_REFERENCE = 0, VACV_LINEAR_NEON = 1, VACV_LINEAR_OPENCV = 2 };

/* A batch of images.  Pitches are in BYTES; 0 selects the dense value.
 *   NHWC: pixel (x,y) channel k of image i at
 *         data + i*batch_pitch + y*row_pitch + (x*c + k)*esize
 *   NCHW: data + i*batch_pitch + k*plane_pitch + y*row_pitch + x*esize
 * For the NV21/NV12 input of vacv_cvt_color the descriptor is the
 * reference's (w, h*3/2, c=1) single-plane tensor (cvt_color.cpp:151-152). */
typedef struct vacv_image {
    void* data;
    int32_t n;
    int32_t w;
    int32_t h;
    int32_t c;
    int32_t dtype;
    int32_t layout;
    int64_t row_pitch;
    int64_t plane_pitch;
    int64_t batch_pitch;
} vacv_image;

int vacv_abi_version(void);
const char* vacv_status_string(int status);
/* bytes of one image's valid data under the dense-pitch rules above */
int64_t vacv_image_bytes(const vacv_image* img);

/* ---- geometry / dtype ------------------------------------------------- */

/* Crop::crop (crop.cpp:22-142, cv.h:209).  The rect is already truncated to
 * int as crop_naive does (crop.cpp:128-131); dst->w/h are the crop size and
 * dst->layout/dtype must equal src's.  Rect must lie inside src. */
int vacv_crop(const vacv_image* src, const vacv_image* dst, int left, int top, void* stream);

/* Tensor::change_layout (tensor.cpp:393-457): NHWC <-> NCHW of 1,2,4 or 8
 * byte elements.  Same layout is a plain copy (clone()) and takes pitched
 * images.  Across layouts (c == 1 included, a copy too) both images must be
 * dense -- no row, plane or batch padding -- or the call returns
 * VACV_ERR_UNSUPPORTED and writes nothing. */
int vacv_change_layout(const vacv_image* src, const vacv_image* dst, void* stream);

/* Tensor::change_dtype (tensor.cpp:459-502): INT8 -> FP32 exact; FP32 ->
 * INT8 with the NEON f32_2_u8_neon semantics (truncate; NaN/negative -> 0;
 * low 8 bits kept: +inf and values >= 2^32 -> 255, 256.7 -> 0).  Same dtype
 * is a copy and takes pitched images; INT8 <-> FP32 needs both images dense
 * (VACV_ERR_UNSUPPORTED otherwise, nothing written); other pairs
 * VACV_ERR_UNSUPPORTED (the reference silently returns an uninitialised
 * tensor). */
int vacv_change_dtype(const vacv_image* src, const vacv_image* dst, void* stream);

/* Resize::resize (resize.cpp:19-100, cv.h:85-87).  Only dst->w/h select the
 * output size (fx/fy are ignored, as in the reference).
 *  INTER_LINEAR: INT8->INT8 (mode = VACV_LINEAR_*), FP32->FP32.
 *  INTER_CUBIC:  FP32->FP32 and INT8->FP32 (the u8->fp32 conversion the
 *                reference requires before cubic, fused).
 *  INTER_NEAREST: INT8->INT8, FP32->FP32 with OpenCV 2.4's resizeNN
 *                semantics, which the reference delegates to cv::resize
 *                (resize.cpp:44-49): sx = min(floor(x / (w_out / w_in)), w_in - 1).
 *  INTER_AREA:   INT8->INT8, FP32->FP32 (OpenCV 2.4's cv::resize, also
 *                behind resize.cpp:44-49): integer down-scales = the mean of
 *                each block (resizeAreaFast_; u8 rounded half to even, 2x2
 *                blocks of 1/3/4 channels half up), other down-scales =
 *                resizeArea_'s weight tables, up-scales = its bilinear with
 *                area-mode taps (parity unpinned).
 * NHWC channels 1..4; NCHW any c (per plane, as resize.cpp:72-88).
 * INTER_LINEAR / INTER_CUBIC with dst->w/h == src->w/h copy the source
 * (resize.cpp:58-61; INT8 -> FP32 under INTER_CUBIC widens it), pitched
 * images included, as at every other size. */
int vacv_resize(const vacv_image* src, const vacv_image* dst, int interpolation, int mode, void* stream);

/* vacv_resize with cv::resize's explicit scale factors (the reference passes
 * fx / fy through to OpenCV, resize.cpp:35, :47): INTER_NEAREST and
 * INTER_AREA only; dst->w/h must be the size cv::resize derives,
 * saturate_cast<int>(w * fx) (round half to even), and the sampling uses
 * inv_scale = fx, fy instead of dst/src. */
int vacv_resize_scaled(const vacv_image* src, const vacv_image* dst, int interpolation, int mode, double fx,
                       double fy, void* stream);

/* WarpAffine::warp_affine (warp_affine.cpp:16-36, :111-169, cv.h:118-122).
 * m = the FORWARD 2x3 map, row-major; it is inverted on the host with the
 * reference's arithmetic and is NOT modified (the reference inverts the
 * caller's M in place).  flags = INTER_LINEAR or INTER_NEAREST, optionally
 * | VACV_WARP_INVERSE_MAP (m is then the dst -> src map, used as is); the
 * reference hands every flag but INTER_LINEAR to cv::warpAffine
 * (warp_affine.cpp:114-118), so those are restated from OpenCV 2.4 (parity
 * unpinned):
 *   INTER_NEAREST  cv::warpAffine's fp64 fixed point (AB_BITS = 10, round
 *                  half to even), remap's nearest sampler; the border modes
 *                  below on the mapped pixel
 * INTER_LINEAR: a pixel whose top-left tap is
 * inside [0,w-2]x[0,h-2] is the reference's naive sampler bit for bit (with
 * VACV_WARP_INVERSE_MAP too: the reference would hand that flag to
 * cv::warpAffine, whose INTER_BITS = 5 remap tables round differently, so
 * LINEAR | WARP_INVERSE_MAP keeps the naive arithmetic and does NOT
 * reproduce OpenCV's); the others depend on border_mode:
 *   BORDER_CONSTANT     border_value (the reference leaves them untouched);
 *                       border_value may be NULL (zeros)
 *   BORDER_TRANSPARENT  left untouched (the reference's own behaviour); dst
 *                       must not alias src
 *   BORDER_REPLICATE, _REFLECT, _WRAP, _REFLECT_101
 *                       the four taps at floor(f), floor(f)+1 mapped through
 *                       OpenCV 2.4's borderInterpolate, the naive sampler's
 *                       weights (the reference hands these modes to OpenCV,
 *                       warp_affine.cpp:114-118; parity unpinned) */
int vacv_warp_affine(const vacv_image* src, const vacv_image* dst, const float m[6],
                     int flags, int border_mode, const double border_value[4], void* stream);

/* get_rotation_matrix_2D(VPoint(0,0), rot, scale) + the aux translation fix
 * of the (scale, rot) overload (warp_affine.cpp:76-109).  Host only. */
int vacv_rotation_matrix(float scale, float rot_deg, const double aux[4], float m_out[6]);
/* The in-place inverse of warp_affine.cpp:121-133, out of place.  Host only. */
int vacv_invert_affine(const float m[6], float inv_out[6]);

/* ---- colour ----------------------------------------------------------- */

/* CvtColor::cvt_color (cvt_color.cpp:20-157, cv.h:95): YUV420sp -> 3ch u8
 * NHWC.  src = (w, h*3/2, 1) INT8; dst = (w, h, 3) INT8 NHWC.  Codes:
 * COLOR_YUV2BGR_NV21 (bit-exact with nv_to_bgr_naive), COLOR_YUV2BGR_NV12
 * (correct UV order; the reference decodes it as NV21), and the two RGB
 * variants.  w and h must be even.
 * The codes the reference hands to cv::cvtColor (cvt_color.cpp:139-141),
 * with OpenCV 2.4's arithmetic (BT.601, 20-bit fixed point; parity
 * unpinned):
 *   COLOR_YUV2RGBA/BGRA_NV12/NV21  src as above, dst (w, h, 4) INT8 NHWC, alpha 255
 *   COLOR_YUV2BGR_YV12             src = (w, h*3/2, 1) INT8 with dense rows:
 *                                  Y, then the (w/2)x(h/2) V and U planes;
 *                                  dst (w, h, 3) INT8 NHWC
 *   COLOR_GRAY2BGR                 src (w, h, 1) INT8 or FP32, dst (w, h, 3) same dtype */
int vacv_cvt_color(const vacv_image* src, const vacv_image* dst, int code, void* stream);

/* ---- normalize / statistics ------------------------------------------- */

/* Normalize::normalize (normalize.cpp:84-121, cv.h:104-106):
 *   dst = (float)(((float)x - mean[k]) / ((double)stddev[k] + 1e-6))
 * src INT8 or FP32, dst FP32, same layout.  mean/stddev are HOST arrays of
 * c floats; both NULL = per-image statistics first (exact, see
 * vacv_mean_stddev; src must then be dense).  Exactly one NULL is
 * VACV_ERR_INVALID_ARG.  With host mean/stddev src and dst may be pitched. */
int vacv_normalize(const vacv_image* src, const vacv_image* dst,
                   const float* mean, const float* stddev, void* stream);

/* Per-channel sums for mean_stddev: sums[g*2c + 2k] = Sum x,
 * sums[g*2c + 2k + 1] = Sum x^2 over channel k, g = image (per_image=1) or
 * the whole batch (per_image=0, one group).  DEVICE output, fp64; exact for
 * INT8 input (integer sums), deterministic order for FP32.  These are the
 * partials the multi-GPU path all-reduces over RCCL.  src must be dense (no
 * row, plane or batch padding; VACV_ERR_UNSUPPORTED otherwise) with NHWC
 * c <= 4; any base address works, 16-byte aligned images are faster. */
int vacv_channel_sums(const vacv_image* src, double* sums, int per_image, void* stream);

/* vacv_resize followed by vacv_channel_sums of its output: the statistics
 * half of BASELINE cfg5 (resize + mean_stddev, normalize_naive.cpp:7-72 on
 * the resized image); on several GPUs the sums are what one all-reduce
 * merges.  dst must be dense (VACV_ERR_UNSUPPORTED otherwise, and nothing
 * is written). */
int vacv_resize_channel_sums(const vacv_image* src, const vacv_image* dst, int interpolation, int mode,
                             double* sums, int per_image, void* stream);

/* vacv_resize_channel_sums followed by vacv_stats_from_sums, for one GPU:
 * the resize (cfg5: u8 -> fp32 INTER_CUBIC), the sums[groups][c][2] of its
 * output and the population mean / stddev [groups][c] (groups = n per
 * image, else 1) -- resize_naive.cpp:130-569, then NormalizeNaive::
 * mean_stddev_naive_* (normalize_naive.cpp:7-48) over the image or the whole
 * batch.  On several GPUs use vacv_resize_channel_sums, all-reduce the sums,
 * then vacv_stats_from_sums.  dst must be dense (VACV_ERR_UNSUPPORTED
 * otherwise, and nothing is written). */
int vacv_resize_mean_stddev(const vacv_image* src, const vacv_image* dst, int interpolation, int mode,
                            double* sums, float* mean, float* stddev, int per_image, void* stream);

/* mean = S1/count, stddev = sqrt(max(S2/count - mean^2, 0)) per group and
 * channel, on the device: sums[groups][c][2] -> mean/stddev[groups][c]. */
int vacv_stats_from_sums(const double* sums, int groups, int c, double count,
                         float* mean, float* stddev, void* stream);

/* NormalizeNaive::mean_stddev_naive_* (normalize_naive.cpp:7-72): per-image
 * population mean/stddev, DEVICE outputs [n][c].  Computed exactly (the
 * reference accumulates sequentially in fp32; DESIGN.md quantifies it).
 * src must be dense, as for vacv_channel_sums (VACV_ERR_UNSUPPORTED). */
int vacv_mean_stddev(const vacv_image* src, float* mean, float* stddev, void* stream);

/* ---- fused pipelines -------------------------------------------------- */

/* ResizeNormalize::resize_normalize (resize_normalize.cpp:15-107, cv.h:154):
 * resize, convert to fp32, normalize -- one pass, dst FP32.  Identical to
 * vacv_resize followed by vacv_normalize (u8 resize results are normalized
 * exactly as the reference normalizes a converted u8 tensor).  NULL mean and
 * stddev: per-image statistics of the resized image; with NULL mean and
 * stddev dst must be dense (no row, plane or batch padding) and NHWC dst at
 * most 4 channels, or the call is VACV_ERR_UNSUPPORTED and writes nothing.
 * The same holds for vacv_warp_affine_normalize, vacv_cvt_color_normalize and
 * vacv_cvt_color_resize_normalize. */
int vacv_resize_normalize(const vacv_image* src, const vacv_image* dst, int interpolation, int mode,
                          const float* mean, const float* stddev, void* stream);

/* WarpAffineNormalize::warp_affine_normalize (warp_affine_normalize.cpp,
 * cv.h:172-201): warp then normalize, dst FP32. */
int vacv_warp_affine_normalize(const vacv_image* src, const vacv_image* dst, const float m[6],
                               int flags, int border_mode, const double border_value[4],
                               const float* mean, const float* stddev, void* stream);

/* Many crops in one launch (the detection-pipeline shape of the reference's
 * warp_affine(src, dst, scale, rot, dsize, aux) overload: one small upright
 * crop per detected object, each with its own map).
 * dst image i = warp_affine of src image src_index[i] under the 2x3 map m[i].
 * src: `src->n` frames, NHWC, c = 1..4, INT8 or FP32, pitched or dense, any
 *      base alignment (NCHW: UNSUPPORTED).
 * dst: `dst->n` = number of ROIs, all dst->w x dst->h, dtype and layout of
 *      src; ROIs may be pitched (row and batch pitch).
 * m:         DEVICE array [dst->n][6] float, row-major.  Forward maps, or
 *            dst -> src maps with flags | VACV_WARP_INVERSE_MAP.
 * src_index: DEVICE array [dst->n] int32, or NULL.
 *            NULL needs src->n == 1 (every ROI reads frame 0)
 *            or src->n == dst->n (ROI i reads frame i).
 *            Any other NULL case is VACV_ERR_INVALID_ARG.
 * Both arrays are read by the kernel, on `stream`, at execution time: the
 * call copies nothing between host and device, allocates nothing and never
 * synchronizes, and host code never dereferences them.
 * flags: INTER_LINEAR, optionally | VACV_WARP_INVERSE_MAP (else UNSUPPORTED).
 * border_mode: CONSTANT, REPLICATE, REFLECT, WRAP, REFLECT_101 as
 * vacv_warp_affine defines them (TRANSPARENT: UNSUPPORTED).
 * ROI i is byte-identical to what vacv_warp_affine writes for the single
 * image src[src_index[i]] with the host matrix m[i]; bytes of the dst
 * allocation outside the ROI rectangles are never written.
 * Device-supplied values cannot fault: a src_index[i] outside [0, src->n)
 * gives a ROI filled with border_value (in every border mode) and reads no
 * source byte; a zero-determinant map inverts to all zeros as
 * vacv_invert_affine defines; a non-finite map under BORDER_CONSTANT gives an
 * all-border ROI; every sampler read is range-checked against the indexed
 * frame by the hardware. */
int vacv_warp_affine_rois(const vacv_image* src, const vacv_image* dst, const float* m,
                          const int32_t* src_index, int flags, int border_mode,
                          const double border_value[4], void* stream);
/* The same, normalized: dst is FP32, NHWC or NCHW (planar output for c = 3
 * and c = 1; other channel counts: UNSUPPORTED), pitched or dense (row, plane
 * and batch pitch).  mean / stddev: host arrays of c floats, both required
 * (one NULL: INVALID_ARG; both NULL, per-image statistics: UNSUPPORTED).
 * ROI i is byte-identical to vacv_warp_affine_normalize on that image,
 * followed by vacv_change_layout when dst is NCHW. */
int vacv_warp_affine_rois_normalize(const vacv_image* src, const vacv_image* dst, const float* m,
                                    const int32_t* src_index, int flags, int border_mode,
                                    const double border_value[4],
                                    const float* mean, const float* stddev, void* stream);
/* The same, each ROI standardized by ITS OWN per-channel mean and standard
 * deviation -- the reference's warp_affine_normalize with mean and stddev left
 * empty (warp_affine_normalize.cpp:145-164), the "prewhiten" input of face
 * embedders: align each face with its own similarity map, then whiten the
 * aligned crop -- in ONE kernel launch.  (A function of its own: NULL / NULL
 * of the _rois_normalize entry points stays UNSUPPORTED.)
 * ROI i of dst and row i of mean_out / stddev_out are bit for bit what this
 * chain gives:
 *   1. vacv_warp_affine_rois(src, m, src_index, flags, border_mode,
 *      border_value) into a dense INT8 NHWC batch u = [n][h][w][c]; border
 *      pixels are part of the ROI and count in its statistics, as in the
 *      reference;
 *   2. vacv_mean_stddev(u): exact integer sums S1, S2 per ROI and channel, then
 *      in fp64 m = S1 / (w h), var = max(S2 / (w h) - m m, 0), mean = (float)m,
 *      stddev = (float)sqrt(var);
 *   3. vacv_normalize(u -> FP32, NULL, NULL):
 *      (float)((double)((float)v - mean) / ((double)stddev + 1e-6));
 *   4. vacv_change_layout to NCHW when dst is NCHW.
 * src: `src->n` frames, INT8, NHWC, c = 1..4, pitched or dense, any base
 *      alignment: the INT8 frames vacv_warp_affine_rois takes.  FP32 frames:
 *      UNSUPPORTED (their sums have vacv_channel_sums' summation order, which
 *      another work shape cannot reproduce bit for bit).
 * dst: `dst->n` ROIs of dst->w x dst->h, FP32, NHWC or NCHW (planar output for
 *      c = 3 and c = 1; other channel counts: UNSUPPORTED), pitched or dense
 *      (row, plane and batch pitch), at any 4-byte alignment.  INT8:
 *      INVALID_ARG.
 * m, src_index, flags, border_mode, border_value: exactly the rules of
 *      vacv_warp_affine_rois (m and src_index are DEVICE arrays read by the
 *      kernel, on `stream`, at execution time; NULL m: INVALID_ARG; the same
 *      NULL-index rules; INTER_LINEAR, optionally | VACV_WARP_INVERSE_MAP;
 *      CONSTANT, REPLICATE, REFLECT, WRAP or REFLECT_101, TRANSPARENT:
 *      UNSUPPORTED).
 * mean_out, stddev_out: DEVICE arrays [dst->n][c] float, written by the kernel;
 *      either or both may be NULL, and a NULL array is not written.  The same
 *      non-NULL pointer for both: INVALID_ARG.
 * The call queues one kernel, takes no workspace, copies nothing between host
 * and device, allocates nothing and never synchronizes, and host code never
 * dereferences the four device arrays.  Bytes of the dst allocation outside
 * the ROI rectangles are never written.
 * Device-supplied values cannot fault: a src_index[i] outside [0, src->n)
 * reads no source byte and is the chain's ROI of border_value -- mean = the u8
 * border value per channel, stddev 0, every output +0.0; zero-determinant and
 * non-finite maps behave as vacv_warp_affine_rois documents; every sampler
 * read goes through a buffer resource that spans exactly the indexed frame.
 * VACV_ERR_UNSUPPORTED, with nothing written and before any HIP call:
 *  - a ROI that does not fit one workgroup's 64 KiB of LDS.  The need is
 *      256 + 16 ceil(w h c / 16) + 1024 c bytes
 *    (a head, the u8 ROI and the table of the 256 normalized values per
 *    channel): 144 x 144 x 3 is exactly 64 KiB; 112 x 112 x 3 and
 *    128 x 128 x 3 fit; one channel fits up to 64,256 pixels;
 *  - a frame of 2 GiB or more;
 *  - dst->n > 4,194,303 (a workgroup of 1,024 threads per ROI).
 * Order of the checks: vacv_warp_affine_rois' own, in its order -- descriptors,
 * m, the channel counts, the src_index rule, the source's dtype / layout /
 * channels (INT8 or FP32, NHWC, c <= 4; then FP32: UNSUPPORTED), flags and
 * border_mode, the 2 x 2 source, dst's dtype, the planar channel counts, the
 * frame's size -- then the LDS and grid limits, then mean_out == stddev_out. */
int vacv_warp_affine_rois_standardize(const vacv_image* src, const vacv_image* dst, const float* m,
                                      const int32_t* src_index, int flags, int border_mode,
                                      const double border_value[4],
                                      float* mean_out, float* stddev_out, void* stream);
/* inv[i] = vacv_invert_affine(m[i]) for n maps, bit for bit.  DEVICE in,
 * DEVICE out, queued on `stream`. */
int vacv_invert_affine_device(const float* m, float* inv, int n, void* stream);

/* Many projective crops in one launch: the rectified quadrilaterals of an OCR,
 * plate or document pipeline, each with its own 3x3 map (no counterpart in the
 * reference; OpenCV's warpPerspective shape).
 * dst image i = warp_perspective of src image src_index[i] under h[i].
 * h: DEVICE array [dst->n][9] float, row-major h0..h8, (x, y, 1) -> (X, Y, W).
 *    Forward maps, or dst -> src maps with flags | VACV_WARP_INVERSE_MAP.
 * Everything else -- src, dst, src_index, flags, border_mode, border_value, the
 * order of the checks, what is UNSUPPORTED, and that nothing is copied,
 * allocated or synchronized -- is vacv_warp_affine_rois', with h in m's place.
 * Pixel (x, y) of ROI i: N = vacv_invert_homography(h[i]), or (double)h[i]
 * under VACV_WARP_INVERSE_MAP; in double, each operation rounded separately,
 *   X = (N0*x + N1*y) + N2, Y = (N3*x + N4*y) + N5, W = (N6*x + N7*y) + N8,
 *   r = 1 / W, fx = (float)(X*r), fy = (float)(Y*r)
 * (cv::warpPerspective's coordinates); from (fx, fy) on the pixel is
 * vacv_warp_affine_rois' -- byte for byte the single pixel of a 1 x 1
 * vacv_warp_affine_rois ROI of the same frame under the map [1 0 fx; 0 1 fy]
 * with VACV_WARP_INVERSE_MAP, the same border mode and value.
 * Device-supplied values cannot fault: an index outside [0, src->n) gives a
 * ROI of border_value in every border mode and reads no source byte; a
 * singular forward map inverts to all zeros; W == 0 or non-finite values give
 * +-inf or NaN coordinates, which are border pixels like any far-away point;
 * every sampler read is range-checked against the indexed frame by the
 * hardware. */
int vacv_warp_perspective_rois(const vacv_image* src, const vacv_image* dst, const float* h,
                               const int32_t* src_index, int flags, int border_mode,
                               const double border_value[4], void* stream);
/* The same, normalized: dst, mean and stddev as vacv_warp_affine_rois_normalize
 * takes them (FP32, NHWC or NCHW for c = 3 and c = 1). */
int vacv_warp_perspective_rois_normalize(const vacv_image* src, const vacv_image* dst, const float* h,
                                         const int32_t* src_index, int flags, int border_mode,
                                         const double border_value[4],
                                         const float* mean, const float* stddev, void* stream);
/* The inverse of a homography up to scale, in double: the floats widened, the
 * adjugate (each cofactor p*q - r*s), det = (h0*c0 + h1*c3) + h2*c6, times
 * 1 / det (all zeros for det == 0).  The kernel's own function.  Host only. */
int vacv_invert_homography(const float h[9], double inv_out[9]);
/* cv::getPerspectiveTransform: the homography (h8 = 1) that maps the four
 * points src_quad (x0 y0 .. x3 y3) to dst_quad, solved in double with partial
 * pivoting and stored as floats.  A degenerate quad (three collinear points):
 * VACV_ERR_INVALID_ARG.  Host only. */
int vacv_perspective_transform(const float src_quad[8], const float dst_quad[8], float h_out[9]);

/* Many upright crops in one launch: the reference's crop(src, box) followed
 * by resize(crop, dsize) per detected box (Crop::crop_naive, crop.cpp:128-142,
 * then ResizeNaive::resize_naive_inter_linear_u8 / _fp32), without the crops
 * in between.  Not a scale-and-translate vacv_warp_affine_rois: the resize has
 * half-pixel centres, 11-bit weights and taps clamped at the crop's edge.
 * dst image i = rect rects[i] of src image src_index[i], resized to
 * dst->w x dst->h.
 * src: `src->n` frames, NHWC, c = 1..4, INT8 or FP32, pitched or dense, any
 *      base alignment (NCHW: UNSUPPORTED; smaller than 2 x 2: INVALID_ARG).
 * dst: `dst->n` = number of ROIs, all dst->w x dst->h, dtype and layout of
 *      src; ROIs may be pitched (row and batch pitch).
 * rects:     DEVICE array [dst->n][4] int32 {left, top, width, height},
 *            already truncated as crop_naive truncates a box (crop.cpp:128-131).
 *            NULL: INVALID_ARG.
 * src_index: DEVICE array [dst->n] int32, or NULL, with the NULL rules of
 *            vacv_warp_affine_rois.
 * Both arrays are read by the kernel, on `stream`, at execution time: the
 * call copies nothing between host and device, allocates nothing and never
 * synchronizes, and host code never dereferences them.
 * interpolation: INTER_LINEAR (else UNSUPPORTED).  mode: VACV_LINEAR_* as in
 * vacv_resize (a value outside them: INVALID_ARG); it selects the INT8
 * arithmetic and has no effect on FP32.
 * ROI i is byte-identical to vacv_crop(frame src_index[i], rect i) followed by
 * vacv_resize(..., INTER_LINEAR, mode) to dst->w x dst->h: the taps clamp at
 * the RECT's edges, never the frame's, and a rect of the output's size is the
 * plain crop.  Bytes of the dst allocation outside the ROI rectangles are
 * never written.
 * Device-supplied values cannot fault: a rect with width < 2, height < 2,
 * left < 0, top < 0, left + width > src->w or top + height > src->h (the sums
 * taken without int overflow), or a src_index[i] outside [0, src->n), gives a
 * ROI of zeros and reads no source byte; every other read is range-checked
 * against the indexed frame by the hardware.
 * A destination wider than 2^20 pixels or a frame of 2 GiB or more:
 * UNSUPPORTED. */
int vacv_crop_resize_rois(const vacv_image* src, const vacv_image* dst, const int32_t* rects,
                          const int32_t* src_index, int interpolation, int mode, void* stream);
/* The same, normalized: dst is FP32, NHWC or NCHW (planar output for c = 3
 * and c = 1; other channel counts: UNSUPPORTED), pitched or dense (row, plane
 * and batch pitch).  mean / stddev: host arrays of c floats, both required
 * (one NULL: INVALID_ARG; both NULL, per-image statistics: UNSUPPORTED).
 * ROI i is byte-identical to vacv_crop and vacv_resize_normalize on that
 * rect, followed by vacv_change_layout when dst is NCHW; an invalid rect or
 * index gives the normalized value of 0 in every channel. */
int vacv_crop_resize_rois_normalize(const vacv_image* src, const vacv_image* dst, const int32_t* rects,
                                    const int32_t* src_index, int interpolation, int mode,
                                    const float* mean, const float* stddev, void* stream);
/* The same, each ROI standardized by ITS OWN per-channel mean and standard
 * deviation -- the reference's crop(src, box) then resize_normalize(crop, dst,
 * dsize) with mean and stddev left empty (normalize.cpp:84-121,
 * normalize_naive.cpp:7-72), the "prewhiten" input of face and re-ID
 * embedders -- in ONE kernel launch.  (A function of its own: NULL / NULL of
 * the _rois_normalize entry points stays UNSUPPORTED.)
 * ROI i of dst and row i of mean_out / stddev_out are bit for bit what this
 * chain gives:
 *   1. vacv_crop_resize_rois(src, rects, src_index, INTER_LINEAR, mode) into a
 *      dense INT8 NHWC batch u = [n][h][w][c];
 *   2. vacv_mean_stddev(u): exact integer sums S1, S2 per ROI and channel, then
 *      in fp64 m = S1 / (w h), var = max(S2 / (w h) - m m, 0), mean = (float)m,
 *      stddev = (float)sqrt(var);
 *   3. vacv_normalize(u -> FP32, NULL, NULL):
 *      (float)((double)((float)v - mean) / ((double)stddev + 1e-6));
 *   4. vacv_change_layout to NCHW when dst is NCHW.
 * src: `src->n` frames, INT8, NHWC, c = 1..4, pitched or dense, any base
 *      alignment: the INT8 frames vacv_crop_resize_rois takes.  FP32 frames:
 *      UNSUPPORTED (their sums have vacv_channel_sums' summation order, which
 *      another work shape cannot reproduce bit for bit).
 * dst: `dst->n` ROIs of dst->w x dst->h, FP32, NHWC or NCHW (planar output for
 *      c = 3 and c = 1; other channel counts: UNSUPPORTED), pitched or dense
 *      (row, plane and batch pitch), at any 4-byte alignment.  INT8:
 *      INVALID_ARG.
 * rects, src_index: DEVICE arrays with exactly the rules of
 *      vacv_crop_resize_rois (NULL rects: INVALID_ARG; the same NULL-index
 *      rules), read by the kernel, on `stream`, at execution time.
 * mean_out, stddev_out: DEVICE arrays [dst->n][c] float, written by the kernel;
 *      either or both may be NULL, and a NULL array is not written.  The same
 *      non-NULL pointer for both: INVALID_ARG.
 * interpolation: INTER_LINEAR (else UNSUPPORTED).  mode: VACV_LINEAR_* (a value
 * outside them: INVALID_ARG).
 * The call queues one kernel, takes no workspace, copies nothing between host
 * and device, allocates nothing and never synchronizes, and host code never
 * dereferences the four device arrays.  Bytes of the dst allocation outside
 * the ROI rectangles are never written.
 * Device-supplied values cannot fault: a rect or index that
 * vacv_crop_resize_rois calls invalid reads no source byte and is the chain's
 * ROI of u8 zeros -- mean 0, stddev 0, every output +0.0; every other read is
 * range-checked against the indexed frame by the hardware.
 * VACV_ERR_UNSUPPORTED, with nothing written and before any HIP call:
 *  - a ROI that does not fit one workgroup's 64 KiB of LDS.  The need is
 *      256 + 16 ceil(w h c / 16) + max(8 (w + h), 1024 c) bytes
 *    (a head, the u8 ROI, and the taps of all columns and rows or the table of
 *    the 256 normalized values per channel, which share their bytes):
 *    144 x 144 x 3 is exactly 64 KiB; 112 x 112 x 3 and 128 x 128 x 3 fit;
 *  - a frame of 2 GiB or more;
 *  - dst->n > 4,194,303 (a workgroup of 1,024 threads per ROI).
 * Order of the checks: vacv_crop_resize_rois' own, in its order -- descriptors,
 * rects, the channel counts, the src_index rule, the source's dtype / layout /
 * channels (INT8 or FP32, NHWC, c <= 4; then FP32: UNSUPPORTED), interpolation,
 * mode, the 2 x 2 source, dst's dtype, the planar channel counts -- then these
 * limits, then mean_out == stddev_out. */
int vacv_crop_resize_rois_standardize(const vacv_image* src, const vacv_image* dst, const int32_t* rects,
                                      const int32_t* src_index, int interpolation, int mode,
                                      float* mean_out, float* stddev_out, void* stream);

/* cvt_color then normalize (the cfg3 pipeline), dst (w,h,3) FP32 NHWC. */
int vacv_cvt_color_normalize(const vacv_image* src, const vacv_image* dst, int code,
                             const float* mean, const float* stddev, void* stream);

/* Camera frame -> model input in ONE pass: YUV420sp
 * decode, u8 bilinear resize, and optionally convert + normalize, with NHWC
 * or NCHW (planar, the model-input layout) output.  Bit-identical to the
 * reference's chain
 *   CvtColor::cvt_color (cvt_color.cpp:39-157)
 *   -> Resize::resize INTER_LINEAR u8 (resize_naive.cpp:10-68; `mode` as in
 *      vacv_resize)
 *   -> Tensor::change_dtype FP32 + Normalize::normalize
 *      (tensor.cpp:459-502, normalize_naive.cpp:74-90)
 *   -> Tensor::change_layout(NCHW) (tensor.cpp:393-457)
 * without materialising the decoded frame.  src = (w, h*3/2, 1) INT8, w and
 * h even, w >= 4; dst = (wo, ho, 3), any wo/ho >= 1, NHWC or NCHW.
 * interpolation must be INTER_LINEAR.
 *  vacv_cvt_color_resize:           dst INT8 (u8 BGR/RGB) or FP32 (widened)
 *  vacv_cvt_color_resize_normalize: dst FP32; NULL mean and stddev = per-image
 *                                   statistics of the resized image; with NULL
 *                                   mean and stddev dst must be dense
 *                                   (VACV_ERR_UNSUPPORTED otherwise, nothing
 *                                   written). */
int vacv_cvt_color_resize(const vacv_image* src, const vacv_image* dst, int code, int interpolation,
                          int mode, void* stream);
int vacv_cvt_color_resize_normalize(const vacv_image* src, const vacv_image* dst, int code, int interpolation,
                                    int mode, const float* mean, const float* stddev, void* stream);

/* The second stage of that pipeline: many crops straight from NV21 / NV12
 * frames in one launch, without materialising the decoded frames.
 * src: `src->n` YUV420sp frames as vacv_cvt_color takes them, (w, h*3/2, 1)
 *      INT8, w and h even (>= 2), pitched (row and batch pitch) or dense, any
 *      base alignment.
 * code: VACV_COLOR_YUV2{BGR,RGB}_{NV21,NV12}; the codes of OpenCV's
 *      arithmetic (RGBA/BGRA, YV12, GRAY2BGR): UNSUPPORTED.
 * dst: `dst->n` ROIs of dst->w x dst->h, c = 3.
 *      vacv_cvt_color_warp_affine_rois:           INT8 NHWC, dense or pitched
 *      vacv_cvt_color_warp_affine_rois_normalize: FP32, NHWC or NCHW, dense or
 *        pitched (row, plane and batch pitch); mean / stddev: host arrays of 3
 *        floats, both required (one NULL: INVALID_ARG; both NULL: UNSUPPORTED).
 * m, src_index, flags, border_mode: exactly as vacv_warp_affine_rois (DEVICE
 * arrays read by the kernel at execution time, never dereferenced by the
 * host; the same NULL-index rules; INTER_LINEAR [| VACV_WARP_INVERSE_MAP];
 * TRANSPARENT: UNSUPPORTED).  border_value[0..2] are in the decoded channel
 * order.
 * ROI i is byte-identical to vacv_cvt_color(frame src_index[i], code)
 * followed by vacv_warp_affine_rois[_normalize] on that decoded (w, h, 3)
 * frame with m[i]; bytes of the dst allocation outside the ROI rectangles
 * are never written.  The call copies nothing between host and device,
 * allocates nothing and never synchronizes.  Device-supplied values cannot
 * fault: every source read is range-checked by the hardware against the
 * indexed frame's Y and chroma rows, and an index outside [0, src->n) gives
 * a ROI of border_value in every border mode. */
int vacv_cvt_color_warp_affine_rois(const vacv_image* src, const vacv_image* dst, int code,
                                    const float* m, const int32_t* src_index, int flags, int border_mode,
                                    const double border_value[4], void* stream);
int vacv_cvt_color_warp_affine_rois_normalize(const vacv_image* src, const vacv_image* dst, int code,
                                    const float* m, const int32_t* src_index, int flags, int border_mode,
                                    const double border_value[4],
                                    const float* mean, const float* stddev, void* stream);

/* The same second stage for upright boxes: many crop + resize ROIs straight
 * from NV21 / NV12 frames in one launch, without the decoded frames and
 * without the crops.
 * src, code: exactly as vacv_cvt_color_warp_affine_rois.
 * dst: `dst->n` ROIs of dst->w x dst->h, c = 3.
 *      vacv_cvt_color_crop_resize_rois:           INT8 NHWC, dense or pitched
 *      vacv_cvt_color_crop_resize_rois_normalize: FP32, NHWC or NCHW, dense or
 *        pitched (row, plane and batch pitch); mean / stddev: host arrays of 3
 *        floats, both required (one NULL: INVALID_ARG; both NULL: UNSUPPORTED).
 * rects, src_index, interpolation, mode: exactly as vacv_crop_resize_rois
 * (DEVICE arrays read by the kernel at execution time, never dereferenced by
 * the host; the same NULL-index rules; INTER_LINEAR only; mode
 * VACV_LINEAR_REFERENCE / _NEON / _OPENCV).  A rect is (left, top, width,
 * height) in the DECODED w x h frame.
 * ROI i is byte-identical to vacv_cvt_color(frame src_index[i], code)
 * followed by vacv_crop_resize_rois[_normalize] on that decoded (w, h, 3)
 * frame with rects[i]; bytes of the dst allocation outside the ROI rectangles
 * are never written.  The call copies nothing between host and device,
 * allocates nothing and never synchronizes.  Device-supplied values cannot
 * fault: an index outside [0, src->n), a width or height below 2, a negative
 * origin or an edge past the decoded frame gives a ROI of zeros (normalize:
 * the normalized value of 0) and reads nothing; every source read is
 * range-checked by the hardware against the indexed frame's Y and chroma
 * rows.  A destination wider than 2^20 pixels or a frame of 2 GiB or more:
 * UNSUPPORTED. */
int vacv_cvt_color_crop_resize_rois(const vacv_image* src, const vacv_image* dst, int code,
                                    const int32_t* rects, const int32_t* src_index,
                                    int interpolation, int mode, void* stream);
int vacv_cvt_color_crop_resize_rois_normalize(const vacv_image* src, const vacv_image* dst, int code,
                                    const int32_t* rects, const int32_t* src_index,
                                    int interpolation, int mode,
                                    const float* mean, const float* stddev, void* stream);

/* The two standardize calls straight from NV21 / NV12 frames: each ROI
 * normalized by ITS OWN per-channel mean and standard deviation, in ONE kernel
 * launch, without the decoded frames, the u8 crops or a statistics pass.
 * ROI i of dst and row i of mean_out / stddev_out are bit for bit what this
 * chain gives:
 *   1. vacv_cvt_color(frame src_index[i], code) into a (w, h, 3) INT8 frame;
 *   2. vacv_crop_resize_rois_standardize (rects[i], interpolation, mode), or
 *      vacv_warp_affine_rois_standardize (m[i], flags, border_mode,
 *      border_value), on the decoded frames.
 * src, code: exactly as vacv_cvt_color_warp_affine_rois.
 * dst: `dst->n` ROIs of dst->w x dst->h, c = 3, FP32, NHWC or NCHW, pitched or
 *      dense (row, plane and batch pitch), at any 4-byte alignment.  INT8:
 *      INVALID_ARG.
 * rects, src_index, interpolation, mode: exactly as
 *      vacv_cvt_color_crop_resize_rois; m, src_index, flags, border_mode,
 *      border_value: exactly as vacv_cvt_color_warp_affine_rois.  DEVICE arrays
 *      read by the kernel, on `stream`, at execution time.
 * mean_out, stddev_out: DEVICE arrays [dst->n][3] float, written by the kernel;
 *      either or both may be NULL, and a NULL array is not written.  The same
 *      non-NULL pointer for both: INVALID_ARG.
 * The call queues one kernel, takes no workspace, copies nothing between host
 * and device, allocates nothing and never synchronizes, and host code never
 * dereferences the four device arrays.  Bytes of the dst allocation outside
 * the ROI rectangles are never written.
 * Device-supplied values cannot fault: every source read is range-checked by
 * the hardware against the indexed frame's Y and chroma rows.  crop_resize: an
 * index outside [0, src->n), a width or height below 2, a negative origin or
 * an edge past the decoded frame reads no source byte and is the chain's ROI
 * of u8 zeros -- mean 0, stddev 0, every output +0.0.  warp_affine: an index
 * outside [0, src->n) reads no source byte and is the chain's ROI of
 * border_value -- mean = the u8 border value per channel, stddev 0, every
 * output +0.0; zero-determinant and non-finite maps behave as
 * vacv_warp_affine_rois documents.
 * VACV_ERR_UNSUPPORTED, with nothing written and before any HIP call:
 *  - a ROI that does not fit one workgroup's 64 KiB of LDS.  The need is
 *      crop_resize: 256 + 16 ceil(3 w h / 16) + max(8 (w + h), 3072) bytes
 *      warp_affine: 256 + 16 ceil(3 w h / 16) + 3072 bytes
 *    (the formulas of the two _rois_standardize calls at c = 3): 144 x 144 is
 *    exactly 64 KiB; 112 x 112 and 128 x 128 fit;
 *  - a frame (Y and chroma rows) of 2 GiB or more;
 *  - dst->n > 4,194,303 (a workgroup of 1,024 threads per ROI).
 * Order of the checks: those of vacv_cvt_color_crop_resize_rois /
 * vacv_cvt_color_warp_affine_rois, in their order -- descriptors, rects / m,
 * the code, the source's dtype / channels / layout, the YUV420sp shape, dst's
 * channels, the src_index rule, interpolation then mode / flags and
 * border_mode, dst's dtype -- then these limits, then mean_out == stddev_out. */
int vacv_cvt_color_crop_resize_rois_standardize(const vacv_image* src, const vacv_image* dst, int code,
                                    const int32_t* rects, const int32_t* src_index,
                                    int interpolation, int mode,
                                    float* mean_out, float* stddev_out, void* stream);
int vacv_cvt_color_warp_affine_rois_standardize(const vacv_image* src, const vacv_image* dst, int code,
                                    const float* m, const int32_t* src_index, int flags, int border_mode,
                                    const double border_value[4],
                                    float* mean_out, float* stddev_out, void* stream);

/* ---- template matching ------------------------------------------------ */

/* va_cv::VMatchMode (cv.h:52-59) */
enum {
    VACV_TM_SQDIFF = 0, VACV_TM_SQDIFF_NORMED = 1, VACV_TM_CCORR = 2, VACV_TM_CCORR_NORMED = 3,
    VACV_TM_CCOEFF = 4, VACV_TM_CCOEFF_NORMED = 5
};

/* MatchTemplate::match_template (match_template.cpp:13-41, cv.h:211-219),
 * which the reference hands to cv::matchTemplate: OpenCV 2.4's algorithm
 * with the correlation computed exactly (parity unpinned).
 * img: n images (W, H, c) NHWC INT8 or FP32, c <= 4; templ: (w, h, c), same
 * dtype, n = 1, shared by every image; result: n x (W-w+1, H-h+1, 1) FP32.
 * A template at least as large as the image in both dimensions and larger
 * in one (w >= W && h >= H && (w > W || h > H)) swaps the two, as
 * cv::matchTemplate does (n = 1 only).  VACV_ERR_UNSUPPORTED, with nothing
 * written, when the template does not fit the kernel's LDS budget (about
 * 64 KiB of template bytes), for more than 65535 * 4 result rows, or when
 * ceil((W-w+1) / 256) * (H-h+1) does not fit an int. */
int vacv_match_template(const vacv_image* img, const vacv_image* templ, const vacv_image* result, int method,
                        void* stream);

/* MatchTemplate::minMaxIdx (match_template.cpp:43-46) = cv::minMaxIdx of a
 * single-channel 2-D array (n = 1, c = 1, INT8 or FP32): the first
 * (row-major) minimum and maximum among the elements whose mask byte is
 * non-zero (mask: NULL, or (w, h, 1) INT8).  DEVICE outputs: vals[2] = {min,
 * max}, idx[4] = {min row, min col, max row, max col}; with no element 0, 0
 * and -1s.  NaNs are never selected. */
int vacv_min_max_idx(const vacv_image* src, const vacv_image* mask, double* vals, int* idx, void* stream);

/* A tracker's step in one launch: many templates matched in per-object search
 * windows, with each result's peaks -- vacv_crop + vacv_match_template +
 * vacv_min_max_idx per object, without the crops and in ONE kernel launch.
 * INT8 only: FP32 is VACV_ERR_UNSUPPORTED (its window sums are order-dependent
 * doubles and need a design of their own).
 * src:    `src->n` frames, NHWC, INT8, c = 1..4, pitched (row and batch pitch)
 *         or dense, any base alignment (NCHW: UNSUPPORTED).
 * templ:  (tw, th, c) INT8 NHWC, pitched or dense.  templ->n == 1: one
 *         template for every ROI; templ->n == result->n: template i for ROI i;
 *         any other count: INVALID_ARG.
 * result: `result->n` ROIs of (rw, rh, 1) FP32, pitched or dense.  Every
 *         search window is W x H with W = rw + tw - 1, H = rh + th - 1.  There
 *         is no template / image swap.
 * origin:    DEVICE array [result->n][2] int32 {left, top} of each search
 *            window in its frame.  NULL: INVALID_ARG.
 * src_index: DEVICE array [result->n] int32, or NULL, with the NULL rules of
 *            vacv_warp_affine_rois.
 * vals:      DEVICE array [result->n][2] double {min, max}
 * idx:       DEVICE array [result->n][4] int32 {min row, min col, max row,
 *            max col}; vals and idx both given, or both NULL (only the maps
 *            are written); one NULL: INVALID_ARG.
 * method: VACV_TM_* (else UNSUPPORTED).
 * All four arrays are used by the kernel, on `stream`, at execution time: the
 * call queues one kernel, takes no workspace, copies nothing between host and
 * device, never synchronizes, and host code never dereferences them.
 * ROI i is byte-identical to vacv_match_template on the W x H vacv_crop at
 * origin[i] of frame src_index[i] with template i; vals[i] / idx[i] are
 * identical to vacv_min_max_idx (no mask) of that result.  Bytes of the result
 * allocation outside the ROI rectangles are never written.
 * Device-supplied values cannot fault: a window with left < 0, top < 0,
 * left + W > src->w or top + H > src->h (the sums taken without int overflow),
 * or a src_index[i] outside [0, src->n), gives a result of zeros, vals {0, 0}
 * and idx {-1, -1, -1, -1} (vacv_min_max_idx's "no element") and reads no
 * source byte; every other source read lies inside the validated window.
 * VACV_ERR_UNSUPPORTED, with nothing written:
 *  - tw * th > 66000 (the uint32 window sums' bound of vacv_match_template);
 *  - a ROI that does not fit one workgroup's 64 KiB of LDS.  With
 *    K4 = ceil(tw c / 4), G = ceil(rw / 4),
 *    WS4 = max(ceil(W c / 4), (G - 1) c + K4 + floor(3 c / 4) + 2) | 1, the need is
 *      256 + 4 (th K4 + H WS4 + H rw (c + 1)) bytes
 *    (the template, the window, the window rows' horizontal sums);
 *  - result->n > 16,777,215 (a workgroup per ROI).
 * Order of the checks: descriptors and origin, then method / dtype / layout,
 * then shapes, then these limits, then the vals / idx and src_index rules. */
int vacv_match_template_rois(const vacv_image* src, const vacv_image* templ, const vacv_image* result,
                             const int32_t* origin, const int32_t* src_index, int method,
                             double* vals, int32_t* idx, void* stream);

/* The same step straight from NV21 / NV12 camera frames: ROI i of the result,
 * vals[i] and idx[i] are bit for bit what vacv_cvt_color(src, code) into
 * (w, h, 3) INT8 frames followed by vacv_match_template_rois on those frames
 * produces, in ONE kernel launch and without the decoded frames ever
 * existing.  (Grey tracking needs no call of its own: describe the Y plane as
 * c = 1 frames with the YUV row and batch pitch for vacv_match_template_rois.)
 * src, code: exactly as vacv_cvt_color_warp_affine_rois -- `src->n` frames
 *         (w, h * 3 / 2, 1) INT8 with w and h even and >= 2 (else
 *         INVALID_ARG), pitched or dense, any base alignment; code one of
 *         VACV_COLOR_YUV2{BGR,RGB}_NV{21,12} (every other code, the
 *         OpenCV-arithmetic ones included: UNSUPPORTED).
 * templ:  (tw, th, 3) INT8 NHWC in the decoded channel order of `code`,
 *         pitched or dense; templ->n == 1 or templ->n == result->n (else
 *         INVALID_ARG); c != 3 or another dtype: INVALID_ARG; NCHW: UNSUPPORTED.
 * result, origin, src_index, method, vals, idx: exactly as
 *         vacv_match_template_rois.  A window {left, top} is given in the
 *         DECODED w x h frame.
 * The call queues one kernel on `stream`, takes no workspace, copies nothing
 * between host and device, never synchronizes, and host code never
 * dereferences the four device arrays.  Bytes of the result allocation outside
 * the ROI rectangles are never written.
 * Device-supplied values cannot fault: a window with left < 0, top < 0,
 * left + W > w or top + H > h (the decoded size; the sums taken without int
 * overflow), or a src_index[i] outside [0, src->n), gives a result of zeros,
 * vals {0, 0} and idx {-1, -1, -1, -1} and reads no source byte.  A valid
 * window reads only bytes of its own Y rows, columns left .. left + W - 1, and
 * of chroma rows h + (top >> 1) .. h + ((top + H - 1) >> 1), columns
 * left & ~1 .. (left + W - 1) | 1: never a byte past a dense frame's last
 * chroma pair.
 * VACV_ERR_UNSUPPORTED, with nothing written: tw * th > 66000; a ROI whose
 * need of LDS, vacv_match_template_rois's formula with c = 3, passes 64 KiB
 * (the decode adds none); result->n > 16,777,215.
 * Order of the checks: descriptors and origin; then code, method, the
 * source's dtype / channels / layout and the template's layout; then shapes
 * (the YUV size, the template's dtype / channels / count, the result); then
 * these limits; then the vals / idx and src_index rules. */
int vacv_cvt_color_match_template_rois(const vacv_image* src, const vacv_image* templ, const vacv_image* result,
                                       int code, const int32_t* origin, const int32_t* src_index, int method,
                                       double* vals, int32_t* idx, void* stream);

/* ---- runtime ---------------------------------------------------------- */

/* Kernel-variant knobs, for A/B measurement and the parity tests that check
 * every variant against the same oracle; normal callers never need them.
 * Each starts from the environment variable of the same name (read once,
 * when the library loads), else -1 = the built-in choice. */
enum {
    VACV_TUNE_RESIZE_DIRECT = 0,     /* u8 bilinear: 0 staged, 1 gather kernel for one-tap rows, 2 gather always, 3 as 1 without the NV21 resize's point-sampling instance (A/B) */
    VACV_TUNE_CUBIC_DIRECT = 1,      /* u8 cubic: 0 staged kernel, else the gather kernel */
    VACV_TUNE_RESIZE_INTERLEAVE = 2, /* staged kernel: 0 strip order, else address-ordered tasks */
    VACV_TUNE_DIRECT_XCD = 3,        /* gather kernel block order: 0 plain, 1 XCD-contiguous */
    VACV_TUNE_WARP_PX = 4,           /* warp gather kernel: lane blocks per wave (4, 5, 8, 10) */
    VACV_TUNE_NEAREST_KERNEL = 5,    /* INTER_NEAREST: 0 per-pixel kernel, 1 row per workgroup, else row per wave (when they apply) */
    VACV_TUNE_AREA_KERNEL = 6,       /* u8 INTER_AREA: 1 per-pixel kernel, 2 dword column sums */
    VACV_TUNE_AREA_ROWS = 7,         /* u8 INTER_AREA column sums: output rows per workgroup */
    VACV_TUNE_RESIZE_WGS = 8,        /* staged kernel: workgroups launched */
    VACV_TUNE_RESIZE_TILE_H = 9,     /* staged kernel planner: tile height */
    VACV_TUNE_RESIZE_TILE_W = 10,    /* staged kernel planner: tile width; column kernel (resize_cols_kernel): 64 / 128 output columns per wave */
    VACV_TUNE_RESIZE_WORK = 11,      /* staged kernel planner: work per thread */
    VACV_TUNE_WARP_KERNEL = 12,      /* u8 CONSTANT warp: 0 per-pixel gathers, 2 batched gathers, 4 LDS-staged frames: an LDS-DMA ring of source boxes (k_warp_frames.hip; 3 channels re-laid as 4-byte pixels, warp_exp_kernel), 6 the same without the re-lay (warp_ring_kernel, A/B); 5: INTER_NEAREST u8 on the per-pixel kernel (A/B) */
    VACV_TUNE_RESIZE_STRIP = 13,     /* two-tap u8 bilinear: column strips with an LDS row ring, 1: 64 columns x 16-row batches, 2 (default): 128 x 8; 0 staged kernel */
    VACV_TUNE_MATCH_KERNEL = 14,     /* u8 match_template correlation: 0 v_dot4 kernel, else i8 MFMA where it fits */
    VACV_TUNE_WARP_FRAMES = 15,      /* u8 CONSTANT warp, LDS-staged kernel: frames per workgroup */
    VACV_TUNE_WARP_TILE_H = 16,      /* u8 CONSTANT warp, LDS-staged kernel: tile rows (16 or 32) */
    VACV_TUNE_WARP_SLOTS = 17,       /* u8 CONSTANT warp, LDS-staged kernel: source boxes in the LDS ring (2-4) */
    VACV_TUNE_LANCZOS_KERNEL = 18,   /* u8 INTER_LANCZOS4: 0 register-ring kernel (staged runs where they fit), 1 the LDS-ring kernel, 2 the register ring with per-lane windows (A/B) */
    VACV_TUNE_COUNT = 19
};
/* value < 0 restores the built-in choice.  Returns VACV_OK or INVALID_ARG. */
int vacv_set_tuning(int key, int value);
/* the current value (-1 = built-in), or VACV_ERR_INVALID_ARG for a bad key */
int vacv_get_tuning(int key);

/* Block until all work this library queued on `stream` has finished. */
int vacv_stream_synchronize(void* stream);
/* Release the per-device workspace the statistics paths cache. */
int vacv_release_workspace(void);

#ifdef __cplusplus
}
#endif
#endif /* VACV_HIP_H */
