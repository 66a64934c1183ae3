// va_cv:: over the C ABI (include/vacv_hip.h).  Each function reproduces the
// reference operator's output-tensor contract (shape, dtype, layout via
// dst.create) and hands the pixel work to the HIP kernels; detail::Staging
// moves host operands across PCIe and leaves device operands in HBM.
#include "cv.h"

#include <cmath>
#include <cstring>
#include <vector>

#include "../common/hip_context.h"

namespace va_cv {

using namespace vision;
using detail::fail;
using detail::Staging;

namespace {

// Small host-side parameter vectors (mean / stddev / M) read from a Tensor of
// FP32 values, wherever it lives.
std::vector<float> host_floats(const char* fn, const Tensor& t, size_t want) {
    if (t.dtype != FP32) fail(fn, "parameter tensors must be FP32");
    if (t.size() != want) fail(fn, "parameter tensor has the wrong number of values");
    const Tensor h = t.to_host();
    std::vector<float> v(want);
    std::memcpy(v.data(), h.data, want * sizeof(float));
    return v;
}

// mean / stddev: (nullptr, nullptr) = per-image statistics.  `either_empty`
// picks the rule of resize_normalize_opencv (resize_normalize.cpp:58: either
// empty -> computed); otherwise both must be empty (normalize.cpp:98).
struct Stats {
    std::vector<float> mean, stdv;
    const float* m() const { return mean.empty() ? nullptr : mean.data(); }
    const float* s() const { return stdv.empty() ? nullptr : stdv.data(); }
};

Stats read_stats(const char* fn, const Tensor& mean, const Tensor& stddev, int c, bool either_empty) {
    Stats st;
    const bool me = mean.empty(), se = stddev.empty();
    if (me && se) return st;
    if (me || se) {
        if (either_empty) return st;
        fail(fn, "mean and stddev must both be given or both be empty");
    }
    // resize_normalize.cpp:82-84 / normalize.cpp: one value per channel
    if ((int)mean.size() != c || (int)stddev.size() != c)
        fail(fn, "The input mean or stddev channels is not matched with tensor dims");
    st.mean = host_floats(fn, mean, c);
    st.stdv = host_floats(fn, stddev, c);
    return st;
}

DType resize_out_dtype(const char* fn, const Tensor& src, int interpolation) {
    if (interpolation == INTER_LINEAR) {
        if (src.dtype != INT8 && src.dtype != FP32) fail(fn, "INTER_LINEAR takes INT8 or FP32");
        return src.dtype;
    }
    if (interpolation == INTER_CUBIC) {
        if (src.dtype != INT8 && src.dtype != FP32) fail(fn, "INTER_CUBIC takes INT8 or FP32");
        return FP32;  // INT8 cubic = fused widen to FP32 (reference: infinite recursion)
    }
    if (interpolation == INTER_NEAREST) {
        // resize.cpp:46-49 hands it to cv::resize; OpenCV 2.4's resizeNN here
        if (src.dtype != INT8 && src.dtype != FP32) fail(fn, "INTER_NEAREST takes INT8 or FP32");
        return src.dtype;
    }
    if (interpolation == INTER_AREA) {
        // resize.cpp:46-49 hands it to cv::resize; OpenCV 2.4's area resize
        // at every scale (resizeAreaFast_, resizeArea_, area-mode bilinear)
        if (src.dtype != INT8 && src.dtype != FP32) fail(fn, "INTER_AREA takes INT8 or FP32");
        return src.dtype;
    }
    if (interpolation == INTER_LANCZOS4) {
        // resize.cpp:46-49 hands it to cv::resize; OpenCV 2.4's 8x8 Lanczos here
        if (src.dtype != INT8 && src.dtype != FP32) fail(fn, "INTER_LANCZOS4 takes INT8 or FP32");
        return src.dtype;
    }
    // every other mode goes to OpenCV in the reference, which this build
    // does not ship (the reference without OpenCV recurses forever)
    fail(fn, "only INTER_NEAREST, INTER_LINEAR, INTER_CUBIC, INTER_AREA and INTER_LANCZOS4 are supported");
}

std::vector<float> affine_of(const char* fn, const Tensor& M) { return host_floats(fn, M, 6); }

void check_warp_modes(const char* fn, const Tensor& src, int flags, int borderMode) {
    // warp_affine.cpp:114-118
    if (src.dtype != INT8 && src.dtype != FP32) fail(fn, "warp_affine takes INT8 or FP32");
    // INTER_LINEAR / INTER_NEAREST, optionally | WARP_INVERSE_MAP (the
    // reference hands all but INTER_LINEAR to cv::warpAffine; OpenCV 2.4's
    // semantics here, vacv_hip.h)
    const int interp = flags & INTER_MAX;
    if ((flags & ~(INTER_MAX | WARP_INVERSE_MAP)) || (interp != INTER_LINEAR && interp != INTER_NEAREST))
        fail(fn, "only INTER_LINEAR and INTER_NEAREST (optionally | WARP_INVERSE_MAP) are supported");
    // BORDER_CONSTANT is the reference's naive path; REPLICATE, REFLECT, WRAP,
    // REFLECT_101 and TRANSPARENT extend it (the reference hands them to
    // OpenCV: warp_affine.cpp:114-118); BORDER_ISOLATED has no meaning here
    if (borderMode < BORDER_CONSTANT || borderMode > BORDER_TRANSPARENT)
        fail(fn, "unsupported border mode");
}

std::vector<float> rotation(float scale, float rot, const VScalar& aux) {
    const double a[4] = {aux.v0, aux.v1, aux.v2, aux.v3};
    std::vector<float> m(6);
    detail::check("va_cv::warp_affine", vacv_rotation_matrix(scale, rot, a, m.data()));
    return m;
}

void warp_into(const char* fn, const Tensor& src, Tensor& dst, const float* m, VSize dsize, int flags,
               int borderMode, const VScalar& bv, bool normalize, const Stats* stats) {
    check_warp_modes(fn, src, flags, borderMode);
    if (dsize.w < 1 || dsize.h < 1) fail(fn, "dsize must be positive");
    const double border[4] = {bv.v0, bv.v1, bv.v2, bv.v3};
    Staging st(fn, src);
    const vacv_image s = st.in(src, 0);
    // BORDER_TRANSPARENT keeps dst's bytes where the sampler has no taps
    const vacv_image d = st.out(dst, dsize.w, dsize.h, src.c, normalize ? FP32 : src.dtype, src.layout, 1,
                                borderMode == BORDER_TRANSPARENT);
    if (normalize) {
        st.run(vacv_warp_affine_normalize(&s, &d, m, flags, borderMode, border, stats->m(), stats->s(),
                                          st.stream()));
    } else {
        st.run(vacv_warp_affine(&s, &d, m, flags, borderMode, border, st.stream()));
    }
    st.finish();
}

int yuv_rows(const char* fn, const Tensor& src) {
    if (src.dtype != INT8 || src.c != 1) fail(fn, "YUV420sp input must be a (w, h*3/2, 1) INT8 tensor");
    return src.h / 3 * 2;  // cvt_color.cpp:152
}

void check_yuv_code(const char* fn, int code) {
    if (code != COLOR_YUV2BGR_NV21 && code != COLOR_YUV2RGB_NV21 && code != COLOR_YUV2BGR_NV12 &&
        code != COLOR_YUV2RGB_NV12)
        fail(fn, "unsupported colour conversion code");
}

}  // namespace

void resize(const Tensor& src, Tensor& dst, VSize dsize, double fx, double fy, int interpolation) {
    static const char* fn = "va_cv::resize";
    const DType out = resize_out_dtype(fn, src, interpolation);
    // INTER_NEAREST / INTER_AREA go to cv::resize in the reference, which also
    // takes dsize = 0 with fx, fy: dsize = saturate_cast<int>(w * fx) (round
    // half to even) and inv_scale = fx, fy.  The naive LINEAR / CUBIC paths
    // use dsize alone (resize.cpp:77-135).
    const bool scaled = dsize.w == 0 && dsize.h == 0 && fx > 0 && fy > 0 &&
                        (interpolation == INTER_NEAREST || interpolation == INTER_AREA || interpolation == INTER_LANCZOS4);
    if (scaled) {
        dsize.w = static_cast<int>(std::nearbyint(src.w * fx));
        dsize.h = static_cast<int>(std::nearbyint(src.h * fy));
    }
    if (dsize.w < 1 || dsize.h < 1) fail(fn, "dsize must be positive");
    Staging st(fn, src);
    const vacv_image s = st.in(src, 0);
    const vacv_image d = st.out(dst, dsize.w, dsize.h, src.c, out, src.layout, 1);
    if (scaled) st.run(vacv_resize_scaled(&s, &d, interpolation, VACV_LINEAR_REFERENCE, fx, fy, st.stream()));
    else st.run(vacv_resize(&s, &d, interpolation, VACV_LINEAR_REFERENCE, st.stream()));
    st.finish();
}

void cvt_color(const Tensor& src, Tensor& dst, int code) {
    static const char* fn = "va_cv::cvt_color";
    // the codes the reference hands to cv::cvtColor (cvt_color.cpp:139-141),
    // with OpenCV 2.4's arithmetic: GRAY2BGR, YUV420 -> RGBA/BGRA, YV12
    if (code == COLOR_GRAY2BGR) {
        if ((src.dtype != INT8 && src.dtype != FP32) || src.c != 1 || src.layout != NHWC)
            fail(fn, "COLOR_GRAY2BGR takes a (w, h, 1) INT8 or FP32 NHWC tensor");
        Staging st(fn, src);
        const vacv_image s = st.in(src, 0);
        const vacv_image d = st.out(dst, src.w, src.h, 3, src.dtype, NHWC, 1);
        st.run(vacv_cvt_color(&s, &d, code, st.stream()));
        st.finish();
        return;
    }
    const bool cv4 = code == COLOR_YUV2RGBA_NV12 || code == COLOR_YUV2BGRA_NV12 || code == COLOR_YUV2RGBA_NV21 ||
                     code == COLOR_YUV2BGRA_NV21;
    if (!cv4 && code != COLOR_YUV2BGR_YV12) check_yuv_code(fn, code);
    const int h = yuv_rows(fn, src);
    Staging st(fn, src);
    const vacv_image s = st.in(src, 0);
    const vacv_image d = st.out(dst, src.w, h, cv4 ? 4 : 3, INT8, NHWC, 1);
    st.run(vacv_cvt_color(&s, &d, code, st.stream()));
    st.finish();
}

void cvt_color_normalize(const Tensor& src, Tensor& dst, int code, const Tensor& mean, const Tensor& stddev) {
    static const char* fn = "va_cv::cvt_color_normalize";
    check_yuv_code(fn, code);
    const int h = yuv_rows(fn, src);
    const Stats stats = read_stats(fn, mean, stddev, 3, false);
    Staging st(fn, src);
    const vacv_image s = st.in(src, 0);
    const vacv_image d = st.out(dst, src.w, h, 3, FP32, NHWC, 1);
    st.run(vacv_cvt_color_normalize(&s, &d, code, stats.m(), stats.s(), st.stream()));
    st.finish();
}

void normalize(const Tensor& src, Tensor& dst, const Tensor& mean, const Tensor& stddev) {
    static const char* fn = "va_cv::normalize";
    if (src.dtype != INT8 && src.dtype != FP32) fail(fn, "normalize takes INT8 or FP32");
    const Stats stats = read_stats(fn, mean, stddev, src.c, false);
    Staging st(fn, src);
    const vacv_image s = st.in(src, 0);
    const vacv_image d = st.out(dst, src.w, src.h, src.c, FP32, src.layout, 1);
    st.run(vacv_normalize(&s, &d, stats.m(), stats.s(), st.stream()));
    st.finish();
}

void mean_stddev(const Tensor& src, Tensor& mean, Tensor& stddev) {
    static const char* fn = "va_cv::mean_stddev";
    if (src.dtype != INT8 && src.dtype != FP32) fail(fn, "mean_stddev takes INT8 or FP32");
    Staging st(fn, src);
    const vacv_image s = st.in(src, 0);
    const vacv_image m = st.out(mean, src.c, 1, 1, FP32, NCHW, 1);
    const vacv_image d = st.out(stddev, src.c, 1, 1, FP32, NCHW, 2);
    st.run(vacv_mean_stddev(&s, static_cast<float*>(m.data), static_cast<float*>(d.data), st.stream()));
    st.finish();
}

void warp_affine(const Tensor& src, Tensor& dst, const Tensor& M, VSize dsize, int flags, int borderMode,
                 const VScalar& borderValue) {
    static const char* fn = "va_cv::warp_affine";
    const std::vector<float> m = affine_of(fn, M);
    warp_into(fn, src, dst, m.data(), dsize, flags, borderMode, borderValue, false, nullptr);
}

void warp_affine(const Tensor& src, Tensor& dst, float scale, float rot, VSize dsize, const VScalar& aux_param,
                 int flags, int borderMode, const VScalar& borderValue) {
    static const char* fn = "va_cv::warp_affine";
    const std::vector<float> m = rotation(scale, rot, aux_param);
    warp_into(fn, src, dst, m.data(), dsize, flags, borderMode, borderValue, false, nullptr);
}

void resize_normalize(const Tensor& src, Tensor& dst, VSize dsize, double /*fx*/, double /*fy*/, int interpolation,
                      const Tensor& mean, const Tensor& stddev) {
    static const char* fn = "va_cv::resize_normalize";
    (void)resize_out_dtype(fn, src, interpolation);
    if (dsize.w < 1 || dsize.h < 1) fail(fn, "dsize must be positive");
    const Stats stats = read_stats(fn, mean, stddev, src.c, true);
    Staging st(fn, src);
    const vacv_image s = st.in(src, 0);
    const vacv_image d = st.out(dst, dsize.w, dsize.h, src.c, FP32, src.layout, 1);
    st.run(vacv_resize_normalize(&s, &d, interpolation, VACV_LINEAR_REFERENCE, stats.m(), stats.s(), st.stream()));
    st.finish();
}

void warp_affine_normalize(const Tensor& src, Tensor& dst, const Tensor& M, VSize dsize, int flags, int borderMode,
                           const VScalar& borderValue, const Tensor& mean, const Tensor& stddev) {
    static const char* fn = "va_cv::warp_affine_normalize";
    const std::vector<float> m = affine_of(fn, M);
    const Stats stats = read_stats(fn, mean, stddev, src.c, false);
    warp_into(fn, src, dst, m.data(), dsize, flags, borderMode, borderValue, true, &stats);
}

void warp_affine_normalize(const Tensor& src, Tensor& dst, float scale, float rot, VSize dsize,
                           const VScalar& aux_param, int flags, int borderMode, const VScalar& borderValue,
                           const Tensor& mean, const Tensor& stddev) {
    static const char* fn = "va_cv::warp_affine_normalize";
    const std::vector<float> m = rotation(scale, rot, aux_param);
    const Stats stats = read_stats(fn, mean, stddev, src.c, false);
    warp_into(fn, src, dst, m.data(), dsize, flags, borderMode, borderValue, true, &stats);
}

void crop(const Tensor& src, Tensor& dst, const VRect& rect) {
    static const char* fn = "va_cv::crop";
    // crop.cpp:128-131
    const int left = static_cast<int>(rect.left);
    const int top = static_cast<int>(rect.top);
    const int cw = static_cast<int>(rect.width());
    const int ch = static_cast<int>(rect.height());
    if (cw < 1 || ch < 1 || left < 0 || top < 0 || left + cw > src.w || top + ch > src.h)
        fail(fn, "rect must lie inside the image");  // the reference reads out of bounds
    Staging st(fn, src);
    const vacv_image s = st.in(src, 0);
    const vacv_image d = st.out(dst, cw, ch, src.c, src.dtype, src.layout, 1);
    st.run(vacv_crop(&s, &d, left, top, st.stream()));
    st.finish();
}

// ---- batched frames (FramePipeline: overlapped PCIe staging) ---------------

namespace {

using detail::FramePipeline;

void check_batch(const char* fn, const std::vector<Tensor>& src, std::vector<Tensor>& dst) {
    if (src.empty()) fail(fn, "empty frame list");
    for (const Tensor& t : src)
        if (t.device() != src[0].device()) fail(fn, "frames live on different devices");
    dst.resize(src.size());
}

}  // namespace

void resize(const std::vector<Tensor>& src, std::vector<Tensor>& dst, VSize dsize, double fx, double fy,
            int interpolation) {
    static const char* fn = "va_cv::resize";
    check_batch(fn, src, dst);
    const DType out = resize_out_dtype(fn, src[0], interpolation);
    // dsize = 0 with fx, fy: cv::resize's form, per frame (see the single-frame overload)
    const bool scaled = dsize.w == 0 && dsize.h == 0 && fx > 0 && fy > 0 &&
                        (interpolation == INTER_NEAREST || interpolation == INTER_AREA || interpolation == INTER_LANCZOS4);
    std::vector<VSize> sizes(src.size(), dsize);
    if (scaled)
        for (size_t i = 0; i < src.size(); ++i)
            sizes[i] = VSize(static_cast<int>(std::nearbyint(src[i].w * fx)), static_cast<int>(std::nearbyint(src[i].h * fy)));
    for (const VSize& z : sizes)
        if (z.w < 1 || z.h < 1) fail(fn, "dsize must be positive");
    FramePipeline p(fn, detail::compute_device(src[0]));
    for (size_t i = 0; i < src.size(); ++i)
        p.frame(src[i], dst[i], sizes[i].w, sizes[i].h, src[i].c, out, src[i].layout,
                [&](const vacv_image& s, const vacv_image& d, hipStream_t st) {
                    if (scaled) return vacv_resize_scaled(&s, &d, interpolation, VACV_LINEAR_REFERENCE, fx, fy, st);
                    return vacv_resize(&s, &d, interpolation, VACV_LINEAR_REFERENCE, st);
                });
    p.finish();
}

void resize_normalize(const std::vector<Tensor>& src, std::vector<Tensor>& dst, VSize dsize, double /*fx*/,
                      double /*fy*/, int interpolation, const Tensor& mean, const Tensor& stddev) {
    static const char* fn = "va_cv::resize_normalize";
    check_batch(fn, src, dst);
    (void)resize_out_dtype(fn, src[0], interpolation);
    if (dsize.w < 1 || dsize.h < 1) fail(fn, "dsize must be positive");
    const Stats stats = read_stats(fn, mean, stddev, src[0].c, true);
    FramePipeline p(fn, detail::compute_device(src[0]));
    for (size_t i = 0; i < src.size(); ++i)
        p.frame(src[i], dst[i], dsize.w, dsize.h, src[i].c, FP32, src[i].layout,
                [&](const vacv_image& s, const vacv_image& d, hipStream_t st) {
                    return vacv_resize_normalize(&s, &d, interpolation, VACV_LINEAR_REFERENCE, stats.m(), stats.s(),
                                                 st);
                });
    p.finish();
}

void warp_affine(const std::vector<Tensor>& src, std::vector<Tensor>& dst, const Tensor& M, VSize dsize, int flags,
                 int borderMode, const VScalar& bv) {
    static const char* fn = "va_cv::warp_affine";
    check_batch(fn, src, dst);
    check_warp_modes(fn, src[0], flags, borderMode);
    if (borderMode == BORDER_TRANSPARENT) fail(fn, "BORDER_TRANSPARENT needs the per-frame call");
    if (dsize.w < 1 || dsize.h < 1) fail(fn, "dsize must be positive");
    const std::vector<float> m = affine_of(fn, M);
    const double border[4] = {bv.v0, bv.v1, bv.v2, bv.v3};
    FramePipeline p(fn, detail::compute_device(src[0]));
    for (size_t i = 0; i < src.size(); ++i)
        p.frame(src[i], dst[i], dsize.w, dsize.h, src[i].c, src[i].dtype, src[i].layout,
                [&](const vacv_image& s, const vacv_image& d, hipStream_t st) {
                    return vacv_warp_affine(&s, &d, m.data(), flags, borderMode, border, st);
                });
    p.finish();
}

// ---- one frame, many crops (vacv_warp_affine_rois) -------------------------

namespace {

// The operands of one launch for all crops of a frame, on a leased stream: the
// frame and the per-crop parameters go to HBM once (host operands through the
// pinned pool, a device frame stays where it is), the kernel writes the crops
// back to back into scratch, and each crop is copied into its own dst tensor
// (placement of src).
struct RoiStage {
    const char* fn;
    detail::Lease lease;
    hipStream_t s;
    Tensor pinned;  // the per-crop parameters on the host
    bool queued = false;
    unsigned char* crops = nullptr;
    unsigned char* tail_ptr = nullptr;
    size_t roi_bytes = 0;

    RoiStage(const char* fn_, const Tensor& src) : fn(fn_), lease(detail::compute_device(src)), s(lease.stream()) {}
    // waits for the stream before the staged operands of an early exit go away
    ~RoiStage() {
        if (queued) (void)hipStreamSynchronize(s);
    }
    // k 4-byte values for each of n crops, contiguous, in pinned memory: the caller fills them
    void* host_params(int k, size_t n, const char* oom) {
        pinned = Tensor(k, (int)n, 1, FP32, NCHW);
        if (!pinned.data) fail(fn, oom);
        return pinned.data;
    }
    // ... and they go to scratch slot 1
    void* params() {
        queued = true;
        void* d = lease.scratch(1, pinned.len());
        detail::check_hip(fn, hipMemcpyAsync(d, pinned.data, pinned.len(), hipMemcpyHostToDevice, s));
        return d;
    }
    // the frame where the kernel reads it: a host frame goes to scratch slot 0
    vacv_image frame(const Tensor& src) {
        void* d = src.data;
        if (!src.on_device()) {
            d = lease.scratch(0, src.len());
            detail::check_hip(fn, hipMemcpyAsync(d, src.data, src.len(), hipMemcpyHostToDevice, s));
        }
        return detail::describe(src, d);
    }
    // n crops back to back: scratch slot 2; `tail` more bytes behind them (16-byte aligned) at tail_ptr
    vacv_image out(size_t n, VSize size, int c, DType dtype, size_t tail = 0) {
        roi_bytes = (size_t)size.w * size.h * c * dtype_size(dtype);
        const size_t body = (n * roi_bytes + 15) / 16 * 16;
        crops = static_cast<unsigned char*>(lease.scratch(2, body + tail));
        tail_ptr = crops + body;
        return vacv_image{crops, (int)n, size.w, size.h, c, dtype, NHWC, 0, 0, 0};  // pitches 0 = dense
    }
    // every crop into a tensor of its own with src's placement, then wait
    void scatter(std::vector<Tensor>& dst, const vacv_image& d, const Tensor& src) {
        dst.resize(d.n);
        for (size_t i = 0; i < dst.size(); ++i) {
            dst[i].create_on(src.device(), d.w, d.h, d.c, static_cast<DType>(d.dtype), NHWC);
            if (roi_bytes > 0 && !dst[i].data) fail(fn, "out of memory creating the output tensor");
            detail::check_hip(fn, hipMemcpyAsync(dst[i].data, crops + i * roi_bytes, roi_bytes,
                                                 dst[i].on_device() ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, s));
        }
        lease.sync(fn);
    }
};

// The crops' own statistics, n rows of c floats each of mean then stddev in
// `host`, as {mean, stddev}: two host (c, n) FP32 tensors
void own_stats_out(const char* fn, std::vector<Tensor>& out, const std::vector<float>& host, int c, size_t n) {
    out.resize(2);
    for (int k = 0; k < 2; ++k) {
        out[k].create(c, (int)n, FP32);
        if (!out[k].data) fail(fn, "out of memory creating the statistics");
        std::memcpy(out[k].data, host.data() + k * n * c, n * c * sizeof(float));
    }
}

// One launch for all crops (RoiStage); each matrix is taken from where it
// lives.  yuv_code != 0: src is a YUV420sp frame and the crops are taken from
// its decoded (w, h, 3) image (vacv_cvt_color_warp_affine_rois).  own: every
// crop standardized by its own statistics (vacv_warp_affine_rois_standardize,
// or vacv_cvt_color_warp_affine_rois_standardize from a YUV frame), which go
// to own_out = {mean, stddev} (own_stats_out) when it is given.
void warp_rois_into(const char* fn, const Tensor& src, std::vector<Tensor>& dst, const std::vector<Tensor>& M,
                    VSize dsize, int flags, int borderMode, const VScalar& bv, const Stats* stats, int yuv_code = 0,
                    bool own = false, std::vector<Tensor>* own_out = nullptr) {
    if (src.empty()) fail(fn, "empty input tensor");
    if (yuv_code) {
        check_yuv_code(fn, yuv_code);
        (void)yuv_rows(fn, src);
    }
    if (src.dtype != INT8 && src.dtype != FP32) fail(fn, "warp_affine takes INT8 or FP32");
    if (own && src.dtype != INT8) fail(fn, "crops standardized by their own statistics take an INT8 frame");
    if (src.layout != NHWC) fail(fn, "the crops of one frame take an NHWC frame");
    if ((flags & ~(INTER_MAX | WARP_INVERSE_MAP)) || (flags & INTER_MAX) != INTER_LINEAR)
        fail(fn, "only INTER_LINEAR (optionally | WARP_INVERSE_MAP) is supported for the crops of one frame");
    if (borderMode < BORDER_CONSTANT || borderMode >= BORDER_TRANSPARENT) fail(fn, "unsupported border mode");
    if (dsize.w < 1 || dsize.h < 1) fail(fn, "dsize must be positive");
    if (M.empty()) fail(fn, "empty matrix list");
    const size_t n = M.size();
    if (n > 0x7FFFFFFFu) fail(fn, "too many matrices");
    RoiStage st(fn, src);
    for (const Tensor& m : M) {
        if (m.dtype != FP32 || m.size() != 6) fail(fn, "every M must be a 2x3 FP32 tensor");
        if (m.on_device() && m.device() != st.lease.device()) fail(fn, "operands live on different devices");
    }
    if (src.on_device() && src.device() != st.lease.device()) fail(fn, "operands live on different devices");
    const hipStream_t s = st.s;
    float* mp = static_cast<float*>(st.host_params(6, n, "out of memory staging the matrices"));
    std::memset(mp, 0, n * 6 * sizeof(float));
    for (size_t i = 0; i < n; ++i)
        if (!M[i].on_device()) std::memcpy(mp + 6 * i, M[i].data, 6 * sizeof(float));
    float* dm = static_cast<float*>(st.params());
    for (size_t i = 0; i < n; ++i)  // over the zeros of its place
        if (M[i].on_device())
            detail::check_hip(fn, hipMemcpyAsync(dm + 6 * i, M[i].data, 6 * sizeof(float), hipMemcpyDeviceToDevice, s));
    const vacv_image sd = st.frame(src);
    const int dc = yuv_code ? 3 : src.c;  // the crops' channels
    const size_t own_bytes = own_out ? n * dc * sizeof(float) : 0;  // of each of the two arrays
    const vacv_image dd = st.out(n, dsize, dc, stats || own ? FP32 : src.dtype, 2 * own_bytes);
    std::vector<float> own_host(2 * own_bytes / sizeof(float));
    const double border[4] = {bv.v0, bv.v1, bv.v2, bv.v3};
    if (own) {
        float* om = own_out ? reinterpret_cast<float*>(st.tail_ptr) : nullptr;
        float* os = own_out ? reinterpret_cast<float*>(st.tail_ptr + own_bytes) : nullptr;
        // a crop past one workgroup's LDS is UNSUPPORTED: check() throws
        if (yuv_code)
            detail::check(fn, vacv_cvt_color_warp_affine_rois_standardize(&sd, &dd, yuv_code, dm, nullptr, flags,
                                                                          borderMode, border, om, os, s));
        else
            detail::check(fn,
                          vacv_warp_affine_rois_standardize(&sd, &dd, dm, nullptr, flags, borderMode, border, om, os, s));
        if (own_out)
            detail::check_hip(fn, hipMemcpyAsync(own_host.data(), st.tail_ptr, 2 * own_bytes, hipMemcpyDeviceToHost, s));
    } else if (yuv_code && stats)
        detail::check(fn, vacv_cvt_color_warp_affine_rois_normalize(&sd, &dd, yuv_code, dm, nullptr, flags, borderMode,
                                                                    border, stats->m(), stats->s(), s));
    else if (yuv_code)
        detail::check(fn, vacv_cvt_color_warp_affine_rois(&sd, &dd, yuv_code, dm, nullptr, flags, borderMode, border, s));
    else if (stats)
        detail::check(fn, vacv_warp_affine_rois_normalize(&sd, &dd, dm, nullptr, flags, borderMode, border, stats->m(),
                                                          stats->s(), s));
    else
        detail::check(fn, vacv_warp_affine_rois(&sd, &dd, dm, nullptr, flags, borderMode, border, s));
    st.scatter(dst, dd, src);  // waits for the stream
    if (own_out) own_stats_out(fn, *own_out, own_host, dc, n);
}

}  // namespace

void warp_affine(const Tensor& src, std::vector<Tensor>& dst, const std::vector<Tensor>& M, VSize dsize, int flags,
                 int borderMode, const VScalar& borderValue) {
    warp_rois_into("va_cv::warp_affine", src, dst, M, dsize, flags, borderMode, borderValue, nullptr);
}

void warp_affine_normalize(const Tensor& src, std::vector<Tensor>& dst, const std::vector<Tensor>& M, VSize dsize,
                           int flags, int borderMode, const VScalar& borderValue, const Tensor& mean,
                           const Tensor& stddev) {
    static const char* fn = "va_cv::warp_affine_normalize";
    const Stats stats = read_stats(fn, mean, stddev, src.c, false);
    if (!stats.m()) fail(fn, "the crops of one frame need mean and stddev (no per-image statistics)");
    warp_rois_into(fn, src, dst, M, dsize, flags, borderMode, borderValue, &stats);
}

void warp_affine_standardize(const Tensor& src, std::vector<Tensor>& dst, const std::vector<Tensor>& M, VSize dsize,
                              int flags, int borderMode, const VScalar& borderValue, std::vector<Tensor>* stats) {
    warp_rois_into("va_cv::warp_affine_standardize", src, dst, M, dsize, flags, borderMode, borderValue, nullptr, 0, true,
                   stats);
}

void cvt_color_warp_affine(const Tensor& yuv, std::vector<Tensor>& dst, const std::vector<Tensor>& M, int code,
                           VSize dsize, int flags, int borderMode, const VScalar& borderValue) {
    warp_rois_into("va_cv::cvt_color_warp_affine", yuv, dst, M, dsize, flags, borderMode, borderValue, nullptr, code);
}

void cvt_color_warp_affine_standardize(const Tensor& yuv, std::vector<Tensor>& dst, const std::vector<Tensor>& M,
                                       int code, VSize dsize, int flags, int borderMode, const VScalar& borderValue,
                                       std::vector<Tensor>* stats) {
    warp_rois_into("va_cv::cvt_color_warp_affine_standardize", yuv, dst, M, dsize, flags, borderMode, borderValue,
                   nullptr, code, true, stats);
}

void cvt_color_warp_affine_normalize(const Tensor& yuv, std::vector<Tensor>& dst, const std::vector<Tensor>& M,
                                     int code, VSize dsize, int flags, int borderMode, const VScalar& borderValue,
                                     const Tensor& mean, const Tensor& stddev) {
    static const char* fn = "va_cv::cvt_color_warp_affine_normalize";
    const Stats stats = read_stats(fn, mean, stddev, 3, false);
    if (!stats.m()) fail(fn, "the crops of one frame need mean and stddev (no per-image statistics)");
    warp_rois_into(fn, yuv, dst, M, dsize, flags, borderMode, borderValue, &stats, code);
}

// ---- one frame, many projective crops (vacv_warp_perspective_rois) ---------

namespace {

// warp_rois_into with 3x3 homographies: one launch for all crops (RoiStage),
// each matrix taken from where it lives
void warp_persp_rois_into(const char* fn, const Tensor& src, std::vector<Tensor>& dst, const std::vector<Tensor>& M,
                          VSize dsize, int flags, int borderMode, const VScalar& bv, const Stats* stats) {
    if (src.empty()) fail(fn, "empty input tensor");
    if (src.dtype != INT8 && src.dtype != FP32) fail(fn, "warp_perspective takes INT8 or FP32");
    if (src.layout != NHWC) fail(fn, "the crops of one frame take an NHWC frame");
    if ((flags & ~(INTER_MAX | WARP_INVERSE_MAP)) || (flags & INTER_MAX) != INTER_LINEAR)
        fail(fn, "only INTER_LINEAR (optionally | WARP_INVERSE_MAP) is supported for the crops of one frame");
    if (borderMode < BORDER_CONSTANT || borderMode >= BORDER_TRANSPARENT) fail(fn, "unsupported border mode");
    if (dsize.w < 1 || dsize.h < 1) fail(fn, "dsize must be positive");
    if (M.empty()) fail(fn, "empty matrix list");
    const size_t n = M.size();
    if (n > 0x7FFFFFFFu) fail(fn, "too many matrices");
    RoiStage st(fn, src);
    for (const Tensor& m : M) {
        if (m.dtype != FP32 || m.size() != 9) fail(fn, "every M must be a 3x3 FP32 tensor");
        if (m.on_device() && m.device() != st.lease.device()) fail(fn, "operands live on different devices");
    }
    if (src.on_device() && src.device() != st.lease.device()) fail(fn, "operands live on different devices");
    const hipStream_t s = st.s;
    float* mp = static_cast<float*>(st.host_params(9, n, "out of memory staging the matrices"));
    std::memset(mp, 0, n * 9 * sizeof(float));
    for (size_t i = 0; i < n; ++i)
        if (!M[i].on_device()) std::memcpy(mp + 9 * i, M[i].data, 9 * sizeof(float));
    float* dm = static_cast<float*>(st.params());
    for (size_t i = 0; i < n; ++i)  // over the zeros of its place
        if (M[i].on_device())
            detail::check_hip(fn, hipMemcpyAsync(dm + 9 * i, M[i].data, 9 * sizeof(float), hipMemcpyDeviceToDevice, s));
    const vacv_image sd = st.frame(src);
    const vacv_image dd = st.out(n, dsize, src.c, stats ? FP32 : src.dtype);
    const double border[4] = {bv.v0, bv.v1, bv.v2, bv.v3};
    if (stats)
        detail::check(fn, vacv_warp_perspective_rois_normalize(&sd, &dd, dm, nullptr, flags, borderMode, border,
                                                               stats->m(), stats->s(), s));
    else
        detail::check(fn, vacv_warp_perspective_rois(&sd, &dd, dm, nullptr, flags, borderMode, border, s));
    st.scatter(dst, dd, src);  // waits for the stream
}

}  // namespace

void warp_perspective(const Tensor& src, std::vector<Tensor>& dst, const std::vector<Tensor>& M, VSize dsize, int flags,
                      int borderMode, const VScalar& borderValue) {
    warp_persp_rois_into("va_cv::warp_perspective", src, dst, M, dsize, flags, borderMode, borderValue, nullptr);
}

void warp_perspective_normalize(const Tensor& src, std::vector<Tensor>& dst, const std::vector<Tensor>& M, VSize dsize,
                                int flags, int borderMode, const VScalar& borderValue, const Tensor& mean,
                                const Tensor& stddev) {
    static const char* fn = "va_cv::warp_perspective_normalize";
    const Stats stats = read_stats(fn, mean, stddev, src.c, false);
    if (!stats.m()) fail(fn, "the crops of one frame need mean and stddev (no per-image statistics)");
    warp_persp_rois_into(fn, src, dst, M, dsize, flags, borderMode, borderValue, &stats);
}

void warp_perspective(const Tensor& src, Tensor& dst, const Tensor& M, VSize dsize, int flags, int borderMode,
                      const VScalar& borderValue) {
    std::vector<Tensor> one;
    warp_persp_rois_into("va_cv::warp_perspective", src, one, std::vector<Tensor>(1, M), dsize, flags, borderMode,
                         borderValue, nullptr);
    dst = one[0];
}

void get_perspective_transform(const float src_quad[8], const float dst_quad[8], Tensor& M) {
    static const char* fn = "va_cv::get_perspective_transform";
    M.create(3, 3, FP32);
    if (!M.data) fail(fn, "out of memory creating the matrix");
    detail::check(fn, vacv_perspective_transform(src_quad, dst_quad, static_cast<float*>(M.data)));
}

// ---- one frame, many upright crops (vacv_crop_resize_rois) -----------------

namespace {

// One launch for all crops (RoiStage) of the rects, truncated as crop() does.
// yuv_code != 0: src is a YUV420sp frame and the rects are taken from its
// decoded (w, h, 3) image (vacv_cvt_color_crop_resize_rois).  own: every crop
// standardized by its own statistics (vacv_crop_resize_rois_standardize, or
// vacv_cvt_color_crop_resize_rois_standardize from a YUV frame), which go to
// own_out = {mean, stddev} (own_stats_out) when it is given.
void crop_resize_into(const char* fn, const Tensor& src, std::vector<Tensor>& dst, const std::vector<VRect>& rects,
                      VSize dsize, int interpolation, const Stats* stats, int yuv_code = 0, bool own = false,
                      std::vector<Tensor>* own_out = nullptr) {
    if (src.empty()) fail(fn, "empty input tensor");
    int fw = src.w, fh = src.h;  // what the rects must lie in
    if (yuv_code) {
        check_yuv_code(fn, yuv_code);
        fh = yuv_rows(fn, src);
    }
    if (src.dtype != INT8 && src.dtype != FP32) fail(fn, "crop_resize takes INT8 or FP32");
    if (own && src.dtype != INT8) fail(fn, "crops standardized by their own statistics take an INT8 frame");
    if (src.layout != NHWC) fail(fn, "the crops of one frame take an NHWC frame");
    if (interpolation != INTER_LINEAR) fail(fn, "only INTER_LINEAR is supported for the crops of one frame");
    if (dsize.w < 1 || dsize.h < 1) fail(fn, "dsize must be positive");
    if (rects.empty()) fail(fn, "empty rect list");
    const size_t n = rects.size();
    if (n > 0x7FFFFFFFu) fail(fn, "too many rects");
    RoiStage st(fn, src);
    if (src.on_device() && src.device() != st.lease.device()) fail(fn, "operands live on different devices");

    int32_t* rp = static_cast<int32_t*>(st.host_params(4, n, "out of memory staging the rects"));
    for (size_t i = 0; i < n; ++i) {
        // crop.cpp:128-131
        const int left = static_cast<int>(rects[i].left), top = static_cast<int>(rects[i].top);
        const int cw = static_cast<int>(rects[i].width()), ch = static_cast<int>(rects[i].height());
        // what crop() and resize() refuse one by one (the kernel would write zeros)
        if (cw < 2 || ch < 2 || left < 0 || top < 0 || cw > fw || left > fw - cw || ch > fh || top > fh - ch)
            fail(fn, "every rect must lie inside the image and hold at least 2 x 2 pixels");
        rp[4 * i] = left;
        rp[4 * i + 1] = top;
        rp[4 * i + 2] = cw;
        rp[4 * i + 3] = ch;
    }
    const int32_t* dr = static_cast<const int32_t*>(st.params());
    const vacv_image sd = st.frame(src);
    const int dc = yuv_code ? 3 : src.c;  // the crops' channels
    const size_t own_bytes = own_out ? n * dc * sizeof(float) : 0;  // of each of the two arrays
    const vacv_image dd = st.out(n, dsize, dc, stats || own ? FP32 : src.dtype, 2 * own_bytes);
    std::vector<float> own_host(2 * own_bytes / sizeof(float));
    if (own) {
        float* dm = own_out ? reinterpret_cast<float*>(st.tail_ptr) : nullptr;
        float* ds = own_out ? reinterpret_cast<float*>(st.tail_ptr + own_bytes) : nullptr;
        // a crop past one workgroup's LDS is UNSUPPORTED: check() throws
        if (yuv_code)
            detail::check(fn, vacv_cvt_color_crop_resize_rois_standardize(&sd, &dd, yuv_code, dr, nullptr, interpolation,
                                                                          VACV_LINEAR_REFERENCE, dm, ds, st.s));
        else
            detail::check(fn, vacv_crop_resize_rois_standardize(&sd, &dd, dr, nullptr, interpolation,
                                                                VACV_LINEAR_REFERENCE, dm, ds, st.s));
        if (own_out)
            detail::check_hip(fn, hipMemcpyAsync(own_host.data(), st.tail_ptr, 2 * own_bytes, hipMemcpyDeviceToHost, st.s));
    } else if (yuv_code && stats)
        detail::check(fn, vacv_cvt_color_crop_resize_rois_normalize(&sd, &dd, yuv_code, dr, nullptr, interpolation,
                                                                    VACV_LINEAR_REFERENCE, stats->m(), stats->s(), st.s));
    else if (yuv_code)
        detail::check(fn, vacv_cvt_color_crop_resize_rois(&sd, &dd, yuv_code, dr, nullptr, interpolation,
                                                          VACV_LINEAR_REFERENCE, st.s));
    else if (stats)
        detail::check(fn, vacv_crop_resize_rois_normalize(&sd, &dd, dr, nullptr, interpolation, VACV_LINEAR_REFERENCE,
                                                          stats->m(), stats->s(), st.s));
    else
        detail::check(fn, vacv_crop_resize_rois(&sd, &dd, dr, nullptr, interpolation, VACV_LINEAR_REFERENCE, st.s));
    st.scatter(dst, dd, src);  // waits for the stream
    if (own_out) own_stats_out(fn, *own_out, own_host, dc, n);
}

}  // namespace

void crop_resize(const Tensor& src, std::vector<Tensor>& dst, const std::vector<VRect>& rects, VSize dsize,
                 int interpolation) {
    crop_resize_into("va_cv::crop_resize", src, dst, rects, dsize, interpolation, nullptr);
}

void crop_resize_normalize(const Tensor& src, std::vector<Tensor>& dst, const std::vector<VRect>& rects, VSize dsize,
                           int interpolation, const Tensor& mean, const Tensor& stddev) {
    static const char* fn = "va_cv::crop_resize_normalize";
    const Stats stats = read_stats(fn, mean, stddev, src.c, false);
    if (!stats.m()) fail(fn, "the crops of one frame need mean and stddev (no per-image statistics)");
    crop_resize_into(fn, src, dst, rects, dsize, interpolation, &stats);
}

void crop_resize_standardize(const Tensor& src, std::vector<Tensor>& dst, const std::vector<VRect>& rects, VSize dsize,
                              int interpolation, std::vector<Tensor>* stats) {
    crop_resize_into("va_cv::crop_resize_standardize", src, dst, rects, dsize, interpolation, nullptr, 0, true, stats);
}

void cvt_color_crop_resize(const Tensor& yuv, std::vector<Tensor>& dst, const std::vector<VRect>& rects, int code,
                           VSize dsize, int interpolation) {
    crop_resize_into("va_cv::cvt_color_crop_resize", yuv, dst, rects, dsize, interpolation, nullptr, code);
}

void cvt_color_crop_resize_standardize(const Tensor& yuv, std::vector<Tensor>& dst, const std::vector<VRect>& rects,
                                       int code, VSize dsize, int interpolation, std::vector<Tensor>* stats) {
    crop_resize_into("va_cv::cvt_color_crop_resize_standardize", yuv, dst, rects, dsize, interpolation, nullptr, code,
                     true, stats);
}

void cvt_color_crop_resize_normalize(const Tensor& yuv, std::vector<Tensor>& dst, const std::vector<VRect>& rects,
                                     int code, VSize dsize, int interpolation, const Tensor& mean,
                                     const Tensor& stddev) {
    static const char* fn = "va_cv::cvt_color_crop_resize_normalize";
    const Stats stats = read_stats(fn, mean, stddev, 3, false);
    if (!stats.m()) fail(fn, "the crops of one frame need mean and stddev (no per-image statistics)");
    crop_resize_into(fn, yuv, dst, rects, dsize, interpolation, &stats, code);
}

void cvt_color(const std::vector<Tensor>& src, std::vector<Tensor>& dst, int code) {
    static const char* fn = "va_cv::cvt_color";
    check_batch(fn, src, dst);
    check_yuv_code(fn, code);
    FramePipeline p(fn, detail::compute_device(src[0]));
    for (size_t i = 0; i < src.size(); ++i) {
        const int h = yuv_rows(fn, src[i]);
        p.frame(src[i], dst[i], src[i].w, h, 3, INT8, NHWC,
                [&](const vacv_image& s, const vacv_image& d, hipStream_t st) {
                    return vacv_cvt_color(&s, &d, code, st);
                });
    }
    p.finish();
}

void cvt_color_normalize(const std::vector<Tensor>& src, std::vector<Tensor>& dst, int code, const Tensor& mean,
                         const Tensor& stddev) {
    static const char* fn = "va_cv::cvt_color_normalize";
    check_batch(fn, src, dst);
    check_yuv_code(fn, code);
    const Stats stats = read_stats(fn, mean, stddev, 3, false);
    FramePipeline p(fn, detail::compute_device(src[0]));
    for (size_t i = 0; i < src.size(); ++i) {
        const int h = yuv_rows(fn, src[i]);
        p.frame(src[i], dst[i], src[i].w, h, 3, FP32, NHWC,
                [&](const vacv_image& s, const vacv_image& d, hipStream_t st) {
                    return vacv_cvt_color_normalize(&s, &d, code, stats.m(), stats.s(), st);
                });
    }
    p.finish();
}

void match_template(const Tensor& src, const Tensor& target, Tensor& result, int method) {
    static const char* fn = "va_cv::match_template";
    // match_template.cpp:13-41 -> cv::matchTemplate (OpenCV 2.4 semantics,
    // exact correlation; the C ABI swaps a larger template as OpenCV does)
    if (src.dtype != INT8 && src.dtype != FP32) fail(fn, "match_template takes INT8 or FP32");
    if (target.dtype != src.dtype || target.c != src.c) fail(fn, "the template must match the image's dtype and channels");
    if (src.layout != NHWC || target.layout != NHWC) fail(fn, "match_template takes NHWC tensors");
    const bool swap = target.w >= src.w && target.h >= src.h && (target.w > src.w || target.h > src.h);
    const Tensor& a = swap ? target : src;
    const Tensor& b = swap ? src : target;
    if (b.w > a.w || b.h > a.h) fail(fn, "the template does not fit the image");
    Staging st(fn, src);
    const vacv_image s = st.in(a, 0);
    const vacv_image t = st.in(b, 1);
    const vacv_image d = st.out(result, a.w - b.w + 1, a.h - b.h + 1, 1, FP32, NHWC, 2);
    st.run(vacv_match_template(&s, &t, &d, method, st.stream()));
    st.finish();
}

void minMaxIdx(const Tensor& src, double* minVal, double* maxVal, int* minIdx, int* maxIdx, const Tensor& mask) {
    static const char* fn = "va_cv::minMaxIdx";
    // match_template.cpp:43-46 -> cv::minMaxIdx of a single-channel array;
    // minIdx / maxIdx receive (row, col)
    if (src.c != 1) fail(fn, "minMaxIdx takes a single-channel tensor");
    Staging st(fn, src);
    const vacv_image s = st.in(src, 0);
    vacv_image m{};
    const bool has_mask = !mask.empty();
    if (has_mask) m = st.in(mask, 1);
    Tensor out;
    const vacv_image o = st.out(out, 48, 1, 1, INT8, NHWC, 2);  // 2 doubles + 4 ints, device scratch
    double* vals = static_cast<double*>(o.data);
    int* idx = reinterpret_cast<int*>(static_cast<char*>(o.data) + 16);
    st.run(vacv_min_max_idx(&s, has_mask ? &m : nullptr, vals, idx, st.stream()));
    double hv[2];
    int hi[4];
    detail::check_hip(fn, hipMemcpyAsync(hv, vals, sizeof(hv), hipMemcpyDeviceToHost, st.stream()));
    detail::check_hip(fn, hipMemcpyAsync(hi, idx, sizeof(hi), hipMemcpyDeviceToHost, st.stream()));
    st.finish();
    if (minVal) *minVal = hv[0];
    if (maxVal) *maxVal = hv[1];
    if (minIdx) { minIdx[0] = hi[0]; minIdx[1] = hi[1]; }
    if (maxIdx) { maxIdx[0] = hi[2]; maxIdx[1] = hi[3]; }
}

namespace {

// One frame, windows.size() matches and their peaks, one launch (RoiStage):
// the origins and the templates go to HBM in one block (host templates through
// the pinned pool, device templates copied into their place), the kernel
// writes the maps back to back with the peaks behind them.  yuv_code != 0: src
// is a YUV420sp frame, the windows are taken from its decoded (w, h, 3) image
// and the templates have its three channels (vacv_cvt_color_match_template_rois).
void match_rois_into(const char* fn, const Tensor& src, const std::vector<Tensor>& targets,
                     const std::vector<VRect>& windows, std::vector<Tensor>& results, int method,
                     std::vector<VMatchPeak>* peaks, int yuv_code = 0) {
    if (src.empty()) fail(fn, "empty input tensor");
    int fw = src.w, fh = src.h, fc = src.c;  // what the windows must lie in, and the templates' channels
    if (yuv_code) {
        check_yuv_code(fn, yuv_code);
        fh = yuv_rows(fn, src);
        fc = 3;
    }
    if (src.dtype != INT8) fail(fn, "the matches of one frame take INT8");
    if (src.layout != NHWC) fail(fn, "the matches of one frame take an NHWC frame");
    if (windows.empty()) fail(fn, "empty window list");
    const size_t n = windows.size();
    if (n > 0x7FFFFFFFu) fail(fn, "too many windows");
    if (targets.size() != 1 && targets.size() != n) fail(fn, "give one template, or one per window");
    const Tensor& t0 = targets[0];
    if (t0.empty()) fail(fn, "empty template");
    for (const Tensor& t : targets) {
        if (t.dtype != src.dtype || t.c != fc || t.layout != NHWC)
            fail(fn, "every template must match the frame's dtype, channels and layout");
        if (t.w != t0.w || t.h != t0.h) fail(fn, "all templates must have one size");
    }
    RoiStage st(fn, src);
    if (src.on_device() && src.device() != st.lease.device()) fail(fn, "operands live on different devices");
    for (const Tensor& t : targets)
        if (t.on_device() && t.device() != st.lease.device()) fail(fn, "operands live on different devices");

    // [n][2] origins, then the templates, each padded to whole dwords
    const size_t tbytes = t0.len(), tstep = (tbytes + 3) / 4 * 4, nt = targets.size();
    int32_t* op = static_cast<int32_t*>(st.host_params(1, 2 * n + nt * (tstep / 4), "out of memory staging the windows"));
    int ww = 0, wh = 0;
    for (size_t i = 0; i < n; ++i) {
        // crop.cpp:128-131
        const int left = static_cast<int>(windows[i].left), top = static_cast<int>(windows[i].top);
        const int cw = static_cast<int>(windows[i].width()), ch = static_cast<int>(windows[i].height());
        if (i == 0) {
            ww = cw;
            wh = ch;
        }
        if (cw != ww || ch != wh) fail(fn, "all windows must have one size");
        if (cw < 1 || ch < 1 || left < 0 || top < 0 || cw > fw || left > fw - cw || ch > fh || top > fh - ch)
            fail(fn, "every window must lie inside the image");
        op[2 * i] = left;
        op[2 * i + 1] = top;
    }
    if (t0.w > ww || t0.h > wh) fail(fn, "the template does not fit the window");
    unsigned char* tp = reinterpret_cast<unsigned char*>(op + 2 * n);
    std::memset(tp, 0, nt * tstep);
    for (size_t i = 0; i < nt; ++i)
        if (!targets[i].on_device()) std::memcpy(tp + i * tstep, targets[i].data, tbytes);
    unsigned char* dp = static_cast<unsigned char*>(st.params());
    unsigned char* dt = dp + 2 * n * sizeof(int32_t);
    for (size_t i = 0; i < nt; ++i)  // over the zeros of its place
        if (targets[i].on_device())
            detail::check_hip(fn, hipMemcpyAsync(dt + i * tstep, targets[i].data, tbytes, hipMemcpyDeviceToDevice, st.s));
    const vacv_image sd = st.frame(src);
    const vacv_image td{dt, (int)nt, t0.w, t0.h, t0.c, INT8, NHWC, 0, 0, (int64_t)tstep};
    const size_t peak_bytes = peaks ? n * (2 * sizeof(double) + 4 * sizeof(int32_t)) : 0;
    const vacv_image rd = st.out(n, VSize(ww - t0.w + 1, wh - t0.h + 1), 1, FP32, peak_bytes);
    double* dv = peaks ? reinterpret_cast<double*>(st.tail_ptr) : nullptr;
    int32_t* di = peaks ? reinterpret_cast<int32_t*>(st.tail_ptr + n * 2 * sizeof(double)) : nullptr;
    if (yuv_code)
        detail::check(fn, vacv_cvt_color_match_template_rois(&sd, &td, &rd, yuv_code, reinterpret_cast<const int32_t*>(dp),
                                                             nullptr, method, dv, di, st.s));
    else
        detail::check(fn, vacv_match_template_rois(&sd, &td, &rd, reinterpret_cast<const int32_t*>(dp), nullptr, method,
                                                   dv, di, st.s));
    std::vector<unsigned char> hp(peak_bytes);
    if (peaks) detail::check_hip(fn, hipMemcpyAsync(hp.data(), st.tail_ptr, peak_bytes, hipMemcpyDeviceToHost, st.s));
    st.scatter(results, rd, src);
    if (!peaks) return;
    peaks->resize(n);
    const double* hv = reinterpret_cast<const double*>(hp.data());
    const int32_t* hi = reinterpret_cast<const int32_t*>(hp.data() + n * 2 * sizeof(double));
    for (size_t i = 0; i < n; ++i) {
        VMatchPeak& p = (*peaks)[i];
        p.minVal = hv[2 * i];
        p.maxVal = hv[2 * i + 1];
        p.minIdx[0] = hi[4 * i];
        p.minIdx[1] = hi[4 * i + 1];
        p.maxIdx[0] = hi[4 * i + 2];
        p.maxIdx[1] = hi[4 * i + 3];
    }
}

}  // namespace

void match_template(const Tensor& src, const std::vector<Tensor>& targets, const std::vector<VRect>& windows,
                    std::vector<Tensor>& results, int method, std::vector<VMatchPeak>* peaks) {
    match_rois_into("va_cv::match_template", src, targets, windows, results, method, peaks);
}

void cvt_color_match_template(const Tensor& yuv, const std::vector<Tensor>& targets, const std::vector<VRect>& windows,
                              std::vector<Tensor>& results, int code, int method, std::vector<VMatchPeak>* peaks) {
    match_rois_into("va_cv::cvt_color_match_template", yuv, targets, windows, results, method, peaks, code);
}

void imencode(const Tensor&, std::vector<unsigned char>&, const char*) {
    fail("va_cv::imencode", "not provided by the MI355X build (OpenCV-only in the reference)");
}

}  // namespace va_cv
