// One YUV420sp frame, many affine crops standardized by their own statistics
// through the C++ layer: va_cv::cvt_color_warp_affine_standardize (one kernel
// launch, no decoded frame) against va_cv::cvt_color followed by
// va_cv::warp_affine_standardize on the decoded frame, and against
// va_cv::warp_affine with the same matrices and va_cv::normalize with mean and
// stddev left empty once per crop, bit for bit; the statistics too.  Host
// operands (staged through the pinned pool) and device-resident ones.  Built
// and run by tests/test_yuv_warp_rois_std_gpu.py; needs a HIP device.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <vector>

#include "cv/cv.h"

using vision::Tensor;

static int g_failed = 0, g_cases = 0;

static void expect(bool ok, const char* what, int i = -1) {
    ++g_cases;
    if (!ok) {
        ++g_failed;
        std::printf("FAIL %s (crop %d)\n", what, i);
    }
}

static Tensor make_yuv(int w, int h) {
    Tensor t(w, h * 3 / 2, 1, vision::INT8, vision::NHWC);
    unsigned s = 54321u;
    for (size_t i = 0; i < t.size(); ++i) {
        s = s * 1664525u + 1013904223u;
        static_cast<unsigned char*>(t.data)[i] = (unsigned char)((s >> 24) & 0xFFu);
    }
    return t;
}

static Tensor make_map(float scale, float deg, float cx, float cy, float ox, float oy) {
    // rotate/scale about (cx, cy) of the frame, onto (ox, oy) of the crop
    const float a = deg * 3.14159265f / 180.f, ca = scale * std::cos(a), sa = scale * std::sin(a);
    Tensor m(3, 2, 1, vision::FP32, vision::NCHW);
    float* p = static_cast<float*>(m.data);
    p[0] = ca; p[1] = sa; p[2] = ox - ca * cx - sa * cy;
    p[3] = -sa; p[4] = ca; p[5] = oy + sa * cx - ca * cy;
    return m;
}

static bool same_bytes(const Tensor& a, const Tensor& b) {
    const Tensor x = a.to_host(), y = b.to_host();
    return x.w == y.w && x.h == y.h && x.c == y.c && x.dtype == y.dtype && x.layout == y.layout && x.len() == y.len() &&
           std::memcmp(x.data, y.data, x.len()) == 0;
}

static void run(const Tensor& yuv, const std::vector<Tensor>& M, bool on_device, int code, int border,
                const char* what) {
    const va_cv::VSize size(37, 29);
    va_cv::VScalar bv;
    bv.v0 = 7; bv.v1 = 99; bv.v2 = 200;
    std::vector<Tensor> crops, again, chain, warped, stats, chain_stats;
    va_cv::cvt_color_warp_affine_standardize(yuv, crops, M, code, size, va_cv::INTER_LINEAR, border, bv, &stats);
    va_cv::cvt_color_warp_affine_standardize(yuv, again, M, code, size, va_cv::INTER_LINEAR, border, bv);
    Tensor bgr;
    va_cv::cvt_color(yuv, bgr, code);
    va_cv::warp_affine_standardize(bgr, chain, M, size, va_cv::INTER_LINEAR, border, bv, &chain_stats);
    va_cv::warp_affine(bgr, warped, M, size, va_cv::INTER_LINEAR, border, bv);
    expect(crops.size() == M.size() && again.size() == M.size() && chain.size() == M.size() && warped.size() == M.size(),
           what);
    expect(stats.size() == 2 && chain_stats.size() == 2, "two statistics tensors");
    if (stats.size() != 2 || chain_stats.size() != 2) return;
    for (int k = 0; k < 2; ++k) {
        expect(!stats[k].on_device() && stats[k].dtype == vision::FP32 && stats[k].w == 3 && stats[k].h == (int)M.size(),
               "statistics: host FP32 (3, n)");
        expect(same_bytes(stats[k], chain_stats[k]), k ? "stddev vs the chain" : "mean vs the chain");
    }
    for (size_t i = 0; i < M.size() && i < crops.size() && i < again.size() && i < chain.size() && i < warped.size();
         ++i) {
        Tensor none, mean, stdv;
        va_cv::normalize(warped[i], none);  // mean and stddev empty: the crop's own statistics
        va_cv::mean_stddev(warped[i], mean, stdv);
        const Tensor mh = mean.to_host(), sh = stdv.to_host();
        expect(crops[i].on_device() == on_device && crops[i].dtype == vision::FP32 && crops[i].c == 3,
               "placement and dtype", (int)i);
        expect(same_bytes(crops[i], chain[i]), "vs cvt_color + warp_affine_standardize", (int)i);
        expect(same_bytes(crops[i], none), what, (int)i);
        expect(same_bytes(again[i], none), "without statistics", (int)i);
        expect(std::memcmp(static_cast<const float*>(stats[0].data) + i * 3, mh.data, 3 * sizeof(float)) == 0, "mean",
               (int)i);
        expect(std::memcmp(static_cast<const float*>(stats[1].data) + i * 3, sh.data, 3 * sizeof(float)) == 0,
               "stddev", (int)i);
    }
}

template <class F>
static int throws(F f) {
    try {
        f();
    } catch (const std::runtime_error&) {
        return 1;
    }
    return 0;
}

int main() {
    try {
        std::vector<Tensor> M;
        M.push_back(make_map(1.0f, 0.f, 80.f, 60.f, 18.f, 14.f));
        M.push_back(make_map(0.7f, 15.f, 40.f, 30.f, 18.f, 14.f));
        M.push_back(make_map(1.9f, -30.f, 120.f, 90.f, 18.f, 14.f));
        M.push_back(make_map(1.0f, 0.f, 159.f, 119.f, 18.f, 14.f));     // the frame's last pixel inside the crop
        M.push_back(make_map(1.1f, 170.f, 5.f, 5.f, 18.f, 14.f));       // mostly off the frame
        M.push_back(make_map(0.5f, 45.f, 1000.f, 1000.f, 18.f, 14.f));  // all border
        const Tensor yuv = make_yuv(160, 120);
        run(yuv, M, false, va_cv::COLOR_YUV2BGR_NV21, va_cv::BORDER_CONSTANT, "host NV21 -> BGR");
        run(yuv, M, false, va_cv::COLOR_YUV2RGB_NV12, va_cv::BORDER_REFLECT, "host NV12 -> RGB, BORDER_REFLECT");
        // device-resident frame, the matrices on the device too (all but one)
        const Tensor dyuv = yuv.to_device(0);
        std::vector<Tensor> dM;
        for (size_t i = 0; i < M.size(); ++i) dM.push_back(i == 2 ? M[i] : M[i].to_device(0));
        run(dyuv, dM, true, va_cv::COLOR_YUV2RGB_NV21, va_cv::BORDER_CONSTANT, "device NV21 -> RGB");
        run(dyuv, dM, true, va_cv::COLOR_YUV2BGR_NV12, va_cv::BORDER_REPLICATE, "device NV12 -> BGR, BORDER_REPLICATE");
        // refused loudly
        const int nv21 = va_cv::COLOR_YUV2BGR_NV21;
        const va_cv::VSize size(8, 8);
        std::vector<Tensor> out;
        const Tensor bgr_frame(16, 12, 3, vision::INT8, vision::NHWC);
        int thrown = 0;
        thrown += throws([&] { va_cv::cvt_color_warp_affine_standardize(yuv, out, M, nv21, va_cv::VSize(145, 144)); });
        thrown += throws([&] { va_cv::cvt_color_warp_affine_standardize(yuv, out, M, va_cv::COLOR_YUV2BGRA_NV21, size); });
        thrown += throws([&] { va_cv::cvt_color_warp_affine_standardize(yuv, out, M, va_cv::COLOR_YUV2BGR_YV12, size); });
        expect(thrown == 3, "an oversize dsize and a bad code throw");
        thrown = 0;
        thrown += throws([&] { va_cv::cvt_color_warp_affine_standardize(yuv, out, std::vector<Tensor>(), nv21, size); });
        thrown += throws([&] { va_cv::cvt_color_warp_affine_standardize(yuv, out, M, nv21, size, va_cv::INTER_NEAREST); });
        thrown += throws([&] {
            va_cv::cvt_color_warp_affine_standardize(yuv, out, M, nv21, size, va_cv::INTER_LINEAR,
                                                     va_cv::BORDER_TRANSPARENT);
        });
        thrown += throws([&] { va_cv::cvt_color_warp_affine_standardize(yuv, out, M, nv21, va_cv::VSize(0, 8)); });
        thrown += throws([&] { va_cv::cvt_color_warp_affine_standardize(bgr_frame, out, M, nv21, size); });
        expect(thrown == 5, "unsupported combinations throw");
        va_cv::cvt_color_warp_affine_standardize(yuv, out, M, nv21, va_cv::VSize(144, 144));  // exactly 64 KiB of LDS
        expect(out.size() == M.size() && out[0].w == 144 && out[0].h == 144 && out[0].c == 3, "144 x 144 fits");
    } catch (const std::exception& e) {
        std::printf("exception: %s\n", e.what());
        return 2;
    }
    std::printf("cases %d failed %d\n", g_cases, g_failed);
    return g_failed ? 1 : 0;
}
