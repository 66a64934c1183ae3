// One YUV420sp frame, many upright crops through the C++ layer:
// va_cv::cvt_color_crop_resize / cvt_color_crop_resize_normalize (one kernel
// launch, no decoded frame, no crops) against va_cv::cvt_color followed by
// va_cv::crop and va_cv::resize / resize_normalize once per rect, byte for
// byte.  A host frame (staged through the pinned pool) and a device-resident
// one.  Built and run by tests/test_yuv_crop_resize_rois_gpu.py; needs a HIP
// device.
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <vector>

#include "cv/cv.h"

using vision::Tensor;
using vision::VRect;

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

static bool same_bytes(const Tensor& a, const Tensor& b) {
    const Tensor x = a.to_host(), y = b.to_host();
    return x.w == y.w && x.h == y.h && x.c == y.c && x.dtype == y.dtype && x.layout == y.layout && x.len() == y.len() &&
           std::memcmp(x.data, y.data, x.len()) == 0;
}

static void run(const Tensor& yuv, const std::vector<VRect>& rects, bool on_device, int code, const char* what) {
    const va_cv::VSize size(37, 29);
    Tensor mean(3, 1, 1, vision::FP32, vision::NCHW), stdv(3, 1, 1, vision::FP32, vision::NCHW);
    const float mv[3] = {104.5f, 117.25f, 123.f}, sv[3] = {57.375f, 57.12f, 58.395f};
    std::memcpy(mean.data, mv, sizeof(mv));
    std::memcpy(stdv.data, sv, sizeof(sv));

    std::vector<Tensor> crops, ncrops;
    va_cv::cvt_color_crop_resize(yuv, crops, rects, code, size);
    va_cv::cvt_color_crop_resize_normalize(yuv, ncrops, rects, code, size, va_cv::INTER_LINEAR, mean, stdv);
    expect(crops.size() == rects.size() && ncrops.size() == rects.size(), what);
    Tensor bgr;
    va_cv::cvt_color(yuv, bgr, code);
    for (size_t i = 0; i < rects.size() && i < crops.size() && i < ncrops.size(); ++i) {
        Tensor cut, one, none;
        va_cv::crop(bgr, cut, rects[i]);
        va_cv::resize(cut, one, size);
        va_cv::resize_normalize(cut, none, size, 0, 0, va_cv::INTER_LINEAR, mean, stdv);
        expect(crops[i].on_device() == on_device && ncrops[i].on_device() == on_device, "placement", (int)i);
        expect(crops[i].dtype == vision::INT8 && ncrops[i].dtype == vision::FP32 && crops[i].c == 3 && ncrops[i].c == 3,
               "dtype", (int)i);
        expect(same_bytes(crops[i], one), what, (int)i);
        expect(same_bytes(ncrops[i], none), "normalize", (int)i);
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
        std::vector<VRect> rects;
        rects.push_back(VRect(0.f, 0.f, 160.f, 120.f));        // the whole frame
        rects.push_back(VRect(10.9f, 20.9f, 110.1f, 70.1f));   // fractional: (10, 20) 99 x 49
        rects.push_back(VRect(101.f, 81.f, 138.f, 110.f));     // the output's own size, odd origin
        rects.push_back(VRect(158.f, 118.f, 160.f, 120.f));    // 2 x 2 in the corner: the last chroma pair
        rects.push_back(VRect(157.f, 117.f, 160.f, 120.f));    // 3 x 3 there, odd origin
        rects.push_back(VRect(31.f, 5.f, 42.f, 100.f));        // 11 x 95
        const Tensor yuv = make_yuv(160, 120);
        run(yuv, rects, false, va_cv::COLOR_YUV2BGR_NV21, "host NV21 -> BGR");
        run(yuv, rects, false, va_cv::COLOR_YUV2RGB_NV12, "host NV12 -> RGB");
        const Tensor dyuv = yuv.to_device(0);
        run(dyuv, rects, true, va_cv::COLOR_YUV2RGB_NV21, "device NV21 -> RGB");
        run(dyuv, rects, true, va_cv::COLOR_YUV2BGR_NV12, "device NV12 -> BGR");
        // refused loudly
        const int nv21 = va_cv::COLOR_YUV2BGR_NV21;
        const va_cv::VSize size(8, 8);
        Tensor mean(3, 1, 1, vision::FP32, vision::NCHW), stdv(3, 1, 1, vision::FP32, vision::NCHW);
        const float mv[3] = {1.f, 2.f, 3.f}, sv[3] = {4.f, 5.f, 6.f};
        std::memcpy(mean.data, mv, sizeof(mv));
        std::memcpy(stdv.data, sv, sizeof(sv));
        std::vector<Tensor> out;
        const Tensor bgr_frame(16, 12, 3, vision::INT8, vision::NHWC);
        int thrown = 0;
        // both functions: no rects, a non-linear interpolation, a rect outside the decoded frame (the Y and
        // chroma rows below it do not count), a rect below 2 x 2, an unsupported code, a non-YUV source
        const std::vector<VRect> none, past_right = {VRect(150.f, 0.f, 161.f, 10.f)}, past_bottom = {VRect(0.f, 100.f, 10.f, 121.f)},
                                 column = {VRect(5.f, 5.f, 6.f, 50.f)}, negative = {VRect(-1.f, 5.f, 6.f, 50.f)};
        for (int normalize = 0; normalize < 2; ++normalize) {
            auto call = [&](const Tensor& src, const std::vector<VRect>& r, int code, int interpolation) {
                if (normalize) va_cv::cvt_color_crop_resize_normalize(src, out, r, code, size, interpolation, mean, stdv);
                else va_cv::cvt_color_crop_resize(src, out, r, code, size, interpolation);
            };
            thrown += throws([&] { call(yuv, none, nv21, va_cv::INTER_LINEAR); });
            thrown += throws([&] { call(yuv, rects, nv21, va_cv::INTER_CUBIC); });
            thrown += throws([&] { call(yuv, rects, nv21, va_cv::INTER_NEAREST); });
            thrown += throws([&] { call(yuv, past_right, nv21, va_cv::INTER_LINEAR); });
            thrown += throws([&] { call(yuv, past_bottom, nv21, va_cv::INTER_LINEAR); });
            thrown += throws([&] { call(yuv, column, nv21, va_cv::INTER_LINEAR); });
            thrown += throws([&] { call(yuv, negative, nv21, va_cv::INTER_LINEAR); });
            thrown += throws([&] { call(yuv, rects, va_cv::COLOR_YUV2BGRA_NV21, va_cv::INTER_LINEAR); });
            thrown += throws([&] { call(yuv, rects, va_cv::COLOR_YUV2BGR_YV12, va_cv::INTER_LINEAR); });
            thrown += throws([&] { call(bgr_frame, {VRect(0.f, 0.f, 4.f, 4.f)}, nv21, va_cv::INTER_LINEAR); });
        }
        expect(thrown == 20, "unsupported combinations throw");
        // per-image statistics
        expect(throws([&] { va_cv::cvt_color_crop_resize_normalize(yuv, out, rects, nv21, size); }) == 1,
               "per-image statistics throw");
        // ... and a rect that reaches the decoded frame's last row and column does not
        expect(throws([&] { va_cv::cvt_color_crop_resize(yuv, out, {VRect(150.f, 100.f, 160.f, 120.f)}, nv21, size); }) == 0,
               "a rect at the frame's edge is taken");
    } catch (const std::exception& e) {
        std::printf("exception: %s\n", e.what());
        return 2;
    }
    std::printf("cases %d failed %d\n", g_cases, g_failed);
    return g_failed ? 1 : 0;
}
