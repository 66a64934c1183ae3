// One YUV420sp frame, many upright crops standardized by their own statistics
// through the C++ layer: va_cv::cvt_color_crop_resize_standardize (one kernel
// launch, no decoded frame, no crops) against va_cv::cvt_color followed by
// va_cv::crop_resize_standardize on the decoded frame, and against
// va_cv::crop, va_cv::resize and va_cv::normalize with mean and stddev left
// empty once per rect, bit for bit; the statistics too.  A host frame (staged
// through the pinned pool) and a device-resident one.  Built and run by
// tests/test_yuv_crop_resize_rois_std_gpu.py; needs a HIP device.
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
    std::vector<Tensor> crops, again, chain, stats, chain_stats;
    va_cv::cvt_color_crop_resize_standardize(yuv, crops, rects, code, size, va_cv::INTER_LINEAR, &stats);
    va_cv::cvt_color_crop_resize_standardize(yuv, again, rects, code, size);  // without the statistics: the same crops
    Tensor bgr;
    va_cv::cvt_color(yuv, bgr, code);
    va_cv::crop_resize_standardize(bgr, chain, rects, size, va_cv::INTER_LINEAR, &chain_stats);
    expect(crops.size() == rects.size() && again.size() == rects.size() && chain.size() == rects.size(), what);
    expect(stats.size() == 2 && chain_stats.size() == 2, "two statistics tensors");
    if (stats.size() != 2 || chain_stats.size() != 2) return;
    for (int k = 0; k < 2; ++k) {
        expect(!stats[k].on_device() && stats[k].dtype == vision::FP32 && stats[k].w == 3 &&
                   stats[k].h == (int)rects.size(),
               "statistics: host FP32 (3, n)");
        expect(same_bytes(stats[k], chain_stats[k]), k ? "stddev vs the chain" : "mean vs the chain");
    }
    for (size_t i = 0; i < rects.size() && i < crops.size() && i < again.size() && i < chain.size(); ++i) {
        Tensor cut, one, none, mean, stdv;
        va_cv::crop(bgr, cut, rects[i]);
        va_cv::resize(cut, one, size);
        va_cv::normalize(one, none);  // mean and stddev empty: the crop's own statistics
        va_cv::mean_stddev(one, mean, stdv);
        const Tensor mh = mean.to_host(), sh = stdv.to_host();
        expect(crops[i].on_device() == on_device && crops[i].dtype == vision::FP32 && crops[i].c == 3,
               "placement and dtype", (int)i);
        expect(same_bytes(crops[i], chain[i]), "vs cvt_color + crop_resize_standardize", (int)i);
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
        std::vector<Tensor> out;
        const Tensor bgr_frame(16, 12, 3, vision::INT8, vision::NHWC);
        auto call = [&](const Tensor& src, const std::vector<VRect>& r, int code, va_cv::VSize sz,
                        int interpolation = va_cv::INTER_LINEAR) {
            va_cv::cvt_color_crop_resize_standardize(src, out, r, code, sz, interpolation);
        };
        int thrown = 0;
        thrown += throws([&] { call(yuv, rects, nv21, va_cv::VSize(145, 144)); });  // past the LDS limit
        thrown += throws([&] { call(yuv, rects, va_cv::COLOR_YUV2BGRA_NV21, size); });
        thrown += throws([&] { call(yuv, rects, va_cv::COLOR_YUV2BGR_YV12, size); });
        expect(thrown == 3, "an oversize dsize and a bad code throw");
        thrown = 0;
        thrown += throws([&] { call(yuv, std::vector<VRect>(), nv21, size); });  // no rects
        thrown += throws([&] { call(yuv, rects, nv21, size, va_cv::INTER_CUBIC); });
        thrown += throws([&] { call(yuv, rects, nv21, va_cv::VSize(0, 8)); });
        thrown += throws([&] { call(yuv, {VRect(150.f, 0.f, 161.f, 10.f)}, nv21, size); });   // past the right edge
        thrown += throws([&] { call(yuv, {VRect(0.f, 100.f, 10.f, 121.f)}, nv21, size); });   // into the chroma rows
        thrown += throws([&] { call(yuv, {VRect(5.f, 5.f, 6.f, 50.f)}, nv21, size); });       // one column
        thrown += throws([&] { call(bgr_frame, {VRect(0.f, 0.f, 4.f, 4.f)}, nv21, size); });  // no YUV420sp frame
        expect(thrown == 7, "unsupported combinations throw");
        call(yuv, rects, nv21, va_cv::VSize(144, 144));  // exactly 64 KiB of LDS
        expect(out.size() == rects.size() && out[0].w == 144 && out[0].h == 144 && out[0].c == 3, "144 x 144 fits");
    } catch (const std::exception& e) {
        std::printf("exception: %s\n", e.what());
        return 2;
    }
    std::printf("cases %d failed %d\n", g_cases, g_failed);
    return g_failed ? 1 : 0;
}
