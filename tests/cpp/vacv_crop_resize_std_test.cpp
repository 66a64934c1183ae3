// One frame, many upright crops standardized by their own statistics through
// the C++ layer: va_cv::crop_resize_standardize with a vector of rects (one
// kernel launch) against va_cv::crop, va_cv::resize and va_cv::normalize with
// mean and stddev left empty once per rect, bit for bit; the statistics against
// va_cv::mean_stddev of the resized crop.  A host frame (staged through the
// pinned pool) and a device-resident one.  Built and run by
// tests/test_crop_resize_rois_std_gpu.py; needs a HIP device.
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

static Tensor make_frame(int w, int h, int c, vision::DType dt) {
    Tensor t(w, h, c, dt, vision::NHWC);
    unsigned s = 12345u;
    for (size_t i = 0; i < t.size(); ++i) {
        s = s * 1664525u + 1013904223u;
        const unsigned v = (s >> 24) & 0xFFu;
        if (dt == vision::INT8) static_cast<unsigned char*>(t.data)[i] = (unsigned char)v;
        else static_cast<float*>(t.data)[i] = (float)v * 0.75f + 0.125f;
    }
    return t;
}

static bool same_bytes(const Tensor& a, const Tensor& b) {
    const Tensor x = a.to_host(), y = b.to_host();
    return x.w == y.w && x.h == y.h && x.c == y.c && x.dtype == y.dtype && x.layout == y.layout && x.len() == y.len() &&
           std::memcmp(x.data, y.data, x.len()) == 0;
}

static void run(const Tensor& frame, const std::vector<VRect>& rects, bool on_device, const char* what) {
    const va_cv::VSize size(37, 29);
    const int c = frame.c;
    std::vector<Tensor> crops, again, stats;
    va_cv::crop_resize_standardize(frame, crops, rects, size, va_cv::INTER_LINEAR, &stats);
    va_cv::crop_resize_standardize(frame, again, rects, size);  // without the statistics: the same crops
    expect(crops.size() == rects.size() && again.size() == rects.size(), what);
    expect(stats.size() == 2, "two statistics tensors");
    if (stats.size() != 2) return;
    for (int k = 0; k < 2; ++k)
        expect(!stats[k].on_device() && stats[k].dtype == vision::FP32 && stats[k].w == c &&
                   stats[k].h == (int)rects.size(),
               "statistics: host FP32 (c, n)");
    for (size_t i = 0; i < rects.size() && i < crops.size() && i < again.size(); ++i) {
        Tensor cut, one, none, mean, stdv;
        va_cv::crop(frame, cut, rects[i]);
        va_cv::resize(cut, one, size);
        va_cv::normalize(one, none);  // mean and stddev empty: the crop's own statistics
        va_cv::mean_stddev(one, mean, stdv);
        const Tensor mh = mean.to_host(), sh = stdv.to_host();
        expect(crops[i].on_device() == on_device && crops[i].dtype == vision::FP32, "placement and dtype", (int)i);
        expect(same_bytes(crops[i], none), what, (int)i);
        expect(same_bytes(again[i], none), "without statistics", (int)i);
        expect(std::memcmp(static_cast<const float*>(stats[0].data) + i * c, mh.data, c * sizeof(float)) == 0, "mean",
               (int)i);
        expect(std::memcmp(static_cast<const float*>(stats[1].data) + i * c, sh.data, c * sizeof(float)) == 0,
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
        rects.push_back(VRect(100.f, 80.f, 137.f, 109.f));     // the output's own size
        rects.push_back(VRect(158.f, 118.f, 160.f, 120.f));    // 2 x 2 in the corner
        rects.push_back(VRect(30.f, 5.f, 41.f, 100.f));        // 11 x 95
        for (int c : {3, 1}) {
            const Tensor frame = make_frame(160, 120, c, vision::INT8);
            run(frame, rects, false, c == 3 ? "host u8 c3" : "host u8 c1");
            run(frame.to_device(0), rects, true, "device frame");
        }
        // refused loudly
        const Tensor frame = make_frame(160, 120, 3, vision::INT8);
        const va_cv::VSize size(8, 8);
        std::vector<Tensor> out;
        int thrown = 0;
        thrown += throws([&] { va_cv::crop_resize_standardize(frame, out, std::vector<VRect>(), size); });  // no rects
        thrown += throws([&] { va_cv::crop_resize_standardize(make_frame(160, 120, 3, vision::FP32), out, rects, size); });
        thrown += throws([&] { va_cv::crop_resize_standardize(frame, out, rects, size, va_cv::INTER_CUBIC); });
        thrown += throws([&] { va_cv::crop_resize_standardize(frame, out, rects, va_cv::VSize(0, 8)); });
        thrown += throws([&] { va_cv::crop_resize_standardize(frame, out, rects, va_cv::VSize(145, 144)); });  // past the LDS limit
        thrown += throws([&] { va_cv::crop_resize_standardize(frame, out, {VRect(150.f, 0.f, 161.f, 10.f)}, size); });
        thrown += throws([&] { va_cv::crop_resize_standardize(frame, out, {VRect(5.f, 5.f, 6.f, 50.f)}, size); });
        Tensor chw(160, 120, 3, vision::INT8, vision::NCHW);
        thrown += throws([&] { va_cv::crop_resize_standardize(chw, out, rects, size); });                     // NCHW frame
        expect(thrown == 8, "unsupported combinations throw");
        va_cv::crop_resize_standardize(frame, out, rects, va_cv::VSize(144, 144));  // exactly 64 KiB of LDS
        expect(out.size() == rects.size() && out[0].w == 144 && out[0].h == 144, "144 x 144 x 3 fits");
    } catch (const std::exception& e) {
        std::printf("exception: %s\n", e.what());
        return 2;
    }
    std::printf("cases %d failed %d\n", g_cases, g_failed);
    return g_failed ? 1 : 0;
}
