// One frame, many upright crops through the C++ layer: va_cv::crop_resize /
// crop_resize_normalize with a vector of rects (one kernel launch) against
// va_cv::crop followed by va_cv::resize / resize_normalize once per rect, byte
// for byte.  A host frame (staged through the pinned pool) and a
// device-resident one.  Built and run by tests/test_crop_resize_rois_gpu.py;
// needs a HIP device.
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
    Tensor mean(3, 1, 1, vision::FP32, vision::NCHW), stdv(3, 1, 1, vision::FP32, vision::NCHW);
    const float mv[3] = {104.5f, 117.25f, 123.f}, sv[3] = {57.375f, 57.12f, 58.395f};
    std::memcpy(mean.data, mv, sizeof(mv));
    std::memcpy(stdv.data, sv, sizeof(sv));

    std::vector<Tensor> crops, ncrops;
    va_cv::crop_resize(frame, crops, rects, size);
    va_cv::crop_resize_normalize(frame, ncrops, rects, size, va_cv::INTER_LINEAR, mean, stdv);
    expect(crops.size() == rects.size() && ncrops.size() == rects.size(), what);
    for (size_t i = 0; i < rects.size() && i < crops.size() && i < ncrops.size(); ++i) {
        Tensor cut, one, none;
        va_cv::crop(frame, cut, rects[i]);
        va_cv::resize(cut, one, size);
        va_cv::resize_normalize(cut, none, size, 0, 0, va_cv::INTER_LINEAR, mean, stdv);
        expect(crops[i].on_device() == on_device && ncrops[i].on_device() == on_device, "placement", (int)i);
        expect(crops[i].dtype == frame.dtype && ncrops[i].dtype == vision::FP32, "dtype", (int)i);
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
        rects.push_back(VRect(100.f, 80.f, 137.f, 109.f));     // the output's own size
        rects.push_back(VRect(158.f, 118.f, 160.f, 120.f));    // 2 x 2 in the corner
        rects.push_back(VRect(30.f, 5.f, 41.f, 100.f));        // 11 x 95
        for (vision::DType dt : {vision::INT8, vision::FP32}) {
            const Tensor frame = make_frame(160, 120, 3, dt);
            run(frame, rects, false, dt == vision::INT8 ? "host u8" : "host f32");
            run(frame.to_device(0), rects, true, "device frame");
        }
        // refused loudly
        const Tensor frame = make_frame(160, 120, 3, vision::INT8);
        const va_cv::VSize size(8, 8);
        std::vector<Tensor> out;
        int thrown = 0;
        thrown += throws([&] { va_cv::crop_resize(frame, out, std::vector<VRect>(), size); });   // no rects
        thrown += throws([&] { va_cv::crop_resize_normalize(frame, out, rects, size); });        // per-image statistics
        thrown += throws([&] { va_cv::crop_resize(frame, out, rects, size, va_cv::INTER_CUBIC); });
        thrown += throws([&] { va_cv::crop_resize(frame, out, rects, size, va_cv::INTER_NEAREST); });
        thrown += throws([&] { va_cv::crop_resize(frame, out, rects, va_cv::VSize(0, 8)); });
        thrown += throws([&] { va_cv::crop_resize(frame, out, {VRect(150.f, 0.f, 161.f, 10.f)}, size); });  // past the edge
        thrown += throws([&] { va_cv::crop_resize(frame, out, {VRect(5.f, 5.f, 6.f, 50.f)}, size); });      // one column
        thrown += throws([&] { va_cv::crop_resize(frame, out, {VRect(-1.f, 5.f, 6.f, 50.f)}, size); });
        Tensor chw(160, 120, 3, vision::INT8, vision::NCHW);
        thrown += throws([&] { va_cv::crop_resize(chw, out, rects, size); });                    // NCHW frame
        thrown += throws([&] { va_cv::crop_resize(make_frame(160, 120, 5, vision::INT8), out, rects, size); });
        expect(thrown == 10, "unsupported combinations throw");
    } catch (const std::exception& e) {
        std::printf("exception: %s\n", e.what());
        return 2;
    }
    std::printf("cases %d failed %d\n", g_cases, g_failed);
    return g_failed ? 1 : 0;
}
