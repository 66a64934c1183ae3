// One YUV420sp frame, many template matches through the C++ layer:
// va_cv::cvt_color_match_template (one kernel launch, no decoded frame) against
// va_cv::cvt_color followed by va_cv::match_template(src, targets, windows, ...)
// on the decoded frame, byte for byte.  A host frame (staged through the pinned
// pool) and a device-resident one, shared and per-window templates, peaks on
// and off, and the conditions that throw.
// Built and run by tests/test_yuv_match_rois_gpu.py; needs a HIP device.
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
        std::printf("FAIL %s (window %d)\n", what, i);
    }
}

static Tensor make_u8(int w, int h, int c, unsigned seed) {
    Tensor t(w, h, c, vision::INT8, vision::NHWC);
    unsigned s = seed;
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

static void run(const Tensor& yuv, const std::vector<Tensor>& targets, const std::vector<VRect>& windows,
                bool on_device, int code, const char* what) {
    Tensor bgr;
    va_cv::cvt_color(yuv, bgr, code);
    for (int method = va_cv::TM_SQDIFF; method <= va_cv::TM_CCOEFF_NORMED; ++method) {
        std::vector<Tensor> maps, only, want;
        std::vector<va_cv::VMatchPeak> peaks, wpeaks;
        va_cv::cvt_color_match_template(yuv, targets, windows, maps, code, method, &peaks);
        va_cv::cvt_color_match_template(yuv, targets, windows, only, code, method);
        va_cv::match_template(bgr, targets, windows, want, method, &wpeaks);
        const size_t n = windows.size();
        expect(maps.size() == n && only.size() == n && peaks.size() == n && want.size() == n && wpeaks.size() == n, what);
        if (maps.size() != n || only.size() != n || peaks.size() != n || want.size() != n || wpeaks.size() != n) continue;
        for (size_t i = 0; i < n; ++i) {
            expect(maps[i].on_device() == on_device && only[i].on_device() == on_device, "placement", (int)i);
            expect(maps[i].dtype == vision::FP32 && maps[i].c == 1, "dtype", (int)i);
            expect(same_bytes(maps[i], want[i]), what, (int)i);
            expect(same_bytes(only[i], want[i]), "without peaks", (int)i);
            // the peaks are plain values: compare their bytes (a NaN would differ from itself)
            expect(std::memcmp(&peaks[i].minVal, &wpeaks[i].minVal, sizeof(double)) == 0 &&
                       std::memcmp(&peaks[i].maxVal, &wpeaks[i].maxVal, sizeof(double)) == 0,
                   "peak values", (int)i);
            expect(std::memcmp(peaks[i].minIdx, wpeaks[i].minIdx, sizeof(peaks[i].minIdx)) == 0 &&
                       std::memcmp(peaks[i].maxIdx, wpeaks[i].maxIdx, sizeof(peaks[i].maxIdx)) == 0,
                   "peak indices", (int)i);
        }
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
        std::vector<VRect> windows;  // all 40 x 30 once truncated; the decoded frame is 160 x 120
        windows.push_back(VRect(0.f, 0.f, 40.f, 30.f));          // a corner
        windows.push_back(VRect(11.9f, 21.9f, 51.95f, 51.95f));  // fractional: (11, 21), odd left and top
        windows.push_back(VRect(120.f, 90.f, 160.f, 120.f));     // the far corner: the last chroma pair
        windows.push_back(VRect(12.f, 21.f, 52.f, 51.f));        // overlaps the second; even left, odd top
        windows.push_back(VRect(119.f, 88.f, 159.f, 118.f));     // odd left, even top
        std::vector<Tensor> per, shared;
        for (unsigned i = 0; i < 5; ++i) per.push_back(make_u8(9, 7, 3, 77u + i));
        shared.push_back(per[2]);
        const Tensor yuv = make_u8(160, 180, 1, 4321u);
        const int nv21 = va_cv::COLOR_YUV2BGR_NV21;
        run(yuv, per, windows, false, nv21, "host NV21 -> BGR, a template per window");
        run(yuv, shared, windows, false, va_cv::COLOR_YUV2RGB_NV12, "host NV12 -> RGB, shared template");
        const Tensor dyuv = yuv.to_device(0);
        std::vector<Tensor> dper;
        for (const Tensor& t : per) dper.push_back(t.to_device(0));
        run(dyuv, dper, windows, true, va_cv::COLOR_YUV2RGB_NV21, "device NV21 -> RGB, device templates");
        run(dyuv, shared, windows, true, va_cv::COLOR_YUV2BGR_NV12, "device NV12 -> BGR, host template");
        dper[1] = per[1];
        run(yuv, dper, windows, false, nv21, "host frame, mixed templates");

        // refused loudly, as match_template(src, targets, windows, ...) refuses
        std::vector<Tensor> out;
        const int sq = va_cv::TM_SQDIFF;
        int thrown = 0;
        thrown += throws([&] { va_cv::cvt_color_match_template(yuv, per, std::vector<VRect>(), out, nv21, sq); });
        thrown += throws([&] { va_cv::cvt_color_match_template(yuv, std::vector<Tensor>(per.begin(), per.begin() + 2),
                                                               windows, out, nv21, sq); });     // 2 templates, 5 windows
        std::vector<VRect> w2 = windows;
        w2[3] = VRect(11.f, 20.f, 52.f, 50.f);                                                  // 41 wide
        thrown += throws([&] { va_cv::cvt_color_match_template(yuv, per, w2, out, nv21, sq); });
        w2[3] = VRect(121.f, 90.f, 161.f, 120.f);                                               // past the right edge
        thrown += throws([&] { va_cv::cvt_color_match_template(yuv, per, w2, out, nv21, sq); });
        w2[3] = VRect(120.f, 91.f, 160.f, 121.f);                                               // into the chroma rows
        thrown += throws([&] { va_cv::cvt_color_match_template(yuv, per, w2, out, nv21, sq); });
        w2[3] = VRect(-1.f, 0.f, 39.f, 30.f);
        thrown += throws([&] { va_cv::cvt_color_match_template(yuv, per, w2, out, nv21, sq); });
        std::vector<Tensor> odd = per;
        odd[2] = make_u8(8, 7, 3, 5u);                                                          // templates of two sizes
        thrown += throws([&] { va_cv::cvt_color_match_template(yuv, odd, windows, out, nv21, sq); });
        odd[2] = make_u8(9, 7, 1, 5u);                                                          // ... of the YUV frame's one channel
        thrown += throws([&] { va_cv::cvt_color_match_template(yuv, odd, windows, out, nv21, sq); });
        std::vector<Tensor> big(1, make_u8(41, 7, 3, 5u));                                      // wider than the window
        thrown += throws([&] { va_cv::cvt_color_match_template(yuv, big, windows, out, nv21, sq); });
        thrown += throws([&] { va_cv::cvt_color_match_template(yuv, shared, windows, out, nv21, 6); });   // no such method
        thrown += throws([&] { va_cv::cvt_color_match_template(yuv, shared, windows, out, va_cv::COLOR_YUV2BGRA_NV21, sq); });
        thrown += throws([&] { va_cv::cvt_color_match_template(yuv, shared, windows, out, va_cv::COLOR_YUV2BGR_YV12, sq); });
        thrown += throws([&] { va_cv::cvt_color_match_template(make_u8(160, 120, 3, 1u), shared, windows, out, nv21, sq); });
        Tensor f32(160, 180, 1, vision::FP32, vision::NHWC);
        thrown += throws([&] { va_cv::cvt_color_match_template(f32, shared, windows, out, nv21, sq); });
        thrown += throws([&] { va_cv::cvt_color_match_template(make_u8(159, 180, 1, 1u), shared, windows, out, nv21, sq); });
        expect(thrown == 15, "unsupported combinations throw");
    } catch (const std::exception& e) {
        std::printf("exception: %s\n", e.what());
        return 2;
    }
    std::printf("cases %d failed %d\n", g_cases, g_failed);
    return g_failed ? 1 : 0;
}
