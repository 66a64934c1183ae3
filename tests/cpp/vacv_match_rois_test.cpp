// One frame, many template matches through the C++ layer: va_cv::match_template
// with a vector of windows (one kernel launch, peaks included) against
// va_cv::crop, va_cv::match_template and va_cv::minMaxIdx once per window, byte
// for byte.  A host frame (staged through the pinned pool) and a
// device-resident one, shared and per-window templates, peaks on and off.
// Built and run by tests/test_match_rois_gpu.py; needs a HIP device.
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

static void run(const Tensor& frame, const std::vector<Tensor>& targets, const std::vector<VRect>& windows,
                bool on_device, const char* what) {
    for (int method = va_cv::TM_SQDIFF; method <= va_cv::TM_CCOEFF_NORMED; ++method) {
        std::vector<Tensor> maps, only;
        std::vector<va_cv::VMatchPeak> peaks;
        va_cv::match_template(frame, targets, windows, maps, method, &peaks);
        va_cv::match_template(frame, targets, windows, only, method);
        expect(maps.size() == windows.size() && only.size() == windows.size() && peaks.size() == windows.size(), what);
        for (size_t i = 0; i < windows.size() && i < maps.size() && i < only.size() && i < peaks.size(); ++i) {
            Tensor cut, one;
            va_cv::crop(frame, cut, windows[i]);
            va_cv::match_template(cut, targets[targets.size() == 1 ? 0 : i], one, method);
            double mn = -1, mx = -1;
            int imn[2] = {-2, -2}, imx[2] = {-2, -2};
            va_cv::minMaxIdx(one, &mn, &mx, imn, imx);
            expect(maps[i].on_device() == on_device && only[i].on_device() == on_device, "placement", (int)i);
            expect(same_bytes(maps[i], one), what, (int)i);
            expect(same_bytes(only[i], one), "without peaks", (int)i);
            const va_cv::VMatchPeak& p = peaks[i];
            expect(std::memcmp(&p.minVal, &mn, sizeof(mn)) == 0 && std::memcmp(&p.maxVal, &mx, sizeof(mx)) == 0,
                   "peak values", (int)i);
            expect(p.minIdx[0] == imn[0] && p.minIdx[1] == imn[1] && p.maxIdx[0] == imx[0] && p.maxIdx[1] == imx[1],
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
        std::vector<VRect> windows;  // all 40 x 30 once truncated
        windows.push_back(VRect(0.f, 0.f, 40.f, 30.f));          // a corner
        windows.push_back(VRect(10.9f, 20.9f, 50.95f, 50.95f));  // fractional: (10, 20), 40.05 x 30.05
        windows.push_back(VRect(120.f, 90.f, 160.f, 120.f));     // the far corner
        windows.push_back(VRect(11.f, 20.f, 51.f, 50.f));        // overlaps the second
        std::vector<Tensor> per, shared;
        for (unsigned i = 0; i < 4; ++i) per.push_back(make_u8(9, 7, 3, 77u + i));
        shared.push_back(per[2]);
        const Tensor frame = make_u8(160, 120, 3, 12345u);
        run(frame, per, windows, false, "host frame, a template per window");
        run(frame, shared, windows, false, "host frame, shared template");
        const Tensor dframe = frame.to_device(0);
        std::vector<Tensor> dper;
        for (const Tensor& t : per) dper.push_back(t.to_device(0));
        run(dframe, dper, windows, true, "device frame, device templates");
        run(dframe, shared, windows, true, "device frame, host template");
        dper[1] = per[1];
        run(frame, dper, windows, false, "host frame, mixed templates");

        // refused loudly
        std::vector<Tensor> out;
        int thrown = 0;
        thrown += throws([&] { va_cv::match_template(frame, per, std::vector<VRect>(), out, va_cv::TM_SQDIFF); });
        thrown += throws([&] { va_cv::match_template(frame, std::vector<Tensor>(per.begin(), per.begin() + 2), windows, out,
                                                     va_cv::TM_SQDIFF); });                     // 2 templates, 4 windows
        std::vector<VRect> w2 = windows;
        w2[3] = VRect(11.f, 20.f, 52.f, 50.f);                                                  // 41 wide
        thrown += throws([&] { va_cv::match_template(frame, per, w2, out, va_cv::TM_SQDIFF); });
        w2[3] = VRect(121.f, 90.f, 161.f, 120.f);                                               // past the edge
        thrown += throws([&] { va_cv::match_template(frame, per, w2, out, va_cv::TM_SQDIFF); });
        w2[3] = VRect(-1.f, 0.f, 39.f, 30.f);
        thrown += throws([&] { va_cv::match_template(frame, per, w2, out, va_cv::TM_SQDIFF); });
        std::vector<Tensor> odd = per;
        odd[2] = make_u8(8, 7, 3, 5u);                                                          // templates of two sizes
        thrown += throws([&] { va_cv::match_template(frame, odd, windows, out, va_cv::TM_SQDIFF); });
        odd[2] = make_u8(9, 7, 1, 5u);                                                          // ... of other channels
        thrown += throws([&] { va_cv::match_template(frame, odd, windows, out, va_cv::TM_SQDIFF); });
        std::vector<Tensor> big(1, make_u8(41, 7, 3, 5u));                                      // wider than the window
        thrown += throws([&] { va_cv::match_template(frame, big, windows, out, va_cv::TM_SQDIFF); });
        thrown += throws([&] { va_cv::match_template(frame, shared, windows, out, 6); });       // no such method
        Tensor f32(160, 120, 3, vision::FP32, vision::NHWC);
        thrown += throws([&] { va_cv::match_template(f32, shared, windows, out, va_cv::TM_SQDIFF); });
        Tensor chw(160, 120, 3, vision::INT8, vision::NCHW);
        thrown += throws([&] { va_cv::match_template(chw, shared, windows, out, va_cv::TM_SQDIFF); });
        expect(thrown == 11, "unsupported combinations throw");
    } catch (const std::exception& e) {
        std::printf("exception: %s\n", e.what());
        return 2;
    }
    std::printf("cases %d failed %d\n", g_cases, g_failed);
    return g_failed ? 1 : 0;
}
