// One YUV420sp frame, many crops through the C++ layer:
// va_cv::cvt_color_warp_affine / cvt_color_warp_affine_normalize (one kernel
// launch, no decoded frame) against va_cv::cvt_color followed by the vector
// warp_affine / warp_affine_normalize overloads, byte for byte.  Host operands
// (staged through the pinned pool) and device-resident ones.
// Built and run by tests/test_yuv_rois_gpu.py; needs a HIP device.
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

static void run(const Tensor& yuv, const std::vector<Tensor>& M, bool on_device, int code, int border, const char* what) {
    const va_cv::VSize size(37, 53);
    va_cv::VScalar bv;
    bv.v0 = 7; bv.v1 = 99; bv.v2 = 200;
    Tensor mean(3, 1, 1, vision::FP32, vision::NCHW), stdv(3, 1, 1, vision::FP32, vision::NCHW);
    const float mv[3] = {104.5f, 117.25f, 123.f}, sv[3] = {57.375f, 57.12f, 58.395f};
    std::memcpy(mean.data, mv, sizeof(mv));
    std::memcpy(stdv.data, sv, sizeof(sv));

    std::vector<Tensor> crops, ncrops, want, nwant;
    va_cv::cvt_color_warp_affine(yuv, crops, M, code, size, va_cv::INTER_LINEAR, border, bv);
    va_cv::cvt_color_warp_affine_normalize(yuv, ncrops, M, code, size, va_cv::INTER_LINEAR, border, bv, mean, stdv);
    Tensor bgr;
    va_cv::cvt_color(yuv, bgr, code);
    va_cv::warp_affine(bgr, want, M, size, va_cv::INTER_LINEAR, border, bv);
    va_cv::warp_affine_normalize(bgr, nwant, M, size, va_cv::INTER_LINEAR, border, bv, mean, stdv);
    expect(crops.size() == M.size() && ncrops.size() == M.size() && want.size() == M.size() && nwant.size() == M.size(),
           what);
    for (size_t i = 0; i < M.size() && i < crops.size() && i < ncrops.size() && i < want.size() && i < nwant.size(); ++i) {
        expect(crops[i].on_device() == on_device && ncrops[i].on_device() == on_device, "placement", (int)i);
        expect(crops[i].dtype == vision::INT8 && ncrops[i].dtype == vision::FP32 && crops[i].c == 3, "dtype", (int)i);
        expect(same_bytes(crops[i], want[i]), what, (int)i);
        expect(same_bytes(ncrops[i], nwant[i]), "normalize", (int)i);
    }
}

int main() {
    try {
        std::vector<Tensor> M;
        M.push_back(make_map(1.0f, 0.f, 80.f, 60.f, 18.f, 26.f));
        M.push_back(make_map(0.7f, 15.f, 40.f, 30.f, 18.f, 26.f));
        M.push_back(make_map(1.9f, -30.f, 120.f, 90.f, 18.f, 26.f));
        M.push_back(make_map(1.0f, 0.f, 150.f, 110.f, 18.f, 26.f));     // the frame's bottom-right corner
        M.push_back(make_map(1.1f, 170.f, 5.f, 5.f, 18.f, 26.f));       // mostly off the frame
        M.push_back(make_map(0.5f, 45.f, 1000.f, 1000.f, 18.f, 26.f));  // all border
        const Tensor yuv = make_yuv(160, 120);
        run(yuv, M, false, va_cv::COLOR_YUV2BGR_NV21, va_cv::BORDER_CONSTANT, "host NV21 -> BGR");
        run(yuv, M, false, va_cv::COLOR_YUV2RGB_NV12, va_cv::BORDER_REPLICATE, "host NV12 -> RGB, BORDER_REPLICATE");
        // device-resident frame, the matrices on the device too (all but one)
        const Tensor dyuv = yuv.to_device(0);
        std::vector<Tensor> dM;
        for (size_t i = 0; i < M.size(); ++i) dM.push_back(i == 2 ? M[i] : M[i].to_device(0));
        run(dyuv, dM, true, va_cv::COLOR_YUV2BGR_NV21, va_cv::BORDER_CONSTANT, "device operands");
        run(dyuv, dM, true, va_cv::COLOR_YUV2RGB_NV21, va_cv::BORDER_REFLECT_101, "device operands, BORDER_REFLECT_101");
        // refused loudly: no matrices, per-image statistics, BORDER_TRANSPARENT, OpenCV's codes, a BGR frame
        std::vector<Tensor> out;
        const va_cv::VSize s8(8, 8);
        int thrown = 0;
        try { va_cv::cvt_color_warp_affine(yuv, out, std::vector<Tensor>(), va_cv::COLOR_YUV2BGR_NV21, s8); } catch (const std::runtime_error&) { ++thrown; }
        try { va_cv::cvt_color_warp_affine_normalize(yuv, out, M, va_cv::COLOR_YUV2BGR_NV21, s8); } catch (const std::runtime_error&) { ++thrown; }
        try { va_cv::cvt_color_warp_affine(yuv, out, M, va_cv::COLOR_YUV2BGR_NV21, s8, va_cv::INTER_LINEAR, va_cv::BORDER_TRANSPARENT); } catch (const std::runtime_error&) { ++thrown; }
        try { va_cv::cvt_color_warp_affine(yuv, out, M, va_cv::COLOR_YUV2BGRA_NV21, s8); } catch (const std::runtime_error&) { ++thrown; }
        try { va_cv::cvt_color_warp_affine(Tensor(16, 12, 3, vision::INT8, vision::NHWC), out, M, va_cv::COLOR_YUV2BGR_NV21, s8); } catch (const std::runtime_error&) { ++thrown; }
        expect(thrown == 5, "unsupported combinations throw");
    } catch (const std::exception& e) {
        std::printf("exception: %s\n", e.what());
        return 2;
    }
    std::printf("cases %d failed %d\n", g_cases, g_failed);
    return g_failed ? 1 : 0;
}
