// One frame, many crops through the C++ layer: va_cv::warp_affine /
// warp_affine_normalize with a vector of matrices (one kernel launch) against
// the single-matrix overloads called once per crop, byte for byte.  Host
// operands (staged through the pinned pool) and device-resident ones.
// Built and run by tests/test_warp_rois_gpu.py; needs a HIP device.
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

static void run(const Tensor& frame, const std::vector<Tensor>& M, bool on_device, int border, const char* what) {
    const va_cv::VSize size(37, 53);
    va_cv::VScalar bv;
    bv.v0 = 7; bv.v1 = 99; bv.v2 = 200;
    Tensor mean(3, 1, 1, vision::FP32, vision::NCHW), stdv(3, 1, 1, vision::FP32, vision::NCHW);
    const float mv[3] = {104.5f, 117.25f, 123.f}, sv[3] = {57.375f, 57.12f, 58.395f};
    std::memcpy(mean.data, mv, sizeof(mv));
    std::memcpy(stdv.data, sv, sizeof(sv));

    std::vector<Tensor> crops, ncrops;
    va_cv::warp_affine(frame, crops, M, size, va_cv::INTER_LINEAR, border, bv);
    va_cv::warp_affine_normalize(frame, ncrops, M, size, va_cv::INTER_LINEAR, border, bv, mean, stdv);
    expect(crops.size() == M.size() && ncrops.size() == M.size(), what);
    for (size_t i = 0; i < M.size() && i < crops.size() && i < ncrops.size(); ++i) {
        Tensor one, none;
        va_cv::warp_affine(frame, one, M[i], size, va_cv::INTER_LINEAR, border, bv);
        va_cv::warp_affine_normalize(frame, none, M[i], size, va_cv::INTER_LINEAR, border, bv, mean, stdv);
        expect(crops[i].on_device() == on_device && ncrops[i].on_device() == on_device, "placement", (int)i);
        expect(crops[i].dtype == frame.dtype && ncrops[i].dtype == vision::FP32, "dtype", (int)i);
        expect(same_bytes(crops[i], one), what, (int)i);
        expect(same_bytes(ncrops[i], none), "normalize", (int)i);
    }
}

int main() {
    try {
        std::vector<Tensor> M;
        M.push_back(make_map(1.0f, 0.f, 80.f, 60.f, 18.f, 26.f));
        M.push_back(make_map(0.7f, 15.f, 40.f, 30.f, 18.f, 26.f));
        M.push_back(make_map(1.9f, -30.f, 120.f, 90.f, 18.f, 26.f));
        M.push_back(make_map(1.1f, 170.f, 5.f, 5.f, 18.f, 26.f));       // mostly off the frame
        M.push_back(make_map(0.5f, 45.f, 1000.f, 1000.f, 18.f, 26.f));  // all border
        for (vision::DType dt : {vision::INT8, vision::FP32}) {
            const Tensor frame = make_frame(160, 120, 3, dt);
            run(frame, M, false, va_cv::BORDER_CONSTANT, dt == vision::INT8 ? "host u8" : "host f32");
            run(frame, M, false, va_cv::BORDER_REPLICATE, "host, BORDER_REPLICATE");
            // device-resident frame, the matrices on the device too (all but one)
            const Tensor dframe = frame.to_device(0);
            std::vector<Tensor> dM;
            for (size_t i = 0; i < M.size(); ++i) dM.push_back(i == 2 ? M[i] : M[i].to_device(0));
            run(dframe, dM, true, va_cv::BORDER_CONSTANT, "device operands");
        }
        // refused loudly: no matrices, per-image statistics, BORDER_TRANSPARENT
        const Tensor frame = make_frame(160, 120, 3, vision::INT8);
        std::vector<Tensor> out;
        int thrown = 0;
        try { va_cv::warp_affine(frame, out, std::vector<Tensor>(), va_cv::VSize(8, 8)); } catch (const std::runtime_error&) { ++thrown; }
        try { va_cv::warp_affine_normalize(frame, out, M, va_cv::VSize(8, 8)); } catch (const std::runtime_error&) { ++thrown; }
        try { va_cv::warp_affine(frame, out, M, va_cv::VSize(8, 8), va_cv::INTER_LINEAR, va_cv::BORDER_TRANSPARENT); } catch (const std::runtime_error&) { ++thrown; }
        expect(thrown == 3, "unsupported combinations throw");
    } catch (const std::exception& e) {
        std::printf("exception: %s\n", e.what());
        return 2;
    }
    std::printf("cases %d failed %d\n", g_cases, g_failed);
    return g_failed ? 1 : 0;
}
