// One frame, many projective crops through the C++ layer: va_cv::
// warp_perspective / warp_perspective_normalize with a vector of homographies
// (one kernel launch) and the single-image overload against the C ABI called
// directly (vacv_warp_perspective_rois[_normalize]), byte for byte.  Host
// operands (staged through the pinned pool) and device-resident ones.
// Built and run by tests/test_warp_persp_rois_gpu.py; needs a HIP device.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <vector>

#include "cv/cv.h"
#include "vacv_hip.h"

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

// the FORWARD map of the frame's quad (TL, TR, BR, BL) onto the w x h crop
static Tensor quad_map(const float quad[8], int w, int h) {
    const float rect[8] = {0.f, 0.f, (float)(w - 1), 0.f, (float)(w - 1), (float)(h - 1), 0.f, (float)(h - 1)};
    Tensor m;
    va_cv::get_perspective_transform(quad, rect, m);
    return m;
}

static bool same_bytes(const Tensor& a, const void* b, size_t len) {
    const Tensor x = a.to_host();
    return x.len() == len && std::memcmp(x.data, b, len) == 0;
}

static const int kW = 37, kH = 53;

// the C ABI's bytes for all crops: device frame, device matrices, dense device output
static Tensor abi(const Tensor& frame, const std::vector<Tensor>& M, int flags, int border, const double bv[4],
                  const float* mean, const float* stdv) {
    const Tensor dframe = frame.on_device() ? frame : frame.to_device(0);
    const int n = (int)M.size();
    Tensor hm(9, n, 1, vision::FP32, vision::NCHW);
    for (int i = 0; i < n; ++i) {
        const Tensor m = M[i].to_host();
        std::memcpy(static_cast<float*>(hm.data) + 9 * i, m.data, 9 * sizeof(float));
    }
    const Tensor dm = hm.to_device(0);
    const vision::DType odt = mean ? vision::FP32 : frame.dtype;
    Tensor out;
    out.create_on(0, kW, kH * n, frame.c, odt, vision::NHWC);  // n dense crops back to back
    const vacv_image sd = {dframe.data, 1, frame.w, frame.h, frame.c, frame.dtype == vision::INT8 ? VACV_INT8 : VACV_FP32,
                           VACV_NHWC, 0, 0, 0};
    const vacv_image dd = {out.data, n, kW, kH, frame.c, odt == vision::INT8 ? VACV_INT8 : VACV_FP32, VACV_NHWC, 0, 0, 0};
    const int st = mean ? vacv_warp_perspective_rois_normalize(&sd, &dd, static_cast<const float*>(dm.data), nullptr, flags,
                                                               border, bv, mean, stdv, nullptr)
                        : vacv_warp_perspective_rois(&sd, &dd, static_cast<const float*>(dm.data), nullptr, flags,
                                                     border, bv, nullptr);
    if (st != VACV_OK) throw std::runtime_error("the C ABI refused the call");
    if (vacv_stream_synchronize(nullptr) != VACV_OK) throw std::runtime_error("synchronize");
    return out.to_host();
}

static void run(const Tensor& frame, const std::vector<Tensor>& M, bool on_device, int flags, int border,
                const char* what) {
    const va_cv::VSize size(kW, kH);
    va_cv::VScalar bv;
    bv.v0 = 7; bv.v1 = 99; bv.v2 = 200;
    const double bvd[4] = {7, 99, 200, 0};
    Tensor mean(3, 1, 1, vision::FP32, vision::NCHW), stdv(3, 1, 1, vision::FP32, vision::NCHW);
    const float mv[3] = {104.5f, 117.25f, 123.f}, sv[3] = {57.375f, 57.12f, 58.395f};
    std::memcpy(mean.data, mv, sizeof(mv));
    std::memcpy(stdv.data, sv, sizeof(sv));

    std::vector<Tensor> crops, ncrops;
    va_cv::warp_perspective(frame, crops, M, size, flags, border, bv);
    va_cv::warp_perspective_normalize(frame, ncrops, M, size, flags, border, bv, mean, stdv);
    expect(crops.size() == M.size() && ncrops.size() == M.size(), what);
    const Tensor want = abi(frame, M, flags, border, bvd, nullptr, nullptr);
    const Tensor nwant = abi(frame, M, flags, border, bvd, mv, sv);
    const size_t roi = (size_t)kW * kH * frame.c;
    const size_t esz = frame.dtype == vision::INT8 ? 1 : 4;
    bool any = false;  // some crop is not all border
    for (size_t i = 0; i < M.size() && i < crops.size() && i < ncrops.size(); ++i) {
        expect(crops[i].on_device() == on_device && ncrops[i].on_device() == on_device, "placement", (int)i);
        expect(crops[i].dtype == frame.dtype && ncrops[i].dtype == vision::FP32, "dtype", (int)i);
        expect(crops[i].w == kW && crops[i].h == kH && crops[i].c == frame.c, "shape", (int)i);
        expect(same_bytes(crops[i], static_cast<const unsigned char*>(want.data) + i * roi * esz, roi * esz), what, (int)i);
        expect(same_bytes(ncrops[i], static_cast<const unsigned char*>(nwant.data) + i * roi * 4, roi * 4), "normalize",
               (int)i);
        Tensor one;
        va_cv::warp_perspective(frame, one, M[i], size, flags, border, bv);
        expect(one.on_device() == on_device, "single image: placement", (int)i);
        expect(same_bytes(one, static_cast<const unsigned char*>(want.data) + i * roi * esz, roi * esz), "single image",
               (int)i);
        const Tensor h = crops[i].to_host();
        const unsigned char* p = static_cast<const unsigned char*>(h.data);
        for (size_t k = esz * (size_t)frame.c; k < roi * esz; ++k) any = any || p[k] != p[k % (esz * frame.c)];
    }
    expect(any, "the crops show the frame");
}

int main() {
    try {
        const float quads[4][8] = {{20.f, 15.f, 120.f, 25.f, 130.f, 100.f, 15.f, 90.f},
                                   {60.f, 5.f, 150.f, 40.f, 110.f, 115.f, 30.f, 70.f},
                                   {-40.f, -30.f, 70.f, -10.f, 80.f, 60.f, -30.f, 70.f},        // hangs off the corner
                                   {1000.f, 1000.f, 1100.f, 1010.f, 1090.f, 1120.f, 990.f, 1100.f}};  // all border
        std::vector<Tensor> M;
        for (const auto& q : quads) M.push_back(quad_map(q, kW, kH));
        // the corners of the crop land on the quad (forward map: quad -> rect)
        {
            const float* m = static_cast<const float*>(M[0].data);
            const float x = quads[0][4], y = quads[0][5];
            const double w = m[6] * x + m[7] * y + m[8];
            expect(std::fabs((m[0] * x + m[1] * y + m[2]) / w - (kW - 1)) < 0.01 &&
                   std::fabs((m[3] * x + m[4] * y + m[5]) / w - (kH - 1)) < 0.01 && m[8] == 1.f, "get_perspective_transform");
        }
        // dst -> src maps for WARP_INVERSE_MAP: the rect onto the quad
        std::vector<Tensor> Minv;
        const float rect[8] = {0.f, 0.f, (float)(kW - 1), 0.f, (float)(kW - 1), (float)(kH - 1), 0.f, (float)(kH - 1)};
        for (const auto& q : quads) {
            Tensor m;
            va_cv::get_perspective_transform(rect, q, m);
            Minv.push_back(m);
        }
        for (vision::DType dt : {vision::INT8, vision::FP32}) {
            const Tensor frame = make_frame(160, 120, 3, dt);
            run(frame, M, false, va_cv::INTER_LINEAR, va_cv::BORDER_CONSTANT, dt == vision::INT8 ? "host u8" : "host f32");
            run(frame, M, false, va_cv::INTER_LINEAR, va_cv::BORDER_REPLICATE, "host, BORDER_REPLICATE");
            run(frame, Minv, false, va_cv::INTER_LINEAR | va_cv::WARP_INVERSE_MAP, va_cv::BORDER_CONSTANT,
                "host, WARP_INVERSE_MAP");
            // device-resident frame, the matrices on the device too (all but one)
            const Tensor dframe = frame.to_device(0);
            std::vector<Tensor> dM;
            for (size_t i = 0; i < M.size(); ++i) dM.push_back(i == 2 ? M[i] : M[i].to_device(0));
            run(dframe, dM, true, va_cv::INTER_LINEAR, va_cv::BORDER_CONSTANT, "device operands");
        }
        // refused loudly: no matrices, per-image statistics, BORDER_TRANSPARENT, a 2x3 matrix, a degenerate quad
        const Tensor frame = make_frame(160, 120, 3, vision::INT8);
        std::vector<Tensor> out;
        int thrown = 0;
        try { va_cv::warp_perspective(frame, out, std::vector<Tensor>(), va_cv::VSize(8, 8)); } catch (const std::runtime_error&) { ++thrown; }
        try { va_cv::warp_perspective_normalize(frame, out, M, va_cv::VSize(8, 8)); } catch (const std::runtime_error&) { ++thrown; }
        try { va_cv::warp_perspective(frame, out, M, va_cv::VSize(8, 8), va_cv::INTER_LINEAR, va_cv::BORDER_TRANSPARENT); } catch (const std::runtime_error&) { ++thrown; }
        try { va_cv::warp_perspective(frame, out, std::vector<Tensor>(1, Tensor(3, 2, 1, vision::FP32, vision::NCHW)), va_cv::VSize(8, 8)); } catch (const std::runtime_error&) { ++thrown; }
        try {
            const float line[8] = {0.f, 0.f, 10.f, 10.f, 20.f, 20.f, 5.f, 30.f};
            Tensor m;
            va_cv::get_perspective_transform(line, rect, m);
        } catch (const std::runtime_error&) { ++thrown; }
        expect(thrown == 5, "unsupported combinations throw");
    } catch (const std::exception& e) {
        std::printf("exception: %s\n", e.what());
        return 2;
    }
    std::printf("cases %d failed %d\n", g_cases, g_failed);
    return g_failed ? 1 : 0;
}
