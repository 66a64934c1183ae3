// va_cv::match_template and va_cv::minMaxIdx through the C++ layer, on host
// tensors (staged through the pinned pool) and on to_device() tensors, against
// results computed by the numpy references of tests/test_gpu_match.py, byte
// for byte: six methods for a 3-channel u8 and a 1-channel fp32 image, a
// template of the image's width but taller (swapped, as cv::matchTemplate
// does), minMaxIdx without a mask, with one, with a mask that selects nothing,
// and with null minIdx / maxIdx.
// Built and run by tests/test_gpu_match.py, which writes the inputs and the
// expected results as raw files into the directory given as argv[1]; needs a
// HIP device.
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "cv/cv.h"

using vision::Tensor;

static int g_failed = 0, g_cases = 0;
static std::string g_dir;

static void expect(bool ok, const std::string& what) {
    ++g_cases;
    if (!ok) {
        ++g_failed;
        std::printf("FAIL %s\n", what.c_str());
    }
}

static std::vector<unsigned char> slurp(const std::string& name) {
    const std::string path = g_dir + "/" + name;
    std::FILE* f = std::fopen(path.c_str(), "rb");
    if (!f) throw std::runtime_error("cannot open " + path);
    std::vector<unsigned char> b;
    unsigned char chunk[4096];
    size_t n;
    while ((n = std::fread(chunk, 1, sizeof(chunk), f)) > 0) b.insert(b.end(), chunk, chunk + n);
    std::fclose(f);
    return b;
}

static Tensor load(const std::string& name, int w, int h, int c, vision::DType dt) {
    Tensor t(w, h, c, dt, vision::NHWC);
    const std::vector<unsigned char> b = slurp(name);
    if (b.size() != t.len()) throw std::runtime_error(name + ": unexpected size");
    std::memcpy(t.data, b.data(), b.size());
    return t;
}

static void expect_result(const Tensor& res, int w, int h, bool on_device, const std::string& want_file,
                          const std::string& what) {
    expect(res.w == w && res.h == h && res.c == 1 && res.dtype == vision::FP32, what + ": shape");
    expect(res.on_device() == on_device, what + ": placement");
    const Tensor host = res.to_host();
    const std::vector<unsigned char> want = slurp(want_file);
    expect(host.len() == want.size() && std::memcmp(host.data, want.data(), want.size()) == 0, what + ": bytes");
}

struct MinMaxWant {  // as tests/test_gpu_match.py packs it: "<dd4i"
    double mn, mx;
    int idx[4];
};

static void expect_minmax(const Tensor& src, const Tensor& mask, const MinMaxWant& want, const std::string& what) {
    double mn = -1, mx = -1;
    int imn[2] = {-7, -7}, imx[2] = {-7, -7};
    va_cv::minMaxIdx(src, &mn, &mx, imn, imx, mask);
    expect(std::memcmp(&mn, &want.mn, 8) == 0 && std::memcmp(&mx, &want.mx, 8) == 0, what + ": values");
    expect(imn[0] == want.idx[0] && imn[1] == want.idx[1] && imx[0] == want.idx[2] && imx[1] == want.idx[3],
           what + ": indices");
    // null index pointers: the values alone
    double mn2 = -1, mx2 = -1;
    va_cv::minMaxIdx(src, &mn2, &mx2, nullptr, nullptr, mask);
    expect(std::memcmp(&mn2, &want.mn, 8) == 0 && std::memcmp(&mx2, &want.mx, 8) == 0, what + ": null indices");
    int only[2] = {-7, -7};
    va_cv::minMaxIdx(src, nullptr, &mx2, only, nullptr, mask);
    expect(only[0] == want.idx[0] && only[1] == want.idx[1], what + ": null minVal and maxIdx");
}

int main(int argc, char** argv) {
    if (argc != 2) {
        std::printf("usage: %s <data directory>\n", argv[0]);
        return 2;
    }
    g_dir = argv[1];
    try {
        int H, W, h, w, Hf, Wf, hf, wf, Ht, Hm, Wm;
        {
            const std::string path = g_dir + "/dims.txt";
            std::FILE* f = std::fopen(path.c_str(), "r");
            if (!f || std::fscanf(f, "%d %d %d %d %d %d %d %d %d %d %d", &H, &W, &h, &w, &Hf, &Wf, &hf, &wf, &Ht, &Hm,
                                  &Wm) != 11)
                throw std::runtime_error("cannot read " + path);
            std::fclose(f);
        }
        const Tensor u_img = load("u8_img.bin", W, H, 3, vision::INT8), u_tpl = load("u8_tpl.bin", w, h, 3, vision::INT8);
        const Tensor f_img = load("f32_img.bin", Wf, Hf, 1, vision::FP32);
        const Tensor f_tpl = load("f32_tpl.bin", wf, hf, 1, vision::FP32);
        const Tensor tall = load("u8_tall.bin", W, Ht, 3, vision::INT8);
        const Tensor mm_src = load("mm_src.bin", Wm, Hm, 1, vision::FP32);
        const Tensor mm_mask = load("mm_mask.bin", Wm, Hm, 1, vision::INT8);
        Tensor mm_none(Wm, Hm, 1, vision::INT8, vision::NHWC);
        std::memset(mm_none.data, 0, mm_none.len());
        const std::vector<unsigned char> mmw = slurp("mm_want.bin");
        if (mmw.size() != 3 * sizeof(MinMaxWant)) throw std::runtime_error("mm_want.bin: unexpected size");
        MinMaxWant want[3];
        std::memcpy(want, mmw.data(), sizeof(want));

        for (int on_device = 0; on_device < 2; ++on_device) {
            const std::string where = on_device ? "device" : "host";
            auto put = [&](const Tensor& t) { return on_device ? t.to_device(0) : t; };
            const Tensor ui = put(u_img), ut = put(u_tpl), fi = put(f_img), ft = put(f_tpl), tl = put(tall);
            for (int m = 0; m < 6; ++m) {
                Tensor ru, rf;
                va_cv::match_template(ui, ut, ru, m);
                expect_result(ru, W - w + 1, H - h + 1, on_device, "u8_want_" + std::to_string(m) + ".bin",
                              where + " u8 c3 method " + std::to_string(m));
                va_cv::match_template(fi, ft, rf, m);
                expect_result(rf, Wf - wf + 1, Hf - hf + 1, on_device, "f32_want_" + std::to_string(m) + ".bin",
                              where + " f32 c1 method " + std::to_string(m));
            }
            Tensor rs;
            va_cv::match_template(ui, tl, rs, 3);  // TM_CCORR_NORMED; the template is the larger one
            expect_result(rs, 1, Ht - H + 1, on_device, "swap_want.bin", where + " swapped");
            expect_minmax(put(mm_src), Tensor(), want[0], where + " minMaxIdx");
            expect_minmax(put(mm_src), put(mm_mask), want[1], where + " minMaxIdx, mask");
            expect_minmax(put(mm_src), put(mm_none), want[2], where + " minMaxIdx, all masked");
        }
        // a template that fits in neither order is refused loudly
        int thrown = 0;
        Tensor r;
        const Tensor wide(W + 3, 2, 3, vision::INT8, vision::NHWC);
        try { va_cv::match_template(u_img, wide, r, 0); } catch (const std::runtime_error&) { ++thrown; }
        expect(thrown == 1, "a template that does not fit throws");
    } catch (const std::exception& e) {
        std::printf("exception: %s\n", e.what());
        return 2;
    }
    std::printf("cases %d failed %d\n", g_cases, g_failed);
    return g_failed ? 1 : 0;
}
