// k_yuv_warp_rois_std.hip -- many small affine crops of NV21 / NV12 frames in
// one launch, each standardized by its OWN per-channel mean and standard
// deviation: ROI i of the destination is what cvt_color of frame src_index[i]
// followed by warp_affine_rois_standardize under m[i] produces, bit for bit,
// without the BGR frame, the u8 crop or its statistics pass ever existing
// (DESIGN.md 3.20).  Both arrays are read from DEVICE memory when the kernel
// runs.
//
// The work shape is k_warp_rois_std.hip's: a ROI's statistics span all its
// pixels, border pixels included, so ONE WORKGROUP PER ROI holds the whole u8
// ROI in LDS:
//   head   256 bytes: the inverted map and the frame, the integer sums, the
//          statistics
//   px     the warped u8 ROI, 3 w h bytes rounded up to 16: interleaved
//          [h][w][3] for an NHWC destination, [3][h][w] for a planar one
//   lut    [3][256] floats: the normalized value of every u8 value of every
//          channel
// yuv_warp_rois_std_lds_bytes() is that sum; the host refuses what passes
// 64 KiB.
//
// Bit identity with the chain vacv_cvt_color -> vacv_warp_affine_rois_standardize
// rests on:
//  1. the u8 ROI is yuv_rois_kernel's kOutSame one, expression for expression:
//     the same inverse (invert_affine_value), the same coordinate, tap and
//     weights, the same loads (Y at (sx, sy), the chroma pair at row
//     h + (sy >> 1), byte sx & ~1; bytes at the frame's end), the same decode
//     (decode_tap) and blend, the same border pixels (the four taps through
//     border_index, each decoded; or the u8 border value in the decoded
//     channel order);
//  2. the sums of a u8 ROI are integers, so their order is free;
//  3. the statistics, the table and the stores are roi_std_tail.hpp's, which
//     are k_warp_rois_std.hip's.
// tests/test_yuv_warp_rois_std_gpu.py compares with that chain and with the
// CPU oracle bit for bit.
//
// Device-supplied values cannot fault: an index outside [0, n_src) reads
// nothing -- its resource spans zero bytes -- and is the chain's ROI of
// border_value; every source read goes through a buffer resource that spans
// exactly the indexed frame's Y and chroma rows, and the border modes' taps
// are mapped into it by border_index.  A dword load that crosses the end of
// the resource is zeroed whole by the range check, so the taps whose aligned
// loads would reach past the frame's last byte are read byte by byte.
#pragma clang fp contract(off)

#include "roi_std_tail.hpp"
#include "roi_tile.hpp"
#include "vacv_device.hpp"

namespace vacv {
namespace {

struct YuvWarpStdHead {
    float inv[6];  // the dst -> src map
    int frame;     // src_index[roi], as read
    int pad;
    StdStats st;
};
static_assert(sizeof(YuvWarpStdHead) <= kYuvStdHeadBytes, "the head of the LDS block");

// What the sampler needs of the ROI's frame, all uniform
struct YuvStdFrame {
    Rsrc srs;  // exactly the frame's Y and chroma rows, or zero bytes (invalid index)
    uint32_t slimit, rp32;
    bool mul24, valid, v_first, rgb;
};

// The decoded pixel (x, y) of the frame behind rs (x < w, y < h): three byte loads
__device__ __forceinline__ void decoded_pixel(const Rsrc& rs, uint32_t rp, int h, int x, int y, bool v_first, bool rgb,
                                              int (&c)[3]) {
    const uint32_t oy = (uint32_t)y * rp + (uint32_t)x + rs.delta;
    const uint32_t oc = (uint32_t)(h + (y >> 1)) * rp + (uint32_t)(x & ~1) + rs.delta;
    const uint32_t pair = load_u8(rs, oc) | (load_u8(rs, oc + 1u) << 8);
    decode_tap((int)load_u8(rs, oy), pair, v_first, rgb, c);
}

// The three u8 values of ROI pixel (x, y) under the dst -> src map iv:
// yuv_rois_kernel's kOutSame arithmetic, expression for expression
template <bool EXT>
__device__ __forceinline__ void sample_yuv(const YuvWarpRoisStdLaunch& L, const YuvStdFrame& F, const float (&iv)[6],
                                           int x, int y, int (&v)[3]) {
    // warp_affine_naive.cpp:23-24: (m0*x + m1*y) + m2, all float
    const float fx = iv[0] * (float)x + iv[1] * (float)y + iv[2];
    const float fy = iv[3] * (float)x + iv[4] * (float)y + iv[5];
    int sx = 0, sy = 0;
    float ax = 0.f, ay = 0.f;
    const bool ok = F.valid && affine_tap(fy, L.h, sy, ay) && affine_tap(fx, L.w, sx, ax);
    if (!ok) {
        if (EXT && F.valid) {  // L.border_mode != kBorderConstant
            // the four taps through the border rule, each decoded, the naive
            // sampler's weights (warp_border_sample on the decoded frame)
            int ix, iy;
            float bx, by;
            border_tap(fx, ix, bx);
            border_tap(fy, iy, by);
            const int x0 = border_index(ix, L.w, L.border_mode), x1 = border_index(ix + 1, L.w, L.border_mode);
            const int y0 = border_index(iy, L.h, L.border_mode), y1 = border_index(iy + 1, L.h, L.border_mode);
            int t00[3], t01[3], t10[3], t11[3];  // t<row><column>
            decoded_pixel(F.srs, F.rp32, L.h, x0, y0, F.v_first, F.rgb, t00);
            decoded_pixel(F.srs, F.rp32, L.h, x1, y0, F.v_first, F.rgb, t01);
            decoded_pixel(F.srs, F.rp32, L.h, x0, y1, F.v_first, F.rgb, t10);
            decoded_pixel(F.srs, F.rp32, L.h, x1, y1, F.v_first, F.rgb, t11);
            const int wy0 = warp_weight(by), wy1 = 2048 - wy0;
            const int wx0 = warp_weight(bx), wx1 = 2048 - wx0;
#pragma unroll
            for (int k = 0; k < 3; ++k)
                v[k] = (int)(uint8_t)((t00[k] * wx0 * wy0 + t10[k] * wx0 * wy1 + t01[k] * wx1 * wy0 +
                                       t11[k] * wx1 * wy1) >> 22);
            return;
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) v[k] = (int)(uint8_t)L.border[k];
        return;
    }
    // sx <= w - 2, sy <= h - 2: both Y rows and both chroma rows are the frame's
    const uint32_t oy0 =
        (F.mul24 ? __umul24((uint32_t)sy, F.rp32) : (uint32_t)sy * F.rp32) + (uint32_t)sx + F.srs.delta;
    const uint32_t oy1 = oy0 + F.rp32;
    const uint32_t crow = (uint32_t)(L.h + (sy >> 1));
    const uint32_t oc0 = (F.mul24 ? __umul24(crow, F.rp32) : crow * F.rp32) + (uint32_t)(sx & ~1) + F.srs.delta;
    const uint32_t oc1 = (sy & 1) ? oc0 + F.rp32 : oc0;  // rows sy and sy + 1 share a chroma row when sy is even
    // Y: bytes sx, sx + 1 of each row.  Chroma: the pair of sx and, for an
    // odd sx, the next one (bytes 2, 3; sx + 2 <= w - 1 then).  Each in one
    // dword-aligned load; oc1 is the largest of the four offsets, and where
    // its load would cross the frame's end all four go byte by byte (bytes
    // 2, 3 past the end read as zero and are not used: sx is even there)
    uint32_t ya, yb, ca, cb, unused;
    if ((oc1 & ~3u) + 4u * kTapDwords<1, true> <= F.slimit) {
        load_taps<1, true, 0>(F.srs, oy0, ya, unused);
        load_taps<1, true, 0>(F.srs, oy1, yb, unused);
        load_taps<1, true, 0>(F.srs, oc0, ca, unused);
        load_taps<1, true, 0>(F.srs, oc1, cb, unused);
    } else {
        ya = load_u8(F.srs, oy0) | (load_u8(F.srs, oy0 + 1u) << 8);
        yb = load_u8(F.srs, oy1) | (load_u8(F.srs, oy1 + 1u) << 8);
        ca = cb = 0u;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            ca |= load_u8(F.srs, oc0 + e) << (8 * e);
            cb |= load_u8(F.srs, oc1 + e) << (8 * e);
        }
    }
    const uint32_t car = (sx & 1) ? ca >> 16 : ca;  // the right tap's pair
    const uint32_t cbr = (sx & 1) ? cb >> 16 : cb;
    int tl[3], tr[3], bl[3], br[3];
    decode_tap((int)(ya & 0xFFu), ca, F.v_first, F.rgb, tl);
    decode_tap((int)((ya >> 8) & 0xFFu), car, F.v_first, F.rgb, tr);
    decode_tap((int)(yb & 0xFFu), cb, F.v_first, F.rgb, bl);
    decode_tap((int)((yb >> 8) & 0xFFu), cbr, F.v_first, F.rgb, br);
    const int wy0 = warp_weight(ay), wy1 = 2048 - wy0;
    const int wx0 = warp_weight(ax), wx1 = 2048 - wx0;
    // warp_affine_naive.cpp:50-54 as (tl*wx0 + tr*wx1)*wy0 + (bl*wx0 +
    // br*wx1)*wy1: the same int32 value (exact, <= 255*2^22)
    const us2 wx = __builtin_bit_cast(us2, (uint32_t)wx0 | ((uint32_t)wx1 << 16));
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const uint32_t top = (uint32_t)tl[k] | ((uint32_t)tr[k] << 16);
        const uint32_t bot = (uint32_t)bl[k] | ((uint32_t)br[k] << 16);
        const uint32_t ht = __builtin_amdgcn_udot2(__builtin_bit_cast(us2, top), wx, 0u, false);
        const uint32_t hb = __builtin_amdgcn_udot2(__builtin_bit_cast(us2, bot), wx, 0u, false);
        v[k] = (int)((__umul24(ht, (uint32_t)wy0) + __umul24(hb, (uint32_t)wy1)) >> 22);
    }
}

// PLANAR: NCHW destination (one run set per plane)
// EXT: border modes other than CONSTANT (a separate instance, as yuv_rois_kernel)
template <bool PLANAR, bool EXT>
__global__ void __launch_bounds__(kYuvStdBlock) yuv_warp_rois_std_kernel(YuvWarpRoisStdLaunch L) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    constexpr int CC = kYuvStdC;
    const int w = L.dst.w, h = L.dst.h, npx = w * h;  // <= 64,256 (the host's LDS gate)
    YuvWarpStdHead* hd = reinterpret_cast<YuvWarpStdHead*>(lds);
    unsigned char* px = lds + kYuvStdHeadBytes;
    float* lut = reinterpret_cast<float*>(px + yuv_std_px_bytes(w, h));
    const int roi = blockIdx.x, tid = threadIdx.x;

    // ---- the ROI's map and frame: one thread reads the device arrays and inverts
    if (tid == 0) {
        float m[6], inv[6];
#pragma unroll
        for (int k = 0; k < 6; ++k) m[k] = L.m[(int64_t)roi * 6 + k];
        if (L.inverse_map) {
#pragma unroll
            for (int k = 0; k < 6; ++k) inv[k] = m[k];
        } else {
            invert_affine_value(m, inv);
        }
#pragma unroll
        for (int k = 0; k < 6; ++k) hd->inv[k] = inv[k];
        hd->frame = L.src_index ? L.src_index[roi] : (L.n_src == 1 ? 0 : roi);
    }
    if (tid < 8) hd->st.sum[tid] = 0ull;
    __syncthreads();
    // into scalar registers: everything derived from them (the frame's buffer
    // resource above all) is then uniform for the compiler too
    float iv[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) iv[k] = uniform_f(hd->inv[k]);
    const int frame = __builtin_amdgcn_readfirstlane(hd->frame);

    YuvStdFrame F;
    F.valid = frame >= 0 && frame < L.n_src;  // uniform; else: all border, nothing read
    const unsigned char* sp = L.src + (int64_t)(F.valid ? frame : 0) * L.src_img;
    F.srs = make_rsrc(sp, F.valid ? L.src_bytes : 0);
    F.slimit = (F.valid ? (uint32_t)L.src_bytes : 0u) + F.srs.delta;
    F.rp32 = (uint32_t)L.src_row;  // src_bytes <= kMaxPlaneBytes (the host's gate)
    F.mul24 = L.src_row < (1 << 24) && L.h < (1 << 23);  // rows up to h * 3 / 2
    F.v_first = L.v_first != 0;
    F.rgb = L.rgb != 0;

    // ---- the u8 ROI into LDS, its sums into registers: 64 consecutive pixels per gather
    uint32_t s1[CC], s2[CC];
#pragma unroll
    for (int k = 0; k < CC; ++k) s1[k] = s2[k] = 0u;
    const float rw = 1.f / (float)w;
#pragma unroll 1
    for (int p = tid; p < npx; p += kYuvStdBlock) {
        int y, x;  // p < 2^16: the float quotient is within one (divmod_w)
        divmod_w((uint32_t)p, (uint32_t)w, rw, y, x);
        int v[CC];
        sample_yuv<EXT>(L, F, iv, x, y, v);
#pragma unroll
        for (int k = 0; k < CC; ++k) {
            px[PLANAR ? k * npx + p : p * CC + k] = (unsigned char)v[k];
            s1[k] += (uint32_t)v[k];
            s2[k] += (uint32_t)(v[k] * v[k]);
        }
    }
    standardize_tail<PLANAR>(&hd->st, px, lut, s1, s2, L.dst, roi, L.mean_out, L.stddev_out);
}

template <bool PLANAR>
hipError_t launch_ext(const YuvWarpRoisStdLaunch& L, size_t lds, hipStream_t s) {
    const dim3 grid(L.n_roi), block(kYuvStdBlock);
    if (L.border_mode == kBorderConstant)
        hipLaunchKernelGGL((yuv_warp_rois_std_kernel<PLANAR, false>), grid, block, lds, s, L);
    else
        hipLaunchKernelGGL((yuv_warp_rois_std_kernel<PLANAR, true>), grid, block, lds, s, L);
    return hipGetLastError();
}

}  // namespace

// A workgroup's dynamic LDS: the head, the u8 ROI and the table of normalized
// values (the layout at the top of this file)
size_t yuv_warp_rois_std_lds_bytes(int w, int h) {
    return kYuvStdHeadBytes + yuv_std_px_bytes(w, h) + 1024 * (size_t)kYuvStdC;
}

bool yuv_warp_rois_std_fits(const YuvWarpRoisStdLaunch& L) {
    // yuv_rois_kernel's 32-bit source offsets; one workgroup's LDS (so
    // w h < 2^16); kYuvStdBlock threads per ROI within a 32-bit grid
    return L.src_bytes <= kMaxPlaneBytes && yuv_warp_rois_std_lds_bytes(L.dst.w, L.dst.h) <= 64 * 1024 &&
           L.n_roi <= (int)(0xFFFFFFFFu / kYuvStdBlock);
}

hipError_t launch_yuv_warp_rois_std(const YuvWarpRoisStdLaunch& L, hipStream_t s) {
    if (!yuv_warp_rois_std_fits(L)) return hipErrorInvalidValue;
    const size_t lds = yuv_warp_rois_std_lds_bytes(L.dst.w, L.dst.h);
    return L.planar ? launch_ext<true>(L, lds, s) : launch_ext<false>(L, lds, s);
}

}  // namespace vacv
