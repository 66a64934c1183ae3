// k_yuv_crop_resize_rois_std.hip -- many upright crops of NV21 / NV12 frames
// in one launch, each standardized by its OWN per-channel mean and standard
// deviation: ROI i of the destination is what cvt_color of frame src_index[i]
// followed by crop_resize_rois_standardize of rects[i] produces, bit for bit,
// without the BGR frame, the u8 crop or its statistics pass ever existing
// (DESIGN.md 3.19).  Both arrays are read from DEVICE memory when the kernel
// runs.
//
// The work shape is k_crop_resize_rois_std.hip's: ONE WORKGROUP PER ROI, the
// whole u8 ROI in LDS:
//   head   256 bytes: the validated rect and frame, the integer sums, the
//          statistics
//   px     the resized u8 ROI, 3 w h bytes rounded up to 16: interleaved
//          [h][w][3] for an NHWC destination, [3][h][w] for a planar one
//   tab    the x taps of all w columns, then the y taps of all h rows: 8 bytes
//          each.  Dead once the ROI is sampled, and then
//   lut    [3][256] floats over the same bytes: the normalized value of every
//          u8 value of every channel
// yuv_crop_resize_rois_std_lds_bytes() is that sum; the host refuses what
// passes 64 KiB.
//
// Bit identity with the chain vacv_cvt_color -> vacv_crop_resize_rois_standardize
// rests on:
//  1. the u8 ROI is yuv_crop_resize_rois_kernel's, expression for expression:
//     the same tap (fixed_tap of the RECT's size, offset by left / top; an
//     index in the decoded frame), the same loads (Y at (sx, sy), the chroma
//     pair at row h + (sy >> 1), byte sx & ~1; bytes at the frame's end), the
//     same decode (decode_tap) and blend (blend_fixed);
//  2. the sums of a u8 ROI are integers, so their order is free;
//  3. the statistics, the table and the stores are roi_std_tail.hpp's, which
//     are k_crop_resize_rois_std.hip's.
// tests/test_yuv_crop_resize_rois_std_gpu.py compares with that chain and with
// the CPU oracle bit for bit.
//
// Device-supplied values cannot fault: one thread validates the rect and the
// index against the DECODED w x h (range checks, no sum of two device values);
// an invalid ROI reads nothing -- its resource spans zero bytes -- and is the
// chain's ROI of u8 zeros: mean 0, stddev 0, output +0.0; a valid one has all
// four taps inside its rect (fixed_tap: i in [0, n_in - 2]), and every source
// read goes through a buffer resource that spans exactly the indexed frame's
// Y and chroma rows.  A dword load that crosses the end of the resource is
// zeroed whole by the range check, so the taps whose aligned loads would reach
// past the frame's last byte are read byte by byte.
#pragma clang fp contract(off)

#include "roi_std_tail.hpp"
#include "roi_tile.hpp"
#include "vacv_device.hpp"

namespace vacv {
namespace {

struct YuvStdHead {
    int roi[5];  // left, top, width, height, frame (-1: invalid)
    int pad;
    StdStats st;
};
static_assert(sizeof(YuvStdHead) <= kYuvStdHeadBytes, "the head of the LDS block");

// What the sampler needs of the ROI's frame, all uniform
struct YuvStdFrame {
    Rsrc srs;  // exactly the frame's Y and chroma rows, or zero bytes (invalid ROI)
    uint32_t slimit, rp32;
    uint32_t h;  // decoded rows: the first chroma row
    bool mul24, v_first, rgb;
};

// One tap of a column (origin = left) or a row (origin = top), as
// yuv_crop_resize_rois_kernel tables it: .x = the first tap's index in the
// decoded frame (the chroma row needs sy itself), .y = w0 | w1 << 16
__device__ __forceinline__ uint2 tap_entry(int d, int n_in, int n_out, float scale_f, double scale_d, int mode,
                                           int origin) {
    const FixedTap t = fixed_tap(d, n_in, n_out, scale_f, scale_d, mode);
    return make_uint2((uint32_t)(t.i + origin), (uint32_t)t.w0 | ((uint32_t)t.w1 << 16));
}

// The three u8 values of the output pixel with column tap cx and row tap ry:
// yuv_crop_resize_rois_kernel's loads, decode and blend
template <bool REF>
__device__ __forceinline__ void sample_yuv(const YuvStdFrame& F, uint2 cx, uint2 ry, int (&v)[3]) {
    // sx in [left, left + cw - 2], sy in [top, top + ch - 2]: both taps of
    // both rows lie inside the validated rect, so both Y rows and both
    // chroma rows are the frame's
    const uint32_t sx = cx.x, sy = ry.x;
    const uint32_t oy0 = (F.mul24 ? __umul24(sy, F.rp32) : sy * F.rp32) + sx + F.srs.delta;
    const uint32_t oy1 = oy0 + F.rp32;
    const uint32_t crow = F.h + (sy >> 1);
    const uint32_t oc0 = (F.mul24 ? __umul24(crow, F.rp32) : crow * F.rp32) + (sx & ~1u) + F.srs.delta;
    const uint32_t oc1 = (sy & 1u) ? oc0 + F.rp32 : oc0;  // rows sy and sy + 1 share a chroma row when sy is even
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
    const uint32_t car = (sx & 1u) ? ca >> 16 : ca;  // the right tap's pair
    const uint32_t cbr = (sx & 1u) ? cb >> 16 : cb;
    int tl[3], tr[3], bl[3], br[3];
    decode_tap((int)(ya & 0xFFu), ca, F.v_first, F.rgb, tl);
    decode_tap((int)((ya >> 8) & 0xFFu), car, F.v_first, F.rgb, tr);
    decode_tap((int)(yb & 0xFFu), cb, F.v_first, F.rgb, bl);
    decode_tap((int)((yb >> 8) & 0xFFu), cbr, F.v_first, F.rgb, br);
    const us2 wx = __builtin_bit_cast(us2, cx.y);
    const uint32_t wA = ry.y & 0xFFFFu, wB = ry.y >> 16;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const uint32_t tp = (uint32_t)tl[k] | ((uint32_t)tr[k] << 16);
        const uint32_t bt = (uint32_t)bl[k] | ((uint32_t)br[k] << 16);
        v[k] = blend_fixed<REF ? VACV_LINEAR_REFERENCE : VACV_LINEAR_NEON>(tp, bt, wx, wA, wB);
    }
}

// PLANAR: NCHW destination (one run set per plane)
// REF: VACV_LINEAR_REFERENCE's blend (else the NEON / OPENCV two-pass one; the
// rounding of their weights is fixed_tap's, by L.mode)
template <bool PLANAR, bool REF>
__global__ void __launch_bounds__(kYuvStdBlock) yuv_crop_resize_rois_std_kernel(YuvCropResizeRoisStdLaunch L) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    constexpr int CC = kYuvStdC;
    const int w = L.dst.w, h = L.dst.h, npx = w * h;  // < 65,536 (the host's LDS gate)
    YuvStdHead* hd = reinterpret_cast<YuvStdHead*>(lds);
    unsigned char* px = lds + kYuvStdHeadBytes;
    const size_t px_bytes = yuv_std_px_bytes(w, h);
    uint2* tab = reinterpret_cast<uint2*>(px + px_bytes);
    float* lut = reinterpret_cast<float*>(px + px_bytes);
    const int roi = blockIdx.x, tid = threadIdx.x;

    // ---- the ROI's rect and frame: one thread reads the device arrays and validates
    if (tid == 0) {
        const int32_t* r = L.rects + (int64_t)roi * 4;
        const int l = r[0], t = r[1], cw = r[2], ch = r[3];
        const int f = L.src_index ? L.src_index[roi] : (L.n_src == 1 ? 0 : roi);
        // left + width <= w as left <= w - width: no sum of two device values
        const bool ok = f >= 0 && f < L.n_src && cw >= 2 && ch >= 2 && l >= 0 && t >= 0 && cw <= L.w &&
                        l <= L.w - cw && ch <= L.h && t <= L.h - ch;
        hd->roi[0] = l;
        hd->roi[1] = t;
        hd->roi[2] = cw;
        hd->roi[3] = ch;
        hd->roi[4] = ok ? f : -1;
    }
    if (tid < 8) hd->st.sum[tid] = 0ull;
    __syncthreads();
    // into scalar registers: everything derived from them (the frame's buffer
    // resource above all) is then uniform for the compiler too
    const int left = __builtin_amdgcn_readfirstlane(hd->roi[0]), top = __builtin_amdgcn_readfirstlane(hd->roi[1]);
    const int cw = __builtin_amdgcn_readfirstlane(hd->roi[2]), ch = __builtin_amdgcn_readfirstlane(hd->roi[3]);
    const int frame = __builtin_amdgcn_readfirstlane(hd->roi[4]);
    const bool valid = frame >= 0;  // uniform; else: u8 zeros, nothing read

    YuvStdFrame F;
    const unsigned char* sp = L.src + (int64_t)(valid ? frame : 0) * L.src_img;
    F.srs = make_rsrc(sp, valid ? L.src_bytes : 0);
    F.slimit = (valid ? (uint32_t)L.src_bytes : 0u) + F.srs.delta;
    F.rp32 = (uint32_t)L.src_row;  // src_bytes <= kMaxPlaneBytes (the host's gate)
    F.h = (uint32_t)L.h;
    F.mul24 = L.src_row < (1 << 24) && L.h < (1 << 23);  // rows up to h * 3 / 2
    F.v_first = L.v_first != 0;
    F.rgb = L.rgb != 0;

    // ---- the taps of all columns and all rows, once per ROI
    // resize_naive.cpp:17-18: float division; resize_neon.cpp:17-18: double
    if (valid) {
        const float sxf = (float)cw / (float)w, syf = (float)ch / (float)h;
        const double sxd = (double)cw / (double)w, syd = (double)ch / (double)h;
#pragma unroll 1
        for (int e = tid; e < w + h; e += kYuvStdBlock) {
            if (e < w) tab[e] = tap_entry(e, cw, w, sxf, sxd, L.mode, left);
            else tab[e] = tap_entry(e - w, ch, h, syf, syd, L.mode, top);
        }
    }
    __syncthreads();

    // ---- the u8 ROI into LDS, its sums into registers: 64 consecutive pixels per gather
    uint32_t s1[CC], s2[CC];
#pragma unroll
    for (int k = 0; k < CC; ++k) s1[k] = s2[k] = 0u;
    const float rw = 1.f / (float)w;
#pragma unroll 1
    for (int p = tid; p < npx; p += kYuvStdBlock) {
        int v[CC];
        if (valid) {
            int y, x;  // p < 2^16: the float quotient is within one (divmod_w)
            divmod_w((uint32_t)p, (uint32_t)w, rw, y, x);
            sample_yuv<REF>(F, tab[x], tab[w + y], v);
        } else {
#pragma unroll
            for (int k = 0; k < CC; ++k) v[k] = 0;
        }
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
hipError_t launch_blend(const YuvCropResizeRoisStdLaunch& L, size_t lds, hipStream_t s) {
    const dim3 grid(L.n_roi), block(kYuvStdBlock);
    if (L.mode == VACV_LINEAR_REFERENCE)
        hipLaunchKernelGGL((yuv_crop_resize_rois_std_kernel<PLANAR, true>), grid, block, lds, s, L);
    else
        hipLaunchKernelGGL((yuv_crop_resize_rois_std_kernel<PLANAR, false>), grid, block, lds, s, L);
    return hipGetLastError();
}

}  // namespace

// A workgroup's dynamic LDS: the head, the u8 ROI, and the taps or the table
// of normalized values, whichever is larger (the layout at the top of this file)
size_t yuv_crop_resize_rois_std_lds_bytes(int w, int h) {
    const size_t taps = 8 * ((size_t)w + h), lut = 1024 * (size_t)kYuvStdC;
    return kYuvStdHeadBytes + yuv_std_px_bytes(w, h) + (taps > lut ? taps : lut);
}

bool yuv_crop_resize_rois_std_fits(const YuvCropResizeRoisStdLaunch& L) {
    // the kernel's 32-bit source offsets; one workgroup's LDS (so w h < 2^16);
    // kYuvStdBlock threads per ROI within a 32-bit grid
    return L.src_bytes <= kMaxPlaneBytes && yuv_crop_resize_rois_std_lds_bytes(L.dst.w, L.dst.h) <= 64 * 1024 &&
           L.n_roi <= (int)(0xFFFFFFFFu / kYuvStdBlock);
}

hipError_t launch_yuv_crop_resize_rois_std(const YuvCropResizeRoisStdLaunch& L, hipStream_t s) {
    if (!yuv_crop_resize_rois_std_fits(L)) return hipErrorInvalidValue;
    const size_t lds = yuv_crop_resize_rois_std_lds_bytes(L.dst.w, L.dst.h);
    return L.planar ? launch_blend<true>(L, lds, s) : launch_blend<false>(L, lds, s);
}

}  // namespace vacv
