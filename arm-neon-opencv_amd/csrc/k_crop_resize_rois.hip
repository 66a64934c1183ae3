// k_crop_resize_rois.hip -- many upright crops in one launch: ROI i of the
// destination is resize(crop(frame src_index[i], rects[i]), w x h), both arrays
// read from DEVICE memory when the kernel runs.
//
// The arithmetic is the reference's crop_naive + resize_naive chain, bit for
// bit, with the crop never materialised:
//   taps   fixed_tap / float_tap (vacv_semantics.hpp) of the RECT's size: the
//          scale is rect_w / w_out, half-pixel centres, taps clamped at the
//          rect's edges (resize_naive.cpp:19-31), then offset by (left, top)
//   blend  u8 (Sum S*wx*wy) >> 22 (resize_naive.cpp:61-64), or the NEON /
//          OPENCV two-pass form (blend_fixed); fp32 left to right
//          (resize_naive.cpp:121-124)
//   a rect of the output's own size is the plain crop (resize.cpp:58-61
//   copies): fp32 pixels are passed through, not multiplied by 1 and 0
// The shape of the work is warp_rois_kernel's (roi_tile.hpp): a workgroup owns
// kRoiTile consecutive row-major pixels of one ROI, its band is laid out in
// LDS at the destination's offset modulo 16 and leaves through copy_run.
// What a resize has that a warp has not is separable taps: the x taps depend
// on the column only and the y taps on the row only, so a workgroup computes
// the taps of its columns and of its band rows ONCE into an LDS table (the
// fp64 products of src_coord_*), and a pixel is two table reads, two gathers
// and the blend.
// Device-supplied values cannot fault: one thread validates the rect and the
// index (range checks, no int overflow); an invalid ROI reads nothing and is
// zero-filled; every source read goes through a buffer resource that spans
// exactly the indexed frame.
#pragma clang fp contract(off)

#include "roi_tile.hpp"
#include "vacv_device.hpp"

namespace vacv {
namespace {

// columns [0, w) then the band's rows: w + rows <= w + 1022 / w + 2 <= 1026
// for w <= kRoiTile; wider ROIs keep only their (at most 2) rows here
constexpr int kTapTable = kRoiTile + 8;

// One tap of a column (origin = left, step = bytes per pixel) or a row
// (origin = top, step = row pitch): .x = byte offset of the first tap in the
// frame, .y = the weights -- u8: w0 | w1 << 16 (11-bit, in [0, 2048]); fp32:
// the bits of w1 (w0 = 1.f - w1 is float_tap's own expression)
template <bool U8>
__device__ __forceinline__ uint2 tap_entry(int d, int n_in, int n_out, float scale_f, double scale_d, int mode,
                                           int origin, uint32_t step, bool same) {
    if constexpr (U8) {
        const FixedTap t = fixed_tap(d, n_in, n_out, scale_f, scale_d, mode);
        return make_uint2((uint32_t)(t.i + origin) * step, (uint32_t)t.w0 | ((uint32_t)t.w1 << 16));
    } else {
        if (same) return make_uint2((uint32_t)(d + origin) * step, 0u);  // the pixel itself
        const FloatTap t = float_tap(d, n_in, scale_f);
        return make_uint2((uint32_t)(t.i + origin) * step, __builtin_bit_cast(uint32_t, t.w1));
    }
}

// PLANAR: fp32 NCHW destination (one LDS region and one byte range per plane)
// REF: VACV_LINEAR_REFERENCE's blend (else the NEON / OPENCV two-pass one; the
// rounding of their weights is fixed_tap's, by L.mode)
template <int CC, typename TIn, int OUT, bool PLANAR, bool REF>
__global__ void __launch_bounds__(kBlock)
crop_resize_rois_kernel(CropResizeRoisLaunch L, int tiles, int total) {
    using TOut = typename std::conditional<(OUT == kOutSame), TIn, float>::type;
    constexpr bool kU8 = std::is_same<TIn, uint8_t>::value;
    constexpr bool kU8Norm = kU8 && (OUT == kOutNorm);
    constexpr int kPlanes = PLANAR ? CC : 1;
    constexpr int kPxB = (PLANAR ? 1 : CC) * (int)sizeof(TOut);  // bytes per pixel of one destination plane
    constexpr int kRegion = kRoiTile * kPxB + 16;                // + the destination's offset modulo 16
    constexpr uint32_t kInPx = CC * (uint32_t)sizeof(TIn);       // bytes per source pixel
    __shared__ __attribute__((aligned(16))) unsigned char xch[kPlanes * kRegion];
    __shared__ uint2 tab[kTapTable];
    __shared__ int s_roi[5];  // left, top, width, height, frame (-1: invalid)

    // an XCD walks a contiguous range of (ROI, tile), so the tiles of one ROI,
    // which share source lines, meet in one L2
    const int id = xcd_block_id(total);
    if (id >= total) return;  // uniform
    const int roi = id / tiles;
    const int tile = id - roi * tiles;
    const int lane = threadIdx.x, wv = __builtin_amdgcn_readfirstlane((int)threadIdx.y);
    const int tid = wv * 64 + lane;

    // ---- the ROI's rect and frame: one thread reads the device arrays and validates
    if (tid == 0) {
        const int32_t* r = L.rects + (int64_t)roi * 4;
        const int l = r[0], t = r[1], cw = r[2], ch = r[3];
        const int f = L.src_index ? L.src_index[roi] : (L.n_src == 1 ? 0 : roi);
        // left + width <= W as left <= W - width: no sum of two device values
        const bool ok = f >= 0 && f < L.n_src && cw >= 2 && ch >= 2 && l >= 0 && t >= 0 && cw <= L.src.w &&
                        l <= L.src.w - cw && ch <= L.src.h && t <= L.src.h - ch;
        s_roi[0] = l;
        s_roi[1] = t;
        s_roi[2] = cw;
        s_roi[3] = ch;
        s_roi[4] = ok ? f : -1;
    }
    __syncthreads();
    // into scalar registers: everything derived from them (the frame's buffer
    // resource above all) is then uniform for the compiler too
    const int left = __builtin_amdgcn_readfirstlane(s_roi[0]), top = __builtin_amdgcn_readfirstlane(s_roi[1]);
    const int cw = __builtin_amdgcn_readfirstlane(s_roi[2]), ch = __builtin_amdgcn_readfirstlane(s_roi[3]);
    const int frame = __builtin_amdgcn_readfirstlane(s_roi[4]);
    const bool valid = frame >= 0;  // uniform; else: zeros, nothing read

    float nmean[CC], nstd[CC];
    if (OUT == kOutNorm) {
#pragma unroll
        for (int k = 0; k < CC; ++k) norm_params(L.norm, 0, k, nmean[k], nstd[k]);
    }
    ChanNorm cn[CC] = {};
    if (kU8Norm) {
#pragma unroll
        for (int k = 0; k < CC; ++k) cn[k] = chan_norm(L.norm, 0, k);
    }

    const unsigned char* sp = L.src.base + (int64_t)(valid ? frame : 0) * L.src.img_pitch;
    const Rsrc srs = make_rsrc(sp, valid ? L.src.plane_bytes : 0);
    const uint32_t slimit = (valid ? (uint32_t)L.src.plane_bytes : 0u) + srs.delta;
    const uint32_t rp32 = (uint32_t)L.src.row_pitch;  // plane_bytes <= kMaxPlaneBytes (launch_crop_resize_rois)

    // ---- the tile: pixels [p0, p0 + npx) of the ROI, first one at (tx0, ty0)
    const int w = L.dst.w, h = L.dst.h;
    const int roi_px = w * h;
    const int p0 = tile * kRoiTile;
    const int npx = min(kRoiTile, roi_px - p0);
    const int ty0 = p0 / w, tx0 = p0 - ty0 * w;  // uniform
    const float rw = 1.f / (float)w;
    int dy1, x1;  // the band's last row (relative) and last column
    divmod_w((uint32_t)(tx0 + npx - 1), (uint32_t)w, rw, dy1, x1);
    const int nrows = dy1 + 1;
    unsigned char* dbase = const_cast<unsigned char*>(L.dst.base) + (int64_t)roi * L.dst.img_pitch;
    const bool dense = L.dst.row_pitch == (int64_t)w * kPxB;  // the band is one byte range per plane
    uint32_t shift[kPlanes];
#pragma unroll
    for (int k = 0; k < kPlanes; ++k) {
        const uintptr_t a = reinterpret_cast<uintptr_t>(dbase + (int64_t)k * L.dst.plane_pitch + (int64_t)p0 * kPxB);
        shift[k] = dense ? ((uint32_t)a & 15u & ~(uint32_t)(sizeof(TOut) - 1)) : 0u;
    }

    // ---- the taps of the ROI's columns and of the band's rows, once per workgroup
    // resize_naive.cpp:17-18: float division; resize_neon.cpp:17-18: double
    const float sxf = (float)cw / (float)w, syf = (float)ch / (float)h;
    const double sxd = (double)cw / (double)w, syd = (double)ch / (double)h;
    const bool same = cw == w && ch == h;  // uniform: the plain crop
    const int ncol = w <= kRoiTile ? w : 0;  // a wider ROI's tile has no column twice: per pixel
    if (valid) {
#pragma unroll 1
        for (int e = tid; e < ncol + nrows; e += kBlock) {
            if (e < ncol) tab[e] = tap_entry<kU8>(e, cw, w, sxf, sxd, L.mode, left, kInPx, same);
            else tab[e] = tap_entry<kU8>(ty0 + e - ncol, ch, h, syf, syd, L.mode, top, rp32, same);
        }
    }
    __syncthreads();

#pragma unroll
    for (int q = 0; q < kRoiPx; ++q) {
        const int loc = (wv * kRoiPx + q) * 64 + lane;  // 64 consecutive pixels per gather
        if (loc >= npx) continue;
        int dy, x;
        divmod_w((uint32_t)(tx0 + loc), (uint32_t)w, rw, dy, x);
        TOut* o[CC];
#pragma unroll
        for (int k = 0; k < CC; ++k)
            o[k] = PLANAR ? reinterpret_cast<TOut*>(xch + k * kRegion + shift[k]) + loc
                          : reinterpret_cast<TOut*>(xch + shift[0]) + loc * CC + k;
        if (!valid) {
#pragma unroll
            for (int k = 0; k < CC; ++k) {
                if (OUT == kOutNorm)
                    *o[k] = kU8Norm ? (TOut)normalize_u8v(cn[k], 0) : (TOut)normalize_value(0.f, nmean[k], nstd[k]);
                else
                    *o[k] = (TOut)0;
            }
            continue;
        }
        const uint2 cx = ncol ? tab[x] : tap_entry<kU8>(x, cw, w, sxf, sxd, L.mode, left, kInPx, same);
        const uint2 ry = tab[ncol + dy];
        // both taps of both rows lie inside the validated rect, so inside the frame
        const uint32_t o0 = ry.x + cx.x + srs.delta;
        const uint32_t o1 = o0 + rp32;
        if constexpr (kU8) {
            // the 2*CC tap bytes of each row in ONE unaligned 8-byte buffer load;
            // a load past the frame's end (its last pixels) falls back to bytes
            uint32_t a0 = 0, a1 = 0, c0 = 0, c1 = 0;
            if (o1 + 8u <= slimit) {
                load_taps<CC, false, 0>(srs, o0, a0, a1);
                load_taps<CC, false, 0>(srs, o1, c0, c1);
            } else {
#pragma unroll
                for (int e = 0; e < 2 * CC; ++e) {
                    const uint32_t t0 = __builtin_amdgcn_raw_buffer_load_b8(srs.r, (int)(o0 + e), 0, 0);
                    const uint32_t t1 = __builtin_amdgcn_raw_buffer_load_b8(srs.r, (int)(o1 + e), 0, 0);
                    if (e < 4) { a0 |= t0 << (8 * e); c0 |= t1 << (8 * e); }
                    else { a1 |= t0 << (8 * (e - 4)); c1 |= t1 << (8 * (e - 4)); }
                }
            }
            const us2 wx = __builtin_bit_cast(us2, cx.y);
            const uint32_t wA = ry.y & 0xFFFFu, wB = ry.y >> 16;
#pragma unroll
            for (int k = 0; k < CC; ++k) {
                const uint32_t tp = tap_pair<CC>(a0, a1, k), bt = tap_pair<CC>(c0, c1, k);
                const int v = blend_fixed<REF ? VACV_LINEAR_REFERENCE : VACV_LINEAR_NEON>(tp, bt, wx, wA, wB);
                *o[k] = emit_u8<OUT, TOut>(cn[k], v);
            }
        } else {
            const float xb = __builtin_bit_cast(float, cx.y), xa = 1.f - xb;
            const float yb = __builtin_bit_cast(float, ry.y), ya = 1.f - yb;
            float f0[2 * CC], f1[2 * CC];
            load_f32<2 * CC>(srs, o0, f0);
            load_f32<2 * CC>(srs, o1, f1);
#pragma unroll
            for (int k = 0; k < CC; ++k) {
                // resize_naive.cpp:121-124, left to right: lt, lb, rt, rb
                float v = f0[k] * xa * ya;
                v += f1[k] * xa * yb;
                v += f0[CC + k] * xb * ya;
                v += f1[CC + k] * xb * yb;
                if (same) v = f0[k];
                if (OUT == kOutNorm) v = normalize_value(v, nmean[k], nstd[k]);
                *o[k] = (TOut)v;
            }
        }
    }
    __syncthreads();

    // ---- LDS -> HBM -----------------------------------------------------------
    if (dense) {  // uniform: one byte range per plane, all four waves on it
#pragma unroll
        for (int k = 0; k < kPlanes; ++k)
            copy_run(dbase + (int64_t)k * L.dst.plane_pitch + (int64_t)p0 * kPxB, xch, (uint32_t)(k * kRegion) + shift[k],
                     npx * kPxB, tid, kBlock);
        return;
    }
    // pitched rows: wave r % 4 copies run r = (plane, band row)
#pragma unroll 1
    for (int r = wv; r < kPlanes * nrows; r += 4) {
        const int k = PLANAR ? r / nrows : 0;
        const int dy = r - k * nrows;
        const int xa = dy == 0 ? tx0 : 0;
        const int xb = dy == dy1 ? x1 + 1 : w;
        const int loc = dy * w + xa - tx0;  // tile-local index of the run's first pixel
        copy_run(dbase + (int64_t)k * L.dst.plane_pitch + (int64_t)(ty0 + dy) * L.dst.row_pitch + (int64_t)xa * kPxB, xch,
                 (uint32_t)(k * kRegion + loc * kPxB), (xb - xa) * kPxB, lane, 64);
    }
}

template <int CC, typename TIn, int OUT, bool PLANAR>
hipError_t launch_blend(const CropResizeRoisLaunch& L, hipStream_t s) {
    const int64_t px = (int64_t)L.dst.w * L.dst.h;
    const int64_t tiles = (px + kRoiTile - 1) / kRoiTile;
    const int64_t total = tiles * L.n_roi;
    if (total >= 0x7FFFFFF0LL) return hipErrorInvalidValue;
    const int64_t blocks = (total + 7) / 8 * 8;
    if constexpr (std::is_same<TIn, uint8_t>::value) {  // fp32 has one blend: one instance
        if (L.mode != VACV_LINEAR_REFERENCE) {
            hipLaunchKernelGGL((crop_resize_rois_kernel<CC, TIn, OUT, PLANAR, false>), dim3((unsigned)blocks),
                               dim3(64, 4), 0, s, L, (int)tiles, (int)total);
            return hipGetLastError();
        }
    }
    hipLaunchKernelGGL((crop_resize_rois_kernel<CC, TIn, OUT, PLANAR, true>), dim3((unsigned)blocks), dim3(64, 4), 0, s,
                       L, (int)tiles, (int)total);
    return hipGetLastError();
}

template <typename TIn, int OUT>
hipError_t launch_cc(const CropResizeRoisLaunch& L, hipStream_t s) {
    if (L.planar) {
        if constexpr (OUT == kOutNorm) {
            if (L.src.cc == 3) return launch_blend<3, TIn, OUT, true>(L, s);
        }
        return hipErrorInvalidValue;
    }
    switch (L.src.cc) {
        case 1: return launch_blend<1, TIn, OUT, false>(L, s);
        case 2: return launch_blend<2, TIn, OUT, false>(L, s);
        case 3: return launch_blend<3, TIn, OUT, false>(L, s);
        case 4: return launch_blend<4, TIn, OUT, false>(L, s);
        default: return hipErrorInvalidValue;
    }
}

}  // namespace

bool crop_resize_rois_fits(const CropResizeRoisLaunch& L) {
    const int64_t px = (int64_t)L.dst.w * L.dst.h;
    return L.src.plane_bytes <= kMaxPlaneBytes && L.dst.w <= (1 << 20) && px <= 0x7FFF0000LL &&
           (px + kRoiTile - 1) / kRoiTile * L.n_roi < 0x7FFFFFF0LL;
}

hipError_t launch_crop_resize_rois(const CropResizeRoisLaunch& L, hipStream_t s) {
    // the kernel's 32-bit source offsets, its float row/column split
    // (divmod_w) and its int pixel and workgroup indices
    if (!crop_resize_rois_fits(L)) return hipErrorInvalidValue;
    if (L.src.esize == 1) {
        if (L.out == kOutSame) return launch_cc<uint8_t, kOutSame>(L, s);
        return launch_cc<uint8_t, kOutNorm>(L, s);
    }
    if (L.out == kOutNorm) return launch_cc<float, kOutNorm>(L, s);
    return launch_cc<float, kOutSame>(L, s);
}

}  // namespace vacv
