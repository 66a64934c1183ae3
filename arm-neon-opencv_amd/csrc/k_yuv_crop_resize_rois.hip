// k_yuv_crop_resize_rois.hip -- many upright crops of NV21 / NV12 frames in
// one launch: ROI i of the destination is what cvt_color of frame src_index[i]
// followed by crop_resize_rois of rects[i] produces, byte for byte, without
// the BGR frame or the crop ever existing.  Both arrays are
// read from DEVICE memory when the kernel runs.
//
// The shape of the work is crop_resize_rois_kernel's (k_crop_resize_rois.hip,
// roi_tile.hpp): kRoiTile consecutive row-major pixels of one ROI per
// workgroup, 64 consecutive ones per gather, (ROI, tile) in XCD-contiguous
// order, the rect and the index read and validated by one thread, the taps of
// the tile's columns and band rows computed once into an LDS table
// (fixed_tap of the RECT's size, offset by (left, top)), the band laid out in
// LDS at the destination's offset modulo 16 and copied out by copy_run.
//
// The per-pixel arithmetic is the chain's: each of the four taps is decoded
// as yuv_rois_kernel decodes it (Y at (x, y), the chroma pair at row
// h + (y >> 1), byte x & ~1; decode_tap), and every channel is then blended
// in the u8 resize's fixed point (blend_fixed: REFERENCE's (Sum S*wx*wy) >> 22
// or the NEON / OPENCV two-pass form).
//
// Device-supplied values cannot fault: an invalid rect or index (judged
// against the DECODED w x h, range checks only) gives a buffer resource of
// zero bytes and a ROI of zeros; a valid one has all four taps inside its
// rect (fixed_tap: i in [0, n_in - 2]), so inside the frame.  A dword load
// that crosses the end of the resource is zeroed whole by the range check, so
// the taps whose aligned loads would reach past the frame's last byte (the
// last chroma pairs of the last chroma row, with a dense frame) are read byte
// by byte.
#pragma clang fp contract(off)

#include "roi_tile.hpp"
#include "vacv_device.hpp"

namespace vacv {
namespace {

// columns [0, w) then the band's rows: w + rows <= w + 1022 / w + 2 <= 1026
// for w <= kRoiTile; wider ROIs keep only their (at most 2) rows here
constexpr int kTapTable = kRoiTile + 8;

// One tap of a column (origin = left) or a row (origin = top): .x = the first
// tap's index in the decoded frame, .y = the 11-bit weights w0 | w1 << 16
__device__ __forceinline__ uint2 tap_entry(int d, int n_in, int n_out, float scale_f, double scale_d, int mode,
                                           int origin) {
    const FixedTap t = fixed_tap(d, n_in, n_out, scale_f, scale_d, mode);
    return make_uint2((uint32_t)(t.i + origin), (uint32_t)t.w0 | ((uint32_t)t.w1 << 16));
}

// PLANAR: fp32 NCHW destination (one LDS region and one byte range per plane)
// REF: VACV_LINEAR_REFERENCE's blend (else the NEON / OPENCV two-pass one; the
// rounding of their weights is fixed_tap's, by L.mode)
template <int OUT, bool PLANAR, bool REF>
__global__ void __launch_bounds__(kBlock)
yuv_crop_resize_rois_kernel(YuvCropResizeRoisLaunch L, int tiles, int total) {
    using TOut = typename std::conditional<(OUT == kOutSame), uint8_t, float>::type;
    constexpr int CC = 3;
    constexpr int kPlanes = PLANAR ? CC : 1;
    constexpr int kPxB = (PLANAR ? 1 : CC) * (int)sizeof(TOut);  // bytes per pixel of one destination plane
    constexpr int kRegion = kRoiTile * kPxB + 16;                // + the destination's offset modulo 16
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
        // left + width <= w as left <= w - width: no sum of two device values
        const bool ok = f >= 0 && f < L.n_src && cw >= 2 && ch >= 2 && l >= 0 && t >= 0 && cw <= L.w &&
                        l <= L.w - cw && ch <= L.h && t <= L.h - ch;
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

    ChanNorm cn[CC] = {};
    if (OUT == kOutNorm) {
#pragma unroll
        for (int k = 0; k < CC; ++k) cn[k] = chan_norm(L.norm, 0, k);
    }

    const unsigned char* sp = L.src + (int64_t)(valid ? frame : 0) * L.src_img;
    const Rsrc srs = make_rsrc(sp, valid ? L.src_bytes : 0);
    const uint32_t slimit = (valid ? (uint32_t)L.src_bytes : 0u) + srs.delta;
    const uint32_t rp32 = (uint32_t)L.src_row;  // src_bytes <= kMaxPlaneBytes (launch_yuv_crop_resize_rois)
    const bool mul24 = L.src_row < (1 << 24) && L.h < (1 << 23);  // rows up to h * 3 / 2
    const bool v_first = L.v_first != 0, rgb = L.rgb != 0;

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
    const int ncol = w <= kRoiTile ? w : 0;  // a wider ROI's tile has no column twice: per pixel
    if (valid) {
#pragma unroll 1
        for (int e = tid; e < ncol + nrows; e += kBlock) {
            if (e < ncol) tab[e] = tap_entry(e, cw, w, sxf, sxd, L.mode, left);
            else tab[e] = tap_entry(ty0 + e - ncol, ch, h, syf, syd, L.mode, top);
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
            for (int k = 0; k < CC; ++k) *o[k] = emit_u8<OUT, TOut>(cn[k], 0);
            continue;
        }
        const uint2 cx = ncol ? tab[x] : tap_entry(x, cw, w, sxf, sxd, L.mode, left);
        const uint2 ry = tab[ncol + dy];
        // sx in [left, left + cw - 2], sy in [top, top + ch - 2]: both taps of
        // both rows lie inside the validated rect, so both Y rows and both
        // chroma rows are the frame's
        const uint32_t sx = cx.x, sy = ry.x;
        const uint32_t oy0 = (mul24 ? __umul24(sy, rp32) : sy * rp32) + sx + srs.delta;
        const uint32_t oy1 = oy0 + rp32;
        const uint32_t crow = (uint32_t)L.h + (sy >> 1);
        const uint32_t oc0 = (mul24 ? __umul24(crow, rp32) : crow * rp32) + (sx & ~1u) + srs.delta;
        const uint32_t oc1 = (sy & 1u) ? oc0 + rp32 : oc0;  // rows sy and sy + 1 share a chroma row when sy is even
        // Y: bytes sx, sx + 1 of each row.  Chroma: the pair of sx and, for an
        // odd sx, the next one (bytes 2, 3; sx + 2 <= w - 1 then).  Each in one
        // dword-aligned load; oc1 is the largest of the four offsets, and where
        // its load would cross the frame's end all four go byte by byte (bytes
        // 2, 3 past the end read as zero and are not used: sx is even there)
        uint32_t ya, yb, ca, cb, unused;
        if ((oc1 & ~3u) + 4u * kTapDwords<1, true> <= slimit) {
            load_taps<1, true, 0>(srs, oy0, ya, unused);
            load_taps<1, true, 0>(srs, oy1, yb, unused);
            load_taps<1, true, 0>(srs, oc0, ca, unused);
            load_taps<1, true, 0>(srs, oc1, cb, unused);
        } else {
            ya = load_u8(srs, oy0) | (load_u8(srs, oy0 + 1u) << 8);
            yb = load_u8(srs, oy1) | (load_u8(srs, oy1 + 1u) << 8);
            ca = cb = 0u;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                ca |= load_u8(srs, oc0 + e) << (8 * e);
                cb |= load_u8(srs, oc1 + e) << (8 * e);
            }
        }
        const uint32_t car = (sx & 1u) ? ca >> 16 : ca;  // the right tap's pair
        const uint32_t cbr = (sx & 1u) ? cb >> 16 : cb;
        int tl[3], tr[3], bl[3], br[3];
        decode_tap((int)(ya & 0xFFu), ca, v_first, rgb, tl);
        decode_tap((int)((ya >> 8) & 0xFFu), car, v_first, rgb, tr);
        decode_tap((int)(yb & 0xFFu), cb, v_first, rgb, bl);
        decode_tap((int)((yb >> 8) & 0xFFu), cbr, v_first, rgb, br);
        const us2 wx = __builtin_bit_cast(us2, cx.y);
        const uint32_t wA = ry.y & 0xFFFFu, wB = ry.y >> 16;
#pragma unroll
        for (int k = 0; k < CC; ++k) {
            const uint32_t tp = (uint32_t)tl[k] | ((uint32_t)tr[k] << 16);
            const uint32_t bt = (uint32_t)bl[k] | ((uint32_t)br[k] << 16);
            const int v = blend_fixed<REF ? VACV_LINEAR_REFERENCE : VACV_LINEAR_NEON>(tp, bt, wx, wA, wB);
            *o[k] = emit_u8<OUT, TOut>(cn[k], v);
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

template <int OUT, bool PLANAR>
hipError_t launch_blend(const YuvCropResizeRoisLaunch& L, hipStream_t s) {
    const int64_t px = (int64_t)L.dst.w * L.dst.h;
    const int64_t tiles = (px + kRoiTile - 1) / kRoiTile;
    const int64_t total = tiles * L.n_roi;
    const int64_t blocks = (total + 7) / 8 * 8;
    if (L.mode != VACV_LINEAR_REFERENCE)
        hipLaunchKernelGGL((yuv_crop_resize_rois_kernel<OUT, PLANAR, false>), dim3((unsigned)blocks), dim3(64, 4), 0, s,
                           L, (int)tiles, (int)total);
    else
        hipLaunchKernelGGL((yuv_crop_resize_rois_kernel<OUT, PLANAR, true>), dim3((unsigned)blocks), dim3(64, 4), 0, s,
                           L, (int)tiles, (int)total);
    return hipGetLastError();
}

}  // namespace

bool yuv_crop_resize_rois_fits(const YuvCropResizeRoisLaunch& L) {
    const int64_t px = (int64_t)L.dst.w * L.dst.h;
    return L.src_bytes <= kMaxPlaneBytes && L.dst.w <= (1 << 20) && px <= 0x7FFF0000LL &&
           (px + kRoiTile - 1) / kRoiTile * L.n_roi < 0x7FFFFFF0LL;
}

hipError_t launch_yuv_crop_resize_rois(const YuvCropResizeRoisLaunch& L, hipStream_t s) {
    // the kernel's 32-bit source offsets, its float row/column split
    // (divmod_w) and its int pixel and workgroup indices
    if (!yuv_crop_resize_rois_fits(L)) return hipErrorInvalidValue;
    if (L.out == kOutSame) return L.planar ? hipErrorInvalidValue : launch_blend<kOutSame, false>(L, s);
    if (L.out != kOutNorm) return hipErrorInvalidValue;
    return L.planar ? launch_blend<kOutNorm, true>(L, s) : launch_blend<kOutNorm, false>(L, s);
}

}  // namespace vacv
