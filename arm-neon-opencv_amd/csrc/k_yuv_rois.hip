// k_yuv_rois.hip -- many small affine crops of NV21 / NV12 frames in one
// launch: ROI i of the destination is what cvt_color of frame src_index[i]
// followed by warp_affine_rois under m[i] produces, byte for byte, without
// the BGR frame ever existing.
//
// The shape of the work is warp_rois_kernel's (k_warp_rois.hip, roi_tile.hpp):
// kRoiTile consecutive row-major pixels of one ROI per workgroup, 64
// consecutive ones per gather, (ROI, tile) in XCD-contiguous order, the map
// read from the device array and inverted by one thread, the band laid out in
// LDS at the destination's offset modulo 16 and copied out by copy_run.
//
// The per-pixel arithmetic is the chain's: fx, fy, affine_tap and the 11-bit
// weights of warp_rois_kernel; each of the four taps is decoded as
// color_kernel decodes a pixel (Y at (x, y), the chroma pair at row
// h + (y >> 1), byte x & ~1; chroma_terms, clamp_u8), and every channel is
// then blended in the u8 warp's fixed point (two v_dot2_u32_u16, two 24-bit
// multiplies, >> 22).
//
// Every source read goes through a buffer resource over the indexed frame's
// Y and chroma rows; an index outside [0, n_src) gives a resource of zero
// bytes and a ROI of border_value.  A dword load that crosses the end of the
// resource is zeroed whole by the range check, so the taps whose aligned
// loads would reach past the frame's last byte (the last chroma pair of the
// last chroma row, with a dense frame) are read byte by byte.
#pragma clang fp contract(off)

#include "roi_tile.hpp"
#include "vacv_device.hpp"

namespace vacv {
namespace {

// The decoded pixel (x, y) of the frame behind rs (x < w, y < h): three byte loads
__device__ __forceinline__ void decoded_pixel(const Rsrc& rs, uint32_t rp, int h, int x, int y, bool v_first, bool rgb,
                                              int (&c)[3]) {
    const uint32_t oy = (uint32_t)y * rp + (uint32_t)x + rs.delta;
    const uint32_t oc = (uint32_t)(h + (y >> 1)) * rp + (uint32_t)(x & ~1) + rs.delta;
    const uint32_t pair = load_u8(rs, oc) | (load_u8(rs, oc + 1u) << 8);
    decode_tap((int)load_u8(rs, oy), pair, v_first, rgb, c);
}

// PLANAR: fp32 NCHW destination (one LDS region and one byte range per plane)
// EXT: border modes other than CONSTANT (a separate instance, as warp_rois_kernel)
template <int OUT, bool PLANAR, bool EXT>
__global__ void __launch_bounds__(kBlock)
yuv_rois_kernel(YuvRoisLaunch L, int tiles, int total) {
    using TOut = typename std::conditional<(OUT == kOutSame), uint8_t, float>::type;
    constexpr int CC = 3;
    constexpr int kPlanes = PLANAR ? CC : 1;
    constexpr int kPxB = (PLANAR ? 1 : CC) * (int)sizeof(TOut);  // bytes per pixel of one destination plane
    constexpr int kRegion = kRoiTile * kPxB + 16;                // + the destination's offset modulo 16
    __shared__ __attribute__((aligned(16))) unsigned char xch[kPlanes * kRegion];
    __shared__ float s_inv[6];
    __shared__ int s_frame;

    // an XCD walks a contiguous range of (ROI, tile), so the tiles of one ROI,
    // which share source lines, meet in one L2
    const int id = xcd_block_id(total);
    if (id >= total) return;  // uniform
    const int roi = id / tiles;
    const int tile = id - roi * tiles;
    const int lane = threadIdx.x, wv = __builtin_amdgcn_readfirstlane((int)threadIdx.y);
    const int tid = wv * 64 + lane;

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
        for (int k = 0; k < 6; ++k) s_inv[k] = inv[k];
        s_frame = L.src_index ? L.src_index[roi] : (L.n_src == 1 ? 0 : roi);
    }
    __syncthreads();
    const float i0 = uniform_f(s_inv[0]), i1 = uniform_f(s_inv[1]), i2 = uniform_f(s_inv[2]);
    const float i3 = uniform_f(s_inv[3]), i4 = uniform_f(s_inv[4]), i5 = uniform_f(s_inv[5]);
    const int frame = __builtin_amdgcn_readfirstlane(s_frame);
    const bool valid = frame >= 0 && frame < L.n_src;  // uniform; else: all border, nothing read

    ChanNorm cn[CC] = {};
    if (OUT == kOutNorm) {
#pragma unroll
        for (int k = 0; k < CC; ++k) cn[k] = chan_norm(L.norm, 0, k);
    }
    TOut bval[CC];
#pragma unroll
    for (int k = 0; k < CC; ++k) bval[k] = emit_u8<OUT, TOut>(cn[k], (int)L.border[k]);

    const unsigned char* sp = L.src + (int64_t)(valid ? frame : 0) * L.src_img;
    const Rsrc srs = make_rsrc(sp, valid ? L.src_bytes : 0);
    const uint32_t slimit = (valid ? (uint32_t)L.src_bytes : 0u) + srs.delta;
    const uint32_t rp32 = (uint32_t)L.src_row;  // src_bytes <= kMaxPlaneBytes (launch_yuv_rois)
    const bool mul24 = L.src_row < (1 << 24) && L.h < (1 << 23);  // rows up to h * 3 / 2
    const bool v_first = L.v_first != 0, rgb = L.rgb != 0;

    // ---- the tile: pixels [p0, p0 + npx) of the ROI, first one at (tx0, ty0)
    const int w = L.dst.w;
    const int roi_px = w * L.dst.h;
    const int p0 = tile * kRoiTile;
    const int npx = min(kRoiTile, roi_px - p0);
    const int ty0 = p0 / w, tx0 = p0 - ty0 * w;  // uniform
    const float rw = 1.f / (float)w;
    unsigned char* dbase = const_cast<unsigned char*>(L.dst.base) + (int64_t)roi * L.dst.img_pitch;
    const bool dense = L.dst.row_pitch == (int64_t)w * kPxB;  // the band is one byte range per plane
    uint32_t shift[kPlanes];
#pragma unroll
    for (int k = 0; k < kPlanes; ++k) {
        const uintptr_t a = reinterpret_cast<uintptr_t>(dbase + (int64_t)k * L.dst.plane_pitch + (int64_t)p0 * kPxB);
        shift[k] = dense ? ((uint32_t)a & 15u & ~(uint32_t)(sizeof(TOut) - 1)) : 0u;
    }

#pragma unroll
    for (int q = 0; q < kRoiPx; ++q) {
        const int loc = (wv * kRoiPx + q) * 64 + lane;  // 64 consecutive pixels per gather
        if (loc >= npx) continue;
        int dy, x;
        divmod_w((uint32_t)(tx0 + loc), (uint32_t)w, rw, dy, x);
        const int y = ty0 + dy;
        TOut* o[CC];
#pragma unroll
        for (int k = 0; k < CC; ++k)
            o[k] = PLANAR ? reinterpret_cast<TOut*>(xch + k * kRegion + shift[k]) + loc
                          : reinterpret_cast<TOut*>(xch + shift[0]) + loc * CC + k;
        // warp_affine_naive.cpp:23-24: (m0*x + m1*y) + m2, all float
        const float fx = i0 * (float)x + i1 * (float)y + i2;
        const float fy = i3 * (float)x + i4 * (float)y + i5;
        int sx = 0, sy = 0;
        float ax = 0.f, ay = 0.f;
        const bool ok = valid && affine_tap(fy, L.h, sy, ay) && affine_tap(fx, L.w, sx, ax);
        if (!ok) {
            if (EXT && valid) {  // L.border_mode != kBorderConstant
                // the four taps through the border rule, each decoded, the naive
                // sampler's weights (warp_border_sample on the decoded frame)
                int ix, iy;
                float bx, by;
                border_tap(fx, ix, bx);
                border_tap(fy, iy, by);
                const int x0 = border_index(ix, L.w, L.border_mode), x1 = border_index(ix + 1, L.w, L.border_mode);
                const int y0 = border_index(iy, L.h, L.border_mode), y1 = border_index(iy + 1, L.h, L.border_mode);
                int t00[3], t01[3], t10[3], t11[3];  // t<row><column>
                decoded_pixel(srs, rp32, L.h, x0, y0, v_first, rgb, t00);
                decoded_pixel(srs, rp32, L.h, x1, y0, v_first, rgb, t01);
                decoded_pixel(srs, rp32, L.h, x0, y1, v_first, rgb, t10);
                decoded_pixel(srs, rp32, L.h, x1, y1, v_first, rgb, t11);
                const int wy0 = warp_weight(by), wy1 = 2048 - wy0;
                const int wx0 = warp_weight(bx), wx1 = 2048 - wx0;
#pragma unroll
                for (int k = 0; k < CC; ++k) {
                    const int v = (t00[k] * wx0 * wy0 + t10[k] * wx0 * wy1 + t01[k] * wx1 * wy0 + t11[k] * wx1 * wy1) >> 22;
                    *o[k] = emit_u8<OUT, TOut>(cn[k], v);
                }
                continue;
            }
#pragma unroll
            for (int k = 0; k < CC; ++k) *o[k] = bval[k];
            continue;
        }
        // sx <= w - 2, sy <= h - 2: both Y rows and both chroma rows are the frame's
        const uint32_t oy0 = (mul24 ? __umul24((uint32_t)sy, rp32) : (uint32_t)sy * rp32) + (uint32_t)sx + srs.delta;
        const uint32_t oy1 = oy0 + rp32;
        const uint32_t crow = (uint32_t)(L.h + (sy >> 1));
        const uint32_t oc0 = (mul24 ? __umul24(crow, rp32) : crow * rp32) + (uint32_t)(sx & ~1) + srs.delta;
        const uint32_t oc1 = (sy & 1) ? oc0 + rp32 : oc0;  // rows sy and sy + 1 share a chroma row when sy is even
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
        const uint32_t car = (sx & 1) ? ca >> 16 : ca;  // the right tap's pair
        const uint32_t cbr = (sx & 1) ? cb >> 16 : cb;
        int tl[3], tr[3], bl[3], br[3];
        decode_tap((int)(ya & 0xFFu), ca, v_first, rgb, tl);
        decode_tap((int)((ya >> 8) & 0xFFu), car, v_first, rgb, tr);
        decode_tap((int)(yb & 0xFFu), cb, v_first, rgb, bl);
        decode_tap((int)((yb >> 8) & 0xFFu), cbr, v_first, rgb, br);
        const int wy0 = warp_weight(ay), wy1 = 2048 - wy0;
        const int wx0 = warp_weight(ax), wx1 = 2048 - wx0;
        // warp_affine_naive.cpp:50-54 as (tl*wx0 + tr*wx1)*wy0 + (bl*wx0 +
        // br*wx1)*wy1: the same int32 value (exact, <= 255*2^22)
        const us2 wx = __builtin_bit_cast(us2, (uint32_t)wx0 | ((uint32_t)wx1 << 16));
#pragma unroll
        for (int k = 0; k < CC; ++k) {
            const uint32_t top = (uint32_t)tl[k] | ((uint32_t)tr[k] << 16);
            const uint32_t bot = (uint32_t)bl[k] | ((uint32_t)br[k] << 16);
            const uint32_t ht = __builtin_amdgcn_udot2(__builtin_bit_cast(us2, top), wx, 0u, false);
            const uint32_t hb = __builtin_amdgcn_udot2(__builtin_bit_cast(us2, bot), wx, 0u, false);
            const int v = (int)((__umul24(ht, (uint32_t)wy0) + __umul24(hb, (uint32_t)wy1)) >> 22);
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
    int dy1, x1;
    divmod_w((uint32_t)(tx0 + npx - 1), (uint32_t)w, rw, dy1, x1);
    const int nrows = dy1 + 1;
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
hipError_t launch_ext(const YuvRoisLaunch& L, hipStream_t s) {
    const int64_t px = (int64_t)L.dst.w * L.dst.h;
    const int64_t tiles = (px + kRoiTile - 1) / kRoiTile;
    const int64_t total = tiles * L.n_roi;
    if (total >= 0x7FFFFFF0LL) return hipErrorInvalidValue;
    const int64_t blocks = (total + 7) / 8 * 8;
    if (L.border_mode == kBorderConstant)
        hipLaunchKernelGGL((yuv_rois_kernel<OUT, PLANAR, false>), dim3((unsigned)blocks), dim3(64, 4), 0, s, L,
                           (int)tiles, (int)total);
    else
        hipLaunchKernelGGL((yuv_rois_kernel<OUT, PLANAR, true>), dim3((unsigned)blocks), dim3(64, 4), 0, s, L,
                           (int)tiles, (int)total);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_yuv_rois(const YuvRoisLaunch& L, hipStream_t s) {
    // the kernel's 32-bit source offsets, its float row/column split
    // (divmod_w) and its int pixel index: launch_warp_rois's limits
    if (L.src_bytes > kMaxPlaneBytes || L.dst.w > (1 << 20) || (int64_t)L.dst.w * L.dst.h > 0x7FFF0000LL)
        return hipErrorInvalidValue;
    if (L.out == kOutSame) return L.planar ? hipErrorInvalidValue : launch_ext<kOutSame, false>(L, s);
    if (L.out != kOutNorm) return hipErrorInvalidValue;
    return L.planar ? launch_ext<kOutNorm, true>(L, s) : launch_ext<kOutNorm, false>(L, s);
}

}  // namespace vacv
