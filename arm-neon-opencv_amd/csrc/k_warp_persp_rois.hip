// k_warp_persp_rois.hip -- many small projective crops in one launch: ROI i of
// the destination is warp_perspective of source frame src_index[i] under its
// own 3x3 homography h[i], both read from DEVICE arrays when the kernel runs
// (DESIGN.md 3.21).
//
// The work shape and the sampler are warp_rois_kernel's (k_warp_rois.hip,
// DESIGN.md 3.10), line for line: kRoiTile consecutive row-major pixels of one
// ROI per workgroup, 64 consecutive ones per gather, (ROI, tile) in
// XCD-contiguous order, every source read through a buffer resource that spans
// exactly the indexed frame, the band laid out in LDS at the destination's
// offset modulo 16 and copied out by copy_run.  Only the coordinates differ:
//  * one thread reads the nine floats and forms the dst -> src map N in double
//    (invert_homography_value, the host's own function, unless the map is
//    already the inverse one);
//  * a pixel's source point is perspective_coords (vacv_semantics.hpp): three
//    double rows, ONE IEEE reciprocal, two products rounded to float, as
//    cv::warpPerspective computes them.  From (fx, fy) on the pixel is
//    warp_rois_kernel's, bit for bit.
// The nine doubles go through LDS into scalar registers, so the per-pixel fp64
// operands and the frame's buffer resource are uniform.
#pragma clang fp contract(off)

#include "roi_tile.hpp"
#include "vacv_device.hpp"

namespace vacv {
namespace {

// a uniform double into a pair of scalar registers
__device__ __forceinline__ double uniform_d(double v) {
    const uint64_t u = __builtin_bit_cast(uint64_t, v);
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)u);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(u >> 32));
    return __builtin_bit_cast(double, (uint64_t)lo | ((uint64_t)hi << 32));
}

// PLANAR: fp32 NCHW destination (one LDS region and one byte range per plane)
// EXT: border modes other than CONSTANT (a separate instance, as warp_kernel)
template <int CC, typename TIn, int OUT, bool PLANAR, bool EXT>
__global__ void __launch_bounds__(kBlock)
warp_persp_rois_kernel(WarpPerspRoisLaunch L, int tiles, int total) {
    using TOut = typename std::conditional<(OUT == kOutSame), TIn, float>::type;
    constexpr bool kU8 = std::is_same<TIn, uint8_t>::value;
    constexpr bool kU8Norm = kU8 && (OUT == kOutNorm);
    constexpr int kPlanes = PLANAR ? CC : 1;
    constexpr int kPxB = (PLANAR ? 1 : CC) * (int)sizeof(TOut);  // bytes per pixel of one destination plane
    constexpr int kRegion = kRoiTile * kPxB + 16;                // + the destination's offset modulo 16
    __shared__ __attribute__((aligned(16))) unsigned char xch[kPlanes * kRegion];
    __shared__ double s_inv[9];
    __shared__ int s_frame;

    // an XCD walks a contiguous range of (ROI, tile), so the tiles of one ROI,
    // which share source lines, meet in one L2
    const int id = xcd_block_id(total);
    if (id >= total) return;  // uniform
    const int roi = id / tiles;
    const int tile = id - roi * tiles;
    // the wave index as a scalar: the per-run addresses of the pitched epilogue stay in SGPRs
    const int lane = threadIdx.x, wv = __builtin_amdgcn_readfirstlane((int)threadIdx.y);
    const int tid = wv * 64 + lane;

    // ---- the ROI's map and frame: one thread reads the device arrays and inverts
    if (tid == 0) {
        float m[9];
        double inv[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) m[k] = L.m[(int64_t)roi * 9 + k];
        if (L.inverse_map) {
#pragma unroll
            for (int k = 0; k < 9; ++k) inv[k] = (double)m[k];
        } else {
            invert_homography_value(m, inv);
        }
#pragma unroll
        for (int k = 0; k < 9; ++k) s_inv[k] = inv[k];
        s_frame = L.src_index ? L.src_index[roi] : (L.n_src == 1 ? 0 : roi);
    }
    __syncthreads();
    // into scalar registers: everything derived from them (the frame's buffer
    // resource above all) is then uniform for the compiler too
    double N[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) N[k] = uniform_d(s_inv[k]);
    const int frame = __builtin_amdgcn_readfirstlane(s_frame);
    const bool valid = frame >= 0 && frame < L.n_src;  // uniform; else: all border, nothing read

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
    TOut bval[CC];
#pragma unroll
    for (int k = 0; k < CC; ++k) {
        if (OUT == kOutNorm)
            bval[k] = kU8Norm ? (TOut)normalize_u8v(cn[k], (int)L.border[k])
                              : (TOut)normalize_value(L.border[k], nmean[k], nstd[k]);
        else
            bval[k] = (TOut)L.border[k];
    }

    const unsigned char* sp = L.src.base + (int64_t)(valid ? frame : 0) * L.src.img_pitch;
    const int64_t rp = L.src.row_pitch;
    const Rsrc srs = make_rsrc(sp, valid ? L.src.plane_bytes : 0);
    const uint32_t slimit = (valid ? (uint32_t)L.src.plane_bytes : 0u) + srs.delta;
    const uint32_t rp32 = (uint32_t)rp;  // plane_bytes <= kMaxPlaneBytes (launch_warp_persp_rois)
    const bool mul24 = rp < (1 << 24) && L.src.h < (1 << 24);

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
        float fx, fy;
        perspective_coords(N, x, y, fx, fy);
        int sx = 0, sy = 0;
        float ax = 0.f, ay = 0.f;
        const bool ok = valid && affine_tap(fy, L.src.h, sy, ay) && affine_tap(fx, L.src.w, sx, ax);
        if (!ok) {
            if (EXT && valid) {  // L.border_mode != kBorderConstant
                int vi[CC];
                float vf[CC];
                warp_border_sample<CC, TIn>(sp, rp, L.src.w, L.src.h, L.border_mode, fx, fy, vi, vf);
#pragma unroll
                for (int k = 0; k < CC; ++k) {
                    if (kU8) {
                        *o[k] = emit_u8<OUT, TOut>(cn[k], vi[k]);
                    } else {
                        *o[k] = (TOut)(OUT == kOutNorm ? normalize_value(vf[k], nmean[k], nstd[k]) : vf[k]);
                    }
                }
                continue;
            }
#pragma unroll
            for (int k = 0; k < CC; ++k) *o[k] = bval[k];
            continue;
        }
        const uint32_t o0 = (mul24 ? __umul24((uint32_t)sy, rp32) : (uint32_t)sy * rp32) +
                            (uint32_t)(sx * CC * (int)sizeof(TIn)) + srs.delta;
        const uint32_t o1 = o0 + rp32;
        if constexpr (kU8) {
            const int wy0 = warp_weight(ay), wy1 = 2048 - wy0;
            const int wx0 = warp_weight(ax), wx1 = 2048 - wx0;
            // the 2*CC tap bytes of each row in ONE dword-aligned buffer load;
            // a load past the frame's end (its last pixel) falls back to bytes
            uint32_t a0 = 0, a1 = 0, c0 = 0, c1 = 0;
            if ((o1 & ~3u) + 4u * kTapDwords<CC, true> <= slimit) {
                load_taps<CC, true, 0>(srs, o0, a0, a1);
                load_taps<CC, true, 0>(srs, o1, c0, c1);
            } else {
#pragma unroll
                for (int e = 0; e < 2 * CC; ++e) {
                    const uint32_t t0 = __builtin_amdgcn_raw_buffer_load_b8(srs.r, (int)(o0 + e), 0, 0);
                    const uint32_t t1 = __builtin_amdgcn_raw_buffer_load_b8(srs.r, (int)(o1 + e), 0, 0);
                    if (e < 4) { a0 |= t0 << (8 * e); c0 |= t1 << (8 * e); }
                    else { a1 |= t0 << (8 * (e - 4)); c1 |= t1 << (8 * (e - 4)); }
                }
            }
            // warp_affine_naive.cpp:50-54 as (tl*wx0 + tr*wx1)*wy0 + (bl*wx0 +
            // br*wx1)*wy1: the same int32 value (exact, <= 255*2^22)
            const us2 wx = __builtin_bit_cast(us2, (uint32_t)wx0 | ((uint32_t)wx1 << 16));
#pragma unroll
            for (int k = 0; k < CC; ++k) {
                // written out, not blend_rows: with the call the 1080p u8 crops measured 1.5-3 % slower
                const uint32_t top = tap_pair<CC>(a0, a1, k), bot = tap_pair<CC>(c0, c1, k);
                const uint32_t ht = __builtin_amdgcn_udot2(__builtin_bit_cast(us2, top), wx, 0u, false);
                const uint32_t hb = __builtin_amdgcn_udot2(__builtin_bit_cast(us2, bot), wx, 0u, false);
                const int v = (int)((__umul24(ht, (uint32_t)wy0) + __umul24(hb, (uint32_t)wy1)) >> 22);
                *o[k] = emit_u8<OUT, TOut>(cn[k], v);
            }
        } else {
            const float yy0 = 1.f - ay, yy1 = ay, xa = 1.f - ax, xb = ax;
            float f0[2 * CC], f1[2 * CC];
            load_f32<2 * CC>(srs, o0, f0);
            load_f32<2 * CC>(srs, o1, f1);
#pragma unroll
            for (int k = 0; k < CC; ++k) {
                // warp_affine_naive.cpp:98-102, left to right
                float v = f0[k] * xa * yy0;
                v += f1[k] * xa * yy1;
                v += f0[CC + k] * xb * yy0;
                v += f1[CC + k] * xb * yy1;
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

template <int CC, typename TIn, int OUT, bool PLANAR>
hipError_t launch_ext(const WarpPerspRoisLaunch& L, hipStream_t s) {
    const int64_t px = (int64_t)L.dst.w * L.dst.h;
    const int64_t tiles = (px + kRoiTile - 1) / kRoiTile;
    const int64_t total = tiles * L.n_roi;
    if (total >= 0x7FFFFFF0LL) return hipErrorInvalidValue;
    const int64_t blocks = (total + 7) / 8 * 8;
    if (L.border_mode == kBorderConstant)
        hipLaunchKernelGGL((warp_persp_rois_kernel<CC, TIn, OUT, PLANAR, false>), dim3((unsigned)blocks), dim3(64, 4), 0, s, L,
                           (int)tiles, (int)total);
    else
        hipLaunchKernelGGL((warp_persp_rois_kernel<CC, TIn, OUT, PLANAR, true>), dim3((unsigned)blocks), dim3(64, 4), 0, s, L,
                           (int)tiles, (int)total);
    return hipGetLastError();
}

template <typename TIn, int OUT>
hipError_t launch_cc(const WarpPerspRoisLaunch& L, hipStream_t s) {
    if (L.planar) {
        if constexpr (OUT == kOutNorm) {
            if (L.src.cc == 3) return launch_ext<3, TIn, OUT, true>(L, s);
        }
        return hipErrorInvalidValue;
    }
    switch (L.src.cc) {
        case 1: return launch_ext<1, TIn, OUT, false>(L, s);
        case 2: return launch_ext<2, TIn, OUT, false>(L, s);
        case 3: return launch_ext<3, TIn, OUT, false>(L, s);
        case 4: return launch_ext<4, TIn, OUT, false>(L, s);
        default: return hipErrorInvalidValue;
    }
}

}  // namespace

hipError_t launch_warp_persp_rois(const WarpPerspRoisLaunch& L, hipStream_t s) {
    // the kernel's 32-bit source offsets, its float row/column split
    // (divmod_w) and its int pixel index
    if (L.src.plane_bytes > kMaxPlaneBytes || L.dst.w > (1 << 20) || (int64_t)L.dst.w * L.dst.h > 0x7FFF0000LL)
        return hipErrorInvalidValue;
    if (L.src.esize == 1) {
        if (L.out == kOutSame) return launch_cc<uint8_t, kOutSame>(L, s);
        return launch_cc<uint8_t, kOutNorm>(L, s);
    }
    if (L.out == kOutNorm) return launch_cc<float, kOutNorm>(L, s);
    return launch_cc<float, kOutSame>(L, s);
}

}  // namespace vacv
