// roi_tile.hpp -- the tiling helpers of the ROI kernels (k_warp_rois.hip,
// k_yuv_rois.hip, k_crop_resize_rois.hip, k_yuv_crop_resize_rois.hip): a
// workgroup owns kRoiTile consecutive row-major pixels of one ROI, lays its
// band out in LDS at the destination's offset modulo 16 and copies it out in
// the widest stores the alignment allows.  The two YUV kernels share the
// decode of one tap.
#pragma once

#include "vacv_device.hpp"

namespace vacv {
namespace {

constexpr int kRoiPx = 4;                // 64-pixel gathers per wave
constexpr int kRoiTile = kBlock * kRoiPx;  // pixels per workgroup

// p / w and p % w for p < w + kRoiTile, w <= 2^20 (rw = 1.f / w): the float
// quotient is within one of the true one, the remainder test settles it
__device__ __forceinline__ void divmod_w(uint32_t p, uint32_t w, float rw, int& q, int& r) {
    int qq = (int)((float)p * rw);
    int rr = (int)p - qq * (int)w;
    if (rr < 0) { --qq; rr += (int)w; }
    else if (rr >= (int)w) { ++qq; rr -= (int)w; }
    q = qq;
    r = rr;
}

__device__ __forceinline__ float uniform_f(float v) {
    return __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, v)));
}

// N consecutive floats at buffer byte offset `off`, one range-checked dword
// load each (the compiler merges neighbours where it can prove it may)
template <int N>
__device__ __forceinline__ void load_f32(const Rsrc& rs, uint32_t off, float (&v)[N]) {
#pragma unroll
    for (int i = 0; i < N; ++i)
        v[i] = __builtin_bit_cast(float, (uint32_t)__builtin_amdgcn_raw_buffer_load_b32(rs.r, (int)(off + 4u * i), 0, 0));
}

// One tap: Y and its chroma pair (byte 0 and byte 1 of `pair`, in memory
// order) to the three output channels, cvt_color.cpp:76-86 as color_kernel
__device__ __forceinline__ void decode_tap(int Y, uint32_t pair, bool v_first, bool rgb, int (&c)[3]) {
    const int b0 = (int)(pair & 0xFFu), b1 = (int)((pair >> 8) & 0xFFu);
    const int v = v_first ? b0 : b1;
    const int u = v_first ? b1 : b0;
    const Chroma ch = chroma_terms(u, v);
    const int R = clamp_u8(Y + ch.ra), G = clamp_u8(Y - ch.ga), B = clamp_u8(Y + ch.ba);
    c[0] = rgb ? R : B;
    c[1] = G;
    c[2] = rgb ? B : R;
}

__device__ __forceinline__ uint32_t load_u8(const Rsrc& rs, uint32_t off) {
    return (uint32_t)__builtin_amdgcn_raw_buffer_load_b8(rs.r, (int)off, 0, 0);
}

// nbytes from LDS offset `lo` of xch (16-byte aligned) to d, by threads t of
// nt: 16-byte stores where LDS offset and destination agree modulo 16,
// dwords where they agree modulo 4, else bytes; heads and tails bytewise.
// The loops stay rolled: a band is at most a few 16-byte chunks per thread,
// and the unrolled copies held the kernel at half of warp_kernel's occupancy.
__device__ __forceinline__ void copy_run(unsigned char* d, const unsigned char* xch, uint32_t lo, int nbytes, int t,
                                         int nt) {
    const uintptr_t da = reinterpret_cast<uintptr_t>(d);
    const unsigned char* xs = xch + lo;
    const uint32_t diff = ((uint32_t)da ^ lo);
    if ((diff & 15u) == 0) {  // uniform per run
        const int head = min(nbytes, (int)((16u - ((uint32_t)da & 15u)) & 15u));
        const int nmid = (nbytes - head) >> 4;
#pragma unroll 1
        for (int e = t; e < head; e += nt) d[e] = xs[e];
#pragma unroll 1
        for (int c = t; c < nmid; c += nt)
            __builtin_nontemporal_store(*reinterpret_cast<const u32x4*>(xs + head + 16 * c),
                                        reinterpret_cast<u32x4*>(d + head) + c);
#pragma unroll 1
        for (int e = head + 16 * nmid + t; e < nbytes; e += nt) d[e] = xs[e];
    } else if ((diff & 3u) == 0) {
        const int head = min(nbytes, (int)((4u - ((uint32_t)da & 3u)) & 3u));
        const int nmid = (nbytes - head) >> 2;
#pragma unroll 1
        for (int e = t; e < head; e += nt) d[e] = xs[e];
#pragma unroll 1
        for (int c = t; c < nmid; c += nt)
            reinterpret_cast<uint32_t*>(d + head)[c] = *reinterpret_cast<const uint32_t*>(xs + head + 4 * c);
#pragma unroll 1
        for (int e = head + 4 * nmid + t; e < nbytes; e += nt) d[e] = xs[e];
    } else {
#pragma unroll 1
        for (int e = t; e < nbytes; e += nt) d[e] = xs[e];
    }
}

}  // namespace
}  // namespace vacv
