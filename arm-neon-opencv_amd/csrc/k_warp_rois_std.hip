// k_warp_rois_std.hip -- many small affine crops in one launch, each
// standardized by its OWN per-channel mean and standard deviation: ROI i of
// the destination is normalize(warp_affine(frame src_index[i], m[i]), NULL,
// NULL), the reference's warp_affine_normalize with mean and stddev left
// empty (warp_affine_normalize.cpp:145-164), both arrays read from DEVICE
// memory when the kernel runs.  u8 frames only.
//
// The work shape is k_crop_resize_rois_std.hip's: a ROI's statistics span all
// its pixels, border pixels included, so ONE WORKGROUP PER ROI holds the whole
// u8 ROI in LDS:
//   head   256 bytes: the inverted map and the frame, the integer sums, the
//          statistics
//   px     the warped u8 ROI, w h c bytes rounded up to 16: interleaved
//          [h][w][c] for an NHWC destination, [c][h][w] for a planar one, so
//          that every destination run reads consecutive LDS bytes
//   lut    [c][256] floats: the normalized value of every u8 value of every
//          channel
// warp_rois_std_lds_bytes() is that sum; the host refuses what passes 64 KiB.
//
// Bit identity with the chain vacv_warp_affine_rois (u8) -> vacv_mean_stddev ->
// vacv_normalize(NULL, NULL) -> vacv_change_layout rests on:
//  1. the u8 ROI is warp_rois_kernel's kOutSame one: the same inverse
//     (invert_affine_value), the same coordinate, tap and weights, the same
//     loads (load_taps, bytes at the frame's end) and blend, the same border
//     pixels (warp_border_sample, or the u8 border value);
//  2. the sums of a u8 ROI are integers, so their order is free: channel_sums'
//     doubles hold the same integers (below 2^53) exactly;
//  3. the statistics are stats_kernel's expressions (k_pixel.hip) and the
//     normalized value is normalize_value (vacv_semantics.hpp), separately
//     rounded fp64 operations in one order (contraction off).
// tests/test_warp_rois_std_gpu.py compares with that chain and with the CPU
// oracle bit for bit.
//
// A u8 value has only 256 normalized results per channel: the workgroup builds
// them once (256 c exact divides, not w h c) and a pixel is one LDS byte, one
// LDS float and its share of a 16-byte store.  Device-supplied values cannot
// fault: an index outside [0, n_src) reads nothing -- its resource spans zero
// bytes -- and is the chain's ROI of border_value; every sampler read goes
// through a buffer resource that spans exactly the indexed frame, and the
// border modes' taps are mapped into it by border_index.
#pragma clang fp contract(off)

#include "roi_tile.hpp"
#include "vacv_device.hpp"

namespace vacv {
namespace {

// 16 waves: with a workgroup per ROI a batch of 256 ROIs is one workgroup per
// CU, and the sampling stage is latency-bound gathers.  k_crop_resize_rois_std.hip's
// measured choice for the same work shape, taken over; 256 and
// 512 were not measured here (-DVACV_WARP_STD_BLOCK builds them)
#ifndef VACV_WARP_STD_BLOCK
#define VACV_WARP_STD_BLOCK 1024
#endif
constexpr int kStdBlock = VACV_WARP_STD_BLOCK;
static_assert(kStdBlock % 64 == 0 && kStdBlock >= 64 && kStdBlock <= 1024, "whole waves, one workgroup");
constexpr int kStdHeadBytes = 256;

struct WarpStdHead {
    float inv[6];  // the dst -> src map
    int frame;     // src_index[roi], as read
    int pad;
    // per channel Sum v [0..3] and Sum v^2 [4..7].  No overflow: a ROI that
    // fits the LDS budget has at most 64,256 pixels, so Sum v^2 <= 64,256 *
    // 65,025 < 2^32 even in a thread's uint32 partial; the workgroup's totals
    // are 64-bit all the same, which needs no such argument
    unsigned long long sum[8];
    float mean[4], stdv[4];
};
static_assert(sizeof(WarpStdHead) <= kStdHeadBytes, "the head of the LDS block");

// What the sampler needs of the ROI's frame, all uniform
struct StdFrame {
    const unsigned char* sp;  // the frame's first byte
    Rsrc srs;                 // exactly the frame, or zero bytes (invalid index)
    uint32_t slimit, rp32;
    bool mul24, valid;
};

// The CC u8 values of ROI pixel (x, y) under the dst -> src map iv:
// warp_rois_kernel's u8 kOutSame arithmetic, expression for expression.  (The
// stage a decoded YUV tap would replace.)
template <int CC, bool EXT>
__device__ __forceinline__ void sample_u8(const WarpRoisStdLaunch& L, const StdFrame& F, const float (&iv)[6], int x,
                                          int y, int (&v)[CC]) {
    // warp_affine_naive.cpp:23-24: (m0*x + m1*y) + m2, all float
    const float fx = iv[0] * (float)x + iv[1] * (float)y + iv[2];
    const float fy = iv[3] * (float)x + iv[4] * (float)y + iv[5];
    int sx = 0, sy = 0;
    float ax = 0.f, ay = 0.f;
    const bool ok = F.valid && affine_tap(fy, L.src.h, sy, ay) && affine_tap(fx, L.src.w, sx, ax);
    if (!ok) {
        if (EXT && F.valid) {  // L.border_mode != kBorderConstant
            float vf[CC];
            warp_border_sample<CC, uint8_t>(F.sp, L.src.row_pitch, L.src.w, L.src.h, L.border_mode, fx, fy, v, vf);
#pragma unroll
            for (int k = 0; k < CC; ++k) v[k] = (int)(uint8_t)v[k];
            return;
        }
#pragma unroll
        for (int k = 0; k < CC; ++k) v[k] = (int)(uint8_t)L.border[k];
        return;
    }
    const uint32_t o0 = (F.mul24 ? __umul24((uint32_t)sy, F.rp32) : (uint32_t)sy * F.rp32) + (uint32_t)(sx * CC) +
                        F.srs.delta;
    const uint32_t o1 = o0 + F.rp32;
    const int wy0 = warp_weight(ay), wy1 = 2048 - wy0;
    const int wx0 = warp_weight(ax), wx1 = 2048 - wx0;
    // the 2*CC tap bytes of each row in ONE dword-aligned buffer load;
    // a load past the frame's end (its last pixel) falls back to bytes
    uint32_t a0 = 0, a1 = 0, c0 = 0, c1 = 0;
    if ((o1 & ~3u) + 4u * kTapDwords<CC, true> <= F.slimit) {
        load_taps<CC, true, 0>(F.srs, o0, a0, a1);
        load_taps<CC, true, 0>(F.srs, o1, c0, c1);
    } else {
#pragma unroll
        for (int e = 0; e < 2 * CC; ++e) {
            const uint32_t t0 = __builtin_amdgcn_raw_buffer_load_b8(F.srs.r, (int)(o0 + e), 0, 0);
            const uint32_t t1 = __builtin_amdgcn_raw_buffer_load_b8(F.srs.r, (int)(o1 + e), 0, 0);
            if (e < 4) { a0 |= t0 << (8 * e); c0 |= t1 << (8 * e); }
            else { a1 |= t0 << (8 * (e - 4)); c1 |= t1 << (8 * (e - 4)); }
        }
    }
    // warp_affine_naive.cpp:50-54 as (tl*wx0 + tr*wx1)*wy0 + (bl*wx0 +
    // br*wx1)*wy1: the same int32 value (exact, <= 255*2^22)
    const us2 wx = __builtin_bit_cast(us2, (uint32_t)wx0 | ((uint32_t)wx1 << 16));
#pragma unroll
    for (int k = 0; k < CC; ++k) {
        const uint32_t top = tap_pair<CC>(a0, a1, k), bot = tap_pair<CC>(c0, c1, k);
        const uint32_t ht = __builtin_amdgcn_udot2(__builtin_bit_cast(us2, top), wx, 0u, false);
        const uint32_t hb = __builtin_amdgcn_udot2(__builtin_bit_cast(us2, bot), wx, 0u, false);
        v[k] = (int)((__umul24(ht, (uint32_t)wy0) + __umul24(hb, (uint32_t)wy1)) >> 22);
    }
}

// n floats to d (4-byte aligned) by threads t of nt: element j is the
// normalized value of LDS byte px[b0 + j], of channel k (PLANAR) or j % CC (a
// run starts at a pixel).  16-byte stores from the destination's first
// 16-byte boundary on, dwords before it and after the last whole one.  px is
// 16-byte aligned and followed by the table, so the dword past a run's last
// byte is LDS of this workgroup.  (k_crop_resize_rois_std.hip's, duplicated:
// that kernel stays as it was measured.)
template <int CC, bool PLANAR>
__device__ __forceinline__ void store_run(float* d, const unsigned char* px, uint32_t b0, int n, int k,
                                          const float* lut, int t, int nt) {
    auto one = [&](int j) { return lut[(PLANAR ? k : j % CC) * 256 + px[b0 + j]]; };
    const int head = min(n, (int)(((16u - ((uint32_t)reinterpret_cast<uintptr_t>(d) & 15u)) & 15u) >> 2));
    const int nmid = (n - head) >> 2;
#pragma unroll 1
    for (int j = t; j < head; j += nt) d[j] = one(j);
#pragma unroll 1
    for (int g = t; g < nmid; g += nt) {
        const int j = head + 4 * g;
        const uint32_t o = b0 + (uint32_t)j;
        const uint32_t* wp = reinterpret_cast<const uint32_t*>(px) + (o >> 2);
        const uint32_t b = __builtin_amdgcn_alignbyte(wp[1], wp[0], o & 3u);
        const int c0 = PLANAR ? k : j % CC;
        u32x4 f;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int ch = PLANAR ? k : (c0 + i) % CC;
            f[i] = __builtin_bit_cast(uint32_t, lut[ch * 256 + ((b >> (8 * i)) & 0xFFu)]);
        }
        __builtin_nontemporal_store(f, reinterpret_cast<u32x4*>(d + j));
    }
#pragma unroll 1
    for (int j = head + 4 * nmid + t; j < n; j += nt) d[j] = one(j);
}

// PLANAR: NCHW destination of CC > 1 channels (one run set per plane)
// EXT: border modes other than CONSTANT (a separate instance, as warp_rois_kernel)
template <int CC, bool PLANAR, bool EXT>
__global__ void __launch_bounds__(kStdBlock) warp_rois_std_kernel(WarpRoisStdLaunch L) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    const int w = L.dst.w, h = L.dst.h, npx = w * h;  // <= 64,256 (the host's LDS gate)
    WarpStdHead* hd = reinterpret_cast<WarpStdHead*>(lds);
    unsigned char* px = lds + kStdHeadBytes;
    const int px_bytes = (npx * CC + 15) & ~15;
    float* lut = reinterpret_cast<float*>(px + px_bytes);
    const int roi = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);

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
    if (tid < 8) hd->sum[tid] = 0ull;
    __syncthreads();
    // into scalar registers: everything derived from them (the frame's buffer
    // resource above all) is then uniform for the compiler too
    float iv[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) iv[k] = uniform_f(hd->inv[k]);
    const int frame = __builtin_amdgcn_readfirstlane(hd->frame);

    StdFrame F;
    F.valid = frame >= 0 && frame < L.n_src;  // uniform; else: all border, nothing read
    F.sp = L.src.base + (int64_t)(F.valid ? frame : 0) * L.src.img_pitch;
    F.srs = make_rsrc(F.sp, F.valid ? L.src.plane_bytes : 0);
    F.slimit = (F.valid ? (uint32_t)L.src.plane_bytes : 0u) + F.srs.delta;
    F.rp32 = (uint32_t)L.src.row_pitch;  // plane_bytes <= kMaxPlaneBytes (the host's gate)
    F.mul24 = L.src.row_pitch < (1 << 24) && L.src.h < (1 << 24);

    // ---- the u8 ROI into LDS, its sums into registers: 64 consecutive pixels per gather
    uint32_t s1[CC], s2[CC];
#pragma unroll
    for (int k = 0; k < CC; ++k) s1[k] = s2[k] = 0u;
    const float rw = 1.f / (float)w;
#pragma unroll 1
    for (int p = tid; p < npx; p += kStdBlock) {
        int y, x;  // p < 2^16: the float quotient is within one (divmod_w)
        divmod_w((uint32_t)p, (uint32_t)w, rw, y, x);
        int v[CC];
        sample_u8<CC, EXT>(L, F, iv, x, y, v);
#pragma unroll
        for (int k = 0; k < CC; ++k) {
            px[PLANAR ? k * npx + p : p * CC + k] = (unsigned char)v[k];
            s1[k] += (uint32_t)v[k];
            s2[k] += (uint32_t)(v[k] * v[k]);
        }
    }
    // per wave, then per workgroup: integers, so any order is the same sum
#pragma unroll
    for (int k = 0; k < CC; ++k) {
        const unsigned long long t1 = wave_sum((unsigned long long)s1[k]);
        const unsigned long long t2 = wave_sum((unsigned long long)s2[k]);
        if (lane == 0) {
            atomicAdd(&hd->sum[k], t1);
            atomicAdd(&hd->sum[4 + k], t2);
        }
    }
    __syncthreads();

    // ---- the statistics: stats_kernel's expressions (k_pixel.hip) on the same integers
    if (tid < CC) {
        const double count = (double)w * h;
        const double m = (double)hd->sum[tid] / count;
        double var = (double)hd->sum[4 + tid] / count - m * m;
        if (var < 0) var = 0;
        const float mf = (float)m, sf = (float)sqrt(var);
        hd->mean[tid] = mf;
        hd->stdv[tid] = sf;
        if (L.mean_out) L.mean_out[(int64_t)roi * CC + tid] = mf;
        if (L.stddev_out) L.stddev_out[(int64_t)roi * CC + tid] = sf;
    }
    __syncthreads();

    // ---- every u8 value's normalized float, the exact divide once per (channel, value)
#pragma unroll 1
    for (int e = tid; e < 256 * CC; e += kStdBlock) {
        const int k = e >> 8;
        lut[e] = normalize_value((float)(e & 255), hd->mean[k], hd->stdv[k]);
    }
    __syncthreads();

    // ---- LDS -> HBM: one run per plane of dense rows, else one per row
    constexpr int kPlanes = PLANAR ? CC : 1;
    const int row_el = w * (PLANAR ? 1 : CC);  // floats per destination row
    unsigned char* dbase = const_cast<unsigned char*>(L.dst.base) + (int64_t)roi * L.dst.img_pitch;
    if (L.dst.row_pitch == (int64_t)row_el * 4) {  // uniform
#pragma unroll
        for (int k = 0; k < kPlanes; ++k)
            store_run<CC, PLANAR>(reinterpret_cast<float*>(dbase + (int64_t)k * L.dst.plane_pitch), px,
                                  (uint32_t)(k * npx), h * row_el, k, lut, tid, kStdBlock);
        return;
    }
#pragma unroll 1
    for (int r = wave; r < kPlanes * h; r += kStdBlock / 64) {  // wave r % 16 stores run r = (plane, row)
        const int k = PLANAR ? r / h : 0;
        const int y = r - k * h;
        store_run<CC, PLANAR>(
            reinterpret_cast<float*>(dbase + (int64_t)k * L.dst.plane_pitch + (int64_t)y * L.dst.row_pitch), px,
            (uint32_t)(k * npx + y * row_el), row_el, k, lut, lane, 64);
    }
}

template <int CC, bool PLANAR>
hipError_t launch_ext(const WarpRoisStdLaunch& L, size_t lds, hipStream_t s) {
    const dim3 grid(L.n_roi), block(kStdBlock);
    if (L.border_mode == kBorderConstant)
        hipLaunchKernelGGL((warp_rois_std_kernel<CC, PLANAR, false>), grid, block, lds, s, L);
    else
        hipLaunchKernelGGL((warp_rois_std_kernel<CC, PLANAR, true>), grid, block, lds, s, L);
    return hipGetLastError();
}

}  // namespace

// A workgroup's dynamic LDS: the head, the u8 ROI and the table of normalized
// values (the layout at the top of this file)
size_t warp_rois_std_lds_bytes(int w, int h, int c) {
    const size_t px = ((size_t)w * h * c + 15) / 16 * 16;
    return kStdHeadBytes + px + 1024 * (size_t)c;
}

bool warp_rois_std_fits(const WarpRoisStdLaunch& L) {
    // one workgroup's LDS (so w h < 2^16); kStdBlock threads per ROI within a 32-bit grid
    return warp_rois_std_lds_bytes(L.dst.w, L.dst.h, L.src.cc) <= 64 * 1024 &&
           L.n_roi <= (int)(0xFFFFFFFFu / kStdBlock);
}

hipError_t launch_warp_rois_std(const WarpRoisStdLaunch& L, hipStream_t s) {
    // warp_rois_kernel's 32-bit source offsets, then this work shape's limits
    if (L.src.plane_bytes > kMaxPlaneBytes || !warp_rois_std_fits(L) || L.src.esize != 1) return hipErrorInvalidValue;
    const size_t lds = warp_rois_std_lds_bytes(L.dst.w, L.dst.h, L.src.cc);
    if (L.planar) return L.src.cc == 3 ? launch_ext<3, true>(L, lds, s) : hipErrorInvalidValue;
    switch (L.src.cc) {
        case 1: return launch_ext<1, false>(L, lds, s);
        case 2: return launch_ext<2, false>(L, lds, s);
        case 3: return launch_ext<3, false>(L, lds, s);
        case 4: return launch_ext<4, false>(L, lds, s);
        default: return hipErrorInvalidValue;
    }
}

}  // namespace vacv
