// k_crop_resize_rois_std.hip -- many upright crops in one launch, each
// standardized by its OWN per-channel mean and standard deviation: ROI i of
// the destination is normalize(resize(crop(frame src_index[i], rects[i]),
// w x h), NULL, NULL), the reference's default normalize of a crop
// (normalize.cpp:84-121), both arrays read from DEVICE memory when the kernel
// runs.  u8 frames only.
//
// A ROI's statistics span all its pixels, so roi_tile.hpp's 1,024-pixel tiles
// cannot finish a ROI alone: ONE WORKGROUP PER ROI (match_rois_kernel's work
// shape), the whole u8 ROI in LDS:
//   head   256 bytes: the validated rect and frame, the integer sums, the
//          statistics
//   px     the resized u8 ROI, w h c bytes rounded up to 16: interleaved
//          [h][w][c] for an NHWC destination, [c][h][w] for a planar one, so
//          that every destination run reads consecutive LDS bytes
//   tab    the x taps of all w columns, then the y taps of all h rows: 8 bytes
//          each.  Dead once the ROI is sampled, and then
//   lut    [c][256] floats over the same bytes: the normalized value of every
//          u8 value of every channel
// crop_resize_rois_std_lds_bytes() is that sum; the host refuses what passes
// 64 KiB.
//
// Bit identity with the chain vacv_crop_resize_rois (u8) -> vacv_mean_stddev ->
// vacv_normalize(NULL, NULL) -> vacv_change_layout rests on:
//  1. the u8 ROI is crop_resize_rois_kernel's: the same tap (fixed_tap of the
//     RECT's size, offset by left / top), the same loads (load_taps, bytes at
//     the frame's end), the same blend (blend_fixed);
//  2. the sums of a u8 ROI are integers, so their order is free: channel_sums'
//     doubles hold the same integers (below 2^53) exactly;
//  3. the statistics are stats_kernel's expressions (k_pixel.hip) and the
//     normalized value is normalize_value (vacv_semantics.hpp), separately
//     rounded fp64 operations in one order (contraction off).
// tests/test_crop_resize_rois_std_gpu.py compares with that chain and with the
// CPU oracle bit for bit.
//
// Per-ROI statistics cannot be host-verified for normalize_u8v's short forms,
// so the exact form is the fp64 divide -- but a u8 value has only 256 results
// per channel: the workgroup builds them once (256 c divides, not w h c) and a
// pixel is one LDS byte, one LDS float and its share of a 16-byte store.
// Device-supplied values cannot fault: one thread validates the rect and the
// index (range checks, no int overflow); an invalid ROI reads nothing -- its
// resource spans zero bytes -- and is the chain's ROI of u8 zeros: mean 0,
// stddev 0, output +0.0; every source read goes through a buffer resource that
// spans exactly the indexed frame.
#pragma clang fp contract(off)

#include "roi_tile.hpp"
#include "vacv_device.hpp"

namespace vacv {
namespace {

// 16 waves: with a workgroup per ROI a batch of 256 ROIs is one workgroup per
// CU, and the sampling stage is latency-bound gathers -- 4 waves per SIMD
// instead of kBlock's 1 (DESIGN.md 3.17 has the measurement; -DVACV_STD_BLOCK
// builds the variants it compares)
#ifndef VACV_STD_BLOCK
#define VACV_STD_BLOCK 1024
#endif
constexpr int kStdBlock = VACV_STD_BLOCK;
static_assert(kStdBlock % 64 == 0 && kStdBlock >= 64 && kStdBlock <= 1024, "whole waves, one workgroup");
constexpr int kStdHeadBytes = 256;

struct StdHead {
    int roi[5];        // left, top, width, height, frame (-1: invalid)
    int pad;
    // per channel Sum v [0..3] and Sum v^2 [4..7].  No overflow: a ROI that
    // fits the LDS budget has fewer than 65,536 pixels, so Sum v^2 <= 65,535 *
    // 65,025 < 2^32 even in a thread's uint32 partial; the workgroup's totals
    // are 64-bit all the same, which needs no such argument
    unsigned long long sum[8];
    float mean[4], stdv[4];
};
static_assert(sizeof(StdHead) <= kStdHeadBytes, "the head of the LDS block");

// One tap of a column (origin = left, step = bytes per pixel) or a row
// (origin = top, step = row pitch), as crop_resize_rois_kernel tables it:
// .x = byte offset of the first tap in the frame, .y = w0 | w1 << 16
__device__ __forceinline__ uint2 std_tap(int d, int n_in, int n_out, float scale_f, double scale_d, int mode,
                                         int origin, uint32_t step) {
    const FixedTap t = fixed_tap(d, n_in, n_out, scale_f, scale_d, mode);
    return make_uint2((uint32_t)(t.i + origin) * step, (uint32_t)t.w0 | ((uint32_t)t.w1 << 16));
}

// The CC u8 values of the output pixel with column tap cx and row tap ry:
// crop_resize_rois_kernel's loads and blend.  (The stage a decoded YUV tap
// would replace.)
template <int CC, bool REF>
__device__ __forceinline__ void sample_u8(const Rsrc& srs, uint32_t slimit, uint32_t rp32, uint2 cx, uint2 ry,
                                          int (&v)[CC]) {
    // both taps of both rows lie inside the validated rect, so inside the frame
    const uint32_t o0 = ry.x + cx.x + srs.delta;
    const uint32_t o1 = o0 + rp32;
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
        v[k] = blend_fixed<REF ? VACV_LINEAR_REFERENCE : VACV_LINEAR_NEON>(tp, bt, wx, wA, wB);
    }
}

// n floats to d (4-byte aligned) by threads t of nt: element j is the
// normalized value of LDS byte px[b0 + j], of channel k (PLANAR) or j % CC (a
// run starts at a pixel).  16-byte stores from the destination's first
// 16-byte boundary on, dwords before it and after the last whole one.  px is
// 16-byte aligned and followed by the table, so the dword past a run's last
// byte is LDS of this workgroup.
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
// REF: VACV_LINEAR_REFERENCE's blend (else the NEON / OPENCV two-pass one; the
// rounding of their weights is fixed_tap's, by L.mode)
template <int CC, bool PLANAR, bool REF>
__global__ void __launch_bounds__(kStdBlock) crop_resize_rois_std_kernel(CropResizeRoisStdLaunch L) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    constexpr uint32_t kInPx = CC;  // bytes per source pixel
    const int w = L.dst.w, h = L.dst.h, npx = w * h;  // < 65,536 (the host's LDS gate)
    StdHead* hd = reinterpret_cast<StdHead*>(lds);
    unsigned char* px = lds + kStdHeadBytes;
    const int px_bytes = (npx * CC + 15) & ~15;
    uint2* tab = reinterpret_cast<uint2*>(px + px_bytes);
    float* lut = reinterpret_cast<float*>(px + px_bytes);
    const int roi = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);

    // ---- the ROI's rect and frame: one thread reads the device arrays and validates
    if (tid == 0) {
        const int32_t* r = L.rects + (int64_t)roi * 4;
        const int l = r[0], t = r[1], cw = r[2], ch = r[3];
        const int f = L.src_index ? L.src_index[roi] : (L.n_src == 1 ? 0 : roi);
        // left + width <= W as left <= W - width: no sum of two device values
        const bool ok = f >= 0 && f < L.n_src && cw >= 2 && ch >= 2 && l >= 0 && t >= 0 && cw <= L.src.w &&
                        l <= L.src.w - cw && ch <= L.src.h && t <= L.src.h - ch;
        hd->roi[0] = l;
        hd->roi[1] = t;
        hd->roi[2] = cw;
        hd->roi[3] = ch;
        hd->roi[4] = ok ? f : -1;
    }
    if (tid < 8) hd->sum[tid] = 0ull;
    __syncthreads();
    // into scalar registers: everything derived from them (the frame's buffer
    // resource above all) is then uniform for the compiler too
    const int left = __builtin_amdgcn_readfirstlane(hd->roi[0]), top = __builtin_amdgcn_readfirstlane(hd->roi[1]);
    const int cw = __builtin_amdgcn_readfirstlane(hd->roi[2]), ch = __builtin_amdgcn_readfirstlane(hd->roi[3]);
    const int frame = __builtin_amdgcn_readfirstlane(hd->roi[4]);
    const bool valid = frame >= 0;  // uniform; else: u8 zeros, nothing read

    const unsigned char* sp = L.src.base + (int64_t)(valid ? frame : 0) * L.src.img_pitch;
    const Rsrc srs = make_rsrc(sp, valid ? L.src.plane_bytes : 0);
    const uint32_t slimit = (valid ? (uint32_t)L.src.plane_bytes : 0u) + srs.delta;
    const uint32_t rp32 = (uint32_t)L.src.row_pitch;  // plane_bytes <= kMaxPlaneBytes (the host's gate)

    // ---- the taps of all columns and all rows, once per ROI
    // resize_naive.cpp:17-18: float division; resize_neon.cpp:17-18: double
    if (valid) {
        const float sxf = (float)cw / (float)w, syf = (float)ch / (float)h;
        const double sxd = (double)cw / (double)w, syd = (double)ch / (double)h;
#pragma unroll 1
        for (int e = tid; e < w + h; e += kStdBlock) {
            if (e < w) tab[e] = std_tap(e, cw, w, sxf, sxd, L.mode, left, kInPx);
            else tab[e] = std_tap(e - w, ch, h, syf, syd, L.mode, top, rp32);
        }
    }
    __syncthreads();

    // ---- the u8 ROI into LDS, its sums into registers: 64 consecutive pixels per gather
    uint32_t s1[CC], s2[CC];
#pragma unroll
    for (int k = 0; k < CC; ++k) s1[k] = s2[k] = 0u;
    const float rw = 1.f / (float)w;
#pragma unroll 1
    for (int p = tid; p < npx; p += kStdBlock) {
        int v[CC];
        if (valid) {
            int y, x;  // p < 2^16: the float quotient is within one (divmod_w)
            divmod_w((uint32_t)p, (uint32_t)w, rw, y, x);
            sample_u8<CC, REF>(srs, slimit, rp32, tab[x], tab[w + y], v);
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
    __syncthreads();  // the taps are dead from here

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
hipError_t launch_blend(const CropResizeRoisStdLaunch& L, size_t lds, hipStream_t s) {
    const dim3 grid(L.n_roi), block(kStdBlock);
    if (L.mode == VACV_LINEAR_REFERENCE)
        hipLaunchKernelGGL((crop_resize_rois_std_kernel<CC, PLANAR, true>), grid, block, lds, s, L);
    else
        hipLaunchKernelGGL((crop_resize_rois_std_kernel<CC, PLANAR, false>), grid, block, lds, s, L);
    return hipGetLastError();
}

}  // namespace

// A workgroup's dynamic LDS: the head, the u8 ROI, and the taps or the table
// of normalized values, whichever is larger (the layout at the top of this file)
size_t crop_resize_rois_std_lds_bytes(int w, int h, int c) {
    const size_t px = ((size_t)w * h * c + 15) / 16 * 16;
    const size_t taps = 8 * ((size_t)w + h), lut = 1024 * (size_t)c;
    return kStdHeadBytes + px + (taps > lut ? taps : lut);
}

bool crop_resize_rois_std_fits(const CropResizeRoisStdLaunch& L) {
    // crop_resize_rois_kernel's 32-bit source offsets; one workgroup's LDS
    // (so w h < 2^16); kStdBlock threads per ROI within a 32-bit grid
    return L.src.plane_bytes <= kMaxPlaneBytes &&
           crop_resize_rois_std_lds_bytes(L.dst.w, L.dst.h, L.src.cc) <= 64 * 1024 &&
           L.n_roi <= (int)(0xFFFFFFFFu / kStdBlock);
}

hipError_t launch_crop_resize_rois_std(const CropResizeRoisStdLaunch& L, hipStream_t s) {
    if (!crop_resize_rois_std_fits(L) || L.src.esize != 1) return hipErrorInvalidValue;
    const size_t lds = crop_resize_rois_std_lds_bytes(L.dst.w, L.dst.h, L.src.cc);
    if (L.planar) return L.src.cc == 3 ? launch_blend<3, true>(L, lds, s) : hipErrorInvalidValue;
    switch (L.src.cc) {
        case 1: return launch_blend<1, false>(L, lds, s);
        case 2: return launch_blend<2, false>(L, lds, s);
        case 3: return launch_blend<3, false>(L, lds, s);
        case 4: return launch_blend<4, false>(L, lds, s);
        default: return hipErrorInvalidValue;
    }
}

}  // namespace vacv
