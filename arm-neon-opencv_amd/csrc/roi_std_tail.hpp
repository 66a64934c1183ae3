// roi_std_tail.hpp -- what the two standardize-from-YUV kernels
// (k_yuv_crop_resize_rois_std.hip, k_yuv_warp_rois_std.hip) do once a ROI's
// three u8 channels lie in LDS: reduce the threads' partial sums, the
// statistics, the table of normalized values, the stores.  It is
// k_crop_resize_rois_std.hip's and k_warp_rois_std.hip's tail at 3 channels,
// expression for expression; those two keep their own copies, as measured.
#pragma once
#pragma clang fp contract(off)

#include "vacv_device.hpp"

namespace vacv {
namespace {

// one workgroup of 16 waves per ROI: the BGR standardize kernels' measured
// choice for this work shape, taken over unmeasured
constexpr int kYuvStdBlock = 1024;
constexpr int kYuvStdHeadBytes = 256;
constexpr int kYuvStdC = 3;  // a decoded frame's channels
static_assert(kYuvStdBlock % 64 == 0 && kYuvStdBlock <= 1024, "whole waves, one workgroup");

// The part of the LDS head the tail owns.  sum: per channel Sum v [0..3] and
// Sum v^2 [4..7].  No overflow: a ROI that fits the LDS budget has fewer than
// 65,536 pixels, so Sum v^2 <= 65,535 * 65,025 < 2^32 even in a thread's
// uint32 partial; the workgroup's totals are 64-bit all the same
struct StdStats {
    unsigned long long sum[8];
    float mean[4], stdv[4];
};

// A workgroup's LDS but the sampler's tables: the head, the u8 ROI, the
// [3][256] floats
__host__ __device__ inline size_t yuv_std_px_bytes(int w, int h) {
    return ((size_t)w * h * kYuvStdC + 15) / 16 * 16;
}

// n floats to d (4-byte aligned) by threads t of nt: element j is the
// normalized value of LDS byte px[b0 + j], of channel k (PLANAR) or j % 3 (a
// run starts at a pixel).  16-byte stores from the destination's first
// 16-byte boundary on, dwords before it and after the last whole one.  px is
// 16-byte aligned and followed by the table, so the dword past a run's last
// byte is LDS of this workgroup.
template <bool PLANAR>
__device__ __forceinline__ void store_run(float* d, const unsigned char* px, uint32_t b0, int n, int k,
                                          const float* lut, int t, int nt) {
    constexpr int CC = kYuvStdC;
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

// Every thread of the workgroup calls this after its last write to px, with
// its partial sums s1 (Sum v) and s2 (Sum v^2) and st->sum zeroed behind a
// barrier.  lut may overlay what the sampler tabled: it is first written after
// the barrier that follows the reduction.
template <bool PLANAR>
__device__ __forceinline__ void standardize_tail(StdStats* st, const unsigned char* px, float* lut,
                                                 const uint32_t (&s1)[kYuvStdC], const uint32_t (&s2)[kYuvStdC],
                                                 const PlaneGeom& dst, int roi, float* mean_out, float* stddev_out) {
    constexpr int CC = kYuvStdC;
    const int w = dst.w, h = dst.h, npx = w * h;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    // per wave, then per workgroup: integers, so any order is the same sum
#pragma unroll
    for (int k = 0; k < CC; ++k) {
        const unsigned long long t1 = wave_sum((unsigned long long)s1[k]);
        const unsigned long long t2 = wave_sum((unsigned long long)s2[k]);
        if (lane == 0) {
            atomicAdd(&st->sum[k], t1);
            atomicAdd(&st->sum[4 + k], t2);
        }
    }
    __syncthreads();  // the sampler's tables are dead from here

    // ---- the statistics: stats_kernel's expressions (k_pixel.hip) on the same integers
    if (tid < CC) {
        const double count = (double)w * h;
        const double m = (double)st->sum[tid] / count;
        double var = (double)st->sum[4 + tid] / count - m * m;
        if (var < 0) var = 0;
        const float mf = (float)m, sf = (float)sqrt(var);
        st->mean[tid] = mf;
        st->stdv[tid] = sf;
        if (mean_out) mean_out[(int64_t)roi * CC + tid] = mf;
        if (stddev_out) stddev_out[(int64_t)roi * CC + tid] = sf;
    }
    __syncthreads();

    // ---- every u8 value's normalized float, the exact divide once per (channel, value)
#pragma unroll 1
    for (int e = tid; e < 256 * CC; e += kYuvStdBlock) {
        const int k = e >> 8;
        lut[e] = normalize_value((float)(e & 255), st->mean[k], st->stdv[k]);
    }
    __syncthreads();

    // ---- LDS -> HBM: one run per plane of dense rows, else one per row
    constexpr int kPlanes = PLANAR ? CC : 1;
    const int row_el = w * (PLANAR ? 1 : CC);  // floats per destination row
    unsigned char* dbase = const_cast<unsigned char*>(dst.base) + (int64_t)roi * dst.img_pitch;
    if (dst.row_pitch == (int64_t)row_el * 4) {  // uniform
#pragma unroll
        for (int k = 0; k < kPlanes; ++k)
            store_run<PLANAR>(reinterpret_cast<float*>(dbase + (int64_t)k * dst.plane_pitch), px, (uint32_t)(k * npx),
                              h * row_el, k, lut, tid, kYuvStdBlock);
        return;
    }
#pragma unroll 1
    for (int r = wave; r < kPlanes * h; r += kYuvStdBlock / 64) {  // wave r % 16 stores run r = (plane, row)
        const int k = PLANAR ? r / h : 0;
        const int y = r - k * h;
        store_run<PLANAR>(reinterpret_cast<float*>(dbase + (int64_t)k * dst.plane_pitch + (int64_t)y * dst.row_pitch),
                          px, (uint32_t)(k * npx + y * row_el), row_el, k, lut, lane, 64);
    }
}

}  // namespace
}  // namespace vacv
