// k_yuv_match_rois.hip -- many template matches in search windows of NV21 /
// NV12 frames in one launch: ROI i of the result is what cvt_color of frame
// src_index[i] followed by match_template_rois of the W x H window at
// origin[i] produces, bit for bit, without the decoded frame ever existing
// (DESIGN.md 3.16).  The arrays are read from DEVICE memory when the kernel
// runs.
//
// The kernel is match_rois_kernel<3, true> (match_rois_body.hpp): one
// workgroup per ROI, the LDS layout of match_rois_kernel<3, false>
// (k_match_rois.hip: head, tpl, win, hs, hq) and the same text for everything
// but the staging of win, so the integer sums, match_normalise,
// match_template_consts and the peak rules are the chain's by construction.
// Only the staging is this file's: it decodes the window into the bytes the u8
// kernel would have copied from the decoded frame.
//
// A staging item is four consecutive window pixels of one row: 12 decoded
// bytes, three whole LDS dwords owned by one thread.  Y comes from
// (left + x, top + y), the chroma pair from row h + ((top + y) >> 1), byte
// (left + x) & ~1 (decode_tap, roi_tile.hpp: the tap color_kernel decodes);
// the four pixels touch two pairs when left is even, three when it is odd.
// Pixels past W and the padding dwords up to WS4 are stored as zero: the
// correlation's sliding window reads them.
//
// Device-supplied values cannot fault: the kernel judges the window and the
// index against the DECODED w x h by range checks only, before any source
// read, and an invalid one gives zeros.  A valid window reads bytes of its own
// Y rows and of chroma rows h + (top >> 1) .. h + ((top + H - 1) >> 1), columns
// left & ~1 .. (left + W - 1) | 1 <= w - 1 (w is even).  The only dword load is
// an aligned one of four Y bytes that are all the window's; the chroma is read
// bytewise, so nothing reaches past a dense frame's last pair.
#pragma clang fp contract(off)

#include "match_rois_body.hpp"
#include "roi_tile.hpp"

namespace vacv {
namespace {

constexpr int kItemPx = 4;  // pixels per staging item: 12 bytes, 3 dwords

// M.src.w x M.src.h is the decoded size; the caller has validated the window
__device__ __forceinline__ void yuv_stage_window(const MatchRoisLaunch& M, int f, int left, int top, int W, int H,
                                                 int WS4, uint32_t* win, int tid) {
    constexpr int CN = 3;
    const unsigned char* fb = M.src.base + (int64_t)f * M.src.img_pitch;
    const bool v_first = M.v_first != 0, rgb = M.rgb != 0;
    const int odd = left & 1;      // pixel p of an item uses pair (odd + p) >> 1 of it
    const int NI = (WS4 + 2) / 3;  // items per row: they cover all WS4 dwords
    // item (y, j) = pixels 4j .. 4j + 3 of row y = dwords 3j .. 3j + 2 of the row
    for (int i = tid; i < H * NI; i += kBlock) {
        const int y = i / NI, j = i - y * NI;
        const int x0 = kItemPx * j;
        const int nv = min(kItemPx, W - x0);     // the item's pixels inside the window (<= 0: padding only)
        const int sy = top + y, sx = left + x0;  // frame coordinates: sy <= h - 1, sx + nv <= w
        const unsigned char* yp = fb + (int64_t)sy * M.src.row_pitch + sx;
        const unsigned char* cp = fb + (int64_t)(M.src.h + (sy >> 1)) * M.src.row_pitch + (sx & ~1);
        uint32_t yy = 0;
        if (nv == kItemPx && (reinterpret_cast<uintptr_t>(yp) & 3) == 0) {
            yy = *reinterpret_cast<const uint32_t*>(yp);
        } else {
#pragma unroll
            for (int p = 0; p < kItemPx; ++p)
                if (p < nv) yy |= (uint32_t)yp[p] << (8 * p);
        }
        // pair k serves pixels max(0, 2k - odd) and up: read when the first of them is the window's
        uint32_t pair[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const int first = max(0, 2 * k - odd);
            pair[k] = first < nv ? (uint32_t)cp[2 * k] | ((uint32_t)cp[2 * k + 1] << 8) : 0u;
        }
        uint32_t out[3] = {0u, 0u, 0u};
#pragma unroll
        for (int p = 0; p < kItemPx; ++p) {
            if (p >= nv) continue;
            const int k = (odd + p) >> 1;
            const uint32_t pr = k == 0 ? pair[0] : (k == 1 ? pair[1] : pair[2]);
            int c[3];
            decode_tap((int)((yy >> (8 * p)) & 0xFFu), pr, v_first, rgb, c);
#pragma unroll
            for (int q = 0; q < CN; ++q) {
                const int b = CN * p + q;  // a constant once unrolled
                out[b >> 2] |= (uint32_t)c[q] << (8 * (b & 3));
            }
        }
        uint32_t* wr = win + y * WS4 + 3 * j;
#pragma unroll
        for (int k = 0; k < 3; ++k)
            if (3 * j + k < WS4) wr[k] = out[k];
    }
}

}  // namespace

hipError_t launch_yuv_match_rois(const MatchRoisLaunch& M, hipStream_t s) {
    if (M.src.cc != 3) return hipErrorInvalidValue;
    // the staging adds no LDS: the block is match_rois_kernel<3, false>'s
    const size_t lds = match_rois_lds_bytes(M.tw, M.th, 3, M.rw, M.rh);
    hipLaunchKernelGGL((match_rois_kernel<3, true>), dim3(M.n_roi), dim3(kBlock), lds, s, M);
    return hipGetLastError();
}

}  // namespace vacv
