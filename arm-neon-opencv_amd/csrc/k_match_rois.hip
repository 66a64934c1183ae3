// k_match_rois.hip -- many template matches in one launch: ROI i of the result
// is match_template(crop(frame src_index[i], W x H at origin[i]), template i)
// and vals[i] / idx[i] its minMaxIdx, the arrays read from DEVICE memory when
// the kernel runs.  u8 only.
//
// One workgroup per ROI, everything it needs in LDS:
//   fixed   256 bytes: the template sums' and the peaks' per-wave partials
//   tpl     [th][K4] dwords, K4 = ceil(tw cn / 4): the template, rows zero
//           padded to dwords as match_corr_u8_kernel (k_match.hip) stages it
//   win     [H][WS4] dwords: the W x H window, rows zero padded to WS4 (what the
//           sliding window of the last lane reads, rounded up to odd)
//   hs, hq  [H][rw][cn] and [H][rw] uint32: each window row's horizontal sums
//           over tw pixels, per channel (hs) and of the squares over all
//           channels (hq)
// match_rois_lds_bytes() is that sum; the host refuses what passes 64 KiB.
//
// Byte identity with vacv_match_template + vacv_min_max_idx on the crop rests
// on three facts:
//  1. every u8 sum is an integer below 2^53 -- the correlation, the window
//     sums S_c and Q, the template sums -- so their summation order is free;
//  2. the normalisation is match_normalise (match_formula.hpp), the one body
//     match_finish_kernel and match_finish_u8_kernel run: separately rounded
//     double operations in one order (contraction off);
//  3. the template constants are match_template_consts (match_formula.hpp),
//     the one body match_tstats_kernel runs, on the same (integer) sums.
// tests/test_match_rois_gpu.py compares both with the single calls bit for bit.
//
// The kernel's text is match_rois_body.hpp, which k_yuv_match_rois.hip compiles
// too, with its own staging of win.
#pragma clang fp contract(off)

#include "match_rois_body.hpp"

namespace vacv {

// A workgroup's dynamic LDS: the fixed head, the template, the window and the
// horizontal sums (the layout at the top of this file)
size_t match_rois_lds_bytes(int tw, int th, int cn, int rw, int rh) {
    const size_t K4 = ((size_t)tw * cn + 3) / 4, H = (size_t)rh + th - 1;
    const size_t WS4 = (size_t)window_row_dwords(tw, cn, rw);
    return kFixedBytes + 4 * ((size_t)th * K4 + H * WS4 + H * (size_t)rw * ((size_t)cn + 1));
}

hipError_t launch_match_rois(const MatchRoisLaunch& M, hipStream_t s) {
    const size_t lds = match_rois_lds_bytes(M.tw, M.th, M.src.cc, M.rw, M.rh);
    const dim3 grid(M.n_roi), block(kBlock);
    switch (M.src.cc) {
        case 1: hipLaunchKernelGGL((match_rois_kernel<1, false>), grid, block, lds, s, M); break;
        case 2: hipLaunchKernelGGL((match_rois_kernel<2, false>), grid, block, lds, s, M); break;
        case 3: hipLaunchKernelGGL((match_rois_kernel<3, false>), grid, block, lds, s, M); break;
        case 4: hipLaunchKernelGGL((match_rois_kernel<4, false>), grid, block, lds, s, M); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

}  // namespace vacv
