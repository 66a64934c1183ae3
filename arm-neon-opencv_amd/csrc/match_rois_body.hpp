// match_rois_body.hpp -- the one kernel body of the batched template matchers:
// match_rois_kernel<CN, false> (k_match_rois.hip: the window copied from u8
// frames) and match_rois_kernel<3, true> (k_yuv_match_rois.hip: the window
// decoded from NV21 / NV12 frames).  The two differ in how `win` is staged and
// in nothing else: validation, the template, the template sums, the sliding
// horizontal sums, match_template_consts, the v_dot4 correlation,
// match_normalise and the peak merge are this text for both, so a fused ROI's
// bytes are the chain's by construction.  The LDS layout
// and the byte-identity argument stand at the top of k_match_rois.hip.  The
// including file sets `fp contract(off)` first.
#pragma once

#include "match_formula.hpp"
#include "vacv_device.hpp"

namespace vacv {
namespace {

constexpr int kOutPerLane = 4;     // adjacent result columns per item, sharing a sliding window
constexpr int kFixedBytes = 256;   // the head of the LDS block

struct Peak {
    double mn, mx;
    int imn, imx;  // row-major indices of the ROI's result, -1 = none
};

// mm_merge's rule (k_match.hip): the smaller index wins ties
__device__ __forceinline__ void peak_merge(Peak& a, const Peak& b) {
    if (b.imn >= 0 && (a.imn < 0 || b.mn < a.mn || (b.mn == a.mn && b.imn < a.imn))) {
        a.mn = b.mn;
        a.imn = b.imn;
    }
    if (b.imx >= 0 && (a.imx < 0 || b.mx > a.mx || (b.mx == a.mx && b.imx < a.imx))) {
        a.mx = b.mx;
        a.imx = b.imx;
    }
}

// the staged dwords of a window row (64-bit: the host asks for any int sizes)
__host__ __device__ inline int64_t window_row_dwords(int64_t tw, int64_t cn, int64_t rw) {
    const int64_t K4 = (tw * cn + 3) / 4, NW = (3 * cn) / 4 + 2, G = (rw + kOutPerLane - 1) / kOutPerLane;
    const int64_t data = ((rw + tw - 1) * cn + 3) / 4, reach = (G - 1) * cn + K4 + NW;
    return (data > reach ? data : reach) | 1;
}

// YUV's staging of win: frame f's W x H window at (left, top) of the decoded
// frame, decoded into the bytes the u8 staging copies.  Defined by
// k_yuv_match_rois.hip, the one file that instantiates YUV = true.
__device__ __forceinline__ void yuv_stage_window(const MatchRoisLaunch& M, int f, int left, int top, int W, int H,
                                                 int WS4, uint32_t* win, int tid);

template <int CN, bool YUV>
__global__ void __launch_bounds__(kBlock) match_rois_kernel(MatchRoisLaunch M) {
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    const int roi = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int tw = M.tw, th = M.th, rw = M.rw, rh = M.rh;
    const int W = rw + tw - 1, H = rh + th - 1;
    const int K = tw * CN, K4 = (K + 3) >> 2;
    constexpr int NW = (3 * CN) / 4 + 2;  // window dwords per k4 step
    const int G = (rw + kOutPerLane - 1) / kOutPerLane;
    const int WS4 = (int)window_row_dwords(tw, CN, rw);
    uint32_t* tsum = lds;                                       // [4 waves][8]: S_c, Q_c of the template
    Peak* wpeak = reinterpret_cast<Peak*>(lds + 32);            // [4 waves]
    uint32_t* tpl = lds + kFixedBytes / 4;                      // [th][K4]
    uint32_t* win = tpl + th * K4;                              // [H][WS4]
    uint32_t* hs = win + H * WS4;                               // [H][rw][CN]
    uint32_t* hq = hs + H * rw * CN;                            // [H][rw]
    unsigned char* res = M.res + (int64_t)roi * M.res_pitch;
    const bool peaks = M.vals != nullptr;

    // ---- the ROI's window and frame: device values, validated before any source read
    const int left = M.origin[2 * (int64_t)roi], top = M.origin[2 * (int64_t)roi + 1];
    const int f = M.src_index ? M.src_index[roi] : (M.n_src == 1 ? 0 : roi);
    // left + W <= w as left <= w - W: no sum of two device values
    const bool ok = f >= 0 && f < M.n_src && left >= 0 && top >= 0 && W <= M.src.w && left <= M.src.w - W &&
                    H <= M.src.h && top <= M.src.h - H;
    if (!ok) {  // uniform
        for (int i = tid; i < rw * rh; i += kBlock) {
            const int r = i / rw, x = i - r * rw;
            reinterpret_cast<float*>(res + (int64_t)r * M.res_row)[x] = 0.f;
        }
        if (peaks && tid == 0) {  // vacv_min_max_idx's "no element"
            M.vals[2 * (int64_t)roi] = 0.0;
            M.vals[2 * (int64_t)roi + 1] = 0.0;
            for (int k = 0; k < 4; ++k) M.idx[4 * (int64_t)roi + k] = -1;
        }
        return;
    }

    // ---- stage the template (zero padded rows) and the window
    const unsigned char* tb = M.tpl + (int64_t)roi * M.tpl_pitch;
    for (int i = tid; i < th * K4; i += kBlock) {
        const int yy = i / K4, k4 = i - yy * K4;
        const unsigned char* tr = tb + (int64_t)yy * M.tpl_row;
        uint32_t v = 0;
#pragma unroll
        for (int b = 0; b < 4; ++b)
            if (4 * k4 + b < K) v |= (uint32_t)tr[4 * k4 + b] << (8 * b);
        tpl[i] = v;
    }
    if constexpr (YUV) {
        static_assert(CN == 3, "decoded frames have three channels");
        yuv_stage_window(M, f, left, top, W, H, WS4, win, tid);
    } else {
        // every read is a byte of [left, left + W) x [top, top + H) of frame f
        const unsigned char* wb = M.src.base + (int64_t)f * M.src.img_pitch + (int64_t)top * M.src.row_pitch +
                                  (int64_t)left * CN;
        const int row_bytes = W * CN;
        for (int i = tid; i < H * WS4; i += kBlock) {
            const int y = i / WS4, d = i - y * WS4;
            const unsigned char* ir = wb + (int64_t)y * M.src.row_pitch;
            const int e = 4 * d;
            uint32_t v = 0;
            if (e + 4 <= row_bytes && ((reinterpret_cast<uintptr_t>(ir + e) & 3) == 0)) {
                v = *reinterpret_cast<const uint32_t*>(ir + e);
            } else {
#pragma unroll
                for (int b = 0; b < 4; ++b)
                    if (e + b < row_bytes) v |= (uint32_t)ir[e + b] << (8 * b);
            }
            win[i] = v;
        }
    }
    __syncthreads();

    const int method = M.method;
    const MatchMethod mm = match_method(method);
    const bool needS = mm.numType == 1, needQ = mm.isNormed || mm.numType == 2;  // what match_normalise asks for

    // ---- the template's per-channel sums (match_tstats_kernel's, as integers:
    // S_c <= 255 tw th and Q_c <= 255^2 tw th < 2^32 for tw th <= 66,000)
    if (method != VACV_TM_CCORR) {
        uint32_t s[4] = {0u, 0u, 0u, 0u}, q[4] = {0u, 0u, 0u, 0u};
        for (int i = tid; i < th * K4; i += kBlock) {
            const int k4 = i % K4;
            const uint32_t d = tpl[i];
            int c = (4 * k4) % CN;  // the padding bytes are zero: they add nothing to any channel
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const uint32_t v = (d >> (8 * b)) & 0xFFu;
#pragma unroll
                for (int cc = 0; cc < CN; ++cc) {
                    s[cc] += c == cc ? v : 0u;
                    q[cc] += c == cc ? v * v : 0u;
                }
                c = c + 1 == CN ? 0 : c + 1;
            }
        }
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            s[c] = wave_sum(s[c]);
            q[c] = wave_sum(q[c]);
        }
        if (lane == 0) {
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                tsum[wave * 8 + c] = s[c];
                tsum[wave * 8 + 4 + c] = q[c];
            }
        }
    }

    // ---- each window row's horizontal sums over tw pixels, sliding: an item is
    // a row and a run of L result columns.  hq sums the squares of tw CN <= W CN
    // bytes: < 2^32, since a row of 64 KiB does not fit the LDS budget
    if (needS || needQ) {
        const int per_row = max(1, kBlock / H);
        const int L = (rw + per_row - 1) / per_row, chunks = (rw + L - 1) / L;
        for (int item = tid; item < H * chunks; item += kBlock) {
            const int ch = item / H, y = item - ch * H;  // consecutive lanes: consecutive rows (WS4 is odd)
            const int x0 = ch * L, x1 = min(x0 + L, rw);
            const unsigned char* rb = reinterpret_cast<const unsigned char*>(win + y * WS4);
            uint32_t s[CN], q = 0u;
#pragma unroll
            for (int c = 0; c < CN; ++c) s[c] = 0u;
            for (int k = x0; k < x0 + tw; ++k) {
#pragma unroll
                for (int c = 0; c < CN; ++c) {
                    const uint32_t v = rb[k * CN + c];
                    s[c] += v;
                    q += v * v;
                }
            }
            for (int x = x0;;) {
#pragma unroll
                for (int c = 0; c < CN; ++c) hs[(y * rw + x) * CN + c] = s[c];
                hq[y * rw + x] = q;
                if (++x >= x1) break;
#pragma unroll
                for (int c = 0; c < CN; ++c) {
                    const uint32_t a = rb[(x - 1 + tw) * CN + c], b = rb[(x - 1) * CN + c];
                    s[c] += a - b;  // wraps when negative: the sum stays exact modulo 2^32
                    q += a * a - b * b;
                }
            }
        }
    }
    __syncthreads();

    // ---- the method's template constants (vacv_match_template skips them for CCORR, which takes none)
    double ts[7] = {0, 0, 0, 0, 0, 0, 0};
    if (method != VACV_TM_CCORR) {
        double s[4] = {0, 0, 0, 0}, q[4] = {0, 0, 0, 0};
#pragma unroll
        for (int c = 0; c < CN; ++c) {
            uint64_t S = 0, Q = 0;
            for (int w = 0; w < kBlock / 64; ++w) {
                S += tsum[w * 8 + c];
                Q += tsum[w * 8 + 4 + c];
            }
            s[c] = (double)S;
            q[c] = (double)Q;
        }
        match_template_consts(s, q, CN, tw * th, method, M.inv_area, ts);
    }
    const bool ones = ts[6] != 0.0;  // CCOEFF_NORMED of a flat template: no correlation needed

    // ---- the result: an item is kOutPerLane adjacent columns of one row, the
    // items flattened over (row, column group) so that a narrow result still
    // fills the waves
    Peak pk = {0, 0, -1, -1};
    for (int item = tid; item < rh * G; item += kBlock) {
        const int r = item / G, g = item - r * G;
        uint64_t acc[kOutPerLane] = {0, 0, 0, 0};
        if (!ones) {
            for (int yy = 0; yy < th; ++yy) {
                // match_corr_u8_kernel's inner loop: the item's outputs start at dword g * CN
                const uint32_t* rp = win + (r + yy) * WS4 + g * CN;
                const uint32_t* tp = tpl + yy * K4;
                uint32_t wd[NW];
#pragma unroll
                for (int j = 0; j < NW; ++j) wd[j] = rp[j];
                uint32_t a32[kOutPerLane] = {0, 0, 0, 0};
                for (int k4 = 0; k4 < K4; ++k4) {
                    const uint32_t t = tp[k4];
#pragma unroll
                    for (int o = 0; o < kOutPerLane; ++o) {
                        const int off = o * CN;  // byte offset of output o's window
                        const uint32_t v = (off & 3) ? __builtin_amdgcn_alignbyte(wd[(off >> 2) + 1], wd[off >> 2], off & 3)
                                                     : wd[off >> 2];
                        a32[o] = __builtin_amdgcn_udot4(v, t, a32[o], false);
                    }
#pragma unroll
                    for (int j = 0; j < NW - 1; ++j) wd[j] = wd[j + 1];
                    wd[NW - 1] = rp[k4 + NW];
                }
#pragma unroll
                for (int o = 0; o < kOutPerLane; ++o) acc[o] += a32[o];  // a row: <= 255^2 * K < 2^32
            }
        }
        float* orow = reinterpret_cast<float*>(res + (int64_t)r * M.res_row);
#pragma unroll
        for (int o = 0; o < kOutPerLane; ++o) {
            const int x = kOutPerLane * g + o;
            if (x >= rw) break;
            // the window's sums, down the th rows of horizontal sums
            uint32_t S[CN];
            uint64_t Q = 0;
#pragma unroll
            for (int c = 0; c < CN; ++c) S[c] = 0u;
            if (needS && !ones) {
                for (int yy = 0; yy < th; ++yy) {
                    const uint32_t* hp = hs + ((r + yy) * rw + x) * CN;
#pragma unroll
                    for (int c = 0; c < CN; ++c) S[c] += hp[c];
                }
            }
            if (needQ && !ones)
                for (int yy = 0; yy < th; ++yy) Q += hq[(r + yy) * rw + x];
            // Q is all channels' sum of squares as one integer (up to 4 * 2^32): handed over
            // as channel 0's, it is the value the formula gets by adding the channels' doubles
            // one by one, all below 2^53 (and + 0.0 changes nothing)
            const float outf = match_normalise(
                (float)(double)acc[o], CN, method, ts, M.inv_area,
                [&](int c) { return (double)S[c]; },  // c is a constant once the loops over CN unroll
                [&](int c) { return c == 0 ? (double)Q : 0.0; });
            orow[x] = outf;
            const double v = (double)outf;
            if (v == v) {  // a thread's indices ascend: strict comparisons keep the first
                const int i = r * rw + x;
                if (pk.imn < 0 || v < pk.mn) {
                    pk.mn = v;
                    pk.imn = i;
                }
                if (pk.imx < 0 || v > pk.mx) {
                    pk.mx = v;
                    pk.imx = i;
                }
            }
        }
    }
    if (!peaks) return;  // uniform

    // ---- the first row-major minimum and maximum over the workgroup
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        Peak b;
        b.mn = __shfl_xor(pk.mn, o, 64);
        b.mx = __shfl_xor(pk.mx, o, 64);
        b.imn = __shfl_xor(pk.imn, o, 64);
        b.imx = __shfl_xor(pk.imx, o, 64);
        peak_merge(pk, b);
    }
    if (lane == 0) wpeak[wave] = pk;
    __syncthreads();
    if (tid != 0) return;
    for (int w = 1; w < kBlock / 64; ++w) peak_merge(pk, wpeak[w]);
    M.vals[2 * (int64_t)roi] = pk.imn >= 0 ? pk.mn : 0.0;
    M.vals[2 * (int64_t)roi + 1] = pk.imx >= 0 ? pk.mx : 0.0;
    int32_t* oi = M.idx + 4 * (int64_t)roi;
    oi[0] = pk.imn >= 0 ? pk.imn / rw : -1;
    oi[1] = pk.imn >= 0 ? pk.imn % rw : -1;
    oi[2] = pk.imx >= 0 ? pk.imx / rw : -1;
    oi[3] = pk.imx >= 0 ? pk.imx % rw : -1;
}

}  // namespace
}  // namespace vacv
