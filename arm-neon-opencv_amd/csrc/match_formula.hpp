// match_formula.hpp -- cv::matchTemplate's double arithmetic (OpenCV 2.4
// templmatch.cpp), shared by the single-call kernels (k_match.hip) and the
// batched ROI kernel (k_match_rois.hip): one body each, so the two paths give
// the same bytes by construction.  Separately rounded IEEE operations in
// OpenCV's order: every file that includes this carries fp contract(off).
#pragma once
#pragma clang fp contract(off)

#include "vacv_internal.hpp"

namespace vacv {

// The method's template constants from the template's per-channel sums s[c]
// and sums of squares q[c] over its n = tw th pixels (channels >= cn: 0):
// o[0..3] the means the numerator subtracts, o[4] templNorm, o[5] templSum2,
// o[6] != 0 for CCOEFF_NORMED of a flat template (the result is all ones).
__device__ __forceinline__ void match_template_consts(const double s[4], const double q[4], int cn, int n, int method,
                                                      double invArea, double o[7]) {
    double tm[4] = {0, 0, 0, 0}, td[4] = {0, 0, 0, 0};
    for (int c = 0; c < cn; ++c) {  // meanStdDev: population
        tm[c] = s[c] / n;
        const double var = q[c] / n - tm[c] * tm[c];
        td[c] = sqrt(var > 0 ? var : 0);
    }
    double templNorm = 0, templSum2 = 0, ones = 0;
    double tmean[4] = {tm[0], tm[1], tm[2], tm[3]};
    if (method != VACV_TM_CCOEFF) {
        templNorm = td[0] * td[0] + td[1] * td[1] + td[2] * td[2] + td[3] * td[3];
        if (templNorm < 2.220446049250313e-16 && method == VACV_TM_CCOEFF_NORMED) ones = 1;
        templSum2 = templNorm + tm[0] * tm[0] + tm[1] * tm[1] + tm[2] * tm[2] + tm[3] * tm[3];
        const bool ccoeff = method == VACV_TM_CCOEFF || method == VACV_TM_CCOEFF_NORMED;
        if (!ccoeff) {
            tmean[0] = tmean[1] = tmean[2] = tmean[3] = 0;
            templNorm = templSum2;
        }
        templSum2 /= invArea;
        templNorm = sqrt(templNorm);
        templNorm /= sqrt(invArea);
    }
    for (int c = 0; c < 4; ++c) o[c] = tmean[c];
    o[4] = templNorm;
    o[5] = templSum2;
    o[6] = ones;
}

struct MatchMethod {
    int numType;    // 0 CCORR, 1 CCOEFF, 2 SQDIFF
    bool isNormed;
};
__device__ __forceinline__ MatchMethod match_method(int method) {
    MatchMethod m;
    m.numType = (method == VACV_TM_CCORR || method == VACV_TM_CCORR_NORMED)     ? 0
                : (method == VACV_TM_CCOEFF || method == VACV_TM_CCOEFF_NORMED) ? 1
                                                                                : 2;
    m.isNormed = method == VACV_TM_CCORR_NORMED || method == VACV_TM_SQDIFF_NORMED || method == VACV_TM_CCOEFF_NORMED;
    return m;
}

// One result element: crossCorr's float `corr`, the constants ts[7] of
// match_template_consts and the window's statistics -- S(c) its sum of channel
// c, Q(c) its sum of squares of channel c, each called only where the method
// takes it, for c = 0 .. cn - 1 in order.
template <class SumFn, class SqFn>
__device__ __forceinline__ float match_normalise(float corr, int cn, int method, const double* ts, double invArea,
                                                 SumFn S, SqFn Q) {
    if (ts[6] != 0.0) return 1.f;  // CCOEFF_NORMED of a flat template
    const MatchMethod mm = match_method(method);
    double num = (double)corr, t;
    double wndMean2 = 0, wndSum2 = 0;
    if (mm.numType == 1) {
        for (int c = 0; c < cn; ++c) {
            t = S(c);
            wndMean2 += t * t;
            num -= t * ts[c];
        }
        wndMean2 *= invArea;
    }
    if (mm.isNormed || mm.numType == 2) {
        for (int c = 0; c < cn; ++c) {
            t = Q(c);
            wndSum2 += t;
        }
        if (mm.numType == 2) {
            num = wndSum2 - 2 * num + ts[5];
            num = num > 0. ? num : 0.;
        }
    }
    if (mm.isNormed) {
        t = sqrt(wndSum2 - wndMean2 > 0. ? wndSum2 - wndMean2 : 0.) * ts[4];
        if (fabs(num) < t) num /= t;
        else if (fabs(num) < t * 1.125) num = num > 0 ? 1 : -1;
        else num = method != VACV_TM_SQDIFF_NORMED ? 0 : 1;
    }
    return (float)num;
}

}  // namespace vacv
