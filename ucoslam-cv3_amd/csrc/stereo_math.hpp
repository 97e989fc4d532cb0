// Per-keypoint arithmetic of the stereo / RGB-D depth stage (stereo.hip), written once for the device and for the host
// (uh_stereo_depth_host; tests/host_helpers/stereo_math_host.cpp): FrameExtractor::processStereo and process_rgbd
// (src/utils/frameextractor.cpp from :1419) for kptImageScaleFactor == 1.
//
// Everything here is integer work, one float product (bl * fx, formed by the caller) and IEEE double + - * / in the written order;
// the library is built with -ffp-contract=off and the pragma below says the same to a host compiler.  The roundings are spelled out
// with truncf and an exact remainder instead of std::round / cvRound, so that no libm or rounding-mode difference can separate the
// two sides.
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define ST_HD __host__ __device__ inline
#else
#define ST_HD inline
#endif
#if defined(__clang__)
#pragma clang fp contract(off)
#else
#pragma STDC FP_CONTRACT OFF
#endif

namespace stm {

constexpr int kHalfWin = 3;      // wsize / 2 with wsize = 7: cv::Range(c - 3, c + 3) is SIX pixels
constexpr int kMaxOff = 7;       // offsets -7 .. 7
constexpr int kNumOff = 2 * kMaxOff + 1;
constexpr int kFar = 1 << 30;    // |v| >= 2^30 and NaN: a coordinate no image holds (int(std::round(v)) would be undefined there)

// int(std::round(v)): halves away from zero.  v - truncf(v) is exact.
ST_HD int round_away(float v) {
    if (!(v > -1073741824.f)) return -kFar;   // (NaN too)
    if (!(v < 1073741824.f)) return kFar;
    float t = truncf(v);
    const float f = v - t;
    if (f >= 0.5f) t += 1.f;
    else if (f <= -0.5f) t -= 1.f;
    return (int)t;
}
// cvRound(v) (cv::Point(Point2f) = saturate_cast<int>): halves to even.
ST_HD int round_even(float v) {
    if (!(v > -1073741824.f)) return -kFar;
    if (!(v < 1073741824.f)) return kFar;
    float t = truncf(v);
    const float f = v - t;
    const bool odd = ((int)t & 1) != 0;
    if (f > 0.5f || (f == 0.5f && odd)) t += 1.f;
    else if (f < -0.5f || (f == -0.5f && odd)) t -= 1.f;
    return (int)t;
}

// The row bucket of a right keypoint: rows max(0, r) .. min(rows - 1, r) with r = int(std::round(double(pt.y))) and a search
// half-height of 0 — that is row r, and NO row when r is outside the image (the loop is empty).  -1 = none.
ST_HD int right_row(float y, int rows) {
    const int r = round_away(y);   // (float -> double is exact: the same integer)
    return (r < 0 || r >= rows) ? -1 : r;
}
// The row a left keypoint looks up.  The reference indexes its bucket vector unchecked; here a row outside the image has no
// candidates (-1).
ST_HD int left_row(float und_y, int rows) {
    const int r = round_away(und_y);
    return (r < 0 || r >= rows) ? -1 : r;
}

// candidate filter: right.pt.x > left.und.x (float compare) or |octave difference| > 1 skips
ST_HD bool candidate_ok(float rx, int roct, float lux, int loct) {
    if (rx > lux) return false;
    const long long d = (long long)roct - (long long)loct;
    return d >= -1 && d <= 1;
}

ST_HD int popc32(uint32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __popc(v);
#else
    return __builtin_popcount(v);
#endif
}
// MapPoint::getDescDistance on two 32-byte ORB descriptors, as eight 32-bit words
ST_HD int hamming256(const uint32_t* a, const uint32_t* b) {
    int d = 0;
    for (int k = 0; k < 8; k++) d += popc32(a[k] ^ b[k]);
    return d;
}
// the distance is compared as a float with maxDescDistance
ST_HD bool distance_ok(int d, float max_desc_dist) { return (float)d < max_desc_dist; }
// best candidate = smallest (distance, j): the reference walks a row in ascending j and replaces on strict <
ST_HD uint64_t match_key(int d, int j) { return ((uint64_t)(uint32_t)d << 32) | (uint32_t)j; }
constexpr uint64_t kNoKey = ~(uint64_t)0;

// a window centre the 6 x 6 window [c - 3, c + 3) fits around: 3 <= c and c + 3 < size
ST_HD bool centre_ok(int c, int size) { return c >= kHalfWin && c + kHalfWin < size; }

// Offsets evaluated around the right centre rx.  The reference runs max(-7, -rx) .. min(7, cols - 1 - rx) and throws from
// cv::Mat::operator() where the window leaves the image; here the range stops where the window still fits, which is the
// reference's range wherever it does not throw.
ST_HD void offset_range(int rx, int cols, int& lo, int& hi) {
    lo = -kMaxOff > kHalfWin - rx ? -kMaxOff : kHalfWin - rx;
    hi = kMaxOff < cols - kHalfWin - rx ? kMaxOff : cols - kHalfWin - rx;
}

// cv::sum(cv::absdiff(L(rows ly-3..ly+3, cols lx-3..lx+3), R(rows ry-3..ry+3, cols cx-3..cx+3)))[0], 8-bit images
ST_HD int sad6(const uint8_t* L, size_t l_stride, int lx, int ly, const uint8_t* R, size_t r_stride, int cx, int ry) {
    int s = 0;
    for (int dy = -kHalfWin; dy < kHalfWin; dy++) {
        const uint8_t* pl = L + (size_t)(ly + dy) * l_stride + (lx - kHalfWin);
        const uint8_t* pr = R + (size_t)(ry + dy) * r_stride + (cx - kHalfWin);
        for (int dx = 0; dx < 2 * kHalfWin; dx++) {
            const int a = pl[dx], b = pr[dx];
            s += a > b ? a - b : b - a;
        }
    }
    return s;
}

// one step of the first-minimum walk over cost[lo + 7 .. hi + 7] in ascending index (strict <)
ST_HD void take_min(int cost, int idx, int& best_cost, int& best_idx) {
    if (best_idx < 0 || cost < best_cost) { best_cost = cost; best_idx = idx; }
}

// The depth of a match whose SAD minimum sits at index b (= offset + 7) strictly inside the evaluated range, c0 c1 c2 the costs at
// b - 1, b, b + 1; blfx = bl * fx, a FLOAT product.  c0 > c1 (first minimum) and c2 >= c1, so the denominator is > 0.
// Negative and infinite depths are returned as computed.
ST_HD float depth_from_costs(int c0i, int c1i, int c2i, int b, float right_x, float left_und_x, float blfx) {
    const double c0 = c0i, c1 = c1i, c2 = c2i;
    const double delta = 0.5 * (c0 - c2) / (c0 + c2 - 2 * c1) + b - kMaxOff;
    const double xr = (double)right_x + delta;
    return (float)((double)blfx / ((double)left_und_x - xr));
}

// The whole refinement of one match, serially (the host form; the device spreads the offsets over lanes and ends in the same
// take_min / depth_from_costs).  0 = no depth.
ST_HD float refine_serial(const uint8_t* L, size_t l_stride, const uint8_t* R, size_t r_stride, int cols, int rows, float lux, float luy,
                          float rpx, float rpy, float blfx) {
    const int lx = round_away(lux), ly = round_away(luy);
    if (!centre_ok(lx, cols) || !centre_ok(ly, rows)) return 0.f;
    const int rx = round_away(rpx), ry = round_away(rpy);
    if (!centre_ok(rx, cols) || !centre_ok(ry, rows)) return 0.f;
    int lo, hi;
    offset_range(rx, cols, lo, hi);
    int cost[kNumOff] = {0};
    int best = 0, b = -1;
    for (int o = lo; o <= hi; o++) {
        const int c = sad6(L, l_stride, lx, ly, R, r_stride, rx + o, ry);
        cost[o + kMaxOff] = c;
        take_min(c, o + kMaxOff, best, b);
    }
    if (!(b > lo + kMaxOff && b < hi + kMaxOff)) return 0.f;
    return depth_from_costs(cost[b - 1], cost[b], cost[b + 1], b, rpx, lux, blfx);
}

// process_rgbd: depth = float(D(kpt)) * rgb_depthscale in float where that pixel is non-zero, else 0; the keypoint is the DISTORTED
// one, Point2f -> Point by cvRound.  The reference reads cv::Mat::at unchecked; a pixel outside the depth image gives 0 here.
ST_HD float rgbd_depth(const uint16_t* D, size_t stride_px, int cols, int rows, float kx, float ky, float scale) {
    const int x = round_even(kx), y = round_even(ky);
    if (x < 0 || x >= cols || y < 0 || y >= rows) return 0.f;
    const uint16_t v = D[(size_t)y * stride_px + x];
    return v != 0 ? (float)(int)v * scale : 0.f;
}

}  // namespace stm
