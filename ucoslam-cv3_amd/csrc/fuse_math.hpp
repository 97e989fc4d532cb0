// Per-point arithmetic of the mapper's fuse search (fuse.hip, fuse_host.hpp), written once for the device and for the host: the body of
// MapManager's search-and-fuse loop (src/utils/mapmanager.cpp, ORB-SLAM's SearchInNeighbors) from the skip test down to the disc the
// kd-tree is asked for — (p2d, level, radius) — plus the status code of the point.
//
// Order of the tests, as the reference writes them (NOT the projection matcher's order): caller's skip, Frame::project(p, true, true)
// (frame.h:140-159: z < 0, then the image test with >= min and < max), the distance from the GLOBAL camera centre against
// [0.8f * min, 1.2f * max] (strict comparisons: both ends are kept), getViewCos(cc) < 0.5 (mappoint.h:99), predictScale of ANOTHER frame
// (frame.h:129-136: the new keyframe's level count and scaleFactors[1] in both halves), radius = th * scaleFactors[level] of the
// SEARCHED frame, widened by 1.4f below viewCos 0.98 in the first half.
//
// Float expressions keep the written order and are not contracted (the library is built with -ffp-contract=off; the pragma below says
// the same to a host compiler); cv::norm and the 1./norm factor of getViewCos are double, as in OpenCV.  logf is glibc's, restated in
// glibc_sincosf.hpp for both sides.
#pragma once
#include <cmath>
#include <cstdint>

#include "glibc_sincosf.hpp"

#if defined(__HIPCC__)
#define FU_HD __host__ __device__ inline
#else
#define FU_HD inline
#endif
#if defined(__clang__)
#pragma clang fp contract(off)
#else
#pragma STDC FP_CONTRACT OFF
#endif

namespace uh_fusem {

enum Status : uint8_t {
    kFound = 0,       // searched, keypoint found
    kSkipped = 1,     // skipped by the caller's mask
    kNoProject = 2,   // Frame::project gave NaN
    kDistance = 3,    // distance outside the invariance range
    kViewCos = 4,     // viewCos < 0.5
    kNoKeypoint = 5,  // searched, no keypoint under the threshold
};

// what the search of one frame needs besides its tree: pose rows, camera centre, camera, image bounds (ints of cv::Point as floats: the
// comparison converts them), and the predictor of the new keyframe
struct View {
    float T[12];
    float cc[3];
    float fx, fy, cx, cy;
    float min_x, min_y, max_x, max_y;
    float log_scale;        // logf(predict_scale_factors[1])
    int predict_levels;
    float th, widen;
};

struct Disc { float px, py; int level; float radius; };

// Frame::getCameraCenter (frame.h:189-197)
inline void camera_center(const float* T /* row-major 4x4 or 3x4 */, float cc[3]) {
    cc[0] = -(T[3] * T[0] + T[7] * T[4] + T[11] * T[8]);
    cc[1] = -(T[3] * T[1] + T[7] * T[5] + T[11] * T[9]);
    cc[2] = -(T[3] * T[2] + T[7] * T[6] + T[11] * T[10]);
}

// Frame::predictScale (frame.h:129-136) with float log (the std::log overloads the reference resolves to)
FU_HD int predict_scale(float dist, float maxd, float log_scale, int levels) {
    const int ns = (int)ceilf(uh_sincosf::logf_glibc(maxd / dist) / log_scale);
    if (ns < 0) return 0;
    if (ns >= levels) return levels - 1;
    return ns;
}

// Status of one point before the tree is asked: kFound stands for "search the disc d", anything else ends the point.
// scale: the SEARCHED frame's scaleFactors (at least v.predict_levels entries — the caller checks).
FU_HD uint8_t point_disc(const View& v, const float* scale, bool skip, float P0, float P1, float P2, float n0, float n1, float n2, float mind, float maxd,
                         Disc& d) {
    if (skip) return kSkipped;
    const float* T = v.T;
    float z = P0 * T[8] + P1 * T[9] + P2 * T[10] + T[11];
    if (z < 0) return kNoProject;
    const float x = P0 * T[0] + P1 * T[1] + P2 * T[2] + T[3];
    const float y = P0 * T[4] + P1 * T[5] + P2 * T[6] + T[7];
    z = (float)(1. / z);
    const float px = ((v.fx * x) * z) + v.cx, py = ((v.fy * y) * z) + v.cy;
    if (!(px >= v.min_x && py >= v.min_y && px < v.max_x && py < v.max_y)) return kNoProject;
    const float v0 = v.cc[0] - P0, v1 = v.cc[1] - P1, v2 = v.cc[2] - P2;
    const double nrm = sqrt((double)v0 * v0 + (double)v1 * v1 + (double)v2 * v2);   // cv::norm(Point3f)
    const float dist = (float)nrm;
    if (dist < 0.8f * mind || dist > 1.2f * maxd) return kDistance;
    const double s = 1. / nrm;                                                       // getViewCos: v *= 1. / cv::norm(v)
    const float u0 = (float)(v0 * s), u1 = (float)(v1 * s), u2 = (float)(v2 * s);
    const float view_cos = u0 * n0 + u1 * n1 + u2 * n2;
    if (view_cos < 0.5) return kViewCos;
    d.level = predict_scale(dist, maxd, v.log_scale, v.predict_levels);
    float radius = v.th * scale[d.level];
    if (view_cos < 0.98) radius *= v.widen;
    d.px = px; d.py = py; d.radius = radius;
    return kFound;
}

// the strict threshold: pair<float,int> best(maxDescDistance + 1e-3, -1)
inline float desc_threshold(float max_desc_dist) { return (float)(max_desc_dist + 1e-3); }

}  // namespace uh_fusem
