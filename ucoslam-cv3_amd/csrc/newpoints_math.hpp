// Per-match arithmetic of the new-map-point stage (newpoints.hip), written once for the device and for the host: the Jacobi sweep
// count below is taken from a host run of exactly this text (tests/host_helpers/newpoints_math_host.cpp).
//
// Float conventions: every float expression of the reference stays a float expression in its written order, without contraction
// (the library is built with -ffp-contract=off; the pragma below says the same to a host compiler).  Products the reference takes
// through cv::Mat's operator* accumulate each element in double and round to float once, as OpenCV's float GEMM does; cv::norm is a
// double.  Those and the null vector of A are UNPINNED: no OpenCV exists to compare against.
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define NP_HD __host__ __device__ inline
#else
#define NP_HD inline
#endif
#if defined(__clang__)
#pragma clang fp contract(off)
#else
#pragma STDC FP_CONTRACT OFF
#endif

namespace npm {

// the smallest count at which every fixture match agrees with the oracle (4: tests/test_newpoints_host.py repeats the search), plus one
constexpr int kJacobiSweeps = 5;

enum Status : uint8_t {
    kAccepted = 0, kParallax = 1, kWZero = 2, kNotFinite = 3, kDepth1 = 4, kDepth2 = 5, kChi1 = 6, kChi2 = 7, kZeroDist = 8, kScaleRatio = 9
};

// what is uniform over the matches of one (new keyframe, neighbour) pair
struct PairConst {
    float P2[12];            // K2 [R | t], double-accumulated, rounded once (misc.cpp:975-978)
    float R[9], t[3];        // RT's rotation and translation: p3dC2 = R p3dC1 + t (misc.cpp:950-952, 1011)
    float fx2, fy2, cx2, cy2, invfx2, invfy2;
    float c2[3];             // the neighbour's camera centre
};
struct FrameConst {
    float fx1, fy1, cx1, cy1, invfx1, invfy1;
    float T[12];             // rows 0..2 of newKF.pose_f2g.inv()
    float c1[3];             // the new keyframe's camera centre
    float max_chi2, ratio_factor;
};

struct MatchOut { float cam[3]; float glob[3]; uint8_t status; };

// One rotation of the one-sided Jacobi (Hestenes): columns p and q of A (and of V) are rotated so that they become orthogonal.
#define NP_ROT(p, q)                                                                                         \
    {                                                                                                        \
        const double al = a0##p * a0##p + a1##p * a1##p + a2##p * a2##p + a3##p * a3##p;                     \
        const double be = a0##q * a0##q + a1##q * a1##q + a2##q * a2##q + a3##q * a3##q;                     \
        const double ga = a0##p * a0##q + a1##p * a1##q + a2##p * a2##q + a3##p * a3##q;                     \
        const double ze = (be - al) / (2.0 * ga);                                                            \
        double tt = (ze >= 0 ? 1.0 : -1.0) / (fabs(ze) + sqrt(1.0 + ze * ze));                               \
        tt = ga == 0.0 ? 0.0 : tt;                                                                           \
        const double cc = 1.0 / sqrt(1.0 + tt * tt), ss = cc * tt;                                           \
        double h;                                                                                            \
        h = a0##p; a0##p = cc * h - ss * a0##q; a0##q = ss * h + cc * a0##q;                                 \
        h = a1##p; a1##p = cc * h - ss * a1##q; a1##q = ss * h + cc * a1##q;                                 \
        h = a2##p; a2##p = cc * h - ss * a2##q; a2##q = ss * h + cc * a2##q;                                 \
        h = a3##p; a3##p = cc * h - ss * a3##q; a3##q = ss * h + cc * a3##q;                                 \
        h = v0##p; v0##p = cc * h - ss * v0##q; v0##q = ss * h + cc * v0##q;                                 \
        h = v1##p; v1##p = cc * h - ss * v1##q; v1##q = ss * h + cc * v1##q;                                 \
        h = v2##p; v2##p = cc * h - ss * v2##q; v2##q = ss * h + cc * v2##q;                                 \
        h = v3##p; v3##p = cc * h - ss * v3##q; v3##q = ss * h + cc * v3##q;                                 \
    }

// The right singular vector of the float 4x4 A (row-major) for its smallest singular value, in double.  Everything is a named
// scalar: no indexed private array, so nothing can end up in scratch memory.  `sweeps` is a compile-time constant at every call
// site of the library (kJacobiSweeps); the host probe passes other counts to find it.
NP_HD void null_vector(const float* A, int sweeps, double x[4]) {
    double a00 = A[0], a01 = A[1], a02 = A[2], a03 = A[3], a10 = A[4], a11 = A[5], a12 = A[6], a13 = A[7];
    double a20 = A[8], a21 = A[9], a22 = A[10], a23 = A[11], a30 = A[12], a31 = A[13], a32 = A[14], a33 = A[15];
    double v00 = 1, v01 = 0, v02 = 0, v03 = 0, v10 = 0, v11 = 1, v12 = 0, v13 = 0;
    double v20 = 0, v21 = 0, v22 = 1, v23 = 0, v30 = 0, v31 = 0, v32 = 0, v33 = 1;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int s = 0; s < sweeps; s++) {
        NP_ROT(0, 1) NP_ROT(2, 3) NP_ROT(0, 2) NP_ROT(1, 3) NP_ROT(0, 3) NP_ROT(1, 2)
    }
    const double n0 = a00 * a00 + a10 * a10 + a20 * a20 + a30 * a30, n1 = a01 * a01 + a11 * a11 + a21 * a21 + a31 * a31;
    const double n2 = a02 * a02 + a12 * a12 + a22 * a22 + a32 * a32, n3 = a03 * a03 + a13 * a13 + a23 * a23 + a33 * a33;
    // the column of the smallest norm; a NaN norm (non-finite A) turns every entry of V into NaN, whichever column is taken
    double nm = n0;
    x[0] = v00; x[1] = v10; x[2] = v20; x[3] = v30;
    if (n1 < nm) { nm = n1; x[0] = v01; x[1] = v11; x[2] = v21; x[3] = v31; }
    if (n2 < nm) { nm = n2; x[0] = v02; x[1] = v12; x[2] = v22; x[3] = v32; }
    if (n3 < nm) { nm = n3; x[0] = v03; x[1] = v13; x[2] = v23; x[3] = v33; }
}
#undef NP_ROT

NP_HD float norm3_as_float(float x, float y, float z) {   // float f = cv::norm(cv::Point3f): the square root of a double sum
    return (float)sqrt((double)x * x + (double)y * y + (double)z * z);
}

// misc.cpp:982-1035 (Triangulate's loop body), then mapmanager.cpp:10139-10314 (the distance-ratio / octave-ratio check).
// (x1, y1) is the new keyframe's keypoint (the reference's kp1 = Train.und_kpts[trainIdx]), (x2, y2) the neighbour's;
// inv_sig1 / inv_sig2 are 1.f / (f * f) of the scale factor at each keypoint's octave, sf1 / sf2 the scale factors themselves.
NP_HD void triangulate_match(const FrameConst& F, const PairConst& Q, float x1, float y1, float x2, float y2, float inv_sig1, float inv_sig2,
                             float sf1, float sf2, int sweeps, MatchOut& o) {
    const float nan = __builtin_nanf("");
    o.cam[0] = o.cam[1] = o.cam[2] = nan;
    o.glob[0] = o.glob[1] = o.glob[2] = nan;
    // :989-994 the parallax of the two rays; xn / cv::norm(xn) is a convertTo with the float scale (float)(1 / norm)
    const float xn1x = (x1 - F.cx1) * F.invfx1, xn1y = (y1 - F.cy1) * F.invfy1;
    const float xn2x = (x2 - Q.cx2) * Q.invfx2, xn2y = (y2 - Q.cy2) * Q.invfy2;
    const float i1 = (float)(1.0 / sqrt((double)xn1x * xn1x + (double)xn1y * xn1y + 1.0));
    const float i2 = (float)(1.0 / sqrt((double)xn2x * xn2x + (double)xn2y * xn2y + 1.0));
    const float r1x = xn1x * i1, r1y = xn1y * i1, r1z = 1.0f * i1;
    const float ux = xn2x * i2, uy = xn2y * i2, uz = 1.0f * i2;
    const float r2x = (float)((double)Q.R[0] * ux + (double)Q.R[3] * uy + (double)Q.R[6] * uz);   // R_t * u
    const float r2y = (float)((double)Q.R[1] * ux + (double)Q.R[4] * uy + (double)Q.R[7] * uz);
    const float r2z = (float)((double)Q.R[2] * ux + (double)Q.R[5] * uy + (double)Q.R[8] * uz);
    const double cosParallaxRays = (double)(r1x * r2x + r1y * r2y + r1z * r2z);
    if (cosParallaxRays < 0 || cosParallaxRays > 0.9998) { o.status = kParallax; return; }   // :996
    // :926-931 with P1 = K1 [I | 0]
    float A[16];
    A[0] = x1 * 0.0f - F.fx1; A[1] = x1 * 0.0f - 0.0f;  A[2] = x1 * 1.0f - F.cx1; A[3] = x1 * 0.0f - 0.0f;
    A[4] = y1 * 0.0f - 0.0f;  A[5] = y1 * 0.0f - F.fy1; A[6] = y1 * 1.0f - F.cy1; A[7] = y1 * 0.0f - 0.0f;
    A[8] = x2 * Q.P2[8] - Q.P2[0];  A[9] = x2 * Q.P2[9] - Q.P2[1];  A[10] = x2 * Q.P2[10] - Q.P2[2]; A[11] = x2 * Q.P2[11] - Q.P2[3];
    A[12] = y2 * Q.P2[8] - Q.P2[4]; A[13] = y2 * Q.P2[9] - Q.P2[5]; A[14] = y2 * Q.P2[10] - Q.P2[6]; A[15] = y2 * Q.P2[11] - Q.P2[7];
    double nv[4];
    null_vector(A, sweeps, nv);
    if (nv[3] == 0) { o.status = kWZero; return; }   // :936
    const float X = (float)(nv[0] / nv[3]), Y = (float)(nv[1] / nv[3]), Z = (float)(nv[2] / nv[3]);   // :938
    if (!std::isfinite(X) || !std::isfinite(Y) || !std::isfinite(Z)) { o.status = kNotFinite; return; }   // :1003
    if (Z <= 0) { o.status = kDepth1; return; }   // :1007
    const float X2 = (float)((double)Q.R[0] * X + (double)Q.R[1] * Y + (double)Q.R[2] * Z + (double)Q.t[0]);   // :1011
    const float Y2 = (float)((double)Q.R[3] * X + (double)Q.R[4] * Y + (double)Q.R[5] * Z + (double)Q.t[1]);
    const float Z2 = (float)((double)Q.R[6] * X + (double)Q.R[7] * Y + (double)Q.R[8] * Z + (double)Q.t[2]);
    if (Z2 <= 0) { o.status = kDepth2; return; }   // :1013
    const float invZ1 = 1.f / Z;   // :1017-1021
    const float qx = F.fx1 * X * invZ1 + F.cx1, qy = F.fy1 * Y * invZ1 + F.cy1;
    float chi2 = inv_sig1 * ((qx - x1) * (qx - x1) + (qy - y1) * (qy - y1));
    if (chi2 > F.max_chi2) { o.status = kChi1; return; }
    const float invZ2 = 1.f / Z2;   // :1025-1030
    const float tx = Q.fx2 * X2 * invZ2 + Q.cx2, ty = Q.fy2 * Y2 * invZ2 + Q.cy2;
    chi2 = inv_sig2 * ((tx - x2) * (tx - x2) + (ty - y2) * (ty - y2));
    if (chi2 > F.max_chi2) { o.status = kChi2; return; }
    o.cam[0] = X; o.cam[1] = Y; o.cam[2] = Z;   // :1033
    // mapmanager.cpp:10160-10170 pg = pose_f2g.inv() * p3d (se3transform.h:109-112)
    const float gx = F.T[0] * X + F.T[1] * Y + F.T[2] * Z + F.T[3];
    const float gy = F.T[4] * X + F.T[5] * Y + F.T[6] * Z + F.T[7];
    const float gz = F.T[8] * X + F.T[9] * Y + F.T[10] * Z + F.T[11];
    const float dist1 = norm3_as_float(gx - F.c1[0], gy - F.c1[1], gz - F.c1[2]);   // :10173-10187
    const float dist2 = norm3_as_float(gx - Q.c2[0], gy - Q.c2[1], gz - Q.c2[2]);   // :10189-10213
    if (dist1 == 0 || dist2 == 0) { o.status = kZeroDist; return; }   // :10214-10227
    const float ratioDist = dist1 / dist2;   // :10231-10238
    const float ratioOctave = sf1 / sf2;     // :10282-10299
    if (ratioDist * F.ratio_factor < ratioOctave || ratioDist > ratioOctave * F.ratio_factor) { o.status = kScaleRatio; return; }   // :10303-10314
    o.glob[0] = gx; o.glob[1] = gy; o.glob[2] = gz;
    o.status = kAccepted;
}

// P2 = K2 * [R | t] (misc.cpp:975-978) from the row-major 4x4 RT
inline void make_pair_const(const float* RT, const float* intr4, const float* cam_center, PairConst& Q) {
    const double K[9] = {intr4[0], 0, intr4[2], 0, intr4[1], intr4[3], 0, 0, 1};
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 4; c++)
            Q.P2[4 * r + c] = (float)(K[3 * r] * (double)RT[c] + K[3 * r + 1] * (double)RT[4 + c] + K[3 * r + 2] * (double)RT[8 + c]);
    for (int r = 0; r < 3; r++) {
        for (int c = 0; c < 3; c++) Q.R[3 * r + c] = RT[4 * r + c];
        Q.t[r] = RT[4 * r + 3];
        Q.c2[r] = cam_center[r];
    }
    Q.fx2 = intr4[0]; Q.fy2 = intr4[1]; Q.cx2 = intr4[2]; Q.cy2 = intr4[3];
    Q.invfx2 = 1.f / Q.fx2; Q.invfy2 = 1.f / Q.fy2;
}

}  // namespace npm
