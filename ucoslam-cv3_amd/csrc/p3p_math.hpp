// Arithmetic of the relocalisation RANSAC (pnp_ransac.hip), written once for the device and for the host:
// PnPSolver::solvePnPRansac, src/optimization/pnpsolver.cpp:36-114 — a three-point pose from four matches (cv::solvePnP with
// SOLVEPNP_P3P), Se3Transform::set (src/basictypes/se3transform.h:143-176) and the inlier test of :75-100.
//
// Double part (not pinned to OpenCV, none exists to compare with; pinned to a 60-digit solve, tests/golden/p3p_golden.npz; the contract is mathematical — every real solution with positive point
// distances, the one with the smallest reprojection error of the fourth point, the lowest index on ties):
//   Grunert's formulation.  Unit bearings j1 j2 j3, point distances s1 s2 s3, s2 = u s1, s3 = v s1, a = |P2 P3|, b = |P1 P3|,
//   c = |P1 P2|, cos(alpha) = j2.j3, cos(beta) = j1.j3, cos(gamma) = j1.j2.  The cosine rule on the three sides gives
//       u = N(v) / D(v),  N = (k - 1) v^2 - 2 k cos(beta) v + (k + 1),  D = 2 (cos(gamma) - v cos(alpha)),  k = (a^2 - c^2) / b^2
//   and, put back into the side c,  N^2 + D^2 (1 - q (1 - 2 cos(beta) v + v^2)) - 2 cos(gamma) N D = 0,  q = c^2 / b^2: a quartic in v,
//   whose coefficients are formed here by multiplying the polynomials out.  Its real roots come from Ferrari's resolvent (largest
//   real root of the cubic, trigonometric or Cardano form) and two Newton steps on the quartic itself; where the leading coefficient
//   is small against the others the same is done in w = 1 / v (reversed_form below).  Solutions are numbered in ascending v = s3 / s1.  The pose of a root is the rigid motion between the orthonormal frames of the triangle in the world and in
//   the camera (exact for an exact root).
// Float part: every float expression of the reference stays a float expression in its written order, without contraction (the library
//   is built with -ffp-contract=off; the pragma below says the same to a host compiler); `1./x` is a double quotient rounded to
//   float and the pixel differences are double differences rounded to float, as the reference's types make them.
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define P3P_HD __host__ __device__ inline
#else
#define P3P_HD inline
#endif
#if defined(__clang__)
#pragma clang fp contract(off)
#else
#pragma STDC FP_CONTRACT OFF
#endif

namespace p3p {

constexpr float kMaxErr = 5.99f;          // pnpsolver.cpp:41
constexpr double kCollinearSin2 = 1e-16;  // sin^2 of the triangle's angle at P1 below which the three points count as collinear
constexpr double kRodriguesSmall = 1e-5;  // sin(theta) below which the matrix -> vector step leaves its general form (as cv::Rodrigues)

// what is uniform over the roots of one hypothesis; every member a named scalar
struct Setup {
    double p1x, p1y, p1z, p2x, p2y, p2z, p3x, p3y, p3z;   // the three world points
    double j1x, j1y, j1z, j2x, j2y, j2z, j3x, j3y, j3z;   // their unit bearings
    double x4, y4, p4x, p4y, p4z;                          // the fourth point: normalised pixel and world point
    double ca, cb, cg, a2, b2, c2, n0, n1, n2, d0, d1;     // cosines, squared side lengths, N and D
    double A0, A1, A2, A3, A4;                             // the quartic in v
    bool ok;                                               // false: degenerate sample (coincident or collinear points, non-finite input)
};

struct Pose { double r00, r01, r02, r10, r11, r12, r20, r21, r22, tx, ty, tz; };

P3P_HD void unit_bearing(double xn, double yn, double& jx, double& jy, double& jz) {
    const double inv = 1.0 / sqrt(xn * xn + yn * yn + 1.0);
    jx = xn * inv; jy = yn * inv; jz = inv;
}

// intr4 = fx fy cx cy (float, widened as OpenCV widens the float camera matrix); P: 4 x 3 world points, px: 4 x 2 pixels (floats widened)
P3P_HD void setup(const float* intr4, const float* P, const float* px, Setup& S) {
    const double fx = intr4[0], fy = intr4[1], cx = intr4[2], cy = intr4[3];
    S.p1x = P[0]; S.p1y = P[1]; S.p1z = P[2]; S.p2x = P[3]; S.p2y = P[4]; S.p2z = P[5]; S.p3x = P[6]; S.p3y = P[7]; S.p3z = P[8];
    S.p4x = P[9]; S.p4y = P[10]; S.p4z = P[11];
    unit_bearing(((double)px[0] - cx) / fx, ((double)px[1] - cy) / fy, S.j1x, S.j1y, S.j1z);
    unit_bearing(((double)px[2] - cx) / fx, ((double)px[3] - cy) / fy, S.j2x, S.j2y, S.j2z);
    unit_bearing(((double)px[4] - cx) / fx, ((double)px[5] - cy) / fy, S.j3x, S.j3y, S.j3z);
    S.x4 = ((double)px[6] - cx) / fx; S.y4 = ((double)px[7] - cy) / fy;
    const double e1x = S.p2x - S.p1x, e1y = S.p2y - S.p1y, e1z = S.p2z - S.p1z;   // P1 -> P2
    const double e2x = S.p3x - S.p1x, e2y = S.p3y - S.p1y, e2z = S.p3z - S.p1z;   // P1 -> P3
    const double e3x = S.p3x - S.p2x, e3y = S.p3y - S.p2y, e3z = S.p3z - S.p2z;   // P2 -> P3
    const double c2 = e1x * e1x + e1y * e1y + e1z * e1z, b2 = e2x * e2x + e2y * e2y + e2z * e2z, a2 = e3x * e3x + e3y * e3y + e3z * e3z;
    const double nx = e1y * e2z - e1z * e2y, ny = e1z * e2x - e1x * e2z, nz = e1x * e2y - e1y * e2x;
    const double cross2 = nx * nx + ny * ny + nz * nz;
    S.ca = S.j2x * S.j3x + S.j2y * S.j3y + S.j2z * S.j3z;
    S.cb = S.j1x * S.j3x + S.j1y * S.j3y + S.j1z * S.j3z;
    S.cg = S.j1x * S.j2x + S.j1y * S.j2y + S.j1z * S.j2z;
    S.a2 = a2; S.b2 = b2; S.c2 = c2;
    // (written so that a NaN anywhere makes the sample degenerate)
    S.ok = (cross2 > kCollinearSin2 * (c2 * b2)) && (a2 > 0.0) && (S.ca + S.cb + S.cg) == (S.ca + S.cb + S.cg) && c2 < INFINITY && b2 < INFINITY && a2 < INFINITY;
    const double k = (a2 - c2) / b2, q = c2 / b2;
    S.n2 = k - 1.0; S.n1 = -2.0 * k * S.cb; S.n0 = k + 1.0;
    S.d1 = -2.0 * S.ca; S.d0 = 2.0 * S.cg;
    const double w0 = 1.0 - q, w1 = 2.0 * q * S.cb, w2 = -q;
    const double g0 = S.d0 * S.d0, g1 = 2.0 * S.d0 * S.d1, g2 = S.d1 * S.d1;   // D^2
    const double m2g = -2.0 * S.cg;
    S.A0 = S.n0 * S.n0 + g0 * w0 + m2g * (S.n0 * S.d0);
    S.A1 = 2.0 * S.n0 * S.n1 + (g0 * w1 + g1 * w0) + m2g * (S.n0 * S.d1 + S.n1 * S.d0);
    S.A2 = (2.0 * S.n0 * S.n2 + S.n1 * S.n1) + (g0 * w2 + g1 * w1 + g2 * w0) + m2g * (S.n1 * S.d1 + S.n2 * S.d0);
    S.A3 = 2.0 * S.n1 * S.n2 + (g1 * w2 + g2 * w1) + m2g * (S.n2 * S.d1);
    S.A4 = S.n2 * S.n2 + g2 * w2;
}

// the largest real root of t^3 + a2 t^2 + a1 t + a0
P3P_HD double cubic_largest_root(double a2, double a1, double a0) {
    const double Q = (a2 * a2 - 3.0 * a1) / 9.0, R = (2.0 * a2 * a2 * a2 - 9.0 * a2 * a1 + 27.0 * a0) / 54.0;
    const double Q3 = Q * Q * Q;
    double t;
    if (R * R < Q3) {
        const double sq = sqrt(Q);
        double ct = R / (Q * sq);
        ct = ct < -1.0 ? -1.0 : (ct > 1.0 ? 1.0 : ct);
        const double th = acos(ct);
        // the three roots are -2 sqrt(Q) cos((th + 2 pi k) / 3) - a2 / 3; k = 1 gives the largest (th / 3 + 2 pi / 3 lies in [2 pi / 3, pi])
        t = -2.0 * sq * cos((th + 6.283185307179586476925286766559) / 3.0) - a2 / 3.0;
    } else {
        const double A = -(R >= 0 ? 1.0 : -1.0) * cbrt(fabs(R) + sqrt(R * R - Q3));
        const double B = A != 0.0 ? Q / A : 0.0;
        t = A + B - a2 / 3.0;
    }
    for (int it = 0; it < 2; it++) {   // Newton on the cubic itself
        const double f = ((t + a2) * t + a1) * t + a0, df = (3.0 * t + 2.0 * a2) * t + a1;
        t = df != 0.0 ? t - f / df : t;
    }
    return t;
}

P3P_HD double polish(double a4, double a3, double a2, double a1, double a0, double v) {
    for (int it = 0; it < 2; it++) {
        const double f = (((a4 * v + a3) * v + a2) * v + a1) * v + a0;
        const double df = ((4.0 * a4 * v + 3.0 * a3) * v + 2.0 * a2) * v + a1;
        const double w = df != 0.0 ? v - f / df : v;
        v = w == w ? w : v;
    }
    return v;
}

#define P3P_CSWAP(a, b) { const double lo = a < b ? a : b, hi = a < b ? b : a; a = lo; b = hi; }

// The leading coefficient A4 = 4 (c^2 / b^2) (cos^2 A - cos^2 alpha) (A: the triangle's angle at P1) vanishes on a whole surface of
// camera centres: P1 and the circumcircle, turned about the line P2 P3.  Ferrari's form divides by it, so below this share of the
// largest coefficient (and below |A0|) the quartic is solved in w = 1 / v instead, A0 w^4 + A1 w^3 + A2 w^2 + A3 w + A4, whose
// leading coefficient is then the larger of the two; a root w = 0 (A4 = 0 exactly) is the root of v at infinity and is no solution.
constexpr double kSmallLead = 1e-4;

P3P_HD bool reversed_form(double A0, double A1, double A2, double A3, double A4) {
    const double m01 = fabs(A0) > fabs(A1) ? fabs(A0) : fabs(A1), m23 = fabs(A2) > fabs(A3) ? fabs(A2) : fabs(A3);
    const double amax = m01 > m23 ? m01 : m23;
    return fabs(A4) < kSmallLead * amax && fabs(A4) < fabs(A0);
}

// The real roots of the quartic in ascending order (r0 <= r1 <= ...), the absent ones +inf; returns their number.
P3P_HD int roots(const Setup& S, double& r0, double& r1, double& r2, double& r3) {
    r0 = r1 = r2 = r3 = INFINITY;
    const bool rev = reversed_form(S.A0, S.A1, S.A2, S.A3, S.A4);
    const double a4 = rev ? S.A0 : S.A4, a3 = rev ? S.A1 : S.A3, a2 = S.A2, a1 = rev ? S.A3 : S.A1, a0 = rev ? S.A4 : S.A0;
    if (!S.ok || !(fabs(a4) > 0.0)) return 0;
    const double B = a3 / a4, Cc = a2 / a4, Dd = a1 / a4, E = a0 / a4;
    const double B2 = B * B;
    const double p = Cc - 0.375 * B2, q = Dd - 0.5 * B * Cc + 0.125 * B2 * B;
    const double r = E - 0.25 * B * Dd + 0.0625 * B2 * Cc - (3.0 / 256.0) * B2 * B2;
    const double shift = -0.25 * B;
    // (y^2 + p / 2 + m)^2 = 2 m (y - q / (4 m))^2 with m the largest root of m^3 + p m^2 + (p^2 / 4 - r) m - q^2 / 8
    const double m = cubic_largest_root(p, 0.25 * p * p - r, -0.125 * q * q);
    const double scale = fabs(p) + sqrt(fabs(r)) + 1e-300;
    if (!(m > 1e-14 * scale)) {
        // q = 0 to working precision: a biquadratic, y^2 = (-p +- sqrt(p^2 - 4 r)) / 2
        const double disc = p * p - 4.0 * r;
        if (disc >= 0.0) {
            const double sd = sqrt(disc), z1 = 0.5 * (-p + sd), z2 = 0.5 * (-p - sd);
            if (z1 >= 0.0) { const double y = sqrt(z1); r0 = shift + y; r1 = shift - y; }
            if (z2 >= 0.0) { const double y = sqrt(z2); r2 = shift + y; r3 = shift - y; }
        }
    } else {
        const double s = sqrt(2.0 * m), h = 0.5 * p + m, g = q / (2.0 * s);
        // y^2 - s y + (h + g) = 0  and  y^2 + s y + (h - g) = 0
        const double dA = s * s - 4.0 * (h + g), dB = s * s - 4.0 * (h - g);
        if (dA >= 0.0) { const double sd = sqrt(dA); r0 = shift + 0.5 * (s + sd); r1 = shift + 0.5 * (s - sd); }
        if (dB >= 0.0) { const double sd = sqrt(dB); r2 = shift + 0.5 * (-s + sd); r3 = shift + 0.5 * (-s - sd); }
    }
    r0 = r0 < INFINITY ? polish(a4, a3, a2, a1, a0, r0) : r0; r1 = r1 < INFINITY ? polish(a4, a3, a2, a1, a0, r1) : r1;
    r2 = r2 < INFINITY ? polish(a4, a3, a2, a1, a0, r2) : r2; r3 = r3 < INFINITY ? polish(a4, a3, a2, a1, a0, r3) : r3;
    if (rev) {   // back to v = 1 / w; w = 0 is the root at infinity (1 / inf = 0 would be a root at v = 0 that does not exist)
        r0 = (r0 < INFINITY && r0 != 0.0) ? 1.0 / r0 : INFINITY; r1 = (r1 < INFINITY && r1 != 0.0) ? 1.0 / r1 : INFINITY;
        r2 = (r2 < INFINITY && r2 != 0.0) ? 1.0 / r2 : INFINITY; r3 = (r3 < INFINITY && r3 != 0.0) ? 1.0 / r3 : INFINITY;
    }
    P3P_CSWAP(r0, r1) P3P_CSWAP(r2, r3) P3P_CSWAP(r0, r2) P3P_CSWAP(r1, r3) P3P_CSWAP(r1, r2)
    return (r0 < INFINITY ? 1 : 0) + (r1 < INFINITY ? 1 : 0) + (r2 < INFINITY ? 1 : 0) + (r3 < INFINITY ? 1 : 0);
}

// orthonormal frame of a triangle: f1 along A -> B, f3 along (A -> B) x (A -> C), f2 = f3 x f1
#define P3P_FRAME(ax, ay, az, bx, by, bz, cx_, cy_, cz_, F)                                                   \
    double F##1x = bx - ax, F##1y = by - ay, F##1z = bz - az;                                                 \
    {   const double i1 = 1.0 / sqrt(F##1x * F##1x + F##1y * F##1y + F##1z * F##1z);                          \
        F##1x *= i1; F##1y *= i1; F##1z *= i1; }                                                              \
    const double F##wx = cx_ - ax, F##wy = cy_ - ay, F##wz = cz_ - az;                                        \
    double F##3x = F##1y * F##wz - F##1z * F##wy, F##3y = F##1z * F##wx - F##1x * F##wz, F##3z = F##1x * F##wy - F##1y * F##wx; \
    {   const double i3 = 1.0 / sqrt(F##3x * F##3x + F##3y * F##3y + F##3z * F##3z);                          \
        F##3x *= i3; F##3y *= i3; F##3z *= i3; }                                                              \
    const double F##2x = F##3y * F##1z - F##3z * F##1y, F##2y = F##3z * F##1x - F##3x * F##1z, F##2z = F##3x * F##1y - F##3y * F##1x;

// The pose of the root v and the squared reprojection error of the fourth point (normalised coordinates).  false: the root gives
// no solution (a distance that is not positive, a vanishing D, a non-finite result).
P3P_HD bool back_substitute(const Setup& S, double v, Pose& T, double& err4) {
    const double N = (S.n2 * v + S.n1) * v + S.n0, D = S.d1 * v + S.d0;
    const double u = N / D;
    const double den = 1.0 + v * v - 2.0 * v * S.cb;
    double s1 = sqrt(S.b2 / den), s2 = u * s1, s3 = v * s1;
    // two Gauss-Newton steps on the three cosine-rule equations themselves: u = N / D loses digits where D is small, and the step
    // makes the distances as good as the data whatever the closed form left
    for (int it = 0; it < 2; it++) {
        const double f1 = s2 * s2 + s3 * s3 - 2.0 * s2 * s3 * S.ca - S.a2, f2 = s1 * s1 + s3 * s3 - 2.0 * s1 * s3 * S.cb - S.b2;
        const double f3 = s1 * s1 + s2 * s2 - 2.0 * s1 * s2 * S.cg - S.c2;
        // J = [0 j12 j13; j21 0 j23; j31 j32 0]
        const double j12 = 2.0 * (s2 - s3 * S.ca), j13 = 2.0 * (s3 - s2 * S.ca), j21 = 2.0 * (s1 - s3 * S.cb), j23 = 2.0 * (s3 - s1 * S.cb);
        const double j31 = 2.0 * (s1 - s2 * S.cg), j32 = 2.0 * (s2 - s1 * S.cg);
        const double det = j12 * j23 * j31 + j13 * j21 * j32;
        const double d1 = (-j23 * j32) * f1 + (j13 * j32) * f2 + (j12 * j23) * f3;
        const double d2 = (j23 * j31) * f1 + (-j13 * j31) * f2 + (j13 * j21) * f3;
        const double d3 = (j21 * j32) * f1 + (j12 * j31) * f2 + (-j12 * j21) * f3;
        const double id = 1.0 / det;
        const bool good = (id - id == 0.0);
        s1 = good ? s1 - d1 * id : s1; s2 = good ? s2 - d2 * id : s2; s3 = good ? s3 - d3 * id : s3;
    }
    const double q1x = s1 * S.j1x, q1y = s1 * S.j1y, q1z = s1 * S.j1z;
    const double q2x = s2 * S.j2x, q2y = s2 * S.j2y, q2z = s2 * S.j2z;
    const double q3x = s3 * S.j3x, q3y = s3 * S.j3y, q3z = s3 * S.j3z;
    P3P_FRAME(S.p1x, S.p1y, S.p1z, S.p2x, S.p2y, S.p2z, S.p3x, S.p3y, S.p3z, w)
    P3P_FRAME(q1x, q1y, q1z, q2x, q2y, q2z, q3x, q3y, q3z, f)
    // R = f1 w1' + f2 w2' + f3 w3'
    T.r00 = f1x * w1x + f2x * w2x + f3x * w3x; T.r01 = f1x * w1y + f2x * w2y + f3x * w3y; T.r02 = f1x * w1z + f2x * w2z + f3x * w3z;
    T.r10 = f1y * w1x + f2y * w2x + f3y * w3x; T.r11 = f1y * w1y + f2y * w2y + f3y * w3y; T.r12 = f1y * w1z + f2y * w2z + f3y * w3z;
    T.r20 = f1z * w1x + f2z * w2x + f3z * w3x; T.r21 = f1z * w1y + f2z * w2y + f3z * w3y; T.r22 = f1z * w1z + f2z * w2z + f3z * w3z;
    T.tx = q1x - (T.r00 * S.p1x + T.r01 * S.p1y + T.r02 * S.p1z);
    T.ty = q1y - (T.r10 * S.p1x + T.r11 * S.p1y + T.r12 * S.p1z);
    T.tz = q1z - (T.r20 * S.p1x + T.r21 * S.p1y + T.r22 * S.p1z);
    const double X = T.r00 * S.p4x + T.r01 * S.p4y + T.r02 * S.p4z + T.tx;
    const double Y = T.r10 * S.p4x + T.r11 * S.p4y + T.r12 * S.p4z + T.ty;
    const double Z = T.r20 * S.p4x + T.r21 * S.p4y + T.r22 * S.p4z + T.tz;
    const double ex = X / Z - S.x4, ey = Y / Z - S.y4;
    err4 = ex * ex + ey * ey;
    const double chk = T.r00 + T.r01 + T.r02 + T.r10 + T.r11 + T.r12 + T.r20 + T.r21 + T.r22 + T.tx + T.ty + T.tz;
    return (v > 0.0) && (v < INFINITY) && (u > 0.0) && (s1 > 0.0) && (s2 > 0.0) && (s3 > 0.0) && (chk - chk == 0.0);
}

// Rotation matrix -> Rodrigues vector in double: theta = atan2(sin, cos) from the skew part and the trace; near theta = 0 the skew
// part itself (first order); near theta = pi the axis from the symmetric part, its sign from the skew part.
P3P_HD void rodrigues(const Pose& T, double& rx, double& ry, double& rz) {
    const double sx = T.r21 - T.r12, sy = T.r02 - T.r20, sz = T.r10 - T.r01;
    const double s = 0.5 * sqrt(sx * sx + sy * sy + sz * sz);
    double c = 0.5 * (T.r00 + T.r11 + T.r22 - 1.0);
    c = c > 1.0 ? 1.0 : (c < -1.0 ? -1.0 : c);
    const double theta = atan2(s, c);
    if (s < kRodriguesSmall) {
        if (c > 0.0) {
            rx = 0.5 * sx; ry = 0.5 * sy; rz = 0.5 * sz;
        } else {
            // (R + R') / 2 - c I = (1 - c) a a': the column of its largest diagonal entry is the axis times a factor of at least
            // (1 - c) / sqrt(3), every component to an absolute 1e-16.  (The square roots of the diagonal, the form cv::Rodrigues has, lose
            // half the digits of a component near zero: 2.8e-7 on R for a turn by pi about a coordinate axis.)
            const double m00 = T.r00 - c, m11 = T.r11 - c, m22 = T.r22 - c;
            const double m01 = 0.5 * (T.r01 + T.r10), m02 = 0.5 * (T.r02 + T.r20), m12 = 0.5 * (T.r12 + T.r21);
            const bool c0 = m00 >= m11 && m00 >= m22, c1 = !c0 && m11 >= m22;
            double ax = c0 ? m00 : (c1 ? m01 : m02), ay = c0 ? m01 : (c1 ? m11 : m12), az = c0 ? m02 : (c1 ? m12 : m22);
            // at pi itself a and -a are the same turn: the first component that is not zero is made positive
            if (ax < 0.0 || (ax == 0.0 && (ay < 0.0 || (ay == 0.0 && az < 0.0)))) { ax = -ax; ay = -ay; az = -az; }
            // short of pi itself the skew part says which of the two it is
            const double sgn = ax * sx + ay * sy + az * sz < 0.0 ? -1.0 : 1.0;
            const double k = sgn * theta / sqrt(ax * ax + ay * ay + az * az);
            rx = ax * k; ry = ay * k; rz = az * k;
        }
    } else {
        const double k = theta / (2.0 * s);
        rx = sx * k; ry = sy * k; rz = sz * k;
    }
}

// (rvec, tvec) in double -> the float rt[6] of Se3Transform::set(cv::Mat, cv::Mat), se3transform.h:124-140
P3P_HD void rt6_of(const Pose& T, float* rt6) {
    double rx, ry, rz;
    rodrigues(T, rx, ry, rz);
    rt6[0] = (float)rx; rt6[1] = (float)ry; rt6[2] = (float)rz; rt6[3] = (float)T.tx; rt6[4] = (float)T.ty; rt6[5] = (float)T.tz;
}

// Se3Transform::set(const float* rt), se3transform.h:143-176: the 12 floats of rows 0..2.  The unqualified cos / sin are taken as the
// double functions on the float angle, rounded to float once (UNPINNED: with OpenCV's headers in scope they may be the float overloads).
struct M34 { float m0, m1, m2, m3, m4, m5, m6, m7, m8, m9, m10, m11; };
P3P_HD void se3_set(const float* rt, M34& M) {
    const float rx = rt[0], ry = rt[1], rz = rt[2], tx = rt[3], ty = rt[4], tz = rt[5];
    const float nsqa = rx * rx + ry * ry + rz * rz;
    const float a = sqrtf(nsqa);
    const float i_a = a ? (float)(1. / (double)a) : 0.f;
    const float rnx = rx * i_a, rny = ry * i_a, rnz = rz * i_a;
    const float cos_a = (float)cos((double)a), sin_a = (float)sin((double)a);
    const float _1_cos_a = (float)(1. - (double)cos_a);
    M.m0 = cos_a + rnx * rnx * _1_cos_a;
    M.m1 = rnx * rny * _1_cos_a - rnz * sin_a;
    M.m2 = rny * sin_a + rnx * rnz * _1_cos_a;
    M.m3 = tx;
    M.m4 = rnz * sin_a + rnx * rny * _1_cos_a;
    M.m5 = cos_a + rny * rny * _1_cos_a;
    M.m6 = -rnx * sin_a + rny * rnz * _1_cos_a;
    M.m7 = ty;
    M.m8 = -rny * sin_a + rnx * rnz * _1_cos_a;
    M.m9 = rnx * sin_a + rny * rnz * _1_cos_a;
    M.m10 = cos_a + rnz * rnz * _1_cos_a;
    M.m11 = tz;
}

// camCenter = f2g.inv() * (0, 0, 0), se3transform.h:89-113 (the float expressions pnp.hip's pnp_decide and projmatch.hip restate)
P3P_HD void cam_center(const M34& M, float& c0, float& c1, float& c2) {
    const float i0 = M.m0, i1 = M.m4, i2 = M.m8, i4 = M.m1, i5 = M.m5, i6 = M.m9, i8 = M.m2, i9 = M.m6, i10 = M.m10;
    const float i3 = -(M.m3 * i0 + M.m7 * i1 + M.m11 * i2), i7 = -(M.m3 * i4 + M.m7 * i5 + M.m11 * i6), i11 = -(M.m3 * i8 + M.m7 * i9 + M.m11 * i10);
    c0 = i0 * 0.f + i1 * 0.f + i2 * 0.f + i3;
    c1 = i4 * 0.f + i5 * 0.f + i6 * 0.f + i7;
    c2 = i8 * 0.f + i9 * 0.f + i10 * 0.f + i11;
}

// MapPoint::getViewCos, mappoint.h:99: v = camCenter - pos3d; v *= 1. / cv::norm(v) (a double factor, each product rounded to float); v.dot(normal)
P3P_HD float view_cos(float c0, float c1, float c2, float px, float py, float pz, float nx, float ny, float nz) {
    float v0 = c0 - px, v1 = c1 - py, v2 = c2 - pz;
    const double s = 1. / sqrt((double)v0 * v0 + (double)v1 * v1 + (double)v2 * v2);
    v0 = (float)(v0 * s); v1 = (float)(v1 * s); v2 = (float)(v2 * s);
    return v0 * nx + v1 * ny + v2 * nz;
}

// pnpsolver.cpp:75-100 for one match: err2 = the squared pixel distance, vc = the view cosine.  Inlier iff err2 < 5.99f and not
// vc < 0.5 — no test of the depth's sign; a zero depth gives inf / NaN and a false comparison.
P3P_HD bool inlier(const M34& M, float fx, float fy, float cx, float cy, float c0, float c1, float c2, float px, float py, float pz,
                   float nx, float ny, float nz, float kx, float ky, float& err2, float& vc) {
    const float x = M.m0 * px + M.m1 * py + M.m2 * pz + M.m3;
    const float y = M.m4 * px + M.m5 * py + M.m6 * pz + M.m7;
    const float z = M.m8 * px + M.m9 * py + M.m10 * pz + M.m11;
    const float iz = (float)(1. / (double)z);
    const float u = ((fx * x) * iz) + cx, v = ((fy * y) * iz) + cy;
    const float dx = (float)((double)kx - (double)u), dy = (float)((double)ky - (double)v);
    err2 = dx * dx + dy * dy;
    vc = view_cos(c0, c1, c2, px, py, pz, nx, ny, nz);
    return (err2 < kMaxErr) && !(vc < 0.5);
}

// One hypothesis on one thread (host builds, the debug comparison): every solution in root order, the pick, the float rt[6].
// sol: up to 4 poses; returns the number of solutions, chosen = -1 when the iteration is skipped.
P3P_HD int hypothesis(const float* intr4, const float* P, const float* px, Pose* sol, int& chosen, float* rt6) {
    Setup S;
    setup(intr4, P, px, S);
    double r0, r1, r2, r3;
    roots(S, r0, r1, r2, r3);
    int n = 0;
    chosen = -1;
    double best = INFINITY;
    for (int k = 0; k < 4; k++) {
        const double v = k == 0 ? r0 : (k == 1 ? r1 : (k == 2 ? r2 : r3));
        Pose T;
        double e;
        if (!(v < INFINITY) || !back_substitute(S, v, T, e)) continue;
        sol[n] = T;
        if (e < best) { best = e; chosen = n; }
        n++;
    }
    if (chosen >= 0) rt6_of(sol[chosen], rt6);
    return n;
}

}  // namespace p3p
