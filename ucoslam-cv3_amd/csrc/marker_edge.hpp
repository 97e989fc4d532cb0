// The marker edge of bundle adjustment (MarkerEdge, typesg2o.h:108-167), kernels and host code alike: fp64 on se3.hpp's helpers.
//
// Vertex 0 = the marker's pose g2m, vertex 1 = the camera c2g, both VertexSE3Expmap held as pose7 = (qx qy qz qw tx ty tz), the state
// SE3Quat keeps.  Error, eight rows: measured corner - projection of the corner (-+s/2, +-s/2, 0) through Transform = c2g * g2m, every
// projected coordinate ROUNDED TO FLOAT.  The edge has no linearizeOplus, so g2o differentiates it numerically on both vertices
// (base_binary_edge.hpp:166-233): central differences with delta = (double)1e-4f (_delta_der is a float member), every perturbed
// vertex is SE3Quat::exp(+-delta e_d) * estimate with the renormalisation SE3Quat's product applies.  That makes 25 evaluations:
//   k = 0         the centre
//   k = 1 + d     marker + delta along dimension d (0..2 rotation, 3..5 translation),  k = 7 + d   marker - delta
//   k = 13 + d    camera + delta,                                                      k = 19 + d  camera - delta
// and Jacobian column d of a vertex = (error(+) - error(-)) / (2 delta).  A rounding of one projection that falls the other way moves
// a Jacobian entry by ulp / (2 delta) ~ 0.1-0.3: callers compare against the reference only where its own jitter screen holds.
#pragma once
#include "se3.hpp"

constexpr double kMkDelta = 0x1.a36e2ep-14;               // (double)1e-4f
constexpr double kMkScalar = 1 / (2 * kMkDelta);
// SE3Quat::exp for omega = +-delta e_d: theta = delta >= 1e-5, R = I + (sin(theta) / theta) Omega + ((1 - cos(theta)) / theta^2) Omega^2;
// the two coefficients in double, as constants (tests/test_ba_marker.py checks them against the host's libm)
constexpr double kMkSinc = 0x1.fffffff1aef63p-1, kMkCosc = 0x1.00000000299fdp-1;

// Marker::get3DPointsLocalRefSystem(size): cv::Point3f(+-size / 2., ...), the halves taken in double and rounded to float
__host__ __device__ __forceinline__ double marker_half(float size) { return (double)(float)((double)size / 2.); }

// a * b of unit quaternions (Eigen::Quaternion::operator*), not normalised
__host__ __device__ __forceinline__ void mk_quat_mul(const double* a, const double* b, double* o) {
    o[3] = a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2];
    o[0] = a[3] * b[0] + a[0] * b[3] + a[1] * b[2] - a[2] * b[1];
    o[1] = a[3] * b[1] + a[1] * b[3] + a[2] * b[0] - a[0] * b[2];
    o[2] = a[3] * b[2] + a[2] * b[3] + a[0] * b[1] - a[1] * b[0];
}
// q * v (Eigen::Quaternion::_transformVector): v + w uv + q.vec x uv with uv = 2 q.vec x v
__host__ __device__ __forceinline__ void mk_quat_rot(const double* q, double v0, double v1, double v2, double& o0, double& o1, double& o2) {
    const double u0 = 2 * (q[1] * v2 - q[2] * v1), u1 = 2 * (q[2] * v0 - q[0] * v2), u2 = 2 * (q[0] * v1 - q[1] * v0);
    o0 = v0 + q[3] * u0 + (q[1] * u2 - q[2] * u1);
    o1 = v1 + q[3] * u1 + (q[2] * u0 - q[0] * u2);
    o2 = v2 + q[3] * u2 + (q[0] * u1 - q[1] * u0);
}
// SE3Quat::operator*: t = A.t + A.r * B.t, r = A.r * B.r, normalizeRotation()
__host__ __device__ __forceinline__ void mk_se3_mul(const double* A, const double* B, double* O) {
    double r0, r1, r2;
    mk_quat_rot(A, B[4], B[5], B[6], r0, r1, r2);
    O[4] = A[4] + r0; O[5] = A[5] + r1; O[6] = A[6] + r2;
    mk_quat_mul(A, B, O);
    quat_norm_pos(O);
}
// SE3Quat::exp(sg * delta * e_d) as pose7.  d < 3: a rotation (upsilon = 0, so t = V * 0 = 0); d >= 3: omega = 0 takes the small-angle
// branch, R = I and V = I, so t = sg * delta * e_(d - 3).  Written with selects: d differs from lane to lane in the kernel.
__host__ __device__ __forceinline__ void mk_se3_exp_unit(int d, double sg, double* E) {
    const double s = sg * kMkDelta;
    const double w0 = d == 0 ? s : 0.0, w1 = d == 1 ? s : 0.0, w2 = d == 2 ? s : 0.0;
    const double a = d < 3 ? kMkSinc : 1.0, b = d < 3 ? kMkCosc : 0.5;
    double R[9];
    R[0] = 1.0 + b * -(w1 * w1 + w2 * w2); R[1] = a * -w2 + b * (w0 * w1);        R[2] = a * w1 + b * (w0 * w2);
    R[3] = a * w2 + b * (w0 * w1);         R[4] = 1.0 + b * -(w0 * w0 + w2 * w2); R[5] = a * -w0 + b * (w1 * w2);
    R[6] = a * -w1 + b * (w0 * w2);        R[7] = a * w0 + b * (w1 * w2);         R[8] = 1.0 + b * -(w0 * w0 + w1 * w1);
    quat_from_R(R, E);
    quat_norm_pos(E);
    E[4] = d == 3 ? s : 0.0; E[5] = d == 4 ? s : 0.0; E[6] = d == 5 ? s : 0.0;
}

// Transform = c2g * g2m of evaluation k (0..24, see the head of the file)
__host__ __device__ __forceinline__ void mk_edge_transform(int k, const double* g2m, const double* c2g, double* c2m) {
    if (k == 0) { mk_se3_mul(c2g, g2m, c2m); return; }
    const bool on_camera = k > 12;
    const int j = on_camera ? k - 13 : k - 1;   // 0..5: + delta, 6..11: - delta
    const int d = j > 5 ? j - 6 : j;
    // (values are selected, not pointers: a select between two register arrays would send both to scratch)
    double E[7], X[7], V[7], A[7], B[7];
    mk_se3_exp_unit(d, j > 5 ? -1.0 : 1.0, E);
    for (int i = 0; i < 7; i++) X[i] = on_camera ? c2g[i] : g2m[i];
    mk_se3_mul(E, X, V);                         // VertexSE3Expmap::oplusImpl: exp(update) * estimate
    for (int i = 0; i < 7; i++) { A[i] = on_camera ? V[i] : c2g[i]; B[i] = on_camera ? g2m[i] : V[i]; }
    mk_se3_mul(A, B, c2m);
}

// The two error rows of corner c (0..3: (-h, h), (h, h), (h, -h), (-h, -h), z = 0) under Transform: obs - (float)(x / z * fx + cx), in double
__host__ __device__ __forceinline__ void mk_corner_error(const double* c2m, int c, double half, const double* intr4, double u, double v, double& ex, double& ey) {
    const double px = (c == 1 || c == 2) ? half : -half, py = c < 2 ? half : -half;
    double p0, p1, p2;
    mk_quat_rot(c2m, px, py, 0.0, p0, p1, p2);
    p0 += c2m[4]; p1 += c2m[5]; p2 += c2m[6];
    const double projx = (double)(float)((p0 / p2) * intr4[0] + intr4[2]), projy = (double)(float)((p1 / p2) * intr4[1] + intr4[3]);
    ex = u - projx;
    ey = v - projy;
}

// What one marker edge adds to the system (constructQuadraticForm, base_binary_edge.hpp:83-122, no robust kernel, information w * I8)
// from the 25 x 8 errors err[k][row]: entry q of
//   [0, 36)    A += Ji^T w Ji     the marker's 6 x 6, row-major          [36, 42)   b_i -= Ji^T w e
//   [42, 78)   B += Jj^T w Jj     the camera's                            [78, 84)   b_j -= Jj^T w e
//   [84, 120)  Ji^T w Jj          row = marker dimension, column = camera dimension
// camera_free == false (a fixed frame, whose Jacobian g2o never computes) leaves [42, 120) zero.
constexpr int kMkBlock = 120;
__host__ __device__ __forceinline__ double mk_jac(const double (*err)[8], int first, int dim, int row) {
    return kMkScalar * (err[first + dim][row] - err[first + 6 + dim][row]);
}
__host__ __device__ __forceinline__ double mk_block_entry(const double (*err)[8], double w, bool camera_free, int q) {
    if (q >= 42 && !camera_free) return 0.0;
    const int part = q < 42 ? 0 : (q < 84 ? 1 : 2), r = q - (part == 0 ? 0 : (part == 1 ? 42 : 84));
    double acc = 0;
    if (part < 2 && r >= 36) {   // right-hand side: J^T (-w e)
        const int first = part == 0 ? 1 : 13;
        for (int row = 0; row < 8; row++) acc += mk_jac(err, first, r - 36, row) * (-(w * err[0][row]));
        return acc;
    }
    const int a = r / 6, c = r - 6 * a;
    const int fa = part == 1 ? 13 : 1, fc = part == 0 ? 1 : 13;
    for (int row = 0; row < 8; row++) acc += (mk_jac(err, fa, a, row) * w) * mk_jac(err, fc, c, row);
    return acc;
}
// chi2 = e^T (w I) e at the centre
__host__ __device__ __forceinline__ double mk_chi2(const double (*err)[8], double w) {
    double acc = 0;
    for (int row = 0; row < 8; row++) acc += err[0][row] * (w * err[0][row]);
    return acc;
}
