// g2o::Sim3 (g2o/types/sim3/sim3.h) restated for the pose-graph kernels (posegraph.hip), kernels and host code alike: fp64, a similarity is
// eight doubles (qx qy qz qw tx ty tz s), matrices are row-major 3x3.  Every branch of the reference's exp and log is kept with its own
// threshold, and which operations normalise the quaternion is kept too: the three-argument constructors and inverse() do, operator* and the
// exponential do not.
#pragma once
#include "se3.hpp"

namespace sim3 {

constexpr double kEps = 0.00001;   // sim3.h:86 / :154

__host__ __device__ __forceinline__ void quat_mul(const double* a, const double* b, double* o) {   // Eigen: a * b, q = (x, y, z, w)
    const double w = a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2];
    const double x = a[3] * b[0] + a[0] * b[3] + a[1] * b[2] - a[2] * b[1];
    const double y = a[3] * b[1] + a[1] * b[3] + a[2] * b[0] - a[0] * b[2];
    const double z = a[3] * b[2] + a[2] * b[3] + a[0] * b[1] - a[1] * b[0];
    o[0] = x; o[1] = y; o[2] = z; o[3] = w;
}

__host__ __device__ __forceinline__ void quat_rot(const double* q, const double* v, double* o) {   // Eigen: q * v (uv = 2 q.vec x v; v + w uv + q.vec x uv)
    double ux = q[1] * v[2] - q[2] * v[1], uy = q[2] * v[0] - q[0] * v[2], uz = q[0] * v[1] - q[1] * v[0];
    ux += ux; uy += uy; uz += uz;
    const double cx = q[1] * uz - q[2] * uy, cy = q[2] * ux - q[0] * uz, cz = q[0] * uy - q[1] * ux;
    o[0] = v[0] + q[3] * ux + cx; o[1] = v[1] + q[3] * uy + cy; o[2] = v[2] + q[3] * uz + cz;
}

// operator*: neither factor nor result is normalised
__host__ __device__ __forceinline__ void mul(const double* a, const double* b, double* o) {
    double q[4], rt[3];
    quat_mul(a, b, q);
    quat_rot(a, b + 4, rt);
    const double s = a[7];
    o[4] = s * rt[0] + a[4]; o[5] = s * rt[1] + a[5]; o[6] = s * rt[2] + a[6];
    o[0] = q[0]; o[1] = q[1]; o[2] = q[2]; o[3] = q[3];
    o[7] = s * b[7];
}

// inverse(): Sim3(r.conjugate(), r.conjugate() * ((-1/s) t), 1/s), a normalising constructor
__host__ __device__ __forceinline__ void inverse(const double* a, double* o) {
    const double qc[4] = {-a[0], -a[1], -a[2], a[3]};
    const double f = -1 / a[7];
    const double v[3] = {f * a[4], f * a[5], f * a[6]};
    double t[3];
    quat_rot(qc, v, t);
    o[0] = qc[0]; o[1] = qc[1]; o[2] = qc[2]; o[3] = qc[3];
    quat_norm_pos(o);
    o[4] = t[0]; o[5] = t[1]; o[6] = t[2];
    o[7] = 1 / a[7];
}

// getSim3 (graphoptsim3.cpp:32-52): Sim3(Matrix3 of the float 4x4 widened, t widened, 1)
__host__ __device__ __forceinline__ void from_pose(const float* M, double* o) {
    const double R[9] = {M[0], M[1], M[2], M[4], M[5], M[6], M[8], M[9], M[10]};
    quat_from_R(R, o);
    quat_norm_pos(o);
    o[4] = M[3]; o[5] = M[7]; o[6] = M[11];
    o[7] = 1.0;
}

// the output of graphoptsim3.cpp:156-165: [sR | t/s] rounded to float, last row 0 0 0 1
__host__ __device__ __forceinline__ void to_pose(const double* a, float* M) {
    double R[9];
    quat_to_R(a, R);
    const double s = a[7], is = 1. / s;
    M[0] = (float)(R[0] * s); M[1] = (float)(R[1] * s); M[2] = (float)(R[2] * s); M[3] = (float)(a[4] * is);
    M[4] = (float)(R[3] * s); M[5] = (float)(R[4] * s); M[6] = (float)(R[5] * s); M[7] = (float)(a[5] * is);
    M[8] = (float)(R[6] * s); M[9] = (float)(R[7] * s); M[10] = (float)(R[8] * s); M[11] = (float)(a[6] * is);
    M[12] = 0.f; M[13] = 0.f; M[14] = 0.f; M[15] = 1.f;
}

__host__ __device__ __forceinline__ void skew(const double* v, double* m) {
    m[0] = 0; m[1] = -v[2]; m[2] = v[1];
    m[3] = v[2]; m[4] = 0; m[5] = -v[0];
    m[6] = -v[1]; m[7] = v[0]; m[8] = 0;
}

__host__ __device__ __forceinline__ void mat3_mul(const double* a, const double* b, double* o) {
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) o[3 * i + j] = a[3 * i] * b[j] + a[3 * i + 1] * b[3 + j] + a[3 * i + 2] * b[6 + j];
}

// Sim3(const Vector7& update), sim3.h:66-135: (omega, upsilon, sigma); r = Quaternion(R) is NOT normalised
__host__ __device__ __forceinline__ void exp(const double* u, double* o) {
    const double sigma = u[6];
    const double theta = sqrt(u[0] * u[0] + u[1] * u[1] + u[2] * u[2]);
    double Om[9], Om2[9], R[9];
    skew(u, Om);
    const double s = ::exp(sigma);
    mat3_mul(Om, Om, Om2);
    double A, B, C;
    if (fabs(sigma) < kEps) {
        C = 1;
        if (theta < kEps) {
            A = 1. / 2.;
            B = 1. / 6.;
#pragma unroll
            for (int i = 0; i < 9; i++) R[i] = ((i % 4 == 0 ? 1.0 : 0.0) + Om[i]) + Om2[i] / 2;
        } else {
            const double theta2 = theta * theta;
            A = (1 - cos(theta)) / (theta2);
            B = (theta - sin(theta)) / (theta2 * theta);
            const double f1 = sin(theta) / theta, f2 = (1 - cos(theta)) / (theta * theta);
#pragma unroll
            for (int i = 0; i < 9; i++) R[i] = ((i % 4 == 0 ? 1.0 : 0.0) + f1 * Om[i]) + f2 * Om2[i];
        }
    } else {
        C = (s - 1) / sigma;
        if (theta < kEps) {
            const double sigma2 = sigma * sigma;
            A = ((sigma - 1) * s + 1) / sigma2;
            B = ((0.5 * sigma2 - sigma + 1) * s - 1) / (sigma2 * sigma);
#pragma unroll
            for (int i = 0; i < 9; i++) R[i] = ((i % 4 == 0 ? 1.0 : 0.0) + Om[i]) + Om2[i] / 2;
        } else {
            const double f1 = sin(theta) / theta, f2 = (1 - cos(theta)) / (theta * theta);
#pragma unroll
            for (int i = 0; i < 9; i++) R[i] = ((i % 4 == 0 ? 1.0 : 0.0) + f1 * Om[i]) + f2 * Om2[i];
            const double a = s * sin(theta);
            const double b = s * cos(theta);
            const double theta2 = theta * theta;
            const double sigma2 = sigma * sigma;
            const double c = theta2 + sigma2;
            A = (a * sigma + (1 - b) * theta) / (theta * c);
            B = (C - ((b - 1) * sigma + a * theta) / (c)) * 1 / (theta2);
        }
    }
    quat_from_R(R, o);
    // t = (A Omega + B Omega2 + C I) upsilon
    double W[9];
#pragma unroll
    for (int i = 0; i < 9; i++) W[i] = (A * Om[i] + B * Om2[i]) + (i % 4 == 0 ? C : 0.0);
#pragma unroll
    for (int i = 0; i < 3; i++) o[4 + i] = W[3 * i] * u[3] + W[3 * i + 1] * u[4] + W[3 * i + 2] * u[5];
    o[7] = s;
}

// W x = t by LU with partial pivoting (Eigen's PartialPivLU on a 3x3: the largest |entry| of the column, the first one on a tie)
__host__ __device__ __forceinline__ void lu_solve3(const double* W, const double* t, double* x) {
    double a0[4] = {W[0], W[1], W[2], t[0]}, a1[4] = {W[3], W[4], W[5], t[1]}, a2[4] = {W[6], W[7], W[8], t[2]};
#define UH_SIM3_SWAP(p, q) { _Pragma("unroll") for (int k = 0; k < 4; k++) { const double h = p[k]; p[k] = q[k]; q[k] = h; } }
    if (fabs(a1[0]) > fabs(a0[0]) && !(fabs(a2[0]) > fabs(a1[0]))) UH_SIM3_SWAP(a0, a1)
    else if (fabs(a2[0]) > fabs(a0[0])) UH_SIM3_SWAP(a0, a2)
    const double l10 = a1[0] / a0[0], l20 = a2[0] / a0[0];
    a1[1] -= l10 * a0[1]; a1[2] -= l10 * a0[2];
    a2[1] -= l20 * a0[1]; a2[2] -= l20 * a0[2];
    if (fabs(a2[1]) > fabs(a1[1])) {
        UH_SIM3_SWAP(a1, a2)
        // (the multipliers of column 0 travel with their rows)
        const double l21 = a2[1] / a1[1];
        a2[2] -= l21 * a1[2];
        const double y0 = a0[3], y1 = a1[3] - l20 * y0, y2 = (a2[3] - l10 * y0) - l21 * y1;
        x[2] = y2 / a2[2];
        x[1] = (y1 - a1[2] * x[2]) / a1[1];
        x[0] = ((y0 - a0[1] * x[1]) - a0[2] * x[2]) / a0[0];
    } else {
        const double l21 = a2[1] / a1[1];
        a2[2] -= l21 * a1[2];
        const double y0 = a0[3], y1 = a1[3] - l10 * y0, y2 = (a2[3] - l20 * y0) - l21 * y1;
        x[2] = y2 / a2[2];
        x[1] = (y1 - a1[2] * x[2]) / a1[1];
        x[0] = ((y0 - a0[1] * x[1]) - a0[2] * x[2]) / a0[0];
    }
#undef UH_SIM3_SWAP
}

// log(), sim3.h:141-220
__host__ __device__ __forceinline__ void log(const double* a, double* res) {
    const double s = a[7];
    const double sigma = ::log(s);
    double R[9], Om[9], om[3];
    quat_to_R(a, R);
    const double d = 0.5 * (R[0] + R[4] + R[8] - 1);
    const double dR[3] = {R[7] - R[5], R[2] - R[6], R[3] - R[1]};
    double A, B, C;
    if (fabs(sigma) < kEps) {
        C = 1;
        if (d > 1 - kEps) {
            om[0] = 0.5 * dR[0]; om[1] = 0.5 * dR[1]; om[2] = 0.5 * dR[2];
            A = 1. / 2.;
            B = 1. / 6.;
        } else {
            const double theta = acos(d);
            const double theta2 = theta * theta;
            const double f = theta / (2 * sqrt(1 - d * d));
            om[0] = f * dR[0]; om[1] = f * dR[1]; om[2] = f * dR[2];
            A = (1 - cos(theta)) / (theta2);
            B = (theta - sin(theta)) / (theta2 * theta);
        }
    } else {
        C = (s - 1) / sigma;
        if (d > 1 - kEps) {
            const double sigma2 = sigma * sigma;
            om[0] = 0.5 * dR[0]; om[1] = 0.5 * dR[1]; om[2] = 0.5 * dR[2];
            A = ((sigma - 1) * s + 1) / (sigma2);
            B = ((0.5 * sigma2 - sigma + 1) * s - 1) / (sigma2 * sigma);
        } else {
            const double theta = acos(d);
            const double f = theta / (2 * sqrt(1 - d * d));
            om[0] = f * dR[0]; om[1] = f * dR[1]; om[2] = f * dR[2];
            const double theta2 = theta * theta;
            const double aa = s * sin(theta);
            const double bb = s * cos(theta);
            const double c = theta2 + sigma * sigma;
            A = (aa * sigma + (1 - bb) * theta) / (theta * c);
            B = (C - ((bb - 1) * sigma + aa * theta) / (c)) * 1 / (theta2);
        }
    }
    skew(om, Om);
    // W = A Omega + B Omega Omega + C I, the middle term as (B Omega) Omega
    double BOm[9], BOm2[9], W[9];
#pragma unroll
    for (int i = 0; i < 9; i++) BOm[i] = B * Om[i];
    mat3_mul(BOm, Om, BOm2);
#pragma unroll
    for (int i = 0; i < 9; i++) W[i] = (A * Om[i] + BOm2[i]) + (i % 4 == 0 ? C : 0.0);
    lu_solve3(W, a + 4, res + 3);
    res[0] = om[0]; res[1] = om[1]; res[2] = om[2];
    res[6] = sigma;
}

// EdgeSim3::computeError (typesg2o.h:729-737): log(C * Si * Sj^-1)
__host__ __device__ __forceinline__ void edge_error(const double* C, const double* si, const double* sj, double* e) {
    double inv[8], m1[8], m2[8];
    inverse(sj, inv);
    mul(C, si, m1);
    mul(m1, inv, m2);
    log(m2, e);
}

// VertexSim3Expmap::oplusImpl (typesg2o.h:684-693) on a copy of the update: Sim3(update) * estimate
__host__ __device__ __forceinline__ void oplus(const double* est, const double* update, bool fix_scale, double* o) {
    double u[7] = {update[0], update[1], update[2], update[3], update[4], update[5], fix_scale ? 0.0 : update[6]};
    double d[8];
    exp(u, d);
    mul(d, est, o);
}

}  // namespace sim3
