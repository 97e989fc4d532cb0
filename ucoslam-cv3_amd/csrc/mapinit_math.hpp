// Arithmetic of the two-view map initialiser (mapinit.hip), written once for the device and for the host: MapInitializer's
// "initialise" (src/utils/mapinitializer.cpp, ORB-SLAM's Initializer) — normalisation, the two 8-point systems and their null vectors,
// the rank-2 projection, both decompositions, the triangulation and the per-match bodies of CheckHomography / CheckFundamental / CheckRT.
//
// Float conventions (those of newpoints_math.hpp and p3p_math.hpp): every float expression of the reference stays a float expression in
// its written order, uncontracted; products taken through cv::Mat's operator* accumulate each element in double and round once;
// cv::norm is a double; a division of a matrix by a scalar is a multiplication by the float (float)(1 / s).  Every SVD runs in double on
// the float matrix and its results are rounded to float once.
//
// SIGN RULE of every singular vector pair (OpenCV's choice cannot be known here): the right singular vector has its component of the
// largest magnitude positive (the first such component on ties), and the left vector follows it (u = A v / sigma).  Where the third
// singular value of a 3x3 is below 1e-10 of the first, A v / sigma carries no direction: then u3 = (u1 x u2) * sign(det V), which
// makes det(U) det(V) = +1.  tests/mapinit_oracle.py applies the same rule to LAPACK's vectors.
//
// UNPINNED (no OpenCV exists to compare against): every cv::SVDecomp / cv::SVD::compute, cv::Mat::inv on 3x3 floats, cv::determinant,
// the float GEMM products, cv::norm, and acos (taken in double on the float cosine, rounded once).
#pragma once
#include <cmath>
#include <cstdint>
#include "newpoints_math.hpp"

#if defined(__HIPCC__)
#define MI_HD __host__ __device__ inline
#else
#define MI_HD inline
#endif
#if defined(__HIP_DEVICE_COMPILE__)
#define MI_SYNC() __syncthreads()
#define MI_UNROLL _Pragma("unroll")
#else
#define MI_SYNC()
#define MI_UNROLL
#endif
#if defined(__clang__)
#pragma clang fp contract(off)
#else
#pragma STDC FP_CONTRACT OFF
#endif

namespace mim {

constexpr int kMaxSweeps = 30;          // one-sided Jacobi on nine columns: converged sweeps end the loop (6 to 9 in practice)
constexpr int kWsRowsH = 16 + 9, kWsRowsF = 8 + 9;   // workspace rows: the system above the 9x9 V
enum Model : int32_t { kNone = 0, kHomography = 1, kFundamental = 2 };
enum State : uint8_t { kNotInlier = 0, kRejected = 1, kCountedLowParallax = 2, kCountedGood = 3, kNonFinite = 4 };

// ---------------------------------------------------------------- Normalize (:633-671): sequential float sums over ALL keypoints
struct Norm { float mx, my, sx, sy; float T[9]; };
inline void normalise(const float* xy, int n, Norm& N) {
    float mx = 0, my = 0;
    for (int i = 0; i < n; i++) { mx += xy[2 * i]; my += xy[2 * i + 1]; }
    mx = mx / n; my = my / n;
    float dx = 0, dy = 0;
    for (int i = 0; i < n; i++) { dx += std::fabs(xy[2 * i] - mx); dy += std::fabs(xy[2 * i + 1] - my); }
    dx = dx / n; dy = dy / n;
    N.mx = mx; N.my = my;
    N.sx = (float)(1.0 / dx); N.sy = (float)(1.0 / dy);
    const float T[9] = {N.sx, 0.f, -mx * N.sx, 0.f, N.sy, -my * N.sy, 0.f, 0.f, 1.f};
    for (int k = 0; k < 9; k++) N.T[k] = T[k];
}
MI_HD void normalised_point(const Norm& N, float x, float y, float& u, float& v) {
    u = (x - N.mx) * N.sx; v = (y - N.my) * N.sy;
}

// ---------------------------------------------------------------- the 8-point systems (ComputeH21 :271-299, ComputeF21 :304-323)
// row pair k of the 16x9 system / row k of the 8x9 system, written into the double workspace W (row-major, 9 columns)
MI_HD void h_rows(double* W, int k, float u1, float v1, float u2, float v2) {
    double* a = W + 18 * k;
    a[0] = 0.0; a[1] = 0.0; a[2] = 0.0; a[3] = -u1; a[4] = -v1; a[5] = -1; a[6] = v2 * u1; a[7] = v2 * v1; a[8] = v2;
    a += 9;
    a[0] = u1; a[1] = v1; a[2] = 1; a[3] = 0.0; a[4] = 0.0; a[5] = 0.0; a[6] = -u2 * u1; a[7] = -u2 * v1; a[8] = -u2;
}
MI_HD void f_row(double* W, int k, float u1, float v1, float u2, float v2) {
    double* a = W + 9 * k;
    a[0] = u2 * u1; a[1] = u2 * v1; a[2] = u2; a[3] = v2 * u1; a[4] = v2 * v1; a[5] = v2; a[6] = u1; a[7] = v1; a[8] = 1;
}

// The right singular vector of the M x 9 system in W for its smallest singular value, in double, under the sign rule.  W holds
// M + 9 rows; rows M .. M + 8 receive V.  One-sided Jacobi (Hestenes): the three sums of a column pair are taken by every caller in row
// order, the rotation is applied to the rows `lane`, `lane + stride`, ...  On the device the callers are the 64 lanes of a one-wave
// workgroup on a workspace in LDS (lane, 64); on the host one caller takes every row (0, 1).  Both give the same numbers.
MI_HD void null_vector9(double* W, int M, int lane, int stride, double x[9]) {
    for (int r = lane; r < 9; r += stride)
        for (int c = 0; c < 9; c++) W[9 * (M + r) + c] = r == c ? 1.0 : 0.0;
    MI_SYNC();
    for (int sweep = 0; sweep < kMaxSweeps; sweep++) {
        int rotated = 0;
        for (int p = 0; p < 8; p++)
            for (int q = p + 1; q < 9; q++) {
                double al = 0, be = 0, ga = 0;
                for (int r = 0; r < M; r++) {
                    const double a = W[9 * r + p], b = W[9 * r + q];
                    al += a * a; be += b * b; ga += a * b;
                }
                const bool rot = ga != 0.0 && fabs(ga) > 1e-16 * sqrt(al * be);
                double cc = 1.0, ss = 0.0;
                if (rot) {
                    const double ze = (be - al) / (2.0 * ga);
                    const double tt = (ze >= 0 ? 1.0 : -1.0) / (fabs(ze) + sqrt(1.0 + ze * ze));
                    cc = 1.0 / sqrt(1.0 + tt * tt); ss = cc * tt;
                    rotated++;
                }
                MI_SYNC();   // every caller has taken its sums before a row changes
                if (rot)
                    for (int r = lane; r < M + 9; r += stride) {
                        const double a = W[9 * r + p], b = W[9 * r + q];
                        W[9 * r + p] = cc * a - ss * b; W[9 * r + q] = ss * a + cc * b;
                    }
                MI_SYNC();
            }
        if (!rotated) break;
    }
    int best = 0;
    double nm = INFINITY;
    for (int c = 0; c < 9; c++) {
        double s = 0;
        for (int r = 0; r < M; r++) s += W[9 * r + c] * W[9 * r + c];
        if (s < nm) { nm = s; best = c; }   // a NaN norm never wins; an all-NaN system gives column 0, which is NaN throughout
    }
    double big = 0;
    bool neg = false;
    for (int r = 0; r < 9; r++) {
        const double v = W[9 * (M + r) + best];
        x[r] = v;
        if (fabs(v) > big) { big = fabs(v); neg = v < 0; }
    }
    if (neg) for (int r = 0; r < 9; r++) x[r] = -x[r];
    MI_SYNC();   // the workspace may be refilled
}

// ---------------------------------------------------------------- 3x3 helpers
MI_HD void mul3(const float* A, const float* B, float* C) {   // cv::Mat * cv::Mat, CV_32F
    MI_UNROLL
    for (int r = 0; r < 3; r++) {
        MI_UNROLL
        for (int c = 0; c < 3; c++)
            C[3 * r + c] = (float)((double)A[3 * r] * (double)B[c] + (double)A[3 * r + 1] * (double)B[3 + c] + (double)A[3 * r + 2] * (double)B[6 + c]);
    }
}
MI_HD void transpose3(const float* A, float* B) {
    B[0] = A[0]; B[1] = A[3]; B[2] = A[6]; B[3] = A[1]; B[4] = A[4]; B[5] = A[7]; B[6] = A[2]; B[7] = A[5]; B[8] = A[8];
}
MI_HD float det3f(const float* m) {   // cv::determinant, 3x3 CV_32F: the cofactor expansion along row 0 in float
    return m[0] * (m[4] * m[8] - m[5] * m[7]) - m[1] * (m[3] * m[8] - m[5] * m[6]) + m[2] * (m[3] * m[7] - m[4] * m[6]);
}
MI_HD void inv3(const float* m, float* o) {   // cv::Mat::inv, 3x3 CV_32F: adjugate over the determinant in double, rounded once; singular: zeros
    const double a = m[0], b = m[1], c = m[2], d = m[3], e = m[4], f = m[5], g = m[6], h = m[7], i = m[8];
    double det = a * (e * i - f * h) - b * (d * i - f * g) + c * (d * h - e * g);
    if (det != 0.0) {
        det = 1.0 / det;
        o[0] = (float)((e * i - f * h) * det); o[1] = (float)((c * h - b * i) * det); o[2] = (float)((b * f - c * e) * det);
        o[3] = (float)((f * g - d * i) * det); o[4] = (float)((a * i - c * g) * det); o[5] = (float)((c * d - a * f) * det);
        o[6] = (float)((d * h - e * g) * det); o[7] = (float)((b * g - a * h) * det); o[8] = (float)((a * e - b * d) * det);
    } else {
        MI_UNROLL
        for (int k = 0; k < 9; k++) o[k] = 0.f;
    }
}

// One rotation of the one-sided Jacobi on the columns p, q of the 3x3 a (and of v); constant indices only, so the arrays stay in registers.
#define MI_ROT3(p, q)                                                                                        \
    {                                                                                                        \
        const double al = a[p] * a[p] + a[3 + p] * a[3 + p] + a[6 + p] * a[6 + p];                           \
        const double be = a[q] * a[q] + a[3 + q] * a[3 + q] + a[6 + q] * a[6 + q];                           \
        const double ga = a[p] * a[q] + a[3 + p] * a[3 + q] + a[6 + p] * a[6 + q];                           \
        const bool rot = ga != 0.0 && fabs(ga) > 1e-16 * sqrt(al * be);                                      \
        const double ze = (be - al) / (2.0 * ga);                                                            \
        double tt = (ze >= 0 ? 1.0 : -1.0) / (fabs(ze) + sqrt(1.0 + ze * ze));                               \
        tt = rot ? tt : 0.0;                                                                                 \
        const double cc = 1.0 / sqrt(1.0 + tt * tt), ss = cc * tt;                                           \
        double h;                                                                                            \
        h = a[p]; a[p] = cc * h - ss * a[q]; a[q] = ss * h + cc * a[q];                                      \
        h = a[3 + p]; a[3 + p] = cc * h - ss * a[3 + q]; a[3 + q] = ss * h + cc * a[3 + q];                  \
        h = a[6 + p]; a[6 + p] = cc * h - ss * a[6 + q]; a[6 + q] = ss * h + cc * a[6 + q];                  \
        h = v[p]; v[p] = cc * h - ss * v[q]; v[q] = ss * h + cc * v[q];                                      \
        h = v[3 + p]; v[3 + p] = cc * h - ss * v[3 + q]; v[3 + q] = ss * h + cc * v[3 + q];                  \
        h = v[6 + p]; v[6 + p] = cc * h - ss * v[6 + q]; v[6 + q] = ss * h + cc * v[6 + q];                  \
    }
#define MI_SWAPCOL(p, q)                                                                                     \
    {                                                                                                        \
        double h;                                                                                            \
        h = w[p]; w[p] = w[q]; w[q] = h;                                                                     \
        h = a[p]; a[p] = a[q]; a[q] = h; h = a[3 + p]; a[3 + p] = a[3 + q]; a[3 + q] = h; h = a[6 + p]; a[6 + p] = a[6 + q]; a[6 + q] = h; \
        h = v[p]; v[p] = v[q]; v[q] = h; h = v[3 + p]; v[3 + p] = v[3 + q]; v[3 + q] = h; h = v[6 + p]; v[6 + p] = v[6 + q]; v[6 + q] = h; \
    }
constexpr int kSweeps3 = 8;   // a 3x3 in double converges in 4 or 5; converged pairs rotate by the identity

// A = U diag(w) V^T of the float 3x3 A in double: w descending, U and V column-wise in row-major 3x3 arrays, under the sign rule.
MI_HD void svd3(const float* A, double* U, double* w, double* V) {
    double a[9], v[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    MI_UNROLL
    for (int k = 0; k < 9; k++) a[k] = A[k];
    MI_UNROLL
    for (int s = 0; s < kSweeps3; s++) { MI_ROT3(0, 1) MI_ROT3(0, 2) MI_ROT3(1, 2) }
    w[0] = sqrt(a[0] * a[0] + a[3] * a[3] + a[6] * a[6]);
    w[1] = sqrt(a[1] * a[1] + a[4] * a[4] + a[7] * a[7]);
    w[2] = sqrt(a[2] * a[2] + a[5] * a[5] + a[8] * a[8]);
    if (w[0] < w[1]) MI_SWAPCOL(0, 1)
    if (w[1] < w[2]) MI_SWAPCOL(1, 2)
    if (w[0] < w[1]) MI_SWAPCOL(0, 1)
    MI_UNROLL
    for (int c = 0; c < 3; c++) {
        double big = fabs(v[c]);
        bool neg = v[c] < 0;
        if (fabs(v[3 + c]) > big) { big = fabs(v[3 + c]); neg = v[3 + c] < 0; }
        if (fabs(v[6 + c]) > big) { big = fabs(v[6 + c]); neg = v[6 + c] < 0; }
        const double sg = neg ? -1.0 : 1.0;
        V[c] = sg * v[c]; V[3 + c] = sg * v[3 + c]; V[6 + c] = sg * v[6 + c];
        const double inv = sg / w[c];
        U[c] = a[c] * inv; U[3 + c] = a[3 + c] * inv; U[6 + c] = a[6 + c] * inv;
    }
    if (!(w[2] > 1e-10 * w[0])) {
        const double dv = V[0] * (V[4] * V[8] - V[5] * V[7]) - V[1] * (V[3] * V[8] - V[5] * V[6]) + V[2] * (V[3] * V[7] - V[4] * V[6]);
        const double sg = dv >= 0 ? 1.0 : -1.0;
        U[2] = sg * (U[3] * U[7] - U[6] * U[4]);
        U[5] = sg * (U[6] * U[1] - U[0] * U[7]);
        U[8] = sg * (U[0] * U[4] - U[3] * U[1]);
    }
}
#undef MI_ROT3
#undef MI_SWAPCOL
// cv::SVD::compute's outputs as the reference reads them: u, w and vt in float
MI_HD void svd3f(const float* A, float* u, float* w, float* vt) {
    double U[9], W[3], V[9];
    svd3(A, U, W, V);
    MI_UNROLL
    for (int k = 0; k < 9; k++) u[k] = (float)U[k];
    MI_UNROLL
    for (int k = 0; k < 3; k++) w[k] = (float)W[k];
    vt[0] = (float)V[0]; vt[1] = (float)V[3]; vt[2] = (float)V[6]; vt[3] = (float)V[1]; vt[4] = (float)V[4]; vt[5] = (float)V[7];
    vt[6] = (float)V[2]; vt[7] = (float)V[5]; vt[8] = (float)V[8];
}

// ---------------------------------------------------------------- from the null vector to the de-normalised model
// FindHomography :226-228: H21 = T2inv * Hn * T1, H12 = H21.inv()
MI_HD void h_model(const double x[9], const float* T1, const float* T2inv, float* H21, float* H12) {
    float Hn[9], t[9];
    MI_UNROLL
    for (int k = 0; k < 9; k++) Hn[k] = (float)x[k];
    mul3(T2inv, Hn, t);
    mul3(t, T1, H21);
    inv3(H21, H12);
}
// ComputeF21 :326-329 (the rank-2 projection), FindFundamental :262: F21 = T2t * Fn * T1
MI_HD void rank2(const float* Fpre, float* Fn) {
    float u[9], w[3], vt[9], ud[9];
    svd3f(Fpre, u, w, vt);
    w[2] = 0;
    const float D[9] = {w[0], 0.f, 0.f, 0.f, w[1], 0.f, 0.f, 0.f, w[2]};
    mul3(u, D, ud);
    mul3(ud, vt, Fn);
}
MI_HD void f_model(const double x[9], const float* T1, const float* T2t, float* F21) {
    float Fpre[9], Fn[9], t[9];
    MI_UNROLL
    for (int k = 0; k < 9; k++) Fpre[k] = (float)x[k];
    rank2(Fpre, Fn);
    mul3(T2t, Fn, t);
    mul3(t, T1, F21);
}

// ---------------------------------------------------------------- per-match bodies of the two scores
// CheckHomography :355-381: the two terms of match (x1, y1) <-> (x2, y2); a rejected term is 0.0f, which leaves a float sum unchanged
MI_HD bool check_h(const float* H21, const float* H12, float inv_sigma2, float x1, float y1, float x2, float y2, float& t1, float& t2) {
    const float th = 5.991;
    bool in = true;
    const float w2in1inv = (float)(1.0 / (H12[6] * x2 + H12[7] * y2 + H12[8]));
    const float u2in1 = (H12[0] * x2 + H12[1] * y2 + H12[2]) * w2in1inv;
    const float v2in1 = (H12[3] * x2 + H12[4] * y2 + H12[5]) * w2in1inv;
    const float sq1 = (x1 - u2in1) * (x1 - u2in1) + (y1 - v2in1) * (y1 - v2in1);
    const float chi1 = sq1 * inv_sigma2;
    if (chi1 > th) { in = false; t1 = 0.f; } else t1 = th - chi1;
    const float w1in2inv = (float)(1.0 / (H21[6] * x1 + H21[7] * y1 + H21[8]));
    const float u1in2 = (H21[0] * x1 + H21[1] * y1 + H21[2]) * w1in2inv;
    const float v1in2 = (H21[3] * x1 + H21[4] * y1 + H21[5]) * w1in2inv;
    const float sq2 = (x2 - u1in2) * (x2 - u1in2) + (y2 - v1in2) * (y2 - v1in2);
    const float chi2 = sq2 * inv_sigma2;
    if (chi2 > th) { in = false; t2 = 0.f; } else t2 = th - chi2;
    return in;
}
// CheckFundamental :400-428
MI_HD bool check_f(const float* F, float inv_sigma2, float x1, float y1, float x2, float y2, float& t1, float& t2) {
    const float th = 3.841, th_score = 5.991;
    bool in = true;
    const float a2 = F[0] * x1 + F[1] * y1 + F[2];
    const float b2 = F[3] * x1 + F[4] * y1 + F[5];
    const float c2 = F[6] * x1 + F[7] * y1 + F[8];
    const float num2 = a2 * x2 + b2 * y2 + c2;
    const float sq1 = num2 * num2 / (a2 * a2 + b2 * b2);
    const float chi1 = sq1 * inv_sigma2;
    if (chi1 > th) { in = false; t1 = 0.f; } else t1 = th_score - chi1;
    const float a1 = F[0] * x2 + F[3] * y2 + F[6];
    const float b1 = F[1] * x2 + F[4] * y2 + F[7];
    const float c1 = F[2] * x2 + F[5] * y2 + F[8];
    const float num1 = a1 * x1 + b1 * y1 + c1;
    const float sq2 = num1 * num1 / (a1 * a1 + b1 * b1);
    const float chi2 = sq2 * inv_sigma2;
    if (chi2 > th) { in = false; t2 = 0.f; } else t2 = th_score - chi2;
    return in;
}
MI_HD float inv_sigma_square(float sigma) { return (float)(1.0 / (sigma * sigma)); }

// ---------------------------------------------------------------- the (R, t) candidates
struct Candidates { float R[8][9]; float t[8][3]; int n; };   // n = 0: ReconstructH's early exit

MI_HD void unit3(const float* v, float* o) {   // v / cv::norm(v)
    const float s = (float)(1.0 / sqrt((double)v[0] * v[0] + (double)v[1] * v[1] + (double)v[2] * v[2]));
    o[0] = v[0] * s; o[1] = v[1] * s; o[2] = v[2] * s;
}
MI_HD void k_of(const float* intr4, float* K) {
    K[0] = intr4[0]; K[1] = 0.f; K[2] = intr4[2]; K[3] = 0.f; K[4] = intr4[1]; K[5] = intr4[3]; K[6] = 0.f; K[7] = 0.f; K[8] = 1.f;
}
// ReconstructF :436-440 with DecomposeE :735-748: (R1, t), (R2, t), (R1, -t), (R2, -t)
MI_HD void decompose_f(const float* F21, const float* intr4, Candidates& C) {
    float K[9], Kt[9], tmp[9], E[9], u[9], w[3], vt[9], t[3], R1[9], R2[9];
    k_of(intr4, K);
    transpose3(K, Kt);
    mul3(Kt, F21, tmp);
    mul3(tmp, K, E);
    svd3f(E, u, w, vt);
    const float u2[3] = {u[2], u[5], u[8]};
    unit3(u2, t);
    const float W[9] = {0.f, -1.f, 0.f, 1.f, 0.f, 0.f, 0.f, 0.f, 1.f}, Wt[9] = {0.f, 1.f, 0.f, -1.f, 0.f, 0.f, 0.f, 0.f, 1.f};
    mul3(u, W, tmp);
    mul3(tmp, vt, R1);
    if (det3f(R1) < 0) { MI_UNROLL for (int k = 0; k < 9; k++) R1[k] = -R1[k]; }
    mul3(u, Wt, tmp);
    mul3(tmp, vt, R2);
    if (det3f(R2) < 0) { MI_UNROLL for (int k = 0; k < 9; k++) R2[k] = -R2[k]; }
    C.n = 4;
    MI_UNROLL
    for (int k = 0; k < 9; k++) { C.R[0][k] = R1[k]; C.R[1][k] = R2[k]; C.R[2][k] = R1[k]; C.R[3][k] = R2[k]; }
    MI_UNROLL
    for (int k = 0; k < 3; k++) { C.t[0][k] = t[k]; C.t[1][k] = t[k]; C.t[2][k] = -t[k]; C.t[3][k] = -t[k]; }
}
// one of Faugeras' eight: R = s * U * Rp * Vt, t = U * tp / |U * tp|
MI_HD void h_candidate(float s, const float* U, const float* Vt, const float* Rp, const float* tp, float* R, float* t) {
    float m[9], ut[3];
    MI_UNROLL
    for (int r = 0; r < 3; r++) {
        MI_UNROLL
        for (int c = 0; c < 3; c++)
            m[3 * r + c] = (float)((double)s * ((double)U[3 * r] * (double)Rp[c] + (double)U[3 * r + 1] * (double)Rp[3 + c] + (double)U[3 * r + 2] * (double)Rp[6 + c]));
    }
    mul3(m, Vt, R);
    MI_UNROLL
    for (int r = 0; r < 3; r++) ut[r] = (float)((double)U[3 * r] * (double)tp[0] + (double)U[3 * r + 1] * (double)tp[1] + (double)U[3 * r + 2] * (double)tp[2]);
    unit3(ut, t);
}
// ReconstructH :503-587.  d3 receives the singular values (diagnostics); C.n = 0 on the early exit.
MI_HD void decompose_h(const float* H21, const float* intr4, Candidates& C, float* d3) {
    float K[9], invK[9], tmp[9], A[9], U[9], w[3], Vt[9];
    k_of(intr4, K);
    inv3(K, invK);
    mul3(invK, H21, tmp);
    mul3(tmp, K, A);
    svd3f(A, U, w, Vt);
    const float s = (float)((double)det3f(U) * (double)det3f(Vt));
    const float d1 = w[0], d2 = w[1], d3_ = w[2];
    d3[0] = d1; d3[1] = d2; d3[2] = d3_;
    C.n = 0;
    if (d1 / d2 < 1.00001 || d2 / d3_ < 1.00001) return;
    C.n = 8;
    const float aux1 = sqrtf((d1 * d1 - d2 * d2) / (d1 * d1 - d3_ * d3_));
    const float aux3 = sqrtf((d2 * d2 - d3_ * d3_) / (d1 * d1 - d3_ * d3_));
    const float x1[4] = {aux1, aux1, -aux1, -aux1}, x3[4] = {aux3, -aux3, aux3, -aux3};
    const float aux_stheta = sqrtf((d1 * d1 - d2 * d2) * (d2 * d2 - d3_ * d3_)) / ((d1 + d3_) * d2);
    const float ctheta = (d2 * d2 + d1 * d3_) / ((d1 + d3_) * d2);
    const float stheta[4] = {aux_stheta, -aux_stheta, -aux_stheta, aux_stheta};
    MI_UNROLL
    for (int i = 0; i < 4; i++) {
        const float Rp[9] = {ctheta, 0.f, -stheta[i], 0.f, 1.f, 0.f, stheta[i], 0.f, ctheta};
        const float sc = d1 - d3_;
        const float tp[3] = {x1[i] * sc, 0.f * sc, -x3[i] * sc};
        h_candidate(s, U, Vt, Rp, tp, C.R[i], C.t[i]);
    }
    const float aux_sphi = sqrtf((d1 * d1 - d2 * d2) * (d2 * d2 - d3_ * d3_)) / ((d1 - d3_) * d2);
    const float cphi = (d1 * d3_ - d2 * d2) / ((d1 - d3_) * d2);
    const float sphi[4] = {aux_sphi, -aux_sphi, -aux_sphi, aux_sphi};
    MI_UNROLL
    for (int i = 0; i < 4; i++) {
        const float Rp[9] = {cphi, 0.f, sphi[i], 0.f, -1.f, 0.f, sphi[i], 0.f, -cphi};
        const float sc = d1 + d3_;
        const float tp[3] = {x1[i] * sc, 0.f * sc, x3[i] * sc};
        h_candidate(s, U, Vt, Rp, tp, C.R[4 + i], C.t[4 + i]);
    }
}

// ---------------------------------------------------------------- CheckRT :672-734
struct RtConst { float fx, fy, cx, cy; float R[9], t[3]; float P2[12]; float O2[3]; float th2; };
MI_HD void make_rt_const(const float* intr4, const float* R, const float* t, float th2, RtConst& Q) {
    Q.fx = intr4[0]; Q.fy = intr4[1]; Q.cx = intr4[2]; Q.cy = intr4[3]; Q.th2 = th2;
    float K[9];
    k_of(intr4, K);
    MI_UNROLL
    for (int k = 0; k < 9; k++) Q.R[k] = R[k];
    MI_UNROLL
    for (int k = 0; k < 3; k++) Q.t[k] = t[k];
    MI_UNROLL
    for (int r = 0; r < 3; r++) {   // P2 = K * [R | t]
        MI_UNROLL
        for (int c = 0; c < 4; c++) {
            const double b0 = c < 3 ? R[c] : t[0], b1 = c < 3 ? R[3 + c] : t[1], b2 = c < 3 ? R[6 + c] : t[2];
            Q.P2[4 * r + c] = (float)((double)K[3 * r] * b0 + (double)K[3 * r + 1] * b1 + (double)K[3 * r + 2] * b2);
        }
    }
    MI_UNROLL
    for (int r = 0; r < 3; r++)   // O2 = -R.t() * t
        Q.O2[r] = (float)(-1.0 * ((double)R[r] * (double)t[0] + (double)R[3 + r] * (double)t[1] + (double)R[6 + r] * (double)t[2]));
}
// one inlier match: its state, the cosine of its parallax and its point (camera 1's frame); p is written for every state but kNonFinite
MI_HD uint8_t check_rt(const RtConst& Q, float x1, float y1, float x2, float y2, float& cosp, float* p) {
    float A[16];   // Triangulate :623-627 with P1 = [K | 0]
    A[0] = x1 * 0.0f - Q.fx; A[1] = x1 * 0.0f - 0.0f; A[2] = x1 * 1.0f - Q.cx; A[3] = x1 * 0.0f - 0.0f;
    A[4] = y1 * 0.0f - 0.0f; A[5] = y1 * 0.0f - Q.fy; A[6] = y1 * 1.0f - Q.cy; A[7] = y1 * 0.0f - 0.0f;
    A[8] = x2 * Q.P2[8] - Q.P2[0];  A[9] = x2 * Q.P2[9] - Q.P2[1];  A[10] = x2 * Q.P2[10] - Q.P2[2]; A[11] = x2 * Q.P2[11] - Q.P2[3];
    A[12] = y2 * Q.P2[8] - Q.P2[4]; A[13] = y2 * Q.P2[9] - Q.P2[5]; A[14] = y2 * Q.P2[10] - Q.P2[6]; A[15] = y2 * Q.P2[11] - Q.P2[7];
    double nv[4];
    npm::null_vector(A, npm::kJacobiSweeps, nv);
    const float v0 = (float)nv[0], v1 = (float)nv[1], v2 = (float)nv[2], v3 = (float)nv[3];
    const float iw = (float)(1.0 / (double)v3);   // :631 x3D.rowRange(0, 3) / x3D.at<float>(3)
    const float X = v0 * iw, Y = v1 * iw, Z = v2 * iw;
    cosp = 0.f; p[0] = X; p[1] = Y; p[2] = Z;
    if (!std::isfinite(X) || !std::isfinite(Y) || !std::isfinite(Z)) return kNonFinite;
    const float n2x = X - Q.O2[0], n2y = Y - Q.O2[1], n2z = Z - Q.O2[2];
    const float dist1 = npm::norm3_as_float(X, Y, Z), dist2 = npm::norm3_as_float(n2x, n2y, n2z);
    cosp = (float)(((double)X * n2x + (double)Y * n2y + (double)Z * n2z) / (double)(dist1 * dist2));
    if (Z <= 0 && cosp < 0.99998) return kRejected;
    const float X2 = (float)((double)Q.R[0] * X + (double)Q.R[1] * Y + (double)Q.R[2] * Z + (double)Q.t[0]);
    const float Y2 = (float)((double)Q.R[3] * X + (double)Q.R[4] * Y + (double)Q.R[5] * Z + (double)Q.t[1]);
    const float Z2 = (float)((double)Q.R[6] * X + (double)Q.R[7] * Y + (double)Q.R[8] * Z + (double)Q.t[2]);
    if (Z2 <= 0 && cosp < 0.99998) return kRejected;
    const float invZ1 = (float)(1.0 / Z);
    const float im1x = Q.fx * X * invZ1 + Q.cx, im1y = Q.fy * Y * invZ1 + Q.cy;
    const float e1 = (im1x - x1) * (im1x - x1) + (im1y - y1) * (im1y - y1);
    if (e1 > Q.th2) return kRejected;
    const float invZ2 = (float)(1.0 / Z2);
    const float im2x = Q.fx * X2 * invZ2 + Q.cx, im2y = Q.fy * Y2 * invZ2 + Q.cy;
    const float e2 = (im2x - x2) * (im2x - x2) + (im2y - y2) * (im2y - y2);
    if (e2 > Q.th2) return kRejected;
    return cosp < 0.99998 ? kCountedGood : kCountedLowParallax;
}
// the order of floats as unsigned keys (the selection of the order statistic works on these)
MI_HD uint32_t float_key(float f) {
    uint32_t u;
    __builtin_memcpy(&u, &f, 4);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
MI_HD float key_float(uint32_t k) {
    const uint32_t u = (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k;
    float f;
    __builtin_memcpy(&f, &u, 4);
    return f;
}
MI_HD float parallax_of(float cosine) { return (float)(acos((double)cosine) * 180 / 3.1415926535897932384626433832795); }

// ---------------------------------------------------------------- the decisions
// RH = SH / (SH + SF); > 0.40 chooses the homography (:190-193)
MI_HD int choose_model(float sh, float sf, float& rh) {
    rh = sh / (sh + sf);
    return rh > 0.40 ? kHomography : kFundamental;
}
// ReconstructF :448-496 / ReconstructH :588-620 on the candidates' counts and parallaxes: the winner's index, and whether it is accepted
MI_HD bool decide(int model, int n_cand, int N, const int* n_good, const float* parallax, float min_parallax, int min_triangulated, int& winner) {
    winner = -1;
    if (model == kFundamental) {
        const int g1 = n_good[0], g2 = n_good[1], g3 = n_good[2], g4 = n_good[3];
        int mx = g3 > g4 ? g3 : g4;
        mx = g2 > mx ? g2 : mx;
        mx = g1 > mx ? g1 : mx;
        const int i09 = (int)(0.9 * N);
        const int n_min_good = i09 > min_triangulated ? i09 : min_triangulated;
        int similar = 0;
        if (g1 > 0.7 * mx) similar++;
        if (g2 > 0.7 * mx) similar++;
        if (g3 > 0.7 * mx) similar++;
        if (g4 > 0.7 * mx) similar++;
        winner = mx == g1 ? 0 : (mx == g2 ? 1 : (mx == g3 ? 2 : 3));
        if (mx < n_min_good || similar > 1) return false;
        return parallax[winner] > min_parallax;
    }
    if (n_cand == 0) return false;
    int best = 0, second = 0;
    float best_parallax = -1;
    for (int i = 0; i < 8; i++) {
        if (n_good[i] > best) { second = best; best = n_good[i]; winner = i; best_parallax = parallax[i]; }
        else if (n_good[i] > second) second = n_good[i];
    }
    return second < 0.75 * best && best_parallax >= min_parallax && best > min_triangulated && best > 0.9 * N;
}

}  // namespace mim
