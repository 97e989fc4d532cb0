// Host build of csrc/p3p_math.hpp (the arithmetic of pnp_ransac.hip, one text for device and host): lets a CPU test compare the
// kernel's three-point solver, its pick, its float matrix and its inlier test with the numpy oracle, and gives the timing script its
// one-core comparison point.  g++ -O2 -ffp-contract=off -shared -fPIC.
#include "../../ucoslam-cv3_amd/csrc/p3p_math.hpp"

extern "C" {

// P: 4 x 3, px: 4 x 2.  Rt_4x12: per solution R row-major then t.  Returns the number of solutions; chosen = -1: skipped.
int p3p_host_hypothesis(const float* intr4, const float* P, const float* px, double* Rt_4x12, int* chosen, float* rt6, double* rvec_tvec6) {
    p3p::Pose sol[4];
    int c;
    const int n = p3p::hypothesis(intr4, P, px, sol, c, rt6);
    for (int k = 0; k < n; k++) {
        const p3p::Pose& T = sol[k];
        const double v[12] = {T.r00, T.r01, T.r02, T.r10, T.r11, T.r12, T.r20, T.r21, T.r22, T.tx, T.ty, T.tz};
        for (int i = 0; i < 12; i++) Rt_4x12[12 * k + i] = v[i];
    }
    if (c >= 0 && rvec_tvec6) {
        p3p::rodrigues(sol[c], rvec_tvec6[0], rvec_tvec6[1], rvec_tvec6[2]);
        rvec_tvec6[3] = sol[c].tx; rvec_tvec6[4] = sol[c].ty; rvec_tvec6[5] = sol[c].tz;
    }
    *chosen = c;
    return n;
}

// the quartic's real roots from its coefficients A[0..4] (A[i] of v^i) alone: r[4] ascending, the absent ones +inf; returns their number
int p3p_host_roots(const double* A, double* r) {
    p3p::Setup S{};
    S.ok = true;
    S.A0 = A[0]; S.A1 = A[1]; S.A2 = A[2]; S.A3 = A[3]; S.A4 = A[4];
    return p3p::roots(S, r[0], r[1], r[2], r[3]);
}

// Which branches roots() takes on the quartic A5 = A0..A4, from the same expressions: form[0] = 1 it is solved in 1 / v, form[1] = 1 the
// resolvent cubic takes its trigonometric form (0: Cardano), form[2] = 1 the biquadratic branch.  Returns 0 when nothing is solved.
int p3p_host_roots_form(const double* A5, int* form) {
    const bool rev = p3p::reversed_form(A5[0], A5[1], A5[2], A5[3], A5[4]);
    const double a4 = rev ? A5[0] : A5[4], a3 = rev ? A5[1] : A5[3], a2 = A5[2], a1 = rev ? A5[3] : A5[1], a0 = rev ? A5[4] : A5[0];
    form[0] = rev; form[1] = form[2] = 0;
    if (!(std::fabs(a4) > 0.0)) return 0;
    const double B = a3 / a4, Cc = a2 / a4, Dd = a1 / a4, E = a0 / a4;
    const double B2 = B * B;
    const double p = Cc - 0.375 * B2, q = Dd - 0.5 * B * Cc + 0.125 * B2 * B;
    const double r = E - 0.25 * B * Dd + 0.0625 * B2 * Cc - (3.0 / 256.0) * B2 * B2;
    const double c2 = p, c1 = 0.25 * p * p - r, c0 = -0.125 * q * q;
    const double Q = (c2 * c2 - 3.0 * c1) / 9.0, R = (2.0 * c2 * c2 * c2 - 9.0 * c2 * c1 + 27.0 * c0) / 54.0;
    form[1] = R * R < Q * Q * Q;
    const double m = p3p::cubic_largest_root(c2, c1, c0);
    form[2] = !(m > 1e-14 * (std::fabs(p) + std::sqrt(std::fabs(r)) + 1e-300));
    return 1;
}

// the same for one hypothesis; A5: its coefficients.  Returns 0 for a degenerate sample.
int p3p_host_form(const float* intr4, const float* P, const float* px, int* form, double* A5) {
    p3p::Setup S;
    p3p::setup(intr4, P, px, S);
    A5[0] = S.A0; A5[1] = S.A1; A5[2] = S.A2; A5[3] = S.A3; A5[4] = S.A4;
    return p3p_host_roots_form(A5, form) && S.ok;
}

void p3p_host_se3(const float* rt6, float* m12) {
    p3p::M34 M;
    p3p::se3_set(rt6, M);
    const float v[12] = {M.m0, M.m1, M.m2, M.m3, M.m4, M.m5, M.m6, M.m7, M.m8, M.m9, M.m10, M.m11};
    for (int i = 0; i < 12; i++) m12[i] = v[i];
}

void p3p_host_rodrigues(const double* R9, double* r3) {
    p3p::Pose T{R9[0], R9[1], R9[2], R9[3], R9[4], R9[5], R9[6], R9[7], R9[8], 0, 0, 0};
    p3p::rodrigues(T, r3[0], r3[1], r3[2]);
}

// the inlier test of one pose over n matches; returns the count
int p3p_host_score(const float* intr4, const float* rt6, int n, const float* p3d, const float* normal, const float* kp, unsigned char* mask, float* err2, float* vc) {
    p3p::M34 M;
    p3p::se3_set(rt6, M);
    float c0, c1, c2;
    p3p::cam_center(M, c0, c1, c2);
    int cnt = 0;
    for (int j = 0; j < n; j++) {
        float e, c;
        const bool in = p3p::inlier(M, intr4[0], intr4[1], intr4[2], intr4[3], c0, c1, c2, p3d[3 * j], p3d[3 * j + 1], p3d[3 * j + 2], normal[3 * j],
                                    normal[3 * j + 1], normal[3 * j + 2], kp[2 * j], kp[2 * j + 1], e, c);
        if (mask) mask[j] = in;
        if (err2) err2[j] = e;
        if (vc) vc[j] = c;
        cnt += in;
    }
    return cnt;
}

// the whole loop of pnpsolver.cpp:62-106 on one thread (counts: iters entries, -1 = skipped); returns the best iteration or -1
int p3p_host_ransac(const float* intr4, int n, const float* p3d, const float* normal, const float* kp, int iters, const int* samples, int* counts, float* rt6_best) {
    int best = -1, best_cnt = 0;
    for (int it = 0; it < iters; it++) {
        float P[12], px[8], rt6[6];
        for (int k = 0; k < 4; k++) {
            const int i = samples[4 * it + k];
            for (int c = 0; c < 3; c++) P[3 * k + c] = p3d[3 * i + c];
            px[2 * k] = kp[2 * i]; px[2 * k + 1] = kp[2 * i + 1];
        }
        p3p::Pose sol[4];
        int chosen;
        p3p::hypothesis(intr4, P, px, sol, chosen, rt6);
        if (chosen < 0) { counts[it] = -1; continue; }
        const int cnt = p3p_host_score(intr4, rt6, n, p3d, normal, kp, nullptr, nullptr, nullptr);
        counts[it] = cnt;
        if (cnt > best_cnt) { best_cnt = cnt; best = it; for (int c = 0; c < 6; c++) rt6_best[c] = rt6[c]; }
    }
    return best;
}

}
