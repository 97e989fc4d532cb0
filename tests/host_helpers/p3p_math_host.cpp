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
