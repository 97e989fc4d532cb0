// TEST INFRASTRUCTURE ONLY — CPU oracle for the per-frame pose-only optimisation (PnPSolver::solvePnp, mono, no markers).
// Only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg may use this file.
//
// Restates  src/optimization/pnpsolver.cpp:116-409  (4 rounds x optimize(10) restarting from the input pose, chi2 > 5.99
//           reclassification after every round, robust kernels dropped from the third round on, early exit below 10 inliers),
//           src/optimization/typesg2o.h:590-650     EdgeSE3ProjectXYZOnlyPose (error, analytic 2x6 Jacobian),
//           src/optimization/typesg2o.h:82-105      WeightedHubberRobustKernel (the weight scales rho only),
//           3rdparty/g2o: BaseUnaryEdge::constructQuadraticForm (base_unary_edge.hpp:55-78), Levenberg (as ba_oracle.cpp),
//           SparseOptimizer::optimize(iterations, minChi2BetweenIter = 0)  (sparse_optimizer.h:120).
// Pinned against the real g2o (oracle/_ref/libg2o_ref.so, driver g2o_ref_pnp_solve) by tests/test_pnp.py.
// oracle_pnp_solve_stereo adds  typesg2o.h:521-588  EdgeStereoSE3ProjectXYZOnlyPose (cam_project rounds 1/z to float, the Jacobian uses
// the double 1/z) for matches with depth > 0, built as pnpsolver.cpp:205-276 does (kp_ur = x - mbf / depth in float, weight doubled,
// Huber sqrt(7.815), relabelling at 7.815); pinned against tests/golden/pnp_stereo_golden.npz (real g2o) by tests/test_track_oracle.py.
// oracle_pnp_trace is oracle_pnp_solve_stereo with a record of the control flow (OraclePnpTrace below) and one test hook; the arithmetic
// is that of the other entries.  Pinned against tests/golden/pnp_hard_golden.npz (real g2o, rarely taken branches) by tests/test_pnp_hard.py.
#include <cmath>
#include <cstdint>
#include <cstring>
#include <limits>
#include <vector>

// What oracle_pnp_trace reports, per round r and outer iteration i at [10 * r + i] (tests/oracle_lib.py mirrors the layout).
struct OraclePnpTrace {
    int32_t trials[40];         // Levenberg trials the iteration took (g2o: G2OBatchStatistics::levenbergIterations)
    int32_t accepted[40];       // the number of the trial that was accepted, counted from 1 (always the iteration's last), or -1
    int32_t fails[40];          // trials whose 6x6 factorisation failed
    int32_t lam_nonfinite[40];  // 1: lambda went non-finite and the loop was left before its increment
    int32_t reason[40];         // why nothing followed the iteration, bits: 1 ten trials, 2 rho == 0, 4 non-finite lambda (Levenberg's
                                // Terminate), 8 the float chi2 did not decrease, 16 the budget of ten iterations is spent; 0: another follows
    double w2_applied[40];      // max |omega|^2 over the steps the iteration applied (accepted or not)
    double w2_accepted[40];     // |omega|^2 of the accepted step, 0 without one
};

namespace {

struct Pose { double q[4]; double t[3]; };

void quat_norm_pos(double* q) {
    if (q[3] < 0) for (int i = 0; i < 4; i++) q[i] = -q[i];
    const double n = std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    for (int i = 0; i < 4; i++) q[i] /= n;
}
void quat_from_R(const double R[9], double* q) {
    double t = R[0] + R[4] + R[8];
    if (t > 0) { t = std::sqrt(t + 1.0); q[3] = 0.5 * t; t = 0.5 / t; q[0] = (R[7] - R[5]) * t; q[1] = (R[2] - R[6]) * t; q[2] = (R[3] - R[1]) * t; }
    else {
        int i = 0; if (R[4] > R[0]) i = 1; if (R[8] > R[i * 4]) i = 2;
        const int j = (i + 1) % 3, k = (j + 1) % 3;
        t = std::sqrt(R[i * 4] - R[j * 4] - R[k * 4] + 1.0); q[i] = 0.5 * t; t = 0.5 / t;
        q[3] = (R[k * 3 + j] - R[j * 3 + k]) * t; q[j] = (R[j * 3 + i] + R[i * 3 + j]) * t; q[k] = (R[k * 3 + i] + R[i * 3 + k]) * t;
    }
}
void quat_to_R(const double* q, double R[9]) {
    const double tx = 2 * q[0], ty = 2 * q[1], tz = 2 * q[2];
    const double twx = tx * q[3], twy = ty * q[3], twz = tz * q[3], txx = tx * q[0], txy = ty * q[0], txz = tz * q[0];
    const double tyy = ty * q[1], tyz = tz * q[1], tzz = tz * q[2];
    R[0] = 1 - (tyy + tzz); R[1] = txy - twz; R[2] = txz + twy; R[3] = txy + twz; R[4] = 1 - (txx + tzz); R[5] = tyz - twx;
    R[6] = txz - twy; R[7] = tyz + twx; R[8] = 1 - (txx + tyy);
}
// small_angle_only (test hook of oracle_pnp_trace): the constants of the theta < 1e-5 branch at every theta >= 0.5 as well
void pose_oplus(Pose& T, const double d[6], bool small_angle_only = false) {   // T <- exp(d) * T, se3quat.h:276-311
    const double w[3] = {d[0], d[1], d[2]}, u[3] = {d[3], d[4], d[5]};
    const double theta = std::sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
    const double O[9] = {0, -w[2], w[1], w[2], 0, -w[0], -w[1], w[0], 0};
    double O2[9];
    for (int r = 0; r < 3; r++) for (int c = 0; c < 3; c++) O2[r * 3 + c] = O[r * 3] * O[c] + O[r * 3 + 1] * O[3 + c] + O[r * 3 + 2] * O[6 + c];
    double a, b, c1, c2;
    if (theta < 0.00001 || (small_angle_only && theta >= 0.5)) { a = 1; b = 0.5; c1 = 0.5; c2 = 1.0 / 6.0; }
    else { a = std::sin(theta) / theta; b = (1 - std::cos(theta)) / (theta * theta); c1 = b; c2 = (theta - std::sin(theta)) / std::pow(theta, 3); }
    double R[9], V[9];
    for (int i = 0; i < 9; i++) { const double I = (i % 4 == 0) ? 1.0 : 0.0; R[i] = I + a * O[i] + b * O2[i]; V[i] = I + c1 * O[i] + c2 * O2[i]; }
    Pose E;
    quat_from_R(R, E.q);
    quat_norm_pos(E.q);
    for (int r = 0; r < 3; r++) E.t[r] = V[r * 3] * u[0] + V[r * 3 + 1] * u[1] + V[r * 3 + 2] * u[2];
    double RE[9];
    quat_to_R(E.q, RE);
    const double* x = E.q; const double* y = T.q;
    double q[4] = {x[3] * y[0] + x[0] * y[3] + x[1] * y[2] - x[2] * y[1], x[3] * y[1] + x[1] * y[3] + x[2] * y[0] - x[0] * y[2],
                   x[3] * y[2] + x[2] * y[3] + x[0] * y[1] - x[1] * y[0], x[3] * y[3] - x[0] * y[0] - x[1] * y[1] - x[2] * y[2]};
    double t[3];
    for (int r = 0; r < 3; r++) t[r] = RE[r * 3] * T.t[0] + RE[r * 3 + 1] * T.t[1] + RE[r * 3 + 2] * T.t[2] + E.t[r];
    std::memcpy(T.q, q, sizeof(q));
    std::memcpy(T.t, t, sizeof(t));
    quat_norm_pos(T.q);
}

struct PnP {
    int n;
    const float* p3d; const float* kp; const float* invsig; const float* weight;
    double fx, fy, cx, cy, delta;
    // stereo form: per edge 0 = monocular, 1 = stereo; its measured right x (kp_ur), bf = mbf, the 3-D Huber width and its doubled weights
    std::vector<char> st;
    std::vector<float> ur, w3;
    double bf = 0, delta3 = 0;
    Pose T;
    std::vector<char> active, robust;
    std::vector<double> err, chi2;
    double H[36], b[6], x[6] = {0, 0, 0, 0, 0, 0}, lambda = -1, ni = 2;   // (g2o's solution vector starts as zeros, solver.cpp:57)
    OraclePnpTrace* tr = nullptr;   // oracle_pnp_trace only
    int tr_at = 0;                  // 10 * round + iteration
    bool small_angle_only = false;  // test hook, see pose_oplus

    void edge_error(int e, const double R[9], double& ex, double& ey, double pc[3]) const {
        const float* X = p3d + 3 * e;
        for (int r = 0; r < 3; r++) pc[r] = R[r * 3] * X[0] + R[r * 3 + 1] * X[1] + R[r * 3 + 2] * X[2] + T.t[r];
        ex = kp[2 * e] - ((pc[0] / pc[2]) * fx + cx);
        ey = kp[2 * e + 1] - ((pc[1] / pc[2]) * fy + cy);
    }
    // EdgeStereoSE3ProjectXYZOnlyPose::computeError: obs - cam_project(pc), invz = (float)(1 / z)
    void edge_error3(int e, const double R[9], double* ev, double pc[3]) const {
        const float* X = p3d + 3 * e;
        for (int r = 0; r < 3; r++) pc[r] = R[r * 3] * X[0] + R[r * 3 + 1] * X[1] + R[r * 3 + 2] * X[2] + T.t[r];
        const float invz = 1.0f / pc[2];
        const double u = pc[0] * invz * fx + cx, v = pc[1] * invz * fy + cy;
        ev[0] = kp[2 * e] - u;
        ev[1] = kp[2 * e + 1] - v;
        ev[2] = ur[e] - (u - bf * invz);
    }
    bool stereo(int e) const { return !st.empty() && st[e]; }
    double& chi2_of(int e, const double R[9]) {   // the edge's error and chi2 at rotation R (information = invsigma * I)
        double pc[3];
        double* ev = &err[3 * e];
        if (stereo(e)) {
            edge_error3(e, R, ev, pc);
            chi2[e] = (double)invsig[e] * (ev[0] * ev[0] + ev[1] * ev[1] + ev[2] * ev[2]);
        } else {
            edge_error(e, R, ev[0], ev[1], pc);
            chi2[e] = (double)invsig[e] * (ev[0] * ev[0] + ev[1] * ev[1]);
        }
        return chi2[e];
    }
    void compute_errors() {
        double R[9]; quat_to_R(T.q, R);
        for (int e = 0; e < n; e++) {
            if (!active[e]) continue;
            chi2_of(e, R);
        }
    }
    double robust_chi2() const {
        double s = 0;
        for (int e = 0; e < n; e++) {
            if (!active[e]) continue;
            const double c = chi2[e];
            const double d = stereo(e) ? delta3 : delta, dsqr = d * d, w = stereo(e) ? (double)w3[e] : (double)weight[e];
            if (robust[e]) s += (c <= dsqr) ? w * c : w * (2 * std::sqrt(c) * d - dsqr);
            else s += c;
        }
        return s;
    }
    void build() {
        std::memset(H, 0, sizeof(H)); std::memset(b, 0, sizeof(b));
        double R[9]; quat_to_R(T.q, R);
        for (int e = 0; e < n; e++) {
            if (!active[e]) continue;
            const bool s3 = stereo(e);
            const double d = s3 ? delta3 : delta, dsqr = d * d;
            double pc[3], ev[3];
            if (s3) edge_error3(e, R, ev, pc);
            else edge_error(e, R, ev[0], ev[1], pc);
            const double X = pc[0], Y = pc[1], invz = 1.0 / pc[2], invz2 = invz * invz;
            double J[18] = {X * Y * invz2 * fx, -(1 + (X * X * invz2)) * fx, Y * invz * fx, -invz * fx, 0, X * invz2 * fx,
                                  (1 + Y * Y * invz2) * fy, -X * Y * invz2 * fy, -X * invz * fy, 0, -invz * fy, Y * invz2 * fy,
                                  0, 0, 0, 0, 0, 0};
            double* J2 = J + 12;
            if (s3) {   // typesg2o.h: the third row
                J2[0] = J[0] - bf * Y * invz2; J2[1] = J[1] + bf * X * invz2; J2[2] = J[2]; J2[3] = J[3]; J2[4] = 0; J2[5] = J[5] - bf * invz2;
            }
            const double w = invsig[e];
            double rho1 = 1.0;
            if (robust[e] && chi2[e] > dsqr) rho1 = d / std::sqrt(chi2[e]);
            for (int a = 0; a < 6; a++) {
                if (s3) {
                    b[a] -= rho1 * (J[a] * w * ev[0] + J[6 + a] * w * ev[1] + J2[a] * w * ev[2]);
                    for (int c = 0; c < 6; c++) H[a * 6 + c] += (rho1 * w) * (J[a] * J[c] + J[6 + a] * J[6 + c] + J2[a] * J2[c]);
                } else {
                    b[a] -= rho1 * (J[a] * w * ev[0] + J[6 + a] * w * ev[1]);
                    for (int c = 0; c < 6; c++) H[a * 6 + c] += (rho1 * w) * (J[a] * J[c] + J[6 + a] * J[6 + c]);
                }
            }
        }
    }
    // 6x6 LDL^T.  Fails as Eigen's SimplicialLDLT does (g2o's LinearSolverEigen): on a pivot that is exactly zero, and on nothing else — a
    // non-finite pivot goes through and leaves a non-finite step.  x is left as it was on failure (so is g2o's solution vector).
    bool solve(double lam) {
        double M[36], L[36] = {0}, d[6];
        for (int i = 0; i < 36; i++) M[i] = H[i] + ((i % 7 == 0) ? lam : 0.0);
        for (int j = 0; j < 6; j++) {
            double dj = M[j * 6 + j];
            for (int k = 0; k < j; k++) dj -= L[j * 6 + k] * L[j * 6 + k] * d[k];
            d[j] = dj;
            if (dj == 0.0) return false;
            for (int i = j + 1; i < 6; i++) { double v = M[i * 6 + j]; for (int k = 0; k < j; k++) v -= L[i * 6 + k] * L[j * 6 + k] * d[k]; L[i * 6 + j] = v / dj; }
        }
        for (int i = 0; i < 6; i++) { double v = b[i]; for (int k = 0; k < i; k++) v -= L[i * 6 + k] * x[k]; x[i] = v; }
        for (int i = 0; i < 6; i++) x[i] /= d[i];
        for (int i = 5; i >= 0; i--) { double v = x[i]; for (int k = i + 1; k < 6; k++) v -= L[k * 6 + i] * x[k]; x[i] = v; }
        return true;
    }
    bool lm_solve(int iteration) {   // true = OK, false = Terminate
        compute_errors();
        double currentChi = robust_chi2(), tempChi = currentChi;
        build();
        if (iteration == 0) { double m = 0; for (int j = 0; j < 6; j++) m = std::max(std::fabs(H[j * 7]), m); lambda = 1e-5 * m; ni = 2; }
        double rho = 0;
        int qmax = 0;
        do {
            const Pose bak = T;
            const bool ok2 = solve(lambda);
            // (also after a failed factorisation, with the step left over: optimization_algorithm_levenberg.cpp:104-109.  pnp.hip evaluates
            // the unchanged pose there instead: the same up to rounding while the step left over is zero, as it is when the first factorisation
            // of a round fails — a zero pivot after an accepted step has not been seen)
            pose_oplus(T, x, small_angle_only);
            const double w2 = x[0] * x[0] + x[1] * x[1] + x[2] * x[2];
            if (tr) {
                tr->trials[tr_at]++;
                if (!ok2) tr->fails[tr_at]++;
                else if (w2 > tr->w2_applied[tr_at]) tr->w2_applied[tr_at] = w2;
            }
            compute_errors();
            tempChi = robust_chi2();
            if (!ok2) tempChi = std::numeric_limits<double>::max();
            rho = currentChi - tempChi;
            double scale = 0;
            for (int i = 0; i < 6; i++) scale += x[i] * (lambda * x[i] + b[i]);
            scale += 1e-3;
            rho /= scale;
            if (rho > 0 && std::isfinite(tempChi)) {
                double alpha = 1. - std::pow((2 * rho - 1), 3);
                alpha = std::min(alpha, 2. / 3.);
                lambda *= std::max(1. / 3., alpha);
                ni = 2;
                currentChi = tempChi;
                if (tr) { tr->accepted[tr_at] = qmax + 1; tr->w2_accepted[tr_at] = w2; }
            } else {
                lambda *= ni; ni *= 2; T = bak;
                if (!std::isfinite(lambda)) { if (tr) tr->lam_nonfinite[tr_at] = 1; break; }
            }
            qmax++;
        } while (rho < 0 && qmax < 10);
        if (tr) tr->reason[tr_at] = (qmax == 10 ? 1 : 0) | (rho == 0 ? 2 : 0) | (!std::isfinite(lambda) ? 4 : 0);
        return !(qmax == 10 || rho == 0 || !std::isfinite(lambda));
    }
    int optimize(int iterations, int round) {
        float prev = std::numeric_limits<float>::max(), cur = prev, diff = prev;
        bool ok = true;
        int done = 0;
        for (int i = 0; i < iterations && ok && diff > 0.f; i++) {
            std::swap(prev, cur);
            tr_at = 10 * round + i;
            ok = lm_solve(i);
            cur = (float)robust_chi2();
            diff = prev - cur;
            ++done;
            if (tr) tr->reason[tr_at] |= (!(diff > 0.f) ? 8 : 0) | (i + 1 >= iterations ? 16 : 0);
        }
        return done;
    }
};

}  // namespace

// the loop of PnPSolver::solvePnp (pnpsolver.cpp:116-409) over the prepared edges
static int pnp_run(PnP& s, const float* pose_f2g, int n, float* pose_out, uint8_t* bad_out, int32_t* iters_out, double* state_out) {
    const double R0[9] = {pose_f2g[0], pose_f2g[1], pose_f2g[2], pose_f2g[4], pose_f2g[5], pose_f2g[6], pose_f2g[8], pose_f2g[9], pose_f2g[10]};
    Pose T0;
    quat_from_R(R0, T0.q);
    quat_norm_pos(T0.q);
    T0.t[0] = pose_f2g[3]; T0.t[1] = pose_f2g[7]; T0.t[2] = pose_f2g[11];
    s.T = T0;
    s.active.assign(n, 1); s.robust.assign(n, 1); s.err.assign(3 * (size_t)n, 0.0); s.chi2.assign(n, 0.0);
    std::vector<char> bad(n, 0);
    for (int it = 0; it < 4; it++) iters_out[it] = 0;
    const float Chi2D = 5.99f, Chi3D = 7.815f;
    if (n > 0)
        for (int it = 0; it < 4; it++) {
            s.T = T0;                                   // every round restarts from the input pose (:354)
            iters_out[it] = s.optimize(10, it);
            int nGood = 0;
            double R[9]; quat_to_R(s.T.q, R);
            for (int e = 0; e < n; e++) {
                if (bad[e]) s.chi2_of(e, R);            // excluded edges get a fresh error at the new pose (:364)
                bad[e] = s.chi2[e] > (double)(s.stereo(e) ? Chi3D : Chi2D);
                s.active[e] = !bad[e];
                if (it >= 2) s.robust[e] = 0;
                if (!bad[e]) nGood++;
            }
            if (nGood < 10) break;
        }
    double R[9]; quat_to_R(s.T.q, R);
    for (int r = 0; r < 3; r++) { for (int c = 0; c < 3; c++) pose_out[r * 4 + c] = (float)R[r * 3 + c]; pose_out[r * 4 + 3] = (float)s.T.t[r]; }
    pose_out[12] = pose_out[13] = pose_out[14] = 0.f; pose_out[15] = 1.f;
    int good = 0;
    for (int e = 0; e < n; e++) { bad_out[e] = bad[e]; good += !bad[e]; }
    if (state_out) { std::memcpy(state_out, s.T.q, 32); std::memcpy(state_out + 4, s.T.t, 24); }
    return good;
}

extern "C" int oracle_pnp_solve(const float* pose_f2g, const float* intr4, int n, const float* p3d, const float* kp, const float* invsigma,
                                const float* weight, float* pose_out, uint8_t* bad_out, int32_t* iters_out /*4*/, double* state_out /*7*/) {
    PnP s;
    s.n = n; s.p3d = p3d; s.kp = kp; s.invsig = invsigma; s.weight = weight;
    s.fx = intr4[0]; s.fy = intr4[1]; s.cx = intr4[2]; s.cy = intr4[3];
    s.delta = (double)(float)std::sqrt(5.99);   // const float thHuber2D = sqrt(5.99)
    return pnp_run(s, pose_f2g, n, pose_out, bad_out, iters_out, state_out);
}

// the edges of oracle_pnp_solve_stereo: depth NULL or <= 0 = the monocular edge
static void pnp_prepare(PnP& s, const float* intr4, int n, const float* p3d, const float* kp, const float* invsigma, const float* weight,
                        const float* depth, float bl) {
    s.n = n; s.p3d = p3d; s.kp = kp; s.invsig = invsigma; s.weight = weight;
    s.fx = intr4[0]; s.fy = intr4[1]; s.cx = intr4[2]; s.cy = intr4[3];
    s.delta = (double)(float)std::sqrt(5.99);    // thHuber2D
    s.delta3 = (double)(float)std::sqrt(7.815);  // thHuber3D
    if (depth) {
        const float mbf = bl * intr4[0];
        s.bf = mbf;
        s.st.assign(n, 0); s.ur.assign(n, 0.f); s.w3.assign(n, 0.f);
        for (int e = 0; e < n; e++) {
            if (!(depth[e] > 0)) continue;        // pnpsolver.cpp:205: depth <= 0 -> monocular edge
            s.st[e] = 1;
            s.ur[e] = kp[2 * e] - mbf / depth[e];  // kp_ur (float)
            float w = weight[e];
            w *= 2;                               // the stereo edge's robust weight is doubled
            s.w3[e] = w;
        }
    }
}

// depth: n floats (Frame::getDepth(queryIdx); <= 0 = monocular edge) or NULL (= oracle_pnp_solve); bl = imageParams.bl
extern "C" int oracle_pnp_solve_stereo(const float* pose_f2g, const float* intr4, int n, const float* p3d, const float* kp, const float* invsigma,
                                       const float* weight, const float* depth, float bl, float* pose_out, uint8_t* bad_out,
                                       int32_t* iters_out /*4*/, double* state_out /*7*/) {
    PnP s;
    pnp_prepare(s, intr4, n, p3d, kp, invsigma, weight, depth, bl);
    return pnp_run(s, pose_f2g, n, pose_out, bad_out, iters_out, state_out);
}

// oracle_pnp_solve_stereo with its control flow recorded in *trace (zeroed here; accepted = -1 where no trial was accepted).
// small_angle_only != 0 is a test hook: SE3's exp keeps its small-angle constants at |omega| >= 0.5, i.e. the step of a solver whose
// large-rotation branch is wrong (tests/test_pnp_hard.py looks at what of the fixture such a solver misses).
extern "C" int oracle_pnp_trace(const float* pose_f2g, const float* intr4, int n, const float* p3d, const float* kp, const float* invsigma,
                                const float* weight, const float* depth, float bl, int small_angle_only, float* pose_out, uint8_t* bad_out,
                                int32_t* iters_out /*4*/, double* state_out /*7*/, OraclePnpTrace* trace) {
    PnP s;
    std::memset(trace, 0, sizeof(*trace));
    for (int i = 0; i < 40; i++) trace->accepted[i] = -1;
    s.tr = trace;
    s.small_angle_only = small_angle_only != 0;
    pnp_prepare(s, intr4, n, p3d, kp, invsigma, weight, depth, bl);
    return pnp_run(s, pose_f2g, n, pose_out, bad_out, iters_out, state_out);
}
