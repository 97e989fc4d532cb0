// Per-frame pose-only optimisation on MI355X (gfx950), fp64, behind the C ABI (uh_pnp_*).
//
// Semantic contract = PnPSolver::solvePnp (reference file:line):
//   src/optimization/pnpsolver.cpp:116-409  four rounds; each restarts from the INPUT pose (:354), runs optimize(10)
//                                           (minChi2BetweenIter = 0), reclassifies every match with chi2 above its limit as outlier
//                                           (excluded edges get a fresh error first, :364), drops the robust kernels from the
//                                           third round on (:368) and stops early below 10 inliers (:379)
//   3rdparty/g2o                            Levenberg loop, lambda init/update, SE3 exp — as in ba.hip
//   src/optimization/typesg2o.h:82-105      WeightedHubberRobustKernel: the weight scales rho (the chi2 sums), not the Jacobian
// and its three edge types, one template parameter each where they cost anything:
//   typesg2o.h:590-650   EdgeSE3ProjectXYZOnlyPose        two rows, limit 5.99: every match without a depth               (project)
//   typesg2o.h:521-590   EdgeStereoSE3ProjectXYZOnlyPose  three rows, limit 7.815, kernel weight doubled: a match with a
//                        depth (pnpsolver.cpp:239-276), STEREO instantiations only                                        (project_st)
//   typesg2o.h:414-471   MarkerEdgeOnlyProject            eight rows per marker, g2o's numeric Jacobian (base_binary_edge.hpp:165-233),
//                        pnpsolver.cpp:280-386, MARKERS instantiations only, see "markers" below                          (marker_err)
// A match goes through ONE evaluation whatever its type: `edge` (project or project_st) and `robust` (the one `huber` with the edge type's
// weight and threshold) are what the classification, the accumulation and the damping ladder all call; `to_camera` is the transform of all
// three edge types; `rt_from_pose16` makes the input pose and the markers' poses.  An instantiation without stereo holds st == false as a
// constant: the three-row branch is not in its code.
//
// MI355X design: one 6x6 system over a few hundred to a few thousand matches, ~20 dependent Levenberg trials — pure latency, so
// the WHOLE solve runs inside ONE workgroup of one launch and every trial costs ONE pass over the matches and ONE barrier:
//   * a pass evaluates a pose: per match the error, chi2, robust weight AND the Jacobian products, i.e. the trial's chi2 and the
//     normal equations of the NEXT linearisation come out of the same pass (g2o re-linearises at the pose it has just accepted and
//     gets exactly these numbers; after a rejection H and b of the old pose are still valid) — one pass per trial instead of two;
//     the classification between two rounds is folded into the first pass of the next round;
//   * the 29 sums (21 + 6 + chi2 + inlier count) go through one butterfly-transpose reduction per wave, one LDS exchange and one
//     barrier (double-buffered by pass parity); every wave then adds the eight partials in wave order and holds the totals as
//     wave-uniform values;
//   * every wave solves the 6x6 system, applies the SE3 update and takes the accept / reject decision REDUNDANTLY from those
//     identical totals: no wave waits for another one between two passes, no single-thread section, no second barrier;
//   * the matches live in LDS for the whole solve (37 bytes each, n <= kPnpLdsMatches; larger n runs the same code on HBM arrays);
//   * host form: the inputs are read straight from a pinned, device-visible staging block, the results go straight into pinned
//     memory behind a completion word the host polls — one launch, no copy engine, no stream synchronisation.
#include <algorithm>
#include <cfloat>
#include <chrono>
#include <cmath>

#include "common.hpp"
#include "reduce.hpp"
#include "se3.hpp"

namespace {

struct PnpArgs {
    const float* pose_in;    // 16
    const float* intr;       // fx fy cx cy
    int n;
    const int* n_dev;        // NULL, or the match count in device memory (written by an earlier launch of the stream; n is then its upper bound)
    const float* p3d; const float* kp; const float* invsig; const float* weight;
    void* work;              // n x 32 bytes of scratch (only used when the matches do not fit LDS)
    float* pose_out;         // 16
    unsigned char* bad_out;  // n
    int* result;             // [0] inliers, [1..4] outer iterations per round
    double* state_out;       // 7 or NULL
    unsigned long long* host_done;   // NULL, or a word in pinned host memory that receives done_word after everything else
    unsigned long long done_word;
    long long* clk;          // NULL, or 8 timestamps (s_memtime) for scripts/time_pnp.py
    uh::PnpDecide dec;       // dyn17 != NULL: the tracker's decision rides on this solve (common.hpp)
    // stereo instantiation only (kept behind the monocular fields: those instantiations read the same offsets as before)
    const float* depth;      // n: Frame::getDepth(queryIdx), <= 0 = monocular match
    float bl;                // imageParams.bl (stereo baseline)
    // marker instantiations only
    int n_mk;                // 1..kPnpMaxMarkers
    const float* mk_pose;    // n_mk x 16: Marker::pose_g2m
    const float* mk_size;    // n_mk: Marker::size
    const float* mk_corners; // n_mk x 8: MarkerObservation::und_corners
};

// one thread: the decision of system.cpp:6646 / :6813 from this solve's inlier count (tracked iff MORE than min_inliers); M = the pose it
// returns (16 floats)
__device__ void pnp_decide(const PnpArgs& A, int inliers, const float* M) {
    const int tracked = inliers > A.dec.min_inliers ? 1 : 0;
    const float* T = tracked ? M : A.pose_in;
    float* d = A.dec.dyn17;
    for (int i = 0; i < 12; i++) d[i] = T[i];
    // camCenter = pose_f2g.inv() * (0,0,0), se3transform.h:89-113 — the float expressions of projmatch.hip's match_enqueue
    const float m0 = T[0], m1 = T[4], m2 = T[8], m4 = T[1], m5 = T[5], m6 = T[9], m8 = T[2], m9 = T[6], m10 = T[10];
    const float m3 = -(T[3] * m0 + T[7] * m1 + T[11] * m2), m7 = -(T[3] * m4 + T[7] * m5 + T[11] * m6), m11 = -(T[3] * m8 + T[7] * m9 + T[11] * m10);
    d[12] = m0 * 0.f + m1 * 0.f + m2 * 0.f + m3;
    d[13] = m4 * 0.f + m5 * 0.f + m6 * 0.f + m7;
    d[14] = m8 * 0.f + m9 * 0.f + m10 * 0.f + m11;
    d[15] = tracked ? A.dec.r_tracked : A.dec.r_lost;
    d[16] = 0.f;
    for (int i = 0; i < 16; i++) A.dec.pose_map[i] = T[i];
    *A.dec.tracked = tracked;
}

// row-major float[16] -> Rt[12] (R row-major, then t) as g2o::SE3Quat(R, t) holds it: the rotation is the one of the NORMALISED quaternion.
// (q, t and Rt as one local object that is copied out: written so, both callers compile to the code they had with the steps written out)
__device__ __forceinline__ void rt_from_pose16(const float* M, double* Rt) {
    struct { double q[4], t[3], Rt[12]; } P;
    const double R0[9] = {M[0], M[1], M[2], M[4], M[5], M[6], M[8], M[9], M[10]};
    quat_from_R(R0, P.q);
    quat_norm_pos(P.q);
    P.t[0] = M[3]; P.t[1] = M[7]; P.t[2] = M[11];
    quat_to_R(P.q, P.Rt);
    P.Rt[9] = P.t[0]; P.Rt[10] = P.t[1]; P.Rt[11] = P.t[2];
#pragma unroll
    for (int i = 0; i < 12; i++) Rt[i] = P.Rt[i];
}
// the camera-frame point of X under Rt
__device__ __forceinline__ void to_camera(const double* Rt, double X0, double X1, double X2, double& p0, double& p1, double& p2) {
    p0 = fma(Rt[2], X2, fma(Rt[1], X1, fma(Rt[0], X0, Rt[9])));
    p1 = fma(Rt[5], X2, fma(Rt[4], X1, fma(Rt[3], X0, Rt[10])));
    p2 = fma(Rt[8], X2, fma(Rt[7], X1, fma(Rt[6], X0, Rt[11])));
}
// ---- fp64 primitives of the serial path: v_rcp_f64 / v_rsq_f64 + two Newton steps (<= 1 ulp) instead of the IEEE division /
// square-root expansions (a dozen instructions each, on a path where every instruction is latency)
__device__ __forceinline__ double rcp_nr(double x) {
    double r = __builtin_amdgcn_rcp(x);
    r = fma(r, fma(-x, r, 1.0), r);
    r = fma(r, fma(-x, r, 1.0), r);
    return r;
}
__device__ __forceinline__ double rsq_nr(double x) {   // x > 0
    double y = __builtin_amdgcn_rsq(x);
    const double h = 0.5 * x;
    y = fma(y, fma(-h * y, y, 0.5), y);
    y = fma(y, fma(-h * y, y, 0.5), y);
    return y;
}

// Hu = the 21 upper-triangle entries row by row (H[a][c], a <= c, at index tri(a, c))
__device__ __forceinline__ constexpr int tri(int a, int c) { return a * 6 - a * (a - 1) / 2 + (c - a); }
__device__ __forceinline__ bool p_solve6(const double* Hu, const double* b, double lam, double* x) {   // LDL^T, fails on a zero pivot
    // Right-looking (every pivot's column updates the trailing block at once) with the right-hand side carried along, then a
    // column-oriented back substitution: the dependent chain per pivot is reciprocal -> scale -> one fma instead of a dot product
    // of growing length — this routine sits on the serial path of every trial.  Fully unrolled, compile-time indices: the system
    // stays in registers.  x is left alone on failure.  Only a pivot that is exactly zero is a failure, as in Eigen's SimplicialLDLT behind
    // g2o's LinearSolverEigen: a non-finite pivot goes through and leaves a non-finite step, the trial is evaluated at a non-finite pose and
    // every edge keeps a non-finite chi2 (no match is relabelled from it: a comparison with NaN is false).
    double a[6][6], L[6][6], id[6], y[6];
#pragma unroll
    for (int i = 0; i < 6; i++) {
        y[i] = b[i];
#pragma unroll
        for (int j = 0; j <= i; j++) a[i][j] = Hu[tri(j, i)] + (i == j ? lam : 0.0);
    }
    bool ok = true;
#pragma unroll
    for (int j = 0; j < 6; j++) {
        const double dj = a[j][j];
        ok = ok && !(dj == 0.0);
        id[j] = rcp_nr(dj);
#pragma unroll
        for (int i = j + 1; i < 6; i++) L[i][j] = a[i][j] * id[j];
#pragma unroll
        for (int k = j + 1; k < 6; k++)
#pragma unroll
            for (int i = k; i < 6; i++) a[i][k] = fma(-L[i][j], a[k][j], a[i][k]);
#pragma unroll
        for (int i = j + 1; i < 6; i++) y[i] = fma(-L[i][j], y[j], y[i]);
    }
    if (!ok) return false;
#pragma unroll
    for (int i = 0; i < 6; i++) y[i] *= id[i];
#pragma unroll
    for (int j = 5; j >= 0; j--) {
#pragma unroll
        for (int i = 0; i < j; i++) y[i] = fma(-L[j][i], y[j], y[i]);
    }
#pragma unroll
    for (int i = 0; i < 6; i++) x[i] = y[i];
    return true;
}

// T <- exp(d) * T on the 3x4 matrix (g2o: SE3Quat::exp(update) * estimate, se3quat.h:276-311 — the same Rodrigues / V matrices; g2o
// goes through a unit quaternion after every product, which changes the result by rounding only).  For |w| < 0.5 the three
// coefficients sin(t)/t, (1 - cos t)/t^2, (t - sin t)/t^3 come from their power series in t^2 (nine terms: truncation < 1e-19):
// no square root, no division, no sincos on the path of every trial.
__device__ __forceinline__ void p_oplus_rt(double (&Rt)[12], const double* d) {
    const double w0 = d[0], w1 = d[1], w2 = d[2];
    const double z = w0 * w0 + w1 * w1 + w2 * w2;   // theta^2
    double a, b, c2;
    if (z < 1e-10) { a = 1; b = 0.5; c2 = 1.0 / 6.0; }      // theta < 0.00001 (se3quat.h:290)
    else if (z < 0.25) {
        // 1/(2k+1)!, 1/(2k+2)!, 1/(2k+3)! with alternating signs, Horner in z
        a = 1.0 / 355687428096000.0; b = 1.0 / 6402373705728000.0; c2 = 1.0 / 121645100408832000.0;
        a = fma(a, z, -1.0 / 1307674368000.0); b = fma(b, z, -1.0 / 20922789888000.0); c2 = fma(c2, z, -1.0 / 355687428096000.0);
        a = fma(a, z, 1.0 / 6227020800.0);     b = fma(b, z, 1.0 / 87178291200.0);     c2 = fma(c2, z, 1.0 / 1307674368000.0);
        a = fma(a, z, -1.0 / 39916800.0);      b = fma(b, z, -1.0 / 479001600.0);      c2 = fma(c2, z, -1.0 / 6227020800.0);
        a = fma(a, z, 1.0 / 362880.0);         b = fma(b, z, 1.0 / 3628800.0);         c2 = fma(c2, z, 1.0 / 39916800.0);
        a = fma(a, z, -1.0 / 5040.0);          b = fma(b, z, -1.0 / 40320.0);          c2 = fma(c2, z, -1.0 / 362880.0);
        a = fma(a, z, 1.0 / 120.0);            b = fma(b, z, 1.0 / 720.0);             c2 = fma(c2, z, 1.0 / 5040.0);
        a = fma(a, z, -1.0 / 6.0);             b = fma(b, z, -1.0 / 24.0);             c2 = fma(c2, z, -1.0 / 120.0);
        a = fma(a, z, 1.0);                    b = fma(b, z, 0.5);                     c2 = fma(c2, z, 1.0 / 6.0);
    } else {
        const double theta = sqrt(z);
        double sn, cs;
        sincos(theta, &sn, &cs);
        a = sn / theta; b = (1 - cs) / z; c2 = (theta - sn) / (z * theta);
    }
    // O = [w]x, O2 = O*O = w w^T - z I;  Rm = I + a O + b O2,  V = I + b O + c2 O2
    const double O[9] = {0, -w2, w1, w2, 0, -w0, -w1, w0, 0};
    const double O2[9] = {w0 * w0 - z, w0 * w1, w0 * w2, w0 * w1, w1 * w1 - z, w1 * w2, w0 * w2, w1 * w2, w2 * w2 - z};
    double Rm[9], V[9];
#pragma unroll
    for (int i = 0; i < 9; i++) {
        const double I = (i % 4 == 0) ? 1.0 : 0.0;
        Rm[i] = fma(b, O2[i], fma(a, O[i], I));
        V[i] = fma(c2, O2[i], fma(b, O[i], I));
    }
    double n[12];
#pragma unroll
    for (int r = 0; r < 3; r++) {
#pragma unroll
        for (int c = 0; c < 3; c++) n[r * 3 + c] = fma(Rm[r * 3 + 2], Rt[6 + c], fma(Rm[r * 3 + 1], Rt[3 + c], Rm[r * 3] * Rt[c]));
        const double rt = fma(Rm[r * 3 + 2], Rt[11], fma(Rm[r * 3 + 1], Rt[10], Rm[r * 3] * Rt[9]));
        const double vu = fma(V[r * 3 + 2], d[5], fma(V[r * 3 + 1], d[4], V[r * 3] * d[3]));
        n[9 + r] = rt + vu;
    }
#pragma unroll
    for (int i = 0; i < 12; i++) Rt[i] = n[i];
}

// The matches live in LDS for the whole solve as 32-byte records {X, Y, Z, u, v, 1/sigma, weight, flags} (n <= kPnpLdsMatches:
// 96 KB): a pass reads a match with two ds_read_b128.  Larger n runs the same code on records packed into the caller's scratch.
constexpr int kPnpLdsMatches = 3000;
// 8 waves = two per SIMD of the one CU this kernel lives on: the per-match fp64 chains of one wave fill the issue gaps of the other.
// Wave 0 owns the Levenberg state and is alone on its SIMD during the serial steps (the other waves wait at the barrier).
constexpr int kPnpThreads = 512, kPnpWaves = kPnpThreads / 64;
constexpr int kNS = 29;               // sums per pass: H (21), b (6), robust chi2, inlier count
constexpr unsigned kActive = 1, kRobust = 2, kBad = 4, kStereo = 8;
enum : int { kModeEval = 0, kModeClassify = 1, kModeExit = 2, kModeLadder = 3 };
constexpr int kLadderMax = 8;         // candidates per ladder pass (one per wave; Levenberg's inner loop tries at most ten damping factors per iteration)

struct __attribute__((aligned(16))) MatchRec { float X, Y, Z, u, v, invsig, weight; unsigned flags; };
static_assert(sizeof(MatchRec) == 32, "match record");
// STEREO: the records are followed by one float per match, the right-image measurement kp_ur (pnpsolver.cpp:245-246; 0 for a monocular
// match); kStereo in flags selects EdgeStereoSE3ProjectXYZOnlyPose for the match.  36 bytes per match: 3000 matches = 105.5 KiB of LDS.
constexpr int kPnpRecBytesStereo = 36;

// ---- markers (pnpsolver.cpp:280-386, typesg2o.h:414-471).  The marker vertex is fixed, so a marker is four points of the global frame
// (g2m applied to the corners (-+s/2, +-s/2, 0), s a float) and their measured, undistorted image positions.  The edge's error rounds
// every projected coordinate to FLOAT and has no analytic Jacobian: g2o differentiates it numerically, col d = (e(+delta e_d) -
// e(-delta e_d)) / (2 delta) with delta = (double)(float)1e-4 on those float-quantised errors — the quantisation is part of the
// behaviour and is reproduced: 13 pose evaluations (the pose itself and exp(+-delta e_d) * pose) x 4 corners per marker and pass.
// exp(+-delta e_d) * T maps a camera-frame point c of T to R_d(+-delta) c (rotations, SE3Quat::exp's sin / (1 - cos) expressions) or
// c +- delta e_d (translations), so the perturbed points are formed from the unperturbed one.
constexpr int kPnpMaxMarkers = UH_PNP_MAX_MARKERS;
// J, e, rho1, rc: the edge's linearisation at the pose a pass evaluates (numeric Jacobian, errors, the kernel's rho[1] and rho[0]), parked
// here by the marker's wave, which then forms the marker's share of the sums from it (marker_linearise)
struct __attribute__((aligned(8))) MarkerRec { double P[4][3]; float uv[8]; int robust, pad; double J[8][6], e[8], rho1, rc; };
// the marker instantiations' dynamic LDS: [match records of the LDS form | kPnpMaxMarkers marker records | weight_marker | per wave: its
// markers' share of the 28 sums of a pass]
constexpr size_t kPnpMarkerLds = kPnpMaxMarkers * sizeof(MarkerRec) + sizeof(double) + 8 * 32 * sizeof(double);
__host__ __device__ constexpr size_t pnp_marker_offset(int n, bool stereo) {
    return (((size_t)(n > 1 ? n : 1) * (stereo ? kPnpRecBytesStereo : 32) + 15) / 16) * 16;
}

template <bool CACHED, bool STEREO = false, bool MARKERS = false>
__global__ __launch_bounds__(kPnpThreads) void pnp_solve_kernel(PnpArgs A) {
    extern __shared__ __attribute__((aligned(16))) unsigned char s_cache[];
    __shared__ __attribute__((aligned(16))) double s_part[kPnpWaves * 32];
    __shared__ __attribute__((aligned(16))) double s_tot[32];
    __shared__ __attribute__((aligned(16))) double s_pose[4][12];   // [0] pose to evaluate + accumulate, [1] pose of the excluded matches' fresh chi2 (end of the last
                                                                    // round), [2] pose the kept chi2 belong to (the last one evaluated), [3] the input pose
    __shared__ __attribute__((aligned(16))) double s_H[28];         // the normal equations of the current pose (21 + 6): wave 0's, parked here between solves
    __shared__ __attribute__((aligned(16))) double s_T[12], s_x[8]; // wave 0's: the current (last accepted) pose and the last solved step
    __shared__ int s_ctl[4];                                        // mode, classify, drop_robust, ladder length
    __shared__ __attribute__((aligned(16))) double s_lad[2];        // ladder request: lambda and ni of its first candidate
    __shared__ __attribute__((aligned(16))) double s_cand[kLadderMax][20];   // per candidate: trial pose (12), step (6), factorisation ok (1)
    const int tid = threadIdx.x, lane = tid & 63;
    int n = A.n;
    if (A.n_dev) {   // (uh_track_pose: the matches were chosen on the device)
        const int nd = __builtin_amdgcn_readfirstlane(*A.n_dev);
        n = nd < n ? nd : n;
        // pnpsolver.cpp:149-150: without matches the pose comes back as it went in.  The tracker's first solve (dec.dyn17) runs only with
        // MORE than min_inliers matches (system.cpp:6595); otherwise the reference tries its FrameMatcher fallback, which is the caller's:
        // taken to find nothing, nInliers = 0 and no solve is reported (pose in, no iterations, no outlier flags)
        // (with markers a solve without matches runs, pnpsolver.cpp:148-158; the tracker's rule for its first solve stays)
        if ((!MARKERS && n <= 0) || (A.dec.dyn17 && n <= A.dec.min_inliers)) {
            if (tid < 16) A.pose_out[tid] = A.pose_in[tid];
            if (tid < 5) A.result[tid] = 0;
            for (int e = tid; e < n; e += kPnpThreads) A.bad_out[e] = 0;
            if (A.dec.dyn17 && tid == 0) pnp_decide(A, 0, A.pose_in);
            return;
        }
    }
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);        // wave index as a scalar: the role split below is an s_cbranch
    if (A.clk && tid == 0) A.clk[0] = __builtin_readcyclecounter();
    const double fx = A.intr[0], fy = A.intr[1], cx = A.intr[2], cy = A.intr[3];
    const double delta = (double)sqrtf(5.99f), dsqr = delta * delta;
    // stereo edges (pnpsolver.cpp:175-181, 248-274): thHuber3D = (float)sqrt(7.815), relabelled above Chi3D = 7.815f, bf = mbf as a double
    double delta3 = 0, dsqr3 = 0, bf = 0;
    if constexpr (STEREO) { delta3 = (double)(float)sqrt(7.815); dsqr3 = delta3 * delta3; bf = (double)(A.bl * A.intr[0]); }
    // one name for both instantiations; in each the pointer has a single provenance (LDS or HBM): ds_* or global_* accesses, never flat
    MatchRec* rec;
    if constexpr (CACHED) rec = reinterpret_cast<MatchRec*>(s_cache);
    else rec = reinterpret_cast<MatchRec*>(A.work);
    float* urs = nullptr;   // STEREO: kp_ur per match, behind the n records
    if constexpr (STEREO) urs = reinterpret_cast<float*>(rec + n);
    for (int e = tid; e < n; e += kPnpThreads) {
        MatchRec r;
        r.X = A.p3d[3 * e]; r.Y = A.p3d[3 * e + 1]; r.Z = A.p3d[3 * e + 2]; r.u = A.kp[2 * e]; r.v = A.kp[2 * e + 1];
        r.invsig = A.invsig[e]; r.weight = A.weight[e]; r.flags = kActive | kRobust;
        if constexpr (STEREO) {
            // pnpsolver.cpp:239-246: depth <= 0 keeps the monocular edge; else mbf = bl * fx and kp_ur = x - mbf / depth, all float
            // (a correctly rounded float division: the build does not use fast math)
            const float depth = A.depth[e];
            float ur = 0.f;
            if (!(depth <= 0.f)) {
                const float mbf = A.bl * A.intr[0];
                ur = r.u - mbf / depth;
                r.flags |= kStereo;
            }
            urs[e] = ur;
        }
        rec[e] = r;
    }
    {
        double Rt0[12];
        rt_from_pose16(A.pose_in, Rt0);
        if (tid == 0) {
#pragma unroll
            for (int i = 0; i < 12; i++) { s_pose[3][i] = Rt0[i]; s_pose[1][i] = Rt0[i]; s_pose[2][i] = Rt0[i]; }
        }
    }
    // markers: the records, and weight_marker of pnpsolver.cpp:305-310 in its mixed float / double arithmetic — KpWeightSum is the
    // double sum of the per-match kernel weights after the stereo doubling (block_sum's fixed pairing instead of the reference's
    // match order: the same bits whenever the partial sums are exact, as they are for the weights 0.5 / 1 / 2); +inf without matches
    // (in the dynamic LDS behind the A.n match records the launch sized it for — nothing is added to the marker-free instantiations)
    const int nmk = MARKERS ? A.n_mk : 0;
    MarkerRec* s_mk = reinterpret_cast<MarkerRec*>(s_cache + (CACHED ? pnp_marker_offset(A.n, STEREO) : 0));
    double* s_mkw = reinterpret_cast<double*>(s_mk + kPnpMaxMarkers);
    double* s_mkpart = s_mkw + 1;
    // marker i belongs to wave 7 - i % 8: wave 0, whose serial steps every pass waits for, is the last to get one
    const int mk_first = kPnpWaves - 1 - wv;
    if constexpr (MARKERS) {
        double ws = 0;
        for (int e = tid; e < n; e += kPnpThreads) {   // (this thread's own records: no second trip to the caller's arrays)
            float w = rec[e].weight;
            if constexpr (STEREO) { if (rec[e].flags & kStereo) w *= 2.f; }
            ws += (double)w;
        }
        ws = block_sum<kPnpWaves>(ws, s_part);
        if (tid == 0) *s_mkw = ((double)(0.3f * (float)(n + nmk)) / (1. - (double)0.3f)) / (double)(float)ws;
        if (tid < nmk) {
            double G[12];   // Marker::pose_g2m
            rt_from_pose16(A.mk_pose + 16 * tid, G);
            const float sz = A.mk_size[tid];
            const double hi = (double)(float)((double)sz / 2.), lo = (double)(float)(-(double)sz / 2.);   // Marker::get3DPointsLocalRefSystem: cv::Point3f
            const double px[4] = {lo, hi, hi, lo}, py[4] = {hi, hi, lo, lo};
            MarkerRec& r = s_mk[tid];
#pragma unroll
            for (int c = 0; c < 4; c++)
#pragma unroll
                for (int a = 0; a < 3; a++) r.P[c][a] = fma(G[3 * a + 1], py[c], fma(G[3 * a], px[c], G[9 + a]));
#pragma unroll
            for (int i = 0; i < 8; i++) r.uv[i] = A.mk_corners[8 * tid + i];
            r.robust = 1; r.pad = 0;
        }
    }
    __syncthreads();
    if (A.clk && tid == 0) A.clk[1] = __builtin_readcyclecounter();
    // the marker edge's kernel: thHuber8D = (float)sqrt(15.507), relabelled against Chi8D = 15.507f
    constexpr double delta8 = 0x1.f80cep+1, dsqr8 = delta8 * delta8;      // (double)(float)sqrt(15.507) = 3.9378929138183594
    constexpr double mk_delta = (double)1e-4f, mk_scalar = 1 / (2 * mk_delta);
    // SE3Quat::exp for omega = delta e_d (theta = delta >= 1e-5): R = I + sin(theta)/theta Omega + (1 - cos(theta))/theta^2 Omega^2, i.e. the
    // entries (sin(delta) / delta) * delta and 1 - ((1 - cos(delta)) / delta^2) * delta^2 in double, as constants (wave-uniform values
    // computed at run time would sit in vector registers for the whole solve)
    constexpr double mk_sin = 0x1.a36e2df44599cp-14, mk_cos = 0x1.ffffffd50ce26p-1;
    // the error of corner c of a marker at the pose Rt perturbed by pattern k: 0 = not, 1..6 = +delta along dimension k - 1, 7..12 =
    // -delta along dimension k - 7.  Projections rounded to float (typesg2o.h:461-465)
    auto marker_err = [&](const MarkerRec& m, int c, int k, const double* Rt, double& ex, double& ey) {
        double p0, p1, p2;
        to_camera(Rt, m.P[c][0], m.P[c][1], m.P[c][2], p0, p1, p2);
        if (k > 0) {
            const double sg = k > 6 ? -1.0 : 1.0;
            const int d = k > 6 ? k - 7 : k - 1;
            if (d < 3) {   // rotation about axis d: (u, v, w) = the components (d, d + 1, d + 2) cyclically
                const double v = d == 0 ? p1 : d == 1 ? p2 : p0, w = d == 0 ? p2 : d == 1 ? p0 : p1;
                const double s = sg * mk_sin;
                const double v2 = mk_cos * v - s * w, w2 = s * v + mk_cos * w;
                if (d == 0) { p1 = v2; p2 = w2; } else if (d == 1) { p2 = v2; p0 = w2; } else { p0 = v2; p1 = w2; }
            } else {
                const double t = sg * mk_delta;
                if (d == 3) p0 += t; else if (d == 4) p1 += t; else p2 += t;
            }
        }
        const double projx = (double)(float)((p0 / p2) * fx + cx), projy = (double)(float)((p1 / p2) * fy + cy);
        ex = (double)m.uv[2 * c] - projx;
        ey = (double)m.uv[2 * c + 1] - projy;
    };
    // chi2 of a marker at Rt (no perturbation), valid in every lane: lane l evaluates corner l & 3, the quad adds up
    auto marker_chi2 = [&](const MarkerRec& m, const double* Rt) -> double {
        double ex, ey;
        marker_err(m, lane & 3, 0, Rt, ex, ey);
        double c = fma(ex, ex, ey * ey);
        c += __shfl_xor(c, 1);
        c += __shfl_xor(c, 2);
        return c;
    };
    auto marker_rho0 = [&](double c) -> double {   // WeightedHubberRobustKernel's rho[0]
        const double wt = *s_mkw;
        return c <= dsqr8 ? wt * c : wt * (2 * sqrt(c) * delta8 - dsqr8);
    };

    // chi2 of a match at the pose Rt; xz, yz, invz for the Jacobian
    auto project = [&](const MatchRec& m, const double* Rt, double& ex, double& ey, double& xz, double& yz, double& invz) -> double {
        double p0, p1, p2;
        to_camera(Rt, m.X, m.Y, m.Z, p0, p1, p2);
        invz = rcp_nr(p2);
        xz = p0 * invz; yz = p1 * invz;
        ex = (double)m.u - fma(xz, fx, cx);
        ey = (double)m.v - fma(yz, fy, cy);
        return (double)m.invsig * fma(ex, ex, ey * ey);
    };
    // EdgeStereoSE3ProjectXYZOnlyPose (typesg2o.h:521-590): cam_project divides in double and ROUNDS 1/z TO FLOAT before it uses it in
    // double, un-fused; the Jacobian uses the double 1/z (invz, as the monocular edge's).  er = kp_ur - (u_proj - bf / z).
    auto project_st = [&](const MatchRec& m, float ur, const double* Rt, double& ex, double& ey, double& er, double& xz, double& yz,
                          double& invz) -> double {
        double p0, p1, p2;
        to_camera(Rt, m.X, m.Y, m.Z, p0, p1, p2);
        invz = rcp_nr(p2);
        xz = p0 * invz; yz = p1 * invz;
        const double izf = (double)(float)(1.0 / p2);
        const double r0 = p0 * izf * fx + cx, r1 = p1 * izf * fy + cy;
        const double r2 = r0 - bf * izf;
        ex = (double)m.u - r0;
        ey = (double)m.v - r1;
        er = (double)ur - r2;
        return (double)m.invsig * fma(er, er, fma(ex, ex, ey * ey));
    };
    // ---- the one edge evaluation of classify, accumulate and the ladder.  st: the match has the three-row edge (STEREO instantiations only;
    // in the others it is the constant false and everything stereo folds away)
    auto edge = [&](const MatchRec& m, bool st, float ur, const double* Rt, double& ex, double& ey, double& er, double& xz, double& yz, double& invz) -> double {
        if constexpr (STEREO) { if (st) return project_st(m, ur, Rt, ex, ey, er, xz, yz, invz); }
        return project(m, Rt, ex, ey, xz, yz, invz);
    };
    // WeightedHubberRobustKernel: returns rho[0] and leaves rho[1] in rho1 above the threshold (the caller's 1 stays below it)
    auto huber = [&](double c, double wt, double dl, double ds, double& rho1) -> double {
        if (c <= ds) return wt * c;
        const double rs = rsq_nr(c);
        const double rc = wt * fma(2 * (c * rs), dl, -ds);   // (rho[0] before rho[1]: the other order renames the monocular kernels' registers)
        rho1 = dl * rs;
        return rc;
    };
    // the kernel of a match: the stereo edge's weight is doubled in float (pnpsolver.cpp:258) and its threshold is thHuber3D
    auto robust = [&](const MatchRec& m, bool st, double c, double& rho1) -> double {
        double wt = m.weight, dl = delta, ds = dsqr;
        if constexpr (STEREO) { if (st) { wt = (double)(m.weight * 2.f); dl = delta3; ds = dsqr3; } }
        return huber(c, wt, dl, ds, rho1);
    };

    // One pass over this thread's matches (every wave).  classify: first the reclassification that ends a round
    // (pnpsolver.cpp:358-371): a match that was excluded gets a fresh chi2 at RtC, the others the chi2 of the LAST pose the optimiser
    // evaluated them at (RtK: g2o keeps the edge errors of its last trial, accepted or not) — recomputed here instead of stored, same
    // bits; chi2 > 5.99 -> outlier; drop_robust as the reference from its third round on.  Then (RtA != nullptr) every active match:
    // error, chi2, robust weight and Jacobian at RtA, accumulated into the 29 sums; the wave's totals go to s_part.
    auto pass = [&](bool accumulate, const double* RtA, bool classify, bool drop_robust) {
        double acc[kNS];
#pragma unroll
        for (int i = 0; i < kNS; i++) acc[i] = 0;
        for (int e = tid; e < n; e += kPnpThreads) {
            const MatchRec m = rec[e];
            unsigned f = m.flags;
            double ex, ey, er = 0, xz, yz, invz;
            bool st = false;
            float ur = 0.f;
            if constexpr (STEREO) { st = (f & kStereo) != 0; ur = urs[e]; }
            if (classify) {
                double Rs[12];
#pragma unroll
                for (int i = 0; i < 12; i++) Rs[i] = s_pose[(f & kBad) ? 1 : 2][i];   // (read per match: four classifying passes per solve)
                const double c = edge(m, st, ur, Rs, ex, ey, er, xz, yz, invz);
                const bool b = c > (double)(st ? 7.815f : 5.99f);   // Chi3D, Chi2D
                f = (b ? kBad : kActive) | (drop_robust ? 0u : (f & kRobust));
                if constexpr (STEREO) f |= m.flags & kStereo;
                rec[e].flags = f;
                acc[28] += b ? 0.0 : 1.0;
            }
            if (!(f & kActive) || !accumulate) continue;
            const double c = edge(m, st, ur, RtA, ex, ey, er, xz, yz, invz);
            const double w = m.invsig;
            double rho1 = 1.0, rc = c;
            if (f & kRobust) rc = robust(m, st, c, rho1);
            acc[27] += rc;
            // 2x6 Jacobian rows (typesg2o.h:614-650): j = d ex / d xi, k = d ey / d xi; j[4] = k[3] = 0
            const double zf = invz * fx, zg = invz * fy, xf = xz * fx, yg = yz * fy;
            const double j0 = xf * yz, j1 = -fma(xf, xz, fx), j2 = yz * fx, j3 = -zf, j5 = xz * zf;
            const double k0 = fma(yg, yz, fy), k1 = -(xz * yg), k2 = -(xz * fy), k4 = -zg, k5 = yz * zg;
            const double s = rho1 * w;
            const double J[6] = {j0, j1, j2, j3, 0.0, j5}, K[6] = {k0, k1, k2, 0.0, k4, k5};
            const double sJ[6] = {s * j0, s * j1, s * j2, s * j3, 0.0, s * j5}, sK[6] = {s * k0, s * k1, s * k2, 0.0, s * k4, s * k5};
#pragma unroll
            for (int a = 0; a < 6; a++)
#pragma unroll
                for (int cc = a; cc < 6; cc++) {   // (the structural zeros are compile-time: their products are never formed)
                    double v = acc[tri(a, cc)];
                    if (a != 4 && cc != 4) v = fma(sJ[a], J[cc], v);
                    if (a != 3 && cc != 3) v = fma(sK[a], K[cc], v);
                    acc[tri(a, cc)] = v;
                }
#pragma unroll
            for (int a = 0; a < 6; a++) {
                double v = acc[21 + a];
                if (a != 4) v = fma(-sJ[a], ex, v);
                if (a != 3) v = fma(-sK[a], ey, v);
                acc[21 + a] = v;
            }
            if constexpr (STEREO) {
                if (st) {
                    // third Jacobian row (typesg2o.h:563-568): row 0 with the bf terms; l[2], l[3] = j[2], j[3]; l[4] = 0
                    const double bi = bf * invz;
                    const double L[6] = {j0 - bi * yz, j1 + bi * xz, j2, j3, 0.0, j5 - bi * invz};
                    const double sL[6] = {s * L[0], s * L[1], s * L[2], s * L[3], 0.0, s * L[5]};
#pragma unroll
                    for (int a = 0; a < 6; a++)
#pragma unroll
                        for (int cc = a; cc < 6; cc++)
                            if (a != 4 && cc != 4) acc[tri(a, cc)] = fma(sL[a], L[cc], acc[tri(a, cc)]);
#pragma unroll
                    for (int a = 0; a < 6; a++)
                        if (a != 4) acc[21 + a] = fma(-sL[a], er, acc[21 + a]);
                }
            }
        }
        int off = 0, real = kNS;
        WaveTransposeValu<kNS, 32>::run(acc, lane, off, real);   // lane l ends with the wave total of one value index
        if (real >= 1) s_part[wv * 32 + off] = acc[0];
    };
    // The markers of a pass, taken before its matches (no sum is live yet; the poses are read from LDS): a wave linearises its markers (mk_first,
    // mk_first + 8, ...); lane = 4 * pattern + corner (52 of the 64 lanes), the twelve perturbed errors of a corner are gathered into its lane
    // 0..3, which parks the two Jacobian rows in the marker's record; lane l < 28 then forms the marker's share of sum l — J^T rho1 J (21),
    // -J^T rho1 e (6), rho[0] (the information is the identity) — and the wave leaves its markers' shares in s_mkpart, where wave 0 adds
    // them to the totals of the pass.
    auto marker_linearise = [&](bool classify, bool drop_robust) __attribute__((noinline)) {
        if (mk_first >= nmk) return;
        int ja = 0, jc = lane;
        while (jc >= 6 - ja && ja < 6) { jc -= 6 - ja; ja++; }   // lane < 21: entry (ja, ja + jc) of the upper triangle; 21..26: b[lane - 21]
        jc += ja;
        double share = 0;
        for (int mi = mk_first; mi < nmk; mi += kPnpWaves) {
            MarkerRec& m = s_mk[mi];
            int robust = m.robust;
            if (classify) {
                // pnpsolver.cpp:376-380: computeError() at the pose the round ended with (the vertex's estimate), the kernel
                // dropped for good above Chi8D or from the third round on; never excluded, never counted
                const double c = marker_chi2(m, s_pose[1]);
                if (c > (double)15.507f || drop_robust) robust = 0;
                if (lane == 0) m.robust = robust;
            }
            const int k = lane < 52 ? lane >> 2 : 0, cn = lane & 3;
            double ex, ey;
            marker_err(m, cn, k, s_pose[0], ex, ey);
#pragma unroll
            for (int d = 0; d < 6; d++) {
                const int lp = (1 + d) * 4 + cn, lm = (7 + d) * 4 + cn;
                const double jx = mk_scalar * (__shfl(ex, lp) - __shfl(ex, lm)), jy = mk_scalar * (__shfl(ey, lp) - __shfl(ey, lm));
                if (lane < 4) { m.J[2 * cn][d] = jx; m.J[2 * cn + 1][d] = jy; }
            }
            double c = fma(ex, ex, ey * ey);   // (lanes 0..3: the unperturbed errors)
            c += __shfl_xor(c, 1);
            c += __shfl_xor(c, 2);
            if (lane < 4) { m.e[2 * cn] = ex; m.e[2 * cn + 1] = ey; }
            if (lane == 0) {
                double rho1 = 1.0, rc = c;
                if (robust) {
                    rc = marker_rho0(c);
                    if (!(c <= dsqr8)) rho1 = delta8 / sqrt(c);
                }
                m.rho1 = rho1; m.rc = rc;
            }
            // (written by this wave: its LDS operations complete in order)
            double v = 0;
            if (lane < 21) {
#pragma unroll
                for (int r = 0; r < 8; r++) v = fma(m.J[r][ja], m.J[r][jc], v);
                v *= m.rho1;
            } else if (lane < 27) {
#pragma unroll
                for (int r = 0; r < 8; r++) v = fma(m.J[r][lane - 21], m.e[r], v);
                v *= -m.rho1;
            } else if (lane == 27) v = m.rc;
            share += v;
        }
        if (lane < 32) s_mkpart[wv * 32 + lane] = share;
    };
    // what a pass does is published by wave 0 through s_ctl / s_pose before barrier A
    auto run_published_pass = [&]() -> int {
        const int mode = s_ctl[0];
        if (mode == kModeExit) return mode;
        if constexpr (MARKERS) { if (mode != kModeClassify) marker_linearise(s_ctl[1] != 0, s_ctl[2] != 0); }
        double RtA[12];
#pragma unroll
        for (int i = 0; i < 12; i++) RtA[i] = s_pose[0][i];
        pass(mode != kModeClassify, RtA, s_ctl[1] != 0, s_ctl[2] != 0);
        return mode;
    };

    // ---- the damping ladder.  When a trial is rejected, Levenberg multiplies lambda by ni, doubles ni and tries again from the SAME
    // pose and normal equations, up to ten times — at convergence (rho < 0 by rounding noise) it walks the whole ladder, which as
    // dependent passes is most of a solve.  The candidates do not depend on each other's outcome, only the DECISION is sequential:
    // wave w solves and applies candidates w, w + 8 (every wave the same bits as the sequential loop would produce), one pass
    // evaluates the robust chi2 of all of them, wave 0 then walks the decisions in order and stops where the loop would have.
    auto solve_candidates = [&]() {
        const int K = s_ctl[3];
        for (int k = wv; k < K; k += kPnpWaves) {
            double lam = s_lad[0], nn = s_lad[1];
            for (int j = 0; j < k; j++) { lam *= nn; nn *= 2; }
            double Hu[21], b[6], Tt[12], xs[6] = {0, 0, 0, 0, 0, 0};
#pragma unroll
            for (int i = 0; i < 21; i++) Hu[i] = s_H[i];
#pragma unroll
            for (int i = 0; i < 6; i++) b[i] = s_H[21 + i];
#pragma unroll
            for (int i = 0; i < 12; i++) Tt[i] = s_pose[0][i];
            const bool ok = p_solve6(Hu, b, lam, xs);
            if (ok) p_oplus_rt(Tt, xs);
            if (lane == 0) {
#pragma unroll
                for (int i = 0; i < 12; i++) s_cand[k][i] = Tt[i];
#pragma unroll
                for (int i = 0; i < 6; i++) s_cand[k][12 + i] = xs[i];
                s_cand[k][18] = ok ? 1.0 : 0.0;
            }
        }
    };
    auto ladder_pass = [&]() {
        const int K = s_ctl[3];
        double chi[kLadderMax];
#pragma unroll
        for (int k = 0; k < kLadderMax; k++) {
            chi[k] = 0;
            if (k < K) {
                double Rt[12];
#pragma unroll
                for (int i = 0; i < 12; i++) Rt[i] = s_cand[k][i];
                for (int e = tid; e < n; e += kPnpThreads) {
                    const MatchRec m = rec[e];
                    if (!(m.flags & kActive)) continue;
                    double ex, ey, er, xz, yz, invz, rho1;
                    bool st = false;
                    if constexpr (STEREO) st = (m.flags & kStereo) != 0;
                    const double c = edge(m, st, st ? urs[e] : 0.f, Rt, ex, ey, er, xz, yz, invz);   // (kp_ur read only for a stereo match: read for every match, a stereo pass costs 1-2 % more clocks)
                    double rc = c;
                    if (m.flags & kRobust) rc = robust(m, st, c, rho1);
                    chi[k] += rc;
                }
            }
        }
        if constexpr (MARKERS) {
            // the wave's markers at ALL candidates at once: lane = 4 * candidate + corner (32 lanes), the candidate's pose read from LDS
            const int kk = lane >> 2;
            for (int mi = mk_first; mi < nmk; mi += kPnpWaves) {
                const MarkerRec& m = s_mk[mi];
                const double c = marker_chi2(m, s_cand[kk < K ? kk : 0]);
                const double rc = m.robust ? marker_rho0(c) : c;
#pragma unroll
                for (int k = 0; k < kLadderMax; k++)
                    if (k < K && lane == 4 * k) chi[k] += rc;
            }
        }
        int off = 0, real = kLadderMax;
        WaveTransposeValu<kLadderMax, 32>::run(chi, lane, off, real);
        if (real >= 1) s_part[wv * 32 + off] = chi[0];
    };

    if (wv != 0) {
        // ---- the seven worker waves: evaluate what wave 0 publishes until it says stop
        for (;;) {
            __syncthreads();                    // A: the request is in LDS
            if (s_ctl[0] == kModeLadder) {
                solve_candidates();
                __syncthreads();                // A2: the candidates' poses are in LDS
                ladder_pass();
            } else {
                const int mode = run_published_pass();
                if (mode == kModeExit) break;
            }
            __syncthreads();                    // B: the partial sums are in LDS
        }
    } else {
        // ---- wave 0: g2o's SparseOptimizer::optimize + OptimizationAlgorithmLevenberg::solve as a state machine whose every
        // transition is ONE pass (or one damping-ladder pass) over the matches: a single call site for the pass keeps the code and
        // the register allocation of this wave small.  The control flow is the reference's, statement for statement:
        //   for round < 4 { T = T0; [classify previous round]; linearise;                         -> ST_INIT
        //     for it < 10 { swap(prev, cur); qmax = 0;
        //        do { solve; oplus; chi2 of the trial; accept / reject; } while (rho < 0 && ++qmax < 10)   -> ST_TRIAL, then ST_LADDER
        //        (a pose accepted inside a ladder pass is linearised by ST_RELIN before the next solve)
        //        stop on terminate or when the float chi2 no longer decreases }
        //   } classify the last round                                                               -> ST_FINAL
        enum : int { ST_INIT, ST_RELIN, ST_TRIAL, ST_LADDER, ST_FINAL, ST_DONE };
        int st = (MARKERS || n > 0) ? ST_INIT : ST_DONE;
        // measurement (A.clk != NULL only): cycles of wave 0 by section of a plain pass — [16] request prepared (solve + update), [17] barrier A,
        // [18] its share of the matches + butterfly, [19] barrier B, [20] totals + decision; [21] ladder passes as a whole
        long long ph[6] = {0, 0, 0, 0, 0, 0}, tp = A.clk ? (long long)__builtin_readcyclecounter() : 0;
        auto stamp = [&](int i) { if (A.clk) { const long long t = (long long)__builtin_readcyclecounter(); ph[i] += t - tp; tp = t; } };
        int n_pass = 0, round = 0, it = 0, qmax = 0, done = 0, last_round = -1, good = n;
        bool stale_H = false, lam_finite = true, ok2 = false;
        double lambda = 0, ni = 2, currentChi = 0, lastChiRaw = 0, rho = 0, scale = 1;
        float prevChi = FLT_MAX, curChi = FLT_MAX;
        // (the pose and the last solved step live in LDS, s_T / s_x: nothing but scalars stays in registers across a pass.  A failed
        // factorisation leaves the step as it was — g2o's solution vector does the same)
        if (lane < 8) s_x[lane] = 0;

        auto iter_begin = [&]() {
            const float t = prevChi; prevChi = curChi; curChi = t;   // swap(prevChi2, curChi2) at loop entry
            qmax = 0; rho = 0; lam_finite = true;
            st = stale_H ? ST_RELIN : ST_TRIAL;
        };
        auto round_end = [&]() {
            if (lane < 12) s_pose[1][lane] = s_T[lane];
            if (lane == 0) A.result[1 + round] = done;
            last_round = round;
            ++round;
            st = round < 4 ? ST_INIT : ST_FINAL;
        };
        auto after_trials = [&]() {          // the do-while of Levenberg's solve() has just evaluated a trial
            if (lam_finite && rho < 0 && qmax < 10) { st = ST_LADDER; return; }
            done++;
            const bool terminate = (qmax == 10 || rho == 0 || !isfinite(lambda));
            curChi = (float)lastChiRaw;
            const float diff = prevChi - curChi;
            if (terminate || !(diff > 0.f) || it + 1 >= 10) round_end();
            else { ++it; iter_begin(); }
        };
        auto decide = [&](bool ok, double chi, const double* pose_lds) -> bool {   // one accept / reject decision (lambda, ni, currentChi, T)
            lastChiRaw = chi;
            const double tempChi = ok ? chi : DBL_MAX;
            const double r = (currentChi - tempChi) / scale;
            const bool acc = r > 0 && isfinite(tempChi);
            if (acc) {
                const double t3 = 2 * r - 1;
                double alpha = 1. - t3 * t3 * t3;
                alpha = fmin(alpha, 2. / 3.);
                lambda *= fmax(1. / 3., alpha);
                ni = 2;
                currentChi = tempChi;
                if (lane < 12) s_T[lane] = pose_lds[lane];
            } else {
                lambda *= ni; ni *= 2;                          // T and the normal equations stay those of the last accepted pose
                if (!isfinite(lambda)) lam_finite = false;
            }
            rho = r;
            return acc;
        };

        while (st != ST_DONE) {
            if (st == ST_LADDER) {
                // ---- rejected: the rest of the damping ladder in one pass
                const int K = 10 - qmax < kLadderMax ? 10 - qmax : kLadderMax;
                if (lane < 12) s_pose[0][lane] = s_T[lane];
                if (lane == 0) {
                    s_ctl[0] = kModeLadder; s_ctl[3] = K;
                    s_lad[0] = lambda; s_lad[1] = ni;
                }
                __syncthreads();                // A
                solve_candidates();
                __syncthreads();                // A2
                ladder_pass();
                __syncthreads();                // B
                ++n_pass;
                if (lane < kLadderMax) {
                    double mine = s_part[lane];
#pragma unroll
                    for (int w2 = 1; w2 < kPnpWaves; w2++) mine += s_part[w2 * 32 + lane];   // wave order
                    s_tot[lane] = mine;
                }
                double bb[6], x[6];
#pragma unroll
                for (int i = 0; i < 6; i++) { bb[i] = s_H[21 + i]; x[i] = s_x[i]; }
                int k_last = 0;
                for (int k = 0; k < K; k++) {   // the decisions, in the order the sequential loop takes them
                    const bool okk = s_cand[k][18] != 0.0;
                    if (okk) {
#pragma unroll
                        for (int i = 0; i < 6; i++) x[i] = s_cand[k][12 + i];
                    }
                    double sc = 0;
#pragma unroll
                    for (int i = 0; i < 6; i++) sc += x[i] * (lambda * x[i] + bb[i]);
                    scale = 1e-3 + sc;
                    k_last = k;
                    if (decide(okk, s_tot[k], s_cand[k])) stale_H = true;   // (a ladder pass does not linearise)
                    if (!lam_finite) break;   // the reference leaves its loop before the increment when lambda overflows
                    qmax++;
                    if (!(rho < 0 && qmax < 10)) break;
                }
                if (lane < 12) s_pose[2][lane] = s_cand[k_last][lane];   // the edges keep the errors of the last trial the loop evaluated
                if (lane == 0) {
#pragma unroll
                    for (int i = 0; i < 6; i++) s_x[i] = x[i];
                }
                after_trials();
                stamp(5);
                continue;
            }
            // ---- the request of this state
            int mode = kModeEval;
            bool classify = false, drop = false;
            if (st == ST_INIT) {
                if (lane < 12) { s_T[lane] = s_pose[3][lane]; s_pose[0][lane] = s_pose[3][lane]; }   // every round restarts from the input pose (:354)
                classify = round > 0; drop = round - 1 >= 2;
            } else if (st == ST_RELIN) {
                if (lane < 12) s_pose[0][lane] = s_T[lane];
            } else if (st == ST_TRIAL) {
                double Tt[12], x[6], Hu[21], b[6];
#pragma unroll
                for (int i = 0; i < 12; i++) Tt[i] = s_T[i];
#pragma unroll
                for (int i = 0; i < 6; i++) x[i] = s_x[i];
#pragma unroll
                for (int i = 0; i < 21; i++) Hu[i] = s_H[i];
#pragma unroll
                for (int i = 0; i < 6; i++) b[i] = s_H[21 + i];
                ok2 = p_solve6(Hu, b, lambda, x);
                if (ok2) p_oplus_rt(Tt, x);
                double sc = 0;
#pragma unroll
                for (int i = 0; i < 6; i++) sc += x[i] * (lambda * x[i] + b[i]);
                scale = 1e-3 + sc;
                if (lane == 0) {
#pragma unroll
                    for (int i = 0; i < 12; i++) s_pose[0][i] = Tt[i];
#pragma unroll
                    for (int i = 0; i < 6; i++) s_x[i] = x[i];
                }
            } else if (st == ST_FINAL) {
                mode = kModeClassify; classify = true; drop = last_round >= 2;
            }
            if (lane == 0) { s_ctl[0] = mode; s_ctl[1] = classify ? 1 : 0; s_ctl[2] = drop ? 1 : 0; }
            stamp(0);
            __syncthreads();                    // A
            stamp(1);
            run_published_pass();
            stamp(2);
            __syncthreads();                    // B
            stamp(3);
            ++n_pass;
            if (lane < kNS) {
                double mine = s_part[lane];
#pragma unroll
                for (int w2 = 1; w2 < kPnpWaves; w2++) mine += s_part[w2 * 32 + lane];   // wave order
                if constexpr (MARKERS) {
                    if (mode == kModeEval)
                        for (int j = 0; j < nmk && j < kPnpWaves; j++) mine += s_mkpart[(kPnpWaves - 1 - j) * 32 + lane];   // marker order
                }
                s_tot[lane] = mine;
            }
            if (mode == kModeEval && lane < 12) s_pose[2][lane] = s_pose[0][lane];   // the pose the edges' errors now belong to
            // (the same wave wrote s_tot: LDS operations of one wave complete in order)
            const double chi_sum = s_tot[27], good_sum = s_tot[28];
            if (st == ST_INIT) {
                if (round > 0) {
                    good = (int)good_sum;
                    if constexpr (!MARKERS) {   // pnpsolver.cpp:383: the stop below ten good matches applies only without markers
                        if (good < 10) { st = ST_DONE; continue; }
                    }
                }
                if (lane < 27) s_H[lane] = s_tot[lane];          // the totals of the pass are the normal equations of the pose it evaluated
                currentChi = chi_sum; lastChiRaw = chi_sum; ni = 2;
                {
                    double m = 0;
#pragma unroll
                    for (int j = 0; j < 6; j++) {   // computeLambdaInit's std::max(fabs(h), m): a NaN diagonal entry is kept unless a number follows it
                        const double h = fabs(s_H[tri(j, j)]);
                        m = h < m ? m : h;
                    }
                    lambda = 1e-5 * m;
                }
                prevChi = FLT_MAX; curChi = FLT_MAX; done = 0; stale_H = false; it = 0;
                iter_begin();
            } else if (st == ST_RELIN) {
                if (lane < 27) s_H[lane] = s_tot[lane];
                stale_H = false;
                st = ST_TRIAL;
            } else if (st == ST_TRIAL) {
                if (decide(ok2, chi_sum, s_pose[0])) { if (lane < 27) s_H[lane] = s_tot[lane]; }   // the pass has linearised at the accepted pose already
                if (lam_finite) qmax++;   // (the reference leaves its loop before the increment when lambda overflows)
                after_trials();
            } else {   // ST_FINAL: the classification that ends the last round
                good = (int)good_sum;
                st = ST_DONE;
            }
            stamp(4);
        }
        if (A.clk && lane == 0) { for (int i = 0; i < 6; i++) A.clk[16 + i] = ph[i]; }
        if (A.clk && lane == 0) A.clk[2] = __builtin_readcyclecounter();
        if (lane == 0) {
            s_ctl[0] = kModeExit;
            for (int r = last_round + 1; r < 4; r++) A.result[1 + r] = 0;
            A.result[0] = n > 0 ? good : 0;
            double Tend[12];
#pragma unroll
            for (int i = 0; i < 12; i++) Tend[i] = s_pose[1][i];
            float M[16];   // the pose this solve returns: pose_out, and what the tracker's decision reads
            for (int r = 0; r < 3; r++) { for (int c = 0; c < 3; c++) M[r * 4 + c] = (float)Tend[r * 3 + c]; M[r * 4 + 3] = (float)Tend[9 + r]; }
            M[12] = M[13] = M[14] = 0.f; M[15] = 1.f;
            for (int i = 0; i < 16; i++) A.pose_out[i] = M[i];
            if (A.dec.dyn17) pnp_decide(A, n > 0 ? good : 0, M);
            if (A.state_out) {
                double q[4];
                quat_from_R(Tend, q);
                quat_norm_pos(q);
                for (int i = 0; i < 4; i++) A.state_out[i] = q[i];
                for (int i = 0; i < 3; i++) A.state_out[4 + i] = Tend[9 + i];
            }
            if (A.clk) A.clk[4] = n_pass;
        }
        __syncthreads();                        // A of the exit request
    }
    for (int e = tid; e < n; e += kPnpThreads) A.bad_out[e] = (rec[e].flags & kBad) ? 1 : 0;
    if (A.host_done) {   // results went to pinned host memory: make them visible, then post the completion word
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");
        __syncthreads();
        if (tid == 0) __hip_atomic_store(A.host_done, A.done_word, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
    if (A.clk && tid == 0) A.clk[3] = __builtin_readcyclecounter();
}
// the eight instantiations, in the order the device code has always held them (launch_as below would name them in another)
template __global__ void pnp_solve_kernel<true, true, false>(PnpArgs);
template __global__ void pnp_solve_kernel<false, true, false>(PnpArgs);
template __global__ void pnp_solve_kernel<true, false, false>(PnpArgs);
template __global__ void pnp_solve_kernel<false, false, false>(PnpArgs);
template __global__ void pnp_solve_kernel<true, true, true>(PnpArgs);
template __global__ void pnp_solve_kernel<false, true, true>(PnpArgs);
template __global__ void pnp_solve_kernel<true, false, true>(PnpArgs);
template __global__ void pnp_solve_kernel<false, false, true>(PnpArgs);

}  // namespace

struct uh_pnp {
    uh_ctx* ctx = nullptr;
    uh::DevBuf d_work;
    uh::MappedBuf h_io;      // pinned, device-visible: [completion word | results | inputs]
    unsigned long long seq = 0;
    bool attr_set[2][2] = {{false, false}, {false, false}};   // the LDS attribute of pnp_solve_kernel<true, STEREO, MARKERS>, per [MARKERS][STEREO]
    long long* d_clk = nullptr;   // measurement hook (uh_pnp_debug_clocks)
    void* ransac = nullptr;       // the relocalisation RANSAC's buffers (pnp_ransac.hip makes them on first use and names their deleter)
    void (*ransac_free)(void*) = nullptr;
    ~uh_pnp() { if (d_clk) (void)hipFree(d_clk); if (ransac && ransac_free) ransac_free(ransac); }
};

namespace {

constexpr size_t pnp_rec_bytes(bool stereo) { return stereo ? kPnpRecBytesStereo : sizeof(MatchRec); }

// the fields every entry sets; the callers add the device-side match count, the decision or the completion word.  mk: device-visible
// arrays; NULL or no markers: the marker-free instantiations run
PnpArgs pnp_args(const float* pose, const float* intr, int n, const uh::PnpMatches& m, const uh_pnp_markers* mk, void* work, float* pose_out, unsigned char* bad_out,
                 int* result, double* state_out) {
    PnpArgs A{};
    A.pose_in = pose; A.intr = intr; A.n = n; A.p3d = m.p3d; A.kp = m.kp; A.invsig = m.inv_sigma; A.weight = m.weight; A.depth = m.depth; A.bl = m.bl;
    A.work = work; A.pose_out = pose_out; A.bad_out = bad_out; A.result = result; A.state_out = state_out;
    if (mk && mk->n > 0) { A.n_mk = mk->n; A.mk_pose = mk->pose_g2m; A.mk_size = mk->size; A.mk_corners = mk->und_corners; }
    return A;
}

// what every entry checks of a uh_pnp_markers before anything is launched; host_arrays: the sizes can be read here
int check_markers(const char* fn, const uh_pnp_markers* m, bool host_arrays) {
    if (!m) return UH_OK;
    UH_REQUIRE(m->n >= 0 && m->n <= UH_PNP_MAX_MARKERS, "%s: %d markers outside [0, %d]", fn, m->n, UH_PNP_MAX_MARKERS);
    if (m->n > 0) UH_REQUIRE(m->pose_g2m && m->size && m->und_corners, "%s: NULL marker arrays", fn);
    if (host_arrays)
        for (int i = 0; i < m->n; i++) UH_REQUIRE(std::isfinite(m->size[i]) && m->size[i] > 0.f, "%s: marker %d has size %g", fn, i, (double)m->size[i]);
    return UH_OK;
}

// one instantiation: the dynamic-LDS limit of a CACHED one is set once per solver object
template <bool C, bool S, bool M>
int launch_as(uh_pnp* p, const PnpArgs& A, size_t lds) {
    if (C && !p->attr_set[M][S]) {
        const size_t most = M ? pnp_marker_offset(kPnpLdsMatches, S) + kPnpMarkerLds : kPnpLdsMatches * pnp_rec_bytes(S);
        UH_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(pnp_solve_kernel<C, S, M>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)most));
        p->attr_set[M][S] = true;
    }
    static constexpr const char* scope[2][2][2] = {   // [C][S][M], the source spelling as UH_LAUNCH's scopes have it
        {{"pnp_solve_kernel<false, false, false>", "pnp_solve_kernel<false, false, true>"}, {"pnp_solve_kernel<false, true, false>", "pnp_solve_kernel<false, true, true>"}},
        {{"pnp_solve_kernel<true, false, false>", "pnp_solve_kernel<true, false, true>"}, {"pnp_solve_kernel<true, true, false>", "pnp_solve_kernel<true, true, true>"}}};
    uh::ProfScope ps(p->ctx, scope[C][S][M]);
    hipLaunchKernelGGL((pnp_solve_kernel<C, S, M>), dim3(1), dim3(kPnpThreads), lds, p->ctx->stream, A);
    return UH_OK;
}

// the instantiation: matches in LDS up to kPnpLdsMatches (CACHED), the stereo edges with a depth array (STEREO), the marker edges with markers
int launch(uh_pnp* p, PnpArgs& A) {
    A.clk = p->d_clk;
    const bool cached = A.n <= kPnpLdsMatches, stereo = A.depth != nullptr, markers = A.n_mk > 0;
    const size_t lds = markers ? (cached ? pnp_marker_offset(A.n, stereo) : 0) + kPnpMarkerLds : cached ? (size_t)std::max(A.n, 1) * pnp_rec_bytes(stereo) : 0;
    static constexpr int (*as[2][2][2])(uh_pnp*, const PnpArgs&, size_t) = {
        {{launch_as<false, false, false>, launch_as<false, false, true>}, {launch_as<false, true, false>, launch_as<false, true, true>}},
        {{launch_as<true, false, false>, launch_as<true, false, true>}, {launch_as<true, true, false>, launch_as<true, true, true>}}};
    const int rc = as[cached][stereo][markers](p, A, lds);
    if (rc) return rc;
    UH_HIP_CHECK(hipGetLastError());
    return UH_OK;
}

// uh_pnp_solve_dev (d_depth == NULL), uh_pnp_solve_stereo_dev and uh_pnp_solve_markers_dev (mk: device arrays, or NULL)
int solve_dev(const char* fn, uh_pnp* p, const float* d_pose_f2g, const float* d_intr4, int n, const uh::PnpMatches& m, const uh_pnp_markers* mk, void* d_work,
              float* d_pose_out, uint8_t* d_bad_out, int32_t* d_result5, double* d_state7) {
    UH_REQUIRE(p && d_pose_f2g && d_intr4 && d_pose_out && d_result5, "%s: NULL argument", fn);
    UH_REQUIRE(n >= 0, "%s: negative match count", fn);
    if (m.depth) UH_REQUIRE(m.bl > 0.f, "%s: a depth array needs a baseline > 0 (bl = %g)", fn, (double)m.bl);
    int rc;
    if ((rc = check_markers(fn, mk, false))) return rc;
    if (n > 0) UH_REQUIRE(m.p3d && m.kp && m.inv_sigma && m.weight && d_work && d_bad_out, "%s: NULL match arrays", fn);
    UH_HIP_CHECK(hipSetDevice(p->ctx->device));
    PnpArgs A = pnp_args(d_pose_f2g, d_intr4, n, m, mk, d_work, d_pose_out, d_bad_out, d_result5, d_state7);
    return launch(p, A);
}

}  // namespace

namespace uh {
uh_ctx* pnp_ctx(uh_pnp* p) { return p->ctx; }
// the slot of the object for pnp_ransac.hip's state; a non-NULL `free_fn` (given once, when the state is made) is kept for the destructor
void** pnp_ransac_slot(uh_pnp* p, void (*free_fn)(void*)) { if (free_fn) p->ransac_free = free_fn; return &p->ransac; }
// the scratch a solve over n_cap matches needs beyond the LDS (uh_track_pose reserves it before its first launch)
int pnp_reserve(uh_pnp* p, int n_cap, bool stereo) {
    return n_cap > kPnpLdsMatches ? p->d_work.reserve((size_t)n_cap * pnp_rec_bytes(stereo)) : UH_OK;
}
// the solve behind uh_track_pose: everything resident, the match count decided by an earlier launch of the same stream
// m.depth != NULL: the stereo form; d_mk: NULL, or the frame's markers (device-visible arrays)
int pnp_enqueue_dev(uh_pnp* p, const float* d_pose, const float* d_intr4, int n_cap, const int* d_n, const PnpMatches& m, const uh_pnp_markers* d_mk, float* d_pose_out,
                    unsigned char* d_bad_out, int* d_result5, const PnpDecide* dec) {
    UH_HIP_CHECK(hipSetDevice(p->ctx->device));
    int rc;
    if ((rc = pnp_reserve(p, n_cap, m.depth != nullptr))) return rc;
    PnpArgs A = pnp_args(d_pose, d_intr4, n_cap, m, d_mk, p->d_work.p, d_pose_out, d_bad_out, d_result5, nullptr);
    A.n_dev = d_n;
    if (dec) A.dec = *dec;
    return launch(p, A);
}
}  // namespace uh

extern "C" {

int uh_pnp_create(uh_ctx* ctx, uh_pnp** out) {
    UH_REQUIRE(ctx && out, "uh_pnp_create: NULL argument");
    uh_pnp* p = new uh_pnp();
    p->ctx = ctx;
    *out = p;
    return UH_OK;
}
void uh_pnp_destroy(uh_pnp* p) { delete p; }

// Everything resident in HBM; asynchronous on the context stream.  d_work: n * 32 bytes of scratch (16-byte aligned), only used
// beyond kPnpLdsMatches matches.
int uh_pnp_solve_dev(uh_pnp* p, const float* d_pose_f2g, const float* d_intr4, int n, const float* d_p3d, const float* d_kp,
                     const float* d_inv_sigma, const float* d_weight, void* d_work, float* d_pose_out, uint8_t* d_bad_out,
                     int32_t* d_result5, double* d_state7) {
    return solve_dev("uh_pnp_solve_dev", p, d_pose_f2g, d_intr4, n, {d_p3d, d_kp, d_inv_sigma, d_weight, nullptr, 0.f}, nullptr, d_work, d_pose_out, d_bad_out, d_result5, d_state7);
}

// Stereo / RGB-D form of uh_pnp_solve_dev: d_depth (n floats, device) as in uh_pnp_solve_stereo; d_work = n * 36 bytes when d_depth is given.
// The depths are not read on the host, so a non-NULL d_depth needs bl > 0.  d_depth == NULL is uh_pnp_solve_dev itself.
int uh_pnp_solve_stereo_dev(uh_pnp* p, const float* d_pose_f2g, const float* d_intr4, int n, const float* d_p3d, const float* d_kp,
                            const float* d_inv_sigma, const float* d_weight, const float* d_depth, float bl, void* d_work, float* d_pose_out,
                            uint8_t* d_bad_out, int32_t* d_result5, double* d_state7) {
    return solve_dev(d_depth ? "uh_pnp_solve_stereo_dev" : "uh_pnp_solve_dev", p, d_pose_f2g, d_intr4, n, {d_p3d, d_kp, d_inv_sigma, d_weight, d_depth, d_depth ? bl : 0.f},
                     nullptr, d_work, d_pose_out, d_bad_out, d_result5, d_state7);
}

// uh_pnp_solve_stereo_dev with markers: the three arrays of `markers` are device arrays too (the struct itself is the host's).  The sizes
// are not read on the host.  markers == NULL or n == 0 markers is uh_pnp_solve_stereo_dev itself.
int uh_pnp_solve_markers_dev(uh_pnp* p, const float* d_pose_f2g, const float* d_intr4, int n, const float* d_p3d, const float* d_kp,
                             const float* d_inv_sigma, const float* d_weight, const float* d_depth, float bl, const uh_pnp_markers* markers,
                             void* d_work, float* d_pose_out, uint8_t* d_bad_out, int32_t* d_result5, double* d_state7) {
    if (!markers || markers->n == 0)
        return uh_pnp_solve_stereo_dev(p, d_pose_f2g, d_intr4, n, d_p3d, d_kp, d_inv_sigma, d_weight, d_depth, bl, d_work, d_pose_out, d_bad_out, d_result5, d_state7);
    return solve_dev("uh_pnp_solve_markers_dev", p, d_pose_f2g, d_intr4, n, {d_p3d, d_kp, d_inv_sigma, d_weight, d_depth, d_depth ? bl : 0.f}, markers, d_work,
                     d_pose_out, d_bad_out, d_result5, d_state7);
}

// Host-pointer form: PnPSolver::solvePnp(frame, map, matches, pose): returns the inlier count (>= 0) or a negative error.
// The caller's arrays are packed into the object's pinned staging block (a few KB), the kernel reads them from there and writes
// pose / flags / counters back into the same block; the host polls the completion word the kernel posts last.
int uh_pnp_solve(uh_pnp* p, const float* pose_f2g, const float* intr4, int n, const float* p3d, const float* kp, const float* inv_sigma,
                 const float* weight, float* pose_out, uint8_t* bad_out, int32_t* iters_out4, double* state_out7) {
    return uh_pnp_solve_stereo(p, pose_f2g, intr4, n, p3d, kp, inv_sigma, weight, nullptr, 0.f, pose_out, bad_out, iters_out4, state_out7);
}

// Stereo / RGB-D form of uh_pnp_solve: depth[i] = Frame::getDepth(queryIdx) (<= 0: monocular match), bl = imageParams.bl.  depth == NULL
// is uh_pnp_solve itself.
int uh_pnp_solve_stereo(uh_pnp* p, const float* pose_f2g, const float* intr4, int n, const float* p3d, const float* kp, const float* inv_sigma,
                        const float* weight, const float* depth, float bl, float* pose_out, uint8_t* bad_out, int32_t* iters_out4, double* state_out7) {
    return uh_pnp_solve_markers(p, pose_f2g, intr4, n, p3d, kp, inv_sigma, weight, depth, bl, nullptr, pose_out, bad_out, iters_out4, state_out7);
}

// uh_pnp_solve_stereo with the frame's markers (pnpsolver.cpp:280-386).  markers == NULL or n == 0 markers: uh_pnp_solve_stereo itself, the
// marker-free kernels on the same staging block.  Without matches but with markers the solve runs (the match arrays may be NULL).
int uh_pnp_solve_markers(uh_pnp* p, const float* pose_f2g, const float* intr4, int n, const float* p3d, const float* kp, const float* inv_sigma,
                         const float* weight, const float* depth, float bl, const uh_pnp_markers* markers, float* pose_out, uint8_t* bad_out,
                         int32_t* iters_out4, double* state_out7) {
    const int nmk = markers ? markers->n : 0;
    const char* fn = nmk ? "uh_pnp_solve_markers" : depth ? "uh_pnp_solve_stereo" : "uh_pnp_solve";
    UH_REQUIRE(p && pose_f2g && intr4 && pose_out, "%s: NULL argument", fn);
    UH_REQUIRE(n >= 0, "%s: negative match count", fn);
    int rc;
    if ((rc = check_markers("uh_pnp_solve_markers", markers, true))) return rc;
    if (n == 0 && nmk == 0) { memcpy(pose_out, pose_f2g, 64); if (iters_out4) memset(iters_out4, 0, 16); return 0; }   // pnpsolver.cpp:149-150
    if (n > 0) UH_REQUIRE(p3d && kp && inv_sigma && weight && bad_out, "%s: NULL match arrays", fn);
    if (n == 0) depth = nullptr;
    const bool any_depth = depth && std::any_of(depth, depth + n, [](float d) { return !(d <= 0.f); });
    UH_REQUIRE(!any_depth || bl > 0.f, "uh_pnp_solve_stereo: stereo matches need a baseline > 0 (bl = %g)", (double)bl);
    UH_HIP_CHECK(hipSetDevice(p->ctx->device));
    const size_t nf = (size_t)n;
    uh::Layout L{64};   // the pinned block, 64-byte regions: [0, 64) the completion word, the results, the inputs
    const size_t o_pout = L.take<float>(16, 64), o_res = L.take<int>(5, 64), o_state = L.take<double>(7, 64), o_pose = L.take<float>(16, 64), o_intr = L.take<float>(4, 64);
    const size_t o_p3d = L.take<float>(3 * nf, 64), o_kp = L.take<float>(2 * nf, 64), o_is = L.take<float>(nf, 64), o_w = L.take<float>(nf, 64), o_bad = L.take<unsigned char>(nf, 64),
                 o_dep = L.take<float>(depth ? nf : 0, 64), o_mkp = L.take<float>(16 * (size_t)nmk, 64), o_mks = L.take<float>((size_t)nmk, 64),
                 o_mkc = L.take<float>(8 * (size_t)nmk, 64), total = L.take<char>(0, 64);
    if ((rc = p->h_io.reserve(total))) return rc;
    if ((rc = uh::pnp_reserve(p, n, depth != nullptr))) return rc;
    char* h = p->h_io.host<char>();
    char* d = p->h_io.dev<char>();
    memcpy(h + o_pose, pose_f2g, 64);
    memcpy(h + o_intr, intr4, 16);
    if (n > 0) {
        memcpy(h + o_p3d, p3d, nf * 12);
        memcpy(h + o_kp, kp, nf * 8);
        memcpy(h + o_is, inv_sigma, nf * 4);
        memcpy(h + o_w, weight, nf * 4);
    }
    if (depth) memcpy(h + o_dep, depth, nf * 4);
    if (nmk) {
        memcpy(h + o_mkp, markers->pose_g2m, (size_t)nmk * 64);
        memcpy(h + o_mks, markers->size, (size_t)nmk * 4);
        memcpy(h + o_mkc, markers->und_corners, (size_t)nmk * 32);
    }
    auto df = [d](size_t o) { return (const float*)(d + o); };
    const uh::PnpMatches dm{df(o_p3d), df(o_kp), df(o_is), df(o_w), depth ? df(o_dep) : nullptr, bl};
    const uh_pnp_markers dmk{nmk, df(o_mkp), df(o_mks), df(o_mkc)};
    PnpArgs A = pnp_args(df(o_pose), df(o_intr), n, dm, nmk ? &dmk : nullptr, p->d_work.p, (float*)(d + o_pout), (unsigned char*)(d + o_bad), (int*)(d + o_res), (double*)(d + o_state));
    A.host_done = (unsigned long long*)d;
    A.done_word = ++p->seq;
    std::atomic_thread_fence(std::memory_order_release);
    if ((rc = launch(p, A))) return rc;
    if ((rc = uh::wait_host_word(reinterpret_cast<volatile unsigned long long*>(h), A.done_word, p->ctx->stream, fn))) return rc;
    int32_t res[5];
    memcpy(res, h + o_res, 20);
    memcpy(pose_out, h + o_pout, 64);
    if (n > 0) memcpy(bad_out, h + o_bad, nf);
    if (state_out7) memcpy(state_out7, h + o_state, 56);
    if (iters_out4) memcpy(iters_out4, res + 1, 16);
    return res[0];
}

// measurement hook (scripts/time_pnp.py): shader-clock timestamps of the next solves — [0] kernel entry, [1] inputs staged,
// [2] rounds done, [3] results posted (s_memtime ticks), [4] number of passes.  on = 0 switches it off again.  out512: 512 entries
// (the whole 4096-byte stamp block is copied).
int uh_pnp_debug_clocks(uh_pnp* p, int on, long long* out512) {
    UH_REQUIRE(p, "uh_pnp_debug_clocks: NULL");
    UH_HIP_CHECK(hipSetDevice(p->ctx->device));
    if (on && !p->d_clk) { UH_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&p->d_clk), 4096)); UH_HIP_CHECK(hipMemset(p->d_clk, 0, 4096)); }
    if (out512 && p->d_clk) { UH_HIP_CHECK(hipStreamSynchronize(p->ctx->stream)); UH_HIP_CHECK(hipMemcpy(out512, p->d_clk, 4096, hipMemcpyDeviceToHost)); }
    if (!on && p->d_clk) { (void)hipFree(p->d_clk); p->d_clk = nullptr; }
    return UH_OK;
}

}  // extern "C"
