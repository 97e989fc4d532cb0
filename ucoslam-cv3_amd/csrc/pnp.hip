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
#include "pnp_solve_body.hpp"
}
// uh_relocalize_pose (relocalize.hpp): one monocular solve per workgroup, each with its own arguments from a device-visible table; a
// workgroup whose match count (n_dev) is zero leaves at once.  The same text as pnp_solve_kernel's (pnp_solve_body.hpp) behind another
// head, so that kernel's code stays what it was.
template <bool CACHED>
__global__ __launch_bounds__(kPnpThreads) void pnp_solve_batch_kernel(const PnpArgs* __restrict__ table) {
    constexpr bool STEREO = false, MARKERS = false;
    const PnpArgs A = table[blockIdx.x];   // (pinned memory: read once, uniform)
#include "pnp_solve_body.hpp"
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
    bool attr_batch = false;   // the LDS attribute of pnp_solve_batch_kernel<true>
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
// the solves behind uh_relocalize_pose: `count` monocular solves in ONE launch, one workgroup each.  The arguments go into the caller's
// pinned table (h_table, read by the launch in place as d_table); an item's scratch for the packed records of more than kPnpLdsMatches
// matches is its own stretch of the object's (reserved here: it only ever grows)
size_t pnp_batch_table_bytes(int count) { return sizeof(PnpArgs) * (size_t)std::max(count, 1); }
int pnp_enqueue_batch(uh_pnp* p, const float* d_intr4, int count, const PnpBatchItem* items, void* h_table, const void* d_table) {
    UH_HIP_CHECK(hipSetDevice(p->ctx->device));
    int n_max = 0, rc;
    for (int i = 0; i < count; i++) n_max = std::max(n_max, items[i].n_cap);
    const bool cached = n_max <= kPnpLdsMatches;
    std::vector<size_t> off((size_t)count + 1, 0);
    for (int i = 0; i < count; i++) off[i + 1] = off[i] + (cached ? 0 : (((size_t)items[i].n_cap * sizeof(MatchRec) + 255) & ~(size_t)255));
    if (!cached && (rc = p->d_work.reserve(off[count]))) return rc;
    PnpArgs* T = static_cast<PnpArgs*>(h_table);
    for (int i = 0; i < count; i++) {
        const PnpBatchItem& it = items[i];
        T[i] = pnp_args(it.d_pose, d_intr4, it.n_cap, it.m, nullptr, cached ? nullptr : static_cast<char*>(p->d_work.p) + off[i], it.d_pose_out, it.d_bad_out, it.d_result5, nullptr);
        T[i].n_dev = it.d_n;
    }
    std::atomic_thread_fence(std::memory_order_release);
    if (cached && !p->attr_batch) {
        UH_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(pnp_solve_batch_kernel<true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)(kPnpLdsMatches * sizeof(MatchRec))));
        p->attr_batch = true;
    }
    const PnpArgs* dT = static_cast<const PnpArgs*>(d_table);
    if (cached) UH_LAUNCH(p->ctx, pnp_solve_batch_kernel<true>, dim3(count), dim3(kPnpThreads), (size_t)std::max(n_max, 1) * sizeof(MatchRec), dT);
    else UH_LAUNCH(p->ctx, pnp_solve_batch_kernel<false>, dim3(count), dim3(kPnpThreads), 0, dT);
    UH_HIP_CHECK(hipGetLastError());
    return UH_OK;
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
