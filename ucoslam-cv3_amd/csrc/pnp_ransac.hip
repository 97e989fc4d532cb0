// Relocalisation RANSAC on the device (uh_pnp_ransac): PnPSolver::solvePnPRansac, src/optimization/pnpsolver.cpp:36-114, for all
// candidate keyframes of one lost frame and all hypotheses of each in two launches.  The contract is in include/ucoslam_hip.h, the
// arithmetic in p3p_math.hpp (one text for device and host).
//
//   host     checks every index the kernels will trust (sample indices, caps), packs all problems into one pinned block: ONE upload
//   pr_hypothesis_kernel   one wave per (problem, hypothesis), four waves per workgroup, grid (ceil(max iters / 4), problems).  The sample
//            and the problem record are wave-uniform.  The quartic is set up once on every lane; lanes take root (lane & 3) each through
//            the back-substitution and the matrix -> Rodrigues step, and the pick is a cross-lane minimum over lanes 0-3 with the lowest
//            lane on ties (the roots are sorted, so the lane order is the solution order).  The chosen float rt[6] is broadcast, every lane
//            builds the same float 3x4, and the 64 lanes stride over the matches: per 64 matches one ballot word goes into the
//            hypothesis' bit mask (device scratch of the uh_pnp object, vector stores) and its popcount into the count.
//   pr_select_kernel       one workgroup per problem: the first hypothesis with the strictly largest count >= 1 through an integer
//            maximum over (count, -iteration) keys, then an ordered prefix popcount over the winner's mask writes the inlier indices
//            in ascending order.
//   host     ONE download of the result block, ONE wait.
// No atomics and no float reductions: the result is a function of the input alone.
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdlib>
#include "common.hpp"
#include "p3p_math.hpp"

namespace uh {
uh_ctx* pnp_ctx(uh_pnp* p);
void** pnp_ransac_slot(uh_pnp* p, void (*free_fn)(void*));
int pnp_ransac_stage(const char* fn, uh_pnp* p, const float* intr4, int n_problems, const uh_ransac_problem* problems, uh_ransac_result* results, bool kp_on_device,
                     RansacStaged* sg);
}

namespace {

constexpr int kHypWaves = 4, kHypThreads = 64 * kHypWaves;
constexpr int kSelThreads = 256, kSelWaves = kSelThreads / 64;
constexpr int kIterBits = 10;   // UH_RANSAC_MAX_ITERS = 1 << kIterBits: a (count, iteration) key fits 31 bits up to 2^20 matches
static_assert(UH_RANSAC_MAX_ITERS == (1 << kIterBits), "the selection key packs the iteration into kIterBits bits");
static_assert((long long)UH_RANSAC_MAX_MATCHES << kIterBits < INT_MAX, "the selection key must fit an int");

struct PrProblemDev {
    int n, iters, m_off, s_off, h_off, words;   // offsets of the matches, samples and hypotheses in the concatenated arrays; mask words per hypothesis
    long long w_off;                            // first mask word of hypothesis 0
    float rt6_in[6];
    int pad[2];
};

struct PrOut { int ok, n_inliers, best_iter, pad; float rt6[6]; float pose[16]; };

struct PrArgs {
    float fx, fy, cx, cy;
    const PrProblemDev* prob;
    const float* p3d; const float* normal; const float* kp;   // all problems, concatenated
    const int* samples;                                        // 4 per hypothesis
    unsigned long long* mask;                                  // scratch: words per hypothesis
    float* hyp_rt6;                                            // scratch: 6 per hypothesis
    int* counts;                                               // result block: per hypothesis, -1 = skipped
    PrOut* out;                                                // result block: per problem
    int* inliers;                                              // result block: n per problem, at m_off
};

// The three-point pose of one sample on one wave: every lane leaves with the wave's number of solutions, the chosen solution's index
// (-1: skipped) and float rt[6]; lanes 0-3 also keep their own root's pose (valid says whether it is a solution).
struct HypPick { int n_solutions, chosen; };
// The other form the design weighed (measured in scripts/time_pnp_ransac.py, selected by uh_pnp_ransac_debug_form): every lane takes all
// four roots one after the other, no cross-lane step.  Same arithmetic in the same order per root, so the same rt[6] bit for bit.
__device__ __forceinline__ HypPick hyp_solve_uniform(const float* intr4, const float* P, const float* px, float* rt6) {
    p3p::Setup S;
    p3p::setup(intr4, P, px, S);
    double r0, r1, r2, r3;
    p3p::roots(S, r0, r1, r2, r3);
    int chosen = -1, n = 0;
    double best = INFINITY;
    p3p::Pose B{};
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const double v = k == 0 ? r0 : (k == 1 ? r1 : (k == 2 ? r2 : r3));
        p3p::Pose T;
        double e;
        if (p3p::back_substitute(S, v, T, e) && (v < INFINITY)) {
            if (e < best) { best = e; chosen = n; B = T; }
            n++;
        }
    }
    p3p::rt6_of(B, rt6);
    return {n, chosen};
}

__device__ __forceinline__ HypPick hyp_solve(const float* intr4, const float* P, const float* px, int lane, p3p::Pose& T, bool& valid, float* rt6,
                                             double& rx, double& ry, double& rz) {
    p3p::Setup S;
    p3p::setup(intr4, P, px, S);
    double r0, r1, r2, r3;
    p3p::roots(S, r0, r1, r2, r3);
    const int k = lane & 3;
    const double v = k == 0 ? r0 : (k == 1 ? r1 : (k == 2 ? r2 : r3));
    double e;
    valid = p3p::back_substitute(S, v, T, e) && (v < INFINITY);
    p3p::rodrigues(T, rx, ry, rz);
    float mine[6] = {(float)rx, (float)ry, (float)rz, (float)T.tx, (float)T.ty, (float)T.tz};
    int chosen_lane = -1, chosen = -1, n = 0;
    double best = INFINITY;
#pragma unroll
    for (int kk = 0; kk < 4; kk++) {
        const double ek = __shfl(e, kk, 64);
        const int vk = __shfl((int)valid, kk, 64);
        if (vk) {
            if (ek < best) { best = ek; chosen_lane = kk; chosen = n; }
            n++;
        }
    }
    const int src = chosen_lane < 0 ? 0 : chosen_lane;
#pragma unroll
    for (int c = 0; c < 6; c++) rt6[c] = __shfl(mine[c], src, 64);
    return {n, chosen};
}

template <bool UNIFORM_ROOTS>
__global__ __launch_bounds__(kHypThreads) void pr_hypothesis_kernel(PrArgs a) {
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
    const PrProblemDev& pb = a.prob[blockIdx.y];
    const int it = blockIdx.x * kHypWaves + wave;
    if (it >= pb.iters) return;
    const int n = pb.n, m_off = pb.m_off, h = pb.h_off + it;
    const int* s = a.samples + (size_t)pb.s_off + 4 * (size_t)it;
    const float intr4[4] = {a.fx, a.fy, a.cx, a.cy};
    float P[12], px[8];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const size_t g = (size_t)m_off + s[k];   // the host checked 0 <= s[k] < n
#pragma unroll
        for (int c = 0; c < 3; c++) P[3 * k + c] = a.p3d[3 * g + c];
        px[2 * k] = a.kp[2 * g]; px[2 * k + 1] = a.kp[2 * g + 1];
    }
    float rt6[6];
    HypPick pick;
    if (UNIFORM_ROOTS) {
        pick = hyp_solve_uniform(intr4, P, px, rt6);
    } else {
        p3p::Pose T;
        bool valid;
        double rx, ry, rz;
        pick = hyp_solve(intr4, P, px, lane, T, valid, rt6, rx, ry, rz);
    }
    if (pick.chosen < 0) {   // wave-uniform: cv::solvePnP returned false, the iteration is skipped
        if (lane == 0) a.counts[h] = -1;
        return;
    }
    p3p::M34 M;
    p3p::se3_set(rt6, M);
    float c0, c1, c2;
    p3p::cam_center(M, c0, c1, c2);
    unsigned long long* mask = a.mask + pb.w_off + (size_t)it * pb.words;
    int cnt = 0;
    for (int base = 0, w = 0; base < n; base += 64, w++) {
        const int j = base + lane;
        bool in = false;
        if (j < n) {
            const size_t g = (size_t)m_off + j;
            float e2, vc;
            in = p3p::inlier(M, a.fx, a.fy, a.cx, a.cy, c0, c1, c2, a.p3d[3 * g], a.p3d[3 * g + 1], a.p3d[3 * g + 2], a.normal[3 * g], a.normal[3 * g + 1],
                             a.normal[3 * g + 2], a.kp[2 * g], a.kp[2 * g + 1], e2, vc);
        }
        const unsigned long long b = __ballot(in);
        if (lane == 0) mask[w] = b;
        cnt += __popcll(b);
    }
    if (lane == 0) {
        a.counts[h] = cnt;
#pragma unroll
        for (int c = 0; c < 6; c++) a.hyp_rt6[6 * (size_t)h + c] = rt6[c];
    }
}

__device__ void write_out(PrOut& o, int n_inliers, int best_iter, const float* rt6) {
    o.ok = n_inliers >= 4 ? 1 : 0; o.n_inliers = n_inliers; o.best_iter = best_iter; o.pad = 0;
    float r[6];
    for (int c = 0; c < 6; c++) { r[c] = rt6[c]; o.rt6[c] = r[c]; }
    p3p::M34 M;
    p3p::se3_set(r, M);
    o.pose[0] = M.m0; o.pose[1] = M.m1; o.pose[2] = M.m2; o.pose[3] = M.m3; o.pose[4] = M.m4; o.pose[5] = M.m5; o.pose[6] = M.m6; o.pose[7] = M.m7;
    o.pose[8] = M.m8; o.pose[9] = M.m9; o.pose[10] = M.m10; o.pose[11] = M.m11; o.pose[12] = 0.f; o.pose[13] = 0.f; o.pose[14] = 0.f; o.pose[15] = 1.f;
}

__global__ __launch_bounds__(kSelThreads) void pr_select_kernel(PrArgs a) {
    __shared__ int s_key[kSelWaves];
    __shared__ int s_wave[kSelWaves];
    const PrProblemDev& pb = a.prob[blockIdx.x];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // the largest count, the lowest iteration among equals: one integer maximum
    int key = -1;
    for (int it = tid; it < pb.iters; it += kSelThreads) {
        const int c = a.counts[pb.h_off + it];
        if (c >= 1) key = max(key, (c << kIterBits) | ((1 << kIterBits) - 1 - it));
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) key = max(key, __shfl_xor(key, d, 64));
    if (lane == 0) s_key[wave] = key;
    __syncthreads();
    key = s_key[0];
#pragma unroll
    for (int w = 1; w < kSelWaves; w++) key = max(key, s_key[w]);
    PrOut& o = a.out[blockIdx.x];
    if (key < 0) {   // no hypothesis had an inlier: the pose comes back as it went in
        if (tid == 0) write_out(o, 0, -1, pb.rt6_in);
        return;
    }
    const int best = (1 << kIterBits) - 1 - (key & ((1 << kIterBits) - 1));
    const unsigned long long* mask = a.mask + pb.w_off + (size_t)best * pb.words;
    int* inl = a.inliers + pb.m_off;
    int base = 0;
    for (int first = 0; first < pb.words; first += kSelThreads) {
        const int w = first + tid;
        unsigned long long bits = w < pb.words ? mask[w] : 0ull;
        const int pc = __popcll(bits);
        int v = pc;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int u = __shfl_up(v, d, 64);
            if (lane >= d) v += u;
        }
        if (lane == 63) s_wave[wave] = v;
        __syncthreads();
        int before = 0, all = 0;
#pragma unroll
        for (int q = 0; q < kSelWaves; q++) { const int sw = s_wave[q]; all += sw; if (q < wave) before += sw; }
        __syncthreads();
        int at = base + before + v - pc;   // < pb.n: the mask has no bit at or beyond n
        while (bits) {
            const int b = __ffsll((long long)bits) - 1;
            inl[at++] = w * 64 + b;
            bits &= bits - 1;
        }
        base += all;
    }
    if (tid == 0) write_out(o, base, best, a.hyp_rt6 + 6 * (size_t)(pb.h_off + best));
}

struct PrDebugArgs { float intr4[4]; float P[12]; float px[8]; double* out; };   // out: 48 Rt | 6 rvec tvec | n_solutions | chosen

__global__ __launch_bounds__(64) void pr_debug_kernel(PrDebugArgs a) {
    const int lane = threadIdx.x;
    p3p::Pose T;
    bool valid;
    float rt6[6];
    double rx, ry, rz;
    const HypPick pick = hyp_solve(a.intr4, a.P, a.px, lane, T, valid, rt6, rx, ry, rz);
    const unsigned long long vm = __ballot(valid && lane < 4);
    if (lane < 4 && valid) {
        const int rank = __popcll(vm & ((1ull << lane) - 1));
        double* o = a.out + 12 * rank;
        o[0] = T.r00; o[1] = T.r01; o[2] = T.r02; o[3] = T.r10; o[4] = T.r11; o[5] = T.r12; o[6] = T.r20; o[7] = T.r21; o[8] = T.r22;
        o[9] = T.tx; o[10] = T.ty; o[11] = T.tz;
        if (rank == pick.chosen) { double* r = a.out + 48; r[0] = rx; r[1] = ry; r[2] = rz; r[3] = T.tx; r[4] = T.ty; r[5] = T.tz; }
    }
    if (lane == 0) { a.out[54] = pick.n_solutions; a.out[55] = pick.chosen; }
}

// test hook: lane i takes the quartic A[5 i .. 5 i + 4] (A0 .. A4) through roots() and writes its four roots (absent: +inf) and their number
__global__ __launch_bounds__(64) void pr_debug_roots_kernel(const double* A, int n, double* out) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    p3p::Setup S{};
    S.ok = true;
    S.A0 = A[5 * (size_t)i]; S.A1 = A[5 * (size_t)i + 1]; S.A2 = A[5 * (size_t)i + 2]; S.A3 = A[5 * (size_t)i + 3]; S.A4 = A[5 * (size_t)i + 4];
    double r0, r1, r2, r3;
    const int k = p3p::roots(S, r0, r1, r2, r3);
    double* o = out + 5 * (size_t)i;
    o[0] = r0; o[1] = r1; o[2] = r2; o[3] = r3; o[4] = k;
}

struct PrState {
    uh::DevBuf d_in, d_work, d_out;
    uh::PinBuf h_in, h_out;
    bool uniform_roots = false;   // measurement hook (uh_pnp_ransac_debug_form)
    // the staged batch (pnp_ransac_stage): the launches' arguments, where the blocks' parts lie, the upload's status
    PrArgs a{};
    int live = 0, max_iters = 0;
    size_t i_prob = 0, r_bytes = 0, r_out = 0, r_cnt = 0, r_inl = 0;
    hipError_t e = hipSuccess;
};
void pr_free(void* s) { delete static_cast<PrState*>(s); }
PrState* pr_state(uh_pnp* p) {
    void** slot = uh::pnp_ransac_slot(p, nullptr);
    if (!*slot) {
        slot = uh::pnp_ransac_slot(p, pr_free);   // the deleter is named once, with the state it deletes
        *slot = new PrState();
    }
    return static_cast<PrState*>(*slot);
}

int check_intr(const char* fn, const float* intr4) {
    UH_REQUIRE(intr4, "%s: NULL intrinsics", fn);
    for (int k = 0; k < 4; k++) UH_REQUIRE(std::isfinite(intr4[k]), "%s: non-finite intrinsics (intr4[%d] = %g)", fn, k, (double)intr4[k]);
    return UH_OK;
}

// what uh_pnp_ransac and the debug hook check of one problem before anything is launched
int check_problem(const char* fn, int j, const uh_ransac_problem& q, bool kp_on_device = false) {
    UH_REQUIRE(q.n >= 0 && q.n <= UH_RANSAC_MAX_MATCHES, "%s: problem %d: %d matches outside [0, %d]", fn, j, q.n, UH_RANSAC_MAX_MATCHES);
    UH_REQUIRE(q.iters >= 1 && q.iters <= UH_RANSAC_MAX_ITERS, "%s: problem %d: %d iterations outside [1, %d]", fn, j, q.iters, UH_RANSAC_MAX_ITERS);
    UH_REQUIRE(q.rt6_in, "%s: problem %d: NULL rt6_in", fn, j);
    if (q.n > 0) UH_REQUIRE(q.p3d && q.normal && (q.kp || kp_on_device), "%s: problem %d: NULL match arrays with n = %d", fn, j, q.n);
    if (q.n < 4) return UH_OK;
    UH_REQUIRE(q.samples, "%s: problem %d: NULL samples", fn, j);
    for (int it = 0; it < q.iters; it++) {
        const int32_t* s = q.samples + 4 * (size_t)it;
        for (int k = 0; k < 4; k++) {
            UH_REQUIRE(s[k] >= 0 && s[k] < q.n, "%s: problem %d iteration %d: sample index %d outside the %d matches", fn, j, it, s[k], q.n);
            for (int l = 0; l < k; l++) UH_REQUIRE(s[l] != s[k], "%s: problem %d iteration %d: index %d occurs twice in the sample", fn, j, it, s[k]);
        }
    }
    return UH_OK;
}

void host_pose(const float* rt6, float* pose16) {
    p3p::M34 M;
    p3p::se3_set(rt6, M);
    const float v[16] = {M.m0, M.m1, M.m2, M.m3, M.m4, M.m5, M.m6, M.m7, M.m8, M.m9, M.m10, M.m11, 0.f, 0.f, 0.f, 1.f};
    std::memcpy(pose16, v, sizeof(v));
}


// the two launches of a staged batch
hipError_t pr_launch(uh_pnp* p, PrState* st) {
    uh_ctx* ctx = uh::pnp_ctx(p);
    const PrArgs& a = st->a;
    const dim3 grid(uh_div_up(st->max_iters, kHypWaves), st->live);
    if (st->uniform_roots) UH_LAUNCH(ctx, pr_hypothesis_kernel<true>, grid, dim3(kHypThreads), 0, a);
    else UH_LAUNCH(ctx, pr_hypothesis_kernel<false>, grid, dim3(kHypThreads), 0, a);
    UH_LAUNCH(ctx, pr_select_kernel, dim3(st->live), dim3(kSelThreads), 0, a);
    return hipGetLastError();
}

// the results of the live problems (n >= 4) from the pinned result block
void pr_unpack(PrState* st, int n_problems, const uh_ransac_problem* problems, uh_ransac_result* results) {
    const char* ho = st->h_out.as<char>();
    const PrProblemDev* hp = (const PrProblemDev*)(st->h_in.as<char>() + st->i_prob);
    const PrOut* out = (const PrOut*)(ho + st->r_out);
    const int* cnt = (const int*)(ho + st->r_cnt);
    const int* inl = (const int*)(ho + st->r_inl);
    for (int j = 0, l = 0; j < n_problems; j++) {
        const uh_ransac_problem& q = problems[j];
        if (q.n < 4) continue;
        const PrProblemDev& d = hp[l];
        const PrOut& o = out[l++];
        uh_ransac_result& r = results[j];
        r.ok = o.ok; r.n_inliers = o.n_inliers; r.best_iter = o.best_iter;
        std::memcpy(r.rt6, o.rt6, sizeof(r.rt6));
        std::memcpy(r.pose, o.pose, sizeof(r.pose));
        if (o.n_inliers > 0 && r.inliers) std::memcpy(r.inliers, inl + d.m_off, sizeof(int) * (size_t)o.n_inliers);
        if (r.counts) std::memcpy(r.counts, cnt + d.h_off, sizeof(int) * (size_t)q.iters);
    }
}

}  // namespace

namespace uh {

// uh_pnp_ransac up to its upload, for `fn`: every check, the results of the problems below four matches, the packed block and its copy to
// the device enqueued (the copy's status stays in the state: the caller drains the stream on a failure, as it does for its launches).
// kp_on_device: the problems carry no keypoints; the caller fills d_kp on the stream before pnp_ransac_launch.  results may then be NULL.
int pnp_ransac_stage(const char* fn, uh_pnp* p, const float* intr4, int n_problems, const uh_ransac_problem* problems, uh_ransac_result* results, bool kp_on_device,
                     RansacStaged* sg) {
    *sg = RansacStaged{};
    // ---- everything the kernels will trust is checked here, before anything is launched (and before the solver object is touched)
    int rc;
    if ((rc = check_intr(fn, intr4))) return rc;
    UH_REQUIRE(n_problems >= 0 && n_problems <= UH_RANSAC_MAX_PROBLEMS, "%s: %d problems outside [0, %d]", fn, n_problems, UH_RANSAC_MAX_PROBLEMS);
    if (n_problems == 0) return UH_OK;
    UH_REQUIRE(problems && (results || kp_on_device), "%s: NULL problem or result array", fn);
    size_t N = 0, H = 0, Wd = 0;
    int live = 0, max_iters = 0;
    for (int j = 0; j < n_problems; j++) {
        const uh_ransac_problem& q = problems[j];
        if ((rc = check_problem(fn, j, q, kp_on_device))) return rc;
        if (results) UH_REQUIRE(results[j].cap >= q.n && (q.n == 0 || results[j].inliers), "%s: problem %d: inlier buffer of %d entries for %d matches", fn, j, results[j].cap, q.n);
        if (q.n < 4) continue;
        live++; N += (size_t)q.n; H += (size_t)q.iters; Wd += (size_t)q.iters * (size_t)uh_div_up(q.n, 64);
        max_iters = std::max(max_iters, q.iters);
    }
    for (int j = 0; results && j < n_problems; j++) {   // a problem below four matches: `matches_io.size() < 4 -> return false`, nothing is touched
        const uh_ransac_problem& q = problems[j];
        if (q.n >= 4) continue;
        uh_ransac_result& r = results[j];
        r.ok = 0; r.n_inliers = 0; r.best_iter = -1;
        std::memcpy(r.rt6, q.rt6_in, sizeof(r.rt6));
        host_pose(r.rt6, r.pose);
        if (r.counts) for (int it = 0; it < q.iters; it++) r.counts[it] = -1;
    }
    if (live == 0) return UH_OK;
    UH_REQUIRE(p, "%s: NULL solver", fn);
    PrState* st = pr_state(p);
    uh_ctx* ctx = uh::pnp_ctx(p);

    uh::Layout I;
    const size_t i_prob = I.take<PrProblemDev>(live, 16), i_p3d = I.take<float>(3 * N, 16), i_nrm = I.take<float>(3 * N, 16), i_kp = I.take<float>(2 * N, 16);
    const size_t i_smp = I.take<int>(4 * H, 16);
    const size_t i_bytes = (I.off + 15) & ~(size_t)15;
    uh::Layout R;
    const size_t r_out = R.take<PrOut>(live, 16), r_cnt = R.take<int>(H, 16), r_inl = R.take<int>(N, 16);
    const size_t r_bytes = (R.off + 15) & ~(size_t)15;
    uh::Layout W;
    const size_t w_mask = W.take<unsigned long long>(Wd, 16), w_rt = W.take<float>(6 * H, 16);
    if ((rc = st->h_in.reserve(i_bytes))) return rc;
    if ((rc = st->h_out.reserve(r_bytes))) return rc;
    UH_HIP_CHECK(hipSetDevice(ctx->device));
    if ((rc = st->d_in.reserve(i_bytes))) return rc;
    if ((rc = st->d_work.reserve(W.off))) return rc;
    if ((rc = st->d_out.reserve(r_bytes))) return rc;

    char* hi = st->h_in.as<char>();
    PrProblemDev* hp = (PrProblemDev*)(hi + i_prob);
    size_t m_off = 0, h_off = 0, w_off = 0;
    for (int j = 0, l = 0; j < n_problems; j++) {
        const uh_ransac_problem& q = problems[j];
        if (q.n < 4) continue;
        PrProblemDev& d = hp[l++];
        d.n = q.n; d.iters = q.iters; d.m_off = (int)m_off; d.s_off = (int)(4 * h_off); d.h_off = (int)h_off; d.words = uh_div_up(q.n, 64);
        d.w_off = (long long)w_off; d.pad[0] = d.pad[1] = 0;
        std::memcpy(d.rt6_in, q.rt6_in, sizeof(d.rt6_in));
        std::memcpy(hi + i_p3d + 12 * m_off, q.p3d, 12 * (size_t)q.n);
        std::memcpy(hi + i_nrm + 12 * m_off, q.normal, 12 * (size_t)q.n);
        if (!kp_on_device) std::memcpy(hi + i_kp + 8 * m_off, q.kp, 8 * (size_t)q.n);
        std::memcpy(hi + i_smp + 16 * h_off, q.samples, 16 * (size_t)q.iters);
        m_off += (size_t)q.n; h_off += (size_t)q.iters; w_off += (size_t)q.iters * (size_t)d.words;
    }
    char* di = st->d_in.as<char>();
    char* dw = st->d_work.as<char>();
    char* dout = st->d_out.as<char>();
    PrArgs a{};
    a.fx = intr4[0]; a.fy = intr4[1]; a.cx = intr4[2]; a.cy = intr4[3];
    a.prob = (const PrProblemDev*)(di + i_prob);
    a.p3d = (const float*)(di + i_p3d); a.normal = (const float*)(di + i_nrm); a.kp = (const float*)(di + i_kp); a.samples = (const int*)(di + i_smp);
    a.mask = (unsigned long long*)(dw + w_mask); a.hyp_rt6 = (float*)(dw + w_rt);
    a.out = (PrOut*)(dout + r_out); a.counts = (int*)(dout + r_cnt); a.inliers = (int*)(dout + r_inl);
    st->a = a; st->live = live; st->max_iters = max_iters;
    st->i_prob = i_prob; st->r_bytes = r_bytes; st->r_out = r_out; st->r_cnt = r_cnt; st->r_inl = r_inl;
    st->e = hipMemcpyAsync(di, hi, i_bytes, hipMemcpyHostToDevice, ctx->stream);
    static_assert(sizeof(RansacOut) == sizeof(PrOut), "RansacOut is PrOut as other units read it");
    sg->live = live; sg->d_out = reinterpret_cast<const RansacOut*>(a.out); sg->d_inliers = a.inliers; sg->d_kp = (float*)(di + i_kp);
    return UH_OK;
}

// the staged batch's two launches (its upload's status first); on a failure the caller drains the stream
int pnp_ransac_launch(uh_pnp* p) {
    PrState* st = pr_state(p);
    hipError_t e = st->e;
    if (e == hipSuccess) e = pr_launch(p, st);
    if (e != hipSuccess) { uh::set_error("uh_pnp_ransac: %s", hipGetErrorString(e)); return UH_ENODEVICE; }
    return UH_OK;
}

void pnp_ransac_host_pose(const float* rt6, float* pose16) { host_pose(rt6, pose16); }

}  // namespace uh

extern "C" {

int uh_pnp_ransac_samples(int n, int iters, int32_t* samples_out) {
    UH_REQUIRE(n >= 4 && iters >= 0 && samples_out, "uh_pnp_ransac_samples: n = %d (at least 4), iters = %d, or a NULL output", n, iters);
    std::vector<int32_t> idx((size_t)n);
    for (int i = 0; i < n; i++) idx[i] = i;
    for (int it = 0; it < iters; it++) {
        // std::random_shuffle of libstdc++ (stl_algo.h): for i = first + 1 .. last - 1: j = first + rand() % (i - first + 1); if (i != j) iter_swap(i, j)
        for (int i = 1; i < n; i++) {
            const int j = std::rand() % (i + 1);
            if (i != j) std::swap(idx[i], idx[j]);
        }
        for (int k = 0; k < 4; k++) samples_out[4 * (size_t)it + k] = idx[k];
    }
    return UH_OK;
}

int uh_pnp_ransac(uh_pnp* p, const float* intr4, int n_problems, const uh_ransac_problem* problems, uh_ransac_result* results) {
    uh::RansacStaged sg;
    int rc;
    if ((rc = uh::pnp_ransac_stage("uh_pnp_ransac", p, intr4, n_problems, problems, results, false, &sg))) return rc;
    if (sg.live == 0) return UH_OK;
    PrState* st = pr_state(p);
    // ---- one chain on the context's stream, one wait.  After the first enqueue every failure drains the stream before it returns:
    // the pinned blocks are rewritten by the next call.
    hipStream_t s = uh::pnp_ctx(p)->stream;
    hipError_t e = st->e;
    if (e == hipSuccess) e = pr_launch(p, st);
    if (e == hipSuccess) e = hipMemcpyAsync(st->h_out.p, st->d_out.p, st->r_bytes, hipMemcpyDeviceToHost, s);
    const hipError_t es = hipStreamSynchronize(s);
    if (e == hipSuccess) e = es;
    if (e != hipSuccess) {
        uh::set_error("uh_pnp_ransac: %s", hipGetErrorString(e));
        return UH_ENODEVICE;
    }
    pr_unpack(st, n_problems, problems, results);
    return UH_OK;
}

int uh_pnp_ransac_debug_form(uh_pnp* p, int uniform_roots) {
    UH_REQUIRE(p, "uh_pnp_ransac_debug_form: NULL solver");
    pr_state(p)->uniform_roots = uniform_roots != 0;
    return UH_OK;
}

int uh_pnp_ransac_debug_hypothesis(uh_pnp* p, const float* intr4, const uh_ransac_problem* q, int iter, int32_t* n_solutions, double* Rt_4x12, int32_t* chosen,
                                   double* rvec_tvec6) {
    int rc;
    if ((rc = check_intr("uh_pnp_ransac_debug_hypothesis", intr4))) return rc;
    UH_REQUIRE(q && n_solutions && Rt_4x12 && chosen && rvec_tvec6, "uh_pnp_ransac_debug_hypothesis: NULL argument");
    if ((rc = check_problem("uh_pnp_ransac_debug_hypothesis", 0, *q))) return rc;
    UH_REQUIRE(q->n >= 4 && iter >= 0 && iter < q->iters, "uh_pnp_ransac_debug_hypothesis: n = %d below 4, or iteration %d outside [0, %d)", q->n, iter, q->iters);
    UH_REQUIRE(p, "uh_pnp_ransac_debug_hypothesis: NULL solver");
    PrState* st = pr_state(p);
    uh_ctx* ctx = uh::pnp_ctx(p);
    UH_HIP_CHECK(hipSetDevice(ctx->device));
    constexpr size_t kBytes = 56 * sizeof(double);
    if ((rc = st->d_out.reserve(kBytes))) return rc;
    PrDebugArgs a{};
    for (int k = 0; k < 4; k++) {
        a.intr4[k] = intr4[k];
        const int i = q->samples[4 * (size_t)iter + k];
        for (int c = 0; c < 3; c++) a.P[3 * k + c] = q->p3d[3 * (size_t)i + c];
        a.px[2 * k] = q->kp[2 * (size_t)i]; a.px[2 * k + 1] = q->kp[2 * (size_t)i + 1];
    }
    a.out = st->d_out.as<double>();
    double h[56];
    hipError_t e = hipMemsetAsync(a.out, 0, kBytes, ctx->stream);
    if (e == hipSuccess) {
        UH_LAUNCH(ctx, pr_debug_kernel, dim3(1), dim3(64), 0, a);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(h, a.out, kBytes, hipMemcpyDeviceToHost, ctx->stream);
    const hipError_t es = hipStreamSynchronize(ctx->stream);
    if (e == hipSuccess) e = es;
    if (e != hipSuccess) {
        uh::set_error("uh_pnp_ransac_debug_hypothesis: %s", hipGetErrorString(e));
        return UH_ENODEVICE;
    }
    std::memcpy(Rt_4x12, h, 48 * sizeof(double));
    std::memcpy(rvec_tvec6, h + 48, 6 * sizeof(double));
    *n_solutions = (int32_t)h[54];
    *chosen = (int32_t)h[55];
    return UH_OK;
}

int uh_pnp_ransac_debug_roots(uh_pnp* p, int n, const double* A_nx5, double* roots_nx4, int32_t* n_roots) {
    UH_REQUIRE(n >= 0 && n <= UH_RANSAC_MAX_ITERS, "uh_pnp_ransac_debug_roots: %d quartics outside [0, %d]", n, UH_RANSAC_MAX_ITERS);
    if (n == 0) return UH_OK;
    UH_REQUIRE(A_nx5 && roots_nx4 && n_roots, "uh_pnp_ransac_debug_roots: NULL argument");
    UH_REQUIRE(p, "uh_pnp_ransac_debug_roots: NULL solver");
    PrState* st = pr_state(p);
    uh_ctx* ctx = uh::pnp_ctx(p);
    UH_HIP_CHECK(hipSetDevice(ctx->device));
    int rc;
    const size_t bytes = 5 * (size_t)n * sizeof(double);
    if ((rc = st->d_in.reserve(bytes))) return rc;
    if ((rc = st->d_out.reserve(bytes))) return rc;
    std::vector<double> h(5 * (size_t)n);
    double* dA = st->d_in.as<double>();
    double* dout = st->d_out.as<double>();
    hipError_t e = hipMemcpyAsync(dA, A_nx5, bytes, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) {
        UH_LAUNCH(ctx, pr_debug_roots_kernel, dim3(uh_div_up(n, 64)), dim3(64), 0, (const double*)dA, n, dout);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(h.data(), dout, bytes, hipMemcpyDeviceToHost, ctx->stream);
    const hipError_t es = hipStreamSynchronize(ctx->stream);   // A_nx5 is pageable caller memory: nothing is left in flight
    if (e == hipSuccess) e = es;
    if (e != hipSuccess) {
        uh::set_error("uh_pnp_ransac_debug_roots: %s", hipGetErrorString(e));
        return UH_ENODEVICE;
    }
    for (int i = 0; i < n; i++) {
        for (int k = 0; k < 4; k++) roots_nx4[4 * (size_t)i + k] = h[5 * (size_t)i + k];
        n_roots[i] = (int32_t)h[5 * (size_t)i + 4];
    }
    return UH_OK;
}

}  // extern "C"
