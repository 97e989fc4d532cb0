// Map initialiser on the device (uh_mapinit_run): MapInitializer's two-view initialise, src/utils/mapinitializer.cpp:152-201, in two
// launches.  The contract is in include/ucoslam_hip.h, the arithmetic in mapinit_math.hpp (one text for device and host).
//
//   host     normalises both frames (sequential float sums over all keypoints), checks every index, gathers the matched coordinates
//            (x1, y1, x2, y2 per match: the kernels never index a keypoint array), packs one pinned block: ONE upload
//   mi_hypothesis_kernel   one wave (= one workgroup) per (model, iteration): lanes 0-7 write the rows of their sample into the
//            double workspace in LDS, the wave finds the null vector by a one-sided Jacobi with the rows spread over the lanes, every
//            lane de-normalises (H also inverts, F projects to rank 2 first), then the lanes stride over the matches: per 64 matches
//            one ballot word into the hypothesis' mask and the 128 terms added IN MATCH ORDER (cross-lane reads, lane 0 .. 63, two
//            terms each): the reference's sequential float sum, not a tree.
//   mi_reconstruct_kernel  one workgroup of eight waves: first strict maximum of each model's scores (every thread scans them: no
//            atomics), RH, the decomposition on every lane, candidate c on wave c (CheckRT over the winner's inliers), the order
//            statistic of the cosines by a bitwise radix selection on ordered keys, the decision, and the winner's states / points.
//   host     ONE download, ONE wait; the per-keypoint scatter in match order.
// No atomics and no float reductions: the result is a function of the input alone.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include "common.hpp"
#include "mapinit_math.hpp"

struct uh_mapinit {
    uh_ctx* ctx = nullptr;
    uh::DevBuf d_in, d_work, d_out;
    uh::PinBuf h_in, h_out;
};

namespace {

constexpr int kRecWaves = 8, kRecThreads = 64 * kRecWaves;

struct MiHead {   // what is uniform over one call
    float intr4[4];
    float T1[9], T2inv[9], T2t[9];
    mim::Norm N1, N2;
    float inv_sigma2, th2, min_parallax;
    int n, iters, words, min_triangulated;
};
struct MiOut {
    int ok, model, winner, best_h, best_f, n_cand, N, pad;
    float sh, sf, rh, pad2;
    int n_good[8];
    float parallax[8];
    float R[9], t[3];
};
struct MiArgs {
    const MiHead* head;
    const float4* xy;                 // n: x1, y1, x2, y2
    const int* samples;               // 8 per iteration
    unsigned long long* mask;         // work: words per hypothesis, H hypotheses first
    float* score;                     // work: 2 * iters
    float* mat;                       // work: 9 per hypothesis
    double* nullvec;                  // work: 9 per hypothesis
    uint8_t* c_state;                 // work: 8 x n
    float* c_cos;                     // work: 8 x n
    float* c_pt;                      // work: 8 x n x 3
    MiOut* out;                       // result block
    uint8_t* state;                   // result block: n
    float* pt;                        // result block: n x 3
};

__global__ __launch_bounds__(64) void mi_hypothesis_kernel(MiArgs a) {
    __shared__ double W[mim::kWsRowsH * 9];
    const MiHead& hd = *a.head;
    const int lane = threadIdx.x, h = blockIdx.x, iters = hd.iters, n = hd.n;
    const bool is_h = h < iters;
    const int it = is_h ? h : h - iters;
    if (lane < 8) {
        const float4 m = a.xy[a.samples[8 * it + lane]];   // the host checked 0 <= sample < n
        float u1, v1, u2, v2;
        mim::normalised_point(hd.N1, m.x, m.y, u1, v1);
        mim::normalised_point(hd.N2, m.z, m.w, u2, v2);
        if (is_h) mim::h_rows(W, lane, u1, v1, u2, v2);
        else mim::f_row(W, lane, u1, v1, u2, v2);
    }
    __syncthreads();
    double x[9];
    mim::null_vector9(W, is_h ? 16 : 8, lane, 64, x);
    float M[9], Minv[9];
    if (is_h) mim::h_model(x, hd.T1, hd.T2inv, M, Minv);
    else mim::f_model(x, hd.T1, hd.T2t, M);
    unsigned long long* mask = a.mask + (size_t)h * hd.words;
    const float inv_sigma2 = hd.inv_sigma2;
    float score = 0.f;
    for (int base = 0, w = 0; base < n; base += 64, w++) {
        const int j = base + lane;
        bool in = false;
        float t1 = 0.f, t2 = 0.f;
        if (j < n) {
            const float4 m = a.xy[j];
            in = is_h ? mim::check_h(M, Minv, inv_sigma2, m.x, m.y, m.z, m.w, t1, t2) : mim::check_f(M, inv_sigma2, m.x, m.y, m.z, m.w, t1, t2);
        }
        const unsigned long long b = __ballot(in);
        if (lane == 0) mask[w] = b;
#pragma unroll
        for (int l = 0; l < 64; l++) {   // match order: lane l's two terms after lane l - 1's
            score += __shfl(t1, l, 64);
            score += __shfl(t2, l, 64);
        }
    }
    if (lane == 0) {
        a.score[h] = score;
#pragma unroll
        for (int k = 0; k < 9; k++) { a.mat[9 * (size_t)h + k] = M[k]; a.nullvec[9 * (size_t)h + k] = x[k]; }
    }
}

// the first strictly largest score above 0 (`if (currentScore > score)` from score = 0), every thread alike
__device__ __forceinline__ int first_best(const float* s, int iters, float& best) {
    int at = -1;
    best = 0.f;
    for (int it = 0; it < iters; it++) {
        const float v = s[it];
        if (v > best) { best = v; at = it; }
    }
    return at;
}

__global__ __launch_bounds__(kRecThreads) void mi_reconstruct_kernel(MiArgs a) {
    __shared__ float s_R[8][9];
    __shared__ float s_t[8][3];
    __shared__ int s_good[8];
    __shared__ float s_par[8];
    __shared__ int s_N;
    __shared__ int s_sel[3];   // model, chosen hypothesis (-1: none), candidates
    const MiHead& hd = *a.head;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int n = hd.n, iters = hd.iters, words = hd.words;
    MiOut& o = *a.out;
    if (wave == 0) {   // the selection and the decomposition once, every lane of wave 0 alike; the other waves take the result from LDS
        float sh, sf, rh;
        const int best_h = first_best(a.score, iters, sh), best_f = first_best(a.score + iters, iters, sf);
        const int model = mim::choose_model(sh, sf, rh);
        const int hyp = model == mim::kHomography ? best_h : (best_f < 0 ? -1 : iters + best_f);
        mim::Candidates C;
        C.n = 0;
        if (hyp >= 0) {
            float M[9], d3[3];
#pragma unroll
            for (int k = 0; k < 9; k++) M[k] = a.mat[9 * (size_t)hyp + k];
            if (model == mim::kHomography) mim::decompose_h(M, hd.intr4, C, d3);
            else mim::decompose_f(M, hd.intr4, C);
        }
        if (lane == 0) {
            o.ok = 0; o.model = model; o.winner = -1; o.best_h = best_h; o.best_f = best_f; o.n_cand = 0; o.N = 0; o.pad = 0;
            o.sh = sh; o.sf = sf; o.rh = rh; o.pad2 = 0.f;
            for (int c = 0; c < 8; c++) { o.n_good[c] = 0; o.parallax[c] = 0.f; }
            for (int k = 0; k < 9; k++) o.R[k] = 0.f;
            for (int k = 0; k < 3; k++) o.t[k] = 0.f;
            s_sel[0] = model; s_sel[1] = hyp; s_sel[2] = C.n;
#pragma unroll
            for (int c = 0; c < 8; c++) {
#pragma unroll
                for (int k = 0; k < 9; k++) s_R[c][k] = c < C.n ? C.R[c][k] : 0.f;
#pragma unroll
                for (int k = 0; k < 3; k++) s_t[c][k] = c < C.n ? C.t[c][k] : 0.f;
            }
        }
    }
    __syncthreads();
    const int model = s_sel[0], hyp = s_sel[1], n_cand = s_sel[2];
    if (hyp < 0) {   // no hypothesis of the chosen model scored: nothing to decompose
        for (int j = tid; j < n; j += kRecThreads) { a.state[j] = mim::kNotInlier; a.pt[3 * j] = 0.f; a.pt[3 * j + 1] = 0.f; a.pt[3 * j + 2] = 0.f; }
        return;
    }
    const unsigned long long* mask = a.mask + (size_t)hyp * words;
    uint8_t* st = a.c_state + (size_t)wave * n;
    float* cs = a.c_cos + (size_t)wave * n;
    float* pt = a.c_pt + 3 * (size_t)wave * n;
    int N = 0, good = 0;
    float par = 0.f;
    if (wave < n_cand) {
        float R[9], t[3];
#pragma unroll
        for (int k = 0; k < 9; k++) R[k] = s_R[wave][k];
#pragma unroll
        for (int k = 0; k < 3; k++) t[k] = s_t[wave][k];
        mim::RtConst Q;
        mim::make_rt_const(hd.intr4, R, t, hd.th2, Q);
        for (int base = 0, w = 0; base < n; base += 64, w++) {
            const unsigned long long bits = mask[w];
            N += __popcll(bits);
            const int j = base + lane;
            uint8_t s = mim::kNotInlier;
            float cosp = 0.f, p[3] = {0.f, 0.f, 0.f};
            if (j < n && ((bits >> lane) & 1ull)) {
                const float4 m = a.xy[j];
                s = mim::check_rt(Q, m.x, m.y, m.z, m.w, cosp, p);
            }
            const bool counted = s == mim::kCountedGood || s == mim::kCountedLowParallax;
            good += __popcll(__ballot(counted));
            if (j < n) { st[j] = s; cs[j] = cosp; pt[3 * j] = p[0]; pt[3 * j + 1] = p[1]; pt[3 * j + 2] = p[2]; }
        }
        if (good > 0) {
            // the order statistic min(50, good - 1) of the counted cosines: one bit of its ordered key per pass, from the top.  Lane l
            // reads back the entries l, l + 64, ... that it wrote itself.
            int k = min(50, good - 1);
            uint32_t prefix = 0;
            for (int bit = 31; bit >= 0; bit--) {
                const uint32_t himask = bit == 31 ? 0u : ~((2u << bit) - 1u);
                int zeros = 0;
                for (int base = 0; base < n; base += 64) {
                    const int j = base + lane;
                    bool z = false;
                    if (j < n) {
                        const uint8_t s = st[j];
                        if (s == mim::kCountedGood || s == mim::kCountedLowParallax) {
                            const uint32_t key = mim::float_key(cs[j]);
                            z = (key & himask) == prefix && !((key >> bit) & 1u);
                        }
                    }
                    zeros += __popcll(__ballot(z));
                }
                if (k >= zeros) { k -= zeros; prefix |= 1u << bit; }
            }
            par = mim::parallax_of(mim::key_float(prefix));
        }
    }
    if (lane == 0) { s_good[wave] = good; s_par[wave] = par; }
    if (tid == 0) s_N = N;   // wave 0 is a candidate's wave unless n_cand = 0, where N stays 0
    __syncthreads();
    N = s_N;
    int winner;
    const bool ok = mim::decide(model, n_cand, N, s_good, s_par, hd.min_parallax, hd.min_triangulated, winner);
    if (tid == 0) {
        o.ok = ok ? 1 : 0; o.winner = winner; o.n_cand = n_cand; o.N = N;
        for (int c = 0; c < 8; c++) { o.n_good[c] = s_good[c]; o.parallax[c] = s_par[c]; }
        if (winner >= 0) {
            for (int k = 0; k < 9; k++) o.R[k] = s_R[winner][k];
            for (int k = 0; k < 3; k++) o.t[k] = s_t[winner][k];
        }
    }
    // every wave has finished its own rows before the barrier above; the winner's rows are read by all.  The rows are global memory written
    // by another wave of this ONE workgroup: __syncthreads() is a barrier with a workgroup-scope release / acquire fence, which covers global
    // memory too (the waves share a compute unit and its L1).  A second workgroup could not read them without a device-scope fence.
    const uint8_t* wst = a.c_state + (size_t)(winner < 0 ? 0 : winner) * n;
    const float* wpt = a.c_pt + 3 * (size_t)(winner < 0 ? 0 : winner) * n;
    for (int j = tid; j < n; j += kRecThreads) {
        const bool have = winner >= 0;
        a.state[j] = have ? wst[j] : (uint8_t)mim::kNotInlier;
        a.pt[3 * j] = have ? wpt[3 * j] : 0.f; a.pt[3 * j + 1] = have ? wpt[3 * j + 1] : 0.f; a.pt[3 * j + 2] = have ? wpt[3 * j + 2] : 0.f;
    }
}

// ---------------------------------------------------------------------------------------------------------------- host side

struct Prepared {
    MiHead head;
    std::vector<float> xy;        // 4 n
    std::vector<int32_t> samples; // 8 iters
    bool too_few = false;
};

int draw_samples(int n, int iterations, int32_t* out) {
    std::vector<int32_t> all((size_t)n), avail;
    for (int i = 0; i < n; i++) all[i] = i;
    std::srand(0);
    for (int it = 0; it < iterations; it++) {
        avail = all;
        for (int j = 0; j < 8; j++) {
            const int r = std::rand() % (int)avail.size();
            out[8 * (size_t)it + j] = avail[r];
            avail[r] = avail.back();
            avail.pop_back();
        }
    }
    return UH_OK;
}

// everything the kernels (and the host form) will trust is checked here
int prepare(const char* fn, const uh_mapinit_args* a, const uh_mapinit_result* r, Prepared& P) {
    UH_REQUIRE(a && r, "%s: NULL args or result", fn);
    UH_REQUIRE(a->intr4, "%s: NULL intrinsics", fn);
    for (int k = 0; k < 4; k++) UH_REQUIRE(std::isfinite(a->intr4[k]), "%s: non-finite intrinsics (intr4[%d] = %g)", fn, k, (double)a->intr4[k]);
    UH_REQUIRE(std::isfinite(a->sigma) && a->sigma > 0, "%s: sigma = %g", fn, (double)a->sigma);
    UH_REQUIRE(a->min_matches >= 8, "%s: min_matches = %d below 8", fn, a->min_matches);
    UH_REQUIRE(a->iterations >= 1 && a->iterations <= UH_MAPINIT_MAX_ITERS, "%s: %d iterations outside [1, %d]", fn, a->iterations, UH_MAPINIT_MAX_ITERS);
    UH_REQUIRE(a->n_matches >= 0 && a->n_matches <= UH_MAPINIT_MAX_MATCHES, "%s: %d matches outside [0, %d]", fn, a->n_matches, UH_MAPINIT_MAX_MATCHES);
    UH_REQUIRE(a->n_kp1 >= 0 && a->n_kp2 >= 0 && (a->n_kp1 == 0 || a->kp1) && (a->n_kp2 == 0 || a->kp2), "%s: NULL keypoint array or negative count", fn);
    UH_REQUIRE(a->n_matches == 0 || a->matches, "%s: NULL matches", fn);
    UH_REQUIRE(r->cap_matches >= a->n_matches && (a->n_matches == 0 || (r->matches_out && r->points_out)),
               "%s: result buffers of %d entries for %d matches", fn, r->cap_matches, a->n_matches);
    const int n = a->n_matches;
    P.too_few = n < a->min_matches;
    if (P.too_few) return UH_OK;
    P.xy.resize(4 * (size_t)n);
    for (int j = 0; j < n; j++) {
        const int tr = a->matches[2 * j], qu = a->matches[2 * j + 1];
        UH_REQUIRE(tr >= 0 && tr < a->n_kp1, "%s: match %d: trainIdx %d outside the %d keypoints of the reference frame", fn, j, tr, a->n_kp1);
        UH_REQUIRE(qu >= 0 && qu < a->n_kp2, "%s: match %d: queryIdx %d outside the %d keypoints of the second frame", fn, j, qu, a->n_kp2);
        P.xy[4 * (size_t)j] = a->kp1[2 * (size_t)tr]; P.xy[4 * (size_t)j + 1] = a->kp1[2 * (size_t)tr + 1];
        P.xy[4 * (size_t)j + 2] = a->kp2[2 * (size_t)qu]; P.xy[4 * (size_t)j + 3] = a->kp2[2 * (size_t)qu + 1];
    }
    P.samples.resize(8 * (size_t)a->iterations);
    if (a->samples) {
        for (size_t k = 0; k < P.samples.size(); k++) {
            UH_REQUIRE(a->samples[k] >= 0 && a->samples[k] < n, "%s: iteration %zu: sample index %d outside the %d matches", fn, k / 8, a->samples[k], n);
            P.samples[k] = a->samples[k];
        }
    } else {
        draw_samples(n, a->iterations, P.samples.data());
    }
    MiHead& h = P.head;
    std::memset(&h, 0, sizeof(h));
    std::memcpy(h.intr4, a->intr4, sizeof(h.intr4));
    mim::normalise(a->kp1, a->n_kp1, h.N1);
    mim::normalise(a->kp2, a->n_kp2, h.N2);
    std::memcpy(h.T1, h.N1.T, sizeof(h.T1));
    mim::inv3(h.N2.T, h.T2inv);
    mim::transpose3(h.N2.T, h.T2t);
    h.inv_sigma2 = mim::inv_sigma_square(a->sigma);
    const float sigma2 = a->sigma * a->sigma;
    h.th2 = (float)(4.0 * sigma2);
    h.min_parallax = a->min_parallax;
    h.n = n; h.iters = a->iterations; h.words = uh_div_up(n, 64); h.min_triangulated = a->min_triangulated;
    return UH_OK;
}

void clear_result(const uh_mapinit_args* a, uh_mapinit_result* r) {
    r->ok = 0; r->model = UH_MAPINIT_NONE; r->winner = -1; r->best_h = r->best_f = -1;
    r->score_h = r->score_f = r->rh = 0.f;
    r->n_candidates = r->n_inliers = 0;
    for (int c = 0; c < 8; c++) { r->n_good[c] = 0; r->parallax[c] = 0.f; }
    std::memset(r->R, 0, sizeof(r->R)); std::memset(r->t, 0, sizeof(r->t)); std::memset(r->pose, 0, sizeof(r->pose));
    r->n_out = 0;
    if (r->triangulated) std::memset(r->triangulated, 0, (size_t)a->n_kp1);
    if (r->p3d) std::memset(r->p3d, 0, 12 * (size_t)a->n_kp1);
    if (r->state) std::memset(r->state, 0, (size_t)a->n_matches);
}

// from the launch's (or the host form's) outputs to the caller's result: the scatter of :677-725 and the removal of :195-198, in match order
void finish(const uh_mapinit_args* a, const MiOut& o, const uint8_t* state, const float* pt, uh_mapinit_result* r) {
    clear_result(a, r);
    r->ok = o.ok; r->model = o.model; r->winner = o.winner; r->best_h = o.best_h; r->best_f = o.best_f;
    r->score_h = o.sh; r->score_f = o.sf; r->rh = o.rh; r->n_candidates = o.n_cand; r->n_inliers = o.N;
    for (int c = 0; c < 8; c++) { r->n_good[c] = o.n_good[c]; r->parallax[c] = o.parallax[c]; }
    const int n = a->n_matches;
    if (r->state) std::memcpy(r->state, state, (size_t)n);
    if (!o.ok) return;
    std::memcpy(r->R, o.R, sizeof(r->R)); std::memcpy(r->t, o.t, sizeof(r->t));
    const float md = a->min_distance;
    const float pose[16] = {o.R[0], o.R[1], o.R[2], o.t[0] * md, o.R[3], o.R[4], o.R[5], o.t[1] * md, o.R[6], o.R[7], o.R[8], o.t[2] * md, 0.f, 0.f, 0.f, 1.f};
    std::memcpy(r->pose, pose, sizeof(pose));
    std::vector<uint8_t> tri((size_t)a->n_kp1, 0);
    std::vector<float> p3d(3 * (size_t)a->n_kp1, 0.f);
    for (int j = 0; j < n; j++) {
        const size_t tr = (size_t)a->matches[2 * j];
        const uint8_t s = state[j];
        if (s == mim::kNonFinite) tri[tr] = 0;
        if (s == mim::kCountedGood || s == mim::kCountedLowParallax) std::memcpy(&p3d[3 * tr], pt + 3 * (size_t)j, 12);
        if (s == mim::kCountedGood) tri[tr] = 1;
    }
    int m = 0;
    for (int j = 0; j < n; j++) {
        const size_t tr = (size_t)a->matches[2 * j];
        if (!tri[tr]) continue;
        r->matches_out[2 * m] = a->matches[2 * j]; r->matches_out[2 * m + 1] = a->matches[2 * j + 1];
        if (r->index_out) r->index_out[m] = j;
        std::memcpy(r->points_out + 3 * (size_t)m, &p3d[3 * tr], 12);
        m++;
    }
    r->n_out = m;
    if (r->triangulated) std::memcpy(r->triangulated, tri.data(), tri.size());
    if (r->p3d) std::memcpy(r->p3d, p3d.data(), 4 * p3d.size());
}

// ---- the host form: the same header text, loops where the kernels have lanes
struct HostHyp { float M[9]; double x[9]; float score; };
void host_hypothesis(const Prepared& P, bool is_h, int it, HostHyp& H, unsigned long long* mask) {
    const MiHead& hd = P.head;
    double W[mim::kWsRowsH * 9];
    for (int k = 0; k < 8; k++) {
        const float* m = &P.xy[4 * (size_t)P.samples[8 * (size_t)it + k]];
        float u1, v1, u2, v2;
        mim::normalised_point(hd.N1, m[0], m[1], u1, v1);
        mim::normalised_point(hd.N2, m[2], m[3], u2, v2);
        if (is_h) mim::h_rows(W, k, u1, v1, u2, v2);
        else mim::f_row(W, k, u1, v1, u2, v2);
    }
    mim::null_vector9(W, is_h ? 16 : 8, 0, 1, H.x);
    float Minv[9];
    if (is_h) mim::h_model(H.x, hd.T1, hd.T2inv, H.M, Minv);
    else mim::f_model(H.x, hd.T1, hd.T2t, H.M);
    for (int w = 0; w < hd.words; w++) mask[w] = 0;
    float score = 0.f;
    for (int j = 0; j < hd.n; j++) {
        const float* m = &P.xy[4 * (size_t)j];
        float t1, t2;
        const bool in = is_h ? mim::check_h(H.M, Minv, hd.inv_sigma2, m[0], m[1], m[2], m[3], t1, t2) : mim::check_f(H.M, hd.inv_sigma2, m[0], m[1], m[2], m[3], t1, t2);
        if (in) mask[j >> 6] |= 1ull << (j & 63);
        score += t1;
        score += t2;
    }
    H.score = score;
}

// what mi_reconstruct_kernel does, from each model's winning hypothesis (o.best_h, o.best_f, o.sh, o.sf are set; best[m] / best_mask[m]
// are read for the chosen model alone)
void host_reconstruct(const Prepared& P, const HostHyp* best, const std::vector<unsigned long long>* best_mask, MiOut& o, std::vector<uint8_t>& state,
                      std::vector<float>& pt) {
    const MiHead& hd = P.head;
    const int n = hd.n, words = hd.words;
    state.assign((size_t)n, 0); pt.assign(3 * (size_t)n, 0.f);
    o.winner = -1;
    o.model = mim::choose_model(o.sh, o.sf, o.rh);
    const int m = o.model == mim::kHomography ? 0 : 1;
    if ((m == 0 ? o.best_h : o.best_f) < 0) return;
    mim::Candidates C;
    float d3[3];
    if (m == 0) mim::decompose_h(best[0].M, hd.intr4, C, d3);
    else mim::decompose_f(best[1].M, hd.intr4, C);
    o.n_cand = C.n;
    std::vector<uint8_t> c_state[8];
    std::vector<float> c_pt[8];
    int N = 0;
    for (int w = 0; w < words; w++) N += __builtin_popcountll(best_mask[m][w]);
    o.N = C.n ? N : 0;
    for (int c = 0; c < C.n; c++) {
        mim::RtConst Q;
        mim::make_rt_const(hd.intr4, C.R[c], C.t[c], hd.th2, Q);
        c_state[c].assign((size_t)n, 0); c_pt[c].assign(3 * (size_t)n, 0.f);
        std::vector<float> cosines;
        for (int j = 0; j < n; j++) {
            if (!((best_mask[m][j >> 6] >> (j & 63)) & 1ull)) continue;
            const float* q = &P.xy[4 * (size_t)j];
            float cosp;
            const uint8_t s = mim::check_rt(Q, q[0], q[1], q[2], q[3], cosp, &c_pt[c][3 * (size_t)j]);
            c_state[c][j] = s;
            if (s == mim::kCountedGood || s == mim::kCountedLowParallax) cosines.push_back(cosp);
        }
        o.n_good[c] = (int)cosines.size();
        if (!cosines.empty()) {
            // the order statistic on the ordered keys, as the device selects it (a NaN cosine has a place in this order too)
            std::vector<uint32_t> keys;
            for (float v : cosines) keys.push_back(mim::float_key(v));
            std::sort(keys.begin(), keys.end());
            o.parallax[c] = mim::parallax_of(mim::key_float(keys[std::min<size_t>(50, keys.size() - 1)]));
        }
    }
    int winner;
    o.ok = mim::decide(o.model, C.n, N, o.n_good, o.parallax, hd.min_parallax, hd.min_triangulated, winner) ? 1 : 0;
    o.winner = winner;
    if (winner >= 0) {
        std::memcpy(o.R, C.R[winner], sizeof(o.R)); std::memcpy(o.t, C.t[winner], sizeof(o.t));
        state = c_state[winner]; pt = c_pt[winner];
    }
}

void host_run(const Prepared& P, MiOut& o, std::vector<uint8_t>& state, std::vector<float>& pt) {
    const int iters = P.head.iters;
    std::memset(&o, 0, sizeof(o));
    std::vector<unsigned long long> cur((size_t)P.head.words), best_mask[2];
    HostHyp best[2];
    int best_at[2] = {-1, -1};
    float best_score[2] = {0.f, 0.f};
    for (int m = 0; m < 2; m++)
        for (int it = 0; it < iters; it++) {
            HostHyp H;
            host_hypothesis(P, m == 0, it, H, cur.data());
            if (H.score > best_score[m]) { best_score[m] = H.score; best_at[m] = it; best[m] = H; best_mask[m] = cur; }
        }
    o.best_h = best_at[0]; o.best_f = best_at[1]; o.sh = best_score[0]; o.sf = best_score[1];
    host_reconstruct(P, best, best_mask, o, state, pt);
}

// upload and the hypothesis launch (and the reconstruction where asked), the download of the result block, one wait
struct Blocks { size_t w_mask, w_score, w_mat, w_null, r_out, r_state, r_pt, r_bytes; };
// (test hook) one hypothesis per model written by the host in place of the hypothesis launch: iters = 1
struct Planted { float score[2]; float mat[18]; std::vector<unsigned long long> mask; /* 2 x words */ };
int device_run(const char* fn, uh_mapinit* mi, const Prepared& P, bool reconstruct, Blocks& B, MiArgs& a, const Planted* planted = nullptr) {
    const MiHead& hd = P.head;
    const size_t n = (size_t)hd.n, H = 2 * (size_t)hd.iters;
    uh::Layout I;
    const size_t i_head = I.take<MiHead>(1, 16), i_xy = I.take<float>(4 * n, 16), i_smp = I.take<int>(8 * (size_t)hd.iters, 16);
    const size_t i_bytes = (I.off + 15) & ~(size_t)15;
    uh::Layout W;
    B.w_mask = W.take<unsigned long long>(H * (size_t)hd.words, 16); B.w_score = W.take<float>(H, 16); B.w_mat = W.take<float>(9 * H, 16);
    B.w_null = W.take<double>(9 * H, 16);
    const size_t w_cst = W.take<uint8_t>(8 * n, 16), w_cos = W.take<float>(8 * n, 16), w_cpt = W.take<float>(24 * n, 16);
    uh::Layout R;
    B.r_out = R.take<MiOut>(1, 16); B.r_state = R.take<uint8_t>(n, 16); B.r_pt = R.take<float>(3 * n, 16);
    B.r_bytes = (R.off + 15) & ~(size_t)15;
    int rc;
    uh_ctx* ctx = mi->ctx;
    if ((rc = mi->h_in.reserve(i_bytes))) return rc;
    if ((rc = mi->h_out.reserve(B.r_bytes))) return rc;
    UH_HIP_CHECK(hipSetDevice(ctx->device));
    if ((rc = mi->d_in.reserve(i_bytes))) return rc;
    if ((rc = mi->d_work.reserve(W.off))) return rc;
    if ((rc = mi->d_out.reserve(B.r_bytes))) return rc;
    char* hi = mi->h_in.as<char>();
    std::memcpy(hi + i_head, &hd, sizeof(hd));
    std::memcpy(hi + i_xy, P.xy.data(), 16 * n);
    std::memcpy(hi + i_smp, P.samples.data(), 4 * P.samples.size());
    char* di = mi->d_in.as<char>();
    char* dw = mi->d_work.as<char>();
    char* dout = mi->d_out.as<char>();
    a.head = (const MiHead*)(di + i_head); a.xy = (const float4*)(di + i_xy); a.samples = (const int*)(di + i_smp);
    a.mask = (unsigned long long*)(dw + B.w_mask); a.score = (float*)(dw + B.w_score); a.mat = (float*)(dw + B.w_mat); a.nullvec = (double*)(dw + B.w_null);
    a.c_state = (uint8_t*)(dw + w_cst); a.c_cos = (float*)(dw + w_cos); a.c_pt = (float*)(dw + w_cpt);
    a.out = (MiOut*)(dout + B.r_out); a.state = (uint8_t*)(dout + B.r_state); a.pt = (float*)(dout + B.r_pt);
    hipStream_t s = ctx->stream;
    hipError_t e = hipMemcpyAsync(di, hi, i_bytes, hipMemcpyHostToDevice, s);
    if (e == hipSuccess && planted) {
        e = hipMemcpyAsync(a.score, planted->score, sizeof(planted->score), hipMemcpyHostToDevice, s);
        if (e == hipSuccess) e = hipMemcpyAsync(a.mat, planted->mat, sizeof(planted->mat), hipMemcpyHostToDevice, s);
        if (e == hipSuccess) e = hipMemcpyAsync(a.mask, planted->mask.data(), 8 * planted->mask.size(), hipMemcpyHostToDevice, s);
    }
    if (e == hipSuccess) {
        if (!planted) UH_LAUNCH(ctx, mi_hypothesis_kernel, dim3((unsigned)H), dim3(64), 0, a);
        if (reconstruct) UH_LAUNCH(ctx, mi_reconstruct_kernel, dim3(1), dim3(kRecThreads), 0, a);
        e = hipGetLastError();
    }
    if (e == hipSuccess && reconstruct) e = hipMemcpyAsync(mi->h_out.as<char>(), dout, B.r_bytes, hipMemcpyDeviceToHost, s);
    if (reconstruct) {
        const hipError_t es = hipStreamSynchronize(s);
        if (e == hipSuccess) e = es;
    }
    if (e != hipSuccess) {
        (void)hipStreamSynchronize(s);   // the pinned blocks are rewritten by the next call
        uh::set_error("%s: %s", fn, hipGetErrorString(e));
        return UH_ENODEVICE;
    }
    return UH_OK;
}

}  // namespace

extern "C" {

int uh_mapinit_create(uh_ctx* ctx, uh_mapinit** out) {
    UH_REQUIRE(ctx && out, "uh_mapinit_create: NULL argument");
    *out = new uh_mapinit();
    (*out)->ctx = ctx;
    return UH_OK;
}

void uh_mapinit_destroy(uh_mapinit* mi) { delete mi; }   // (the context is not read: it may be gone already)

int uh_mapinit_samples(int32_t n, int32_t iterations, int32_t* samples_out) {
    UH_REQUIRE(n >= 8 && iterations >= 0 && samples_out, "uh_mapinit_samples: n = %d (at least 8), iterations = %d, or a NULL output", n, iterations);
    return draw_samples(n, iterations, samples_out);
}

int uh_mapinit_run_host(const uh_mapinit_args* args, uh_mapinit_result* result) {
    Prepared P;
    int rc;
    if ((rc = prepare("uh_mapinit_run_host", args, result, P))) return rc;
    if (P.too_few) { clear_result(args, result); return UH_OK; }
    MiOut o;
    std::vector<uint8_t> state;
    std::vector<float> pt;
    host_run(P, o, state, pt);
    finish(args, o, state.data(), pt.data(), result);
    return UH_OK;
}

int uh_mapinit_run(uh_mapinit* mi, const uh_mapinit_args* args, uh_mapinit_result* result) {
    Prepared P;
    int rc;
    if ((rc = prepare("uh_mapinit_run", args, result, P))) return rc;
    if (P.too_few) { clear_result(args, result); return UH_OK; }   // `matches.size() < minNumMatches -> return false`: nothing is launched
    UH_REQUIRE(mi, "uh_mapinit_run: NULL initialiser");
    Blocks B;
    MiArgs a{};
    if ((rc = device_run("uh_mapinit_run", mi, P, true, B, a))) return rc;
    const char* ho = mi->h_out.as<char>();
    finish(args, *(const MiOut*)(ho + B.r_out), (const uint8_t*)(ho + B.r_state), (const float*)(ho + B.r_pt), result);
    return UH_OK;
}

int uh_mapinit_debug_hypothesis(uh_mapinit* mi, const uh_mapinit_args* args, int32_t model, int32_t iter, double* M9_double, float* M9_float, float* score,
                                uint64_t* mask_words) {
    UH_REQUIRE(mi && M9_double && M9_float && score && mask_words, "uh_mapinit_debug_hypothesis: NULL argument");
    UH_REQUIRE(model == UH_MAPINIT_HOMOGRAPHY || model == UH_MAPINIT_FUNDAMENTAL, "uh_mapinit_debug_hypothesis: model %d", model);
    uh_mapinit_result dummy{};
    std::vector<int32_t> mo(2 * (size_t)std::max(args ? args->n_matches : 0, 1));
    std::vector<float> po(3 * (size_t)std::max(args ? args->n_matches : 0, 1));
    dummy.matches_out = mo.data(); dummy.points_out = po.data(); dummy.cap_matches = args ? args->n_matches : 0;
    Prepared P;
    int rc;
    if ((rc = prepare("uh_mapinit_debug_hypothesis", args, &dummy, P))) return rc;
    UH_REQUIRE(!P.too_few && iter >= 0 && iter < args->iterations, "uh_mapinit_debug_hypothesis: fewer matches than min_matches, or iteration %d outside [0, %d)",
               iter, args ? args->iterations : 0);
    Blocks B;
    MiArgs a{};
    if ((rc = device_run("uh_mapinit_debug_hypothesis", mi, P, false, B, a))) return rc;
    const size_t h = (size_t)(model == UH_MAPINIT_HOMOGRAPHY ? iter : P.head.iters + iter);
    double x[9];
    hipStream_t s = mi->ctx->stream;
    hipError_t e = hipMemcpyAsync(x, a.nullvec + 9 * h, sizeof(x), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipMemcpyAsync(M9_float, a.mat + 9 * h, 9 * sizeof(float), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipMemcpyAsync(score, a.score + h, sizeof(float), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipMemcpyAsync(mask_words, a.mask + h * (size_t)P.head.words, 8 * (size_t)P.head.words, hipMemcpyDeviceToHost, s);
    const hipError_t es = hipStreamSynchronize(s);
    if (e == hipSuccess) e = es;
    if (e != hipSuccess) {
        uh::set_error("uh_mapinit_debug_hypothesis: %s", hipGetErrorString(e));
        return UH_ENODEVICE;
    }
    // the de-normalisation in double, from the device's double null vector
    const MiHead& hd = P.head;
    double T1[9], T2[9], L[9], X[9], tmp[9];
    for (int k = 0; k < 9; k++) { T1[k] = hd.N1.T[k]; T2[k] = hd.N2.T[k]; X[k] = x[k]; }
    if (model == UH_MAPINIT_HOMOGRAPHY) {   // T2^-1 of the diagonal-plus-offset T2, exactly
        const double sx = T2[0], sy = T2[4];
        const double inv[9] = {1.0 / sx, 0, -T2[2] / sx, 0, 1.0 / sy, -T2[5] / sy, 0, 0, 1};
        std::memcpy(L, inv, sizeof(L));
    } else {
        const double t[9] = {T2[0], T2[3], T2[6], T2[1], T2[4], T2[7], T2[2], T2[5], T2[8]};
        std::memcpy(L, t, sizeof(L));
        float Xf[9];
        for (int k = 0; k < 9; k++) Xf[k] = (float)x[k];
        double U[9], w[3], V[9];
        mim::svd3(Xf, U, w, V);   // the projection of the float matrix the reference projects, without rounding U, w, V
        for (int r = 0; r < 3; r++)
            for (int c = 0; c < 3; c++) X[3 * r + c] = U[3 * r] * w[0] * V[3 * c] + U[3 * r + 1] * w[1] * V[3 * c + 1];
    }
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) tmp[3 * r + c] = L[3 * r] * X[c] + L[3 * r + 1] * X[3 + c] + L[3 * r + 2] * X[6 + c];
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) M9_double[3 * r + c] = tmp[3 * r] * T1[c] + tmp[3 * r + 1] * T1[3 + c] + tmp[3 * r + 2] * T1[6 + c];
    return UH_OK;
}

// model, matrix and mask of the planted winner -> what prepare() left, cut to one iteration
static int plant(const char* fn, int32_t model, const float* M9, const uint64_t* mask_words, Prepared& P, Planted& pl, MiOut& o) {
    UH_REQUIRE(M9 && mask_words, "%s: NULL argument", fn);
    UH_REQUIRE(model == UH_MAPINIT_HOMOGRAPHY || model == UH_MAPINIT_FUNDAMENTAL, "%s: model %d", fn, model);
    UH_REQUIRE(!P.too_few, "%s: fewer matches than min_matches", fn);
    // (prepare() has normalised both frames, possibly over the planted non-finite keypoints: the head's T matrices are read by the hypothesis
    // launch alone, which this path does not run)
    const int h = model == UH_MAPINIT_HOMOGRAPHY ? 0 : 1, words = P.head.words, n = P.head.n;
    P.head.iters = 1;
    P.samples.resize(8);
    pl.score[h] = 1.f; pl.score[1 - h] = 0.f;
    std::memset(pl.mat, 0, sizeof(pl.mat));
    std::memcpy(pl.mat + 9 * h, M9, 9 * sizeof(float));
    pl.mask.assign(2 * (size_t)words, 0ull);
    for (int w = 0; w < words; w++) {
        const int left = n - 64 * w;   // bits past the last match are dropped: the kernels count the words' bits
        pl.mask[(size_t)h * words + w] = mask_words[w] & (left >= 64 ? ~0ull : (1ull << left) - 1ull);
    }
    std::memset(&o, 0, sizeof(o));
    o.best_h = h == 0 ? 0 : -1; o.best_f = h == 1 ? 0 : -1; o.sh = pl.score[0]; o.sf = pl.score[1];
    return UH_OK;
}

int uh_mapinit_debug_reconstruct(uh_mapinit* mi, const uh_mapinit_args* args, int32_t model, const float* M9, const uint64_t* mask_words,
                                 uh_mapinit_result* result) {
    const char* fn = "uh_mapinit_debug_reconstruct";
    Prepared P;
    Planted pl;
    MiOut o;
    int rc;
    if ((rc = prepare(fn, args, result, P))) return rc;
    if ((rc = plant(fn, model, M9, mask_words, P, pl, o))) return rc;
    if (!mi) {   // the host form
        HostHyp best[2];
        std::vector<unsigned long long> best_mask[2];
        for (int m = 0; m < 2; m++) {
            std::memcpy(best[m].M, pl.mat + 9 * m, sizeof(best[m].M));
            best_mask[m].assign(pl.mask.begin() + (size_t)m * P.head.words, pl.mask.begin() + (size_t)(m + 1) * P.head.words);
        }
        std::vector<uint8_t> state;
        std::vector<float> pt;
        host_reconstruct(P, best, best_mask, o, state, pt);
        finish(args, o, state.data(), pt.data(), result);
        return UH_OK;
    }
    Blocks B;
    MiArgs a{};
    if ((rc = device_run(fn, mi, P, true, B, a, &pl))) return rc;
    const char* ho = mi->h_out.as<char>();
    finish(args, *(const MiOut*)(ho + B.r_out), (const uint8_t*)(ho + B.r_state), (const float*)(ho + B.r_pt), result);
    return UH_OK;
}

}  // extern "C"
