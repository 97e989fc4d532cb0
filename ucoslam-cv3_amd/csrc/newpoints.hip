// New map points on the device (uh_newpoints_*): stage 3 of the mapper's per-keyframe step — for every covisible neighbour,
// Triangulate(newKF, neighbour, RT, matches) (src/basictypes/misc.cpp:923-1041), the distance-ratio / octave-ratio check and the
// per-keypoint merge of MapManager (src/utils/mapmanager.cpp:10087-10696, line numbers of the de-obfuscated text).
//
//   host     checks every index the kernels will trust, packs all pairs of the keyframe into one pinned block: ONE upload
//   np_triangulate_kernel   one lane per match, grid (ceil(max matches / 64), n_pairs): everything per pair is wave-uniform and arrives
//            through scalar loads.  The per-match arithmetic is newpoints_math.hpp (one text for device and host).  An accepted match
//            writes its position and its neighbour keypoint's octave into a dense n_pairs x n_kpts table (-1 = none), its queryIdx
//            into a second one: a trainIdx occurs at most once per pair
//            (matchEpipolar ends with filter_ambiguous_train; the host checks it), so no two lanes write one cell.
//   np_merge_kernel   one workgroup; one lane per keypoint of the new keyframe walks its column of the table in pair order — the
//            order in which the reference fills its std::map<trainIdx, vector> (:10416-10479) — counts the candidates and picks one
//            (:10495-10641); an ordered scan over the counts places the points in ascending trainIdx and their observation lists in
//            CSR form.  No atomics anywhere: the output is a function of the input alone.
//   host     ONE download of the result block into pinned memory owned by the handle, ONE wait.
//
// The null vector of A comes from a one-sided Jacobi in double where the reference calls cv::SVD in float, and the cv::Mat products
// accumulate in double: both UNPINNED (no OpenCV to compare with); see include/ucoslam_hip.h.
#include <algorithm>
#include <climits>
#include <cmath>
#include "common.hpp"
#include "newpoints_math.hpp"

namespace {

constexpr int kTriThreads = 64;
constexpr int kMergeThreads = 1024;
constexpr int kMergeWaves = kMergeThreads / 64;
constexpr int kMergeUnroll = 8;   // measured: 32 in flight spills 629 SGPRs and is slower (53.7 us against 47.1)
// a table cell: the match's position in its pair's list, the neighbour keypoint's octave above it; -1 = no accepted match
constexpr int kOctShift = 24, kMatchMask = (1 << kOctShift) - 1, kMaxLevels = 1 << (31 - kOctShift);

struct NpPairDev {
    npm::PairConst Q;
    int n_matches, m_off, k_off, lvl_off;   // offsets of this pair's matches, keypoints and scale tables in the concatenated arrays
};

struct NpArgs {
    npm::FrameConst F;
    int nk, n_pairs, merge_rule, pad;
    const NpPairDev* pairs;
    const float* pt_new; const int* oct_new;
    const float* sf; const float* inv_sig;      // scale factors and 1.f / (f * f), the new keyframe's levels first, then pair by pair
    const float* pt_nb; const int* oct_nb;      // the neighbours' keypoints, pair by pair
    const uh_dmatch* matches;                   // pair by pair
    int* table;                                 // n_pairs x nk cells
    int* q_table;                               // n_pairs x nk: the accepted match's queryIdx (defined where the cell is taken)
    float* match_glob;                          // n_total x 3: pg of every accepted match
    // the result block
    int* hdr;                                   // n_new, n_obs
    uint8_t* status; float* xyz_cam;
    int* kp_idx; float* xyz_global; float* distance; int* chosen_pair; int* chosen_match;
    int* obs_ptr; int* obs_pair; int* obs_kpt;
};

__global__ __launch_bounds__(kTriThreads) void np_triangulate_kernel(NpArgs a) {
    const NpPairDev& pr = a.pairs[blockIdx.y];
    const int k = blockIdx.x * kTriThreads + threadIdx.x;
    if (k >= pr.n_matches) return;
    const uh_dmatch m = a.matches[pr.m_off + k];
    const float x1 = a.pt_new[2 * (size_t)m.trainIdx], y1 = a.pt_new[2 * (size_t)m.trainIdx + 1];
    const float x2 = a.pt_nb[2 * ((size_t)pr.k_off + m.queryIdx)], y2 = a.pt_nb[2 * ((size_t)pr.k_off + m.queryIdx) + 1];
    const int o1 = a.oct_new[m.trainIdx], o2 = a.oct_nb[pr.k_off + m.queryIdx];
    npm::MatchOut o;
    npm::triangulate_match(a.F, pr.Q, x1, y1, x2, y2, a.inv_sig[o1], a.inv_sig[pr.lvl_off + o2], a.sf[o1], a.sf[pr.lvl_off + o2], npm::kJacobiSweeps, o);
    const size_t g = (size_t)pr.m_off + k;
    a.status[g] = o.status;
#pragma unroll
    for (int c = 0; c < 3; c++) { a.xyz_cam[3 * g + c] = o.cam[c]; a.match_glob[3 * g + c] = o.glob[c]; }
    if (o.status == npm::kAccepted) {
        const size_t cell = (size_t)blockIdx.y * a.nk + m.trainIdx;
        a.table[cell] = k | (o2 << kOctShift);
        a.q_table[cell] = m.queryIdx;
    }
}

// inclusive scan over the workgroup in thread order; returns this thread's inclusive value, *total = the workgroup's sum
__device__ int block_scan_inclusive(int v, int* s_wave, int* total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int u = __shfl_up(v, d, 64);
        if (lane >= d) v += u;
    }
    if (lane == 63) s_wave[wave] = v;
    __syncthreads();
    int before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < kMergeWaves; w++) { const int s = s_wave[w]; all += s; if (w < wave) before += s; }
    __syncthreads();
    *total = all;
    return v + before;
}

__global__ __launch_bounds__(kMergeThreads) void np_merge_kernel(NpArgs a) {
    __shared__ int s_wave[kMergeWaves];
    int base_new = 0, base_obs = 0;
    for (int first = 0; first < a.nk; first += kMergeThreads) {
        const int kp = first + (int)threadIdx.x;
        int cnt = 0, best_pair = -1, best_match = -1, best_oct = INT_MAX;
        if (kp < a.nk) {
            // the column in pair order, kMergeUnroll cells in flight at a time: a cell holds all the choice needs, no load depends on another
            for (int j0 = 0; j0 < a.n_pairs; j0 += kMergeUnroll) {
                int e[kMergeUnroll];
#pragma unroll
                for (int u = 0; u < kMergeUnroll; u++) e[u] = j0 + u < a.n_pairs ? a.table[(size_t)(j0 + u) * a.nk + kp] : -1;
#pragma unroll
                for (int u = 0; u < kMergeUnroll; u++) {
                    if (e[u] < 0) continue;
                    cnt++;
                    const int oct = e[u] >> kOctShift;
                    // :10604-10618; UH_NEWPOINTS_MERGE_AS_COMPILED: the reference never assigns its running minimum, so every candidate wins in turn
                    if (a.merge_rule == UH_NEWPOINTS_MERGE_AS_COMPILED || oct < best_oct) { best_oct = oct; best_pair = j0 + u; best_match = e[u] & kMatchMask; }
                }
            }
        }
        const int is_new = cnt > 0 ? 1 : 0, n_obs = cnt > 0 ? cnt + 1 : 0;
        int tot_new, tot_obs;
        const int at_new = base_new + block_scan_inclusive(is_new, s_wave, &tot_new) - is_new;
        const int at_obs = base_obs + block_scan_inclusive(n_obs, s_wave, &tot_obs) - n_obs;
        if (is_new) {
            const size_t g = (size_t)a.pairs[best_pair].m_off + best_match;
            a.kp_idx[at_new] = kp;
#pragma unroll
            for (int c = 0; c < 3; c++) a.xyz_global[3 * (size_t)at_new + c] = a.match_glob[3 * g + c];   // :10645
            a.distance[at_new] = a.matches[g].distance;                                                   // :10649
            a.chosen_pair[at_new] = best_pair;
            a.chosen_match[at_new] = best_match;
            a.obs_ptr[at_new] = at_obs;
            int w = at_obs;
            a.obs_pair[w] = -1; a.obs_kpt[w] = kp; w++;                                                   // :10653-10661 the new keyframe itself
            for (int j0 = 0; j0 < a.n_pairs; j0 += kMergeUnroll) {                                         // :10669-10687 every candidate, in list order
                int e[kMergeUnroll], q[kMergeUnroll];
#pragma unroll
                for (int u = 0; u < kMergeUnroll; u++) {
                    const bool in = j0 + u < a.n_pairs;
                    e[u] = in ? a.table[(size_t)(j0 + u) * a.nk + kp] : -1;
                    q[u] = in ? a.q_table[(size_t)(j0 + u) * a.nk + kp] : 0;   // read whether or not the cell is taken: nothing waits for e[u]
                }
#pragma unroll
                for (int u = 0; u < kMergeUnroll; u++)
                    if (e[u] >= 0) { a.obs_pair[w] = j0 + u; a.obs_kpt[w] = q[u]; w++; }
            }
        }
        base_new += tot_new; base_obs += tot_obs;
    }
    if (threadIdx.x == 0) { a.obs_ptr[base_new] = base_obs; a.hdr[0] = base_new; a.hdr[1] = base_obs; }
}

}  // namespace

struct uh_newpoints {
    uh_ctx* ctx = nullptr;
    uh::DevBuf d_in, d_work, d_out;
    uh::PinBuf h_in, h_out;
    std::vector<int> seen;   // per keypoint of the new keyframe: the last pair (+1) that matched it
};

extern "C" {

int uh_fundamental_12(const float* intr4_train, const float* intr4_query, const float* RT, float* F12_out) {
    UH_REQUIRE(intr4_train && intr4_query && RT && F12_out, "uh_fundamental_12: NULL argument");
    // computeF12(eye, Ktrain, RT, Kquery), misc.cpp:901-907 with R1w = I, t1w = 0: R12 = R2w', t12 = -R2w' t2w (+ 0)
    double R12[9], t12[3];
    for (int i = 0; i < 3; i++) {
        for (int j = 0; j < 3; j++) R12[3 * i + j] = RT[4 * j + i];
        t12[i] = (double)(float)(-(double)RT[i] * RT[3] + -(double)RT[4 + i] * RT[7] + -(double)RT[8 + i] * RT[11]);
    }
    const double tx[9] = {0, -t12[2], t12[1], t12[2], 0, -t12[0], -t12[1], t12[0], 0};   // :909-913
    // :918 CameraMatrix1.t().inv() * t12x * R12 * K2.inv(), left to right; the inverse of the upper-triangular K in closed form
    auto kinv = [](const float* i4, double* o) {
        const double fx = i4[0], fy = i4[1], cx = i4[2], cy = i4[3];
        const double m[9] = {1 / fx, 0, -cx / fx, 0, 1 / fy, -cy / fy, 0, 0, 1};
        for (int k = 0; k < 9; k++) o[k] = (double)(float)m[k];
    };
    auto mul = [](const double* A, const double* B, double* C) {   // a float GEMM: double sums, one rounding
        double t[9];
        for (int i = 0; i < 3; i++)
            for (int j = 0; j < 3; j++) t[3 * i + j] = (double)(float)(A[3 * i] * B[j] + A[3 * i + 1] * B[3 + j] + A[3 * i + 2] * B[6 + j]);
        for (int k = 0; k < 9; k++) C[k] = t[k];
    };
    double K1i[9], K1it[9], K2i[9], M[9];
    kinv(intr4_train, K1i);
    kinv(intr4_query, K2i);
    for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) K1it[3 * i + j] = K1i[3 * j + i];
    mul(K1it, tx, M);
    mul(M, R12, M);
    mul(M, K2i, M);
    for (int k = 0; k < 9; k++) F12_out[k] = (float)M[k];
    return UH_OK;
}

int uh_newpoints_create(uh_ctx* ctx, uh_newpoints** out) {
    UH_REQUIRE(ctx && out, "uh_newpoints_create: NULL argument");
    uh_newpoints* np = new uh_newpoints();
    np->ctx = ctx;
    *out = np;
    return UH_OK;
}

void uh_newpoints_destroy(uh_newpoints* np) { delete np; }

int uh_newpoints_run(uh_newpoints* np, const uh_newpoints_args* args, uh_newpoints_result* res) {
    UH_REQUIRE(np && args && res, "uh_newpoints_run: NULL argument");
    std::memset(res, 0, sizeof(*res));
    const int nk = args->n_kpts, n_pairs = args->n_pairs;
    // ---- everything the kernels will trust is checked here, before anything is launched
    UH_REQUIRE(nk >= 0 && (nk == 0 || (args->pt && args->octave)), "uh_newpoints_run: the new keyframe's keypoint arrays are missing");
    if (nk > UH_NEWPOINTS_MAX_KPTS) {
        uh::set_error("uh_newpoints_run: %d keypoints in the new keyframe exceed the cap of %d (the merge is one workgroup)", nk, UH_NEWPOINTS_MAX_KPTS);
        return UH_EINVAL;
    }
    UH_REQUIRE(args->n_levels >= 1 && args->scale_factors, "uh_newpoints_run: the new keyframe has no scale factors");
    UH_REQUIRE(n_pairs >= 0 && n_pairs <= UH_NEWPOINTS_MAX_PAIRS && (n_pairs == 0 || args->pairs), "uh_newpoints_run: n_pairs outside 0..%d or a NULL pair array", UH_NEWPOINTS_MAX_PAIRS);
    UH_REQUIRE(args->merge_rule == UH_NEWPOINTS_MERGE_SMALLEST_OCTAVE || args->merge_rule == UH_NEWPOINTS_MERGE_AS_COMPILED, "uh_newpoints_run: unknown merge_rule %d", args->merge_rule);
    np->seen.assign((size_t)nk, 0);
    size_t n_total = 0, nk_nb = 0, n_lvl = (size_t)args->n_levels;
    int max_matches = 0;
    for (int j = 0; j < n_pairs; j++) {
        const uh_newpoints_pair& p = args->pairs[j];
        UH_REQUIRE(p.n_kpts >= 0 && (p.n_kpts == 0 || (p.pt && p.octave)), "uh_newpoints_run: pair %d: keypoint arrays are missing", j);
        UH_REQUIRE(p.n_levels >= 1 && p.n_levels <= kMaxLevels && p.scale_factors, "uh_newpoints_run: pair %d: no scale factors, or more than %d levels", j, kMaxLevels);
        UH_REQUIRE(p.n_matches >= 0 && p.n_matches <= kMatchMask && (p.n_matches == 0 || p.matches), "uh_newpoints_run: pair %d: bad match list", j);
        for (int k = 0; k < p.n_matches; k++) {
            const uh_dmatch& m = p.matches[k];
            UH_REQUIRE(m.queryIdx >= 0 && m.queryIdx < p.n_kpts, "uh_newpoints_run: pair %d match %d: queryIdx %d outside the neighbour's %d keypoints", j, k, m.queryIdx, p.n_kpts);
            UH_REQUIRE(m.trainIdx >= 0 && m.trainIdx < nk, "uh_newpoints_run: pair %d match %d: trainIdx %d outside the new keyframe's %d keypoints", j, k, m.trainIdx, nk);
            const int o1 = args->octave[m.trainIdx], o2 = p.octave[m.queryIdx];
            UH_REQUIRE(o1 >= 0 && o1 < args->n_levels, "uh_newpoints_run: pair %d match %d: octave %d of the new keyframe's keypoint %d outside its %d levels", j, k, o1, m.trainIdx, args->n_levels);
            UH_REQUIRE(o2 >= 0 && o2 < p.n_levels, "uh_newpoints_run: pair %d match %d: octave %d of the neighbour's keypoint %d outside its %d levels", j, k, o2, m.queryIdx, p.n_levels);
            UH_REQUIRE(np->seen[m.trainIdx] != j + 1, "uh_newpoints_run: pair %d match %d: trainIdx %d occurs twice in this pair (filter_ambiguous_train guarantees at most once)", j, k, m.trainIdx);
            np->seen[m.trainIdx] = j + 1;
        }
        n_total += (size_t)p.n_matches; nk_nb += (size_t)p.n_kpts; n_lvl += (size_t)p.n_levels;
        max_matches = std::max(max_matches, p.n_matches);
    }
    UH_REQUIRE(n_total <= (size_t)INT_MAX / 4 && nk_nb <= (size_t)INT_MAX / 4, "uh_newpoints_run: too many matches or keypoints in all pairs together");

    // ---- the result block: one layout for the device copy and the pinned copy
    uh::Layout R;
    const size_t r_hdr = R.take<int>(4, 16), r_status = R.take<uint8_t>(n_total, 16), r_cam = R.take<float>(3 * n_total, 16);
    const size_t r_kp = R.take<int>(nk, 16), r_xyz = R.take<float>(3 * (size_t)nk, 16), r_dist = R.take<float>(nk, 16);
    const size_t r_cp = R.take<int>(nk, 16), r_cm = R.take<int>(nk, 16), r_op = R.take<int>((size_t)nk + 1, 16);
    const size_t r_opair = R.take<int>((size_t)nk + n_total, 16), r_okpt = R.take<int>((size_t)nk + n_total, 16);
    const size_t r_bytes = (R.off + 15) & ~(size_t)15;
    if (const int rc = np->h_out.reserve(r_bytes)) return rc;
    char* ho = np->h_out.as<char>();
    auto publish = [&](int n_new, int n_obs) {
        res->n_total = (int32_t)n_total; res->status = (const uint8_t*)(ho + r_status); res->xyz_cam = (const float*)(ho + r_cam);
        res->n_new = n_new; res->n_obs = n_obs;
        res->kp_idx = (const int32_t*)(ho + r_kp); res->xyz_global = (const float*)(ho + r_xyz); res->distance = (const float*)(ho + r_dist);
        res->chosen_pair = (const int32_t*)(ho + r_cp); res->chosen_match = (const int32_t*)(ho + r_cm);
        res->obs_ptr = (const int32_t*)(ho + r_op); res->obs_pair = (const int32_t*)(ho + r_opair); res->obs_kpt = (const int32_t*)(ho + r_okpt);
    };
    if (n_total == 0) {   // nothing to triangulate: no launch
        *(int*)(ho + r_op) = 0;
        publish(0, 0);
        return UH_OK;
    }

    // ---- the input block, packed into pinned memory
    uh::Layout I;
    const size_t i_pairs = I.take<NpPairDev>(n_pairs, 16), i_pt = I.take<float>(2 * (size_t)nk, 16), i_oct = I.take<int>(nk, 16);
    const size_t i_sf = I.take<float>(n_lvl, 16), i_inv = I.take<float>(n_lvl, 16);
    const size_t i_ptn = I.take<float>(2 * nk_nb, 16), i_octn = I.take<int>(nk_nb, 16), i_m = I.take<uh_dmatch>(n_total, 16);
    const size_t i_bytes = (I.off + 15) & ~(size_t)15;
    uh::Layout W;
    const size_t w_table = W.take<int>((size_t)n_pairs * nk, 16), w_q = W.take<int>((size_t)n_pairs * nk, 16), w_glob = W.take<float>(3 * n_total, 16);
    if (const int rc = np->h_in.reserve(i_bytes)) return rc;
    UH_HIP_CHECK(hipSetDevice(np->ctx->device));
    if (const int rc = np->d_in.reserve(i_bytes)) return rc;
    if (const int rc = np->d_work.reserve(W.off)) return rc;
    if (const int rc = np->d_out.reserve(r_bytes)) return rc;
    char* hi = np->h_in.as<char>();
    std::memcpy(hi + i_pt, args->pt, 8 * (size_t)nk);
    std::memcpy(hi + i_oct, args->octave, 4 * (size_t)nk);
    float* sf = (float*)(hi + i_sf);
    float* inv = (float*)(hi + i_inv);
    for (int l = 0; l < args->n_levels; l++) { const float f = args->scale_factors[l]; sf[l] = f; inv[l] = 1.f / (f * f); }   // misc.cpp:947-949
    NpPairDev* hp = (NpPairDev*)(hi + i_pairs);
    size_t m_off = 0, k_off = 0, lvl_off = (size_t)args->n_levels;
    for (int j = 0; j < n_pairs; j++) {
        const uh_newpoints_pair& p = args->pairs[j];
        npm::make_pair_const(p.RT, p.intr4, p.cam_center, hp[j].Q);
        hp[j].n_matches = p.n_matches; hp[j].m_off = (int)m_off; hp[j].k_off = (int)k_off; hp[j].lvl_off = (int)lvl_off;
        if (p.n_kpts) {
            std::memcpy(hi + i_ptn + 8 * k_off, p.pt, 8 * (size_t)p.n_kpts);
            std::memcpy(hi + i_octn + 4 * k_off, p.octave, 4 * (size_t)p.n_kpts);
        }
        if (p.n_matches) std::memcpy(hi + i_m + sizeof(uh_dmatch) * m_off, p.matches, sizeof(uh_dmatch) * (size_t)p.n_matches);
        for (int l = 0; l < p.n_levels; l++) { const float f = p.scale_factors[l]; sf[lvl_off + l] = f; inv[lvl_off + l] = 1.f / (f * f); }
        m_off += (size_t)p.n_matches; k_off += (size_t)p.n_kpts; lvl_off += (size_t)p.n_levels;
    }

    NpArgs a{};
    a.F.fx1 = args->intr4[0]; a.F.fy1 = args->intr4[1]; a.F.cx1 = args->intr4[2]; a.F.cy1 = args->intr4[3];
    a.F.invfx1 = 1.f / a.F.fx1; a.F.invfy1 = 1.f / a.F.fy1;   // misc.cpp:955-958
    for (int k = 0; k < 12; k++) a.F.T[k] = args->pose_g2f[k];
    for (int k = 0; k < 3; k++) a.F.c1[k] = args->cam_center[k];
    a.F.max_chi2 = args->max_chi2; a.F.ratio_factor = args->ratio_factor;
    a.nk = nk; a.n_pairs = n_pairs; a.merge_rule = args->merge_rule;
    char* di = np->d_in.as<char>();
    char* dw = np->d_work.as<char>();
    char* dout = np->d_out.as<char>();
    a.pairs = (const NpPairDev*)(di + i_pairs);
    a.pt_new = (const float*)(di + i_pt); a.oct_new = (const int*)(di + i_oct);
    a.sf = (const float*)(di + i_sf); a.inv_sig = (const float*)(di + i_inv);
    a.pt_nb = (const float*)(di + i_ptn); a.oct_nb = (const int*)(di + i_octn); a.matches = (const uh_dmatch*)(di + i_m);
    a.table = (int*)(dw + w_table); a.q_table = (int*)(dw + w_q); a.match_glob = (float*)(dw + w_glob);
    a.hdr = (int*)(dout + r_hdr); a.status = (uint8_t*)(dout + r_status); a.xyz_cam = (float*)(dout + r_cam);
    a.kp_idx = (int*)(dout + r_kp); a.xyz_global = (float*)(dout + r_xyz); a.distance = (float*)(dout + r_dist);
    a.chosen_pair = (int*)(dout + r_cp); a.chosen_match = (int*)(dout + r_cm);
    a.obs_ptr = (int*)(dout + r_op); a.obs_pair = (int*)(dout + r_opair); a.obs_kpt = (int*)(dout + r_okpt);

    // ---- one chain on the context's stream, one wait.  After the first enqueue every failure drains the stream before it returns:
    // the pinned blocks are rewritten by the next call.
    hipStream_t st = np->ctx->stream;
    hipError_t e = hipMemcpyAsync(di, hi, i_bytes, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemsetAsync(a.table, 0xFF, sizeof(int) * (size_t)n_pairs * nk, st);
    if (e == hipSuccess) {
        UH_LAUNCH(np->ctx, np_triangulate_kernel, dim3(uh_div_up(max_matches, kTriThreads), n_pairs), dim3(kTriThreads), 0, a);
        UH_LAUNCH(np->ctx, np_merge_kernel, dim3(1), dim3(kMergeThreads), 0, a);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(ho, dout, r_bytes, hipMemcpyDeviceToHost, st);
    const hipError_t es = hipStreamSynchronize(st);
    if (e == hipSuccess) e = es;
    if (e != hipSuccess) {
        uh::set_error("uh_newpoints_run: %s", hipGetErrorString(e));
        return UH_ENODEVICE;
    }
    const int* hdr = (const int*)(ho + r_hdr);
    publish(hdr[0], hdr[1]);
    return UH_OK;
}

}  // extern "C"
