// Projection matcher on MI355X (gfx950) behind the C ABI (uh_projmatch_*): map points of the neighbouring keyframes are
// projected into the current frame and matched to its keypoints inside a scale-dependent disc.
//
// Semantic contract (reference file:line):
//   src/map.cpp:651-770                 Map::matchFrameToMapPoints: view-cosine >= 0.5, depth >= 0, distance-invariance window,
//                                       in-image test, predicted octave, disc radius scale*maxRepjDist (x1.6 if cos < 0.98),
//                                       octaves [p-1, p], best / second-best Hamming bookkeeping IN CANDIDATE ORDER, the 0.8
//                                       ratio rule when both have the same octave, then filter_ambiguous_query
//   src/map_types/frame.cpp:102-115     Frame::getKeyPointsInRegion (kd-tree radius search, unsorted, octave filter)
//   src/map_types/frame.h:129-136       Frame::predictScale
//   src/map_types/mappoint.h:99,146-177 getViewCos, getHammDescDistance_2 (float result)
//   src/basictypes/picoflann.h          KdTreeIndex<2>: build :150-163,238-345 (mean/variance split on <=100 samples,
//                                       planeSplit, std::sort fallback, leaves <= 10) and searchExactLevel :545-590
//
// The candidate ORDER is observable (a candidate that fails "d < best" updates the second-best, one that succeeds does not
// demote the old best), so the disc search cannot be replaced by a grid: the kernel walks the SAME kd-tree in the SAME
// order.  Division of work:
//   host   (uh_projmatch_set_frame)  builds the tree exactly like picoflann does — the reference also builds it on the CPU,
//          once per frame (Frame::create_kdtree, frame.h:124) — and uploads it flattened (24-byte nodes + leaf index list)
//   device (projmatch_kernel)        one lane per map point: visibility tests, predicted octave, iterative tree walk with an
//          explicit stack (the recursion's after-best-child / restore steps are stack records), Hamming distances against the
//          frame's descriptors, best / second-best rule.  ~10^3..10^4 map points x a few dozen candidates each: the kernel is
//          bound by dependent L2 round trips of the walk, not by bandwidth.
//   host   orders the per-point results into the DMatch list and runs filter_ambiguous_query (matcher.hip).
// Floating-point conventions are those of oracle/proj_oracle.cpp (float ops in source order, no contraction; cv::norm in
// double); predictScale's logf is libm's, reproduced on the device by glibc_sincosf.hpp.
#include <immintrin.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "common.hpp"
#include "devframe.hpp"
#include "glibc_sincosf.hpp"

extern "C" int uh_filter_ambiguous(uh_dmatch* matches, int n, int by_train);

namespace {

constexpr int kLeafMax = 10;          // picoflann _maxLeafSize
constexpr int kMaxDepth = 90;         // deeper trees (pathological inputs) are refused: the walk stacks live in LDS
constexpr size_t kLdsBudget = 150 * 1024;   // of the CU's 160 KB
constexpr int kPmThreads = 768;       // at most twelve waves share the LDS copy of the frame (the launch picks 4 .. 12: see uh_projmatch_match; 170 registers per lane)
constexpr int kGroup = 64;            // lanes per map point: ONE point per wave (round 5; a leaf holds <= 10 keypoints, the drain uses all 64)
constexpr int kGroupsMax = kPmThreads / kGroup;   // groups (map points in flight) per workgroup, at most
constexpr int kPmMaxBlocks = 768;     // workgroups loop over chunks of 16 map points: the frame is staged once per workgroup
constexpr int kCandCap = 128;         // per-point list of disc hits between two drains (a leaf adds at most 10)

struct KdNodeDev {
    float divlow, divhigh;
    int left, right;        // -1/-1 = leaf
    int leaf_begin;
    short leaf_count, col;
};
static_assert(sizeof(KdNodeDev) == 24, "node layout");

// ---------------------------------------------------------------------------------------------------------- host: tree build
// Flat-array restatement of picoflann::KdTreeIndex<2>::build for (x,y) float points.  std::sort is used exactly where the
// reference uses it (same libstdc++ => same permutation of equal keys).
class KdBuilder {
public:
    std::vector<KdNodeDev> nodes;
    std::vector<uint32_t> leaf_idx;
    double root_box[4] = {0, 0, 0, 0};   // x.min x.max y.min y.max
    int max_depth = 0;

    void build(const float* xy, int n) {
        xy_ = xy;
        nodes.clear();
        leaf_idx.clear();
        leaf_idx.reserve(n);
        order_.resize(n);
        px_.resize(n); py_.resize(n);
        tmp_l_.resize(n + 1); tmp_r_.resize(n + 1);
        // (the same loop finds the exponent spread of the non-zero coordinates — see sample_moments; branch-free: a zero counts as neither
        // bound, a non-finite value shows as exponent 255, a denormal as exponent 0)
        uint32_t emin = 255, emax = 0;
        for (int i = 0; i < n; i++) {
            order_[i] = (uint32_t)i;
            const float x = xy[2 * (size_t)i], y = xy[2 * (size_t)i + 1];
            px_[i] = x; py_[i] = y;
            uint32_t bx, by;
            std::memcpy(&bx, &x, 4); std::memcpy(&by, &y, 4);
            const uint32_t ex = (bx >> 23) & 0xffu, ey = (by >> 23) & 0xffu;
            const bool zx = (bx & 0x7fffffffu) == 0, zy = (by & 0x7fffffffu) == 0;
            emin = std::min(emin, std::min(zx ? 255u : ex, zy ? 255u : ey));
            emax = std::max(emax, std::max(zx ? 0u : ex, zy ? 0u : ey));
        }
        max_depth = 0;
        if (n == 0) return;
        exact_sums_ = emax != 255 /* finite */ && emin >= 1 /* no denormals */ && emax - emin <= 10;   // (a cloud of zeros only: the unsigned difference wraps and the ordered chains stay — equally right)
        Box root;
        bounds(0, n, root);
        nodes.reserve(2 * (size_t)n + 2);
        nodes.push_back(KdNodeDev{0, 0, -1, -1, 0, 0, 0});
        split(0, 0, n, root, 1);
        root_box[0] = root.lo[0]; root_box[1] = root.hi[0]; root_box[2] = root.lo[1]; root_box[3] = root.hi[1];
    }

private:
    struct Box { double lo[2], hi[2]; };
    const float* xy_ = nullptr;
    // the index permutation the reference partitions in place, with the points' coordinates carried along in the same order: every
    // scan below reads contiguous floats instead of gathering through the permutation
    std::vector<uint32_t> order_;
    std::vector<float> px_, py_;
    std::vector<int> tmp_l_, tmp_r_;
    float* coords(int d) { return d == 0 ? px_.data() : py_.data(); }

    void bounds(int b, int e, Box& box) const {
        float lx = px_[b], hx = px_[b], ly = py_[b], hy = py_[b];
        for (int k = b + 1; k < e; k++) {
            const float x = px_[k], y = py_[k];
            lx = x < lx ? x : lx; hx = x > hx ? x : hx;
            ly = y < ly ? y : ly; hy = y > hy ? y : hy;
        }
        box.lo[0] = lx; box.hi[0] = hx; box.lo[1] = ly; box.hi[1] = hy;
    }

    // picoflann.h:362-391: mean / variance over at most ~100 evenly spaced samples (float squares, double sums IN SAMPLE ORDER: four
    // dependent addition chains, ~a third of the build).  Round 6: when every coordinate of the cloud lies within a factor 2^10 of every
    // other (exponent spread <= 10: any extractor output — pixels 19 .. 4095 — does), no partial sum of <= 256 samples is ever rounded
    // (x: multiples of 2^(e_min-23) below 2^(e_max+9); fl(x*x): multiples of 2^(2 e_min-23) below 2^(2 e_max+10) — both fit 53 bits), so
    // the sums are the exact real sums in ANY order and four partial accumulators per sum give the same bits; otherwise the chains stay.
    bool exact_sums_ = false;
    void sample_moments(int b, int e, double mean[2], double var[2]) const {
        double s1[2] = {0, 0}, s2[2] = {0, 0};
        int step = 1, cnt = 0;
        if (e - b >= 200) step = (e - b) / 100;
        if (exact_sums_ && avx512_ && step == 1) {
            cnt = e - b;
            moments_avx512(px_.data() + b, py_.data() + b, cnt, s1, s2);
        } else if (exact_sums_) {
            double a1[4] = {0, 0, 0, 0}, a2[4] = {0, 0, 0, 0}, c1[4] = {0, 0, 0, 0}, c2[4] = {0, 0, 0, 0};
            cnt = (e - b + step - 1) / step;
            const float* qx = px_.data() + b; const float* qy = py_.data() + b;
            int k = 0;
            for (; k + 4 <= cnt; k += 4) {
#pragma GCC unroll 4
                for (int u = 0; u < 4; u++) {
                    const float x = qx[(size_t)(k + u) * step], y = qy[(size_t)(k + u) * step];
                    a1[u] += x; a2[u] += x * x; c1[u] += y; c2[u] += y * y;
                }
            }
            for (; k < cnt; k++) { const float x = qx[(size_t)k * step], y = qy[(size_t)k * step]; a1[0] += x; a2[0] += x * x; c1[0] += y; c2[0] += y * y; }
            s1[0] = (a1[0] + a1[1]) + (a1[2] + a1[3]); s2[0] = (a2[0] + a2[1]) + (a2[2] + a2[3]);
            s1[1] = (c1[0] + c1[1]) + (c1[2] + c1[3]); s2[1] = (c2[0] + c2[1]) + (c2[2] + c2[3]);
        } else {
            for (int i = b; i < e; i += step, cnt++) {
                const float x = px_[i], y = py_[i];
                s1[0] += x; s2[0] += x * x;
                s1[1] += y; s2[1] += y * y;
            }
        }
        const double inv = 1. / double(cnt);
        for (int d = 0; d < 2; d++) {
            mean[d] = s1[d] * inv;
            var[d] = s2[d] * inv - mean[d] * mean[d];
        }
    }

    // exact sums (see above) of cnt contiguous samples, eight doubles per accumulator: fl(x), fl(x * x) in float as picoflann squares it
    __attribute__((target("avx512f,avx512vl"))) static void moments_avx512(const float* qx, const float* qy, int cnt, double s1[2], double s2[2]) {
        __m512d a1 = _mm512_setzero_pd(), a2 = a1, c1 = a1, c2 = a1;
        int k = 0;
        for (; k + 8 <= cnt; k += 8) {
            const __m256 x = _mm256_loadu_ps(qx + k), y = _mm256_loadu_ps(qy + k);
            a1 = _mm512_add_pd(a1, _mm512_cvtps_pd(x)); a2 = _mm512_add_pd(a2, _mm512_cvtps_pd(_mm256_mul_ps(x, x)));
            c1 = _mm512_add_pd(c1, _mm512_cvtps_pd(y)); c2 = _mm512_add_pd(c2, _mm512_cvtps_pd(_mm256_mul_ps(y, y)));
        }
        if (k < cnt) {
            const __mmask8 m = (__mmask8)((1u << (cnt - k)) - 1u);
            const __m256 x = _mm256_maskz_loadu_ps(m, qx + k), y = _mm256_maskz_loadu_ps(m, qy + k);   // (zeros add nothing)
            a1 = _mm512_add_pd(a1, _mm512_cvtps_pd(x)); a2 = _mm512_add_pd(a2, _mm512_cvtps_pd(_mm256_mul_ps(x, x)));
            c1 = _mm512_add_pd(c1, _mm512_cvtps_pd(y)); c2 = _mm512_add_pd(c2, _mm512_cvtps_pd(_mm256_mul_ps(y, y)));
        }
        s1[0] = _mm512_reduce_add_pd(a1); s2[0] = _mm512_reduce_add_pd(a2);
        s1[1] = _mm512_reduce_add_pd(c1); s2[1] = _mm512_reduce_add_pd(c2);
    }

    void swap_items(int i, int j) {
        std::swap(order_[i], order_[j]); std::swap(px_[i], px_[j]); std::swap(py_[i], py_[j]);
    }

    // One Hoare pass of picoflann.h:403-424 over [b, e) with the predicate "belongs left" = (v < cut) or (v <= cut): the reference
    // walks l up to the first element that belongs right, r down to the last that belongs left, swaps them and repeats until the
    // two meet.  That is: with m = the number of elements that belong left, the misplaced elements in front of b + m (ascending)
    // are exchanged pairwise with the misplaced elements from b + m on (descending) — the same permutation, obtained here with a
    // count and two branch-free compactions instead of two data-dependent scans (the scans mispredict on every other element).
    template <bool INCLUSIVE>
    int hoare_pass(int b, int e, const float* v, float cut) {
        if (avx512_) return hoare_pass_avx512<INCLUSIVE>(b, e, v, cut);
        int m = 0;
        for (int i = b; i < e; i++) m += INCLUSIVE ? (v[i] <= cut) : (v[i] < cut);
        const int mid = b + m;
        if (m == 0 || mid == e) return mid;   // one side is empty: nothing is misplaced (the usual outcome of the second pass: no point EQUALS the cut)
        int* L = tmp_l_.data();
        int* R = tmp_r_.data();
        int nl = 0, nr = 0;
        for (int i = b; i < mid; i++) { L[nl] = i; nl += INCLUSIVE ? !(v[i] <= cut) : !(v[i] < cut); }
        for (int j = e - 1; j >= mid; j--) { R[nr] = j; nr += INCLUSIVE ? (v[j] <= cut) : (v[j] < cut); }
        for (int k = 0; k < nl; k++) swap_items(L[k], R[k]);   // (nl == nr)
        return mid;
    }
    // The same pass with AVX-512 where the host has it (round 6; the count and the two index lists are ~half of a build): sixteen
    // predicates per compare, the misplaced positions leave through vpcompressd.  Same permutation: the k-th misplaced position of the front
    // part (ascending) meets the k-th of the back part counted from the end.
    bool avx512_ = __builtin_cpu_supports("avx512f") && __builtin_cpu_supports("avx512vl") && !getenv("UH_KD_NO_AVX512");
    template <bool INCLUSIVE>
    __attribute__((target("avx512f,avx512vl,popcnt"))) int hoare_pass_avx512(int b, int e, const float* v, float cut) {
        const __m512 vc = _mm512_set1_ps(cut);
#define left_mask(i_, n_) _mm512_mask_cmp_ps_mask((__mmask16)((1u << (n_)) - 1u), _mm512_maskz_loadu_ps((__mmask16)((1u << (n_)) - 1u), v + (i_)), vc, INCLUSIVE ? _CMP_LE_OQ : _CMP_LT_OQ)   /* "belongs left" of v[i .. i + n), n <= 16 */
        int m = 0;
        for (int i = b; i < e; i += 16) m += __builtin_popcount(left_mask(i, std::min(16, e - i)));
        const int mid = b + m;
        if (m == 0 || mid == e) return mid;
        int* L = tmp_l_.data();
        int* R = tmp_r_.data();
        int nl = 0, nr = 0;
        const __m512i lane = _mm512_setr_epi32(0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15);
        for (int i = b; i < mid; i += 16) {
            const int n = std::min(16, mid - i);
            const __mmask16 mis = (__mmask16)(~left_mask(i, n) & ((1u << n) - 1u));
            _mm512_mask_compressstoreu_epi32(L + nl, mis, _mm512_add_epi32(lane, _mm512_set1_epi32(i)));
            nl += __builtin_popcount(mis);
        }
        for (int i = mid; i < e; i += 16) {   // ascending here; paired from the end below
            const int n = std::min(16, e - i);
            const __mmask16 mis = left_mask(i, n);
            _mm512_mask_compressstoreu_epi32(R + nr, mis, _mm512_add_epi32(lane, _mm512_set1_epi32(i)));
            nr += __builtin_popcount(mis);
        }
        for (int k = 0; k < nl; k++) swap_items(L[k], R[nr - 1 - k]);   // (nl == nr)
#undef left_mask
        return mid;
    }

    // picoflann.h:238-345.  `box` is in/out: on return it is the tight box of the subtree.
    void split(int node, int b, int e, Box& box, int depth) {
        max_depth = std::max(max_depth, depth);
        const int count = e - b;
        if (count <= kLeafMax) {
            nodes[node].leaf_begin = (int)leaf_idx.size();
            nodes[node].leaf_count = (short)count;
            for (int i = b; i < e; i++) leaf_idx.push_back(order_[i]);
            bounds(b, e, box);
            return;
        }
        const int lch = (int)nodes.size();
        nodes.push_back(KdNodeDev{0, 0, -1, -1, 0, 0, 0});
        nodes.push_back(KdNodeDev{0, 0, -1, -1, 0, 0, 0});
        double mean[2], var[2];
        sample_moments(b, e, mean, var);
        const int dim = var[1] > var[0] ? 1 : 0;
        double cut = mean[dim];
        // picoflann.h:403-424: two Hoare passes -> [< cut | == cut | > cut]
        const int lim1 = hoare_pass<false>(b, e, coords(dim), (float)cut) - b;
        const int lim2 = hoare_pass<true>(b + lim1, e, coords(dim), (float)cut) - b;
        int at = count / 2;
        if (lim1 > count / 2) at = lim1;
        else if (lim2 < count / 2) at = lim2;
        if (lim1 == count || lim2 == 0) at = count / 2;
        if (at < kLeafMax || count - at < kLeafMax) {
            // std::sort exactly where the reference uses it (same libstdc++ => same permutation of equal keys).  Up to 16 elements — most of
            // the nodes that come here hold 11..19 points — libstdc++'s std::sort IS its insertion sort (introsort's loop does nothing below
            // _S_threshold = 16, __final_insertion_sort is one guarded __insertion_sort): done here on the carried coordinates, no gathers
            // through the permutation in the comparisons and none behind them.
            if (count <= 16) {
                float* key = coords(dim); float* oth = coords(dim ^ 1);
                for (int i = b + 1; i < e; i++) {
                    const float k = key[i], o = oth[i];
                    const uint32_t id = order_[i];
                    int j = i;
                    if (k < key[b]) {   // (libstdc++ moves the whole prefix when the element is smaller than the first one: same result)
                        for (; j > b; j--) { key[j] = key[j - 1]; oth[j] = oth[j - 1]; order_[j] = order_[j - 1]; }
                    } else {
                        for (; k < key[j - 1]; j--) { key[j] = key[j - 1]; oth[j] = oth[j - 1]; order_[j] = order_[j - 1]; }
                    }
                    key[j] = k; oth[j] = o; order_[j] = id;
                }
            } else {
                const float* xy = xy_;
                std::sort(order_.begin() + b, order_.begin() + e, [xy, dim](const uint32_t& p, const uint32_t& q) { return xy[2 * (size_t)p + dim] < xy[2 * (size_t)q + dim]; });
                for (int i = b; i < e; i++) { px_[i] = xy[2 * (size_t)order_[i]]; py_[i] = xy[2 * (size_t)order_[i] + 1]; }
            }
            at = count / 2;
            cut = coords(dim)[b + at];
        }
        Box lbox = box, rbox = box;
        lbox.hi[dim] = cut;
        split(lch, b, b + at, lbox, depth + 1);
        lbox.hi[dim] = cut;
        rbox.lo[dim] = cut;
        split(lch + 1, b + at, e, rbox, depth + 1);
        KdNodeDev& nd = nodes[node];
        nd.left = lch; nd.right = lch + 1; nd.col = (short)dim;
        nd.divlow = (float)lbox.hi[dim];
        nd.divhigh = (float)rbox.lo[dim];
        for (int d = 0; d < 2; d++) { box.lo[d] = std::min(lbox.lo[d], rbox.lo[d]); box.hi[d] = std::max(lbox.hi[d], rbox.hi[d]); }
    }
};

// ---------------------------------------------------------------------------------------------------------- device
struct PmFrame {
    const uint64_t* kp_desc;        // n_kpts x 4
    const KdNodeDev* nodes;
    const float4* leaf_rec;         // n_kpts records in LEAF order: {x, y, bits(keypoint << 4 | octave), 0} — what a leaf visit needs, in one 16-byte read
                                    // (round 3 chased leaf index -> coordinates -> octave through three dependent LDS reads per visit)
    double box[4];
    const float* scale; int n_levels; int n_kpts;
    float fx, fy, cx, cy, min_x, min_y, max_x, max_y;
    float log_scale;
};

struct PmPoints {
    int n;
    // one 64-byte record per candidate, in the pinned staging block (read by the kernel in place): position (3 floats), then normal (3),
    // min / max distance — or, PREV mode, the previous frame's keypoint octave in word 3 —, then the 32-byte descriptor.  Five separate
    // arrays (rounds 3-5a) were five small reads over the host link per candidate — 15 000 requests for 3000 map points, ~6 us before a walk
    // could start; one record is one 64-byte request.
    const uint4* rec;
    int* best_kp; float* best_dist; unsigned char* visible;
    float4* pos_out;   // NULL, or HBM: every candidate's position again (uh_track_pose's look-ups gather from it instead of from pinned memory)
    const uint4* aux_in; uint4* aux_out;   // with pos_out: a 16-byte record per candidate the caller staged in pinned memory ({id, map row, weight, -}), moved to HBM likewise
};

struct PmPose { float T[12]; float cc[3]; };
struct PmDyn { PmPose ps; float radius; int skip; };   // a search whose pose / radius an earlier launch of the same stream decides (uh_track_pose); skip: nothing to do
// The call's hand-over, done by the kernel itself (round 5; rounds 3-4: a copy launch in front and a publish launch behind, ~6 us of kernel
// and a launch gap each): the candidates' arrays are read from the pinned staging block in place, the per-point results go to HBM with
// write-through (agent-scope) stores, every workgroup takes a ticket behind its acknowledged stores, and the workgroup that draws the last
// one copies the result block into pinned memory 8 bytes a lane, clears the ticket and the walk-overflow word for the next call and posts
// the completion word (one system-scope release).
struct PmPublish {
    unsigned* ticket;                          // HBM, 0 between calls
    const unsigned long long* dev_out; unsigned long long* host_out; unsigned n8;   // the result block in HBM, its pinned twin, 8-byte words
    unsigned long long* host_done; unsigned long long word;                        // pinned: completion word; word [1] low half receives the overflow flag
};

__device__ __forceinline__ float logf_cr(float x) { return uh_sincosf::logf_glibc(x); }   // libm's logf, bit for bit
__device__ __forceinline__ double readlane_f64(double v, int lane_uniform) {   // lane index must be wave-uniform
    const long long b = __double_as_longlong(v);
    const int lo = __builtin_amdgcn_readlane((int)(b & 0xffffffffll), lane_uniform);
    const int hi = __builtin_amdgcn_readlane((int)(b >> 32), lane_uniform);
    return __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
}

// Walk records (one per tree level at most): (other child << 2) | (col << 1) | state, with the other child's mindistsq, the
// cut distance and the float dists[col] to restore; state 0 = other child still to be searched, 1 = being searched (restore
// dists[col] when it is done).  The node to visit next is carried in registers (cur / cur_m), not pushed.
//
// Work decomposition: kGroup = 16 lanes per map point, 4 points per wave, 4 waves per workgroup; a workgroup stages the frame
// in LDS once and then loops over chunks of 16 map points.  The lanes of a group walk
// the tree together (identical control flow); in a leaf each lane tests ONE of its <= 10 keypoints, the hits are appended in
// leaf order (group ballot + prefix popcount) to the point's candidate list.  The list is drained by the 16 lanes in parallel
// (descriptor fetch + Hamming), then scanned in order for the best / second-best rule.  Compared with one lane per point this
// cuts the divergence (max over 4 instead of 64 walks per wave), parallelises the leaf and the L2 fetches, and fills 16x
// more SIMDs.
//
// LDS layout of a workgroup: [nodes | leaf records] when the frame fits (IN_LDS), then per group the
// walk stack (double m, int rec per level) and the candidate list ((keypoint << 4) | octave, then the Hamming distance).
// A frame of 2000 keypoints is ~40 KB, of 4000 ~80 KB: every node / leaf / coordinate access of the walk is an LDS access;
// only descriptors of disc hits come from L2.
// PREV = false: Map::matchFrameToMapPoints (map.cpp:689-759).  PREV = true: the tracker's search against the previous frame's
// keypoints (system.cpp:5930-6460): Frame::project visibility, the keypoint's own octave as the only admissible level, radius
// maxRepjDist * scaleFactors[octave], best/second without demotion from (float)(minDescDist + 0.01), accept best < 0.7 * second.
// LANE_STACK (levels <= 64, i.e. always but for pathological trees): the walk records live across the LANES of the point's wave — record i in
// lane i, pushed by a predicated move, popped by v_readlane with the (wave-uniform) stack pointer — instead of in LDS: a pop was three to four
// dependent LDS round trips of an iteration that has five.
template <bool IN_LDS, bool PREV, bool LANE_STACK>
__global__ __launch_bounds__(kPmThreads) void projmatch_kernel(PmFrame f, PmPoints mp, PmPose ps, float minDescDist, float maxRepjDist,
                                                               int n_nodes, int levels, int* overflow, PmPublish pub, const PmDyn* __restrict__ dyn) {
#include "projmatch_kernel_body.hpp"
}

// uh_relocalize_pose (relocalize.hpp): Map::matchFrameToMapPoints for several point lists in one launch — the list is blockIdx.y, its
// candidates, result arrays and pose / radius (PmDyn, written by an earlier launch of the stream) come from a device-visible table.  The
// workgroups of a list that is skipped, and those beyond its last chunk, leave at once; no hand-over (the caller's last launch publishes).
// The same text as projmatch_kernel's (projmatch_kernel_body.hpp) behind another head, so that kernel's code stays what it was.
struct PmBatchItem { PmPoints mp; const PmDyn* dyn; };
template <bool IN_LDS, bool LANE_STACK>
__global__ __launch_bounds__(kPmThreads) void projmatch_batch_kernel(PmFrame f, const PmBatchItem* __restrict__ items, float minDescDist, int n_nodes, int levels, int* overflow) {
    constexpr bool PREV = false;
    const PmBatchItem it = items[blockIdx.y];   // (pinned memory: read once, uniform)
    if (it.dyn->skip || (int)(blockIdx.x * (blockDim.x / kGroup)) >= it.mp.n) return;
    const PmPoints mp = it.mp;
    const PmDyn* __restrict__ dyn = it.dyn;
    PmPose ps{};
    float maxRepjDist = 0.f;
    const PmPublish pub{};   // (no ticket: the body returns in front of its hand-over, whose code the compiler drops — and warns about)
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wnonnull"
#include "projmatch_kernel_body.hpp"
#pragma clang diagnostic pop
}

}  // namespace

struct uh_projmatch {
    uh_ctx* ctx = nullptr;
    bool have_frame = false;
    int n_kpts = 0, n_levels = 0;
    PmFrame fr{};
    uh::DevBuf d_frame;    // kp_desc | nodes | leaf records | scale
    // pinned, device-visible staging: the frame block (set_frame), the points of a match call, its results + completion word.
    // Everything moves as 16-byte-wide launches on the context stream (uh::copy16 / publish16); the host never synchronises the stream.
    uh::MappedBuf h_frame;
    // the buffers of a match call: slot 0 serves uh_projmatch_match / _match_prev; uh_track_pose (track.hpp) enqueues its two searches
    // back to back without waiting in between and gives the second one slot 1
    struct Slot {
        uh::DevBuf d_points;          // status block | best_kp | best_dist | visible
        uh::MappedBuf h_in, h_out;    // the candidates' records (read by the kernel in place); results + completion word
        bool ovf_zeroed = false;
        unsigned ovf_gen = 0;
    } slot[2];
    unsigned long long seq = 0, frame_word = 0;   // completion words: of the last match call / of the last frame upload (posted only on demand, see upload_pending)
    // The frame upload (a copy launch reading the pinned staging block) needs no completion word of its own: every match call that follows
    // runs behind it on the same stream and the host waits for THAT call's word — which also proves the upload has been read.  Only two
    // set_frame calls with no match in between post and wait for a word (round 6: the word launch sat between the upload and the first
    // match of every frame, 4 us of dispatch on the tracker's critical path).
    bool upload_pending = false;
    std::vector<float> xy;
    std::vector<int> oct;
    std::vector<uh_dmatch> mm;
    KdBuilder kd;
    int n_nodes = 0, max_depth = 0;     // of the current frame's tree (built on the host by set_frame, on the device for set_frame_dev)
    uh_dev_frame* dev = nullptr;        // the current frame is this device-resident one (uh_projmatch_set_frame_dev)
    uh::DevBuf d_scale;                 // set_frame_dev: the scale factors (uploaded when they change)
    std::vector<float> scale_host;
    bool attr_set = false;
    struct uh_track_state* track = nullptr;   // uh_track_pose's buffers (track.hpp), created on first use
    void* reloc = nullptr;                    // uh_relocalize_pose's buffers (relocalize.hpp), created on first use with their deleter
    void (*reloc_free)(void*) = nullptr;
    ~uh_projmatch();
};

// The tree over the frame's undistorted keypoints, built by this core (uh_projmatch_set_frame; uh_projmatch_set_frame_dev with a host-built tree).
// t0: uh_projmatch_set_frame's UH_PM_TIMING clock, started in front of the build (NULL: no timing)
static int pm_build_tree(uh_projmatch* h, const uh_proj_frame* f, const char* what, std::chrono::steady_clock::time_point* t0) {
    const int n = f->n_kpts;
    h->xy.resize(2 * (size_t)std::max(n, 1));
    h->oct.resize(std::max(n, 1));
    for (int i = 0; i < n; i++) {
        // the kernel packs a candidate's octave into 4 bits and an int8: anything outside [0,16) would silently corrupt bestLevel / bestLevel2
        UH_REQUIRE(f->und_kpts[i].octave >= 0 && f->und_kpts[i].octave < 16, "%s: octave %d of keypoint %d outside [0,16)", what, f->und_kpts[i].octave, i);
        h->xy[2 * i] = f->und_kpts[i].x; h->xy[2 * i + 1] = f->und_kpts[i].y; h->oct[i] = f->und_kpts[i].octave;
    }
    if (t0) *t0 = std::chrono::steady_clock::now();
    h->kd.build(h->xy.data(), n);
    if (t0) fprintf(stderr, "kd build: %.1f us (n=%d, depth %d, nodes %zu)\n", std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - *t0).count(), n, h->kd.max_depth, h->kd.nodes.size());
    UH_REQUIRE(h->kd.max_depth <= kMaxDepth, "%s: kd-tree depth %d exceeds the walk stack (%d levels)", what, h->kd.max_depth, kMaxDepth);
    return UH_OK;
}

// the leaf records of the host-built tree, in leaf order: {x, y, bits(keypoint << 4 | octave), 0}
static void pm_leaf_records(const uh_projmatch* h, float* lr, int n) {
    for (int i = 0; i < n; i++) {
        const uint32_t id = h->kd.leaf_idx[i], io = (id << 4) | (uint32_t)h->oct[id];
        lr[4 * i] = h->xy[2 * (size_t)id]; lr[4 * i + 1] = h->xy[2 * (size_t)id + 1];
        std::memcpy(lr + 4 * i + 2, &io, 4); lr[4 * i + 3] = 0.f;
    }
}

// the matcher's frame from now on: its arrays and tree, and the camera / scale / image-bounds fields of f
static void pm_adopt(uh_projmatch* h, const uh_proj_frame* f, const void* desc, const void* nodes, const float4* leaf, const float* scale, const double* box, int n, int n_nodes,
                     int max_depth, uh_dev_frame* dev) {
    PmFrame& d = h->fr;
    d.kp_desc = reinterpret_cast<const uint64_t*>(desc); d.nodes = reinterpret_cast<const KdNodeDev*>(nodes); d.leaf_rec = leaf; d.scale = scale;
    for (int i = 0; i < 4; i++) d.box[i] = box[i];
    d.n_levels = f->n_levels; d.n_kpts = n;
    d.fx = f->fx; d.fy = f->fy; d.cx = f->cx; d.cy = f->cy;
    d.min_x = (float)f->min_x; d.min_y = (float)f->min_y; d.max_x = (float)f->max_x; d.max_y = (float)f->max_y;
    d.log_scale = f->n_levels > 1 ? std::log(f->scale_factors[1]) : 1.f;   // float overload = libm logf, as Frame::predictScale
    h->n_kpts = n; h->n_levels = f->n_levels;
    h->n_nodes = n_nodes; h->max_depth = max_depth; h->dev = dev;
    h->have_frame = true;
}

extern "C" {

int uh_projmatch_create(uh_ctx* ctx, uh_projmatch** out) {
    UH_REQUIRE(ctx && out, "uh_projmatch_create: NULL argument");
    uh_projmatch* h = new uh_projmatch();
    h->ctx = ctx;
    *out = h;
    return UH_OK;
}

void uh_projmatch_destroy(uh_projmatch* h) { delete h; }

// before the pinned staging block of the frame upload is written again: make sure the previous upload has been read (see upload_pending)
static int pm_staging_free(uh_projmatch* h, const char* what) {
    if (!h->upload_pending) return UH_OK;
    int rc;
    h->frame_word = ++h->seq;
    if ((rc = uh::post_host_word(h->ctx, h->h_frame.dev<unsigned long long>(), h->frame_word))) return rc;
    if ((rc = uh::wait_host_word(reinterpret_cast<volatile unsigned long long*>(h->h_frame.host<char>()), h->frame_word, h->ctx->stream, what))) return rc;
    h->upload_pending = false;
    return UH_OK;
}

int uh_projmatch_set_frame(uh_projmatch* h, const uh_proj_frame* f) {
    UH_REQUIRE(h && f, "uh_projmatch_set_frame: NULL argument");
    UH_REQUIRE(f->n_kpts >= 0 && (f->n_kpts == 0 || (f->und_kpts && f->desc)), "uh_projmatch_set_frame: keypoints / descriptors missing");
    UH_REQUIRE(f->n_levels >= 1 && f->scale_factors, "uh_projmatch_set_frame: scale factors missing");
    UH_HIP_CHECK(hipSetDevice(h->ctx->device));
    const int n = f->n_kpts;
    const bool timing = getenv("UH_PM_TIMING") != nullptr;   // (measurement: the build's and the call's time)
    std::chrono::steady_clock::time_point t0;
    int rc;
    if ((rc = pm_build_tree(h, f, "uh_projmatch_set_frame", timing ? &t0 : nullptr))) return rc;
    const size_t nn = h->kd.nodes.size();
    uh::Layout L;
    const size_t o_desc = L.take<uint8_t>(32 * (size_t)n), o_nodes = L.take<KdNodeDev>(nn), o_leaf = L.take<float4>(n), o_scale = L.take<float>(f->n_levels), total = L.take<char>(0);
    if ((rc = h->d_frame.reserve(total + 256))) return rc;
    char* base = h->d_frame.as<char>();
    {   // one pinned staging block, one 16-byte-wide copy launch, no synchronisation: the block is only reused by the NEXT set_frame,
        // which first makes sure this upload has landed (its completion word — long since posted unless two set_frame calls follow
        // each other with nothing in between)
        if ((rc = pm_staging_free(h, "uh_projmatch_set_frame"))) return rc;
        if ((rc = h->h_frame.reserve(total + 64))) return rc;
        char* hi = h->h_frame.host<char>() + 64;   // (the first 64 bytes hold the completion word)
        if (n) {
            std::memcpy(hi + o_desc, f->desc, 32 * (size_t)n);
            std::memcpy(hi + o_nodes, h->kd.nodes.data(), sizeof(KdNodeDev) * nn);
            pm_leaf_records(h, reinterpret_cast<float*>(hi + o_leaf), n);
        }
        std::memcpy(hi + o_scale, f->scale_factors, 4 * (size_t)f->n_levels);
        std::atomic_thread_fence(std::memory_order_release);
        if ((rc = uh::copy16(h->ctx, base, h->h_frame.dev<char>() + 64, total))) return rc;
        h->upload_pending = true;
    }
    if (timing) fprintf(stderr, "set_frame total: %.1f us (bytes %zu)\n", std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count(), total);
    pm_adopt(h, f, base + o_desc, base + o_nodes, reinterpret_cast<const float4*>(base + o_leaf), reinterpret_cast<const float*>(base + o_scale), h->kd.root_box, n, (int)nn,
             h->kd.max_depth, nullptr);
    return UH_OK;
}

// The frame the extractor left on the device (uh_orb_extract_frame_dev: descriptors, undistorted keypoints in leaf order, kd-tree built by
// kdbuild.hip) becomes the matcher's frame: no keypoints or descriptors cross the host link, no tree is built on the host.  `f` carries the
// camera / scale / image-bounds fields (desc is ignored; und_kpts / n_kpts too, but for a frame whose tree the host core builds).
int uh_projmatch_set_frame_dev(uh_projmatch* h, uh_dev_frame* fr, const uh_proj_frame* f) {
    UH_REQUIRE(h && fr && f, "uh_projmatch_set_frame_dev: NULL argument");
    UH_REQUIRE(fr->ctx == h->ctx, "uh_projmatch_set_frame_dev: the device frame belongs to another context");
    UH_REQUIRE(f->n_levels >= 1 && f->n_levels <= 16 && f->scale_factors, "uh_projmatch_set_frame_dev: scale factors missing");
    UH_HIP_CHECK(hipSetDevice(h->ctx->device));
    int rc;
    if (h->scale_host.size() != (size_t)f->n_levels || std::memcmp(h->scale_host.data(), f->scale_factors, 4 * (size_t)f->n_levels) != 0) {
        h->scale_host.assign(f->scale_factors, f->scale_factors + f->n_levels);
        if ((rc = h->d_scale.reserve(64))) return rc;
        UH_HIP_CHECK(hipMemcpyAsync(h->d_scale.p, h->scale_host.data(), 4 * (size_t)f->n_levels, hipMemcpyHostToDevice, h->ctx->stream));
    }
    if (fr->host_tree) {
        // the tree by this core (KdBuilder, as uh_projmatch_set_frame), nodes and leaf records uploaded into the frame object; the descriptors
        // and everything else stay where the extractor left them.  The keypoints must be the frame's own: as many as the host last learned
        // it has (a stale or foreign array would pair leaf ids with other keypoints' descriptors).
        const int n = f->n_kpts;
        UH_REQUIRE(n >= 0 && n == fr->n_known && n <= fr->n_cap && (n == 0 || f->und_kpts), "uh_projmatch_set_frame_dev: %d keypoints for a device frame of %d (host-built tree)",
                   n, fr->n_known);   // (n >= 0: an unknown count, n_known = -1, matches no request)
        if ((rc = pm_build_tree(h, f, "uh_projmatch_set_frame_dev", nullptr))) return rc;
        const size_t nn = h->kd.nodes.size(), gap = fr->o_leaf - fr->o_nodes, span = gap + 16 * (size_t)n;
        UH_REQUIRE(sizeof(KdNodeDev) * nn <= gap, "uh_projmatch_set_frame_dev: %zu nodes exceed the device frame's node block", nn);
        if ((rc = pm_staging_free(h, "uh_projmatch_set_frame_dev"))) return rc;
        if ((rc = h->h_frame.reserve(span + 64))) return rc;
        char* hi = h->h_frame.host<char>() + 64;   // (the first 64 bytes hold the completion word)
        if (n) {
            std::memcpy(hi, h->kd.nodes.data(), sizeof(KdNodeDev) * nn);
            pm_leaf_records(h, reinterpret_cast<float*>(hi + gap), n);
            std::atomic_thread_fence(std::memory_order_release);
            // (one launch over the node block and the leaf records: the unused tail of the node block travels with them — a few KB against a second launch)
            if ((rc = uh::copy16(h->ctx, reinterpret_cast<char*>(fr->nodes()), h->h_frame.dev<char>() + 64, span))) return rc;
            h->upload_pending = true;
        }
        pm_adopt(h, f, fr->desc(), fr->nodes(), fr->leaf(), h->d_scale.as<float>(), h->kd.root_box, n, (int)nn, h->kd.max_depth, fr);
        return UH_OK;
    }
    const uh_kd::Meta* m = nullptr;
    if ((rc = uh::dev_frame_wait(fr, &m, "uh_projmatch_set_frame_dev"))) return rc;   // (the build runs behind the extractor's completion word: normally done)
    UH_REQUIRE(m->max_depth <= kMaxDepth, "uh_projmatch_set_frame_dev: kd-tree depth %d exceeds the walk stack (%d levels)", m->max_depth, kMaxDepth);
    pm_adopt(h, f, fr->desc(), fr->nodes(), fr->leaf(), h->d_scale.as<float>(), m->box, m->n, m->n_nodes, m->max_depth, fr);
    return UH_OK;
}

// host-only test hook (no device call): the tree set_frame would build for these points.  nodes24_out: 2n+2 nodes of room.
int uh_kdtree_build_host(const float* xy, int32_t n, int32_t* n_nodes, void* nodes24_out, uint32_t* leaf_idx_out, double* root_box4, int32_t* max_depth) {
    UH_REQUIRE(n >= 0 && (n == 0 || xy) && n_nodes && nodes24_out && leaf_idx_out && root_box4, "uh_kdtree_build_host: bad arguments");
    KdBuilder kd;
    kd.build(xy, n);
    *n_nodes = (int32_t)kd.nodes.size();
    if (!kd.nodes.empty()) std::memcpy(nodes24_out, kd.nodes.data(), sizeof(KdNodeDev) * kd.nodes.size());
    if (n) std::memcpy(leaf_idx_out, kd.leaf_idx.data(), 4 * (size_t)n);
    std::memcpy(root_box4, kd.root_box, 32);
    if (max_depth) *max_depth = kd.max_depth;
    return UH_OK;
}

// flattened tree of the current frame (for tests: compared with the oracle's / the real picoflann's build)
int uh_projmatch_debug_tree(uh_projmatch* h, int32_t* n_nodes, const void** nodes24, const uint32_t** leaf_idx, double* root_box4, int32_t* max_depth) {
    UH_REQUIRE(h && h->have_frame, "uh_projmatch_debug_tree: no frame set");
    UH_REQUIRE(!h->dev, "uh_projmatch_debug_tree: the current frame is device-resident (use uh_dev_frame_tree)");
    if (n_nodes) *n_nodes = (int32_t)h->kd.nodes.size();
    if (nodes24) *nodes24 = h->kd.nodes.data();
    if (leaf_idx) *leaf_idx = h->kd.leaf_idx.data();
    if (root_box4) std::memcpy(root_box4, h->kd.root_box, 32);
    if (max_depth) *max_depth = h->kd.max_depth;
    return UH_OK;
}

}  // extern "C"

namespace {

// What a search leaves behind until its results are collected: where they lie (HBM) and the call's completion word.
struct PmPending {
    int n = 0, slot = 0; bool prev = false;
    unsigned long long word = 0;
    const int* d_best_kp = nullptr; const float* d_best_dist = nullptr;   // HBM (for launches behind this one on the same stream)
};

// A slot's blocks for n candidates: byte offsets.  d_points: [0, 256) the walk status word (overflow flag, UH_PM_CLK stamps, the publish
// ticket at +128), then best_kp | best_dist | visible, which the kernel's last workgroup copies to +64 of h_out (behind the completion word).
// h_in: the candidates' 64-byte records, then uh_track_pose's 16-byte {id, map row, weight} records.
struct PmSlotLayout { size_t bk, bd, vis, end, rec, aux, in_bytes; };
PmSlotLayout pm_slot_layout(int n) {
    PmSlotLayout L;
    uh::Layout d{256};
    L.bk = d.take<int>(n); L.bd = d.take<float>(n, 4); L.vis = d.take<unsigned char>(n, 4); L.end = d.take<char>(0);
    uh::Layout in;
    L.rec = in.take<uint4>(4 * (size_t)n); L.aux = in.take<uint4>(n, 16); L.in_bytes = in.off + 64;
    return L;
}

// The slot's buffers for n candidates (uh_track_pose reserves both slots before its first launch: a buffer that grows is freed, which
// synchronises the device)
int match_reserve(uh_projmatch* h, int slot, int n) {
    uh_projmatch::Slot& S = h->slot[slot];
    const PmSlotLayout L = pm_slot_layout(n);
    int rc = S.d_points.reserve(L.end + 256);
    if (!rc) rc = S.h_out.reserve(L.end - L.bk + 64);
    return rc ? rc : S.h_in.reserve(L.in_bytes);
}

// uh_track_pose's part of a search: each candidate's position and {id, map row, solver weight} record, left in HBM for the look-ups
struct PmTrack {
    const int32_t* rows;       // previous-frame items: row of the same point in the local map or -1 (NULL: all -1); a map candidate's row is its own
    const float* map_weight;   // per map row (NULL: all 1)
    const float* prev_weight;  // previous-frame items outside the local map (uh_track_pose_stereo; NULL: all 1)
    float4* pos_out; uint4* aux_out;
};

// The candidates as the kernel reads them: 64-byte records at rec; with trk also the 16-byte records {id, row of the same point in the local
// map, the solver weight of that row — or, outside the local map, the item's own} at aux
void pm_pack(char* rec_bytes, char* aux_bytes, const uh_map_points* mp, const uh_prev_points* pp, const PmTrack* trk) {
    const bool prev = pp != nullptr;
    const int n = prev ? pp->n : mp->n;
    const float* pos3d = prev ? pp->pos3d : mp->pos3d;
    const uint8_t* desc = prev ? pp->desc : mp->desc;
    if (trk) {
        const uint32_t* ids = prev ? pp->ids : mp->ids;
        uint32_t* ax = reinterpret_cast<uint32_t*>(aux_bytes);
        for (int i = 0; i < n; i++, ax += 4) {
            const int row = !prev ? i : trk->rows ? trk->rows[i] : -1;
            const float w = row >= 0 ? (trk->map_weight ? trk->map_weight[row] : 1.f) : (trk->prev_weight ? trk->prev_weight[i] : 1.f);
            ax[0] = ids[i]; std::memcpy(ax + 1, &row, 4); std::memcpy(ax + 2, &w, 4); ax[3] = 0;
        }
    }
    float* rec = reinterpret_cast<float*>(rec_bytes);
    for (int i = 0; i < n; i++, rec += 16) {
        rec[0] = pos3d[3 * i]; rec[1] = pos3d[3 * i + 1]; rec[2] = pos3d[3 * i + 2];
        if (prev) { std::memcpy(rec + 3, pp->octave + i, 4); rec[4] = rec[5] = rec[6] = rec[7] = 0.f; }
        else { rec[3] = mp->normal[3 * i]; rec[4] = mp->normal[3 * i + 1]; rec[5] = mp->normal[3 * i + 2]; rec[6] = mp->min_dist[i]; rec[7] = mp->max_dist[i]; }
        std::memcpy(rec + 8, desc + 32 * (size_t)i, 32);
    }
}

// Stage the candidates — the local map's points (mp: Map::matchFrameToMapPoints) or the previous frame's items (pp) — and enqueue the search
// (no waiting).  dyn != nullptr: pose and radius are read from device memory at launch time (written by an earlier launch of this stream).
int match_enqueue(uh_projmatch* h, int slot, const float* pose_f2g, const PmDyn* dyn, const uh_map_points* mp, const uh_prev_points* pp,
                  float min_desc_dist, float max_repj_dist, PmPending* pend, const PmTrack* trk = nullptr) {
    const bool prev = pp != nullptr;
    const int n = prev ? pp->n : mp->n;
    uh_projmatch::Slot& S = h->slot[slot];
    UH_HIP_CHECK(hipSetDevice(h->ctx->device));
    hipStream_t st = h->ctx->stream;
    int rc = match_reserve(h, slot, n);
    if (rc) return rc;
    const PmSlotLayout L = pm_slot_layout(n);
    char* base = S.d_points.as<char>();
    if (!S.ovf_zeroed || S.ovf_gen != S.d_points.gen) {   // the walk-overflow word: zero once per allocation, the kernel's last workgroup clears it after every call
        UH_HIP_CHECK(hipMemsetAsync(base, 0, 256, st));
        S.ovf_zeroed = true; S.ovf_gen = S.d_points.gen;
    }
    static const bool pm_clk = getenv("UH_PM_CLK") != nullptr;
    if (pm_clk) { const unsigned magic[2] = {0u, 0x434c4bu}; UH_HIP_CHECK(hipMemcpyAsync(base, magic, 8, hipMemcpyHostToDevice, st)); }
    static const bool pm_timing = getenv("UH_PM_TIMING") != nullptr;
    const auto t_pack0 = std::chrono::steady_clock::now();
    {   // one pinned staging block (the previous call's launches are complete: its results were awaited): the candidates as 64-byte records
        char* hi = S.h_in.host<char>();
        pm_pack(hi + L.rec, trk ? hi + L.aux : nullptr, mp, pp, trk);
        std::atomic_thread_fence(std::memory_order_release);
    }
    if (pm_timing) fprintf(stderr, "projmatch%s: packing %d records %.1f us\n", prev ? "_prev" : "", n, std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t_pack0).count());
    PmPoints P;
    P.n = n;
    P.rec = reinterpret_cast<const uint4*>(S.h_in.dev<char>() + L.rec);   // (read by the kernel where they lie: every wave fetches its own candidate once)
    P.best_kp = (int*)(base + L.bk); P.best_dist = (float*)(base + L.bd); P.visible = (unsigned char*)(base + L.vis);
    P.pos_out = trk ? trk->pos_out : nullptr;
    P.aux_in = reinterpret_cast<const uint4*>(S.h_in.dev<char>() + L.aux); P.aux_out = trk ? trk->aux_out : nullptr;
    PmPose ps{};
    if (pose_f2g) {
        const float* T = pose_f2g;
        for (int i = 0; i < 12; i++) ps.T[i] = T[i];
        // camCenter = pose_f2g.inv() * (0,0,0), se3transform.h:89-113
        const float m0 = T[0], m1 = T[4], m2 = T[8], m4 = T[1], m5 = T[5], m6 = T[9], m8 = T[2], m9 = T[6], m10 = T[10];
        const float m3 = -(T[3] * m0 + T[7] * m1 + T[11] * m2), m7 = -(T[3] * m4 + T[7] * m5 + T[11] * m6), m11 = -(T[3] * m8 + T[7] * m9 + T[11] * m10);
        ps.cc[0] = m0 * 0.f + m1 * 0.f + m2 * 0.f + m3;
        ps.cc[1] = m4 * 0.f + m5 * 0.f + m6 * 0.f + m7;
        ps.cc[2] = m8 * 0.f + m9 * 0.f + m10 * 0.f + m11;
    }
    {
        const int n_nodes = h->n_nodes, levels = h->max_depth + 2;
        // Points per workgroup (= waves: one point per wave).  The walk is issue-bound — ~70 instructions per tree step and point, whatever shares
        // the SIMD — so the points are spread over as many compute units as there are: 800 previous-frame items ran on 50 CUs at 16 per
        // workgroup (match_prev 58 us); every workgroup stages the frame itself (~80 KB from L2: 2-3 us), so not below 4.
        const int ncu = std::max(h->ctx->num_cus, 64);
        const int gpw = std::min(kGroupsMax, std::max(4, uh_div_up(n, ncu)));
        const size_t stack_bytes = (size_t)levels * gpw * 24 + (size_t)kCandCap * gpw * 8 + 64;
        const size_t tree_bytes = (((size_t)n_nodes * sizeof(KdNodeDev) + 15) & ~(size_t)15) + 16 * (size_t)h->n_kpts;
        const bool no_lds = getenv("UH_PROJMATCH_NO_LDS") != nullptr;   // env: test knob for the big-frame path (read per call: tests set it within a process)
        const bool in_lds = tree_bytes + stack_bytes <= kLdsBudget && !no_lds;
        const size_t lds = stack_bytes + (in_lds ? tree_bytes : 0);
        if (!h->attr_set) {
#define UH_PM_ATTR(A, B, C) UH_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(projmatch_kernel<A, B, C>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsBudget))
            UH_PM_ATTR(true, false, true); UH_PM_ATTR(false, false, true); UH_PM_ATTR(true, true, true); UH_PM_ATTR(false, true, true);
            UH_PM_ATTR(true, false, false); UH_PM_ATTR(false, false, false); UH_PM_ATTR(true, true, false); UH_PM_ATTR(false, true, false);
#undef UH_PM_ATTR
            h->attr_set = true;
        }
        const dim3 grid(std::min(uh_div_up(n, gpw), kPmMaxBlocks));
        int* d_ovf = (int*)base;
        const unsigned long long word = ++h->seq;
        const PmPublish pub{reinterpret_cast<unsigned*>(base + 128), reinterpret_cast<const unsigned long long*>(base + L.bk), reinterpret_cast<unsigned long long*>(S.h_out.dev<char>() + 64),
                            (unsigned)((L.end - L.bk) / 8), S.h_out.dev<unsigned long long>(), word};
        const bool lane_stack = levels <= kGroup;
#define UH_PM_LAUNCH(A, B, C) UH_LAUNCH(h->ctx, (projmatch_kernel<A, B, C>), grid, dim3(gpw * kGroup), lds, h->fr, P, ps, min_desc_dist, max_repj_dist, n_nodes, levels, d_ovf, pub, dyn)
        if (lane_stack) {
            if (in_lds && !prev) UH_PM_LAUNCH(true, false, true); else if (!prev) UH_PM_LAUNCH(false, false, true);
            else if (in_lds) UH_PM_LAUNCH(true, true, true); else UH_PM_LAUNCH(false, true, true);
        } else {
            if (in_lds && !prev) UH_PM_LAUNCH(true, false, false); else if (!prev) UH_PM_LAUNCH(false, false, false);
            else if (in_lds) UH_PM_LAUNCH(true, true, false); else UH_PM_LAUNCH(false, true, false);
        }
#undef UH_PM_LAUNCH
        pend->word = word;
    }
    UH_HIP_CHECK(hipGetLastError());
    pend->n = n; pend->slot = slot; pend->prev = prev;
    pend->d_best_kp = P.best_kp; pend->d_best_dist = P.best_dist;
    return UH_OK;
}

// Wait for a search and collect its per-candidate results (pinned block -> the caller's arrays, any may be NULL).
int match_collect(uh_projmatch* h, const PmPending& pd, const char* what, const int** bk_out, const float** bd_out, int32_t* best_kp_out, float* best_dist_out, uint8_t* visible_out) {
    uh_projmatch::Slot& S = h->slot[pd.slot];
    int rc;
    // results: the kernel's last workgroup copies [best_kp | best_dist | visible] and the overflow flag into pinned memory and posts the completion word
    if ((rc = uh::wait_host_word(reinterpret_cast<volatile unsigned long long*>(S.h_out.host<char>()), pd.word, h->ctx->stream, what))) {
        S.ovf_zeroed = false;   //  a launch that died may have left its ticket / overflow word behind: the next call clears the block again
        return rc;
    }
    h->upload_pending = false;   // (this call ran behind the frame upload on the same stream)
    static const bool pm_clk = getenv("UH_PM_CLK") != nullptr;
    if (pm_clk) {
        long long c[8];
        UH_HIP_CHECK(hipMemcpy(c, S.d_points.as<char>() + 16, sizeof(c), hipMemcpyDeviceToHost));
        fprintf(stderr, "projmatch%s workgroup 0 cycles: stage %lld  visibility+walk %lld (group 0: %lld loop iterations, %lld leaves)  final drain (%lld hits) %lld  tail %lld  total %lld\n",
                pd.prev ? "_prev" : "", c[1] - c[0], c[2] - c[1], c[6], c[7], c[5], c[3] - c[2], c[4] - c[3], c[4] - c[0]);
    }
    const PmSlotLayout L = pm_slot_layout(pd.n);
    const char* ho = S.h_out.host<char>() + 64;
    const int* bk = (const int*)ho;
    const float* bd = (const float*)(ho + (L.bd - L.bk));
    const unsigned char* vis = (const unsigned char*)(ho + (L.vis - L.bk));
    const int ovf = *reinterpret_cast<const int*>(S.h_out.host<char>() + 8);
    UH_REQUIRE(!ovf, "%s: kd-tree walk stack overflow", what);
    if (best_kp_out) std::memcpy(best_kp_out, bk, 4 * (size_t)pd.n);
    if (best_dist_out) std::memcpy(best_dist_out, bd, 4 * (size_t)pd.n);
    if (visible_out) std::memcpy(visible_out, vis, (size_t)pd.n);
    if (bk_out) *bk_out = bk;
    if (bd_out) *bd_out = bd;
    return UH_OK;
}

// one implementation behind uh_projmatch_match (mp) and uh_projmatch_match_prev (pp), their checks included (`what`: the entry's name)
int match_common(const char* what, uh_projmatch* h, const float* pose_f2g, const uh_map_points* mp, const uh_prev_points* pp, float min_desc_dist,
                 float max_repj_dist, uh_dmatch* matches_out, int32_t cap, int32_t* best_kp_out, float* best_dist_out, uint8_t* visible_out) {
    const int n = mp ? mp->n : pp ? pp->n : -1;
    UH_REQUIRE(h && h->have_frame, "%s: no frame set (call uh_projmatch_set_frame first)", what);
    UH_REQUIRE(pose_f2g && n >= 0, "%s: NULL / negative argument", what);
    UH_REQUIRE(max_repj_dist > 0, "%s: maxRepjDist must be > 0 (a non-positive radius turns the reference's search into an unbounded one)", what);
    if (n == 0) return 0;
    if (mp) UH_REQUIRE(mp->ids && mp->pos3d && mp->normal && mp->min_dist && mp->max_dist && mp->desc, "%s: map point arrays missing", what);
    else UH_REQUIRE(pp->ids && pp->pos3d && pp->octave && pp->desc, "%s: point arrays missing", what);
    UH_REQUIRE(matches_out && cap >= 0, "%s: output buffer missing", what);
    for (int i = 0; pp && i < n; i++)   // Frame::scaleFactors[octave] (system.cpp:6130): out of range is undefined in the reference
        UH_REQUIRE(pp->octave[i] >= 0 && pp->octave[i] < h->n_levels, "%s: octave %d of item %d outside [0,%d)", what, pp->octave[i], i, h->n_levels);
    PmPending pd;
    int rc = match_enqueue(h, 0, pose_f2g, nullptr, mp, pp, min_desc_dist, max_repj_dist, &pd);
    if (rc) return rc;
    const int* bk = nullptr; const float* bd = nullptr;
    if ((rc = match_collect(h, pd, "uh_projmatch_match", &bk, &bd, best_kp_out, best_dist_out, visible_out))) return rc;
    const uint32_t* ids = pp ? pp->ids : mp->ids;
    std::vector<uh_dmatch>& mm = h->mm;
    mm.clear();
    mm.reserve(n);
    for (int i = 0; i < n; i++)
        if (bk[i] >= 0) mm.push_back(uh_dmatch{bk[i], (int32_t)ids[i], -1, bd[i]});
    int k = mm.empty() ? 0 : uh_filter_ambiguous(mm.data(), (int)mm.size(), 0);
    if (k < 0) return k;
    UH_REQUIRE(k <= cap, "uh_projmatch_match: %d matches do not fit the output buffer (cap %d)", k, (int)cap);
    if (k) std::memcpy(matches_out, mm.data(), sizeof(uh_dmatch) * (size_t)k);
    return k;
}

}  // namespace

extern "C" {

int uh_projmatch_match(uh_projmatch* h, const float* pose_f2g, const uh_map_points* mp, float min_desc_dist, float max_repj_dist,
                       uh_dmatch* matches_out, int32_t cap, int32_t* best_kp_out, float* best_dist_out, uint8_t* visible_out) {
    return match_common("uh_projmatch_match", h, pose_f2g, mp, nullptr, min_desc_dist, max_repj_dist, matches_out, cap, best_kp_out, best_dist_out, visible_out);
}

int uh_projmatch_match_prev(uh_projmatch* h, const float* pose_f2g, const uh_prev_points* pp, float min_desc_dist, float max_repj_dist,
                            uh_dmatch* matches_out, int32_t cap, int32_t* best_kp_out, float* best_dist_out) {
    return match_common("uh_projmatch_match_prev", h, pose_f2g, nullptr, pp, min_desc_dist, max_repj_dist, matches_out, cap, best_kp_out, best_dist_out, nullptr);
}

}  // extern "C"

#include "track.hpp"
#include "relocalize.hpp"
