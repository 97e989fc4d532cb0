// The mapper's fuse search on MI355X (gfx950) behind the C ABI (uh_fuse_*): one projection search of MapManager's search-and-fuse step
// (src/utils/mapmanager.cpp, the private member that is ORB-SLAM's SearchInNeighbors) — the points of a table against ONE resident
// keyframe.  The caller (include/ucoslam_hip/adaptors.hpp: MapPointFuser; fuse.py: search_in_neighbors) runs one search per target
// keyframe and one for the second half and applies each search's events in between: within one search no point depends on another.
//
// Per point (fuse_math.hpp): the caller's skip, Frame::project(p, true, true), the distance from the global camera centre against the
// invariance range, viewCos, the level predicted by the NEW keyframe, the disc th * scaleFactors[level] (x widen below viewCos 0.98).
// Then Frame::getKeyPointsInRegion(p2d, radius, level - 1, level) — picoflann's radius walk in picoflann's order over the frame's
// kd-tree — and the first strict minimum of the Hamming distances below (float)(maxDescDistance + 1e-3).  There is no second-best rule.
//
// fuse_search_kernel: one point per wave, the frame (nodes + leaf records) staged in LDS per workgroup where it fits, the walk spread over
// the wave's lanes with the serial lane-stack walk behind it, hits drained 64 at a time, results to HBM and from there to pinned memory by
// the last workgroup (ticket + completion word) — the forms measured best for projmatch_kernel (projmatch.hip), restated here for the
// fuse rules; the matcher's kernel is untouched.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "common.hpp"
#include "devframe.hpp"
#include "fuse_host.hpp"
#include "fuse_math.hpp"

namespace {

constexpr size_t kLdsBudget = 150 * 1024;   // of the CU's 160 KB
constexpr int kThreads = 768;               // at most twelve waves share the LDS copy of the frame
constexpr int kWave = 64;                   // ONE point per wave
constexpr int kWavesMax = kThreads / kWave;
constexpr int kMaxBlocks = 768;
constexpr int kCandCap = 128;               // per-point list of disc hits between two drains
constexpr int kLeafMax = 10;                // picoflann _maxLeafSize
constexpr int kMaxLevels = 64;              // walk records live in the lanes of the point's wave: deeper trees are refused before the launch
constexpr int kMaxPoints = 1 << 20;         // rows of a point table (64 MB of pinned records)

using Node = uh_kd::Node24;

struct FuFrame {
    const uint64_t* kp_desc;        // n_kpts x 4
    const Node* nodes;
    const float4* leaf_rec;         // n_kpts records in LEAF order: {x, y, bits(keypoint << 4 | octave), 0}
    double box[4];
    int n_kpts, n_nodes;
    float scale[16];                // the searched frame's scaleFactors
};

struct FuPoints {
    int n;
    const uint4* rec;               // pinned: 64-byte records {pos3d, normal, min, max, descriptor}
    const unsigned char* skip;      // pinned, n bytes, or NULL
    int* best_kp; float* best_dist; unsigned char* status;   // HBM
};

struct FuPublish {
    unsigned* ticket;                          // HBM, 0 between calls
    int* overflow;                             // HBM, 0 between calls
    const unsigned long long* dev_out; unsigned long long* host_out; unsigned n8;   // the result block in HBM, its pinned twin, 8-byte words
    unsigned long long* host_done; unsigned long long word;                        // pinned: completion word; the 4 bytes at +8 receive the overflow flag
};

__device__ __forceinline__ double readlane_f64(double v, int lane_uniform) {
    const long long b = __double_as_longlong(v);
    const int lo = __builtin_amdgcn_readlane((int)(b & 0xffffffffll), lane_uniform);
    const int hi = __builtin_amdgcn_readlane((int)(b >> 32), lane_uniform);
    return __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
}

// LDS of a workgroup: [nodes | leaf records] when the frame fits (IN_LDS), then per wave the hit list ((keypoint << 4) | octave) and
// the Hamming distances of its entries.
template <bool IN_LDS>
__global__ __launch_bounds__(kThreads) void fuse_search_kernel(FuFrame f, FuPoints mp, uh_fusem::View vw, float thr, FuPublish pub) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tid = threadIdx.x, g = tid / kWave, gl = tid % kWave;
    const int nthr = (int)blockDim.x, gpw = nthr / kWave;
    const int n = f.n_kpts;
    size_t off = 0;
    Node* s_nodes = reinterpret_cast<Node*>(smem);
    if (IN_LDS) off += ((size_t)f.n_nodes * sizeof(Node) + 15) & ~(size_t)15;
    float4* s_rec = reinterpret_cast<float4*>(smem + off);
    if (IN_LDS) off += (size_t)n * 16;
    unsigned int* s_cand = reinterpret_cast<unsigned int*>(smem + off) + (size_t)g * kCandCap;
    off += (size_t)kCandCap * gpw * 4;
    int* s_hd = reinterpret_cast<int*>(smem + off) + (size_t)g * kCandCap;
    // the point of this wave's FIRST chunk is requested before the frame is staged: it lies in pinned host memory
    struct Cand { float P0, P1, P2, n0, n1, n2, mind, maxd; bool skip; uint64_t q0, q1, q2, q3; };
    auto load_cand = [&](int mc) {
        const uint4* r = mp.rec + 4 * (size_t)mc;
        const uint4 a = r[0], b = r[1], d0 = r[2], d1 = r[3];
        Cand c;
        c.skip = mp.skip ? mp.skip[mc] != 0 : false;
        c.P0 = __uint_as_float(a.x); c.P1 = __uint_as_float(a.y); c.P2 = __uint_as_float(a.z);
        c.n0 = __uint_as_float(a.w); c.n1 = __uint_as_float(b.x); c.n2 = __uint_as_float(b.y);
        c.mind = __uint_as_float(b.z); c.maxd = __uint_as_float(b.w);
        c.q0 = ((uint64_t)d0.y << 32) | d0.x; c.q1 = ((uint64_t)d0.w << 32) | d0.z; c.q2 = ((uint64_t)d1.y << 32) | d1.x; c.q3 = ((uint64_t)d1.w << 32) | d1.z;
        return c;
    };
    const int m_first = (int)blockIdx.x * gpw + g;
    const Cand c_first = load_cand(m_first < mp.n ? m_first : 0);
    if (IN_LDS) {
        // 16-byte loads, eight in flight per lane and round (the node block is 256-byte aligned and padded: the last chunk may run 8 bytes past the nodes)
        const uint4* gn = reinterpret_cast<const uint4*>(f.nodes);
        uint4* sn = reinterpret_cast<uint4*>(s_nodes);
        constexpr int U = 8;
        const int n16 = (f.n_nodes * (int)sizeof(Node) + 15) / 16;
        for (int i0 = tid; i0 < n16; i0 += U * nthr) {
            uint4 v[U];
#pragma unroll
            for (int u = 0; u < U; u++) { const int i = i0 + u * nthr; v[u] = gn[i < n16 ? i : 0]; }
#pragma unroll
            for (int u = 0; u < U; u++) { const int i = i0 + u * nthr; if (i < n16) sn[i] = v[u]; }
        }
        for (int i0 = tid; i0 < n; i0 += U * nthr) {
            float4 a[U];
#pragma unroll
            for (int u = 0; u < U; u++) { const int i = i0 + u * nthr; a[u] = f.leaf_rec[i < n ? i : 0]; }
#pragma unroll
            for (int u = 0; u < U; u++) { const int i = i0 + u * nthr; if (i < n) s_rec[i] = a[u]; }
        }
        __syncthreads();
    }
  for (int chunk = blockIdx.x; chunk * gpw < mp.n; chunk += gridDim.x) {
    const int m = chunk * gpw + g;
    const bool live = m < mp.n;
    const int mc = live ? m : 0;
    const Cand cd = chunk == (int)blockIdx.x ? c_first : load_cand(mc);
    // ---- fuse_math.hpp: status and disc (identical in the lanes of the wave)
    uh_fusem::Disc dc{0.f, 0.f, 0, 0.f};
    unsigned char st = uh_fusem::point_disc(vw, f.scale, cd.skip, cd.P0, cd.P1, cd.P2, cd.n0, cd.n1, cd.n2, cd.mind, cd.maxd, dc);
    const bool search = live && st == uh_fusem::kFound;
    const float px = dc.px, py = dc.py;
    const int level = dc.level, oct_lo = dc.level - 1;
    const double worst = (double)dc.radius * (double)dc.radius;
    int best_kp = -1;
    float best_d = thr;
    bool ovf = false;
    const uint64_t q0 = cd.q0, q1 = cd.q1, q2 = cd.q2, q3 = cd.q3;
    int ncand = 0;
    // drain: Hamming distances of the listed hits (one hit per lane and round), then the first strict minimum in list order
    auto drain = [&](int cnt) {
        for (int k = gl; k < cnt; k += kWave) {
            const uint64_t* kd = f.kp_desc + 4 * (size_t)(s_cand[k] >> 4);
            s_hd[k] = __popcll(q0 ^ kd[0]) + __popcll(q1 ^ kd[1]) + __popcll(q2 ^ kd[2]) + __popcll(q3 ^ kd[3]);
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        for (int k = 0; k < cnt; k++) {
            const float hd = (float)s_hd[k];
            const bool isbest = hd < best_d;
            best_kp = isbest ? (int)(s_cand[k] >> 4) : best_kp;
            best_d = isbest ? hd : best_d;
        }
        __builtin_amdgcn_wave_barrier();   // the list is rewritten after this
    };
    if (search && n > 0 && worst > 0) {
        // computeInitialDistances (float accumulator)
        double dd0 = 0, dd1 = 0;
        float distsq = 0.f;
        {
            const double ex = px, ey = py;
            if (ex < f.box[0]) { const double d = ex - f.box[0]; dd0 = d * d; distsq += dd0; }
            if (ex > f.box[1]) { const double d = ex - f.box[1]; dd0 = d * d; distsq += dd0; }
            if (ey < f.box[2]) { const double d = ey - f.box[2]; dd1 = d * d; distsq += dd1; }
            if (ey > f.box[3]) { const double d = ey - f.box[3]; dd1 = d * d; distsq += dd1; }
        }
        // ---- the walk of ONE point spread over the lanes of its wave.  A radius search never changes `worst`, and what a node sees — mindistsq
        // and the two dists[] entries — depends on the path from the root only, so the subtrees are expanded side by side: lane 0 starts at the
        // root, every lane follows its best-child chain down to a leaf, and an "other" child that must be searched too is handed to a free lane.
        // A lane's path is its KEY (bit 63 - depth set where it was the other child); the leaves' depth-first order, which the hit list must keep
        // (the first strict minimum is order-dependent), is the order of the keys.  More than 64 leaves or levels: the serial walk below.
        bool walked = false;
        {
            int node = gl == 0 ? 0 : -1;      // >= 0: node to expand; -1: free lane; -2: this lane has reached its leaf
            double pm = (double)distsq, pd0 = dd0, pd1 = dd1;
            unsigned long long key = 0;
            int lbeg = 0, lcnt = 0;
            int nl = 1;                       // lanes in use (wave-uniform)
            bool fits = true;
            for (int depth = 0;; ++depth) {
                const bool act = node >= 0;
                if (__ballot(act) == 0) break;
                if (depth >= 64) { fits = false; break; }
                const int nsafe = act ? node : 0;
                const uint2* np = reinterpret_cast<const uint2*>(IN_LDS ? s_nodes + nsafe : f.nodes + nsafe);
                uint2 w0 = np[0], w1 = np[1], w2 = np[2];
                asm volatile("" : "+v"(w0.x), "+v"(w0.y), "+v"(w1.x), "+v"(w1.y), "+v"(w2.x), "+v"(w2.y));
                const float divlow = __uint_as_float(w0.x), divhigh = __uint_as_float(w0.y);
                const int left = (int)w1.x, right = (int)w1.y;
                const int col = (int)(w2.y >> 16);
                const bool isleaf = left < 0;
                if (act && isleaf) { lbeg = (int)w2.x; lcnt = (int)(w2.y & 0xFFFFu); node = -2; }
                const bool inner = act && !isleaf;
                const double val = col == 0 ? px : py;
                const double diff1 = val - divlow, diff2 = val - divhigh;
                const bool go_left = diff1 + diff2 < 0;
                const double cut = go_left ? diff2 * diff2 : diff1 * diff1;
                const float dst = (float)(col == 0 ? pd0 : pd1);
                const double m2 = pm + cut - dst;
                const bool wantB = inner && (m2 * 1.0 <= worst);
                const unsigned long long mb = __ballot(wantB);
                const int cntB = __popcll(mb);
                if (nl + cntB > kWave) { fits = false; break; }
                if (cntB) {
                    int src = gl, k = 0;      // receiving lane nl + k pulls from the k-th lane that hands a child over
                    for (unsigned long long t = mb; t; t &= t - 1, ++k) { const int b = __builtin_ctzll(t); src = gl == nl + k ? b : src; }
                    const int bnode = go_left ? right : left;
                    const double bd0 = col == 0 ? cut : pd0, bd1 = col == 0 ? pd1 : cut;
                    const unsigned long long bkey = key | (1ull << (63 - depth));
                    const int sa = src << 2;
                    auto pull64 = [&](unsigned long long v) {
                        const unsigned lo = (unsigned)__builtin_amdgcn_ds_bpermute(sa, (int)(unsigned)v), hi = (unsigned)__builtin_amdgcn_ds_bpermute(sa, (int)(unsigned)(v >> 32));
                        return ((unsigned long long)hi << 32) | lo;
                    };
                    const int r_node = __builtin_amdgcn_ds_bpermute(sa, bnode);
                    const double r_m = __longlong_as_double((long long)pull64((unsigned long long)__double_as_longlong(m2)));
                    const double r_d0 = __longlong_as_double((long long)pull64((unsigned long long)__double_as_longlong(bd0)));
                    const double r_d1 = __longlong_as_double((long long)pull64((unsigned long long)__double_as_longlong(bd1)));
                    const unsigned long long r_key = pull64(bkey);
                    if (gl >= nl && gl < nl + cntB) { node = r_node; pm = r_m; pd0 = r_d0; pd1 = r_d1; key = r_key; }
                    nl += cntB;
                }
                if (inner) node = go_left ? left : right;   // the best child: same mindistsq, same dists, same key
            }
            if (fits) {
                walked = true;
                // every used lane holds one leaf.  Its slots' place in the depth-first order: the leaf counts of all leaves with a smaller key
                int loff = 0, total = 0;
                for (int j = 0; j < nl; j++) {
                    const unsigned long long kj = ((unsigned long long)(unsigned)__builtin_amdgcn_readlane((int)(unsigned)(key >> 32), j) << 32) | (unsigned)__builtin_amdgcn_readlane((int)(unsigned)key, j);
                    const int cj = __builtin_amdgcn_readlane(lcnt, j);
                    loff += kj < key ? cj : 0;
                    total += cj;
                }
                for (int s0 = 0; s0 < total; s0 += kWave) {
                    const int sidx = s0 + gl;
                    int kp = -1;
                    for (int j = 0; j < nl; j++) {
                        const int oj = __builtin_amdgcn_readlane(loff, j), cj = __builtin_amdgcn_readlane(lcnt, j), bj = __builtin_amdgcn_readlane(lbeg, j);
                        kp = (sidx >= oj && sidx < oj + cj) ? bj + (sidx - oj) : kp;
                    }
                    bool hit = false;
                    unsigned int id = 0;
                    int oc = 0;
                    if (kp >= 0) {
                        const float4 c = IN_LDS ? s_rec[kp] : f.leaf_rec[kp];
                        const unsigned io = __float_as_uint(c.z);
                        id = io >> 4; oc = (int)(io & 15u);
                        const double dx = px - c.x;
                        double sqd = dx * dx;
                        if (!(sqd > worst)) { const double dy = py - c.y; sqd += dy * dy; }
                        hit = sqd < worst && oc >= oct_lo && oc <= level;
                    }
                    const unsigned long long hm = __ballot(hit);
                    if (hit) s_cand[ncand + (int)__builtin_amdgcn_mbcnt_hi((unsigned)(hm >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)hm, 0u))] = (id << 4) | (unsigned int)oc;
                    ncand += __popcll(hm);
                    if (ncand > kCandCap - kWave) { drain(ncand); ncand = 0; }
                }
            }
        }
        // ---- the serial walk: records (other child << 2) | (col << 1) | state with the other child's mindistsq, the cut distance and the float
        // dists[col] to restore; record i lives in lane i (pushed by a predicated move, popped by v_readlane with the wave-uniform stack pointer)
        int sp = 0;
        int l_rec = 0; double l_m = 0, l_c = 0; float l_d = 0;
        int cur = walked ? -1 : 0;   // node to visit (-1: take the top record)
        double cur_m = (double)distsq;
        for (;;) {
            if (walked) break;
            if (cur < 0) {
                if (sp == 0) break;
                const int top = __builtin_amdgcn_readfirstlane(sp) - 1;
                const int rec = __builtin_amdgcn_readlane(l_rec, top);
                const int col = (rec >> 1) & 1;
                if (rec & 1) {       // the other child's subtree is done: dists[col] = dst
                    const double dstd = (double)__uint_as_float((unsigned)__builtin_amdgcn_readlane((int)__float_as_uint(l_d), top));
                    if (col == 0) dd0 = dstd; else dd1 = dstd;
                    --sp;
                    continue;
                }
                const double cutv = readlane_f64(l_c, top);   // enter the other child: dists[col] = cut
                if (col == 0) dd0 = cutv; else dd1 = cutv;
                cur = rec >> 2;
                cur_m = readlane_f64(l_m, top);
                if (gl == top) l_rec = rec | 1;
            }
            Node nd;
            {
                const uint2* np = reinterpret_cast<const uint2*>(IN_LDS ? s_nodes + cur : f.nodes + cur);
                uint2 w0 = np[0], w1 = np[1], w2 = np[2];
                asm volatile("" : "+v"(w0.x), "+v"(w0.y), "+v"(w1.x), "+v"(w1.y), "+v"(w2.x), "+v"(w2.y));
                nd.divlow = __uint_as_float(w0.x); nd.divhigh = __uint_as_float(w0.y);
                nd.left = (int)w1.x; nd.right = (int)w1.y; nd.leaf_begin = (int)w2.x;
                nd.leaf_count = (short)(w2.y & 0xFFFFu); nd.col = (short)(w2.y >> 16);
            }
            if (nd.left < 0) {   // leaf: lane i tests keypoint i; hits are appended in leaf order
                bool hit = false;
                unsigned int id = 0;
                int oc = 0;
                if (gl < nd.leaf_count) {
                    const float4 c = IN_LDS ? s_rec[nd.leaf_begin + gl] : f.leaf_rec[nd.leaf_begin + gl];
                    const unsigned io = __float_as_uint(c.z);
                    id = io >> 4; oc = (int)(io & 15u);
                    const double dx = px - c.x;
                    double sqd = dx * dx;
                    if (!(sqd > worst)) { const double dy = py - c.y; sqd += dy * dy; }
                    hit = sqd < worst && oc >= oct_lo && oc <= level;
                }
                const unsigned long long hm = __ballot(hit);
                if (hit) s_cand[ncand + (int)__builtin_amdgcn_mbcnt_hi((unsigned)(hm >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)hm, 0u))] = (id << 4) | (unsigned int)oc;
                ncand += __popcll(hm);
                if (ncand > kCandCap - kLeafMax) { drain(ncand); ncand = 0; }
                cur = -1;
                continue;
            }
            const double val = nd.col == 0 ? px : py;
            const double diff1 = val - nd.divlow, diff2 = val - nd.divhigh;
            const bool go_left = diff1 + diff2 < 0;
            const double cut = go_left ? diff2 * diff2 : diff1 * diff1;
            const float dst = (float)(nd.col == 0 ? dd0 : dd1);
            const double m2 = cur_m + cut - dst;
            if (m2 * 1.0 <= worst) {
                if (sp >= kMaxLevels) { ovf = true; break; }
                const int nrec = ((go_left ? nd.right : nd.left) << 2) | ((int)nd.col << 1);
                if (gl == sp) { l_rec = nrec; l_m = m2; l_c = cut; l_d = dst; }
                sp++;
            }
            cur = go_left ? nd.left : nd.right;   // best child, same mindistsq
        }
    }
    if (!ovf) drain(ncand);
    if (ovf) { if (gl == 0) __hip_atomic_store(pub.overflow, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); best_kp = -1; best_d = thr; }
    if (st == uh_fusem::kFound && best_kp < 0) st = uh_fusem::kNoKeypoint;
    if (live && gl == 0) {   // (write-through: the publishing workgroup may sit on another XCD)
        __hip_atomic_store(mp.best_kp + m, best_kp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(mp.best_dist + m, best_d, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(mp.status + m, st, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
    // ---- hand-over: ticket behind this workgroup's acknowledged stores; the last workgroup publishes
    __shared__ int s_last;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) s_last = __hip_atomic_fetch_add(pub.ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == gridDim.x - 1 ? 1 : 0;
    __syncthreads();
    if (!s_last) return;
    for (unsigned i = threadIdx.x; i < pub.n8; i += 4 * (unsigned)nthr) {   // four words in flight per lane
        unsigned long long v[4];
#pragma unroll
        for (int u = 0; u < 4; u++) if (i + u * nthr < pub.n8) v[u] = __hip_atomic_load(pub.dev_out + i + u * nthr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
        for (int u = 0; u < 4; u++) if (i + u * nthr < pub.n8) __hip_atomic_store(pub.host_out + i + u * nthr, v[u], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
    if (threadIdx.x == 0) {
        const int ov = __hip_atomic_load(pub.overflow, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        reinterpret_cast<unsigned*>(pub.host_done)[2] = (unsigned)ov;      // the status word travels in the header, behind the completion word
        __hip_atomic_store(pub.overflow, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(pub.ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");   // every thread: its stores into pinned memory before the word
    __syncthreads();
    if (threadIdx.x == 0) __hip_atomic_store(pub.host_done, pub.word, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

// byte offsets of the result block for n points: best_kp | best_dist | status, each 8-byte aligned
struct ResLayout { size_t bk, bd, st, end; };
ResLayout res_layout(int n) {
    ResLayout L;
    uh::Layout d;
    L.bk = d.take<int>(n, 8); L.bd = d.take<float>(n, 8); L.st = d.take<unsigned char>(n, 8); L.end = (d.off + 7) & ~(size_t)7;
    return L;
}

}  // namespace

struct uh_fuse {
    uh_ctx* ctx = nullptr;
    int n = -1;                      // rows of the point table (-1: none set)
    uh::MappedBuf h_points;          // 64-byte records, read by the kernel in place
    uh::MappedBuf h_skip;            // the call's skip bytes
    uh::MappedBuf h_out;             // [completion word, overflow flag : 64 bytes | results]
    uh::DevBuf d_out;                // [ticket, overflow : 256 bytes | results]
    bool zeroed = false; unsigned zeroed_gen = 0;
    unsigned long long seq = 0;
    uh_dev_frame* own = nullptr;     // target == NULL: the caller's host arrays, uploaded here
    bool attr_set = false;
    std::vector<uint8_t> tree_nodes; std::vector<uint32_t> tree_leaf; std::vector<float> tree_xy, tree_rec;   // a host-built tree on its way into a device frame
    ~uh_fuse() { if (own) uh_dev_frame_destroy(own); }
};

namespace {

void pack_row(float* rec, const uh_map_points* p, int i) {
    rec[0] = p->pos3d[3 * (size_t)i]; rec[1] = p->pos3d[3 * (size_t)i + 1]; rec[2] = p->pos3d[3 * (size_t)i + 2];
    rec[3] = p->normal[3 * (size_t)i]; rec[4] = p->normal[3 * (size_t)i + 1]; rec[5] = p->normal[3 * (size_t)i + 2];
    rec[6] = p->min_dist[i]; rec[7] = p->max_dist[i];
    std::memcpy(rec + 8, p->desc + 32 * (size_t)i, 32);
}

// what both forms check before anything else, and the view they share
int fuse_view(const char* what, const uh_proj_frame* tp, const float* pose_f2g, const float* predict_scale_factors, int predict_n_levels, float th, float widen,
              uh_fusem::View* v) {
    UH_REQUIRE(tp && pose_f2g && predict_scale_factors, "%s: NULL argument", what);
    UH_REQUIRE(tp->n_levels >= 1 && tp->n_levels <= 16 && tp->scale_factors, "%s: the target's scale factors are missing or more than 16", what);
    UH_REQUIRE(predict_n_levels >= 2, "%s: predict_n_levels %d < 2 (Frame::predictScale reads scaleFactors[1])", what, predict_n_levels);
    UH_REQUIRE(predict_n_levels <= tp->n_levels, "%s: predict_n_levels %d > the target's %d levels (the reference would index past the target's scaleFactors)", what,
               predict_n_levels, tp->n_levels);
    UH_REQUIRE(th >= 0 && widen > 0, "%s: th must be >= 0 (0 = 2.5) and widen > 0", what);
    for (int i = 0; i < 12; i++) v->T[i] = pose_f2g[i];
    uh_fusem::camera_center(pose_f2g, v->cc);
    v->fx = tp->fx; v->fy = tp->fy; v->cx = tp->cx; v->cy = tp->cy;
    v->min_x = (float)tp->min_x; v->min_y = (float)tp->min_y; v->max_x = (float)tp->max_x; v->max_y = (float)tp->max_y;
    v->log_scale = std::log(predict_scale_factors[1]);   // float overload = libm logf, as Frame::predictScale
    v->predict_levels = predict_n_levels;
    v->th = th == 0 ? 2.5f : th; v->widen = widen;
    return UH_OK;
}

int check_keypoints(const char* what, const uh_proj_frame* tp) {
    UH_REQUIRE(tp->n_kpts >= 0 && (tp->n_kpts == 0 || (tp->und_kpts && tp->desc)), "%s: keypoints / descriptors missing", what);
    for (int i = 0; i < tp->n_kpts; i++)
        UH_REQUIRE(tp->und_kpts[i].octave >= 0 && tp->und_kpts[i].octave < 16, "%s: octave %d of keypoint %d outside [0,16)", what, tp->und_kpts[i].octave, i);
    return UH_OK;
}

// picoflann's tree over the keypoints of tp, by this core (uh_kdtree_build_host)
int build_host_tree(const char* what, const uh_proj_frame* tp, std::vector<uint8_t>& nodes, std::vector<uint32_t>& leaf, std::vector<float>& xy, double box[4], int* n_nodes,
                    int* max_depth) {
    const int n = tp->n_kpts;
    xy.resize(2 * (size_t)std::max(n, 1));
    for (int i = 0; i < n; i++) { xy[2 * (size_t)i] = tp->und_kpts[i].x; xy[2 * (size_t)i + 1] = tp->und_kpts[i].y; }
    nodes.resize(24 * (2 * (size_t)n + 2));
    leaf.resize(std::max(n, 1));
    int32_t nn = 0, md = 0;
    const int rc = uh_kdtree_build_host(xy.data(), n, &nn, nodes.data(), leaf.data(), box, &md);
    if (rc) return rc;
    UH_REQUIRE(md + 2 <= kMaxLevels, "%s: kd-tree depth %d exceeds the walk stack (%d levels)", what, md, kMaxLevels - 2);
    *n_nodes = nn; *max_depth = md;
    return UH_OK;
}

}  // namespace

extern "C" {

int uh_fuse_create(uh_ctx* ctx, uh_fuse** out) {
    UH_REQUIRE(ctx && out, "uh_fuse_create: NULL argument");
    uh_fuse* h = new uh_fuse();
    h->ctx = ctx;
    *out = h;
    return UH_OK;
}

void uh_fuse_destroy(uh_fuse* f) { delete f; }

int32_t uh_fuse_max_points(void) { return kMaxPoints; }

int uh_fuse_set_points(uh_fuse* h, const uh_map_points* p) {
    UH_REQUIRE(h && p, "uh_fuse_set_points: NULL argument");
    UH_REQUIRE(p->n >= 0 && p->n <= kMaxPoints, "uh_fuse_set_points: %d points outside [0, %d]", p->n, kMaxPoints);
    UH_REQUIRE(p->n == 0 || (p->pos3d && p->normal && p->min_dist && p->max_dist && p->desc), "uh_fuse_set_points: map point arrays missing");
    UH_HIP_CHECK(hipSetDevice(h->ctx->device));
    h->n = -1;
    int rc = h->h_points.reserve(64 * (size_t)std::max(p->n, 1));
    if (rc) return rc;
    float* rec = h->h_points.host<float>();
    for (int i = 0; i < p->n; i++, rec += 16) pack_row(rec, p, i);
    std::atomic_thread_fence(std::memory_order_release);
    h->n = p->n;
    return UH_OK;
}

int uh_fuse_update_points(uh_fuse* h, int32_t n_rows, const int32_t* rows, const uh_map_points* nv) {
    UH_REQUIRE(h && h->n >= 0, "uh_fuse_update_points: no point table set (call uh_fuse_set_points first)");
    UH_REQUIRE(n_rows >= 0 && (n_rows == 0 || (rows && nv)), "uh_fuse_update_points: NULL / negative argument");
    if (n_rows == 0) return UH_OK;
    UH_REQUIRE(nv->n == n_rows && nv->pos3d && nv->normal && nv->min_dist && nv->max_dist && nv->desc, "uh_fuse_update_points: new_values must hold n_rows = %d points", n_rows);
    for (int k = 0; k < n_rows; k++) UH_REQUIRE(rows[k] >= 0 && rows[k] < h->n, "uh_fuse_update_points: rows[%d] = %d outside the table of %d", k, rows[k], h->n);
    for (int k = 0; k < n_rows; k++) pack_row(h->h_points.host<float>() + 16 * (size_t)rows[k], nv, k);
    std::atomic_thread_fence(std::memory_order_release);
    return UH_OK;
}

int uh_fuse_search(uh_fuse* h, uh_dev_frame* target, const uh_proj_frame* tp, const float* pose_f2g, const float* predict_scale_factors, int32_t predict_n_levels,
                   const uint8_t* skip, float th, float widen, float max_desc_dist, int32_t* best_kp_out, float* best_dist_out, uint8_t* status_out) {
    const char* what = "uh_fuse_search";
    UH_REQUIRE(h && h->n >= 0, "%s: no point table set (call uh_fuse_set_points first)", what);
    uh_fusem::View vw;
    int rc = fuse_view(what, tp, pose_f2g, predict_scale_factors, predict_n_levels, th, widen, &vw);
    if (rc) return rc;
    const int n = h->n;
    UH_REQUIRE(n == 0 || (best_kp_out && best_dist_out && status_out), "%s: output arrays missing", what);
    UH_HIP_CHECK(hipSetDevice(h->ctx->device));
    hipStream_t st = h->ctx->stream;
    // ---- the frame
    if (!target) {   // utility path: the host arrays into a frame object of the handle's own
        if ((rc = check_keypoints(what, tp))) return rc;
        UH_REQUIRE(tp->n_kpts <= uh_kd::kDevMaxPoints, "%s: %d keypoints exceed a device frame's %d", what, tp->n_kpts, uh_kd::kDevMaxPoints);
        if (!h->own && (rc = uh_dev_frame_create(h->ctx, &h->own))) return rc;
        if ((rc = uh_dev_frame_upload(h->own, tp->und_kpts, tp->n_kpts, tp->desc))) return rc;
        target = h->own;
    }
    UH_REQUIRE(target->ctx == h->ctx, "%s: the device frame belongs to another context", what);
    FuFrame fr{};
    int max_depth = 0;
    if (target->host_tree) {
        const int nk = tp->n_kpts;
        UH_REQUIRE(nk >= 0 && nk == target->n_known && nk <= target->n_cap && (nk == 0 || tp->und_kpts), "%s: %d keypoints for a device frame of %d (host-built tree)", what, nk,
                   target->n_known);
        for (int i = 0; i < nk; i++)
            UH_REQUIRE(tp->und_kpts[i].octave >= 0 && tp->und_kpts[i].octave < 16, "%s: octave %d of keypoint %d outside [0,16)", what, tp->und_kpts[i].octave, i);
        int nn = 0;
        if ((rc = build_host_tree(what, tp, h->tree_nodes, h->tree_leaf, h->tree_xy, fr.box, &nn, &max_depth))) return rc;
        UH_REQUIRE(24 * (size_t)nn <= target->o_leaf - target->o_nodes, "%s: %d nodes exceed the device frame's node block", what, nn);
        if (nk) {
            h->tree_rec.resize(4 * (size_t)nk);
            for (int i = 0; i < nk; i++) {
                const uint32_t id = h->tree_leaf[i], io = (id << 4) | (uint32_t)tp->und_kpts[id].octave;
                h->tree_rec[4 * (size_t)i] = tp->und_kpts[id].x; h->tree_rec[4 * (size_t)i + 1] = tp->und_kpts[id].y;
                std::memcpy(&h->tree_rec[4 * (size_t)i + 2], &io, 4); h->tree_rec[4 * (size_t)i + 3] = 0.f;
            }
            UH_HIP_CHECK(hipMemcpyAsync(target->nodes(), h->tree_nodes.data(), 24 * (size_t)nn, hipMemcpyHostToDevice, st));
            UH_HIP_CHECK(hipMemcpyAsync(target->leaf(), h->tree_rec.data(), 16 * (size_t)nk, hipMemcpyHostToDevice, st));
            UH_HIP_CHECK(hipStreamSynchronize(st));   // (the staging vectors are pageable and reused by the next call)
        }
        fr.n_kpts = nk; fr.n_nodes = nn;
    } else {
        const uh_kd::Meta* m = nullptr;
        UH_REQUIRE(target->seq != 0, "%s: the device frame holds no complete kd-tree (no extraction or upload yet)", what);
        if ((rc = uh::dev_frame_wait(target, &m, what))) return rc;
        UH_REQUIRE(m->max_depth + 2 <= kMaxLevels, "%s: kd-tree depth %d exceeds the walk stack (%d levels)", what, m->max_depth, kMaxLevels - 2);
        for (int i = 0; i < 4; i++) fr.box[i] = m->box[i];
        fr.n_kpts = m->n; fr.n_nodes = m->n_nodes; max_depth = m->max_depth;
    }
    fr.kp_desc = reinterpret_cast<const uint64_t*>(target->desc()); fr.nodes = target->nodes(); fr.leaf_rec = target->leaf();
    for (int i = 0; i < 16; i++) fr.scale[i] = i < tp->n_levels ? tp->scale_factors[i] : 0.f;
    if (n == 0) return UH_OK;
    // ---- the call's blocks
    const ResLayout L = res_layout(n);
    if ((rc = h->d_out.reserve(256 + L.end))) return rc;
    if ((rc = h->h_out.reserve(64 + L.end))) return rc;
    if (skip) {
        if ((rc = h->h_skip.reserve(n))) return rc;
        std::memcpy(h->h_skip.host<uint8_t>(), skip, n);
        std::atomic_thread_fence(std::memory_order_release);
    }
    char* base = h->d_out.as<char>();
    if (!h->zeroed || h->zeroed_gen != h->d_out.gen) {   // ticket and overflow word: zero once per allocation, the kernel's last workgroup clears them after every call
        UH_HIP_CHECK(hipMemsetAsync(base, 0, 256, st));
        h->zeroed = true; h->zeroed_gen = h->d_out.gen;
    }
    FuPoints P;
    P.n = n;
    P.rec = h->h_points.dev<uint4>();
    P.skip = skip ? h->h_skip.dev<unsigned char>() : nullptr;
    P.best_kp = (int*)(base + 256 + L.bk); P.best_dist = (float*)(base + 256 + L.bd); P.status = (unsigned char*)(base + 256 + L.st);
    const unsigned long long word = ++h->seq;
    const FuPublish pub{reinterpret_cast<unsigned*>(base + 128), reinterpret_cast<int*>(base), reinterpret_cast<const unsigned long long*>(base + 256),
                        reinterpret_cast<unsigned long long*>(h->h_out.dev<char>() + 64), (unsigned)(L.end / 8), h->h_out.dev<unsigned long long>(), word};
    // points per workgroup (= waves): spread over the compute units, but not below 4 — every workgroup stages the frame itself
    const int ncu = std::max(h->ctx->num_cus, 64);
    const int gpw = std::min(kWavesMax, std::max(4, uh_div_up(n, ncu)));
    const size_t list_bytes = (size_t)kCandCap * gpw * 8 + 64;
    const size_t tree_bytes = (((size_t)fr.n_nodes * sizeof(Node) + 15) & ~(size_t)15) + 16 * (size_t)fr.n_kpts;
    const bool no_lds = getenv("UH_FUSE_NO_LDS") != nullptr;   // env: test knob for the big-frame path (read per call: tests set it within a process)
    const bool in_lds = tree_bytes + list_bytes <= kLdsBudget && !no_lds;
    const size_t lds = list_bytes + (in_lds ? tree_bytes : 0);
    if (!h->attr_set) {
        UH_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(fuse_search_kernel<true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsBudget));
        UH_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(fuse_search_kernel<false>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsBudget));
        h->attr_set = true;
    }
    const dim3 grid(std::min(uh_div_up(n, gpw), kMaxBlocks));
    const float thr = uh_fusem::desc_threshold(max_desc_dist);
    if (in_lds) UH_LAUNCH(h->ctx, fuse_search_kernel<true>, grid, dim3(gpw * kWave), lds, fr, P, vw, thr, pub);
    else UH_LAUNCH(h->ctx, fuse_search_kernel<false>, grid, dim3(gpw * kWave), lds, fr, P, vw, thr, pub);
    UH_HIP_CHECK(hipGetLastError());
    if ((rc = uh::wait_host_word(reinterpret_cast<volatile unsigned long long*>(h->h_out.host<char>()), word, st, what))) {
        h->zeroed = false;   // a launch that died may have left its ticket / overflow word behind
        return rc;
    }
    const int ovf = *reinterpret_cast<const int*>(h->h_out.host<char>() + 8);
    UH_REQUIRE(!ovf, "%s: kd-tree walk stack overflow", what);
    const char* ho = h->h_out.host<char>() + 64;
    std::memcpy(best_kp_out, ho + L.bk, 4 * (size_t)n);
    std::memcpy(best_dist_out, ho + L.bd, 4 * (size_t)n);
    std::memcpy(status_out, ho + L.st, (size_t)n);
    return UH_OK;
}

int uh_fuse_search_host(const uh_map_points* points, const uh_proj_frame* tp, const float* pose_f2g, const float* predict_scale_factors, int32_t predict_n_levels,
                        const uint8_t* skip, float th, float widen, float max_desc_dist, int32_t* best_kp_out, float* best_dist_out, uint8_t* status_out) {
    const char* what = "uh_fuse_search_host";
    UH_REQUIRE(points, "%s: NULL argument", what);
    UH_REQUIRE(points->n >= 0 && points->n <= kMaxPoints, "%s: %d points outside [0, %d]", what, points->n, kMaxPoints);
    UH_REQUIRE(points->n == 0 || (points->pos3d && points->normal && points->min_dist && points->max_dist && points->desc), "%s: map point arrays missing", what);
    uh_fusem::View vw;
    int rc = fuse_view(what, tp, pose_f2g, predict_scale_factors, predict_n_levels, th, widen, &vw);
    if (rc) return rc;
    if ((rc = check_keypoints(what, tp))) return rc;
    UH_REQUIRE(tp->n_kpts <= uh_kd::kDevMaxPoints, "%s: %d keypoints exceed a device frame's %d", what, tp->n_kpts, uh_kd::kDevMaxPoints);
    UH_REQUIRE(points->n == 0 || (best_kp_out && best_dist_out && status_out), "%s: output arrays missing", what);
    std::vector<uint8_t> nodes; std::vector<uint32_t> leaf; std::vector<float> xy;
    double box[4];
    int nn = 0, md = 0;
    if ((rc = build_host_tree(what, tp, nodes, leaf, xy, box, &nn, &md))) return rc;
    std::vector<int32_t> oct(std::max(tp->n_kpts, 1));
    for (int i = 0; i < tp->n_kpts; i++) oct[i] = tp->und_kpts[i].octave;
    const uh_fusem::HostTree t{reinterpret_cast<const uh_fusem::HostNode*>(nodes.data()), nn, leaf.data(), box, xy.data(), oct.data(), tp->desc, tp->n_kpts};
    const uh_fusem::HostPoints p{points->n, points->pos3d, points->normal, points->min_dist, points->max_dist, points->desc};
    float scale[16];
    for (int i = 0; i < 16; i++) scale[i] = i < tp->n_levels ? tp->scale_factors[i] : 0.f;
    uh_fusem::search_host(vw, scale, t, p, skip, max_desc_dist, best_kp_out, best_dist_out, status_out);
    return UH_OK;
}

}  // extern "C"
