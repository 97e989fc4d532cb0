// Host form of the fuse search (uh_fuse_search_host; tests/host_helpers/fuse_host.cpp builds it alone): fuse_math.hpp per point, picoflann's
// radius walk (src/basictypes/picoflann.h:545-590, 411-437) over the flattened tree uh_kdtree_build_host returns, the octave filter
// [level - 1, level], and the first-strict-minimum Hamming rule in the walk's order.  Plain C++, no GPU, no OpenCV; the device kernel
// (fuse.hip) gives the same three outputs bit for bit.
#pragma once
#include <cstring>
#include <vector>

#include "fuse_math.hpp"

namespace uh_fusem {

struct HostNode { float divlow, divhigh; int left, right; int leaf_begin; short leaf_count, col; };   // = the 24-byte nodes of uh_kdtree_build_host
static_assert(sizeof(HostNode) == 24, "node layout");

struct HostTree {
    const HostNode* nodes; int n_nodes;
    const uint32_t* leaf_idx;       // n
    const double* box;              // x.min x.max y.min y.max
    const float* xy;                // n x 2 (keypoint order)
    const int32_t* octave;          // n
    const uint8_t* desc;            // n x 32
    int n;
};

struct HostPoints { int n; const float* pos3d; const float* normal; const float* min_dist; const float* max_dist; const uint8_t* desc; };

inline int hamming256(const uint8_t* a, const uint8_t* b) {
    uint64_t x[4], y[4];
    std::memcpy(x, a, 32); std::memcpy(y, b, 32);
    return __builtin_popcountll(x[0] ^ y[0]) + __builtin_popcountll(x[1] ^ y[1]) + __builtin_popcountll(x[2] ^ y[2]) + __builtin_popcountll(x[3] ^ y[3]);
}

// searchExactLevel with a radius result set (worst = r^2 throughout): the hits in visiting order
inline void walk(const HostTree& t, int node, float qx, float qy, double worst, double mindistsq, double dists[2], std::vector<uint32_t>& out) {
    const HostNode& nd = t.nodes[node];
    if (nd.left < 0) {
        for (int i = 0; i < nd.leaf_count; i++) {
            const uint32_t id = t.leaf_idx[nd.leaf_begin + i];
            const double dx = qx - t.xy[2 * (size_t)id];          // float difference, double square
            double sqd = dx * dx;
            if (!(sqd > worst)) { const double dy = qy - t.xy[2 * (size_t)id + 1]; sqd += dy * dy; }
            if (sqd < worst) out.push_back(id);
        }
        return;
    }
    const double val = nd.col == 0 ? qx : qy;
    const double diff1 = val - nd.divlow, diff2 = val - nd.divhigh;
    const bool go_left = diff1 + diff2 < 0;
    const double cut = go_left ? diff2 * diff2 : diff1 * diff1;
    walk(t, go_left ? nd.left : nd.right, qx, qy, worst, mindistsq, dists, out);
    const float dst = (float)dists[nd.col];
    mindistsq = mindistsq + cut - dst;
    dists[nd.col] = cut;
    if (mindistsq * 1.0 <= worst) walk(t, go_left ? nd.right : nd.left, qx, qy, worst, mindistsq, dists, out);
    dists[nd.col] = dst;
}

inline void radius_search(const HostTree& t, float qx, float qy, double radius, std::vector<uint32_t>& out) {
    out.clear();
    if (t.n == 0) return;
    const double worst = radius * radius;
    if (!(worst > 0)) return;
    double dists[2] = {0, 0};
    float distsq = 0.f;       // computeInitialDistances: float accumulator
    const float q[2] = {qx, qy};
    for (int i = 0; i < 2; i++) {
        const double e = q[i];
        if (e < t.box[2 * i]) { const double d = e - t.box[2 * i]; dists[i] = d * d; distsq += dists[i]; }
        if (e > t.box[2 * i + 1]) { const double d = e - t.box[2 * i + 1]; dists[i] = d * d; distsq += dists[i]; }
    }
    walk(t, 0, qx, qy, worst, distsq, dists, out);
}

// One search: every point of `p` against the frame behind `t`.  scale: the searched frame's scaleFactors.
inline void search_host(const View& v, const float* scale, const HostTree& t, const HostPoints& p, const uint8_t* skip, float max_desc_dist, int32_t* best_kp_out,
                        float* best_dist_out, uint8_t* status_out) {
    const float thr = desc_threshold(max_desc_dist);
    std::vector<uint32_t> hits;
    for (int m = 0; m < p.n; m++) {
        Disc d;
        const float* P = p.pos3d + 3 * (size_t)m;
        const float* N = p.normal + 3 * (size_t)m;
        uint8_t st = point_disc(v, scale, skip && skip[m], P[0], P[1], P[2], N[0], N[1], N[2], p.min_dist[m], p.max_dist[m], d);
        int best = -1;
        float best_d = thr;
        if (st == kFound) {
            radius_search(t, d.px, d.py, (double)d.radius, hits);
            for (uint32_t id : hits) {
                const int oc = t.octave[id];
                if (!(oc >= d.level - 1 && oc <= d.level)) continue;
                const float hd = (float)hamming256(p.desc + 32 * (size_t)m, t.desc + 32 * (size_t)id);
                if (hd < best_d) { best_d = hd; best = (int)id; }
            }
            if (best < 0) st = kNoKeypoint;
        }
        best_kp_out[m] = best;
        best_dist_out[m] = best_d;
        status_out[m] = st;
    }
}

}  // namespace uh_fusem
