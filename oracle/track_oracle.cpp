// TEST INFRASTRUCTURE ONLY — CPU oracle for the tracker's pose estimation of one frame (what uh_track_pose / uh_track_pose_stereo fuse).
// Only tests/ and scripts/fuzz_parity.py may use this file.
//
// Restates, statement by statement, the control flow of  src/utils/system.cpp:6559-6954  (the file is token-pasted; line numbers are the
// statement starts in the raw file, read after preprocessing), with the map modelled the way the reference holds it: ONE table keyed by
// map-point id (position, normal, min / max distance, descriptor, stability, lastFIdxSeen).  The previous frame's items name ids in that
// table, the local map is a list of ids, and every look-up goes by id (TheMap->map_points[trainIdx]).  Nothing here knows the product's
// candidate rows (prev_map_row) or its device lists.
// The steps themselves are the oracles that are pinned elsewhere, called through their C entry points:
//   oracle_proj_match_prev          the search against the previous frame   (proj_oracle.cpp; picoflann pinned)
//   oracle_proj_match               Map::matchFrameToMapPoints               (proj_oracle.cpp)
//   oracle_filter_ambiguous_query   misc.cpp:117-150                         (proj_oracle.cpp)
//   oracle_pnp_solve_stereo         PnPSolver::solvePnp                      (pnp_oracle.cpp; real g2o pinned)
// The FrameMatcher fallback (:6664-6780) is not modelled: with too few matches it is taken to find nothing.
#include <cstdint>
#include <cstring>
#include <unordered_map>
#include <unordered_set>
#include <vector>

// The entries below live in the other files of liboracle.so.  The two that were added to those files together with this one are referenced
// weakly: the library (every oracle/*.cpp, linked without --no-undefined) must still load when it is built next to older copies of its
// sibling files, for the tests that do not use this oracle; oracle_track_pose then refuses to run (-2).
extern "C" {
struct oracle_keypoint { float x, y, size, angle, response; int32_t octave, class_id; };   // cv::KeyPoint (as proj_oracle.cpp)
int oracle_proj_match(const oracle_keypoint* und_kpts, int n_kpts, const uint8_t* desc, const float* scale_factors, int n_levels,
                      float fx, float fy, float cx, float cy, int min_x, int min_y, int max_x, int max_y, const float* pose_f2g,
                      int n_pts, const uint32_t* ids, const float* pos3d, const float* normal, const float* min_dist,
                      const float* max_dist, const uint8_t* mp_desc, float minDescDist, float maxRepjDist, int32_t* best_kp_out,
                      float* best_dist_out, uint8_t* visible_out, int32_t* matches_out);
int oracle_proj_match_prev(const oracle_keypoint* und_kpts, int n_kpts, const uint8_t* desc, const float* scale_factors, int n_levels,
                           float fx, float fy, float cx, float cy, int min_x, int min_y, int max_x, int max_y, const float* pose_f2g,
                           int n_pts, const uint32_t* ids, const float* pos3d, const int32_t* octave, const uint8_t* prev_desc,
                           float minDescDist, float maxRepjDist, int32_t* best_kp_out, float* best_dist_out, int32_t* matches_out);
__attribute__((weak)) int oracle_filter_ambiguous_query(int32_t* matches, int n);
__attribute__((weak)) int oracle_pnp_solve_stereo(const float* pose_f2g, const float* intr4, int n, const float* p3d, const float* kp, const float* invsigma,
                            const float* weight, const float* depth, float bl, float* pose_out, uint8_t* bad_out, int32_t* iters_out,
                            double* state_out);
}

namespace {

struct DMatch { int32_t queryIdx, trainIdx, imgIdx; float distance; };

struct MapPoint {                 // map_types/mappoint.h: what the tracker reads of one point
    const float* pos; const float* normal; float min_dist, max_dist; const uint8_t* desc;
    bool stable;                  // isStable()
    int64_t lastFIdxSeen = -1;
};

struct Frame {                    // map_types/frame.h: what the tracker reads of the current frame
    const oracle_keypoint* und_kpts; int n_kpts; const uint8_t* desc; const float* scaleFactors; int n_levels;
    float fx, fy, cx, cy; int min_x, min_y, max_x, max_y;
    const float* depth; float bl;
    int64_t fseq_idx = 0;
    float getDepth(int q) const { return depth ? depth[q] : 0.f; }
};

struct Solve { int nInliers = 0; float pose[16]; std::vector<uint8_t> bad; int32_t iters[4] = {0, 0, 0, 0}; };

// PnPSolver::solvePnp(frame, TheMap, matches, pose): the per-match look-ups of pnpsolver.cpp:192-232 by id, then the solve.
// pnpsolver.cpp:149-150: without matches it returns 0 and leaves the pose as it came in.
bool solve_pnp(const Frame& fr, const std::unordered_map<uint32_t, MapPoint>& map_points, const std::vector<DMatch>& matches, const float* pose_in,
               Solve& s) {
    const int n = (int)matches.size();
    std::memcpy(s.pose, pose_in, 64);
    s.bad.assign(n, 0);
    s.nInliers = 0;
    for (int i = 0; i < 4; i++) s.iters[i] = 0;
    if (n == 0) return true;
    std::vector<float> p3d(3 * (size_t)n), kp(2 * (size_t)n), invs(n), w(n), dep(n);
    for (int i = 0; i < n; i++) {
        const oracle_keypoint& kpt = fr.und_kpts[matches[i].queryIdx];
        auto it = map_points.find((uint32_t)matches[i].trainIdx);   // TheMap->map_points[trainIdx]
        if (it == map_points.end()) return false;
        const MapPoint& mp = it->second;
        for (int r = 0; r < 3; r++) p3d[3 * i + r] = mp.pos[r];
        w[i] = mp.stable ? 1.f : 0.5f;                              // :210-211: edge_weight 0.5 when !mp.isStable()
        kp[2 * i] = kpt.x; kp[2 * i + 1] = kpt.y;
        invs[i] = (float)(1. / fr.scaleFactors[kpt.octave]);         // :192-193 invScaleFactor, :229 invSigma2
        dep[i] = fr.getDepth(matches[i].queryIdx);                  // :214 depth <= 0: monocular edge
    }
    const float intr[4] = {fr.fx, fr.fy, fr.cx, fr.cy};
    double state[7];
    s.nInliers = oracle_pnp_solve_stereo(pose_in, intr, n, p3d.data(), kp.data(), invs.data(), w.data(), fr.depth ? dep.data() : nullptr, fr.bl,
                                         s.pose, s.bad.data(), s.iters, state);
    return true;
}

}  // namespace

extern "C" {

// One frame of the tracker.  Frame: und_kpts / desc / scaleFactors, intr4 = fx fy cx cy, minmax_xy = min_x min_y max_x max_y, depth
// (n_kpts floats or NULL) and bl.  The map table: n_tab points keyed by tab_ids (tab_stable: 1 = isStable()).  The previous frame: n_prev
// items (map-point id, keypoint octave, keypoint descriptor).  The local map: n_local ids.  params = {previous-frame min descriptor
// distance, its search radius, map min descriptor distance, map radius when tracked, when lost}; min_inliers = the reference's 30.
// pose_for_map != NULL: the map search and the second solve start from that pose instead of the first solve's (when tracked).
// counts: [0] matches_prev [1] matches_map [2] matches_all [3] tracked [4] inliers1 [5..8] iters1 [9] inliers2 [10..13] iters2.
// Match lists are cv::DMatch (4 words); capacities n_prev / n_local / n_prev + n_local.  Returns 0, -1 for an id not in the table, -2
// when the library lacks the steps it calls (see above).
int oracle_track_pose(const oracle_keypoint* und_kpts, int n_kpts, const uint8_t* desc, const float* scale_factors, int n_levels, const float* intr4,
                      const int32_t* minmax_xy, const float* depth, float bl,
                      int n_tab, const uint32_t* tab_ids, const float* tab_pos3d, const float* tab_normal, const float* tab_min_dist,
                      const float* tab_max_dist, const uint8_t* tab_desc, const uint8_t* tab_stable,
                      int n_prev, const uint32_t* prev_ids, const int32_t* prev_octave, const uint8_t* prev_desc,
                      int n_local, const uint32_t* local_ids,
                      const float* pose0, const float* pose_for_map, const float* params, int min_inliers,
                      int32_t* counts, float* pose1_out, float* pose2_out, int32_t* m_prev_out, uint8_t* bad_prev_out, int32_t* m_map_out,
                      int32_t* m_all_out, uint8_t* bad_all_out) {
    if (!oracle_filter_ambiguous_query || !oracle_pnp_solve_stereo) return -2;
    Frame fr{und_kpts, n_kpts, desc, scale_factors, n_levels, intr4[0], intr4[1], intr4[2], intr4[3], minmax_xy[0], minmax_xy[1], minmax_xy[2],
             minmax_xy[3], depth, bl};
    fr.fseq_idx = 1;
    std::unordered_map<uint32_t, MapPoint> map_points;   // TheMap->map_points
    for (int i = 0; i < n_tab; i++)
        map_points[tab_ids[i]] = MapPoint{tab_pos3d + 3 * (size_t)i, tab_normal + 3 * (size_t)i, tab_min_dist[i], tab_max_dist[i], tab_desc + 32 * (size_t)i,
                                          tab_stable[i] != 0};
    const float prev_min_desc = params[0], prev_repj = params[1], map_min_desc = params[2], r_tracked = params[3], r_lost = params[4];
    float pose[16];                                       // the tracker's current pose estimate (_5769551021164122736)
    std::memcpy(pose, pose0, 64);

    // :6559-6565  matches = the search against the previous frame (its items' coordinates are their map points')
    std::vector<float> prev_pos(3 * (size_t)n_prev);
    for (int i = 0; i < n_prev; i++) {
        auto it = map_points.find(prev_ids[i]);
        if (it == map_points.end()) return -1;
        for (int r = 0; r < 3; r++) prev_pos[3 * i + r] = it->second.pos[r];
    }
    std::vector<int32_t> bk(n_prev + 1), mbuf(4 * ((size_t)n_prev + (size_t)n_local + 1));
    std::vector<float> bd(n_prev + 1);
    const int n1 = oracle_proj_match_prev(und_kpts, n_kpts, desc, scale_factors, n_levels, fr.fx, fr.fy, fr.cx, fr.cy, fr.min_x, fr.min_y, fr.max_x, fr.max_y,
                                          pose, n_prev, prev_ids, prev_pos.data(), prev_octave, prev_desc, prev_min_desc, prev_repj, bk.data(), bd.data(), mbuf.data());
    if (n1 < 0) return -1;
    std::vector<DMatch> matches(n1);
    std::memcpy(matches.data(), mbuf.data(), 16 * (size_t)n1);
    std::memcpy(m_prev_out, matches.data(), 16 * (size_t)n1);

    Solve s1;
    std::memcpy(s1.pose, pose, 64);
    s1.bad.assign(n1, 0);
    int nInliers = 0;                                     // :6590  int nInliers = 0
    if ((int)matches.size() > min_inliers) {              // :6595  matches.size() > 30
        float pose_copy[16];                              //        auto pose_copy = current pose
        std::memcpy(pose_copy, pose, 64);
        if (!solve_pnp(fr, map_points, matches, pose_copy, s1)) return -1;   // :6626  nInliers = PnPSolver::solvePnp(...)
        nInliers = s1.nInliers;
        if (nInliers > min_inliers) std::memcpy(pose, s1.pose, 64);         // :6646  nInliers > 30: keep the refined pose
    } else {
        // :6664-6780  FrameMatcher against the reference keyframe: not modelled, taken to find nothing -> :6780's else: nInliers = 0
        nInliers = 0;
    }
    const bool tracked = nInliers > min_inliers;          // :6813  nInliers > 30
    float radius;
    std::unordered_set<uint32_t> seen;
    if (tracked) {
        radius = r_tracked;                               // :6813-6820  4 px
        for (const DMatch& m : matches) {                 // :6842  EVERY match (inliers and outliers): lastFIdxSeen = fseq_idx
            map_points[(uint32_t)m.trainIdx].lastFIdxSeen = fr.fseq_idx;
            seen.insert((uint32_t)m.trainIdx);
        }
        if (pose_for_map) std::memcpy(pose, pose_for_map, 64);
    } else {
        matches.clear();                                  // :6877  matches.clear(); radius = projDistThr
        radius = r_lost;
    }

    // :6897  Map::matchFrameToMapPoints(local map, frame, pose, maxDescDistance*2, radius, true) — useAllPoints = false: map.cpp:657-668
    // drops every point whose lastFIdxSeen is this frame before the search
    std::vector<uint32_t> cid;
    std::vector<float> cpos, cnrm, cmin, cmax;
    std::vector<uint8_t> cdesc;
    for (int i = 0; i < n_local; i++) {
        auto it = map_points.find(local_ids[i]);
        if (it == map_points.end()) return -1;
        const MapPoint& mp = it->second;
        if (mp.lastFIdxSeen == fr.fseq_idx) continue;
        cid.push_back(local_ids[i]);
        for (int r = 0; r < 3; r++) { cpos.push_back(mp.pos[r]); cnrm.push_back(mp.normal[r]); }
        cmin.push_back(mp.min_dist); cmax.push_back(mp.max_dist);
        cdesc.insert(cdesc.end(), mp.desc, mp.desc + 32);
    }
    const int nc = (int)cid.size();
    std::vector<int32_t> bk2(nc + 1);
    std::vector<float> bd2(nc + 1);
    std::vector<uint8_t> vis(nc + 1);
    const int n2 = nc ? oracle_proj_match(und_kpts, n_kpts, desc, scale_factors, n_levels, fr.fx, fr.fy, fr.cx, fr.cy, fr.min_x, fr.min_y, fr.max_x, fr.max_y, pose, nc,
                                          cid.data(), cpos.data(), cnrm.data(), cmin.data(), cmax.data(), cdesc.data(), map_min_desc, radius, bk2.data(), bd2.data(),
                                          vis.data(), mbuf.data())
                      : 0;                                // (map.cpp:670: no points, no matches)
    std::memcpy(m_map_out, mbuf.data(), 16 * (size_t)n2);
    // :6913  matches.insert(end, map matches);  :6931  filter_ambiguous_query(matches)
    std::vector<DMatch> uni(matches);
    uni.resize(matches.size() + n2);
    std::memcpy(uni.data() + matches.size(), mbuf.data(), 16 * (size_t)n2);
    const int na = uni.empty() ? 0 : oracle_filter_ambiguous_query(reinterpret_cast<int32_t*>(uni.data()), (int)uni.size());
    uni.resize(na);
    // :6954  PnPSolver::solvePnp over the union from the current pose
    Solve s2;
    if (!solve_pnp(fr, map_points, uni, pose, s2)) return -1;

    std::memcpy(m_all_out, uni.data(), 16 * (size_t)na);
    for (int i = 0; i < n1; i++) bad_prev_out[i] = s1.bad[i];
    for (int i = 0; i < na; i++) bad_all_out[i] = s2.bad[i];
    std::memcpy(pose1_out, s1.pose, 64);
    std::memcpy(pose2_out, s2.pose, 64);
    counts[0] = n1; counts[1] = n2; counts[2] = na; counts[3] = tracked ? 1 : 0;
    counts[4] = s1.nInliers;
    for (int i = 0; i < 4; i++) counts[5 + i] = s1.iters[i];
    counts[9] = s2.nInliers;
    for (int i = 0; i < 4; i++) counts[10 + i] = s2.iters[i];
    return 0;
}

}  // extern "C"
