// Stages 3 and 4 of the mapper's per-keyframe step through the C++ adaptors: new map points of one keyframe against its covisible
// neighbours (ucoslam_hip::NewPointCreator, utils/mapmanager.cpp:10087-10696), then the search-and-fuse step over the same window
// (ucoslam_hip::MapPointFuser: MapManager's private SearchInNeighbors member, which precedes local BA).
//
// Scene: 600 points in front of the new keyframe (index 3), seen by three neighbours (0, 1, 2) on a ring around it; descriptors are random
// 256-bit strings, a neighbour's copy has a few bits flipped.  The epipolar matches are the true pairs of neighbours 0 and 1 — neighbour
// 2 was not matched, so the fuse step finds the new points there: free keypoints get an observation, the 150 keypoints of neighbour 2
// that already carry an older map point absorb the new one.  The map is the small stand-in of tests/host_helpers/toy_fuse_map.hpp (the
// reference's member names); with ucoslam::Map the two adaptor calls are the same.  `host` as first argument runs the fuse searches on
// the calling core (no GPU needed for that stage).
//
//   g++ -std=c++17 -O2 -o fuse_points examples/fuse_points.cpp -Lucoslam-cv3_amd -lucoslam_hip -Wl,-rpath,$PWD/ucoslam-cv3_amd -Wl,-rpath,/opt/rocm/lib
#include <cmath>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "../include/ucoslam_hip/adaptors.hpp"
#include "../tests/host_helpers/toy_fuse_map.hpp"

using namespace ucoslam_hip;

static void set_pose(ToyFuseFrame& f, double yaw, double cx, double cy, double cz) {
    const double c = std::cos(yaw), s = std::sin(yaw), R[9] = {c, 0, s, 0, 1, 0, -s, 0, c};
    for (int k = 0; k < 16; k++) f.pose_f2g[k] = k == 15 ? 1.f : 0.f;
    for (int r = 0; r < 3; r++) {
        for (int k = 0; k < 3; k++) f.pose_f2g[4 * r + k] = (float)R[3 * r + k];
        f.pose_f2g[4 * r + 3] = (float)-(R[3 * r] * cx + R[3 * r + 1] * cy + R[3 * r + 2] * cz);
    }
}

int main(int argc, char** argv) {
    const bool host_fuse = argc > 1 && !strcmp(argv[1], "host");
    const int n_pts = 600, n_levels = 8;
    const uint32_t cur = 3;
    std::mt19937 rng(7);
    std::uniform_real_distribution<double> U(0, 1);
    std::normal_distribution<double> N(0, 0.3);
    ToyFuseMap map;
    for (uint32_t i = 0; i <= cur; i++) {
        ToyFuseFrame f;
        f.idx = i;
        f.imageParams = ToyImageParams{517.3f, 516.5f, 318.6f, 255.3f};
        f.maxXY = {640, 480};
        for (int l = 0; l < n_levels; l++) f.scaleFactors.push_back(l ? f.scaleFactors[l - 1] * 1.2f : 1.f);
        if (i == cur) set_pose(f, 0.0, 0, 0, 0);
        else set_pose(f, 0.03 * ((int)i - 1), 0.5 * std::cos(2.1 * i), 0.3 * std::sin(2.1 * i), 0.1 * i);
        map.keyframes.emplace(i, f);
        if (i != cur) map.TheKpGraph.nb[cur].push_back(i);
    }
    for (int i = 0; i < n_pts; i++) {   // keypoint i of every frame is world point i
        const double X[3] = {-1.5 + 3 * U(rng), -1.1 + 2.2 * U(rng), 4 + 4 * U(rng)};
        uint8_t d[32];
        for (auto& b : d) b = (uint8_t)rng();
        const int oct = 1 + (int)(rng() % 3);
        for (auto& kv : map.keyframes) {
            ToyFuseFrame& f = kv.second;
            double c[3];
            for (int r = 0; r < 3; r++) c[r] = f.pose_f2g[4 * r] * X[0] + f.pose_f2g[4 * r + 1] * X[1] + f.pose_f2g[4 * r + 2] * X[2] + f.pose_f2g[4 * r + 3];
            f.und_kpts.push_back(ToyKeyPoint{{(float)(f.imageParams.fx() * c[0] / c[2] + f.imageParams.cx() + N(rng)), (float)(f.imageParams.fy() * c[1] / c[2] + f.imageParams.cy() + N(rng))}, oct});
            f.desc.insert(f.desc.end(), d, d + 32);
            for (int k = 0; k < (kv.first == cur ? 0 : 5); k++) f.desc[f.desc.size() - 32 + rng() % 32] ^= (uint8_t)(1u << (rng() % 8));
            f.ids.push_back(kToyNoId);
        }
    }
    uint32_t next_id = 0;
    auto new_point = [&](const float xyz[3]) {
        ToyFuseMapPoint mp;
        mp.id = next_id++;
        mp.pos3d = {xyz[0], xyz[1], xyz[2]};
        map.map_points.emplace(mp.id, mp);
        return mp.id;
    };
    for (int i = 0; i < 150; i++) {   // older map points of neighbour 2, at the positions its keypoints see
        const ToyFuseFrame& f = map.keyframes[2];
        const float z = 6.f, xc[3] = {(f.und_kpts[i].pt.x - f.imageParams.cx()) / f.imageParams.fx() * z, (f.und_kpts[i].pt.y - f.imageParams.cy()) / f.imageParams.fy() * z, z};
        float inv[16], g[3];
        se3_inverse(f.pose_f2g.data(), inv);
        for (int r = 0; r < 3; r++) g[r] = inv[4 * r] * xc[0] + inv[4 * r + 1] * xc[1] + inv[4 * r + 2] * xc[2] + inv[4 * r + 3];
        map.addMapPointObservation(new_point(g), 2, (uint32_t)i);
    }

    Context ctx(0);
    // ---- new map points: the true pairs of neighbours 0 and 1 stand for matchEpipolar's result
    NewPointCreator creator(ctx);
    std::vector<const ToyFuseFrame*> nbs = {&map.keyframes[0], &map.keyframes[1]};
    std::vector<std::vector<uh_dmatch>> matches(2);
    for (auto& m : matches)
        for (int i = 0; i < n_pts; i++) m.push_back(uh_dmatch{i, i, -1, 10.f});
    const std::vector<NewPointInfo> created = creator.create(map.keyframes[cur], nbs, matches, 1.2f);
    for (const NewPointInfo& p : created) {
        const uint32_t id = new_point(p.xyz);
        for (const auto& fk : p.frame_kpt) map.addMapPointObservation(id, fk.first, fk.second);
    }
    // ---- search and fuse
    MapPointFuser fuser(ctx);
    if (host_fuse) fuser.setHostForm(true);
    size_t obs0 = 0;
    for (const auto& kv : map.map_points) obs0 += kv.second.frames.size();
    const std::vector<uint32_t> removed = fuser.searchInNeighbors(map, map.keyframes[cur], 100.f);
    size_t obs1 = 0, bad = 0;
    for (const auto& kv : map.map_points) { obs1 += kv.second.frames.size(); bad += kv.second.isBad(); }
    std::printf("{\"new_points\": %zu, \"fused_away\": %zu, \"bad_points\": %zu, \"observations_before\": %zu, \"observations_after\": %zu, \"device_frames\": %zu}\n", created.size(),
                removed.size(), bad, obs0, obs1, fuser.cachedFrames());
    return (!created.empty() && !removed.empty() && obs1 > obs0) ? 0 : 1;
}
