// Stage 3 of the mapper's per-keyframe step over the C ABI: new map points of one keyframe against three covisible neighbours
// (reference: utils/mapmanager.cpp:9914-10696, statement starts of the token-pasted source).
//
//   FrameMatcher::matchEpipolar   index over the new keyframe's descriptors, the neighbour's as queries,   uh_knn_build / uh_knn_search
//                                 the filter chain with the epipolar gate of getFund12                     uh_fundamental_12 + uh_match_filter
//   Triangulate + ratio checks    every pair of the keyframe in ONE call: per-match triangulation,          uh_newpoints_run
//   + merge per keypoint          distance-ratio / octave-ratio check, merge into NewPointInfo lists
//
// Scene: 600 points in front of the new keyframe, seen by three neighbours on a ring around it; descriptors are random 256-bit strings
// (a neighbour's copy has a few bits flipped), projections carry half a pixel of noise.  Prints the match and point counts.
//
//   g++ -std=c++17 -O2 -o new_points examples/new_points.cpp -Lucoslam-cv3_amd -lucoslam_hip -Wl,-rpath,$PWD/ucoslam-cv3_amd -Wl,-rpath,/opt/rocm/lib
#include <climits>
#include <cmath>
#include <cstdio>
#include <random>
#include <vector>

#include "../include/ucoslam_hip/adaptors.hpp"

using namespace ucoslam_hip;

struct Frame {
    float pose[16];   // pose_f2g
    float intr4[4] = {517.3f, 516.5f, 318.6f, 255.3f};
    std::vector<float> pt, angle;
    std::vector<int32_t> octave;
    std::vector<uint8_t> desc;
};

static void set_pose(Frame& f, double yaw, double cx, double cy, double cz) {
    const double c = std::cos(yaw), s = std::sin(yaw), R[9] = {c, 0, s, 0, 1, 0, -s, 0, c};
    for (int k = 0; k < 16; k++) f.pose[k] = k == 15 ? 1.f : 0.f;
    for (int r = 0; r < 3; r++) {
        for (int k = 0; k < 3; k++) f.pose[4 * r + k] = (float)R[3 * r + k];
        f.pose[4 * r + 3] = (float)-(R[3 * r] * cx + R[3 * r + 1] * cy + R[3 * r + 2] * cz);
    }
}

int main() {
    const int n_pts = 600, n_nb = 3, n_levels = 8, nn = 10;
    std::vector<float> sf(n_levels);
    for (int l = 0; l < n_levels; l++) sf[l] = l ? sf[l - 1] * 1.2f : 1.f;
    std::mt19937 rng(7);
    std::uniform_real_distribution<double> U(0, 1);
    std::normal_distribution<double> N(0, 0.5);
    Frame kf;
    std::vector<Frame> nb(n_nb);
    set_pose(kf, 0.0, 0, 0, 0);
    for (int j = 0; j < n_nb; j++) set_pose(nb[j], 0.03 * (j - 1), std::cos(2.1 * j), 0.6 * std::sin(2.1 * j), 0.1 * j);
    auto add = [&](Frame& f, const double X[3], int oct, const uint8_t* d, int flips) {
        double c[3];
        for (int r = 0; r < 3; r++) c[r] = f.pose[4 * r] * X[0] + f.pose[4 * r + 1] * X[1] + f.pose[4 * r + 2] * X[2] + f.pose[4 * r + 3];
        f.pt.push_back((float)(f.intr4[0] * c[0] / c[2] + f.intr4[2] + N(rng)));
        f.pt.push_back((float)(f.intr4[1] * c[1] / c[2] + f.intr4[3] + N(rng)));
        f.octave.push_back(oct);
        f.angle.push_back(40.f);
        f.desc.insert(f.desc.end(), d, d + 32);
        for (int k = 0; k < flips; k++) f.desc[f.desc.size() - 32 + rng() % 32] ^= (uint8_t)(1u << (rng() % 8));
    };
    for (int i = 0; i < n_pts; i++) {
        const double X[3] = {-2 + 4 * U(rng), -1.5 + 3 * U(rng), 4 + 5 * U(rng)};
        uint8_t d[32];
        for (auto& b : d) b = (uint8_t)rng();
        const int oct = (int)(rng() % 4);
        add(kf, X, oct, d, 0);
        for (int j = 0; j < n_nb; j++) add(nb[j], X, oct + (int)(rng() % 2), d, 6);
    }

    Context ctx(0);
    uh_knn* knn = nullptr;
    check(uh_knn_create(ctx.get(), &knn));
    check(uh_knn_build(knn, kf.desc.data(), n_pts, 32, 32));   // FrameMatcher::setParams(newKF, ...): the train index
    float inv[16], center_kf[3];
    se3_inverse(kf.pose, inv);
    camera_center(kf.pose, center_kf);
    std::vector<std::vector<uh_dmatch>> matches(n_nb);
    std::vector<uh_newpoints_pair> pairs(n_nb);
    for (int j = 0; j < n_nb; j++) {
        uh_newpoints_pair& p = pairs[j];
        mat44_product(nb[j].pose, inv, p.RT);                   // mapmanager.cpp:10045-10062
        float F12[9];
        check(uh_fundamental_12(kf.intr4, nb[j].intr4, p.RT, F12));   // framematcher.cpp:234
        std::vector<int32_t> idx((size_t)n_pts * nn), dist((size_t)n_pts * nn);
        check(uh_knn_search(knn, nb[j].desc.data(), n_pts, 32, nn, idx.data(), dist.data(), 0, -1));
        uh_match_filter_args fa{};
        fa.nq = n_pts; fa.nn = nn; fa.indices = idx.data(); fa.distances = dist.data();
        fa.q_octave = nb[j].octave.data(); fa.q_angle = nb[j].angle.data(); fa.q_pt = nb[j].pt.data();
        fa.t_octave = kf.octave.data(); fa.t_angle = kf.angle.data(); fa.t_pt = kf.pt.data();
        fa.scale_factors = sf.data(); fa.F12 = F12;
        fa.min_desc_dist = 100.f; fa.nn_match_ratio = 0.6f; fa.check_orientation = 1; fa.max_octave_diff = INT_MAX;   // mapmanager.cpp:9953-9989
        fa.n_query_kpts = n_pts; fa.n_train_kpts = n_pts; fa.n_levels = n_levels;
        matches[j].resize(n_pts);
        const int nm = uh_match_filter(&fa, matches[j].data(), n_pts);
        check(nm);
        matches[j].resize(nm);
        for (int k = 0; k < 4; k++) p.intr4[k] = nb[j].intr4[k];
        camera_center(nb[j].pose, p.cam_center);
        p.n_levels = n_levels; p.scale_factors = sf.data();
        p.n_kpts = n_pts; p.pt = nb[j].pt.data(); p.octave = nb[j].octave.data();
        p.n_matches = nm; p.matches = matches[j].data();
    }
    uh_newpoints_args a{};
    for (int k = 0; k < 4; k++) a.intr4[k] = kf.intr4[k];
    for (int k = 0; k < 16; k++) a.pose_g2f[k] = inv[k];
    for (int k = 0; k < 3; k++) a.cam_center[k] = center_kf[k];
    a.n_levels = n_levels; a.scale_factors = sf.data();
    a.n_kpts = n_pts; a.pt = kf.pt.data(); a.octave = kf.octave.data();
    a.n_pairs = n_nb; a.pairs = pairs.data();
    a.max_chi2 = 5.998f; a.ratio_factor = 1.5f * 1.2f; a.merge_rule = UH_NEWPOINTS_MERGE_SMALLEST_OCTAVE;
    uh_newpoints* np = nullptr;
    check(uh_newpoints_create(ctx.get(), &np));
    uh_newpoints_result r{};
    check(uh_newpoints_run(np, &a, &r));
    int hist[10] = {0}, right = 0;
    for (int i = 0; i < r.n_total; i++) hist[r.status[i]]++;
    for (int j = 0, g = 0; j < n_nb; j++)
        for (const uh_dmatch& m : matches[j]) { if (m.queryIdx == m.trainIdx && r.status[g] == 0) right++; g++; }
    std::printf("{\"matches\": [%zu, %zu, %zu], \"accepted\": %d, \"accepted_true_pairs\": %d, \"new_points\": %d, \"observations\": %d}\n", matches[0].size(),
                matches[1].size(), matches[2].size(), hist[0], right, r.n_new, r.n_obs);
    uh_newpoints_destroy(np);
    uh_knn_destroy(knn);
    return r.n_new > 0 ? 0 : 1;
}
