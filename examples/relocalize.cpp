// System::relocalize's pose search over the C ABI (reference: utils/system.cpp, the statements around raw lines 4950-5500) for the candidate
// keyframes of one lost frame:
//
//   PnPSolver::solvePnPRansac      every candidate with >= 25 matches in ONE call, samples drawn as the    uh_pnp_ransac_samples + uh_pnp_ransac
//                                  reference's std::random_shuffle draws them
//   Map::matchFrameToMapPoints     per survivor (>= 15 matches): its neighbourhood's points from the       uh_projmatch_set_frame (once) + uh_projmatch_match
//                                  RANSAC pose, maxDescDistance * 2, radius 2.5
//   PnPSolver::solvePnp            per survivor (>= 30 matches), inv_sigma by octave, weight 1 / 0.5       uh_pnp_solve
//   the candidate with the most good matches (>= 30) wins, the first on ties
//
// The candidate selection (uh_bowdb_query) and the descriptor matching (uh_knn_* + uh_match_filter / uh_bowmatch_match) are the callers' and
// are played here by a synthetic match list: 1500 keypoints, 1200 map points behind them seen from a planted pose (0.5 px noise), three
// candidates — one whose matches are 70 % right, one with 20 matches, one whose matches are all wrong.
//
//   g++ -std=c++17 -O2 -o relocalize examples/relocalize.cpp -Lucoslam-cv3_amd -lucoslam_hip -Wl,-rpath,$PWD/ucoslam-cv3_amd -Wl,-rpath,/opt/rocm/lib
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "../include/ucoslam_hip.h"

#define CHECK(expr)                                                                              \
    do {                                                                                         \
        const int rc_ = (expr);                                                                  \
        if (rc_ < 0) { std::printf("%s failed: %s\n", #expr, uh_last_error()); return 1; }      \
    } while (0)

struct Candidate {
    std::vector<uh_dmatch> matches;   // queryIdx = the frame's keypoint, trainIdx = the map point's id
    float rt6[6];                     // the keyframe's pose as (rvec, tvec)
};

int main() {
    uh_ctx* ctx = nullptr;
    if (uh_ctx_create(0, nullptr, &ctx) < 0) { std::printf("no device: %s (there is no CPU path)\n", uh_last_error()); return 0; }
    const float intr4[4] = {718.856f, 718.856f, 607.19f, 185.22f};
    const int W = 1241, H = 376, n_kp = 1500, n_pt = 1200, n_levels = 8, max_iters = 50;
    const float max_desc_dist = 50.f;
    std::mt19937 rng(7);
    std::uniform_real_distribution<double> U(0, 1);
    std::normal_distribution<double> G(0, 1);
    std::vector<float> sf(n_levels, 1.f), inv_sf(n_levels, 1.f);
    for (int l = 1; l < n_levels; l++) sf[l] = sf[l - 1] * 1.2f;
    for (int l = 0; l < n_levels; l++) inv_sf[l] = 1.f / sf[l];
    // ---- the lost frame
    std::vector<uh_keypoint> kps(n_kp);
    std::vector<uint8_t> desc(32 * (size_t)n_kp);
    for (int i = 0; i < n_kp; i++) {
        kps[i] = uh_keypoint{(float)(20 + U(rng) * (W - 40)), (float)(20 + U(rng) * (H - 40)), 31.f, 0.f, 50.f, (int32_t)(U(rng) * 4), -1};
        for (int b = 0; b < 32; b++) desc[32 * (size_t)i + b] = (uint8_t)(rng() & 255);
    }
    // ---- the map: point p lies behind keypoint p, seen from the planted pose (yaw 0.05, t = 0.3 -0.05 0.1)
    const double yaw = 0.05, c = std::cos(yaw), s = std::sin(yaw), R[9] = {c, 0, s, 0, 1, 0, -s, 0, c}, t[3] = {0.3, -0.05, 0.1};
    const double cc[3] = {-(R[0] * t[0] + R[3] * t[1] + R[6] * t[2]), -(R[1] * t[0] + R[4] * t[1] + R[7] * t[2]), -(R[2] * t[0] + R[5] * t[1] + R[8] * t[2])};
    std::vector<uint32_t> ids(n_pt);
    std::vector<float> pos(3 * (size_t)n_pt), nrm(3 * (size_t)n_pt), mind(n_pt), maxd(n_pt), weight(n_pt);
    std::vector<uint8_t> pdesc(32 * (size_t)n_pt);
    for (int p = 0; p < n_pt; p++) {
        ids[p] = 100 + (uint32_t)p;
        const double z = 3 + U(rng) * 27, u = kps[p].x + 0.5 * G(rng), v = kps[p].y + 0.5 * G(rng);
        const double xc[3] = {(u - intr4[2]) / intr4[0] * z - t[0], (v - intr4[3]) / intr4[1] * z - t[1], z - t[2]};
        double d2 = 0;
        for (int k = 0; k < 3; k++) { pos[3 * (size_t)p + k] = (float)(R[k] * xc[0] + R[3 + k] * xc[1] + R[6 + k] * xc[2]); d2 += (cc[k] - pos[3 * (size_t)p + k]) * (cc[k] - pos[3 * (size_t)p + k]); }
        const double dist = std::sqrt(d2);
        for (int k = 0; k < 3; k++) nrm[3 * (size_t)p + k] = (float)((cc[k] - pos[3 * (size_t)p + k]) / dist);
        maxd[p] = (float)(dist * sf[kps[p].octave]); mind[p] = maxd[p] / sf[n_levels - 1];   // Map::updatePointNormalAndDistances
        weight[p] = U(rng) < 0.2 ? 0.5f : 1.f;                                               // MapPoint::isStable
        for (int b = 0; b < 32; b++) pdesc[32 * (size_t)p + b] = desc[32 * (size_t)p + b];
        for (int f = 0; f < 6; f++) { const unsigned bit = rng() & 255; pdesc[32 * (size_t)p + bit / 8] ^= (uint8_t)(1u << (bit % 8)); }
    }
    // ---- the candidates' match lists
    std::vector<Candidate> cand(3);
    for (Candidate& q : cand) { const float kf[6] = {0.f, 0.04f, 0.f, 0.25f, -0.02f, 0.05f}; for (int k = 0; k < 6; k++) q.rt6[k] = kf[k]; }
    for (int p = 0; p < 400; p++) cand[0].matches.push_back(uh_dmatch{U(rng) < 0.7 ? p : (int)(U(rng) * n_kp), (int)ids[p], 0, 20.f});
    for (int p = 0; p < 20; p++) cand[1].matches.push_back(uh_dmatch{p, (int)ids[p], 0, 20.f});
    for (int p = 0; p < 300; p++) cand[2].matches.push_back(uh_dmatch{(p * 7 + 3) % n_kp, (int)ids[(p + 500) % n_pt], 0, 20.f});

    uh_pnp* pnp = nullptr;
    uh_projmatch* pm = nullptr;
    CHECK(uh_pnp_create(ctx, &pnp));
    CHECK(uh_projmatch_create(ctx, &pm));
    const uh_proj_frame frame{kps.data(), n_kp, desc.data(), sf.data(), n_levels, intr4[0], intr4[1], intr4[2], intr4[3], 0, 0, W, H};
    CHECK(uh_projmatch_set_frame(pm, &frame));

    // ---- solvePnPRansac for every candidate with >= 25 matches, one call
    struct Flat { std::vector<float> p3d, normal, kp; std::vector<int32_t> samples, inliers; };
    std::vector<Flat> flat(cand.size());
    std::vector<uh_ransac_problem> prob;
    std::vector<uh_ransac_result> res;
    std::vector<int> live;
    std::srand(1);
    for (size_t ci = 0; ci < cand.size(); ci++) {
        const std::vector<uh_dmatch>& m = cand[ci].matches;
        if (m.size() < 25) { std::printf("candidate %zu: %zu matches, below 25\n", ci, m.size()); continue; }
        Flat& f = flat[ci];
        for (const uh_dmatch& d : m) {
            const size_t p = (size_t)d.trainIdx - 100;
            for (int k = 0; k < 3; k++) { f.p3d.push_back(pos[3 * p + k]); f.normal.push_back(nrm[3 * p + k]); }
            f.kp.push_back(kps[d.queryIdx].x); f.kp.push_back(kps[d.queryIdx].y);
        }
        f.samples.resize(4 * (size_t)max_iters); f.inliers.resize(m.size());
        CHECK(uh_pnp_ransac_samples((int)m.size(), max_iters, f.samples.data()));
        prob.push_back(uh_ransac_problem{(int32_t)m.size(), f.p3d.data(), f.normal.data(), f.kp.data(), max_iters, f.samples.data(), cand[ci].rt6});
        uh_ransac_result r{};
        r.inliers = f.inliers.data(); r.cap = (int32_t)m.size();
        res.push_back(r);
        live.push_back((int)ci);
    }
    CHECK(uh_pnp_ransac(pnp, intr4, (int)prob.size(), prob.data(), res.data()));

    // ---- per survivor: the projection search from the RANSAC pose, then the pose-only optimisation
    const uh_map_points pts{n_pt, ids.data(), pos.data(), nrm.data(), mind.data(), maxd.data(), pdesc.data()};
    int best = -1, best_n = 0;
    float best_pose[16] = {0};
    for (size_t l = 0; l < live.size(); l++) {
        const int ci = live[l];
        const uh_ransac_result& r = res[l];
        // the reference ignores solvePnPRansac's return value: a failed call leaves the list as it was
        const size_t left = r.ok ? (size_t)r.n_inliers : cand[ci].matches.size();
        std::printf("candidate %d: RANSAC %s, best iteration %d, %d inliers of %zu\n", ci, r.ok ? "ok" : "failed", r.best_iter, r.n_inliers, cand[ci].matches.size());
        if (left < 15) continue;
        std::vector<uh_dmatch> mm(n_pt);
        std::vector<uint8_t> visible(n_pt);
        const int nm = uh_projmatch_match(pm, r.pose, &pts, 2 * max_desc_dist, 2.5f, mm.data(), n_pt, nullptr, nullptr, visible.data());
        CHECK(nm);
        std::printf("candidate %d: %d matches from the projection search\n", ci, nm);
        if (nm < 30) continue;
        std::vector<float> p3d(3 * (size_t)nm), kp(2 * (size_t)nm), isg(nm), w(nm);
        for (int i = 0; i < nm; i++) {
            const size_t p = (size_t)mm[i].trainIdx - 100;
            for (int k = 0; k < 3; k++) p3d[3 * (size_t)i + k] = pos[3 * p + k];
            kp[2 * (size_t)i] = kps[mm[i].queryIdx].x; kp[2 * (size_t)i + 1] = kps[mm[i].queryIdx].y;
            isg[i] = inv_sf[kps[mm[i].queryIdx].octave]; w[i] = weight[p];
        }
        float pose[16];
        std::vector<uint8_t> bad(nm);
        int32_t iters[4];
        const int good = uh_pnp_solve(pnp, r.pose, intr4, nm, p3d.data(), kp.data(), isg.data(), w.data(), pose, bad.data(), iters, nullptr);
        CHECK(good);
        std::printf("candidate %d: %d good matches after solvePnp\n", ci, good);
        if (good < 30) continue;
        if (good > best_n) { best = ci; best_n = good; for (int k = 0; k < 16; k++) best_pose[k] = pose[k]; }
    }
    if (best < 0) { std::printf("not relocalised\n"); return 2; }
    const double dt = std::fabs(best_pose[3] - t[0]) + std::fabs(best_pose[7] - t[1]) + std::fabs(best_pose[11] - t[2]);
    std::printf("relocalised on candidate %d with %d matches, |t - planted| = %.4f\n", best, best_n, dt);
    uh_projmatch_destroy(pm);
    uh_pnp_destroy(pnp);
    uh_ctx_destroy(ctx);
    return best == 0 && dt < 0.03 ? 0 : 3;
}
