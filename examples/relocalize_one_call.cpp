// System::relocalize's pose search for the candidate keyframes of one lost frame through BOTH routes of the C ABI, on the scene of
// examples/relocalize.cpp:
//   (a) operator by operator, as examples/relocalize.cpp does it: uh_pnp_ransac for every candidate with >= 25 matches, then per survivor
//       uh_projmatch_match, the host's id -> row look-ups and uh_pnp_solve;
//   (b) ucoslam_hip::Relocalizer::relocalize (include/ucoslam_hip/adaptors.hpp) = ONE uh_relocalize_pose over a device-resident frame.
// Every stage, list, flag, count and pose of (b) must equal (a) bit for bit; any difference ends the program with a non-zero status.
//
//   g++ -std=c++17 -O2 -o relocalize_one_call examples/relocalize_one_call.cpp -Lucoslam-cv3_amd -lucoslam_hip -Wl,-rpath,$PWD/ucoslam-cv3_amd -Wl,-rpath,/opt/rocm/lib
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "../include/ucoslam_hip/adaptors.hpp"

#define CHECK(expr)                                                                              \
    do {                                                                                         \
        const int rc_ = (expr);                                                                  \
        if (rc_ < 0) { std::printf("%s failed: %s\n", #expr, uh_last_error()); return 1; }      \
    } while (0)

using ucoslam_hip::Relocalizer;

int main() {
    std::shared_ptr<ucoslam_hip::Context> context;
    try { context = std::make_shared<ucoslam_hip::Context>(0); }
    catch (const std::exception& e) { std::printf("no device: %s (there is no CPU path)\n", e.what()); return 0; }
    uh_ctx* ctx = context->get();
    const float intr4[4] = {718.856f, 718.856f, 607.19f, 185.22f};
    const int W = 1241, H = 376, n_kp = 1500, n_pt = 1200, n_levels = 8, max_iters = 50;
    const float max_desc_dist = 50.f;
    std::mt19937 rng(7);
    std::uniform_real_distribution<double> U(0, 1);
    std::normal_distribution<double> G(0, 1);
    std::vector<float> sf(n_levels, 1.f), inv_sf(n_levels, 1.f);
    for (int l = 1; l < n_levels; l++) sf[l] = sf[l - 1] * 1.2f;
    for (int l = 0; l < n_levels; l++) inv_sf[l] = 1.f / sf[l];
    // ---- the lost frame, the map and the candidates' match lists: examples/relocalize.cpp's, draw for draw
    std::vector<uh_keypoint> kps(n_kp);
    std::vector<uint8_t> desc(32 * (size_t)n_kp);
    for (int i = 0; i < n_kp; i++) {
        kps[i] = uh_keypoint{(float)(20 + U(rng) * (W - 40)), (float)(20 + U(rng) * (H - 40)), 31.f, 0.f, 50.f, (int32_t)(U(rng) * 4), -1};
        for (int b = 0; b < 32; b++) desc[32 * (size_t)i + b] = (uint8_t)(rng() & 255);
    }
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
        maxd[p] = (float)(dist * sf[kps[p].octave]); mind[p] = maxd[p] / sf[n_levels - 1];
        weight[p] = U(rng) < 0.2 ? 0.5f : 1.f;
        for (int b = 0; b < 32; b++) pdesc[32 * (size_t)p + b] = desc[32 * (size_t)p + b];
        for (int f = 0; f < 6; f++) { const unsigned bit = rng() & 255; pdesc[32 * (size_t)p + bit / 8] ^= (uint8_t)(1u << (bit % 8)); }
    }
    const uh_map_points pts{n_pt, ids.data(), pos.data(), nrm.data(), mind.data(), maxd.data(), pdesc.data()};
    std::vector<Relocalizer::Candidate> cand(3);
    for (Relocalizer::Candidate& q : cand) {
        const float kf[6] = {0.f, 0.04f, 0.f, 0.25f, -0.02f, 0.05f};
        for (int k = 0; k < 6; k++) q.rt6[k] = kf[k];
        q.points = pts; q.weight = weight.data();
    }
    for (int p = 0; p < 400; p++) cand[0].matches.push_back(uh_dmatch{U(rng) < 0.7 ? p : (int)(U(rng) * n_kp), (int)ids[p], 0, 20.f});
    for (int p = 0; p < 20; p++) cand[1].matches.push_back(uh_dmatch{p, (int)ids[p], 0, 20.f});
    for (int p = 0; p < 300; p++) cand[2].matches.push_back(uh_dmatch{(p * 7 + 3) % n_kp, (int)ids[(p + 500) % n_pt], 0, 20.f});
    std::vector<std::vector<float>> kp2(cand.size());
    for (size_t ci = 0; ci < cand.size(); ci++)
        for (const uh_dmatch& d : cand[ci].matches) {
            const size_t p = (size_t)d.trainIdx - 100;
            for (int k = 0; k < 3; k++) { cand[ci].p3d.push_back(pos[3 * p + k]); cand[ci].normal.push_back(nrm[3 * p + k]); }
            kp2[ci].push_back(kps[d.queryIdx].x); kp2[ci].push_back(kps[d.queryIdx].y);
        }
    const uh_proj_frame frame{kps.data(), n_kp, desc.data(), sf.data(), n_levels, intr4[0], intr4[1], intr4[2], intr4[3], 0, 0, W, H};

    // ================= (a) operator by operator =================
    uh_pnp* pnp = nullptr;
    uh_projmatch* pm = nullptr;
    CHECK(uh_pnp_create(ctx, &pnp));
    CHECK(uh_projmatch_create(ctx, &pm));
    CHECK(uh_projmatch_set_frame(pm, &frame));
    std::vector<Relocalizer::Step> want(cand.size());
    std::vector<std::vector<int32_t>> samples(cand.size());
    std::vector<uh_ransac_problem> prob;
    std::vector<uh_ransac_result> res;
    std::vector<int> live;
    std::srand(1);
    for (size_t ci = 0; ci < cand.size(); ci++) {
        const size_t n = cand[ci].matches.size();
        if (n < 25) continue;
        samples[ci].resize(4 * (size_t)max_iters); want[ci].inliers.resize(n);
        CHECK(uh_pnp_ransac_samples((int)n, max_iters, samples[ci].data()));
        prob.push_back(uh_ransac_problem{(int32_t)n, cand[ci].p3d.data(), cand[ci].normal.data(), kp2[ci].data(), max_iters, samples[ci].data(), cand[ci].rt6});
        uh_ransac_result r{};
        r.inliers = want[ci].inliers.data(); r.cap = (int32_t)n;
        res.push_back(r);
        live.push_back((int)ci);
    }
    CHECK(uh_pnp_ransac(pnp, intr4, (int)prob.size(), prob.data(), res.data()));
    const int after_draws = std::rand();
    int best = -1, best_n = 0;
    float best_pose[16] = {0};
    for (size_t l = 0; l < live.size(); l++) {
        const int ci = live[l];
        const uh_ransac_result& r = res[l];
        Relocalizer::Step& w = want[ci];
        w.stage = UH_RELOC_FEW_AFTER_RANSAC; w.ok = r.ok; w.n_inliers = r.n_inliers; w.best_iter = r.best_iter;
        std::memcpy(w.rt6, r.rt6, sizeof(w.rt6)); std::memcpy(w.pose_ransac, r.pose, sizeof(w.pose_ransac));
        w.inliers.resize((size_t)r.n_inliers);
        const size_t left = r.ok ? (size_t)r.n_inliers : cand[ci].matches.size();
        if (left < 15) continue;
        w.stage = UH_RELOC_FEW_MAP;
        w.matches_map.resize(n_pt);
        const int nm = uh_projmatch_match(pm, r.pose, &pts, 2 * max_desc_dist, 2.5f, w.matches_map.data(), n_pt, nullptr, nullptr, nullptr);
        CHECK(nm);
        w.matches_map.resize((size_t)nm);
        if (nm < 30) continue;
        w.stage = UH_RELOC_FEW_GOOD;
        std::vector<float> p3d(3 * (size_t)nm), kp(2 * (size_t)nm), isg(nm), wg(nm);
        for (int i = 0; i < nm; i++) {
            const size_t p = (size_t)w.matches_map[i].trainIdx - 100;
            for (int k = 0; k < 3; k++) p3d[3 * (size_t)i + k] = pos[3 * p + k];
            kp[2 * (size_t)i] = kps[w.matches_map[i].queryIdx].x; kp[2 * (size_t)i + 1] = kps[w.matches_map[i].queryIdx].y;
            isg[i] = inv_sf[kps[w.matches_map[i].queryIdx].octave]; wg[i] = weight[p];
        }
        w.bad.assign((size_t)nm, 0);
        w.solve_inliers = uh_pnp_solve(pnp, r.pose, intr4, nm, p3d.data(), kp.data(), isg.data(), wg.data(), w.pose_solve, w.bad.data(), w.iters, nullptr);
        CHECK(w.solve_inliers);
        for (int i = 0; i < nm; i++) w.n_good += w.bad[i] == 0;
        if (w.n_good < 30) continue;
        w.stage = UH_RELOC_SOLVED;
        if (w.n_good > best_n) { best = ci; best_n = w.n_good; std::memcpy(best_pose, w.pose_solve, sizeof(best_pose)); }
    }
    uh_projmatch_destroy(pm);
    uh_pnp_destroy(pnp);

    // ================= (b) one call =================
    Relocalizer::Result got;
    int after_draws_b = 0;
    try {
        Relocalizer rl(context);
        rl.setFrame(frame);
        std::srand(1);
        got = rl.relocalize(intr4, inv_sf, cand, max_desc_dist, max_iters);   // (samples == NULL: drawn inside, as route (a) drew them)
        after_draws_b = std::rand();
    } catch (const std::exception& e) { std::printf("Relocalizer failed: %s\n", e.what()); return 1; }

    // ================= compare =================
    int diffs = 0;
#define SAME(what, cond) do { if (!(cond)) { std::printf("DIFFERENT: %s\n", what); diffs++; } } while (0)
    SAME("rand() after the call", after_draws == after_draws_b);
    SAME("best", got.best == best);
    SAME("n_matches", got.n_matches == best_n);
    SAME("pose", best < 0 || std::memcmp(got.pose, best_pose, sizeof(best_pose)) == 0);
    for (size_t ci = 0; ci < cand.size(); ci++) {
        const Relocalizer::Step &w = want[ci], &g = got.steps[ci];
        std::printf("candidate %zu: stage %d / %d, RANSAC ok %d / %d with %d / %d inliers, %zu / %zu matches from the projection search, %d / %d good\n", ci, w.stage, g.stage, w.ok,
                    g.ok, w.n_inliers, g.n_inliers, w.matches_map.size(), g.matches_map.size(), w.n_good, g.n_good);
        SAME("stage", w.stage == g.stage);
        SAME("RANSAC result", w.ok == g.ok && w.n_inliers == g.n_inliers && w.best_iter == g.best_iter);
        SAME("rt6 / pose_ransac", std::memcmp(w.rt6, g.rt6, sizeof(w.rt6)) == 0 && std::memcmp(w.pose_ransac, g.pose_ransac, sizeof(w.pose_ransac)) == 0);
        SAME("inliers", w.inliers.size() == g.inliers.size() && (w.inliers.empty() || std::memcmp(w.inliers.data(), g.inliers.data(), 4 * w.inliers.size()) == 0));
        SAME("matches_map", w.matches_map.size() == g.matches_map.size() &&
                                (w.matches_map.empty() || std::memcmp(w.matches_map.data(), g.matches_map.data(), sizeof(uh_dmatch) * w.matches_map.size()) == 0));
        SAME("bad", w.bad == g.bad);
        SAME("pose_solve / iters / counts", std::memcmp(w.pose_solve, g.pose_solve, sizeof(w.pose_solve)) == 0 && std::memcmp(w.iters, g.iters, sizeof(w.iters)) == 0 &&
                                                w.solve_inliers == g.solve_inliers && w.n_good == g.n_good);
    }
    if (diffs) { std::printf("%d differences between the two routes\n", diffs); return 4; }
    if (got.best < 0) { std::printf("not relocalised\n"); return 2; }
    const double dt = std::fabs(got.pose[3] - t[0]) + std::fabs(got.pose[7] - t[1]) + std::fabs(got.pose[11] - t[2]);
    std::printf("relocalised on candidate %d with %d matches, |t - planted| = %.4f\n", got.best, got.n_matches, dt);
    return got.best == 0 && dt < 0.03 ? 0 : 3;
}
