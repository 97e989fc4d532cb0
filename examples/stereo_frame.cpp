// A stereo frame through the C ABI: FrameExtractor::processStereo as ONE call, then the tracker's pose estimation with the depths it returned.
//
//   uh_orb_extract_stereo    gray conversion + ORB of both images, row index, descriptor match, SAD refinement:   frameextractor.cpp from :1419
//                            Frame::kpts / desc / und_kpts / depth on the host, the frame resident on the device
//   uh_projmatch_set_frame_dev  the resident frame (kd-tree built behind the extraction) becomes the matcher's frame
//   uh_track_pose_stereo     previous-frame search, solvePnp, local-map search, solvePnp — with depth[queryIdx] per match    system.cpp:6559-6954
//
// Scene: a procedural 1241 x 376 image and the same scene 12 px further left with other noise (a rectified pair of constant disparity).  The
// map is made FROM the frame: a point behind every keypoint that got a depth, at that depth, seen from the identity pose; the tracker starts
// 5 cm off.  Prints one JSON line: counts, the pose error after tracking and the median latencies of the two calls.
//
//   g++ -std=c++17 -O2 -o stereo_frame examples/stereo_frame.cpp -Lucoslam-cv3_amd -lucoslam_hip -Wl,-rpath,$PWD/ucoslam-cv3_amd -Wl,-rpath,/opt/rocm/lib
//   ./stereo_frame [frames=100]
#include <algorithm>
#include <chrono>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "../include/ucoslam_hip.h"

#define CHECK(call) do { const int rc_ = (call); if (rc_ < 0) { std::printf("error: %s -> %s\n", #call, uh_last_error()); return 2; } } while (0)

namespace {

constexpr int W = 1241, H = 376, NFEAT = 2000, NLEV = 8, DISPARITY = 12;
constexpr float FX = 718.856f, FY = 718.856f, CX = 607.19f, CY = 185.22f, BL = 0.54f;
constexpr float MAX_DESC_DIST = 50.f, PROJ_DIST_THR = 15.f;   // ORBextractor::getMinDescDistance, Params::projDistThr

void make_frame(uint8_t* out, int shift_x, unsigned seed) {
    std::mt19937 scene(1234);
    const int bw = W + 256, bh = H + 256;
    std::vector<float> img((size_t)bw * bh);
    for (int y = 0; y < bh; y++) for (int x = 0; x < bw; x++) img[(size_t)y * bw + x] = 110.f + 40.f * std::sin(x / 211.f) + 30.f * std::cos(y / 97.f);
    for (int i = 0; i < 3000; i++) {
        const int cx = scene() % bw, cy = scene() % bh, sx = 3 + scene() % 25, sy = 3 + scene() % 25;
        const float c = (30.f + scene() % 91) * ((scene() & 1) ? 1.f : -1.f);
        for (int y = std::max(cy - sy, 0); y < std::min(cy + sy, bh); y++) for (int x = std::max(cx - sx, 0); x < std::min(cx + sx, bw); x++) img[(size_t)y * bw + x] += c;
    }
    std::mt19937 noise(seed);
    std::normal_distribution<float> nd(0.f, 3.f);
    for (int y = 0; y < H; y++) for (int x = 0; x < W; x++) {
        const float v = img[(size_t)(y + 128) * bw + x + 128 + shift_x] + nd(noise);
        out[(size_t)y * W + x] = (uint8_t)std::min(255.f, std::max(0.f, std::nearbyint(v)));
    }
}

double median(std::vector<double> v) { std::sort(v.begin(), v.end()); return v.empty() ? 0.0 : v[v.size() / 2]; }

}  // namespace

int main(int argc, char** argv) {
    const int frames = argc > 1 ? std::max(1, std::atoi(argv[1])) : 100;
    std::vector<uint8_t> left((size_t)W * H), right((size_t)W * H);
    make_frame(left.data(), 0, 5);
    make_frame(right.data(), DISPARITY, 6);

    uh_ctx* ctx = nullptr;
    CHECK(uh_ctx_create_private(0, &ctx));
    uh_orb* orb = nullptr;
    CHECK(uh_orb_create(ctx, &orb));
    const uh_feat_params fp{-1, NFEAT, NLEV, 1.2f, 0.f};
    CHECK(uh_orb_set_params(orb, &fp));
    const uh_camera cam{FX, FY, CX, CY, {0}, 0};
    CHECK(uh_orb_set_camera(orb, &cam));
    CHECK(uh_orb_set_stereo(orb, BL, MAX_DESC_DIST));
    uh_dev_frame* fr = nullptr;
    CHECK(uh_dev_frame_create(ctx, &fr));
    uh_projmatch* pm = nullptr;
    CHECK(uh_projmatch_create(ctx, &pm));
    uh_pnp* pnp = nullptr;
    CHECK(uh_pnp_create(ctx, &pnp));

    std::vector<uh_keypoint> kps(NFEAT);
    std::vector<uint8_t> desc((size_t)NFEAT * 32);
    std::vector<float> und((size_t)NFEAT * 2), depth(NFEAT);
    int n = 0;
    CHECK(uh_orb_extract_stereo(orb, left.data(), right.data(), W, H, W, 1, kps.data(), desc.data(), und.data(), depth.data(), NFEAT, &n, fr, nullptr));

    // the map: a point behind every keypoint with a depth (camera = world at the identity pose), every third of them also a previous-frame item
    std::vector<float> sf(NLEV, 1.f), inv_sf(NLEV, 1.f);
    for (int l = 1; l < NLEV; l++) sf[l] = sf[l - 1] * 1.2f;
    for (int l = 0; l < NLEV; l++) inv_sf[l] = 1.f / sf[l];
    std::vector<uint32_t> ids, prev_ids;
    std::vector<float> pos, nrm, mind, maxd, prev_pos;
    std::vector<uint8_t> mdesc, prev_desc;
    std::vector<int32_t> prev_oct, prev_row;
    int with_depth = 0;
    for (int i = 0; i < n; i++) {
        if (!(depth[i] > 0.f) || !std::isfinite(depth[i])) continue;
        ++with_depth;
        const float z = depth[i], x = (und[2 * i] - CX) / FX * z, y = (und[2 * i + 1] - CY) / FY * z;
        const float d = std::sqrt(x * x + y * y + z * z);
        const int row = (int)ids.size();
        ids.push_back(10 + row);
        pos.insert(pos.end(), {x, y, z});
        nrm.insert(nrm.end(), {-x / d, -y / d, -z / d});
        maxd.push_back(d * sf[kps[i].octave] * 1.02f);
        mind.push_back(maxd.back() / sf[NLEV - 1]);
        mdesc.insert(mdesc.end(), desc.begin() + (size_t)i * 32, desc.begin() + (size_t)(i + 1) * 32);
        if (row % 3 == 0) {
            prev_ids.push_back(ids.back());
            prev_pos.insert(prev_pos.end(), {x, y, z});
            prev_oct.push_back(kps[i].octave);
            prev_desc.insert(prev_desc.end(), desc.begin() + (size_t)i * 32, desc.begin() + (size_t)(i + 1) * 32);
            prev_row.push_back(row);
        }
    }
    const uh_map_points map{(int32_t)ids.size(), ids.data(), pos.data(), nrm.data(), mind.data(), maxd.data(), mdesc.data()};
    const uh_prev_points prev{(int32_t)prev_ids.size(), prev_ids.data(), prev_pos.data(), prev_oct.data(), prev_desc.data()};
    const uh_proj_frame pf{nullptr, 0, nullptr, sf.data(), NLEV, FX, FY, CX, CY, 0, 0, W, H};
    const float pose0[16] = {1, 0, 0, 0.05f, 0, 1, 0, -0.02f, 0, 0, 1, 0.03f, 0, 0, 0, 1};
    const float intr4[4] = {FX, FY, CX, CY};
    uh_track_args ta{};
    ta.pose0 = pose0; ta.intr4 = intr4; ta.inv_sigma_levels = inv_sf.data(); ta.n_levels = NLEV; ta.prev = &prev; ta.prev_map_row = prev_row.data();
    ta.map = &map; ta.map_weight = nullptr; ta.prev_min_desc_dist = MAX_DESC_DIST * 1.5f; ta.prev_max_repj_dist = PROJ_DIST_THR;
    ta.map_min_desc_dist = MAX_DESC_DIST * 2.f; ta.map_radius_tracked = 4.f; ta.map_radius_lost = PROJ_DIST_THR; ta.min_inliers = 30;
    std::vector<uh_dmatch> m_prev(prev.n + 1), m_map(map.n + 1), m_all(prev.n + map.n + 1);
    std::vector<uint8_t> bad_prev(prev.n + 1), bad_all(prev.n + map.n + 1);
    uh_track_result tr{};
    tr.matches_prev = m_prev.data(); tr.bad_prev = bad_prev.data(); tr.cap_prev = (int32_t)m_prev.size();
    tr.matches_map = m_map.data(); tr.cap_map = (int32_t)m_map.size();
    tr.matches_all = m_all.data(); tr.bad_all = bad_all.data(); tr.cap_all = (int32_t)m_all.size();
    const uh_track_stereo ts{depth.data(), BL, nullptr};

    std::vector<double> t_extract, t_track;
    for (int f = 0; f < frames + 10; f++) {
        const auto t0 = std::chrono::steady_clock::now();
        CHECK(uh_orb_extract_stereo(orb, left.data(), right.data(), W, H, W, 1, kps.data(), desc.data(), und.data(), depth.data(), NFEAT, &n, fr, nullptr));
        const auto t1 = std::chrono::steady_clock::now();
        CHECK(uh_projmatch_set_frame_dev(pm, fr, &pf));
        CHECK(uh_track_pose_stereo(pm, pnp, &ta, &ts, &tr));
        const auto t2 = std::chrono::steady_clock::now();
        if (f >= 10) {
            t_extract.push_back(std::chrono::duration<double, std::milli>(t1 - t0).count());
            t_track.push_back(std::chrono::duration<double, std::milli>(t2 - t1).count());
        }
    }
    const double err = std::sqrt((double)tr.pose2[3] * tr.pose2[3] + (double)tr.pose2[7] * tr.pose2[7] + (double)tr.pose2[11] * tr.pose2[11]);
    std::printf("{\"keypoints\": %d, \"with_depth\": %d, \"map_points\": %d, \"prev_items\": %d, \"tracked\": %d, \"inliers1\": %d, \"inliers2\": %d, "
                "\"translation_error_m\": %.5f, \"extract_stereo_ms\": %.4f, \"set_frame_and_track_ms\": %.4f}\n",
                n, with_depth, map.n, prev.n, tr.tracked, tr.inliers1, tr.inliers2, err, median(t_extract), median(t_track));
    uh_pnp_destroy(pnp);
    uh_projmatch_destroy(pm);
    uh_dev_frame_destroy(fr);
    uh_orb_destroy(orb);
    uh_ctx_destroy(ctx);
    return tr.tracked && err < 0.02 ? 0 : 1;
}
