// Compiles ucoslam_hip::PnPSolver::solvePnPRansac (include/ucoslam_hip/adaptors.hpp), the single and the batched overload, against stub
// views with g++ (no OpenCV, no GPU needed).  Without a GPU the context fails loudly ("no device"); with one, a planted scene is solved:
// 80 map points seen from a known pose, every fifth match a gross outlier; beside it a candidate with 3 matches (false, nothing touched)
// and one whose keypoints are all wrong (false, matches untouched).  With an argument, the inputs and results are dumped for the Python
// mirror to repeat.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include "../../include/ucoslam_hip/adaptors.hpp"
#include "toy_frames.hpp"

struct StubMap {   // the two members the adaptor reads
    std::vector<std::array<float, 3>> xyz, normal;
    void point_coordinates(uint32_t p, float* out) const { for (int i = 0; i < 3; i++) out[i] = xyz[p][i]; }
    void point_normal(uint32_t p, float* out) const { for (int i = 0; i < 3; i++) out[i] = normal[p][i]; }
};

int main(int argc, char** argv) {
    try {
        auto ctx = std::make_shared<ucoslam_hip::Context>(0);
        ToyViewFrame frame;
        frame.imageParams = ToyImageParams{718.856f, 718.856f, 607.19f, 185.22f};
        StubMap map;
        const int n = 80;
        // the planted pose: a rotation of 0.2 rad about y and a shift
        const double th = 0.2, c = std::cos(th), s = std::sin(th), R[9] = {c, 0, s, 0, 1, 0, -s, 0, c}, t[3] = {0.3, -0.1, 0.2};
        const double centre[3] = {-(R[0] * t[0] + R[3] * t[1] + R[6] * t[2]), -(R[1] * t[0] + R[4] * t[1] + R[7] * t[2]), -(R[2] * t[0] + R[5] * t[1] + R[8] * t[2])};
        std::vector<uh_dmatch> good, wrong, few;
        for (int i = 0; i < n; i++) {
            const double u = 40 + (i % 10) * 125.0, v = 30 + (i / 10) * 42.0, z = 2.5 + (i * 7 % 13) * 0.55;
            const double xc[3] = {(u - 607.19) / 718.856 * z, (v - 185.22) / 718.856 * z, z}, d[3] = {xc[0] - t[0], xc[1] - t[1], xc[2] - t[2]};
            std::array<float, 3> X, N;
            double w[3], nn = 0;
            for (int k = 0; k < 3; k++) { w[k] = R[k] * d[0] + R[3 + k] * d[1] + R[6 + k] * d[2]; X[k] = (float)w[k]; }
            for (int k = 0; k < 3; k++) nn += (centre[k] - w[k]) * (centre[k] - w[k]);
            for (int k = 0; k < 3; k++) N[k] = (float)((centre[k] - w[k]) / std::sqrt(nn));
            map.xyz.push_back(X); map.normal.push_back(N);
            const double xr[3] = {R[0] * X[0] + R[1] * X[1] + R[2] * X[2] + t[0], R[3] * X[0] + R[4] * X[1] + R[5] * X[2] + t[1], R[6] * X[0] + R[7] * X[1] + R[8] * X[2] + t[2]};
            ToyKeyPoint kp{{(float)(718.856 * xr[0] / xr[2] + 607.19), (float)(718.856 * xr[1] / xr[2] + 185.22)}, 0};
            if (i % 5 == 4) { kp.pt.x += 60.f; kp.pt.y -= 45.f; }
            frame.und_kpts.push_back(kp);
            good.push_back(uh_dmatch{i, i, 0, 10.f});
            if (i < 3) few.push_back(uh_dmatch{i, i, 0, 10.f});
        }
        // six map points on keypoints that have nothing to do with them (few enough that no hypothesis meets a fourth inlier by chance:
        // a keypoint falls into a given 2.45 px disc of the 1241 x 376 image with probability 4e-5)
        unsigned lcg = 12345u;
        for (int i = 0; i < 6; i++) {
            lcg = lcg * 1664525u + 1013904223u; const float x = 20.f + (float)(lcg >> 8) / 16777216.f * 1200.f;
            lcg = lcg * 1664525u + 1013904223u; const float y = 20.f + (float)(lcg >> 8) / 16777216.f * 330.f;
            frame.und_kpts.push_back(ToyKeyPoint{{x, y}, 0});
            wrong.push_back(uh_dmatch{n + i, 7 * i + 2, 0, 10.f});
        }
        ucoslam_hip::PnPSolver pnp(ctx);
        const float start[6] = {0.01f, 0.02f, 0.03f, 0.f, 0.f, 0.f};
        float pose_good[6], pose_wrong[6], pose_few[6];
        for (int k = 0; k < 6; k++) pose_good[k] = pose_wrong[k] = pose_few[k] = start[k];
        const std::vector<uh_dmatch> good_in = good, wrong_in = wrong;
        std::srand(4711);
        const std::vector<bool> ok = pnp.solvePnPRansac(frame, map, {&good, &few, &wrong}, {pose_good, pose_few, pose_wrong}, 50);
        const double dr = std::fabs(pose_good[1] - th) + std::fabs(pose_good[0]) + std::fabs(pose_good[2]);
        const double dt = std::fabs(pose_good[3] - t[0]) + std::fabs(pose_good[4] - t[1]) + std::fabs(pose_good[5] - t[2]);
        if (!ok[0] || good.size() != 64 || !(dr < 1e-3) || !(dt < 1e-2)) { std::printf("planted candidate wrong: ok %d, %zu inliers, dr %g dt %g\n", (int)ok[0], good.size(), dr, dt); return 2; }
        for (const uh_dmatch& m : good) if (m.queryIdx % 5 == 4) { std::printf("an outlier was kept\n"); return 3; }
        bool few_same = !ok[1] && few.size() == 3;
        for (int k = 0; k < 6; k++) few_same = few_same && pose_few[k] == start[k];
        if (!few_same) { std::printf("three matches: something was touched\n"); return 4; }
        if (ok[2] || wrong.size() != wrong_in.size()) { std::printf("wrong matches accepted or altered\n"); return 5; }
        // the single overload draws the same samples after the same srand and gives the same answer
        std::vector<uh_dmatch> again = good_in;
        float pose_again[6];
        for (int k = 0; k < 6; k++) pose_again[k] = start[k];
        std::srand(4711);
        const bool ok1 = pnp.solvePnPRansac(frame, map, again, pose_again);
        bool same = ok1 && again.size() == good.size();
        for (int k = 0; k < 6 && same; k++) same = pose_again[k] == pose_good[k];
        if (!same) { std::printf("single overload differs from the batched one\n"); return 6; }
        if (argc > 1) {
            FILE* f = std::fopen(argv[1], "wb");
            if (!f) return 7;
            const int32_t hdr[2] = {n, (int32_t)good.size()};
            std::fwrite(hdr, sizeof hdr, 1, f);
            for (int i = 0; i < n; i++) { std::fwrite(map.xyz[i].data(), 4, 3, f); std::fwrite(map.normal[i].data(), 4, 3, f); std::fwrite(&frame.und_kpts[i].pt, 4, 2, f); }
            std::fwrite(pose_good, 4, 6, f);
            for (const uh_dmatch& m : good) std::fwrite(&m.queryIdx, 4, 1, f);
            std::fclose(f);
        }
        std::printf("ransac adaptor ok: %zu inliers, dr %g dt %g\n", good.size(), dr, dt);
    } catch (const std::runtime_error& e) {
        std::printf("no device: %s\n", e.what());   // expected on the CPU-only build box: no fallback exists
    }
    return 0;
}
