// Compiles the stereo / RGB-D overload of the C++ adaptor ucoslam_hip::PnPSolver::solvePnp (include/ucoslam_hip/adaptors.hpp) with g++
// (no OpenCV, no GPU needed).  Without a GPU the context fails loudly ("no device"); with one, a small stereo problem is solved through the
// overload: 60 points seen from the identity pose, two thirds of them with their depth, the start pose shifted by a few centimetres.
#include <cmath>
#include <cstdio>
#include "../../include/ucoslam_hip/adaptors.hpp"

int main() {
    try {
        auto ctx = std::make_shared<ucoslam_hip::Context>(0);
        const float fx = 500.f, fy = 500.f, cx = 320.f, cy = 240.f, intr[4] = {fx, fy, cx, cy}, bl = 0.12f;
        const int n = 60;
        std::vector<float> p3d(3 * n), kp(2 * n), isg(n, 1.f), w(n, 1.f), depth(n, 0.f);
        for (int i = 0; i < n; i++) {
            const float x = -2.f + 4.f * (float)(i % 10) / 9.f, y = -1.5f + 3.f * (float)(i / 10) / 5.f, z = 4.f + (float)((i * 7) % 11);
            p3d[3 * i] = x; p3d[3 * i + 1] = y; p3d[3 * i + 2] = z;
            kp[2 * i] = x / z * fx + cx; kp[2 * i + 1] = y / z * fy + cy;
            if (i % 3) depth[i] = z;
            if (i % 5 == 0) w[i] = 0.5f;
        }
        float pose[16] = {1, 0, 0, 0.05f, 0, 1, 0, -0.03f, 0, 0, 1, 0.04f, 0, 0, 0, 1};
        std::vector<uint8_t> bad;
        ucoslam_hip::PnPSolver pnp(ctx);
        const int good = pnp.solvePnp(pose, intr, n, p3d.data(), kp.data(), isg.data(), w.data(), depth.data(), bl, bad);
        const float err = std::fabs(pose[3]) + std::fabs(pose[7]) + std::fabs(pose[11]);
        if (good != n || bad.size() != (size_t)n || !(err < 1e-3f)) { std::printf("stereo solve wrong: %d inliers, |t| %g\n", good, err); return 2; }
        // a depth without a baseline is refused
        bool refused = false;
        try { pnp.solvePnp(pose, intr, n, p3d.data(), kp.data(), isg.data(), w.data(), depth.data(), 0.f, bad); } catch (const std::runtime_error&) { refused = true; }
        if (!refused) { std::printf("bl = 0 accepted\n"); return 3; }
        std::printf("stereo ok: %d inliers, |t| %g\n", good, err);
    } catch (const std::runtime_error& e) {
        std::printf("no device: %s\n", e.what());   // expected on the CPU-only build box: no fallback exists
    }
    return 0;
}
