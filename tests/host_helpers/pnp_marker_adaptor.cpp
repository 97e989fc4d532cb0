// Compiles the marker overload of the C++ adaptor ucoslam_hip::PnPSolver::solvePnp (include/ucoslam_hip/adaptors.hpp) with g++ (no OpenCV,
// no GPU needed).  Without a GPU the context fails loudly ("no device"); with one, two small problems are solved through the overload from
// a start pose shifted by a few centimetres: 60 points plus two markers seen from the identity pose, and the two markers alone.
#include <cmath>
#include <cstdio>
#include "../../include/ucoslam_hip/adaptors.hpp"

int main() {
    try {
        auto ctx = std::make_shared<ucoslam_hip::Context>(0);
        const float fx = 500.f, fy = 500.f, cx = 320.f, cy = 240.f, intr[4] = {fx, fy, cx, cy};
        const int n = 60;
        std::vector<float> p3d(3 * n), kp(2 * n), isg(n, 1.f), w(n, 1.f);
        for (int i = 0; i < n; i++) {
            const float x = -2.f + 4.f * (float)(i % 10) / 9.f, y = -1.5f + 3.f * (float)(i / 10) / 5.f, z = 4.f + (float)((i * 7) % 11);
            p3d[3 * i] = x; p3d[3 * i + 1] = y; p3d[3 * i + 2] = z;
            kp[2 * i] = x / z * fx + cx; kp[2 * i + 1] = y / z * fy + cy;
            if (i % 5 == 0) w[i] = 0.5f;
        }
        // two markers facing the camera (a half turn about x), at different depths; the camera's true pose is the identity
        std::vector<ucoslam_hip::PnPSolver::Marker> markers(2);
        for (int m = 0; m < 2; m++) {
            ucoslam_hip::PnPSolver::Marker& mk = markers[m];
            const float tx = m ? 0.6f : -0.5f, ty = m ? -0.2f : 0.3f, tz = m ? 3.f : 2.f;
            const float G[16] = {1, 0, 0, tx, 0, -1, 0, ty, 0, 0, -1, tz, 0, 0, 0, 1};
            for (int i = 0; i < 16; i++) mk.pose_g2m[i] = G[i];
            mk.size = m ? 0.2f : 0.15f;
            const float h = mk.size / 2, lx[4] = {-h, h, h, -h}, ly[4] = {h, h, -h, -h};
            for (int c = 0; c < 4; c++) {
                const float X = lx[c] + tx, Y = -ly[c] + ty, Z = tz;
                mk.und_corners[2 * c] = X / Z * fx + cx; mk.und_corners[2 * c + 1] = Y / Z * fy + cy;
            }
        }
        const float start[16] = {1, 0, 0, 0.05f, 0, 1, 0, -0.03f, 0, 0, 1, 0.04f, 0, 0, 0, 1};
        std::vector<uint8_t> bad;
        ucoslam_hip::PnPSolver pnp(ctx);
        float pose[16];
        std::copy(start, start + 16, pose);
        const int good = pnp.solvePnp(pose, intr, n, p3d.data(), kp.data(), isg.data(), w.data(), nullptr, 0.f, markers, bad);
        const float err = std::fabs(pose[3]) + std::fabs(pose[7]) + std::fabs(pose[11]);
        if (good != n || bad.size() != (size_t)n || !(err < 1e-3f)) { std::printf("marker solve wrong: %d inliers, |t| %g\n", good, err); return 2; }
        // the markers alone (no keypoint match: infinite marker weight, the robust kernels go after the first round)
        std::copy(start, start + 16, pose);
        const int good0 = pnp.solvePnp(pose, intr, 0, nullptr, nullptr, nullptr, nullptr, nullptr, 0.f, markers, bad);
        const float err0 = std::fabs(pose[3]) + std::fabs(pose[7]) + std::fabs(pose[11]);
        if (good0 != 0 || !bad.empty() || !(err0 < 5e-3f)) { std::printf("marker-only solve wrong: %d, |t| %g\n", good0, err0); return 3; }
        // a marker without a size is refused
        markers[1].size = 0.f;
        bool refused = false;
        try { pnp.solvePnp(pose, intr, n, p3d.data(), kp.data(), isg.data(), w.data(), nullptr, 0.f, markers, bad); } catch (const std::runtime_error&) { refused = true; }
        if (!refused) { std::printf("size = 0 accepted\n"); return 4; }
        std::printf("markers ok: %d inliers, |t| %g, marker-only |t| %g\n", good, err, err0);
    } catch (const std::runtime_error& e) {
        std::printf("no device: %s\n", e.what());   // expected on the CPU-only build box: no fallback exists
    }
    return 0;
}
