// Compiles ucoslam_hip::MapInitializer (include/ucoslam_hip/adaptors.hpp) against the toy frames with g++ (no OpenCV, no GPU needed).
// Without a GPU the context fails loudly ("no device"); with one, two views of 160 planted points initialise a map: the second camera
// 0.5 to the side of the first, points 4 to 8 deep.  With an argument the inputs and results are dumped for the Python mirror to repeat.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include "../../include/ucoslam_hip/adaptors.hpp"
#include "toy_frames.hpp"

int main(int argc, char** argv) {
    try {
        auto ctx = std::make_shared<ucoslam_hip::Context>(0);
        ToyViewFrame f1, f2;
        f1.imageParams = f2.imageParams = ToyImageParams{500.f, 500.f, 320.f, 240.f};
        const int n = 160;
        const double th = -0.05, c = std::cos(th), s = std::sin(th), R[9] = {c, 0, s, 0, 1, 0, -s, 0, c}, t[3] = {0.5, 0.03, 0.02};
        std::vector<uh_dmatch> matches;
        unsigned lcg = 2024u;
        auto rnd = [&lcg]() { lcg = lcg * 1664525u + 1013904223u; return (double)(lcg >> 8) / 16777216.0; };
        for (int i = 0; i < n; i++) {
            const double z = 4.0 + 4.0 * rnd(), x = (rnd() - 0.5) * 0.7 * z, y = (rnd() - 0.5) * 0.5 * z;
            const double q[3] = {R[0] * x + R[1] * y + R[2] * z + t[0], R[3] * x + R[4] * y + R[5] * z + t[1], R[6] * x + R[7] * y + R[8] * z + t[2]};
            f1.und_kpts.push_back(ToyKeyPoint{{(float)(500 * x / z + 320), (float)(500 * y / z + 240)}, 0});
            f2.und_kpts.push_back(ToyKeyPoint{{(float)(500 * q[0] / q[2] + 320), (float)(500 * q[1] / q[2] + 240)}, 0});
            matches.push_back(uh_dmatch{i, i, 0, 10.f});
        }
        ucoslam_hip::MapInitializer init(ctx);
        ucoslam_hip::MapInitializer::Params p;
        p.minDistance = 0.2f;
        init.setParams(p);
        bool threw = false;
        try { init.initialize(f2, matches); } catch (const std::runtime_error&) { threw = true; }
        if (!threw) { std::printf("initialize without a reference frame did not throw\n"); return 2; }
        init.setReferenceFrame(f1);
        const std::vector<uh_dmatch> few(matches.begin(), matches.begin() + 49);
        if (init.initialize(f2, few).ok) { std::printf("49 matches initialised a map\n"); return 3; }
        const auto r = init.initialize(f2, matches);
        if (!r.ok || r.matches.size() != r.points.size() || r.matches.size() < 150) { std::printf("planted scene: ok %d, %zu survivors\n", (int)r.ok, r.matches.size()); return 4; }
        // t * minDistance: the translation column has length 0.2 and points along the planted direction
        const double tn = std::sqrt((double)r.pose_f2g[3] * r.pose_f2g[3] + (double)r.pose_f2g[7] * r.pose_f2g[7] + (double)r.pose_f2g[11] * r.pose_f2g[11]);
        const double dir = (r.pose_f2g[3] * t[0] + r.pose_f2g[7] * t[1] + r.pose_f2g[11] * t[2]) / (tn * std::sqrt(t[0] * t[0] + t[1] * t[1] + t[2] * t[2]));
        if (std::fabs(tn - 0.2) > 1e-5 || dir < 0.99 || std::fabs(r.pose_f2g[2] - s) > 0.01) { std::printf("pose wrong: |t| %g, cos %g, R02 %g\n", tn, dir, (double)r.pose_f2g[2]); return 5; }
        for (const auto& pt : r.points) if (!(pt[2] > 0)) { std::printf("a point behind the reference camera\n"); return 6; }
        init.reset();
        if (init.hasReferenceFrame()) return 7;
        if (argc > 1) {
            FILE* f = std::fopen(argv[1], "wb");
            if (!f) return 8;
            const int32_t hdr[2] = {n, (int32_t)r.matches.size()};
            std::fwrite(hdr, sizeof hdr, 1, f);
            for (int i = 0; i < n; i++) { std::fwrite(&f1.und_kpts[i].pt, 4, 2, f); std::fwrite(&f2.und_kpts[i].pt, 4, 2, f); }
            std::fwrite(r.pose_f2g.data(), 4, 16, f);
            for (const uh_dmatch& m : r.matches) std::fwrite(&m.trainIdx, 4, 1, f);
            for (const auto& pt : r.points) std::fwrite(pt.data(), 4, 3, f);
            std::fclose(f);
        }
        std::printf("mapinit adaptor ok: %zu points, model %d\n", r.matches.size(), r.model);
    } catch (const std::runtime_error& e) {
        std::printf("no device: %s\n", e.what());   // expected on the CPU-only build box: no fallback exists
    }
    return 0;
}
