// Map initialisation from two frames: the exact kNN search pairs the keypoints of the second frame with those of the reference frame,
// ucoslam_hip::MapInitializer runs the two-view initialise on the device (200 homography and 200 fundamental hypotheses, the model
// choice, the decomposition and the triangulation checks), and the result is what MapInitializer::initialize_ turns into two keyframes
// and one map point per surviving match.
//
//   g++ -std=c++17 -O2 -I include examples/map_init.cpp -L ucoslam-cv3_amd -lucoslam_hip -Wl,-rpath,$PWD/ucoslam-cv3_amd -o map_init
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include "ucoslam_hip/adaptors.hpp"

struct Point2f { float x, y; };
struct KeyPoint { Point2f pt; int octave; };
struct ImageParams {
    float fx_, fy_, cx_, cy_;
    float fx() const { return fx_; }
    float fy() const { return fy_; }
    float cx() const { return cx_; }
    float cy() const { return cy_; }
};
struct Frame {   // the members of ucoslam::Frame this stage reads
    std::vector<KeyPoint> und_kpts;
    std::vector<uint8_t> desc;   // 32 bytes per keypoint
    ImageParams imageParams{500.f, 500.f, 320.f, 240.f};
};

int main() {
    try {
        auto ctx = std::make_shared<ucoslam_hip::Context>(0);
        // two toy frames: 300 points 4 to 8 units deep, the second camera half a unit to the side and slightly turned; every point
        // carries a random 256-bit descriptor, seen in the second frame with eight of its bits flipped
        const int n = 300;
        Frame ref, cur;
        unsigned lcg = 7u;
        auto rnd = [&lcg]() { lcg = lcg * 1664525u + 1013904223u; return (double)(lcg >> 8) / 16777216.0; };
        const double th = -0.04, c = std::cos(th), s = std::sin(th), R[9] = {c, 0, s, 0, 1, 0, -s, 0, c}, t[3] = {0.5, 0.02, 0.03};
        for (int i = 0; i < n; i++) {
            const double z = 4.0 + 4.0 * rnd(), x = (rnd() - 0.5) * 0.7 * z, y = (rnd() - 0.5) * 0.5 * z;
            const double q[3] = {R[0] * x + R[1] * y + R[2] * z + t[0], R[3] * x + R[4] * y + R[5] * z + t[1], R[6] * x + R[7] * y + R[8] * z + t[2]};
            ref.und_kpts.push_back(KeyPoint{{(float)(500 * x / z + 320), (float)(500 * y / z + 240)}, 0});
            cur.und_kpts.push_back(KeyPoint{{(float)(500 * q[0] / q[2] + 320), (float)(500 * q[1] / q[2] + 240)}, 0});
            for (int b = 0; b < 32; b++) ref.desc.push_back((uint8_t)(rnd() * 256.0));
            cur.desc.insert(cur.desc.end(), ref.desc.end() - 32, ref.desc.end());
            for (int k = 0; k < 8; k++) cur.desc[32 * (size_t)i + (size_t)(rnd() * 32.0) % 32] ^= (uint8_t)(1u << ((int)(rnd() * 8.0) % 8));
        }
        // the exact search: for every keypoint of the second frame its nearest descriptor in the reference frame
        ucoslam_hip::Index index(ctx);
        index.build(ucoslam_hip::Matrix(ref.desc.data(), n, 32, 1));
        std::vector<int32_t> idx((size_t)n), dist((size_t)n);
        index.search(ucoslam_hip::Matrix(cur.desc.data(), n, 32, 1), 1, ucoslam_hip::Matrix(idx.data(), n, 1, 4), ucoslam_hip::Matrix(dist.data(), n, 1, 4), true);
        std::vector<uh_dmatch> matches;
        for (int i = 0; i < n; i++)
            if (dist[i] < 50) matches.push_back(uh_dmatch{i, idx[i], 0, (float)dist[i]});   // queryIdx: second frame, trainIdx: reference frame
        std::printf("%zu matches\n", matches.size());

        ucoslam_hip::MapInitializer init(ctx);
        ucoslam_hip::MapInitializer::Params params;
        params.minDistance = 0.1f;
        init.setParams(params);
        init.setReferenceFrame(ref);
        const auto r = init.initialize(cur, matches);
        if (!r.ok) { std::printf("not initialised (model %d, RH %.3f): keep the reference frame and try the next frame\n", r.model, r.diagnostics.rh); return 0; }
        std::printf("initialised through the %s: %zu map points, RH %.3f\n", r.model == UH_MAPINIT_HOMOGRAPHY ? "homography" : "fundamental matrix",
                    r.points.size(), r.diagnostics.rh);
        std::printf("pose of the second keyframe:\n");
        for (int i = 0; i < 4; i++) std::printf("  % .5f % .5f % .5f % .5f\n", r.pose_f2g[4 * i], r.pose_f2g[4 * i + 1], r.pose_f2g[4 * i + 2], r.pose_f2g[4 * i + 3]);
        // what initialize_ does next: keyframe 0 = ref with the identity pose, keyframe 1 = cur with r.pose_f2g, and per surviving match a
        // map point at r.points[k] observed by ref's keypoint matches[k].trainIdx and cur's keypoint matches[k].queryIdx
    } catch (const std::runtime_error& e) {
        std::printf("no device: %s\n", e.what());
    }
    return 0;
}
