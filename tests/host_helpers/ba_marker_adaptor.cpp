// The marker route of the C++ adaptor ucoslam_hip::GlobalOptimizer (include/ucoslam_hip/adaptors.hpp): a toy map of mk_single's shape —
// 4 keyframes (the first fixed), ~120 landmarks, one marker seen by two free frames and the fixed one — -> flatten_for_ba_markers ->
// uh_ba_set_problem_markers -> optimise -> apply_results / apply_marker_results onto the map.  Compiles with g++ (no OpenCV, no GPU
// needed); without a GPU the context fails loudly ("no device").  With one, the flattened problem and the results are written to the
// file named on the command line (int32 K P E M EM nbad, then poses, fixed, intr, points, obs records, depth, bl, marker poses, sizes,
// edge_marker, edge_frame, corners, weights, result poses, result points, result marker poses) so that the test can run the Python
// route on the same data.
#include <cmath>
#include <cstdio>
#include "../../include/ucoslam_hip/adaptors.hpp"
#include "toy_marker_map.hpp"

static unsigned lcg(unsigned& s) { s = s * 1664525u + 1013904223u; return s >> 8; }
static float unit(unsigned& s) { return (float)(lcg(s) & 0xFFFF) / 65536.f; }

static ToyMarkerMap make_map() {
    ToyMarkerMap m;
    const int K = 4, P = 120;
    const float fx = 500.f, cx = 320.f, cy = 240.f;
    m.frames.resize(K);
    unsigned s = 4242u;
    for (int f = 0; f < K; f++) {
        m.frames[f].valid = true;
        m.frames[f].pose[3] = -0.25f * f + (f ? 0.004f * (unit(s) - 0.5f) : 0.f);   // x_cam = x_world - 0.25 f (+ start error on the free frames)
        m.frames[f].pose[7] = f ? 0.004f * (unit(s) - 0.5f) : 0.f;
        m.order.push_back(f);
    }
    m.points.resize(P);
    m.sf = {1.f, 1.2f, 1.44f};
    for (int p = 0; p < P; p++) {
        const float z = 4.f + 10.f * unit(s), x = (unit(s) - 0.3f) * z, y = (unit(s) - 0.5f) * 0.8f * z;
        m.points[p].xyz[0] = x + 0.01f * (unit(s) - 0.5f); m.points[p].xyz[1] = y + 0.01f * (unit(s) - 0.5f); m.points[p].xyz[2] = z + 0.01f * (unit(s) - 0.5f);
        for (int f = 0; f < K; f++) {
            const float xc = x - 0.25f * f;
            const float u = xc / z * fx + cx + 0.6f * (unit(s) - 0.5f), v = y / z * fx + cy + 0.6f * (unit(s) - 0.5f);
            if (u < 0 || u >= 640 || v < 0 || v >= 480) continue;
            m.observe(p, f, u, v, (int)(lcg(s) % 3));
        }
    }
    // one marker, 0.2 m, facing the cameras 3 m ahead (a half turn about x), seen by frames 0 (fixed), 1 and 2; its map pose starts 1 cm off
    ToyMarker& mk = m.markers[11];
    const float G[16] = {1, 0, 0, 0.30f, 0, -1, 0, 0.05f, 0, 0, -1, 3.0f, 0, 0, 0, 1};
    for (int i = 0; i < 16; i++) mk.pose[i] = G[i];
    mk.size = 0.2f;
    const float h = 0.1f, cxy[4][2] = {{-h, h}, {h, h}, {h, -h}, {-h, -h}};
    m.frame_markers.resize(K);
    for (int f = 0; f < 3; f++) {
        ToyMarkerObs o;
        o.id = 11;
        for (int c = 0; c < 4; c++) {
            const float X = G[3] + cxy[c][0] - 0.25f * f, Y = G[7] - cxy[c][1], Z = G[11];
            o.und_corners[2 * c] = X / Z * fx + cx + 0.4f * (unit(s) - 0.5f);
            o.und_corners[2 * c + 1] = Y / Z * fx + cy + 0.4f * (unit(s) - 0.5f);
        }
        m.frame_markers[f].push_back(o);
        mk.frames.insert(f);
    }
    mk.pose[3] += 0.01f; mk.pose[11] -= 0.01f;
    return m;
}

template <class T> static void put(FILE* f, const T* p, size_t n) { std::fwrite(p, sizeof(T), n, f); }

int main(int argc, char** argv) {
    using namespace ucoslam_hip;
    ToyMarkerMap m = make_map();
    BAParamSet ps;
    ps.nIters = 5;
    StereoVectorSink flat;
    MarkerVectorSink mk;
    FlatBAMarkerIndex mix;
    const FlatBAIndex fix = flatten_for_ba_markers(m, ps, flat, mk, mix);
    const int K = (int)fix.frame_of.size(), P = (int)fix.point_of.size(), E = fix.n_obs, M = (int)mix.marker_of.size(), EM = mix.n_edges;
    bool computed = false;
    for (double w : mk.edge_weight) computed = computed || w != 1.0;
    if (K != 4 || P < 100 || M != 1 || EM != 3 || !computed) { std::printf("toy map not as intended: K %d P %d E %d M %d EM %d\n", K, P, E, M, EM); return 2; }
    try {
        auto ctx = std::make_shared<Context>(0);
        GlobalOptimizer opt(ctx);
        opt.setParamsMarkers(m, ps);
        if (uh_ba_form(opt.handle(), nullptr) != 2) { std::printf("a problem with marker edges must run the wide form\n"); return 3; }
        opt.optimize();
        opt.getResults(m);
        opt.getMarkerResults(m);
        std::vector<float> poses(16 * (size_t)K), points(3 * (size_t)P), mposes(16 * (size_t)M);
        for (int k = 0; k < K; k++) for (int j = 0; j < 16; j++) poses[16 * k + j] = m.frames[fix.frame_of[k]].pose[j];
        for (int p = 0; p < P; p++) for (int j = 0; j < 3; j++) points[3 * p + j] = m.points[fix.point_of[p]].xyz[j];
        for (int i = 0; i < M; i++) for (int j = 0; j < 16; j++) mposes[16 * i + j] = m.markers[mix.marker_of[i]].pose[j];
        const int nbad = (int)opt.getBadAssociations().size();
        if (argc > 1) {
            FILE* f = std::fopen(argv[1], "wb");
            if (!f) { std::printf("cannot write %s\n", argv[1]); return 4; }
            const int32_t head[6] = {K, P, E, M, EM, nbad};
            put(f, head, 6); put(f, flat.poses.data(), flat.poses.size()); put(f, flat.fixed.data(), flat.fixed.size()); put(f, flat.intr.data(), flat.intr.size());
            put(f, flat.points.data(), flat.points.size()); put(f, flat.obs.data(), flat.obs.size()); put(f, flat.depth.data(), flat.depth.size());
            put(f, flat.bl.data(), flat.bl.size());
            put(f, mk.pose_g2m.data(), mk.pose_g2m.size()); put(f, mk.size.data(), mk.size.size()); put(f, mk.edge_marker.data(), mk.edge_marker.size());
            put(f, mk.edge_frame.data(), mk.edge_frame.size()); put(f, mk.und_corners.data(), mk.und_corners.size()); put(f, mk.edge_weight.data(), mk.edge_weight.size());
            put(f, poses.data(), poses.size()); put(f, points.data(), points.size()); put(f, mposes.data(), mposes.size());
            std::fclose(f);
        }
        std::printf("ba marker ok: K %d P %d E %d markers %d edges %d bad %d\n", K, P, E, M, EM, nbad);
    } catch (const std::runtime_error& e) {
        std::printf("no device: %s\n", e.what());   // expected on the CPU-only build box: no fallback exists
    }
    return 0;
}
