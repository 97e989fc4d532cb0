// The stereo route of the C++ adaptor ucoslam_hip::GlobalOptimizer (include/ucoslam_hip/adaptors.hpp): a toy map with depths ->
// flatten_for_ba_stereo into the optimiser's staging block -> optimise -> apply_results onto the map.  Compiles with g++ (no OpenCV, no
// GPU needed); without a GPU the context fails loudly ("no device").  With one, the flattened problem and the results are written to the
// file named on the command line (int32 K P E, then poses, fixed, intr, points, obs records, depth, bl, result poses, result points,
// number of bad associations) so that the test can run the Python route on the same data.
#include <cmath>
#include <cstdio>
#include "../../include/ucoslam_hip/adaptors.hpp"
#include "toy_map.hpp"

struct StereoToyMap : ToyMap {
    std::vector<float> bl;
    float frame_baseline(uint32_t f) const { return bl[f]; }
};

static unsigned lcg(unsigned& s) { s = s * 1664525u + 1013904223u; return s >> 8; }
static float unit(unsigned& s) { return (float)(lcg(s) & 0xFFFF) / 65536.f; }

static StereoToyMap make_map() {
    StereoToyMap m;
    const int K = 6, P = 120;
    const float fx = 500.f, cx = 320.f, cy = 240.f;
    m.frames.resize(K); m.bl.assign(K, 0.12f);
    unsigned s = 12345u;
    for (int f = 0; f < K; f++) {
        m.frames[f].valid = true;
        m.frames[f].pose[3] = -0.25f * f + (f ? 0.02f * (unit(s) - 0.5f) : 0.f);   // x_cam = x_world - 0.25 f (+ start error on the free frames)
        m.frames[f].pose[7] = f ? 0.02f * (unit(s) - 0.5f) : 0.f;
        m.order.push_back(f);
    }
    m.points.resize(P);
    m.sf = {1.f, 1.2f, 1.44f};
    for (int p = 0; p < P; p++) {
        const float z = 4.f + 10.f * unit(s), x = (unit(s) - 0.3f) * z, y = (unit(s) - 0.5f) * 0.8f * z;
        m.points[p].xyz[0] = x + 0.03f * (unit(s) - 0.5f); m.points[p].xyz[1] = y + 0.03f * (unit(s) - 0.5f); m.points[p].xyz[2] = z + 0.03f * (unit(s) - 0.5f);
        const bool once = p % 10 == 9;   // seen by one frame, with depth: a stereo point
        m.points[p].stereo = once;
        for (int f = 0; f < K; f++) {
            if (once && f != p % K) continue;
            const float xc = x - 0.25f * f;
            const float u = xc / z * fx + cx + (unit(s) - 0.5f), v = y / z * fx + cy + (unit(s) - 0.5f);
            if (u < 0 || u >= 640 || v < 0 || v >= 480) continue;
            const float depth = (once || (p + f) % 3) ? z * (1.f + 0.004f * (unit(s) - 0.5f)) : 0.f;
            m.observe(p, f, u, v, (int)(lcg(s) % 3), depth);
        }
        if (once && m.points[p].frames.empty()) m.points[p].stereo = false;
    }
    return m;
}

template <class T> static void put(FILE* f, const T* p, size_t n) { std::fwrite(p, sizeof(T), n, f); }

int main(int argc, char** argv) {
    using namespace ucoslam_hip;
    StereoToyMap m = make_map();
    BAParamSet ps;
    ps.nIters = 5;
    StereoVectorSink flat;
    const FlatBAIndex fix = flatten_for_ba_stereo(m, ps, flat);
    const int K = (int)fix.frame_of.size(), P = (int)fix.point_of.size(), E = fix.n_obs;
    int n_st = 0, n_once = 0;
    for (float d : flat.depth) n_st += d > 0;
    for (uint32_t p : fix.point_of) n_once += m.points[p].frames.size() == 1;
    if (K != 6 || P < 100 || n_st < E / 3 || n_st == E || n_once < 5) { std::printf("toy map not as intended: K %d P %d E %d stereo %d once %d\n", K, P, E, n_st, n_once); return 2; }
    try {
        auto ctx = std::make_shared<Context>(0);
        GlobalOptimizer opt(ctx);
        opt.setParamsStereo(m, ps);
        if (uh_ba_form(opt.handle(), nullptr) != 0) { std::printf("a stereo window must run the launch chain\n"); return 3; }
        opt.optimize();
        opt.getResults(m);
        std::vector<float> poses(16 * (size_t)K), points(3 * (size_t)P);
        for (int k = 0; k < K; k++) for (int j = 0; j < 16; j++) poses[16 * k + j] = m.frames[fix.frame_of[k]].pose[j];
        for (int p = 0; p < P; p++) for (int j = 0; j < 3; j++) points[3 * p + j] = m.points[fix.point_of[p]].xyz[j];
        const int nbad = (int)opt.getBadAssociations().size();
        if (argc > 1) {
            FILE* f = std::fopen(argv[1], "wb");
            if (!f) { std::printf("cannot write %s\n", argv[1]); return 4; }
            const int32_t head[4] = {K, P, E, nbad};
            put(f, head, 4); put(f, flat.poses.data(), flat.poses.size()); put(f, flat.fixed.data(), flat.fixed.size()); put(f, flat.intr.data(), flat.intr.size());
            put(f, flat.points.data(), flat.points.size()); put(f, flat.obs.data(), flat.obs.size()); put(f, flat.depth.data(), flat.depth.size());
            put(f, flat.bl.data(), flat.bl.size()); put(f, poses.data(), poses.size()); put(f, points.data(), points.size());
            std::fclose(f);
        }
        std::printf("ba stereo ok: K %d P %d E %d stereo %d bad %d\n", K, P, E, n_st, nbad);
    } catch (const std::runtime_error& e) {
        std::printf("no device: %s\n", e.what());   // expected on the CPU-only build box: no fallback exists
    }
    return 0;
}
