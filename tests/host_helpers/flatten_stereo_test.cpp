// flatten_for_ba_stereo on a toy map with depths (no GPU: the sink is plain vectors): same walk as flatten_for_ba, plus the depth per
// observation and the baseline per frame; a point with ONE observer is taken when it is a stereo point (globaloptimizer_g2o.cpp:142) and
// rejected when it is not; flatten_for_ba on the same map still refuses.  Also the layout of the new ABI structs.
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include "../../include/ucoslam_hip/flatten_ba.hpp"
#include "toy_map.hpp"

#define EXPECT(c) do { if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); std::exit(1); } } while (0)
using namespace ucoslam_hip;

struct StereoToyMap : ToyMap {
    std::vector<float> bl;
    float frame_baseline(uint32_t f) const { return bl[f]; }
};

int main() {
    static_assert(sizeof(uh_ba_stereo) == 32 && offsetof(uh_ba_stereo, frame_bl) == 8 && offsetof(uh_ba_stereo, huber_delta_3d) == 16, "uh_ba_stereo");
    static_assert(sizeof(uh_ba_staging_stereo) == 72 && offsetof(uh_ba_staging_stereo, obs_depth) == 40 && offsetof(uh_ba_staging_stereo, frame_bl) == 48 &&
                      offsetof(uh_ba_staging_stereo, cap_frames) == 56, "uh_ba_staging_stereo");
    static_assert(sizeof(uh_ba_obs) == 24 && sizeof(uh_ba_staging) == 56 && sizeof(uh_ba_problem) == 80 && sizeof(uh_ba_params) == 32, "existing structs keep their layout");

    // frames 0..3 (baselines 0.5 + 0.01 f), all used, frame 0 fixed (fixFirstFrame).
    //   P0: frames 0 (mono), 1 (depth 4), 2 (mono)     -> taken at f=0
    //   P1: frame 1 only, depth 6, stereo point        -> taken at f=1 (:142: one observer is enough for a stereo point)
    //   P2: frame 1 only, no depth, not stereo         -> rejected
    //   P3: frames 2 (depth 8), 3 (depth 9)            -> taken at f=2
    // points in taking order 0 1 3; edges in observer order: P0: 0 1 2 | P1: 1 | P3: 2 3  -> 6
    StereoToyMap m;
    m.frames.resize(4);
    m.bl.resize(4);
    for (int f = 0; f < 4; f++) { m.frames[f].valid = true; m.frames[f].pose[3] = 0.1f * f; m.bl[f] = 0.5f + 0.01f * f; }
    m.order = {0, 1, 2, 3};
    m.points.resize(4);
    for (int p = 0; p < 4; p++) { m.points[p].xyz[0] = (float)p; m.points[p].xyz[2] = 5.f; }
    m.sf = {1.f, 1.2f};
    m.observe(0, 0, 10, 11, 0);
    m.observe(0, 1, 12, 13, 1, 4.f);
    m.observe(1, 1, 20, 21, 0, 6.f);
    m.observe(2, 1, 30, 31, 0);
    m.observe(0, 2, 14, 15, 0);
    m.observe(3, 2, 40, 41, 1, 8.f);
    m.observe(3, 3, 42, 43, 0, 9.f);
    m.points[1].stereo = true;
    BAParamSet ps;
    StereoVectorSink sink;
    const FlatBAIndex ix = flatten_for_ba_stereo(m, ps, sink);
    EXPECT((ix.frame_of == std::vector<uint32_t>{0, 1, 2, 3}));
    EXPECT((sink.fixed == std::vector<uint8_t>{1, 0, 0, 0}));
    EXPECT((ix.point_of == std::vector<uint32_t>{0, 1, 3}));
    EXPECT(ix.n_obs == 6 && sink.obs.size() == 6 && sink.depth.size() == 6 && sink.bl.size() == 4);
    const int exp_pt[6] = {0, 0, 0, 1, 2, 2}, exp_fr[6] = {0, 1, 2, 1, 2, 3};
    const float exp_u[6] = {10, 12, 14, 20, 40, 42}, exp_depth[6] = {0, 4, 0, 6, 8, 9};
    const int exp_oct[6] = {0, 1, 0, 0, 1, 0};
    for (int e = 0; e < 6; e++) {
        EXPECT(sink.obs[e].point == exp_pt[e] && sink.obs[e].frame == exp_fr[e] && sink.obs[e].u == exp_u[e] && sink.obs[e].v == exp_u[e] + 1);
        EXPECT(sink.obs[e].inv_sigma == (double)(float)(1. / m.sf[exp_oct[e]]));
        EXPECT(sink.depth[e] == exp_depth[e]);
    }
    for (int f = 0; f < 4; f++) EXPECT(sink.bl[f] == 0.5f + 0.01f * f);
    // the same single observer without the stereo mark: rejected, its edge gone
    m.points[1].stereo = false;
    StereoVectorSink sink2;
    const FlatBAIndex ix2 = flatten_for_ba_stereo(m, ps, sink2);
    EXPECT((ix2.point_of == std::vector<uint32_t>{0, 3}) && ix2.n_obs == 5);
    // the monocular entry still refuses this map
    VectorSink mono;
    bool threw = false;
    try { flatten_for_ba(m, ps, mono); } catch (const std::runtime_error&) { threw = true; }
    EXPECT(threw);
    // ... and takes it, with the same records, once the depths are gone
    StereoToyMap m0 = m;
    for (auto& fr : m0.frames) for (auto& k : fr.kpts) k.depth = 0.f;
    const FlatBAIndex ixm = flatten_for_ba(m0, ps, mono);
    StereoVectorSink sink3;
    const FlatBAIndex ixs = flatten_for_ba_stereo(m0, ps, sink3);
    EXPECT(ixm.point_of == ixs.point_of && ixm.n_obs == ixs.n_obs && mono.obs.size() == sink3.obs.size());
    for (size_t e = 0; e < mono.obs.size(); e++) EXPECT(mono.obs[e].point == sink3.obs[e].point && mono.obs[e].frame == sink3.obs[e].frame && mono.obs[e].u == sink3.obs[e].u && sink3.depth[e] == 0.f);
    // apply_results is the monocular one: bad associations by (map point id, frame index)
    std::vector<float> poses = sink.poses, pts = sink.points;
    std::vector<uint8_t> bad(6, 0);
    bad[3] = 1;
    m.points[1].stereo = true;
    const auto ba = apply_results(m, ix, poses.data(), pts.data(), bad.data(), sink.obs.data());
    EXPECT(ba.size() == 1 && ba[0] == std::make_pair(1u, 1u));
    std::printf("flatten stereo ok\n");
    return 0;
}
