// The loop-closure adaptor (include/ucoslam_hip/adaptors.hpp: flatten_posegraph, apply_posegraph_results, loopClosurePathOptimization)
// on a toy map.  Without arguments: the host-side checks (key order, weight look-up under CovisGraph::join's key, write-back, the throw
// above the cap, the throw for an unknown id, the library's argument checks on the flattened problem); prints "posegraph flatten ok".
// With a file name: also runs the whole call on the device and dumps the flattened problem and the corrected poses for the Python side
// to repeat (tests/test_posegraph_adaptor.py); prints "no device" and succeeds where there is none.
#include <array>
#include <cstdio>
#include <cstdlib>

#include "../../include/ucoslam_hip/adaptors.hpp"

using Pose = std::array<float, 16>;
using namespace ucoslam_hip;

#define REQUIRE(c) do { if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)

static Pose translation(float x, float y, float z) { return Pose{1, 0, 0, x, 0, 1, 0, y, 0, 0, 1, z, 0, 0, 0, 1}; }

int main(int argc, char** argv) {
    // keys deliberately not 0..n-1 and inserted out of order: a square walked 40 -> 7 -> 300 -> 12, drifted, closed by (12, 40)
    std::map<uint32_t, Pose> poses;
    poses[300] = translation(1.05f, 0, 1.02f);
    poses[7] = translation(1.01f, 0, 0.01f);
    poses[40] = translation(0, 0, 0);
    poses[12] = translation(0.08f, 0, 1.06f);
    poses[5] = translation(9, 9, 9);   // no edge
    const Pose expected = translation(0, 0, 1);
    const std::vector<std::pair<uint32_t, uint32_t>> edges = {{40, 7}, {300, 7}, {300, 12}, {12, 40}};
    std::map<uint64_t, float> weight;
    weight[covis_join(7, 300)] = 2.5f;      // found for the edge given as (300, 7)
    weight[covis_join(40, 12)] = 0.5f;
    weight[((uint64_t)300 << 32) | 7] = 99.f;   // the key with the larger id in the high word is NOT join's: never used

    const FlatPoseGraph f = flatten_posegraph(edges, 12, 40, expected, poses, true, weight);
    REQUIRE((f.id_of == std::vector<uint32_t>{5, 7, 12, 40, 300}));
    REQUIRE(f.poses.size() == 80 && f.poses[16 * 4 + 3] == 1.05f && f.poses[16 * 0 + 3] == 9.f);
    REQUIRE((f.edge_i == std::vector<int32_t>{3, 4, 4, 2}) && (f.edge_j == std::vector<int32_t>{1, 1, 2, 3}));
    REQUIRE((f.weight == std::vector<float>{1.f, 2.5f, 1.f, 0.5f}));
    REQUIRE(f.idx_new == 2 && f.idx_old == 3 && f.fix_scale == 1 && f.expected[11] == 1.f);
    const uh_posegraph_problem pr = f.view();
    REQUIRE(uh_posegraph_check_problem(&pr, nullptr) == UH_OK);

    // write-back: entry k of the result goes to key id_of[k]
    {
        std::map<uint32_t, Pose> copy = poses;
        std::vector<float> res(80);
        for (int k = 0; k < 80; k++) res[k] = (float)k;
        apply_posegraph_results(copy, f, res.data());
        REQUIRE(copy[5][0] == 0.f && copy[7][0] == 16.f && copy[12][15] == 47.f && copy[40][0] == 48.f && copy[300][15] == 79.f);
    }
    // an id that the map does not hold
    bool threw = false;
    try { flatten_posegraph(edges, 13, 40, expected, poses, true, weight); } catch (const std::runtime_error&) { threw = true; }
    REQUIRE(threw);
    // above the cap: std::length_error, nothing flattened; the library refuses the same size with UH_ECAPACITY
    {
        std::map<uint32_t, Pose> big;
        for (uint32_t k = 0; k <= (uint32_t)UH_POSEGRAPH_MAX_POSES; k++) big[k] = translation((float)k, 0, 0);
        threw = false;
        try { flatten_posegraph({{0, 1}}, 1, 0, expected, big, true, weight); } catch (const std::length_error&) { threw = true; }
        REQUIRE(threw);
        uh_posegraph_problem p2 = pr;
        p2.n_poses = UH_POSEGRAPH_MAX_POSES + 1;
        REQUIRE(uh_posegraph_check_problem(&p2, nullptr) == UH_ECAPACITY);
    }
    std::printf("posegraph flatten ok\n");
    if (argc < 2) return 0;

    std::unique_ptr<Context> ctx;
    try { ctx.reset(new Context(0)); } catch (const std::exception& e) { std::printf("no device: %s\n", e.what()); return 0; }
    std::map<uint32_t, Pose> out = poses;
    loopClosurePathOptimization(*ctx, edges, 12, 40, expected, out, true, weight);
    FILE* fp = std::fopen(argv[1], "wb");
    REQUIRE(fp);
    const int32_t head[4] = {(int32_t)f.id_of.size(), (int32_t)f.edge_i.size(), f.idx_new, f.idx_old};
    std::fwrite(head, 4, 4, fp);
    std::fwrite(f.poses.data(), 4, f.poses.size(), fp);
    std::fwrite(f.edge_i.data(), 4, f.edge_i.size(), fp);
    std::fwrite(f.edge_j.data(), 4, f.edge_j.size(), fp);
    std::fwrite(f.weight.data(), 4, f.weight.size(), fp);
    std::fwrite(f.expected, 4, 16, fp);
    for (uint32_t id : f.id_of) std::fwrite(out.at(id).data(), 4, 16, fp);
    std::fclose(fp);
    std::printf("posegraph adaptor ok\n");
    return 0;
}
