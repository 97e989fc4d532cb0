// ucoslam_hip::MapPointFuser (include/ucoslam_hip/adaptors.hpp) on the toy map of tests/host_helpers/toy_fuse_map.hpp:
//   fuse_adaptor map.bin state.bin [device]
// reads the map tests/fuse_map_cases.py dumped, runs searchInNeighbors — through uh_fuse_search_host, or on the GPU with `device` — and
// writes the returned list and the final map state, which the test compares with the oracle's.  Prints a summary of the final map.
#include <cstdio>
#include <cstring>
#include <memory>

#include "../../include/ucoslam_hip/adaptors.hpp"
#include "toy_fuse_map.hpp"

int main(int argc, char** argv) {
    if (argc < 3) { fprintf(stderr, "usage: %s map.bin state.bin [device]\n", argv[0]); return 2; }
    const bool device = argc > 3 && !strcmp(argv[3], "device");
    try {
        FILE* in = fopen(argv[1], "rb");
        if (!in) throw std::runtime_error("cannot open the map");
        ToyFuseMap map;
        uint32_t cur = 0;
        float maxDescDistance = 0;
        std::vector<uint32_t> kf_order, mp_order;
        toy_fuse_map_read(in, map, cur, maxDescDistance, kf_order, mp_order);
        fclose(in);
        std::unique_ptr<ucoslam_hip::Context> ctx;
        std::unique_ptr<ucoslam_hip::MapPointFuser> fuser;
        if (device) { ctx.reset(new ucoslam_hip::Context(0)); fuser.reset(new ucoslam_hip::MapPointFuser(*ctx)); }
        else fuser.reset(new ucoslam_hip::MapPointFuser());
        const std::vector<uint32_t> removed = fuser->searchInNeighbors(map, map.keyframes[cur], maxDescDistance);
        FILE* out = fopen(argv[2], "wb");
        if (!out) throw std::runtime_error("cannot open the output");
        toy_fuse_map_write(out, map, removed, kf_order, mp_order);
        fclose(out);
        size_t bad = 0, obs = 0;
        for (const auto& kv : map.map_points) { bad += kv.second.bad; obs += kv.second.frames.size(); }
        printf("fuse adaptor ok (%s): %zu removed, %zu of %zu points bad, %zu observations, %zu device frames cached\n", device ? "device" : "host", removed.size(), bad,
               map.map_points.size(), obs, fuser->cachedFrames());
        {   // a second call on the fused map (not written out): its first half now also carries the inherited points; the cached frames are reused
            const size_t cached = fuser->cachedFrames();
            const std::vector<uint32_t> again = fuser->searchInNeighbors(map, map.keyframes[cur], maxDescDistance);
            size_t obs2 = 0;
            for (const auto& kv : map.map_points) obs2 += kv.second.frames.size();
            printf("second call: %zu removed, %zu observations, %zu device frames cached (%zu before)\n", again.size(), obs2, fuser->cachedFrames(), cached);
        }
    } catch (const std::exception& e) {
        printf("fuse adaptor failed: %s\n", e.what());
        return 1;
    }
    return 0;
}
