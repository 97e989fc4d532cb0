// flatten_for_ba_markers on a toy map (no GPU: the sinks are plain vectors).  The structural expectations (join rule, edge order,
// refusals, the marker-less identity) are checked here; the flattened problem is also printed, one record per line, so that
// tests/test_flatten_markers.py can check the weights against its own restatement of globaloptimizer_g2o.cpp:281-299.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include "../../include/ucoslam_hip/flatten_ba.hpp"
#include "toy_marker_map.hpp"

#define EXPECT(c) do { if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); std::exit(1); } } while (0)
using namespace ucoslam_hip;

// frames 0..4 (capacity 6, index 5 a hole).  Points 0..29 are seen by frames 0 and 1 (octaves 0..2, every fifth observation of frame 1
// with depth), points 30..34 by frames 1 and 2.  Frame 3 sees no point and is not in used_frames; frame 4 is never reached.
// Markers: 7 (valid) seen by frames 0, 1, 3; 3 (valid) by 1, 2; 5 (NO valid pose) by 1; 9 (valid) by 4 only.
static ToyMarkerMap make_map() {
    ToyMarkerMap m;
    m.frames.resize(6);
    for (int f = 0; f < 5; f++) { m.frames[f].valid = true; m.frames[f].pose[3] = 0.1f * f; m.frames[f].intr[0] = 500.f + f; }
    m.order = {0, 1, 2, 3, 4};
    m.points.resize(35);
    m.sf = {1.f, 1.2f, 1.44f};
    for (int p = 0; p < 30; p++) {
        m.observe(p, 0, 10.f + p, 11.f + p, p % 3);
        m.observe(p, 1, 12.f + p, 13.f + p, (p + 1) % 3, p % 5 == 0 ? 3.5f : 0.f);
    }
    for (int p = 30; p < 35; p++) { m.observe(p, 1, 40.f + p, 41.f + p, 0); m.observe(p, 2, 42.f + p, 43.f + p, 1); }
    m.see(0, 7, 100.f);
    m.see(1, 3, 200.f); m.see(1, 5, 300.f); m.see(1, 7, 110.f);
    m.see(2, 3, 210.f);
    m.see(3, 7, 120.f);
    m.see(4, 9, 400.f);
    m.markers[5].valid = false;
    m.markers[7].size = 0.25f; m.markers[7].pose[7] = 1.5f;
    m.markers[3].size = 0.15f; m.markers[3].pose[11] = 2.5f;
    return m;
}

int main() {
    // ---- case 1: used = {0, 1, 2}, frame 0 fixed (front).  f=0 takes marker 7: frame 3 joins as FIXED_WITHOUTPOINTS.  f=1 takes marker 3
    //   (frames 1, 2: used), skips 5 (no valid pose) and 7 (taken).  Frame 3 contributes nothing; marker 9 is never reached.
    //   markers in ascending id: 3, 7; edges: 3-1, 3-2, 7-0, 7-1, 7-3.
    {
        ToyMarkerMap m = make_map();
        BAParamSet ps;
        ps.used_frames = {0, 1, 2};
        StereoVectorSink sink;
        MarkerVectorSink ms;
        FlatBAMarkerIndex mix;
        const FlatBAIndex ix = flatten_for_ba_markers(m, ps, sink, ms, mix);
        EXPECT((ix.frame_of == std::vector<uint32_t>{0, 1, 2, 3}));
        EXPECT((ix.frame_fixed == std::vector<uint8_t>{1, 0, 0, 2}));
        EXPECT((mix.marker_of == std::vector<uint32_t>{3, 7}) && mix.n_edges == 5);
        EXPECT((ms.edge_marker == std::vector<int32_t>{0, 0, 1, 1, 1}));
        EXPECT((ms.edge_frame == std::vector<int32_t>{1, 2, 0, 1, 3}));
        EXPECT(ms.size[0] == 0.15f && ms.size[1] == 0.25f && ms.pose_g2m[11] == 2.5f && ms.pose_g2m[16 + 7] == 1.5f);
        const float c0[5] = {200.f, 210.f, 100.f, 110.f, 120.f};
        for (int e = 0; e < 5; e++) for (int j = 0; j < 8; j++) EXPECT(ms.und_corners[8 * e + j] == c0[e] + (float)j);
        EXPECT(ix.n_obs == 70 && ix.point_of.size() == 35);
        const uh_ba_markers v = ms.view();
        EXPECT(v.n_markers == 2 && v.n_edges == 5 && v.edge_weight == ms.edge_weight.data() && v.und_corners == ms.und_corners.data());
        for (int k = 0; k < 4; k++) std::printf("frame %d n_markers %zu\n", k, m.frame_n_markers(ix.frame_of[k]));
        for (int e = 0; e < ix.n_obs; e++) std::printf("obs %d %.17g %.9g\n", sink.obs[e].frame, sink.obs[e].inv_sigma, (double)sink.depth[e]);
        for (int e = 0; e < 5; e++) std::printf("edge %d %d %.17g\n", ms.edge_marker[e], ms.edge_frame[e], ms.edge_weight[e]);
        // getResults' marker part
        std::vector<float> mp = ms.pose_g2m;
        for (auto& x : mp) x += 1.f;
        apply_marker_results(m, mix, mp.data());
        EXPECT(m.markers[3].pose[11] == 3.5f && m.markers[7].pose[7] == 2.5f && m.markers[9].pose[0] == 1.f && m.markers[5].pose[0] == 1.f);
        // other weights in the parameter set are taken over
        ps.markersOptWeight = 0.25f; ps.minMarkersForMaxWeight = 2;
        ToyMarkerMap m2 = make_map();
        flatten_for_ba_markers(m2, ps, sink, ms, mix);
        for (int e = 0; e < 5; e++) std::printf("edge2 %d %d %.17g\n", ms.edge_marker[e], ms.edge_frame[e], ms.edge_weight[e]);
    }
    // ---- case 2: every keyframe.  Frame 4 is used, so marker 9 is taken too; nobody joins without points
    {
        ToyMarkerMap m = make_map();
        BAParamSet ps;
        StereoVectorSink sink;
        MarkerVectorSink ms;
        FlatBAMarkerIndex mix;
        const FlatBAIndex ix = flatten_for_ba_markers(m, ps, sink, ms, mix);
        EXPECT((ix.frame_fixed == std::vector<uint8_t>{1, 0, 0, 0, 0}));
        EXPECT((mix.marker_of == std::vector<uint32_t>{3, 7, 9}) && mix.n_edges == 6);
        EXPECT(ms.edge_marker[5] == 2 && ms.edge_frame[5] == 4);
    }
    // ---- case 3: the planar constraint is refused with two valid markers in the map, not with one
    {
        ToyMarkerMap m = make_map();
        BAParamSet ps;
        ps.InPlaneMarkers = true;
        StereoVectorSink sink;
        MarkerVectorSink ms;
        FlatBAMarkerIndex mix;
        bool threw = false;
        try { flatten_for_ba_markers(m, ps, sink, ms, mix); } catch (const std::runtime_error&) { threw = true; }
        EXPECT(threw);
        m.markers[3].valid = false; m.markers[9].valid = false;   // only marker 7 has a pose
        flatten_for_ba_markers(m, ps, sink, ms, mix);
        EXPECT((mix.marker_of == std::vector<uint32_t>{7}));
        // a marker seen by a frame that is not in the map
        ToyMarkerMap m3 = make_map();
        m3.markers[7].frames.insert(5);
        ps.InPlaneMarkers = false;
        threw = false;
        try { flatten_for_ba_markers(m3, ps, sink, ms, mix); } catch (const std::runtime_error&) { threw = true; }
        EXPECT(threw);
    }
    // ---- case 4: a map without markers gives what flatten_for_ba gives (the monocular toy map of flatten_test.cpp's shape)
    {
        ToyMarkerMap m;
        m.frames.resize(4);
        for (int f = 0; f < 4; f++) { m.frames[f].valid = true; m.frames[f].pose[3] = 0.1f * f; }
        m.order = {0, 1, 2, 3};
        m.points.resize(6);
        m.sf = {1.f, 1.2f};
        for (int p = 0; p < 6; p++) { m.observe(p, p % 4, 10.f + p, 20.f + p, p % 2); m.observe(p, (p + 1) % 4, 30.f + p, 40.f + p, (p + 1) % 2); }
        m.frame_markers.resize(4);
        BAParamSet ps;
        VectorSink plain;
        const FlatBAIndex a = flatten_for_ba(m, ps, plain);
        StereoVectorSink sink;
        MarkerVectorSink ms;
        FlatBAMarkerIndex mix;
        const FlatBAIndex b = flatten_for_ba_markers(m, ps, sink, ms, mix);
        EXPECT(a.frame_of == b.frame_of && a.frame_fixed == b.frame_fixed && a.point_of == b.point_of && a.n_obs == b.n_obs);
        EXPECT(plain.poses == sink.poses && plain.intr == sink.intr && plain.points == sink.points && plain.fixed == sink.fixed);
        for (int e = 0; e < a.n_obs; e++)
            EXPECT(plain.obs[e].point == sink.obs[e].point && plain.obs[e].frame == sink.obs[e].frame && plain.obs[e].u == sink.obs[e].u &&
                   plain.obs[e].v == sink.obs[e].v && plain.obs[e].inv_sigma == sink.obs[e].inv_sigma && sink.depth[e] == 0.f);
        EXPECT(mix.marker_of.empty() && mix.n_edges == 0 && ms.view().n_edges == 0);
    }
    // ---- the marker-less entries still refuse a map with markers
    {
        struct WithFlag : ToyMarkerMap { bool frame_has_valid_markers(uint32_t f) const { return frame_n_markers(f) > 0; } };
        WithFlag m;
        static_cast<ToyMarkerMap&>(m) = make_map();
        BAParamSet ps;
        StereoVectorSink sink;
        bool threw = false;
        try { flatten_for_ba_stereo(m, ps, sink); } catch (const std::runtime_error&) { threw = true; }
        EXPECT(threw);
    }
    std::printf("flatten markers ok\n");
    return 0;
}
