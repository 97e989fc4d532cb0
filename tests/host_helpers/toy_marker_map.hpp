// toy_map.hpp's map with markers: what flatten_for_ba_markers needs on top of the MapView members there, shaped like the reference's
// containers (Frame::markers a vector of observations, Map::map_markers a std::map by id, Marker::frames a std::set).
#pragma once
#include <array>
#include <set>
#include "toy_map.hpp"

struct ToyMarkerObs { uint32_t id; std::array<float, 8> und_corners; };
struct ToyMarker {
    bool valid = true;
    float pose[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    float size = 0.2f;
    std::set<uint32_t> frames;            // Marker::frames
};
struct ToyMarkerMap : ToyMap {
    std::vector<std::vector<ToyMarkerObs>> frame_markers;   // Frame::markers, per frame index
    std::map<uint32_t, ToyMarker> markers;                  // Map::map_markers
    float frame_baseline(uint32_t) const { return 0.54f; }  // Frame::imageParams.bl
    size_t frame_n_markers(uint32_t f) const { return f < frame_markers.size() ? frame_markers[f].size() : 0; }
    uint32_t frame_marker_id(uint32_t f, size_t i) const { return frame_markers[f][i].id; }
    const float* frame_marker_corners(uint32_t f, uint32_t id) const {
        for (const auto& o : frame_markers[f]) if (o.id == id) return o.und_corners.data();
        return nullptr;
    }
    template <class F> void for_each_marker(F fn) const { for (const auto& m : markers) fn(m.first); }
    bool marker_valid(uint32_t id) const { return markers.at(id).valid; }
    const float* marker_pose_g2m(uint32_t id) const { return markers.at(id).pose; }
    float marker_size(uint32_t id) const { return markers.at(id).size; }
    template <class F> void for_each_marker_frame(uint32_t id, F fn) const { for (uint32_t f : markers.at(id).frames) fn(f); }
    void set_marker_pose_g2m(uint32_t id, const float* m) { for (int i = 0; i < 16; i++) markers[id].pose[i] = m[i]; }
    // helper: frame f sees marker id with corners c0 + 0..7
    void see(uint32_t f, uint32_t id, float c0) {
        if (frame_markers.size() < frames.size()) frame_markers.resize(frames.size());
        ToyMarkerObs o; o.id = id;
        for (int i = 0; i < 8; i++) o.und_corners[i] = c0 + (float)i;
        frame_markers[f].push_back(o);
        markers[id].frames.insert(f);
    }
};
