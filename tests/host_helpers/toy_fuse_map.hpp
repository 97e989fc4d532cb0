// A map shaped like ucoslam::Map as far as ucoslam_hip::MapPointFuser (include/ucoslam_hip/adaptors.hpp) reads and changes it:
// TheKpGraph.getNeighbors, keyframes, map_points, fuseMapPoints, addMapPointObservation, getMapPointsInFrames — with removePoint,
// updatePointInfo and updatePointNormalAndDistances behind them, restated from the behaviour of src/map.cpp:114-130, 165-185, 264-276,
// 849-930 and map.h:203-233 (float sums in observation order, cv::norm and the 1/sum factor in double, the first strict minimum of the
// descriptor distance sums).  The covisibility graph keeps its neighbour lists only; edge weights are not modelled.
#pragma once
#include <algorithm>
#include <array>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <map>
#include <set>
#include <stdexcept>
#include <string>
#include <vector>

#include "toy_frames.hpp"

struct ToyPoint3f { float x, y, z; };
struct ToyPointI { int x, y; };
constexpr uint32_t kToyNoId = std::numeric_limits<uint32_t>::max();

struct ToyFuseFrame {
    uint32_t idx = 0;
    bool bad = false;
    std::array<float, 16> pose_f2g{};
    std::vector<ToyKeyPoint> und_kpts;
    std::vector<uint8_t> desc;            // n x 32
    std::vector<uint32_t> ids;
    std::vector<float> scaleFactors;
    ToyImageParams imageParams{};
    ToyPointI minXY{0, 0}, maxXY{std::numeric_limits<int>::max(), std::numeric_limits<int>::max()};
    bool isBad() const { return bad; }
    std::vector<uint32_t> getMapPoints() const {
        std::vector<uint32_t> r;
        for (uint32_t id : ids) if (id != kToyNoId) r.push_back(id);
        return r;
    }
    ToyPoint3f getCameraCenter() const {
        const float* p = pose_f2g.data();
        return {-(p[3] * p[0] + p[7] * p[4] + p[11] * p[8]), -(p[3] * p[1] + p[7] * p[5] + p[11] * p[9]), -(p[3] * p[2] + p[7] * p[6] + p[11] * p[10])};
    }
};

struct ToyFuseMapPoint {
    uint32_t id = kToyNoId;
    bool bad = false;
    ToyPoint3f pos3d{}, normal{};
    float mind = 0, maxd = 0;
    std::array<uint8_t, 32> desc{};
    std::map<uint32_t, uint32_t> frames;   // frame idx -> keypoint (SafeMap is a std::map: ascending)
    bool isBad() const { return bad; }
    void setBad(bool v) { bad = v; }
    ToyPoint3f getCoordinates() const { return pos3d; }
    ToyPoint3f getNormal() const { return normal; }
    float getMinDistanceInvariance() const { return mind; }
    float getMaxDistanceInvariance() const { return maxd; }
};

template <class V> struct ToySafeMap : std::map<uint32_t, V> {
    bool is(uint32_t k) const { return this->count(k) != 0; }
    V& operator[](uint32_t k) {
        auto it = this->find(k);
        if (it == this->end()) throw std::runtime_error("toy map: no element " + std::to_string(k));
        return it->second;
    }
};

struct ToyFuseMap {
    struct Graph {
        std::map<uint32_t, std::vector<uint32_t>> nb;
        const std::vector<uint32_t>& getNeighbors(uint32_t idx) { return nb[idx]; }
    } TheKpGraph;
    ToySafeMap<ToyFuseFrame> keyframes;
    ToySafeMap<ToyFuseMapPoint> map_points;

    static double norm3(float x, float y, float z) { return std::sqrt((double)x * x + (double)y * y + (double)z * z); }
    static int hamming(const uint8_t* a, const uint8_t* b) {
        uint64_t x[4], y[4];
        std::memcpy(x, a, 32); std::memcpy(y, b, 32);
        return __builtin_popcountll(x[0] ^ y[0]) + __builtin_popcountll(x[1] ^ y[1]) + __builtin_popcountll(x[2] ^ y[2]) + __builtin_popcountll(x[3] ^ y[3]);
    }

    void updatePointInfo(uint32_t pid) {
        ToyFuseMapPoint& mp = map_points[pid];
        float ax = 0, ay = 0, az = 0;
        double normSum = 0;
        int bestOct = std::numeric_limits<int>::max();
        uint32_t bestFrame = kToyNoId, bestKp = kToyNoId;
        for (const auto& f : mp.frames) {
            const ToyFuseFrame& fr = keyframes[f.first];
            const ToyPoint3f c = fr.getCameraCenter();
            const float nx = c.x - mp.pos3d.x, ny = c.y - mp.pos3d.y, nz = c.z - mp.pos3d.z;
            ax += nx; ay += ny; az += nz;
            normSum += norm3(nx, ny, nz);
            if (bestOct > fr.und_kpts[f.second].octave) { bestOct = fr.und_kpts[f.second].octave; bestFrame = f.first; bestKp = f.second; }
        }
        const double s = 1. / normSum;
        mp.normal = {(float)(ax * s), (float)(ay * s), (float)(az * s)};
        {
            const ToyFuseFrame& bf = keyframes[bestFrame];
            const ToyPoint3f c = bf.getCameraCenter();
            const float dist = (float)norm3(mp.pos3d.x - c.x, mp.pos3d.y - c.y, mp.pos3d.z - c.z);
            mp.maxd = dist * bf.scaleFactors[bf.und_kpts[bestKp].octave];
            mp.mind = mp.maxd / bf.scaleFactors.back();
        }
        std::vector<std::pair<uint32_t, uint32_t>> obs(mp.frames.begin(), mp.frames.end());
        const size_t k = obs.size();
        std::vector<float> dd(k * k, 0.f);
        for (size_t i = 0; i < k; i++)
            for (size_t j = i + 1; j < k; j++)
                dd[i * k + j] = dd[j * k + i] = (float)hamming(&keyframes[obs[i].first].desc[32 * (size_t)obs[i].second], &keyframes[obs[j].first].desc[32 * (size_t)obs[j].second]);
        int best = -1;
        float bestSum = std::numeric_limits<float>::max();
        for (size_t r = 0; r < k; r++) {
            float sum = 0;
            for (size_t c = 0; c < k; c++) sum += dd[r * k + c];
            if (sum < bestSum) { best = (int)r; bestSum = sum; }
        }
        std::memcpy(mp.desc.data(), &keyframes[obs[best].first].desc[32 * (size_t)obs[best].second], 32);
    }
    void addMapPointObservation(uint32_t mapId, uint32_t frameId, uint32_t kp) {
        keyframes[frameId].ids[kp] = mapId;
        map_points[mapId].frames[frameId] = kp;
        updatePointInfo(mapId);
    }
    void removePoint(uint32_t pid, bool full) {
        ToyFuseMapPoint& mp = map_points[pid];
        mp.setBad(true);
        for (const auto& f : mp.frames)
            if (keyframes[f.first].ids[f.second] == pid) keyframes[f.first].ids[f.second] = kToyNoId;
        if (full) map_points.erase(pid);
    }
    void fuseMapPoints(uint32_t mp1, uint32_t mp2, bool fullRemovePoint2) {
        const std::map<uint32_t, uint32_t> obs2 = map_points[mp2].frames;
        removePoint(mp2, fullRemovePoint2);
        for (const auto& o : obs2)
            if (!map_points[mp1].frames.count(o.first)) addMapPointObservation(mp1, o.first, o.second);
    }
    template <class It> std::vector<uint32_t> getMapPointsInFrames(It b, It e) {
        std::set<uint32_t> used;
        for (It f = b; f != e; ++f) {
            if (!keyframes.is(*f) || keyframes[*f].isBad()) continue;
            for (uint32_t id : keyframes[*f].ids) if (id != kToyNoId) used.insert(id);
        }
        std::vector<uint32_t> out;
        for (uint32_t id : used) if (map_points.is(id) && !map_points[id].isBad()) out.push_back(id);
        return out;
    }
};

// the dump of tests/fuse_map_cases.py: dump_map
template <class T> inline std::vector<T> toy_take(FILE* f, size_t n) {
    std::vector<T> v(n);
    if (n && fread(v.data(), sizeof(T), n, f) != n) throw std::runtime_error("toy map: short read");
    return v;
}
inline void toy_fuse_map_read(FILE* in, ToyFuseMap& m, uint32_t& cur, float& maxDescDistance, std::vector<uint32_t>& kf_order, std::vector<uint32_t>& mp_order) {
    cur = (uint32_t)toy_take<int32_t>(in, 1)[0];
    maxDescDistance = toy_take<float>(in, 1)[0];
    const int nkf = toy_take<int32_t>(in, 1)[0];
    for (int k = 0; k < nkf; k++) {
        const auto hd = toy_take<int32_t>(in, 4);
        ToyFuseFrame fr;
        fr.idx = (uint32_t)hd[0]; fr.bad = hd[1] != 0;
        const int n = hd[2], levels = hd[3];
        const auto pose = toy_take<float>(in, 16);
        std::copy(pose.begin(), pose.end(), fr.pose_f2g.begin());
        const auto cam = toy_take<float>(in, 4);
        fr.imageParams = ToyImageParams{cam[0], cam[1], cam[2], cam[3]};
        const auto bounds = toy_take<int32_t>(in, 4);
        fr.minXY = {bounds[0], bounds[1]}; fr.maxXY = {bounds[2], bounds[3]};
        fr.scaleFactors = toy_take<float>(in, levels);
        const auto xy = toy_take<float>(in, 2 * (size_t)n);
        const auto oct = toy_take<int32_t>(in, n);
        fr.und_kpts.resize(n);
        for (int i = 0; i < n; i++) fr.und_kpts[i] = ToyKeyPoint{{xy[2 * i], xy[2 * i + 1]}, oct[i]};
        fr.desc = toy_take<uint8_t>(in, 32 * (size_t)n);
        fr.ids = toy_take<uint32_t>(in, n);
        kf_order.push_back(fr.idx);
        m.keyframes.emplace(fr.idx, std::move(fr));
    }
    const int nnb = toy_take<int32_t>(in, 1)[0];
    m.TheKpGraph.nb[cur] = toy_take<uint32_t>(in, nnb);
    const int nmp = toy_take<int32_t>(in, 1)[0];
    for (int k = 0; k < nmp; k++) {
        ToyFuseMapPoint mp;
        mp.id = toy_take<uint32_t>(in, 1)[0];
        mp.bad = toy_take<int32_t>(in, 1)[0] != 0;
        const auto v = toy_take<float>(in, 8);
        mp.pos3d = {v[0], v[1], v[2]}; mp.normal = {v[3], v[4], v[5]}; mp.mind = v[6]; mp.maxd = v[7];
        const auto d = toy_take<uint8_t>(in, 32);
        std::copy(d.begin(), d.end(), mp.desc.begin());
        const int nobs = toy_take<int32_t>(in, 1)[0];
        const auto obs = toy_take<uint32_t>(in, 2 * (size_t)nobs);
        for (int i = 0; i < nobs; i++) mp.frames[obs[2 * i]] = obs[2 * i + 1];
        mp_order.push_back(mp.id);
        m.map_points.emplace(mp.id, std::move(mp));
    }
}
// the final state in the form tests/fuse_map_cases.py: load_state reads
inline void toy_fuse_map_write(FILE* out, ToyFuseMap& m, const std::vector<uint32_t>& removed, const std::vector<uint32_t>& kf_order, const std::vector<uint32_t>& mp_order) {
    const int32_t nr = (int32_t)removed.size();
    fwrite(&nr, 4, 1, out);
    if (nr) fwrite(removed.data(), 4, nr, out);
    for (uint32_t k : kf_order) { const auto& ids = m.keyframes[k].ids; if (!ids.empty()) fwrite(ids.data(), 4, ids.size(), out); }
    for (uint32_t id : mp_order) {
        const ToyFuseMapPoint& mp = m.map_points[id];
        const int32_t bad = mp.bad ? 1 : 0, nobs = (int32_t)mp.frames.size();
        const float v[5] = {mp.normal.x, mp.normal.y, mp.normal.z, mp.mind, mp.maxd};
        fwrite(&bad, 4, 1, out); fwrite(v, 4, 5, out); fwrite(mp.desc.data(), 1, 32, out); fwrite(&nobs, 4, 1, out);
        for (const auto& f : mp.frames) { const uint32_t p[2] = {f.first, f.second}; fwrite(p, 4, 2, out); }
    }
}
