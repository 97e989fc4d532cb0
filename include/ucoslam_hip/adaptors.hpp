// C++ host adaptors over the C ABI (ucoslam_hip.h): the reference's plugin surfaces for the tracking hot path.
//
//   ucoslam_hip::ORBextractor     ~ ucoslam::Feature2DSerializable / ORBextractor   (feature2dserializable.h:30-95)
//   ucoslam_hip::Index            ~ xflann::Index (Linear)                          (3rdparty/xflann/xflann/index.h:41-135)
//   ucoslam_hip::Vocabulary/fBow  ~ fbow::Vocabulary / fbow::fBow                   (3rdparty/fbow/fbow/fbow.h:54-116)
//   ucoslam_hip::GlobalOptimizer  ~ ucoslam::GlobalOptimizer                        (src/optimization/globaloptimizer.h:28-68)
//
// Same method names, argument meaning and error behaviour (std::runtime_error where the reference throws, `false` where
// xflann returns false).  This header needs no OpenCV: images/descriptors are plain pointers, keypoints are uh_keypoint
// (layout of cv::KeyPoint), matches are uh_dmatch (layout of cv::DMatch).  The classes that literally derive from the
// reference's bases (so that System/MapManager can hold them) are NOT in this header: they need the reference's headers and
// OpenCV, neither of which exists where this repository is built and tested, so they have never been compiled — INTEGRATION.md
// sections 1 and 4 list them as the binding a maintainer adds inside the reference tree, on top of the classes below.
#pragma once
#include <algorithm>
#include <array>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <map>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "../ucoslam_hip.h"
#include "flatten_ba.hpp"

namespace ucoslam_hip {

inline void check(int rc) { if (rc < 0) throw std::runtime_error(uh_last_error()); }

class Context {
   public:
    explicit Context(int device = 0, void* hip_stream = nullptr) { check(uh_ctx_create(device, hip_stream, &c_)); }
    ~Context() { uh_ctx_destroy(c_); }
    Context(const Context&) = delete;
    Context& operator=(const Context&) = delete;
    uh_ctx* get() const { return c_; }
    void synchronize() { check(uh_ctx_synchronize(c_)); }
   private:
    uh_ctx* c_ = nullptr;
};

// ------------------------------------------------------------------------------------------------ extractor
struct FeatParams {   // Feature2DSerializable::FeatParams (same defaults)
    int nthreads = -1, maxFeatures = 4000, nOctaveLevels = 8;
    float scaleFactor = 1.2f, sensitivity = 0;
    FeatParams() {}
    FeatParams(int MaxFeatures, int NOctaveLevels, float ScaleFactor, int NThreads)
        : nthreads(NThreads), maxFeatures(MaxFeatures), nOctaveLevels(NOctaveLevels), scaleFactor(ScaleFactor) {}
    bool operator==(const FeatParams& fp) const {
        return nthreads == fp.nthreads && maxFeatures == fp.maxFeatures && nOctaveLevels == fp.nOctaveLevels && scaleFactor == fp.scaleFactor;
    }
};

class ORBextractor {
   public:
    explicit ORBextractor(std::shared_ptr<Context> ctx) : ctx_(std::move(ctx)) { check(uh_orb_create(ctx_->get(), &o_)); }
    ~ORBextractor() { uh_orb_destroy(o_); }
    static std::shared_ptr<ORBextractor> create(std::shared_ptr<Context> ctx) { return std::make_shared<ORBextractor>(std::move(ctx)); }

    // detectAndCompute(image, mask, keypoints, descriptors, params); mask is ignored like the reference (ORBextractor.cpp:1253)
    void detectAndCompute(const uint8_t* image, int width, int height, size_t stride, std::vector<uh_keypoint>& keypoints,
                          std::vector<uint8_t>& descriptors, const FeatParams& params) {
        uh_feat_params fp{params.nthreads, params.maxFeatures, params.nOctaveLevels, params.scaleFactor, params.sensitivity};
        check(uh_orb_set_params(o_, &fp));
        const int cap = std::max(uh_orb_max_keypoints(o_), 1);
        keypoints.resize(cap);
        descriptors.resize((size_t)cap * 32);
        int n = 0;
        check(uh_orb_extract(o_, image, width, height, stride, keypoints.data(), descriptors.data(), cap, &n));
        keypoints.resize(n);
        descriptors.resize((size_t)n * 32);
    }
    FeatParams getParams() const {
        uh_feat_params fp;
        check(uh_orb_get_params(o_, &fp));
        FeatParams r(fp.maxFeatures, fp.nOctaveLevels, fp.scaleFactor, fp.nthreads);
        r.sensitivity = fp.sensitivity;
        return r;
    }
    float getMinDescDistance() const { return 50; }          // ORBextractor.h:105
    void setSensitivity(float v) { check(uh_orb_set_sensitivity(o_, v)); }
    void doGaussianBlur(bool b) { check(uh_orb_set_blur(o_, b)); }
    // multi-GPU extraction of one frame: this instance extracts pyramid levels [first, end) (end < 0: all)
    void setLevelRange(int first, int end) { check(uh_orb_set_level_range(o_, first, end)); }
    uh_orb* handle() const { return o_; }
   private:
    std::shared_ptr<Context> ctx_;
    uh_orb* o_ = nullptr;
};

// ------------------------------------------------------------------------------------------------ kNN index
struct Matrix {   // xflann::Matrix as a non-owning view (types.h:275-400): rows x cols elements, row stride in bytes
    void* data = nullptr; int rows = 0, cols = 0; size_t stride = 0; int elem_size = 1;
    Matrix() {}
    Matrix(void* d, int r, int c, int esize, size_t s = 0) : data(d), rows(r), cols(c), stride(s ? s : (size_t)c * esize), elem_size(esize) {}
};

class Index {
   public:
    explicit Index(std::shared_ptr<Context> ctx) : ctx_(std::move(ctx)) { check(uh_knn_create(ctx_->get(), &k_)); }
    ~Index() { uh_knn_destroy(k_); }
    // build(features, LinearParams): uint8 rows of 32 bytes
    void build(const Matrix& features) {
        if (features.elem_size != 1) throw std::runtime_error("Index::build: features must be XFLANN_8U");
        check(uh_knn_build(k_, static_cast<const uint8_t*>(features.data), features.rows, features.stride, features.cols));
    }
    // search(features, nn, indices, distances, KnnSearchParams(maxChecks, sorted)): outputs pre-allocated nq x nn int32
    bool search(const Matrix& q, int nn, Matrix indices, Matrix distances, bool sorted = false, int maxDist = -1) {
        if (q.rows != indices.rows || distances.rows != q.rows)
            throw std::runtime_error("knnsearch indices and distances must be already allocated with the same size as the number of features");
        if (distances.cols != nn || indices.cols != nn) throw std::runtime_error("knnsearch indices and distances number of cols must == nn");
        if (indices.elem_size != 4 || distances.elem_size != 4) throw std::runtime_error("Index::search undefined search distance type");
        const int rc = uh_knn_search(k_, static_cast<const uint8_t*>(q.data), q.rows, q.stride, nn, static_cast<int32_t*>(indices.data),
                                     static_cast<int32_t*>(distances.data), sorted, maxDist);
        if (rc == UH_ENOTBUILT) return false;   // index.cpp:82-85
        check(rc);
        return true;
    }
    // build(features, HKMeansParams(k, maxIters)) — the index FrameMatcher_Flann uses (framematcher.cpp:213); rows contiguous
    void buildKMeans(const Matrix& features, int k = 32, int maxIters = 0) {
        if (features.elem_size != 1 || features.cols != 32 || (features.rows > 1 && features.stride != 32))
            throw std::runtime_error("Index::buildKMeans: features must be contiguous XFLANN_8U rows of 32 bytes");
        check(uh_knn_build_kmeans(k_, static_cast<const uint8_t*>(features.data), features.rows, k, maxIters));
        kmeans_ = features.rows > 0;
    }
    // search(features, nn, indices, distances, KnnSearchParams(maxChecks, sorted)) on the k-means form
    bool searchKMeans(const Matrix& q, int nn, Matrix indices, Matrix distances, int maxChecks = 1, bool sorted = false) {
        if (q.rows != indices.rows || distances.rows != q.rows)
            throw std::runtime_error("KMeanIndex::knnsearch indices and distances must be already allocated with the same size as the number of features");
        if (distances.cols != nn || indices.cols != nn) throw std::runtime_error("KMeanIndex::knnsearch indices and distances number of cols must == nn");
        if (q.rows > 1 && q.stride != 32) throw std::runtime_error("Index::searchKMeans: query rows must be contiguous");
        const int rc = uh_knn_search_kmeans(k_, static_cast<const uint8_t*>(q.data), q.rows, nn, maxChecks, sorted, static_cast<int32_t*>(indices.data),
                                            static_cast<int32_t*>(distances.data));
        if (rc == UH_ENOTBUILT) return false;   // index.cpp:82-85
        check(rc);
        return true;
    }
    int size() const { return uh_knn_size(k_); }
    uh_knn* handle() const { return k_; }
   private:
    std::shared_ptr<Context> ctx_;
    uh_knn* k_ = nullptr;
    bool kmeans_ = false;
};

// ------------------------------------------------------------------------------------------------ bag of words
struct fBow : std::map<uint32_t, float> {
    static double score(const fBow& a, const fBow& b) {
        std::vector<uint32_t> ia, ib;
        std::vector<float> wa, wb;
        for (auto& e : a) { ia.push_back(e.first); wa.push_back(e.second); }
        for (auto& e : b) { ib.push_back(e.first); wb.push_back(e.second); }
        return uh_bow_score(ia.data(), wa.data(), (int)ia.size(), ib.data(), wb.data(), (int)ib.size());
    }
};
struct fBow2 : std::map<uint32_t, std::vector<uint32_t>> {};

class Vocabulary {
   public:
    explicit Vocabulary(std::shared_ptr<Context> ctx) : ctx_(std::move(ctx)) { check(uh_bow_create(ctx_->get(), &b_)); }
    ~Vocabulary() { uh_bow_destroy(b_); }
    void fromStream(const void* bytes, size_t n) { check(uh_bow_load(b_, bytes, n)); }
    // transform(features, level, fBow&, fBow2&) (fbow.cpp:51-90)
    void transform(const uint8_t* features, int rows, int desc_bytes, size_t stride, int level, fBow& r1, fBow2& r2) {
        if (rows == 0) throw std::runtime_error("Vocabulary::transform No input data");
        std::vector<uint32_t> word(rows), node(rows);
        std::vector<float> weight(rows);
        std::vector<uint8_t> valid(rows);
        check(uh_bow_transform(b_, features, rows, stride, desc_bytes, level, word.data(), weight.data(), node.data(), valid.data()));
        r1.clear(); r2.clear();
        for (int i = 0; i < rows; i++) {
            if (word[i] != 0xFFFFFFFFu) r1[word[i]] += weight[i];
            if (valid[i]) r2[node[i]].push_back((uint32_t)i);
        }
    }
    // fBow transform(features): raw bag, then L2 normalisation (fbow.cpp:92-143)
    fBow transform(const uint8_t* features, int rows, int desc_bytes, size_t stride) {
        fBow r; fBow2 unused;
        transform(features, rows, desc_bytes, stride, -1, r, unused);
        double norm = 0;
        for (auto& e : r) norm += e.second * e.second;
        if (norm > 0.0) { const double inv = 1. / std::sqrt(norm); for (auto& e : r) e.second *= inv; }
        return r;
    }
   private:
    std::shared_ptr<Context> ctx_;
    uh_bow* b_ = nullptr;
};

// ------------------------------------------------------------------------------------------------ bundle adjustment
class GlobalOptimizer {
   public:
    using ParamSet = BAParamSet;   // globaloptimizer.h:31-47: used_frames, fixed_frames, fixFirstFrame, nIters, verbose
    explicit GlobalOptimizer(std::shared_ptr<Context> ctx) : ctx_(std::move(ctx)) { check(uh_ba_create(ctx_->get(), &b_)); }
    ~GlobalOptimizer() { uh_ba_destroy(b_); }
    // GlobalOptimizer::create(type): "" / "hip" select this implementation, anything else throws (globaloptimizer.cpp:27-33)
    static std::shared_ptr<GlobalOptimizer> create(std::shared_ptr<Context> ctx, const std::string& type = "") {
        if (!type.empty() && type != "hip") throw std::runtime_error("GlobalOptimizer::create invalid type " + type);
        return std::make_shared<GlobalOptimizer>(std::move(ctx));
    }
    std::string getName() const { return "hip"; }
    // setParams(map, params) (globaloptimizer_g2o.cpp:77-401): the selection rules of flatten_ba.hpp, written straight into the optimiser's
    // pinned staging block; then ONE H2D copy + one kernel on the device.  Snapshots everything: the map may change afterwards.
    template <class MapView>
    void setParams(const MapView& map, const ParamSet& p) {
        StagingSink sink(b_);
        index_ = flatten_for_ba(map, p, sink);
        uh_ba_params bp{p.nIters, 0.0, 0.0, 1.0f};
        check(uh_ba_set_problem_staged(b_, (int)index_.frame_of.size(), (int)index_.point_of.size(), index_.n_obs, &bp));
        staged_ = true;
        obs_keep_.assign(sink.st.obs, sink.st.obs + index_.n_obs);   // (getResults names the bad associations by these)
    }
    // setParams on a map with stereo / RGB-D observations (Frame::getDepth > 0, :250-272): flatten_for_ba_stereo + the stereo staging block.
    // The MapView also needs frame_baseline(f).  A map without any depth ends on the monocular route.
    template <class MapView>
    void setParamsStereo(const MapView& map, const ParamSet& p) {
        StereoStagingSink sink(b_);
        index_ = flatten_for_ba_stereo(map, p, sink);
        uh_ba_params bp{p.nIters, 0.0, 0.0, 1.0f};
        check(uh_ba_set_problem_staged_stereo(b_, (int)index_.frame_of.size(), (int)index_.point_of.size(), index_.n_obs, &bp, 0.0, 0.0));
        staged_ = true;
        obs_keep_.assign(sink.st.obs, sink.st.obs + index_.n_obs);
    }
    // setParams on a map with markers (globaloptimizer_g2o.cpp:156-171, 277-352; any mix of monocular and stereo / RGB-D observations):
    // flatten_for_ba_markers into plain vectors, then uh_ba_set_problem_markers — the wide form; the staging block has no marker form.  The
    // MapView also needs the marker members listed in flatten_ba.hpp.  A map without markers ends on the marker-free route.
    template <class MapView>
    void setParamsMarkers(const MapView& map, const ParamSet& p) {
        StereoVectorSink flat;
        MarkerVectorSink mk;
        index_ = flatten_for_ba_markers(map, p, flat, mk, mindex_);
        const int E = index_.n_obs;
        std::vector<int32_t> op(E), of(E);
        std::vector<float> uv(2 * (size_t)E);
        std::vector<double> w(E);
        for (int e = 0; e < E; e++) { op[e] = flat.obs[e].point; of[e] = flat.obs[e].frame; uv[2 * e] = flat.obs[e].u; uv[2 * e + 1] = flat.obs[e].v; w[e] = flat.obs[e].inv_sigma; }
        const uh_ba_problem pr{(int32_t)index_.frame_of.size(), (int32_t)index_.point_of.size(), E, flat.poses.data(), flat.fixed.data(), flat.intr.data(),
                               flat.points.data(), op.data(), of.data(), uv.data(), w.data()};
        const uh_ba_stereo sx{flat.depth.data(), flat.bl.data(), 0.0, 0.0};
        const uh_ba_markers m = mk.view();
        uh_ba_params bp{p.nIters, 0.0, 0.0, 1.0f};
        check(uh_ba_set_problem_markers(b_, &pr, &sx, &m, &bp));
        staged_ = true;
        obs_keep_ = flat.obs;
    }
    // getResults' marker part (:526-527), after getResults(map): Marker::pose_g2m of the markers setParamsMarkers took
    template <class MapView>
    void getMarkerResults(MapView& map) {
        if (mindex_.marker_of.empty()) return;
        std::vector<float> poses(16 * mindex_.marker_of.size());
        check(uh_ba_get_marker_results(b_, poses.data(), nullptr, nullptr));
        apply_marker_results(map, mindex_, poses.data());
    }
    const FlatBAMarkerIndex& marker_index() const { return mindex_; }
    // ... and on flattened arrays with the stereo block beside them
    void setParams(const uh_ba_problem& problem, const uh_ba_stereo& stereo, const ParamSet& p) {
        uh_ba_params bp{p.nIters, 0.0, 0.0, 1.0f};
        check(uh_ba_set_problem_stereo(b_, &problem, &stereo, &bp));
        keep_flat(problem);
    }
    // setParams on a map the caller has flattened already
    void setParams(const uh_ba_problem& problem, const ParamSet& p) {
        uh_ba_params bp{p.nIters, 0.0, 0.0, 1.0f};
        check(uh_ba_set_problem(b_, &problem, &bp));
        keep_flat(problem);
    }
    void optimize(bool* stopASAP = nullptr) { check(uh_ba_optimize(b_, reinterpret_cast<const volatile uint8_t*>(stopASAP))); }
    // getResults(map) (:466-537): poses of the free frames, point coordinates, updatePointNormalAndDistances; fills getBadAssociations()
    template <class MapView>
    void getResults(MapView& map) {
        if (!staged_) throw std::runtime_error("GlobalOptimizer::getResults(map): setParams(map, ...) has not been called");
        std::vector<float> poses(16 * index_.frame_of.size()), points(3 * index_.point_of.size() + 1);
        std::vector<uint8_t> bad(index_.n_obs + 1);
        check(uh_ba_get_results(b_, poses.data(), points.data(), nullptr, bad.data(), nullptr));
        bad_ = apply_results(map, index_, poses.data(), points.data(), bad.data(), obs_keep_.data());
    }
    // getResults into plain arrays: poses K x 16 float, points P x 3 float (flattened indices)
    void getResults(std::vector<float>& poses_f2g, std::vector<float>& points) {
        const size_t K = staged_ ? index_.frame_of.size() : (size_t)K_, P = staged_ ? index_.point_of.size() : (size_t)P_;
        poses_f2g.resize(K * 16);
        points.resize(P * 3);
        std::vector<uint8_t> bad(obs_keep_.size() + 1);
        check(uh_ba_get_results(b_, poses_f2g.data(), points.data(), nullptr, bad.data(), nullptr));
        bad_.clear();
        for (size_t e = 0; e < obs_keep_.size(); e++)
            if (bad[e]) bad_.push_back(staged_ ? std::make_pair(index_.point_of[obs_keep_[e].point], index_.frame_of[obs_keep_[e].frame])
                                               : std::make_pair((uint32_t)obs_keep_[e].point, (uint32_t)obs_keep_[e].frame));
    }
    // one function to do everything (globaloptimizer_g2o.cpp:404-414)
    template <class MapView>
    void optimize(MapView& map, const ParamSet& p = ParamSet()) { setParams(map, p); optimize(); getResults(map); }
    std::vector<std::pair<uint32_t, uint32_t>> getBadAssociations() { return bad_; }
    const FlatBAIndex& index() const { return index_; }
    uh_ba* handle() const { return b_; }
   private:
    void keep_flat(const uh_ba_problem& problem) {   // what getResults needs of a problem given as arrays
        staged_ = false;
        obs_keep_.resize(problem.n_obs);
        for (int e = 0; e < problem.n_obs; e++) obs_keep_[e] = uh_ba_obs{problem.obs_point[e], problem.obs_frame[e], 0.f, 0.f, 0.0};
        index_ = FlatBAIndex{};
        index_.n_obs = problem.n_obs;
        K_ = problem.n_frames; P_ = problem.n_points;
    }
    std::shared_ptr<Context> ctx_;
    uh_ba* b_ = nullptr;
    int K_ = 0, P_ = 0;
    bool staged_ = false;
    FlatBAIndex index_;
    FlatBAMarkerIndex mindex_;
    std::vector<uh_ba_obs> obs_keep_;
    std::vector<std::pair<uint32_t, uint32_t>> bad_;
};

// ---- ucoslam::PnPSolver::solvePnp (optimization/pnpsolver.h:30-38) on flattened matches ----------------------------------
class PnPSolver {
   public:
    explicit PnPSolver(std::shared_ptr<Context> ctx) : ctx_(std::move(ctx)) { check(uh_pnp_create(ctx_->get(), &p_)); }
    ~PnPSolver() { uh_pnp_destroy(p_); }
    // pose_io: row-major 4x4 float, refined in place; bad[i] = 1 marks an outlier match (the reference sets imgIdx = -1);
    // returns the number of inliers like solvePnp (pnpsolver.cpp:116-409)
    int solvePnp(float* pose_io, const float intr4[4], int n, const float* p3d, const float* kp, const float* inv_sigma, const float* weight,
                 std::vector<uint8_t>& bad) {
        bad.assign(n > 0 ? n : 1, 0);
        float out[16];
        int32_t iters[4];
        const int rc = uh_pnp_solve(p_, pose_io, intr4, n, p3d, kp, inv_sigma, weight, out, bad.data(), iters, nullptr);
        if (rc < 0) check(rc);
        std::copy(out, out + 16, pose_io);
        bad.resize(n);
        return rc;
    }
    // stereo / RGB-D frames (pnpsolver.cpp:205-276): depth[i] = frame.getDepth(queryIdx) of match i (<= 0: monocular match),
    // bl = frame.imageParams.bl; the weights are the monocular ones (the solver doubles those of stereo matches)
    int solvePnp(float* pose_io, const float intr4[4], int n, const float* p3d, const float* kp, const float* inv_sigma, const float* weight,
                 const float* depth, float bl, std::vector<uint8_t>& bad) {
        bad.assign(n > 0 ? n : 1, 0);
        float out[16];
        int32_t iters[4];
        const int rc = uh_pnp_solve_stereo(p_, pose_io, intr4, n, p3d, kp, inv_sigma, weight, depth, bl, out, bad.data(), iters, nullptr);
        if (rc < 0) check(rc);
        std::copy(out, out + 16, pose_io);
        bad.resize(n);
        return rc;
    }
    // a marker of the frame as solvePnp's marker_poses holds it (pnpsolver.cpp:281-299: the frame's markers with a valid pose_g2m that a
    // neighbour keyframe of currentKeyFrame sees — the selection stays the caller's)
    struct Marker {
        float pose_g2m[16];    // ucoslam::Marker::pose_g2m, row-major 4x4
        float size;            // ucoslam::Marker::size
        float und_corners[8];  // ucoslam::MarkerObservation::und_corners: x0 y0 .. x3 y3
    };
    // keypoint matches and markers in one optimisation (pnpsolver.cpp:280-386); depth may be NULL (monocular frame).  n = 0 with markers is
    // a valid, marker-only solve.  The return value stays the number of good keypoint matches.
    int solvePnp(float* pose_io, const float intr4[4], int n, const float* p3d, const float* kp, const float* inv_sigma, const float* weight,
                 const float* depth, float bl, const std::vector<Marker>& markers, std::vector<uint8_t>& bad) {
        bad.assign(n > 0 ? n : 1, 0);
        std::vector<float> g2m(16 * markers.size()), size(markers.size()), corners(8 * markers.size());
        for (size_t m = 0; m < markers.size(); m++) {
            std::copy(markers[m].pose_g2m, markers[m].pose_g2m + 16, g2m.begin() + 16 * m);
            size[m] = markers[m].size;
            std::copy(markers[m].und_corners, markers[m].und_corners + 8, corners.begin() + 8 * m);
        }
        const uh_pnp_markers mk{(int32_t)markers.size(), g2m.data(), size.data(), corners.data()};
        float out[16];
        int32_t iters[4];
        const int rc = uh_pnp_solve_markers(p_, pose_io, intr4, n, p3d, kp, inv_sigma, weight, depth, bl, &mk, out, bad.data(), iters, nullptr);
        if (rc < 0) check(rc);
        std::copy(out, out + 16, pose_io);
        bad.resize(n);
        return rc;
    }
    // ---- ucoslam::PnPSolver::solvePnPRansac (pnpsolver.cpp:36-114), the relocalisation RANSAC (uh_pnp_ransac) ----
    // frame: und_kpts[i].pt.x / .y and imageParams.fx() fy() cx() cy() as ucoslam::Frame has them; map: point_coordinates(id, float[3])
    // and point_normal(id, float[3]) (MapPoint::getCoordinates / getNormal); matches_io: queryIdx = the frame's keypoint, trainIdx = the
    // map point's id; pose_io: the se3's rt[6] (rvec, tvec).  Returns what the reference returns and leaves matches_io / pose_io as it
    // leaves them: false below 4 matches (nothing touched, no sample drawn), false below 4 inliers (matches untouched, pose overwritten
    // by the best hypothesis if one had an inlier), else the inliers in their order.  The samples come from libc rand() exactly as the
    // reference's std::random_shuffle draws them (uh_pnp_ransac_samples).
    template <class Frame, class MapView>
    bool solvePnPRansac(const Frame& frame, const MapView& map, std::vector<uh_dmatch>& matches_io, float pose_io[6], int maxIters = 50) {
        std::vector<std::vector<uh_dmatch>*> m{&matches_io};
        std::vector<float*> p{pose_io};
        return solvePnPRansac(frame, map, m, p, maxIters)[0];
    }
    // all candidate keyframes of one lost frame in one call (System::relocalize runs the function once per candidate): candidate c has
    // matches_io[c] and pose_io[c]; the samples are drawn candidate by candidate in that order
    template <class Frame, class MapView>
    std::vector<bool> solvePnPRansac(const Frame& frame, const MapView& map, const std::vector<std::vector<uh_dmatch>*>& matches_io, const std::vector<float*>& pose_io,
                                     int maxIters = 50) {
        if (matches_io.size() != pose_io.size()) throw std::runtime_error("PnPSolver::solvePnPRansac: one pose per match list");
        const size_t C = matches_io.size();
        const float intr4[4] = {frame.imageParams.fx(), frame.imageParams.fy(), frame.imageParams.cx(), frame.imageParams.cy()};
        std::vector<std::vector<float>> p3d(C), nrm(C), kp(C);
        std::vector<std::vector<int32_t>> smp(C), inl(C);
        std::vector<uh_ransac_problem> pr(C);
        std::vector<uh_ransac_result> res(C);
        for (size_t c = 0; c < C; c++) {
            const std::vector<uh_dmatch>& m = *matches_io[c];
            const size_t n = m.size();
            p3d[c].resize(3 * n); nrm[c].resize(3 * n); kp[c].resize(2 * n); inl[c].resize(n ? n : 1);
            for (size_t i = 0; i < n; i++) {
                map.point_coordinates((uint32_t)m[i].trainIdx, &p3d[c][3 * i]);
                map.point_normal((uint32_t)m[i].trainIdx, &nrm[c][3 * i]);
                kp[c][2 * i] = frame.und_kpts[m[i].queryIdx].pt.x; kp[c][2 * i + 1] = frame.und_kpts[m[i].queryIdx].pt.y;
            }
            smp[c].assign(4 * (size_t)(maxIters > 0 ? maxIters : 0), 0);
            if (n >= 4 && maxIters > 0) check(uh_pnp_ransac_samples((int)n, maxIters, smp[c].data()));
            pr[c] = uh_ransac_problem{(int32_t)n, p3d[c].data(), nrm[c].data(), kp[c].data(), maxIters, smp[c].data(), pose_io[c]};
            res[c] = uh_ransac_result{};
            res[c].inliers = inl[c].data(); res[c].cap = (int32_t)n;
        }
        std::vector<bool> ok(C, false);
        if (maxIters <= 0) {   // the reference's loop does not run: below four matches or not, nothing is found
            return ok;
        }
        check(uh_pnp_ransac(p_, intr4, (int)C, pr.data(), res.data()));
        for (size_t c = 0; c < C; c++) {
            if (matches_io[c]->size() < 4) continue;
            std::copy(res[c].rt6, res[c].rt6 + 6, pose_io[c]);   // (equal to what went in when no hypothesis had an inlier)
            if (!res[c].ok) continue;
            std::vector<uh_dmatch> kept((size_t)res[c].n_inliers);
            for (int i = 0; i < res[c].n_inliers; i++) kept[i] = (*matches_io[c])[inl[c][i]];
            *matches_io[c] = std::move(kept);
            ok[c] = true;
        }
        return ok;
    }
   private:
    std::shared_ptr<Context> ctx_;
    uh_pnp* p_ = nullptr;
};

// ---- ucoslam::Map::matchFrameToMapPoints (map.cpp:651-770) on a flattened frame / candidate list -------------------------
// ucoslam::FrameMatcher (TYPE_BOW), framematcher.cpp:395-535, on flattened frames (see uh_bow_frame)
class FrameMatcherBoW {
   public:
    explicit FrameMatcherBoW(std::shared_ptr<Context> ctx) : ctx_(std::move(ctx)) { check(uh_bowmatch_create(ctx_->get(), &h_)); }
    ~FrameMatcherBoW() { uh_bowmatch_destroy(h_); }
    std::vector<uh_dmatch> matchEpipolar(const uh_bow_match_args& args) {
        std::vector<uh_dmatch> out(args.query.n_kpts > 0 ? args.query.n_kpts : 1);
        const int k = uh_bowmatch_match(h_, &args, out.data(), (int)out.size());
        if (k < 0) check(k);
        out.resize(k);
        return out;
    }
   private:
    std::shared_ptr<Context> ctx_;
    uh_bowmatch* h_ = nullptr;
};

class ProjectionMatcher {
   public:
    explicit ProjectionMatcher(std::shared_ptr<Context> ctx) : ctx_(std::move(ctx)) { check(uh_projmatch_create(ctx_->get(), &h_)); }
    ~ProjectionMatcher() { uh_projmatch_destroy(h_); }
    // once per frame, where the reference calls Frame::create_kdtree (frame.h:124)
    void setFrame(const uh_proj_frame& f) { check(uh_projmatch_set_frame(h_, &f)); }
    // returns the reference's vector<cv::DMatch> (uh_dmatch has cv::DMatch's layout); visible (optional) gets the
    // markMapPointsAsVisible flags for the caller to apply MapPoint::setVisible()
    std::vector<uh_dmatch> matchFrameToMapPoints(const float pose_f2g[16], const uh_map_points& pts, float minDescDist, float maxRepjDist,
                                                 std::vector<uint8_t>* visible = nullptr) {
        std::vector<uh_dmatch> out(pts.n > 0 ? pts.n : 1);
        if (visible) visible->assign(pts.n > 0 ? pts.n : 1, 0);
        const int k = uh_projmatch_match(h_, pose_f2g, &pts, minDescDist, maxRepjDist, out.data(), (int32_t)out.size(), nullptr, nullptr,
                                         visible ? visible->data() : nullptr);
        if (k < 0) check(k);
        out.resize(k);
        if (visible) visible->resize(pts.n);
        return out;
    }
    // the tracker's search against the previous frame (System's private member at system.cpp:5930-6460, called at :6559-6565):
    // pose_f2g = the current frame's predicted pose, pts = the previous frame's keypoints that carry a good map point
    std::vector<uh_dmatch> matchFrameToPrevFrame(const float pose_f2g[16], const uh_prev_points& pts, float minDescDist, float maxRepjDist) {
        std::vector<uh_dmatch> out(pts.n > 0 ? pts.n : 1);
        const int k = uh_projmatch_match_prev(h_, pose_f2g, &pts, minDescDist, maxRepjDist, out.data(), (int32_t)out.size(), nullptr, nullptr);
        if (k < 0) check(k);
        out.resize(k);
        return out;
    }
   private:
    std::shared_ptr<Context> ctx_;
    uh_projmatch* h_ = nullptr;
};

// ---- System::relocalize's pose search (utils/system.cpp ~4950-5500) for all candidate keyframes of a lost frame in ONE call -------------
// (uh_relocalize_pose): solvePnPRansac per candidate, matchFrameToMapPoints from its pose over the candidate's points, solvePnp, the
// candidate with the most good matches.  The object owns its matcher, solver and the device-resident copy of the lost frame.
class Relocalizer {
   public:
    struct Candidate {
        std::vector<uh_dmatch> matches;      // queryIdx = the frame's keypoint (trainIdx is not read: the projection search replaces the list)
        std::vector<float> p3d, normal;      // matches.size() x 3 each: the matched map points' coordinates and normals
        float rt6[6];                        // the keyframe's pose_f2g as (rvec, tvec)
        uh_map_points points;                // getNeighborsVLevel2(kf, true), flattened
        const float* weight = nullptr;       // points.n: 1 / 0.5 (MapPoint::isStable), NULL = all 1
        const int32_t* samples = nullptr;    // maxIters x 4, or NULL: drawn from libc rand() as the reference draws them
    };
    struct Step {
        int stage = 0, ok = 0, n_inliers = 0, best_iter = -1, solve_inliers = 0, n_good = 0;   // stage: UH_RELOC_*
        float rt6[6] = {0}, pose_ransac[16] = {0}, pose_solve[16] = {0};
        int32_t iters[4] = {0, 0, 0, 0};
        std::vector<int32_t> inliers;        // RANSAC's inliers (indices into matches)
        std::vector<uh_dmatch> matches_map;  // the projection search's list
        std::vector<uint8_t> bad;            // the solve's outlier flags over matches_map (empty when the solve did not run)
    };
    struct Result { int best = -1; float pose[16] = {0}; int n_matches = 0; std::vector<Step> steps; };

    explicit Relocalizer(std::shared_ptr<Context> ctx) : ctx_(std::move(ctx)) {
        check(uh_projmatch_create(ctx_->get(), &pm_));
        check(uh_pnp_create(ctx_->get(), &pnp_));
        check(uh_dev_frame_create(ctx_->get(), &fr_));
    }
    ~Relocalizer() { uh_projmatch_destroy(pm_); uh_pnp_destroy(pnp_); uh_dev_frame_destroy(fr_); }
    Relocalizer(const Relocalizer&) = delete;
    Relocalizer& operator=(const Relocalizer&) = delete;
    // the lost frame: f.und_kpts / f.desc / f.n_kpts (at most 4096) go to the device once, f's camera, scale and bounds fields to the matcher
    void setFrame(const uh_proj_frame& f) {
        check(uh_dev_frame_upload(fr_, f.und_kpts, f.n_kpts, f.desc));
        check(uh_projmatch_set_frame_dev(pm_, fr_, &f));
        n_kpts_ = f.n_kpts;
    }
    // gates: System::relocalize's 25 / 15 / 30 / 30
    Result relocalize(const float intr4[4], const std::vector<float>& inv_sigma_levels, const std::vector<Candidate>& cands, float maxDescDistance, int maxIters = 50,
                      int minMatchesRansac = 25, int minMatchesAfterRansac = 15, int minMatchesMap = 30, int minGood = 30) {
        const uh_reloc_args args{intr4, inv_sigma_levels.data(), (int32_t)inv_sigma_levels.size(), 2 * maxDescDistance, 2.5f, maxIters,
                                 minMatchesRansac, minMatchesAfterRansac, minMatchesMap, minGood};
        const size_t C = cands.size();
        std::vector<std::vector<int32_t>> q(C);
        std::vector<uh_reloc_candidate> cs(C);
        std::vector<uh_reloc_step> ss(C);
        Result out;
        out.steps.resize(C);
        for (size_t c = 0; c < C; c++) {
            const Candidate& k = cands[c];
            const size_t n = k.matches.size();
            if (k.p3d.size() != 3 * n || k.normal.size() != 3 * n) throw std::runtime_error("Relocalizer::relocalize: p3d / normal need three floats per match");
            q[c].resize(n ? n : 1);
            for (size_t i = 0; i < n; i++) q[c][i] = k.matches[i].queryIdx;
            cs[c] = uh_reloc_candidate{(int32_t)n, q[c].data(), k.p3d.data(), k.normal.data(), k.rt6, k.samples, &k.points, k.weight};
            Step& s = out.steps[c];
            const size_t cap = (size_t)std::max(1, std::min(k.points.n, n_kpts_));
            s.inliers.assign(n ? n : 1, 0); s.matches_map.assign(cap, uh_dmatch{}); s.bad.assign(cap, 0);
            ss[c] = uh_reloc_step{};
            ss[c].inliers = s.inliers.data(); ss[c].cap_inliers = (int32_t)s.inliers.size();
            ss[c].matches_map = s.matches_map.data(); ss[c].bad = s.bad.data(); ss[c].cap_map = (int32_t)cap;
        }
        uh_reloc_result res{};
        res.steps = ss.data();
        check(uh_relocalize_pose(pm_, pnp_, &args, (int)C, cs.data(), &res));
        for (size_t c = 0; c < C; c++) {
            Step& s = out.steps[c];
            const uh_reloc_step& r = ss[c];
            s.stage = r.stage; s.ok = r.ok; s.n_inliers = r.n_inliers; s.best_iter = r.best_iter; s.solve_inliers = r.solve_inliers; s.n_good = r.n_good;
            std::copy(r.rt6, r.rt6 + 6, s.rt6); std::copy(r.pose_ransac, r.pose_ransac + 16, s.pose_ransac); std::copy(r.pose_solve, r.pose_solve + 16, s.pose_solve);
            std::copy(r.iters, r.iters + 4, s.iters);
            s.inliers.resize((size_t)r.n_inliers); s.matches_map.resize((size_t)r.n_map); s.bad.resize(r.stage >= UH_RELOC_FEW_GOOD ? (size_t)r.n_map : 0);
        }
        out.best = res.best; out.n_matches = res.n_matches;
        std::copy(res.pose, res.pose + 16, out.pose);
        return out;
    }
   private:
    std::shared_ptr<Context> ctx_;
    uh_projmatch* pm_ = nullptr;
    uh_pnp* pnp_ = nullptr;
    uh_dev_frame* fr_ = nullptr;
    int n_kpts_ = 0;
};

// ---- ucoslam::loopClosurePathOptimizationg2o (optimization/graphoptsim3.cpp:74-168) ---------------------------------------
// The pose type is a template parameter (the reference's is cv::Mat, CV_32F 4x4): posegraph_pose_ptr(pose) must give its 16
// row-major floats; the overloads below cover anything with data() — for cv::Mat add one that returns m.ptr<float>().
template <class Pose> inline auto posegraph_pose_ptr(Pose& p) -> decltype(p.data()) { return p.data(); }
template <class Pose> inline auto posegraph_pose_ptr(const Pose& p) -> decltype(p.data()) { return p.data(); }

struct FlatPoseGraph {
    std::vector<uint32_t> id_of;         // index -> key of optimPoses, in key order (std::map's, which is the reference's vertex order too)
    std::vector<float> poses;            // id_of.size() x 16
    std::vector<int32_t> edge_i, edge_j;
    std::vector<float> weight;           // one per edge: edgeWeight[CovisGraph::join(first, second)], 1 where the map has none
    float expected[16];
    int32_t idx_new = -1, idx_old = -1;
    int32_t fix_scale = 0;
    uh_posegraph_problem view() const {
        return uh_posegraph_problem{(int32_t)id_of.size(), poses.data(), (int32_t)edge_i.size(), edge_i.data(), edge_j.data(), weight.data(), idx_new, idx_old,
                                    expected, fix_scale};
    }
};

// CovisGraph::join (map_types/covisgraph.h:102-109): the smaller id in the high word
inline uint64_t covis_join(uint32_t a, uint32_t b) { if (a > b) std::swap(a, b); return ((uint64_t)a << 32) | b; }

// Throws std::length_error above UH_POSEGRAPH_MAX_POSES, so that a caller can keep "g2o" for such a map, and std::runtime_error for an
// id that optimPoses does not hold (the reference asserts).
template <class Pose>
FlatPoseGraph flatten_posegraph(const std::vector<std::pair<uint32_t, uint32_t>>& edges, uint32_t IdClosesLoopNew, uint32_t IdClosesLoopOld,
                                const Pose& expectedPoseNew, const std::map<uint32_t, Pose>& optimPoses, bool bFixScale,
                                const std::map<uint64_t, float>& edgeWeight) {
    if (optimPoses.size() > (size_t)UH_POSEGRAPH_MAX_POSES)
        throw std::length_error("loopClosurePathOptimization: " + std::to_string(optimPoses.size()) + " keyframes exceed the dense solver's cap of " +
                                std::to_string(UH_POSEGRAPH_MAX_POSES));
    FlatPoseGraph f;
    std::map<uint32_t, int32_t> index;
    for (const auto& kv : optimPoses) {
        index[kv.first] = (int32_t)f.id_of.size();
        f.id_of.push_back(kv.first);
        const float* M = posegraph_pose_ptr(kv.second);
        f.poses.insert(f.poses.end(), M, M + 16);
    }
    auto at = [&](uint32_t id) {
        const auto it = index.find(id);
        if (it == index.end()) throw std::runtime_error("loopClosurePathOptimization: keyframe " + std::to_string(id) + " is not in optimPoses");
        return it->second;
    };
    for (const auto& e : edges) {
        f.edge_i.push_back(at(e.first));
        f.edge_j.push_back(at(e.second));
        const auto w = edgeWeight.find(covis_join(e.first, e.second));
        f.weight.push_back(w != edgeWeight.end() ? w->second : 1.f);
    }
    f.idx_new = at(IdClosesLoopNew);
    f.idx_old = at(IdClosesLoopOld);
    std::memcpy(f.expected, posegraph_pose_ptr(expectedPoseNew), sizeof f.expected);
    f.fix_scale = bFixScale ? 1 : 0;
    return f;
}

// graphoptsim3.cpp:156-165: every pose of optimPoses is replaced by its corrected [sR | t/s]
template <class Pose>
void apply_posegraph_results(std::map<uint32_t, Pose>& optimPoses, const FlatPoseGraph& f, const float* poses) {
    for (size_t k = 0; k < f.id_of.size(); k++) std::memcpy(posegraph_pose_ptr(optimPoses.at(f.id_of[k])), poses + 16 * k, 16 * sizeof(float));
}

// the reference's argument list behind the context
template <class Pose>
void loopClosurePathOptimization(Context& ctx, const std::vector<std::pair<uint32_t, uint32_t>>& edges, uint32_t IdClosesLoopNew, uint32_t IdClosesLoopOld,
                                 const Pose& expectedPoseNew, std::map<uint32_t, Pose>& optimPoses, bool bFixScale,
                                 const std::map<uint64_t, float>& edgeWeight = std::map<uint64_t, float>()) {
    const FlatPoseGraph f = flatten_posegraph(edges, IdClosesLoopNew, IdClosesLoopOld, expectedPoseNew, optimPoses, bFixScale, edgeWeight);
    uh_posegraph* g = nullptr;
    check(uh_posegraph_create(ctx.get(), &g));
    std::unique_ptr<uh_posegraph, void (*)(uh_posegraph*)> hold(g, uh_posegraph_destroy);
    const uh_posegraph_problem pr = f.view();
    check(uh_posegraph_optimize(g, &pr, nullptr));
    std::vector<float> poses(16 * f.id_of.size());
    check(uh_posegraph_get_results(g, poses.data(), nullptr, nullptr, nullptr));
    apply_posegraph_results(optimPoses, f, poses.data());
}

// ---- ucoslam::Triangulate (basictypes/misc.h:65) and MapManager's new-point loop (utils/mapmanager.cpp:10087-10696) ------------
// The frame type is a template parameter shaped like ucoslam::Frame: idx, pose_f2g (16 row-major floats through posegraph_pose_ptr),
// und_kpts (elements with pt.x, pt.y, octave), scaleFactors (std::vector<float>) and imageParams with fx() fy() cx() cy()
// (imageparams.h:52-55).
inline void se3_inverse(const float* M, float* o) {   // Se3Transform::inv, basictypes/se3transform.h:89-107
    o[0] = M[0]; o[1] = M[4]; o[2] = M[8]; o[4] = M[1]; o[5] = M[5]; o[6] = M[9]; o[8] = M[2]; o[9] = M[6]; o[10] = M[10];
    o[3] = -(M[3] * o[0] + M[7] * o[1] + M[11] * o[2]);
    o[7] = -(M[3] * o[4] + M[7] * o[5] + M[11] * o[6]);
    o[11] = -(M[3] * o[8] + M[7] * o[9] + M[11] * o[10]);
    o[12] = o[13] = o[14] = 0;
    o[15] = 1;
}
inline void camera_center(const float* p, float c[3]) {   // Frame::getCameraCenter, map_types/frame.h:189-197
    c[0] = -(p[3] * p[0] + p[7] * p[4] + p[11] * p[8]);
    c[1] = -(p[3] * p[1] + p[7] * p[5] + p[11] * p[9]);
    c[2] = -(p[3] * p[2] + p[7] * p[6] + p[11] * p[10]);
}
inline void mat44_product(const float* A, const float* B, float* C) {   // cv::Mat's operator* on CV_32F: double sums, one rounding (unpinned)
    for (int i = 0; i < 4; i++)
        for (int j = 0; j < 4; j++) {
            double s = 0;
            for (int k = 0; k < 4; k++) s += (double)A[4 * i + k] * (double)B[4 * k + j];
            C[4 * i + j] = (float)s;
        }
}

// the arrays uh_newpoints_run reads of one frame, owned
struct NewPointsFrame {
    float intr4[4], center[3];
    std::vector<float> pt, scale_factors;
    std::vector<int32_t> octave;
    template <class Frame> explicit NewPointsFrame(const Frame& f) : scale_factors(f.scaleFactors.begin(), f.scaleFactors.end()) {
        intr4[0] = f.imageParams.fx(); intr4[1] = f.imageParams.fy(); intr4[2] = f.imageParams.cx(); intr4[3] = f.imageParams.cy();
        camera_center(posegraph_pose_ptr(f.pose_f2g), center);
        pt.reserve(2 * f.und_kpts.size());
        octave.reserve(f.und_kpts.size());
        for (const auto& k : f.und_kpts) { pt.push_back(k.pt.x); pt.push_back(k.pt.y); octave.push_back((int32_t)k.octave); }
    }
    void fill(uh_newpoints_pair& p, const float* RT, const std::vector<uh_dmatch>& matches) const {
        std::memcpy(p.RT, RT, sizeof p.RT);
        std::memcpy(p.intr4, intr4, sizeof intr4);
        std::memcpy(p.cam_center, center, sizeof center);
        p.n_levels = (int32_t)scale_factors.size(); p.scale_factors = scale_factors.data();
        p.n_kpts = (int32_t)octave.size(); p.pt = pt.data(); p.octave = octave.data();
        p.n_matches = (int32_t)matches.size(); p.matches = matches.data();
    }
    void fill(uh_newpoints_args& a, const float* pose_f2g) const {
        std::memcpy(a.intr4, intr4, sizeof intr4);
        se3_inverse(pose_f2g, a.pose_g2f);
        std::memcpy(a.cam_center, center, sizeof center);
        a.n_levels = (int32_t)scale_factors.size(); a.scale_factors = scale_factors.data();
        a.n_kpts = (int32_t)octave.size(); a.pt = pt.data(); a.octave = octave.data();
    }
};

struct NewPointInfo {   // MapManager::NewPointInfo (utils/mapmanager.h) + the keypoint of the new keyframe
    uint32_t kp_idx;
    float xyz[3];       // the reference's `pose` (cv::Point3f, global coordinates)
    float dist;
    std::vector<std::pair<uint32_t, uint32_t>> frame_kpt;   // (frame idx, keypoint): the new keyframe first
};

class NewPointCreator {
   public:
    explicit NewPointCreator(Context& ctx) { check(uh_newpoints_create(ctx.get(), &h_)); }
    ~NewPointCreator() { uh_newpoints_destroy(h_); }
    NewPointCreator(const NewPointCreator&) = delete;
    NewPointCreator& operator=(const NewPointCreator&) = delete;

    // matchesPerNeighbour[j] = matchEpipolar(neighbour j, MODE_UNASSIGNED, RT) of a FrameMatcher set up on newKF: queryIdx in the
    // neighbour, trainIdx in newKF.  scaleFactorParam = System::getParams().scaleFactor.  mergeRule: UH_NEWPOINTS_MERGE_* (see ucoslam_hip.h:
    // AS_COMPILED is what the reference binary does, SMALLEST_OCTAVE what its source is written to do).
    template <class Frame>
    std::vector<NewPointInfo> create(const Frame& newKF, const std::vector<const Frame*>& neighbours, const std::vector<std::vector<uh_dmatch>>& matchesPerNeighbour,
                                     float scaleFactorParam, int mergeRule = UH_NEWPOINTS_MERGE_SMALLEST_OCTAVE, float maxChi2 = 5.998f) {
        if (neighbours.size() != matchesPerNeighbour.size()) throw std::runtime_error("NewPointCreator::create: one match list per neighbour");
        const NewPointsFrame nf(newKF);
        std::vector<NewPointsFrame> nb;
        nb.reserve(neighbours.size());
        std::vector<uh_newpoints_pair> pairs(neighbours.size());
        float inv[16], RT[16];
        se3_inverse(posegraph_pose_ptr(newKF.pose_f2g), inv);
        for (size_t j = 0; j < neighbours.size(); j++) {
            nb.emplace_back(*neighbours[j]);
            mat44_product(posegraph_pose_ptr(neighbours[j]->pose_f2g), inv, RT);   // mapmanager.cpp:10045-10062
            nb.back().fill(pairs[j], RT, matchesPerNeighbour[j]);
        }
        uh_newpoints_args a{};
        nf.fill(a, posegraph_pose_ptr(newKF.pose_f2g));
        a.n_pairs = (int32_t)pairs.size(); a.pairs = pairs.data();
        a.max_chi2 = maxChi2; a.ratio_factor = 1.5f * scaleFactorParam; a.merge_rule = mergeRule;
        uh_newpoints_result r{};
        check(uh_newpoints_run(h_, &a, &r));
        last_ = r;
        std::vector<NewPointInfo> out(r.n_new);
        for (int i = 0; i < r.n_new; i++) {
            NewPointInfo& p = out[i];
            p.kp_idx = (uint32_t)r.kp_idx[i];
            for (int c = 0; c < 3; c++) p.xyz[c] = r.xyz_global[3 * i + c];
            p.dist = r.distance[i];
            for (int k = r.obs_ptr[i]; k < r.obs_ptr[i + 1]; k++)
                p.frame_kpt.emplace_back(r.obs_pair[k] < 0 ? (uint32_t)newKF.idx : (uint32_t)neighbours[r.obs_pair[k]]->idx, (uint32_t)r.obs_kpt[k]);
        }
        return out;
    }
    const uh_newpoints_result& last_result() const { return last_; }   // per-match status / xyz_cam of the latest create (valid until the next)
   private:
    uh_newpoints* h_ = nullptr;
    uh_newpoints_result last_{};
};

// misc.h:65 — as many points as matches, NaN where the triangulation is refused; RT = Query.pose_f2g * Train.pose_f2g.inv()
template <class TrainView, class QueryView>
std::vector<std::array<float, 3>> Triangulate(Context& ctx, const TrainView& Train, const QueryView& Query, const float RT[16], const std::vector<uh_dmatch>& matches,
                                              float maxChi2 = 5.998f) {
    const NewPointsFrame tf(Train), qf(Query);
    uh_newpoints_pair pair{};
    qf.fill(pair, RT, matches);
    uh_newpoints_args a{};
    tf.fill(a, posegraph_pose_ptr(Train.pose_f2g));
    a.n_pairs = 1; a.pairs = &pair;
    a.max_chi2 = maxChi2; a.ratio_factor = 1.f; a.merge_rule = UH_NEWPOINTS_MERGE_SMALLEST_OCTAVE;   // the ratio check comes after Triangulate's surface
    uh_newpoints* h = nullptr;
    check(uh_newpoints_create(ctx.get(), &h));
    std::unique_ptr<uh_newpoints, void (*)(uh_newpoints*)> hold(h, uh_newpoints_destroy);
    uh_newpoints_result r{};
    check(uh_newpoints_run(h, &a, &r));
    std::vector<std::array<float, 3>> out(matches.size());
    for (size_t i = 0; i < out.size(); i++) out[i] = {r.xyz_cam[3 * i], r.xyz_cam[3 * i + 1], r.xyz_cam[3 * i + 2]};
    return out;
}

// ---- MapManager's search-and-fuse step (utils/mapmanager.cpp, the private vector<uint32_t> member taking Frame&: ORB-SLAM's --------------
// SearchInNeighbors), between the new map points and local BA.  MapPointFuser::searchInNeighbors(map, cur) is that function: one search per
// non-bad neighbour keyframe with the points of `cur` (ascending keyframe index), one search of every neighbour's points in `cur`, each
// search's events applied in point order through the map's own fuseMapPoints / addMapPointObservation before the next search starts.
//
// The map type is a template parameter with the reference's member names: TheKpGraph.getNeighbors(idx), keyframes[idx], map_points.is(id) /
// map_points[id], fuseMapPoints(a, b, false), addMapPointObservation(id, frame, kp), getMapPointsInFrames(begin, end).  A keyframe gives
// idx, isBad(), pose_f2g (posegraph_pose_ptr), und_kpts (pt.x, pt.y, octave), ids, scaleFactors, imageParams fx() fy() cx() cy(), minXY /
// maxXY (.x, .y), getMapPoints() and its n x 32 descriptor bytes through frame_desc_ptr(frame); a map point gives id, isBad(), setBad(),
// frames.count(idx), getCoordinates() / getNormal() (.x .y .z), get{Min,Max}DistanceInvariance() and its 32 descriptor bytes through
// mappoint_desc_ptr(point).  The overloads below read a `desc` member with data(); for cv::Mat add ones that return m.ptr<uint8_t>().
template <class Frame> inline auto frame_desc_ptr(const Frame& f) -> decltype(f.desc.data()) { return f.desc.data(); }
template <class Point> inline auto mappoint_desc_ptr(const Point& p) -> decltype(p.desc.data()) { return p.desc.data(); }

class MapPointFuser {
   public:
    explicit MapPointFuser(Context& ctx) : ctx_(&ctx), host_(false) { check(uh_fuse_create(ctx.get(), &h_)); }
    MapPointFuser() = default;   // host form only: every search through uh_fuse_search_host, no GPU needed
    ~MapPointFuser() {
        for (auto& kv : cache_) uh_dev_frame_destroy(kv.second);
        if (h_) uh_fuse_destroy(h_);
    }
    MapPointFuser(const MapPointFuser&) = delete;
    MapPointFuser& operator=(const MapPointFuser&) = delete;

    // run the searches on the calling core (the fallback of a host without a free GPU; the same results bit for bit)
    void setHostForm(bool on) { if (!on && !h_) throw std::runtime_error("MapPointFuser: no device context"); host_ = on; }
    // One uh_dev_frame per keyframe of the window is kept, keyed by keyframe index, and uploaded on first use: a keyframe's keypoints and
    // descriptors never change.  forget(idx) when a keyframe leaves the map; adopt(idx, frame) hands over the frame the extractor left on the
    // device (uh_orb_extract_frame_dev) instead of an upload — the fuser destroys it.
    void forget(uint32_t idx) { auto it = cache_.find(idx); if (it != cache_.end()) { uh_dev_frame_destroy(it->second); cache_.erase(it); } }
    void adopt(uint32_t idx, uh_dev_frame* frame) { forget(idx); cache_[idx] = frame; }
    size_t cachedFrames() const { return cache_.size(); }

    template <class Map, class Frame>
    std::vector<uint32_t> searchInNeighbors(Map& map, Frame& cur, float maxDescDistance, float th = 2.5f) {
        std::vector<uint32_t> removed;
        std::vector<uint32_t> targets;   // std::set<uint32_t> of the non-bad neighbours: ascending, unique
        for (auto n : map.TheKpGraph.getNeighbors(cur.idx))
            if (!map.keyframes[n].isBad()) targets.push_back((uint32_t)n);
        std::sort(targets.begin(), targets.end());
        targets.erase(std::unique(targets.begin(), targets.end()), targets.end());
        const std::vector<float> predict(cur.scaleFactors.begin(), cur.scaleFactors.end());
        const std::vector<uint32_t> pts = cur.getMapPoints();
        std::map<uint32_t, int> row_of;
        for (size_t r = 0; r < pts.size(); r++) row_of[pts[r]] = (int)r;
        std::vector<uint8_t> skip(pts.size());
        std::vector<uint32_t> dirty;
        bool fresh = true;
        for (uint32_t t : targets) {
            auto& KF = map.keyframes[t];
            for (size_t r = 0; r < pts.size(); r++)
                skip[r] = !map.map_points.is(pts[r]) || map.map_points[pts[r]].isBad() || map.map_points[pts[r]].frames.count(KF.idx) != 0;
            search(map, KF, pts, skip, predict, th, 1.4f, maxDescDistance, fresh, dirty, row_of);
            fresh = false;
            apply(map, KF, pts, removed, dirty);
        }
        const std::vector<uint32_t> cands = map.getMapPointsInFrames(targets.begin(), targets.end());
        skip.assign(cands.size(), 0);
        for (size_t r = 0; r < cands.size(); r++) skip[r] = map.map_points[cands[r]].isBad() || map.map_points[cands[r]].frames.count(cur.idx) != 0;
        dirty.clear();
        search(map, cur, cands, skip, predict, th, 1.f, maxDescDistance, true, dirty, row_of);
        apply(map, cur, cands, removed, dirty);
        return removed;
    }

   private:
    struct Table {
        std::vector<float> pos, nrm, mind, maxd;
        std::vector<uint8_t> desc;
        uh_map_points view() const { return uh_map_points{(int32_t)mind.size(), nullptr, pos.data(), nrm.data(), mind.data(), maxd.data(), desc.data()}; }
    };
    template <class Map> static void fill(Map& map, const std::vector<uint32_t>& ids, Table& t) {
        const size_t n = ids.size();
        t.pos.assign(3 * n, 0.f); t.nrm.assign(3 * n, 0.f); t.mind.assign(n, 0.f); t.maxd.assign(n, 0.f); t.desc.assign(32 * n, 0);
        for (size_t r = 0; r < n; r++) {
            if (!map.map_points.is(ids[r])) continue;   // (skipped by the mask: the row is never read)
            auto& mp = map.map_points[ids[r]];
            const auto p = mp.getCoordinates();
            const auto nv = mp.getNormal();
            t.pos[3 * r] = p.x; t.pos[3 * r + 1] = p.y; t.pos[3 * r + 2] = p.z;
            t.nrm[3 * r] = nv.x; t.nrm[3 * r + 1] = nv.y; t.nrm[3 * r + 2] = nv.z;
            t.mind[r] = mp.getMinDistanceInvariance(); t.maxd[r] = mp.getMaxDistanceInvariance();
            std::memcpy(&t.desc[32 * r], mappoint_desc_ptr(mp), 32);
        }
    }
    template <class Map, class Frame>
    void search(Map& map, Frame& KF, const std::vector<uint32_t>& ids, const std::vector<uint8_t>& skip, const std::vector<float>& predict, float th, float widen,
                float maxDescDistance, bool fresh, std::vector<uint32_t>& dirty, const std::map<uint32_t, int>& row_of) {
        const int n = (int)ids.size();
        bk_.assign(n > 0 ? n : 1, -1); bd_.assign(n > 0 ? n : 1, 0.f); st_.assign(n > 0 ? n : 1, 0);
        const std::vector<float> scale(KF.scaleFactors.begin(), KF.scaleFactors.end());
        kps_.resize(KF.und_kpts.size());
        for (size_t i = 0; i < kps_.size(); i++) {
            kps_[i] = uh_keypoint{};
            kps_[i].x = KF.und_kpts[i].pt.x; kps_[i].y = KF.und_kpts[i].pt.y; kps_[i].octave = (int32_t)KF.und_kpts[i].octave;
        }
        uh_proj_frame f{};
        f.und_kpts = kps_.data(); f.n_kpts = (int32_t)kps_.size(); f.desc = frame_desc_ptr(KF);
        f.scale_factors = scale.data(); f.n_levels = (int32_t)scale.size();
        f.fx = KF.imageParams.fx(); f.fy = KF.imageParams.fy(); f.cx = KF.imageParams.cx(); f.cy = KF.imageParams.cy();
        f.min_x = (int32_t)KF.minXY.x; f.min_y = (int32_t)KF.minXY.y; f.max_x = (int32_t)KF.maxXY.x; f.max_y = (int32_t)KF.maxXY.y;
        const float* pose = posegraph_pose_ptr(KF.pose_f2g);
        if (host_) {
            Table t;
            fill(map, ids, t);
            const uh_map_points v = t.view();
            check(uh_fuse_search_host(&v, &f, pose, predict.data(), (int32_t)predict.size(), skip.data(), th, widen, maxDescDistance, bk_.data(), bd_.data(), st_.data()));
            return;
        }
        if (fresh) {
            Table t;
            fill(map, ids, t);
            const uh_map_points v = t.view();
            check(uh_fuse_set_points(h_, &v));
        } else if (!dirty.empty()) {   // the rows the last apply step changed
            std::vector<uint32_t> changed;
            std::vector<int32_t> rows;
            for (uint32_t id : dirty) { auto it = row_of.find(id); if (it != row_of.end()) { changed.push_back(id); rows.push_back(it->second); } }
            if (!rows.empty()) {
                Table t;
                fill(map, changed, t);
                const uh_map_points v = t.view();
                check(uh_fuse_update_points(h_, (int32_t)rows.size(), rows.data(), &v));
            }
        }
        dirty.clear();
        auto it = cache_.find((uint32_t)KF.idx);
        if (it == cache_.end()) {
            uh_dev_frame* d = nullptr;
            check(uh_dev_frame_create(ctx_->get(), &d));
            it = cache_.emplace((uint32_t)KF.idx, d).first;
            check(uh_dev_frame_upload(d, f.und_kpts, f.n_kpts, f.desc));
        }
        check(uh_fuse_search(h_, it->second, &f, pose, predict.data(), (int32_t)predict.size(), skip.data(), th, widen, maxDescDistance, bk_.data(), bd_.data(), st_.data()));
    }
    template <class Map, class Frame>
    void apply(Map& map, Frame& KF, const std::vector<uint32_t>& ids, std::vector<uint32_t>& removed, std::vector<uint32_t>& dirty) {
        for (size_t r = 0; r < ids.size(); r++) {
            if (st_[r] != UH_FUSE_FOUND) continue;
            const uint32_t kp = (uint32_t)bk_[r], held = KF.ids[kp];
            if (held != 0xFFFFFFFFu) {
                map.fuseMapPoints(held, ids[r], false);
                removed.push_back(ids[r]);
                map.map_points[ids[r]].setBad(true);
                dirty.push_back(held);
            } else {
                map.addMapPointObservation(ids[r], KF.idx, kp);
                dirty.push_back(ids[r]);
            }
        }
    }
    Context* ctx_ = nullptr;
    uh_fuse* h_ = nullptr;
    bool host_ = true;
    std::map<uint32_t, uh_dev_frame*> cache_;
    std::vector<uh_keypoint> kps_;
    std::vector<int32_t> bk_;
    std::vector<float> bd_;
    std::vector<uint8_t> st_;
};

// ---- ucoslam::FrameExtractor::processStereo / process_rgbd (utils/frameextractor.cpp from :1419), kptImageScaleFactor == 1 --------------
// Images are non-owning views (for cv::Mat: {m.data, m.cols, m.rows, m.step, m.channels()}).  The frame type is a template parameter shaped
// like ucoslam::Frame: kpts (elements with x, y), und_kpts (elements with pt.x, pt.y, size, angle, response, octave, class_id), depth
// (std::vector<float>), fseq_idx, and its descriptors through frame_set_desc(frame, bytes, n) — the overload below fills a
// std::vector<uint8_t> desc; for cv::Mat add one that creates n x 32 CV_8UC1 and copies.  Markers, the image-scale branch and the frame's
// id / pose bookkeeping stay with the caller; `dev` (optional) also leaves the frame on the device as uh_orb_extract_frame_dev does.
struct ImageView { const void* data; int cols, rows; size_t step; int channels; };
struct StereoImageParams {   // the fields of ucoslam::ImageParams this stage reads
    float fx, fy, cx, cy;
    std::vector<float> dist;   // k1 k2 p1 p2 [k3 [k4 k5 k6]]
    float bl = 0, rgb_depthscale = 1;
};
template <class Frame> inline auto frame_set_desc(Frame& f, const uint8_t* bytes, int n) -> decltype(f.desc.assign(bytes, bytes)) { return f.desc.assign(bytes, bytes + (size_t)n * 32); }

class FrameExtractor {
   public:
    FrameExtractor(std::shared_ptr<Context> ctx, const FeatParams& fp, float maxDescDistance) : orb_(std::move(ctx)), max_desc_dist_(maxDescDistance) {
        uh_feat_params p{fp.nthreads, fp.maxFeatures, fp.nOctaveLevels, fp.scaleFactor, fp.sensitivity};
        check(uh_orb_set_params(orb_.handle(), &p));
    }
    template <class Frame>
    void processStereo(const ImageView& LeftRect, const ImageView& RightRect, const StereoImageParams& ip, Frame& frame, uint32_t frameseq_idx = UINT32_MAX,
                       uh_dev_frame* dev = nullptr) {
        if (LeftRect.cols != RightRect.cols || LeftRect.rows != RightRect.rows || LeftRect.step != RightRect.step || LeftRect.channels != RightRect.channels)
            throw std::runtime_error("processStereo: the two images differ in size, step or channels");
        set_camera(ip);
        check(uh_orb_set_stereo(orb_.handle(), ip.bl, max_desc_dist_));
        reserve();
        int n = 0;
        check(uh_orb_extract_stereo(orb_.handle(), static_cast<const uint8_t*>(LeftRect.data), static_cast<const uint8_t*>(RightRect.data), LeftRect.cols,
                                    LeftRect.rows, LeftRect.step, LeftRect.channels, kps_.data(), desc_.data(), und_.data(), depth_.data(), (int)kps_.size(), &n, dev,
                                    nullptr));
        fill(frame, n, frameseq_idx);
    }
    template <class Frame>
    void process_rgbd(const ImageView& image, const ImageView& depthImage, const StereoImageParams& ip, Frame& frame, uint32_t frameseq_idx = UINT32_MAX,
                      uh_dev_frame* dev = nullptr) {
        if (image.cols != depthImage.cols || image.rows != depthImage.rows) throw std::runtime_error("process_rgbd: colour and depth image differ in size");
        set_camera(ip);
        reserve();
        int n = 0;
        check(uh_orb_extract_rgbd(orb_.handle(), static_cast<const uint8_t*>(image.data), image.cols, image.rows, image.step, image.channels,
                                  static_cast<const uint16_t*>(depthImage.data), depthImage.step, ip.rgb_depthscale, kps_.data(), desc_.data(), und_.data(),
                                  depth_.data(), (int)kps_.size(), &n, dev));
        fill(frame, n, frameseq_idx);
    }
    ORBextractor& extractor() { return orb_; }
   private:
    void set_camera(const StereoImageParams& ip) {
        if (ip.dist.size() > 8) throw std::runtime_error("FrameExtractor: more than 8 distortion coefficients");
        uh_camera c{ip.fx, ip.fy, ip.cx, ip.cy, {0}, (int32_t)ip.dist.size()};
        for (size_t i = 0; i < ip.dist.size(); i++) c.dist[i] = ip.dist[i];
        check(uh_orb_set_camera(orb_.handle(), &c));
    }
    void reserve() {
        const size_t cap = (size_t)std::max(uh_orb_max_keypoints(orb_.handle()), 1);
        kps_.resize(cap); desc_.resize(cap * 32); und_.resize(cap * 2); depth_.resize(cap);
    }
    template <class Frame>
    void fill(Frame& f, int n, uint32_t frameseq_idx) {
        f.kpts.resize(n); f.und_kpts.resize(n); f.depth.assign(depth_.begin(), depth_.begin() + n);
        for (int i = 0; i < n; i++) {
            const uh_keypoint& k = kps_[i];
            f.kpts[i].x = k.x; f.kpts[i].y = k.y;
            auto& u = f.und_kpts[i];
            u.pt.x = und_[2 * i]; u.pt.y = und_[2 * i + 1]; u.size = k.size; u.angle = k.angle; u.response = k.response; u.octave = k.octave; u.class_id = k.class_id;
        }
        frame_set_desc(f, desc_.data(), n);
        f.fseq_idx = frameseq_idx;
    }
    ORBextractor orb_;
    float max_desc_dist_;
    std::vector<uh_keypoint> kps_;
    std::vector<uint8_t> desc_;
    std::vector<float> und_, depth_;
};

// ------------------------------------------------------------------------------------------------ map initialiser
// ucoslam::MapInitializer (src/utils/mapinitializer.h), the keypoint route: setParams / reset / setReferenceFrame as there, and
// initialize(frame2, matches) for what initialize_ does between the matcher and the map — the two-view initialise on the device
// (uh_mapinit_run).  The caller matches the two frames (FrameMatcher, MODE_ALL) and, on success, turns the result into two keyframes
// and one map point per surviving match (initialize_ :64-99).  The marker route (ARUCO_initialize) and the one-frame marker route are
// not built.  Frames are anything shaped like ucoslam::Frame: und_kpts (elements with pt.x, pt.y), imageParams with fx() fy() cx() cy().
class MapInitializer {
   public:
    struct Params {   // the fields of MapInitializer::Params the keypoint route reads, with their defaults
        float minDistance = 0.1f, minNumMatches = 50;
        float sigma = 1.0f;
        int iterations = 200;
    };
    struct Result {
        bool ok = false;
        std::array<float, 16> pose_f2g{};            // of frame2, row-major 4x4: [R | t * minDistance]; the reference frame's is the identity
        std::vector<uh_dmatch> matches;              // the survivors, in the order they came
        std::vector<std::array<float, 3>> points;    // their points, in the reference frame's camera system
        int model = UH_MAPINIT_NONE;
        uh_mapinit_result diagnostics{};             // scores, RH, every candidate's nGood and parallax (the buffers inside are not valid)
    };
    explicit MapInitializer(std::shared_ptr<Context> ctx) : ctx_(std::move(ctx)) { check(uh_mapinit_create(ctx_->get(), &mi_)); }
    ~MapInitializer() { uh_mapinit_destroy(mi_); }
    MapInitializer(const MapInitializer&) = delete;
    MapInitializer& operator=(const MapInitializer&) = delete;
    void setParams(const Params& p) { params_ = p; }
    void reset() { ref_kp_.clear(); has_ref_ = false; }
    bool hasReferenceFrame() const { return has_ref_; }
    template <class Frame> void setReferenceFrame(const Frame& f) {
        flatten(f, ref_kp_);
        intr_ = {f.imageParams.fx(), f.imageParams.fy(), f.imageParams.cx(), f.imageParams.cy()};
        has_ref_ = true;
    }
    // matches: trainIdx -> keypoint of the reference frame, queryIdx -> keypoint of frame2
    template <class Frame> Result initialize(const Frame& frame2, const std::vector<uh_dmatch>& matches) {
        if (!has_ref_) throw std::runtime_error("MapInitializer::initialize invalid reference frame");
        Result out;
        std::vector<float> kp2;
        flatten(frame2, kp2);
        const int n = (int)matches.size();
        std::vector<int32_t> m(2 * (size_t)n), mo(2 * (size_t)std::max(n, 1));
        std::vector<int32_t> at((size_t)std::max(n, 1));
        std::vector<float> po(3 * (size_t)std::max(n, 1));
        for (int i = 0; i < n; i++) { m[2 * i] = matches[i].trainIdx; m[2 * i + 1] = matches[i].queryIdx; }
        uh_mapinit_args a{};
        a.intr4 = intr_.data();
        a.kp1 = ref_kp_.data(); a.n_kp1 = (int32_t)(ref_kp_.size() / 2);
        a.kp2 = kp2.data(); a.n_kp2 = (int32_t)(kp2.size() / 2);
        a.matches = m.data(); a.n_matches = n;
        a.sigma = params_.sigma; a.iterations = params_.iterations;
        a.min_matches = (int32_t)std::ceil(params_.minNumMatches);   // `matches.size() < minNumMatches` with a float bound
        a.min_parallax = 1.0f; a.min_triangulated = 50; a.min_distance = params_.minDistance;
        a.samples = nullptr;
        uh_mapinit_result r{};
        r.matches_out = mo.data(); r.points_out = po.data(); r.index_out = at.data(); r.cap_matches = n;
        check(uh_mapinit_run(mi_, &a, &r));
        out.ok = r.ok != 0;
        out.model = r.model;
        std::memcpy(out.pose_f2g.data(), r.pose, sizeof(r.pose));
        for (int j = 0; j < r.n_out; j++) {
            out.matches.push_back(matches[(size_t)at[j]]);
            out.points.push_back({po[3 * j], po[3 * j + 1], po[3 * j + 2]});
        }
        r.matches_out = nullptr; r.points_out = nullptr; r.index_out = nullptr;
        out.diagnostics = r;
        return out;
    }
   private:
    template <class Frame> static void flatten(const Frame& f, std::vector<float>& xy) {
        xy.resize(2 * f.und_kpts.size());
        for (size_t i = 0; i < f.und_kpts.size(); i++) { xy[2 * i] = f.und_kpts[i].pt.x; xy[2 * i + 1] = f.und_kpts[i].pt.y; }
    }
    std::shared_ptr<Context> ctx_;
    uh_mapinit* mi_ = nullptr;
    Params params_;
    std::vector<float> ref_kp_;
    std::array<float, 4> intr_{};
    bool has_ref_ = false;
};

}  // namespace ucoslam_hip
